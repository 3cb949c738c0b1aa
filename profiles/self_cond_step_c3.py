"""Writes profiles/self_cond_step_c3.json: the cost of self-conditioning (Unet(self_cond=True)) at the C3 shape.

  python profiles/self_cond_step_c3.py --out DIR/self_cond_step_c3.json
      the DDPM step of the C3 plan (unet2 of train_ultra_res.py:39-48 at 256^2, batch 16, low-res + cond images,
      dynamic threshold, cond table on, graph replay) with and without self_cond, alternated on one GPU; and the fused
      6-plane init conv launch against the two-launch form (the 3-plane kernel twice, the second taking the first's
      output as its residual), both through kd_init_conv_planes_nchw with device events.
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/self_cond_step_c3.py --out DIR/trace_run.json
      the same run under the kernel tracer (a separate run: tracing slows the host)
  python profiles/self_cond_step_c3.py --merge DIR/self_cond_step_c3.json --stats DIR/run_results.db
      folds that run's kernel statistics (rocprofv3's results database DIR/run_results.db, or a *_kernel_stats.csv)
      into the record (no GPU needed).
"""
import argparse
import csv
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kidney-diffusion_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def plans(device):
    import torch

    import bench
    import imagen_pytorch as ip

    plain = bench.build_unet(0)
    sc = ip.Unet(**bench.SR_UNET_KW, lowres_cond=True, cond_on_text=False, text_embed_dim=None, self_cond=True)
    sd = plain.state_dict()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, v in sc.state_dict().items():
            if v.shape == sd[k].shape:
                v.copy_(sd[k])
            else:   # init_conv.convs.*.weight: the plain weights + random self_cond input channels (cond | x | SC | lowres)
                c0 = 3 + 3
                v[:, :c0].copy_(sd[k][:, :c0])
                v[:, c0 + 3:].copy_(sd[k][:, c0:])
                v[:, c0:c0 + 3].copy_(torch.randn(v[:, c0:c0 + 3].shape, generator=g) * v.shape[-1] ** -1)
    return plain.to(device), sc.to(device)


def step_times(device, steps=20, reps=3):
    import torch

    import bench
    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes, beta_linear_log_snr, log_snr_to_alpha_sigma

    lib = E.load()
    B, S, T = bench.BATCH, bench.SIZE, bench.T_SCHED
    units = plans(device)
    x, lowres, noise, cond = bench.synthetic_inputs(B, device, seed=1234)
    ls = beta_linear_log_snr(torch.full((B,), 0.2))
    a, s = log_snr_to_alpha_sigma(ls)
    lowres = (a.to(device)[:, None, None, None] * lowres + s.to(device)[:, None, None, None] * noise).contiguous()
    lls = ls.to(device)
    tables = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=T).step_tables()
    sch = E.kd_schedule_t()
    sch.T = T
    for name, v in tables.items():
        setattr(sch, name, v.numpy().ctypes.data_as(C.POINTER(C.c_float)))
    sa = E.kd_sample_args_t()
    sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times = 0, 1, 0.95, 1
    sa.d_lowres, sa.d_lowres_log_snr, sa.d_cond_images = E.ptr(lowres), E.ptr(lls), E.ptr(cond)
    sa.lowres_log_snr_uniform, sa.lowres_log_snr_value = 1, float(ls[0])
    sa.seed, sa.use_graph = 1234, 1
    hs = [u.engine(B, S, device, with_text=False) for u in units]
    xs = [x.clone() for _ in units]
    launches = [lib.kd_unet_num_launches(h) for h in hs]
    for h, xx in zip(hs, xs):   # warm-up: capture, table rows
        E.check(lib.kd_sample_steps(h, C.byref(sch), C.byref(sa), E.ptr(xx), 0, 2, E.current_stream()))
    torch.cuda.synchronize()
    reps_ms = [[], []]
    for _ in range(reps):
        for i, (h, xx) in enumerate(zip(hs, xs)):   # alternated, same box
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            E.check(lib.kd_sample_steps(h, C.byref(sch), C.byref(sa), E.ptr(xx), 2, 2 + steps, E.current_stream()))
            e1.record()
            torch.cuda.synchronize()
            reps_ms[i].append(round(e0.elapsed_time(e1) / steps, 3))
    assert all(bool(torch.isfinite(xx).all()) for xx in xs)
    return dict(plain_step_ms=min(reps_ms[0]), self_cond_step_ms=min(reps_ms[1]), plain_reps=reps_ms[0],
                self_cond_reps=reps_ms[1], launches_per_forward=dict(plain=launches[0], self_cond=launches[1]))


def init_conv_times(device, iters=50, reps=3):
    import torch

    import bench
    from imagen_pytorch import _engine as E

    lib = E.load()
    B, S = bench.BATCH, bench.SIZE
    dim = bench.SR_UNET_KW["dim"]
    n3, n7, n15 = dim // 2, dim // 4, dim - dim // 2 - dim // 4
    Itot, Cc = 12, 3   # cond | x | self_cond | lowres
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 3, S, S, generator=g).to(device)
    sc = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(device)
    ws = [(torch.randn(n, Itot, k, k, generator=g) * (Itot * k * k) ** -0.5).to(device)
          for n, k in ((n3, 3), (n7, 7), (n15, 15))]
    C_ = n3 + n7 + n15
    res = torch.randn(B, S, S, C_, generator=g).to(device)   # the step-invariant share of cond | lowres
    y1 = torch.empty(B, S, S, C_, device=device)
    y2 = torch.empty_like(y1)
    tmp = torch.empty_like(y1)

    def run(xp, scp, c0, resp, y):
        ms = C.c_float(0)
        E.check(lib.kd_init_conv_planes_nchw(E.ptr(xp), E.ptr(scp), E.ptr(ws[0]), E.ptr(ws[1]), E.ptr(ws[2]), Itot, c0,
                                             None, E.ptr(resp), E.ptr(y), B, S, n3, n7, n15, iters, C.byref(ms),
                                             E.current_stream()))
        return ms.value

    fused, two, three = [], [], []
    for _ in range(reps):
        fused.append(run(x, sc, Cc, res, y1))
        two.append(run(x, None, Cc, res, tmp) + run(sc, None, Cc + 3, tmp, y2))
        three.append(run(x, None, Cc, res, tmp))
    torch.cuda.synchronize()
    rel = float((y1 - y2).double().norm() / y2.double().norm())
    return dict(fused_6plane_ms=round(min(fused), 4), two_launch_ms=round(min(two), 4),
                three_plane_ms=round(min(three), 4), fused_reps=[round(v, 4) for v in fused],
                two_launch_reps=[round(v, 4) for v in two], fused_vs_two_launch_rel_l2=rel,
                extra_bytes_two_launch=2 * B * S * S * C_ * 4)


def merge(path, stats):
    """Kernel statistics of the traced run: rocprofv3's database (*.db, its default output) or *_kernel_stats.csv."""
    rec = json.loads(Path(path).read_text())
    keep = ("init_conv_kernel", "ddpm_update_kernel", "pack_init_kernel")
    rows = []
    if str(stats).endswith(".db"):
        import sqlite3

        with sqlite3.connect(stats) as db:
            rows = list(db.execute("select name, count(*), avg(end - start) from kernels group by name"))
    else:
        with open(stats) as f:
            rows = [(r["Name"], int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(f)]
    rec["kernel_trace_avg_us"] = {name.split("(")[0].replace("void ", ""): dict(launches=int(n), avg_us=round(ns / 1e3, 2))
                                  for name, n, ns in rows if any(t in name for t in keep)}
    Path(path).write_text(json.dumps(rec, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--merge")
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, a.stats)
        return
    import torch

    device = torch.device("cuda:0")
    rec = dict(what="Self-conditioned DDPM step (Unet(self_cond=True)) against the plain step of the same UNet; the fused "
                    "6-plane init conv against the two-launch form",
               shape="unet2 of train_ultra_res.py:39-48, 256^2, batch 16 (C3), random weights, default plan, graph replay")
    rec.update(step_times(device))
    rec["self_cond_extra_ms"] = round(rec["self_cond_step_ms"] - rec["plain_step_ms"], 3)
    rec["init_conv"] = init_conv_times(device)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
