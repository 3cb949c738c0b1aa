"""Writes profiles/channels_step_c3.json: the DDPM step of the SR UNet at the C3 shape for images of 1, 3 and 4 channels.

  python profiles/channels_step_c3.py --out DIR/channels_step_c3.json
      the DDPM step of the C3 plan (unet2 of train_ultra_res.py:39-48 at 256^2, batch 16, low-res + cond images, dynamic
      threshold, cond table on, graph replay) built with channels = 3, 1 and 4, alternated on one GPU.
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/channels_step_c3.py --out DIR/trace_run.json
      the same run under the kernel tracer (a separate run, no counters: tracing slows the host)
  python profiles/channels_step_c3.py --merge DIR/channels_step_c3.json --stats DIR/run_results.db
      folds that run's kernel statistics (rocprofv3's results database, or a *_kernel_stats.csv) into the record (no
      GPU needed): the init conv (init_conv_kernel<2, C>) and the final conv's gather (final_gather_kernel<C>).
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

CHANNELS = (3, 1, 4)


def plan_unet(channels, device):
    import torch

    import bench
    import imagen_pytorch as ip

    if channels == 3:
        return bench.build_unet(0).to(device)
    torch.manual_seed(0)
    u = ip.Unet(**bench.SR_UNET_KW, channels=channels, lowres_cond=True, cond_on_text=False, text_embed_dim=None)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():   # as bench.build_unet: the library zero-inits final_conv
        u.final_conv.weight.copy_(torch.randn(u.final_conv.weight.shape, generator=g) * 0.02)
        u.final_conv.bias.copy_(torch.randn(u.final_conv.bias.shape, generator=g) * 0.02)
    return u.to(device)


def step_times(device, steps=20, reps=3):
    import torch

    import bench
    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes, beta_linear_log_snr, log_snr_to_alpha_sigma

    lib = E.load()
    B, S, T = bench.BATCH, bench.SIZE, bench.T_SCHED
    x3, lowres3, noise3, cond = bench.synthetic_inputs(B, device, seed=1234)
    ls = beta_linear_log_snr(torch.full((B,), 0.2))
    a, s = log_snr_to_alpha_sigma(ls)
    lls = ls.to(device)
    tables = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=T).step_tables()
    sch = E.kd_schedule_t()
    sch.T = T
    for name, v in tables.items():
        setattr(sch, name, v.numpy().ctypes.data_as(C.POINTER(C.c_float)))
    runs = []
    for ch in CHANNELS:
        g = torch.Generator().manual_seed(ch)
        pick = lambda t: (t[:, :ch] if ch <= 3 else torch.cat((t, torch.randn(B, 1, S, S, generator=g).to(device)), 1)).contiguous()
        x, lr, nz = pick(x3), pick(lowres3), pick(noise3)
        lowres = (a.to(device)[:, None, None, None] * lr + s.to(device)[:, None, None, None] * nz).contiguous()
        sa = E.kd_sample_args_t()
        sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times = 0, 1, 0.95, 1
        sa.d_lowres, sa.d_lowres_log_snr, sa.d_cond_images = E.ptr(lowres), E.ptr(lls), E.ptr(cond)
        sa.lowres_log_snr_uniform, sa.lowres_log_snr_value = 1, float(ls[0])
        sa.seed, sa.use_graph = 1234, 1
        u = plan_unet(ch, device)
        h = u.engine(B, S, device, with_text=False)
        runs.append(dict(ch=ch, unet=u, h=h, x=x, sa=sa, keep=(lowres,), launches=lib.kd_unet_num_launches(h), ms=[]))
    for r in runs:   # warm-up: capture, table rows
        E.check(lib.kd_sample_steps(r["h"], C.byref(sch), C.byref(r["sa"]), E.ptr(r["x"]), 0, 2, E.current_stream()))
    torch.cuda.synchronize()
    for _ in range(reps):
        for r in runs:   # alternated, same box
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            E.check(lib.kd_sample_steps(r["h"], C.byref(sch), C.byref(r["sa"]), E.ptr(r["x"]), 2, 2 + steps, E.current_stream()))
            e1.record()
            torch.cuda.synchronize()
            r["ms"].append(round(e0.elapsed_time(e1) / steps, 3))
    assert all(bool(torch.isfinite(r["x"]).all()) for r in runs)
    return dict(step_ms={f"c{r['ch']}": min(r["ms"]) for r in runs}, step_reps={f"c{r['ch']}": r["ms"] for r in runs},
                launches_per_forward={f"c{r['ch']}": r["launches"] for r in runs})


def merge(path, stats):
    """Kernel statistics of the traced run: rocprofv3's database (*.db, its default output) or *_kernel_stats.csv."""
    rec = json.loads(Path(path).read_text())
    keep = ("init_conv_kernel", "final_gather_kernel")
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
    rec = dict(what="DDPM step of the SR UNet built for images of 3, 1 and 4 channels (Unet(channels=C))",
               shape="unet2 of train_ultra_res.py:39-48, 256^2, batch 16 (C3), random weights, default plan, graph replay")
    rec.update(step_times(device))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
