"""Writes profiles/linear_attn_step_c3.json: the cost of linear attention (Unet(use_linear_attn=True)) at the C3 shape.

  python profiles/linear_attn_step_c3.py --out DIR/linear_attn_step_c3.json
      the DDPM step of the C3 plan (unet2 of train_ultra_res.py:39-48 at 256^2, batch 16, low-res + cond images, dynamic
      threshold, cond table on, graph replay) with and without use_linear_attn=True (a LinearAttentionTransformerBlock at
      the 128^2, 64^2 and 32^2 levels, down and up: six blocks), alternated on one GPU.
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/linear_attn_step_c3.py --trace-only --out DIR/t.json
      the linear plan alone under the kernel tracer (a separate run: tracing slows the host)
  python profiles/linear_attn_step_c3.py --merge DIR/linear_attn_step_c3.json --stats DIR/run_results.db
      folds that run's statistics of the kernels of kernels_linattn.hip into the record, with their algorithmic bytes and
      FLOP per step (from the shapes, below) and the share of the bound that limits each (no GPU needed).
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

HBM_BPS = 6.3e12        # achievable HBM bandwidth (MI355X_MICROARCH: ~6.3 TB/s of the 8 TB/s spec)
MFMA_F32 = 157.3e12     # fp32 MFMA peak FLOP/s
HEADS, DH = 8, 64


def block_shapes():
    """(H W, channels) of the six linear blocks of the C3 plan: memory-efficient unet2, levels 0-2 (level 3 has full
    attention), one block on each path."""
    import bench

    S, dim, mults = bench.SIZE, bench.SR_UNET_KW["dim"], bench.SR_UNET_KW["dim_mults"]
    out = []
    for l in range(3):
        s = S >> (l + 1)
        out += [(s * s, dim * mults[l])] * 2
    return out


def algorithmic(B):
    """Bytes and FLOP per step of each kernel, summed over the six blocks (fp32; each map read / written once)."""
    inner = HEADS * DH
    rec = {}
    for name in ("la_dwconv_kernel", "la_ctx_reduce_kernel", "la_ctx_combine_kernel", "la_apply_kernel"):
        rec[name] = dict(bytes=0, flop=0, launches=0)
    for hw, _ in block_shapes():
        nch = (hw + 63) // 64
        d = rec["la_dwconv_kernel"]
        d["bytes"] += 2 * B * hw * 3 * inner * 4 + B * nch * inner * 8
        d["flop"] += 2 * 9 * B * hw * 3 * inner
        r = rec["la_ctx_reduce_kernel"]
        r["bytes"] += B * hw * 2 * inner * 4
        r["flop"] += 2 * B * HEADS * hw * DH * DH
        a = rec["la_apply_kernel"]
        a["bytes"] += 2 * B * hw * inner * 4
        a["flop"] += 2 * B * hw * inner * DH
        c = rec["la_ctx_combine_kernel"]
        c["bytes"] += B * HEADS * DH * DH * 4
        for v in rec.values():
            v["launches"] += 1
    return rec


def plans(device):
    import torch

    import bench
    import imagen_pytorch as ip

    plain = bench.build_unet(0)
    lin = ip.Unet(**bench.SR_UNET_KW, lowres_cond=True, cond_on_text=False, text_embed_dim=None, use_linear_attn=True)
    sd = plain.state_dict()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, v in lin.state_dict().items():
            if k in sd:
                v.copy_(sd[k])
            elif k.endswith(".g"):
                v.copy_(1.0 + 0.1 * torch.randn(v.shape, generator=g))
            elif v.dim() == 1:
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            else:   # the new blocks' weights, fan-in scaled
                v.copy_(torch.randn(v.shape, generator=g) * v[0].numel() ** -0.5)
    return plain.to(device), lin.to(device)


def step_times(device, units, steps=20, reps=3):
    import torch

    import bench
    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes, beta_linear_log_snr, log_snr_to_alpha_sigma

    lib = E.load()
    B, S, T = bench.BATCH, bench.SIZE, bench.T_SCHED
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
    reps_ms = [[] for _ in units]
    for _ in range(reps):
        for i, (h, xx) in enumerate(zip(hs, xs)):   # alternated, same box
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            E.check(lib.kd_sample_steps(h, C.byref(sch), C.byref(sa), E.ptr(xx), 2, 2 + steps, E.current_stream()))
            e1.record()
            torch.cuda.synchronize()
            reps_ms[i].append(round(e0.elapsed_time(e1) / steps, 3))
    assert all(bool(torch.isfinite(xx).all()) for xx in xs)
    return reps_ms, launches


def merge(path, stats):
    """Kernel statistics of the traced run: rocprofv3's database (*.db, its default output) or *_kernel_stats.csv."""
    import bench

    rec = json.loads(Path(path).read_text())
    alg = algorithmic(bench.BATCH)
    if str(stats).endswith(".db"):
        import sqlite3

        with sqlite3.connect(stats) as db:
            rows = list(db.execute("select name, count(*), avg(end - start) from kernels group by name"))
    else:
        with open(stats) as f:
            rows = [(r["Name"], int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(f)]
    out = {}
    for name, n, ns in rows:
        short = next((k for k in alg if k in name), None)
        if short is None:
            continue
        a = alg[short]
        step_s = ns * 1e-9 * a["launches"]   # the step's launches of this kernel at the traced average
        t_hbm, t_mfma = a["bytes"] / HBM_BPS, a["flop"] / MFMA_F32
        bound = "HBM" if t_hbm >= t_mfma else "MFMA fp32"
        out[short] = dict(launches_traced=int(n), avg_us=round(ns / 1e3, 2), per_step_us=round(step_s * 1e6, 1),
                          alg_bytes_per_step=a["bytes"], alg_flop_per_step=a["flop"],
                          achieved_GBps=round(a["bytes"] / step_s / 1e9, 1), achieved_TFLOPs=round(a["flop"] / step_s / 1e12, 2),
                          bound=bound, share_of_bound=round(max(t_hbm, t_mfma) / step_s, 3))
    rec["kernels"] = out
    Path(path).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--merge")
    ap.add_argument("--stats")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, a.stats)
        return
    import torch

    device = torch.device("cuda:0")
    plain, lin = plans(device)
    if a.trace_only:
        reps, launches = step_times(device, [lin], steps=5, reps=1)
        print(json.dumps(dict(linear_attn_step_ms=reps[0], launches=launches)))
        return
    reps, launches = step_times(device, [plain, lin], reps=5)
    rec = dict(what="DDPM step with use_linear_attn=True (six LinearAttentionTransformerBlocks: 128^2, 64^2, 32^2 levels, "
                    "down and up) against the same UNet without it; alternated, 20 steps per repetition",
               shape="unet2 of train_ultra_res.py:39-48, 256^2, batch 16 (C3), random weights, default plan, graph replay",
               plain_step_ms=min(reps[0]), linear_attn_step_ms=min(reps[1]), plain_reps=reps[0], linear_attn_reps=reps[1],
               launches_per_forward=dict(plain=launches[0], linear_attn=launches[1]),
               peaks=dict(hbm_achievable_Bps=HBM_BPS, mfma_f32_flops=MFMA_F32))
    rec["linear_attn_extra_ms"] = round(rec["linear_attn_step_ms"] - rec["plain_step_ms"], 3)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
