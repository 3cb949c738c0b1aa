"""Writes profiles/attn_dim_head_step_c3.json: the DDPM step of the SR UNet at the C3 shape with attn_dim_head 32 / 64 / 128
at equal inner width and with layer_attns_depth 1 / 2 at the attention level, and the attention kernels' time per launch.

  python profiles/attn_dim_head_step_c3.py --out DIR/attn_dim_head_step_c3.json
      the DDPM step of the C3 plan (unet2 of train_ultra_res.py:39-48 at 256^2, batch 16, low-res + cond images, dynamic
      threshold, cond table on, graph replay) built by default (D = 64, 8 heads, depth 1), with (D, heads) = (32, 16) and
      (128, 4) - the same inner width of 512 - and with layer_attns_depth = (1, 1, 1, 2), alternated on one GPU, warm,
      `reps` timed runs each (all kept: the spread is in the record).  The UNet attends at its last level: 16 x 16 = 256
      tokens, 1 + 2 + 256 keys.  Per variant, from `reps` runs of kd_unet_profile over the plan: the time of its "attn N256"
      launches (attention_mfma_kernel<D>: 2 x heads x 16 blocks of 128 queries).  Per D, through kd_attention (one dense
      K/V segment of 259 keys, one shared K/V head, `iters` launches between two events, `reps` times): the matrix-core
      kernel at batch 16 x 256 queries, and the vector kernel at batch 1 x 64 queries - the launch rule (128 queries and 16
      blocks of them) never gives the vector kernel the level's 256 queries at these head counts.  `mfma_d128_h8` repeats the
      D = 128 launch with 8 heads - twice the work on 256 instead of 128 workgroups - to tell a launch that does not fill the
      256 CUs from a slower kernel.
      `d64_run_to_run_spread_ms`: max - min of the default plan's runs.  That plan is the parent commit's (same launches, same
      bits), so its step time is to be read against the parent's, taken in the same session with bench.py on both trees.
"""
import argparse
import csv
import ctypes as C
import io
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kidney-diffusion_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

VARIANTS = {"d64_h8": {}, "d32_h16": dict(attn_dim_head=32, attn_heads=16), "d128_h4": dict(attn_dim_head=128, attn_heads=4),
            "d64_h8_depth2": dict(layer_attns_depth=(1, 1, 1, 2))}
HEADS = {32: 16, 64: 8, 128: 4}
TOKENS, KEYS = 256, 1 + 2 + 256


def plan_unet(over, device):
    import torch

    import bench
    import imagen_pytorch as ip

    if not over:
        return bench.build_unet(0).to(device)
    torch.manual_seed(0)
    u = ip.Unet(**bench.SR_UNET_KW, lowres_cond=True, cond_on_text=False, text_embed_dim=None, **over)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():   # as bench.build_unet: the library zero-inits final_conv
        u.final_conv.weight.copy_(torch.randn(u.final_conv.weight.shape, generator=g) * 0.02)
        u.final_conv.bias.copy_(torch.randn(u.final_conv.bias.shape, generator=g) * 0.02)
    return u.to(device)


def spread(v, nd=1):
    return dict(min=round(min(v), nd), median=round(statistics.median(v), nd), max=round(max(v), nd))


def step_times(device, steps=10, reps=5):
    import torch

    import bench
    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes, beta_linear_log_snr, log_snr_to_alpha_sigma

    lib = E.load()
    B, S, T = bench.BATCH, bench.SIZE, bench.T_SCHED
    x0, lr, nz, cond = bench.synthetic_inputs(B, device, seed=1234)
    ls = beta_linear_log_snr(torch.full((B,), 0.2))
    a, s = log_snr_to_alpha_sigma(ls)
    lls = ls.to(device)
    lowres = (a.to(device)[:, None, None, None] * lr + s.to(device)[:, None, None, None] * nz).contiguous()
    tables = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=T).step_tables()
    sch = E.kd_schedule_t()
    sch.T = T
    for name, v in tables.items():
        setattr(sch, name, v.numpy().ctypes.data_as(C.POINTER(C.c_float)))
    runs = []
    for name, over in VARIANTS.items():
        sa = E.kd_sample_args_t()
        sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times = 0, 1, 0.95, 1
        sa.d_lowres, sa.d_lowres_log_snr, sa.d_cond_images = E.ptr(lowres), E.ptr(lls), E.ptr(cond)
        sa.lowres_log_snr_uniform, sa.lowres_log_snr_value = 1, float(ls[0])
        sa.seed, sa.use_graph = 1234, 1
        u = plan_unet(over, device)
        h = u.engine(B, S, device, with_text=False)
        runs.append(dict(name=name, unet=u, h=h, x=x0.clone(), sa=sa, launches=lib.kd_unet_num_launches(h), ms=[],
                         gmacs=round(lib.kd_unet_macs(h) / 1e9, 2)))
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
    rec = dict(step_ms={r["name"]: statistics.median(r["ms"]) for r in runs}, step_reps={r["name"]: r["ms"] for r in runs},
               launches_per_forward={r["name"]: r["launches"] for r in runs}, gmacs_per_forward={r["name"]: r["gmacs"] for r in runs})
    base = next(r for r in runs if r["name"] == "d64_h8")["ms"]
    rec["d64_run_to_run_spread_ms"] = round(max(base) - min(base), 3)
    # the plan's own attention launches (the profile replays the inputs of the last forward)
    plan_rows = {}
    for r in runs:
        r["unet"](x0, torch.zeros(B, device=device), lowres_cond_img=lowres, lowres_noise_times=torch.full((B,), 0.2, device=device),
                  cond_images=cond)
        per_rep = []
        for _ in range(reps):
            buf = C.create_string_buffer(1 << 22)
            E.check(lib.kd_unet_profile(r["h"], 3, buf, len(buf), E.current_stream()))
            rows = [row for row in csv.reader(io.StringIO(buf.value.decode())) if len(row) >= 5]
            us = [float(row[3]) for row in rows if row[1] == f"attn N{TOKENS}"]
            per_rep.append(us)
        plan_rows[r["name"]] = dict(launches=len(per_rep[0]), us_per_launch=spread([statistics.mean(u) for u in per_rep]),
                                    us_all_launches=spread([sum(u) for u in per_rep]))
    rec["plan_attention_launches"] = plan_rows
    return rec


def kernel_times(device, reps=5, iters=50):
    """Both kernels of every instantiation at equal H D = 512 through kd_attention (asynchronous: `iters` launches between
    two events)."""
    import torch

    from imagen_pytorch import _engine as E

    lib = E.load()
    out = {}
    for D, H in list(HEADS.items()) + [(128, 8)]:
        for kernel, (B, Nq) in (("mfma", (16, TOKENS)), ("vector", (1, 64))):
            if H != HEADS[D] and kernel != "mfma":
                continue
            mfma = Nq >= 128 and ((Nq + 127) // 128) * H * B >= 16
            assert mfma == (kernel == "mfma")
            g = torch.Generator().manual_seed(D)
            q = (torch.randn(B, Nq, H, D, generator=g) * D ** -0.5).to(device)
            k, v = (torch.randn(B, KEYS, 1, D, generator=g).to(device) for _ in range(2))
            o = torch.empty_like(q)
            run = lambda: E.check(lib.kd_attention(E.ptr(q), E.ptr(k), E.ptr(v), E.ptr(o), B, Nq, KEYS, H, 1, D, E.current_stream()))
            run()
            torch.cuda.synchronize()
            us = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    run()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) / iters * 1e3)
            assert bool(torch.isfinite(o).all())
            macs = 2 * B * H * Nq * KEYS * D
            blocks = ((Nq + 127) // 128 if mfma else (Nq + (31 if D == 128 else 63)) // (32 if D == 128 else 64)) * H * B
            out[f"{kernel}_d{D}_h{H}"] = dict(B=B, Nq=Nq, keys=KEYS, H=H, D=D, key_tile=lib.kd_attention_key_tile(D), workgroups=blocks,
                                              us=spread(us, 2), gflops=round(2 * macs / statistics.median(us) / 1e3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch

    device = torch.device("cuda:0")
    rec = dict(what="DDPM step of the SR UNet with attn_dim_head 32 / 64 / 128 at inner width 512 and with layer_attns_depth 1 / 2 "
                    "at the attention level; time per launch of every attention instantiation on both kernels",
               shape="unet2 of train_ultra_res.py:39-48, 256^2, batch 16 (C3), random weights, default plan, graph replay; "
                     "attention at 16 x 16 = 256 tokens, 259 keys")
    rec.update(step_times(device))
    rec["attention_kernels"] = kernel_times(device)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
