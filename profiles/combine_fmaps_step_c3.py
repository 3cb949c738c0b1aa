"""Writes profiles/combine_fmaps_step_c3.json: the DDPM step of the SR UNet at the C3 shape with and without
`combine_upsample_fmaps=True`, and the combiner's kernel per level beside the same layer built from existing entries.

  python profiles/combine_fmaps_step_c3.py --out DIR/combine_fmaps_step_c3.json
      the DDPM step of the C3 plan (unet2 of train_ultra_res.py:39-48 at 256^2, batch 16, low-res + cond images, dynamic
      threshold, cond table on, graph replay) built by default and with combine_upsample_fmaps=True, alternated on one GPU,
      warm, `reps` timed runs each (all kept: the spread is in the record); per level of the combiner, from `reps` runs of
      kd_unet_profile over the plan: the time of the launch of kernels_upcombine.hip ("upsample combine s=..") with the HBM
      rate of the output it writes, and of the low-resolution GroupNorm work in front of it; and the same layer as a
      composition of existing entries on the materialised map: nearest upsample (torch), kd_groupnorm_silu_nhwc at full
      resolution, kd_conv2d_nhwc (which also re-packs the weight on each call) - each timed warm, `reps` times.
      `slower_levels` names the levels where the kernel's slowest run does not beat the composition's fastest.
"""
import argparse
import csv
import ctypes as C
import io
import json
import re
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kidney-diffusion_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

VARIANTS = {"default": {}, "combine": dict(combine_upsample_fmaps=True)}


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


def spread(v):
    return dict(min=round(min(v), 1), median=round(statistics.median(v), 1), max=round(max(v), 1))


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
        runs.append(dict(name=name, unet=u, h=h, x=x0.clone(), sa=sa, launches=lib.kd_unet_num_launches(h), ms=[]))
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
               launches_per_forward={r["name"]: r["launches"] for r in runs})
    comb = next(r for r in runs if r["name"] == "combine")
    # (the profile replays the inputs of the last forward)
    comb["unet"](x0, torch.zeros(B, device=device), lowres_cond_img=lowres, lowres_noise_times=torch.full((B,), 0.2, device=device),
                 cond_images=cond)
    levels = {}
    for _ in range(reps):
        buf = C.create_string_buffer(1 << 22)
        E.check(lib.kd_unet_profile(comb["h"], 3, buf, len(buf), E.current_stream()))
        rows = [row for row in csv.reader(io.StringIO(buf.value.decode())) if len(row) >= 5]
        for i, row in enumerate(rows):
            if not row[1].startswith("upsample combine s="):
                continue
            sc, M, cin, cout = (int(v) for v in re.search(r"s=(\d+) M(\d+) Cin(\d+) Cout(\d+)", row[1]).groups())
            lv = levels.setdefault(row[1], dict(label=row[1], scale=sc, M=M, cin=cin, cout=cout, us=[], lowres_norm_us=[]))
            lv["us"].append(float(row[3]))
            # the GroupNorm work in front of the launch: one "gn fold seg" row, or "gn stats" + "gn apply" at low resolution
            pre = 0.0
            for back in rows[max(0, i - 2):i]:
                if back[1].startswith(("gn fold seg", "gn stats", "gn apply")) and f" C{cin}" in back[1]:
                    pre += float(back[3])
            lv["lowres_norm_us"].append(pre)
    out = []
    for lv in levels.values():
        out_bytes = 4 * lv["M"] * lv["scale"] ** 2 * lv["cout"]
        us = lv.pop("us")
        pre = lv.pop("lowres_norm_us")
        lv.update(kernel_us=spread(us), lowres_norm_us=spread(pre), output_mb=round(out_bytes / 1e6, 1),
                  hbm_write_tbps=round(out_bytes / statistics.median(us) / 1e6, 2))
        lv["composition_us"] = composition(lv, B, device, reps)
        lv["kernel_faster_beyond_spread"] = bool(lv["kernel_us"]["max"] + lv["lowres_norm_us"]["max"]
                                                 < lv["composition_us"]["total"]["min"])
        out.append(lv)
    rec["combiner_levels"] = out
    rec["slower_levels"] = [lv["label"] for lv in out if not lv["kernel_faster_beyond_spread"]]
    return rec


def composition(lv, B, device, reps, iters=2):
    """The same layer from existing entries on the materialised map: nearest upsample (torch), kd_groupnorm_silu_nhwc,
    kd_conv2d_nhwc; each piece timed by itself, warm."""
    import torch
    import torch.nn.functional as F

    from imagen_pytorch import _engine as E

    lib = E.load()
    sc, cin, cout = lv["scale"], lv["cin"], lv["cout"]
    side = int(round((lv["M"] // B) ** 0.5))
    x = torch.randn(B, side, side, cin, device=device)
    w = torch.randn(cout, cin, 3, 3, device=device) * 0.02
    b = torch.zeros(cout, device=device)
    gamma, beta = torch.ones(cin, device=device), torch.zeros(cin, device=device)
    S = sc * side
    up = torch.empty(B, S, S, cin, device=device)
    act = torch.empty_like(up)
    y = torch.empty(B, S, S, cout, device=device)
    xn = x.permute(0, 3, 1, 2)   # NCHW view of the NHWC map: interpolate keeps the channels-last memory

    def upsample():
        up.copy_(F.interpolate(xn, scale_factor=sc, mode="nearest").permute(0, 2, 3, 1))

    def norm():
        E.check(lib.kd_groupnorm_silu_nhwc(E.ptr(up), E.ptr(gamma), E.ptr(beta), None, E.ptr(act), B, S * S, cin, 8, 1e-5,
                                           E.current_stream()))

    def conv():
        E.check(lib.kd_conv2d_nhwc(E.ptr(act), E.ptr(w), E.ptr(b), E.ptr(y), B, S, S, cin, cout, 3, 3, 1, 1, 0, E.current_stream()))

    times = {"upsample": [], "groupnorm_silu": [], "conv3x3": []}
    for name, fn in (("upsample", upsample), ("groupnorm_silu", norm), ("conv3x3", conv)):
        fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters * 1e3)
    total = [sum(v) for v in zip(*times.values())]
    del x, up, act, y
    torch.cuda.empty_cache()
    return dict({k: spread(v) for k, v in times.items()}, total=spread(total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch

    device = torch.device("cuda:0")
    rec = dict(what="DDPM step of the SR UNet with and without combine_upsample_fmaps=True, and the combiner's kernel per "
                    "level beside nearest upsample + kd_groupnorm_silu_nhwc + kd_conv2d_nhwc on the materialised map",
               shape="unet2 of train_ultra_res.py:39-48, 256^2, batch 16 (C3), random weights, default plan, graph replay")
    rec.update(step_times(device))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
