"""Writes profiles/resample_step_c3.json: the DDPM step of the SR UNet at the C3 shape with the library's other resampling
layers, and the nearest-x2 + conv3x3 kernel by itself.

  python profiles/resample_step_c3.py --out DIR/resample_step_c3.json
      the DDPM step of the C3 plan (unet2 of train_ultra_res.py:39-48 at 256^2, batch 16, low-res + cond images, dynamic
      threshold, cond table on, graph replay) built by default, with cross_embed_downsample=True, with
      pixel_shuffle_upsample=False and with both, alternated on one GPU; per launch of upsample_nearest_conv3x3_kernel in
      the plan with both switches (kd_unet_profile): time, fp32 MFMA rate of the MACs it issues, HBM rate of its
      algorithmic bytes (input and weights read once, output written once); and the same layers as the generic conv over a
      materialised nearest upsample (kd_conv2d_nhwc, which also re-packs the weight on each call).
"""
import argparse
import csv
import ctypes as C
import io
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kidney-diffusion_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

VARIANTS = {"default": {}, "cross_embed": dict(cross_embed_downsample=True), "nearest": dict(pixel_shuffle_upsample=False),
            "both": dict(cross_embed_downsample=True, pixel_shuffle_upsample=False)}


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


def step_times(device, steps=20, reps=3):
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
    rec = dict(step_ms={r["name"]: min(r["ms"]) for r in runs}, step_reps={r["name"]: r["ms"] for r in runs},
               launches_per_forward={r["name"]: r["launches"] for r in runs})
    both = next(r for r in runs if r["name"] == "both")
    # (the profile replays the inputs of the last forward)
    both["unet"](x0, torch.zeros(B, device=device), lowres_cond_img=lowres, lowres_noise_times=torch.full((B,), 0.2, device=device),
                 cond_images=cond)
    buf = C.create_string_buffer(1 << 22)
    E.check(lib.kd_unet_profile(both["h"], 10, buf, len(buf), E.current_stream()))
    layers = []
    for row in csv.reader(io.StringIO(buf.value.decode())):
        if len(row) < 5 or not row[1].startswith("upsample nearest conv3"):
            continue
        M, cin, cout = (int(v) for v in re.search(r"M(\d+) Cin(\d+) Cout(\d+)", row[1]).groups())
        us, mfma = float(row[3]), int(row[4])
        bytes_ = 4 * (M * cin + 16 * cin * cout + 4 * M * cout)
        layers.append(dict(label=row[1], us=round(us, 1), mfma_tflops=round(2 * mfma / us / 1e6, 1),
                           hbm_tbps=round(bytes_ / us / 1e6, 2)))
    rec["upsample_nearest_conv3x3_launches"] = layers
    rec["generic_conv_over_materialised_upsample_us"] = generic_conv(layers, B, device)
    return rec


def generic_conv(layers, B, device, iters=5):
    """The same layers as nearest upsample (torch) + the generic 3x3 conv (kd_conv2d_nhwc): the conv alone is timed."""
    import torch
    import torch.nn.functional as F

    from imagen_pytorch import _engine as E

    lib = E.load()
    out = {}
    for l in layers:
        M, cin, cout = (int(v) for v in re.search(r"M(\d+) Cin(\d+) Cout(\d+)", l["label"]).groups())
        side = int(round((M // B) ** 0.5))
        x = torch.randn(B, cin, side, side, device=device)
        up = F.interpolate(x, scale_factor=2, mode="nearest").permute(0, 2, 3, 1).contiguous()
        w = torch.randn(cout, cin, 3, 3, device=device) * 0.02
        b = torch.zeros(cout, device=device)
        y = torch.empty(B, 2 * side, 2 * side, cout, device=device)
        call = lambda: E.check(lib.kd_conv2d_nhwc(E.ptr(up), E.ptr(w), E.ptr(b), E.ptr(y), B, 2 * side, 2 * side, cin, cout, 3, 3, 1,
                                                  1, 0, E.current_stream()))
        call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        out[l["label"]] = round(e0.elapsed_time(e1) / iters * 1e3, 1)
        del x, up, y
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch

    device = torch.device("cuda:0")
    rec = dict(what="DDPM step of the SR UNet with cross_embed_downsample=True / pixel_shuffle_upsample=False, and the "
                    "nearest-x2 + conv3x3 kernel per launch",
               shape="unet2 of train_ultra_res.py:39-48, 256^2, batch 16 (C3), random weights, default plan, graph replay")
    rec.update(step_times(device))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
