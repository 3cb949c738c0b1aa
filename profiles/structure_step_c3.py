"""Writes profiles/structure_step_c3.json: the DDPM step of the SR UNet at the C3 shape built by default and with each of the
first / last layer's structural switches alone, and the launches of the new kernels beside the existing paths.

  python profiles/structure_step_c3.py --out DIR/structure_step_c3.json
      the DDPM step of the C3 plan (unet2 of train_ultra_res.py:39-48 at 256^2, batch 16, low-res + cond images, dynamic
      threshold, cond table on, graph replay) for every entry of VARIANTS, alternated on one GPU, warm, `reps` timed runs each
      (all kept: the spread is in the record); then, from `reps` runs of kd_unet_profile over each plan, the time of
        * the plain init conv's one kernel ("init conv plain fused k7 ..", 3 planes) and of the generic path on the same plan
          shape (`unet.init_conv_generic = 1`: the pack of the planes + one implicit-GEMM conv k = 7);
        * the final conv's two launches - the 1x1 GEMM to the k^2 C columns and the gather - at k = 1, 3, 5 and 7.
      `plain_init_kernel_faster_beyond_spread`: the kernel's slowest run beats the generic path's fastest.
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

VARIANTS = {
    "default": {},
    "init_cross_embed=False": dict(init_cross_embed=False),
    "init_cross_embed=False (generic conv)": dict(init_cross_embed=False),   # unet.init_conv_generic = 1
    "init_cross_embed_kernel_sizes=(3, 5)": dict(init_cross_embed_kernel_sizes=(3, 5)),
    "final_conv_kernel_size=1": dict(final_conv_kernel_size=1),
    "final_conv_kernel_size=5": dict(final_conv_kernel_size=5),
    "final_conv_kernel_size=7": dict(final_conv_kernel_size=7),
    "final_resnet_block=False": dict(final_resnet_block=False),
    "scale_skip_connection=False": dict(scale_skip_connection=False),
}
GENERIC = "init_cross_embed=False (generic conv)"


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


def measure(device, steps=10, reps=5):
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
        if name == GENERIC:
            u.init_conv_generic = 1   # engine extension, read when the plan is built
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
    rec = dict(step_ms={r["name"]: dict(min=min(r["ms"]), median=statistics.median(r["ms"]), max=max(r["ms"])) for r in runs},
               step_reps={r["name"]: r["ms"] for r in runs}, launches_per_forward={r["name"]: r["launches"] for r in runs})

    def rows_of(r):
        """label -> [us per run] over `reps` profiles of the plan (the profile replays the inputs of the last forward)"""
        r["unet"](x0, torch.zeros(B, device=device), lowres_cond_img=lowres, lowres_noise_times=torch.full((B,), 0.2, device=device),
                  cond_images=cond)
        out = []
        for _ in range(reps):
            buf = C.create_string_buffer(1 << 22)
            E.check(lib.kd_unet_profile(r["h"], 3, buf, len(buf), E.current_stream()))
            rows = [row for row in csv.reader(io.StringIO(buf.value.decode())) if len(row) >= 5][1:]
            out.append([(row[1], float(row[3])) for row in rows])
        return out

    by = {r["name"]: r for r in runs}
    # ---- the plain init conv: the one kernel, and pack + generic conv on the same shape
    fused = [[us for lb, us in run if lb.startswith("init conv plain fused")] for run in rows_of(by["init_cross_embed=False"])]
    assert all(len(f) == 1 for f in fused)
    gen = []
    for run in rows_of(by[GENERIC]):
        i = next(i for i, (lb, _) in enumerate(run) if lb.startswith("conv k7 s1") and " Cin4 " in lb)
        assert not any(lb.startswith("init conv") for lb, _ in run)
        gen.append(dict(pack=run[i - 1][1], conv=run[i][1], conv_label=run[i][0], pack_label=run[i - 1][0]))
    k_us, g_us = [f[0] for f in fused], [g["pack"] + g["conv"] for g in gen]
    rec["plain_init_k7_np3"] = dict(kernel_us=spread(k_us), generic_us=dict(total=spread(g_us), pack=spread([g["pack"] for g in gen]),
                                                                            conv=spread([g["conv"] for g in gen]),
                                                                            labels=[gen[0]["pack_label"], gen[0]["conv_label"]]))
    rec["plain_init_kernel_faster_beyond_spread"] = bool(max(k_us) < min(g_us))
    # ---- the final conv: the column GEMM + the gather
    fin = {}
    for k, name in ((3, "default"), (1, "final_conv_kernel_size=1"), (5, "final_conv_kernel_size=5"), (7, "final_conv_kernel_size=7")):
        gemm, gather, labels = [], [], None
        for run in rows_of(by[name]):
            assert run[-1][0].startswith("final gather") and run[-2][0].startswith("conv k1 s1")
            gemm.append(run[-2][1])
            gather.append(run[-1][1])
            labels = [run[-2][0], run[-1][0]]
        fin[f"k={k}"] = dict(column_gemm_us=spread(gemm), gather_us=spread(gather), total_us=spread([a + b for a, b in zip(gemm, gather)]),
                             labels=labels)
    rec["final_conv"] = fin
    rec["final_conv_alternative_form"] = ("the gather's first form (unpadded k^2 columns, 4-byte staging loads, 256 threads), measured with this "
                                          "script before it was replaced: 662 us at k = 5, 2027 us at k = 7; no direct kernel was built")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch

    device = torch.device("cuda:0")
    rec = dict(what="DDPM step of the SR UNet by default and with each structural switch of the first / last layer alone; the "
                    "plain init conv's kernel beside pack + generic conv; the final conv's launches at k = 1, 3, 5, 7",
               shape="unet2 of train_ultra_res.py:39-48, 256^2, batch 16 (C3), random weights, default plan, graph replay")
    rec.update(measure(device))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
