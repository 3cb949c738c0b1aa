"""Writes profiles/solver3_step_c3.json: ms per sampling step at the C3 shape for DPM-Solver++(2M), DPM-Solver++(3M) and the
SDE form of 3M at eta = 1.

  python profiles/solver3_step_c3.py --out profiles/solver3_step_c3.json

The C3 plan (unet2 of train_ultra_res.py:39-48 at 256^2, batch 16, low-res + cond images, dynamic threshold, cond table on,
graph replay, in-kernel noise), one process, one plan, as profiles/solver_step_c3.py.  Every form is warmed (capture, table
rows, the histories), then five runs of 20 steps per form, the order of the forms rotating from run to run; min - max over
the runs is the run-to-run spread.  3M reads one more image than 2M per step (12.6 MB); the SDE form also draws the
ancestral step's noise."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
STEPS, RUNS = 20, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    for p in (ROOT, ROOT / "kidney-diffusion_amd"):
        sys.path.insert(0, str(p))
    import torch

    import bench
    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import (GaussianDiffusionContinuousTimes, beta_linear_log_snr, log_snr_to_alpha_sigma,
                                               solver_tables)

    device = torch.device("cuda:0")
    lib = E.load()
    B, S, T = bench.BATCH, bench.SIZE, bench.T_SCHED
    x, lowres, noise, cond = bench.synthetic_inputs(B, device, seed=1234)
    ls = beta_linear_log_snr(torch.full((B,), 0.2))
    al, sg = log_snr_to_alpha_sigma(ls)
    lowres = (al.to(device)[:, None, None, None] * lowres + sg.to(device)[:, None, None, None] * noise).contiguous()
    lls = ls.to(device)
    tables = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=T).step_tables()
    fptr = lambda v: v.numpy().ctypes.data_as(C.POINTER(C.c_float))

    sa = E.kd_sample_args_t()
    sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times = 0, 1, 0.95, 1
    sa.d_lowres, sa.d_lowres_log_snr, sa.d_cond_images = E.ptr(lowres), E.ptr(lls), E.ptr(cond)
    sa.lowres_log_snr_uniform, sa.lowres_log_snr_value = 1, float(ls[0])
    sa.seed, sa.use_graph = 1234, 1

    keep = []

    def solver(name, eta):
        coef = solver_tables(tables, name, eta=eta)
        sc = E.kd_solver3_schedule_t() if "coef_prev2" in coef else E.kd_solver_schedule_t()
        sc.T = T
        for n in ("log_snr", "alpha", "sigma", "rn_a", "rn_b"):
            setattr(sc, n, fptr(tables[n]))
        for n, v in coef.items():
            setattr(sc, n, fptr(v))
        keep.append(coef)
        return (lib.kd_solver3_sample_steps if "coef_prev2" in coef else lib.kd_solver_sample_steps), sc

    forms = {"dpmpp_2m": solver("dpmpp_2m", 0.0), "dpmpp_3m": solver("dpmpp_3m", 0.0), "dpmpp_3m_sde": solver("dpmpp_3m_sde", 1.0)}
    unet = bench.build_unet(0).to(device)   # (kept: the plan handle dies with it)
    h = unet.engine(B, S, device, with_text=False)
    xs = {k: x.clone() for k in forms}
    k0 = 3   # (3M is third order from step 2 on)
    assert k0 + STEPS < T - 2
    for k, (fn, sc) in forms.items():   # warm-up: capture, table rows, history
        E.check(fn(h, C.byref(sc), C.byref(sa), E.ptr(xs[k]), 0, k0, E.current_stream()))
    torch.cuda.synchronize()
    reps = {k: [] for k in forms}
    names = list(forms)
    for run in range(RUNS):
        for k in names[run % len(names):] + names[:run % len(names)]:
            fn, sc = forms[k]
            y = xs[k].clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            E.check(fn(h, C.byref(sc), C.byref(sa), E.ptr(y), k0, k0 + STEPS, E.current_stream()))
            e1.record()
            torch.cuda.synchronize()
            reps[k].append(round(e0.elapsed_time(e1) / STEPS, 3))
            assert bool(torch.isfinite(y).all())
        print(f"run {run}: " + ", ".join(f"{k} {v[-1]} ms" for k, v in reps.items()), flush=True)
    rec = dict(what="ms per sampling step: DPM-Solver++(2M), DPM-Solver++(3M) and 3M-SDE (eta 1) on one plan in one "
                    f"process; {RUNS} warm runs of {STEPS} steps per form, the order of the forms rotating between runs",
               shape="unet2 of train_ultra_res.py:39-48, 256^2, batch 16 (C3), random weights, default plan, graph replay",
               step_ms={k: dict(min=min(v), max=max(v), reps=v) for k, v in reps.items()})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
