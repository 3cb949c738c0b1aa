"""Writes profiles/per_image_seeds_step_c3.json: what per-image Philox keys cost a DDPM step at the C3 shape.

  python profiles/per_image_seeds_step_c3.py --out profiles/per_image_seeds_step_c3.json [--parent DIR]
      ms per DDPM step of the C3 plan (unet2 of train_ultra_res.py:39-48 at 256^2, batch 16, low-res + cond images, dynamic
      threshold, cond table on, graph replay, in-kernel noise) keyed by an int seed and by 16 distinct seeds - and, with
      --parent, by an int seed on a checkout of the parent commit whose library is built (DIR).  Five rounds; a round is
      one fresh process per tree, run one after the other (parent, then this tree: int seed and seed list on one plan,
      which of the two is timed first alternating from round to round), each warming its plan and timing 20 steps per
      form.  min - max over the rounds is the run-to-run spread.

The update kernels that read the keys are about 0.1 ms of the step, so the forms should not differ beyond that spread."""
import argparse
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve()
STEPS, ROUNDS = 20, 5


def child(tree, list_first=False):
    """One process on `tree`: the plan, two warm-up steps per form, then 20 timed steps per form (the seed list before
    the int seed with list_first).  Prints one JSON line."""
    for p in (tree, tree / "kidney-diffusion_amd"):
        sys.path.insert(0, str(p))
    import torch

    import bench
    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes, beta_linear_log_snr, log_snr_to_alpha_sigma

    device = torch.device("cuda:0")
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

    def args(seeds):
        sa = E.kd_sample_args_t()
        sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times = 0, 1, 0.95, 1
        sa.d_lowres, sa.d_lowres_log_snr, sa.d_cond_images = E.ptr(lowres), E.ptr(lls), E.ptr(cond)
        sa.lowres_log_snr_uniform, sa.lowres_log_snr_value = 1, float(ls[0])
        sa.seed, sa.use_graph = 1234, 1
        if seeds is not None:
            sa.seeds = seeds
        return sa

    forms = {"int_seed": args(None)}
    if hasattr(E, "seed_array"):   # (the parent commit has no per-image keys)
        keys = E.seed_array([1234 + 7919 * b for b in range(B)])
        forms["seed_list"] = args(keys)
    unet = bench.build_unet(0).to(device)   # (kept: the plan handle dies with it)
    h = unet.engine(B, S, device, with_text=False)
    xs = {k: x.clone() for k in forms}
    for k, sa in forms.items():   # warm-up: capture, table rows
        E.check(lib.kd_sample_steps(h, C.byref(sch), C.byref(sa), E.ptr(xs[k]), 0, 2, E.current_stream()))
    torch.cuda.synchronize()
    out = {}
    for k, sa in (reversed(list(forms.items())) if list_first else forms.items()):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        E.check(lib.kd_sample_steps(h, C.byref(sch), C.byref(sa), E.ptr(xs[k]), 2, 2 + STEPS, E.current_stream()))
        e1.record()
        torch.cuda.synchronize()
        out[k] = round(e0.elapsed_time(e1) / STEPS, 3)
        assert bool(torch.isfinite(xs[k]).all())
    print("RESULT " + json.dumps(out))


def run_child(tree, list_first=False):
    cmd = [sys.executable, str(HERE), "--child", str(tree)] + (["--list-first"] if list_first else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"child on {tree} failed ({p.returncode}):\n{p.stderr[-2000:]}")
    line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--child")
    ap.add_argument("--list-first", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(Path(a.child).resolve(), a.list_first)
        return
    here = HERE.parent.parent
    reps = {"int_seed": [], "seed_list": [], "parent_int_seed": []}
    for i in range(ROUNDS):   # alternated: parent, this tree, parent, ...
        if a.parent:
            reps["parent_int_seed"].append(run_child(Path(a.parent).resolve())["int_seed"])
        r = run_child(here, list_first=i % 2 == 1)   # which form is timed first alternates
        reps["int_seed"].append(r["int_seed"])
        reps["seed_list"].append(r["seed_list"])
        print(f"round {i}: " + ", ".join(f"{k} {v[-1]} ms" for k, v in reps.items() if v), flush=True)
    span = lambda v: dict(min=min(v), max=max(v), reps=v) if v else None
    rec = dict(what="ms per DDPM step, in-kernel Philox noise keyed by an int seed, by 16 distinct per-image seeds, and by an int "
                    "seed on the parent commit; five rounds of one fresh process per tree (parent first), 20 warm steps per form, "
                    "the form timed first alternating between rounds",
               shape="unet2 of train_ultra_res.py:39-48, 256^2, batch 16 (C3), random weights, default plan, graph replay",
               step_ms={k: span(v) for k, v in reps.items()})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
