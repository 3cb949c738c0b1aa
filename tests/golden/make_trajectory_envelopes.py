"""Generates tests/golden/trajectory_envelopes.json from the CPU oracle alone (no product import, no GPU).

For every configuration of tests/trajectory_ref.py it runs the oracle's sampler unperturbed and with an error of relative
size eps = FWD_REL_L2 (the tolerance of one UNet forward, tests/test_unet_gpu.py) added to every UNet output in three ways
(a fresh random direction per call, one direction for the whole run, a scale factor), and stores per step the largest
deviation the three cause: what a forward sitting exactly on its tolerance does to the trajectory.  That envelope is the
tolerance of tests/test_trajectory_gpu.py.  It pins the amplification of a tolerance-sized forward error through the
ORACLE'S sampler on random weights - not the library (parity is unpinned, see README.md) and not the engine.

    python tests/golden/make_trajectory_envelopes.py          # rewrites the .json (a few minutes on 8 cores)
"""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import trajectory_ref as TR  # noqa: E402

OUT = Path(__file__).resolve().parent / "trajectory_envelopes.json"
PIN_T = 6          # the short record of configuration A that tests/test_trajectory.py regenerates


def r(v):
    return [r(x) for x in v] if isinstance(v, (list, tuple)) else float(f"{v:.4e}")


def main():
    torch.set_num_threads(8)
    eps = TR.FWD_REL_L2
    out = dict(eps=eps, margin=1.0, modes=list(TR.MODES), configs={})
    problems = []      # every configuration is measured and printed before a failed condition stops the write
    for name in TR.CONFIGS:
        base = TR.Case(name).run()
        env = TR.envelope(name, eps, base=base)
        fl = TR.floor(name, base=base)
        T = len(env["rel"])
        # the oracle must resolve what it is asked to judge: its own summation-order floor at most a quarter of the envelope
        worst = max(fl["rel"][k] / env["rel"][k] for k in range(T))
        if worst > 0.25 or fl["final"] > 0.25 * env["final"]:
            problems.append((name, "floor", worst, fl["final"], env["final"]))
        print(f"{name}: envelope rel k=0 {env['rel'][0]:.2e} k={T // 2 - 1} {env['rel'][T // 2 - 1]:.2e} k={T - 1} {env['rel'][-1]:.2e} "
              f"final max-abs {env['final']:.2e}; floor / envelope at most {worst:.3f}", flush=True)
        for m in TR.MODES:
            d = env["modes"][m]
            print(f"    {m:5s} rel k=0 {d['rel'][0]:.2e} k={T // 2 - 1} {d['rel'][T // 2 - 1]:.2e} k={T - 1} {d['rel'][-1]:.2e} "
                  f"final {d['final']:.2e}", flush=True)
        print(f"    floor rel k=0 {fl['rel'][0]:.2e} k={T - 1} {fl['rel'][-1]:.2e} final {fl['final']:.2e}", flush=True)
        if name == "base128":
            # a larger forward error must not give a smaller envelope
            env2 = TR.envelope(name, 2 * eps, base=base)
            if not (all(b >= a for a, b in zip(env["rel"], env2["rel"])) and env2["final"] >= env["final"]):
                problems.append((name, "not monotone in eps", env["rel"], env2["rel"]))
            print(f"    at 2 eps: rel k=0 {env2['rel'][0]:.2e} k={T - 1} {env2['rel'][-1]:.2e} final {env2['final']:.2e}", flush=True)
        out["configs"][name] = dict(
            params=TR.json_cfg(name), rel=r(env["rel"]), final=r(env["final"]), floor_rel=r(fl["rel"]), floor_final=r(fl["final"]),
            mode_rel={m: r(env["modes"][m]["rel"]) for m in TR.MODES}, mode_final={m: r(env["modes"][m]["final"]) for m in TR.MODES})
    pin = TR.envelope("base128", eps, T=PIN_T)
    out["base128_short"] = dict(T=PIN_T, rel=r(pin["rel"]), final=r(pin["final"]))
    assert not problems, problems
    OUT.write_text(json.dumps(out, indent=1) + "\n")
    print(OUT.name, OUT.stat().st_size)


if __name__ == "__main__":
    main()
