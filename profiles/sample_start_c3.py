"""Writes profiles/sample_start_c3.json: the cost of the stage start kd_sample_start at the C3 shape (batch 16, 3 x 256^2)
against what sample() ran before it - the draw into a fresh tensor (kd_philox_normal or kd_philox_normal_rows), the copy
into the stable buffer and, for the EDM sampler, img.mul_(sigma_0).

  python profiles/sample_start_c3.py --out DIR/sample_start_c3.json

Each figure is microseconds per call: CALLS back-to-back calls on torch's stream between two device events, so it holds
the launches' host cost where that is the longer of the two; the min and max of five warm repetitions, the forms alternated
inside every repetition.  `with_source` adds a 64 x 64 init image (x 4 nearest); the forms of before have no such case.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kidney-diffusion_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

B, CH, S, SRC = 16, 3, 256, 64
CALLS, REPS = 200, 5
SID = (16 << 32) | 2


def forms(device):
    import torch

    from imagen_pytorch import _engine as E

    lib = E.load()
    n = CH * S * S
    img = torch.empty(B, CH, S, S, device=device)
    init = torch.rand(B, CH, SRC, SRC, device=device)
    seeds = E.seed_array(range(1, B + 1))
    st = E.current_stream

    def start(scale, keys, src):
        return lambda: E.check(lib.kd_sample_start(E.ptr(img), B, CH, S, scale, 7, keys, None, E.ptr(src), SRC if src is not None else 0,
                                                   SRC if src is not None else 0, st()))

    def before(scale, keys):
        def run():
            z = torch.empty(B, CH, S, S, device=device)
            if keys is None:
                E.check(lib.kd_philox_normal(E.ptr(z), B * n, 7, SID, st()))
            else:
                E.check(lib.kd_philox_normal_rows(E.ptr(z), B, n, keys, SID, st()))
            img.copy_(z)
            if scale != 1.0:
                img.mul_(scale)
        return run

    out = {}
    for kname, keys in (("int_seed", None), ("seed_list", seeds)):
        out[f"ddpm_{kname}"] = dict(start=start(1.0, keys, None), before=before(1.0, keys), with_source=start(1.0, keys, init))
        out[f"edm_{kname}"] = dict(start=start(80.0, keys, None), before=before(80.0, keys), with_source=start(80.0, keys, init))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    device = torch.device("cuda:0")
    fs = forms(device)
    flat = [(case, form, fn) for case, d in fs.items() for form, fn in d.items()]
    for _, _, fn in flat:   # warm-up: code objects, the allocator's blocks
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    us = {(case, form): [] for case, form, _ in flat}
    for _ in range(REPS):
        for case, form, fn in flat:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[case, form].append(round(e0.elapsed_time(e1) * 1e3 / CALLS, 2))
    rec = dict(what="kd_sample_start against the draw + copy (+ mul_) it replaces; microseconds per call, min and max of "
                    f"{REPS} warm repetitions of {CALLS} back-to-back calls between device events (host launch cost included)",
               shape=f"batch {B}, {CH} x {S}^2 (C3); with_source: a {SRC} x {SRC} init image", bytes_written=B * CH * S * S * 4,
               us_per_call={case: {form: dict(min=min(us[case, form]), max=max(us[case, form]), reps=us[case, form])
                                   for form in d} for case, d in fs.items()})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
