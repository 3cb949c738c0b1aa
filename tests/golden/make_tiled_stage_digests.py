"""Records tests/golden/tiled_stage_digests.json: the SHA-256 of the canvas that Imagen.sample_tiled returns for every
case of tests/test_tiled_stage_golden_gpu.py (the whole `into` canvas where a case has one), and for its sharded cases.
Needs the GPU.  The committed file was recorded on an MI355X in a checkout of the last commit that had the whole stage
driver inside Imagen._tiled_stage, with this file and the test module copied in and nothing else changed; a digest
recorded from a later tree only pins that tree to itself.

    python tests/golden/make_tiled_stage_digests.py [OUT]
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "kidney-diffusion_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

import test_tiled_stage_golden_gpu as T  # noqa: E402


def main():
    device = torch.device("cuda:0")
    models, out = {}, {}
    model = lambda name: models.setdefault(T.CASES[name]["model"], T.build_model(T.CASES[name]["model"], device))
    for name in T.CASES:
        out[name] = T.digest(T.run_case(name, model(name), device))
        print(name, out[name], flush=True)
    for name, base in T.SHARDED.items():
        out[name] = T.digest(T.run_case(base, model(base), device, shards=3))
        print(name, out[name], flush=True)
        assert out[name] == out[base], f"{name}: three shards differ from {base}"
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else T.GOLDEN
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(f"{path}: {path.stat().st_size} bytes, {len(out)} digests")


if __name__ == "__main__":
    main()
