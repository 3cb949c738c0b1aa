"""Records tests/golden/tiles_plain_kernels.pt: what kd_tiles_fuse_update and kd_tiles_finalize write for the cases of
tests/test_tiles_plain_golden_gpu.py.  Needs the GPU.  The committed file was recorded on an MI355X with the library of
the last commit that had the plain kernels on their own (before tiles_fuse_update_kernel / tiles_finalize_kernel became
instantiations of the templates they now share with the known forms); recording it again from a later build only pins
that build to itself.

    python tests/golden/make_tiles_plain_kernels.py [OUT]
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "kidney-diffusion_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

import test_tiles_plain_golden_gpu as T  # noqa: E402


def main():
    device = torch.device("cuda:0")
    out = {}
    for name in T.FUSE:
        x, xb, _ = T.run_fuse(T.fuse_plain, name, device)
        out[f"fuse/{name}/x"], out[f"fuse/{name}/x0bar"] = x.cpu(), xb.cpu()
    for name in T.FINALIZE:
        wins = []
        for oy, ox in T.OFFSETS:
            res, before, win, cov = T.run_finalize(T.finalize_plain, name, oy, ox, device)
            untouched = torch.ones_like(res, dtype=torch.bool)
            untouched[win] = ~cov
            assert torch.equal(res[untouched], before[untouched]), (name, oy, ox)
            wins.append(torch.where(cov, res[win], torch.zeros_like(res[win])).cpu())
        assert all(torch.equal(T._bits(w), T._bits(wins[0])) for w in wins), name   # the covered values do not follow the offset
        out[f"finalize/{name}"] = wins[0]
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else T.GOLDEN
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save(out, path)
    print(f"{path}: {path.stat().st_size} bytes, {len(out)} tensors")


if __name__ == "__main__":
    main()
