"""Writes profiles/tiled_canvas_hist2.json: the canvas step with and without the second history at the stage-3 shape.

  python profiles/tiled_canvas_hist2.py --out profiles/tiled_canvas_hist2.json

As profiles/tiled_canvas.py measures kd_tiles_fuse_update: the 8 x 8 lattice of 1024^2 tiles at overlap 0.25 (canvas
3 x 6400^2, 64 tiles), microseconds and achieved TB/s against the 6.3 TB/s a streaming kernel reaches, five repetitions of
20 launches after 5 warm ones.  kd_tiles_fuse_update_known with one history (2M) beside kd_tiles_fuse_update_hist2 with two
(3M), the estimate written over the second history as sample_tiled does, and with in-kernel noise (3M-SDE).  Bytes from the
shapes: the canvas read and written, the estimate written, one canvas read per history, every tile element read once."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kidney-diffusion_amd", ROOT / "profiles"):
    sys.path.insert(0, str(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch

    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import normalize_tiling
    from tiled_canvas import rate, timed

    device = torch.device("cuda:0")
    lib = E.load()
    geo = normalize_tiling((64, 256, 1024), (8, 8), 0.25)[2]
    Cn, S, st, ny, nx, Hc, Wc = 3, geo["S"], geo["st"], geo["ny"], geo["nx"], geo["Hc"], geo["Wc"]
    N = len(geo["origins"])
    g = torch.Generator(device=device).manual_seed(1)
    x = torch.randn(Cn, Hc, Wc, device=device, generator=g)
    h1, h2 = torch.zeros_like(x), torch.zeros_like(x)
    store = torch.randn(N, Cn, S, S, device=device, generator=g)
    thr = torch.rand(N, device=device, generator=g) * 2 + 1
    tile_of = torch.tensor(geo["tile_of"], dtype=torch.int32, device=device)
    canvas_b, tiles_b = x.numel() * 4, store.numel() * 4
    head = lambda out, P, Sn: (E.ptr(x), E.ptr(h1), E.ptr(out), E.ptr(store), E.ptr(thr), C.c_void_p(tile_of.data_ptr()), N, Cn, S, st,
                              ny, nx, 0, 0.9, 0.1, P, Sn, None, 7, (1 << 32) | 3, 0, 0.0, 0.0, None, 0, None, None, 0.0, 0.0, None, 0)
    forms = {
        "one history (2M): kd_tiles_fuse_update_known, estimate over the history":
            (lambda: E.check(lib.kd_tiles_fuse_update_known(*head(h1, -0.05, 0.0), E.current_stream())), 1),
        "two histories (3M): kd_tiles_fuse_update_hist2, estimate over the second history":
            (lambda: E.check(lib.kd_tiles_fuse_update_hist2(*head(h2, -0.05, 0.0), E.ptr(h2), 0.02, E.current_stream())), 2),
        "two histories and in-kernel Philox noise (3M-SDE)":
            (lambda: E.check(lib.kd_tiles_fuse_update_hist2(*head(h2, -0.05, 0.3), E.ptr(h2), 0.02, E.current_stream())), 2),
    }
    out = {}
    for label, (fn, hists) in forms.items():
        x.normal_(generator=g)
        out[label] = rate(timed(fn), 3 * canvas_b + tiles_b + hists * canvas_b)
        assert bool(torch.isfinite(x).all())
        print(label, out[label], flush=True)
    rec = dict(what="the canvas step of fused-tile sampling with one and with two histories, 8 x 8 lattice of 1024^2 tiles, "
                    "canvas 3 x 6400^2, uniform weights, dynamic thresholds", kernels=out)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
