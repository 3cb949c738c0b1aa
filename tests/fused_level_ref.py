"""TEST INFRASTRUCTURE ONLY: pure-torch restatements of the three level kernels of csrc/kernels_tiles.hip, written from
their descriptions in include/kd_engine.h, and the cases the CPU and the GPU tests of the fused level share.

kd_tiles_cond_gather   per axis, output coordinate p of a tile with shift sh: w = map[p], g = top + w; filled when
                       sh > 0 ? g < sh : g >= (W + sh) % W, else source index (g - sh) mod W; a pixel is `fill` if either
                       axis is filled; channels Cs + c go through the centre map.
kd_tiles_gather_lowres a (2 nearest(prev) - 1) + s z, cut per tile; nearest is min(floor(fp32(dst) * (fp32(in) / fp32(out))),
                       in - 1).
kd_tiles_finalize      (clamp(x, -1, 1) + 1) * 0.5 over the pixels a present tile covers, pasted at (oy, ox).
"""
from __future__ import annotations

import contextlib

import torch


def cond_gather(src, shifts, top, win_of, centre_of, fill):
    """src [Cs, W, W], shifts [(sy, sx)] -> [B, Cs | 2 Cs, S, S] on src's device."""
    Cs, W, _ = src.shape
    dev = src.device

    def axis(sh, m):
        g = top + m.to(dev).long()
        filled = (g < sh) if sh > 0 else (g >= (W + sh) % W)
        return torch.remainder(g - sh, W), filled

    out = []
    for sy, sx in shifts:
        parts = []
        for m in (win_of, centre_of):
            if m is None:
                continue
            (ry, fy), (rx, fx) = axis(sy, m), axis(sx, m)
            t = src[:, ry][:, :, rx]
            t = torch.where((fy[:, None] | fx[None, :])[None], torch.full_like(t, fill), t)
            parts.append(t)
        out.append(torch.cat(parts, 0))
    return torch.stack(out)


def nearest_index(n_in, n_out):
    """torch's nearest source index of every output coordinate, in fp32 as the device kernels compute it."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    return (torch.arange(n_out, dtype=torch.float32) * scale).floor().long().clamp_(max=n_in - 1)


def finish(x, origins, S):
    """The torch finish of Imagen._tiled_stage: ((clamp(x) + 1) / 2 where a tile lies, covered [Hc, Wc])."""
    covered = torch.zeros(x.shape[-2:], dtype=torch.bool)
    for y0, x0 in origins:
        covered[y0:y0 + S, x0:x0 + S] = True
    return (x.clamp(-1.0, 1.0) + 1) * 0.5, covered.to(x.device)


@contextlib.contextmanager
def window_of(G, window):
    """ultra_res.grid with its crop window (PATCH_SIZE, 1024) set to `window` for the block: cond_images_for_grid at toy sizes."""
    keep = G.PATCH_SIZE
    G.PATCH_SIZE = window
    try:
        yield
    finally:
        G.PATCH_SIZE = keep


def materialised(G, zoomed, geom, pos, window, S, fill, v2):
    """resize_image_to(cond_images_for_grid(...), S): what the fused path used to hold per tile."""
    from imagen_pytorch.imagen_pytorch import resize_image_to

    with window_of(G, window):
        return resize_image_to(G.cond_images_for_grid(zoomed, geom, pos, fill_color=fill, centre_crop_channels=v2), S)


def shifts_of(W, geom, pos):
    h = geom.patch_width // 2
    return [(W // 2 - (i * geom.patch_dist + h), W // 2 - (j * geom.patch_dist + h)) for i, j in pos]


# (W, window, GridGeometry arguments, positions, tile sizes): the toy lattice with its shift-0 row and column and the
# half-to-even offset, then the pipeline's real numbers at a few positions, corners included
def cond_cases(G):
    toy = G.GridGeometry(8, 6, 7, 24, 176)
    every = [(i, j) for i in range(7) for j in range(7)]
    return [
        ("toy W44", 44, 24, toy, every, (24, 16, 8)),
        ("toy W45", 45, 24, toy, every, (24, 16, 8)),
        ("mag 1", 1024, 1024, G.GridGeometry(166, 124, 8, 768, 6400), [(0, 0), (0, 7), (3, 4), (7, 0), (7, 7)], (1024, 256)),
        ("mag 2", 6400, 1024, G.GridGeometry(161, 120, 53, 768, 40960), [(0, 0), (26, 26), (52, 52), (26, 0)], (1024, 64)),
    ]
