"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of a fused-tile canvas cut into
shards by lattice rows - ``Imagen.sample_tiled(devices=...)`` - in plain torch over tests/tiled_ref.py (cut, fuse,
CanvasSolver) and the loop of tests/tiled_known_ref.py.  Nothing here comes from imagen-pytorch: the library has no canvas.

Every shard holds a canvas, a solver (the 2M history) and a tile store of its own.  Per resample slot:

1. a shard denoises its OWN tiles, cut out of its own canvas (and, for a self-conditioned denoiser, out of its own fused
   estimate of the slot before);
2. its store is NaN everywhere but for those estimates and for the strips - rows ``row0 .. row0 + rows`` of a halo tile -
   that the exchange lists send it, copied out of the owner's store;
3. it fuses own and halo tiles in canvas order and runs the one update, the mix and the re-noise on its canvas, all of
   them with the canvas' noise; then its canvas is set to NaN outside its band extent.

So a shard never sees a value it would not hold on a device of its own, and a read outside what the decomposition
guarantees turns the result into NaN.  The owned rows of the shards, put together, are the canvas.  ``brute_cover`` is the
cover computation the strip ranges are checked against: pixel by pixel, no formula.
"""
from __future__ import annotations

import torch

import tiled_known_ref as KR
import tiled_ref as TR
from oracle.imagen_ref import exists

NAN = float("nan")


def brute_cover(geo, band):
    """For the band of lattice rows [r0, r1) of the lattice `geo` (normalize_tiling's dict): (extent, {tile: sorted local
    rows}) - the canvas rows that the band's own tiles cover, and for every OTHER present tile the rows of that tile that
    lie on a canvas row of the extent; found by marking rows one by one."""
    S, st, ny, tile_of = geo["S"], geo["st"], geo["ny"], geo["tile_of"]
    r0, r1 = band
    rows = set()
    for r in range(r0, r1):   # (the extent is stated for the band's lattice rows, whether a row holds a tile or not)
        rows.update(range(r * st, r * st + S))
    need = {}
    for r in range(ny):
        if r0 <= r < r1:
            continue
        local = sorted(y - r * st for y in range(r * st, r * st + S) if y in rows)
        if local:
            for t in tile_of[r]:
                if t >= 0:
                    need[t] = local
    return (min(rows), max(rows) + 1), need


def run_canvas_sharded(denoise_tiles, x, lat, plan, noise_scheduler, name, eta, noise_fn, stage, weights="uniform", known=None,
                       mask=None, R=1, skip=0):
    """tiled_known_ref.run_canvas over the shards of `plan` (one stage's dict of normalize_shards; `lat` the lattice of
    tiled_ref).  Returns (the canvas assembled from the owned rows, covered, the shards' canvases)."""
    S, origins = lat["S"], lat["origins"]
    w = TR.weight(S, lat["st"], weights)
    covered = KR.covered_of(lat)
    shape = tuple(x.shape)
    has_known = exists(known) and exists(mask)
    R = R if has_known else 1
    if has_known:
        kn, m = known * 2 - 1, mask & covered
    shards = plan["shards"]
    sub = lambda tiles: dict(lat, origins=[origins[t] for t in tiles])
    xs = [x.clone() for _ in shards]
    solvers = [TR.CanvasSolver(noise_scheduler, name, eta) for _ in shards]
    latest = [None for _ in shards]
    steps = solvers[0].steps
    T = len(steps)
    for k, (times, times_next) in enumerate(steps):
        if k < skip:
            continue
        for r in reversed(range(R)):
            zm = noise_fn(("inpaint", stage, k, r), shape) if has_known else None
            noise = noise_fn(("step", stage, k, r), shape) if solvers[0].wants_noise(k) else None
            zr = noise_fn(("renoise", stage, k, r), shape) if r > 0 and k < T - 1 else None
            stores = []
            for i, sh in enumerate(shards):   # 1. the own tiles, from the shard's own canvas
                if has_known:
                    xs[i] = torch.where(m, noise_scheduler.q_sample(kn, times, zm), xs[i])
                own = sub(sh["own"])
                n = len(sh["own"])
                prev = TR.cut(latest[i], own) if exists(latest[i]) else None
                x0c = denoise_tiles(k, times.expand(n), times_next.expand(n), TR.cut(xs[i], own), prev)
                store = torch.full((len(origins),) + tuple(x0c.shape[1:]), NAN, dtype=x0c.dtype)
                store[sh["own"]] = x0c
                stores.append(store)
            for e in plan["exchange"]:   # 2. the strips, out of the owner's store
                for t, row0, rows in e["items"]:
                    stores[e["dst"]][t, :, row0:row0 + rows] = stores[e["src"]][t, :, row0:row0 + rows]
            for i, sh in enumerate(shards):   # 3. the canvas step over own and halo, then NaN outside the extent
                x0bar, cov = TR.fuse(stores[i][sh["tiles"]], sub(sh["tiles"]), w)
                solver = solvers[i]
                kept = (solver.x0_prev, solver.h_prev)
                stepped = solver.step(k, xs[i], x0bar, noise)
                if r > 0:
                    solver.x0_prev, solver.h_prev = kept
                xi = torch.where(cov, stepped, xs[i])
                if exists(zr):
                    xi = torch.where(cov, noise_scheduler.q_sample_from_to(xi, times_next, times, zr), xi)
                e0, e1 = sh["extent"]
                xi[:, :, :e0], xi[:, :, e1:] = NAN, NAN
                x0bar[:, :, :e0], x0bar[:, :, e1:] = NAN, NAN
                xs[i], latest[i] = xi, x0bar
    out = torch.cat([xs[i][:, :, sh["owned"][0]:sh["owned"][1]] for i, sh in enumerate(shards)], dim=2)
    return out, covered, xs
