"""Writes profiles/tiled_known.json: what the three kernels of a canvas that keeps known pixels cost beside what they fuse,
and what regenerating a block of a finished level costs beside regenerating the level.

  python profiles/tiled_known.py --out profiles/tiled_known.json [--level] [--steps T]

Kernels (always), at the stage-3 shape - an 8 x 8 lattice of 1024^2 tiles, canvas 3 x 6400^2, the centre 3 x 3 block of tiles
unknown and the rest known (the mask of `fused_level(keep=level_keep_mask(rest))`): microseconds and achieved TB/s, five
repetitions of 20 launches between two device events after 5 warm launches, min - max, the variants of a group ALTERNATED
repetition by repetition in one process.  Bytes are what the algorithm moves, from the shapes and the mask's known share:
  canvas step   kd_tiles_fuse_update (2M: history read); kd_tiles_fuse_update_known with the mix of the next slot (R = 1),
                and with the re-noise as well (R = 2); the composition it replaces - kd_tiles_fuse_update, then re-noise and
                mix as torch ops over the canvas
  start         kd_tiles_start (Philox x_T, init image and first mix) beside kd_philox_normal x 2 and the torch expression
  end           kd_tiles_finalize_known beside kd_tiles_finalize into a copy and torch.where

Level (--level): a finished mag-1 level (8 x 8 tiles, canvas 6400^2, full-width models with random weights, T steps per
stage) - regenerating its centre 3 x 3 block with `canvas=`, `keep=` beside regenerating the whole level; three warm runs
each, min - max."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kidney-diffusion_amd"):
    sys.path.insert(0, str(p))

from tiled_canvas import HBM_ACHIEVABLE, LAUNCHES, REPS, WARM, rate   # noqa: E402  (profiles/ is the script's directory)


def alternated(fns):
    """{label: [microseconds per launch]} over REPS repetitions of LAUNCHES launches between two device events, the
    functions taking turns repetition by repetition after WARM warm launches each."""
    import torch

    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    return out


def kernels(device):
    import torch

    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import normalize_tiling
    from ultra_res import grid as G
    from ultra_res import tiled as UT

    lib = E.load()
    geo = normalize_tiling((64, 256, 1024), (8, 8), 0.25)[2]
    Cn, S, st, ny, nx, Hc, Wc = 3, geo["S"], geo["st"], geo["ny"], geo["nx"], geo["Hc"], geo["Wc"]
    N = len(geo["origins"])
    g = torch.Generator(device=device).manual_seed(1)
    stream = E.current_stream
    n = Cn * Hc * Wc
    block = [(i, j) for i in (3, 4, 5) for j in (3, 4, 5)]
    geom = G.GridGeometry(256, 192, 8, st, Hc)
    keep = UT.level_keep_mask(geom, [p for p in geom.positions if p not in block], device)
    known_share = float(keep.float().mean())
    kn = torch.rand(Cn, Hc, Wc, device=device, generator=g)
    x = torch.randn(Cn, Hc, Wc, device=device, generator=g)
    hist = torch.rand(Cn, Hc, Wc, device=device, generator=g)
    store = torch.randn(N, Cn, S, S, device=device, generator=g)
    tile_of = torch.tensor(geo["tile_of"], dtype=torch.int32, device=device)
    tof = C.c_void_p(tile_of.data_ptr())
    kn_s, km_s = E.tiles_image(kn), E.tiles_mask(keep)
    A, B, P, Sn, rn_a, rn_b, a, s, seed = 0.83, 0.21, -0.07, 0.0, 1.07, 0.31, 0.66, 0.75, 7
    sid = E.stream_id
    out = dict(known_share_of_the_canvas=round(known_share, 4))

    # ---- the canvas step (2M: x and the history read, x and the estimate written, every tile element read once)
    plain = lambda: E.check(lib.kd_tiles_fuse_update(E.ptr(x), E.ptr(hist), E.ptr(store), None, tof, N, Cn, S, st, ny, nx, 0, A, B, P,
                                                     Sn, None, seed, sid(1, 3), stream()))

    def known(renoise):
        return lambda: E.check(lib.kd_tiles_fuse_update_known(
            E.ptr(x), E.ptr(hist), E.ptr(hist), E.ptr(store), None, tof, N, Cn, S, st, ny, nx, 0, A, B, P, Sn, None, seed, sid(1, 3),
            renoise, rn_a, rn_b, None, sid(3, 3), E.ref(kn_s), E.ref(km_s), a, s, None, sid(2, 4), stream()))

    keep_b = keep.bool()
    zr, zm = torch.empty_like(x), torch.empty_like(x)

    def two_pass(renoise):
        def fn():
            plain()
            if renoise:
                E.check(lib.kd_philox_normal(E.ptr(zr), n, seed, sid(3, 3), stream()))
                x.mul_(rn_a).add_(zr * rn_b)
            E.check(lib.kd_philox_normal(E.ptr(zm), n, seed, sid(2, 4), stream()))
            x.copy_(torch.where(keep_b, a * (2 * kn - 1) + s * zm, x))
        return fn

    tiles_b = store.numel() * 4
    step_b = tiles_b + 4 * n * 4                       # tiles; x read and written, history read, estimate written
    # known: a known float4 skips x and the history; the mask is read per channel; the known image where the mask is set
    known_b = tiles_b + n * 4 * (2 + 2 * (1 - known_share) + known_share) + n
    us = alternated({"plain": plain, "known_R1": known(0), "two_pass_R1": two_pass(False), "known_R2": known(1),
                     "two_pass_R2": two_pass(True)})
    out["kd_tiles_fuse_update (2M)"] = rate(us["plain"], step_b)
    out["kd_tiles_fuse_update_known, mix of the next slot (R = 1)"] = rate(us["known_R1"], int(known_b))
    out["replaces: kd_tiles_fuse_update, then the mix as torch ops"] = dict(us=dict(min=round(min(us["two_pass_R1"]), 1),
                                                                                  max=round(max(us["two_pass_R1"]), 1)))
    out["kd_tiles_fuse_update_known, re-noise and mix (R = 2, a slot before the last)"] = rate(us["known_R2"], int(known_b))
    out["replaces: kd_tiles_fuse_update, then re-noise and mix as torch ops"] = dict(us=dict(min=round(min(us["two_pass_R2"]), 1),
                                                                                           max=round(max(us["two_pass_R2"]), 1)))

    # ---- the start of a stage
    init = torch.rand(Cn, Hc, Wc, device=device, generator=g)
    in_s = E.tiles_image(init)
    start = lambda: E.check(lib.kd_tiles_start(E.ptr(x), Cn, Hc, Wc, 1.0, None, seed, E.ref(in_s), E.ref(kn_s), E.ref(km_s), a, s, None,
                                               sid(2, 0), stream()))

    def start_torch():
        E.check(lib.kd_philox_normal(E.ptr(zr), n, seed, sid(16, 2), stream()))
        E.check(lib.kd_philox_normal(E.ptr(zm), n, seed, sid(2, 0), stream()))
        x.copy_(torch.where(keep_b, a * (2 * kn - 1) + s * zm, zr + (2 * init - 1)))

    us = alternated({"start": start, "torch": start_torch})
    start_b = n * 4 * (1 + (1 - known_share) + known_share) + n   # x written; init where unknown, known image where known; mask
    out["kd_tiles_start (Philox x_T, init image, first mix)"] = rate(us["start"], int(start_b))
    out["replaces: two Philox draws and the torch expression"] = dict(us=dict(min=round(min(us["torch"]), 1), max=round(max(us["torch"]), 1)))

    # ---- the end of a stage
    res = torch.rand(Cn, Hc, Wc, device=device, generator=g)
    res_s = E.tiles_image(res)
    fin_known = lambda: E.check(lib.kd_tiles_finalize_known(E.ptr(x), tof, N, Cn, S, st, ny, nx, E.ptr(res), Hc, Wc, 0, 0, E.ref(res_s),
                                                            E.ref(km_s), stream()))
    tmp = torch.empty_like(res)

    def fin_torch():
        E.check(lib.kd_tiles_finalize(E.ptr(x), tof, N, Cn, S, st, ny, nx, E.ptr(tmp), Hc, Wc, 0, 0, stream()))
        res.copy_(torch.where(keep_b, res, tmp))

    us = alternated({"known": fin_known, "torch": fin_torch})
    fin_b = n * 4 * ((1 - known_share) + 2 * known_share + (1 - known_share)) + n   # x where unknown; known read and written back
    out["kd_tiles_finalize_known (the known image is the canvas written)"] = rate(us["known"], int(fin_b))
    out["replaces: kd_tiles_finalize into a spare canvas and torch.where"] = dict(us=dict(min=round(min(us["torch"]), 1),
                                                                                        max=round(max(us["torch"]), 1)))
    return out


def level(device, T):
    """Regenerating the centre 3 x 3 block of a finished mag-1 level beside regenerating the level: seconds, min - max."""
    import torch

    import bench
    import imagen_pytorch as ip
    from ultra_res import pipeline as P
    from ultra_res import tiled as UT

    imagens = {}

    def load_imagen(stage):
        if stage not in imagens:
            unets = tuple(ip.Unet(**bench.ULTRA_UNETS[i]) if i == stage else ip.NullUnet() for i in (1, 2, 3))
            for i, u in enumerate(unets):
                if isinstance(u, ip.NullUnet):
                    u.lowres_cond = i > 0
            imagens[stage] = ip.Imagen(unets=unets, image_sizes=(64, 256, 1024), timesteps=(T, T, T), pred_objectives=("noise",) * 3,
                                       random_crop_sizes=(None, None, 256), condition_on_text=False).to(device)
        return imagens[stage]

    zoomed = torch.rand(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(3)).to(device)
    geom, pos = P.level_patches(zoomed, 1, 0.25)
    assert (geom.num_patches_width, geom.canvas_width, len(pos)) == (8, 6400, 64)
    block = [(i, j) for i in (3, 4, 5) for j in (3, 4, 5)]
    keep = UT.level_keep_mask(geom, [p for p in pos if p not in block], device)

    def runs(fn, reps=3):
        fn()   # plans, captured steps, conditioning tables
        torch.cuda.synchronize()
        secs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(round(time.perf_counter() - t0, 3))
            print(secs[-1], flush=True)
        return secs

    whole = lambda: P.generate_high_res_image_fused(load_imagen, zoomed, 1, tile_batch=16, seed=1, device=device)
    done = whole()
    out = {}
    for R in (1, 2):
        canvas = done.clone()
        part = lambda: P.generate_high_res_image_fused(load_imagen, zoomed, 1, patch_pos=block, tile_batch=16, seed=2, device=device,
                                                       canvas=canvas, keep=keep, known_resample_times=R)
        secs = runs(part)
        assert torch.equal(canvas[:, :, keep.bool()], done[:, :, keep.bool()])
        out[f"regenerate the centre 3 x 3 block (9 tiles), known_resample_times {R}"] = dict(seconds=secs)
    out["regenerate the level (64 tiles)"] = dict(seconds=runs(whole))
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--level", action="store_true")
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU path"
    device = torch.device("cuda:0")
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(what="a fused-tile canvas that keeps known pixels: the three kernels at the stage-3 shape (8 x 8 tiles of 3 x 1024^2, "
                    "canvas 3 x 6400^2, the centre 3 x 3 block unknown) and the partial regeneration of one mag-1 level",
               device=torch.cuda.get_device_name(0), hbm_achievable_tb_per_s=HBM_ACHIEVABLE / 1e12,
               method=f"{REPS} repetitions of {LAUNCHES} launches between device events after {WARM} warm launches, the variants "
                      "of a group alternated; min - max")
    write = lambda: (out.parent.mkdir(parents=True, exist_ok=True), out.write_text(json.dumps(rec, indent=1) + "\n"))
    rec["kernels"] = kernels(device)
    rec.setdefault("level", "not measured yet")
    write()
    if a.level:
        rec["level"] = dict(mag_level=1, grid=8, steps_per_stage=a.steps, results=level(device, a.steps))
        write()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
