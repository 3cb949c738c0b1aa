"""Writes profiles/fused_level.json: what the three level kernels of csrc/kernels_tiles.hip cost beside what they replace,
one mag-1 level end to end, its peak memory, and whether torch's nearest interpolate takes the mag-2 canvas.

  python profiles/fused_level.py --out profiles/fused_level.json [--level [--parts fused,r1,r5]] [--steps T] [--probe]

Kernels (always), at the stage-3 shape - a chunk of 16 tiles of 3 x 1024^2 out of a 3 x 6400^2 source (the level above at
mag 2), a 3 x 1600^2 previous canvas and a 3 x 6400^2 canvas (8 x 8 tiles): microseconds and achieved TB/s, five
repetitions of 20 launches between two device events after 5 warm launches, min - max.  Bytes are what the algorithm
moves, from the shapes.  Beside each kernel, what the default path of Imagen._tiled_stage does in its place:
  kd_tiles_cond_gather    the copy of the chunk out of the materialised [N, 3, 1024, 1024] conditioning tiles
  kd_tiles_gather_lowres  kd_tiles_gather out of the materialised low-res canvas, and that canvas' one-off build
                          (interpolate, * 2 - 1, a * ... + s * gauss) - once per stage, not per chunk
  kd_tiles_finalize       the torch finish (host mask tile by tile, upload, clamp, + 1, * 0.5, where, zeros_like), timed by
                          the host clock around a device synchronise: it holds host work

Level (--level): one mag-1 level (zoomed image 1024^2, 8 x 8 tiles, canvas 6400^2) through
pipeline.generate_high_res_image_fused, beside pipeline.generate_high_res_image over distributed.imagen_sample_fn at
inpaint_resample 1 and 5, with the models, T steps per stage (default 8), tile_batch 16 and max_batch {1: 8, 2: 8, 3: 1} of
profiles/tiled_canvas.py --canvas, here with the 3 conditioning channels a level has; five warm runs each, min - max.
torch.cuda.max_memory_allocated of the fused level, and of the same level with everything materialised
(cond_images_for_grid tiles, streamed=False, pasted in torch): torch's allocations only, the engine's plans are its own.

Probe (--probe, last: nothing runs behind it): F.interpolate(..., "nearest") to 3 x 40960^2, accepted or refused."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kidney-diffusion_amd"):
    sys.path.insert(0, str(p))

from tiled_canvas import HBM_ACHIEVABLE, LAUNCHES, REPS, WARM, rate, timed   # noqa: E402  (profiles/ is the script's directory)


def host_timed(fn):
    """[microseconds per call] by the host clock around a device synchronise, REPS calls after one warm call."""
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def kernels(device):
    import torch
    import torch.nn.functional as F

    from imagen_pytorch import _engine as E
    from imagen_pytorch import cond_crop_maps
    from imagen_pytorch.imagen_pytorch import normalize_tiling
    from ultra_res import grid as G

    lib = E.load()
    geo = normalize_tiling((64, 256, 1024), (8, 8), 0.25)[2]
    Cn, S, st, ny, nx, Hc, Wc = 3, geo["S"], geo["st"], geo["ny"], geo["nx"], geo["Hc"], geo["Wc"]
    N, B = len(geo["origins"]), 16
    g = torch.Generator(device=device).manual_seed(1)
    tile_b = B * Cn * S * S * 4
    stream = E.current_stream
    out = {}

    # conditioning tiles: 16 tiles of the mag-2 lattice's middle rows out of the 6400^2 level above
    W = 6400
    src = torch.rand(Cn, W, W, device=device, generator=g)
    geom = G.GridGeometry(161, 120, 53, 768, 40960)
    pos = [(26, j) for j in range(20, 20 + B)]
    shifts = [(W // 2 - (i * 120 + 80), W // 2 - (j * 120 + 80)) for i, j in pos]
    yx = (C.c_int * (2 * B))(*[v for sh in shifts for v in sh])
    win = cond_crop_maps(1024, S)[0].to(device)
    dst = torch.empty(B, Cn, S, S, device=device)
    top = G.center_crop_offset(W, 1024)
    fn = lambda: E.check(lib.kd_tiles_cond_gather(E.ptr(src), Cn, W, E.ptr(dst), B, S, yx, top, C.c_void_p(win.data_ptr()), None,
                                                  0.95, stream()))
    out["kd_tiles_cond_gather, 16 tiles"] = rate(timed(fn), 2 * tile_b)
    mat = G.cond_images_for_grid(src[None], geom, pos, fill_color=0.95)
    assert torch.equal(dst, mat)
    out["replaces: copy of the chunk out of materialised tiles"] = rate(timed(lambda: dst.copy_(mat)), 2 * tile_b)
    out["materialised conditioning tiles it does without, bytes"] = dict(mag1_64_tiles=64 * Cn * S * S * 4,
                                                                         mag2_2809_tiles=2809 * Cn * S * S * 4)
    del mat, src

    # low-res conditioning tiles out of the 1600^2 canvas of stage 2
    prev = torch.rand(1, Cn, 1600, 1600, device=device, generator=g)
    oyx = (C.c_int * (2 * B))(*[v for o in geo["origins"][:B] for v in o])
    a, s, seed, sid = 0.9689, 0.2474, 7, (16 << 32) | 1
    fn = lambda: E.check(lib.kd_tiles_gather_lowres(E.ptr(prev), 1600, 1600, E.ptr(dst), B, Cn, Hc, Wc, S, oyx, a, s, None, seed,
                                                    sid, stream()))
    out["kd_tiles_gather_lowres, 16 tiles, Philox noise"] = rate(timed(fn), tile_b + tile_b // 16)
    got = dst.clone()

    def build():
        z = torch.empty(1, Cn, Hc, Wc, device=device)
        E.check(lib.kd_philox_normal(E.ptr(z), z.numel(), seed, sid, stream()))
        low = F.interpolate(prev, (Hc, Wc), mode="nearest") * 2 - 1
        return (a * low + s * z).contiguous()

    low = build()
    fn = lambda: E.check(lib.kd_tiles_gather(E.ptr(low), E.ptr(dst), B, Cn, Hc, Wc, S, oyx, stream()))
    out["replaces: kd_tiles_gather out of the materialised low-res canvas"] = rate(timed(fn), 2 * tile_b)
    assert torch.equal(dst, got)
    us = timed(build)
    out["replaces: one-off build of that canvas, per stage"] = dict(us=dict(min=round(min(us), 1), max=round(max(us), 1)),
                                                                    canvas_bytes=low.numel() * 4)
    del low, prev

    # the end of a stage: the 6400^2 canvas into a 6400^2 output
    x = torch.randn(Cn, Hc, Wc, device=device, generator=g) * 1.5
    res = torch.zeros(Cn, Hc, Wc, device=device)
    tile_of = torch.tensor(geo["tile_of"], dtype=torch.int32, device=device)
    fn = lambda: E.check(lib.kd_tiles_finalize(E.ptr(x), C.c_void_p(tile_of.data_ptr()), N, Cn, S, st, ny, nx, E.ptr(res), Hc, Wc,
                                               0, 0, stream()))
    out["kd_tiles_finalize, canvas 6400^2"] = rate(timed(fn), 2 * x.numel() * 4)

    def finish():
        covered = torch.zeros(Hc, Wc, dtype=torch.bool)
        for y0, x0 in geo["origins"]:
            covered[y0:y0 + S, x0:x0 + S] = True
        o = (x.clamp(-1.0, 1.0) + 1) * 0.5
        return torch.where(covered.to(device), o, torch.zeros_like(o))

    assert torch.equal(res, finish())
    us = host_timed(finish)
    out["replaces: the torch finish (host mask, upload, five canvas ops), host clock"] = dict(
        us=dict(min=round(min(us), 1), max=round(max(us), 1)))
    return out


def level(device, T, parts):
    """One mag-1 level end to end: seconds and patches/s of the fused level and of the sequential one (R = 1, 5); peak memory."""
    import torch

    import bench
    import imagen_pytorch as ip
    from ultra_res import distributed as D
    from ultra_res import grid as G
    from ultra_res import pipeline as P
    from ultra_res import tiled as UT

    imagens = {}

    def load_imagen(stage):
        if stage not in imagens:
            unets = tuple(ip.Unet(**bench.ULTRA_UNETS[i]) if i == stage else ip.NullUnet() for i in (1, 2, 3))
            for i, u in enumerate(unets):
                if isinstance(u, ip.NullUnet):
                    u.lowres_cond = i > 0   # (train_ultra_res.py:65-75: the placeholder of an SR stage says so)
            imagens[stage] = ip.Imagen(unets=unets, image_sizes=(64, 256, 1024), timesteps=(T, T, T),
                                       pred_objectives=("noise",) * 3, random_crop_sizes=(None, None, 256),
                                       condition_on_text=False).to(device)
        return imagens[stage]

    zoomed = torch.rand(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(3)).to(device)
    geom, pos = P.level_patches(zoomed, 1, 0.25)
    assert (geom.num_patches_width, geom.canvas_width, len(pos)) == (8, 6400, 64)

    last = {}

    def runs(label, fn):
        fn()   # plans, captured steps, conditioning tables
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(device)
        secs = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            assert tuple(r.shape) == (1, 3, 6400, 6400)
            last[label] = r
            del r
            print(f"{label}: {secs[-1]:.2f} s", flush=True)
        return dict(patches_per_s=dict(min=round(64 / max(secs), 3), max=round(64 / min(secs), 3)),
                    seconds=[round(s, 3) for s in secs], max_memory_allocated_gb=round(torch.cuda.max_memory_allocated(device) / 1e9, 3))

    def materialised():   # the same level without the three arguments: every piece built in full
        cond = G.cond_images_for_grid(zoomed, geom, pos, fill_color=0.95)
        tiles = UT.fused_canvas(load_imagen, num_patches_width=8, tile_batch=16, seed=1, cond_images=cond, device=device)
        full = torch.nn.functional.interpolate(zoomed, size=(6400, 6400), mode="bilinear", align_corners=False)
        full.copy_(tiles)   # (8 x 8 present tiles cover the canvas)
        return full

    out = {}
    if "fused" in parts:
        label = "generate_high_res_image_fused (streamed, cond_crops, into), tile_batch 16"
        out[label] = runs(label, lambda: P.generate_high_res_image_fused(load_imagen, zoomed, 1, tile_batch=16, seed=1, device=device))
        label = "the same level with everything materialised (cond_images, streamed=False, pasted in torch), tile_batch 16"
        out[label] = runs(label, materialised)
        a, b = last.values()
        out["the two canvases are bit-equal"] = bool(torch.equal(a, b))
        last.clear()
    for R in (1, 5):
        if f"r{R}" not in parts:
            continue
        fn = D.imagen_sample_fn(load_imagen, R, device, seed=1, max_batch={1: 8, 2: 8, 3: 1})
        label = f"generate_high_res_image, inpaint_resample {R}, max_batch 8 (stage 3: 1)"
        out[label] = runs(label, lambda: P.generate_high_res_image(fn, zoomed, 1, overlap=0.25, device=device))
    return out


def probe(device):
    """F.interpolate(..., "nearest") to 3 x 40960^2 (6.7e9 elements): what Imagen._tiled_stage would ask of torch at mag 2."""
    import torch
    import torch.nn.functional as F

    prev = torch.rand(1, 3, 10240, 10240, device=device, generator=torch.Generator(device=device).manual_seed(2))
    try:
        up = F.interpolate(prev, (40960, 40960), mode="nearest")
        torch.cuda.synchronize()
    except RuntimeError as e:
        return dict(accepted=False, error=str(e).splitlines()[0][:300])
    ys = torch.tensor([0, 1, 4097, 20479, 32768, 40959], device=device)
    ok = torch.equal(up[0][:, ys][:, :, ys], prev[0][:, ys // 4][:, :, ys // 4])
    return dict(accepted=True, sampled_points_right=bool(ok), output_gb=round(up.numel() * 4 / 1e9, 1))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--level", action="store_true")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--parts", default="fused,r1,r5", help="--level: which of its runs (a later call adds to the file)")
    ap.add_argument("--probe", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU path"
    device = torch.device("cuda:0")
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(what="a fused-tile stage at the sizes of a magnification level: the three level kernels at the stage-3 shape "
                    "(16 tiles of 3 x 1024^2; source 6400^2, previous canvas 1600^2, canvas 6400^2) and one mag-1 level",
               device=torch.cuda.get_device_name(0), hbm_achievable_tb_per_s=HBM_ACHIEVABLE / 1e12,
               method=f"{REPS} repetitions of {LAUNCHES} launches between device events after {WARM} warm launches; min - max")
    write = lambda: (out.parent.mkdir(parents=True, exist_ok=True), out.write_text(json.dumps(rec, indent=1) + "\n"))
    rec["kernels"] = kernels(device)
    rec.setdefault("level", "not measured yet")
    rec.setdefault("nearest_interpolate_to_3x40960x40960", "not measured yet")
    write()
    if a.level:
        lv = rec["level"] if isinstance(rec["level"], dict) and rec["level"].get("steps_per_stage") == a.steps else \
            dict(mag_level=1, grid=8, steps_per_stage=a.steps, results={})
        lv["results"].update(level(device, a.steps, a.parts.split(",")))
        rec["level"] = lv
        write()
    if a.probe:
        rec["nearest_interpolate_to_3x40960x40960"] = probe(device)
        write()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
