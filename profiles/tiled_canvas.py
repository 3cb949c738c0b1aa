"""Writes profiles/tiled_canvas.json: what fused-tile canvas sampling costs at the stage-3 shape.

  python profiles/tiled_canvas.py --out profiles/tiled_canvas.json [--canvas] [--grid N] [--steps T]

Kernel bandwidth (always): microseconds and achieved TB/s of kd_tiles_fuse_update and kd_tiles_gather on the 8 x 8 lattice
of 1024^2 tiles at overlap 0.25 (canvas 3 x 6400^2, 64 tiles), as a fraction of the 6.3 TB/s a streaming kernel reaches on
the MI355X.  Bytes are what the algorithm moves, from the shapes: the canvas read and written, the fused estimate written
(and read where the step has a history term), every tile element read once; a gather reads and writes its tiles once.
Five repetitions of 20 launches between two device events after 5 warm launches; min - max over the repetitions.

Canvas throughput (--canvas): patches/s of ultra_res.tiled.fused_canvas on the N x N grid (default 8) through the three
stages of train_ultra_res.py:29-60 at T steps per stage (default 8) and tile_batch 16, beside distributed.outpaint_canvas at
inpaint_resample 1 and 5 with max_batch 8 (stages 1 and 2; stage 3 one patch per call, as `bench.py --grid-batch 8` runs
it), in the same process; five warm runs each, min - max.  Two different algorithms: the numbers are reported side by
side, not against a target."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kidney-diffusion_amd"):
    sys.path.insert(0, str(p))

HBM_ACHIEVABLE = 6.3e12   # bytes / s of a streaming kernel on the MI355X (8 TB/s peak)
REPS, LAUNCHES, WARM = 5, 20, 5


def timed(fn):
    """[microseconds per launch] over REPS repetitions of LAUNCHES launches between two device events."""
    import torch

    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    return out


def rate(us, nbytes):
    tbs = [nbytes / (u * 1e-6) / 1e12 for u in us]
    return dict(us=dict(min=round(min(us), 1), max=round(max(us), 1)), bytes=nbytes,
                tb_per_s=dict(min=round(min(tbs), 3), max=round(max(tbs), 3)),
                of_achievable_hbm=dict(min=round(min(tbs) * 1e12 / HBM_ACHIEVABLE, 3), max=round(max(tbs) * 1e12 / HBM_ACHIEVABLE, 3)))


def kernels(device):
    import torch

    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import normalize_tiling

    lib = E.load()
    geo = normalize_tiling((64, 256, 1024), (8, 8), 0.25)[2]
    Cn, S, st, ny, nx, Hc, Wc = 3, geo["S"], geo["st"], geo["ny"], geo["nx"], geo["Hc"], geo["Wc"]
    N = len(geo["origins"])
    assert (Hc, Wc, N) == (6400, 6400, 64)
    g = torch.Generator(device=device).manual_seed(1)
    x = torch.randn(Cn, Hc, Wc, device=device, generator=g)
    x0bar = torch.zeros_like(x)
    store = torch.randn(N, Cn, S, S, device=device, generator=g)
    thr = torch.rand(N, device=device, generator=g) * 2 + 1
    tile_of = torch.tensor(geo["tile_of"], dtype=torch.int32, device=device)
    canvas_b, tiles_b = x.numel() * 4, store.numel() * 4
    out = {}

    def fuse(ramp, P, Sn):
        return lambda: E.check(lib.kd_tiles_fuse_update(E.ptr(x), E.ptr(x0bar), E.ptr(store), E.ptr(thr), C.c_void_p(tile_of.data_ptr()),
                                                        N, Cn, S, st, ny, nx, ramp, 0.9, 0.1, P, Sn, None, 7, (1 << 32) | 3,
                                                        E.current_stream()))

    for label, ramp, P, Sn in (("fuse_update first order, no noise (DDIM(0); uniform)", 0, 0.0, 0.0),
                               ("fuse_update first order, no noise (DDIM(0); ramp)", 1, 0.0, 0.0),
                               ("fuse_update with history (2M; uniform)", 0, -0.05, 0.0),
                               ("fuse_update with in-kernel Philox noise (ancestral, DDIM(eta); uniform)", 0, 0.0, 0.3)):
        x.normal_(generator=g)   # (x <- 0.9 x + ... stays bounded; fresh values per form all the same)
        nbytes = 3 * canvas_b + tiles_b + (canvas_b if P != 0 else 0)
        out[label] = rate(timed(fuse(ramp, P, Sn)), nbytes)
        assert bool(torch.isfinite(x).all())
    for B in (16, 64):
        dst = torch.empty(B, Cn, S, S, device=device)
        yx = (C.c_int * (2 * B))(*[v for o in geo["origins"][:B] for v in o])
        fn = lambda: E.check(lib.kd_tiles_gather(E.ptr(x), E.ptr(dst), B, Cn, Hc, Wc, S, yx, E.current_stream()))
        out[f"gather of {B} tiles"] = rate(timed(fn), 2 * dst.numel() * 4)
        assert torch.equal(dst[B - 1], x[:, geo["origins"][B - 1][0]:geo["origins"][B - 1][0] + S,
                                         geo["origins"][B - 1][1]:geo["origins"][B - 1][1] + S])
    return out


def canvas(device, n, T):
    """patches/s of fused_canvas and of outpaint_canvas (R = 1, 5) on an n x n grid, T steps per stage."""
    import torch

    import bench
    import imagen_pytorch as ip
    from ultra_res import distributed as D
    from ultra_res import tiled as UT

    kws = {i: dict(kw, cond_images_channels=0) for i, kw in bench.ULTRA_UNETS.items()}   # the unconditional outpainting driver
    imagens = {}

    def load_imagen(stage):
        if stage not in imagens:
            unets = tuple(ip.Unet(**kws[i]) if i == stage else ip.NullUnet() for i in (1, 2, 3))
            for i, u in enumerate(unets):
                if isinstance(u, ip.NullUnet):
                    u.lowres_cond = i > 0   # (train_ultra_res.py:65-75: the placeholder of an SR stage says so)
            imagens[stage] = ip.Imagen(unets=unets, image_sizes=(64, 256, 1024), timesteps=(T, T, T),
                                       pred_objectives=("noise",) * 3, random_crop_sizes=(None, None, 256),
                                       condition_on_text=False).to(device)
        return imagens[stage]

    def runs(label, fn):
        fn()   # plans, captured steps, conditioning tables
        torch.cuda.synchronize()
        secs = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            print(f"{label}: {secs[-1]:.2f} s", flush=True)
        return dict(patches_per_s=dict(min=round(n * n / max(secs), 3), max=round(n * n / min(secs), 3)),
                    seconds=[round(s, 3) for s in secs])

    label = "fused_canvas, tile_batch 16"
    out = {label: runs(label, lambda: UT.fused_canvas(load_imagen, num_patches_width=n, tile_batch=16, seed=1, device=device))}
    for R in (1, 5):   # max_batch as `bench.py --grid-batch 8` gives it: stage 3 keeps one patch per call (10 GB of workspace per sample)
        fn = D.imagen_sample_fn(load_imagen, R, device, seed=1, max_batch={1: 8, 2: 8, 3: 1})
        label = f"outpaint_canvas, inpaint_resample {R}, max_batch 8 (stage 3: 1)"
        out[label] = runs(label, lambda: D.outpaint_canvas(fn, n, overlap=0.25, device=device))
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--canvas", action="store_true")
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU path"
    device = torch.device("cuda:0")
    rec = dict(what="fused-tile canvas sampling at the stage-3 shape: 8 x 8 lattice of 1024^2 tiles, overlap 0.25, canvas 3 x 6400^2",
               device=torch.cuda.get_device_name(0), hbm_achievable_tb_per_s=HBM_ACHIEVABLE / 1e12,
               method=f"{REPS} repetitions of {LAUNCHES} launches between device events after {WARM} warm launches; min - max",
               kernels=kernels(device))
    if a.canvas:
        rec["canvas"] = dict(grid=a.grid, steps_per_stage=a.steps, results=canvas(device, a.grid, a.steps))
    else:
        rec["canvas"] = "not measured yet"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
