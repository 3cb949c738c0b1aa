"""Writes profiles/tiled_sharded.json: what cutting a fused-tile canvas into shards costs, and what it gives on several GPUs.

  python profiles/tiled_sharded.py --out profiles/tiled_sharded.json [--canvas] [--lists "none;0,0;0,0,0,0"] [--steps T]
  python profiles/tiled_sharded.py --default-call --out FILE      # the devices=None call alone (run it on two commits, alternated)
  python profiles/tiled_sharded.py --merge-default-call --out profiles/tiled_sharded.json --parent P1.json P2.json \
      --this T1.json T2.json --bench-parent MS MS --bench-this MS MS --bench-dumps-equal yes        # no GPU needed

The section "default_call_against_the_parent_commit" of the JSON is written by no measuring run of this script: it compares
two commits, and one checkout holds one.  It is made in one session that alternates parent / this tree / parent / this tree,
in each tree `bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs` and then this script with --default-call, and is put
into the JSON by --merge-default-call: the --default-call files of the parent and of this tree in the order they were run,
the ms per step that bench.py printed, and whether its dumps compared equal (`cmp`).  A measuring run re-loads the JSON first
and leaves the section as it is.

Kernel (always): kd_tiles_rows_copy per launch at the stage-3 shape - 32 strips of 3 x 256 x 1024 fp32 (the overlap rows of
32 boundary tiles of 1024^2 at stride 768) with their thresholds: pack (tile store -> strip buffer), unpack (strip buffer ->
tile store) and store -> store; microseconds and achieved TB/s, five repetitions of 20 launches between two device events
after 5 warm launches, min - max, beside the streaming figure the project quotes (6.3 TB/s).  Bytes are what the copy moves:
every strip read once and written once.

Canvas (--canvas): seconds per canvas of the STAGE-3 canvas - an 8 x 8 lattice of 1024^2 tiles (canvas 6400^2), tile_batch
16, T steps (default 8), the SR-1024 UNet of train_ultra_res.py:50-60 on the stage-2 canvas of a fixed seed - for every
device list of --lists ("none" = devices=None; "0,0" = two shards on device 0; "0,1,2,3" = four devices).  One warm run of
every list, then five timed rounds that walk the lists in turn (alternated, one session), min - max; every list's canvas is
compared with the first list's (bit-equal where the chunks have one batch size: 64 tiles over 1, 2, 4 or 8 shards in chunks
of 16 or 8).  The default lists: on one GPU none, 2 and 4 shards on it - the cost of the decomposition (halo re-fusion, pack /
copy / unpack, a full-canvas pass per shard), nothing gained; with more GPUs none, then 2, 4, 8 distinct devices as far
as they go."""
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


def kernel(device):
    import torch

    from imagen_pytorch import _engine as E

    lib = E.load()
    Cn, S, rows, n, N = 3, 1024, 256, 32, 48
    g = torch.Generator(device=device).manual_seed(1)
    a, b = torch.randn(N, Cn, S, S, device=device, generator=g), torch.zeros(N, Cn, S, S, device=device)
    thr_a, thr_b = torch.rand(N, device=device, generator=g), torch.zeros(N, device=device)
    words = n * Cn * rows * S
    buf = torch.empty(words + n, device=device)
    tail = C.c_void_p(buf.data_ptr() + 4 * words)
    flat = lambda quads: (C.c_int * (4 * n))(*[v for q in quads for v in q])
    pack = flat((N - n + m, m, S - rows, rows) for m in range(n))
    unpack = flat((m, m, S - rows, rows) for m in range(n))
    across = flat((N - n + m, m, S - rows, rows) for m in range(n))
    stream = E.current_stream
    moved = 2 * words * 4
    out = {}
    fn = lambda: E.check(lib.kd_tiles_rows_copy(E.ptr(a), N, S, E.ptr(buf), n, rows, E.ptr(thr_a), tail, n, Cn, S, pack, stream()))
    out["pack: 32 strips of 3 x 256 x 1024 out of a tile store into the strip buffer"] = rate(timed(fn), moved)
    fn = lambda: E.check(lib.kd_tiles_rows_copy(E.ptr(buf), n, rows, E.ptr(b), N, S, tail, E.ptr(thr_b), n, Cn, S, unpack, stream()))
    out["unpack: the strip buffer into the halo slots of a tile store"] = rate(timed(fn), moved)
    assert torch.equal(b[:n, :, S - rows:], a[N - n:, :, S - rows:]) and not bool(b[:n, :, :S - rows].any())
    assert torch.equal(thr_b[:n], thr_a[N - n:])
    fn = lambda: E.check(lib.kd_tiles_rows_copy(E.ptr(a), N, S, E.ptr(b), N, S, None, None, n, Cn, S, across, stream()))
    out["store to store, the same strips"] = rate(timed(fn), moved)
    fn = lambda: buf[:words].copy_(b.view(-1)[:words])
    out["beside it: torch copy_ of a contiguous buffer of that size"] = rate(timed(fn), moved)
    return out


def models(device, T):
    import torch

    import bench
    import imagen_pytorch as ip

    kws = {i: dict(kw, cond_images_channels=0) for i, kw in bench.ULTRA_UNETS.items()}
    unets = tuple(ip.Unet(**kws[i]) if i == 3 else ip.NullUnet() for i in (1, 2, 3))
    for i, u in enumerate(unets):
        if isinstance(u, ip.NullUnet):
            u.lowres_cond = i > 0   # (train_ultra_res.py:65-75: the placeholder of an SR stage says so)
    imagen = ip.Imagen(unets=unets, image_sizes=(64, 256, 1024), timesteps=(T, T, T), pred_objectives=("noise",) * 3,
                       random_crop_sizes=(None, None, 256), condition_on_text=False).to(device)
    start = torch.rand(1, 3, 1600, 1600, generator=torch.Generator().manual_seed(5)).to(device)   # the canvas of stage 2
    return imagen, start


def parse_lists(text):
    import torch

    if text is None:
        n = torch.cuda.device_count()
        if n == 1:
            return [None, [0, 0], [0, 0, 0, 0]]
        return [None] + [list(range(k)) for k in (2, 4, 8) if k <= n]
    return [None if part.strip() == "none" else [int(v) for v in part.split(",")] for part in text.split(";")]


def canvas(device, T, lists):
    import torch

    from ultra_res import tiled as UT

    imagen, start = models(device, T)
    name = lambda devs: "devices=None" if devs is None else f"devices={devs} ({len(devs)} shards on {len(set(devs))} GPU)"
    run = lambda devs: UT.fused_canvas(lambda stage: imagen, num_patches_width=8, stages=(3,), start_canvas=start, tile_batch=16,
                                       seed=1, device=device, devices=None if devs is None else [torch.device("cuda", i) for i in devs])
    out, live, first = {}, [], None
    for devs in lists:   # plans, captured steps, conditioning tables
        try:
            r = run(devs)
            torch.cuda.synchronize()
        except torch.cuda.OutOfMemoryError as e:   # a list this box cannot hold (plans of every shard stay resident): recorded;
            out[name(devs)] = dict(not_measured=f"{type(e).__name__}: {str(e).splitlines()[0][:300]}")   # any other error ends the script
            continue
        first = r if first is None else first
        out[name(devs)] = dict(seconds=[], equals_the_first_list=bool(torch.equal(r, first)),
                               max_abs_diff_to_the_first_list=float((r - first).abs().max()))
        live.append(devs)
        del r
    for _ in range(REPS):
        for devs in live:
            t0 = time.perf_counter()
            r = run(devs)
            torch.cuda.synchronize()
            out[name(devs)]["seconds"].append(round(time.perf_counter() - t0, 3))
            print(f"{name(devs)}: {out[name(devs)]['seconds'][-1]:.2f} s", flush=True)
            del r
    for devs in live:
        rec = out[name(devs)]
        rec["seconds_per_canvas"] = dict(min=min(rec["seconds"]), max=max(rec["seconds"]))
        rec["patches_per_s"] = dict(min=round(64 / max(rec["seconds"]), 3), max=round(64 / min(rec["seconds"]), 3))
    return out


def default_call(device, T):
    """The devices=None call alone: seconds of the stage-3 canvas, REPS warm runs."""
    import torch

    from ultra_res import tiled as UT

    imagen, start = models(device, T)
    run = lambda: UT.fused_canvas(lambda stage: imagen, num_patches_width=8, stages=(3,), start_canvas=start, tile_batch=16, seed=1,
                                  device=device)
    r = run()
    torch.cuda.synchronize()
    secs = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        r = run()
        torch.cuda.synchronize()
        secs.append(round(time.perf_counter() - t0, 3))
    import hashlib

    return dict(seconds=secs, sha256_of_the_canvas=hashlib.sha256(r.cpu().numpy().tobytes()).hexdigest())


def merge_default_call(out, a):
    """The section "default_call_against_the_parent_commit" out of --default-call files of both commits (see the top)."""
    load = lambda files: [json.loads(Path(f).read_text()) for f in files]
    parent, this = load(a.parent), load(a.this)
    assert parent and this, "--merge-default-call needs --parent and --this files"
    shas = {r["sha256_of_the_canvas"] for r in parent + this}
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec["default_call_against_the_parent_commit"] = dict(
        what="alternated in one session, parent / this tree / parent / this tree: bench.py --gpus 1 --steps 20 --warmup 3 "
             "--dump-outputs, then profiles/tiled_sharded.py --default-call (the stage-3 canvas by sample_tiled(devices=None), "
             f"{REPS} warm runs each)",
        bench_ms_per_step=dict(parent=a.bench_parent, this_tree=a.bench_this),
        bench_dump_outputs_bit_equal=None if a.bench_dumps_equal is None else a.bench_dumps_equal == "yes",
        default_sample_tiled_seconds=dict(parent=[r["seconds"] for r in parent], this_tree=[r["seconds"] for r in this]),
        default_sample_tiled_canvas_sha256_equal=len(shas) == 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--canvas", action="store_true")
    ap.add_argument("--default-call", action="store_true")
    ap.add_argument("--lists", default=None, help='device lists, ";" between them: "none;0,0;0,1,2,3"')
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--merge-default-call", action="store_true")
    ap.add_argument("--parent", nargs="*", default=[], help="--default-call files of the parent commit, in run order")
    ap.add_argument("--this", nargs="*", default=[], help="--default-call files of this tree, in run order")
    ap.add_argument("--bench-parent", nargs="*", type=float, default=[], help="bench.py ms per step on the parent commit")
    ap.add_argument("--bench-this", nargs="*", type=float, default=[], help="bench.py ms per step on this tree")
    ap.add_argument("--bench-dumps-equal", choices=("yes", "no"), default=None, help="bench.py --dump-outputs compared equal")
    a = ap.parse_args()
    out = Path(a.out)
    write = lambda rec: (out.parent.mkdir(parents=True, exist_ok=True), out.write_text(json.dumps(rec, indent=1) + "\n"))
    if a.merge_default_call:
        write(merge_default_call(out, a))
        return
    import torch

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU path"
    device = torch.device("cuda:0")
    if a.default_call:
        rec = dict(what="the stage-3 canvas (8 x 8 tiles of 1024^2, tile_batch 16) by sample_tiled(devices=None)",
                   device=torch.cuda.get_device_name(0), steps=a.steps, **default_call(device, a.steps))
        write(rec)
        print(json.dumps(rec))
        return
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(what="a fused-tile canvas cut into shards by lattice rows (sample_tiled(devices=...)): kd_tiles_rows_copy per launch, "
                    "and the stage-3 canvas (8 x 8 tiles of 1024^2, canvas 6400^2, tile_batch 16) over device lists",
               device=torch.cuda.get_device_name(0), gpus_visible=torch.cuda.device_count(),
               hbm_achievable_tb_per_s=HBM_ACHIEVABLE / 1e12,
               method=f"kernel: {REPS} repetitions of {LAUNCHES} launches between device events after {WARM} warm launches; canvas: one "
                      f"warm run of every list, then {REPS} rounds over the lists in turn, host clock around a device synchronise; min - max")
    rec["kd_tiles_rows_copy"] = kernel(device)
    rec.setdefault("canvas", "not measured yet")
    if torch.cuda.device_count() == 1:
        rec["several_gpus"] = "not measured: one GPU"
    write(rec)
    if a.canvas:
        rec["canvas"] = dict(steps=a.steps, results=canvas(device, a.steps, parse_lists(a.lists)))
        write(rec)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
