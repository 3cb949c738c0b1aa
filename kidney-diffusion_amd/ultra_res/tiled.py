"""Fused-tile canvas driver: the counterpart of `distributed.outpaint_canvas` in which the tiles of a canvas are denoised
together (`Imagen.sample_tiled`: MultiDiffusion / Mixture of Diffusers) instead of one after the other with inpainted overlap
strips (reference: outpainting.py:173-243, sample_ultra_res.py:183-195).  No inpainting, no resampling, no waves: every
schedule step runs all tiles in full batches and one canvas update.  `fused_level` is the counterpart of
`pipeline.generate_high_res_image`: one magnification level - conditioning windows of the level above, a sparse tile
set, the paste over the enlarged level above - at the pipeline's real sizes.  Both keep known pixels (`known=`, `canvas=`
with `keep=`: a finished level regenerated in part, or grown) and start from an image (`init_canvas=`,
`refine_skip_steps=`), at the level of the canvas."""
from typing import Callable, Optional, Sequence

import torch
import torch.nn.functional as F

from . import grid as G


def _check_stages(stages, from_one):   # -> a tuple of ints: consecutive unet numbers, ascending, from 1 with `from_one`
    stages = tuple(int(s) for s in stages)
    if not stages or (stages[0] != 1 if from_one else stages[0] < 1) or any(b != a + 1 for a, b in zip(stages, stages[1:])):
        raise ValueError(f"stages must be consecutive unet numbers {'from 1 ' if from_one else ''}in ascending order, got {stages}")
    return stages


def _per_unet(v, default, n):   # {stage: value} -> one entry per unet 1 .. n (`default` where left out); anything else as it is
    return tuple(v.get(s, default) for s in range(1, n + 1)) if isinstance(v, dict) else v


def _run_stages(load_imagen, stages, device, canvas, solver, first_stage=None, devices=None, **kw):
    """`canvas` through `stages`, one `sample_tiled(**kw)` call of `load_imagen(stage)` each; `solver = (sampler, sampler_eta,
    sample_steps)`; `first_stage(geometry of the last stage, device)` returns the last stage's `into` and keywords for
    every stage's call.  `init_canvas` / `init_skip_steps` in `kw` are a scalar or {stage: value}, like the solver's.
    `devices`: every stage's canvas over these devices (`sample_tiled(devices=)`), everything else on `devices[0]`."""
    from imagen_pytorch.imagen_pytorch import normalize_devices, normalize_shards, normalize_tiling
    devices = normalize_devices(devices, kw.get("noise_fn"))
    if devices is not None:
        device = devices[0]
    device = torch.device(device if device is not None else "cuda")
    for stage in stages:
        imagen = load_imagen(stage)
        n = len(imagen.unets)
        if stage == stages[0]:   # the geometry is checked before anything moves to the device
            if stages[-1] > n:
                raise ValueError(f"stages={stages} name unet {stages[-1]}, the Imagen holds {n}")
            tiling = normalize_tiling(imagen.image_sizes, kw["grid"], kw["overlap"], kw["present"], kw["tile_weights"])
            if devices is not None and len(devices) > 1:
                normalize_shards(tiling, len(devices))
            into, more = first_stage(tiling[stages[-1] - 1], device) if first_stage else (None, {})
            kw = dict(kw, **more)
        sampler, eta, steps = (_per_unet(v, d, n) for v, d in zip(solver, (None, None, None)))
        starts = {name: _per_unet(kw[name], None, n) for name in ("init_canvas", "init_skip_steps") if name in kw}
        canvas = imagen.to(device).sample_tiled(sampler=sampler, sampler_eta=eta, sample_steps=steps, start_at_unet_number=stage,
                                                stop_at_unet_number=stage, start_image_or_video=canvas, device=device,
                                                into=into if stage == stages[-1] else None, devices=devices,
                                                **dict(kw, **starts))
    return canvas


def fused_canvas(load_imagen: Callable, num_patches_width: Optional[int] = None, grid: Optional[Sequence[int]] = None,
                 overlap: float = 0.25, stages: Sequence[int] = (1, 2, 3), tile_batch: int = 16, sampler=None, sampler_eta=None,
                 sample_steps=None, seed: Optional[int] = None, cond_images: Optional[torch.Tensor] = None, present=None,
                 tile_weights: str = "uniform", use_graph: bool = True, noise_fn: Optional[Callable] = None,
                 start_canvas: Optional[torch.Tensor] = None, device: Optional[torch.device] = None, known=None,
                 known_resample_times: int = 1, init_canvas=None, init_skip_steps=None, devices=None) -> torch.Tensor:
    """One canvas through `stages` by fused-tile sampling.  `load_imagen(stage)` returns the Imagen holding the real unet
    of that stage, as for `distributed.imagen_sample_fn` (the reference re-loads one stage at a time; all stay resident
    here).  The lattice is `grid = (ny, nx)` or `num_patches_width` squared, at `overlap`, with `present[ny][nx]` marking
    the slots that hold a tile (None: all); every stage is one `sample_tiled(start_at_unet_number=stage,
    stop_at_unet_number=stage)` call on the previous stage's canvas (`start_canvas` when `stages` does not begin at 1).
    `sampler`, `sampler_eta`, `sample_steps`: one value for every stage, or {stage: value} (a stage the dict leaves out
    keeps the default; `sampler_eta` None: 0, and 1 for the `_sde` samplers).  `cond_images` [tiles, Cc, h, w]: one per present tile, for every stage.  Returns the last stage's
    canvas [1, C, Hc, Wc] in [0, 1].  `known = (image [1, C, Hk, Wk], mask [Hk, Wk])` with `known_resample_times`: the
    pixels every stage keeps (`sample_tiled(known_image=, known_mask=)`, read at each stage's canvas size);
    `init_canvas`, `init_skip_steps`: one value for every stage or {stage: value} - the stage starts from the image at
    that step.

    A single process.  `devices` (a sequence of CUDA devices, one per shard; a device may repeat) spreads the canvas of
    every stage over them by bands of lattice rows, as `sample_tiled(devices=)` describes: the tiles of one canvas meet in
    every schedule step, so the overlap strips of the boundary tiles' estimates cross per step; the canvas comes back on
    `devices[0]`, the canvas of `devices=None`.  `torch.distributed` ranks for one canvas stay out of scope; independent
    canvases can run on different ranks as they are."""
    if (num_patches_width is None) == (grid is None):
        raise ValueError(f"fused_canvas takes num_patches_width or grid, one of them; got num_patches_width={num_patches_width!r}, "
                         f"grid={grid!r}")
    grid = (num_patches_width, num_patches_width) if grid is None else tuple(grid)
    stages = _check_stages(stages, from_one=False)
    if stages[0] > 1 and start_canvas is None:
        raise ValueError(f"stages={stages} begin at unet {stages[0]}: start_canvas, the canvas of unet {stages[0] - 1}, is needed")
    if known is not None and (not isinstance(known, (tuple, list)) or len(known) != 2):
        raise ValueError("known must be (image [1, C, Hk, Wk], mask [Hk, Wk])")
    image, mask = known if known is not None else (None, None)
    return _run_stages(load_imagen, stages, device, start_canvas, (sampler, sampler_eta, sample_steps), grid=grid, overlap=overlap,
                       present=present, tile_batch=tile_batch, tile_weights=tile_weights, cond_images=cond_images, seed=seed,
                       noise_fn=noise_fn, use_graph=use_graph, known_image=image, known_mask=mask,
                       known_resample_times=known_resample_times, init_canvas=init_canvas, init_skip_steps=init_skip_steps,
                       devices=devices)


def level_box(positions: Sequence[G.Pos]):
    """The lattice of a (sparse) position set: its bounding box.  Returns (r0, c0, grid = (rows, columns), present
    [rows][columns], tiles): `tiles` are the positions without repeats in row-major order, the order in which
    `normalize_tiling` numbers the present slots."""
    tiles = sorted({(int(i), int(j)) for i, j in positions})
    if not tiles:
        raise ValueError("level_box: no positions")
    r0, r1 = min(p[0] for p in tiles), max(p[0] for p in tiles)
    c0, c1 = min(p[1] for p in tiles), max(p[1] for p in tiles)
    present = [[False] * (c1 - c0 + 1) for _ in range(r1 - r0 + 1)]
    for i, j in tiles:
        present[i - r0][j - c0] = True
    return r0, c0, (r1 - r0 + 1, c1 - c0 + 1), present, tiles


def level_keep_mask(geom: G.GridGeometry, positions: Sequence[G.Pos], device=None) -> torch.Tensor:
    """uint8 [W, W], W = geom.canvas_width: 1 on the union of the tile squares of `positions` (tile (i, j) covers rows
    i out_patch_dist .. + S, S = W - (n - 1) out_patch_dist, columns likewise), 0 elsewhere - `fused_level(keep=...)` for
    the tiles that stay.  "Regenerate P of the finished set `done`": `positions=P, keep=level_keep_mask(geom, done - P)`;
    the strips P shares with kept neighbours stay, as in the sequential path."""
    W, st, n = int(geom.canvas_width), int(geom.out_patch_dist), int(geom.num_patches_width)
    S = W - (n - 1) * st
    keep = torch.zeros(W, W, dtype=torch.uint8, device=device)
    for i, j in positions:
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError(f"positions must lie inside the {n} x {n} grid of geom")
        keep[i * st:i * st + S, j * st:j * st + S] = 1
    return keep


def level_background(zoomed_image: torch.Tensor, width: int) -> torch.Tensor:
    """`zoomed_image` enlarged bilinearly to `width`, exactly as `grid.stitch_canvas` builds its background."""
    if zoomed_image.shape[1] * width * width >= 2 ** 31 - 1:
        return G.bilinear_resize_large(zoomed_image, width)
    return F.interpolate(zoomed_image, size=(width, width), mode="bilinear", align_corners=False)


def fused_level(load_imagen: Callable, zoomed_image: torch.Tensor, geom: G.GridGeometry, positions: Sequence[G.Pos], *,
                overlap: float = 0.25, version: str = "ultra", fill_color: Optional[float] = None, window: int = G.PATCH_SIZE,
                stages: Sequence[int] = (1, 2, 3), tile_batch: int = 16, tile_weights: str = "uniform", sampler=None,
                sampler_eta=None, sample_steps=None, seed: Optional[int] = None, noise_fn: Optional[Callable] = None,
                use_graph: bool = True, background: bool = True, device: Optional[torch.device] = None,
                canvas: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, known_resample_times: int = 1,
                refine_skip_steps=None, devices=None) -> torch.Tensor:
    """One magnification level by fused-tile sampling, with the semantics of `pipeline.generate_high_res_image`: the
    tiles at `positions` (grid positions (i, j) of `geom`; all of them at mag 1, the tissue set at mag 2) are conditioned
    on windows of `zoomed_image` [1, 3, W, W], the level above, denoised together through `stages`, and written over the
    bilinearly enlarged `zoomed_image` (`background=False`: zeros).  Returns the canvas [1, 3, canvas_width, canvas_width]
    on the device.  No positions: the enlarged background alone.

    The lattice is the bounding box of `positions` with `present` marking them (`level_box`), so a sparse tissue set pays
    for its box only: the stage canvases, the fused estimate and the noise span the box.  THE CANVAS NOISE IS KEYED BY THE
    ELEMENT OF THE BOX CANVAS - x_T, the low-res augmentation and the step noise of a pixel follow its offset from the
    box' corner, so the same tile set inside another box (a position added far away) draws other noise.

    Nothing canvas-sized is materialised beside the result: the conditioning images are described, not built
    (`TileCondCrops` with `cond_images_for_grid`'s shifts `W // 2 - (i patch_dist + patch_width // 2)`, the window at
    `center_crop_offset(W, window)`, the `v2` centre channels with `version == "v2"`), every stage runs `streamed`, and the
    last one writes its covered pixels `into` the full canvas at the box' corner.  `fill_color` None: 0 for 'airs', else
    0.95.  `geom.out_patch_dist` and `geom.canvas_width` must be the stride and the full lattice of the last stage
    (ValueError otherwise).  `load_imagen`, `stages` (from 1), `sampler`, `sampler_eta`, `sample_steps`: as `fused_canvas`.

    A finished level regenerated in part, or grown: `canvas` [1, 3, W, W] (fp32, contiguous, on the device; needs
    `background=True`, whose place it takes) is written into in place and returned; `keep` [W, W] (bool / uint8 on the
    device, non-zero = this pixel of `canvas` is known; `level_keep_mask`) with `known_resample_times`: the tiles at
    `positions` are denoised with the kept pixels mixed in at every step, so they meet their finished neighbours without a
    seam, and every kept pixel keeps its bits.  `refine_skip_steps` (int or {stage: value}): every stage starts from the
    window of `canvas` (or of the enlarged background) at that step instead of from noise.  The known image, the mask
    and the init image are the WINDOWS of `canvas` and `keep` at the box' corner, read in place at every stage's canvas
    size: no copy of a level is made.

    `devices`: the box' canvas over several devices, a band of its lattice rows each (`sample_tiled(devices=)`); the level,
    `canvas` and `keep` live on `devices[0]`, every other device takes its copy of the windows once per stage."""
    from imagen_pytorch.imagen_pytorch import TileCondCrops

    stages = _check_stages(stages, from_one=True)
    if zoomed_image.dim() != 4 or zoomed_image.shape[0] != 1 or zoomed_image.shape[2] != zoomed_image.shape[3]:
        raise ValueError(f"zoomed_image must be one square image [1, C, W, W], got {tuple(zoomed_image.shape)}")
    width = int(geom.canvas_width)
    positions = list(positions)
    if canvas is not None:
        if not background:
            raise ValueError("fused_level(canvas=...) needs background=True: the canvas takes the place of the enlarged level above")
        if (not torch.is_tensor(canvas) or canvas.dtype != torch.float32 or not canvas.is_contiguous()
                or tuple(canvas.shape) != (1, zoomed_image.shape[1], width, width)):
            raise ValueError(f"canvas must be a contiguous float32 [1, {zoomed_image.shape[1]}, {width}, {width}], got "
                             f"{tuple(canvas.shape) if torch.is_tensor(canvas) else type(canvas).__name__}")
    if keep is not None:
        if canvas is None:
            raise ValueError("fused_level(keep=...) needs canvas=: keep marks the known pixels of that canvas")
        if not torch.is_tensor(keep) or keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (width, width):
            raise ValueError(f"keep must be a bool / uint8 [{width}, {width}], got "
                             f"{(tuple(keep.shape), keep.dtype) if torch.is_tensor(keep) else type(keep).__name__}")
    elif known_resample_times != 1:
        raise ValueError(f"known_resample_times={known_resample_times} needs keep=: without known pixels nothing is resampled")
    if refine_skip_steps is not None and not background:
        raise ValueError("fused_level(refine_skip_steps=...) needs background=True: a stage starts from the canvas or the "
                         "enlarged level above")
    if not positions:   # nothing to generate (a mag-2 canvas without tissue)
        if canvas is not None:
            return canvas
        dev = zoomed_image.device if device is None else torch.device(device)
        full = level_background(zoomed_image.to(dev), width)
        return full if background else torch.zeros_like(full)
    n = int(geom.num_patches_width)
    if any(not (0 <= i < n and 0 <= j < n) for i, j in positions):
        raise ValueError(f"positions must lie inside the {n} x {n} grid of geom")
    r0, c0, grid, present, tiles = level_box(positions)
    W = int(zoomed_image.shape[3])
    half = geom.patch_width // 2
    shifts = [(W // 2 - (i * geom.patch_dist + half), W // 2 - (j * geom.patch_dist + half)) for i, j in tiles]
    if fill_color is None:
        fill_color = 0.0 if version == "airs" else 0.95  # sample_ultra_res.py:374-377
    crops = TileCondCrops(zoomed_image, shifts, int(window), float(fill_color),
                          centre_width=geom.patch_width if version == "v2" else None)

    def first_stage(last, device):
        S, st = last["S"], last["st"]
        if geom.out_patch_dist != st or width != (n - 1) * st + S:
            raise ValueError(f"geom (out_patch_dist={geom.out_patch_dist}, canvas_width={width}, {n} patches wide) is not the "
                             f"lattice of unet {stages[-1]}: stride st={st}, canvas (n - 1) st + S = {(n - 1) * st + S}")
        crops.checked(len(tiles))
        crops.image = zoomed = zoomed_image.to(device)   # moved once, for the background and every stage
        if canvas is not None:
            full = canvas
        else:
            full = level_background(zoomed.float(), width) if background else \
                torch.zeros(1, zoomed.shape[1], width, width, device=device, dtype=torch.float32)
        oy, ox = r0 * st, c0 * st
        box = (slice(oy, oy + last["Hc"]), slice(ox, ox + last["Wc"]))   # the lattice's canvas inside the level: views, no copy
        more = {}
        if keep is not None:
            more.update(known_image=full[:, :, box[0], box[1]], known_mask=keep[box], known_resample_times=known_resample_times)
        if refine_skip_steps is not None:
            more.update(init_canvas=full[:, :, box[0], box[1]], init_skip_steps=refine_skip_steps)
        return (full, oy, ox), more

    return _run_stages(load_imagen, stages, device, None, (sampler, sampler_eta, sample_steps), first_stage, grid=grid,
                       overlap=overlap, present=present, tile_batch=tile_batch, tile_weights=tile_weights, cond_crops=crops,
                       seed=seed, noise_fn=noise_fn, use_graph=use_graph, streamed=True, devices=devices)
