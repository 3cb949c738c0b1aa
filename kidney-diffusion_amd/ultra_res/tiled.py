"""Fused-tile canvas driver: the counterpart of `distributed.outpaint_canvas` in which the tiles of a canvas are denoised
together (`Imagen.sample_tiled`: MultiDiffusion / Mixture of Diffusers) instead of one after the other with inpainted overlap
strips (reference: outpainting.py:173-243, sample_ultra_res.py:183-195).  No inpainting, no resampling, no waves: every
schedule step runs all tiles in full batches and one canvas update."""
from typing import Callable, Optional, Sequence

import torch


def fused_canvas(load_imagen: Callable, num_patches_width: Optional[int] = None, grid: Optional[Sequence[int]] = None,
                 overlap: float = 0.25, stages: Sequence[int] = (1, 2, 3), tile_batch: int = 16, sampler=None, sampler_eta=0.0,
                 sample_steps=None, seed: Optional[int] = None, cond_images: Optional[torch.Tensor] = None, present=None,
                 tile_weights: str = "uniform", use_graph: bool = True, noise_fn: Optional[Callable] = None,
                 start_canvas: Optional[torch.Tensor] = None, device: Optional[torch.device] = None) -> torch.Tensor:
    """One canvas through `stages` by fused-tile sampling.  `load_imagen(stage)` returns the Imagen holding the real unet
    of that stage, as for `distributed.imagen_sample_fn` (the reference re-loads one stage at a time; all stay resident
    here).  The lattice is `grid = (ny, nx)` or `num_patches_width` squared, at `overlap`, with `present[ny][nx]` marking
    the slots that hold a tile (None: all); every stage is one `sample_tiled(start_at_unet_number=stage,
    stop_at_unet_number=stage)` call on the previous stage's canvas (`start_canvas` when `stages` does not begin at 1).
    `sampler`, `sampler_eta`, `sample_steps`: one value for every stage, or {stage: value} (a stage the dict leaves out
    keeps the default).  `cond_images` [tiles, Cc, h, w]: one per present tile, for every stage.  Returns the last stage's
    canvas [1, C, Hc, Wc] in [0, 1].

    A single process: the tiles of one canvas meet in every schedule step (the fused estimate needs all of them), so
    spreading them over ranks would take an exchange per step - out of scope here.  Independent canvases can run on
    different ranks as they are."""
    from imagen_pytorch.imagen_pytorch import normalize_tiling

    if (num_patches_width is None) == (grid is None):
        raise ValueError(f"fused_canvas takes num_patches_width or grid, one of them; got num_patches_width={num_patches_width!r}, "
                         f"grid={grid!r}")
    grid = (num_patches_width, num_patches_width) if grid is None else tuple(grid)
    stages = tuple(int(s) for s in stages)
    if not stages or stages[0] < 1 or any(b != a + 1 for a, b in zip(stages, stages[1:])):
        raise ValueError(f"stages must be consecutive unet numbers in ascending order, got {stages}")
    if stages[0] > 1 and start_canvas is None:
        raise ValueError(f"stages={stages} begin at unet {stages[0]}: start_canvas, the canvas of unet {stages[0] - 1}, is needed")
    device = torch.device(device if device is not None else "cuda")
    cache = {}
    canvas = start_canvas
    for stage in stages:
        imagen = cache[stage] = load_imagen(stage)
        n = len(imagen.unets)
        if stage == stages[0]:   # the geometry is checked before anything moves to the device
            if stages[-1] > n:
                raise ValueError(f"stages={stages} name unet {stages[-1]}, the Imagen holds {n}")
            normalize_tiling(imagen.image_sizes, grid, overlap, present, tile_weights)
        per_unet = lambda v, d: tuple(v.get(s, d) for s in range(1, n + 1)) if isinstance(v, dict) else v
        imagen = cache[stage] = imagen.to(device)
        canvas = imagen.sample_tiled(grid, overlap=overlap, present=present, tile_batch=tile_batch, tile_weights=tile_weights,
                                     cond_images=cond_images, sampler=per_unet(sampler, None),
                                     sampler_eta=per_unet(sampler_eta, 0.0), sample_steps=per_unet(sample_steps, None),
                                     seed=seed, noise_fn=noise_fn, use_graph=use_graph, start_at_unet_number=stage,
                                     stop_at_unet_number=stage, start_image_or_video=canvas, device=device)
    return canvas
