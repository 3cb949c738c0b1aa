"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of fused-tile canvas sampling
that keeps known pixels or starts from an image - ``Imagen.sample_tiled(known_image=, known_mask=, known_resample_times=,
init_canvas=, init_skip_steps=)`` - written from its description over tests/tiled_ref.py (lattice, cut, fuse, CanvasSolver)
and the oracle's ``q_sample`` / ``q_sample_from_to``.  Nothing here comes from imagen-pytorch: the library has no canvas.

RePaint mixing (Lugmayr et al. 2022) and the image start at the level of the canvas, mirroring what ``p_sample_loop`` of
oracle/sampler_ref.py and tests/init_images_ref.py do per image.  With the known image ``kn`` in [0, 1], the mask ``m`` and R
resamples, a stage over the steps ``k = skip .. T - 1`` is

    x = z_init [+ nearest(2 init - 1)]
    for k, for r = R - 1 .. 0:
        x = m ? q_sample(2 kn - 1, t_k, z("inpaint", stage, k, r)) : x
        the tiles denoised, x0bar fused, x <- the solver's step with x0bar        (tests/tiled_ref.py)
        if r > 0 and k < T - 1:  x = q_sample_from_to(x, t_{k+1}, t_k, z("renoise", stage, k, r))
    out = m ? kn : unnormalize(clamp(x))

on covered pixels; a pixel no tile covers is never touched and comes back as 0.  Every stage sees ``kn``, ``m`` and ``init``
resized (nearest) to its own canvas.  DPM-Solver++(2M): the history takes the fused estimate of a step's LAST resample only,
all R resamples of step k read step k - 1's; the first step walked is first order.  A self-conditioned UNet reads the tile's
crop of the fused estimate of the previous ITERATION (None at the first one walked).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import self_cond_ref as SC
import tiled_ref as TR
from oracle import sampler_ref as RS
from oracle.imagen_ref import exists, resize_image_to

lattice, cut, fuse, CanvasSolver = TR.lattice, TR.cut, TR.fuse, TR.CanvasSolver


def nearest(img, size):
    """[.., H, W] -> [.., *size] by torch's nearest rule; a source of that size is taken as it is."""
    return img if tuple(img.shape[-2:]) == tuple(size) else F.interpolate(img, tuple(size), mode="nearest")


def covered_of(lat):
    c = torch.zeros(lat["Hc"], lat["Wc"], dtype=torch.bool)
    for y0, x0 in lat["origins"]:
        c[y0:y0 + lat["S"], x0:x0 + lat["S"]] = True
    return c


def run_canvas(denoise_tiles, x, lat, noise_scheduler, name, eta, noise_fn, stage, weights="uniform", known=None, mask=None,
               R=1, skip=0):
    """x at step `skip` [1, C, Hc, Wc] -> the canvas after the last step (before clamp / unnormalise), and the covered mask.
    `known` [1, C, Hc, Wc] in [0, 1] and `mask` [Hc, Wc] bool at the canvas' size, or None; `denoise_tiles` as
    tiled_ref.run_canvas takes it."""
    solver = CanvasSolver(noise_scheduler, name, eta)
    w = TR.weight(lat["S"], lat["st"], weights)
    N = len(lat["origins"])
    covered = covered_of(lat)
    shape = tuple(x.shape)
    has_known = exists(known) and exists(mask)
    R = R if has_known else 1
    if has_known:
        kn, m = known * 2 - 1, mask & covered
    T = len(solver.steps)
    latest = None
    for k, (times, times_next) in enumerate(solver.steps):
        if k < skip:
            continue
        for r in reversed(range(R)):
            if has_known:
                x = torch.where(m, noise_scheduler.q_sample(kn, times, noise_fn(("inpaint", stage, k, r), shape)), x)
            prev = cut(latest, lat) if exists(latest) else None
            x0c = denoise_tiles(k, times.expand(N), times_next.expand(N), cut(x, lat), prev)
            x0bar, cov = fuse(x0c, lat, w)
            assert torch.equal(cov, covered)
            noise = noise_fn(("step", stage, k, r), shape) if solver.wants_noise(k) else None
            kept = (solver.x0_prev, solver.h_prev)
            stepped = solver.step(k, x, x0bar, noise)
            if r > 0:   # the history follows the schedule, not the resample loop
                solver.x0_prev, solver.h_prev = kept
            x = torch.where(covered, stepped, x)
            latest = x0bar
            if r > 0 and k < T - 1:
                again = noise_scheduler.q_sample_from_to(x, times_next, times, noise_fn(("renoise", stage, k, r), shape))
                x = torch.where(covered, again, x)
    return x, covered


@torch.no_grad()
def sample_tiled(oim, *, grid, noise_fn, overlap=0.25, present=None, tile_weights="uniform", cond_images=None, text_embeds=None,
                 text_masks=None, cond_scale=1.0, sampler=None, sampler_eta=0.0, sample_steps=None, start_at_unet_number=1,
                 stop_at_unet_number=None, start_image_or_video=None, return_all_unet_outputs=False,
                 lowres_sample_noise_level=None, known_image=None, known_mask=None, known_resample_times=1, init_canvas=None,
                 init_skip_steps=None):
    """Imagen.sample_tiled with the canvas-level arguments over an oracle Imagen `oim`."""
    oim.eval()
    n = len(oim.unets)
    per = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * n
    names, etas, steps, scales = per(sampler), per(sampler_eta), per(sample_steps), per(cond_scale)
    inits, skips = per(init_canvas), per(init_skip_steps)
    level = oim.lowres_sample_noise_level if lowres_sample_noise_level is None else lowres_sample_noise_level
    lats = [lattice(S, grid, overlap, present) for S in oim.image_sizes]
    N = len(lats[0]["origins"])
    if exists(text_embeds):
        text_masks = torch.any(text_embeds != 0.0, dim=-1) if text_masks is None else text_masks
        text_embeds, text_masks = text_embeds.expand(N, -1, -1), text_masks.expand(N, -1)
    if exists(known_image):
        known_image = known_image.float() / 255.0 if known_image.dtype == torch.uint8 else known_image.float()
        known_mask = (known_mask.reshape(known_mask.shape[-2:]) != 0)
    canvas, outputs = None, []
    if start_at_unet_number > 1:
        g = lats[start_at_unet_number - 2]
        canvas = F.interpolate(start_image_or_video, (g["Hc"], g["Wc"]), mode="nearest")
    for num, unet, lat, sched, obj, dyn in zip(range(1, n + 1), oim.unets, lats, oim.noise_schedulers, oim.pred_objectives,
                                               oim.dynamic_thresholding):
        if num < start_at_unet_number:
            continue
        if exists(steps[num - 1]):
            kind = "cosine" if sched.log_snr is RS.alpha_cosine_log_snr else "linear"
            sched = RS.GaussianDiffusionContinuousTimes(noise_schedule=kind, timesteps=int(steps[num - 1]))
        size = (lat["Hc"], lat["Wc"])
        shape = (1, oim.channels) + size
        lowres_tiles = lowres_times = None
        if unet.lowres_cond:
            low = oim.normalize_img(F.interpolate(canvas, size, mode="nearest"))
            low = oim.lowres_noise_schedule.q_sample(low, oim.lowres_noise_schedule.get_times(1, level),
                                                     noise_fn(("lowres", num), shape))
            lowres_tiles, lowres_times = cut(low, lat), oim.lowres_noise_schedule.get_times(N, level)
        cond = resize_image_to(cond_images, lat["S"]) if exists(cond_images) else None

        def denoise(k, times, times_next, tiles, prev, unet=unet, sched=sched, obj=obj, dyn=dyn, cond=cond,
                    lowres_tiles=lowres_tiles, lowres_times=lowres_times, cs=scales[num - 1]):
            net = SC._SelfCondCall(unet, prev) if getattr(unet, "self_cond", False) else unet
            _, x0c = oim.p_mean_variance(net, tiles, times, noise_scheduler=sched, t_next=times_next, text_embeds=text_embeds,
                                         text_mask=text_masks, cond_images=cond, lowres_cond_img=lowres_tiles,
                                         lowres_noise_times=lowres_times, cond_scale=cs, pred_objective=obj,
                                         dynamic_threshold=dyn)
            return x0c

        x = noise_fn(("init", num), shape)
        init = inits[num - 1]
        if exists(init):
            init = init.float() / 255.0 if init.dtype == torch.uint8 else init.float()
            x = x + nearest(oim.normalize_img(init), size)
        kn = nearest(known_image, size) if exists(known_image) else None
        m = (nearest(known_mask[None, None].float(), size)[0, 0] != 0) if exists(known_image) else None
        x, covered = run_canvas(denoise, x, lat, sched, names[num - 1] or "ddpm", etas[num - 1] or 0.0, noise_fn, num,
                                tile_weights, kn, m, known_resample_times, int(skips[num - 1] or 0))
        canvas = oim.unnormalize_img(x.clamp(-1.0, 1.0))
        if exists(kn):
            canvas = torch.where(m, kn, canvas)
        canvas = torch.where(covered, canvas, torch.zeros_like(x))
        outputs.append(canvas)
        if exists(stop_at_unet_number) and stop_at_unet_number == num:
            break
    return outputs if return_all_unet_outputs else outputs[-1]


def assert_mask_condition(mask, lats):
    """What every test's mask must satisfy, at every stage's canvas size (`lats`: the stages' lattices; `mask` [Hk, Wk] is
    resized to each as the sampler does): between 25 % and 75 % of the canvas known, every present tile holding both known
    and unknown pixels, and - where tiles overlap - at least one overlap strip holding both."""
    for lat in lats:
        S = lat["S"]
        m = nearest(mask[None, None].float(), (lat["Hc"], lat["Wc"]))[0, 0] != 0
        share = float(m.float().mean())
        assert 0.25 <= share <= 0.75, f"{share:.0%} of the {lat['Hc']} x {lat['Wc']} canvas is known"
        boxes = [(y0, y0 + S, x0, x0 + S) for y0, x0 in lat["origins"]]
        mixed = lambda t: bool(t.any()) and not bool(t.all())
        assert all(mixed(m[a:b, c:d]) for a, b, c, d in boxes), "a tile is all known or all unknown"
        strips = [(max(p[0], q[0]), min(p[1], q[1]), max(p[2], q[2]), min(p[3], q[3])) for i, p in enumerate(boxes) for q in boxes[i + 1:]]
        strips = [s for s in strips if s[0] < s[1] and s[2] < s[3]]
        assert not strips or any(mixed(m[a:b, c:d]) for a, b, c, d in strips), "no overlap strip holds known and unknown pixels"
