"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of fused-tile canvas sampling
- ``Imagen.sample_tiled`` - written from its description (MultiDiffusion, Bar-Tal et al. 2023; Mixture of Diffusers,
Jimenez 2023) over the oracle UNets and the formulas of tests/solver_ref.py.  Nothing here comes from imagen-pytorch: the
library has no such sampler.

The canvas of a stage is ONE noisy image ``x`` [1, C, Hc, Wc] over a lattice of ``ny x nx`` tile slots of size ``S`` at
stride ``st = int(S (1 - overlap))``, ``Hc = (ny - 1) st + S``.  Per schedule step k:

1. every present tile (row-major) is cut out of ``x`` and denoised by itself: ``p_mean_variance`` of the oracle gives its
   thresholded estimate ``x0c_t`` (its own dynamic threshold); a self-conditioned UNet reads the tile's crop of the
   previous step's FUSED estimate (None at step 0);
2. ``x0bar = (sum_t w_t x0c_t) / (sum_t w_t)`` over the tiles that cover a pixel, summed in tile order in fp32;
   ``w = 1`` ("uniform") or ``r(y) r(x)``, ``r(i) = min(i + 1, S - i, ov) / ov``, ``ov = max(S - st, 1)`` ("ramp");
3. ONE update of the canvas with ``x0bar`` in the place of the estimate, in the published forms tests/solver_ref.py uses:
   the ancestral step (``q_posterior`` mean plus ``exp(log_var / 2) z``, no noise into t = 0), DDIM(eta) in its eps form, or
   DPM-Solver++(2M) with the fused estimate of step k - 1 as its history.  ``z`` has the canvas' shape: tag
   ("step", stage, k, 0), asked for only when the step adds noise.

A pixel that no tile covers is never updated and comes back as 0.  The low-res conditioning of a stage is the previous
canvas resized (nearest) to this canvas, augmented once with noise of the canvas' shape (tag ("lowres", stage)), then cut
per tile.  ``cond_images`` holds one image per tile; ``text_embeds`` holds one row, given to every tile.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import self_cond_ref as SC
from oracle import sampler_ref as RS
from oracle.imagen_ref import exists, resize_image_to

_pad = RS._pad


def lattice(S, grid, overlap=0.25, present=None):
    """dict(S, st, ny, nx, Hc, Wc, origins): the tile origins (y0, x0) in row-major order over the present slots."""
    ny, nx = grid
    st = int(S * (1 - overlap))
    assert S % 4 == 0 and st % 4 == 0 and 1 <= st <= S
    present = [[True] * nx for _ in range(ny)] if present is None else present
    origins = [(r * st, q * st) for r in range(ny) for q in range(nx) if present[r][q]]
    assert origins
    return dict(S=S, st=st, ny=ny, nx=nx, Hc=(ny - 1) * st + S, Wc=(nx - 1) * st + S, origins=origins)


def weight(S, st, kind):
    if kind == "uniform":
        return torch.ones(S, S)
    assert kind == "ramp"
    ov = max(S - st, 1)
    r = torch.tensor([min(i + 1, S - i, ov) for i in range(S)], dtype=torch.float32) / ov
    return r[:, None] * r[None, :]


def cut(canvas, lat):
    """[1, C, Hc, Wc] -> [N, C, S, S]"""
    S = lat["S"]
    return torch.cat([canvas[:, :, y0:y0 + S, x0:x0 + S] for y0, x0 in lat["origins"]])


def fuse(tiles, lat, w):
    """(x0bar [1, C, Hc, Wc], covered [Hc, Wc]): the weighted mean of the tiles over every covered pixel, 0 elsewhere."""
    S = lat["S"]
    num = torch.zeros(1, tiles.shape[1], lat["Hc"], lat["Wc"], dtype=tiles.dtype)
    den = torch.zeros(lat["Hc"], lat["Wc"], dtype=tiles.dtype)
    w = w.to(tiles.dtype)
    for t, (y0, x0) in enumerate(lat["origins"]):
        num[0, :, y0:y0 + S, x0:x0 + S] += w * tiles[t]
        den[y0:y0 + S, x0:x0 + S] += w
    covered = den > 0
    return torch.where(covered, num / torch.where(covered, den, torch.ones_like(den)), torch.zeros_like(num)), covered


class CanvasSolver:
    """The update of one canvas over a schedule; holds the 2M history.  step(k, x, x0bar, noise) -> x."""

    def __init__(self, noise_scheduler, name, eta=0.0):
        assert name in ("ddpm", "ddim", "dpmpp_2m")
        self.sched, self.name, self.eta = noise_scheduler, name, float(eta)
        self.steps = noise_scheduler.get_sampling_timesteps(1)
        self.x0_prev = self.h_prev = None

    def wants_noise(self, k):
        last = k == len(self.steps) - 1
        return (self.name == "ddpm" or (self.name == "ddim" and self.eta > 0)) and not last

    def step(self, k, x, x0bar, noise=None):
        times, times_next = self.steps[k]
        last = k == len(self.steps) - 1
        ls, ls_next = _pad(x, self.sched.log_snr(times)), _pad(x, self.sched.log_snr(times_next))
        a, s = RS.log_snr_to_alpha_sigma(ls)
        a_next, s_next = RS.log_snr_to_alpha_sigma(ls_next)
        h = ls_next / 2 - ls / 2
        if self.name == "ddpm":
            mean, _, log_var = self.sched.q_posterior(x_start=x0bar, x_t=x, t=times, t_next=times_next)
            out = mean if last else mean + (0.5 * log_var).exp() * noise
        elif self.name == "ddim":
            d = self.eta * torch.sqrt((s_next ** 2) * (-torch.expm1(ls - ls_next)))
            eps = (x - a * x0bar) / s
            out = a_next * x0bar + torch.sqrt((s_next ** 2 - d ** 2).clamp(min=0.0)) * eps
            if self.eta > 0 and not last:
                out = out + d * noise
        else:
            D = x0bar
            if exists(self.x0_prev) and not last:
                rr = self.h_prev / h
                D = (1 + 1 / (2 * rr)) * x0bar - (1 / (2 * rr)) * self.x0_prev
            out = (s_next / s) * x - a_next * torch.expm1(-h) * D
        self.x0_prev, self.h_prev = x0bar, h
        return out


def run_canvas(denoise_tiles, x, lat, noise_scheduler, name, eta, noise_fn, stage, weights="uniform"):
    """x_T [1, C, Hc, Wc] -> the canvas after the last step (before clamp / unnormalise), and the covered mask.
    denoise_tiles(k, times [N], times_next [N], tiles [N, C, S, S], prev [N, C, S, S] or None) -> thresholded x0 [N, C, S, S]."""
    solver = CanvasSolver(noise_scheduler, name, eta)
    w = weight(lat["S"], lat["st"], weights)
    N = len(lat["origins"])
    x0bar = covered = None
    for k, (times, times_next) in enumerate(solver.steps):
        prev = cut(x0bar, lat) if exists(x0bar) else None
        x0c = denoise_tiles(k, times.expand(N), times_next.expand(N), cut(x, lat), prev)
        x0bar, covered = fuse(x0c, lat, w)
        noise = noise_fn(("step", stage, k, 0), tuple(x.shape)) if solver.wants_noise(k) else None
        x = torch.where(covered, solver.step(k, x, x0bar, noise), x)
    return x, covered


@torch.no_grad()
def sample_tiled(oim, *, grid, noise_fn, overlap=0.25, present=None, tile_weights="uniform", cond_images=None, text_embeds=None,
                 text_masks=None, cond_scale=1.0, sampler=None, sampler_eta=0.0, sample_steps=None, start_at_unet_number=1,
                 stop_at_unet_number=None, start_image_or_video=None, return_all_unet_outputs=False,
                 lowres_sample_noise_level=None):
    """Imagen.sample_tiled over an oracle Imagen `oim` (oracle/sampler_ref.py or a subclass)."""
    oim.eval()
    n = len(oim.unets)
    per = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * n
    names, etas, steps, scales = per(sampler), per(sampler_eta), per(sample_steps), per(cond_scale)
    level = oim.lowres_sample_noise_level if lowres_sample_noise_level is None else lowres_sample_noise_level
    lats = [lattice(S, grid, overlap, present) for S in oim.image_sizes]
    N = len(lats[0]["origins"])
    if exists(text_embeds):
        text_masks = torch.any(text_embeds != 0.0, dim=-1) if text_masks is None else text_masks
        text_embeds, text_masks = text_embeds.expand(N, -1, -1), text_masks.expand(N, -1)
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
        shape = (1, oim.channels, lat["Hc"], lat["Wc"])
        lowres_tiles = lowres_times = None
        if unet.lowres_cond:
            low = oim.normalize_img(F.interpolate(canvas, shape[-2:], mode="nearest"))
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

        x, covered = run_canvas(denoise, noise_fn(("init", num), shape), lat, sched, names[num - 1] or "ddpm",
                                etas[num - 1] or 0.0, noise_fn, num, tile_weights)
        canvas = torch.where(covered, oim.unnormalize_img(x.clamp(-1.0, 1.0)), torch.zeros_like(x))
        outputs.append(canvas)
        if exists(stop_at_unet_number) and stop_at_unet_number == num:
            break
    return outputs if return_all_unet_outputs else outputs[-1]
