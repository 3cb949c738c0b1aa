"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of few-step sampling of
DDPM-trained UNets - ``sample(sampler=..., sampler_eta=..., sample_steps=...)`` - written from the published formulas.
Nothing here comes from imagen-pytorch: the library has neither sampler.  Built on the existing restatements by
subclassing them; ``p_sample_loop`` is ``init_images_ref.Imagen``'s loop with the ancestral update replaced.

With a, s = alpha, sigma at t_k, a', s' at t_{k+1}, x0c the thresholded estimate ``p_mean_variance`` returns:

* DDIM(eta) (Song et al. 2021, eq. 12), in its eps form:  ``eps = (x - a x0c) / s``,
  ``x = a' x0c + sqrt(s'^2 - d^2) eps + d z`` with ``d = eta sqrt(s'^2 c)``, the ancestral posterior deviation
  (``c = -expm1(log_snr - log_snr')``); no noise on the last step.  Tag ("step", stage, k, r), asked for only when eta > 0.
* DPM-Solver++(2M) (Lu et al. 2022, algorithm 2), data prediction:  ``lambda = log_snr / 2``, ``h = lambda' - lambda``,
  ``r = h_prev / h``, ``D = (1 + 1/(2r)) x0c - (1/(2r)) x0c_prev``, ``x = (s'/s) x - a' expm1(-h) D``;
  first order (``D = x0c``) on the first step walked and on the last step.

Under inpainting with resampling every resample of step k reads the estimate that the LAST resample of step k - 1 left
(the multistep history follows the schedule, not the resample loop); inpaint mix and re-noise are the parent's.
``sample_steps=N`` walks the N-step schedule of the stage's kind, for any sampler ("ddpm" = the parent's loop on it).
The self-conditioning restatement combines by inheritance: ``class X(self_cond_ref.Imagen, solver_ref.Imagen)``.
"""
from __future__ import annotations

import torch

import init_images_ref as IR
from oracle import sampler_ref as RS
from oracle.imagen_ref import exists, resize_image_to

_pad = RS._pad
cast_per_unet = IR.cast_per_unet


def never_step_noise(noise_fn):
    """`noise_fn` that refuses any ("step", ...) tag: what a deterministic sampler must get through."""

    def fn(tag, shape):
        assert tag[0] != "step", f"a deterministic sampler asked for {tag}"
        return noise_fn(tag, shape)

    return fn


class Imagen(IR.Imagen):
    _solvers = None

    @torch.no_grad()
    def sample(self, *, sampler=None, sampler_eta=0.0, sample_steps=None, **kw):
        n = len(self.unets)
        names, etas, steps = (cast_per_unet(v, n) for v in (sampler, sampler_eta, sample_steps))
        assert len(names) == n and len(etas) == n and len(steps) == n
        self._solvers = [(nm or "ddpm", float(e or 0.0)) for nm, e in zip(names, etas)]
        kept = self.noise_schedulers
        self.noise_schedulers = [
            sch if st is None else RS.GaussianDiffusionContinuousTimes(
                noise_schedule="cosine" if sch.log_snr is RS.alpha_cosine_log_snr else "linear", timesteps=int(st))
            for sch, st in zip(kept, steps)]
        try:
            return super().sample(**kw)
        finally:
            self._solvers, self.noise_schedulers = None, kept

    def p_sample_loop(self, unet, shape, *, stage, noise_fn, noise_scheduler, lowres_cond_img, lowres_noise_times,
                      text_embeds, text_mask, cond_images, inpaint_images, inpaint_masks, inpaint_resample_times,
                      cond_scale, pred_objective, dynamic_threshold, trace=None):
        name, eta = self._solvers[stage - 1] if exists(self._solvers) else ("ddpm", 0.0)
        if name == "ddpm":
            return super().p_sample_loop(
                unet, shape, stage=stage, noise_fn=noise_fn, noise_scheduler=noise_scheduler,
                lowres_cond_img=lowres_cond_img, lowres_noise_times=lowres_noise_times, text_embeds=text_embeds,
                text_mask=text_mask, cond_images=cond_images, inpaint_images=inpaint_images, inpaint_masks=inpaint_masks,
                inpaint_resample_times=inpaint_resample_times, cond_scale=cond_scale, pred_objective=pred_objective,
                dynamic_threshold=dynamic_threshold, trace=trace)
        assert name in ("ddim", "dpmpp_2m")
        batch = shape[0]
        init, skip = self.start_of(stage, shape[-1])
        img = noise_fn(("init", stage), shape)
        if exists(init):
            img = img + init
        has_inpainting = exists(inpaint_images) and exists(inpaint_masks)
        resample_times = inpaint_resample_times if has_inpainting else 1
        if has_inpainting:
            inpaint_images = self.normalize_img(inpaint_images)
            inpaint_images = resize_image_to(inpaint_images, shape[-1])
            inpaint_masks = resize_image_to(inpaint_masks[:, None].float(), shape[-1]).bool()
        kw = dict(noise_scheduler=noise_scheduler, text_embeds=text_embeds, text_mask=text_mask,
                  cond_images=cond_images, lowres_cond_img=lowres_cond_img,
                  lowres_noise_times=lowres_noise_times, cond_scale=cond_scale,
                  pred_objective=pred_objective, dynamic_threshold=dynamic_threshold)
        steps = noise_scheduler.get_sampling_timesteps(batch)
        x0_prev = h_prev = None                                                          # of step k - 1 (2M)
        for k, (times, times_next) in enumerate(steps):
            if k < skip:
                continue
            is_last_timestep = times_next == 0
            last = k == len(steps) - 1
            ls, ls_next = _pad(img, noise_scheduler.log_snr(times)), _pad(img, noise_scheduler.log_snr(times_next))
            a, s = RS.log_snr_to_alpha_sigma(ls)
            a_next, s_next = RS.log_snr_to_alpha_sigma(ls_next)
            h = ls_next / 2 - ls / 2
            for r in reversed(range(resample_times)):
                if has_inpainting:
                    noised = noise_scheduler.q_sample(inpaint_images, times, noise_fn(("inpaint", stage, k, r), shape))
                    img = img * ~inpaint_masks + noised * inpaint_masks
                # the thresholded estimate of this iteration (the ancestral image that comes with it is not used)
                _, x0c = self.p_sample(unet, img, times, torch.zeros(shape), t_next=times_next, **kw)
                if name == "ddim":
                    d = eta * torch.sqrt((s_next ** 2) * (-torch.expm1(ls - ls_next)))
                    eps = (img - a * x0c) / s
                    img = a_next * x0c + torch.sqrt((s_next ** 2 - d ** 2).clamp(min=0.0)) * eps
                    if eta > 0 and not last:
                        img = img + d * noise_fn(("step", stage, k, r), shape)
                    elif eta > 0:
                        noise_fn(("step", stage, k, r), shape)                           # drawn and unused, as the ancestral step's
                else:
                    D = x0c
                    if exists(x0_prev) and not last:
                        rr = h_prev / h
                        D = (1 + 1 / (2 * rr)) * x0c - (1 / (2 * rr)) * x0_prev
                    img = (s_next / s) * img - a_next * torch.expm1(-h) * D
                if r == 0:
                    x0_new = x0c
                if has_inpainting and not (r == 0 or bool(torch.all(is_last_timestep))):
                    renoised = noise_scheduler.q_sample_from_to(
                        img, times_next, times, noise_fn(("renoise", stage, k, r), shape))
                    img = torch.where(_pad(img, is_last_timestep), img, renoised)
            x0_prev, h_prev = x0_new, h
            if exists(trace):
                trace.append(img.clone())
        img = img.clamp(-1.0, 1.0)
        if has_inpainting:
            img = img * ~inpaint_masks + inpaint_images * inpaint_masks
        return self.unnormalize_img(img)
