"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of ``sample(init_images=...,
skip_steps=...)`` of imagen-pytorch 1.18.x from the library's published algorithm, built on the existing restatements by
subclassing them.  Each ``p_sample_loop`` below is its parent's loop with two changes, the start and the step range:

* ``Imagen`` (DDPM):        ``img = z + resize_nearest(2 init - 1, S)`` - the image is added unscaled - and the loop walks
                            the schedule steps ``skip .. T - 1``.
* ``ElucidatedImagen``:     ``x = sigma_0 z + resize_nearest(2 init - 1, S)`` with sigma_0 the first sigma of the full
                            schedule whatever ``skip`` is; steps ``skip .. N - 1``.

A step keeps its index k: its schedule times, its ``noise_fn`` tags ("step" | "inpaint" | "renoise" | "churn", stage, k, r)
and its slot in ``trace`` (one state per step walked) are those of step k of a full run.  ``init_images`` (None, one tensor
for every UNet sampled, or one entry per UNet) and ``skip_steps`` (None, an int, or one entry per UNet) are cast per UNet by
``sample``.  The self-conditioning restatements of tests/self_cond_ref.py reset their carry per ``p_sample_loop`` call and
combine with these classes by inheritance (``class X(self_cond_ref.Imagen, init_images_ref.Imagen)``).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import elucidated_ref as ER
from oracle import sampler_ref as RS
from oracle.imagen_ref import exists, resize_image_to

_pad = RS._pad


def nearest_index(dst, n_in, n_out):
    """Source index of F.interpolate(mode="nearest") for destination index `dst`: the ratio and the product in fp32."""
    import numpy as np

    return min(int(np.floor(np.float32(dst) * (np.float32(n_in) / np.float32(n_out)))), n_in - 1)


def resize_nearest(img, size):
    """To [.., size, size]; a source of that size is taken as it is, any other (square or not) goes through F.interpolate."""
    if tuple(img.shape[-2:]) == (size, size):
        return img
    return F.interpolate(img, (size, size), mode="nearest")


def cast_per_unet(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


class _Starts:
    """sample() with the two arguments: cast per UNet and handed to the stage loops through the instance."""

    _starts = None

    @torch.no_grad()
    def sample(self, *, init_images=None, skip_steps=None, **kw):
        n = len(self.unets)
        inits, skips = cast_per_unet(init_images, n), cast_per_unet(skip_steps, n)
        assert len(inits) == n and len(skips) == n
        self._starts = [(i, 0 if s is None else int(s)) for i, s in zip(inits, skips)]
        try:
            return super().sample(**kw)
        finally:
            self._starts = None

    def start_of(self, stage, size):
        """(2 init - 1 at the stage's size or None, skip) of a stage; (None, 0) outside sample()."""
        init, skip = self._starts[stage - 1] if exists(self._starts) else (None, 0)
        if exists(init):
            init = init.float() / 255.0 if init.dtype == torch.uint8 else init
            init = resize_nearest(self.normalize_img(init), size)
        return init, skip


class Imagen(_Starts, RS.Imagen):
    def p_sample_loop(self, unet, shape, *, stage, noise_fn, noise_scheduler, lowres_cond_img, lowres_noise_times,
                      text_embeds, text_mask, cond_images, inpaint_images, inpaint_masks, inpaint_resample_times,
                      cond_scale, pred_objective, dynamic_threshold, trace=None):
        batch = shape[0]
        init, skip = self.start_of(stage, shape[-1])
        img = noise_fn(("init", stage), shape)
        if exists(init):
            img = img + init                                                             # the start
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
        for k, (times, times_next) in enumerate(noise_scheduler.get_sampling_timesteps(batch)):
            if k < skip:                                                                 # the step range
                continue
            is_last_timestep = times_next == 0
            for r in reversed(range(resample_times)):
                if has_inpainting:
                    noised = noise_scheduler.q_sample(inpaint_images, times, noise_fn(("inpaint", stage, k, r), shape))
                    img = img * ~inpaint_masks + noised * inpaint_masks
                img, x_start = self.p_sample(unet, img, times, noise_fn(("step", stage, k, r), shape),
                                             t_next=times_next, **kw)
                if has_inpainting and not (r == 0 or bool(torch.all(is_last_timestep))):
                    renoised = noise_scheduler.q_sample_from_to(
                        img, times_next, times, noise_fn(("renoise", stage, k, r), shape))
                    img = torch.where(_pad(img, is_last_timestep), img, renoised)
            if exists(trace):
                trace.append(img.clone())
        img = img.clamp(-1.0, 1.0)
        if has_inpainting:
            img = img * ~inpaint_masks + inpaint_images * inpaint_masks
        return self.unnormalize_img(img)


class ElucidatedImagen(_Starts, ER.ElucidatedImagen):
    def p_sample_loop(self, unet, shape, *, stage, noise_fn, noise_scheduler, lowres_cond_img, lowres_noise_times,
                      text_embeds, text_mask, cond_images, inpaint_images, inpaint_masks, inpaint_resample_times,
                      cond_scale, pred_objective, dynamic_threshold, trace=None):
        hp = self.hparams[stage - 1]
        N = hp["num_sample_steps"]
        sigmas, gammas = self.sample_schedule(hp)
        pairs = list(zip(sigmas[:-1], sigmas[1:], gammas[:-1]))
        init, skip = self.start_of(stage, shape[-1])
        x = sigmas[0] * noise_fn(("init", stage), shape)
        if exists(init):
            x = x + init                                                                 # the start
        has_inpainting = exists(inpaint_images) and exists(inpaint_masks)
        R = inpaint_resample_times if has_inpainting else 1
        if has_inpainting:
            inpaint_images = resize_image_to(self.normalize_img(inpaint_images), shape[-1])
            inpaint_masks = resize_image_to(inpaint_masks[:, None].float(), shape[-1]).bool()
        net_kw = dict(text_embeds=text_embeds, text_mask=text_mask, cond_images=cond_images, cond_scale=cond_scale,
                      lowres_cond_img=lowres_cond_img,
                      lowres_noise_times=(self.lowres_noise_schedule.log_snr(lowres_noise_times)
                                          if exists(lowres_noise_times) else None))
        for k, (sigma, sigma_next, gamma) in enumerate(pairs):
            if k < skip:                                                                 # the step range
                continue
            sigma, sigma_next, gamma = (t.item() for t in (sigma, sigma_next, gamma))
            for r in reversed(range(R)):
                eps = hp["S_noise"] * noise_fn(("churn", stage, k, r), shape)
                sigma_hat = sigma + gamma * sigma
                added = math.sqrt(sigma_hat ** 2 - sigma ** 2) * eps
                x_hat = x + added
                if has_inpainting:
                    x_hat = x_hat * ~inpaint_masks + (inpaint_images + added) * inpaint_masks
                den = self.preconditioned(unet, x_hat, sigma_hat, hp, net_kw, dynamic_threshold)
                d = (x_hat - den) / sigma_hat
                x_next = x_hat + (sigma_next - sigma_hat) * d
                if sigma_next != 0:
                    den2 = self.preconditioned(unet, x_next, sigma_next, hp, net_kw, dynamic_threshold)
                    d2 = (x_next - den2) / sigma_next
                    x_next = x_hat + 0.5 * (sigma_next - sigma_hat) * (d + d2)
                x = x_next
                if has_inpainting and not (r == 0 or k == N - 1):
                    x = x + (sigma - sigma_next) * noise_fn(("renoise", stage, k, r), shape)
            if exists(trace):
                trace.append(x.clone())
        x = x.clamp(-1.0, 1.0)
        if has_inpainting:
            x = x * ~inpaint_masks + inpaint_images * inpaint_masks
        return self.unnormalize_img(x)
