"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED**: imagen-pytorch 1.18.x is not installed and the reference pins it
without shipping it, so this is a restatement of its ``ElucidatedImagen`` sampler (``elucidated_imagen.py``:
``sample_schedule``, ``c_skip`` / ``c_out`` / ``c_in`` / ``c_noise``, ``preconditioned_network_forward``,
``one_unet_sample``) from the library's published algorithm, not a copy checked against it.

It drives ``oracle.imagen_ref.Unet`` through the stage loop of ``oracle.sampler_ref.Imagen`` (low-res augmentation,
start / stop unet, cond images, text, guidance: as for ``Imagen``) with the EDM loop per stage.  Every Gaussian
draw goes through ``noise_fn(tag, shape)``:

    ("lowres", stage)            low-res conditioning augmentation (as Imagen)
    ("init", stage)              x = sigma_0 * N(0,1)
    ("churn", stage, k, r)       eps = S_noise * N(0,1), drawn every iteration (also when gamma = 0)
    ("renoise", stage, k, r)     RePaint re-noise (inpainting, not after r == 0 nor on the last step)
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import sampler_ref as RS
from oracle.imagen_ref import cast_tuple, exists, resize_image_to

HPARAM_DEFAULTS = dict(num_sample_steps=32, sigma_min=0.002, sigma_max=80, sigma_data=0.5, rho=7, P_mean=-1.2, P_std=1.2,
                       S_churn=80, S_tmin=0.05, S_tmax=50, S_noise=1.003)


def _right_pad(x, t):
    return t.reshape(t.shape + (1,) * (x.ndim - t.ndim))


class ElucidatedImagen(RS.Imagen):
    def __init__(self, unets, *, image_sizes, **kw):
        hp = {k: kw.pop(k, v) for k, v in HPARAM_DEFAULTS.items()}
        super().__init__(unets, image_sizes=image_sizes, **kw)
        n = len(self.unets)
        cast = {k: cast_tuple(v, n) for k, v in hp.items()}
        self.hparams = [{k: cast[k][i] for k in HPARAM_DEFAULTS} for i in range(n)]

    # ---- preconditioning (fp32 tensors of shape [B], the library's op order)
    @staticmethod
    def c_skip(sd, sigma):
        return (sd ** 2) / (sigma ** 2 + sd ** 2)

    @staticmethod
    def c_out(sd, sigma):
        return sigma * sd * (sd ** 2 + sigma ** 2) ** -0.5

    @staticmethod
    def c_in(sd, sigma):
        return 1 * (sigma ** 2 + sd ** 2) ** -0.5

    @staticmethod
    def c_noise(sigma):
        return torch.log(sigma.clamp(min=1e-20)) * 0.25

    def sample_schedule(self, hp):
        N = hp["num_sample_steps"]
        inv_rho = 1 / hp["rho"]
        steps = torch.arange(N, dtype=torch.float32)
        sigmas = (hp["sigma_max"] ** inv_rho + steps / (N - 1) *
                  (hp["sigma_min"] ** inv_rho - hp["sigma_max"] ** inv_rho)) ** hp["rho"]
        sigmas = F.pad(sigmas, (0, 1), value=0.0)
        gammas = torch.where((sigmas >= hp["S_tmin"]) & (sigmas <= hp["S_tmax"]),
                             min(hp["S_churn"] / N, math.sqrt(2) - 1), 0.0)
        return sigmas, gammas

    def threshold(self, x_start, dynamic_threshold):
        if not dynamic_threshold:
            return x_start.clamp(-1.0, 1.0)
        s = torch.quantile(x_start.flatten(1).abs(), self.dynamic_thresholding_percentile, dim=-1)
        s.clamp_(min=1.0)
        s = _right_pad(x_start, s)
        return x_start.clamp(-s, s) / s

    def preconditioned(self, unet, x, sigma, hp, net_kw, dynamic_threshold):
        sd = hp["sigma_data"]
        sigma = torch.full((x.shape[0],), sigma, dtype=torch.float32)
        ps = _right_pad(x, sigma)
        net_out = unet.forward_with_cond_scale(self.c_in(sd, ps) * x, self.c_noise(sigma), **net_kw)
        out = self.c_skip(sd, ps) * x + self.c_out(sd, ps) * net_out
        return self.threshold(out, dynamic_threshold)

    def p_sample_loop(self, unet, shape, *, stage, noise_fn, noise_scheduler, lowres_cond_img, lowres_noise_times,
                      text_embeds, text_mask, cond_images, inpaint_images, inpaint_masks, inpaint_resample_times,
                      cond_scale, pred_objective, dynamic_threshold, trace=None):
        hp = self.hparams[stage - 1]
        N = hp["num_sample_steps"]
        sigmas, gammas = self.sample_schedule(hp)
        pairs = list(zip(sigmas[:-1], sigmas[1:], gammas[:-1]))
        x = sigmas[0] * noise_fn(("init", stage), shape)
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
