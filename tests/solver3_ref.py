"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of the third-order and the
stochastic few-step solvers - ``sample(sampler="dpmpp_3m" | "dpmpp_2m_sde" | "dpmpp_3m_sde", sampler_eta=...)`` - written
from the formulas of the multistep exponential integrator in data prediction, over the step of tests/solver_ref.py
(``p_sample`` for the thresholded estimate; inpaint mix and re-noise the parent's).  Nothing here comes from
imagen-pytorch: the library has none of them.  Every other sampler is solver_ref's.

With a, s = alpha, sigma at t_k, a', s' at t_{k+1}, lambda = log_snr / 2, h_k = lambda' - lambda, he = h_k (1 + eta):

    A = (s'/s) exp(-eta h_k)      b = -a' expm1(-he)      S = s' sqrt(-expm1(-2 eta h_k))   (no noise on the last step)
    phi2 = expm1(-he) / he + 1    phi3 = phi2 / he - 1/2

and the order of step k is ``o = min(cap, k - skip + 1, N - k)``, cap 3 for the 3M names and 2 for ``dpmpp_2m_sde``:

    o = 1:  x = A x + b x0c + S z
    o = 2:  r = h_{k-1} / h_k,  D1 = (x0c - x0c_{k-1}) / r;  x = A x + b x0c + a' phi2 D1 + S z
    o = 3:  r0 = h_{k-1} / h_k, r1 = h_{k-2} / h_k, D1_0 = (x0c - x0c_{k-1}) / r0, D1_1 = (x0c_{k-1} - x0c_{k-2}) / r1,
            D1 = D1_0 + r0 / (r0 + r1) (D1_0 - D1_1),  D2 = (D1_0 - D1_1) / (r0 + r1);
            x = A x + b x0c + a' phi2 D1 - a' phi3 D2 + S z

(the divided differences of the estimates over lambda; eta = 0 is the deterministic solver).  ``sampler_eta`` None is 1 for
the ``_sde`` names.  The scalars are formed in float64 from the scheduler's fp32 log-SNRs and applied to fp32 images.  Tag
("step", stage, k, r), asked for only in the steps that add noise.  Under inpainting with resampling every resample of step
k reads the estimates that the LAST resamples of steps k - 1 and k - 2 left.
The self-conditioning restatement combines by inheritance: ``class X(self_cond_ref.Imagen, solver3_ref.Imagen)``.
"""
from __future__ import annotations

import math

import torch

import solver_ref as SR
from oracle import sampler_ref as RS
from oracle.imagen_ref import exists, resize_image_to

_pad = RS._pad
CAPS = {"dpmpp_3m": 3, "dpmpp_2m_sde": 2, "dpmpp_3m_sde": 3}


class Imagen(SR.Imagen):
    _solvers3 = None

    @torch.no_grad()
    def sample(self, *, sampler=None, sampler_eta=None, **kw):
        n = len(self.unets)
        names, etas = SR.cast_per_unet(sampler, n), SR.cast_per_unet(sampler_eta, n)
        assert len(names) == n and len(etas) == n
        etas = [(1.0 if str(nm).endswith("_sde") else 0.0) if e is None else float(e) for nm, e in zip(names, etas)]
        self._solvers3 = list(zip(names, etas))
        # the parent walks every stage; a stage of the new names is taken over in p_sample_loop below
        parent = [nm if nm not in CAPS else "ddim" for nm in names]
        try:
            return super().sample(sampler=parent, sampler_eta=[e if nm not in CAPS else 0.0 for nm, e in zip(names, etas)], **kw)
        finally:
            self._solvers3 = None

    def p_sample_loop(self, unet, shape, *, stage, noise_fn, noise_scheduler, lowres_cond_img, lowres_noise_times,
                      text_embeds, text_mask, cond_images, inpaint_images, inpaint_masks, inpaint_resample_times,
                      cond_scale, pred_objective, dynamic_threshold, trace=None):
        name, eta = self._solvers3[stage - 1] if exists(self._solvers3) else (None, 0.0)
        if name not in CAPS:
            return super().p_sample_loop(
                unet, shape, stage=stage, noise_fn=noise_fn, noise_scheduler=noise_scheduler,
                lowres_cond_img=lowres_cond_img, lowres_noise_times=lowres_noise_times, text_embeds=text_embeds,
                text_mask=text_mask, cond_images=cond_images, inpaint_images=inpaint_images, inpaint_masks=inpaint_masks,
                inpaint_resample_times=inpaint_resample_times, cond_scale=cond_scale, pred_objective=pred_objective,
                dynamic_threshold=dynamic_threshold, trace=trace)
        cap = CAPS[name]
        assert (eta > 0) == name.endswith("_sde")
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
        N = len(steps)
        f64 = lambda t: float(t.double().flatten()[0])
        lam = [f64(noise_scheduler.log_snr(t)) / 2 for t, _ in steps]
        lam_next = [f64(noise_scheduler.log_snr(tn)) / 2 for _, tn in steps]
        hs = [b - a for a, b in zip(lam, lam_next)]
        x0_1 = x0_2 = None                                                               # of steps k - 1 and k - 2
        for k, (times, times_next) in enumerate(steps):
            if k < skip:
                continue
            is_last_timestep = times_next == 0
            last = k == N - 1
            a, s = (f64(v) for v in RS.log_snr_to_alpha_sigma(noise_scheduler.log_snr(times)))
            a_next, s_next = (f64(v) for v in RS.log_snr_to_alpha_sigma(noise_scheduler.log_snr(times_next)))
            h = hs[k]
            he = h * (1 + eta)
            A = (s_next / s) * math.exp(-eta * h)
            b = -a_next * math.expm1(-he)
            phi2 = math.expm1(-he) / he + 1
            phi3 = phi2 / he - 0.5
            S = 0.0 if last or eta == 0 else s_next * math.sqrt(-math.expm1(-2 * eta * h))
            order = min(cap, k - skip + 1, N - k)
            for r in reversed(range(resample_times)):
                if has_inpainting:
                    noised = noise_scheduler.q_sample(inpaint_images, times, noise_fn(("inpaint", stage, k, r), shape))
                    img = img * ~inpaint_masks + noised * inpaint_masks
                # the thresholded estimate of this iteration (the ancestral image that comes with it is not used)
                _, x0c = self.p_sample(unet, img, times, torch.zeros(shape), t_next=times_next, **kw)
                new = A * img + b * x0c
                if order == 2:
                    D1 = (x0c - x0_1) / (hs[k - 1] / h)
                    new = new + a_next * phi2 * D1
                elif order == 3:
                    r0, r1 = hs[k - 1] / h, hs[k - 2] / h
                    D1_0, D1_1 = (x0c - x0_1) / r0, (x0_1 - x0_2) / r1
                    D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
                    D2 = (D1_0 - D1_1) / (r0 + r1)
                    new = new + a_next * phi2 * D1 - a_next * phi3 * D2
                if S != 0.0:
                    new = new + S * noise_fn(("step", stage, k, r), shape)
                img = new
                if r == 0:
                    x0_new = x0c
                if has_inpainting and not (r == 0 or bool(torch.all(is_last_timestep))):
                    renoised = noise_scheduler.q_sample_from_to(
                        img, times_next, times, noise_fn(("renoise", stage, k, r), shape))
                    img = torch.where(_pad(img, is_last_timestep), img, renoised)
            x0_2, x0_1 = x0_1, x0_new
            if exists(trace):
                trace.append(img.clone())
        img = img.clamp(-1.0, 1.0)
        if has_inpainting:
            img = img * ~inpaint_masks + inpaint_images * inpaint_masks
        return self.unnormalize_img(img)
