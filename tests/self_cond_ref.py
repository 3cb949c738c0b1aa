"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of the self-conditioning of
imagen-pytorch 1.18.x (``Unet(self_cond=True)``) from the library's published algorithm, built on the existing
restatements by subclassing them:

* ``Unet``: ``init_channels = channels * (1 + lowres_cond + self_cond) + cond_images_channels``; the forward input is
  ``cat(cond_images, x, self_cond, lowres_cond_img)`` (``self_cond = None`` -> zeros).  The state-dict keys are the
  plain UNet's; only ``init_conv.convs.{0,1,2}.weight`` has 3 more input channels.
* ``Imagen`` (DDPM, ``p_sample_loop``): ``x_start = None`` per stage; every iteration (every resample of every
  timestep) feeds the previous iteration's THRESHOLDED x0 estimate as ``self_cond`` - to both forwards of guidance.
* ``ElucidatedImagen`` (``one_unet_sample``): the first forward of a step reads the previous step's last estimate, the
  Heun forward reads the first forward's thresholded denoised estimate; ``self_cond`` is not scaled by ``c_in``.

A UNet without ``self_cond`` gets no ``self_cond`` argument, so stages can be mixed.
"""
from __future__ import annotations

import torch

import elucidated_ref as ER
from oracle import imagen_ref as RI
from oracle import sampler_ref as RS


class Unet(RI.Unet):
    def __init__(self, *, self_cond=False, **kw):
        super().__init__(**kw)
        self.self_cond = bool(self_cond)
        self._locals["self_cond"] = self.self_cond   # cast_model_parameters re-creates the UNet with it
        if self.self_cond:
            old = self.init_conv
            c_in = old.convs[0].in_channels + self.channels
            self.init_conv = RI.CrossEmbedLayer(c_in, dim_out=self._locals["dim"],
                                                kernel_sizes=self._locals["init_cross_embed_kernel_sizes"], stride=1)

    def forward(self, x, time, *, self_cond=None, **kw):
        if self.self_cond:
            self_cond = self_cond if self_cond is not None else torch.zeros_like(x)
            # the base prepends cond_images and appends lowres_cond_img: cat(cond, x, self_cond, lowres)
            x = torch.cat((x, self_cond), dim=1)
        return super().forward(x, time, **kw)


def self_cond_channels(unet):
    """Input channels of init_conv that carry self_cond (cond_images | x | SELF_COND | lowres)."""
    c0 = unet.cond_images_channels + unet.channels
    return list(range(c0, c0 + unet.channels))


def plain_state_dict(sd, unet):
    """`sd` of a self-cond UNet with the self_cond input channels of the init conv dropped (the plain UNet's layout)."""
    drop = set(self_cond_channels(unet))
    out = dict(sd)
    for i in range(3):
        k = f"init_conv.convs.{i}.weight"
        keep = [c for c in range(sd[k].shape[1]) if c not in drop]
        out[k] = sd[k][:, keep].contiguous()
    return out


class _SelfCondCall:
    """Hands `self_cond` to every forward_with_cond_scale call of a self-cond UNet (both forwards of guidance)."""

    def __init__(self, unet, self_cond):
        self.unet, self.sc = unet, self_cond

    def forward_with_cond_scale(self, *a, **k):
        return self.unet.forward_with_cond_scale(*a, self_cond=self.sc, **k)


def _wants(unet):
    return bool(getattr(unet, "self_cond", False))


class Imagen(RS.Imagen):
    """DDPM sampler with the x_start carry.  `x_start_log` (if a list) receives, per iteration, the (self_cond fed,
    x_start returned) pair of a self-cond stage."""

    x_start_log = None

    def p_sample(self, unet, x, t, noise, **kw):
        if not _wants(unet):
            return super().p_sample(unet, x, t, noise, **kw)
        fed = self._x_start
        img, x_start = super().p_sample(_SelfCondCall(unet, fed), x, t, noise, **kw)
        if self.x_start_log is not None:
            self.x_start_log.append((fed, x_start))
        self._x_start = x_start
        return img, x_start

    def p_sample_loop(self, unet, shape, **kw):
        self._x_start = None   # per stage
        return super().p_sample_loop(unet, shape, **kw)


class ElucidatedImagen(ER.ElucidatedImagen):
    """EDM sampler with the x_start carry: each preconditioned forward reads the last thresholded estimate."""

    def preconditioned(self, unet, x, sigma, hp, net_kw, dynamic_threshold):
        if not _wants(unet):
            return super().preconditioned(unet, x, sigma, hp, net_kw, dynamic_threshold)
        out = super().preconditioned(unet, x, sigma, hp, {**net_kw, "self_cond": self._x_start}, dynamic_threshold)
        self._x_start = out
        return out

    def p_sample_loop(self, unet, shape, **kw):
        self._x_start = None
        return super().p_sample_loop(unet, shape, **kw)
