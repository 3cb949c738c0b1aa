"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of the two other resampling
forms of imagen-pytorch 1.18.x from the library's published code, built on the existing restatements by subclassing
them (oracle.imagen_ref -> self_cond_ref -> linear_attn_ref), with stock torch ops only:

* ``Unet(cross_embed_downsample=True)`` (``cross_embed_downsample_kernel_sizes=(2, 4)``): every ``Downsample(d, d_out)`` -
  the pre-downsample ``downs.L.0`` of a memory_efficient UNet, the post-downsample ``downs.L.4`` otherwise - is
  ``CrossEmbedLayer(d, kernel_sizes=(2, 4), dim_out=d_out, stride=2)`` =
  ``cat([Conv2d(d, d_out // 2, 2, stride 2, pad 0)(x), Conv2d(d, d_out - d_out // 2, 4, stride 2, pad 1)(x)], dim=1)``,
  keys ``<pre>.convs.{0,1}.{weight,bias}``.  The last level's ``Parallel(conv3x3, conv1x1)`` is unchanged.
* ``Unet(pixel_shuffle_upsample=False)``: every ``PixelShuffleUpsample(d, d_out)`` is
  ``nn.Sequential(nn.Upsample(scale_factor=2, mode='nearest'), nn.Conv2d(d, d_out, 3, padding=1))``, keys
  ``ups.j.3.1.{weight,bias}``, no activation; ``Identity`` stays where it was (the last up level of a UNet that is not
  memory_efficient).

The samplers are the existing restatements: they only call the UNet.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

import linear_attn_ref as LR
from oracle import imagen_ref as RI


class NearestUpsample(nn.Module):   # nn.Upsample(scale_factor=2, mode='nearest')
    def forward(self, x):
        return F.interpolate(x, scale_factor=2, mode="nearest")


class CrossEmbedDownsample(nn.Module):
    """CrossEmbedLayer(dim_in, kernel_sizes, dim_out, stride=2) spelled out with F.conv2d and torch.cat."""

    def __init__(self, dim_in, kernel_sizes, dim_out):
        super().__init__()
        kernel_sizes = sorted(kernel_sizes)
        scales = [int(dim_out / (2 ** i)) for i in range(1, len(kernel_sizes))]
        scales = [*scales, dim_out - sum(scales)]
        self.convs = nn.ModuleList([nn.Conv2d(dim_in, s, k, stride=2, padding=(k - 2) // 2) for k, s in zip(kernel_sizes, scales)])

    def forward(self, x):
        return torch.cat([F.conv2d(x, c.weight, c.bias, stride=2, padding=c.padding) for c in self.convs], dim=1)


def nearest_conv_upsample(dim, dim_out):
    return nn.Sequential(NearestUpsample(), nn.Conv2d(dim, dim_out, 3, padding=1))


class Unet(LR.SelfCondUnet):
    def __init__(self, *, cross_embed_downsample=False, cross_embed_downsample_kernel_sizes=(2, 4),
                 pixel_shuffle_upsample=True, **kw):
        super().__init__(**kw)
        loc = self._locals
        loc.update(cross_embed_downsample=cross_embed_downsample,
                   cross_embed_downsample_kernel_sizes=cross_embed_downsample_kernel_sizes,
                   pixel_shuffle_upsample=pixel_shuffle_upsample)
        self.cross_embed_downsample = bool(cross_embed_downsample)
        L = len(loc["dim_mults"])
        dims = [loc["dim"], *[loc["dim"] * m for m in loc["dim_mults"]]]
        for l in range(L):
            j = L - 1 - l
            if cross_embed_downsample:
                for slot in (0, 4):
                    if isinstance(self.downs[l][slot], (nn.Sequential, nn.Conv2d)):   # a Downsample: not None, not the Parallel
                        self.downs[l][slot] = CrossEmbedDownsample(dims[l], cross_embed_downsample_kernel_sizes, dims[l + 1])
            if not pixel_shuffle_upsample and isinstance(self.ups[j][3], RI.PixelShuffleUpsample):
                self.ups[j][3] = nearest_conv_upsample(dims[l + 1], dims[l])

    def set_version_forks(self, downsample_form=None, mid_attn_form=None):
        # a cross-embed UNet has no Downsample fork (its slots hold neither form of it)
        return super().set_version_forks(None if self.cross_embed_downsample else downsample_form, mid_attn_form)
