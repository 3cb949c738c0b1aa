"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of the structural switches of
the first and the last layer of ``Unet`` in imagen-pytorch 1.18.x, from the library's published code, on top of
``combine_fmaps_ref.Unet`` (and so of every other restatement: self-conditioning, linear attention, the resampling forms,
the UpsampleCombiner) with stock torch ops only.

The oracle takes three of the five switches itself: ``scale_skip_connection`` (skips times 1 instead of 2^-0.5),
``final_conv_kernel_size`` (``final_conv`` is k x k, padding k // 2) and ``init_cross_embed_kernel_sizes`` (the
CrossEmbedLayer sorts the sizes; widths ``dim / 2, dim / 4, .., the rest``).  Added here:

* ``init_cross_embed=False`` / ``init_conv_kernel_size=7``: ``init_conv = Conv2d(init_channels, dim, k, padding=k // 2)``,
  keys ``init_conv.{weight,bias}``.
* ``final_resnet_block=False``: the library sets ``final_res_block = None`` and skips it; ``final_conv`` then reads
  ``cat(x[, combiner maps][, init conv residual][, lowres_cond_img])``: ``dim (+ dim L) (+ dim) (+ channels)`` input
  channels.  Here a parameter-free pass-through sits in the slot (the parents' forwards call it, and the combiner's concat is
  rebuilt in its pre-hook), so the state dict has no ``final_res_block.*`` keys.
"""
from __future__ import annotations

from torch import nn

import combine_fmaps_ref as CR


class _PassThrough(nn.Module):
    def forward(self, x, *a, **k):
        return x


class Unet(CR.Unet):
    def __init__(self, *, init_cross_embed=True, init_conv_kernel_size=7, final_resnet_block=True, **kw):
        super().__init__(**kw)
        self._locals.update(init_cross_embed=init_cross_embed, init_conv_kernel_size=init_conv_kernel_size,
                            final_resnet_block=final_resnet_block)
        loc = self._locals
        dim = loc["dim"]
        if not init_cross_embed:
            c_in = self.init_conv.convs[0].in_channels   # (the parents have counted self_cond / lowres / cond_images in)
            self.init_conv = nn.Conv2d(c_in, dim, init_conv_kernel_size, padding=init_conv_kernel_size // 2)
        if not final_resnet_block:
            fin = dim + (dim * len(loc["dim_mults"]) if self.combine_upsample_fmaps else 0) + \
                (dim if self.init_conv_to_final_conv_residual else 0)
            self.final_res_block = _PassThrough()
            if self.combine_upsample_fmaps:
                self.final_res_block.register_forward_pre_hook(self._combine)
            k = loc["final_conv_kernel_size"]
            self.final_conv = nn.Conv2d(fin + (self.channels if self.lowres_cond else 0), self.channels_out, k, padding=k // 2)
            nn.init.zeros_(self.final_conv.weight)
            nn.init.zeros_(self.final_conv.bias)


FIVE = dict(init_cross_embed=False, init_conv_kernel_size=5, final_conv_kernel_size=5, final_resnet_block=False,
            scale_skip_connection=False)
