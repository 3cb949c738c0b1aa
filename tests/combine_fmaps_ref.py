"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of
``Unet(combine_upsample_fmaps=True)`` of imagen-pytorch 1.18.x from the library's published code, on top of
``resample_ref.Unet`` with stock torch ops only.

Constructor, with ``dims = [dim, *dim * dim_mults]`` and L levels: up level i (deepest first) works at ``dims[L - i]``
channels; ``upsample_combiner.fmap_convs = ModuleList([Block(dims[L - i], dim) for i in range(L)])`` where ``Block`` is
``GroupNorm(8, dim_in) -> SiLU -> Conv2d(dim_in, dim, 3, padding=1)`` with Block's OWN default of 8 groups (not
``resnet_groups``) and no FiLM; ``final_res_block`` takes ``dim * (1 + L) (+ dim with init_conv_to_final_conv_residual)``
channels.  Disabled: no parameters, nothing changes.

Forward: in up level i, after its attention slot ``ups.i.2`` (Identity included) and before its upsample, the map is kept.
After the loop every kept map is brought to x's size with ``F.interpolate(mode='nearest')``, goes through its Block, and
``x = cat((x, *outs), dim=1)``; only then comes the optional ``cat((x, init_conv_residual), dim=1)`` and final_res_block.
Channel order in front of final_res_block: ``[x | out_0 (deepest) .. out_{L-1} | init residual]``.

The maps are collected with forward hooks on ``ups.i.2`` and the concat is rebuilt in a forward pre-hook of
``final_res_block`` (whose input is ``cat(x, init residual)``), so every forward variant of the parents is covered.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

import resample_ref as RR
from oracle import imagen_ref as RI


class UpsampleCombiner(nn.Module):
    def __init__(self, dim_ins, dim_out):
        super().__init__()
        self.fmap_convs = nn.ModuleList([RI.Block(d, dim_out) for d in dim_ins])   # groups = Block's default, 8

    def forward(self, x, fmaps):
        size = x.shape[-1]
        fmaps = [F.interpolate(f, size, mode="nearest") for f in fmaps]
        outs = [conv(f) for f, conv in zip(fmaps, self.fmap_convs)]
        return torch.cat((x, *outs), dim=1)


class Unet(RR.Unet):
    def __init__(self, *, combine_upsample_fmaps=False, **kw):
        super().__init__(**kw)
        self._locals.update(combine_upsample_fmaps=combine_upsample_fmaps)
        self.combine_upsample_fmaps = bool(combine_upsample_fmaps)
        if not combine_upsample_fmaps:
            return
        loc = self._locals
        dim, L = loc["dim"], len(loc["dim_mults"])
        dims = [dim, *[dim * m for m in loc["dim_mults"]]]
        old = self.final_res_block
        self.upsample_combiner = UpsampleCombiner(tuple(dims[L - i] for i in range(L)), dim)
        fin = dim * (1 + L) + (dim if self.init_conv_to_final_conv_residual else 0)
        self.final_res_block = RI.ResnetBlock(fin, dim, time_cond_dim=old.time_mlp[1].in_features,
                                              groups=old.block1.groupnorm.num_groups, use_gca=True)
        self._dim = dim
        self._up_hiddens = []
        for lvl in self.ups:
            lvl[2].register_forward_hook(self._keep_map)
        self.final_res_block.register_forward_pre_hook(self._combine)

    def _keep_map(self, module, args, output):
        self._up_hiddens.append(output)

    def _combine(self, module, args):
        x, *rest = args
        maps, self._up_hiddens = self._up_hiddens, []
        assert len(maps) == len(self.ups)
        x, init_residual = x[:, :self._dim], x[:, self._dim:]   # (the residual half is empty without the switch)
        x = self.upsample_combiner(x, maps)
        return (torch.cat((x, init_residual), dim=1), *rest)
