"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): a restatement of the linear attention of
imagen-pytorch 1.18.x (``Unet(use_linear_attn=..., use_linear_cross_attn=...)``) from the library's published algorithm,
built on the existing restatements by subclassing them:

* ``LinearAttention`` / ``ChanFeedForward`` / ``LinearAttentionTransformerBlock`` on NCHW maps: ChanLayerNorm, q / k / v
  as (Dropout, 1x1 conv, depthwise 3x3 conv), the context tokens' keys / values (``to_context``) appended AFTER the
  H*W tokens, softmax of q over d (times dim_head^-0.5), of k over all tokens, SiLU(q (k^T v)), 1x1 conv + ChanLayerNorm.
* ``LinearCrossAttention``: CrossAttention's parameters; the null key / value (shared by the heads) in front of to_kv(c),
  the same two softmaxes, q (k^T v) without SiLU.
* ``Unet``: at level l the attention slot holds a TransformerBlock if layer_attns[l], else a
  LinearAttentionTransformerBlock if use_linear_attn[l]; the level's first ResnetBlocks get cross-attention when
  layer_cross_attns[l] or use_linear_cross_attn[l], the linear form when use_linear_cross_attn[l].  Both kwargs are a
  bool or a per-level tuple.

The samplers are the existing restatements (``oracle.sampler_ref``, ``tests/elucidated_ref.py``): they only call the UNet.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

import self_cond_ref as SR
from oracle import imagen_ref as RI


class ChanLayerNorm(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.g = nn.Parameter(torch.ones(1, dim, 1, 1))

    def forward(self, x):
        var = torch.var(x, dim=1, unbiased=False, keepdim=True)
        mean = torch.mean(x, dim=1, keepdim=True)
        return (x - mean) * (var + 1e-5).rsqrt() * self.g


def linear_attention_core(q, k, v, scale, silu):
    """q [b h n d], k / v [b h j d] (every key in place): SiLU?(softmax_d(q) scale (softmax_j(k)^T v))."""
    q = q.softmax(dim=-1) * scale
    k = k.softmax(dim=-2)
    ctx = torch.einsum("bhnd,bhne->bhde", k, v)
    out = torch.einsum("bhnd,bhde->bhne", q, ctx)
    return F.silu(out) if silu else out


class LinearAttention(nn.Module):
    def __init__(self, dim, *, dim_head=32, heads=8, context_dim=None):
        super().__init__()
        self.scale = dim_head ** -0.5
        self.heads = heads
        inner = dim_head * heads
        self.norm = ChanLayerNorm(dim)

        def proj():
            return nn.Sequential(nn.Dropout(0.0), nn.Conv2d(dim, inner, 1, bias=False),
                                 nn.Conv2d(inner, inner, 3, bias=False, padding=1, groups=inner))

        self.to_q, self.to_k, self.to_v = proj(), proj(), proj()
        self.to_context = (nn.Sequential(nn.LayerNorm(context_dim), nn.Linear(context_dim, inner * 2, bias=False))
                           if context_dim is not None else None)
        self.to_out = nn.Sequential(nn.Conv2d(inner, dim, 1, bias=False), ChanLayerNorm(dim))

    def forward(self, fmap, context=None):
        b, _, hh, ww = fmap.shape
        h = self.heads
        fmap = self.norm(fmap)
        heads = lambda t: t.reshape(b, h, -1, hh * ww).transpose(-1, -2)   # b (h c) x y -> b h (x y) c
        q, k, v = (heads(fn(fmap)) for fn in (self.to_q, self.to_k, self.to_v))
        if context is not None:
            ck, cv = self.to_context(context).chunk(2, dim=-1)
            split = lambda t: t.reshape(b, t.shape[1], h, -1).transpose(1, 2)
            k = torch.cat((k, split(ck)), dim=-2)
            v = torch.cat((v, split(cv)), dim=-2)
        out = linear_attention_core(q, k, v, self.scale, silu=True)   # b h (x y) d
        return self.to_out(out.transpose(-1, -2).reshape(b, -1, hh, ww))


def ChanFeedForward(dim, mult=2):
    hidden = int(dim * mult)
    return nn.Sequential(ChanLayerNorm(dim), nn.Conv2d(dim, hidden, 1, bias=False), nn.GELU(), ChanLayerNorm(hidden),
                         nn.Conv2d(hidden, dim, 1, bias=False))


class LinearAttentionTransformerBlock(nn.Module):
    def __init__(self, dim, *, depth=1, heads=8, dim_head=32, ff_mult=2, context_dim=None):
        super().__init__()
        self.layers = nn.ModuleList([
            nn.ModuleList([LinearAttention(dim, heads=heads, dim_head=dim_head, context_dim=context_dim),
                           ChanFeedForward(dim, mult=ff_mult)]) for _ in range(depth)])

    def forward(self, x, context=None):
        for attn, ff in self.layers:
            x = attn(x, context=context) + x
            x = ff(x) + x
        return x


class LinearCrossAttention(RI.CrossAttention):
    def forward(self, x, context):
        b, n, _ = x.shape
        h = self.heads
        x = self.norm(x)
        q = self.to_q(x)
        k, v = self.to_kv(context).chunk(2, dim=-1)
        split = lambda t: t.reshape(b, t.shape[1], h, -1).transpose(1, 2)
        q, k, v = split(q), split(k), split(v)
        nk, nv = self.null_kv.unbind(dim=-2)
        k = torch.cat((nk.expand(b, h, 1, -1), k), dim=-2)
        v = torch.cat((nv.expand(b, h, 1, -1), v), dim=-2)
        out = linear_attention_core(q, k, v, self.scale, silu=False)
        return self.to_out(out.transpose(1, 2).reshape(b, n, -1))


def _place_cross_attn(rb):
    """A cross_attn added to a ResnetBlock built without one goes where the library registers it: behind time_mlp."""
    mods = rb._modules
    items = [(k, m) for k, m in mods.items() if k != "cross_attn"]
    items.insert(1 if "time_mlp" in mods else 0, ("cross_attn", mods["cross_attn"]))
    mods.clear()
    mods.update(items)


class Unet(RI.Unet):
    def __init__(self, *, use_linear_attn=False, use_linear_cross_attn=False, **kw):
        super().__init__(**kw)
        loc = self._locals
        loc.update(use_linear_attn=use_linear_attn, use_linear_cross_attn=use_linear_cross_attn)
        L = len(loc["dim_mults"])
        lin = RI.cast_tuple(use_linear_attn, L)
        lcross = RI.cast_tuple(use_linear_cross_attn, L)
        attns = RI.cast_tuple(loc["layer_attns"], L)
        dims = [loc["dim"], *[loc["dim"] * m for m in loc["dim_mults"]]]
        ak = dict(heads=loc["attn_heads"], dim_head=loc["attn_dim_head"], ff_mult=loc["ff_mult"], context_dim=self.cond_dim)
        for l in range(L):
            j = L - 1 - l
            cur = dims[l + 1] if loc["memory_efficient"] else dims[l]
            if lin[l] and not attns[l]:
                self.downs[l][3] = LinearAttentionTransformerBlock(cur, **ak)
                self.ups[j][2] = LinearAttentionTransformerBlock(dims[l + 1], **ak)
            if lcross[l]:
                for rb in (self.downs[l][1], self.ups[j][0]):
                    had = rb.cross_attn is not None
                    rb.cross_attn = LinearCrossAttention(rb.block2.project.out_channels, context_dim=self.cond_dim,
                                                         heads=loc["attn_heads"], dim_head=loc["attn_dim_head"])
                    if not had:
                        _place_cross_attn(rb)
        self.set_attn_qk_norm(self.attn_qk_norm)


class SelfCondUnet(SR.Unet, Unet):
    """Unet(self_cond=True, use_linear_attn=...): both restatements (MRO: the self_cond input, then the linear modules)."""
