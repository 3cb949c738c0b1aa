"""Drop-in `imagen_pytorch` surface for the sampling path of jameshball/kidney-diffusion,
backed by the MI355X HIP engine (``libkd_engine.so``).

What the reference imports and calls:
  * ``Unet(...)``     kwargs at train_ultra_res.py:29-60, train.py:30-65, train_uncond.py:30-61
  * ``NullUnet``      subclassed at train_ultra_res.py:65-75
  * ``Imagen(...)``   kwargs at train_ultra_res.py:79-90, train.py:83-93, train_uncond.py:79-90
  * ``imagen.sample`` sample_ultra_res.py:183-195, outpainting.py:146-157
  * checkpoint dict   {'model', 'version', ...}  sample_ultra_res.py:53-63

The classes are ``nn.Module``s whose parameter tree (names, shapes, default init) follows
imagen-pytorch 1.18.5 so that ``state_dict`` / ``load_state_dict(strict=True)``
behave as the reference expects; they hold no torch arithmetic.  ``Unet.forward`` and
``Imagen.sample`` hand device pointers to the engine.  Without the HIP library or a GPU they raise
— there is no CPU fallback in this package.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
from typing import Callable, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _engine as E


def exists(v):
    return v is not None


def default(v, d):
    if exists(v):
        return v
    return d() if callable(d) else d


def cast_tuple(v, length=None):
    if isinstance(v, list):
        v = tuple(v)
    out = v if isinstance(v, tuple) else ((v,) * default(length, 1))
    if exists(length):
        assert len(out) == length, f"expected a tuple of length {length}, got {out}"
    return out


# ============================================================================ parameter tree
# Containers below only declare parameters; `_no_forward` documents that the arithmetic lives in
# the engine.
class _Decl(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError(f"{type(self).__name__} holds parameters only; the forward pass runs in libkd_engine")


class LayerNorm(_Decl):  # gain-only
    def __init__(self, feats):
        super().__init__()
        self.g = nn.Parameter(torch.ones(feats))


class _Stateless(_Decl):  # placeholder that keeps nn.Sequential indices aligned with the library
    pass


class LearnedSinusoidalPosEmb(_Decl):
    def __init__(self, dim):
        super().__init__()
        assert dim % 2 == 0
        self.weights = nn.Parameter(torch.randn(dim // 2))


class CrossEmbedLayer(_Decl):
    def __init__(self, dim_in, kernel_sizes, dim_out, stride=1):
        super().__init__()
        kernel_sizes = sorted(kernel_sizes)
        scales = [int(dim_out / (2 ** i)) for i in range(1, len(kernel_sizes))]
        scales.append(dim_out - sum(scales))
        self.convs = nn.ModuleList(
            [nn.Conv2d(dim_in, s, k, stride=stride, padding=(k - stride) // 2) for k, s in zip(kernel_sizes, scales)])


def _downsample(dim, dim_out, form="unshuffle"):
    """Library 1.18.x: Rearrange (pixel-unshuffle) + Conv2d(4 dim, dim_out, 1), keys `<pre>.1.*`; earlier versions:
    Conv2d(dim, dim_out, 4, 2, 1), keys `<pre>.*` with a [dim_out, dim, 4, 4] weight (SURVEY A.1 version fork)."""
    if form == "conv4x4":
        return nn.Conv2d(dim, dim_out, 4, 2, 1)
    assert form == "unshuffle"
    return nn.Sequential(_Stateless(), nn.Conv2d(dim * 4, dim_out, 1))


class PixelShuffleUpsample(_Decl):
    def __init__(self, dim, dim_out):
        super().__init__()
        conv = nn.Conv2d(dim, dim_out * 4, 1)
        self.net = nn.Sequential(conv, _Stateless(), _Stateless())
        o, i, h, w = conv.weight.shape
        w0 = torch.empty(o // 4, i, h, w)
        nn.init.kaiming_uniform_(w0)
        with torch.no_grad():
            conv.weight.copy_(w0.repeat_interleave(4, dim=0))
            conv.bias.zero_()


class Parallel(_Decl):
    def __init__(self, *fns):
        super().__init__()
        self.fns = nn.ModuleList(fns)


class _QKNorm:
    """Attention similarity variant of the module (include/kd_engine.h `attn_qk_norm`): 0 scaled dot product,
    1 cosine-sim (l2norm q, k; x16), 2 learned q_scale / k_scale on the normalised q, k (x8).  Variant 2 owns
    two more parameters; a module switches to it when a checkpoint carries them (Unet._load_from_state_dict)."""
    dim_head = 64

    def set_qk_norm(self, mode):
        if mode == 2 and not hasattr(self, "q_scale"):
            ref = self.to_q.weight
            self.q_scale = nn.Parameter(torch.ones(self.dim_head, device=ref.device, dtype=ref.dtype))
            self.k_scale = nn.Parameter(torch.ones(self.dim_head, device=ref.device, dtype=ref.dtype))
        if mode != 2 and hasattr(self, "q_scale"):
            del self.q_scale, self.k_scale


class Attention(_Decl, _QKNorm):
    def __init__(self, dim, *, dim_head, heads, context_dim=None):
        super().__init__()
        self.dim_head = dim_head
        inner = dim_head * heads
        self.norm = LayerNorm(dim)
        self.null_kv = nn.Parameter(torch.randn(2, dim_head))
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(dim, dim_head * 2, bias=False)
        self.to_context = (nn.Sequential(nn.LayerNorm(context_dim), nn.Linear(context_dim, dim_head * 2))
                           if exists(context_dim) else None)
        self.to_out = nn.Sequential(nn.Linear(inner, dim, bias=False), LayerNorm(dim))


class CrossAttention(_Decl, _QKNorm):
    def __init__(self, dim, *, context_dim, dim_head, heads):
        super().__init__()
        self.dim_head = dim_head
        inner = dim_head * heads
        self.norm = LayerNorm(dim)
        self.null_kv = nn.Parameter(torch.randn(2, dim_head))
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(context_dim, inner * 2, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim, bias=False), LayerNorm(dim))


class LinearCrossAttention(CrossAttention):
    """The library's linear-attention form of CrossAttention: the same parameters and keys (q_scale / k_scale of the
    learned-qk-norm fork load with it and are not used by the linear form)."""


class ChanLayerNorm(_Decl):  # gain-only, over the channels of an NCHW map
    def __init__(self, dim):
        super().__init__()
        self.g = nn.Parameter(torch.ones(1, dim, 1, 1))


class LinearAttention(_Decl):
    """q / k / v: (Dropout, 1x1 conv, depthwise 3x3 conv), no biases; to_context: LayerNorm + Linear without bias."""

    def __init__(self, dim, *, dim_head, heads, context_dim=None):
        super().__init__()
        inner = dim_head * heads
        self.norm = ChanLayerNorm(dim)

        def proj():
            return nn.Sequential(_Stateless(), nn.Conv2d(dim, inner, 1, bias=False),
                                 nn.Conv2d(inner, inner, 3, bias=False, padding=1, groups=inner))

        self.to_q, self.to_k, self.to_v = proj(), proj(), proj()
        self.to_context = (nn.Sequential(nn.LayerNorm(context_dim), nn.Linear(context_dim, inner * 2, bias=False))
                           if exists(context_dim) else None)
        self.to_out = nn.Sequential(nn.Conv2d(inner, dim, 1, bias=False), ChanLayerNorm(dim))


def _chan_feed_forward(dim, mult):
    hidden = int(dim * mult)
    return nn.Sequential(ChanLayerNorm(dim), nn.Conv2d(dim, hidden, 1, bias=False), _Stateless(), ChanLayerNorm(hidden),
                         nn.Conv2d(hidden, dim, 1, bias=False))


class LinearAttentionTransformerBlock(_Decl):
    def __init__(self, dim, *, depth, heads, dim_head, ff_mult, context_dim=None):
        super().__init__()
        self.layers = nn.ModuleList([
            nn.ModuleList([LinearAttention(dim, dim_head=dim_head, heads=heads, context_dim=context_dim),
                           _chan_feed_forward(dim, ff_mult)]) for _ in range(depth)])


def _feed_forward(dim, mult):
    hidden = int(dim * mult)
    return nn.Sequential(LayerNorm(dim), nn.Linear(dim, hidden, bias=False), _Stateless(), LayerNorm(hidden),
                         nn.Linear(hidden, dim, bias=False))


class _Fn(_Decl):   # one `.fn` level of the key path (Residual / EinopsToAndFrom wrappers of the library)
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


class ResidualAttentionBlock(_Decl):
    """mid_attn of earlier library versions: EinopsToAndFrom(Residual(Attention(mid_dim))) - keys `mid_attn.fn.fn.*`,
    attention + residual without a feed-forward (SURVEY A.1 version fork)."""

    def __init__(self, dim, *, heads, dim_head):
        super().__init__()
        self.fn = _Fn(Attention(dim, dim_head=dim_head, heads=heads))


class TransformerBlock(_Decl):
    def __init__(self, dim, *, depth, heads, dim_head, ff_mult, context_dim=None):
        super().__init__()
        self.layers = nn.ModuleList([
            nn.ModuleList([Attention(dim, dim_head=dim_head, heads=heads, context_dim=context_dim),
                           _feed_forward(dim, ff_mult)]) for _ in range(depth)])


class PerceiverAttention(_Decl, _QKNorm):
    def __init__(self, *, dim, dim_head, heads):
        super().__init__()
        self.dim_head = dim_head
        inner = dim_head * heads
        self.norm = nn.LayerNorm(dim)
        self.norm_latents = nn.LayerNorm(dim)
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(dim, inner * 2, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim, bias=False), nn.LayerNorm(dim))


class PerceiverResampler(_Decl):
    def __init__(self, *, dim, depth, dim_head, heads, num_latents, num_latents_mean_pooled=4, max_seq_len=512,
                 ff_mult=4):
        super().__init__()
        self.pos_emb = nn.Embedding(max_seq_len, dim)
        self.latents = nn.Parameter(torch.randn(num_latents, dim))
        self.to_latents_from_mean_pooled_seq = nn.Sequential(
            LayerNorm(dim), nn.Linear(dim, dim * num_latents_mean_pooled), _Stateless())
        self.layers = nn.ModuleList([
            nn.ModuleList([PerceiverAttention(dim=dim, dim_head=dim_head, heads=heads), _feed_forward(dim, ff_mult)])
            for _ in range(depth)])
        self.num_tokens = num_latents + num_latents_mean_pooled


class GlobalContext(_Decl):
    def __init__(self, *, dim_in, dim_out):
        super().__init__()
        self.to_k = nn.Conv2d(dim_in, 1, 1)
        hidden = max(3, dim_out // 2)
        self.net = nn.Sequential(nn.Conv2d(dim_in, hidden, 1), _Stateless(), nn.Conv2d(hidden, dim_out, 1),
                                 _Stateless())


class Block(_Decl):
    def __init__(self, dim, dim_out, groups):
        super().__init__()
        self.groupnorm = nn.GroupNorm(groups, dim)
        self.project = nn.Conv2d(dim, dim_out, 3, padding=1)


class UpsampleCombiner(_Decl):   # enabled form only: a disabled combiner has no parameters and is not declared
    def __init__(self, dim_ins, dim_out):
        super().__init__()
        self.fmap_convs = nn.ModuleList([Block(d, dim_out, 8) for d in dim_ins])


class ResnetBlock(_Decl):
    def __init__(self, dim, dim_out, *, cond_dim=None, time_cond_dim=None, groups=8, use_gca=False, heads=8,
                 dim_head=64, linear_attn=False):
        super().__init__()
        if exists(time_cond_dim):
            self.time_mlp = nn.Sequential(_Stateless(), nn.Linear(time_cond_dim, dim_out * 2))
        if exists(cond_dim):
            klass = LinearCrossAttention if linear_attn else CrossAttention
            self.cross_attn = klass(dim_out, context_dim=cond_dim, dim_head=dim_head, heads=heads)
        self.block1 = Block(dim, dim_out, groups)
        self.block2 = Block(dim_out, dim_out, groups)
        if use_gca:
            self.gca = GlobalContext(dim_in=dim_out, dim_out=dim_out)
        if dim != dim_out:
            self.res_conv = nn.Conv2d(dim, dim_out, 1)


def _invalidate_engine_hook(module, incompatible_keys):  # module-level: a pickled / deep-copied Unet keeps it
    module.invalidate_engine()


# ============================================================================ Unet
class Unet(nn.Module):
    """Same constructor surface as ``imagen_pytorch.Unet`` for every kwarg the reference passes;
    library defaults elsewhere.  Unsupported library switches raise early."""

    def __init__(
        self, *, dim, text_embed_dim=768, num_resnet_blocks=1, cond_dim=None, num_time_tokens=2,
        learned_sinu_pos_emb_dim=16, dim_mults=(1, 2, 4, 8), cond_images_channels=0, channels=3,
        channels_out=None, attn_dim_head=64, attn_heads=8, ff_mult=2.0, lowres_cond=False, layer_attns=True,
        layer_attns_depth=1, attend_at_middle=True, layer_cross_attns=True, use_linear_attn=False,
        use_linear_cross_attn=False, cond_on_text=True, max_text_len=256, resnet_groups=8,
        init_conv_kernel_size=7, init_cross_embed=True, init_cross_embed_kernel_sizes=(3, 7, 15),
        cross_embed_downsample=False, cross_embed_downsample_kernel_sizes=(2, 4),
        attn_pool_text=True, attn_pool_num_latents=32, dropout=0.0, memory_efficient=False,
        init_conv_to_final_conv_residual=False, use_global_context_attn=True, scale_skip_connection=True,
        final_resnet_block=True, final_conv_kernel_size=3, self_cond=False, pixel_shuffle_upsample=True,
        cosine_sim_attn=False, attn_qk_norm=None, downsample_form="unshuffle", mid_attn_form="transformer",
        combine_upsample_fmaps=False,
    ):
        """`downsample_form` / `mid_attn_form` (engine extensions) name the two structural forks between library
        versions - "unshuffle" | "conv4x4" and "transformer" | "residual_attention"; load_state_dict() selects them
        from the incoming keys and shapes, as it does for the attention similarity.
        `cosine_sim_attn` is the library's kwarg (1.18.x: l2-normalised q, k with a fixed scale of 16).
        `attn_qk_norm` (engine extension, 0 / 1 / 2, see include/kd_engine.h) overrides it; 2 = the learned
        q_scale / k_scale attention of later library versions, which load_state_dict() also selects by itself
        when the incoming keys contain `q_scale` - so the first real checkpoint decides the variant."""
        super().__init__()
        self._locals = {k: v for k, v in locals().items() if k not in ("self", "__class__")}
        if tuple(cross_embed_downsample_kernel_sizes) != (2, 4):
            raise NotImplementedError("cross_embed_downsample_kernel_sizes: the engine plans the library's default (2, 4) only")
        if channels not in (1, 2, 3, 4):
            raise NotImplementedError(
                f"Unet option outside what the reference's configs use and the HIP engine plans: channels={channels}")
        # the structural switches of the first and the last layer: every value the engine cannot plan is refused here by name
        init_cross_embed, final_resnet_block = bool(init_cross_embed), bool(final_resnet_block)
        scale_skip_connection = bool(scale_skip_connection)
        odd_to_15 = lambda k: isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= 15 and k % 2 == 1
        if not init_cross_embed and not odd_to_15(init_conv_kernel_size):
            raise NotImplementedError(f"init_conv_kernel_size={init_conv_kernel_size}: the engine plans odd sizes from 1 to 15")
        init_cross_embed_kernel_sizes = tuple(init_cross_embed_kernel_sizes)
        if init_cross_embed:
            ks = init_cross_embed_kernel_sizes
            if not 1 <= len(ks) <= 4 or not all(odd_to_15(k) for k in ks):
                raise NotImplementedError(f"init_cross_embed_kernel_sizes={ks}: the engine plans one to four odd sizes "
                                          "from 1 to 15")
            # the library's widths: dim / 2, dim / 4, .., the rest; every conv writes a slice of the NHWC map in 16-byte steps
            widths = [int(dim / 2 ** (i + 1)) for i in range(len(ks) - 1)]
            widths.append(dim - sum(widths))
            if any(w < 4 or w % 4 for w in widths):
                raise NotImplementedError(f"init_cross_embed_kernel_sizes={ks} with dim={dim}: the width split {widths} "
                                          "has a conv of a width that is no multiple of 4")
        if final_conv_kernel_size not in (1, 3, 5, 7) or isinstance(final_conv_kernel_size, bool):
            raise NotImplementedError(f"final_conv_kernel_size={final_conv_kernel_size}: the engine plans 1, 3, 5 and 7")
        if attn_dim_head not in (32, 64, 128):
            raise NotImplementedError(f"attn_dim_head={attn_dim_head}: the attention kernels are built for 32, 64 and 128")
        if channels != 3 and channels_out is not None and channels_out != channels:
            raise NotImplementedError("channels_out must equal channels: the engine's final conv writes the image's channels")
        # scalar options the engine cannot plan: refused here, not by a launcher's precondition at the first forward
        if cond_on_text and not attn_pool_text:
            raise NotImplementedError("attn_pool_text=False with cond_on_text=True: the engine plans the text tokens through the "
                                      "PerceiverResampler only (pass cond_on_text=False for a UNet without text conditioning)")
        if cond_on_text and attn_pool_text and max_text_len > 512:
            raise NotImplementedError(f"max_text_len={max_text_len}: the PerceiverResampler's position table holds 512 rows")
        if learned_sinu_pos_emb_dim < 2 or learned_sinu_pos_emb_dim % 2:
            raise NotImplementedError(f"learned_sinu_pos_emb_dim={learned_sinu_pos_emb_dim} must be even "
                                      "(sines and cosines of learned_sinu_pos_emb_dim / 2 frequencies)")
        if not float(ff_mult * 2).is_integer() or ff_mult <= 0:
            raise NotImplementedError(f"ff_mult={ff_mult}: the engine plans feed-forward widths of dim * ff_mult for "
                                      "multiples of 0.5")
        if num_time_tokens < 1 or attn_heads < 1 or attn_pool_num_latents < 1:
            raise NotImplementedError("num_time_tokens, attn_heads and attn_pool_num_latents must be at least 1")
        if dim % 32:
            raise NotImplementedError(f"dim={dim}: the engine plans UNets whose dim is a multiple of 32")

        self.channels = channels
        self.channels_out = default(channels_out, channels)
        self.lowres_cond = lowres_cond
        self.cond_on_text = cond_on_text
        self.cond_images_channels = cond_images_channels
        self.has_cond_image = cond_images_channels > 0
        self.memory_efficient = memory_efficient
        self.init_conv_to_final_conv_residual = init_conv_to_final_conv_residual
        # the library's other resampling layers: a CrossEmbedLayer (kernel sizes 2 and 4, stride 2) in every Downsample slot;
        # nearest x2 + conv3x3 instead of the PixelShuffleUpsample
        self.cross_embed_downsample = bool(cross_embed_downsample)
        self.pixel_shuffle_upsample = bool(pixel_shuffle_upsample)
        # the library's UpsampleCombiner: every up level's map goes through a Block of its own at full resolution into the
        # concat in front of final_res_block
        self.combine_upsample_fmaps = bool(combine_upsample_fmaps)
        self.max_text_len = max_text_len
        self.dim = dim
        # self_cond: every forward also reads the previous step's thresholded x0 estimate (zeros when not given); the
        # library's input order is cat(cond_images, x, self_cond, lowres_cond_img)
        self.self_cond = bool(self_cond)
        init_channels = channels * (1 + int(lowres_cond) + int(self.self_cond)) + cond_images_channels

        # init_cross_embed=False: the library's plain Conv2d(init_channels, dim, init_conv_kernel_size), keys init_conv.{weight,bias}
        self.init_conv = CrossEmbedLayer(init_channels, init_cross_embed_kernel_sizes, dim, stride=1) if init_cross_embed \
            else nn.Conv2d(init_channels, dim, init_conv_kernel_size, padding=init_conv_kernel_size // 2)
        dims = [dim, *[dim * m for m in dim_mults]]
        in_out = list(zip(dims[:-1], dims[1:]))
        L = len(in_out)
        cond_dim = default(cond_dim, dim)
        tcd = dim * 4 * (2 if lowres_cond else 1)
        self.cond_dim, self.time_cond_dim = cond_dim, tcd
        sw = learned_sinu_pos_emb_dim + 1

        def trio():
            return (nn.Sequential(LearnedSinusoidalPosEmb(learned_sinu_pos_emb_dim), nn.Linear(sw, tcd), _Stateless()),
                    nn.Sequential(nn.Linear(tcd, tcd)),
                    nn.Sequential(nn.Linear(tcd, cond_dim * num_time_tokens), _Stateless()))

        self.to_time_hiddens, self.to_time_cond, self.to_time_tokens = trio()
        if lowres_cond:
            self.to_lowres_time_hiddens, self.to_lowres_time_cond, self.to_lowres_time_tokens = trio()
        self.norm_cond = nn.LayerNorm(cond_dim)
        self.text_to_cond = None
        if cond_on_text:
            assert exists(text_embed_dim), "text_embed_dim must be given to the unet if cond_on_text is True"
            self.text_to_cond = nn.Linear(text_embed_dim, cond_dim)
        self.attn_pool = PerceiverResampler(dim=cond_dim, depth=2, dim_head=attn_dim_head, heads=attn_heads,
                                            num_latents=attn_pool_num_latents) if attn_pool_text else None
        self.null_text_embed = nn.Parameter(torch.randn(1, max_text_len, cond_dim))
        self.null_text_hidden = nn.Parameter(torch.randn(1, tcd))
        self.to_text_non_attn_cond = None
        if cond_on_text:
            self.to_text_non_attn_cond = nn.Sequential(nn.LayerNorm(cond_dim), nn.Linear(cond_dim, tcd),
                                                       _Stateless(), nn.Linear(tcd, tcd))

        ak = dict(heads=attn_heads, dim_head=attn_dim_head)
        nrb = cast_tuple(num_resnet_blocks, L)
        groups = cast_tuple(resnet_groups, L)
        attns = cast_tuple(layer_attns, L)
        cross = cast_tuple(layer_cross_attns, L)
        # use_linear_attn: a LinearAttentionTransformerBlock at the levels without full attention; use_linear_cross_attn:
        # the level's first ResnetBlocks get cross-attention, in its linear form
        lin = cast_tuple(use_linear_attn, L)
        lcross = cast_tuple(use_linear_cross_attn, L)
        # layer_attns_depth: (attention, feed-forward) pairs of each level's TransformerBlocks
        depths = tuple(int(d) for d in cast_tuple(layer_attns_depth, L))
        assert len(depths) == L and all(d >= 1 for d in depths), "layer_attns_depth: one depth >= 1 per level"
        if (any(lin) or any(lcross)) and attn_dim_head != 64:
            raise NotImplementedError("use_linear_attn / use_linear_cross_attn with attn_dim_head != 64: "
                                      "the linear-attention kernels are built for dim_head 64")
        if any(ll and not la and d != 1 for ll, la, d in zip(lin, attns, depths)):
            raise NotImplementedError("layer_attns_depth > 1 on a linear-attention level (use_linear_attn) is not planned: "
                                      "the engine's LinearAttentionTransformerBlock has depth 1")
        assert len(set(groups)) == 1, "per-level resnet_groups are not planned by the engine"
        # every GroupNorm of the plan is a ResnetBlock's block1 (over the block's input) or block2 (over its output), and the
        # statistics pass reads whole groups in 16-byte steps: each such width must be a multiple of 4 * resnet_groups.
        # (The UpsampleCombiner's Blocks have 8 groups of their own: dims[l] / 8 is a multiple of 4 since dim % 32 == 0.)
        gn_widths = {dims[-1]}                                    # mid_block1 / mid_block2
        if memory_efficient:
            gn_widths.add(dim)                                    # init_resnet_block
        for d_in, d_out in in_out:
            cur = d_out if memory_efficient else d_in
            gn_widths |= {cur, d_out, d_out + cur}                # the level's down blocks; its up blocks behind the skip concat
        if final_resnet_block:                                    # (without it no GroupNorm reads the concat in front of final_conv)
            gn_widths |= {dim, dim * (1 + int(bool(init_conv_to_final_conv_residual)) + (L if combine_upsample_fmaps else 0))}
        self._gn_widths = sorted(gn_widths)
        bad_w = sorted(w for w in gn_widths if groups[0] < 1 or w % (4 * groups[0]))
        if bad_w:
            raise NotImplementedError(f"resnet_groups={groups[0]}: the GroupNorm over {bad_w[0]} channels would have groups of "
                                      f"{bad_w[0] / max(groups[0], 1):g} channels, the engine plans multiples of 4 "
                                      f"(ResnetBlock widths of this UNet: {sorted(gn_widths)})")
        self._plan = dict(dim=dim, dim_mults=tuple(dim_mults), num_resnet_blocks=nrb, layer_attns=attns,
                          layer_cross_attns=cross, use_linear_attn=lin, use_linear_cross_attn=lcross,
                          attn_heads=attn_heads, attn_dim_head=attn_dim_head, layer_attns_depth=depths,
                          ff_mult=ff_mult, num_time_tokens=num_time_tokens, sinu_dim=learned_sinu_pos_emb_dim,
                          groups=groups[0], attend_at_middle=attend_at_middle, use_gca=use_global_context_attn,
                          cross_embed_downsample=self.cross_embed_downsample,
                          upsample_nearest=not self.pixel_shuffle_upsample,
                          combine_upsample_fmaps=self.combine_upsample_fmaps,
                          init_cross_embed=init_cross_embed, init_conv_kernel_size=init_conv_kernel_size,
                          init_cross_embed_kernel_sizes=tuple(sorted(init_cross_embed_kernel_sizes)),
                          final_conv_kernel_size=final_conv_kernel_size, final_resnet_block=final_resnet_block,
                          scale_skip_connection=scale_skip_connection)

        self.init_resnet_block = ResnetBlock(dim, dim, time_cond_dim=tcd, groups=groups[0],
                                             use_gca=use_global_context_attn, **ak) if memory_efficient else None
        self.downs = nn.ModuleList([])
        self.ups = nn.ModuleList([])
        skip_dims = []

        def attn_block(d, la, ll, depth):   # full attention wins over linear attention
            if la:
                return TransformerBlock(d, depth=depth, ff_mult=ff_mult, context_dim=cond_dim, **ak)
            if ll:
                return LinearAttentionTransformerBlock(d, depth=1, ff_mult=ff_mult, context_dim=cond_dim, **ak)
            return _Stateless()

        def down(d, d_out):
            if self.cross_embed_downsample:
                return CrossEmbedLayer(d, cross_embed_downsample_kernel_sizes, d_out, stride=2)
            return _downsample(d, d_out, downsample_form)

        def up(d, d_out):
            if self.pixel_shuffle_upsample:
                return PixelShuffleUpsample(d, d_out)
            return nn.Sequential(_Stateless(), nn.Conv2d(d, d_out, 3, padding=1))   # nn.Upsample(2, nearest), conv

        for ind, ((d_in, d_out), n, g, la, lc, ll, lx, dep) in enumerate(zip(in_out, nrb, groups, attns, cross, lin, lcross,
                                                                            depths)):
            is_last = ind >= L - 1
            cur = d_in
            pre = None
            if memory_efficient:
                pre = down(d_in, d_out)
                cur = d_out
            skip_dims.append(cur)
            post = None
            if not memory_efficient:
                post = down(cur, d_out) if not is_last else Parallel(
                    nn.Conv2d(d_in, d_out, 3, padding=1), nn.Conv2d(d_in, d_out, 1))
            self.downs.append(nn.ModuleList([
                pre,
                ResnetBlock(cur, cur, cond_dim=cond_dim if lc or lx else None, time_cond_dim=tcd, groups=g,
                            linear_attn=bool(lx), **ak),
                nn.ModuleList([ResnetBlock(cur, cur, time_cond_dim=tcd, groups=g, use_gca=use_global_context_attn)
                               for _ in range(n)]),
                attn_block(cur, la, ll, dep),
                post,
            ]))
        mid = dims[-1]
        # (the library builds the two middle ResnetBlocks without the attention kwargs: their cross-attention has its own
        # defaults, 8 heads of 64, whatever attn_heads / attn_dim_head say)
        self.mid_block1 = ResnetBlock(mid, mid, cond_dim=cond_dim, time_cond_dim=tcd, groups=groups[-1])
        assert downsample_form in ("unshuffle", "conv4x4") and mid_attn_form in ("transformer", "residual_attention")
        self.downsample_form, self.mid_attn_form = downsample_form, mid_attn_form
        self._dims = dims
        self.mid_attn = None
        if attend_at_middle:
            self.mid_attn = TransformerBlock(mid, depth=1, ff_mult=2, **ak) if mid_attn_form == "transformer" \
                else ResidualAttentionBlock(mid, **ak)
        self.mid_block2 = ResnetBlock(mid, mid, cond_dim=cond_dim, time_cond_dim=tcd, groups=groups[-1])
        for ind, ((d_in, d_out), n, g, la, lc, ll, lx, dep) in enumerate(
                zip(reversed(in_out), reversed(nrb), reversed(groups), reversed(attns), reversed(cross), reversed(lin),
                    reversed(lcross), reversed(depths))):
            is_last = ind == L - 1
            sd = skip_dims.pop()
            self.ups.append(nn.ModuleList([
                ResnetBlock(d_out + sd, d_out, cond_dim=cond_dim if lc or lx else None, time_cond_dim=tcd, groups=g,
                            linear_attn=bool(lx), **ak),
                nn.ModuleList([ResnetBlock(d_out + sd, d_out, time_cond_dim=tcd, groups=g,
                                           use_gca=use_global_context_attn) for _ in range(n)]),
                attn_block(d_out, la, ll, dep),
                up(d_out, d_in) if (not is_last or memory_efficient) else _Stateless(),
            ]))
        fin = dim + (dim if init_conv_to_final_conv_residual else 0)
        if self.combine_upsample_fmaps:   # Block's own default of 8 groups, not resnet_groups; up level i works at dims[L - i]
            self.upsample_combiner = UpsampleCombiner(tuple(dims[L - i] for i in range(L)), dim)
            fin += dim * L
        # final_resnet_block=False: no final_res_block, final_conv reads the concat itself
        self.final_res_block = ResnetBlock(fin, dim, time_cond_dim=tcd, groups=groups[0], use_gca=True) \
            if final_resnet_block else None
        self.final_conv = nn.Conv2d((dim if final_resnet_block else fin) + (channels if lowres_cond else 0), self.channels_out,
                                    final_conv_kernel_size, padding=final_conv_kernel_size // 2)
        nn.init.zeros_(self.final_conv.weight)
        nn.init.zeros_(self.final_conv.bias)

        self._engines = {}
        self._engines_fingerprint = None
        self._io_buffers = {}  # per (batch, size, device): sampler inputs at stable addresses (step graph reuse)
        self.attn_qk_norm = 0
        # what the CONSTRUCTOR asked for: the variant a checkpoint without q_scale / k_scale falls back to
        self._ctor_qk_norm = int(attn_qk_norm) if exists(attn_qk_norm) else (1 if cosine_sim_attn else 0)
        self._ctor_qk_explicit = exists(attn_qk_norm)
        self.set_attn_qk_norm(self._ctor_qk_norm)
        self.register_load_state_dict_post_hook(_invalidate_engine_hook)

    def set_attn_qk_norm(self, mode: int):
        assert mode in (0, 1, 2), "attn_qk_norm: 0 scaled dot product, 1 cosine-sim, 2 learned q/k scales"
        if getattr(self, "_engines", None):
            self.invalidate_engine()
        self.attn_qk_norm = mode   # the LIVE mode; _locals keeps what the constructor was asked for (clones: cast_model_parameters)
        for m in self.modules():
            if isinstance(m, _QKNorm):
                m.set_qk_norm(mode)

    def set_version_forks(self, downsample_form=None, mid_attn_form=None):
        """Rebuilds the parameter containers of the two structural version forks in place (fresh parameters, same
        device / dtype) and drops the execution plans.  The replaced modules get NEW Parameter objects: an optimizer
        or EMA copy built before the switch (e.g. before a load_state_dict that triggers it) keeps the old ones -
        build those after loading, as ImagenTrainer.load does."""
        ref = self.final_conv.weight
        changed = False
        # (a Unet built with cross_embed_downsample=True has no such fork: its Downsample slots hold CrossEmbedLayers)
        if downsample_form is not None and downsample_form != self.downsample_form and not self.cross_embed_downsample:
            for l, lvl in enumerate(self.downs):
                for slot in (0, 4):
                    if isinstance(lvl[slot], (nn.Sequential, nn.Conv2d)):   # (not the last level's Parallel, not None)
                        lvl[slot] = _downsample(self._dims[l], self._dims[l + 1], downsample_form).to(ref)
            self.downsample_form = self._locals["downsample_form"] = downsample_form
            changed = True
        if mid_attn_form is not None and mid_attn_form != self.mid_attn_form and exists(self.mid_attn):
            ak = dict(heads=self._plan["attn_heads"], dim_head=self._plan["attn_dim_head"])
            self.mid_attn = (TransformerBlock(self._dims[-1], depth=1, ff_mult=2, **ak) if mid_attn_form == "transformer"
                             else ResidualAttentionBlock(self._dims[-1], **ak)).to(ref)
            self.mid_attn_form = self._locals["mid_attn_form"] = mid_attn_form
            self.set_attn_qk_norm(self.attn_qk_norm)
            changed = True
        if changed and getattr(self, "_engines", None):
            self.invalidate_engine()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, *args, **kwargs):
        # Runs before the children load.  The library's module tree forked between versions (SURVEY A.1 "version
        # forks"); the incoming key set / shapes name the fork, and the tree (and so the engine's plan) follows it, so
        # that a checkpoint of a neighbouring version loads STRICTLY instead of falling into restore_parts half-loaded:
        #   * Downsample: `downs.L.{0,4}.weight` [d_out, d, 4, 4] (strided conv) vs `downs.L.{0,4}.1.weight` (unshuffle + 1x1)
        #   * mid_attn:   `mid_attn.fn.fn.*` (residual attention) vs `mid_attn.layers.*` (TransformerBlock)
        #   * attention similarity: `*.q_scale` / `*.k_scale` present (learned qk-norm) or not
        if any(k.startswith(prefix + "downs.") for k in state_dict):
            conv4 = any(re.fullmatch(re.escape(prefix) + r"downs\.\d+\.[04]\.weight", k) and v.dim() == 4 and v.shape[-1] == 4
                        for k, v in state_dict.items())
            plain = any(k.startswith(prefix + "mid_attn.fn.") for k in state_dict)
            want = ("conv4x4" if conv4 else "unshuffle", "residual_attention" if plain else "transformer")
            if self.cross_embed_downsample:   # `downs.L.{0,4}.convs.K.*`: neither form of the fork, nothing to follow
                want = (self.downsample_form, want[1])
            if want != (self.downsample_form, self.mid_attn_form):
                print(f"imagen_pytorch: checkpoint keys name the library fork downsample={want[0]}, mid_attn={want[1]} "
                      "-> module tree and engine plan follow it")
                self.set_version_forks(*want)
        has = any(k.startswith(prefix) and k.endswith(".q_scale") for k in state_dict)
        if has and self.attn_qk_norm != 2:
            print("imagen_pytorch: checkpoint carries q_scale / k_scale -> attention variant switched to qk-norm "
                  "(learned scales, x8)")
            self.set_attn_qk_norm(2)
        elif not has and self.attn_qk_norm == 2 and any(k.startswith(prefix) for k in state_dict) \
                and not (self._ctor_qk_explicit and self._ctor_qk_norm == 2):
            # (a Unet BUILT with attn_qk_norm=2 keeps it: torch then reports the missing q_scale / k_scale keys - an
            # error under strict=True, defaults of one under strict=False)
            back = self._ctor_qk_norm if self._ctor_qk_norm != 2 else 0   # cosine_sim_attn=True stays cosine-sim
            print("imagen_pytorch: checkpoint has no q_scale / k_scale -> attention variant back to "
                  + ("cosine-sim (x16)" if back == 1 else "the scaled dot product"))
            self.set_attn_qk_norm(back)
        return super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, *args, **kwargs)

    # ---- library API used by Imagen
    def cast_model_parameters(self, *, lowres_cond, text_embed_dim, channels, channels_out, cond_on_text):
        if (lowres_cond == self.lowres_cond and channels == self.channels and cond_on_text == self.cond_on_text
                and text_embed_dim == self._locals["text_embed_dim"] and channels_out == self.channels_out):
            return self
        clone = self.__class__(**{**self._locals, **dict(
            lowres_cond=lowres_cond, text_embed_dim=text_embed_dim, channels=channels, channels_out=channels_out,
            cond_on_text=cond_on_text)})
        # a mode a checkpoint switched on travels to the clone as a live mode, not as a constructor request: the clone
        # still follows the next checkpoint's keys (with or without q_scale / k_scale) the way the original would
        if clone.attn_qk_norm != self.attn_qk_norm:
            clone.set_attn_qk_norm(self.attn_qk_norm)
        return clone

    # ---- engine plumbing
    def invalidate_engine(self):
        """Drops every execution plan (and the packed-weight store they share).  Called automatically by
        load_state_dict, .to()/.cuda()/.float() and whenever a parameter was changed in place since the
        plans were built (see `_weights_fingerprint`)."""
        lib = E._lib
        for h in self._engines.values():
            if lib is not None:
                lib.kd_unet_destroy(h)
        self._engines = {}
        self._io_buffers = {}
        self._engines_fingerprint = None

    def _weights_fingerprint(self):
        """(storage address, in-place version counter) of every parameter / buffer: the engine keeps PACKED
        COPIES of the weights, so restore_parts() on a live state_dict, `p.copy_()` / `p.add_()` under no_grad
        or an optimizer step must rebuild them.  torch bumps `_version` on every in-place write through the
        parameter or a `detach()`ed alias (what state_dict() hands out).  Writes through `p.data` carry their
        own version counter and are invisible here: after those, call `invalidate_engine()` yourself."""
        import itertools

        # (parameters() / buffers() walk the live module tree - a replaced Parameter object is seen - without building the
        # state_dict's OrderedDict and running its hooks: this runs on every sample() call, once per patch and stage)
        return tuple((t.data_ptr(), t._version) for t in itertools.chain(self.parameters(), self.buffers()))

    def __deepcopy__(self, memo):
        """copy.deepcopy(unet) - ImagenTrainer's EMA copies (trainer.py), the reference builds the trainer around
        a live Imagen (sample_uncond.py:22-23): the copy gets the parameters, never the engine handles (ctypes
        pointers cannot be copied, and two owners would destroy one plan twice) nor the I/O staging buffers."""
        import copy

        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k in ("_engines", "_io_buffers", "_engines_fingerprint"):
                continue
            new.__dict__[k] = copy.deepcopy(v, memo)
        new._engines, new._io_buffers, new._engines_fingerprint = {}, {}, None
        # the load_state_dict post hook registered in __init__ was deep-copied with the hooks dict and still
        # refers to its `module` argument (not to `self`): it stays valid for the copy
        return new

    def __getstate__(self):  # pickling (torch.save of a module): same rule
        d = dict(self.__dict__)
        d["_engines"], d["_io_buffers"], d["_engines_fingerprint"] = {}, {}, None
        return d

    def _apply(self, fn, *a, **k):  # .to()/.cuda()/.float(): packed copies are stale iff a parameter really moved
        before = self._weights_fingerprint() if self._engines else None
        out = super()._apply(fn, *a, **k)
        if before is not None and before != self._weights_fingerprint():
            self.invalidate_engine()
        return out

    def __del__(self):
        try:
            self.invalidate_engine()
        except Exception:
            pass

    @property
    def n_text_tokens(self):
        return self.attn_pool.num_tokens if (self.cond_on_text and exists(self.attn_pool)) else 0

    def engine(self, batch: int, image_size: int, device, with_text: bool, replica: int = 0) -> C.c_void_p:
        """Creates (or returns the cached) execution plan for a static (batch, image_size).  `replica` > 0 gives
        further plans of the same shape with their own workspace (plans on different streams run concurrently;
        all plans of a UNet share one packed-weight store)."""
        E.require_gpu()
        lib = E.load()
        device = torch.device(device)
        # engine extension (not a library kwarg): 0 = auto (Winograd for the deep 3x3 convs), 1 = direct only
        conv_algo = int(getattr(self, "conv_algo", os.environ.get("KD_CONV_ALGO", "0")))
        slice_mb = int(getattr(self, "wino_slice_mb", 0))   # engine extension: workspace cap of the batched Winograd layers
        w43 = int(getattr(self, "wino43_min_cin", 0))       # engine extension: F(4x4,3x3) threshold (0 = default, < 0 = never)
        x3 = int(getattr(self, "gemm_bf16x3", 0))           # engine extension: bf16x3 position GEMMs (0 = default on, < 0 = fp32 MFMA)
        x3lin = int(getattr(self, "x3_linear", 0))          # engine extension: token GEMMs / 1x1 convs on bf16x3 (0 = default: K >= 512, < 0 = never)
        w4img = int(getattr(self, "wino4_max_images", 0))   # engine extension: F(4x4,3x3) layers in sets of at most n images (0 = default)
        init_generic = int(bool(getattr(self, "init_conv_generic", 0)))   # engine extension (A/B): init conv on the generic conv path
        key = (batch, image_size, device.index, bool(with_text), conv_algo, self.attn_qk_norm, slice_mb, w43, x3, x3lin, w4img) + \
            ((("init_generic",),) if init_generic else ()) + \
            ((replica,) if replica else ())   # (the structural forks drop every plan when they change)
        if self._engines:
            fp = self._weights_fingerprint()
            if fp != self._engines_fingerprint:   # a parameter was written in place: packed copies are stale
                self.invalidate_engine()
        if key in self._engines:
            return self._engines[key]
        p = self._plan
        cfg = E.kd_unet_config_t()
        L = len(p["dim_mults"])
        assert L <= E.KD_MAX_LEVELS
        cfg.dim, cfg.num_levels = p["dim"], L
        for i in range(L):
            cfg.dim_mults[i] = int(p["dim_mults"][i])
            cfg.num_resnet_blocks[i] = int(p["num_resnet_blocks"][i])
            cfg.layer_attns[i] = int(bool(p["layer_attns"][i]))
            cfg.layer_cross_attns[i] = int(bool(p["layer_cross_attns"][i]))
        cfg.cond_dim, cfg.channels = self.cond_dim, self.channels
        cfg.cond_images_channels = self.cond_images_channels
        cfg.lowres_cond = int(self.lowres_cond)
        cfg.memory_efficient = int(self.memory_efficient)
        cfg.init_conv_to_final_conv_residual = int(self.init_conv_to_final_conv_residual)
        cfg.cond_on_text = int(self.cond_on_text)
        cfg.text_tokens = self.n_text_tokens if with_text else 0
        cfg.attn_heads, cfg.attn_dim_head = p["attn_heads"], p["attn_dim_head"]
        ff2 = p["ff_mult"] * 2
        assert float(ff2).is_integer(), "ff_mult must be a multiple of 0.5"
        cfg.ff_mult_x2 = int(ff2)
        cfg.num_time_tokens, cfg.sinu_dim = p["num_time_tokens"], p["sinu_dim"]
        cfg.resnet_groups = p["groups"]
        cfg.attend_at_middle, cfg.use_gca = int(p["attend_at_middle"]), int(p["use_gca"])
        cfg.batch, cfg.image_size = batch, image_size
        cfg.conv_algo = conv_algo
        cfg.attn_qk_norm = self.attn_qk_norm
        cfg.wino_slice_mb = slice_mb
        cfg.wino43_min_cin = w43
        cfg.gemm_bf16x3 = x3
        cfg.x3_linear = x3lin
        cfg.wino4_max_images = w4img
        cfg.downsample_conv4 = int(self.downsample_form == "conv4x4")
        cfg.mid_attn_plain = int(self.mid_attn_form == "residual_attention")

        with torch.cuda.device(device):
            sd = {k: v.detach().to(device=device, dtype=torch.float32).contiguous()
                  for k, v in self.state_dict().items()}
            torch.cuda.synchronize()
            names = list(sd.keys())
            arr = (E.kd_param_t * len(names))()
            keep = []
            for i, n in enumerate(names):
                b = n.encode()
                keep.append(b)
                arr[i].name = b
                arr[i].d_data = sd[n].data_ptr()
                arr[i].numel = sd[n].numel()
            handle = C.c_void_p()
            # further plans of this UNet on the same device (other batch / image size) share its packed weights
            share = next((h for k, h in self._engines.items() if k[2] == device.index), None)
            ext = E.kd_unet_ext_t()
            ext.self_cond = int(self.self_cond)
            for i in range(L):
                ext.use_linear_attn[i] = int(bool(p["use_linear_attn"][i]))
                ext.use_linear_cross_attn[i] = int(bool(p["use_linear_cross_attn"][i]))
            ext.cross_embed_downsample = int(p["cross_embed_downsample"])
            ext.upsample_nearest = int(p["upsample_nearest"])
            ext2 = E.kd_unet_ext2_t()
            ext2.combine_upsample_fmaps = int(p["combine_upsample_fmaps"])
            ext4 = E.kd_unet_ext4_t()
            ext4.init_plain = int(not p["init_cross_embed"])
            ext4.init_kernel_size = int(p["init_conv_kernel_size"]) if ext4.init_plain else 0
            if p["init_cross_embed"] and p["init_cross_embed_kernel_sizes"] != (3, 7, 15):
                ext4.n_init_kernel_sizes = len(p["init_cross_embed_kernel_sizes"])
                for i, k in enumerate(p["init_cross_embed_kernel_sizes"]):
                    ext4.init_kernel_sizes[i] = int(k)
            ext4.final_kernel_size = 0 if p["final_conv_kernel_size"] == 3 else int(p["final_conv_kernel_size"])
            ext4.no_final_resnet_block = int(not p["final_resnet_block"])
            ext4.no_skip_scale = int(not p["scale_skip_connection"])
            ext4.init_generic = init_generic
            if any(bytes(ext4)):   # one of the first / last layer's structural switches
                ext3 = E.kd_unet_ext3_t()
                for i in range(L):
                    ext3.layer_attns_depth[i] = int(p["layer_attns_depth"][i])
                E.check(lib.kd_unet_create_ext4(C.byref(cfg), arr, len(names), share, C.byref(ext), C.byref(ext2), C.byref(ext3),
                                                C.byref(ext4), C.byref(handle)))
            elif any(d != 1 for d in p["layer_attns_depth"]):
                ext3 = E.kd_unet_ext3_t()
                for i in range(L):
                    ext3.layer_attns_depth[i] = int(p["layer_attns_depth"][i])
                E.check(lib.kd_unet_create_ext3(C.byref(cfg), arr, len(names), share, C.byref(ext), C.byref(ext2), C.byref(ext3),
                                                C.byref(handle)))
            else:   # depth 1 everywhere: the entry of before (kd_unet_create_ext3 with ext3 = NULL)
                E.check(lib.kd_unet_create_ext2(C.byref(cfg), arr, len(names), share, C.byref(ext), C.byref(ext2), C.byref(handle)))
            del sd
        self._engines[key] = handle
        self._engines_fingerprint = self._weights_fingerprint()
        return handle

    def forward(self, x, time, *, lowres_cond_img=None, lowres_noise_times=None, text_embeds=None, text_mask=None,
                cond_images=None, self_cond=None, cond_drop_prob=0.0):
        """One UNet forward on the engine.  ``time`` is the log-SNR, as in the library.  ``self_cond`` [B,C,S,S]
        (None = zeros) is read by a UNet built with self_cond=True and ignored by any other, as in the library."""
        assert not (self.lowres_cond and not exists(lowres_cond_img)), "low resolution conditioning image must be present"
        assert not (self.lowres_cond and not exists(lowres_noise_times)), "low resolution conditioning noise time must be present"
        assert not (self.has_cond_image ^ exists(cond_images)), \
            "you either requested to condition on an image on the unet, but the conditioning image is not supplied, or vice versa"
        E.require_gpu()
        b, c, s, _ = x.shape
        assert c == self.channels, f"x has {c} channels, the UNet was built with channels={self.channels}"
        f32 = lambda t: None if t is None else t.to(device=x.device, dtype=torch.float32).contiguous()
        if exists(cond_images):
            assert cond_images.shape[1] == self.cond_images_channels, "invalid number of channels in conditioning image"
            cond_images = resize_image_to(cond_images, s)
        self_cond = f32(self_cond) if self.self_cond else None
        if exists(self_cond):
            assert self_cond.shape == x.shape, "self_cond must have the shape of x"
        x, lowres_cond_img, cond_images = f32(x), f32(lowres_cond_img), f32(cond_images)
        time, lowres_noise_times = f32(time), f32(lowres_noise_times)
        out = torch.empty_like(x)
        with_text = exists(text_embeds) and self.cond_on_text
        assert cond_drop_prob in (0.0, 1.0), "sampling uses keep-all (0) or drop-all (1) conditioning only"
        with torch.cuda.device(x.device):
            h = self.engine(b, s, x.device, with_text=with_text)
            tok = hid = None
            if with_text:
                tok, hid = self.text_cond(h, text_embeds, text_mask, drop=cond_drop_prob == 1.0, device=x.device)
            E.check(E.load().kd_unet_forward_self_cond(h, E.ptr(x), E.ptr(self_cond), E.ptr(lowres_cond_img),
                                                       E.ptr(cond_images), E.ptr(time), E.ptr(lowres_noise_times),
                                                       E.ptr(tok), E.ptr(hid), E.ptr(out), E.current_stream()))
        return out

    def text_cond(self, handle, text_embeds, text_mask, drop, device):
        """(text_tokens [B,n,cond_dim], text_hiddens [B,time_cond_dim]) on the engine — the
        step-invariant text branch of the library's Unet.forward, computed once per sample call."""
        f32 = lambda t: t.to(device=device, dtype=torch.float32).contiguous()
        text_embeds = f32(text_embeds)[:, : self.max_text_len].contiguous()
        b, L, _ = text_embeds.shape
        # text_mask = None: no mask reaches the engine, which then keeps the library's zero padding of the rows L .. max_text_len
        # (a mask of ones would select null_text_embed there)
        mask = None if text_mask is None else f32(text_mask)[:, : self.max_text_len].contiguous()
        # named tensors: they must outlive the asynchronous launches below
        tok = torch.empty(b, self.n_text_tokens, self.cond_dim, device=device)
        hid = torch.empty(b, self.time_cond_dim, device=device)
        E.check(E.load().kd_unet_text_cond(handle, E.ptr(text_embeds), E.ptr(mask), L, int(bool(drop)), E.ptr(tok),
                                           E.ptr(hid), E.current_stream()))
        # no host synchronisation: the launches are on torch's current stream, and torch's caching allocator
        # hands the memory of text_embeds / mask to later allocations of the SAME stream only (stream-ordered reuse)
        return tok, hid

    def forward_with_cond_scale(self, *args, cond_scale=1.0, **kwargs):
        """Library method: one forward at cond_scale == 1, else a second forward with the
        conditioning dropped and null + (cond - null) * cond_scale (sample.py:55-59 reaches it through
        trainer.sample(cond_scale=...)).  Both forwards and the combine run on the engine."""
        logits = self.forward(*args, **kwargs)
        if cond_scale == 1:
            return logits
        null_logits = self.forward(*args, **{**kwargs, "cond_drop_prob": 1.0})
        with torch.cuda.device(logits.device):
            E.check(E.load().kd_cfg_combine(E.ptr(logits), E.ptr(null_logits), E.ptr(logits), float(cond_scale),
                                            logits.numel(), E.current_stream()))
        return logits


class NullUnet(nn.Module):
    """Placeholder; the reference subclasses it (train_ultra_res.py:65-75)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.lowres_cond = False
        self.dummy_parameter = nn.Parameter(torch.tensor([0.0]))

    def cast_model_parameters(self, *_, **__):
        return self

    def forward(self, x, *args, **kwargs):
        return x


class SRUnet1024(Unet):
    """Imported by the reference (train_ultra_res.py:8), never instantiated there."""

    def __init__(self, *args, **kwargs):
        d = dict(dim_mults=(1, 2, 4, 8), num_resnet_blocks=(2, 4, 8, 8), layer_attns=False,
                 layer_cross_attns=(False, False, False, True), attn_heads=8, ff_mult=2.0, memory_efficient=True)
        super().__init__(*args, **{**d, **kwargs})


# ============================================================================ schedules (host scalars)
def _log(t, eps=1e-12):
    return torch.log(t.clamp(min=eps))


def beta_linear_log_snr(t):
    return -torch.log(torch.expm1(1e-4 + 10 * (t ** 2)))


def alpha_cosine_log_snr(t, s: float = 0.008):
    return -_log((torch.cos((t + s) / (1 + s) * math.pi * 0.5) ** -2) - 1, eps=1e-5)


def log_snr_to_alpha_sigma(log_snr):
    return torch.sqrt(torch.sigmoid(log_snr)), torch.sqrt(torch.sigmoid(-log_snr))


class GaussianDiffusionContinuousTimes(nn.Module):
    """Per-step scalars, computed on the host in fp32 with the library's op order;
    the per-pixel arithmetic they feed runs in the engine's sampler kernels."""

    def __init__(self, *, noise_schedule, timesteps=1000):
        super().__init__()
        if noise_schedule == "linear":
            self.log_snr = beta_linear_log_snr
        elif noise_schedule == "cosine":
            self.log_snr = alpha_cosine_log_snr
        else:
            raise ValueError(f"invalid noise schedule {noise_schedule}")
        self.noise_schedule = noise_schedule
        self.num_timesteps = timesteps

    def with_timesteps(self, timesteps):
        """The schedule of the same kind on `timesteps` steps (time is continuous: sample(sample_steps=...))."""
        if timesteps == self.num_timesteps:
            return self
        return GaussianDiffusionContinuousTimes(noise_schedule=self.noise_schedule, timesteps=timesteps)

    def step_tables(self):
        ts = torch.linspace(1.0, 0.0, self.num_timesteps + 1)
        t, t_next = ts[:-1], ts[1:]
        ls, ls_next = self.log_snr(t), self.log_snr(t_next)
        alpha, sigma = log_snr_to_alpha_sigma(ls)
        alpha_next, sigma_next = log_snr_to_alpha_sigma(ls_next)
        c = -torch.expm1(ls - ls_next)
        log_var = _log((sigma_next ** 2) * c, eps=1e-20)
        noise_scale = (1 - (t_next == 0).float()) * (0.5 * log_var).exp()
        # q_sample_from_to(t_next -> t): x*(alpha_to/alpha) + n*(sigma_to*alpha - sigma*alpha_to)/alpha
        rn_a = alpha / alpha_next
        rn_b = (sigma * alpha_next - sigma_next * alpha) / alpha_next
        names = ("log_snr", "alpha", "sigma", "alpha_next", "sigma_next", "c", "noise_scale", "rn_a", "rn_b")
        vals = (ls, alpha, sigma, alpha_next, sigma_next, c, noise_scale, rn_a, rn_b)
        return {n: v.to(torch.float32).contiguous() for n, v in zip(names, vals)}


SAMPLERS = ("ddpm", "ddim", "dpmpp_2m", "dpmpp_3m", "dpmpp_2m_sde", "dpmpp_3m_sde")
# the multistep solvers of the exponential-integrator form: name -> (order cap, stochastic)
_MULTISTEP = {"dpmpp_3m": (3, False), "dpmpp_2m_sde": (2, True), "dpmpp_3m_sde": (3, True)}
SOLVER_COEFS = ("coef_x", "coef_x0", "coef_prev", "coef_noise")


def solver_tables(step_tables, sampler, eta=0.0, skip=0):
    """Coefficients of the few-step solvers' update  x <- coef_x x + coef_x0 x0c + coef_prev h1 + coef_prev2 h2 + coef_noise z
    for every step of a schedule (the arrays of kd_solver_schedule_t / kd_solver3_schedule_t; DESIGN.md "Few-step
    solvers"); h1, h2 the thresholded estimates of steps k - 1 and k - 2.  ``step_tables`` are the fp32 entries of
    ``GaussianDiffusionContinuousTimes.step_tables()``; they are evaluated in float64 and rounded to fp32 once.
    With a, s = alpha, sigma at t_k, a', s' those at t_{k+1} and c the table's c:

    ``"ddim"``, 0 <= eta <= 1: d = eta sqrt(s'^2 c) (the ancestral step's posterior deviation, from the table's c),
    A = sqrt(max(s'^2 - d^2, 0)) / s, B = a' - A a, P = 0, S = d; the last step adds no noise (S = 0, its A and B still
    formed with d).  eta = 1 is the ancestral step, eta = 0 is deterministic.

    ``"dpmpp_2m"`` (DPM-Solver++(2M), data prediction): lambda = log_snr / 2, h_k = lambda'_k - lambda_k,
    b_k = -a' expm1(-h_k), A = s' / s, S = 0; first-order steps - the first step walked (k == ``skip``) and the last -
    have B = b, P = 0; every other step w = h_k / (2 h_{k-1}), B = b (1 + w), P = -b w.

    ``"dpmpp_3m"`` (eta = 0), ``"dpmpp_2m_sde"``, ``"dpmpp_3m_sde"`` (0 < eta <= 1): the multistep exponential integrator
    of order up to 3 / 2 / 3 over the same lambda and h_k.  he = h_k (1 + eta), A = (s' / s) exp(-eta h_k),
    b = -a' expm1(-he), phi2 = expm1(-he) / he + 1, phi3 = phi2 / he - 1/2, S = s' sqrt(-expm1(-2 eta h_k)) (0 on the last
    step, whose A and B are still formed with eta).  Step k has order o = min(cap, k - skip + 1, N - k):
    o = 1: B = b, P = Q = 0;  o = 2: r = h_{k-1} / h_k, c = a' phi2 / r, B = b + c, P = -c, Q = 0;
    o = 3: r0 = h_{k-1} / h_k, r1 = h_{k-2} / h_k, g = r0 / (r0 + r1), c1 = a' phi2, c2 = -a' phi3,
    u0 = c1 (1 + g) + c2 / (r0 + r1), u1 = -c1 g - c2 / (r0 + r1), B = b + u0 / r0, P = -u0 / r0 + u1 / r1, Q = -u1 / r1.
    B + P + Q = b at every order.  These three names return a fifth array, ``coef_prev2`` (Q); ``"ddim"`` and
    ``"dpmpp_2m"`` keep their four.

    Pure host arithmetic; needs no GPU."""
    if sampler not in ("ddim", "dpmpp_2m") and sampler not in _MULTISTEP:
        raise ValueError(f"solver_tables: sampler must be 'ddim', 'dpmpp_2m' or one of {tuple(_MULTISTEP)}, got {sampler!r}")
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"solver_tables: eta={eta} is outside [0, 1]")
    stochastic = sampler == "ddim" or _MULTISTEP.get(sampler, (0, False))[1]
    if eta != 0 and not stochastic:
        raise ValueError(f"solver_tables: eta={eta} needs sampler 'ddim', got {sampler!r}")
    if eta == 0 and sampler in _MULTISTEP and stochastic:
        raise ValueError(f"solver_tables: {sampler!r} needs eta > 0; eta = 0 is {sampler[:-4]!r}")
    t = {n: step_tables[n].to(torch.float64) for n in ("log_snr", "alpha", "sigma", "alpha_next", "sigma_next", "c")}
    a, s, an, sn = t["alpha"], t["sigma"], t["alpha_next"], t["sigma_next"]
    N = a.numel()
    if not 0 <= int(skip) < N:
        raise ValueError(f"solver_tables: skip={skip} is outside 0 .. {N - 1}")
    skip = int(skip)
    P = torch.zeros(N, dtype=torch.float64)
    S = torch.zeros(N, dtype=torch.float64)
    if sampler == "ddim":
        d = float(eta) * torch.sqrt(sn ** 2 * t["c"])
        A = torch.sqrt((sn ** 2 - d ** 2).clamp(min=0.0)) / s
        B = an - A * a
        S = d.clone()
        S[N - 1] = 0.0
        return {n: v.to(torch.float32).contiguous() for n, v in zip(SOLVER_COEFS, (A, B, P, S))}
    lam = t["log_snr"] / 2
    # log-SNR at t_{k+1}: the next row's entry; behind the last row the tables hold alpha and sigma alone
    lam_next = torch.cat([lam[1:], torch.log(an[-1:] / sn[-1:])])
    h = lam_next - lam
    if sampler == "dpmpp_2m":
        b = -an * torch.expm1(-h)
        A = sn / s
        B = b.clone()
        for k in range(skip + 1, N - 1):
            w = h[k] / (2 * h[k - 1])
            B[k] = b[k] * (1 + w)
            P[k] = -b[k] * w
        return {n: v.to(torch.float32).contiguous() for n, v in zip(SOLVER_COEFS, (A, B, P, S))}
    cap, eta = _MULTISTEP[sampler][0], float(eta)
    he = h * (1 + eta)
    A = (sn / s) * torch.exp(-eta * h)
    b = -an * torch.expm1(-he)
    phi2 = torch.expm1(-he) / he + 1
    phi3 = phi2 / he - 0.5
    if eta != 0:
        S = sn * torch.sqrt(-torch.expm1(-2 * eta * h))
        S[N - 1] = 0.0
    B, Q = b.clone(), torch.zeros(N, dtype=torch.float64)
    for k in range(skip, N):
        o = min(cap, k - skip + 1, N - k)
        if o == 2:
            c = an[k] * phi2[k] / (h[k - 1] / h[k])
            B[k], P[k] = b[k] + c, -c
        elif o == 3:
            r0, r1 = h[k - 1] / h[k], h[k - 2] / h[k]
            g = r0 / (r0 + r1)
            c1, c2 = an[k] * phi2[k], -an[k] * phi3[k]
            u0 = c1 * (1 + g) + c2 / (r0 + r1)
            u1 = -c1 * g - c2 / (r0 + r1)
            B[k], P[k], Q[k] = b[k] + u0 / r0, -u0 / r0 + u1 / r1, -u1 / r1
    names = SOLVER_COEFS[:3] + ("coef_prev2", "coef_noise")
    return {n: v.to(torch.float32).contiguous() for n, v in zip(names, (A, B, P, Q, S))}


def normalize_sampler(sampler, sampler_eta, sample_steps, num_unets):
    """``sample(sampler=..., sampler_eta=..., sample_steps=...)`` cast per UNet: each is a scalar or a tuple / list with
    one entry per UNet.  ``sampler``: None or ``"ddpm"`` (the ancestral sampler), ``"ddim"``, ``"dpmpp_2m"``,
    ``"dpmpp_3m"``, ``"dpmpp_2m_sde"``, ``"dpmpp_3m_sde"``; ``sampler_eta`` None or in [0, 1]: None is 0 for the
    deterministic names and ``"ddim"`` and 1 for the ``_sde`` names, a non-zero value needs ``"ddim"`` or an ``_sde``
    name, and an ``_sde`` name refuses 0; ``sample_steps`` None (the constructor's timesteps) or an int >= 1.  Returns a
    list of ``(name, eta, steps or None)``.  Anything else raises ValueError.  Needs no GPU."""
    import numbers

    def per_unet(v, name):
        if isinstance(v, (tuple, list)):
            if len(v) != num_unets:
                raise ValueError(f"{name} holds {len(v)} entries for {num_unets} unets: one per unet is needed")
            return list(v)
        return [v] * num_unets

    out = []
    for i, (name, eta, steps) in enumerate(zip(per_unet(sampler, "sampler"), per_unet(sampler_eta, "sampler_eta"),
                                               per_unet(sample_steps, "sample_steps"))):
        num = i + 1
        name = default(name, "ddpm")
        if name not in SAMPLERS:
            raise ValueError(f"sampler of unet {num} must be one of {SAMPLERS} or None, got {name!r}")
        sde = name.endswith("_sde")
        eta = default(eta, 1.0 if sde else 0.0)
        if not isinstance(eta, numbers.Real) or isinstance(eta, bool) or not 0.0 <= float(eta) <= 1.0:
            raise ValueError(f"sampler_eta of unet {num} must be a number in [0, 1], got {eta!r}")
        if float(eta) != 0.0 and name != "ddim" and not sde:
            raise ValueError(f"sampler_eta={eta} of unet {num} needs sampler='ddim', got {name!r}")
        if float(eta) == 0.0 and sde:
            raise ValueError(f"sampler_eta=0 of unet {num} makes {name!r} deterministic: use sampler={name[:-4]!r}")
        if exists(steps):
            if not isinstance(steps, numbers.Integral) or isinstance(steps, bool) or int(steps) < 1:
                raise ValueError(f"sample_steps of unet {num} must be an int >= 1 or None, got {steps!r}")
            steps = int(steps)
        out.append((name, float(eta), steps))
    return out


TILE_WEIGHTS = ("uniform", "ramp")
TILE_COVER = 3   # kd_tiles_fuse_update visits at most this many tile slots per axis


def normalize_tiling(image_sizes, grid, overlap=0.25, present=None, tile_weights="uniform"):
    """``sample_tiled(grid=..., overlap=..., present=..., tile_weights=...)`` as the per-stage geometry of a fused-tile
    canvas.  The canvas of stage s is a lattice of ``ny x nx`` tile slots of size ``S`` (the stage's image size) at stride
    ``st = int(S * (1 - overlap))``; ``present[ny][nx]`` (None: all) marks the slots that hold a tile, and tiles are numbered
    in row-major order over the present slots.  Returns one dict per stage: ``S, st, ny, nx, Hc, Wc`` (canvas size
    ``(n - 1) st + S``), ``ov = max(S - st, 1)``, ``origins`` [(y0, x0)] per tile, ``tile_of`` [ny][nx] (tile index or -1),
    ``weights``.  Raises ValueError for a tile size or stride that is no multiple of 4 (the kernels move 16 bytes), a
    stride outside 1 .. S, a pixel covered by more than 3 tiles per axis, no present slot, and stages whose lattices are
    not images of one another (``st_s S_{s-1} != st_{s-1} S_s``: the canvas of stage s - 1 must resize onto the canvas of
    stage s exactly).  Needs no GPU."""
    import numbers

    if tile_weights not in TILE_WEIGHTS:
        raise ValueError(f"tile_weights must be one of {TILE_WEIGHTS}, got {tile_weights!r}")
    if (not isinstance(grid, (tuple, list)) or len(grid) != 2
            or any(not isinstance(g, numbers.Integral) or isinstance(g, bool) or int(g) < 1 for g in grid)):
        raise ValueError(f"grid must be (ny, nx), two ints >= 1, got {grid!r}")
    ny, nx = int(grid[0]), int(grid[1])
    if not isinstance(overlap, numbers.Real) or isinstance(overlap, bool):
        raise ValueError(f"overlap must be a number, got {overlap!r}")
    if present is None:
        rows = [[True] * nx for _ in range(ny)]
    else:
        rows = present.tolist() if torch.is_tensor(present) else [list(r) for r in present]
        if len(rows) != ny or any(len(r) != nx for r in rows):
            raise ValueError(f"present must be [ny={ny}][nx={nx}], got {len(rows)} rows of lengths {[len(r) for r in rows]}")
        rows = [[bool(v) for v in r] for r in rows]
    if not any(any(r) for r in rows):
        raise ValueError(f"present marks no slot of the {ny} x {nx} lattice: a canvas needs at least one tile")
    out = []
    for i, S in enumerate(image_sizes):
        num, S = i + 1, int(S)
        st = int(S * (1 - overlap))
        if S % 4 != 0:
            raise ValueError(f"tile size S={S} of unet {num} must be a multiple of 4")
        if st < 1:
            raise ValueError(f"tile stride st={st} of unet {num} (S={S}, overlap={overlap}) must be at least 1")
        if st > S:
            raise ValueError(f"tile stride st={st} of unet {num} must not exceed the tile size S={S}")
        if st % 4 != 0:
            raise ValueError(f"tile stride st={st} of unet {num} (S={S}, overlap={overlap}) must be a multiple of 4")
        if S > TILE_COVER * st:
            raise ValueError(f"tile stride st={st} of unet {num} lets more than {TILE_COVER} tiles per axis cover a pixel "
                             f"(S={S} > {TILE_COVER} st)")
        if out and st * out[-1]["S"] != out[-1]["st"] * S:
            raise ValueError(f"the lattices of unets {num - 1} and {num} are not images of one another: "
                             f"st={st} * S={out[-1]['S']} != st={out[-1]['st']} * S={S}")
        tile_of, origins = [[-1] * nx for _ in range(ny)], []
        for r in range(ny):
            for q in range(nx):
                if rows[r][q]:
                    tile_of[r][q] = len(origins)
                    origins.append((r * st, q * st))
        out.append(dict(S=S, st=st, ny=ny, nx=nx, Hc=(ny - 1) * st + S, Wc=(nx - 1) * st + S, ov=max(S - st, 1),
                        origins=origins, tile_of=tile_of, weights=tile_weights))
    return out


def normalize_devices(devices, noise_fn=None):
    """``sample_tiled(devices=...)`` as a list of ``torch.device``, one per shard of the canvas (a device may repeat: each
    shard then owns plans of its own on it); None stays None.  Raises ValueError for ``devices`` that is no sequence or is
    empty, an entry that is not a device (``torch.device``, a string or an index that names one), a device that is not
    CUDA, and ``devices`` together with ``noise_fn`` (injected noise lives on one device; a sharded canvas draws Philox
    noise, keyed by the canvas element, on every device).  Needs no GPU."""
    import numbers

    if devices is None:
        return None
    if isinstance(devices, (str, torch.device)) or not isinstance(devices, (tuple, list)) or len(devices) == 0:
        raise ValueError(f"devices must be a non-empty sequence of CUDA devices, one per shard, got {devices!r}")
    out = []
    for d in devices:
        if isinstance(d, bool) or not isinstance(d, (torch.device, str, numbers.Integral)):
            raise ValueError(f"devices: {d!r} is not a device (a torch.device, a string such as 'cuda:0' or an index)")
        try:
            dev = torch.device("cuda", int(d)) if isinstance(d, numbers.Integral) else torch.device(d)
        except (RuntimeError, ValueError) as e:
            raise ValueError(f"devices: {d!r} is not a device ({e})") from None
        if dev.type != "cuda":
            raise ValueError(f"devices: {dev} is not a CUDA device - the shards of a canvas run on the HIP engine only")
        out.append(dev)
    if len(out) > 1 and exists(noise_fn):
        raise ValueError("sample_tiled takes devices or noise_fn, one of them: a sharded canvas draws its noise on every device")
    return out


def normalize_shards(tiling, n_shards, bands=None):
    """The decomposition of a fused-tile canvas (``tiling``: normalize_tiling's) into ``n_shards`` shards by lattice rows.
    Returns one dict per stage: ``d`` (the halo depth ``ceil(S / st) - 1`` in lattice rows), ``shards`` and ``exchange``.

    A shard of ``shards`` holds: ``band = (r0, r1)``, a contiguous band of lattice rows - the bands partition the rows and
    are balanced by the number of PRESENT tiles (the largest band as small as it can be, every band holding at least one;
    ``bands = [(r0, r1), ...]`` gives them instead); ``own``: the present tiles of those rows (canvas tile numbers,
    ascending); ``halo``: the present tiles of the ``d`` lattice rows above and below the band; ``strips``: {halo tile: (row0,
    rows)}, the rows of that tile inside the band's extent; ``extent = (r0 st, (r1 - 1) st + S)``, the canvas rows the own
    tiles cover; ``owned = (r0 st, r1 st)``, through ``Hc`` for the last band - the canvas rows this shard ends; ``tiles``:
    own and halo, ascending - the order of the shard's tile store; ``base``: where the own tiles (contiguous) begin in it;
    ``tile_of`` [ny][nx]: the store slot of every tile of that set, -1 for every other slot of the lattice.
    ``exchange`` lists, per pair of shards with something to send, ``dict(src, dst, items = [(tile, row0, rows)])``: the
    strips of ``src``'s own tiles that ``dst`` holds as halo.

    Every tile that covers a pixel of a shard's extent is one of its own or halo tiles, and covers it with a row inside
    its strip: fusing own and halo over the extent gives the canvas' fused estimate there.

    Raises ValueError for ``n_shards`` that is no int >= 1, more shards than lattice rows that hold a present tile, and
    ``bands`` that do not partition the rows or hold a band without a present tile.  Needs no GPU."""
    import numbers

    if not isinstance(n_shards, numbers.Integral) or isinstance(n_shards, bool) or int(n_shards) < 1:
        raise ValueError(f"n_shards must be an int >= 1, got {n_shards!r}")
    n = int(n_shards)
    ny, nx = tiling[0]["ny"], tiling[0]["nx"]
    count = [sum(1 for t in row if t >= 0) for row in tiling[0]["tile_of"]]   # present tiles per lattice row
    filled = sum(1 for c in count if c > 0)
    if n > filled:
        raise ValueError(f"{n} shards are more than the {filled} lattice rows that hold a present tile: a shard owns at least "
                         "one row of tiles")
    if bands is None:
        # best[i][r]: the smallest largest band when the rows [0, r) make i bands that each hold a tile; the first cut wins ties
        pre = [0]
        for c in count:
            pre.append(pre[-1] + c)
        INF = float("inf")
        best = [[INF] * (ny + 1) for _ in range(n + 1)]
        cut = [[0] * (ny + 1) for _ in range(n + 1)]
        best[0][0] = 0
        for i in range(1, n + 1):
            for r in range(1, ny + 1):
                for q in range(i - 1, r):
                    load = pre[r] - pre[q]
                    if load > 0 and best[i - 1][q] < INF and max(best[i - 1][q], load) < best[i][r]:
                        best[i][r], cut[i][r] = max(best[i - 1][q], load), q
        bands, r = [], ny
        for i in range(n, 0, -1):
            bands.append((cut[i][r], r))
            r = cut[i][r]
        bands.reverse()
    else:
        bands = [tuple(int(v) for v in b) for b in bands]
        if (len(bands) != n or bands[0][0] != 0 or bands[-1][1] != ny or any(a[1] != b[0] for a, b in zip(bands, bands[1:]))
                or any(r0 >= r1 for r0, r1 in bands)):
            raise ValueError(f"bands must be {n} ranges [r0, r1) that partition the {ny} lattice rows in order, got {bands}")
    for r0, r1 in bands:
        if sum(count[r0:r1]) == 0:
            raise ValueError(f"the band of lattice rows [{r0}, {r1}) holds no present tile: a shard owns at least one tile")
    out = []
    for geo in tiling:
        S, st, Hc, tile_of = geo["S"], geo["st"], geo["Hc"], geo["tile_of"]
        d = -(-S // st) - 1
        row_tiles = lambda a, b: [t for r in range(max(a, 0), min(b, ny)) for t in tile_of[r] if t >= 0]
        owner, shards = {}, []
        for i, (r0, r1) in enumerate(bands):
            own = row_tiles(r0, r1)
            owner.update({t: i for t in own})
            extent = (r0 * st, (r1 - 1) * st + S)
            strips = {}
            for r in list(range(max(r0 - d, 0), r0)) + list(range(r1, min(r1 + d, ny))):
                lo, hi = max(extent[0] - r * st, 0), min(extent[1] - r * st, S)
                strips.update({t: (lo, hi - lo) for t in tile_of[r] if t >= 0})
            halo = sorted(strips)
            tiles = sorted(own + halo)
            slot = {t: j for j, t in enumerate(tiles)}
            shards.append(dict(band=(r0, r1), own=own, halo=halo, strips=strips, extent=extent,
                               owned=(r0 * st, r1 * st if i < n - 1 else Hc), tiles=tiles, base=slot[own[0]],
                               tile_of=[[slot.get(t, -1) for t in row] for row in tile_of]))
        pairs = {}
        for j, sh in enumerate(shards):
            for t in sh["halo"]:
                pairs.setdefault((owner[t], j), []).append((t,) + sh["strips"][t])
        out.append(dict(d=d, shards=shards, exchange=[dict(src=a, dst=b, items=items) for (a, b), items in sorted(pairs.items())]))
    return out


def tile_weight(S, st, weights="uniform"):
    """The weight of a tile's pixels in the fused estimate, fp32 [S, S]: ``"uniform"`` is 1; ``"ramp"`` is separable,
    ``w(y, x) = r(y) r(x)`` with ``r(i) = min(i + 1, S - i, ov) / ov``, ``ov = max(S - st, 1)`` - strictly positive, 1 in the
    interior, falling linearly over the overlap strip.  What kd_tiles_fuse_update forms per pixel."""
    if weights not in TILE_WEIGHTS:
        raise ValueError(f"tile_weights must be one of {TILE_WEIGHTS}, got {weights!r}")
    if weights == "uniform":
        return torch.ones(S, S, dtype=torch.float32)
    ov = max(S - st, 1)
    i = torch.arange(S)
    r = torch.minimum(torch.minimum(i + 1, S - i), torch.tensor(ov)).to(torch.float32) / float(ov)
    return r[:, None] * r[None, :]


def canvas_tables(step_tables, sampler, eta=0.0, skip=0):
    """Coefficients of the canvas step  x <- A x + B x0bar + P hist + S z  of fused-tile sampling, as solver_tables gives
    them (``coef_x, coef_x0, coef_prev, coef_noise``; with ``coef_prev2``, the coefficient of the second history, for the
    names that have one).  Every solver's are solver_tables' as they are (``skip``: the first step walked, first order for
    the multistep solvers); ``"ddpm"`` is the ancestral step in the same linear form,
    ``A = alpha_next (1 - c) / alpha``, ``B = alpha_next c``, ``P = 0``, ``S = noise_scale``, formed in float64 from the fp32
    step tables and rounded once."""
    if sampler != "ddpm":
        return solver_tables(step_tables, sampler, eta=eta, skip=skip)
    if eta != 0:
        raise ValueError(f"canvas_tables: eta={eta} needs sampler 'ddim', got 'ddpm'")
    a, an, c = (step_tables[n].to(torch.float64) for n in ("alpha", "alpha_next", "c"))
    vals = (an * (1 - c) / a, an * c, torch.zeros_like(a), step_tables["noise_scale"].to(torch.float64))
    return {n: v.to(torch.float32).contiguous() for n, v in zip(("coef_x", "coef_x0", "coef_prev", "coef_noise"), vals)}


def resize_image_to(image, target_image_size, mode="nearest"):
    if image.shape[-1] == target_image_size:
        return image
    return F.interpolate(image, target_image_size, mode=mode)


def cond_crop_maps(window, S, centre_width=None):
    """The index maps of kd_tiles_cond_gather for a conditioning window of ``window`` pixels seen at tile size ``S``:
    ``win_of`` int32 [S], the window coordinate that output coordinate p shows, and ``centre_of`` int32 [S] (None without
    ``centre_width``), the same for the `v2` centre channels.  An index ramp is pushed through the very functions the
    materialised path uses - ``resize_image_to`` for the window, ``ultra_res.grid.center_crop``, ``F.interpolate(...,
    "nearest")`` to the window and ``resize_image_to`` for the centre crop - so the maps are torch's own rounding, whatever
    it is, and one map serves both axes (every step is separable and square).  Needs no GPU."""
    from ultra_res import grid as G

    window, S = int(window), int(S)
    if window < 1 or S < 1 or window >= 2 ** 24:
        raise ValueError(f"cond_crop_maps: window={window} and S={S} must be positive (window below 2^24: the ramp is fp32)")
    ramp = torch.arange(window, dtype=torch.float32).expand(1, 1, window, window)
    read = lambda img: img[0, 0, 0].to(torch.int32).contiguous()
    win_of = read(resize_image_to(ramp, S))
    centre_of = None
    if centre_width is not None:
        if not 1 <= int(centre_width) <= window:
            raise ValueError(f"cond_crop_maps: centre_width={centre_width} must lie in 1 .. window={window}")
        centre = G.center_crop(ramp[0], int(centre_width))
        centre = F.interpolate(centre.unsqueeze(0), window, mode="nearest")
        centre_of = read(resize_image_to(centre, S))
    return win_of, centre_of


class TileCondCrops:
    """``sample_tiled(cond_crops=...)``: the conditioning images of a canvas' tiles as windows of ONE image of the level
    above, never materialised - what ``ultra_res.grid.cond_images_for_grid`` builds, described instead of built.
    ``image`` [1, Cs, W, W] (fp32 in [0, 1], or uint8); ``shifts`` [N][2], the roll (sy, sx) of each present tile in
    row-major order; ``window``: width of the centre window that is cut after the roll (it starts at
    ``center_crop_offset(W, window)``); ``fill``: the value of the pixels the roll wraps; ``centre_width``: when given,
    the centre crop of that width, enlarged (nearest) to the window, follows as Cs more channels (`v2`)."""

    def __init__(self, image, shifts, window, fill, centre_width=None):
        self.image, self.window, self.fill, self.centre_width = image, window, fill, centre_width
        self.shifts = shifts.tolist() if torch.is_tensor(shifts) else shifts

    def checked(self, n_tiles):
        """(Cs, W, channels of a tile, top, shifts as a list of int pairs); ValueError by name for what the kernel cannot
        take.  Needs no GPU."""
        import numbers

        from ultra_res import grid as G

        isint = lambda v: isinstance(v, numbers.Integral) and not isinstance(v, bool)
        img = self.image
        if not torch.is_tensor(img) or img.dim() != 4 or img.shape[0] != 1 or img.shape[2] != img.shape[3]:
            raise ValueError(f"cond_crops.image must be one square image [1, Cs, W, W], got "
                             f"{tuple(img.shape) if torch.is_tensor(img) else type(img).__name__}")
        Cs, W = int(img.shape[1]), int(img.shape[3])
        if not isint(self.window) or self.window < 1:
            raise ValueError(f"cond_crops.window must be an int >= 1, got {self.window!r}")
        if W < self.window:
            raise ValueError(f"cond_crops: the image is W={W} wide, narrower than window={self.window}: that branch of "
                             "cond_images_for_grid (roll, fill, zero padding) stays on the materialised path (cond_images=)")
        shifts = self.shifts
        if (not isinstance(shifts, (list, tuple)) or len(shifts) != n_tiles
                or any(not isinstance(s, (list, tuple)) or len(s) != 2 or not all(isint(v) for v in s) for s in shifts)):
            raise ValueError(f"cond_crops.shifts must be [tiles {n_tiles}][2] ints (sy, sx), one pair per present tile")
        shifts = [(int(sy), int(sx)) for sy, sx in shifts]
        if any(abs(v) >= W for s in shifts for v in s):
            raise ValueError(f"cond_crops.shifts must lie inside (-W, W) = (-{W}, {W})")
        if self.centre_width is not None and (not isint(self.centre_width) or not 1 <= self.centre_width <= self.window):
            raise ValueError(f"cond_crops.centre_width={self.centre_width!r} must be an int in 1 .. window={self.window}")
        return Cs, W, Cs * (2 if self.centre_width is not None else 1), G.center_crop_offset(W, int(self.window)), shifts


STAGE_SEED_STRIDE = 0x9E3779B97F4A7C15   # stage s of a cascade draws under (seed + STAGE_SEED_STRIDE * s) mod 2^64


def normalize_seed(seed, batch_size):
    """``sample(seed=...)``: None and an int pass through (one key for the whole batch tensor); a sequence of ints or a
    1-D integer tensor of length ``batch_size`` becomes a list of python ints in [0, 2^64), one Philox key per image.
    Anything else raises ValueError.  Needs no GPU."""
    import numbers

    if seed is None or (isinstance(seed, numbers.Integral) and not isinstance(seed, bool)):
        return seed
    if torch.is_tensor(seed):
        if seed.dim() != 1 or seed.dtype.is_floating_point or seed.dtype.is_complex or seed.dtype == torch.bool:
            raise ValueError(f"seed tensor must be 1-D and of an integer dtype, got shape {tuple(seed.shape)} {seed.dtype}")
        seeds = seed.tolist()
    elif isinstance(seed, (str, bytes)) or not hasattr(seed, "__len__") or not hasattr(seed, "__iter__"):
        raise ValueError(f"seed must be an int, a sequence of ints or a 1-D integer tensor, got {type(seed).__name__}")
    else:
        seeds = list(seed)
    if len(seeds) != batch_size:
        raise ValueError(f"seed holds {len(seeds)} values for a batch of {batch_size}: one per image is needed")
    out = []
    for s in seeds:
        if not isinstance(s, numbers.Integral) or isinstance(s, bool):
            raise ValueError(f"per-image seeds must be ints, got {s!r}")
        if not 0 <= int(s) < 2 ** 64:
            raise ValueError(f"per-image seed {int(s)} is outside [0, 2^64)")
        out.append(int(s))
    return out


def normalize_init_images(init_images, skip_steps, *, steps, batch_size, channels, start_at_unet_number=1,
                          stop_at_unet_number=None):
    """``sample(init_images=..., skip_steps=...)`` cast per UNet, as the library does: ``init_images`` is None, one tensor
    [batch, channels, H, W] used by every UNet sampled, or a tuple / list with one entry (tensor or None) per UNet;
    ``skip_steps`` is None (0), an int, or a tuple / list with one entry (int or None) per UNet.  ``steps[i]`` is the
    number of schedule steps of UNet i + 1; its skip must lie in 0 .. steps[i] - 1.  Returns a list of
    ``(float tensor in [0, 1] or None, skip)``, one pair per UNet; entries of UNets that ``start_at_unet_number`` /
    ``stop_at_unet_number`` leave out are not looked at and come back as ``(None, 0)``.  uint8 images are divided by 255,
    as cond_images are.  Anything else raises ValueError.  Needs no GPU."""
    import numbers

    n = len(steps)

    def per_unet(v, name):
        if isinstance(v, (tuple, list)):
            if len(v) != n:
                raise ValueError(f"{name} holds {len(v)} entries for {n} unets: one per unet is needed")
            return list(v)
        return [v] * n

    inits, skips = per_unet(init_images, "init_images"), per_unet(skip_steps, "skip_steps")
    out = []
    for i, (init, skip, T) in enumerate(zip(inits, skips, steps)):
        num = i + 1
        if num < start_at_unet_number or (exists(stop_at_unet_number) and num > stop_at_unet_number):
            out.append((None, 0))
            continue
        skip = default(skip, 0)
        if not isinstance(skip, numbers.Integral) or isinstance(skip, bool):
            raise ValueError(f"skip_steps of unet {num} must be an int, got {skip!r}")
        if not 0 <= int(skip) < T:
            raise ValueError(f"skip_steps={int(skip)} of unet {num} is outside 0 .. {T - 1}, the steps of its schedule")
        if exists(init):
            if not torch.is_tensor(init):
                raise ValueError(f"init_images of unet {num} must be a tensor or None, got {type(init).__name__}")
            if init.dim() != 4 or init.shape[0] != batch_size or init.shape[1] != channels or 0 in init.shape[2:]:
                raise ValueError(f"init_images of unet {num} must be [batch {batch_size}, channels {channels}, H, W], "
                                 f"got {tuple(init.shape)}")
            if init.dtype == torch.uint8:
                init = init.float() / 255.0
            elif not init.dtype.is_floating_point:
                raise ValueError(f"init_images of unet {num} must be of a floating dtype or uint8, got {init.dtype}")
        out.append((init, int(skip)))
    return out


def normalize_known(known_image, known_mask, known_resample_times=1, *, channels):
    """``sample_tiled(known_image=..., known_mask=..., known_resample_times=...)``: the pixels a canvas keeps.
    ``known_image`` is ONE image [1, channels, Hk, Wk] with values in [0, 1] - float32 (any view with unit x stride: a
    window of a larger canvas is used in place) or uint8 (divided by 255 once); ``known_mask`` is [Hk, Wk] or [1, Hk, Wk],
    non-zero = keep - bool / uint8 (a view with unit x stride, used in place) or floating (``!= 0``, converted once);
    ``known_resample_times`` is an int >= 1, more than 1 only with a mask.  Returns ``(image, mask [Hk, Wk], R)``, or
    ``(None, None, 1)`` without the pair.  Anything else raises ValueError by name.  Needs no GPU."""
    import numbers

    R = known_resample_times
    if not isinstance(R, numbers.Integral) or isinstance(R, bool) or int(R) < 1:
        raise ValueError(f"known_resample_times must be an int >= 1, got {R!r}")
    if exists(known_image) != exists(known_mask):
        raise ValueError("known_image and known_mask come together: "
                         f"{'known_mask' if exists(known_image) else 'known_image'} is missing")
    if not exists(known_image):
        if int(R) != 1:
            raise ValueError(f"known_resample_times={int(R)} needs known_image and known_mask: without known pixels nothing is resampled")
        return None, None, 1
    img, mask = known_image, known_mask
    if not torch.is_tensor(img) or img.dim() != 4 or img.shape[0] != 1 or img.shape[1] != channels or 0 in img.shape[2:]:
        raise ValueError(f"known_image must be one image [1, channels {channels}, Hk, Wk], got "
                         f"{tuple(img.shape) if torch.is_tensor(img) else type(img).__name__}")
    if not torch.is_tensor(mask) or mask.dim() not in (2, 3) or (mask.dim() == 3 and mask.shape[0] != 1):
        raise ValueError(f"known_mask must be [Hk, Wk] or [1, Hk, Wk], got "
                         f"{tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__}")
    mask = mask[0] if mask.dim() == 3 else mask
    if tuple(mask.shape) != tuple(img.shape[2:]):
        raise ValueError(f"known_image is {tuple(img.shape[2:])} and known_mask {tuple(mask.shape)}: the sizes must agree")
    if img.dtype == torch.uint8:
        img = img.float() / 255.0
    elif not img.dtype.is_floating_point:
        raise ValueError(f"known_image must be of a floating dtype or uint8, got {img.dtype}")
    elif img.dtype != torch.float32:
        img = img.float()
    elif img.stride(3) != 1:
        raise ValueError(f"known_image must have unit x stride (it is used in place), got strides {tuple(img.stride())}")
    if mask.dtype.is_floating_point:
        mask = (mask != 0).to(torch.uint8)
    elif mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"known_mask must be bool, uint8 or floating, got {mask.dtype}")
    elif mask.stride(1) != 1:
        raise ValueError(f"known_mask must have unit x stride (it is used in place), got strides {tuple(mask.stride())}")
    return img, mask, int(R)


def normalize_init_canvas(init_canvas, init_skip_steps, *, steps, channels, start_at_unet_number=1, stop_at_unet_number=None):
    """``sample_tiled(init_canvas=..., init_skip_steps=...)`` cast per UNet, the canvas-level ``normalize_init_images``:
    ``init_canvas`` is None, one canvas-shaped image [1, channels, H, W] (float32 with unit x stride, used in place; uint8
    divided by 255) for every UNet sampled, or one entry per UNet; ``init_skip_steps`` None (0), an int, or one entry per
    UNet, each in 0 .. steps[i] - 1.  Returns ``[(image or None, skip)]``; ValueError by name otherwise.  Needs no GPU."""
    try:
        out = normalize_init_images(init_canvas, init_skip_steps, steps=steps, batch_size=1, channels=channels,
                                    start_at_unet_number=start_at_unet_number, stop_at_unet_number=stop_at_unet_number)
    except ValueError as e:   # the same rules under the canvas-level names
        raise ValueError(str(e).replace("init_images", "init_canvas").replace("skip_steps", "init_skip_steps")
                         .replace("[batch 1,", "[1,")) from None
    for i, (init, _) in enumerate(out):
        if exists(init) and init.dtype == torch.float32 and init.stride(3) != 1:
            raise ValueError(f"init_canvas of unet {i + 1} must have unit x stride (it is used in place), got strides "
                             f"{tuple(init.stride())}")
    return [(None if init is None else init.float(), skip) for init, skip in out]


# ============================================================================ one stage on the engine (host side)
_OBJECTIVES = {"noise": 0, "v": 1, "x_start": 2}


def normalize_into(into, *, streamed, channels, Hc, Wc, unet=None):
    """``sample_tiled(into=(canvas, oy, ox))`` as ``(canvas, int(oy), int(ox))``; None stays None.  ``canvas`` is a contiguous
    fp32 [1, channels, Ho, Wo] that holds the ``Hc x Wc`` canvas of the last sampled UNet (number ``unet``, for the message)
    at row ``oy``, column ``ox``.  Raises ValueError for ``into`` without ``streamed`` (only kd_tiles_finalize_rows writes a
    stage in place), anything that is not such a triple, an offset or a canvas width that is no multiple of 4 (the kernels
    move 16 bytes), a window out of bounds, and - last, so that every other rule can be met without a GPU - a canvas that
    is not on the device."""
    import numbers

    if into is None:
        return None
    if not streamed:
        raise ValueError("sample_tiled(into=...) needs streamed=True: only kd_tiles_finalize writes a stage in place")
    if not isinstance(into, (tuple, list)) or len(into) != 3 or not torch.is_tensor(into[0]):
        raise ValueError("into must be (canvas [1, C, Ho, Wo], oy, ox)")
    dst, oy, ox = into
    if dst.dtype != torch.float32:
        raise ValueError(f"into: the canvas must be float32, got {dst.dtype}")
    if dst.dim() != 4 or dst.shape[0] != 1 or dst.shape[1] != channels or not dst.is_contiguous():
        raise ValueError(f"into: the canvas must be a contiguous [1, {channels}, Ho, Wo], got shape {tuple(dst.shape)}")
    if any(not isinstance(v, numbers.Integral) or isinstance(v, bool) for v in (oy, ox)):
        raise ValueError(f"into: the offset (oy, ox) must be two ints, got ({oy!r}, {ox!r})")
    if oy % 4 != 0 or ox % 4 != 0 or dst.shape[3] % 4 != 0:
        raise ValueError(f"into: the offset (oy, ox) = ({oy}, {ox}) and the canvas width {dst.shape[3]} must be multiples "
                         "of 4 (the kernels move 16 bytes)")
    if oy < 0 or ox < 0 or oy + Hc > dst.shape[2] or ox + Wc > dst.shape[3]:
        raise ValueError(f"into: the {Hc} x {Wc} canvas of unet {unet} at ({oy}, {ox}) is out of bounds of the "
                         f"{dst.shape[2]} x {dst.shape[3]} canvas")
    if not dst.is_cuda:
        raise ValueError(f"into: the canvas must live on the device, got {dst.device}")
    return dst, int(oy), int(ox)


def _f32(t, device):
    return None if t is None else t.to(device=device, dtype=torch.float32).contiguous()


class _StepSchedule:
    """The host tables of one stage's sampler together with the ctypes struct the engine reads them through:
    ``kd_schedule_t`` for ``"ddpm"`` (the arrays of ``step_tables()``), ``kd_solver_schedule_t`` for ``"ddim"`` /
    ``"dpmpp_2m"`` (five of them plus ``solver_tables``), ``kd_solver3_schedule_t`` for the solvers whose tables hold a
    ``coef_prev2`` (``"dpmpp_3m"`` and the ``_sde`` names), ``kd_edm_schedule_t`` through ``_StepSchedule.edm``.  ``steps`` and
    ``loop`` name the library entries that take the struct, ``T`` is the number of steps.

    Pointer lifetime: the struct's pointers point into the memory of the tensors in ``self.tables`` and nothing else keeps
    that memory alive, so ``struct`` is valid exactly as long as this object is.  Hold the object over every call that is
    given ``byref(struct)``; the engine copies the arrays into its own staging buffer inside the call, so nothing has to
    outlive it."""

    def __init__(self, step_tables, sampler="ddpm", eta=0.0, skip=0):
        if sampler == "ddpm":
            self._own(E.kd_schedule_t(), step_tables, "kd_sample")
        else:   # the solver's coefficients in place of the ancestral step's; its own entries, tables and step graph
            coefs = solver_tables(step_tables, sampler, eta=eta, skip=skip)
            if "coef_prev2" in coefs:
                # the first two steps walked read nothing the plan's history ring holds (the engine checks step 0 itself)
                assert not coefs["coef_prev"][skip] and not coefs["coef_prev2"][skip:skip + 2].any(), "solver order at the start"
                self._own(E.kd_solver3_schedule_t(), {**step_tables, **coefs}, "kd_solver3_sample")
            else:
                self._own(E.kd_solver_schedule_t(), {**step_tables, **coefs}, "kd_solver_sample")
            self.draws = bool(coefs["coef_noise"].any())   # some step adds noise: the ancestral step's draw
        self.struct.T = self.T = int(step_tables["alpha"].numel())

    @classmethod
    def edm(cls, edm_tables, S_noise):
        self = cls.__new__(cls)
        self._own(E.kd_edm_schedule_t(), edm_tables, "kd_edm_sample")
        self.struct.N = self.T = int(edm_tables["sigma"].numel())
        self.struct.S_noise = float(S_noise)
        return self

    def _own(self, struct, tables, entry):
        self.struct, self.steps, self.loop, self.tables = struct, entry + "_steps", entry + "_loop", {}
        for name, ctype in struct._fields_:
            if ctype is C.POINTER(C.c_float):   # (ctypes caches pointer types: one object per pointee)
                t = self.tables[name] = tables[name]
                assert t.dtype == torch.float32 and t.is_contiguous() and not t.is_cuda, f"schedule table {name}: fp32 on the host"
                setattr(struct, name, t.numpy().ctypes.data_as(C.POINTER(C.c_float)))


def _walk(lib, sc, h, args, img, *, skip=0, trace=None, self_cond=False):
    """Steps ``skip .. T - 1`` of the schedule ``sc`` (a _StepSchedule) on the plan ``h``, in place on ``img`` (x at step
    ``skip`` in, the unnormalised sample out).  A self-conditioned plan starts step ``skip`` > 0 from zeros, as step 0
    does by itself.  ``trace`` receives a copy of the state behind every step walked (one step per call)."""
    steps, stream = getattr(lib, sc.steps), E.current_stream
    if skip > 0 and self_cond:
        E.check(lib.kd_sample_set_self_cond(h, None, stream()))
    if exists(trace):
        for k in range(skip, sc.T):
            E.check(steps(h, C.byref(sc.struct), C.byref(args), E.ptr(img), k, k + 1, stream()))
            trace.append(img.clone())
        E.check(lib.kd_sample_finalize(h, C.byref(args), E.ptr(img), stream()))
    elif skip > 0:
        E.check(steps(h, C.byref(sc.struct), C.byref(args), E.ptr(img), skip, sc.T, stream()))
        E.check(lib.kd_sample_finalize(h, C.byref(args), E.ptr(img), stream()))
    else:
        E.check(getattr(lib, sc.loop)(h, C.byref(sc.struct), C.byref(args), E.ptr(img), stream()))


def _stage_noise(lib, noise_fn, seed, stage, device):
    """The Gaussian draws of one stage: ``(gauss, key, keys)``.  An int ``seed`` gives the stage's Philox key ``key`` and
    ``keys = None``; a list of per-image seeds (normalize_seed) gives ``key = 0`` and ``keys``, the host array of one key
    per image, each derived per stage like the int.  ``gauss(tag, shape, sid)`` is ``noise_fn(tag, shape)`` when noise is
    injected, else Philox stream ``sid`` under ``key`` - with ``keys``, row b is the batch-1 draw under image b's key."""
    derive = lambda s: (s + STAGE_SEED_STRIDE * stage) % (2 ** 64)
    key, keys = (0, E.seed_array([derive(s) for s in seed])) if isinstance(seed, list) else (derive(seed), None)

    def gauss(tag, shape, sid):
        if exists(noise_fn):
            return _f32(noise_fn(tag, tuple(shape)), device)
        out = torch.empty(tuple(shape), device=device, dtype=torch.float32)
        if exists(keys):
            E.check(lib.kd_philox_normal_rows(E.ptr(out), shape[0], out.numel() // shape[0], keys, sid, E.current_stream()))
        else:
            E.check(lib.kd_philox_normal(E.ptr(out), out.numel(), key, sid, E.current_stream()))
        return out

    return gauss, key, keys


class _StageIO:
    """The inputs of one plan (UNet, batch, size, device) at stable addresses, and the kd_sample_args_t that names them.
    The engine caches the captured step graph keyed on the device addresses it was captured with.  Per-call tensors are
    therefore copied into per-(batch, size, device) buffers of the UNet that keep their address, so that e.g. the 64
    patches of an ultra-res grid replay one graph per stage instead of re-capturing it for every patch; sample() and
    sample_tiled() share them by name.  The object owns everything ``args`` points into: the buffers, and ``keys``, the
    host array of per-image Philox keys."""

    def __init__(self, imagen, unet, batch, size, device, *, dynamic_threshold, use_graph, key, keys=None, resample_times=1,
                 replica=0):
        self.unet, self.batch, self.device, self.keys = unet, batch, device, keys
        # (`replica` > 0: the buffers of a further plan of the same shape - Unet.engine(replica=) - apart from the first's)
        self._io = unet._io_buffers.setdefault((batch, size, device.index) + ((replica,) if replica else ()), {})
        args = self.args = E.kd_sample_args_t()
        args.dynamic_threshold = int(bool(dynamic_threshold))
        args.percentile = imagen.dynamic_thresholding_percentile
        args.resample_times = resample_times
        args.seed = key
        if exists(keys):
            args.seeds = keys
        args.use_graph = int(bool(use_graph))
        args.cond_table = int(getattr(imagen, "cond_table", 0))   # engine extension: < 0 switches the table off

    def buf(self, name, shape):
        """The stable fp32 buffer of this name and shape (allocated on first use and when the shape changes)."""
        t = self._io.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._io[name] = torch.empty(tuple(shape), device=self.device, dtype=torch.float32)
        return t

    def put(self, name, t):
        """`t` copied into its stable buffer (stream-ordered); None stays None."""
        if t is None:
            return None
        b = self.buf(name, t.shape)
        b.copy_(t)
        return b

    def lowres_level(self, log_snr):
        """One augmentation level for the whole batch (the library's sample() has no other form): lets the engine table the
        time conditioning per schedule step."""
        self.args.d_lowres_log_snr = E.ptr(self.put("lowres_log_snr", log_snr.to(self.device).expand(self.batch)))
        self.args.lowres_log_snr_uniform = 1
        self.args.lowres_log_snr_value = float(log_snr[0])

    def text(self, h, text_embeds, text_masks, cond_scale):
        """Step-invariant: pooled text tokens + text hiddens, once per stage; with guidance, their null twins for the second
        forward."""
        args = self.args
        tok, hid = self.unet.text_cond(h, text_embeds, text_masks, drop=False, device=self.device)
        args.d_text_tokens, args.d_text_hiddens = E.ptr(self.put("text_tokens", tok)), E.ptr(self.put("text_hiddens", hid))
        args.cond_scale = cond_scale
        if cond_scale != 1.0:
            tok, hid = self.unet.text_cond(h, text_embeds, text_masks, drop=True, device=self.device)
            args.d_null_text_tokens = E.ptr(self.put("null_text_tokens", tok))
            args.d_null_text_hiddens = E.ptr(self.put("null_text_hiddens", hid))


# ============================================================================ Imagen
class Imagen(nn.Module):
    def __init__(self, unets, *, image_sizes, text_encoder_name=None, text_embed_dim=None, channels=3,
                 timesteps=1000, cond_drop_prob=0.1, loss_type="l2", noise_schedules="cosine",
                 pred_objectives="noise", random_crop_sizes=None, lowres_noise_schedule="linear",
                 lowres_sample_noise_level=0.2, per_sample_random_aug_noise_level=False, condition_on_text=True,
                 auto_normalize_img=True, dynamic_thresholding=True, dynamic_thresholding_percentile=0.95,
                 only_train_unet_number=None, **ignored_training_kwargs):
        super().__init__()
        assert auto_normalize_img, "the engine's finalize step assumes auto_normalize_img=True"
        self.condition_on_text = condition_on_text
        self.unconditional = not condition_on_text
        self.channels = channels
        unets = cast_tuple(unets)
        n = len(unets)
        timesteps = cast_tuple(timesteps, n)
        ns = cast_tuple(noise_schedules)
        ns = (*ns, *("cosine",) * max(0, 2 - len(ns)))
        ns = (*ns, *("linear",) * max(0, n - len(ns)))
        self.noise_schedulers = nn.ModuleList(
            [GaussianDiffusionContinuousTimes(noise_schedule=s, timesteps=t) for t, s in zip(timesteps, ns)])
        self.random_crop_sizes = cast_tuple(random_crop_sizes, n)
        self.lowres_noise_schedule = GaussianDiffusionContinuousTimes(noise_schedule=lowres_noise_schedule)
        self.pred_objectives = cast_tuple(pred_objectives, n)
        self.text_embed_dim = default(text_embed_dim, 768)  # google/t5-v1_1-base
        self.unets = nn.ModuleList([])
        for ind, u in enumerate(unets):
            assert isinstance(u, (Unet, NullUnet)), "unets must be Unet or NullUnet instances"
            u = u.cast_model_parameters(
                lowres_cond=ind != 0, cond_on_text=condition_on_text,
                text_embed_dim=self.text_embed_dim if condition_on_text else None, channels=channels,
                channels_out=channels)
            self.unets.append(u)
        self.image_sizes = cast_tuple(image_sizes)
        assert n == len(self.image_sizes), \
            f"you did not supply the correct number of u-nets ({n}) for resolutions {self.image_sizes}"
        lowres = tuple(u.lowres_cond for u in self.unets)
        assert lowres == (False, *((True,) * (n - 1))), \
            "the first unet must be unconditioned (by low resolution image), the rest must have lowres_cond=True"
        self.lowres_sample_noise_level = lowres_sample_noise_level
        self.cond_drop_prob = cond_drop_prob
        self.dynamic_thresholding = cast_tuple(dynamic_thresholding, n)
        self.dynamic_thresholding_percentile = dynamic_thresholding_percentile
        self.register_buffer("_temp", torch.tensor([0.0]), persistent=False)

    @property
    def device(self):
        return self._temp.device

    def get_unet(self, unet_number):
        assert 0 < unet_number <= len(self.unets)
        return self.unets[unet_number - 1]

    def forward(self, *a, **k):
        raise NotImplementedError("training is outside the sampling hot path this package replaces (SURVEY §2)")

    # ------------------------------------------------------------------ sampling
    @torch.no_grad()
    def sample(self, texts=None, text_masks=None, text_embeds=None, video_frames=None, cond_images=None,
               cond_video_frames=None, post_cond_video_frames=None, inpaint_videos=None, inpaint_images=None,
               inpaint_masks=None, inpaint_resample_times=5, init_images=None, skip_steps=None, batch_size=1,
               cond_scale=1.0, lowres_sample_noise_level=None, start_at_unet_number=1, start_image_or_video=None,
               stop_at_unet_number=None, return_all_unet_outputs=False, return_pil_images=False, device=None,
               use_tqdm=True, use_one_unet_in_gpu=True, *, noise_fn: Optional[Callable] = None,
               seed: Optional[int] = None, use_graph: bool = True, trace: Optional[list] = None,
               sampler=None, sampler_eta=None, sample_steps=None):
        """Signature of the library's ``Imagen.sample``.  Extensions (keyword-only):
        ``noise_fn(tag, shape)`` injects every Gaussian draw (parity tests, see oracle/sampler_ref.py
        for the tags); ``seed`` keys the on-device Philox stream when no ``noise_fn`` is given
        (default: drawn from torch's global generator, so ``torch.manual_seed`` reproduces a run).  An int keys
        one stream over the whole batch tensor; a sequence of ints or a 1-D integer tensor of length ``batch_size``
        keys every image by itself: image b then draws the noise of ``sample(batch_size=1, seed=seed[b])``, whatever
        batch it runs in.
        ``init_images`` / ``skip_steps`` (the library's, cast per UNet by ``normalize_init_images``): the stage starts from
        ``z + nearest(2 init - 1)`` (EDM: ``sigma_0 z + ...``, sigma_0 the first sigma of the full schedule) and walks the
        schedule steps ``skip .. T - 1`` only; a step keeps its index, hence its table rows, noise streams and
        ``noise_fn`` tags, and ``trace`` receives one state per step walked.
        ``sampler`` / ``sampler_eta`` / ``sample_steps`` (a scalar or one entry per UNet, ``normalize_sampler``): few-step
        sampling of the same DDPM-trained weights.  ``sampler`` None or ``"ddpm"`` is the ancestral sampler, ``"ddim"`` is
        DDIM(``sampler_eta``), ``"dpmpp_2m"`` / ``"dpmpp_3m"`` DPM-Solver++(2M / 3M) with data prediction and
        ``"dpmpp_2m_sde"`` / ``"dpmpp_3m_sde"`` their stochastic forms at ``sampler_eta`` (None: 1) (``solver_tables``);
        ``sample_steps=N`` walks the N-step schedule of the UNet's kind instead of the constructor's ``timesteps``, with any
        sampler, and is what ``skip_steps`` then counts in.  DDIM(eta > 0) and the ``_sde`` solvers draw the ancestral step's
        noise (``noise_fn`` tag ``("step", stage, k, r)``, Philox purpose 1) in the steps that add some - the last adds
        none; DDIM(0), 2M and 3M draw none."""
        for name, v in dict(texts=texts, video_frames=video_frames, cond_video_frames=cond_video_frames,
                            post_cond_video_frames=post_cond_video_frames, inpaint_videos=inpaint_videos).items():
            if exists(v):
                raise NotImplementedError(f"sample({name}=...) is not used by the reference and not planned")
        n_images = batch_size   # as settled below: the batched tensor arguments win over batch_size
        if not self.unconditional and exists(text_embeds):
            n_images = text_embeds.shape[0]
        if exists(inpaint_images) and self.unconditional and n_images == 1:
            n_images = inpaint_images.shape[0]
        seed = normalize_seed(seed, n_images)
        solvers = self._solver_args(sampler, sampler_eta, sample_steps)
        starts = normalize_init_images(init_images, skip_steps,
                                       steps=[default(st, T) for (_, _, st), T in zip(solvers, self._num_steps())],
                                       batch_size=n_images,
                                       channels=self.channels, start_at_unet_number=start_at_unet_number,
                                       stop_at_unet_number=stop_at_unet_number)
        device, text_masks, cond_images, seed, cond_scale, lowres_sample_noise_level, img = self._sampling_setup(
            device, text_embeds, text_masks, cond_images, seed, cond_scale, lowres_sample_noise_level, start_at_unet_number,
            start_image_or_video)
        # with the text asserts passed (text_embeds given exactly when the model is conditioned on text), the library's
        # batch size - text_embeds' rows, else an unconditional batch of 1 follows inpaint_images - is n_images as settled above
        batch_size = n_images
        if exists(inpaint_images):
            assert inpaint_images.shape[0] == batch_size, \
                "number of inpainting images must be equal to the specified batch size on sample `sample(batch_size=<int>)``"
        assert not (exists(inpaint_images) ^ exists(inpaint_masks)), "inpaint images and masks must be both passed in to do inpainting"
        if start_at_unet_number > 1:
            assert start_at_unet_number <= len(self.unets), "must start a unet that is less than the total number of unets"
            assert not exists(stop_at_unet_number) or start_at_unet_number <= stop_at_unet_number
            img = resize_image_to(img, self.image_sizes[start_at_unet_number - 2])

        outputs = []
        for num, unet, sched, obj, dyn, cs, solver in self._stages(solvers, cond_scale, start_at_unet_number,
                                                                  stop_at_unet_number):
            init_image, skip = starts[num - 1]
            img = self._p_sample_loop(
                unet, num, self.image_sizes[num - 1], sched, obj, dyn, batch_size, device, img, cond_images, inpaint_images,
                inpaint_masks, inpaint_resample_times, lowres_sample_noise_level, noise_fn, seed, use_graph, trace,
                text_embeds=text_embeds, text_masks=text_masks, cond_scale=cs, init_image=init_image, skip=skip,
                solver=solver)
            outputs.append(img)

        out = outputs if return_all_unet_outputs else outputs[-1]
        if not return_pil_images:
            return out
        from PIL import Image  # noqa: local import, PIL only needed for this branch
        # the library maps T.ToPILImage() over the images: float -> mul(255).byte(), i.e. truncation; mode by channel
        # count: L (one channel: a 2-D array), LA, RGB, RGBA
        def to_pil(t):
            arrs = [i.clamp(0, 1).mul(255).to(torch.uint8).permute(1, 2, 0).cpu().numpy() for i in t]
            return [Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a) for a in arrs]

        return [to_pil(o) for o in out] if return_all_unet_outputs else to_pil(out)

    def _sampling_setup(self, device, text_embeds, text_masks, cond_images, seed, cond_scale, lowres_level,
                        start_at_unet_number, start_image):
        """What sample() and sample_tiled() share behind their own argument refusals: the GPU and device check, eval mode,
        the library's text asserts, and the defaults.  Returns (device, text_masks, cond_images as floats, seed, cond_scale
        per UNet, low-res noise level, the start image as fp32 on the device - None when sampling starts at UNet 1)."""
        E.require_gpu()
        device = torch.device(default(device, self.device))
        if device.type != "cuda":
            raise E.EngineUnavailable(f"sampling runs on the HIP engine only; got device {device}")
        self.eval()
        assert not (self.condition_on_text and not exists(text_embeds)), "text or text encodings must be passed into imagen if specified"
        assert not (not self.condition_on_text and exists(text_embeds)), "imagen specified not to be conditioned on text, yet it is presented"
        assert not (exists(text_embeds) and text_embeds.shape[-1] != self.text_embed_dim), \
            f"invalid text embedding dimension being passed in (should be {self.text_embed_dim})"
        if exists(text_embeds):
            text_masks = default(text_masks, lambda: torch.any(text_embeds != 0.0, dim=-1))
        if exists(cond_images) and cond_images.dtype == torch.uint8:
            cond_images = cond_images.float() / 255.0
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if start_at_unet_number > 1:
            assert exists(start_image), "starting image or video must be supplied if only doing upscaling"
            start_image = _f32(start_image, device)
        else:
            start_image = None
        return (device, text_masks, cond_images, seed, cast_tuple(cond_scale, len(self.unets)),
                default(lowres_level, self.lowres_sample_noise_level), start_image)

    def _stages(self, solvers, cond_scale, start_at_unet_number=1, stop_at_unet_number=None):
        """The UNets a sampling call walks, ``start_at_unet_number .. stop_at_unet_number``: per stage ``(number, unet,
        schedule, objective, dynamic-threshold flag, cond_scale, (solver, eta))``, the schedule already on the stage's
        ``sample_steps``.  ``solvers`` as ``_solver_args`` gives them, ``cond_scale`` one entry per UNet."""
        for num, (unet, sched, obj, dyn, cs, (solver, eta, steps)) in enumerate(
                zip(self.unets, self.noise_schedulers, self.pred_objectives, self.dynamic_thresholding, cond_scale, solvers), 1):
            if num < start_at_unet_number:
                continue
            assert not isinstance(unet, NullUnet), "one cannot sample from null / placeholder unets"
            assert not (cs != 1.0 and not self.condition_on_text), \
                "imagen was not trained with conditional dropout, and thus one cannot use classifier free guidance (cond_scale anything other than 1)"
            yield num, unet, sched.with_timesteps(steps) if exists(steps) else sched, obj, dyn, float(cs), (solver, eta)
            if exists(stop_at_unet_number) and stop_at_unet_number == num:
                break

    def _p_sample_loop(self, unet, stage, size, sched, objective, dynamic_threshold, batch, device, prev_img,
                       cond_images, inpaint_images, inpaint_masks, resample_times, lowres_level, noise_fn, seed,
                       use_graph, trace, text_embeds=None, text_masks=None, cond_scale=1.0, init_image=None, skip=0,
                       solver=("ddpm", 0.0)):
        lib = E.load()
        shape = (batch, self.channels, size, size)
        f32 = lambda t: _f32(t, device)
        gauss, key, keys = _stage_noise(lib, noise_fn, seed, stage, device)
        has_inpaint = exists(inpaint_images) and exists(inpaint_masks)
        R = resample_times if has_inpaint else 1
        io = _StageIO(self, unet, batch, size, device, dynamic_threshold=dynamic_threshold, use_graph=use_graph, key=key,
                      keys=keys, resample_times=R)
        args = io.args
        with torch.cuda.device(device):
            if unet.lowres_cond:
                ls = self.lowres_noise_schedule.log_snr(torch.full((batch,), lowres_level, dtype=torch.float32))
                a, s = log_snr_to_alpha_sigma(ls)
                lowres = resize_image_to(prev_img, size) * 2 - 1
                lowres = (a.to(device)[:, None, None, None] * lowres
                          + s.to(device)[:, None, None, None] * gauss(("lowres", stage), lowres.shape, (16 << 32) | 1))
                args.d_lowres = E.ptr(io.put("lowres", lowres.contiguous()))
                io.lowres_level(ls)
            if exists(cond_images):
                assert cond_images.shape[1] == unet.cond_images_channels, "invalid number of channels in conditioning image"
                args.d_cond_images = E.ptr(io.put("cond", f32(resize_image_to(f32(cond_images), size))))
            if has_inpaint:
                args.d_inpaint_images = E.ptr(io.put("inpaint", f32(resize_image_to(f32(inpaint_images) * 2 - 1, size))))
                args.d_inpaint_masks = E.ptr(io.put("mask", f32(resize_image_to(f32(inpaint_masks)[:, None], size).bool().float())))
            keep = []
            # x_T = scale * z + (2 * nearest(init_image) - 1), written into the stable buffer by one engine call: z drawn in
            # the kernel (stream (16 << 32) | 2 under the stage's key or keys) or read from the injected tensor
            img = io.buf("img", shape)
            z = f32(noise_fn(("init", stage), shape)) if exists(noise_fn) else None
            init_image = f32(init_image)
            hs, ws = init_image.shape[2:] if exists(init_image) else (0, 0)
            E.check(lib.kd_sample_start(E.ptr(img), batch, self.channels, size, self._start_scale(stage), key, keys, E.ptr(z),
                                        E.ptr(init_image), hs, ws, E.current_stream()))
            keep += [z, init_image]
            with_text = exists(text_embeds) and unet.cond_on_text
            h = unet.engine(batch, size, device, with_text=with_text)
            if with_text:
                io.text(h, text_embeds, text_masks, cond_scale)

            def stack(kind, T):   # injected noise of every iteration, [T*R, *shape], indexed k*R + (R-1-r)
                ts = [noise_fn((kind, stage, k, r), shape) for k in range(skip, T) for r in reversed(range(R))]
                t = f32(torch.stack(ts))
                if skip:   # the steps not walked are not asked for; a step keeps its slot
                    t = torch.cat([t.new_zeros((skip * R, *t.shape[1:])), t])
                keep.append(t)
                return E.ptr(t)

            self._stage_loop(lib, h, args, img, stage=stage, sched=sched, objective=objective, has_inpaint=has_inpaint,
                             R=R, stack=stack if exists(noise_fn) else None, trace=trace, skip=skip,
                             self_cond=bool(unet.self_cond), solver=solver)
            # No host synchronisation here: the engine copies the schedule tables into its own staging buffer inside
            # the call, and the injected-noise tensors in `keep` are device memory of torch's current stream - the
            # caching allocator re-uses it for later allocations of that stream only, i.e. after these launches.
            del keep
            img = img.clone()  # the stable buffer is overwritten by the next call (stream-ordered copy)
        return img

    # ------------------------------------------------------------------ fused-tile canvas sampling
    @torch.no_grad()
    def sample_tiled(self, grid, overlap=0.25, present=None, tile_batch=16, tile_weights="uniform", cond_images=None,
                     text_embeds=None, text_masks=None, cond_scale=1.0, sampler=None, sampler_eta=None, sample_steps=None,
                     seed: Optional[int] = None, noise_fn: Optional[Callable] = None, use_graph: bool = True,
                     start_at_unet_number=1, stop_at_unet_number=None, start_image_or_video=None,
                     return_all_unet_outputs=False, lowres_sample_noise_level=None, device=None, inpaint_images=None,
                     inpaint_masks=None, inpaint_resample_times=None, init_images=None, skip_steps=None, streamed=False,
                     cond_crops=None, into=None, known_image=None, known_mask=None, known_resample_times=1, init_canvas=None,
                     init_skip_steps=None, devices=None):
        """A canvas of overlapping tiles denoised jointly (MultiDiffusion / Mixture of Diffusers; an engine extension, the
        alternative to sequential outpainting).  The canvas of a stage is ONE noisy image over the ``grid = (ny, nx)``
        lattice of ``normalize_tiling``; at every schedule step every present tile is denoised by itself, ``tile_batch``
        tiles per UNet forward, their thresholded x0 estimates are averaged where tiles overlap (``tile_weights``) and the
        update of ``sampler`` (None / ``"ddpm"``, ``"ddim"`` with ``sampler_eta``, ``"dpmpp_2m"``, ``"dpmpp_3m"`` and the
        ``_sde`` names; ``sample_steps`` as in ``sample``) runs once, on the canvas, with canvas-level noise
        (kd_tiles_fuse_update_hist2; without a second history for all but the third-order names).  There is no inpainting, no
        resampling and no order among the tiles, and the canvas does not depend on ``tile_batch`` beyond the rounding of
        plans of different batch sizes.

        ``cond_images`` [N, Cc, h, w] holds one image per tile (row-major over the present slots); ``text_embeds`` /
        ``text_masks`` hold ONE row, given to every tile; ``seed`` is an int (None: drawn from torch's generator);
        ``noise_fn(tag, shape)`` injects the draws: ``("init", stage)`` and ``("lowres", stage)`` of the canvas shape, and
        ``("step", stage, k, 0)`` only for the steps whose update adds noise.  The low-res conditioning of a stage is the
        previous canvas resized to this stage's canvas and augmented ONCE, so overlapping tiles see the same conditioning on
        shared pixels; ``start_image_or_video`` is a canvas.  Returns the canvas [1, C, Hc, Wc] in [0, 1] (a list of the
        stages' canvases with ``return_all_unet_outputs``); pixels that no tile covers are 0.

        Three arguments carry a stage to the sizes of a magnification level (a 40960 x 40960 canvas of 1024-pixel tiles);
        a call without them keeps its bits.  ``streamed=True``: the low-res conditioning tiles are cut
        straight out of the previous canvas (kd_tiles_gather_lowres: no resized, augmented canvas is built) and the stage
        ends in one pass into a zero canvas (kd_tiles_finalize_rows: no host mask, no temporaries) - bit-equal to
        ``streamed=False``.  ``cond_crops``: a ``TileCondCrops`` in the place of ``cond_images`` - the tiles'
        conditioning images are windows of one image, cut per chunk by kd_tiles_cond_gather, bit-equal to
        ``cond_images=cond_images_for_grid(...)``.  ``into=(canvas, oy, ox)`` (needs ``streamed``): the last sampled stage
        writes its covered pixels into ``canvas`` [1, C, Ho, Wo] (fp32, contiguous, on the device) at row ``oy``, column
        ``ox`` (multiples of 4) in place, leaves every other pixel of it alone and returns it.

        A canvas that keeps known pixels or starts from an image (canvas-level; the per-tile ``inpaint_*`` / ``init_images``
        / ``skip_steps`` of ``sample`` stay refused - a canvas holds no image per tile).  ``known_image`` [1, C, Hk, Wk] in
        [0, 1], ``known_mask`` [Hk, Wk] (non-zero = keep) and ``known_resample_times = R`` (``normalize_known``): RePaint
        mixing on the canvas.  Every stage reads both at its own canvas size (nearest); before each of the R resample
        slots of step k the known pixels become ``alpha_k (2 kn - 1) + sigma_k z``, after every slot but a step's last the
        canvas is re-noised to step k (``rn_a``, ``rn_b``), and the result holds the known image's values, copied.  The
        draws are canvas-level like x_T: ``noise_fn`` tags ``("inpaint" | "renoise" | "step", stage, k, r)``, r counting
        down from R - 1, or Philox purposes 2, 3 and 1 at iteration ``k R + (R - 1 - r)`` - ``sample``'s, so a 1 x 1 lattice
        draws what ``sample(batch_size=1, inpaint_images=...)`` draws.  2M and 3M keep the fused estimate of a step's last
        slot as their history (3M: of the last two steps); a self-conditioned UNet carries the previous slot's.  ``init_canvas`` (one image, or one per UNet)
        and ``init_skip_steps`` (``normalize_init_canvas``; counted in ``sample_steps`` where given): the stage starts from
        ``z + nearest(2 init - 1)`` and walks steps ``skip .. T - 1``; a step keeps its index - table row, streams, tags -
        and 2M is first order on the first step walked.  Every stage, with or without them, starts through kd_tiles_start,
        steps through kd_tiles_fuse_update_hist2 (update, re-noise and the next slot's mix in the one canvas pass) and ends
        through kd_tiles_finalize_rows (``streamed``) or the same clamp and paste in torch; a call without them passes
        NULL sources and keeps its bits.  ``known_image`` may be a window of the ``into`` canvas itself.

        ``devices``: a sequence of CUDA devices, one per SHARD of the canvas (``normalize_devices``, ``normalize_shards``);
        None or one device is one shard that holds the whole lattice.  The lattice rows are dealt over the shards in
        contiguous bands balanced by present tiles; every shard denoises the tiles of its band with plans of its own on
        its device, the overlap strips of the boundary tiles' estimates cross per step (kd_tiles_rows_copy), and the
        canvas comes back on ``devices[0]`` (where ``into`` must live) - the canvas of one shard bit for bit
        wherever the chunks of both calls have one batch size, and within the rounding of plans of different batch
        sizes otherwise.  A device may repeat (``[d, d]``: two shards on one GPU, each with its own plans).  One process,
        one host thread, no collectives; ``noise_fn`` is refused with more than one shard."""
        for name, v in dict(inpaint_images=inpaint_images, inpaint_masks=inpaint_masks,
                            inpaint_resample_times=inpaint_resample_times).items():
            if exists(v):
                raise NotImplementedError(f"sample_tiled({name}=...): a fused canvas holds no inpainting - its tiles are "
                                          "denoised together")
        for name, v in dict(init_images=init_images, skip_steps=skip_steps).items():
            if exists(v):
                raise NotImplementedError(f"sample_tiled({name}=...) is not provided: a canvas starts from noise at step 0")
        import numbers

        if exists(seed) and (not isinstance(seed, numbers.Integral) or isinstance(seed, bool)):
            raise ValueError(f"sample_tiled(seed=...) takes one int for the canvas (per-image seed lists belong to sample()), "
                             f"got {type(seed).__name__}")
        if not isinstance(tile_batch, numbers.Integral) or isinstance(tile_batch, bool) or int(tile_batch) < 1:
            raise ValueError(f"tile_batch must be an int >= 1, got {tile_batch!r}")
        n = len(self.unets)
        solvers = self._solver_args(sampler, sampler_eta, sample_steps)
        tiling = normalize_tiling(self.image_sizes, grid, overlap, present, tile_weights)
        n_tiles = len(tiling[0]["origins"])
        devices = normalize_devices(devices, noise_fn)
        sharding = normalize_shards(tiling, len(devices) if exists(devices) else 1)
        if exists(devices):
            device = devices[0]
        if exists(cond_images) and (cond_images.dim() != 4 or cond_images.shape[0] != n_tiles):
            raise ValueError(f"cond_images must be [tiles {n_tiles}, Cc, h, w], one per present tile, got {tuple(cond_images.shape)}")
        if exists(text_embeds) and (text_embeds.dim() != 3 or text_embeds.shape[0] != 1):
            raise ValueError(f"text_embeds must hold one row [1, L, D] for the whole canvas, got {tuple(text_embeds.shape)}")
        if not 1 <= start_at_unet_number <= n:
            raise ValueError(f"start_at_unet_number={start_at_unet_number} is outside 1 .. {n}")
        last = stop_at_unet_number if exists(stop_at_unet_number) and start_at_unet_number <= stop_at_unet_number <= n else n
        crops = None
        if exists(cond_crops):
            if exists(cond_images):
                raise ValueError("sample_tiled takes cond_images or cond_crops, one of them: cond_crops describes the same "
                                 "images as windows of one image")
            if not isinstance(cond_crops, TileCondCrops):
                raise ValueError(f"cond_crops must be a TileCondCrops, got {type(cond_crops).__name__}")
            crops = (cond_crops,) + cond_crops.checked(n_tiles)
        into = normalize_into(into, streamed=streamed, channels=self.channels, Hc=tiling[last - 1]["Hc"], Wc=tiling[last - 1]["Wc"],
                              unet=last)
        known = normalize_known(known_image, known_mask, known_resample_times, channels=self.channels)
        starts = normalize_init_canvas(init_canvas, init_skip_steps,
                                       steps=[default(st, T) for (_, _, st), T in zip(solvers, self._num_steps())],
                                       channels=self.channels, start_at_unet_number=start_at_unet_number,
                                       stop_at_unet_number=stop_at_unet_number)
        device, text_masks, cond_images, seed, cond_scale, lowres_level, canvas = self._sampling_setup(
            device, text_embeds, text_masks, cond_images, seed, cond_scale, lowres_sample_noise_level, start_at_unet_number,
            start_image_or_video)
        if exists(canvas):
            g = tiling[start_at_unet_number - 2]
            canvas = F.interpolate(canvas, (g["Hc"], g["Wc"]), mode="nearest")
        if exists(devices) and len(devices) > 1:   # every shard's device by its index: two spellings of one device are one device
            devices = [d if exists(d.index) else torch.device("cuda", torch.cuda.current_device()) for d in devices]
            if any(d.index >= torch.cuda.device_count() for d in devices):
                raise ValueError(f"devices={devices} name a device this process does not see ({torch.cuda.device_count()} visible)")
            device = devices[0]
            if exists(into) and into[0].device != device:   # before any forward: the stage ends on devices[0]
                raise ValueError(f"into: with devices=... the canvas must live on devices[0] = {device}, got {into[0].device}")
        else:
            devices = [device]
        outputs = []
        for num, unet, sched, obj, dyn, cs, solver in self._stages(solvers, cond_scale, start_at_unet_number,
                                                                  stop_at_unet_number):
            canvas = self._tiled_stage(unet, num, tiling[num - 1], sched, obj, dyn, device, canvas, cond_images, lowres_level,
                                       noise_fn, int(seed), use_graph, int(tile_batch), text_embeds=text_embeds,
                                       text_masks=text_masks, cond_scale=cs, solver=solver, streamed=bool(streamed),
                                       crops=crops, into=into if num == last else None, known=known, start=starts[num - 1],
                                       shards=(devices, sharding[num - 1]))
            outputs.append(canvas)
        return outputs if return_all_unet_outputs else outputs[-1]

    def _tiled_stage(self, unet, stage, geo, sched, objective, dynamic_threshold, device, prev_canvas, cond_images,
                     lowres_level, noise_fn, seed, use_graph, tile_batch, text_embeds=None, text_masks=None, cond_scale=1.0,
                     solver=("ddpm", 0.0), streamed=False, crops=None, into=None, known=(None, None, 1), start=(None, 0),
                     shards=None, _poison_halo=False):
        """One stage of sample_tiled, driven through imagen_pytorch/_canvas.py: a _CanvasStage (what every shard reads), one
        _CanvasShard per entry of `shards = (devices, normalize_shards' dict of this stage)` - one shard is the whole
        lattice on its device - and one _StripLink per pair of shards that trade strips.  Every shard starts its canvas;
        per resample slot every shard denoises its own tiles, the links trade, every shard takes the canvas step; at the
        end every shard finishes the canvas rows it owns, onto devices[0] (`device`): `streamed` through
        kd_tiles_finalize_rows into `into = (canvas, oy, ox)` or a zero canvas, else in torch.
        `_poison_halo` is for tests alone (no public call passes it): _CanvasShard.poison_halo before each slot."""
        from . import _canvas

        devs, layout = shards
        st = _canvas._CanvasStage(self, unet, stage, geo, sched, objective, dynamic_threshold, prev_canvas, cond_images,
                                  lowres_level, noise_fn, seed, use_graph, tile_batch, text_embeds, text_masks, cond_scale, solver,
                                  streamed, crops, known, start)
        on, parts = torch.cuda.device, []
        for num, (dev, lay) in enumerate(zip(devs, layout["shards"])):
            with on(dev):
                parts.append(_canvas._CanvasShard(st, num, dev, lay))
                parts[-1].start()
        links = [_canvas._StripLink(st, parts[e["src"]], parts[e["dst"]], e["items"]) for e in layout["exchange"]]
        for i, (k, j) in enumerate(st.slots):
            for sh in parts:
                with on(sh.dev):
                    if _poison_halo:
                        sh.poison_halo()
                    sh.denoise(i, k)
            for ln in links:
                ln.trade()
            for sh in parts:
                with on(sh.dev):
                    sh.step(i, k, j)
        head, bands, covered = parts[0], [], None if streamed else st.covered()
        if streamed:   # in place: the covered pixels into `into` (or a zero canvas), nothing else touched
            with on(head.dev):
                out, oy, ox = into if exists(into) else (torch.zeros(st.shape, device=head.dev, dtype=torch.float32), 0, 0)
            assert out.device == head.x.device, f"into: the canvas lives on {out.device}, the stage runs on {head.x.device}"
        for sh in parts:
            with on(sh.dev):
                bands.append(sh.finish_rows(out, oy, ox, sh is head) if streamed else sh.finish_torch(covered))
        with on(head.dev):
            return out if streamed else bands[0] if len(bands) == 1 else torch.cat([b.to(head.dev) for b in bands], dim=2)

    def _num_steps(self):
        """Schedule steps of every UNet's sampler: what skip_steps is checked against."""
        return [s.num_timesteps for s in self.noise_schedulers]

    def _solver_args(self, sampler, sampler_eta, sample_steps):
        """sample()'s sampler / sampler_eta / sample_steps per UNet: [(name, eta, steps or None)]."""
        return normalize_sampler(sampler, sampler_eta, sample_steps, len(self.unets))

    def _start_scale(self, stage):
        """x_T = scale * N(0,1) (+ the init image): 1 for the DDPM sampler."""
        return 1.0

    def _stage_loop(self, lib, h, args, img, *, stage, sched, objective, has_inpaint, R, stack, trace, skip=0,
                    self_cond=False, solver=("ddpm", 0.0)):
        """The sampler proper of one stage, in place on `img` (x_T in, the unnormalised sample out): the DDPM loop of
        p_sample_loop over the steps skip .. T - 1, its update the ancestral one or that of `solver` = (name, eta).
        `stack(kind, T)` gives the injected noise of a kind (None: on-device Philox).  A self-conditioned plan starts step
        `skip` > 0 from zeros, as step 0 does by itself."""
        name, eta = solver
        sc = _StepSchedule(sched.step_tables(), name, eta, skip)
        args.objective = _OBJECTIVES[objective]
        if exists(stack):
            if name == "ddpm" or sc.draws:   # DDIM(0), 2M and 3M draw nothing in the step
                args.d_noise_step = stack("step", sc.T)
            if has_inpaint:
                args.d_noise_inpaint = stack("inpaint", sc.T)
                if R > 1:
                    args.d_noise_renoise = stack("renoise", sc.T)
        _walk(lib, sc, h, args, img, skip=skip, trace=trace, self_cond=self_cond)


# ============================================================================ ElucidatedImagen (EDM)
EDM_HPARAMS = ("num_sample_steps", "sigma_min", "sigma_max", "sigma_data", "rho", "P_mean", "P_std", "S_churn", "S_tmin",
               "S_tmax", "S_noise")


def edm_step_tables(num_sample_steps=32, sigma_min=0.002, sigma_max=80, sigma_data=0.5, rho=7, S_churn=80, S_tmin=0.05,
                    S_tmax=50, S_noise=1.003, **_):
    """Host scalars of imagen-pytorch 1.18.x's ElucidatedImagen sampler for one UNet (the arrays of kd_edm_schedule_t):
    the Karras schedule and churn in fp32 torch ops, the step's sigmas as python floats (`.item()`), hence sigma_hat,
    the churn scale and the step sizes in double, and the preconditioning c_* of sigma_hat / sigma_next as fp32 torch
    ops on the rounded sigmas - the library's op order throughout."""
    N = num_sample_steps
    inv_rho = 1 / rho
    steps = torch.arange(N, dtype=torch.float32)
    sigmas = (sigma_max ** inv_rho + steps / (N - 1) * (sigma_min ** inv_rho - sigma_max ** inv_rho)) ** rho
    sigmas = F.pad(sigmas, (0, 1), value=0.0)
    gammas = torch.where((sigmas >= S_tmin) & (sigmas <= S_tmax), min(S_churn / N, math.sqrt(2) - 1), 0.0)
    sd = sigma_data
    c_skip = lambda sg: (sd ** 2) / (sg ** 2 + sd ** 2)
    c_out = lambda sg: sg * sd * (sd ** 2 + sg ** 2) ** -0.5
    c_in = lambda sg: 1 * (sg ** 2 + sd ** 2) ** -0.5
    c_noise = lambda sg: _log(sg, eps=1e-20) * 0.25
    rows = {n: [] for n in ("sigma", "sigma_hat", "sigma_next", "churn", "euler_step", "heun_step", "renoise")}
    for sigma, sigma_next, gamma in zip(sigmas[:-1].tolist(), sigmas[1:].tolist(), gammas[:-1].tolist()):
        sigma_hat = sigma + gamma * sigma
        for n, v in (("sigma", sigma), ("sigma_hat", sigma_hat), ("sigma_next", sigma_next),
                     ("churn", math.sqrt(sigma_hat ** 2 - sigma ** 2)), ("euler_step", sigma_next - sigma_hat),
                     ("heun_step", 0.5 * (sigma_next - sigma_hat)), ("renoise", sigma - sigma_next)):
            rows[n].append(v)
    out = {n: torch.tensor(v, dtype=torch.float64).to(torch.float32) for n, v in rows.items()}
    for tag, sg in (("hat", out["sigma_hat"]), ("next", out["sigma_next"])):
        out[f"c_in_{tag}"], out[f"c_skip_{tag}"] = c_in(sg), c_skip(sg)
        out[f"c_out_{tag}"], out[f"c_noise_{tag}"] = c_out(sg), c_noise(sg)
    out["init_sigma"] = sigmas[0]
    return {n: v.to(torch.float32).contiguous() for n, v in out.items()}


class ElucidatedImagen(Imagen):
    """imagen-pytorch 1.18.x's ElucidatedImagen for sampling: the UNets, checkpoint layout, low-res augmentation,
    guidance, thresholding and inpainting inputs of `Imagen` (state_dict keys equal), the per-stage loop replaced by
    the EDM stochastic Heun sampler of the engine (kd_edm_sample_loop).  Constructor as train.py:97-110 writes it;
    the per-UNet hyperparameters are cast to the number of UNets.  Training (`forward`) is not provided."""

    def __init__(self, unets, *, image_sizes, text_encoder_name=None, text_embed_dim=None, channels=3, cond_drop_prob=0.1,
                 random_crop_sizes=None, lowres_noise_schedule="linear", lowres_sample_noise_level=0.2,
                 per_sample_random_aug_noise_level=False, condition_on_text=True, auto_normalize_img=True,
                 dynamic_thresholding=True, dynamic_thresholding_percentile=0.95, only_train_unet_number=None,
                 num_sample_steps=32, sigma_min=0.002, sigma_max=80, sigma_data=0.5, rho=7, P_mean=-1.2, P_std=1.2,
                 S_churn=80, S_tmin=0.05, S_tmax=50, S_noise=1.003, **ignored_training_kwargs):
        super().__init__(unets, image_sizes=image_sizes, text_encoder_name=text_encoder_name, text_embed_dim=text_embed_dim,
                         channels=channels, cond_drop_prob=cond_drop_prob, random_crop_sizes=random_crop_sizes,
                         lowres_noise_schedule=lowres_noise_schedule, lowres_sample_noise_level=lowres_sample_noise_level,
                         per_sample_random_aug_noise_level=per_sample_random_aug_noise_level,
                         condition_on_text=condition_on_text, auto_normalize_img=auto_normalize_img,
                         dynamic_thresholding=dynamic_thresholding,
                         dynamic_thresholding_percentile=dynamic_thresholding_percentile,
                         only_train_unet_number=only_train_unet_number, **ignored_training_kwargs)
        n = len(self.unets)
        vals = dict(num_sample_steps=num_sample_steps, sigma_min=sigma_min, sigma_max=sigma_max, sigma_data=sigma_data,
                    rho=rho, P_mean=P_mean, P_std=P_std, S_churn=S_churn, S_tmin=S_tmin, S_tmax=S_tmax, S_noise=S_noise)
        cast = {k: cast_tuple(v, n) for k, v in vals.items()}
        self.hparams = [{k: cast[k][i] for k in EDM_HPARAMS} for i in range(n)]   # per UNet

    def step_tables(self, unet_number):
        """Host tables of UNet `unet_number`'s sampler (edm_step_tables)."""
        return edm_step_tables(**self.hparams[unet_number - 1])

    def _num_steps(self):
        return [hp["num_sample_steps"] for hp in self.hparams]

    def _solver_args(self, sampler, sampler_eta, sample_steps):
        """ElucidatedImagen has its own sampler and step count (num_sample_steps): the DDPM solvers do not apply."""
        if exists(sampler) or exists(sample_steps) or sampler_eta not in (0, 0.0, None):
            raise ValueError("ElucidatedImagen.sample takes no sampler / sampler_eta / sample_steps: it samples with the EDM "
                             "Heun sampler on num_sample_steps steps")
        return [("ddpm", 0.0, None)] * len(self.unets)

    def _start_scale(self, stage):
        """x = sigma_0 * N(0,1) (+ the init image): the first sigma of the full schedule, whatever skip_steps is; a python
        float of the fp32 value, so the kernel's product is the library's fp32 tensor product."""
        return float(self.step_tables(stage)["init_sigma"])

    def sample_tiled(self, *args, **kwargs):
        raise NotImplementedError("ElucidatedImagen.sample_tiled: fused-tile canvas sampling runs the DDPM-trained samplers of "
                                  "Imagen (ancestral, DDIM, DPM-Solver++); the EDM Heun sampler has no canvas step")

    def _stage_loop(self, lib, h, args, img, *, stage, sched, objective, has_inpaint, R, stack, trace, skip=0,
                    self_cond=False, solver=None):
        """one_unet_sample of the library's ElucidatedImagen on the engine, on x = sigma_0 * N(0,1) (+ the init image) as
        kd_sample_start wrote it: per step skip .. N - 1 churn, a preconditioned forward and the Euler step, and (not on
        the last step) a second forward and the Heun correction; RePaint re-noise between resamples.  Noise tags
        ("churn" | "renoise", stage, k, r)."""
        sc = _StepSchedule.edm(self.step_tables(stage), self.hparams[stage - 1]["S_noise"])
        if exists(stack):
            args.d_noise_step = stack("churn", sc.T)
            if has_inpaint and R > 1:
                args.d_noise_renoise = stack("renoise", sc.T)
        _walk(lib, sc, h, args, img, skip=skip, trace=trace, self_cond=self_cond)
