"""TEST INFRASTRUCTURE ONLY: the UNet configurations of tests/test_unet_options.py (CPU: constructor, strict load, oracle
forward) and tests/test_unet_options_gpu.py (the same models on the engine against the oracle).  No product imports.

The "scalar" constructor options - num_time_tokens, learned_sinu_pos_emb_dim, resnet_groups, ff_mult, attn_heads,
attend_at_middle, use_global_context_attn, cond_dim, attn_pool_num_latents, max_text_len - each at values other than the ones
every other suite runs (GroupNorm(8), ff_mult 2, two time tokens, a 17-wide sinusoidal embedding, GlobalContext and mid
attention on), one case per value.  The oracle is tests/self_cond_ref.Unet: oracle/imagen_ref.Unet plus `self_cond`.
"""
from __future__ import annotations

import torch

import helpers as H
import self_cond_ref as SR
import trajectory_ref as TR

NARROW = dict(dim=32, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, True, True),
              layer_cross_attns=(False, True, True))
TEXT = dict(NARROW, cond_dim=64, text_embed_dim=3)
EVERYTHING = dict(resnet_groups=4, ff_mult=1.5, attn_heads=3, learned_sinu_pos_emb_dim=8, num_time_tokens=3,
                  use_global_context_attn=False, attend_at_middle=False, lowres_cond=True, self_cond=True)


def _case(kw, B=2, S=32, base=NARROW, text=None, seed=0):
    """text: None, or dict(L=tokens given, keep=None | per-sample number of leading tokens the text_mask keeps)."""
    return dict(kw=kw, B=B, S=S, base=base, text=text, seed=seed)


# ---- a. the narrow model: dim 32, 32 px
FORWARD = {
    "time_tokens_1": _case(dict(num_time_tokens=1)),
    "time_tokens_4": _case(dict(num_time_tokens=4), B=3),
    "time_tokens_4_lowres": _case(dict(num_time_tokens=4, lowres_cond=True)),        # 8 time tokens
    "sinu_8": _case(dict(learned_sinu_pos_emb_dim=8)),                               # first time Linear: K = 9
    "sinu_32": _case(dict(learned_sinu_pos_emb_dim=32), B=3),                        # K = 33
    "groups_4": _case(dict(resnet_groups=4)),      # groups of 8 channels at level 0 (statistics pass), 16 n below (folded)
    "groups_2": _case(dict(resnet_groups=2), B=3),                                   # groups of 16 at level 0
    "ff_mult_1": _case(dict(ff_mult=1.0)),
    "ff_mult_4": _case(dict(ff_mult=4.0)),
    "ff_mult_1.5": _case(dict(ff_mult=1.5), B=3),                                    # hidden 96 / 192: no multiple of 128
    "heads_2": _case(dict(attn_heads=2)),
    "heads_16": _case(dict(attn_heads=16)),
    "heads_3": _case(dict(attn_heads=3), B=3),                                       # q | kv projection of 192 + 128 columns
    "no_mid_attn": _case(dict(attend_at_middle=False)),
    "no_gca": _case(dict(use_global_context_attn=False)),
    "no_gca_mem_eff": _case(dict(use_global_context_attn=False, memory_efficient=True, init_conv_to_final_conv_residual=True)),
    "mults_123": _case(dict(dim_mults=(1, 2, 3))),
    "mults_113": _case(dict(dim_mults=(1, 1, 3))),                                   # a level with dim_in == dim_out
    "mults_113_no_gca": _case(dict(dim_mults=(1, 1, 3), use_global_context_attn=False), B=3),
    "cond_dim_48": _case(dict(cond_dim=48)),
    "resnet_blocks_132": _case(dict(num_resnet_blocks=(1, 3, 2))),
    "everything": _case(EVERYTHING, B=3),
    # text conditioning: cond_dim 64, text_embed_dim 3
    "text_latents_8": _case(dict(attn_pool_num_latents=8), base=TEXT, text=dict(L=2, keep=None)),
    "text_len16_L5": _case(dict(max_text_len=16), base=TEXT, text=dict(L=5, keep=None)),
    "text_len16_L16": _case(dict(max_text_len=16), base=TEXT, text=dict(L=16, keep=None), B=3),
    "text_len16_L20": _case(dict(max_text_len=16), base=TEXT, text=dict(L=20, keep=None)),   # the library truncates to 16
    "text_len16_L5_masked": _case(dict(max_text_len=16), base=TEXT, text=dict(L=5, keep=(3, 5, 1)), B=3),
    "text_time_tokens_4": _case(dict(num_time_tokens=4), base=TEXT, text=dict(L=2, keep=None)),   # text rows behind 4 time rows
}

# ---- b. the smallest model on which the default fast plan engages: dim 128, 64 px, batch 4 (trajectory_ref.MODEL_A)
FAST = {
    "fast_groups_32": _case(dict(resnet_groups=32), B=4, S=64, base=TR.MODEL_A),
    "fast_groups_16": _case(dict(resnet_groups=16), B=4, S=64, base=TR.MODEL_A),
    "fast_groups_4": _case(dict(resnet_groups=4), B=4, S=64, base=TR.MODEL_A),
    "fast_no_gca": _case(dict(use_global_context_attn=False), B=4, S=64, base=TR.MODEL_A),
    "fast_ff4_heads4": _case(dict(ff_mult=4.0, attn_heads=4), B=4, S=64, base=TR.MODEL_A),
    "fast_time_tokens_4_lowres": _case(dict(num_time_tokens=4, lowres_cond=True), B=4, S=64, base=TR.MODEL_A),
}
ALL = {**FORWARD, **FAST}

# ---- c. the sampled cascade 32 -> 64
BASE = dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True), layer_cross_attns=(False, True),
            resnet_groups=4, ff_mult=1.5, attn_heads=3, learned_sinu_pos_emb_dim=8, num_time_tokens=3,
            use_global_context_attn=False)
SR2 = dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, memory_efficient=True, layer_attns=(False, True),
           layer_cross_attns=(False, True), init_conv_to_final_conv_residual=True, attend_at_middle=False, resnet_groups=2)
DDPM_KW = dict(noise_schedules=("linear", "cosine"), dynamic_thresholding_percentile=0.9, pred_objectives=("noise", "v"),
               timesteps=(4, 4))

# what the engine cannot plan and Unet.__init__ refuses: (kwargs over NARROW, words the message must contain)
REFUSED = {
    "attn_pool_text_off": (dict(cond_on_text=True, text_embed_dim=3, attn_pool_text=False), ("attn_pool_text",)),
    "groups_16_dim_32": (dict(resnet_groups=16), ("resnet_groups", "32")),            # 32 / 16 = 2 channels per group
    "groups_32_dim_32": (dict(resnet_groups=32), ("resnet_groups", "32")),
    "groups_12": (dict(resnet_groups=12), ("resnet_groups", "32")),                   # no divisor of 32 at all
    "groups_3_mults_123": (dict(resnet_groups=3, dim_mults=(1, 2, 3)), ("resnet_groups", "32")),   # 96 / 3 = 32 fits, 32 / 3 not
    "groups_0": (dict(resnet_groups=0), ("resnet_groups",)),
    "sinu_odd": (dict(learned_sinu_pos_emb_dim=9), ("learned_sinu_pos_emb_dim",)),
    "ff_mult_third": (dict(ff_mult=1.3), ("ff_mult",)),
    "max_text_len_600": (dict(cond_on_text=True, text_embed_dim=3, max_text_len=600), ("max_text_len",)),
    "dim_48": (dict(dim=48), ("dim=48",)),
}


def oracle_unet(name):
    c = ALL[name]
    tk = dict(cond_on_text=True) if c["text"] else dict(cond_on_text=False, text_embed_dim=None)
    return H.randomize_(SR.Unet(**{**c["base"], **tk, **c["kw"]}), 40 + c["seed"] + sum(map(ord, name)) % 50).eval()


def inputs(ou, case, seed=3):
    """x, log-SNR and the keyword inputs of one forward of `ou` under `case`."""
    B, S = case["B"], case["S"]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, S, S, generator=g)
    t = torch.randn(B, generator=g) * 3
    kw = {}
    if ou.lowres_cond:
        kw.update(lowres_cond_img=torch.randn(B, 3, S, S, generator=g), lowres_noise_times=torch.full((B,), 1.5))
    if ou.self_cond:
        kw["self_cond"] = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    if case["text"]:
        L, keep = case["text"]["L"], case["text"]["keep"]
        kw["text_embeds"] = torch.randn(B, L, 3, generator=g)
        if keep is not None:   # trailing tokens dropped, a different number per sample
            kw["text_mask"] = torch.arange(L)[None, :] < torch.tensor(keep[:B])[:, None]
    return x, t, kw
