"""The UNet's scalar constructor options without a GPU: every configuration tests/test_unet_options_gpu.py runs on the engine
constructs, strict-loads the oracle's state dict and has a finite oracle forward; and what the engine cannot plan is refused
by Unet.__init__ with the kwarg's name in the message, not by a launcher's precondition at the first forward."""
import pytest
import torch

import unet_options_cases as OC


def _product(**kw):
    import imagen_pytorch as ip

    return ip.Unet(**kw)


@pytest.mark.parametrize("name", list(OC.ALL))
def test_case_constructs_loads_strictly_and_the_oracle_forward_is_finite(name):
    case = OC.ALL[name]
    ou = OC.oracle_unet(name)
    pu = _product(**ou._locals)
    missing, unexpected = pu.load_state_dict(ou.state_dict(), strict=True)
    assert not missing and not unexpected
    got, want = pu.state_dict(), ou.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    for k, v in case["kw"].items():   # the option reached the plan's description, not only the module tree
        plan_key = {"learned_sinu_pos_emb_dim": "sinu_dim", "resnet_groups": "groups", "use_global_context_attn": "use_gca"}.get(k, k)
        if plan_key in pu._plan and k != "num_resnet_blocks":
            assert pu._plan[plan_key] == v, (k, pu._plan[plan_key])
    x, t, kw = OC.inputs(ou, case)
    with torch.no_grad():
        y = ou(x, t, **kw)
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    assert float(y.abs().max()) > 1e-3   # (randomize_ gives the zero-initialised final conv weights)


@pytest.mark.parametrize("which", ["base", "sr"])
def test_cascade_unets_construct_and_load(which):
    import self_cond_ref as SR
    import helpers as H

    kw = dict(OC.BASE) if which == "base" else dict(OC.SR2, lowres_cond=True)
    ou = H.randomize_(SR.Unet(**kw, cond_on_text=False, text_embed_dim=None), 1)
    _product(**ou._locals).load_state_dict(ou.state_dict(), strict=True)


@pytest.mark.parametrize("name", list(OC.REFUSED))
def test_what_the_engine_cannot_plan_is_refused_at_construction(name):
    over, words = OC.REFUSED[name]
    kw = {**OC.NARROW, "cond_on_text": False, "text_embed_dim": None, **over}
    with pytest.raises(NotImplementedError) as ei:
        _product(**kw)
    msg = str(ei.value)
    assert all(w in msg for w in words), msg


def test_refusals_leave_their_neighbours_alone():
    """The values next to each refused one construct: the un-pooled text switch on a UNet without text conditioning (the
    library builds no attn_pool then, and the engine plans no text sub-plan), group widths of exactly 4 channels, the
    PerceiverResampler's whole position table, a per-level resnet_groups tuple of equal entries."""
    plain = dict(OC.NARROW, cond_on_text=False, text_embed_dim=None)
    u = _product(**plain, attn_pool_text=False)
    assert u.attn_pool is None and u.n_text_tokens == 0
    assert _product(**plain, resnet_groups=8).final_res_block.block1.groupnorm.num_groups == 8
    assert _product(**{**plain, "dim": 64}, resnet_groups=16).mid_block1.block2.groupnorm.num_groups == 16
    assert _product(**{**plain, "dim": 128}, resnet_groups=32).mid_block1.block1.groupnorm.num_groups == 32
    assert _product(**plain, resnet_groups=(4, 4, 4))._plan["groups"] == 4
    assert _product(**OC.NARROW, cond_on_text=True, text_embed_dim=3, max_text_len=512).n_text_tokens == 36
    assert _product(**OC.NARROW, cond_on_text=True, text_embed_dim=3, attn_pool_num_latents=8).n_text_tokens == 12
    with pytest.raises(AssertionError, match="per-level resnet_groups"):   # stays refused as before
        _product(**plain, resnet_groups=(8, 4, 8))


def test_group_widths_come_from_where_the_builder_normalises():
    """Every GroupNorm module of a constructed UNet outside the UpsampleCombiner has a width the constructor's check covered:
    whole groups of 4 n channels.  (The combiner's Blocks keep 8 groups whatever resnet_groups says.)"""
    from torch import nn

    for over in (dict(resnet_groups=4), dict(resnet_groups=2, memory_efficient=True, init_conv_to_final_conv_residual=True),
                 dict(resnet_groups=4, combine_upsample_fmaps=True, init_conv_to_final_conv_residual=True),
                 dict(resnet_groups=2, dim_mults=(1, 1, 3), num_resnet_blocks=(1, 3, 2))):
        u = _product(**{**OC.NARROW, "cond_on_text": False, "text_embed_dim": None, **over})
        widths = set()
        for n, m in u.named_modules():
            if isinstance(m, nn.GroupNorm):
                g = 8 if n.startswith("upsample_combiner") else over["resnet_groups"]
                assert m.num_groups == g and m.num_channels % (4 * g) == 0, (n, m.num_groups, m.num_channels)
                if g != 8:
                    widths.add(m.num_channels)
        assert widths == set(u._gn_widths), (sorted(widths), u._gn_widths)   # the check saw exactly the widths that exist
