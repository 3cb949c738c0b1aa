"""Every plan Builder::build() can emit, pinned to what the plan builder gave before build() was split into its stages
(tests/golden/plan_pins.json, written by tests/golden/make_plan_pins.py on the MI355X from the library of the commit
before the split): per case the number of launches and of conditioning launches, kd_unet_hbm_bytes (workspace, cond
region and packed weights), the sha256 of the profile's (label, MACs, matrix-core MACs) rows, the sha256 of one forward's
output bytes and, for one case per family, the label list itself so that a mismatch can be diffed.

The golden holds results only.  Weights (helpers.randomize_) and inputs (helpers.unet_inputs) are rebuilt here from the
seeds; every field must be equal, no tolerance.  The models are unet_options_cases.NARROW (dim 32 at 32 px) and
trajectory_ref.MODEL_A (dim 128 at 64 px, the smallest on which the default fast plan engages) with one switch or one
combination of switches each; make_plan_pins.py lists which case covers which branch of build()."""
import hashlib
import json
import pathlib

import pytest
import torch

import helpers as H
import trajectory_ref as TR
import unet_options_cases as UC

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).parent / "golden" / "plan_pins.json"
RES = dict(init_conv_to_final_conv_residual=True)
MEM = dict(memory_efficient=True)
COMBINE = dict(combine_upsample_fmaps=True)
NO_FINAL = dict(final_resnet_block=False)
LINEAR = dict(layer_attns=(False, False, True), layer_cross_attns=(False, False, True), use_linear_attn=True,
              use_linear_cross_attn=(False, True, False))


def _case(kw=None, B=2, S=32, base=UC.NARROW, text=False, plan=None, labels=False):
    """kw: constructor arguments over `base`; text: text conditioning (cond_dim 64, 2 tokens of width 3); plan: attributes set
    on the product UNet before its plan is built; labels: the golden keeps the case's label list."""
    return dict(kw=dict(kw or {}), B=B, S=S, base=base, text=text, plan=dict(plan or {}), labels=labels)


CASES = {
    # ---- the baseline and its batches
    "narrow_b2": _case(labels=True),
    "narrow_b1": _case(B=1),
    "narrow_b3": _case(B=3),
    # ---- the walk
    "no_gca": _case(dict(use_global_context_attn=False)),
    "mem_eff": _case(MEM),
    "mem_eff_residual": _case(dict(**MEM, **RES), labels=True),
    "residual": _case(RES),
    "no_gca_mem_eff_residual": _case(dict(use_global_context_attn=False, **MEM, **RES)),
    "no_gca_residual": _case(dict(use_global_context_attn=False, **RES)),
    "linear_attn": _case(LINEAR, labels=True),
    "linear_attn_mem_eff": _case(dict(LINEAR, **MEM)),
    "attn_depth_2_3": _case(dict(layer_attns_depth=(1, 2, 3))),
    "blocks_132": _case(dict(num_resnet_blocks=(1, 3, 2))),
    "blocks_3_mem_eff": _case(dict(num_resnet_blocks=3, **MEM)),
    "blocks_011": _case(dict(num_resnet_blocks=(0, 1, 1))),
    "blocks_0_no_gca_mem_eff": _case(dict(num_resnet_blocks=0, use_global_context_attn=False, **MEM)),
    "no_mid_attn": _case(dict(attend_at_middle=False)),
    "residual_attention_mid": _case(dict(mid_attn_form="residual_attention")),
    "no_skip_scale": _case(dict(scale_skip_connection=False)),
    "conv4x4_down": _case(dict(downsample_form="conv4x4")),
    "conv4x4_down_mem_eff": _case(dict(downsample_form="conv4x4", **MEM)),
    "cross_embed_down": _case(dict(cross_embed_downsample=True)),
    "cross_embed_down_mem_eff": _case(dict(cross_embed_downsample=True, **MEM)),
    "nearest_up": _case(dict(pixel_shuffle_upsample=False)),
    "nearest_up_mem_eff_residual": _case(dict(pixel_shuffle_upsample=False, **MEM, **RES)),
    # ---- the UpsampleCombiner
    "combine": _case(COMBINE, labels=True),
    "combine_mem_eff": _case(dict(**COMBINE, **MEM)),
    "combine_residual": _case(dict(**COMBINE, **RES)),
    "combine_mem_eff_residual": _case(dict(**COMBINE, **MEM, **RES)),
    "combine_attn_outer": _case(dict(COMBINE, layer_attns=(True, True, True))),
    "combine_linear_outer": _case(dict(COMBINE, use_linear_attn=(True, False, False))),
    "combine_no_gca": _case(dict(COMBINE, use_global_context_attn=False)),
    # ---- conditioning and the init conv
    "lowres": _case(dict(lowres_cond=True)),
    "cond_images": _case(dict(cond_images_channels=3)),
    "self_cond": _case(dict(self_cond=True)),
    "self_cond_lowres_cond_images": _case(dict(self_cond=True, lowres_cond=True, cond_images_channels=2), B=3),
    "text": _case(text=True),
    "text_lowres": _case(dict(lowres_cond=True), text=True),
    "plain_init_k3": _case(dict(init_cross_embed=False, init_conv_kernel_size=3)),
    "plain_init_k7_lowres": _case(dict(init_cross_embed=False, lowres_cond=True)),
    "plain_init_k9": _case(dict(init_cross_embed=False, init_conv_kernel_size=9)),
    "init_sizes_3_5": _case(dict(init_cross_embed_kernel_sizes=(3, 5))),
    "init_sizes_3_7_15_5_lowres": _case(dict(init_cross_embed_kernel_sizes=(3, 7, 15, 5), lowres_cond=True)),
    "init_generic": _case(plan=dict(init_conv_generic=1)),
    "init_generic_self_cond_lowres_residual": _case(dict(self_cond=True, lowres_cond=True, **RES), plan=dict(init_conv_generic=1)),
    "plain_init_k7_generic": _case(dict(init_cross_embed=False), plan=dict(init_conv_generic=1)),
    # ---- the final conv
    "final_k1": _case(dict(final_conv_kernel_size=1)),
    "final_k5_lowres": _case(dict(final_conv_kernel_size=5, lowres_cond=True)),
    "final_k7": _case(dict(final_conv_kernel_size=7)),
    "no_final_block": _case(NO_FINAL),
    "no_final_block_blocks_0": _case(dict(NO_FINAL, num_resnet_blocks=(0, 1, 1))),
    "no_final_block_mem_eff": _case(dict(**NO_FINAL, **MEM)),
    "no_final_block_residual": _case(dict(**NO_FINAL, **RES)),
    "no_final_block_mem_eff_residual_lowres": _case(dict(**NO_FINAL, **MEM, **RES, lowres_cond=True)),
    "no_final_block_combine_residual": _case(dict(**NO_FINAL, **COMBINE, **RES)),
    "channels_1": _case(dict(channels=1)),
    "channels_4_lowres": _case(dict(channels=4, lowres_cond=True)),
    "channels_4_final_k7_self_cond": _case(dict(channels=4, final_conv_kernel_size=7, self_cond=True)),
    # ---- the fast plan: dim 128 at 64 px, batch 4
    "fast": _case(B=4, S=64, base=TR.MODEL_A, labels=True),
    "fast_no_gca": _case(dict(use_global_context_attn=False), B=4, S=64, base=TR.MODEL_A),
    "fast_no_skip_scale": _case(dict(scale_skip_connection=False), B=4, S=64, base=TR.MODEL_A),
    "fast_mem_eff_residual_lowres": _case(dict(**MEM, **RES, lowres_cond=True), B=4, S=64, base=TR.MODEL_A),
    "fast_combine": _case(COMBINE, B=4, S=64, base=TR.MODEL_A),
}


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def record(name, device):
    """What the golden holds for CASES[name], from the library that is loaded."""
    c = CASES[name]
    tk = dict(cond_on_text=True, cond_dim=64, text_embed_dim=3) if c["text"] else H.NOTEXT
    pu = H.random_product_unet(seed=100 + sum(map(ord, name)) % 900, **{**c["base"], **tk, **c["kw"]})
    for k, v in c["plan"].items():
        setattr(pu, k, v)
    pu = pu.to(device)
    x, t, kw = H.unet_inputs(pu, c["B"], c["S"], seed=3)
    out = pu(x.to(device), t.to(device), **{k: v.to(device) for k, v in kw.items()}).cpu()
    assert bool(torch.isfinite(out).all()), name
    E = H.engine()
    lib, h = E.load(), pu.engine(c["B"], c["S"], device, with_text=c["text"])
    rows = [r.split(",") for r in H.plan_csv(h).strip().split("\n")[1:]]   # index, label, macs, avg_us, mfma_macs
    assert all(len(r) == 5 for r in rows), name
    got = dict(launches=lib.kd_unet_num_launches(h), cond_launches=lib.kd_unet_num_cond_launches(h),
               hbm_bytes=lib.kd_unet_hbm_bytes(h),
               csv_sha256=_sha("\n".join(",".join((r[1], r[2], r[4])) for r in rows).encode()),
               out_sha256=_sha(out.contiguous().numpy().tobytes()))
    if c["labels"]:
        got["labels"] = [r[1] for r in rows]
    pu.invalidate_engine()
    return got


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_golden_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_and_output_are_the_recorded_ones(device, golden, name):
    got, want = record(name, device), golden[name]
    if "labels" in want and got["labels"] != want["labels"]:
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(want["labels"], got["labels"])) if a != b][:5]
        raise AssertionError(f"{name}: {len(want['labels'])} labels recorded, {len(got['labels'])} now; first differences {diff}")
    assert got == want, name
