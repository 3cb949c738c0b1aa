"""TEST INFRASTRUCTURE ONLY: the (model, image size, batch) table of tests/test_plan_shapes_gpu.py (the engine's plans at
every batch a patch grid runs, against the oracle) and of its CPU check in tests/test_plan_shapes.py.  No product imports.

The engine picks its kernels from the static shape - conv3x3_choice / wino4_images / wino4_whole_ok / fwino_ok / gemm_ok
(csrc/engine.hip), gemm_bf16x3_ok and the k-cut rule (csrc/kernels_gemm_bf16x3.hip), downsample_x3_ok and SkipStack::pop
(csrc/unet_build.inc) - and `ultra_res/distributed.py::imagen_sample_fn(max_batch=n)` hands it every batch 1 .. n of one
UNet over one packed-weight store.  SWEEP is those batches at the widths where the fast paths engage (dim 128); EXTRA are
the cases added so that every label family of test_plan_shapes_gpu.FAMILIES occurs in some plan (plan options through the
attributes Unet.engine() reads).
"""
from __future__ import annotations

import zlib

import torch

import combine_fmaps_ref as CR
import helpers as H
import trajectory_ref as TR
from oracle import imagen_ref as R

PLAN_ATTRS = ("conv_algo", "gemm_bf16x3", "x3_linear", "wino43_min_cin", "wino4_max_images")   # 0 = the default rule

# name -> Unet kwargs, the oracle's class, lowres_cond, weight seed.  "SW" is MODEL_A with the library's other down- and
# upsample forms, the UpsampleCombiner and linear attention on the levels without full attention (kernels_resample.hip,
# kernels_upcombine.hip, kernels_linattn.hip: shape rules of their own); "A_sc" MODEL_A with self-conditioning.
MODELS = {
    "A": dict(kw=TR.MODEL_A, cls=R.Unet, lowres=False, seed=29),
    "B": dict(kw=TR.MODEL_B, cls=R.Unet, lowres=True, seed=31),
    "SW": dict(kw=dict(TR.MODEL_A, cross_embed_downsample=True, pixel_shuffle_upsample=False, combine_upsample_fmaps=True,
                       use_linear_attn=(True, True, False)), cls=CR.Unet, lowres=False, seed=37),
    "A_sc": dict(kw=dict(TR.MODEL_A, self_cond=True), cls=CR.Unet, lowres=False, seed=33),
}


class Case:
    """One forward shape: `model` of MODELS at `S` x `S`, batch `B`, under the plan options `plan`.  fresh: the case whose
    history check also runs on a fresh plan of a fresh product UNet (one odd batch per model and size)."""

    def __init__(self, model, S, B, plan=None, fresh=False):
        self.model, self.S, self.B, self.plan, self.fresh = model, S, B, dict(plan or {}), fresh
        assert set(self.plan) <= set(PLAN_ATTRS)
        self.id = f"{model}-S{S}-B{B}" + "".join(f"-{k}{v}" for k, v in sorted(self.plan.items()))
        self.seed = zlib.crc32(self.id.encode()) & 0x3fffffff   # of the inputs: 2 seed ("a") and 2 seed + 1 ("b")

    @property
    def key(self):
        return self.model, self.S, self.B, tuple(sorted(self.plan.items()))


def _cases(model, S, batches, fresh):
    return [Case(model, S, b, fresh=b == fresh) for b in batches]


SWEEP = (
    _cases("B", 64, range(1, 9), 5)           # every batch of an 8 x 8 grid's waves under --grid-batch 8
    + _cases("B", 128, (1, 2, 3, 4), 3)       # the 128 x 128 maps: fp32-V and plane form of the position GEMMs, k-cut sums
    + _cases("B", 32, (2, 5), 5)
    + _cases("B", 96, (2, 5), 5)              # maps of 96, 48, 24, 12, 6: no multiples of 16, of 8 only in part
    + _cases("A", 64, (1, 3, 5, 7, 8), 7)
    + _cases("A", 40, (3,), 3)                # maps of 40, 20, 10: F(4x4,3x3) takes 10 x 10 nowhere
    + _cases("SW", 64, (1, 3, 6), 3)
)
# what no default plan of SWEEP reaches on 256 CUs (read from the rules, then seen in the plans' labels):
# - V of the bf16x3 position GEMMs as planes by default needs Cin Cout >= 40 (6 Cin + 4 Cout), 512 -> 512, whose GEMMs fill the
#   chip from batch 16 on only: gemm_bf16x3 = 1 writes planes everywhere;
# - a token GEMM / 1x1 conv / 2x2-s2 downsample on bf16x3 whose tiles are cut in k needs K >= 1024 by default and 64 tiles:
#   x3_linear = 128 takes K >= 128 (4096 tokens x 512 -> 1024: 128 tiles on 256 CUs, every one cut; the 128 x 128 -> 64 x 64
#   downsample: 64 tiles)
# - no ResnetBlock conv of MODEL_B at 64 x 64 is planned on three paths by the default rule (the 64 x 64 convs go direct or
#   F(2x2,3x3) GEMMs -> F(4x4,3x3) at batch 4, the 16 x 16 ones direct <-> F(2x2,3x3) GEMMs with Mt % 256): conv_algo = 3 runs the
#   fused F(2x2,3x3) kernel wherever its shape rule allows, here at an odd batch on the 64 x 64, 32 x 32 and 16 x 16 maps;
# - F(4x4,3x3) on the fp32 MFMA is what a plan without bf16x3 runs: conv_algo = 4 (wherever the shape fits) at an odd batch;
# - F(4x4,3x3) layers in launch sets (every per-image pointer moved on by a set: what the per-image bound is for) need maps
#   past 4 GB by default: wino4_max_images = 2 cuts batch 6 in three sets (on conv_algo = 4: a set of 2 does not fill 256 CUs)
EXTRA = [
    Case("A", 128, 4, dict(gemm_bf16x3=1, x3_linear=128)),
    Case("B", 64, 7, dict(conv_algo=3)),
    Case("B", 64, 3, dict(conv_algo=4, gemm_bf16x3=-1)),
    Case("B", 64, 6, dict(conv_algo=4, wino4_max_images=2)),
]
ALL = SWEEP + EXTRA


def levels(model):
    return len(MODELS[model]["kw"]["dim_mults"])


def num_skips(model):
    """Skip concats of one forward: a hidden per ResnetBlock of the down path's `.2` lists and one per level's attention slot."""
    kw = MODELS[model]["kw"]
    L = levels(model)
    nb = kw["num_resnet_blocks"]
    nb = tuple(nb) if isinstance(nb, (tuple, list)) else (nb,) * L
    return sum(nb) + L


def oracle_unet(model):
    m = MODELS[model]
    return H.randomize_(m["cls"](**m["kw"], lowres_cond=m["lowres"], cond_on_text=False, text_embed_dim=None), m["seed"]).eval()


def inputs(case, which="a"):
    """x, log-SNR and the keyword inputs of forward `which` ("a" | "b": independent in every tensor) of `case`: t differs per
    image (as _inputs of tests/test_unet_gpu.py draws it), and so do the low-res noise times."""
    m = MODELS[case.model]
    B, S = case.B, case.S
    g = torch.Generator().manual_seed(2 * case.seed + {"a": 0, "b": 1}[which])
    x = torch.randn(B, 3, S, S, generator=g)
    t = torch.randn(B, generator=g) * 3
    kw = {}
    if m["lowres"]:
        kw["lowres_cond_img"] = torch.randn(B, 3, S, S, generator=g)
        kw["lowres_noise_times"] = torch.rand(B, generator=g) * 4 - 2
    cc = m["kw"].get("cond_images_channels", 0)
    if cc:
        kw["cond_images"] = torch.rand(B, cc, 2 * S, 2 * S, generator=g)   # resized inside (nearest)
    if m["kw"].get("self_cond"):
        kw["self_cond"] = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    return x, t, kw
