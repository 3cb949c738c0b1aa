"""Long sampling trajectories of the engine's fast plans against the CPU oracle, held to a calibrated tolerance.

The per-kernel files hold every kernel to fp64 and test_unet_gpu.py / test_fullsize_gpu.py hold one forward to FWD_REL_L2;
here the forward errors feed back on themselves: 12 to 24 sampler steps at dim 128, batch 4, 64 x 64 - the smallest shapes
at which the default plan runs Winograd F(4x4,3x3) on bf16x3 (64 x 64 level), the batched F(2x2,3x3) GEMMs (32 x 32, 16 x 16)
and matrix-core attention (256 queries) - under plain DDPM, the SR call with inpainting resampling, EDM Heun and
self-conditioning (tests/trajectory_ref.py: CONFIGS, PLANS).

The tolerance is tests/golden/trajectory_envelopes.json: per step k, the deviation a forward error of exactly FWD_REL_L2
causes in the ORACLE'S trajectory (the worst of a fresh random direction per call, one fixed direction, a scale factor),
measured on the oracle alone by tests/golden/make_trajectory_envelopes.py.  Margin 1.0: an engine whose forwards sit inside
their tolerance stays inside the envelope; the `plain` plan (direct convs, fp32 MFMA) tells a sampler bug from a
fast-kernel bug when a variant leaves it.

wino4_sets2: on 256 CUs the default rule takes a F(4x4,3x3) layer only where its 36 GEMMs fill the chip (wino4_whole_ok:
36 Mt / 128 x Cout / 64 >= 512), which a set of 2 of the 4 images does not, so `wino4_max_images = 2` alone removes the
layers instead of cutting them.  The two launch sets per layer run on the conv_algo = 4 plan (as in test_unet_gpu.py),
bf16x3 position GEMMs included; no batch had to be moved.

Measured on an MI355X (256 CUs), largest engine deviation / envelope over the steps (rel-L2, at step k) and for the final
image (max-abs):

    configuration / plan          rel-L2: ratio (k)   engine / envelope at that k   final max-abs: ratio
    base128 / default             0.135 (k = 0)       9.27e-08 / 6.85e-07           0.047
    base128 / x3_planes           0.135 (k = 0)       9.27e-08 / 6.85e-07           0.047   (the bits of the default plan)
    base128 / x3_fp32v            0.135 (k = 0)       9.27e-08 / 6.85e-07           0.047   (is the default plan at these shapes)
    base128 / x3_linear128        0.138 (k = 0)       9.47e-08 / 6.85e-07           0.049
    base128 / wino_fused          0.082 (k = 0)       5.63e-08 / 6.85e-07           0.023
    base128 / wino4_all           0.137 (k = 0)       9.36e-08 / 6.85e-07           0.053
    base128 / wino4_sets2         0.129 (k = 0)       8.82e-08 / 6.85e-07           0.048
    base128 / plain               0.094 (k = 0)       6.44e-08 / 6.85e-07           0.027
    sr128 / default               0.105 (k = 0)       1.54e-07 / 1.46e-06           0.040
    sr128 / plain                 0.077 (k = 0)       1.13e-07 / 1.46e-06           0.028
    edm128 / default              0.295 (k = 0)       2.33e-08 / 7.91e-08           0.087
    edm128 / plain                0.223 (k = 0)       1.76e-08 / 7.91e-08           0.042
    selfcond128 / default         0.141 (k = 0)       1.44e-07 / 1.02e-06           0.075
    selfcond128 / plain           0.097 (k = 0)       9.93e-08 / 1.02e-06           0.038

Every variant is widest at the first step and the ratio falls from there: nothing grows faster than a tolerance-sized error
would (base128 / default at k = 23: 8.92e-07 against 1.89e-05, 0.047).  The engine sits at the oracle's own resolution - the
channels_last floor of the fixture is 0.098 (base128), 0.089 (sr128), 0.23 (edm128, k = 0) and 0.100 (selfcond128) of the
envelope - so these ratios bound the engine from above rather than measure it.  Default plans on 256 CUs: base128 / edm128 /
selfcond128 10 F(4x4,3x3) layers on bf16x3 (V as fp32) + 16 F(2x2,3x3) GEMM layers, sr128 4 + 15 and one bf16x3 1x1 conv;
wino4_all 18 F(4x4,3x3) layers, wino4_sets2 36 launch sets (20 on bf16x3), wino_fused 30 fused layers, x3_linear128 two
token GEMMs on bf16x3.
"""
import json
from pathlib import Path

import pytest
import torch

import helpers as H
import trajectory_ref as TR

pytestmark = pytest.mark.gpu

ENV = json.loads((Path(__file__).resolve().parent / "golden" / "trajectory_envelopes.json").read_text())
MARGIN = 1.0
CASES = [(name, plan) for name, c in TR.CONFIGS.items() for plan in c["plans"]]


@pytest.fixture(scope="module")
def oracle():
    """name -> (Case, trace, final image): the oracle's trajectory of a configuration, run once (10 - 20 s of host time)
    and shared, unchanged, by every plan variant and identity check of that configuration."""
    done = {}

    def get(name):
        if name not in done:
            case = TR.Case(name)
            done[name] = (case, *case.run())
        return done[name]

    return get


def _product(case, device, plan):
    """The product sampler over the oracle's weights, its sampled UNet set to the plan variant."""
    cls = "ElucidatedImagen" if case.cfg["sampler"] == "edm" else "Imagen"
    pim = H.product_imagen(case.imagen, cls, device, **case.imagen_kw)
    for k, v in TR.PLANS[plan].items():
        setattr(pim.unets[-1], k, v)
    return pim


def _sample(pim, case, device, **kw):
    skw = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in case.sample_kw.items()}
    return pim.sample(noise_fn=case.noise_fn(), device=device, **skw, **kw).cpu()


def _case_labels(pim, case, device):
    """kd_unet_profile labels of the plan sample() will run: one forward at the configuration's batch and size first."""
    pu, B, S = pim.unets[-1], case.cfg["batch"], case.cfg["size"]
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(B, 3, S, S, generator=g).to(device), (torch.randn(B, generator=g) * 3).to(device)
    kw = {}
    if pu.lowres_cond:
        kw.update(lowres_cond_img=torch.randn(B, 3, S, S, generator=g).to(device), lowres_noise_times=torch.full((B,), -1.3).to(device))
    if pu.has_cond_image:
        kw.update(cond_images=torch.rand(B, 3, S, S, generator=g).to(device))
    pu(x, t, **kw)
    return H.plan_labels(pu, B, S, device)


_count = H.count_labels


def _check_plan(plan, labels, default_labels):
    """The plan is what its name says (labels of Builder::conv3x3_choice's paths, engine.hip)."""
    n4x3, n4, n2, nf = (_count(labels, p) for p in ("wino4 gemm bf16x3", "wino4 gemm", "wino gemm", "wino fused"))
    nlin = _count(labels, "conv k1 x3 M") + _count(labels, "conv k2 x3 M")
    planes, f32v = _count(labels, "wino4_in3 M"), _count(labels, "wino4_in M")
    d4, dlin = _count(default_labels, "wino4 gemm"), _count(default_labels, "conv k1 x3 M") + _count(default_labels, "conv k2 x3 M")
    print(f"  plan {plan}: {n4} F(4x4,3x3) layers ({n4x3} bf16x3; V as planes {planes}, as fp32 {f32v}), {n2} F(2x2,3x3) GEMM layers, "
          f"{nf} fused F(2x2,3x3), {nlin} bf16x3 token GEMMs / 1x1 convs, {len(labels)} launches")
    if plan == "default":
        assert n4x3 >= 1 and n4x3 == n4 and n2 >= 1
    elif plan == "plain":
        assert not any("wino" in l or "x3" in l for l in labels), [l for l in labels if "wino" in l or "x3" in l]
    elif plan == "x3_planes":
        assert n4x3 == d4 >= 1 and planes == n4x3 and f32v == 0
    elif plan == "x3_fp32v":
        assert n4x3 == d4 >= 1 and f32v == n4x3 and planes == 0
    elif plan == "x3_linear128":
        assert nlin > dlin and n4x3 == d4
    elif plan == "wino_fused":
        assert nf >= 1 and n4 == 0
    elif plan == "wino4_all":
        assert n4 > d4 and n2 == 0 and nf == 0
    elif plan == "wino4_sets2":   # (twice the whole-batch plan's launches: checked by the caller; the 64 x 64 level's sets of
        # 2 x 256 tiles stay on bf16x3, the 32 x 32 level's 128 tiles are below its 256-row tile: fp32 MFMA)
        assert n4x3 >= 2 and n4 > n4x3 and n2 == 0 and nf == 0
    else:
        raise AssertionError(plan)


_default_labels = {}


def _labels_of_default(case, device):
    if case.name not in _default_labels:
        _default_labels[case.name] = _case_labels(_product(case, device, "default"), case, device)
    return _default_labels[case.name]


@pytest.mark.parametrize("name,plan", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_trajectory_stays_inside_the_envelope(device, oracle, name, plan):
    case, otrace, ofinal = oracle(name)
    env = ENV["configs"][name]
    T = case.T
    pim = _product(case, device, plan)
    labels = _case_labels(pim, case, device)
    print(f"\n{name}:")
    _check_plan(plan, labels, labels if plan == "default" else _labels_of_default(case, device))
    if case.cfg["unet"] is TR.MODEL_A:   # 256 queries x 8 heads x 4: launch_attention takes the matrix-core kernel from 128 queries
        assert _count(labels, "attn N256") >= 1
    if plan == "wino4_sets2":   # twice the launches of the whole-batch plan
        assert _count(labels, "wino4 gemm") == 2 * _count(_case_labels(_product(case, device, "wino4_all"), case, device), "wino4 gemm")
    trace = []
    final = _sample(pim, case, device, trace=trace)
    assert len(trace) == T == len(env["rel"])
    assert all(bool(torch.isfinite(x).all()) for x in trace) and bool(torch.isfinite(final).all())
    dev = TR.deviation(trace, otrace, final, ofinal)
    ratios = [dev["rel"][k] / env["rel"][k] for k in range(T)]
    kmax = max(range(T), key=lambda k: ratios[k])
    print(f"  {name} / {plan}: largest rel-L2 / envelope {ratios[kmax]:.3f} at k = {kmax} ({dev['rel'][kmax]:.2e} / {env['rel'][kmax]:.2e}); "
          f"rel-L2 k=0 {dev['rel'][0]:.2e} k={T - 1} {dev['rel'][-1]:.2e}; final max-abs / envelope {dev['final'] / env['final']:.3f} "
          f"({dev['final']:.2e} / {env['final']:.2e})")
    out = [(k, dev["rel"][k], env["rel"][k]) for k in range(T) if not dev["rel"][k] <= MARGIN * env["rel"][k]]
    assert not out, f"{name} / {plan}: steps outside the envelope (k, rel-L2, envelope): {out}"
    assert dev["final"] <= MARGIN * env["final"], (dev["final"], env["final"])
    if case.mask is not None:   # the known pixels are pasted back exactly
        m = case.mask[:, None].expand_as(ofinal)
        assert torch.equal(final[m], ofinal[m])


@pytest.mark.parametrize("name", list(TR.CONFIGS))
def test_graph_table_and_traced_runs_are_bit_identical(device, name):
    """On the default (fast) plan over the whole trajectory: graph replay equals eager launches, the conditioning table on
    equals off (A, B, D), and a traced run (one kd_sample_steps call per step) equals the single-call run."""
    case = TR.Case(name)
    pim = _product(case, device, "default")
    whole = _sample(pim, case, device)
    assert bool(torch.isfinite(whole).all())
    assert torch.equal(_sample(pim, case, device, use_graph=False), whole), "graph replay != eager"
    trace = []
    assert torch.equal(_sample(pim, case, device, trace=trace), whole) and len(trace) == case.T, "traced run != single call"
    if name != "edm128":
        pim.cond_table = -1
        off = _sample(pim, case, device)
        off_eager = _sample(pim, case, device, use_graph=False)
        pim.cond_table = 0
        assert torch.equal(off, whole) and torch.equal(off_eager, whole), "cond_table = -1 != cond_table = 0"
