"""CPU checks of the trajectory envelopes (tests/golden/trajectory_envelopes.json) and of the helpers that make them
(tests/trajectory_ref.py): the fixture belongs to the configurations the GPU test runs, the oracle of this commit still
reproduces it, the perturbations have the size they claim, and the per-step check the GPU test applies does reject a
forward error four times the tolerance."""
import json
from pathlib import Path

import pytest
import torch

import trajectory_ref as TR

ENV = json.loads((Path(__file__).resolve().parent / "golden" / "trajectory_envelopes.json").read_text())


def test_fixture_belongs_to_the_configurations_and_the_forward_tolerance():
    import test_unet_gpu

    assert TR.FWD_REL_L2 == test_unet_gpu.FWD_REL_L2 == ENV["eps"]
    assert ENV["margin"] == 1.0 and ENV["modes"] == list(TR.MODES)
    assert set(ENV["configs"]) == set(TR.CONFIGS)
    for name, c in TR.CONFIGS.items():
        e = ENV["configs"][name]
        assert e["params"] == TR.json_cfg(name), name
        assert len(e["rel"]) == len(e["floor_rel"]) == c["T"] and all(v > 0 for v in e["rel"]) and e["final"] > 0
        # what the generator asserted before it wrote: the oracle resolves a quarter of the envelope
        assert all(f <= 0.25 * v for f, v in zip(e["floor_rel"], e["rel"])) and e["floor_final"] <= 0.25 * e["final"], name
        assert all(p in TR.PLANS for p in c["plans"]) and {"default", "plain"} <= set(c["plans"])
    assert set(TR.CONFIGS["base128"]["plans"]) == set(TR.PLANS)


def test_short_record_of_configuration_a_is_reproduced():
    """Configuration A at T = 6, regenerated: within a factor 1.5 of the stored record either way, per step.  Not tighter:
    the host's summation order alone (threads, oneDNN kernels) is about a tenth of the envelope at k = 0."""
    rec = ENV["base128_short"]
    env = TR.envelope("base128", ENV["eps"], T=rec["T"])
    for k, (got, want) in enumerate(zip(env["rel"], rec["rel"])):
        assert want / 1.5 <= got <= want * 1.5, (k, got, want)
    assert rec["final"] / 1.5 <= env["final"] <= rec["final"] * 1.5, (env["final"], rec["final"])


class _Stub:
    """forward_with_cond_scale of a UNet that returns a fixed map."""

    def __init__(self, y):
        self.y = y

    def forward_with_cond_scale(self, *a, **k):
        return self.y.clone()


@pytest.mark.parametrize("eps", [TR.FWD_REL_L2, 4 * TR.FWD_REL_L2])
def test_perturbations_have_the_norm_they_claim(eps):
    """||y' - y|| = eps ||y|| for every mode, in fp64 of the fp32 result: the fp32 rounding of y' (2^-24 |y| per element,
    orthogonal to the perturbation) moves that norm by (6e-8 / eps)^2 / 2 < 1e-5 of itself; 1 % is asserted."""
    y = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(0)) * 0.7 + 0.1
    outs = {}
    for mode in TR.MODES:
        u = _Stub(y)
        with TR.perturbed(u, mode, eps, seed=3):
            a, b = u.forward_with_cond_scale(None), u.forward_with_cond_scale(None)
        assert "forward_with_cond_scale" not in vars(u) and torch.equal(u.forward_with_cond_scale(None), y)   # restored
        for out in (a, b):
            size = float((out.double() - y.double()).norm() / y.double().norm())
            assert abs(size / eps - 1) < 0.01, (mode, size)
        outs[mode] = (a, b)
    assert not torch.equal(*outs["rand"])                                    # a fresh direction per call
    assert torch.equal(*outs["fixed"]) and torch.equal(*outs["scale"])       # one direction for the run
    d = (outs["scale"][0].double() - y.double())
    assert float((d - eps * y.double()).norm() / d.norm()) < 0.01            # along y itself


def test_envelope_check_rejects_four_times_the_forward_tolerance():
    """The check of test_trajectory_gpu.py discriminates: the oracle with one fixed error direction of 4 x FWD_REL_L2 per
    forward - still 20 times inside what SAMPLE_ABS accepts - leaves configuration A's stored envelope (the oracle's
    own floor stays inside a quarter of it: asserted by the generator, re-checked on the stored numbers above)."""
    e = ENV["configs"]["base128"]
    case = TR.Case("base128")
    base = case.run()
    tr, fin = case.run(perturb=("fixed", 4 * ENV["eps"]))
    dev = TR.deviation(tr, base[0], fin, base[1])
    outside = [k for k in range(case.T) if not dev["rel"][k] <= ENV["margin"] * e["rel"][k]]
    print(f"4 eps, fixed direction: {len(outside)} of {case.T} steps outside; largest ratio "
          f"{max(d / v for d, v in zip(dev['rel'], e['rel'])):.2f}, final {dev['final'] / e['final']:.2f}")
    assert outside and dev["final"] > ENV["margin"] * e["final"]
