"""The case table of tests/test_plan_shapes_gpu.py without a GPU: every case is a shape build_unet takes, the inputs come back
from the case's seed, the product constructs every model and strict-loads the oracle's weights, and the oracle's output at
the cheapest shapes is finite and not degenerate - so that a passing rel-L2 on the GPU means something."""
import pytest
import torch

import plan_shapes_cases as PC


def test_cases_are_unique_and_shapes_the_builder_takes():
    assert len({c.id for c in PC.ALL}) == len(PC.ALL) and len({c.key for c in PC.ALL}) == len(PC.ALL)
    triples = [(c.model, c.B, c.S) for c in PC.SWEEP]            # (an EXTRA case may repeat one under other plan options)
    assert len(set(triples)) == len(triples), sorted(triples)
    assert all(c.plan or (c.model, c.B, c.S) not in triples for c in PC.EXTRA)
    assert len({c.seed for c in PC.ALL}) == len(PC.ALL)
    for c in PC.ALL:
        assert c.S % 2 ** (PC.levels(c.model) - 1) == 0, c.id    # build_unet's only shape precondition
        assert c.B >= 1 and set(c.plan) <= set(PC.PLAN_ATTRS), c.id
    assert not any(c.plan for c in PC.SWEEP)                     # the sweep runs the default rule
    # one fresh-plan comparison per model and size, at an odd batch
    groups = {(c.model, c.S) for c in PC.SWEEP}
    fresh = [c for c in PC.SWEEP if c.fresh]
    assert {(c.model, c.S) for c in fresh} == groups and len(fresh) == len(groups) and all(c.B % 2 for c in fresh)
    # what the sweep is for: every batch of a grid run with --grid-batch 8 at the headline shape
    assert sorted(c.B for c in PC.SWEEP if (c.model, c.S) == ("B", 64)) == list(range(1, 9))


@pytest.mark.parametrize("case", PC.ALL, ids=lambda c: c.id)
def test_inputs_come_back_from_the_seed(case):
    a, a2, b = PC.inputs(case, "a"), PC.inputs(case, "a"), PC.inputs(case, "b")
    flat = lambda inp: [inp[0], inp[1], *inp[2].values()]
    assert list(a[2]) == list(b[2])
    for u, v, w in zip(flat(a), flat(a2), flat(b)):
        assert torch.equal(u, v) and u.shape == w.shape and not torch.equal(u, w)
    x, t, kw = a
    assert x.shape == (case.B, 3, case.S, case.S) and t.shape == (case.B,)
    assert len(set(t.tolist())) == case.B                        # a time of its own per image
    m = PC.MODELS[case.model]
    assert ("lowres_noise_times" in kw) == m["lowres"] and ("cond_images" in kw) == bool(m["kw"].get("cond_images_channels"))
    if m["lowres"]:
        assert len(set(kw["lowres_noise_times"].tolist())) == case.B


@pytest.mark.parametrize("model", list(PC.MODELS))
def test_product_constructs_the_model_and_loads_the_oracle_weights(model):
    import imagen_pytorch as ip

    ou = PC.oracle_unet(model)
    pu = ip.Unet(**ou._locals)
    missing, unexpected = pu.load_state_dict(ou.state_dict(), strict=True)
    assert not missing and not unexpected
    assert PC.num_skips(model) == sum(pu._plan["num_resnet_blocks"]) + len(pu._plan["dim_mults"])


@pytest.mark.parametrize("case", sorted(PC.ALL, key=lambda c: c.B * c.S * c.S)[:2], ids=lambda c: c.id)
def test_oracle_output_of_the_cheapest_cases_is_finite_and_not_degenerate(case):
    ou = PC.oracle_unet(case.model)
    x, t, kw = PC.inputs(case)
    with torch.no_grad():
        y = ou(x, t, **kw)
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    assert float(y.std()) > 1e-3 and all(float(y[i].std()) > 1e-3 for i in range(case.B))
