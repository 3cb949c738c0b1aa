"""The fast plans at every batch a patch grid runs, against the oracle (tests/plan_shapes_cases.py).

The engine picks its kernels from the static (batch, image size) - five ResnetBlock conv paths, bf16x3 or fp32-MFMA token
GEMMs with or without a k-cut sum, a skip scale folded into its consumer or applied in memory, GroupNorm statistics folded from
partials or taken in a pass - and a grid run builds the plans of batches 1 .. n on ONE UNet over one packed-weight store.  One
oracle UNet and one product UNet per model serve the whole module, so the plans pile up on a store as they do there.

1. every case's forward against the oracle, PER IMAGE and on each image's 4-pixel border ring alone (an error confined to
   the last image of an odd batch, or to the ring where a Winograd tile or a buffer bound goes wrong, is diluted in a
   whole-batch rel-L2);
2. history independence with DIFFERENT inputs: f(a), f(b), f(a) on one plan, and f(b) against a fresh plan of a fresh UNet;
3. the packed-weight store does not depend on the order the plans were built in;
4. the sweep reaches the paths it was written for (kd_unet_profile labels);
5. odd batches of the full-size SR UNet against its batch-1 plan.

Bound: the project's FWD_REL_L2 (tests/test_unet_gpu.py), per image."""
import ctypes as C
import re

import pytest
import torch

import helpers as H
import plan_shapes_cases as PC

pytestmark = pytest.mark.gpu

FWD_REL_L2 = 2e-5
RING = 4
_ids = lambda c: c.id


def _set_plan(pu, plan):
    for k in PC.PLAN_ATTRS:   # engine extensions, read when a forward looks its plan up (0 = the default rule)
        setattr(pu, k, plan.get(k, 0))


def _ring(img):
    """The RING-pixel-wide border of [C, S, S] as [C, n]."""
    S = img.shape[-1]
    m = torch.ones(S, S, dtype=torch.bool)
    m[RING:S - RING, RING:S - RING] = False
    return img[:, m]


def _errors(got, ref):
    """Per image: rel-L2 of the whole image and of its border ring alone."""
    per = [H.rel_l2(got[i], ref[i]) for i in range(ref.shape[0])]
    ring = [H.rel_l2(_ring(got[i]), _ring(ref[i])) for i in range(ref.shape[0])]
    return per, ring


class Sweep:
    """The module's shared state: per model one (oracle, product) pair, per case its oracle output, its engine output and
    its plan's launch labels - computed once, shared unchanged by the tests."""

    def __init__(self, device):
        self.device, self.models, self.done = device, {}, {}
        self.worst_image, self.worst_ring = (0.0, None), (0.0, None)

    def product(self, model):
        return H.product_unet_like(self.model(model)[0]).to(self.device)

    def model(self, model):
        if model not in self.models:
            ou = PC.oracle_unet(model)
            self.models[model] = (ou, H.product_unet_like(ou).to(self.device))
        return self.models[model]

    def dev(self, inp):
        x, t, kw = inp
        return x.to(self.device), t.to(self.device), {k: v.to(self.device) for k, v in kw.items()}

    def forward(self, pu, case, inp, **plan_over):
        """One forward of `pu` on the plan of `case`; returns the output on the host."""
        _set_plan(pu, {**case.plan, **plan_over})
        x, t, kw = self.dev(inp)
        return pu(x, t, **kw).cpu()

    def handle(self, pu, case):
        _set_plan(pu, case.plan)
        return pu.engine(case.B, case.S, self.device, with_text=False)

    def labels(self, pu, case, inp):
        """The label column of kd_unet_profile, one per launch (it runs the plan again, on the pointers of the last forward:
        the inputs stay alive here)."""
        E = H.engine()
        _set_plan(pu, case.plan)
        x, t, kw = self.dev(inp)
        pu(x, t, **kw)
        buf = C.create_string_buffer(1 << 20)
        E.check(E.load().kd_unet_profile(self.handle(pu, case), 1, buf, len(buf), E.current_stream()))
        torch.cuda.synchronize()
        return [row.split(",")[1] for row in buf.value.decode().strip().split("\n")[1:]]

    def run(self, case):
        if case.id not in self.done:
            ou, pu = self.model(case.model)
            inp = PC.inputs(case, "a")
            with torch.no_grad():
                ref = ou(inp[0], inp[1], **inp[2])
            got = self.forward(pu, case, inp)
            self.done[case.id] = dict(ref=ref, got=got, labels=self.labels(pu, case, inp))
        return self.done[case.id]

    def note(self, case, per, ring):
        if max(per) > self.worst_image[0]:
            self.worst_image = (max(per), case.id)
        if max(ring) > self.worst_ring[0]:
            self.worst_ring = (max(ring), case.id)


@pytest.fixture(scope="module")
def sweep(device):
    return Sweep(device)


# ------------------------------------------------------------------------------- 1. forward against the oracle
@pytest.mark.parametrize("case", PC.ALL, ids=_ids)
def test_forward_matches_the_oracle_per_image_and_on_the_border_ring(sweep, case):
    r = sweep.run(case)
    got, ref = r["got"], r["ref"]
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    per, ring = _errors(got, ref)
    sweep.note(case, per, ring)
    print(f"plan shapes {case.id}: per image {' '.join(f'{e:.2e}' for e in per)} | ring {' '.join(f'{e:.2e}' for e in ring)}")
    assert max(per) < FWD_REL_L2, (case.id, per)
    if max(ring) >= FWD_REL_L2:
        # the ring holds a fifth of the pixels, whose error the rest of the image no longer averages: where a plan passes the
        # constant there, it is held to 3 x the ring error of the direct-conv plan of the same case (conv_algo = 1, a k-ordered
        # fmaf chain held to the oracle all over the suite) - the max(3 * err_cpu, ...) form of test_conv_igemm
        direct = sweep.forward(sweep.model(case.model)[1], case, PC.inputs(case, "a"), conv_algo=1)
        _, dring = _errors(direct, ref)
        print(f"  ring on the direct-conv plan: {' '.join(f'{e:.2e}' for e in dring)}")
        assert all(e < max(FWD_REL_L2, 3 * d) for e, d in zip(ring, dring)), (case.id, ring, dring)


# ------------------------------------------------------------------------------- 2. history independence
@pytest.mark.parametrize("case", PC.ALL, ids=_ids)
def test_a_forward_does_not_depend_on_the_forward_before_it(sweep, case):
    """f(a), f(b), f(a) on the case's plan, b independent of a in every tensor argument: the second f(a) is the first one bit
    for bit - nothing a forward leaves in the workspace (accumulated GroupNorm partials, k-part slabs, a region no launch of
    this shape writes) reaches the next.  Asserted with the same inputs twice, as elsewhere, both forwards would leave and
    read the same state.  Where case.fresh: f(b) is also what a fresh plan of a fresh UNet gives for b as its first forward."""
    y_a = sweep.run(case)["got"]
    _, pu = sweep.model(case.model)
    a, b = PC.inputs(case, "a"), PC.inputs(case, "b")
    y_b = sweep.forward(pu, case, b)
    y_a2 = sweep.forward(pu, case, a)
    assert not torch.equal(y_b, y_a)
    assert torch.equal(y_a2, y_a), (case.id, H.rel_l2(y_a2, y_a))
    if case.fresh:
        y_b_fresh = sweep.forward(sweep.product(case.model), case, b)
        assert torch.equal(y_b, y_b_fresh), (case.id, H.rel_l2(y_b, y_b_fresh))


def test_a_forward_without_self_cond_does_not_read_the_one_before_it(sweep):
    """Unet(self_cond=True): f(a, self_cond=s), then f(a, self_cond=None) on the same plan equals a fresh plan's
    f(a, self_cond=None) - the plan's self_cond buffer is zeroed, not left from the call before.  Both against the oracle."""
    case = PC.Case("A_sc", 64, 3)
    ou, pu = sweep.model("A_sc")
    x, t, kw = PC.inputs(case, "a")
    assert set(kw) == {"self_cond"}
    with torch.no_grad():
        ref_s, ref_0 = ou(x, t, **kw), ou(x, t)
    y_s = sweep.forward(pu, case, (x, t, kw))
    y_0 = sweep.forward(pu, case, (x, t, {}))
    y_0_fresh = sweep.forward(sweep.product("A_sc"), case, (x, t, {}))
    assert torch.equal(y_0, y_0_fresh), H.rel_l2(y_0, y_0_fresh)
    assert H.rel_l2(ref_s, ref_0) > 1e-3    # the input matters
    for got, ref in ((y_s, ref_s), (y_0, ref_0)):
        per, ring = _errors(got, ref)
        print(f"plan shapes {case.id}: per image {' '.join(f'{e:.2e}' for e in per)} | ring {' '.join(f'{e:.2e}' for e in ring)}")
        assert max(per) < FWD_REL_L2 and max(ring) < FWD_REL_L2, (per, ring)


# ------------------------------------------------------------------------------- 3. the shared weight store
def test_packed_weights_do_not_depend_on_the_order_the_plans_were_built_in(sweep):
    """The plans of MODEL_B at 64 x 64, batches 1 .. 8, on one UNet in ascending and on another in descending order: the
    store is filled by whichever plan asks for a key first ("wino4:" + prefix, "res_conv_skipscaled:" + prefix + ":" + c0,
    "x3lin:" + pointer + shape ...), so every batch must give the same bits on both - and the bits of a UNet that owns that
    one plan alone, and of the module's UNet, whose plans were built in the order the tests ran."""
    lib = H.engine().load()
    cases = [c for c in PC.SWEEP if (c.model, c.S) == ("B", 64)]
    assert [c.B for c in cases] == list(range(1, 9))
    up, down = sweep.product("B"), sweep.product("B")
    outs = {}
    for pu, order in ((up, cases), (down, cases[::-1])):
        for c in order:
            outs[id(pu), c.B] = sweep.forward(pu, c, PC.inputs(c, "a"))
    for c in cases:
        assert torch.equal(outs[id(up), c.B], outs[id(down), c.B]), c.id
        assert torch.equal(outs[id(up), c.B], sweep.run(c)["got"]), c.id
    for pu in (up, down):
        assert len(pu._engines) == len(cases)
        sizes = {lib.kd_unet_weight_bytes(h) for h in pu._engines.values()}
        assert len(sizes) == 1 and min(sizes) > 0, sizes
    # one that takes F(4x4,3x3) at the top level and one that does not
    top = lambda c: any(l.startswith(f"wino4 gemm bf16x3 M{c.B * c.S * c.S} ") for l in sweep.run(c)["labels"])
    with_f4, without = next(c for c in cases[::-1] if top(c)), next(c for c in cases[::-1] if not top(c))
    for c in (with_f4, without):
        own = sweep.product("B")
        assert torch.equal(sweep.forward(own, c, PC.inputs(c, "a")), outs[id(up), c.B]), c.id
        assert len(own._engines) == 1


# ------------------------------------------------------------------------------- 4. the paths the sweep reaches
_SHAPE = r" M(\d+) Cin(\d+) Cout(\d+)"
_X3_GEMM = re.compile(r"(wino4 gemm bf16x3|conv k[12] x3) M")
_X3_SUM = re.compile(r"(wino4 x3|conv k[12] x3) sum M")


def _followed(labels, first, then):
    """A launch whose label starts with `first` directly followed by one that starts with `then`."""
    return any(a.startswith(first) and b.startswith(then) for a, b in zip(labels, labels[1:]))


def _unsummed(labels, stem):
    return any(l.startswith(stem + " M") and not (i + 1 < len(labels) and _X3_SUM.match(labels[i + 1]))
               for i, l in enumerate(labels))


def _resnet_convs(labels, B):
    """(pixels per image, Cin, Cout) -> the paths the plan runs ResnetBlock 3x3 convs of that shape on."""
    out = {}
    for i, l in enumerate(labels):
        path = None
        if l.startswith(("wino4 gemm M", "wino4 gemm bf16x3 M")):
            path = "F(4x4,3x3)"
        elif l.startswith("wino gemm M"):
            path = "F(2x2,3x3) GEMMs"
        elif l.startswith("wino fused M"):
            path = "F(2x2,3x3) fused"
        elif l.startswith("conv k3 s1 M") and i > 0 and labels[i - 1].startswith("gn apply"):   # gn_silu + the direct conv
            path = "direct"
        if path:
            M, cin, cout = (int(v) for v in re.search(_SHAPE, l).groups())
            out.setdefault((M // B, cin, cout), set()).add(path)
    return out


def _in_memory_scales(labels):
    """Skip concats whose 2^-1/2 a launch applies in memory: in place, or by the copy that builds the concat."""
    return sum(l.startswith(("scale slice rows", "concat rows", "concat tail rows")) for l in labels)


# family -> (case, labels) -> bool.  Label strings: Builder's emit() calls in csrc/engine.hip and csrc/unet_build.inc
FAMILIES = {
    "F(4x4,3x3) on bf16x3, V as planes": lambda c, ls: _followed(ls, "wino4_in3 M", "wino4 gemm bf16x3 M"),
    "F(4x4,3x3) on bf16x3, V as fp32": lambda c, ls: _followed(ls, "wino4_in M", "wino4 gemm bf16x3 M"),
    "F(4x4,3x3) on the fp32 MFMA": lambda c, ls: _followed(ls, "wino4_in M", "wino4 gemm M"),
    # (rows of a set at the top level: wino4_max_images x S x S, one launch per set and layer)
    "F(4x4,3x3) in sets of images": lambda c, ls: bool(c.plan.get("wino4_max_images")) and sum(
        l.startswith(f"wino4_in M{c.plan['wino4_max_images'] * c.S * c.S} ") for l in ls) >= c.B // c.plan["wino4_max_images"],
    "F(2x2,3x3) batched GEMMs": lambda c, ls: any(l.startswith("wino gemm M") for l in ls),
    "F(2x2,3x3) fused": lambda c, ls: any(l.startswith("wino fused M") for l in ls),
    # (not on "SW": the UpsampleCombiner's full-resolution Block is GroupNorm + direct conv too)
    "ResnetBlock 3x3 on the direct conv": lambda c, ls: c.model != "SW" and "direct" in set().union(*_resnet_convs(ls, c.B).values()),
    "wino4 x3 sum": lambda c, ls: _followed(ls, "wino4 gemm bf16x3 M", "wino4 x3 sum M"),
    "conv k1 x3 sum": lambda c, ls: _followed(ls, "conv k1 x3 M", "conv k1 x3 sum M"),
    "conv k1 x3 without a sum": lambda c, ls: _unsummed(ls, "conv k1 x3"),
    "conv k2 x3": lambda c, ls: any(l.startswith("conv k2 x3 M") for l in ls),
    "2x2-s2 downsample off bf16x3": lambda c, ls: any(l.startswith("conv k2 s2 M") for l in ls),
    "scale slice rows": lambda c, ls: any(l.startswith("scale slice rows") for l in ls),
    "skip concat with the scale folded": lambda c, ls: _in_memory_scales(ls) < PC.num_skips(c.model),
    "gn fold seg": lambda c, ls: any(l.startswith("gn fold seg") for l in ls),
    "gn stats": lambda c, ls: any(l.startswith("gn stats") for l in ls),
}


def test_the_sweep_reaches_the_paths_it_was_written_for(sweep):
    """Over the union of the cases, every label family occurs in at least one plan; and within MODEL_B at 64 x 64 one
    ResnetBlock conv (the same pixels, Cin and Cout per image) is planned on three different paths across the batches.
    No per-shape path table is asserted: the rules are tuned by measurement and move."""
    plans = {c.id: (c, sweep.run(c)["labels"]) for c in PC.ALL}
    for c, ls in plans.values():
        assert 0 <= _in_memory_scales(ls) <= PC.num_skips(c.model), (c.id, [l for l in ls if "concat" in l or "scale" in l])
        for i, l in enumerate(ls):   # a sum launch directly follows its GEMM
            assert not _X3_SUM.match(l) or (i > 0 and _X3_GEMM.match(ls[i - 1])), (c.id, ls[i - 1:i + 1])
    missing = []
    for name, has in FAMILIES.items():
        where = [c.id for c, ls in plans.values() if has(c, ls)]
        print(f"plan shapes family '{name}': {len(where)} plans ({' '.join(where[:6])}{' ...' if len(where) > 6 else ''})")
        if not where:
            missing.append(name)
    assert not missing, missing
    paths = {}
    for c, ls in plans.values():
        if (c.model, c.S) == ("B", 64) and not c.plan.get("wino4_max_images"):   # (a set's rows are not the batch's)
            for shape, p in _resnet_convs(ls, c.B).items():
                for name in p:
                    paths.setdefault(shape, {}).setdefault(name, []).append(c.B)
    for shape, p in sorted(paths.items()):
        print(f"plan shapes MODEL_B 64 x 64, conv HW{shape[0]} Cin{shape[1]} Cout{shape[2]}: " +
              "; ".join(f"{name} at batch {sorted(set(bs))}" for name, bs in sorted(p.items())))
    assert any(len(p) >= 3 for p in paths.values()), {k: sorted(v) for k, v in paths.items()}


# ------------------------------------------------------------------------------- 5. odd batches at the reference's size
@pytest.fixture(scope="module")
def full_size(device):
    """The full C3 SR UNet (dim 128, 256 x 256) built on the meta device with weights drawn on the GPU, as
    test_full_size_sr_unet_is_deterministic_and_batch_independent does; 7 images of inputs "a" and "b" with per-image times,
    and every image of "a" run alone on the batch-1 plan (held to the oracle in tests/test_fullsize_gpu.py)."""
    import imagen_pytorch as ip

    def build():
        with torch.device("meta"):
            u = ip.Unet(dim=128, dim_mults=(1, 2, 4, 8), num_resnet_blocks=2, memory_efficient=True,
                        layer_attns=(False, False, False, True), layer_cross_attns=(False, False, True, True),
                        init_conv_to_final_conv_residual=True, cond_images_channels=3, lowres_cond=True,
                        **H.NOTEXT)
        return u.to_empty(device=device)

    u = build()
    g = torch.Generator(device=device).manual_seed(0)
    with torch.no_grad():
        for name, p in u.named_parameters():
            if name.endswith(".g") or name.endswith("norm.weight") or name.endswith("groupnorm.weight") \
                    or name.endswith("norm_cond.weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g, device=device))
            elif p.dim() == 1:
                p.copy_(0.05 * torch.randn(p.shape, generator=g, device=device))
            else:
                p.copy_(torch.randn(p.shape, generator=g, device=device) * p[0].numel() ** -0.5)
    N, S = 7, 256

    def draw():
        return dict(x=torch.randn(N, 3, S, S, generator=g, device=device), lr=torch.randn(N, 3, S, S, generator=g, device=device),
                    cond=torch.rand(N, 3, S, S, generator=g, device=device), t=torch.randn(N, generator=g, device=device) * 3,
                    tl=torch.rand(N, generator=g, device=device) * 4 - 2)

    a, b = draw(), draw()
    assert len(set(a["t"].tolist())) == N and len(set(a["tl"].tolist())) == N
    run = lambda net, d, sl: net(d["x"][sl], d["t"][sl], lowres_cond_img=d["lr"][sl], lowres_noise_times=d["tl"][sl],
                                 cond_images=d["cond"][sl])
    singles = torch.cat([run(u, a, slice(i, i + 1)) for i in range(N)])
    assert bool(torch.isfinite(singles).all()) and float(singles.std()) > 1e-3

    def twin():   # a fresh UNet with the same weights and no plan
        v = build()
        v.load_state_dict(u.state_dict(), strict=True)
        return v

    return dict(u=u, a=a, b=b, run=run, singles=singles, twin=twin)


@pytest.mark.parametrize("B", [5, 6, 7])
def test_full_size_sr_unet_at_odd_batches_equals_its_batch_1_plan(full_size, B):
    """Batches 5, 6 and 7 of the full-size SR UNet (the oracle is too slow there): every image equals the same image run alone
    on the batch-1 plan to rel-L2 1e-5 (the constant of the batch-3 test: another tile mapping, so to fp32 rounding), repeated
    calls are bit-identical, and so is f(a) after f(b); at batch 7 f(b) is also a fresh UNet's first forward."""
    fs = full_size
    u, run, sl = fs["u"], fs["run"], slice(0, B)
    full = run(u, fs["a"], sl)
    assert full.shape == (B, 3, 256, 256) and bool(torch.isfinite(full).all())
    errs = [H.rel_l2(full[i], fs["singles"][i]) for i in range(B)]
    print(f"plan shapes full size B={B}: per image against the batch-1 plan {' '.join(f'{e:.2e}' for e in errs)}")
    assert max(errs) < 1e-5, errs
    assert torch.equal(full, run(u, fs["a"], sl))
    y_b = run(u, fs["b"], sl)
    assert not torch.equal(y_b, full)
    assert torch.equal(run(u, fs["a"], sl), full)
    if B == 7:
        assert torch.equal(run(fs["twin"](), fs["b"], sl), y_b)


# ------------------------------------------------------------------------------- the module's figures (README, parity row)
def test_report_the_largest_per_image_and_per_ring_error(sweep):
    for c in PC.ALL:
        per, ring = _errors(sweep.run(c)["got"], sweep.run(c)["ref"])
        sweep.note(c, per, ring)
    (e_img, c_img), (e_ring, c_ring) = sweep.worst_image, sweep.worst_ring
    print(f"plan shapes: {len(PC.ALL)} cases, largest per-image rel-L2 {e_img:.2e} ({c_img}), "
          f"largest per-ring rel-L2 {e_ring:.2e} ({c_ring})")
    assert e_img < FWD_REL_L2
