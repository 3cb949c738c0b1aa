"""No forward and no sampler of a plan may read scratch that no op of the same call has written.

A plan's scratch - the arena, the conditioning region, the k-cut slabs of the bf16x3 GEMMs, the sampler's buffers - is
allocated uninitialised; at the start of a forward or of a sampling call every byte of it is undefined.  A read of a
never-written word passes every parity test while the allocator happens to return zeros: a GroupNorm partial nobody stored
adds 0.0, one k-cut slab too many adds 0.0, a padded column meets a zero weight.  kd_unet_poison_scratch
(include/kd_engine.h) fills all of it with one 32-bit word; results must not move, bit for bit, under any of

    0xFFFFFFFF   NaN as a float, NaN as a pair (double), -1 as an integer
    0x7149F2CA   1e30 as a float, about 1e237 as a pair: max / min / clamps / selects drop a NaN operand, not this one
    0            what fresh memory usually holds

1. the forward of the plans the other suites hold to the oracle (tests/plan_shapes_cases.py, tests/unet_options_cases.py,
   the channel counts of tests/test_channels_gpu.py) - no oracle forward here, four engine forwards per case;
2. both samplers (graph replay on and off, guidance, inpainting with resampling, self-conditioning, Heun steps, a reused
   conditioning table), every stage's plan poisoned before each sample() call;
3. kd_unet_forward_self_cond through the C ABI with every input and the output a slice of a NaN-filled allocation: the
   output equals the plain-tensor forward and every guard word is still NaN.

No tolerance anywhere: torch.equal.

What the check sees is a read of a word that NO op of the same call has written.  A word that an earlier op of the same
forward left in a block the arena has since handed to another tensor is written, deterministic and finite: a store skipped
into such a block (tried: the last chunk's partial of gate_add, whose buffer is carved from the block of the ResnetBlock's
own intermediate, released just before - Builder::resnet, engine.hip) changes nothing from call to call and passes.  The
same skipped store in the init conv's partials, whose buffer is the first use of its block, does not (DESIGN.md,
"Workspace")."""
import ctypes as C

import pytest
import torch

import elucidated_ref as ER
import helpers as H
import plan_shapes_cases as PC
import self_cond_ref as SR
import test_plan_shapes_gpu as TP
import test_unet_options_gpu as TO
import unet_options_cases as OC
from oracle import imagen_ref as R

pytestmark = pytest.mark.gpu

WORDS = (0xFFFFFFFF, 0x7149F2CA, 0)   # in this order
GUARD = 1024                          # floats of NaN on each side of a slice: 4 KiB
NAN_BITS = 0x7FC00000                 # torch.full(.., nan) in fp32


def test_the_words_are_what_the_docstring_says():
    f = torch.tensor([0x7149F2CA], dtype=torch.int32).view(torch.float32)
    assert float(f) == pytest.approx(1e30, rel=1e-6)
    d = torch.tensor([0x7149F2CA, 0x7149F2CA], dtype=torch.int32).view(torch.float64)
    assert 1e236 < float(d) < 1e238
    assert torch.isnan(torch.tensor([-1], dtype=torch.int32).view(torch.float32)).all()
    assert torch.isnan(torch.tensor([-1, -1], dtype=torch.int32).view(torch.float64)).all()


def _poison(h, word):
    E = H.engine()
    n = C.c_int64(-1)
    E.check(E.load().kd_unet_poison_scratch(h, word, C.byref(n), E.current_stream()))
    return n.value


def _diff(got, base):
    """What a failing comparison prints: differing and non-finite elements, the largest difference among the finite ones."""
    got, base = got.double().cpu(), base.double().cpu()
    ne = got != base
    fin = torch.isfinite(got)
    big = float((got - base)[fin & ne].abs().max()) if bool((fin & ne).any()) else 0.0
    return f"{int(ne.sum())} of {got.numel()} elements differ, {int((~fin).sum())} not finite, largest finite difference {big:.3e}"


def _check_forward(pu, run, handle, label):
    """One un-poisoned forward, then poison + forward per word (Unet.forward runs kd_unet_text_cond on the same plan first
    where the UNet has text): all four outputs equal and finite; the fill covers at least the arena and the cond region."""
    E = H.engine()
    lib = E.load()
    base = run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(base).all()) and float(base.std()) > 0
    h, n_plans = handle(), len(pu._engines)
    assert any(h is v for v in pu._engines.values())
    # hbm = arena + cond region + conditioning table + weights; no sampling call has run on this plan, so there is no table
    assert lib.kd_unet_cond_table_build_ms(h, None, None) < 0
    table = 0
    want = lib.kd_unet_hbm_bytes(h) - lib.kd_unet_weight_bytes(h) - table
    assert want > 0
    bad = []
    for word in WORDS:
        filled = _poison(h, word)
        assert filled >= want, (label, hex(word), filled, want)
        out = run()
        torch.cuda.synchronize()
        if not torch.equal(out, base):
            bad.append(f"{word:#010x}: {_diff(out, base)}")
    assert len(pu._engines) == n_plans, "the forwards ran on another plan than the one poisoned"
    print(f"poisoned scratch {label}: {want} bytes of arena + cond region, {filled} filled, {len(bad)} of {len(WORDS)} words differ")
    assert not bad, (label, bad)


# ------------------------------------------------------------------------------- 1. forward
def _plan_case(model, S, B, plan=None):
    """The case of PC.ALL with this shape (A_sc is built as tests/test_plan_shapes_gpu.py builds it: it is in no table)."""
    key = PC.Case(model, S, B, plan).key
    hits = [c for c in PC.ALL if c.key == key]
    assert len(hits) == (0 if model == "A_sc" else 1), key
    return hits[0] if hits else PC.Case(model, S, B, plan)


PLAN_CASES = (
    [_plan_case("B", 64, b) for b in (1, 4, 5, 8)] + [_plan_case("B", 128, b) for b in (1, 3)] + [_plan_case("B", 96, 5)]
    + [_plan_case("A", 64, b) for b in (3, 8)] + [_plan_case("A", 40, 3)] + [_plan_case("SW", 64, b) for b in (3, 6)]
    + [_plan_case("A_sc", 64, 3)] + list(PC.EXTRA)
)
assert len(PC.EXTRA) == 4


@pytest.fixture(scope="module")
def sweep(device):
    """tests/test_plan_shapes_gpu.py's holder: one product UNet per model, the plans pile up on its weight store."""
    return TP.Sweep(device)


@pytest.mark.parametrize("case", PLAN_CASES, ids=lambda c: c.id)
def test_plan_shapes_forward_under_poisoned_scratch(sweep, case):
    _, pu = sweep.model(case.model)
    x, t, kw = sweep.dev(PC.inputs(case, "a"))

    def run():
        TP._set_plan(pu, case.plan)
        return pu(x, t, **kw)

    _check_forward(pu, run, lambda: sweep.handle(pu, case), case.id)


# every FAST case (the 16- and 32-group ones take a statistics pass where the others fold), the everything-at-once case
# (lowres_cond + self_cond), the text cases given 5 and 20 tokens, and the direct-conv plan of the two models
# tests/test_unet_options_gpu.py runs it on
OPTION_CASES = (
    [(n, "default") for n in OC.FAST] + [("everything", "default")]
    + [(n, "default") for n, c in OC.FORWARD.items() if c["text"] and c["text"]["L"] in (5, 20)]
    + [("fast_groups_32", "direct"), ("fast_no_gca", "direct")]
)
assert {"fast_groups_16", "fast_groups_32"} <= set(OC.FAST) and sum(n.startswith("text_") for n, _ in OPTION_CASES) >= 2
assert OC.EVERYTHING["lowres_cond"] and OC.EVERYTHING["self_cond"]


def _option_model(name, plan, device):
    case = OC.ALL[name]
    ou = OC.oracle_unet(name)
    x, t, kw = OC.inputs(ou, case)
    pu = H.product_like(ou, device, **TO.PLANS[plan])
    return case, pu, x.to(device), t.to(device), {k: v.to(device) for k, v in kw.items()}


@pytest.mark.parametrize("name,plan", OPTION_CASES, ids=lambda v: str(v))
def test_unet_options_forward_under_poisoned_scratch(device, name, plan):
    case, pu, x, t, kw = _option_model(name, plan, device)
    _check_forward(pu, lambda: pu(x, t, **kw), lambda: TO._handle(pu, case, device), f"{name} ({plan})")


def _channels_model(Cx, device):
    """As tests/test_channels_gpu.py builds them: the base UNet with one channel, the SR UNet (low-res and cond images) with four."""
    name, lowres = ("small1", False) if Cx == 1 else ("small2", True)
    ou = H.ref_unet(R.Unet, H.UNET_KW[name], seed=11, channels=Cx, lowres_cond=lowres)
    x, t, kw = H.unet_inputs(ou, 2, 32, seed=3)
    return H.product_like(ou, device), x.to(device), t.to(device), {k: v.to(device) for k, v in kw.items()}


@pytest.mark.parametrize("Cx", [1, 4])
def test_c_channel_forward_under_poisoned_scratch(device, Cx):
    pu, x, t, kw = _channels_model(Cx, device)
    _check_forward(pu, lambda: pu(x, t, **kw), lambda: pu.engine(2, 32, device, with_text=False), f"channels={Cx}")


# ------------------------------------------------------------------------------- 2. samplers
def _handles(pim):
    return [h for u in pim.unets if hasattr(u, "_engines") for h in u._engines.values()]


def _check_sampler(pim, sample, label, n_plans):
    """sample() un-poisoned (it builds the plans, the sampler scratch, the graphs and the conditioning table), then once per
    word with every stage's plan poisoned before the call: images equal and finite."""
    base = sample()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(base).all()) and float(base.std()) > 0
    hs = _handles(pim)
    assert len(hs) == n_plans, (label, len(hs))
    bad = []
    for word in WORDS:
        filled = [_poison(h, word) for h in hs]
        assert min(filled) > 0
        out = sample()
        torch.cuda.synchronize()
        if not torch.equal(out, base):
            bad.append(f"{word:#010x}: {_diff(out, base)}")
    assert len(_handles(pim)) == n_plans
    print(f"poisoned scratch sampler {label}: {filled} bytes filled per plan, {len(bad)} of {len(WORDS)} words differ")
    assert not bad, (label, bad)
    return hs


_ref_unet = TO._ref_unet   # SR.Unet over H.ref_unet


def _ddpm(device, ous, sizes, T, **kw):
    return H.imagen_pair(device, SR.Imagen, "Imagen", ous, image_sizes=sizes, timesteps=(T,) * len(ous), **kw)[1]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_ddpm_sampling_under_poisoned_scratch(device, use_graph):
    """Base UNet, 4 steps, dynamic thresholding (the quantile's integer workspace is poisoned too), on-device noise from a
    fixed seed.  The calls after the first find their rows in the conditioning table - state, not filled - and restore the
    poisoned cond region from it: the table's build time and row count stay those of the first call."""
    lib = H.engine().load()
    pim = _ddpm(device, [_ref_unet(OC.BASE, seed=71)], (32,), 4, dynamic_thresholding=True, condition_on_text=False)
    sample = lambda: pim.sample(batch_size=3, seed=7, use_graph=use_graph, device=device)
    built = []

    def counted():
        out = sample()
        rows, runs = C.c_int(-1), C.c_int(-1)
        built.append((lib.kd_unet_cond_table_build_ms(_handles(pim)[0], C.byref(rows), C.byref(runs)), rows.value, runs.value))
        return out

    (h,) = _check_sampler(pim, counted, f"DDPM T=4 use_graph={use_graph}", 1)
    assert lib.kd_unet_num_cond_launches(h) > 0 and lib.kd_unet_cond_table_refused_bytes(h) == 0
    assert built[0][0] >= 0 and built[0][1] == 4, built          # the first call built the 4 rows ...
    assert all(b == built[0] for b in built[1:]), built          # ... and no later call built any


def test_text_guided_sampling_under_poisoned_scratch(device):
    """cond_scale 2.5: two forwards per step, the second into pred_null; the text conditioning of both is computed on the
    poisoned plan at the start of every call."""
    ou = _ref_unet(OC.TEXT, seed=73, text=True)
    pim = _ddpm(device, [ou], (16,), 3, text_embed_dim=3)
    text = torch.randn(2, 5, 3, generator=H.gen(4)).to(device)
    _check_sampler(pim, lambda: pim.sample(text_embeds=text, cond_scale=2.5, seed=9, device=device), "DDPM text, cond_scale 2.5", 1)


def test_sr_stage_with_inpainting_under_poisoned_scratch(device):
    """The SR stage alone (low-res conditioning), inpainting with inpaint_resample_times = 2: re-noise between the resamples."""
    pim = _ddpm(device, [R.NullUnet(), _ref_unet(OC.SR2, seed=75, lowres_cond=True)], (16, 32), 3, condition_on_text=False)
    g = H.gen(8)
    B = 2
    start, inp = torch.rand(B, 3, 16, 16, generator=g).to(device), torch.rand(B, 3, 32, 32, generator=g).to(device)
    mask = torch.zeros(B, 32, 32, dtype=torch.bool)
    mask[:, 4:20, 6:30] = True
    mask = mask.to(device)
    sample = lambda: pim.sample(batch_size=B, start_at_unet_number=2, start_image_or_video=start, inpaint_images=inp,
                                inpaint_masks=mask, inpaint_resample_times=2, seed=11, device=device)
    _check_sampler(pim, sample, "DDPM SR + inpainting R=2", 1)


def test_self_conditioned_sampling_under_poisoned_scratch(device):
    """Unet(self_cond=True): the carried x0 estimate is poisoned with the rest - step 0 of a call must start from zeros."""
    pim = _ddpm(device, [_ref_unet(OC.BASE, seed=77, self_cond=True)], (32,), 3, condition_on_text=False)
    assert pim.unets[0].self_cond
    _check_sampler(pim, lambda: pim.sample(batch_size=2, seed=13, device=device), "DDPM self_cond", 1)


def test_elucidated_sampling_under_poisoned_scratch(device):
    """3 Heun steps: x_hat, d and the preconditioned UNet input are scratch of the EDM iteration."""
    pim = H.imagen_pair(device, ER.ElucidatedImagen, "ElucidatedImagen", [_ref_unet(OC.BASE, seed=79)], image_sizes=(32,),
                        condition_on_text=False, num_sample_steps=3)[1]
    _check_sampler(pim, lambda: pim.sample(batch_size=2, seed=15, device=device), "EDM N=3", 1)


# ------------------------------------------------------------------------------- 3. caller-side slices
class Guarded:
    """A contiguous fp32 tensor as a slice of a NaN-filled allocation with GUARD floats of NaN in front and behind."""

    def __init__(self, shape, device, value=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = H.nan_dev(GUARD + n + GUARD).to(device)
        self.view = self.buf[GUARD:GUARD + n].view(*shape)
        if value is not None:
            self.view.copy_(value)
        assert self.view.is_contiguous() and self.view.data_ptr() == self.buf.data_ptr() + 4 * GUARD

    def guards_intact(self):
        bits = self.buf.view(torch.int32)
        return bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[-GUARD:] == NAN_BITS).all())


def _slice_models(device):
    """name -> builder of (product UNet, x, t, kw) on the device: MODEL_B at 64 x 64 batch 3, the 4-channel SR UNet, the
    everything-at-once case, and a text-conditioned one (tokens and hiddens as slices too)."""
    def plan_b():
        case = _plan_case("B", 64, 3)
        pu = H.product_like(PC.oracle_unet("B"), device)
        x, t, kw = PC.inputs(case, "a")
        return pu, x.to(device), t.to(device), {k: v.to(device) for k, v in kw.items()}

    def options(name):
        _, pu, x, t, kw = _option_model(name, "default", device)
        return pu, x, t, kw

    return {"B-S64-B3": plan_b, "channels=4": lambda: _channels_model(4, device), "everything": lambda: options("everything"),
            "text_len16_L5": lambda: options("text_len16_L5")}


@pytest.mark.parametrize("name", ["B-S64-B3", "channels=4", "everything", "text_len16_L5"])
def test_forward_on_slices_of_nan_filled_allocations(device, name):
    """kd_unet_forward_self_cond with x, the low-res image, the cond images, self_cond, both log-SNR rows, the text tokens and
    hiddens and the output each inside its own NaN-filled allocation: the init and final conv kernels address the caller's
    NCHW tensors directly, and must neither read nor write past them."""
    E = H.engine()
    lib = E.load()
    pu, x, t, kw = _slice_models(device)[name]()
    want = pu(x, t, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all())
    B, _, S, _ = x.shape
    with_text = "text_embeds" in kw
    h = pu.engine(B, S, device, with_text=with_text)
    gd = lambda v: None if v is None else Guarded(tuple(v.shape), device, v.float().contiguous())
    cond = kw.get("cond_images")
    if cond is not None:   # to the plan's size, as Unet.forward does before it hands them to the engine
        from imagen_pytorch.imagen_pytorch import resize_image_to

        cond = resize_image_to(cond.float(), S)
    g = dict(x=gd(x), self_cond=gd(kw.get("self_cond") if pu.self_cond else None), lowres=gd(kw.get("lowres_cond_img")),
             cond=gd(cond), t=gd(t), lowres_t=gd(kw.get("lowres_noise_times")), tok=None, hid=None)
    if with_text:
        tok, hid = pu.text_cond(h, kw["text_embeds"], kw.get("text_mask"), drop=False, device=device)
        g["tok"], g["hid"] = gd(tok), gd(hid)
    out = Guarded(tuple(x.shape), device)
    p = lambda k: None if g[k] is None else E.ptr(g[k].view)
    E.check(lib.kd_unet_forward_self_cond(h, p("x"), p("self_cond"), p("lowres"), p("cond"), p("t"), p("lowres_t"), p("tok"),
                                          p("hid"), E.ptr(out.view), E.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.view, want), (name, _diff(out.view, want))
    assert out.guards_intact(), f"{name}: the forward wrote outside its output"
    for k, v in g.items():
        assert v is None or v.guards_intact(), (name, k)
    n_in = sum(v is not None for v in g.values())
    print(f"poisoned scratch slices {name}: {n_in} inputs and the output inside {4 * GUARD}-byte NaN guards, output bit-equal")
