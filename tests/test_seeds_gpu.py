"""Per-image Philox keys on the MI355X: image b of a call with `seeds` draws, bit for bit, what a batch-1 call keyed
seeds[b] draws - in the row fill kd_philox_normal_rows, in each of the five in-kernel consumers (one step through
kd_sample_steps / kd_edm_sample_steps against the same step on injected noise tensors), under graph replay, and through
the whole samplers, the trainer's chunks and the patch grid.  The int seed keeps its layout: one stream over the whole
batch tensor.

Shapes: B = 3, C = 3, S = 16 (192 float4 per image: image boundaries inside a block's 256 threads) and B = 5, C = 1, S = 16
(64 float4 per image: boundaries at every wave); B = 33 passes the 32 keys one key-upload launch carries."""
import ctypes as C

import numpy as np
import pytest
import torch

import elucidated_ref as ER
import helpers as H
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

S = 16
SHAPES = [(3, 3), (5, 1)]   # (B, C)
SEEDS = [0x9E3779B97F4A7C15, 7, 0x1_0000_0001, 2 ** 64 - 1, 12345]   # at, below and above 2^32
INT_SEED = 0xD1B54A32D192ED03
PHILOX_ATOL = 2e-5   # tests/test_kernels_gpu.py: libm against ocml
SAMPLE_ABS = 4e-3    # twice the sampler tolerance: each run is within 2e-3 of the oracle on identical noise


def _philox(out, n, seed, sid):
    E = H.engine()
    E.check(E.load().kd_philox_normal(E.ptr(out), n, seed, sid, E.current_stream()))


# ------------------------------------------------------------------------------------------------ row fills
@pytest.mark.parametrize("B,n", [(3, 768), (5, 256), (33, 256)])
def test_row_fill_equals_the_batch_1_fill_of_each_key(device, B, n):
    from oracle.philox_ref import philox_normal

    E = H.engine()
    seeds = [SEEDS[b % len(SEEDS)] + (b // len(SEEDS)) for b in range(B)]
    sid = E.stream_id(16, 2)
    out = torch.full((B, n), 7.0, device=device)
    E.check(E.load().kd_philox_normal_rows(E.ptr(out), B, n, E.seed_array(seeds), sid, E.current_stream()))
    worst = 0.0
    for b, s in enumerate(seeds):
        row = torch.empty(n, device=device)
        _philox(row, n, s, sid)
        assert torch.equal(out[b], row), f"row {b}"
        if b < 5:
            worst = max(worst, float(np.abs(row.cpu().numpy().astype(np.float64) - philox_normal(n, s, sid)).max()))
    print(f"philox rows B{B} n{n}: max|row - philox_ref| {worst:.2e}")
    assert worst < PHILOX_ATOL
    assert not torch.equal(out[0], out[1])


def test_row_fill_refuses_a_row_length_that_is_no_multiple_of_4(device):
    E = H.engine()
    out = torch.full((3, 8), 7.0, device=device)
    with pytest.raises(E.EngineError, match="multiple of 4"):
        E.check(E.load().kd_philox_normal_rows(E.ptr(out), 3, 6, E.seed_array([1, 2, 3]), E.stream_id(16, 2), E.current_stream()))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())   # nothing was launched


# ------------------------------------------------------------------------------------------------ one step per consumer
# purpose of each noise tensor (include/kd_engine.h): DDPM step 1, inpaint mix 2, re-noise 3; EDM churn 4, re-noise 5
CASES = {
    "ddpm": dict(edm=False, inpaint=False, R=1, k=2, purposes=dict(d_noise_step=1)),
    "ddpm_inpaint_r2": dict(edm=False, inpaint=True, R=2, k=2, purposes=dict(d_noise_step=1, d_noise_inpaint=2, d_noise_renoise=3)),
    "edm_churn": dict(edm=True, inpaint=False, R=1, k=1, purposes=dict(d_noise_step=4)),
    "edm_renoise_r2": dict(edm=True, inpaint=True, R=2, k=1, purposes=dict(d_noise_step=4, d_noise_renoise=5)),
}
T_DDPM, N_EDM = 6, 3


def _unet(Cimg):
    return H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=4, channels=Cimg)


class Ctx:
    """One plan of small1 at (B, C, 16, 16) with the inputs of its steps."""

    def __init__(self, device, B, Cimg, h=None):
        self.device, self.B, self.C = device, B, Cimg
        self.shape = (B, Cimg, S, S)
        self.n = Cimg * S * S
        self.pu = H.product_like(_unet(Cimg), device)
        self.h = self.pu.engine(B, S, device, with_text=False)
        g = torch.Generator().manual_seed(100 * B + Cimg)
        self.x_in = torch.randn(self.shape, generator=g) * 1.5
        self.inp = (torch.rand(self.shape, generator=g) * 2 - 1).to(device)
        mask = torch.zeros(B, 1, S, S)
        for b in range(B):   # edges inside a float4, another rectangle per image
            mask[b, :, 2 + b % 3:9 + b % 4, 3 - b % 2:14 - b % 5] = 1
        self.mask = mask.to(device)


@pytest.fixture(scope="module")
def ctxs(device):
    made = {}

    def get(B, Cimg):
        if (B, Cimg) not in made:
            made[(B, Cimg)] = Ctx(device, B, Cimg)
        return made[(B, Cimg)]

    return get


def _ddpm_schedule():
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes

    E = H.engine()
    tables = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=T_DDPM).step_tables()
    sc = E.kd_schedule_t()
    sc.T = T_DDPM
    for name, v in tables.items():
        setattr(sc, name, v.numpy().ctypes.data_as(C.POINTER(C.c_float)))
    return sc, tables


def _edm_schedule():
    from imagen_pytorch.imagen_pytorch import edm_step_tables

    E = H.engine()
    tab = edm_step_tables(num_sample_steps=N_EDM)
    sc = E.kd_edm_schedule_t()
    sc.N, sc.S_noise = N_EDM, 1.003
    for name, _ in E.kd_edm_schedule_t._fields_[2:]:
        setattr(sc, name, tab[name].numpy().ctypes.data_as(C.POINTER(C.c_float)))
    assert float(tab["churn"][1]) > 0 and float(tab["renoise"][1]) > 0 and float(tab["sigma_next"][1]) != 0   # the step tested
    return sc, tab


def _noise_tensor(ctx, slots, its, purpose, seed):
    """[slots, B, C, S, S] with the slots `its` filled from Philox: per image (seed a list: row b under seed[b], counter
    inside the image) or as one stream over the whole batch tensor (seed an int)."""
    E = H.engine()
    z = torch.zeros(slots, ctx.B, ctx.n, device=ctx.device)
    for it in its:
        sid = E.stream_id(purpose, it)
        if isinstance(seed, list):
            for b, s in enumerate(seed):
                _philox(z[it, b], ctx.n, s, sid)
        else:
            _philox(z[it], ctx.B * ctx.n, seed, sid)
    return z


def _run(ctx, name, seed, inject, use_graph=1, h=None):
    """Step k of the case on ctx.x_in -> x.  inject: the noise comes from tensors filled by kd_philox_normal instead of the
    kernels' own draws."""
    E = H.engine()
    lib = E.load()
    case = CASES[name]
    Rr, k = case["R"], case["k"]
    sa = E.kd_sample_args_t()
    sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times, sa.use_graph = 0, 1, 0.95, Rr, use_graph
    keep = []
    if isinstance(seed, list):
        keep.append(E.seed_array(seed))
        sa.seeds = keep[-1]
        sa.seed = 99   # not read
    else:
        sa.seed = seed
    if case["inpaint"]:
        sa.d_inpaint_images, sa.d_inpaint_masks = E.ptr(ctx.inp), E.ptr(ctx.mask)
    slots = (N_EDM if case["edm"] else T_DDPM) * Rr
    if inject:
        for field, purpose in case["purposes"].items():
            keep.append(_noise_tensor(ctx, slots, range(k * Rr, (k + 1) * Rr), purpose, seed))
            setattr(sa, field, E.ptr(keep[-1]))
    x = (ctx.x_in * (2.0 if case["edm"] else 1.0)).to(ctx.device)
    h = ctx.h if h is None else h
    if case["edm"]:
        sc, tab = _edm_schedule()
        E.check(lib.kd_edm_sample_steps(h, C.byref(sc), C.byref(sa), E.ptr(x), k, k + 1, E.current_stream()))
    else:
        sc, tab = _ddpm_schedule()
        E.check(lib.kd_sample_steps(h, C.byref(sc), C.byref(sa), E.ptr(x), k, k + 1, E.current_stream()))
    torch.cuda.synchronize()
    del keep, tab
    return x


def _maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


# (the second key-upload launch of a batch of 33 is the same for every consumer: one case runs it)
@pytest.mark.parametrize("name,B,Cimg", [(name, B, Cimg) for name in CASES for B, Cimg in SHAPES] + [("ddpm_inpaint_r2", 33, 1)])
def test_step_with_per_image_seeds_equals_the_step_on_batch_1_noise(ctxs, name, B, Cimg):
    """seeds = [s_0 ..] and no noise tensors against noise tensors whose row b is kd_philox_normal(n, s_b, stream id of the
    purpose and iteration): the same bits."""
    ctx = ctxs(B, Cimg)
    seeds = [SEEDS[b % len(SEEDS)] + (b // len(SEEDS)) for b in range(B)]
    got = _run(ctx, name, seeds, inject=False)
    want = _run(ctx, name, seeds, inject=True)
    print(f"{name} B{B} C{Cimg} per-image seeds: max|in-kernel - injected| {_maxdiff(got, want):.2e}")
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    # ... and it is the seeds that decide: another key for image 1 changes image 1 alone
    other = list(seeds)
    other[1] ^= 1
    got2 = _run(ctx, name, other, inject=False)
    assert not torch.equal(got2[1], got[1]) and torch.equal(got2[0], got[0]) and torch.equal(got2[2:], got[2:])


@pytest.mark.parametrize("B,Cimg", SHAPES)
@pytest.mark.parametrize("name", list(CASES))
def test_step_with_an_int_seed_keeps_the_whole_batch_stream(ctxs, name, B, Cimg):
    """seed = int: element i of the batch tensor is element i of ONE stream, kd_philox_normal(B n, seed, sid) - the layout of
    before, pinned; and it is not the per-image layout under equal keys."""
    ctx = ctxs(B, Cimg)
    got = _run(ctx, name, INT_SEED, inject=False)
    want = _run(ctx, name, INT_SEED, inject=True)
    print(f"{name} B{B} C{Cimg} int seed: max|in-kernel - injected| {_maxdiff(got, want):.2e}")
    assert torch.equal(got, want)
    same_keys = _run(ctx, name, [INT_SEED] * B, inject=False)
    assert torch.equal(same_keys[0], got[0]) and not torch.equal(same_keys[1], got[1])


# ------------------------------------------------------------------------------------------------ graph independence
@pytest.mark.parametrize("name", ["ddpm_inpaint_r2", "edm_renoise_r2"])
def test_one_captured_step_serves_int_seeds_and_seed_lists(device, ctxs, name):
    B, Cimg = SHAPES[0]
    ctx = ctxs(B, Cimg)
    seeds = SEEDS[:B]
    a = _run(ctx, name, seeds, inject=False, use_graph=1)
    assert torch.equal(a, _run(ctx, name, seeds, inject=False, use_graph=0))   # replay == eager launches
    assert torch.equal(a, _run(ctx, name, seeds, inject=False, use_graph=1))   # twice the same
    # int -> list -> other list -> int on ONE plan against each on a plan of its own
    live = Ctx(device, B, Cimg)
    order = [INT_SEED, seeds, list(reversed(seeds)), INT_SEED]
    got = [_run(ctx, name, s, inject=False, h=live.h) for s in order]
    for s, g in zip(order[:3], got):
        fresh = Ctx(device, B, Cimg)
        assert torch.equal(g, _run(ctx, name, s, inject=False, h=fresh.h)), s
    assert torch.equal(got[3], got[0]) and torch.equal(got[1], a) and not torch.equal(got[2], got[1])


# ------------------------------------------------------------------------------------------------ whole samplers
def _cascade(device):
    ous = [H.oracle_unet("small1", seed=3), H.oracle_unet("small1", lowres_cond=True, seed=6)]
    kw = dict(image_sizes=(16, 32), timesteps=(8, 8), pred_objectives=("noise", "noise"), condition_on_text=False)
    return H.product_imagen(RS.Imagen(ous, **kw), "Imagen", device, **kw)


def _edm(device):
    kw = dict(image_sizes=(16,), condition_on_text=False, num_sample_steps=4)
    return H.product_imagen(ER.ElucidatedImagen([H.oracle_unet("small1", seed=3)], **kw), "ElucidatedImagen", device, **kw)


@pytest.mark.parametrize("sampler", ["ddpm_cascade", "edm"])
def test_an_image_of_a_seed_does_not_depend_on_its_batch(device, sampler):
    """sample(batch_size=3, seed=[11, 22, 33]) against the three batch-1 calls, against the trainer's chunks of 2 + 1 and
    against the same batch in another order.  Identical noise in every form, so what is left is the difference between
    plans of different batch sizes: each is held to the oracle within the sampler tolerance 2e-3, hence 4e-3."""
    from imagen_pytorch import ImagenTrainer

    seeds = [11, 22, 33]
    kw = dict(device=device)
    if sampler == "ddpm_cascade":
        pim = _cascade(device)
        g = torch.Generator().manual_seed(5)
        inp = torch.rand(3, 3, 32, 32, generator=g).to(device)
        mask = torch.zeros(3, 32, 32, dtype=torch.bool)
        mask[0, 4:20, 6:30] = mask[1, 10:32, 0:9] = mask[2, 0:7, 3:17] = True
        mask = mask.to(device)
        cut = lambda sl: dict(inpaint_images=inp[sl], inpaint_masks=mask[sl], inpaint_resample_times=2)
    else:
        pim = _edm(device)
        cut = lambda sl: {}
    full = pim.sample(batch_size=3, seed=seeds, **cut(slice(None)), **kw)
    assert bool(torch.isfinite(full).all()) and float(full.min()) >= 0 and float(full.max()) <= 1
    assert torch.equal(full, pim.sample(batch_size=3, seed=torch.tensor(seeds), **cut(slice(None)), **kw))
    singles = torch.cat([pim.sample(batch_size=1, seed=s, **cut(slice(b, b + 1)), **kw) for b, s in enumerate(seeds)])
    chunked = ImagenTrainer(pim, use_ema=False).sample(batch_size=3, max_batch_size=2, seed=seeds, **cut(slice(None)))
    perm = [2, 0, 1]
    permuted = pim.sample(batch_size=3, seed=[seeds[p] for p in perm], **cut(perm), **kw)
    d1, d2, d3 = _maxdiff(full, singles), _maxdiff(full, chunked), _maxdiff(full[perm], permuted)
    print(f"{sampler}: batch 3 vs three batch-1 calls max|diff| {d1:.2e}, vs trainer chunks 2 + 1 {d2:.2e}, "
          f"vs the batch in the order {perm} {d3:.2e} (bit-equal: {torch.equal(full[perm], permuted)})")
    assert d1 < SAMPLE_ABS and d2 < SAMPLE_ABS and d3 < SAMPLE_ABS
    # the int seed of the same value is another image for b > 0 (one stream over the batch), the same for batch 1
    assert _maxdiff(full[1], pim.sample(batch_size=3, seed=11, **cut(slice(None)), **kw)[1]) > 10 * SAMPLE_ABS
    assert torch.equal(singles[:1], pim.sample(batch_size=1, seed=[11], **cut(slice(0, 1)), **kw))


# ------------------------------------------------------------------------------------------------ patch grid
def test_grid_canvas_with_per_patch_seeds_does_not_depend_on_max_batch(device):
    """outpaint_canvas 2 x 2 over the three-stage dim-32 pair of test_drivers_gpu.py, seed = 3, per_patch_seeds: one patch
    per call against the waves' patches sharing calls.  Same bound as above."""
    from ultra_res import distributed as D

    ous = [H.fast_oracle(H.ref_unet(R.Unet, H.UNET_KW[name], seed=500 + s, cond_images_channels=0, lowres_cond=s > 1))
           for s, name in ((1, "ultra1"), (2, "ultra2"), (3, "ultra3"))]
    kw = dict(image_sizes=(64, 256, 1024), pred_objectives=("noise", "noise", "noise"), condition_on_text=False,
              timesteps=(2, 2, 1))
    pim = H.product_imagen(RS.Imagen(ous, **kw), "Imagen", device, random_crop_sizes=(None, None, 256), **kw)
    canvases = []
    for max_batch in (1, 4):
        fn = D.imagen_sample_fn(lambda stage: pim, 2, device, seed=3, max_batch=max_batch, per_patch_seeds=True)
        canvases.append(D.outpaint_canvas(fn, 2, overlap=0.25, device=device)[0])
    a, b = canvases
    assert tuple(a.shape) == (1, 3, 1792, 1792) and bool(torch.isfinite(a).all())
    d = _maxdiff(a, b)
    print(f"outpaint 2x2, per-patch seeds: max_batch 1 vs 4 max|diff| {d:.2e}")
    assert d < SAMPLE_ABS
