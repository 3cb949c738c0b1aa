"""sample(init_images=..., skip_steps=...) on the MI355X: both samplers against the restatement tests/init_images_ref.py on
identical weights and injected noise, and the invariants of the start call and of a run that begins at step `skip` - all
on the small 16 -> 32 cascade of test_seeds_gpu.py, T = 8 (EDM: N = 5), batch 3."""
import ctypes as C

import pytest
import torch

import helpers as H
import init_images_ref as IR
import self_cond_ref as SR
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

SAMPLE_ABS = 2e-3    # the project's sampler bound against the oracle on identical noise
TWO_PLANS = 4e-3     # test_seeds_gpu.py: two plans of different batch, each within 2e-3 of the oracle
B, T, N = 3, 8, 5
CASCADE_KW = dict(image_sizes=(16, 32), timesteps=(T, T), pred_objectives=("noise", "noise"), condition_on_text=False)
EDM_KW = dict(image_sizes=(16,), condition_on_text=False, num_sample_steps=N)


class SelfCondImagen(SR.Imagen, IR.Imagen):
    """The x_start carry of tests/self_cond_ref.py (reset per stage) over the start and step range of init_images_ref."""


def _unets(channels=3):
    return [H.ref_unet(RS.Unet, H.UNET_KW["small1"], seed=3, channels=channels),
            H.ref_unet(RS.Unet, H.UNET_KW["small1"], seed=6, channels=channels, lowres_cond=True)]


def _cascade(device, channels=3):
    kw = dict(CASCADE_KW, channels=channels)
    oim = IR.Imagen(_unets(channels), **kw)
    return oim, H.product_imagen(oim, "Imagen", device, **kw)


def _edm(device):
    oim = IR.ElucidatedImagen(_unets()[:1], **EDM_KW)
    return oim, H.product_imagen(oim, "ElucidatedImagen", device, **EDM_KW)


@pytest.fixture(scope="module")
def cascade(device):
    return _cascade(device)


@pytest.fixture(scope="module")
def edm(device):
    return _edm(device)


def _rand(*shape, seed):
    return torch.rand(*shape, generator=H.gen(seed))


def _inpaint(S, seed=5):
    inp = _rand(B, 3, S, S, seed=seed)
    mask = torch.zeros(B, S, S, dtype=torch.bool)
    mask[0, S // 8:S // 2 + 4, S // 5:S - 2] = mask[1, S // 3:, :S // 4 + 1] = mask[2, :S // 4, 3:S // 2 + 1] = True
    return dict(inpaint_images=inp, inpaint_masks=mask, inpaint_resample_times=2)


def _to(device, kw):
    mv = lambda v: v.to(device) if torch.is_tensor(v) else type(v)(mv(e) for e in v) if isinstance(v, (tuple, list)) else v
    return {k: mv(v) for k, v in kw.items()}


def _err(oim, pim, device, label, **kw):
    nf = RS.generator_noise_fn(41)
    ref = oim.sample(noise_fn=nf, batch_size=B, **kw)
    got = pim.sample(noise_fn=nf, batch_size=B, device=device, **_to(device, kw)).cpu()
    assert bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max())
    print(f"init_images {label}: max|diff| {err:.2e}")
    return err


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("inpaint", [False, True])
@pytest.mark.parametrize("form", ["one_tensor", "tuple_none_tensor"])
def test_ddpm_cascade_matches_the_restatement(device, cascade, form, inpaint):
    """One 24 x 20 tensor for both UNets (resized to 16 and to 32) or (None, a 37 x 50 tensor), skip_steps = (3, 5); with
    inpainting the mix, the step and the re-noise of R = 2 resamples run from step `skip` on."""
    oim, pim = cascade
    init = _rand(B, 3, 24, 20, seed=1) if form == "one_tensor" else (None, _rand(B, 3, 37, 50, seed=2))
    kw = dict(init_images=init, skip_steps=(3, 5), **(_inpaint(32) if inpaint else {}))
    assert _err(oim, pim, device, f"DDPM cascade {form} skip (3, 5){' inpaint R=2' if inpaint else ''}", **kw) < SAMPLE_ABS


def test_self_conditioned_unet_matches_the_restatement(device):
    ou = H.ref_unet(SR.Unet, H.UNET_KW["small1"], seed=21, self_cond=True)
    kw = dict(image_sizes=(16,), timesteps=(T,), pred_objectives=("noise",), condition_on_text=False)
    oim = SelfCondImagen([ou], **kw)
    pim = H.product_imagen(oim, "Imagen", device, **kw)
    assert pim.unets[0].self_cond
    assert _err(oim, pim, device, "DDPM self-cond skip 3", init_images=_rand(B, 3, 16, 16, seed=3), skip_steps=3) < SAMPLE_ABS


@pytest.mark.parametrize("inpaint", [False, True])
def test_edm_matches_the_restatement(device, edm, inpaint):
    oim, pim = edm
    kw = dict(init_images=_rand(B, 3, 32, 32, seed=4), skip_steps=2, **(_inpaint(16) if inpaint else {}))
    assert _err(oim, pim, device, f"EDM N=5 skip 2{' inpaint R=2' if inpaint else ''}", **kw) < SAMPLE_ABS


def test_one_channel_cascade_matches_the_restatement(device):
    oim, pim = _cascade(device, channels=1)
    assert _err(oim, pim, device, "DDPM cascade channels=1 skip (3, 5)", init_images=_rand(B, 1, 24, 20, seed=5),
                skip_steps=(3, 5)) < SAMPLE_ABS


# ------------------------------------------------------------------------------------------------ invariants, bit for bit
@pytest.mark.parametrize("sampler", ["ddpm", "edm"])
def test_a_zero_image_and_no_skip_is_the_plain_call(device, cascade, edm, sampler):
    """init_images = 0.5 normalises to 0 and adds nothing; skip_steps = 0 is the whole loop."""
    pim = (cascade if sampler == "ddpm" else edm)[1]
    half = torch.full((B, 3, 24, 20), 0.5, device=device)
    for seed in (17, [11, 22, 33]):
        plain = pim.sample(batch_size=B, seed=seed, device=device)
        assert torch.equal(pim.sample(batch_size=B, seed=seed, device=device, init_images=half, skip_steps=0), plain)
        assert not torch.equal(pim.sample(batch_size=B, seed=seed, device=device, init_images=half * 1.5), plain)


def test_a_skipped_call_is_the_step_range_run_by_hand_on_the_start_calls_x_T(device, cascade):
    """sample(stop_at_unet_number=1, skip_steps=s) against kd_sample_start, kd_sample_steps(s, T) and kd_sample_finalize."""
    from imagen_pytorch.imagen_pytorch import STAGE_SEED_STRIDE

    E = H.engine()
    lib = E.load()
    pim = cascade[1]
    s, seed = 3, 29
    init = _rand(B, 3, 24, 20, seed=6).to(device)
    got = pim.sample(batch_size=B, seed=seed, device=device, init_images=init, skip_steps=s, stop_at_unet_number=1)
    h = pim.unets[0].engine(B, 16, device, with_text=False)
    stage_seed = (seed + STAGE_SEED_STRIDE) % 2 ** 64
    x = torch.full((B, 3, 16, 16), float("nan"), device=device)
    E.check(lib.kd_sample_start(E.ptr(x), B, 3, 16, 1.0, stage_seed, None, None, E.ptr(init), 24, 20, E.current_stream()))
    tables = pim.noise_schedulers[0].step_tables()
    sc = E.kd_schedule_t()
    sc.T = T
    for name, v in tables.items():
        setattr(sc, name, v.numpy().ctypes.data_as(C.POINTER(C.c_float)))
    sa = E.kd_sample_args_t()
    sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times, sa.use_graph = 0, 1, 0.95, 1, 1
    sa.seed = stage_seed
    E.check(lib.kd_sample_steps(h, C.byref(sc), C.byref(sa), E.ptr(x), s, T, E.current_stream()))
    E.check(lib.kd_sample_finalize(h, C.byref(sa), E.ptr(x), E.current_stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, x)


@pytest.mark.parametrize("sampler", ["ddpm", "edm"])
def test_graph_on_equals_off_and_trace_holds_the_steps_walked(device, cascade, edm, sampler):
    pim = (cascade if sampler == "ddpm" else edm)[1]
    steps, skip = (T, 5) if sampler == "ddpm" else (N, 2)
    kw = dict(batch_size=B, seed=[5, 6, 7], device=device, init_images=_rand(B, 3, 16, 16, seed=7).to(device),
              skip_steps=skip, stop_at_unet_number=1)
    a = pim.sample(use_graph=True, **kw)
    assert torch.equal(a, pim.sample(use_graph=False, **kw))
    trace = []
    assert torch.equal(a, pim.sample(trace=trace, **kw))
    assert len(trace) == steps - skip and all(tuple(t.shape) == (B, 3, 16, 16) for t in trace)


def test_cond_table_on_equals_off_with_the_skipped_call_first_on_a_fresh_plan(device):
    """The table's rows are built for the steps walked: a fresh plan whose first call starts at step 3 / 5."""
    init = _rand(B, 3, 24, 20, seed=8).to(device)
    outs = []
    for table in (0, -1):
        pim = _cascade(device)[1]   # fresh plans
        pim.cond_table = table
        outs.append(pim.sample(batch_size=B, seed=3, device=device, init_images=init, skip_steps=(3, 5)))
        if table == 0:   # ... and the full call behind it builds the rest
            full = pim.sample(batch_size=B, seed=3, device=device)
    assert torch.equal(outs[0], outs[1])
    fresh = _cascade(device)[1]
    assert torch.equal(full, fresh.sample(batch_size=B, seed=3, device=device))


@pytest.mark.parametrize("sampler", ["Imagen", "ElucidatedImagen"])
def test_a_self_conditioned_skipped_call_does_not_read_an_earlier_calls_estimate(device, sampler):
    """The stale-estimate trap: a full call leaves its last x0 estimate in the plan; the skipped call behind it starts its
    first step from zeros, as on a freshly built plan."""
    ou = H.ref_unet(SR.Unet, H.UNET_KW["small1"], seed=21, self_cond=True)
    kw = dict(image_sizes=(16,), condition_on_text=False)
    kw.update(dict(timesteps=(T,)) if sampler == "Imagen" else dict(num_sample_steps=N))
    oim = (SelfCondImagen if sampler == "Imagen" else SR.ElucidatedImagen)([ou], **kw)
    call = dict(batch_size=B, seed=9, device=device, init_images=_rand(B, 3, 16, 16, seed=9).to(device), skip_steps=2)
    used = H.product_imagen(oim, sampler, device, **kw)
    used.sample(batch_size=B, seed=1, device=device)
    after_full = used.sample(**call)
    assert torch.equal(after_full, H.product_imagen(oim, sampler, device, **kw).sample(**call))
    assert torch.equal(after_full, used.sample(trace=[], **call))


# ------------------------------------------------------------------------------------------------ per-image seeds, chunks
def test_per_image_seeds_with_init_images_do_not_depend_on_the_batch(device, cascade):
    from imagen_pytorch import ImagenTrainer

    pim = cascade[1]
    seeds = [11, 22, 33]
    init = (_rand(B, 3, 16, 16, seed=10).to(device), _rand(B, 3, 37, 50, seed=11).to(device))
    kw = dict(device=device, skip_steps=(3, 5))
    full = pim.sample(batch_size=B, seed=seeds, init_images=init, **kw)
    singles = torch.cat([pim.sample(batch_size=1, seed=s, init_images=tuple(t[b:b + 1] for t in init), **kw)
                         for b, s in enumerate(seeds)])
    chunked = ImagenTrainer(pim, use_ema=False).sample(batch_size=B, max_batch_size=2, seed=seeds, init_images=init,
                                                       skip_steps=(3, 5))
    d1, d2 = float((full - singles).abs().max()), float((full - chunked).abs().max())
    print(f"init_images, seed list: batch 3 vs three batch-1 calls max|diff| {d1:.2e}, vs trainer chunks 2 + 1 {d2:.2e}")
    assert d1 < TWO_PLANS and d2 < TWO_PLANS
    # the image decides: the inverted init of image 1 under the same key moves it by more than the bound
    other = pim.sample(batch_size=1, seed=seeds[1], init_images=tuple(1 - t[1:2] for t in init), **kw)
    assert float((other - singles[1:2]).abs().max()) > TWO_PLANS
