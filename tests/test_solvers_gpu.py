"""Few-step solvers on the MI355X: DDIM(eta) and DPM-Solver++(2M) through kd_solver_sample_steps / kd_solver_sample_loop.

1. solver_update_kernel one step at a time, in the manner of tests/test_ddpm_step_gpu.py: the engine's own UNet output, x0
   estimate and thresholds are read back with kd_sample_last and the update is recomputed from them in fp64 over the fp32
   coefficient tables, so the UNet's error is not in the comparison (rel-L2 1e-6, that file's bound: the expressions are of
   the same form and length).
2. its noise: the Philox stream of the ancestral step, bit for bit; none for the deterministic solvers.
3. - 4. whole samplers on the 16 -> 32 cascade of tests/test_seeds_gpu.py (N = 8, batch 3) against today's sampler (eta = 1)
   and against the restatement tests/solver_ref.py on identical weights and injected noise (max-abs 2e-3, the project's
   sampler bound).
5. - 7. invariants, bit for bit; per-image seeds; the patch-grid driver."""
import ctypes as C

import pytest
import torch

import helpers as H
import self_cond_ref as SC
import solver_ref as SR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

REL = 1e-6           # tests/test_ddpm_step_gpu.py
SAMPLE_ABS = 2e-3    # the project's sampler bound against the oracle on identical noise
TWO_PLANS = 4e-3     # tests/test_seeds_gpu.py: two plans of different batch, each within 2e-3 of the oracle
B1, S1 = 2, 16
SHP = (B1, 3, S1, S1)
N1 = 3 * S1 * S1
OBJ = {"noise": 0, "v": 1, "x_start": 2}
SOLVERS = [("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp_2m", 0.0)]


# ------------------------------------------------------------------------------------------------ single steps
@pytest.fixture(scope="module")
def plan(device):
    pu = H.product_like(H.oracle_unet("small1", seed=4), device)
    return pu, pu.engine(B1, S1, device, with_text=False)


def _schedule(T, name, eta=0.0, skip=0):
    """(kd_solver_schedule_t, step tables, coefficient tables); the struct points into the tables: keep all three."""
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes, solver_tables

    E = H.engine()
    tab = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=T).step_tables()
    coef = solver_tables(tab, name, eta=eta, skip=skip)
    sc = E.kd_solver_schedule_t()
    sc.T = T
    for n in ("log_snr", "alpha", "sigma", "rn_a", "rn_b"):
        setattr(sc, n, tab[n].numpy().ctypes.data_as(C.POINTER(C.c_float)))
    for n, v in coef.items():
        setattr(sc, n, v.numpy().ctypes.data_as(C.POINTER(C.c_float)))
    return sc, tab, coef


def _args(objective, dynamic_threshold, use_graph=1, seed=9):
    sa = H.engine().kd_sample_args_t()
    sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times = OBJ[objective], dynamic_threshold, 0.95, 1
    sa.seed, sa.use_graph = seed, use_graph
    return sa


def _steps(h, sc, sa, x, k0, k1=None):
    E = H.engine()
    E.check(E.load().kd_solver_sample_steps(h, C.byref(sc), C.byref(sa), E.ptr(x), k0, k0 + 1 if k1 is None else k1,
                                            E.current_stream()))


def _last(h, device, shp=SHP):
    return [H.sample_last(h, which, shape, device) for which, shape in ((0, shp), (1, shp), (2, (shp[0],)))]


def _x0_of(objective, x, pred, alpha, sigma):
    if objective == "noise":
        return (x - sigma * pred) / max(alpha, 1e-8)
    if objective == "v":
        return alpha * x - sigma * pred
    return pred


def _x0c(x0, s):
    s = s[:, None, None, None]
    return torch.maximum(torch.minimum(x0, s), -s) / s


@pytest.mark.parametrize("T,k", [(6, 0), (6, 2), (6, 5), (1000, 0), (1000, 333), (1000, 999)])
@pytest.mark.parametrize("objective", ["noise", "v", "x_start"])
def test_solver_step_matches_fp64_expression(device, plan, T, k, objective):
    """x <- A x + B x0c + P hist + S z at both ends and the middle of a short and a long cosine schedule, the three
    objectives, dynamic and static threshold, DDIM at eta 0, 0.5, 1 with z the slot k of an injected tensor, and 2M: its
    history is what step k - 1, run first on another image, kept - recomputed from that step's read-back.  At k = 0 the
    result is finite; at k = T - 1 (S = 0) it does not depend on the noise."""
    pu, h = plan
    gen = torch.Generator().manual_seed(100 * k + T)
    x_in = torch.randn(*SHP, generator=gen) * 1.5
    x_before = torch.randn(*SHP, generator=gen) * 1.5
    noise = torch.randn(T, *SHP, generator=gen).to(device)
    for name, eta in SOLVERS:
        sc, tab, coef = _schedule(T, name, eta)
        A, Bc, P, Sn = (float(coef[n][k]) for n in ("coef_x", "coef_x0", "coef_prev", "coef_noise"))
        assert (P != 0) == (name == "dpmpp_2m" and 0 < k < T - 1) and (Sn != 0) == (eta > 0 and k < T - 1)
        for dyn in (1, 0):
            sa = _args(objective, dyn)
            sa.d_noise_step = H.engine().ptr(noise)
            one = torch.ones(B1, dtype=torch.float64)
            hist = 0.0
            if P != 0:   # the history of step k - 1
                y = x_before.to(device)
                _steps(h, sc, sa, y, k - 1)
                _, x0p, thrp = _last(h, device)
                hist = _x0c(x0p, thrp.clamp(min=1.0) if dyn else one)
            x = x_in.to(device)
            _steps(h, sc, sa, x, k)
            pred, x0, thr = _last(h, device)
            got, xd = x.double().cpu(), x_in.double()
            assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(x0).all())
            e_x0 = H.rel_l2(x0, _x0_of(objective, xd, pred, float(tab["alpha"][k]), float(tab["sigma"][k])))
            xs = _x0c(x0, thr.clamp(min=1.0) if dyn else one)
            want = A * xd + Bc * xs + P * hist + Sn * noise[k].double().cpu()
            e_x = H.rel_l2(got, want)
            print(f"solver step {name} eta {eta} T{T} k{k} {objective} dyn{dyn}: x0 rel-L2 {e_x0:.2e}, x_next rel-L2 {e_x:.2e}")
            assert e_x0 < REL and e_x < REL
            if P != 0:   # (the history term is large enough to be seen)
                assert H.rel_l2(got, want - P * hist) > 20 * REL
            if k == T - 1 or eta == 0:   # no noise term: another noise tensor, the same bits
                other = torch.flip(noise, dims=(0,)) * 3 + 1
                sa.d_noise_step = H.engine().ptr(other)
                x2 = x_in.to(device)
                if P != 0:
                    _steps(h, sc, sa, x_before.to(device), k - 1)
                _steps(h, sc, sa, x2, k)
                torch.cuda.synchronize()
                assert torch.equal(x2, x)


def test_history_follows_the_schedule_step_not_the_resample_slot(device, plan):
    """2M with inpainting, R = 2, steps 1 and 2 of T = 6 in one call: both resamples of step 2 read the estimate that the
    LAST resample of step 1 kept.  The last iteration is recomputed from the read-back of the call's last forward, the
    history from a call that stops after step 1."""
    E = H.engine()
    pu, h = plan
    T, R, k = 6, 2, 2
    sc, tab, coef = _schedule(T, "dpmpp_2m", skip=1)   # step 1 is the first step walked: first order, as sample() builds it
    assert float(coef["coef_prev"][1]) == 0.0 and float(coef["coef_prev"][2]) != 0.0
    gen = torch.Generator().manual_seed(12)
    inp = (torch.rand(SHP, generator=gen) * 2 - 1).to(device)
    mask = torch.zeros(B1, 1, S1, S1)
    mask[0, :, 2:9, 3:14] = 1
    mask[1, :, 5:12, 1:6] = 1
    mask = mask.to(device)
    zs = [torch.randn(T * R, *SHP, generator=gen).to(device) for _ in range(2)]
    x_in = torch.randn(*SHP, generator=gen) * 1.5
    sa = _args("noise", 1)
    sa.resample_times = R
    sa.d_inpaint_images, sa.d_inpaint_masks = E.ptr(inp), E.ptr(mask)
    sa.d_noise_inpaint, sa.d_noise_renoise = E.ptr(zs[0]), E.ptr(zs[1])
    f = lambda n: float(coef[n][k])
    # steps 1 .. 1: the history step 2 will read
    y = x_in.to(device)
    _steps(h, sc, sa, y, 1, 2)
    _, x0p, thrp = _last(h, device)
    hist = _x0c(x0p, thrp.clamp(min=1.0))
    # the first resample of step 2 alone is not reachable through the ABI; what the second forward saw is alpha x0 + sigma pred
    x = x_in.to(device)
    _steps(h, sc, sa, x, 1, 3)
    pred, x0, thr = _last(h, device)
    seen = float(tab["alpha"][k]) * x0 + float(tab["sigma"][k]) * pred
    want = f("coef_x") * seen + f("coef_x0") * _x0c(x0, thr.clamp(min=1.0)) + f("coef_prev") * hist
    e = H.rel_l2(x, want)
    print(f"2M inpaint R2, last iteration of step 2: rel-L2 {e:.2e}")
    assert e < 2e-6   # `seen` is rebuilt from x0 (three more fp32 roundings than the plain step test)
    # (had the first resample of step 2 overwritten the history, the second would have read step 2's own estimate: the
    # term is large enough for that to show)
    assert H.rel_l2(x, want - f("coef_prev") * hist) > 1e-3


def test_thresholded_estimate_reaches_the_self_conditioning_planes(device):
    """sc_out on a self-conditioned plan: after a solver step the plan's self-cond planes hold this step's x0c."""
    ou = H.ref_unet(SC.Unet, H.UNET_KW["small1"], seed=21, self_cond=True)
    pu = H.product_like(ou, device)
    h = pu.engine(B1, S1, device, with_text=False)
    x_in = torch.randn(*SHP, generator=H.gen(3)) * 1.5
    for name, eta in (("ddim", 0.0), ("dpmpp_2m", 0.0)):
        sc, tab, coef = _schedule(6, name, eta)
        x = x_in.to(device)
        _steps(h, sc, _args("v", 1), x, 0, 2)
        _, x0, thr = _last(h, device)
        planes = H.sample_last(h, 5, SHP, device)
        assert H.rel_l2(planes, _x0c(x0, thr.clamp(min=1.0))) < REL and float(planes.abs().max()) <= 1.0


def test_engine_refuses_a_schedule_it_cannot_walk(device, plan):
    E = H.engine()
    pu, h = plan
    x = torch.zeros(SHP, device=device)
    sc, tab, coef = _schedule(6, "ddim")
    for k0, k1 in ((-1, 2), (3, 2), (0, 7)):
        with pytest.raises(E.EngineError, match="step range out of bounds"):
            _steps(h, sc, _args("noise", 1), x, k0, k1)
    sc.coef_prev = None
    with pytest.raises(E.EngineError, match="coef_x, coef_x0, coef_prev and coef_noise are required"):
        _steps(h, sc, _args("noise", 1), x, 0)
    sc, tab, coef = _schedule(6, "ddim")
    sc.T = 0
    with pytest.raises(E.EngineError, match="at least one step"):
        _steps(h, sc, _args("noise", 1), x, 0, 0)
    sc, tab, coef = _schedule(6, "ddim")
    sc.rn_a = None
    sa = _args("noise", 1)
    sa.resample_times = 2
    keep = (torch.zeros(SHP, device=device), torch.zeros(B1, 1, S1, S1, device=device))
    sa.d_inpaint_images, sa.d_inpaint_masks = E.ptr(keep[0]), E.ptr(keep[1])
    with pytest.raises(E.EngineError, match="re-noise tables are required"):
        _steps(h, sc, sa, x, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ noise
def _fill(device, seed, it, batch=B1):
    """Slot `it` of a [T, B, C, S, S] tensor from Philox stream (1, it): one stream over the batch (int) or a row per key."""
    E = H.engine()
    lib = E.load()
    z = torch.zeros(6, batch, N1, device=device)
    sid = E.stream_id(1, it)
    if isinstance(seed, list):
        E.check(lib.kd_philox_normal_rows(E.ptr(z[it]), batch, N1, E.seed_array(seed), sid, E.current_stream()))
    else:
        E.check(lib.kd_philox_normal(E.ptr(z[it]), batch * N1, seed, sid, E.current_stream()))
    return z


@pytest.mark.parametrize("seed", [0x9E3779B97F4A7C15, [7, 0x1_0000_0001]], ids=["int", "per_image"])
def test_ddim_draws_the_ancestral_steps_philox_stream(device, plan, seed):
    """DDIM(0.5) with in-kernel noise is torch.equal to the same step on a tensor filled by kd_philox_normal (int seed) or
    kd_philox_normal_rows (per-image seeds) with stream (1, it); graph replay and eager launches give the same bits."""
    E = H.engine()
    pu, h = plan
    T, k = 6, 2
    sc, tab, coef = _schedule(T, "ddim", 0.5)
    assert float(coef["coef_noise"][k]) > 0.1
    x_in = torch.randn(*SHP, generator=H.gen(77)) * 1.5

    def run(inject, use_graph=1):
        sa = _args("noise", 1, use_graph=use_graph, seed=seed if isinstance(seed, int) else 99)
        keep = []
        if isinstance(seed, list):
            keep.append(E.seed_array(seed))
            sa.seeds = keep[-1]
        if inject:
            keep.append(_fill(device, seed, k))
            sa.d_noise_step = E.ptr(keep[-1])
        x = x_in.to(device)
        _steps(h, sc, sa, x, k)
        torch.cuda.synchronize()
        return x

    got = run(False)
    assert torch.equal(got, run(True)) and torch.equal(got, run(False, use_graph=0))
    assert not torch.equal(got, x_in.to(device)) and bool(torch.isfinite(got).all())


@pytest.mark.parametrize("name", ["ddim", "dpmpp_2m"])
def test_deterministic_solvers_do_not_depend_on_the_seed(device, plan, name):
    pu, h = plan
    sc, tab, coef = _schedule(6, name)
    x_in = torch.randn(*SHP, generator=H.gen(78)) * 1.5
    outs = []
    for seed in (1, 2 ** 63 + 5):
        x = x_in.to(device)
        _steps(h, sc, _args("noise", 1, seed=seed), x, 0, 6)
        torch.cuda.synchronize()
        outs.append(x)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


# ------------------------------------------------------------------------------------------------ whole samplers
B, N = 3, 8
CASCADE_KW = dict(image_sizes=(16, 32), timesteps=(N, N), pred_objectives=("noise", "v"), condition_on_text=False)


def _unets(channels=3):
    return [H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=3, channels=channels),
            H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=6, channels=channels, lowres_cond=True)]


def _cascade(device, cls=SR.Imagen, **over):
    kw = dict(CASCADE_KW, **over)
    oim = cls(_unets(kw.get("channels", 3)), **kw)
    return oim, H.product_imagen(oim, "Imagen", device, **kw)


@pytest.fixture(scope="module")
def cascade(device):
    return _cascade(device)


def _rand(*shape, seed):
    return torch.rand(*shape, generator=H.gen(seed))


def _inpaint(S, seed=5):
    inp = _rand(B, 3, S, S, seed=seed)
    mask = torch.zeros(B, S, S, dtype=torch.bool)
    mask[0, S // 8:S // 2 + 4, S // 5:S - 2] = mask[1, S // 3:, :S // 4 + 1] = mask[2, :S // 4, 3:S // 2 + 1] = True
    return dict(inpaint_images=inp, inpaint_masks=mask, inpaint_resample_times=2)


def _to(device, kw):
    mv = lambda v: v.to(device) if torch.is_tensor(v) else type(v)(mv(e) for e in v) if isinstance(v, (tuple, list)) and any(
        torch.is_tensor(e) for e in v) else v
    return {k: mv(v) for k, v in kw.items()}


def _err(oim, pim, device, label, sampler, eta=0.0, **kw):
    nf = RS.generator_noise_fn(41)
    if sampler != "ddpm" and eta == 0:
        nf = SR.never_step_noise(nf)   # DDIM(0) and 2M never ask for a "step" tag
    kw = dict(kw, sampler=sampler, sampler_eta=eta)
    ref = oim.sample(noise_fn=nf, batch_size=B, **kw)
    got = pim.sample(noise_fn=nf, batch_size=B, device=device, **_to(device, kw)).cpu()
    assert bool(torch.isfinite(got).all()) and float(got.std()) > 0.01
    err = float((got - ref).abs().max())
    print(f"solvers {label}: max|diff| {err:.2e}")
    return err


def test_ddim_eta_1_is_todays_sampler(device, cascade):
    """The whole cascade on the same injected noise: sampler="ddim", sampler_eta=1 against the default call."""
    oim, pim = cascade
    nf = RS.generator_noise_fn(43)
    plain = pim.sample(noise_fn=nf, batch_size=B, device=device)
    got = pim.sample(noise_fn=nf, batch_size=B, device=device, sampler="ddim", sampler_eta=1.0)
    err = float((got - plain).abs().max())
    print(f"solvers DDIM(1) against the ancestral sampler, cascade N=8: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
    assert float((pim.sample(noise_fn=nf, batch_size=B, device=device, sampler="ddim") - plain).abs().max()) > 10 * SAMPLE_ABS


@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_cascade_matches_the_restatement(device, cascade, sampler, eta):
    oim, pim = cascade
    assert _err(oim, pim, device, f"{sampler} eta {eta} cascade N=8", sampler, eta) < SAMPLE_ABS


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_inpainting_with_resampling_matches_the_restatement(device, cascade, sampler):
    oim, pim = cascade
    assert _err(oim, pim, device, f"{sampler} cascade inpaint R=2", sampler, **_inpaint(32)) < SAMPLE_ABS


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_init_images_and_skip_steps_match_the_restatement(device, cascade, sampler):
    oim, pim = cascade
    kw = dict(init_images=_rand(B, 3, 24, 20, seed=1), skip_steps=(3, 5))
    assert _err(oim, pim, device, f"{sampler} cascade init_images skip (3, 5)", sampler, **kw) < SAMPLE_ABS


class SelfCondImagen(SC.Imagen, SR.Imagen):
    """The x_start carry of tests/self_cond_ref.py (reset per stage) over the solver loop of tests/solver_ref.py."""


def test_self_conditioned_unet_matches_the_restatement(device):
    ou = H.ref_unet(SC.Unet, H.UNET_KW["small1"], seed=21, self_cond=True)
    kw = dict(image_sizes=(16,), timesteps=(N,), pred_objectives=("noise",), condition_on_text=False)
    oim = SelfCondImagen([ou], **kw)
    pim = H.product_imagen(oim, "Imagen", device, **kw)
    assert pim.unets[0].self_cond
    assert _err(oim, pim, device, "dpmpp_2m self-cond N=8", "dpmpp_2m") < SAMPLE_ABS


def test_text_guided_sampling_matches_the_restatement(device):
    ou = H.ref_unet(R.Unet, dict(H.UNET_KW["small1"], cond_dim=64, text_embed_dim=3), seed=17, text=True)
    kw = dict(image_sizes=(16,), timesteps=(N,), text_embed_dim=3)
    oim = SR.Imagen([ou], **kw)
    pim = H.product_imagen(oim, "Imagen", device, **kw)
    text = torch.randn(B, 2, 3, generator=H.gen(4))
    assert _err(oim, pim, device, "dpmpp_2m text cond_scale 3", "dpmpp_2m", text_embeds=text, cond_scale=3.0) < SAMPLE_ABS


def test_one_channel_cascade_matches_the_restatement(device):
    oim, pim = _cascade(device, channels=1)
    assert _err(oim, pim, device, "dpmpp_2m cascade channels=1", "dpmpp_2m") < SAMPLE_ABS


@pytest.mark.parametrize("sampler,steps", [("dpmpp_2m", (8, 6)), ("ddpm", 8)])
def test_sample_steps_walks_the_short_schedule_of_a_1000_step_model(device, sampler, steps):
    oim, pim = _cascade(device, timesteps=1000)
    assert pim.noise_schedulers[0].num_timesteps == 1000
    assert _err(oim, pim, device, f"{sampler} timesteps=1000 sample_steps={steps}", sampler, sample_steps=steps) < SAMPLE_ABS


# ------------------------------------------------------------------------------------------------ bit for bit
KW3 = dict(batch_size=B, seed=[5, 6, 7])


@pytest.mark.parametrize("sampler,eta", [("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_graph_table_and_trace_do_not_change_a_bit(device, cascade, sampler, eta):
    pim = cascade[1]
    kw = dict(KW3, device=device, sampler=sampler, sampler_eta=eta)
    a = pim.sample(use_graph=True, **kw)
    assert torch.equal(a, pim.sample(use_graph=False, **kw))
    trace = []
    assert torch.equal(a, pim.sample(trace=trace, **kw))   # one kd_solver_sample_steps per step
    assert len(trace) == 2 * N
    off = _cascade(device)[1]
    off.cond_table = -1
    assert torch.equal(a, off.sample(**kw))


def test_alternating_samplers_on_one_plan_equal_fresh_plans(device, cascade):
    """ancestral -> 2M -> DDIM(0.5) -> 2M -> ancestral on one plan, each against the same call on a fresh plan; and
    sampler="ddpm" is the call without the argument."""
    pim = cascade[1]
    calls = [dict(), dict(sampler="dpmpp_2m"), dict(sampler="ddim", sampler_eta=0.5), dict(sampler="dpmpp_2m"), dict(),
             dict(sampler="ddpm")]
    got = [pim.sample(device=device, **KW3, **c) for c in calls]
    assert torch.equal(got[1], got[3]) and torch.equal(got[0], got[4]) and torch.equal(got[0], got[5])
    for c, g in list(zip(calls, got))[:3]:
        assert torch.equal(g, _cascade(device)[1].sample(device=device, **KW3, **c)), c
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


def _poison(pim, word):
    E = H.engine()
    n = 0
    for u in pim.unets:
        for h in u._engines.values():
            filled = C.c_int64(-1)
            E.check(E.load().kd_unet_poison_scratch(h, word, C.byref(filled), E.current_stream()))
            assert filled.value > 0
            n += 1
    return n


@pytest.mark.parametrize("case", ["ddim", "dpmpp_2m", "dpmpp_2m_inpaint", "dpmpp_2m_skip"])
def test_sampling_under_poisoned_scratch(device, cascade, case):
    """Every word of every plan's scratch - the history included - set to NaN, 1e30 and 0 before the call."""
    pim = cascade[1]
    kw = dict(KW3, device=device, sampler=case.split("_inpaint")[0].split("_skip")[0])
    if case.endswith("inpaint"):
        kw.update(_to(device, _inpaint(32)))
    if case.endswith("skip"):
        kw.update(init_images=_rand(B, 3, 16, 16, seed=2).to(device), skip_steps=3)
    base = pim.sample(**kw)
    assert bool(torch.isfinite(base).all())
    for word in (0xFFFFFFFF, 0x7149F2CA, 0):
        assert _poison(pim, word) >= 2
        assert torch.equal(pim.sample(**kw), base), hex(word)


# ------------------------------------------------------------------------------------------------ per-image seeds
def test_per_image_seeds_do_not_depend_on_the_batch(device, cascade):
    from imagen_pytorch import ImagenTrainer

    pim = cascade[1]
    seeds = [11, 22, 33]
    kw = dict(device=device, sampler="ddim", sampler_eta=0.5)
    full = pim.sample(batch_size=B, seed=seeds, **kw)
    singles = torch.cat([pim.sample(batch_size=1, seed=s, **kw) for s in seeds])
    chunked = ImagenTrainer(pim, use_ema=False).sample(batch_size=B, max_batch_size=2, seed=seeds, sampler="ddim", sampler_eta=0.5)
    d1, d2 = float((full - singles).abs().max()), float((full - chunked).abs().max())
    print(f"solvers DDIM(0.5), seed list: batch 3 vs three batch-1 calls max|diff| {d1:.2e}, vs trainer chunks 2 + 1 {d2:.2e}")
    assert d1 < TWO_PLANS and d2 < TWO_PLANS
    assert float((full[1] - pim.sample(batch_size=B, seed=11, **kw)[1]).abs().max()) > 10 * TWO_PLANS


# ------------------------------------------------------------------------------------------------ patch grid
def test_grid_driver_hands_the_sampler_to_every_call(device):
    """outpaint_canvas 2 x 2 over the three-stage dim-32 trio of tests/test_seeds_gpu.py through imagen_sample_fn(sampler=
    "dpmpp_2m", sample_steps={1: 4, 2: 3}, per_patch_seeds=True): every patch equals the sample() call made by hand with its
    task's seed and tensors (stage 3 keeps the constructor's one step), and the canvas does not follow max_batch."""
    from ultra_res import distributed as D

    ous = [H.fast_oracle(H.ref_unet(R.Unet, H.UNET_KW[name], seed=500 + s, cond_images_channels=0, lowres_cond=s > 1))
           for s, name in ((1, "ultra1"), (2, "ultra2"), (3, "ultra3"))]
    kw = dict(image_sizes=(64, 256, 1024), pred_objectives=("noise", "noise", "noise"), condition_on_text=False,
              timesteps=(2, 2, 1))
    pim = H.product_imagen(RS.Imagen(ous, **kw), "Imagen", device, random_crop_sizes=(None, None, 256), **kw)
    steps = {1: 4, 2: 3}
    canvases, calls = [], []
    for max_batch in (1, 4):
        fn = D.imagen_sample_fn(lambda stage: pim, 2, device, seed=3, max_batch=max_batch, per_patch_seeds=True,
                                sampler="dpmpp_2m", sample_steps=steps)

        def rec(stage, tasks, lows, conds, ips, ims, _fn=fn, _keep=max_batch == 1, **k):
            outs = _fn(stage, tasks, lows, conds, ips, ims, **k)
            if _keep:
                calls.extend(zip([stage] * len(tasks), tasks, lows, conds, ips, ims, [o.clone() for o in outs]))
            return outs

        rec.takes_base_seed = fn.takes_base_seed
        canvases.append(D.outpaint_canvas(rec, 2, overlap=0.25, device=device)[0])
    a, b = canvases
    assert tuple(a.shape) == (1, 3, 1792, 1792) and bool(torch.isfinite(a).all())
    d = float((a - b).abs().max())
    print(f"solvers outpaint 2x2 dpmpp_2m, per-patch seeds: max_batch 1 vs 4 max|diff| {d:.2e}")
    assert d < TWO_PLANS
    assert len(calls) == 12
    up = lambda t: None if t is None else t[None].to(device)
    for stage, task, low, cond, ip_, im, out in calls:
        hand = dict(batch_size=1, seed=[3 + 7919 * stage + 104729 * hash(task) % (2 ** 31)], device=device, use_tqdm=False,
                    start_at_unet_number=stage, stop_at_unet_number=stage, start_image_or_video=up(low), cond_images=up(cond),
                    sampler="dpmpp_2m", sample_steps=(4, 3, None))
        if ip_ is not None:
            hand.update(inpaint_images=up(ip_), inpaint_masks=up(im), inpaint_resample_times=2)
        assert torch.equal(pim.sample(**hand)[0], out), (stage, task)
    # ... and the arguments do something: the same grid without them is another canvas
    plain = D.imagen_sample_fn(lambda stage: pim, 2, device, seed=3, max_batch=1, per_patch_seeds=True)
    assert float((D.outpaint_canvas(plain, 2, overlap=0.25, device=device)[0] - a).abs().max()) > 10 * TWO_PLANS
