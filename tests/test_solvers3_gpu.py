"""DPM-Solver++(3M) and the SDE forms of 2M and 3M on the MI355X, through kd_solver3_sample_steps / kd_solver3_sample_loop.

1. the update x <- A x + B x0c + P h1 + Q h2 + S z one step at a time, in the manner of tests/test_solvers_gpu.py: the
   engine's own x0 estimate and thresholds are read back with kd_sample_last and the update is recomputed from them in fp64
   over the fp32 coefficient tables (rel-L2 1e-6, the project's step bound); both histories are what the two preceding
   steps kept in the plan's ring.
2. whole samplers on the 16 -> 32 cascade (N = 8, batch 3) against the restatement tests/solver3_ref.py on identical weights
   and injected noise (max-abs 2e-3, the project's sampler bound).
3. invariants, bit for bit."""
import ctypes as C

import pytest
import torch

import helpers as H
import self_cond_ref as SC
import solver3_ref as S3
from oracle import imagen_ref as R
from oracle import sampler_ref as RS
from solver_ref import never_step_noise

pytestmark = pytest.mark.gpu

REL = 1e-6           # tests/test_ddpm_step_gpu.py, tests/test_solvers_gpu.py
SAMPLE_ABS = 2e-3    # the project's sampler bound against the oracle on identical noise
B1, S1 = 2, 16
SHP = (B1, 3, S1, S1)
OBJ = {"noise": 0, "v": 1, "x_start": 2}
NAMES3 = ("dpmpp_3m", "dpmpp_2m_sde", "dpmpp_3m_sde")
COEFS = ("coef_x", "coef_x0", "coef_prev", "coef_prev2", "coef_noise")


def _eta(name):
    return 1.0 if name.endswith("_sde") else 0.0


# ------------------------------------------------------------------------------------------------ single steps
@pytest.fixture(scope="module")
def plan(device):
    pu = H.product_like(H.oracle_unet("small1", seed=4), device)
    return pu, pu.engine(B1, S1, device, with_text=False)


def _schedule(T, name, eta=0.0, skip=0, struct="kd_solver3_schedule_t"):
    """(schedule struct, step tables, coefficient tables); the struct points into the tables: keep all three."""
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes, solver_tables

    E = H.engine()
    tab = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=T).step_tables()
    coef = solver_tables(tab, name, eta=eta, skip=skip)
    sc = getattr(E, struct)()
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


def _steps(h, sc, sa, x, k0, k1=None, entry="kd_solver3_sample_steps"):
    E = H.engine()
    E.check(getattr(E.load(), entry)(h, C.byref(sc), C.byref(sa), E.ptr(x), k0, k0 + 1 if k1 is None else k1,
                                     E.current_stream()))


def _last(h, device, shp=SHP):
    return [H.sample_last(h, which, shape, device) for which, shape in ((0, shp), (1, shp), (2, (shp[0],)))]


def _x0c(x0, s):
    s = s[:, None, None, None]
    return torch.maximum(torch.minimum(x0, s), -s) / s


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("name", NAMES3)
def test_solver3_step_matches_fp64_expression(device, plan, name, k):
    """T = 6 at k = 2, 3 (third order for the 3M names) and T - 1 (first order, no noise), dynamic and static threshold,
    eta = 0 and eta = 1 with z the slot k of an injected tensor.  Steps k - 2 and k - 1 run first, each on an image of its
    own, and leave their estimates in the ring; both are recomputed from those steps' read-backs."""
    pu, h = plan
    T, eta = 6, _eta(name)
    gen = torch.Generator().manual_seed(100 * k + T)
    x_in, x_1, x_2 = (torch.randn(*SHP, generator=gen) * 1.5 for _ in range(3))
    noise = torch.randn(T, *SHP, generator=gen).to(device)
    sc, tab, coef = _schedule(T, name, eta)
    A, Bc, P, Q, Sn = (float(coef[n][k]) for n in COEFS)
    assert (Q != 0) == (name != "dpmpp_2m_sde" and 2 <= k < T - 2) and (P != 0) == (k < T - 1) and (Sn != 0) == (eta > 0 and k < T - 1)
    for dyn in (1, 0):
        sa = _args("noise", dyn)
        sa.d_noise_step = H.engine().ptr(noise)
        one = torch.ones(B1, dtype=torch.float64)

        def walk():
            kept = []
            for xs, kk in ((x_2, k - 2), (x_1, k - 1)):   # the estimates of steps k - 2 and k - 1
                _steps(h, sc, sa, xs.to(device), kk)
                _, x0p, thrp = _last(h, device)
                kept.append(_x0c(x0p, thrp.clamp(min=1.0) if dyn else one))
            x = x_in.to(device)
            _steps(h, sc, sa, x, k)
            return x, kept

        x, (h2, h1) = walk()
        pred, x0, thr = _last(h, device)
        got, xd = x.double().cpu(), x_in.double()
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(x0).all())
        xs = _x0c(x0, thr.clamp(min=1.0) if dyn else one)
        want = A * xd + Bc * xs + P * h1 + Q * h2 + Sn * noise[k].double().cpu()
        e_x = H.rel_l2(got, want)
        print(f"solver3 step {name} eta {eta} T{T} k{k} dyn{dyn}: x_next rel-L2 {e_x:.2e}  (A {A:.4f} B {Bc:.4f} P {P:.4f} Q {Q:.4f} S {Sn:.4f})")
        assert e_x < REL
        if abs(P) > 0.01:   # (a history term of this size is seen)
            assert H.rel_l2(got, want - P * h1) > 20 * REL
        if abs(Q) > 0.01:
            assert H.rel_l2(got, want - Q * h2) > 20 * REL and H.rel_l2(got, A * xd + Bc * xs + P * h2 + Q * h1 + Sn * noise[k].double().cpu()) > 20 * REL
        if Sn == 0:   # no noise term: another noise tensor, the same bits
            other = torch.flip(noise, dims=(0,)) * 3 + 1
            sa.d_noise_step = H.engine().ptr(other)
            x2, _ = walk()
            torch.cuda.synchronize()
            assert torch.equal(x2, x)


def test_histories_follow_the_schedule_step_not_the_resample_slot(device, plan):
    """3M with inpainting, R = 2, steps 1 .. 3 of T = 6 (step 1 the first step walked): the last slot of step 3 reads what the
    LAST slots of steps 2 and 1 kept.  The last iteration is recomputed from the read-back of the call's last forward, the
    histories from calls that stop after step 1 and after step 2."""
    E = H.engine()
    pu, h = plan
    T, R, k = 6, 2, 3
    sc, tab, coef = _schedule(T, "dpmpp_3m", skip=1)
    assert float(coef["coef_prev"][1]) == 0.0 and float(coef["coef_prev2"][2]) == 0.0 and abs(float(coef["coef_prev2"][3])) > 0.01
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
    y = x_in.to(device)
    kept = []
    for kk in (1, 2):   # the same walk, stopped after step 1 and after step 2
        _steps(h, sc, sa, y, kk, kk + 1)
        _, x0p, thrp = _last(h, device)
        kept.append(_x0c(x0p, thrp.clamp(min=1.0)))
    h2, h1 = kept
    x = x_in.to(device)
    _steps(h, sc, sa, x, 1, 4)
    pred, x0, thr = _last(h, device)
    # the first slot of step 3 alone is not reachable through the ABI; what the second forward saw is alpha x0 + sigma pred
    seen = float(tab["alpha"][k]) * x0 + float(tab["sigma"][k]) * pred
    want = f("coef_x") * seen + f("coef_x0") * _x0c(x0, thr.clamp(min=1.0)) + f("coef_prev") * h1 + f("coef_prev2") * h2
    e = H.rel_l2(x, want)
    print(f"3M inpaint R2, last iteration of step 3: rel-L2 {e:.2e}")
    assert e < 2e-6   # `seen` is rebuilt from x0 (three more fp32 roundings than the plain step test), tests/test_solvers_gpu.py
    # (had the first slot of step 3 overwritten a ring slot, the second would have read step 3's own estimate there)
    assert H.rel_l2(x, want - f("coef_prev2") * h2) > 1e-3 and H.rel_l2(x, want - f("coef_prev") * h1) > 1e-3


def test_no_second_history_is_the_parent_call_bit_for_bit(device, plan):
    """DDIM(0.5) and 2M through kd_solver3_sample_steps with coef_prev2 NULL and all zero, against kd_solver_sample_steps."""
    pu, h = plan
    T = 6
    x_in = torch.randn(*SHP, generator=H.gen(31)) * 1.5
    for name, eta in (("ddim", 0.5), ("dpmpp_2m", 0.0)):
        outs = []
        for struct, entry, zeros in (("kd_solver_schedule_t", "kd_solver_sample_steps", False),
                                     ("kd_solver3_schedule_t", "kd_solver3_sample_steps", False),
                                     ("kd_solver3_schedule_t", "kd_solver3_sample_steps", True)):
            sc, tab, coef = _schedule(T, name, eta, struct=struct)
            z = torch.zeros(T)
            if zeros:
                sc.coef_prev2 = z.numpy().ctypes.data_as(C.POINTER(C.c_float))
            x = x_in.to(device)
            _steps(h, sc, _args("noise", 1), x, 0, T, entry=entry)
            torch.cuda.synchronize()
            outs.append(x)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and bool(torch.isfinite(outs[0]).all())


def test_engine_refuses_a_third_order_first_step(device, plan):
    E = H.engine()
    pu, h = plan
    x = torch.zeros(SHP, device=device)
    sc, tab, coef = _schedule(6, "dpmpp_3m")
    bad = coef["coef_prev2"].clone()
    bad[1] = 0.25
    sc.coef_prev2 = bad.numpy().ctypes.data_as(C.POINTER(C.c_float))
    with pytest.raises(E.EngineError, match="step 0 must be first order"):
        _steps(h, sc, _args("noise", 1), x, 0, 2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ whole samplers
B, N = 3, 8
CASCADE_KW = dict(image_sizes=(16, 32), timesteps=(N, N), pred_objectives=("noise", "v"), condition_on_text=False)


def _unets(channels=3):
    return [H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=3, channels=channels),
            H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=6, channels=channels, lowres_cond=True)]


def _cascade(device, cls=S3.Imagen, **over):
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


def _err(oim, pim, device, label, sampler, **kw):
    nf = RS.generator_noise_fn(41)
    if not sampler.endswith("_sde"):
        nf = never_step_noise(nf)   # 3M never asks for a "step" tag
    kw = dict(kw, sampler=sampler)
    ref = oim.sample(noise_fn=nf, batch_size=B, **kw)
    got = pim.sample(noise_fn=nf, batch_size=B, device=device, **_to(device, kw)).cpu()
    assert bool(torch.isfinite(got).all()) and float(got.std()) > 0.01
    err = float((got - ref).abs().max())
    print(f"solvers3 {label}: max|diff| {err:.2e}")
    return err


@pytest.mark.parametrize("sampler", NAMES3)
def test_cascade_matches_the_restatement(device, cascade, sampler):
    oim, pim = cascade
    assert _err(oim, pim, device, f"{sampler} cascade N=8", sampler) < SAMPLE_ABS


def test_the_samplers_differ_from_one_another(device, cascade):
    """(the comparisons above are not between copies of one sampler)"""
    pim = cascade[1]
    nf = RS.generator_noise_fn(41)
    got = [pim.sample(noise_fn=nf, batch_size=B, device=device, sampler=s) for s in ("dpmpp_2m",) + NAMES3]
    for i in range(len(got)):
        for j in range(i + 1, len(got)):
            assert float((got[i] - got[j]).abs().max()) > 10 * SAMPLE_ABS


def test_inpainting_with_resampling_matches_the_restatement(device, cascade):
    oim, pim = cascade
    assert _err(oim, pim, device, "dpmpp_3m cascade inpaint R=2", "dpmpp_3m", **_inpaint(32)) < SAMPLE_ABS


def test_init_images_and_skip_steps_match_the_restatement(device, cascade):
    oim, pim = cascade
    kw = dict(init_images=_rand(B, 3, 24, 20, seed=1), skip_steps=(3, 5))
    assert _err(oim, pim, device, "dpmpp_3m cascade init_images skip (3, 5)", "dpmpp_3m", **kw) < SAMPLE_ABS


class SelfCondImagen(SC.Imagen, S3.Imagen):
    """The x_start carry of tests/self_cond_ref.py (reset per stage) over the solver loop of tests/solver3_ref.py."""


def test_self_conditioned_unet_matches_the_restatement(device):
    ou = H.ref_unet(SC.Unet, H.UNET_KW["small1"], seed=21, self_cond=True)
    kw = dict(image_sizes=(16,), timesteps=(N,), pred_objectives=("noise",), condition_on_text=False)
    oim = SelfCondImagen([ou], **kw)
    pim = H.product_imagen(oim, "Imagen", device, **kw)
    assert pim.unets[0].self_cond
    assert _err(oim, pim, device, "dpmpp_3m self-cond N=8", "dpmpp_3m") < SAMPLE_ABS


def test_one_channel_cascade_matches_the_restatement(device):
    oim, pim = _cascade(device, channels=1)
    assert _err(oim, pim, device, "dpmpp_3m cascade channels=1", "dpmpp_3m") < SAMPLE_ABS


# ------------------------------------------------------------------------------------------------ bit for bit
KW3 = dict(batch_size=B, seed=[5, 6, 7])


@pytest.mark.parametrize("sampler", ["dpmpp_3m", "dpmpp_3m_sde"])
def test_graph_table_and_trace_do_not_change_a_bit(device, cascade, sampler):
    pim = cascade[1]
    kw = dict(KW3, device=device, sampler=sampler)
    a = pim.sample(use_graph=True, **kw)
    assert torch.equal(a, pim.sample(use_graph=False, **kw))
    trace = []
    assert torch.equal(a, pim.sample(trace=trace, **kw))   # one kd_solver3_sample_steps per step: the ring lives across calls
    assert len(trace) == 2 * N
    off = _cascade(device)[1]
    off.cond_table = -1
    assert torch.equal(a, off.sample(**kw))


def test_alternating_samplers_on_one_plan_equal_fresh_plans(device, cascade):
    """2M -> 3M -> ancestral -> 3M on one plan, each against the same call on a fresh plan."""
    pim = cascade[1]
    calls = [dict(sampler="dpmpp_2m"), dict(sampler="dpmpp_3m"), dict(), dict(sampler="dpmpp_3m")]
    got = [pim.sample(device=device, **KW3, **c) for c in calls]
    assert torch.equal(got[1], got[3])
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


@pytest.mark.parametrize("case", ["dpmpp_3m", "dpmpp_3m_skip"])
def test_sampling_under_poisoned_scratch(device, cascade, case):
    """Every word of every plan's scratch - both slots of the history ring included - set to NaN, 1e30 and 0 before the call."""
    pim = cascade[1]
    kw = dict(KW3, device=device, sampler="dpmpp_3m")
    if case.endswith("skip"):
        kw.update(init_images=_rand(B, 3, 16, 16, seed=2).to(device), skip_steps=3)
    base = pim.sample(**kw)
    assert bool(torch.isfinite(base).all())
    for word in (0xFFFFFFFF, 0x7149F2CA, 0):
        assert _poison(pim, word) >= 2
        assert torch.equal(pim.sample(**kw), base), hex(word)
