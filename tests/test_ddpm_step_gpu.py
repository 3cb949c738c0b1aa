"""The DDPM step kernels of kernels_sampler.hip (x0, the fused reverse step, RePaint mix and re-noise, finalize) one
step at a time through kd_sample_steps, in the manner of the EDM kernel tests (test_elucidated_gpu.py): the engine's own
UNet output, x0 estimate and thresholds are read back with kd_sample_last and every kernel's result is recomputed from
them in fp64, so the UNet's error is not in the comparison.  Bound: rel-L2 1e-6 (fp32 torch evaluates these expressions
within 8e-8 of fp64 at every step tested here)."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

REL = 1e-6
B, S = 2, 16
SHP = (B, 3, S, S)
N = B * 3 * S * S
OBJ = {"noise": 0, "v": 1, "x_start": 2}


@pytest.fixture(scope="module")
def plan(device):
    pu = H.product_like(H.oracle_unet("small1", seed=4), device)
    return pu, pu.engine(B, S, device, with_text=False)


def _schedule(T):
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes

    E = H.engine()
    tables = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=T).step_tables()
    sc = E.kd_schedule_t()
    sc.T = T
    for name, v in tables.items():
        setattr(sc, name, v.numpy().ctypes.data_as(C.POINTER(C.c_float)))
    return sc, tables   # (sc points into the tables: keep both)


def _args(objective, dynamic_threshold, use_graph=1, seed=9):
    sa = H.engine().kd_sample_args_t()
    sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times = OBJ[objective], dynamic_threshold, 0.95, 1
    sa.seed, sa.use_graph = seed, use_graph
    return sa


def _steps(h, sc, sa, x, k):
    E = H.engine()
    E.check(E.load().kd_sample_steps(h, C.byref(sc), C.byref(sa), E.ptr(x), k, k + 1, E.current_stream()))


def _last(h, device):
    """(pred, x0, thresholds) of the last iteration, fp64 on the CPU."""
    return [H.sample_last(h, which, shape, device) for which, shape in ((0, SHP), (1, SHP), (2, (B,)))]


def _x0_of(objective, x, pred, alpha, sigma):
    if objective == "noise":
        return (x - sigma * pred) / max(alpha, 1e-8)
    if objective == "v":
        return alpha * x - sigma * pred
    return pred


def _mean_of(tab, k, x, x0, s):
    """alpha_next * (x (1 - c) / alpha + c clamp(x0, -s, s) / s), fp64 from the fp32 table entries."""
    f = lambda n: float(tab[n][k])
    s = s[:, None, None, None]
    x0c = torch.maximum(torch.minimum(x0, s), -s) / s
    return f("alpha_next") * (x * (1.0 - f("c")) / f("alpha") + f("c") * x0c)


def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


# ------------------------------------------------------------------------------------------------ step arithmetic
@pytest.mark.parametrize("T,k", [(6, 0), (6, 2), (6, 5), (1000, 0), (1000, 333), (1000, 999)])
@pytest.mark.parametrize("objective", ["noise", "v", "x_start"])
def test_ddpm_step_matches_fp64_expressions(device, plan, T, k, objective):
    """x0_kernel and ddpm_update_kernel at both ends and the middle of a short and a long cosine schedule, for the three
    objectives, with the dynamic threshold and with the static clamp to +-1: x0 against its formula, x_{t-1} against
    alpha_next (x (1 - c) / alpha + c clamp(x0, -s, s) / s) + noise_scale z with z the slot k of the noise tensor.  At
    k = 0 (alpha = 4.4e-8, c = 1, x0 about 1e8 under the noise objective) the result is finite; at k = T - 1
    (noise_scale = 0) it does not depend on the noise."""
    pu, h = plan
    sc, tab = _schedule(T)
    gen = torch.Generator().manual_seed(100 * k + T)
    x_in = _randn(gen, *SHP, scale=1.5)
    noise = _randn(gen, T, *SHP).to(device)
    f = lambda n: float(tab[n][k])
    for dyn in (1, 0):
        sa = _args(objective, dyn)
        sa.d_noise_step = H.engine().ptr(noise)
        x = x_in.to(device)
        _steps(h, sc, sa, x, k)
        pred, x0, thr = _last(h, device)
        got, xd = x.double().cpu(), x_in.double()
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(x0).all())
        e_x0 = H.rel_l2(x0, _x0_of(objective, xd, pred, f("alpha"), f("sigma")))
        if dyn:
            q = torch.quantile(x0.float().flatten(1).abs(), 0.95, dim=-1).double()
            assert torch.allclose(thr, q.clamp(min=1.0), rtol=1e-6, atol=0), (thr, q)
        s = thr.clamp(min=1.0) if dyn else torch.ones(B, dtype=torch.float64)
        want = _mean_of(tab, k, xd, x0, s) + f("noise_scale") * noise[k].double().cpu()
        e_x = H.rel_l2(got, want)
        print(f"ddpm step T{T} k{k} {objective} dyn{dyn}: x0 rel-L2 {e_x0:.2e}, x_next rel-L2 {e_x:.2e}, "
              f"max|x0| {float(x0.abs().max()):.3g}, s {thr.tolist() if dyn else 1}")
        assert e_x0 < REL and e_x < REL
        if k == T - 1:   # no noise is added to the last step: another noise tensor, the same bits
            assert f("noise_scale") == 0.0
            other = torch.flip(noise, dims=(0,)) * 3 + 1
            sa.d_noise_step = H.engine().ptr(other)
            x2 = x_in.to(device)
            _steps(h, sc, sa, x2, k)
            torch.cuda.synchronize()
            assert torch.equal(x2, x)
    if k == 0 and objective == "noise":
        assert f("c") == 1.0 and float(x0.abs().max()) > 1e6   # (the case the docstring names is the one that ran)


# ------------------------------------------------------------------------------------------------ inpainting, R = 2
def _inpaint_setup(device, gen, T, R):
    inp = (torch.rand(SHP, generator=gen) * 2 - 1)
    mask = torch.zeros(B, 1, S, S)
    mask[0, :, 2:9, 3:14] = 1    # edges at columns 3 and 14, 1 and 6: inside a float4
    mask[1, :, 5:12, 1:6] = 1
    zs = [_randn(gen, T * R, *SHP).to(device) for _ in range(3)]   # step, inpaint, renoise: T * R slots each
    return inp, mask, zs


def _mix(tab, k, x, inp, mask, z):
    """The known pixels are alpha inp + sigma z."""
    m = mask.bool().expand(SHP)
    return torch.where(m, float(tab["alpha"][k]) * inp.double() + float(tab["sigma"][k]) * z, x)


def _tail(t, n):
    """View of a [slots, ...] noise tensor from slot n on: a run with R = 1 that reads slot k of it reads slot n + k."""
    v = t[n:]
    assert v.is_contiguous()
    return v


@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("objective", ["noise", "v"])
def test_ddpm_inpaint_resample_slots_and_renoise(device, plan, k, objective):
    """One call over step k of T = 6 with inpainting and R = 2 runs iterations it = 2 k and 2 k + 1.  Each mixes the known
    pixels in (alpha inp + sigma z_inpaint[it]), runs the UNet and the reverse step with z_step[it]; the re-noise
    x rn_a + z_renoise[it] rn_b follows the first iteration only, and none at k = T - 1.  The first iteration is run alone
    (R = 1, its noise tensors offset so that its slot k is slot 2 k) and checked by itself; then the second is recomputed
    from it in fp64 and from the preds the R = 2 call left behind.  Slot it = k R + (R - 1 - r) for resample r = R - 1 .. 0."""
    E = H.engine()
    pu, h = plan
    T, R = 6, 2
    sc, tab = _schedule(T)
    gen = torch.Generator().manual_seed(31 + k)
    inp, mask, (z_step, z_inp, z_ren) = _inpaint_setup(device, gen, T, R)
    inp_d, mask_d = inp.to(device), mask.to(device)
    x_in = _randn(gen, *SHP, scale=1.5)
    f = lambda n: float(tab[n][k])
    cpu = lambda t: t.double().cpu()

    def args(R_, zs):
        sa = _args(objective, 1)
        sa.resample_times = R_
        sa.d_inpaint_images, sa.d_inpaint_masks = E.ptr(inp_d), E.ptr(mask_d)
        sa.d_noise_step, sa.d_noise_inpaint, sa.d_noise_renoise = (E.ptr(z) if z is not None else None for z in zs)
        return sa

    it0, it1 = k * R, k * R + 1
    # the first iteration alone
    y = x_in.to(device)
    _steps(h, sc, args(1, (_tail(z_step, it0 - k), _tail(z_inp, it0 - k), None)), y, k)
    pred, x0, thr = _last(h, device)
    xm = _mix(tab, k, x_in.double(), inp, mask, cpu(z_inp[it0]))
    assert H.rel_l2(x0, _x0_of(objective, xm, pred, f("alpha"), f("sigma"))) < REL
    y1 = _mean_of(tab, k, xm, x0, thr.clamp(min=1.0)) + f("noise_scale") * cpu(z_step[it0])
    assert H.rel_l2(y, y1) < REL
    # both iterations in one call
    x = x_in.to(device)
    _steps(h, sc, args(R, (z_step, z_inp, z_ren)), x, k)
    pred2, x02, thr2 = _last(h, device)
    x1 = cpu(y)
    if k != T - 1:
        x1 = x1 * f("rn_a") + cpu(z_ren[it0]) * f("rn_b")
    xm2 = _mix(tab, k, x1, inp, mask, cpu(z_inp[it1]))
    e_x0 = H.rel_l2(x02, _x0_of(objective, xm2, pred2, f("alpha"), f("sigma")))   # what the second forward was given
    want = _mean_of(tab, k, xm2, x02, thr2.clamp(min=1.0)) + f("noise_scale") * cpu(z_step[it1])
    e_x = H.rel_l2(x, want)
    print(f"ddpm inpaint R2 k{k} {objective}: second x0 rel-L2 {e_x0:.2e}, x_next rel-L2 {e_x:.2e}")
    assert e_x0 < REL and e_x < REL
    if k != T - 1:   # (the re-noise is large enough to be seen: without it the check above fails)
        assert H.rel_l2(cpu(y), x1) > 0.1


# ------------------------------------------------------------------------------------------------ in-kernel Philox
PHILOX_ATOL = 2e-5   # test_philox_normal_matches_host_reference_and_is_normal: libm against ocml


def _philox(device, seed, purpose, it):
    from oracle.philox_ref import philox_normal

    E = H.engine()
    sid = (purpose << 32) | it
    out = torch.empty(N, device=device)
    E.check(E.load().kd_philox_normal(E.ptr(out), N, seed, sid, E.current_stream()))
    torch.cuda.synchronize()
    return out.double().cpu().reshape(SHP), torch.from_numpy(philox_normal(N, seed, sid).astype(np.float64)).reshape(SHP)


def test_ddpm_step_draws_its_noise_from_philox_stream_1(device, plan):
    """d_noise_step = NULL: the step adds noise_scale times element i of Philox stream (1 << 32) | it under the seed.
    (x_next - mean) / noise_scale is compared with kd_philox_normal and with oracle/philox_ref.py.  Bound: the 2e-5 of
    test_philox_normal_matches_host_reference_and_is_normal (libm against ocml) plus 2^-23 max|x_next| / noise_scale for the
    fp32 rounding of mean + noise_scale z (x_next is rounded once, half an ulp, and the mean it is compared with is the
    kernel's fp32 mean to about the same).  k = 2 of T = 6: noise_scale = 0.58.  Graph replay and eager launches: same bits."""
    pu, h = plan
    T, k, seed = 6, 2, 0x9E3779B97F4A7C15
    sc, tab = _schedule(T)
    x_in = _randn(torch.Generator().manual_seed(77), *SHP, scale=1.5)
    ns = float(tab["noise_scale"][k])
    runs = []
    for use_graph in (1, 0):
        x = x_in.to(device)
        _steps(h, sc, _args("noise", 1, use_graph=use_graph, seed=seed), x, k)
        pred, x0, thr = _last(h, device)
        runs.append(x)
        got = x.double().cpu()
        z = (got - _mean_of(tab, k, x_in.double(), x0, thr.clamp(min=1.0))) / ns
        bound = PHILOX_ATOL + 2.0 ** -23 * float(got.abs().max()) / ns
        z_dev, z_host = _philox(device, seed, 1, k)
        print(f"philox step stream, graph {use_graph}: max|z - kd_philox_normal| {float((z - z_dev).abs().max()):.2e}, "
              f"max|z - philox_ref| {float((z - z_host).abs().max()):.2e}, bound {bound:.2e}")
        assert float((z - z_dev).abs().max()) < bound and float((z - z_host).abs().max()) < bound
    assert torch.equal(runs[0], runs[1])


def test_ddpm_inpaint_and_renoise_draw_from_philox_streams_2_and_3(device, plan):
    """Inpainting with R = 2 at k = 2 of T = 6 (iterations it = 4, 5), noise objective.
    Stream 2: with d_noise_inpaint = NULL the known pixels the second forward saw are alpha inp + sigma z, z = element i of
    stream (2 << 32) | 5.  What it saw is alpha x0 + sigma pred of the read-back (x0 = (x - sigma pred) / alpha), so
    z = (alpha x0 + sigma pred - alpha inp) / sigma.  fp32 roundings on the way: three in the mix, three in x0, each at most
    2^-24 of M = max|x| + sigma max|pred|: bound 2e-5 + 6 2^-24 M / sigma.
    Stream 3: with d_noise_renoise = NULL the first iteration's result y (run alone, R = 1) is re-noised to y rn_a + z rn_b,
    z from stream (3 << 32) | 4, and the unknown pixels reach the second forward unchanged: z = (alpha x0 + sigma pred -
    y rn_a) / rn_b there.  Two roundings in the re-noise, three in x0: bound 2e-5 + 5 2^-24 M / rn_b (rn_b = 0.37)."""
    E = H.engine()
    pu, h = plan
    T, R, k, seed = 6, 2, 2, 0xD1B54A32D192ED03
    it0, it1 = k * R, k * R + 1
    sc, tab = _schedule(T)
    gen = torch.Generator().manual_seed(78)
    inp, mask, (z_step, z_inp, z_ren) = _inpaint_setup(device, gen, T, R)
    inp_d, mask_d = inp.to(device), mask.to(device)
    x_in = _randn(gen, *SHP, scale=1.5)
    f = lambda n: float(tab[n][k])
    m = mask.bool().expand(SHP)

    def run(R_, zs, use_graph):
        sa = _args("noise", 1, use_graph=use_graph, seed=seed)
        sa.resample_times = R_
        sa.d_inpaint_images, sa.d_inpaint_masks = E.ptr(inp_d), E.ptr(mask_d)
        sa.d_noise_step, sa.d_noise_inpaint, sa.d_noise_renoise = (E.ptr(z) if z is not None else None for z in zs)
        x = x_in.to(device)
        _steps(h, sc, sa, x, k)
        pred, x0, _ = _last(h, device)
        seen = f("alpha") * x0 + f("sigma") * pred   # the x the last forward was given
        M = float(seen.abs().max()) + f("sigma") * float(pred.abs().max())
        return x, seen, M

    for which in ("inpaint", "renoise"):
        outs = []
        for use_graph in (1, 0):
            if which == "inpaint":
                x, seen, M = run(R, (z_step, None, z_ren), use_graph)
                z = ((seen - f("alpha") * inp.double()) / f("sigma"))[m]
                bound = PHILOX_ATOL + 6 * 2.0 ** -24 * M / f("sigma")
                z_dev, z_host = (t[m] for t in _philox(device, seed, 2, it1))
            else:
                y, _, _ = run(1, (_tail(z_step, it0 - k), _tail(z_inp, it0 - k), None), use_graph)
                x, seen, M = run(R, (z_step, z_inp, None), use_graph)
                z = ((seen - y.double().cpu() * f("rn_a")) / f("rn_b"))[~m]
                bound = PHILOX_ATOL + 5 * 2.0 ** -24 * M / f("rn_b")
                z_dev, z_host = (t[~m] for t in _philox(device, seed, 3, it0))
            outs.append(x)
            print(f"philox {which} stream, graph {use_graph}: max|z - kd_philox_normal| {float((z - z_dev).abs().max()):.2e}, "
                  f"max|z - philox_ref| {float((z - z_host).abs().max()):.2e}, bound {bound:.2e}")
            assert float((z - z_dev).abs().max()) < bound and float((z - z_host).abs().max()) < bound
        assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ finalize
@pytest.mark.parametrize("inpaint", [False, True])
def test_sample_finalize_is_clamp_paste_unnormalise(device, plan, inpaint):
    """kd_sample_finalize: (clamp(x, -1, 1), the known pixels pasted over it, + 1) * 0.5 - the same bits as fp32 torch,
    on values beyond +-1, exactly +-1 and inside."""
    E = H.engine()
    pu, h = plan
    gen = torch.Generator().manual_seed(5)
    x = _randn(gen, *SHP)   # about a third beyond +-1
    x.flatten()[:8] = torch.tensor([1.0, -1.0, 1.0000001, -1.0000001, 0.99999994, -0.99999994, 0.0, -0.0])
    x[1, 2, -1, -4:] = torch.tensor([7.5, -7.5, 1.0, -1.0])
    inp = torch.rand(SHP, generator=gen) * 2 - 1
    mask = torch.zeros(B, 1, S, S)
    mask[0, :, 2:9, 3:14] = 1
    mask[1, :, 0:3, 0:2] = 1   # covers x[1, :, 0, 0:2], not the special values of x[0] / the last row
    sa = _args("noise", 1)
    keep = (inp.to(device), mask.to(device))
    if inpaint:
        sa.d_inpaint_images, sa.d_inpaint_masks = E.ptr(keep[0]), E.ptr(keep[1])
    xd = x.to(device)
    x_cpu = xd.cpu()
    E.check(E.load().kd_sample_finalize(h, C.byref(sa), E.ptr(xd), E.current_stream()))
    torch.cuda.synchronize()
    want = x_cpu.clamp(-1.0, 1.0)
    if inpaint:
        want = torch.where(mask.bool().expand(SHP), inp, want)
    want = (want + 1.0) * 0.5
    assert torch.equal(xd.cpu(), want)
    assert float(want.min()) == 0.0 and float(want.max()) == 1.0
