"""Few-step solvers without a GPU: the coefficient tables of solver_tables (DDIM(eta), DPM-Solver++(2M)) against the
ancestral step, against each other, against the exact solution of a constant and of a Gaussian denoiser, and the argument
rules of sample(sampler=..., sampler_eta=..., sample_steps=...)."""
import itertools
import math

import pytest
import torch

SCHEDULES = ("cosine", "linear")


def _tables(kind, N):
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes

    return GaussianDiffusionContinuousTimes(noise_schedule=kind, timesteps=N).step_tables()


def _solver(tables, name, **kw):
    from imagen_pytorch.imagen_pytorch import solver_tables

    out = solver_tables(tables, name, **kw)
    assert set(out) == {"coef_x", "coef_x0", "coef_prev", "coef_noise"}
    N = tables["alpha"].numel()
    assert all(v.dtype == torch.float32 and v.shape == (N,) and bool(torch.isfinite(v).all()) for v in out.values())
    return out


# ------------------------------------------------------------------------------------------------ eta = 1: the ancestral step
@pytest.mark.parametrize("kind,N", list(itertools.product(SCHEDULES, (1, 2, 8, 250, 1000))))
def test_ddim_eta_1_is_the_ancestral_step(kind, N):
    """coef_x, coef_x0, coef_noise of DDIM(1) against alpha_next (1 - c) / alpha, alpha_next c and noise_scale formed in
    fp32 from the same tables: below 1e-6.  (The posterior variance comes from the table's c; recomputing c from the
    log-SNRs in float64 moves the coefficients by 3e-5 at N = 1000.)"""
    t = _tables(kind, N)
    got = _solver(t, "ddim", eta=1.0)
    want_x = t["alpha_next"] * (1 - t["c"]) / t["alpha"]
    want_x0 = t["alpha_next"] * t["c"]
    errs = [float((got[n] - w).abs().max()) for n, w in (("coef_x", want_x), ("coef_x0", want_x0), ("coef_noise", t["noise_scale"]))]
    print(f"{kind} N={N}: max |diff| coef_x {errs[0]:.2e}, coef_x0 {errs[1]:.2e}, coef_noise {errs[2]:.2e}")
    assert max(errs) < 1e-6
    assert float(got["coef_noise"][-1]) == 0.0 and bool((got["coef_prev"] == 0).all())


# ------------------------------------------------------------------------------------------------ first-order 2M = DDIM(0)
@pytest.mark.parametrize("kind,N,skip", [(k, n, s) for k in SCHEDULES for n in (8, 32, 250) for s in (0, 3)])
def test_first_order_steps_of_2m_are_ddim_0(kind, N, skip):
    t = _tables(kind, N)
    ddim = _solver(t, "ddim", eta=0.0)
    m2 = _solver(t, "dpmpp_2m", skip=skip)
    for k in (skip, N - 1):
        for n in ("coef_x", "coef_x0"):
            err = abs(float(m2[n][k]) - float(ddim[n][k]))
            print(f"{kind} N={N} skip={skip} k={k} {n}: {err:.2e}")
            assert err <= 2.4e-7   # two fp32 ulps at 1
        assert float(m2["coef_prev"][k]) == 0.0 and float(m2["coef_noise"][k]) == 0.0
    assert bool((m2["coef_noise"] == 0).all()) and bool((ddim["coef_noise"] == 0).all())
    # the steps in between are second order: they read the history
    assert bool((m2["coef_prev"][skip + 1:N - 1] != 0).all())


# ------------------------------------------------------------------------------------------------ exactness
def _run(coefs, tables, denoiser, x, skip=0):
    """The recursion x <- A x + B x0_k + P x0_{k-1} in float64 over fp32 tables; denoiser(k, x) -> x0."""
    A, B, P = (coefs[n].double() for n in ("coef_x", "coef_x0", "coef_prev"))
    prev = 0.0
    for k in range(skip, A.numel()):
        x0 = denoiser(k, x)
        x = A[k] * x + B[k] * x0 + P[k] * prev
        prev = x0
    return float(x)


@pytest.mark.parametrize("kind,N,name", list(itertools.product(SCHEDULES, (8, 32), ("ddim", "dpmpp_2m"))))
def test_a_constant_denoiser_is_solved_exactly(kind, N, name):
    """x0 = mu at every step: the solvers are exact, x_end = a'_{N-1} mu + s'_{N-1} (x_T - a_0 mu) / s_0, up to the fp32
    rounding of the coefficients accumulated over N steps (bound 1e-5)."""
    t = {n: v.double() for n, v in _tables(kind, N).items()}
    mu, x_T = 0.37, -1.1
    got = _run(_solver(_tables(kind, N), name), t, lambda k, x: mu, x_T)
    want = float(t["alpha_next"][-1] * mu + t["sigma_next"][-1] * (x_T - t["alpha"][0] * mu) / t["sigma"][0])
    print(f"{kind} N={N} {name}: |x_end - exact| = {abs(got - want):.2e}")
    assert abs(got - want) < 1e-5


# ------------------------------------------------------------------------------------------------ order
GAUSS = ((0.3, 0.5, 0.7), (-0.6, 0.25, -1.3), (0.0, 1.0, 2.0))
ORDER_N = (16, 24, 32, 48, 64)


def _gauss_error(kind, N, name, mu, sd, xi):
    """|x_end - exact| for data N(mu, sd^2): denoiser x0 = (a sd^2 x + s^2 mu) / (a^2 sd^2 + s^2), probability-flow
    solution x_t = a_t mu + sqrt(a_t^2 sd^2 + s_t^2) xi."""
    t32 = _tables(kind, N)
    t = {n: v.double() for n, v in t32.items()}
    a, s = t["alpha"], t["sigma"]
    flow = lambda al, sg: float(al * mu + math.sqrt(float(al) ** 2 * sd ** 2 + float(sg) ** 2) * xi)
    den = lambda k, x: (a[k] * sd ** 2 * x + s[k] ** 2 * mu) / (a[k] ** 2 * sd ** 2 + s[k] ** 2)
    got = _run(_solver(t32, name), t, den, flow(a[0], s[0]))
    return abs(got - flow(t["alpha_next"][-1], t["sigma_next"][-1]))


@pytest.mark.parametrize("kind,case", list(itertools.product(SCHEDULES, GAUSS)))
def test_2m_is_second_order_on_a_gaussian(kind, case):
    err = {(name, N): _gauss_error(kind, N, name, *case) for name in ("ddim", "dpmpp_2m") for N in ORDER_N}
    for N in ORDER_N:
        print(f"{kind} {case} N={N}: ddim {err['ddim', N]:.3e}  2m {err['dpmpp_2m', N]:.3e}  "
              f"ratio {err['dpmpp_2m', N] / err['ddim', N]:.3f}")
    for N in ORDER_N:
        assert err["dpmpp_2m", N] < err["ddim", N]
    assert err["dpmpp_2m", 64] < 0.5 * err["ddim", 64]
    assert err["ddim", 64] < 0.6 * err["ddim", 32]


# ------------------------------------------------------------------------------------------------ the argument rules
def _norm(*a, n=2):
    from imagen_pytorch.imagen_pytorch import normalize_sampler

    return normalize_sampler(*a, n)


def test_sampler_arguments_are_cast_per_unet():
    assert _norm(None, 0.0, None) == [("ddpm", 0.0, None)] * 2
    assert _norm("ddpm", 0, 16) == [("ddpm", 0.0, 16)] * 2
    assert _norm(("ddim", "dpmpp_2m"), (0.5, 0.0), (8, None)) == [("ddim", 0.5, 8), ("dpmpp_2m", 0.0, None)]
    assert _norm(["ddim", None], [1, None], [None, 3]) == [("ddim", 1.0, None), ("ddpm", 0.0, 3)]


@pytest.mark.parametrize("args,match", [
    (("euler", 0.0, None), "sampler of unet 1"),
    ((("ddim", "heun"), 0.0, None), "sampler of unet 2"),
    (("ddim", 1.5, None), "sampler_eta"),
    (("ddim", -0.1, None), "sampler_eta"),
    (("ddim", "x", None), "sampler_eta"),
    (("dpmpp_2m", 0.5, None), "needs sampler='ddim'"),
    ((None, 0.5, None), "needs sampler='ddim'"),
    (("ddim", 0.0, 0), "sample_steps"),
    (("ddim", 0.0, -4), "sample_steps"),
    (("ddim", 0.0, 2.5), "sample_steps"),
    (("ddim", 0.0, True), "sample_steps"),
    ((("ddim",), 0.0, None), "sampler holds 1 entries for 2 unets"),
    (("ddim", (0.0, 0.0, 0.0), None), "sampler_eta holds 3 entries"),
    (("ddim", 0.0, (8,)), "sample_steps holds 1 entries"),
])
def test_every_refusal_is_a_value_error(args, match):
    with pytest.raises(ValueError, match=match):
        _norm(*args)


def test_solver_tables_refuses_what_it_cannot_tabulate():
    from imagen_pytorch.imagen_pytorch import solver_tables

    t = _tables("cosine", 8)
    for a, k in ((("ddpm",), {}), (("ddim",), dict(eta=1.5)), (("dpmpp_2m",), dict(eta=0.5)), (("dpmpp_2m",), dict(skip=8))):
        with pytest.raises(ValueError):
            solver_tables(t, *a, **k)


def _imagen(cls, **kw):
    import imagen_pytorch as ip

    unets = [ip.Unet(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False)]
    return cls(unets, image_sizes=(16,), condition_on_text=False, **kw)


def test_sample_refuses_bad_sampler_arguments_before_it_needs_a_gpu():
    import imagen_pytorch as ip

    im = _imagen(ip.Imagen, timesteps=8)
    for kw in (dict(sampler="euler"), dict(sampler="ddim", sampler_eta=2.0), dict(sampler="dpmpp_2m", sampler_eta=0.5),
               dict(sample_steps=0), dict(sampler=("ddim", "ddim")), dict(sampler="ddim", sample_steps=4, skip_steps=4),
               dict(sample_steps=4, skip_steps=5)):
        with pytest.raises(ValueError):
            im.sample(batch_size=1, **kw)
    # skip_steps counts in sample_steps: 6 is inside the constructor's 8 steps but outside the 4 asked for, and inside 16
    with pytest.raises(ValueError, match="skip_steps=6"):
        im.sample(batch_size=1, sampler="dpmpp_2m", sample_steps=4, skip_steps=6)
    from imagen_pytorch.imagen_pytorch import normalize_init_images, normalize_sampler

    steps = [st or 8 for _, _, st in normalize_sampler("ddim", 0.0, 16, 1)]
    assert normalize_init_images(None, 12, steps=steps, batch_size=1, channels=3) == [(None, 12)]


def test_elucidated_imagen_refuses_the_ddpm_solvers():
    import imagen_pytorch as ip

    im = _imagen(ip.ElucidatedImagen, num_sample_steps=4)
    for kw in (dict(sampler="ddim"), dict(sampler="ddpm"), dict(sample_steps=8), dict(sampler="dpmpp_2m", sample_steps=8)):
        with pytest.raises(ValueError, match="ElucidatedImagen"):
            im.sample(batch_size=1, **kw)


def test_a_schedule_with_other_timesteps_is_of_the_same_kind():
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes

    for kind in SCHEDULES:
        g = GaussianDiffusionContinuousTimes(noise_schedule=kind, timesteps=1000)
        assert g.with_timesteps(1000) is g
        h = g.with_timesteps(8)
        assert h.num_timesteps == 8 and h.log_snr is g.log_snr and g.num_timesteps == 1000
        want = GaussianDiffusionContinuousTimes(noise_schedule=kind, timesteps=8).step_tables()
        assert all(torch.equal(v, want[n]) for n, v in h.step_tables().items())
