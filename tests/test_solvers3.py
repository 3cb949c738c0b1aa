"""DPM-Solver++(3M) and the SDE forms of 2M and 3M without a GPU: the argument rules, the coefficient tables of
solver_tables against the first-order form, DDIM(0) and each other, the exact solution of a constant denoiser, the order on
Gaussian data, and the end distribution of the stochastic recursions (mean and variance propagated exactly)."""
import itertools
import math

import pytest
import torch

SCHEDULES = ("cosine", "linear")
NAMES3 = ("dpmpp_3m", "dpmpp_2m_sde", "dpmpp_3m_sde")
KEYS5 = {"coef_x", "coef_x0", "coef_prev", "coef_prev2", "coef_noise"}


def _tables(kind, N):
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes

    return GaussianDiffusionContinuousTimes(noise_schedule=kind, timesteps=N).step_tables()


def _eta(name, eta=None):
    return (1.0 if name.endswith("_sde") else 0.0) if eta is None else eta


def _solver(tables, name, eta=None, **kw):
    from imagen_pytorch.imagen_pytorch import solver_tables

    out = solver_tables(tables, name, eta=_eta(name, eta), **kw)
    assert set(out) == (KEYS5 if name in NAMES3 else KEYS5 - {"coef_prev2"})
    N = tables["alpha"].numel()
    assert all(v.dtype == torch.float32 and v.shape == (N,) and bool(torch.isfinite(v).all()) for v in out.values())
    return out


def _first_order(tables, eta):
    """A, b, S of the first-order step in float64 over the fp32 tables, and h."""
    t = {n: v.double() for n, v in tables.items()}
    lam = t["log_snr"] / 2
    lam_next = torch.cat([lam[1:], torch.log(t["alpha_next"][-1:] / t["sigma_next"][-1:])])
    h = lam_next - lam
    A = t["sigma_next"] / t["sigma"] * torch.exp(-eta * h)
    b = -t["alpha_next"] * torch.expm1(-h * (1 + eta))
    S = t["sigma_next"] * torch.sqrt(-torch.expm1(-2 * eta * h))
    S[-1] = 0.0
    return A, b, S, h


# ------------------------------------------------------------------------------------------------ the argument rules
def _norm(*a, n=1):
    from imagen_pytorch.imagen_pytorch import normalize_sampler

    return normalize_sampler(*a, n)


def test_sample_accepts_the_new_sampler_names():
    """Fails without the feature: "dpmpp_3m" is a ValueError there."""
    from imagen_pytorch.imagen_pytorch import SAMPLERS

    assert set(NAMES3) <= set(SAMPLERS) and {"ddpm", "ddim", "dpmpp_2m"} <= set(SAMPLERS)
    assert _norm("dpmpp_3m", None, None) == [("dpmpp_3m", 0.0, None)]
    assert _norm("dpmpp_3m", 0.0, 8) == [("dpmpp_3m", 0.0, 8)]
    assert _norm(("dpmpp_3m", "dpmpp_3m_sde"), None, (8, None), n=2) == [("dpmpp_3m", 0.0, 8), ("dpmpp_3m_sde", 1.0, None)]


def test_eta_none_is_0_and_1_for_the_sde_names():
    for name in (None, "ddpm", "ddim", "dpmpp_2m", "dpmpp_3m"):
        assert _norm(name, None, None)[0][1] == 0.0
    for name in ("dpmpp_2m_sde", "dpmpp_3m_sde"):
        assert _norm(name, None, None) == [(name, 1.0, None)]
        assert _norm(name, 0.5, None) == [(name, 0.5, None)]
    assert _norm(("ddim", "dpmpp_2m_sde"), (None, None), None, n=2) == [("ddim", 0.0, None), ("dpmpp_2m_sde", 1.0, None)]
    assert _norm(("ddim", "dpmpp_2m_sde"), (0.3, 0.4), None, n=2) == [("ddim", 0.3, None), ("dpmpp_2m_sde", 0.4, None)]


@pytest.mark.parametrize("args,match", [
    (("dpmpp_2m_sde", 0.0, None), "use sampler='dpmpp_2m'"),
    (("dpmpp_3m_sde", 0, None), "use sampler='dpmpp_3m'"),
    (("dpmpp_3m", 0.5, None), "needs sampler='ddim'"),
    (("dpmpp_3m", 1, None), "needs sampler='ddim'"),
    (("dpmpp_3m_sde", 1.5, None), "sampler_eta"),
    (("dpmpp_2m_sde", -0.1, None), "sampler_eta"),
    (("dpmpp_2m_sde", "x", None), "sampler_eta"),
    (("dpmpp_3m", None, 0), "sample_steps"),
    # what the existing tests pin keeps its type and message
    (("euler", 0.0, None), "sampler of unet 1"),
    (("euler", None, None), "sampler of unet 1"),
    (("dpmpp_2m", 0.5, None), "needs sampler='ddim'"),
    ((None, 0.5, None), "needs sampler='ddim'"),
])
def test_every_refusal_is_a_value_error(args, match):
    with pytest.raises(ValueError, match=match):
        _norm(*args)


def test_solver_tables_refuses_what_it_cannot_tabulate():
    from imagen_pytorch.imagen_pytorch import solver_tables

    t = _tables("cosine", 8)
    for a, k in ((("dpmpp_3m",), dict(eta=0.5)), (("dpmpp_3m_sde",), dict(eta=0.0)), (("dpmpp_2m_sde",), {}),
                 (("dpmpp_3m_sde",), dict(eta=1.5)), (("dpmpp_3m",), dict(skip=8)), (("dpmpp_4m",), {})):
        with pytest.raises(ValueError):
            solver_tables(t, *a, **k)


def _imagen(cls, **kw):
    import imagen_pytorch as ip

    unets = [ip.Unet(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False)]
    return cls(unets, image_sizes=(16,), condition_on_text=False, **kw)


def test_public_calls_take_eta_none_and_refuse_before_they_need_a_gpu():
    import inspect

    import imagen_pytorch as ip
    from ultra_res import distributed as D
    from ultra_res import tiled as TL

    for fn in (ip.Imagen.sample, ip.Imagen.sample_tiled, D.imagen_sample_fn, TL.fused_canvas, TL.fused_level):
        assert inspect.signature(fn).parameters["sampler_eta"].default is None, fn.__qualname__
    im = _imagen(ip.Imagen, timesteps=8)
    for kw in (dict(sampler="dpmpp_3m", sampler_eta=0.5), dict(sampler="dpmpp_2m_sde", sampler_eta=0.0),
               dict(sampler="dpmpp_3m_sde", sampler_eta=2.0), dict(sampler="dpmpp_3m", sample_steps=4, skip_steps=4)):
        with pytest.raises(ValueError):
            im.sample(batch_size=1, **kw)
        if "skip_steps" not in kw:
            with pytest.raises(ValueError):
                im.sample_tiled((1, 1), **kw)
    el = _imagen(ip.ElucidatedImagen, num_sample_steps=4)
    for kw in (dict(sampler="dpmpp_3m"), dict(sampler="dpmpp_3m_sde"), dict(sampler_eta=1.0)):
        with pytest.raises(ValueError, match="ElucidatedImagen"):
            el.sample(batch_size=1, **kw)


# ------------------------------------------------------------------------------------------------ tables
CASES = [(k, n, s) for k in SCHEDULES for n in (8, 32, 250) for s in (0, 3)]


def test_ddim_and_2m_keep_their_keys_and_their_bits():
    """The parent's arithmetic restated: the tables of the two names that existed are equal bit for bit."""
    for kind, N, skip in CASES:
        t = _tables(kind, N)
        d = {n: v.double() for n, v in t.items()}
        lam = d["log_snr"] / 2
        h = torch.cat([lam[1:], torch.log(d["alpha_next"][-1:] / d["sigma_next"][-1:])]) - lam
        b = -d["alpha_next"] * torch.expm1(-h)
        B, P = b.clone(), torch.zeros_like(b)
        for k in range(skip + 1, N - 1):
            w = h[k] / (2 * h[k - 1])
            B[k], P[k] = b[k] * (1 + w), -b[k] * w
        got = _solver(t, "dpmpp_2m", skip=skip)
        want = dict(coef_x=d["sigma_next"] / d["sigma"], coef_x0=B, coef_prev=P, coef_noise=torch.zeros_like(b))
        assert all(torch.equal(got[n], w.float()) for n, w in want.items())
        for eta in (0.0, 0.5):
            dd = eta * torch.sqrt(d["sigma_next"] ** 2 * d["c"])
            A = torch.sqrt((d["sigma_next"] ** 2 - dd ** 2).clamp(min=0.0)) / d["sigma"]
            S = dd.clone()
            S[-1] = 0.0
            got = _solver(t, "ddim", eta=eta)
            want = dict(coef_x=A, coef_x0=d["alpha_next"] - A * d["alpha"], coef_prev=torch.zeros_like(A), coef_noise=S)
            assert all(torch.equal(got[n], w.float()) for n, w in want.items())


@pytest.mark.parametrize("kind,N,skip", CASES)
def test_first_and_last_rows_are_first_order(kind, N, skip):
    t = _tables(kind, N)
    ddim = _solver(t, "ddim", eta=0.0)
    for name in NAMES3:
        for eta in sorted({_eta(name), 0.5 if name.endswith("_sde") else 0.0}):
            co = _solver(t, name, eta=eta, skip=skip)
            A, b, S, _ = _first_order(t, eta)
            for k in (skip, N - 1):
                assert float(co["coef_x"][k]) == float(A[k].float()) and float(co["coef_x0"][k]) == float(b[k].float())
                assert float(co["coef_prev"][k]) == 0.0 and float(co["coef_prev2"][k]) == 0.0
                assert float(co["coef_noise"][k]) == float(S[k].float())
        # at eta = 0 the first-order step is DDIM(0)
        co = _solver(t, "dpmpp_3m", skip=skip)
        for k in (skip, N - 1):
            for n in ("coef_x", "coef_x0"):
                err = abs(float(co[n][k]) - float(ddim[n][k]))
                print(f"{kind} N={N} skip={skip} k={k} {n}: 3M - DDIM(0) = {err:.2e}")
                assert err <= 2.4e-7   # two fp32 ulps at 1


@pytest.mark.parametrize("kind,N,skip", CASES)
def test_second_history_is_read_exactly_between_the_low_order_rows(kind, N, skip):
    t = _tables(kind, N)
    for name in ("dpmpp_3m", "dpmpp_3m_sde"):
        q = _solver(t, name, skip=skip)["coef_prev2"]
        zero = [skip, skip + 1, N - 2, N - 1]
        assert all(float(q[k]) == 0.0 for k in zero)
        between = [k for k in range(skip, N) if k not in zero]
        assert len(between) == N - skip - 4 and all(float(q[k]) != 0.0 for k in between)
        p = _solver(t, name, skip=skip)["coef_prev"]
        assert float(p[skip]) == 0.0 and float(p[N - 1]) == 0.0 and bool((p[skip + 1:N - 1] != 0).all())
    co = _solver(t, "dpmpp_2m_sde", skip=skip)
    assert bool((co["coef_prev2"] == 0).all()) and bool((co["coef_prev"][skip + 1:N - 1] != 0).all())


@pytest.mark.parametrize("kind,N,skip", CASES)
def test_coefficients_of_the_estimates_sum_to_the_first_order_one(kind, N, skip):
    t = _tables(kind, N)
    for name in NAMES3:
        eta = _eta(name)
        co = _solver(t, name, skip=skip)
        _, b, _, _ = _first_order(t, eta)
        total = co["coef_x0"].double() + co["coef_prev"].double() + co["coef_prev2"].double()
        err = float((total - b)[skip:].abs().max())
        print(f"{kind} N={N} skip={skip} {name}: max |B + P + Q - b| = {err:.2e}")
        assert err < 1e-6


@pytest.mark.parametrize("kind,N,skip", CASES)
def test_noise_is_added_on_every_row_but_the_last_and_never_at_eta_0(kind, N, skip):
    t = _tables(kind, N)
    assert bool((_solver(t, "dpmpp_3m", skip=skip)["coef_noise"] == 0).all())
    for name in ("dpmpp_2m_sde", "dpmpp_3m_sde"):
        for eta in (1.0, 0.3):
            s = _solver(t, name, eta=eta, skip=skip)["coef_noise"]
            assert float(s[-1]) == 0.0 and bool((s[:-1] > 0).all())


# ------------------------------------------------------------------------------------------------ exactness
def _run(coefs, denoiser, x, skip=0):
    """x <- A x + B x0_k + P x0_{k-1} + Q x0_{k-2} in float64 over the fp32 tables (z = 0); denoiser(k, x) -> x0."""
    A, B, P = (coefs[n].double() for n in ("coef_x", "coef_x0", "coef_prev"))
    Q = coefs["coef_prev2"].double() if "coef_prev2" in coefs else torch.zeros_like(A)
    h1 = h2 = 0.0
    for k in range(skip, A.numel()):
        x0 = denoiser(k, x)
        x = A[k] * x + B[k] * x0 + P[k] * h1 + Q[k] * h2
        h2, h1 = h1, x0
    return float(x)


@pytest.mark.parametrize("kind,N,name", list(itertools.product(SCHEDULES, (8, 32), NAMES3)))
def test_a_constant_denoiser_is_solved_exactly(kind, N, name):
    """x0 = mu at every step and z = 0: x_end - a' mu = prod(A) (x_T - a_0 mu), prod(A) = (s'_end / s_0) exp(-eta (lambda_end -
    lambda_0)), up to the fp32 rounding of the coefficients accumulated over N steps (bound 1e-5, tests/test_solvers.py's)."""
    t32 = _tables(kind, N)
    t = {n: v.double() for n, v in t32.items()}
    eta, mu, x_T = _eta(name), 0.37, -1.1
    got = _run(_solver(t32, name), lambda k, x: mu, x_T)
    lam_0, lam_end = float(t["log_snr"][0]) / 2, math.log(float(t["alpha_next"][-1] / t["sigma_next"][-1]))
    prod_A = float(t["sigma_next"][-1] / t["sigma"][0]) * math.exp(-eta * (lam_end - lam_0))
    want = float(t["alpha_next"][-1]) * mu + prod_A * (x_T - float(t["alpha"][0]) * mu)
    print(f"{kind} N={N} {name}: |x_end - exact| = {abs(got - want):.2e}")
    assert abs(got - want) < 1e-5


# ------------------------------------------------------------------------------------------------ order on Gaussian data
GAUSS = ((0.3, 0.5, 0.7), (-0.6, 0.25, -1.3), (0.0, 1.0, 2.0), (0.8, 0.1, -0.4))
ORDER_N = (6, 8, 12, 16, 24, 32, 48, 64)


def _gauss_error(kind, N, name, mu, sd, xi):
    """|x_end - exact| for data N(mu, sd^2): denoiser x0 = (a sd^2 x + s^2 mu) / (a^2 sd^2 + s^2), probability-flow
    solution x_t = a_t mu + sqrt(a_t^2 sd^2 + s_t^2) xi (tests/test_solvers.py)."""
    t32 = _tables(kind, N)
    t = {n: v.double() for n, v in t32.items()}
    a, s = t["alpha"], t["sigma"]
    flow = lambda al, sg: float(al * mu + math.sqrt(float(al) ** 2 * sd ** 2 + float(sg) ** 2) * xi)
    den = lambda k, x: (a[k] * sd ** 2 * x + s[k] ** 2 * mu) / (a[k] ** 2 * sd ** 2 + s[k] ** 2)
    got = _run(_solver(t32, name), den, flow(a[0], s[0]))
    return abs(got - flow(t["alpha_next"][-1], t["sigma_next"][-1]))


@pytest.mark.parametrize("kind", SCHEDULES)
def test_3m_beats_ddim_on_a_gaussian(kind):
    """Worst case over four (mu, sd, xi): printed for DDIM(0), 2M and 3M; asserted only 3M < DDIM(0) at every N.  (3M beats 2M
    up to N = 16 on the cosine schedule and loses to it at N >= 24, where the uniform time grid's last, first-order step
    dominates the error: printed, not promised.)"""
    for N in ORDER_N:
        err = {name: max(_gauss_error(kind, N, name, *case) for case in GAUSS) for name in ("ddim", "dpmpp_2m", "dpmpp_3m")}
        print(f"{kind} N={N}: ddim {err['ddim']:.3e}  2m {err['dpmpp_2m']:.3e}  3m {err['dpmpp_3m']:.3e}  "
              f"ddim / 3m {err['ddim'] / err['dpmpp_3m']:.2f}")
        assert err["dpmpp_3m"] < err["ddim"]


def _sde_end_moments(tables, coefs, mu, sd, order):
    """Mean and std of x_end under x <- A x + B x0 + P h1 + Q h2 + S z with the Gaussian denoiser x0 = g_k x + c_k, z ~ N(0, 1)
    independent per step, x_T ~ N(a_0 mu, a_0^2 sd^2 + s_0^2): the state (x, h1, h2) is Gaussian and the recursion linear, so
    its mean vector and covariance matrix are propagated exactly (float64).  `order` 1 drops the history terms:
    B + P + Q -> x0, the first-order SDE step."""
    t = {n: v.double() for n, v in tables.items()}
    a, s = t["alpha"], t["sigma"]
    A, B, P, Q, S = (coefs[n].double() for n in ("coef_x", "coef_x0", "coef_prev", "coef_prev2", "coef_noise"))
    if order == 1:
        B, P, Q = B + P + Q, torch.zeros_like(P), torch.zeros_like(Q)
    m = torch.tensor([float(a[0]) * mu, 0.0, 0.0], dtype=torch.float64)
    cov = torch.zeros(3, 3, dtype=torch.float64)
    cov[0, 0] = float(a[0]) ** 2 * sd ** 2 + float(s[0]) ** 2
    for k in range(A.numel()):
        den = float(a[k]) ** 2 * sd ** 2 + float(s[k]) ** 2
        g, c = float(a[k]) * sd ** 2 / den, float(s[k]) ** 2 * mu / den
        # (x, h1, h2) -> (A x + B (g x + c) + P h1 + Q h2 + S z,  g x + c,  h1)
        M = torch.tensor([[float(A[k] + B[k] * g), float(P[k]), float(Q[k])], [g, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
        off = torch.tensor([float(B[k]) * c, c, 0.0], dtype=torch.float64)
        m = M @ m + off
        cov = M @ cov @ M.T
        cov[0, 0] += float(S[k]) ** 2
    return float(m[0]), math.sqrt(float(cov[0, 0]))


@pytest.mark.parametrize("kind", SCHEDULES)
def test_sde_forms_reproduce_the_end_distribution_of_gaussian_data(kind):
    """(mu, sd) = (0.3, 0.5), eta = 1: the end distribution is N(a' mu, a'^2 sd^2 + s'^2) at the last t_next.  The mean is
    reproduced (a linear denoiser whose mean is on the exact path: |error| < 1e-6); the |std error| of order 2 and of order
    3 is below the first-order SDE's at N = 16, 32, 64."""
    mu, sd = 0.3, 0.5
    for N in (16, 32, 64):
        t32 = _tables(kind, N)
        an, sn = float(t32["alpha_next"][-1].double()), float(t32["sigma_next"][-1].double())
        want_m, want_s = an * mu, math.sqrt(an ** 2 * sd ** 2 + sn ** 2)
        std_err = {}
        for label, name, order in (("order 1", "dpmpp_2m_sde", 1), ("order 2", "dpmpp_2m_sde", 2), ("order 3", "dpmpp_3m_sde", 3)):
            m, s = _sde_end_moments(t32, _solver(t32, name), mu, sd, order)
            std_err[label] = abs(s - want_s)
            print(f"{kind} N={N} {label}: |mean error| {abs(m - want_m):.2e}  |std error| {std_err[label]:.3e}")
            assert abs(m - want_m) < 1e-6
        assert std_err["order 2"] < std_err["order 1"] and std_err["order 3"] < std_err["order 1"]
