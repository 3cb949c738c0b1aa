"""Fused-tile canvas sampling without a GPU: the geometry and its refusals (normalize_tiling), the tile weights, the
ancestral step in the canvas step's linear form (canvas_tables), the restatement tests/tiled_ref.py against the same solver on
the whole canvas (exact for a pointwise denoiser) and against tests/solver_ref.py on a 1 x 1 lattice, and the argument rules
of Imagen.sample_tiled."""
import itertools
import math

import pytest
import torch

import helpers as H
import solver_ref as SR
import tiled_ref as TR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

SCHEDULES = ("cosine", "linear")


def _tiling(*a, **k):
    from imagen_pytorch.imagen_pytorch import normalize_tiling

    return normalize_tiling(*a, **k)


# ------------------------------------------------------------------------------------------------ geometry
def test_sizes_origins_and_numbering():
    (g,) = _tiling((16,), (2, 2))
    assert (g["S"], g["st"], g["Hc"], g["Wc"], g["ov"]) == (16, 12, 28, 28, 4)
    assert g["origins"] == [(0, 0), (0, 12), (12, 0), (12, 12)] and g["tile_of"] == [[0, 1], [2, 3]]
    (g,) = _tiling((16,), (3, 2), overlap=0.5, present=[[True, True], [False, True], [True, True]])
    assert (g["st"], g["Hc"], g["Wc"]) == (8, 32, 24)
    assert g["tile_of"] == [[0, 1], [-1, 2], [3, 4]] and g["origins"] == [(0, 0), (0, 8), (8, 8), (16, 0), (16, 8)]
    assert _tiling((16,), (1, 1))[0]["Hc"] == 16
    (g,) = _tiling((16,), (2, 1), present=torch.tensor([[True], [True]]))
    assert (g["Hc"], g["Wc"]) == (28, 16)


def test_the_cascades_lattices_are_images_of_one_another():
    gs = _tiling((64, 256, 1024), (8, 8), overlap=0.25)
    assert [(g["st"], g["Hc"]) for g in gs] == [(48, 400), (192, 1600), (768, 6400)]
    assert all(g["Hc"] * 4 == h["Hc"] for g, h in zip(gs, gs[1:]))
    assert [g["Hc"] for g in _tiling((16, 32), (2, 2))] == [28, 56]
    with pytest.raises(ValueError):
        _tiling((64, 256), (2, 2), overlap=0.3)   # strides 44 and 179


@pytest.mark.parametrize("args,kw,match", [
    (((18,), (2, 2)), {}, "tile size S=18 of unet 1 must be a multiple of 4"),
    (((16, 30), (2, 2)), dict(overlap=0.5), "tile size S=30 of unet 2"),
    (((16,), (2, 2)), dict(overlap=0.3), "tile stride st=11 of unet 1 .* must be a multiple of 4"),
    (((16,), (2, 2)), dict(overlap=0.99), "tile stride st=0 of unet 1 .* must be at least 1"),
    (((16,), (2, 2)), dict(overlap=-0.25), "tile stride st=20 of unet 1 must not exceed the tile size S=16"),
    (((16,), (2, 2)), dict(overlap=0.75), "more than 3 tiles per axis"),
    (((16,), (2, 2)), dict(present=[[False, False], [False, False]]), "present marks no slot"),
    (((16,), (2, 2)), dict(present=[[True, True]]), r"present must be \[ny=2\]\[nx=2\]"),
    (((16, 40), (2, 2)), dict(overlap=0.2), "lattices of unets 1 and 2 are not images of one another: st=32 \\* S=16 != st=12 \\* S=40"),
    (((16,), (0, 2)), {}, "grid must be"),
    (((16,), 2), {}, "grid must be"),
    (((16,), (2, 2)), dict(tile_weights="cosine"), "tile_weights must be one of"),
    (((16,), (2, 2)), dict(overlap="x"), "overlap must be a number"),
])
def test_every_refusal_names_what_it_refuses(args, kw, match):
    with pytest.raises(ValueError, match=match):
        _tiling(*args, **kw)


ACCEPTED = [((16,), (2, 2), 0.25), ((16,), (3, 3), 0.5), ((20,), (3, 3), 0.6), ((20,), (4, 5), 0.6), ((16, 32), (3, 2), 0.25),
            ((64, 256, 1024), (2, 3), 0.25), ((40,), (4, 4), 0.6)]


@pytest.mark.parametrize("sizes,grid,overlap", ACCEPTED)
def test_no_pixel_is_covered_by_more_than_nine_tiles(sizes, grid, overlap):
    for g in _tiling(sizes, grid, overlap=overlap):
        count = torch.zeros(g["Hc"], g["Wc"], dtype=torch.int64)
        for y0, x0 in g["origins"]:
            assert y0 % 4 == 0 and x0 % 4 == 0 and y0 + g["S"] <= g["Hc"] and x0 + g["S"] <= g["Wc"]
            count[y0:y0 + g["S"], x0:x0 + g["S"]] += 1
        assert int(count.min()) >= 1 and int(count.max()) <= 9
        assert math.ceil(g["S"] / g["st"]) <= 3


@pytest.mark.parametrize("S,st", [(16, 12), (16, 8), (20, 8), (16, 16), (1024, 768)])
def test_ramp_weights(S, st):
    from imagen_pytorch.imagen_pytorch import tile_weight

    w = tile_weight(S, st, "ramp")
    assert w.dtype == torch.float32 and w.shape == (S, S) and float(w.min()) > 0 and float(w.max()) <= 1.0
    assert torch.equal(w, w.flip(0)) and torch.equal(w, w.flip(1)) and torch.equal(w, w.t())
    ov = max(S - st, 1)
    if S + 1 >= 2 * ov:   # an interior exists (the overlap strips of the two sides do not meet): the weight is 1 there
        assert bool((w[ov - 1:S - ov + 1, ov - 1:S - ov + 1] == 1).all()) and float(w.max()) == 1.0
    else:
        assert float(w.max()) < 1.0
    assert float(w[0, 0]) == float(torch.tensor(1.0 / ov, dtype=torch.float32) ** 2)
    assert torch.equal(w, TR.weight(S, st, "ramp"))
    assert torch.equal(tile_weight(S, st, "uniform"), torch.ones(S, S))
    with pytest.raises(ValueError, match="tile_weights"):
        tile_weight(S, st, "flat")


# ------------------------------------------------------------------------------------------------ the ancestral coefficients
@pytest.mark.parametrize("kind,N", list(itertools.product(SCHEDULES, (1, 2, 8, 250, 1000))))
def test_ancestral_coefficients_give_the_posterior_mean(kind, N):
    """canvas_tables("ddpm"): A x + B x0 over the fp32 coefficients against the oracle's q_posterior mean at every step;
    bound 2.4e-7 max|.| (two fp32 ulps at 1, the bound of the DDIM(1) comparison in tests/test_solvers.py).  P = 0 and S is
    the table's noise_scale.  x and x0 are float64 on both sides, so the oracle's scalars (fp32: alpha, alpha_next, c and
    1 - c) meet the coefficients without the rounding of its five vector ops - on fp32 vectors that rounding alone puts
    the oracle's own mean 2.45e-7 max|.| from the float64 value (linear, N = 1000; 2.0e-7 cosine), whatever the
    coefficients are."""
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes, canvas_tables

    t = GaussianDiffusionContinuousTimes(noise_schedule=kind, timesteps=N).step_tables()
    co = canvas_tables(t, "ddpm")
    assert set(co) == {"coef_x", "coef_x0", "coef_prev", "coef_noise"} and all(v.dtype == torch.float32 for v in co.values())
    assert bool((co["coef_prev"] == 0).all()) and torch.equal(co["coef_noise"], t["noise_scale"])
    osch = RS.GaussianDiffusionContinuousTimes(noise_schedule=kind, timesteps=N)
    g = H.gen(N)
    x, x0 = torch.randn(64, generator=g).double() * 1.5, torch.rand(64, generator=g).double() * 2 - 1
    worst = 0.0
    for k, (tm, tn) in enumerate(osch.get_sampling_timesteps(1)):
        mean, _, _ = osch.q_posterior(x_start=x0[None], x_t=x[None], t=tm, t_next=tn)
        assert mean.dtype == torch.float64
        got = co["coef_x"][k].double() * x + co["coef_x0"][k].double() * x0
        scale = max(float(x.abs().max()), float(x0.abs().max()), float(mean.abs().max()))
        worst = max(worst, float((got - mean[0]).abs().max()) / scale)
    print(f"ancestral coefficients {kind} N={N}: max |A x + B x0 - mean| / max|.| = {worst:.2e}")
    assert worst <= 2.4e-7
    with pytest.raises(ValueError):
        canvas_tables(t, "ddpm", eta=0.5)
    for name, eta in (("ddim", 0.5), ("dpmpp_2m", 0.0)):
        from imagen_pytorch.imagen_pytorch import solver_tables

        assert all(torch.equal(v, solver_tables(t, name, eta=eta)[n]) for n, v in canvas_tables(t, name, eta).items())


# ------------------------------------------------------------------------------------------------ exactness
MU, SD = 0.3, 0.5


def _gauss_denoiser(sched):
    """The closed-form denoiser of data N(mu, sd^2) (tests/test_solvers.py), pointwise, with the static threshold."""

    def den(times, x):
        a, s = RS.log_snr_to_alpha_sigma(RS._pad(x, sched.log_snr(times)))
        return ((a * SD ** 2 * x + s ** 2 * MU) / (a ** 2 * SD ** 2 + s ** 2)).clamp(-1.0, 1.0)

    return den


@pytest.mark.parametrize("overlap", [0.25, 0.5])
@pytest.mark.parametrize("name,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)])
@pytest.mark.parametrize("weights", ["uniform", "ramp"])
def test_a_pointwise_denoiser_makes_the_tiled_canvas_the_whole_canvas(weights, name, eta, overlap):
    """A denoiser that acts on every pixel by itself gives equal estimates wherever tiles overlap, and averaging equal
    values is exact up to rounding: tiled_ref on a 3 x 2 lattice equals the same solver run on the whole canvas as one
    image under the same canvas noise.  Bound 1e-5, the bound of the exact case of tests/test_solvers.py."""
    sched = RS.GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=8)
    lat = TR.lattice(16, (3, 2), overlap)
    nf = RS.generator_noise_fn(7)
    den = _gauss_denoiser(sched)
    x_T = nf(("init", 1), (1, 3, lat["Hc"], lat["Wc"]))
    got, covered = TR.run_canvas(lambda k, t, tn, tiles, prev: den(t, tiles), x_T, lat, sched, name, eta, nf, 1, weights)
    assert bool(covered.all())
    solver, x = TR.CanvasSolver(sched, name, eta), x_T
    for k, (t, tn) in enumerate(solver.steps):
        noise = nf(("step", 1, k, 0), tuple(x.shape)) if solver.wants_noise(k) else None
        x = solver.step(k, x, den(t, x), noise)
    err = float((got - x).abs().max())
    print(f"tiled exactness {weights} {name} eta {eta} overlap {overlap}: max|tiled - whole canvas| = {err:.2e}")
    assert err < 1e-5 and float(x.std()) > 0.1


@pytest.mark.parametrize("name", ["ddim", "dpmpp_2m"])
def test_one_tile_is_the_solver_restatement(name):
    """A 1 x 1 lattice holds one tile, the canvas itself: tiled_ref equals tests/solver_ref.py's sampler at batch 1 on the
    same injected noise, bit for bit."""
    kw = dict(image_sizes=(16,), timesteps=(8,), pred_objectives=("noise",), condition_on_text=False)
    oim = SR.Imagen([H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=3)], **kw)
    nf = SR.never_step_noise(RS.generator_noise_fn(11))
    want = oim.sample(noise_fn=nf, batch_size=1, sampler=name)
    got = TR.sample_tiled(oim, grid=(1, 1), noise_fn=nf, sampler=name)
    assert got.shape == (1, 3, 16, 16) and torch.equal(got, want)


def test_a_hole_stays_zero_and_its_neighbours_do_not_see_it():
    present = [[True, True], [True, False], [True, True]]
    lat = TR.lattice(16, (3, 2), 0.25, present)
    assert len(lat["origins"]) == 5
    tiles = torch.randn(5, 3, 16, 16, generator=H.gen(1))
    x0bar, covered = TR.fuse(tiles, lat, TR.weight(16, 12, "uniform"))
    assert not bool(covered[16:24, 16:].any()) and bool(covered[:12].all()) and bool((x0bar[0, :, ~covered] == 0).all())
    assert torch.equal(x0bar[0, :, :12, :12], tiles[0, :, :12, :12])   # covered by tile 0 alone
    assert torch.equal(x0bar[0, :, 12:16, 16:], tiles[1, :, 12:, 4:])  # the strip tile 1 would share with the missing tile


# ------------------------------------------------------------------------------------------------ the argument rules
def _imagen(cls, **kw):
    import imagen_pytorch as ip

    unets = [ip.Unet(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False)]
    return cls(unets, image_sizes=(16,), condition_on_text=False, **kw)


def test_sample_tiled_refuses_by_name_before_it_needs_a_gpu():
    import imagen_pytorch as ip

    im = _imagen(ip.Imagen, timesteps=8)
    img, mask = torch.zeros(4, 3, 16, 16), torch.zeros(4, 16, 16)
    for kw, exc, match in [
            (dict(inpaint_images=img), NotImplementedError, "inpaint_images"),
            (dict(inpaint_masks=mask), NotImplementedError, "inpaint_masks"),
            (dict(inpaint_resample_times=5), NotImplementedError, "inpaint_resample_times"),
            (dict(init_images=img), NotImplementedError, "init_images"),
            (dict(skip_steps=2), NotImplementedError, "skip_steps"),
            (dict(seed=[1, 2, 3, 4]), ValueError, "seed"),
            (dict(seed=torch.tensor([1, 2, 3, 4])), ValueError, "seed"),
            (dict(tile_batch=0), ValueError, "tile_batch"),
            (dict(sampler="euler"), ValueError, "sampler of unet 1"),
            (dict(sampler="dpmpp_2m", sampler_eta=0.5), ValueError, "needs sampler='ddim'"),
            (dict(overlap=0.3), ValueError, "tile stride st=11"),
            (dict(tile_weights="flat"), ValueError, "tile_weights"),
            (dict(cond_images=torch.zeros(3, 3, 16, 16)), ValueError, "cond_images must be \\[tiles 4"),
            (dict(start_at_unet_number=2), ValueError, "start_at_unet_number"),
    ]:
        with pytest.raises(exc, match=match):
            im.sample_tiled((2, 2), **kw)
    with pytest.raises(NotImplementedError, match="ElucidatedImagen"):
        _imagen(ip.ElucidatedImagen, num_sample_steps=4).sample_tiled((2, 2))
    if not torch.cuda.is_available():   # and what passes the checks reaches the engine: there is no CPU path
        with pytest.raises(ip._engine.EngineUnavailable):
            im.sample_tiled((2, 2), seed=3)


def test_fused_canvas_refuses_by_name_before_it_needs_a_gpu():
    from ultra_res import tiled as UT

    load = lambda stage: (_ for _ in ()).throw(AssertionError("no model may be loaded for a refused call"))
    with pytest.raises(ValueError, match="num_patches_width or grid"):
        UT.fused_canvas(load)
    with pytest.raises(ValueError, match="num_patches_width or grid"):
        UT.fused_canvas(load, num_patches_width=2, grid=(2, 2))
    with pytest.raises(ValueError, match="stages"):
        UT.fused_canvas(load, num_patches_width=2, stages=(1, 3))
    with pytest.raises(ValueError, match="start_canvas"):
        UT.fused_canvas(load, num_patches_width=2, stages=(2, 3))
    import imagen_pytorch as ip

    one = lambda stage: _imagen(ip.Imagen, timesteps=8)   # the geometry is refused before the model moves to a device
    with pytest.raises(ValueError, match="tile stride st=11"):
        UT.fused_canvas(one, num_patches_width=2, overlap=0.3, stages=(1,))
    with pytest.raises(ValueError, match="the Imagen holds 1"):
        UT.fused_canvas(one, num_patches_width=2, stages=(1, 2))
