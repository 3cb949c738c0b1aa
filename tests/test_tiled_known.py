"""Fused-tile canvases that keep known pixels or start from an image, without a GPU: the argument rules (normalize_known,
normalize_init_canvas), the restatement tests/tiled_known_ref.py against tests/tiled_ref.py (nothing known), against
tests/solver_ref.py / tests/init_images_ref.py on a 1 x 1 lattice and against the same solver on the whole canvas (exact for a
pointwise denoiser), canvas_tables(skip=), level_keep_mask and the windows fused_level hands down."""
import pytest
import torch

import helpers as H
import solver_ref as SR
import tiled_known_ref as KR
import tiled_ref as TR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

SOLVERS = [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)]


def cascade_mask():
    """The 56 x 56 mask of the 16 -> 32 cascade at 2 x 2 (canvases 28 and 56): columns [0, 20) and the square [30, 40)^2."""
    m = torch.zeros(56, 56, dtype=torch.bool)
    m[:, :20] = True
    m[30:40, 30:40] = True
    return m


def test_the_cascade_mask_meets_the_mask_condition():
    m = cascade_mask()
    KR.assert_mask_condition(m, [KR.lattice(16, (2, 2)), KR.lattice(32, (2, 2))])
    assert abs(float(m.float().mean()) - 0.39) < 0.005
    with pytest.raises(AssertionError):
        KR.assert_mask_condition(torch.zeros(56, 56, dtype=torch.bool), [KR.lattice(32, (2, 2))])


# ------------------------------------------------------------------------------------------------ the argument rules
def _imagen(**kw):
    import imagen_pytorch as ip

    unets = [ip.Unet(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False)]
    return ip.Imagen(unets, image_sizes=(16,), condition_on_text=False, timesteps=8, **kw)


def test_sample_tiled_refuses_the_canvas_arguments_by_name_before_it_needs_a_gpu():
    im = _imagen()
    img, mask = torch.rand(1, 3, 28, 28), torch.zeros(28, 28, dtype=torch.bool)
    wide = torch.rand(1, 3, 28, 56)
    for kw, match in [
            (dict(known_image=img), "known_mask is missing"),
            (dict(known_mask=mask), "known_image is missing"),
            (dict(known_image=img[0], known_mask=mask), r"known_image must be one image \[1, channels 3"),
            (dict(known_image=img[:, :2], known_mask=mask), r"known_image must be one image \[1, channels 3"),
            (dict(known_image=torch.rand(2, 3, 28, 28), known_mask=mask), "known_image must be one image"),
            (dict(known_image=img, known_mask=torch.zeros(2, 28, 28)), r"known_mask must be \[Hk, Wk\] or \[1, Hk, Wk\]"),
            (dict(known_image=img, known_mask=torch.zeros(28)), "known_mask must be"),
            (dict(known_image=img, known_mask=torch.zeros(28, 24, dtype=torch.bool)), "the sizes must agree"),
            (dict(known_image=img.long(), known_mask=mask), "known_image must be of a floating dtype or uint8"),
            (dict(known_image=img, known_mask=mask.long()), "known_mask must be bool, uint8 or floating"),
            (dict(known_image=img, known_mask=mask, known_resample_times=0), "known_resample_times must be an int >= 1"),
            (dict(known_image=img, known_mask=mask, known_resample_times=1.5), "known_resample_times must be an int >= 1"),
            (dict(known_resample_times=2), "known_resample_times=2 needs known_image and known_mask"),
            (dict(known_image=wide[..., ::2], known_mask=mask), "known_image must have unit x stride"),
            (dict(known_image=img, known_mask=torch.zeros(28, 56, dtype=torch.uint8)[:, ::2]), "known_mask must have unit x stride"),
            (dict(init_skip_steps=8), "init_skip_steps=8 of unet 1 is outside 0 .. 7"),
            (dict(init_skip_steps=-1), "init_skip_steps=-1 of unet 1 is outside"),
            (dict(init_skip_steps=2.0), "init_skip_steps of unet 1 must be an int"),
            (dict(init_skip_steps=(1, 2)), "init_skip_steps holds 2 entries for 1 unets"),
            (dict(init_skip_steps=4, sample_steps=4), "init_skip_steps=4 of unet 1 is outside 0 .. 3"),
            (dict(init_canvas=img[0]), r"init_canvas of unet 1 must be \[1, channels 3, H, W\]"),
            (dict(init_canvas=torch.rand(2, 3, 28, 28)), "init_canvas of unet 1 must be"),
            (dict(init_canvas=img.long()), "init_canvas of unet 1 must be of a floating dtype or uint8"),
            (dict(init_canvas=wide[..., ::2]), "init_canvas of unet 1 must have unit x stride"),
    ]:
        with pytest.raises(ValueError, match=match):
            im.sample_tiled((2, 2), **kw)
    # the per-tile names stay refused as they are, whatever comes with them
    with pytest.raises(NotImplementedError, match="inpaint_images"):
        im.sample_tiled((2, 2), inpaint_images=img, known_image=img, known_mask=mask)
    with pytest.raises(NotImplementedError, match="skip_steps"):
        im.sample_tiled((2, 2), skip_steps=2, init_skip_steps=2)
    import imagen_pytorch as ip

    unets = [ip.Unet(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False)]
    with pytest.raises(NotImplementedError, match="ElucidatedImagen"):
        ip.ElucidatedImagen(unets, image_sizes=(16,), condition_on_text=False, num_sample_steps=4).sample_tiled(
            (2, 2), known_image=img, known_mask=mask)
    if not torch.cuda.is_available():   # what passes the checks reaches the engine
        with pytest.raises(ip._engine.EngineUnavailable):
            im.sample_tiled((2, 2), seed=3, known_image=img, known_mask=mask, known_resample_times=2, init_canvas=img,
                            init_skip_steps=3)


def test_normalize_known_converts_once_and_keeps_views():
    from imagen_pytorch.imagen_pytorch import normalize_init_canvas, normalize_known

    big, keep = torch.rand(1, 3, 64, 64), torch.rand(64, 64) > 0.5
    win, mwin = big[:, :, 8:36, 12:40], keep[8:36, 12:40]
    img, mask, R_ = normalize_known(win, mwin, 3, channels=3)
    assert img.data_ptr() == win.data_ptr() and img.stride() == win.stride() and R_ == 3       # used in place
    assert mask.data_ptr() == mwin.data_ptr() and mask.stride() == mwin.stride()
    img, mask, _ = normalize_known((win * 255).to(torch.uint8), mwin.float()[None] * 0.5, channels=3)
    assert img.dtype == torch.float32 and float(img.max()) <= 1.0 and mask.dtype == torch.uint8 and mask.shape == (28, 28)
    assert torch.equal(mask.bool(), mwin)
    assert normalize_known(None, None, channels=3) == (None, None, 1)
    (init, skip), = normalize_init_canvas(win, 3, steps=[8], channels=3)
    assert init.data_ptr() == win.data_ptr() and skip == 3
    assert normalize_init_canvas((None, win), (None, 2), steps=[8, 8], channels=3, start_at_unet_number=2)[0] == (None, 0)
    assert normalize_init_canvas(None, None, steps=[8], channels=3) == [(None, 0)]


def test_fused_drivers_refuse_by_name_before_a_model_is_loaded():
    from ultra_res import grid as G
    from ultra_res import tiled as UT

    load = lambda stage: (_ for _ in ()).throw(AssertionError("no model may be loaded for a refused call"))
    with pytest.raises(ValueError, match="known must be"):
        UT.fused_canvas(load, num_patches_width=2, known=torch.zeros(1, 3, 28, 28))
    geom = G.GridGeometry(8, 6, 3, 24, 80)
    zoomed, canvas, keep = torch.rand(1, 3, 20, 20), torch.rand(1, 3, 80, 80), torch.zeros(80, 80, dtype=torch.uint8)
    for kw, match in [
            (dict(canvas=canvas, background=False), "needs background=True"),
            (dict(canvas=canvas[:, :, :40]), "canvas must be a contiguous float32"),
            (dict(canvas=canvas.double()), "canvas must be a contiguous float32"),
            (dict(keep=keep), "needs canvas="),
            (dict(canvas=canvas, keep=keep[:40]), "keep must be a bool / uint8"),
            (dict(canvas=canvas, keep=keep.float()), "keep must be a bool / uint8"),
            (dict(canvas=canvas, known_resample_times=2), "needs keep="),
            (dict(refine_skip_steps=2, background=False), "needs background=True"),
    ]:
        with pytest.raises(ValueError, match=match):
            UT.fused_level(load, zoomed, geom, [(0, 0)], **kw)


# ------------------------------------------------------------------------------------------------ tables, masks, windows
@pytest.mark.parametrize("name,eta", SOLVERS[1:])
def test_canvas_tables_take_the_first_step_walked(name, eta):
    from imagen_pytorch.imagen_pytorch import GaussianDiffusionContinuousTimes, canvas_tables, solver_tables

    t = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=8).step_tables()
    for skip in (0, 3, 7):
        got, want = canvas_tables(t, name, eta, skip=skip), solver_tables(t, name, eta=eta, skip=skip)
        assert all(torch.equal(got[n], want[n]) for n in want)
    assert all(torch.equal(v, canvas_tables(t, name, eta, skip=0)[n]) for n, v in canvas_tables(t, name, eta).items())
    if name == "dpmpp_2m":
        assert float(canvas_tables(t, name, skip=3)["coef_prev"][3]) == 0.0 != float(canvas_tables(t, name)["coef_prev"][3])
    ddpm = canvas_tables(t, "ddpm", skip=3)
    assert all(torch.equal(v, canvas_tables(t, "ddpm")[n]) for n, v in ddpm.items())


def test_level_keep_mask_is_the_union_of_the_tile_squares():
    from ultra_res import grid as G
    from ultra_res import tiled as UT

    geom = G.GridGeometry(8, 6, 4, 12, 52)   # 4 x 4 tiles of 16 at stride 12
    positions = [(0, 0), (1, 2), (3, 3), (1, 2)]
    got = UT.level_keep_mask(geom, positions)
    want = torch.zeros(52, 52, dtype=torch.uint8)
    for y in range(52):
        for x in range(52):
            want[y, x] = int(any(i * 12 <= y < i * 12 + 16 and j * 12 <= x < j * 12 + 16 for i, j in positions))
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert int(UT.level_keep_mask(geom, []).sum()) == 0 and bool(UT.level_keep_mask(geom, geom.positions).all())
    with pytest.raises(ValueError, match="inside the 4 x 4 grid"):
        UT.level_keep_mask(geom, [(4, 0)])


class _Recorder:
    """Stands in for an Imagen: records what fused_level hands to sample_tiled, stage by stage."""

    def __init__(self):
        self.unets, self.image_sizes, self.calls = [None, None], (16, 32), []

    def to(self, device):
        return self

    def sample_tiled(self, **kw):
        self.calls.append(kw)
        return kw["into"][0] if kw.get("into") else torch.zeros(1)


def test_fused_level_hands_down_windows_of_the_canvas_and_the_mask():
    from ultra_res import grid as G
    from ultra_res import tiled as UT

    geom = G.GridGeometry(8, 6, 4, 24, 104)   # the last stage: 4 x 4 tiles of 32 at stride 24
    zoomed, canvas = torch.rand(1, 3, 26, 26), torch.rand(1, 3, 104, 104)
    positions = [(1, 2), (2, 2), (2, 3)]
    keep = UT.level_keep_mask(geom, [p for p in geom.positions if p not in positions])
    before = canvas.clone()
    rec = _Recorder()
    common = dict(stages=(1, 2), device="cpu", window=16, seed=1)
    out = UT.fused_level(lambda stage: rec, zoomed, geom, positions, canvas=canvas, keep=keep, known_resample_times=2,
                         refine_skip_steps={2: 3}, **common)
    assert out is canvas and torch.equal(canvas, before) and len(rec.calls) == 2
    box = (slice(24, 24 + 56), slice(48, 48 + 56))   # rows 1 .. 2, columns 2 .. 3 of the 32 / 24 lattice
    for stage, kw in zip((1, 2), rec.calls):
        for got, want in ((kw["known_image"], canvas[:, :, box[0], box[1]]), (kw["known_mask"], keep[box]),
                          (kw["init_canvas"], canvas[:, :, box[0], box[1]])):
            assert got.data_ptr() == want.data_ptr() and got.shape == want.shape and got.stride() == want.stride()
        assert kw["known_resample_times"] == 2 and kw["init_skip_steps"] == (None, 3) and kw["streamed"]
        assert kw["present"] == [[True, False], [True, True]] and kw["grid"] == (2, 2)
        assert (kw["into"] is None) == (stage == 1)
    assert rec.calls[1]["into"][0] is canvas and tuple(rec.calls[1]["into"][1:]) == (24, 48)
    # without keep and refine nothing new is handed down; the canvas takes the place of the background
    rec = _Recorder()
    UT.fused_level(lambda stage: rec, zoomed, geom, positions, canvas=canvas, **common)
    assert all(k not in rec.calls[0] for k in ("known_image", "known_mask", "init_canvas")) and rec.calls[1]["into"][0] is canvas
    rec = _Recorder()
    out = UT.fused_level(lambda stage: rec, zoomed, geom, positions, refine_skip_steps=2, **common)
    init = rec.calls[0]["init_canvas"]
    assert init.data_ptr() == out[:, :, box[0], box[1]].data_ptr() and init.shape == (1, 3, 56, 56)
    assert torch.equal(out, UT.level_background(zoomed, 104)) and rec.calls[0]["init_skip_steps"] == 2


# ------------------------------------------------------------------------------------------------ the restatement
KW1 = dict(image_sizes=(16,), timesteps=(8,), pred_objectives=("noise",), condition_on_text=False)


def _one_stage():
    return SR.Imagen([H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=3)], **KW1)


def test_nothing_known_is_the_canvas_of_before():
    """An all-zero mask, R = 1, no init image: tests/tiled_ref.py bit for bit."""
    oim = _one_stage()
    nf = RS.generator_noise_fn(13)
    want = TR.sample_tiled(oim, grid=(2, 2), noise_fn=nf, sampler="dpmpp_2m")
    got = KR.sample_tiled(oim, grid=(2, 2), noise_fn=nf, sampler="dpmpp_2m", known_image=torch.rand(1, 3, 28, 28),
                          known_mask=torch.zeros(28, 28, dtype=torch.bool))
    assert torch.equal(got, want)
    assert torch.equal(KR.sample_tiled(oim, grid=(2, 2), noise_fn=nf, sampler="dpmpp_2m"), want)


def _tile_mask():
    m = torch.zeros(16, 16, dtype=torch.bool)
    m[:, :6] = True
    m[9:13, 8:14] = True
    return m


@pytest.mark.parametrize("R_", [1, 2])
@pytest.mark.parametrize("name,eta", SOLVERS)
def test_one_tile_with_a_mask_is_the_solver_restatement(name, eta, R_):
    """A 1 x 1 lattice: the canvas is tests/solver_ref.py's sampler at batch 1 under inpainting, bit for bit on the unknown
    pixels; a known pixel is the known value copied, where the oracle leaves ((2 v - 1) + 1) / 2 - two roundings of at most
    2^-24 each: 1.2e-7."""
    oim = _one_stage()
    m = _tile_mask()
    KR.assert_mask_condition(m, [KR.lattice(16, (1, 1))])
    kn = torch.rand(1, 3, 16, 16, generator=H.gen(5))
    nf = RS.generator_noise_fn(11)
    want = oim.sample(noise_fn=nf, batch_size=1, sampler=name, sampler_eta=eta, inpaint_images=kn, inpaint_masks=m[None],
                      inpaint_resample_times=R_)
    got = KR.sample_tiled(oim, grid=(1, 1), noise_fn=nf, sampler=name, sampler_eta=eta, known_image=kn, known_mask=m,
                          known_resample_times=R_)
    assert torch.equal(got[0, :, ~m], want[0, :, ~m]) and float(got[0, :, ~m].std()) > 0.01
    assert torch.equal(got[0, :, m], kn[0, :, m])
    err = float((got - want)[0, :, m].abs().max())
    print(f"1x1 {name} eta {eta} R {R_}: known pixels max|copied - round trip| = {err:.2e}")
    assert err <= 1.2e-7


@pytest.mark.parametrize("name,skip", [("ddpm", 3), ("ddpm", 5), ("dpmpp_2m", 3), ("ddim", 7)])
def test_one_tile_from_an_image_is_the_init_images_restatement(name, skip):
    oim = _one_stage()
    init = torch.rand(1, 3, 24, 20, generator=H.gen(6))
    nf = RS.generator_noise_fn(12)
    want = oim.sample(noise_fn=nf, batch_size=1, sampler=name, init_images=init, skip_steps=skip)
    got = KR.sample_tiled(oim, grid=(1, 1), noise_fn=nf, sampler=name, init_canvas=init, init_skip_steps=skip)
    assert torch.equal(got, want)
    assert not torch.equal(got, KR.sample_tiled(oim, grid=(1, 1), noise_fn=nf, sampler=name, init_canvas=init, init_skip_steps=skip - 1))


# ------------------------------------------------------------------------------------------------ exactness
MU, SD = 0.3, 0.5


def _gauss_denoiser(sched):
    """The closed-form denoiser of data N(mu, sd^2) that tests/test_tiled.py uses, pointwise, with the static threshold."""

    def den(times, x):
        a, s = RS.log_snr_to_alpha_sigma(RS._pad(x, sched.log_snr(times)))
        return ((a * SD ** 2 * x + s ** 2 * MU) / (a ** 2 * SD ** 2 + s ** 2)).clamp(-1.0, 1.0)

    return den


def _lattice_mask():
    """For the 3 x 2 lattice of 16-pixel tiles at overlap 0.25 (canvas 40 x 28): columns [0, 8), rows [20, 24) and a patch
    inside the top right and the bottom right tile (41 % known)."""
    m = torch.zeros(40, 28, dtype=torch.bool)
    m[:, :8] = True
    m[20:24, :] = True
    m[2:6, 18:26] = True
    m[30:34, 14:22] = True
    return m


@pytest.mark.parametrize("R_", [1, 2])
@pytest.mark.parametrize("name,eta", SOLVERS)
@pytest.mark.parametrize("weights", ["uniform", "ramp"])
def test_a_pointwise_denoiser_makes_the_masked_tiled_canvas_the_whole_canvas(weights, name, eta, R_):
    """Equal estimates wherever tiles overlap: the restatement on a 3 x 2 lattice with a mask equals the same solver, mix
    and re-noise on the whole canvas as one image.  Uniform weights: sums of 1, 2 or 4 equal values divided by their count
    are exact, the difference is 0; ramp weights: the bound 1e-5 of tests/test_tiled.py."""
    sched = RS.GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=8)
    lat = KR.lattice(16, (3, 2), 0.25)
    m = _lattice_mask()
    KR.assert_mask_condition(m, [lat])
    nf = RS.generator_noise_fn(7)
    den = _gauss_denoiser(sched)
    shape = (1, 3, lat["Hc"], lat["Wc"])
    kn = torch.rand(shape, generator=H.gen(9))
    x_T = nf(("init", 1), shape)
    got, covered = KR.run_canvas(lambda k, t, tn, tiles, prev: den(t, tiles), x_T, lat, sched, name, eta, nf, 1, weights, kn, m, R_)
    assert bool(covered.all())
    solver, x = KR.CanvasSolver(sched, name, eta), x_T
    for k, (t, tn) in enumerate(solver.steps):
        for r in reversed(range(R_)):
            x = torch.where(m, sched.q_sample(kn * 2 - 1, t, nf(("inpaint", 1, k, r), shape)), x)
            kept = (solver.x0_prev, solver.h_prev)
            x = solver.step(k, x, den(t, x), nf(("step", 1, k, r), shape) if solver.wants_noise(k) else None)
            if r > 0:
                solver.x0_prev, solver.h_prev = kept
                if k < len(solver.steps) - 1:
                    x = sched.q_sample_from_to(x, tn, t, nf(("renoise", 1, k, r), shape))
    err = float((got - x).abs().max())
    print(f"masked tiled exactness {weights} {name} eta {eta} R {R_}: max|tiled - whole canvas| = {err:.2e}")
    assert (err == 0.0 if weights == "uniform" else err < 1e-5) and float(x.std()) > 0.1
