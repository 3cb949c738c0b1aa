"""Fused-tile canvas sampling on the MI355X: kd_tiles_gather against slicing, kd_tiles_fuse_update against the fp64
expression on the same inputs, Imagen.sample_tiled against the restatement tests/tiled_ref.py on the 16 -> 32 cascade of
tests/test_solvers_gpu.py (tiles 16 and 32, T = 8), its invariants bit for bit, and the driver ultra_res.tiled.fused_canvas."""
import ctypes as C

import pytest
import torch

import helpers as H
import self_cond_ref as SC
import tiled_ref as TR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

REL = 1e-6           # the solver-step bound (tests/test_solvers_gpu.py, tests/test_ddpm_step_gpu.py)
SAMPLE_ABS = 2e-3    # the project's sampler bound against the oracle on identical noise
TWO_PLANS = 4e-3     # tests/test_seeds_gpu.py: two plans of different batch, each within 2e-3 of the oracle
N = 8
HOLE = [[True, True], [True, False], [True, True]]


def _lattice(S, st, grid, present=None):
    ny, nx = grid
    present = [[True] * nx for _ in range(ny)] if present is None else present
    origins = [(r * st, q * st) for r in range(ny) for q in range(nx) if present[r][q]]
    tile_of, n = [], 0
    for r in range(ny):
        tile_of.append([])
        for q in range(nx):
            tile_of[-1].append(n if present[r][q] else -1)
            n += int(present[r][q])
    return dict(S=S, st=st, ny=ny, nx=nx, Hc=(ny - 1) * st + S, Wc=(nx - 1) * st + S, origins=origins, tile_of=tile_of)


# ------------------------------------------------------------------------------------------------ kd_tiles_gather
def _gather(canvas, lat, origins):
    E = H.engine()
    Cn = canvas.shape[0]
    out = torch.full((len(origins), Cn, lat["S"], lat["S"]), float("nan"), device=canvas.device)
    yx = (C.c_int * (2 * len(origins)))(*[v for o in origins for v in o])
    E.check(E.load().kd_tiles_gather(E.ptr(canvas), E.ptr(out), len(origins), Cn, lat["Hc"], lat["Wc"], lat["S"], yx,
                                     E.current_stream()))
    return out


@pytest.mark.parametrize("Cn", [1, 3, 4])
@pytest.mark.parametrize("st", [12, 8])
def test_gather_is_slicing(device, Cn, st):
    """Lattices 2 x 2, 3 x 2 and 1 x 1 of 16-pixel tiles; B = 1, 3, 5 with repeated and out-of-order origins, and 33 (two
    launches: the origins travel 32 per kernel argument)."""
    for grid in ((2, 2), (3, 2), (1, 1)):
        lat = _lattice(16, st, grid)
        canvas = torch.randn(Cn, lat["Hc"], lat["Wc"], generator=H.gen(st + Cn)).to(device)
        o = lat["origins"]
        for idx in ([len(o) - 1], [2, 0, 2], [2, 0, 2, 1, 0], list(range(33))):
            origins = [o[i % len(o)] for i in idx]
            got = _gather(canvas, lat, origins)
            want = torch.stack([canvas[:, y0:y0 + 16, x0:x0 + 16] for y0, x0 in origins])
            assert torch.equal(got, want), (grid, idx)


def test_gather_refuses_what_it_cannot_move(device):
    E = H.engine()
    lat = _lattice(16, 12, (2, 2))
    canvas = torch.zeros(3, 28, 28, device=device)
    for origins, match in (([(0, 2)], "multiple of 4"), ([(16, 0)], "outside the canvas"), ([(0, -4)], "outside the canvas")):
        with pytest.raises(E.EngineError, match=match):
            _gather(canvas, lat, origins)
    with pytest.raises(E.EngineError, match="S % 4"):
        _gather(canvas, dict(lat, S=18), [(0, 0)])


# ------------------------------------------------------------------------------------------------ kd_tiles_fuse_update
def _fuse(x, x0bar, tiles, thr, lat, ramp, A, B, P, Sn, noise=None, seed=0, sid=0):
    E = H.engine()
    tile_of = torch.tensor(lat["tile_of"], dtype=torch.int32, device=x.device)
    E.check(E.load().kd_tiles_fuse_update(E.ptr(x), E.ptr(x0bar), E.ptr(tiles), E.ptr(thr), C.c_void_p(tile_of.data_ptr()),
                                          tiles.shape[0], tiles.shape[1], lat["S"], lat["st"], lat["ny"], lat["nx"], int(ramp),
                                          A, B, P, Sn, E.ptr(noise), seed, sid, E.current_stream()))
    torch.cuda.synchronize()


def _fuse_fp64(x, hist, tiles, thr, lat, ramp, A, B, P, Sn, z):
    """(x_next, x0bar, covered) in fp64 over the fp32 inputs and the fp32 weights."""
    S = lat["S"]
    w = TR.weight(S, lat["st"], "ramp" if ramp else "uniform").double()
    s = (thr.double().clamp(min=1.0) if thr is not None else torch.ones(tiles.shape[0], dtype=torch.float64))[:, None, None, None]
    x0c = torch.maximum(torch.minimum(tiles.double(), s), -s) / s
    num, den = torch.zeros_like(x, dtype=torch.float64), torch.zeros(lat["Hc"], lat["Wc"], dtype=torch.float64)
    for t, (y0, x0) in enumerate(lat["origins"]):
        num[:, y0:y0 + S, x0:x0 + S] += w * x0c[t]
        den[y0:y0 + S, x0:x0 + S] += w
    covered = den > 0
    xb = num / den.clamp(min=1e-30)
    out = A * x.double() + B * xb
    if P != 0:
        out = out + P * hist.double()
    if Sn != 0:
        out = out + Sn * z.double()
    return torch.where(covered, out, x.double()), xb, covered


@pytest.mark.parametrize("grid,present", [((2, 2), None), ((3, 3), None), ((3, 2), HOLE)])
@pytest.mark.parametrize("S,st", [(16, 12), (16, 8), (20, 8)])
def test_fuse_update_matches_fp64_expression(device, S, st, grid, present):
    """Up to 2 (S 16) and 3 (S 20 / st 8: 9 tiles) covering tiles per axis; uniform and ramp weights; dynamic thresholds in
    [1, 3] and d_thr = NULL; all four terms, then P = 0 over a NaN-filled d_x0bar and Sn = 0 over a NaN d_noise: a zero
    coefficient leaves its operand unread.  The hole's uncovered pixels keep their bits in both buffers."""
    lat = _lattice(S, st, grid, present)
    Cn, n = 3, len(lat["origins"])
    g = H.gen(S + st + n)
    x_in = torch.randn(Cn, lat["Hc"], lat["Wc"], generator=g) * 1.5
    hist_in = torch.rand(Cn, lat["Hc"], lat["Wc"], generator=g) * 2 - 1
    tiles = torch.randn(n, Cn, S, S, generator=g) * 1.5
    z = torch.randn(Cn, lat["Hc"], lat["Wc"], generator=g)
    nan = torch.full_like(x_in, float("nan"))
    worst = 0.0
    for ramp in (0, 1):
        for thr in (torch.rand(n, generator=g) * 2 + 1, None):
            for A, B, P, Sn, hist, noise in ((0.83, 0.21, -0.07, 0.4, hist_in, z), (0.83, 0.21, 0.0, 0.4, nan, z),
                                             (0.83, 0.21, -0.07, 0.0, hist_in, nan)):
                x, xb = x_in.to(device), hist.to(device)
                _fuse(x, xb, tiles.to(device), None if thr is None else thr.to(device), lat, ramp, A, B, P, Sn, noise.to(device))
                want_x, want_xb, covered = _fuse_fp64(x_in, hist, tiles, thr, lat, ramp, A, B, P, Sn, noise)
                # (at S = 2 st and above the hole's neighbours cover its slot: only S 16 / st 12 leaves pixels bare)
                assert bool(covered.all()) == (present is None or S >= 2 * st)
                x, xb = x.cpu(), xb.cpu()
                assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(xb[:, covered]).all())
                e = max(H.rel_l2(x[:, covered], want_x[:, covered]), H.rel_l2(xb[:, covered], want_xb[:, covered]))
                worst = max(worst, e)
                assert e <= REL, (ramp, thr is None, P, Sn, e)
                # bit-unchanged where no tile lies (NaN fill included: compare the words)
                assert torch.equal(x[:, ~covered], x_in[:, ~covered])
                assert torch.equal(xb[:, ~covered].view(torch.int32), hist[:, ~covered].view(torch.int32))
    print(f"fuse update S{S} st{st} {grid} {'hole' if present else 'full'}: worst rel-L2 {worst:.2e}")


def test_fuse_update_draws_the_canvas_stream(device):
    """A = B = P = 0, Sn = 1, no noise tensor: the output is kd_philox_normal over the canvas' numel under the same key and
    stream id, bit for bit - whatever the tiling (two lattices over one 32 x 32 canvas)."""
    E = H.engine()
    seed, sid = 0x1234567, E.stream_id(1, 5)
    want = torch.empty(3, 32, 32, device=device)
    E.check(E.load().kd_philox_normal(E.ptr(want), want.numel(), seed, sid, E.current_stream()))
    for S, st, grid in ((16, 8, (3, 3)), (20, 12, (2, 2))):
        lat = _lattice(S, st, grid)
        assert (lat["Hc"], lat["Wc"]) == (32, 32)
        x = torch.randn(3, 32, 32, generator=H.gen(1)).to(device)
        xb = torch.zeros_like(x)
        tiles = torch.randn(len(lat["origins"]), 3, S, S, generator=H.gen(2)).to(device)
        _fuse(x, xb, tiles, None, lat, 0, 0.0, 0.0, 0.0, 1.0, None, seed, sid)
        assert torch.equal(x, want)


@pytest.mark.parametrize("st", [12, 8])
def test_crops_of_one_canvas_fuse_back_to_it(device, st):
    """Tiles that are crops of one canvas X0, threshold 1, uniform weights, at most 2 tiles per axis: sums of 1, 2 or 4
    equal values divided by 1, 2 or 4 are exact, x0bar is clamp(X0) bit for bit."""
    lat = _lattice(16, st, (3, 3))
    X0 = torch.randn(3, lat["Hc"], lat["Wc"], generator=H.gen(st)) * 1.2
    tiles = torch.stack([X0[:, y0:y0 + 16, x0:x0 + 16] for y0, x0 in lat["origins"]]).contiguous()
    for thr in (None, torch.ones(9)):
        x, xb = torch.zeros_like(X0).to(device), torch.zeros_like(X0).to(device)
        _fuse(x, xb, tiles.to(device), None if thr is None else thr.to(device), lat, 0, 0.5, 0.5, 0.0, 0.0)
        assert torch.equal(xb.cpu(), X0.clamp(-1.0, 1.0))


def test_fuse_update_refuses_more_than_nine_tiles(device):
    E = H.engine()
    lat = _lattice(16, 4, (2, 2))
    x = torch.zeros(3, 20, 20, device=device)
    with pytest.raises(E.EngineError, match="more than 3 tiles per axis"):
        _fuse(x, torch.zeros_like(x), torch.zeros(4, 3, 16, 16, device=device), None, lat, 0, 1.0, 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ whole sampler
CASCADE_KW = dict(image_sizes=(16, 32), timesteps=(N, N), pred_objectives=("noise", "v"), condition_on_text=False)


def _unets(channels=3, **extra):
    return [H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=3, channels=channels, **extra),
            H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=6, channels=channels, lowres_cond=True, **extra)]


def _cascade(device, unets=None, **over):
    kw = dict(CASCADE_KW, **over)
    oim = RS.Imagen(unets or _unets(kw.get("channels", 3)), **kw)
    return oim, H.product_imagen(oim, "Imagen", device, **kw)


@pytest.fixture(scope="module")
def cascade(device):
    return _cascade(device)


def _err(oim, pim, device, label, grid=(2, 2), **kw):
    nf = RS.generator_noise_fn(41)
    ref = TR.sample_tiled(oim, grid=grid, noise_fn=nf, **kw)
    dv = {k: v.to(device) if torch.is_tensor(v) else v for k, v in kw.items()}
    got = pim.sample_tiled(grid, noise_fn=nf, device=device, **dv).cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and float(got.std()) > 0.01
    err = float((got - ref).abs().max())
    print(f"tiled {label}: canvas {tuple(got.shape[-2:])}, max|diff| {err:.2e}")
    return err


@pytest.mark.parametrize("sampler,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_canvas_matches_the_restatement(device, cascade, sampler, eta):
    """2 x 2 lattice, canvases 28 and 56, injected noise."""
    oim, pim = cascade
    assert _err(oim, pim, device, f"{sampler} eta {eta} 2x2", sampler=sampler, sampler_eta=eta) < SAMPLE_ABS


def test_ramp_weights_match_the_restatement(device, cascade):
    oim, pim = cascade
    assert _err(oim, pim, device, "dpmpp_2m ramp 2x2", sampler="dpmpp_2m", tile_weights="ramp") < SAMPLE_ABS


def test_a_lattice_with_a_hole_matches_the_restatement(device, cascade):
    oim, pim = cascade
    nf = RS.generator_noise_fn(41)
    assert _err(oim, pim, device, "ddim 0.5 3x2 with a hole", grid=(3, 2), present=HOLE, sampler="ddim", sampler_eta=0.5) < SAMPLE_ABS
    got = pim.sample_tiled((3, 2), present=HOLE, noise_fn=nf, device=device, sampler="ddim", sampler_eta=0.5)
    assert got.shape == (1, 3, 80, 56) and bool((got[0, :, 32:48, 32:] == 0).all()) and float(got[0, :, :24].std()) > 0.01


def test_cond_images_match_the_restatement(device):
    oim, pim = _cascade(device, _unets(cond_images_channels=3))
    cond = torch.rand(4, 3, 20, 20, generator=H.gen(8))
    assert _err(oim, pim, device, "dpmpp_2m cond_images 2x2", sampler="dpmpp_2m", cond_images=cond) < SAMPLE_ABS


def test_self_conditioned_unet_matches_the_restatement(device):
    """The carry of a tile is its crop of the previous step's FUSED estimate."""
    ou = H.ref_unet(SC.Unet, H.UNET_KW["small1"], seed=21, self_cond=True)
    kw = dict(image_sizes=(16,), timesteps=(N,), pred_objectives=("noise",), condition_on_text=False)
    oim = RS.Imagen([ou], **kw)
    pim = H.product_imagen(oim, "Imagen", device, **kw)
    assert pim.unets[0].self_cond
    assert _err(oim, pim, device, "dpmpp_2m self-cond 2x2", sampler="dpmpp_2m") < SAMPLE_ABS


def test_text_guided_canvas_matches_the_restatement(device):
    ou = H.ref_unet(R.Unet, dict(H.UNET_KW["small1"], cond_dim=64, text_embed_dim=3), seed=17, text=True)
    kw = dict(image_sizes=(16,), timesteps=(N,), text_embed_dim=3)
    oim = RS.Imagen([ou], **kw)
    pim = H.product_imagen(oim, "Imagen", device, **kw)
    text = torch.randn(1, 2, 3, generator=H.gen(4))
    assert _err(oim, pim, device, "dpmpp_2m text cond_scale 3 2x2", sampler="dpmpp_2m", text_embeds=text, cond_scale=3.0) < SAMPLE_ABS


def test_one_channel_canvas_matches_the_restatement(device):
    oim, pim = _cascade(device, channels=1)
    assert _err(oim, pim, device, "dpmpp_2m channels=1 2x2", sampler="dpmpp_2m") < SAMPLE_ABS


def test_sample_steps_walks_the_short_schedule_of_a_1000_step_model(device):
    oim, pim = _cascade(device, timesteps=1000)
    assert _err(oim, pim, device, "dpmpp_2m timesteps=1000 sample_steps=(8, 6) 2x2", sampler="dpmpp_2m", sample_steps=(8, 6)) < SAMPLE_ABS


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0), ("ddpm", 0.0)])
def test_one_tile_is_sample_at_batch_1(device, cascade, sampler, eta):
    """A 1 x 1 lattice with uniform weights: the solvers' canvas is sample(batch_size=1, seed=s, sampler=...) bit for bit
    through both stages (the same start, low-res augmentation and step streams; w x / w = x); "ddpm" runs the ancestral
    step in the linear form and stays within the sampler bound of sample()'s."""
    pim = cascade[1]
    kw = dict(seed=77, sampler=sampler, sampler_eta=eta, device=device)
    got, want = pim.sample_tiled((1, 1), **kw), pim.sample(batch_size=1, **kw)
    assert got.shape == want.shape == (1, 3, 32, 32)
    if sampler == "ddpm":
        err = float((got - want).abs().max())
        print(f"tiled 1x1 ddpm against the ancestral sample(): max|diff| {err:.2e}")
        assert err < SAMPLE_ABS
    else:
        assert torch.equal(got, want)


def test_graph_and_repetition_do_not_change_a_bit(device, cascade):
    pim = cascade[1]
    kw = dict(seed=5, sampler="ddim", sampler_eta=0.5, device=device, tile_batch=3)
    a = pim.sample_tiled((2, 2), **kw)
    assert torch.equal(a, pim.sample_tiled((2, 2), **kw))
    assert torch.equal(a, pim.sample_tiled((2, 2), use_graph=False, **kw))
    assert not torch.equal(a, pim.sample_tiled((2, 2), **dict(kw, seed=6)))


def test_tiled_sampling_leaves_nothing_behind_that_sample_reads(device, cascade):
    pim = cascade[1]
    calls = [dict(batch_size=3, seed=[5, 6, 7], sampler="dpmpp_2m"), dict(batch_size=1, seed=9)]
    before = [pim.sample(device=device, **c) for c in calls]
    pim.sample_tiled((2, 2), seed=3, sampler="dpmpp_2m", tile_batch=3, device=device)
    fresh = _cascade(device)[1]
    for c, b in zip(calls, before):
        assert torch.equal(pim.sample(device=device, **c), b) and torch.equal(fresh.sample(device=device, **c), b), c


def test_tiled_sampling_under_poisoned_scratch(device, cascade):
    E = H.engine()
    pim = cascade[1]
    kw = dict(seed=5, sampler="dpmpp_2m", tile_batch=3, device=device)
    base = pim.sample_tiled((2, 2), **kw)
    assert bool(torch.isfinite(base).all())
    for word in (0xFFFFFFFF, 0x7149F2CA, 0):
        n = 0
        for u in pim.unets:
            for h in u._engines.values():
                filled = C.c_int64(-1)
                E.check(E.load().kd_unet_poison_scratch(h, word, C.byref(filled), E.current_stream()))
                assert filled.value > 0
                n += 1
        assert n >= 4   # two stages, the plans of batch 3 and batch 1
        assert torch.equal(pim.sample_tiled((2, 2), **kw), base), hex(word)


def test_the_canvas_does_not_follow_the_tile_batch(device, cascade):
    """tile_batch 1, 3 (chunks of 3 + 1) and 4 under one seed: plans of different batch sizes, each within the sampler
    bound of the oracle."""
    pim = cascade[1]
    outs = [pim.sample_tiled((2, 2), seed=12, sampler="ddim", sampler_eta=0.5, tile_batch=tb, device=device) for tb in (1, 3, 4)]
    d = max(float((outs[0] - o).abs().max()) for o in outs[1:])
    print(f"tiled 2x2 DDIM(0.5): tile_batch 1 vs 3 and 4 max|diff| {d:.2e}")
    assert d < TWO_PLANS


def test_fused_canvas_is_the_call_made_by_hand(device, cascade):
    from ultra_res import tiled as UT

    pim = cascade[1]
    kw = dict(overlap=0.25, tile_batch=4, sampler="dpmpp_2m", seed=21, tile_weights="ramp")
    got = UT.fused_canvas(lambda stage: pim, num_patches_width=2, stages=(1, 2), device=device, **kw)
    assert got.shape == (1, 3, 56, 56)
    assert torch.equal(got, pim.sample_tiled((2, 2), device=device, **kw))
    steps = UT.fused_canvas(lambda stage: pim, grid=(2, 2), stages=(1, 2), device=device, **dict(kw, sample_steps={2: 5}))
    assert torch.equal(steps, pim.sample_tiled((2, 2), device=device, **dict(kw, sample_steps=(None, 5))))
    assert not torch.equal(steps, got)
