"""The fused level on the MI355X: the three level kernels of csrc/kernels_tiles.hip bit for bit against what they replace
(kd_tiles_cond_gather against the materialised conditioning images, kd_tiles_gather_lowres against kd_tiles_gather of the
augmented canvas, kd_tiles_finalize against the torch finish), their addressing past 2^31 canvas elements, their refusals;
sample_tiled(streamed=, cond_crops=, into=) bit for bit against the default call on the 16 -> 32 cascade of
tests/test_tiled_gpu.py; ultra_res.tiled.fused_level against the call made by hand and against the restatement
tests/tiled_ref.py over the oracle; and one mag-2 level at the pipeline's real sizes."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import fused_level_ref as FR
import helpers as H
import self_cond_ref as SC
import tiled_ref as TR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

SAMPLE_ABS = 2e-3    # the project's sampler bound against the oracle on identical noise
N = 8
HOLE = [[True, True], [True, False], [True, True]]
NAN = float("nan")


def _G():
    from ultra_res import grid as G

    return G


def _ints(pairs):
    return (C.c_int * (2 * len(pairs)))(*[int(v) for p in pairs for v in p])


def _iptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


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


# ------------------------------------------------------------------------------------------------ kd_tiles_cond_gather
def _cond_gather(src, shifts, top, win, centre, fill, S, out=None):
    E = H.engine()
    Cs, W = src.shape[0], src.shape[2]
    if out is None:
        out = torch.full((len(shifts), Cs * (1 if centre is None else 2), S, S), NAN, device=src.device)
    E.check(E.load().kd_tiles_cond_gather(E.ptr(src), Cs, W, E.ptr(out), len(shifts), S, _ints(shifts), top, _iptr(win),
                                          _iptr(centre), fill, E.current_stream()))
    return out


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("v2", [False, True], ids=["3ch", "6ch"])
def test_cond_gather_is_the_materialised_images(device, case, v2):
    """The cases of tests/test_fused_level.py (toy lattice with its shift-0 row and the half-to-even offset; mag 1 and mag 2
    at their real numbers), B = 1, 5 and 33 tiles (two launches: the shifts travel 32 per kernel argument)."""
    from imagen_pytorch import cond_crop_maps

    G = _G()
    label, W, window, geom, pos, sizes = FR.cond_cases(G)[case]
    zoomed = torch.rand(1, 3, W, W, generator=H.gen(W)).to(device)
    top = G.center_crop_offset(W, window)
    shifts = FR.shifts_of(W, geom, pos)
    for S in sizes:
        want = FR.materialised(G, zoomed, geom, pos, window, S, 0.95, v2)
        win, centre = (None if m is None else m.to(device) for m in cond_crop_maps(window, S, geom.patch_width if v2 else None))
        for B in (1, 5, 33):
            idx = [(7 * k + B) % len(pos) for k in range(B)]
            got = _cond_gather(zoomed[0], [shifts[i] for i in idx], top, win, centre, 0.95, S)
            assert torch.equal(got, want[idx]), (label, S, B)


def test_cond_gather_refuses_what_it_cannot_move(device):
    from imagen_pytorch import cond_crop_maps

    E = H.engine()
    src = torch.rand(3, 44, 44, device=device)
    win = cond_crop_maps(24, 16)[0].to(device)
    out = torch.full((1, 3, 16, 16), NAN, device=device)
    for kw, match in ((dict(S=18), "S % 4"), (dict(shifts=[(44, 0)]), r"inside \(-W, W\)"), (dict(shifts=[(0, -44)]), r"inside \(-W, W\)"),
                      (dict(top=44), "window offset"), (dict(top=-1), "window offset")):
        a = dict(dict(shifts=[(1, 1)], top=10, S=16), **kw)
        with pytest.raises(E.EngineError, match=match):
            _cond_gather(src, a["shifts"], a["top"], win, None, 0.95, a["S"], out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())   # nothing was launched
    # a map entry outside the window is clamped into it: nothing is read outside the source
    wild = torch.tensor([-5, 10 ** 6] * 8, dtype=torch.int32, device=device)
    got = _cond_gather(src, [(0, 3)], 10, wild, None, 0.95, 16)
    assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------ kd_tiles_gather_lowres
def _gather(canvas, lat, origins):
    E = H.engine()
    out = torch.full((len(origins), canvas.shape[0], lat["S"], lat["S"]), NAN, device=canvas.device)
    E.check(E.load().kd_tiles_gather(E.ptr(canvas), E.ptr(out), len(origins), canvas.shape[0], lat["Hc"], lat["Wc"], lat["S"],
                                     _ints(origins), E.current_stream()))
    return out


def _gather_lowres(prev, lat, origins, a, s, noise=None, seed=0, sid=0, out=None, **over):
    E = H.engine()
    g = dict(lat, **over)
    if out is None:
        out = torch.full((len(origins), prev.shape[0], g["S"], g["S"]), NAN, device=prev.device)
    E.check(E.load().kd_tiles_gather_lowres(E.ptr(prev), prev.shape[1], prev.shape[2], E.ptr(out), len(origins), prev.shape[0],
                                            g["Hc"], g["Wc"], g["S"], _ints(origins), a, s, E.ptr(noise), seed, sid,
                                            E.current_stream()))
    return out


def _philox(shape, seed, sid, device):
    E = H.engine()
    z = torch.empty(shape, device=device)
    E.check(E.load().kd_philox_normal(E.ptr(z), z.numel(), seed, sid, E.current_stream()))
    return z


LOWRES_CASES = [((28, 28), 32, 24, (2, 2)),    # 28 -> 56
                ((28, 28), 16, 12, (9, 9)),    # 28 -> 112
                ((56, 56), 32, 24, (2, 2)),    # 56 -> 56: the same size
                ((10, 28), 16, 12, (3, 2))]    # 10 x 28 -> 40 x 28: another ratio per axis


@pytest.mark.parametrize("Cn", [1, 3, 4])
@pytest.mark.parametrize("prev_hw,S,st,grid", LOWRES_CASES)
def test_gather_lowres_is_the_gather_of_the_augmented_canvas(device, Cn, prev_hw, S, st, grid):
    """Against kd_tiles_gather of a (2 interpolate(prev) - 1) + s noise formed as Imagen._tiled_stage forms it, with injected
    noise and with the Philox stream (kd_philox_normal over the canvas); every tile, the tile at the last origin alone, and
    33 tiles with repeats; s = 0 over a NaN noise buffer."""
    lat = _lattice(S, st, grid)
    shape = (Cn, lat["Hc"], lat["Wc"])
    prev = torch.rand((Cn,) + prev_hw, generator=H.gen(S + Cn)).to(device)
    a, s = 0.9689, 0.2474
    seed, sid = 0xC0FFEE, H.engine().stream_id(16, 1)
    base = F.interpolate(prev[None], shape[1:], mode="nearest") * 2 - 1
    o = lat["origins"]
    for noise in (torch.randn(shape, generator=H.gen(3)).to(device), None):
        z = noise if noise is not None else _philox(shape, seed, sid, device)
        low = (a * base + s * z[None]).contiguous()[0]
        for origins in (o, [o[-1]], [o[(5 * k) % len(o)] for k in range(33)]):
            got = _gather_lowres(prev, lat, origins, a, s, noise, seed, sid)
            assert torch.equal(got, _gather(low, lat, origins)), (noise is None, len(origins))
    got = _gather_lowres(prev, lat, o, a, 0.0, torch.full(shape, NAN, device=device))
    assert torch.equal(got, _gather((a * base).contiguous()[0], lat, o))


def test_gather_lowres_refuses_what_it_cannot_move(device):
    E = H.engine()
    lat = _lattice(16, 12, (2, 2))
    prev = torch.rand(3, 14, 14, device=device)
    out = torch.full((1, 3, 16, 16), NAN, device=device)
    for origins, over, match in (([(0, 2)], {}, "multiple of 4"), ([(16, 0)], {}, "outside the canvas"), ([(0, -4)], {}, "outside the canvas"),
                                 ([(0, 0)], dict(S=18), "S % 4"), ([(0, 0)], dict(Wc=30), "Wc % 4"), ([(0, 0)], dict(Hc=12), "smaller than a tile")):
        with pytest.raises(E.EngineError, match=match):
            _gather_lowres(prev, lat, origins, 1.0, 0.5, out=out, **over)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())   # nothing was launched


# ------------------------------------------------------------------------------------------------ kd_tiles_finalize
def _finalize(x, lat, out, oy, ox, tile_of=None, n=None, **over):
    E = H.engine()
    g = dict(lat, **over)
    tile_of = torch.tensor(lat["tile_of"], dtype=torch.int32, device=x.device) if tile_of is None else tile_of
    E.check(E.load().kd_tiles_finalize(E.ptr(x), _iptr(tile_of), len(lat["origins"]) if n is None else n, x.shape[0], g["S"], g["st"],
                                       g["ny"], g["nx"], E.ptr(out), out.shape[1], out.shape[2], oy, ox, E.current_stream()))
    return out


@pytest.mark.parametrize("grid,present", [((2, 2), None), ((3, 2), HOLE)])
@pytest.mark.parametrize("oy,ox", [(0, 0), (8, 12)])
def test_finalize_is_the_torch_finish_pasted_in_place(device, grid, present, oy, ox):
    lat = _lattice(16, 12, grid, present)
    Hc, Wc = lat["Hc"], lat["Wc"]
    x = (torch.randn(3, Hc, Wc, generator=H.gen(Hc)) * 1.5).to(device)
    fin, covered = FR.finish(x, lat["origins"], 16)
    assert bool(covered.all()) == (present is None) and float(fin.min()) == 0.0 and float(fin.max()) == 1.0
    before = torch.randn(3, Hc + 16, Wc + 20, generator=H.gen(7)).to(device)
    want = before.clone()
    want[:, oy:oy + Hc, ox:ox + Wc] = torch.where(covered, fin, before[:, oy:oy + Hc, ox:ox + Wc])
    got = _finalize(x, lat, before.clone(), oy, ox)
    assert torch.equal(got, want)   # the finish where a tile lies, every other bit unchanged
    # and into a zero canvas of its own size it is the default path's result
    zero = _finalize(x, lat, torch.zeros_like(x), 0, 0)
    assert torch.equal(zero, torch.where(covered, fin, torch.zeros_like(fin)))


def test_finalize_refuses_what_it_cannot_write(device):
    E = H.engine()
    lat = _lattice(16, 12, (2, 2))
    x = torch.zeros(3, 28, 28, device=device)
    out = torch.full((3, 40, 40), NAN, device=device)
    for oy, ox, o, over, match in ((0, 2, out, {}, "ox % 4"), (0, 0, out[:, :, :38].contiguous(), {}, "Wo % 4"),
                                   (16, 0, out, {}, "outside the output"), (0, 16, out, {}, "outside the output"),
                                   (-4, 0, out, {}, "outside the output"), (0, 0, out, dict(st=4), "more than 3 tiles per axis"),
                                   (0, 0, out, dict(S=18), "S % 4")):
        with pytest.raises(E.EngineError, match=match):
            _finalize(x, lat, o, oy, ox, **over)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())   # nothing was launched


# ------------------------------------------------------------------------------------------------ past 2^31 elements
def test_canvas_offsets_are_64_bit(device):
    """C = 3, canvas 26760^2: 2 148 292 800 elements, just over 2^31 (8.6 GB); S 24 / st 12, 2229 x 2229 slots of which
    only the first and the last hold a tile - the last one lies wholly past element 2^31 in channel 2.  kd_tiles_gather_lowres
    (Philox stream over the canvas, previous canvas 6690^2) and kd_tiles_finalize against slicing."""
    S, st, n = 24, 12, 2229
    Hc = (n - 1) * st + S
    assert Hc == 26760 and 3 * Hc * Hc > 2 ** 31 > 3 * Hc * Hc - 2 ** 20 and (2 * Hc + Hc - S) * Hc + Hc - S > 2 ** 31
    seed, sid = 99, H.engine().stream_id(16, 1)
    z = _philox((3, Hc, Hc), seed, sid, device)   # the noise of gather_lowres, then the x of finalize
    last = Hc - S
    origins = [(0, 0), (last, last)]
    # gather_lowres
    prev = torch.rand(3, 6690, 6690, generator=H.gen(1)).to(device)
    a, s = 0.9689, 0.2474
    lat = dict(S=S, Hc=Hc, Wc=Hc)
    got = _gather_lowres(prev, lat, origins, a, s, None, seed, sid)
    idx = FR.nearest_index(6690, Hc).to(device)
    for t, (y0, x0) in enumerate(origins):
        v = prev[:, idx[y0:y0 + S]][:, :, idx[x0:x0 + S]] * 2 - 1
        assert torch.equal(got[t], a * v + s * z[:, y0:y0 + S, x0:x0 + S]), t
    del prev
    # finalize
    tile_of = torch.full((n, n), -1, dtype=torch.int32, device=device)
    tile_of[0, 0], tile_of[-1, -1] = 0, 1
    out = torch.full((3, Hc, Hc), 0.25, device=device)
    _finalize(z, dict(S=S, st=st, ny=n, nx=n), out, 0, 0, tile_of=tile_of, n=2)
    changed = 0
    for y0, x0 in origins:
        want = (z[:, y0:y0 + S, x0:x0 + S].clamp(-1.0, 1.0) + 1) * 0.5
        assert torch.equal(out[:, y0:y0 + S, x0:x0 + S], want), (y0, x0)
        changed += int((want != 0.25).sum())
    assert 0 < changed <= 2 * 3 * S * S
    total = sum(int((out[c] != 0.25).sum()) for c in range(3))
    assert total == changed   # nothing outside the two tiles was written


# ------------------------------------------------------------------------------------------------ sample_tiled
CASCADE_KW = dict(image_sizes=(16, 32), timesteps=(N, N), pred_objectives=("noise", "v"), condition_on_text=False)
TOY_W, TOY_WINDOW = 44, 24


def _toy_geom():
    return _G().GridGeometry(8, 6, 7, 24, 176)


def _cascade(device, cond_channels=3, cls=R.Unet, **extra):
    unets = [H.ref_unet(cls, H.UNET_KW["small1"], seed=3, cond_images_channels=cond_channels, **extra),
             H.ref_unet(cls, H.UNET_KW["small1"], seed=6, cond_images_channels=cond_channels, lowres_cond=True, **extra)]
    oim = RS.Imagen(unets, **CASCADE_KW)
    return oim, H.product_imagen(oim, "Imagen", device, **CASCADE_KW)


_PAIRS = {}


def _pair(device, cond_channels):   # one (oracle, product) cascade per conditioning width for the module
    if cond_channels not in _PAIRS:
        _PAIRS[cond_channels] = _cascade(device, cond_channels)
    return _PAIRS[cond_channels]


@pytest.fixture(scope="module")
def cascade(device):
    return _pair(device, 3)


@pytest.fixture(scope="module")
def zoomed():
    return torch.rand(1, 3, TOY_W, TOY_W, generator=H.gen(44))


@pytest.mark.parametrize("grid,present,kw", [
    ((2, 2), None, dict(seed=5)),
    ((3, 2), HOLE, dict(seed=5, sampler="ddim", sampler_eta=0.5)),
    ((2, 2), None, dict(seed=5, sampler="dpmpp_2m", tile_batch=3)),
    ((2, 2), None, dict(sampler="dpmpp_2m", tile_weights="ramp")),   # (no seed: injected noise)
], ids=["2x2", "3x2-hole", "dpmpp_2m", "injected-noise"])
def test_streamed_does_not_change_a_bit(device, cascade, grid, present, kw):
    """Both stages, low-res conditioning and 3 conditioning channels; graph on and off."""
    pim = cascade[1]
    n = sum(map(sum, present)) if present else grid[0] * grid[1]
    kw = dict(kw, present=present, cond_images=torch.rand(n, 3, 20, 20, generator=H.gen(8)).to(device), device=device)
    if "seed" not in kw:
        kw["noise_fn"] = RS.generator_noise_fn(41)
    want = pim.sample_tiled(grid, **kw)
    assert bool(torch.isfinite(want).all()) and float(want.std()) > 0.01
    for graph in (True, False):
        outs = pim.sample_tiled(grid, streamed=True, use_graph=graph, return_all_unet_outputs=True, **kw)
        assert torch.equal(outs[-1], want), graph
    assert outs[0].shape[-2:] == tuple(((g - 1) * 12 + 16) for g in grid)


def test_streamed_self_conditioned_cascade_does_not_change_a_bit(device):
    pim = _cascade(device, cls=SC.Unet, self_cond=True)[1]
    assert all(u.self_cond for u in pim.unets)
    kw = dict(seed=9, sampler="dpmpp_2m", cond_images=torch.rand(4, 3, 20, 20, generator=H.gen(8)).to(device), device=device)
    want = pim.sample_tiled((2, 2), **kw)
    assert torch.equal(pim.sample_tiled((2, 2), streamed=True, **kw), want)
    assert torch.equal(pim.sample_tiled((2, 2), streamed=True, use_graph=False, **kw), want)


def _crops(zoomed, pos, v2=False, fill=0.95):
    import imagen_pytorch as ip

    geom = _toy_geom()
    return ip.TileCondCrops(zoomed, FR.shifts_of(TOY_W, geom, pos), TOY_WINDOW, fill, centre_width=geom.patch_width if v2 else None)


def _materialised(zoomed, pos, v2=False, fill=0.95):
    G = _G()
    with FR.window_of(G, TOY_WINDOW):
        return G.cond_images_for_grid(zoomed, _toy_geom(), pos, fill_color=fill, centre_crop_channels=v2)


def test_cond_crops_are_the_materialised_cond_images(device, cascade, zoomed):
    """One seed; the 24-pixel windows are seen at 16 (stage 1) and 32 (stage 2); the shift-0 row of the toy lattice is in."""
    pim = cascade[1]
    pos = [(2, 3), (2, 4), (3, 3), (3, 4)]
    kw = dict(seed=11, sampler="dpmpp_2m", tile_batch=3, device=device)
    want = pim.sample_tiled((2, 2), cond_images=_materialised(zoomed, pos).to(device), **kw)
    assert torch.equal(pim.sample_tiled((2, 2), cond_crops=_crops(zoomed, pos), **kw), want)
    assert torch.equal(pim.sample_tiled((2, 2), cond_crops=_crops(zoomed.to(device), pos), streamed=True, **kw), want)
    other = pim.sample_tiled((2, 2), cond_crops=_crops(zoomed, [(p[0], p[1] - 1) for p in pos]), **kw)
    assert not torch.equal(other, want)   # the conditioning is read


def test_into_writes_the_covered_pixels_in_place(device, cascade):
    pim = cascade[1]
    kw = dict(present=HOLE, seed=5, sampler="ddim", cond_images=torch.rand(5, 3, 20, 20, generator=H.gen(8)).to(device), device=device)
    want = pim.sample_tiled((3, 2), **kw)
    assert want.shape == (1, 3, 80, 56)
    covered = FR.finish(want[0], _lattice(32, 24, (3, 2), HOLE)["origins"], 32)[1]
    assert not bool(covered.all())
    before = torch.rand(1, 3, 100, 72, generator=H.gen(2)).to(device)
    canvas = before.clone()
    got = pim.sample_tiled((3, 2), streamed=True, into=(canvas, 8, 12), **kw)
    assert got is canvas
    expect = before.clone()
    expect[0, :, 8:88, 12:68] = torch.where(covered, want[0], before[0, :, 8:88, 12:68])
    assert torch.equal(canvas, expect)
    # a call that stops at stage 1 writes stage 1's canvas
    small = torch.zeros(1, 3, 40, 28, device=device)
    pim.sample_tiled((3, 2), streamed=True, into=(small, 0, 0), stop_at_unet_number=1, **kw)
    assert torch.equal(small, pim.sample_tiled((3, 2), stop_at_unet_number=1, **kw))


# ------------------------------------------------------------------------------------------------ fused_level
BLOCK = [(i, j) for i in (2, 3, 4) for j in (2, 3, 4)]
SPARSE = [(2, 3), (2, 4), (3, 3)]


def _covered_full(pos, S=32, st=24, width=176):
    c = torch.zeros(width, width, dtype=torch.bool)
    for i, j in pos:
        c[i * st:i * st + S, j * st:j * st + S] = True
    return c


@pytest.mark.parametrize("pos", [BLOCK, SPARSE], ids=["3x3", "sparse"])
@pytest.mark.parametrize("v2", [False, True], ids=["ultra", "v2"])
def test_fused_level_is_the_call_made_by_hand_over_the_enlarged_background(device, zoomed, pos, v2):
    from ultra_res import tiled as UT

    pim = _pair(device, 6 if v2 else 3)[1]
    kw = dict(overlap=0.25, tile_batch=4, sampler="dpmpp_2m", seed=21)
    got = UT.fused_level(lambda stage: pim, zoomed, _toy_geom(), pos, version="v2" if v2 else "ultra", window=TOY_WINDOW,
                         stages=(1, 2), device=device, **kw)
    assert got.is_cuda and got.shape == (1, 3, 176, 176)
    r0, c0, grid, present, tiles = UT.level_box(pos)
    hand = pim.sample_tiled(grid, present=present, cond_crops=_crops(zoomed, tiles, v2), streamed=True, device=device, **kw)
    covered = _covered_full(pos).to(device)
    box = (slice(None), slice(None), slice(r0 * 24, r0 * 24 + hand.shape[2]), slice(c0 * 24, c0 * 24 + hand.shape[3]))
    assert bool(covered[box[2:]].all()) == (pos is BLOCK)   # the sparse set leaves part of its box bare
    assert torch.equal(got[box][:, :, covered[box[2:]]], hand[:, :, covered[box[2:]]])
    back = F.interpolate(zoomed.to(device), 176, mode="bilinear", align_corners=False)
    assert torch.equal(got[:, :, ~covered], back[:, :, ~covered])
    # the materialised conditioning images give the same canvas
    mat = pim.sample_tiled(grid, present=present, cond_images=_materialised(zoomed, tiles, v2).to(device), device=device, **kw)
    assert torch.equal(mat, hand)
    # background=False: the same tiles over zeros
    bare = UT.fused_level(lambda stage: pim, zoomed, _toy_geom(), pos, version="v2" if v2 else "ultra", window=TOY_WINDOW,
                          stages=(1, 2), device=device, background=False, **kw)
    assert torch.equal(bare, torch.where(covered, got, torch.zeros_like(got)))


@pytest.mark.parametrize("pos", [BLOCK, SPARSE], ids=["3x3", "sparse"])
@pytest.mark.parametrize("v2", [False, True], ids=["ultra", "v2"])
def test_fused_level_matches_the_restatement_over_the_oracle(device, zoomed, pos, v2):
    """The whole canvas against tests/tiled_ref.sample_tiled over the oracle, given cond_images_for_grid's images and the same
    injected noise, composited in torch over the bilinear background: the project's sampler bound."""
    from ultra_res import tiled as UT

    oim, pim = _pair(device, 6 if v2 else 3)
    nf = RS.generator_noise_fn(41)
    got = UT.fused_level(lambda stage: pim, zoomed, _toy_geom(), pos, version="v2" if v2 else "ultra", window=TOY_WINDOW,
                         stages=(1, 2), sampler="dpmpp_2m", noise_fn=nf, device=device).cpu()
    r0, c0, grid, present, tiles = UT.level_box(pos)
    ref = TR.sample_tiled(oim, grid=grid, present=present, noise_fn=nf, sampler="dpmpp_2m", cond_images=_materialised(zoomed, tiles, v2))
    want = F.interpolate(zoomed, 176, mode="bilinear", align_corners=False)
    covered = _covered_full(pos)
    ys, xs = slice(r0 * 24, r0 * 24 + ref.shape[2]), slice(c0 * 24, c0 * 24 + ref.shape[3])
    want[:, :, ys, xs] = torch.where(covered[ys, xs], ref, want[:, :, ys, xs])
    err = float((got - want).abs().max())
    print(f"fused_level {'v2' if v2 else 'ultra'} {len(pos)} tiles vs the restatement over the oracle: max|diff| {err:.2e}")
    assert float(got[:, :, covered].std()) > 0.01 and err < SAMPLE_ABS


def test_mag2_level_at_the_pipelines_sizes(device):
    """generate_high_res_image_fused at mag 2 on the dim-32 models and the tissue canvas of tests/test_drivers_gpu.py, one
    step per stage: 53 x 53 candidates, the tissue set in its box, the 40960^2 canvas (20 GB) on the device."""
    import test_drivers_gpu as TD
    from ultra_res import pipeline as P
    from ultra_res import tiled as UT

    zoomed = TD._mag1_canvas_with_tissue()
    zoomed_d = zoomed.to(device)
    pim = TD._pair(device, 3, (1, 1, 1), seed=400)[1]
    geom, pos = P.level_patches(zoomed_d, 2, 0.25)
    assert (geom.patch_width, geom.patch_dist, geom.num_patches_width, geom.canvas_width) == (161, 120, 53, 40960)
    r0, c0, grid, present, tiles = UT.level_box(pos)
    assert 4 <= len(tiles) < grid[0] * grid[1] and r0 * 768 >= 18000   # a sparse box, below the rows sampled at the end
    canvas = P.generate_high_res_image_fused(lambda stage: pim, zoomed_d, 2, overlap=0.25, seed=3, tile_batch=4, device=device)
    assert canvas.is_cuda and tuple(canvas.shape) == (1, 3, 40960, 40960)
    for i, j in tiles:
        t = canvas[0, :, i * 768:i * 768 + 1024, j * 768:j * 768 + 1024]
        assert bool(torch.isfinite(t).all()) and float(t.min()) >= 0.0 and float(t.max()) <= 1.0 and float(t.std()) > 0.0, (i, j)
    # the background: the mag-1 canvas enlarged bilinearly (align_corners False), checked at random points in fp64
    gen = torch.Generator().manual_seed(5)
    ys = torch.randint(0, 18000, (2000,), generator=gen)
    xs = torch.randint(0, 40960, (2000,), generator=gen)
    z = zoomed[0].double()

    def tap(d):
        s = ((d.double() + 0.5) * (6400 / 40960) - 0.5).clamp(min=0)
        i0 = s.floor().long().clamp(max=6399)
        return i0, (i0 + 1).clamp(max=6399), s - i0

    y0, y1, ly = tap(ys)
    x0, x1, lx = tap(xs)
    want = (1 - ly) * ((1 - lx) * z[:, y0, x0] + lx * z[:, y0, x1]) + ly * ((1 - lx) * z[:, y1, x0] + lx * z[:, y1, x1])
    have = canvas[0][:, ys.to(device), xs.to(device)].cpu().double()
    assert float((have - want).abs().max()) < 2e-4   # fp32 source coordinates at 40960 px, as torch computes them
    del canvas
