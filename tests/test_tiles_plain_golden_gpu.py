"""The plain fused-tile canvas step and finish pinned to bits recorded before the plain and the known kernels became one
template each (tests/golden/tiles_plain_kernels.pt, written by tests/golden/make_tiles_plain_kernels.py on the MI355X at
the commit before the fold): kd_tiles_fuse_update and kd_tiles_finalize themselves, and the general entries
kd_tiles_fuse_update_known / kd_tiles_finalize_known with nothing known, which must give the same bits.

The golden holds outputs only; the inputs are rebuilt here from helpers.gen seeds.  Lattices of the unit tests in
tests/test_tiled_gpu.py (C = 3, canvases at most 40 x 28): one, two and three tiles cover a pixel per axis, and the 3 x 2
lattice with a hole leaves pixels uncovered, which must keep their bits in x and in x0bar.  The golden file has to stay
below the 115 KB of tests/golden/tiled_seed5_2x2.pt and a canvas pair is about 20 KB, so four canvas steps are pinned, not
the cross product: every (S, st), both grids, every pair of (uniform | ramp) x (thresholds | none), each of the three
coefficient sets and both kinds of draw occur once; the 2 x 2 grid of (16, 12) and (20, 8) is left out.  The finish is
pinned on both grids of (16, 12); its covered values do not depend on the offset, so one window per grid serves the
offsets (0, 0) and (8, 12), and every other element of the 72 x 76 canvas is held to the canvas' own bits from before."""
import ctypes as C
import pathlib

import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).parent / "golden" / "tiles_plain_kernels.pt"
HOLE = [[True, True], [True, False], [True, True]]
NAN = float("nan")
CN = 3
SEED = 77

# name: S, st, grid, present, ramp, thresholds, (A, B, P, Sn), NaN history, draw ("injected" | "philox" | "unread")
FUSE = {
    "S20_st8_hole_ramp_thr_2M_injected": (20, 8, (3, 2), HOLE, 1, True, (0.83, 0.21, -0.07, 0.4), False, "injected"),
    "S16_st8_hole_uniform_P0_nan_history_philox": (16, 8, (3, 2), HOLE, 0, False, (0.83, 0.21, 0.0, 0.4), True, "philox"),
    "S16_st12_hole_ramp_Sn0": (16, 12, (3, 2), HOLE, 1, False, (0.83, 0.21, -0.07, 0.0), False, "unread"),
    "S16_st8_full_uniform_thr_P0_nan_history_injected": (16, 8, (2, 2), None, 0, True, (0.83, 0.21, 0.0, 0.4), True, "injected"),
}
FINALIZE = {"S16_st12_full": ((2, 2), None), "S16_st12_hole": ((3, 2), HOLE)}
OFFSETS = [(0, 0), (8, 12)]
OUT_HW = (72, 76)


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


def _covered(lat, device):
    cov = torch.zeros(lat["Hc"], lat["Wc"], dtype=torch.bool)
    for y0, x0 in lat["origins"]:
        cov[y0:y0 + lat["S"], x0:x0 + lat["S"]] = True
    return cov.to(device)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tile_of(lat, device):
    return torch.tensor(lat["tile_of"], dtype=torch.int32, device=device)


# ------------------------------------------------------------------------------------------------ the entries
def fuse_plain(x, hist, out, tiles, thr, lat, ramp, A, B, P, Sn, noise, seed, sid):
    assert out is hist   # kd_tiles_fuse_update has one buffer for the history and the estimate
    E = H.engine()
    tile_of = _tile_of(lat, x.device)
    E.check(E.load().kd_tiles_fuse_update(E.ptr(x), E.ptr(hist), E.ptr(tiles), E.ptr(thr), C.c_void_p(tile_of.data_ptr()),
                                          tiles.shape[0], CN, lat["S"], lat["st"], lat["ny"], lat["nx"], ramp, A, B, P, Sn,
                                          E.ptr(noise), seed, sid, E.current_stream()))


def fuse_general(x, hist, out, tiles, thr, lat, ramp, A, B, P, Sn, noise, seed, sid):
    E = H.engine()
    tile_of = _tile_of(lat, x.device)
    E.check(E.load().kd_tiles_fuse_update_known(
        E.ptr(x), E.ptr(hist), E.ptr(out), E.ptr(tiles), E.ptr(thr), C.c_void_p(tile_of.data_ptr()), tiles.shape[0], CN, lat["S"],
        lat["st"], lat["ny"], lat["nx"], ramp, A, B, P, Sn, E.ptr(noise), seed, sid, 0, 0.0, 0.0, None, 0, None, None, 0.0, 0.0, None, 0,
        E.current_stream()))


def finalize_plain(x, lat, out, oy, ox):
    E = H.engine()
    tile_of = _tile_of(lat, x.device)
    E.check(E.load().kd_tiles_finalize(E.ptr(x), C.c_void_p(tile_of.data_ptr()), len(lat["origins"]), CN, lat["S"], lat["st"],
                                       lat["ny"], lat["nx"], E.ptr(out), out.shape[1], out.shape[2], oy, ox, E.current_stream()))


def finalize_general(x, lat, out, oy, ox):
    E = H.engine()
    tile_of = _tile_of(lat, x.device)
    E.check(E.load().kd_tiles_finalize_known(E.ptr(x), C.c_void_p(tile_of.data_ptr()), len(lat["origins"]), CN, lat["S"], lat["st"],
                                             lat["ny"], lat["nx"], E.ptr(out), out.shape[1], out.shape[2], oy, ox, None, None,
                                             E.current_stream()))


# ------------------------------------------------------------------------------------------------ inputs and runs
def fuse_inputs(name, device):
    S, st, grid, present, ramp, with_thr, coef, nan_hist, draw = FUSE[name]
    lat = _lattice(S, st, grid, present)
    n, Hc, Wc = len(lat["origins"]), lat["Hc"], lat["Wc"]
    g = H.gen(1000 + S + st + n)
    x = torch.randn(CN, Hc, Wc, generator=g) * 1.5
    hist = torch.rand(CN, Hc, Wc, generator=g) * 2 - 1
    tiles = torch.randn(n, CN, S, S, generator=g) * 1.5
    thr = torch.rand(n, generator=g) * 2 + 1
    z = torch.randn(CN, Hc, Wc, generator=g)
    if nan_hist:
        hist = torch.full_like(hist, NAN)
    noise = dict(injected=z, philox=None, unread=torch.full_like(z, NAN))[draw]
    dv = lambda t: None if t is None else t.to(device)
    return dict(lat=lat, x=dv(x), hist=dv(hist), tiles=dv(tiles), thr=dv(thr) if with_thr else None, ramp=ramp, coef=coef,
                noise=dv(noise), sid=H.engine().stream_id(1, 9))


def run_fuse(entry, name, device, aliased=True):
    """(x, estimate buffer, history buffer) after one canvas step; apart: the estimate goes to a buffer filled with 0.125."""
    i = fuse_inputs(name, device)
    x, hist = i["x"].clone(), i["hist"].clone()
    out = hist if aliased else torch.full_like(hist, 0.125)
    entry(x, hist, out, i["tiles"], i["thr"], i["lat"], i["ramp"], *i["coef"], i["noise"], SEED, i["sid"])
    return x, out, hist


def finalize_inputs(name, device):
    grid, present = FINALIZE[name]
    lat = _lattice(16, 12, grid, present)
    g = H.gen(2000 + lat["Hc"])
    x = (torch.randn(CN, lat["Hc"], lat["Wc"], generator=g) * 1.5).to(device)
    before = torch.rand(CN, *OUT_HW, generator=g).to(device)
    return lat, x, before


def run_finalize(entry, name, oy, ox, device):
    """(the canvas after the finish, the canvas before, the window written, the covered pixels of the window)"""
    lat, x, before = finalize_inputs(name, device)
    out = before.clone()
    entry(x, lat, out, oy, ox)
    win = (slice(None), slice(oy, oy + lat["Hc"]), slice(ox, ox + lat["Wc"]))
    return out, before, win, _covered(lat, device)


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


# ------------------------------------------------------------------------------------------------ the tests
def test_plain_step_and_finish_keep_the_recorded_bits(device, golden):
    for name in FUSE:
        x, xb, _ = run_fuse(fuse_plain, name, device)
        assert torch.equal(_bits(x), _bits(golden[f"fuse/{name}/x"].to(device))), name
        assert torch.equal(_bits(xb), _bits(golden[f"fuse/{name}/x0bar"].to(device))), name
    for name in FINALIZE:
        for oy, ox in OFFSETS:
            out, before, win, cov = run_finalize(finalize_plain, name, oy, ox, device)
            want = before.clone()
            want[win] = torch.where(cov, golden[f"finalize/{name}"].to(device), before[win])
            assert torch.equal(_bits(out), _bits(want)), (name, oy, ox)


def test_general_entries_with_nothing_known_give_the_plain_bits(device, golden):
    """kd_tiles_fuse_update_known without re-noise and mix, history and estimate one buffer and apart (the history is then
    only read and the uncovered pixels of the estimate keep the buffer's bits), and kd_tiles_finalize_known(NULL, NULL)."""
    for name in FUSE:
        gx, gxb = golden[f"fuse/{name}/x"].to(device), golden[f"fuse/{name}/x0bar"].to(device)
        cov = _covered(fuse_inputs(name, device)["lat"], device)
        x, xb, _ = run_fuse(fuse_general, name, device, aliased=True)
        assert torch.equal(_bits(x), _bits(gx)) and torch.equal(_bits(xb), _bits(gxb)), name
        x, xb, hist = run_fuse(fuse_general, name, device, aliased=False)
        assert torch.equal(_bits(x), _bits(gx)), name
        assert torch.equal(_bits(xb), _bits(torch.where(cov, gxb, torch.full_like(gxb, 0.125)))), name
        assert torch.equal(_bits(hist), _bits(fuse_inputs(name, device)["hist"])), name
    for name in FINALIZE:
        for oy, ox in OFFSETS:
            out, before, win, cov = run_finalize(finalize_general, name, oy, ox, device)
            want = before.clone()
            want[win] = torch.where(cov, golden[f"finalize/{name}"].to(device), before[win])
            assert torch.equal(_bits(out), _bits(want)), (name, oy, ox)
