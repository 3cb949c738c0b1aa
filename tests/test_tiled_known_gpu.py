"""Fused-tile canvases that keep known pixels or start from an image, on the MI355X: kd_tiles_start, kd_tiles_fuse_update_known
and kd_tiles_finalize_known bit for bit against what they fuse (the Philox draw, kd_tiles_fuse_update, kd_tiles_finalize and the
torch expressions behind them), their addressing past 2^31 canvas elements and their refusals; Imagen.sample_tiled(known_image=,
known_mask=, known_resample_times=, init_canvas=, init_skip_steps=) against the restatement tests/tiled_known_ref.py on the
16 -> 32 cascade of tests/test_tiled_gpu.py and bit for bit against sample() on a 1 x 1 lattice; ultra_res.tiled.fused_level(
canvas=, keep=, refine_skip_steps=) on the 7 x 7 toy level of tests/test_fused_level_gpu.py."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import fused_level_ref as FR
import helpers as H
import self_cond_ref as SC
import tiled_known_ref as KR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

REL = 1e-6           # the solver-step bound (tests/test_tiled_gpu.py)
SAMPLE_ABS = 2e-3    # the project's sampler bound against the oracle on identical noise
N = 8
HOLE = [[True, True], [True, False], [True, True]]
NAN = float("nan")


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


def _iptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _philox(shape, seed, sid, device):
    E = H.engine()
    out = torch.empty(shape, device=device)
    E.check(E.load().kd_philox_normal(E.ptr(out), out.numel(), seed, sid, E.current_stream()))
    return out


def _near(t, size):
    """[C, H, W] or [H, W] -> the canvas' size by torch's nearest rule (a source of that size as it is)."""
    if tuple(t.shape[-2:]) == tuple(size):
        return t
    lead = (None,) * (4 - t.dim())
    return F.interpolate(t[lead].float(), tuple(size), mode="nearest").reshape(t.shape[:-2] + tuple(size)).to(t.dtype)


def _mix(x, kn, m, a, s, zm):
    """x = m ? a (2 kn - 1) + s z : x in torch ops, one rounding each (s == 0: the term left out)."""
    v = a * (2 * kn - 1)
    if s != 0:
        v = v + s * zm
    return torch.where(m, v, x)


# ------------------------------------------------------------------------------------------------ kd_tiles_start
def _start(shape, scale=1.0, noise=None, seed=0, init=None, known=None, mask=None, a=0.0, s=0.0, mix_noise=None, mix_sid=0,
           out=None):
    E = H.engine()
    Cn, Hc, Wc = shape
    x = torch.full(shape, NAN, device="cuda:0") if out is None else out
    im, kn, mk = E.tiles_image(init), E.tiles_image(known), E.tiles_mask(mask)
    E.check(E.load().kd_tiles_start(E.ptr(x), Cn, Hc, Wc, scale, E.ptr(noise), seed, E.ref(im), E.ref(kn), E.ref(mk), a, s,
                                    E.ptr(mix_noise), mix_sid, E.current_stream()))
    return x


@pytest.mark.parametrize("shape", [(3, 28, 28), (1, 28, 40), (4, 16, 16)])
def test_start_without_image_and_mask_is_the_philox_draw(device, shape):
    E = H.engine()
    assert torch.equal(_start(shape, seed=0xABCDEF), _philox(shape, 0xABCDEF, E.stream_id(16, 2), device))


def _src_mask(h, w, g):
    """Known where a smooth pattern says so, plus whole and partial float4s: columns [0, 10) of the upper half."""
    m = torch.rand(h, w, generator=g) > 0.6
    m[: h // 2, : (10 * w) // 28] = True
    m[h // 2:, (16 * w) // 28:(24 * w) // 28] = False
    return m


@pytest.mark.parametrize("Cn", [1, 3, 4])
@pytest.mark.parametrize("canvas", [(28, 28), (28, 40)])
@pytest.mark.parametrize("src", ["same", (56, 56), (50, 44), "window"])
def test_start_is_the_torch_expression(device, Cn, canvas, src):
    """scale z + (2 nearest(init) - 1), then where(m, a (2 nearest(kn) - 1) + s z', .): sources of the canvas' size (the
    16-byte / 4-byte path), 56^2 and 50 x 44 (scalar gathers) and an unaligned window of a larger tensor (strided: no copy);
    injected and Philox noise; the init image alone, the mask alone, both."""
    E = H.engine()
    g = H.gen(Cn * 100 + canvas[1] + (0 if isinstance(src, str) else src[0]))
    Hc, Wc = canvas
    shape = (Cn, Hc, Wc)
    hw = canvas if isinstance(src, str) else src
    if src == "window":   # a window at an odd offset inside a larger tensor
        big_i, big_k = torch.rand(Cn, Hc + 9, Wc + 14, generator=g).to(device), torch.rand(Cn, Hc + 9, Wc + 14, generator=g).to(device)
        big_m = _src_mask(Hc + 9, Wc + 14, g).to(device)
        init, kn, m = big_i[:, 5:5 + Hc, 3:3 + Wc], big_k[:, 4:4 + Hc, 7:7 + Wc], big_m[6:6 + Hc, 5:5 + Wc]
        assert not init.is_contiguous() and not m.is_contiguous()
    else:
        init, kn = torch.rand(Cn, *hw, generator=g).to(device), torch.rand(Cn, *hw, generator=g).to(device)
        m = _src_mask(*hw, g).to(device)
    a, s, scale, seed, sid = 0.81, 0.58, 1.25, 4242, E.stream_id(2, 6)
    z_in, zm_in = torch.randn(shape, generator=g).to(device), torch.randn(shape, generator=g).to(device)
    init_r, kn_r, m_r = _near(init, canvas), _near(kn, canvas), _near(m, canvas)
    assert 0.2 < float(m_r.float().mean()) < 0.8
    for injected in (True, False):
        z = z_in if injected else _philox(shape, seed, E.stream_id(16, 2), device)
        zm = zm_in if injected else _philox(shape, seed, sid, device)
        noise, mix_noise = (z_in, zm_in) if injected else (None, None)
        plain = scale * z
        with_init = plain + (2 * init_r - 1)
        kw = dict(scale=scale, noise=noise, seed=seed)
        assert torch.equal(_start(shape, init=init, **kw), with_init)
        got = _start(shape, known=kn, mask=m, a=a, s=s, mix_noise=mix_noise, mix_sid=sid, **kw)
        assert torch.equal(got, _mix(plain, kn_r, m_r, a, s, zm))
        got = _start(shape, init=init, known=kn, mask=m, a=a, s=s, mix_noise=mix_noise, mix_sid=sid, **kw)
        assert torch.equal(got, _mix(with_init, kn_r, m_r, a, s, zm))
    # s == 0 leaves the mix noise unread; a uint8 mask with values other than 1 counts as set
    got = _start(shape, noise=z_in, known=kn, mask=m.to(torch.uint8) * 7, a=a, s=0.0, mix_noise=torch.full(shape, NAN, device=device))
    assert torch.equal(got, _mix(1.0 * z_in, kn_r, m_r, a, 0.0, None))


# ------------------------------------------------------------------------------------------------ kd_tiles_fuse_update_known
def _fuse(x, x0bar, tiles, thr, lat, ramp, A, B, P, Sn, noise=None, seed=0, sid=0):
    E = H.engine()
    tile_of = torch.tensor(lat["tile_of"], dtype=torch.int32, device=x.device)
    E.check(E.load().kd_tiles_fuse_update(E.ptr(x), E.ptr(x0bar), E.ptr(tiles), E.ptr(thr), _iptr(tile_of), tiles.shape[0],
                                          tiles.shape[1], lat["S"], lat["st"], lat["ny"], lat["nx"], int(ramp), A, B, P, Sn,
                                          E.ptr(noise), seed, sid, E.current_stream()))


def _fuse_known(x, hist, out, tiles, thr, lat, ramp, A, B, P, Sn, noise=None, seed=0, sid=0, renoise=0, rn_a=0.0, rn_b=0.0,
                rn_noise=None, rn_sid=0, known=None, mask=None, a=0.0, s=0.0, mix_noise=None, mix_sid=0, tile_of=None, n=None,
                **over):
    E = H.engine()
    g = dict(lat, **over)
    tile_of = torch.tensor(lat["tile_of"], dtype=torch.int32, device=x.device) if tile_of is None else tile_of
    kn, mk = E.tiles_image(known), E.tiles_mask(mask)
    E.check(E.load().kd_tiles_fuse_update_known(
        E.ptr(x), E.ptr(hist), E.ptr(out), E.ptr(tiles), E.ptr(thr), _iptr(tile_of), tiles.shape[0] if n is None else n,
        tiles.shape[1], g["S"], g["st"], g["ny"], g["nx"], int(ramp), A, B, P, Sn, E.ptr(noise), seed, sid, int(renoise), rn_a, rn_b,
        E.ptr(rn_noise), rn_sid, E.ref(kn), E.ref(mk), a, s, E.ptr(mix_noise), mix_sid, E.current_stream()))


def _fuse_fp64(x, hist, tiles, thr, lat, ramp, A, B, P, Sn, z):
    """(x_next, x0bar, covered) of the canvas step in fp64 over the fp32 inputs and weights (tests/test_tiled_gpu.py)."""
    S = lat["S"]
    w = KR.TR.weight(S, lat["st"], "ramp" if ramp else "uniform").double()
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


def _canvas_mask(Hc, Wc, g):
    """Whole known float4s (columns [0, 8)), a partial one (columns [8, 10)), whole unknown ones, and scattered pixels."""
    m = torch.rand(Hc, Wc, generator=g) > 0.7
    m[:, :10] = True
    m[:, 12:20] = False
    m[Hc // 2:Hc // 2 + 3, :] = True
    return m


@pytest.mark.parametrize("grid,present", [((2, 2), None), ((3, 3), None), ((3, 2), HOLE)])
@pytest.mark.parametrize("S,st", [(16, 12), (16, 8), (20, 8)])
def test_fuse_update_known_is_the_three_passes(device, S, st, grid, present):
    """Uniform and ramp weights, thresholds and none, hist and out aliased and apart.  Without mask and re-noise: the bits
    of kd_tiles_fuse_update.  With them: kd_tiles_fuse_update, then x rn_a + z rn_b, then the mix, in torch ops - bit for
    bit - and rel-L2 1e-6 of the fp64 expression; P = 0 over a NaN history, mix s = 0 over NaN mix noise, Philox and
    injected draws; the pixels no tile covers keep their bits in every buffer."""
    E = H.engine()
    lat = _lattice(S, st, grid, present)
    Cn, n, Hc, Wc = 3, len(lat["origins"]), lat["Hc"], lat["Wc"]
    g = H.gen(S + st + n)
    dv = lambda t: None if t is None else t.to(device)
    x_in = torch.randn(Cn, Hc, Wc, generator=g) * 1.5
    hist_in = torch.rand(Cn, Hc, Wc, generator=g) * 2 - 1
    tiles = torch.randn(n, Cn, S, S, generator=g) * 1.5
    z, zr, zm = (torch.randn(Cn, Hc, Wc, generator=g) for _ in range(3))
    kn = torch.rand(Cn, Hc, Wc, generator=g)
    m = _canvas_mask(Hc, Wc, g)
    nan = torch.full_like(x_in, NAN)
    seed, sid, rn_sid, mix_sid = 77, E.stream_id(1, 9), E.stream_id(3, 9), E.stream_id(2, 10)
    rn_a, rn_b, a, s = 1.07, 0.31, 0.66, 0.75
    worst = 0.0
    for ramp in (0, 1):
        for thr in (torch.rand(n, generator=g) * 2 + 1, None):
            for A, B, P, Sn, hist in ((0.83, 0.21, -0.07, 0.4, hist_in), (0.83, 0.21, 0.0, 0.4, nan), (0.83, 0.21, -0.07, 0.0, hist_in)):
                base_x, base_xb = dv(x_in), dv(hist)
                _fuse(base_x, base_xb, dv(tiles), dv(thr), lat, ramp, A, B, P, Sn, dv(z))
                _, _, covered = _fuse_fp64(x_in, hist, tiles, thr, lat, ramp, A, B, P, Sn, z)
                cov = covered.to(device)
                for aliased in (True, False):
                    def run(**kw):
                        x, h = dv(x_in), dv(hist)
                        out = h if aliased else torch.full_like(h, 0.125)
                        untouched = dv(hist) if aliased else torch.full_like(h, 0.125)
                        _fuse_known(x, h, out, dv(tiles), dv(thr), lat, ramp, A, B, P, Sn, dv(z), **kw)
                        assert torch.equal(out[:, ~cov].view(torch.int32), untouched[:, ~cov].view(torch.int32))
                        if not aliased:   # the history is read, never written
                            assert torch.equal(h.view(torch.int32), dv(hist).view(torch.int32))
                        assert torch.equal(out[:, cov], base_xb[:, cov])
                        return x

                    # nothing known, no re-noise: kd_tiles_fuse_update's bits
                    assert torch.equal(run(), base_x)
                    # re-noise and mix, injected
                    want = torch.where(cov, _mix(base_x * rn_a + dv(zr) * rn_b, dv(kn), dv(m), a, s, dv(zm)), base_x)
                    got = run(renoise=1, rn_a=rn_a, rn_b=rn_b, rn_noise=dv(zr), known=dv(kn), mask=dv(m), a=a, s=s, mix_noise=dv(zm))
                    assert torch.equal(got, want), (ramp, thr is None, P, Sn, aliased)
                    # the mix alone, s = 0 over NaN mix noise
                    want0 = torch.where(cov, _mix(base_x, dv(kn), dv(m), a, 0.0, None), base_x)
                    assert torch.equal(run(known=dv(kn), mask=dv(m), a=a, s=0.0, mix_noise=dv(nan)), want0)
                # against fp64 (injected draws)
                fx, _, _ = _fuse_fp64(x_in, hist, tiles, thr, lat, ramp, A, B, P, Sn, z)
                f64 = fx * rn_a + zr.double() * rn_b
                f64 = torch.where(m & covered, a * (2 * kn.double() - 1) + s * zm.double(), torch.where(covered, f64, x_in.double()))
                e = H.rel_l2(want[:, cov].cpu(), f64[:, covered])
                worst = max(worst, e)
                assert e <= REL, (ramp, thr is None, P, Sn, e)
    # the draws of the three streams, on the device
    A, B, P, Sn = 0.83, 0.21, -0.07, 0.4
    base_x, base_xb = dv(x_in), dv(hist_in)
    _fuse(base_x, base_xb, dv(tiles), None, lat, 1, A, B, P, Sn, None, seed, sid)
    cov = covered.to(device)
    want = base_x * rn_a + _philox((Cn, Hc, Wc), seed, rn_sid, device) * rn_b
    want = torch.where(cov, _mix(want, dv(kn), dv(m), a, s, _philox((Cn, Hc, Wc), seed, mix_sid, device)), base_x)
    x, h = dv(x_in), dv(hist_in)
    _fuse_known(x, h, h, dv(tiles), None, lat, 1, A, B, P, Sn, None, seed, sid, 1, rn_a, rn_b, None, rn_sid, dv(kn), dv(m), a, s, None, mix_sid)
    assert torch.equal(x, want) and torch.equal(h, base_xb)
    assert torch.equal(x[:, ~cov], dv(x_in)[:, ~cov])
    print(f"fuse update known S{S} st{st} {grid} {'hole' if present else 'full'}: worst rel-L2 {worst:.2e}")


def test_fuse_update_known_reads_resized_and_strided_sources(device):
    """The known image and the mask at 56^2 and as an unaligned window, seen at a 28^2 canvas."""
    lat = _lattice(16, 12, (2, 2))
    g = H.gen(3)
    x_in, tiles = torch.randn(3, 28, 28, generator=g).to(device), torch.randn(4, 3, 16, 16, generator=g).to(device)
    zm = torch.randn(3, 28, 28, generator=g).to(device)
    big, bigm = torch.rand(3, 61, 70, generator=g).to(device), _canvas_mask(61, 70, g).to(device)
    base_x, base_xb = x_in.clone(), torch.zeros_like(x_in)
    _fuse(base_x, base_xb, tiles, None, lat, 0, 0.9, 0.1, 0.0, 0.0)
    for kn, m in ((big[:, 2:58, 5:61], bigm[2:58, 5:61]), (big[:, 3:31, 9:37], bigm[3:31, 9:37])):
        x, xb = x_in.clone(), torch.zeros_like(x_in)
        _fuse_known(x, xb, xb, tiles, None, lat, 0, 0.9, 0.1, 0.0, 0.0, known=kn, mask=m, a=0.5, s=0.5, mix_noise=zm)
        assert torch.equal(x, _mix(base_x, _near(kn, (28, 28)), _near(m, (28, 28)), 0.5, 0.5, zm)) and torch.equal(xb, base_xb)


# ------------------------------------------------------------------------------------------------ kd_tiles_finalize_known
def _finalize_known(x, lat, out, oy, ox, known, mask, tile_of=None, n=None, **over):
    E = H.engine()
    g = dict(lat, **over)
    tile_of = torch.tensor(lat["tile_of"], dtype=torch.int32, device=x.device) if tile_of is None else tile_of
    kn, mk = E.tiles_image(known), E.tiles_mask(mask)
    E.check(E.load().kd_tiles_finalize_known(E.ptr(x), _iptr(tile_of), len(lat["origins"]) if n is None else n, x.shape[0], g["S"],
                                             g["st"], g["ny"], g["nx"], E.ptr(out), out.shape[1], out.shape[2], oy, ox, E.ref(kn),
                                             E.ref(mk), E.current_stream()))
    return out


@pytest.mark.parametrize("grid,present", [((2, 2), None), ((3, 2), HOLE)])
@pytest.mark.parametrize("oy,ox", [(0, 0), (8, 12)])
def test_finalize_known_is_the_torch_paste_in_place(device, grid, present, oy, ox):
    """The known source is the window of the canvas that is written; then a source of another size and place."""
    lat = _lattice(16, 12, grid, present)
    Hc, Wc = lat["Hc"], lat["Wc"]
    g = H.gen(Hc + oy)
    x = (torch.randn(3, Hc, Wc, generator=g) * 1.5).to(device)
    fin, covered = FR.finish(x, lat["origins"], 16)
    m = _canvas_mask(Hc, Wc, g).to(device)
    before = torch.rand(3, Hc + 16, Wc + 20, generator=g).to(device)
    win = (slice(None), slice(oy, oy + Hc), slice(ox, ox + Wc))
    want = before.clone()
    want[win] = torch.where(covered, torch.where(m, before[win], fin), before[win])
    canvas = before.clone()
    got = _finalize_known(x, lat, canvas, oy, ox, canvas[win], m)
    assert torch.equal(got, want) and bool((got[win][:, m & covered] == before[win][:, m & covered]).all())
    other, om = torch.rand(3, 50, 44, generator=g).to(device), _canvas_mask(50, 44, g).to(device)
    want = before.clone()
    want[win] = torch.where(covered, torch.where(_near(om, (Hc, Wc)), _near(other, (Hc, Wc)), fin), before[win])
    assert torch.equal(_finalize_known(x, lat, before.clone(), oy, ox, other, om), want)


# ------------------------------------------------------------------------------------------------ past 2^31 elements
def test_canvas_offsets_of_the_known_kernels_are_64_bit(device):
    """C = 3, canvas 26760^2 (just over 2^31 elements), S 24 / st 12, only the first and the last slot present, as
    tests/test_fused_level_gpu.py::test_canvas_offsets_are_64_bit: the three kernels against slicing, sources 6690^2."""
    E = H.engine()
    S, st, n = 24, 12, 2229
    Hc = (n - 1) * st + S
    assert Hc == 26760 and 3 * Hc * Hc > 2 ** 31 and (2 * Hc + Hc - S) * Hc + Hc - S > 2 ** 31
    shape = (3, Hc, Hc)
    seed, a, s = 99, 0.9689, 0.2474
    last = Hc - S
    origins = [(0, 0), (last, last)]
    g = H.gen(1)
    init, kn = torch.rand(3, 6690, 6690, generator=g).to(device), torch.rand(3, 6690, 6690, generator=g).to(device)
    m = (torch.rand(6690, 6690, generator=g) > 0.5).to(device)
    idx = FR.nearest_index(6690, Hc).to(device)
    cut = lambda t, y0, x0: t[..., idx[y0:y0 + S], :][..., idx[x0:x0 + S]]
    sl = lambda t, y0, x0: t[..., y0:y0 + S, x0:x0 + S]
    # start
    x = _start(shape, seed=seed, init=init, known=kn, mask=m, a=a, s=s, mix_sid=E.stream_id(2, 0), out=torch.empty(shape, device=device))
    z = _philox(shape, seed, E.stream_id(16, 2), device)
    zm = _philox(shape, seed, E.stream_id(2, 0), device)
    x_win = []
    for y0, x0 in origins:
        want = _mix(sl(z, y0, x0) + (2 * cut(init, y0, x0) - 1), cut(kn, y0, x0), cut(m, y0, x0), a, s, sl(zm, y0, x0))
        assert torch.equal(sl(x, y0, x0), want), (y0, x0)
        x_win.append(want)
    del z
    # fuse_update_known, hist and out one buffer (zm serves as the history, then holds the estimate)
    tile_of = torch.full((n, n), -1, dtype=torch.int32, device=device)
    tile_of[0, 0], tile_of[-1, -1] = 0, 1
    tiles = (torch.randn(2, 3, S, S, generator=g) * 1.5).to(device)
    hist_win = [sl(zm, y0, x0).clone() for y0, x0 in origins]
    A, B, P, Sn, rn_a, rn_b = 0.83, 0.21, -0.07, 0.4, 1.07, 0.31
    sids = [E.stream_id(p, 1) for p in (1, 3, 2)]
    probe = [(3, 17, 4000), (1, Hc // 2, Hc // 2), (5, Hc - 1, Hc - S - 4)]   # uncovered pixels: (row, column) in channel 2
    before = [float(x[2, r, c]) for _, r, c in probe]
    _fuse_known(x, zm, zm, tiles, None, dict(S=S, st=st, ny=n, nx=n), 0, A, B, P, Sn, None, seed, sids[0], 1, rn_a, rn_b, None, sids[1],
                kn, m, a, s, None, sids[2], tile_of=tile_of, n=2)
    assert [float(x[2, r, c]) for _, r, c in probe] == before
    zs = [_philox(shape, seed, sid, device) for sid in sids[:2]]
    upd = []
    for t, (y0, x0) in enumerate(origins):
        xb = tiles[t].clamp(-1.0, 1.0)
        assert torch.equal(sl(zm, y0, x0), xb), t
        upd.append(((A * x_win[t] + B * xb) + P * hist_win[t]) + Sn * sl(zs[0], y0, x0))
        upd[t] = upd[t] * rn_a + sl(zs[1], y0, x0) * rn_b
    del zs
    zmix = _philox(shape, seed, sids[2], device)
    for t, (y0, x0) in enumerate(origins):
        want = _mix(upd[t], cut(kn, y0, x0), cut(m, y0, x0), a, s, sl(zmix, y0, x0))
        assert torch.equal(sl(x, y0, x0), want), t
    del zmix, zm
    # finalize_known into a canvas of the same size
    out = torch.full(shape, 0.25, device=device)
    _finalize_known(x, dict(S=S, st=st, ny=n, nx=n, origins=origins), out, 0, 0, kn, m, tile_of=tile_of, n=2)
    changed = 0
    for y0, x0 in origins:
        want = torch.where(cut(m, y0, x0), cut(kn, y0, x0), (sl(x, y0, x0).clamp(-1.0, 1.0) + 1) * 0.5)
        assert torch.equal(sl(out, y0, x0), want), (y0, x0)
        changed += int((want != 0.25).sum())
    assert sum(int((out[c] != 0.25).sum()) for c in range(3)) == changed > 0   # nothing outside the two tiles was written


# ------------------------------------------------------------------------------------------------ refusals
def test_the_known_kernels_refuse_and_launch_nothing(device):
    E = H.engine()
    lat = _lattice(16, 12, (2, 2))
    x = torch.full((3, 28, 28), NAN, device=device)
    xb, tiles = torch.full_like(x, NAN), torch.zeros(4, 3, 16, 16, device=device)
    kn, m = torch.rand(3, 28, 28, device=device), torch.ones(28, 28, dtype=torch.uint8, device=device)
    out = torch.full((3, 40, 40), NAN, device=device)
    img = lambda t, **over: E.kd_tiles_image_t(**dict(dict(d=t.data_ptr(), H=t.shape[1], W=t.shape[2], row_stride=t.stride(1),
                                                           plane_stride=t.stride(0)), **over))
    lib, st = E.load(), E.current_stream
    tile_of = torch.tensor(lat["tile_of"], dtype=torch.int32, device=device)
    mk = E.tiles_mask(m)
    cases = [
        (lambda: lib.kd_tiles_start(E.ptr(x), 3, 28, 30, 1.0, None, 0, None, None, None, 0.0, 0.0, None, 0, st()), "Wc % 4"),
        (lambda: lib.kd_tiles_start(E.ptr(x), 3, 28, 28, 1.0, None, 0, None, E.ref(img(kn)), None, 0.5, 0.5, None, 0, st()), "come together"),
        (lambda: lib.kd_tiles_start(E.ptr(x), 3, 28, 28, 1.0, None, 0, None, None, E.ref(mk), 0.5, 0.5, None, 0, st()), "come together"),
        (lambda: lib.kd_tiles_start(E.ptr(x), 3, 28, 28, 1.0, None, 0, E.ref(img(kn, row_stride=20)), None, None, 0.0, 0.0, None, 0, st()),
         "row stride below the width"),
        (lambda: lib.kd_tiles_start(E.ptr(x), 3, 28, 28, 1.0, None, 0, E.ref(img(kn, H=0)), None, None, 0.0, 0.0, None, 0, st()), "size out of range"),
        (lambda: lib.kd_tiles_start(E.ptr(x), 3, 28, 28, 1.0, C.c_void_p(x.data_ptr() + 4), 0, None, None, None, 0.0, 0.0, None, 0, st()),
         "16-byte aligned"),
        (lambda: _fuse_known(x, xb, xb, tiles, None, lat, 0, 1.0, 0.0, 0.0, 0.0, st=4), "more than 3 tiles per axis"),
        (lambda: _fuse_known(x, xb, xb, tiles, None, lat, 0, 1.0, 0.0, 0.0, 0.0, S=18), "S % 4"),
        (lambda: _fuse_known(x, x, xb, tiles, None, lat, 0, 1.0, 0.0, 0.5, 0.0), "x must not be the history"),
        (lambda: _fuse_known(x, None, xb, tiles, None, lat, 0, 1.0, 0.0, 0.5, 0.0), "null argument"),
        (lambda: lib.kd_tiles_fuse_update_known(E.ptr(x), E.ptr(xb), E.ptr(xb), E.ptr(tiles), None, _iptr(tile_of), 4, 3, 16, 12, 2, 2, 0, 1.0,
                                                0.0, 0.0, 0.0, None, 0, 0, 0, 0.0, 0.0, None, 0, E.ref(img(kn)), None, 0.5, 0.5, None, 0, st()),
         "come together"),
        (lambda: _finalize_known(x, lat, out, 0, 2, kn, m), "ox % 4"),
        (lambda: _finalize_known(x, lat, out, 16, 0, kn, m), "outside the output"),
        (lambda: _finalize_known(x, lat, out, 0, 0, None, m), "come together"),
        (lambda: _finalize_known(x, lat, out, 0, 0, kn, None), "come together"),
        (lambda: _finalize_known(x, lat, out, 0, 0, out[:, 4:32, 4:32], m), "must be the window at"),   # inside out, elsewhere
        (lambda: _finalize_known(x, lat, out, 0, 0, out[:, 0:28, 0:36], m), "must be the window at"),   # inside out, another size
    ]
    for call, match in cases:
        with pytest.raises(E.EngineError, match=match):
            rc = call()
            if rc is not None:
                E.check(rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all()) and bool(torch.isnan(xb).all()) and bool(torch.isnan(out).all())   # nothing was launched


# ------------------------------------------------------------------------------------------------ whole sampler
CASCADE_KW = dict(image_sizes=(16, 32), timesteps=(N, N), pred_objectives=("noise", "v"), condition_on_text=False)


def _unets(channels=3, cls=R.Unet, **extra):
    return [H.ref_unet(cls, H.UNET_KW["small1"], seed=3, channels=channels, **extra),
            H.ref_unet(cls, H.UNET_KW["small1"], seed=6, channels=channels, lowres_cond=True, **extra)]


def _cascade(device, unets=None, **over):
    kw = dict(CASCADE_KW, **over)
    oim = RS.Imagen(unets or _unets(kw.get("channels", 3)), **kw)
    return oim, H.product_imagen(oim, "Imagen", device, **kw)


@pytest.fixture(scope="module")
def cascade(device):
    return _cascade(device)


def _mask(grid):
    """56^2 for the 2 x 2 cascade (canvases 28 and 56): columns [0, 20) and the square [30, 40)^2, 39 % known.  80 x 56 for
    3 x 2 with a hole (canvases 40 x 28 and 80 x 56): columns [0, 20), rows [36, 44) and a patch inside the top right and the
    bottom right tile.  32^2 for 1 x 1."""
    if grid == (2, 2):
        m = torch.zeros(56, 56, dtype=torch.bool)
        m[:, :20] = True
        m[30:40, 30:40] = True
    elif grid == (3, 2):
        m = torch.zeros(80, 56, dtype=torch.bool)
        m[:, :20] = True
        m[36:44, :] = True
        m[6:14, 34:46] = True
        m[60:68, 30:42] = True
    else:
        m = torch.zeros(32, 32, dtype=torch.bool)
        m[:, :12] = True
        m[18:26, 16:28] = True
    return m


def _known(grid, channels=3, present=None, sizes=(16, 32)):
    m = _mask(grid)
    KR.assert_mask_condition(m, [KR.lattice(S, grid, 0.25, present) for S in sizes])
    return torch.rand(1, channels, *m.shape, generator=H.gen(31)), m


def _err(oim, pim, device, label, grid=(2, 2), known=None, **kw):
    """max|product - restatement| on identical injected noise; with `known = (image, mask)` the known pixels of the
    product's result are the known image's, bit for bit."""
    nf = RS.generator_noise_fn(41)
    if known is not None:
        kw = dict(kw, known_image=known[0], known_mask=known[1])
    ref = KR.sample_tiled(oim, grid=grid, noise_fn=nf, **kw)
    dv = {k: v.to(device) if torch.is_tensor(v) else v for k, v in kw.items()}
    got = pim.sample_tiled(grid, noise_fn=nf, device=device, **dv).cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and float(got.std()) > 0.01
    if known is not None:
        size = tuple(got.shape[-2:])
        m = _near(known[1], size) & KR.covered_of(KR.lattice(oim.image_sizes[-1], grid, 0.25, kw.get("present")))
        assert torch.equal(got[0, :, m], _near(known[0][0], size)[:, m])
        assert float(got[0, :, ~m].std()) > 0.01
    err = float((got - ref).abs().max())
    print(f"tiled known {label}: canvas {tuple(got.shape[-2:])}, max|diff| {err:.2e}")
    return err


@pytest.mark.parametrize("sampler,eta,R_", [("ddpm", 0.0, 1), ("ddim", 0.0, 1), ("ddim", 0.5, 1), ("dpmpp_2m", 0.0, 1),
                                            ("ddim", 0.0, 2), ("dpmpp_2m", 0.0, 2)])
def test_masked_canvas_matches_the_restatement(device, cascade, sampler, eta, R_):
    """2 x 2 lattice, canvases 28 and 56, the 56^2 mask read at both sizes."""
    oim, pim = cascade
    err = _err(oim, pim, device, f"{sampler} eta {eta} R {R_} 2x2", known=_known((2, 2)), sampler=sampler, sampler_eta=eta,
               known_resample_times=R_)
    assert err < SAMPLE_ABS


def test_masked_ramp_weights_match_the_restatement(device, cascade):
    oim, pim = cascade
    assert _err(oim, pim, device, "dpmpp_2m ramp R 2 2x2", known=_known((2, 2)), sampler="dpmpp_2m", tile_weights="ramp",
                known_resample_times=2) < SAMPLE_ABS


def test_masked_lattice_with_a_hole_matches_the_restatement(device, cascade):
    oim, pim = cascade
    assert _err(oim, pim, device, "ddim 0.5 R 2 3x2 with a hole", grid=(3, 2), present=HOLE, known=_known((3, 2), present=HOLE),
                sampler="ddim", sampler_eta=0.5, known_resample_times=2) < SAMPLE_ABS


def test_masked_self_conditioned_unet_matches_the_restatement(device):
    """2M at R = 2: the history is the last slot's estimate, the carry the previous slot's - two canvases."""
    ou = H.ref_unet(SC.Unet, H.UNET_KW["small1"], seed=21, self_cond=True)
    kw = dict(image_sizes=(16,), timesteps=(N,), pred_objectives=("noise",), condition_on_text=False)
    oim = RS.Imagen([ou], **kw)
    pim = H.product_imagen(oim, "Imagen", device, **kw)
    assert pim.unets[0].self_cond
    known = _known((2, 2), sizes=(16,))
    assert _err(oim, pim, device, "dpmpp_2m self-cond R 2 2x2", known=known, sampler="dpmpp_2m", known_resample_times=2) < SAMPLE_ABS
    assert _err(oim, pim, device, "dpmpp_2m self-cond skip 3 2x2", sampler="dpmpp_2m", init_canvas=known[0], init_skip_steps=3) < SAMPLE_ABS


@pytest.mark.parametrize("masked", [False, True], ids=["alone", "with-a-mask"])
def test_canvas_from_an_image_matches_the_restatement(device, cascade, masked):
    """init_canvas (50 x 44, resized to both canvases) with skip (3, 5); 2M is first order on the first step walked."""
    oim, pim = cascade
    init = torch.rand(1, 3, 50, 44, generator=H.gen(32))
    kw = dict(known=_known((2, 2)), known_resample_times=2) if masked else {}
    assert _err(oim, pim, device, f"dpmpp_2m init skip (3, 5) {'masked' if masked else ''}", sampler="dpmpp_2m", init_canvas=init,
                init_skip_steps=(3, 5), **kw) < SAMPLE_ABS


def test_masked_text_guided_canvas_matches_the_restatement(device):
    ou = H.ref_unet(R.Unet, dict(H.UNET_KW["small1"], cond_dim=64, text_embed_dim=3), seed=17, text=True)
    kw = dict(image_sizes=(16,), timesteps=(N,), text_embed_dim=3)
    oim = RS.Imagen([ou], **kw)
    pim = H.product_imagen(oim, "Imagen", device, **kw)
    text = torch.randn(1, 2, 3, generator=H.gen(4))
    assert _err(oim, pim, device, "dpmpp_2m text cond_scale 3 R 2 2x2", known=_known((2, 2), sizes=(16,)), sampler="dpmpp_2m",
                text_embeds=text, cond_scale=3.0, known_resample_times=2) < SAMPLE_ABS


def test_masked_one_channel_canvas_matches_the_restatement(device):
    oim, pim = _cascade(device, channels=1)
    assert _err(oim, pim, device, "dpmpp_2m channels=1 R 2 2x2", known=_known((2, 2), channels=1), sampler="dpmpp_2m",
                known_resample_times=2) < SAMPLE_ABS


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("R_", [1, 2])
@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0), ("ddpm", 0.0)])
def test_one_masked_tile_is_sample_at_batch_1(device, cascade, sampler, eta, R_):
    """A 1 x 1 lattice draws what sample(batch_size=1, inpaint_images=...) draws: the solvers' canvas equals it bit for bit
    on the unknown pixels through both stages; the known pixels are the known image's, copied.  "ddpm" runs the ancestral
    step in the linear form: the sampler bound, as in tests/test_tiled_gpu.py."""
    pim = cascade[1]
    kn, m = (t.to(device) for t in _known((1, 1)))
    kw = dict(seed=77, sampler=sampler, sampler_eta=eta, device=device)
    got = pim.sample_tiled((1, 1), known_image=kn, known_mask=m, known_resample_times=R_, **kw)
    want = pim.sample(batch_size=1, inpaint_images=kn, inpaint_masks=m[None], inpaint_resample_times=R_, **kw)
    assert got.shape == want.shape == (1, 3, 32, 32) and torch.equal(got[0, :, m], kn[0, :, m])
    if sampler == "ddpm":
        err = float((got - want).abs().max())
        print(f"tiled 1x1 masked ddpm R {R_} against the ancestral sample(): max|diff| {err:.2e}")
        assert err < SAMPLE_ABS
    else:
        assert torch.equal(got[0, :, ~m], want[0, :, ~m]) and float((got - want).abs().max()) <= 1.2e-7


@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0), ("ddpm", 0.0)])
def test_one_tile_from_an_image_is_sample_at_batch_1(device, cascade, sampler, eta):
    pim = cascade[1]
    init = torch.rand(1, 3, 24, 20, generator=H.gen(33)).to(device)
    kw = dict(seed=78, sampler=sampler, sampler_eta=eta, device=device)
    got = pim.sample_tiled((1, 1), init_canvas=init, init_skip_steps=(3, 5), **kw)
    want = pim.sample(batch_size=1, init_images=init, skip_steps=(3, 5), **kw)
    if sampler == "ddpm":
        assert float((got - want).abs().max()) < SAMPLE_ABS
    else:
        assert torch.equal(got, want)


def test_graph_streaming_and_poison_do_not_change_a_bit(device, cascade):
    """Graph on = off, streamed = not streamed (kd_tiles_finalize_known = the torch paste), poisoned plan scratch, and a
    spare canvas (2M at R = 2) that the allocator hands out full of NaN."""
    E = H.engine()
    pim = cascade[1]
    kn, m = (t.to(device) for t in _known((2, 2)))
    kw = dict(seed=5, sampler="dpmpp_2m", tile_batch=3, device=device, known_image=kn, known_mask=m, known_resample_times=2,
              init_canvas=kn, init_skip_steps=(0, 2))
    base = pim.sample_tiled((2, 2), **kw)
    assert bool(torch.isfinite(base).all()) and torch.equal(base[0, :, m], kn[0, :, m])
    assert torch.equal(pim.sample_tiled((2, 2), **kw), base)
    assert torch.equal(pim.sample_tiled((2, 2), use_graph=False, **kw), base)
    assert torch.equal(pim.sample_tiled((2, 2), streamed=True, **kw), base)
    assert not torch.equal(pim.sample_tiled((2, 2), **dict(kw, seed=6)), base)
    # streamed into a canvas whose window is the known image itself
    canvas = torch.rand(1, 3, 72, 76, generator=H.gen(2)).to(device)
    canvas[:, :, 8:64, 12:68] = kn
    before = canvas.clone()
    pim.sample_tiled((2, 2), streamed=True, into=(canvas, 8, 12), **dict(kw, known_image=canvas[:, :, 8:64, 12:68], init_canvas=kn.clone()))
    assert torch.equal(canvas[:, :, 8:64, 12:68], base)
    canvas[:, :, 8:64, 12:68] = before[:, :, 8:64, 12:68]
    assert torch.equal(canvas, before)
    for word in (0xFFFFFFFF, 0x7149F2CA):
        for u in pim.unets:
            for h in u._engines.values():
                filled = C.c_int64(-1)
                E.check(E.load().kd_unet_poison_scratch(h, word, C.byref(filled), E.current_stream()))
                assert filled.value > 0
        for shape in ((1, 3, 28, 28), (1, 3, 56, 56)):   # blocks of the spare canvases' sizes, freed full of NaN
            spare = [torch.full(shape, NAN, device=device) for _ in range(4)]
            del spare
        assert torch.equal(pim.sample_tiled((2, 2), **kw), base), hex(word)


def test_a_call_without_the_new_arguments_keeps_its_bits(device, cascade):
    """The canvas of the parent commit under seed 5 (tests/golden/tiled_seed5_2x2.pt: 2 x 2, DDIM(0.5) and 2M with ramp
    weights, recorded on the MI355X before this change), streamed on and off."""
    import pathlib

    pim = cascade[1]
    gold = torch.load(pathlib.Path(__file__).parent / "golden" / "tiled_seed5_2x2.pt")
    for name, kw in (("ddim", dict(sampler="ddim", sampler_eta=0.5, tile_batch=3)), ("dpmpp_2m", dict(sampler="dpmpp_2m", tile_weights="ramp")),
                     ("ddpm", {})):
        for streamed in (False, True):
            got = pim.sample_tiled((2, 2), seed=5, device=device, streamed=streamed, **kw).cpu()
            assert torch.equal(got, gold[name]), (name, streamed)


# ------------------------------------------------------------------------------------------------ fused_level
TOY_W, TOY_WINDOW = 44, 24
BLOCK = [(i, j) for i in (2, 3, 4) for j in (2, 3, 4)]


def _toy_geom():
    from ultra_res import grid as G

    return G.GridGeometry(8, 6, 7, 24, 176)


@pytest.fixture(scope="module")
def level(device):
    """(oracle, product, zoomed image, the finished 7 x 7 toy level [1, 3, 176, 176]) with 3 conditioning channels."""
    from ultra_res import tiled as UT

    unets = [H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=3, cond_images_channels=3),
             H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=6, cond_images_channels=3, lowres_cond=True)]
    oim = RS.Imagen(unets, **CASCADE_KW)
    pim = H.product_imagen(oim, "Imagen", device, **CASCADE_KW)
    zoomed = torch.rand(1, 3, TOY_W, TOY_W, generator=H.gen(44))
    geom = _toy_geom()
    done = UT.fused_level(lambda stage: pim, zoomed, geom, geom.positions, window=TOY_WINDOW, stages=(1, 2), device=device,
                          sampler="dpmpp_2m", seed=21, tile_batch=16)
    return oim, pim, zoomed, done


def _crops(zoomed, pos):
    import imagen_pytorch as ip

    geom = _toy_geom()
    return ip.TileCondCrops(zoomed, FR.shifts_of(TOY_W, geom, pos), TOY_WINDOW, 0.95)


def test_fused_level_regenerates_a_block_of_a_finished_level(device, level):
    """The 3 x 3 block regenerated with keep = the rest: every kept pixel keeps its bits, the canvas is the sample_tiled
    call made by hand (windows of the canvas and the mask at the box, written in place), and it is within the sampler
    bound of the restatement composited in torch.  The mask is the issue's: the kept tiles' squares, so inside the box
    (80^2) the known pixels are the 8-pixel strips shared with the neighbours - 36 % known, every overlap strip of the
    border mixed; the centre tile touches no kept tile and is all unknown by construction."""
    from ultra_res import tiled as UT

    oim, pim, zoomed, done = level
    geom = _toy_geom()
    keep = UT.level_keep_mask(geom, [p for p in geom.positions if p not in BLOCK], device)
    box = (slice(48, 128), slice(48, 128))
    share = float(keep[box].float().mean())
    assert 0.25 <= share <= 0.75 and bool(keep[48:56, 48:128].all()) and not bool(keep[56:120, 56:120].any())
    kw = dict(overlap=0.25, tile_batch=4, sampler="dpmpp_2m", known_resample_times=2)
    canvas = done.clone()
    got = UT.fused_level(lambda stage: pim, zoomed, geom, BLOCK, window=TOY_WINDOW, stages=(1, 2), device=device, canvas=canvas,
                         keep=keep, seed=22, **kw)
    assert got is canvas and torch.equal(got[:, :, keep.bool()], done[:, :, keep.bool()])
    assert not torch.equal(got[:, :, 56:120, 56:120], done[:, :, 56:120, 56:120]) and bool(torch.isfinite(got).all())
    r0, c0, grid, present, tiles = UT.level_box(BLOCK)
    hand = done.clone()
    pim.sample_tiled(grid, present=present, cond_crops=_crops(zoomed, tiles), streamed=True, device=device, seed=22,
                     into=(hand, 48, 48), known_image=hand[:, :, box[0], box[1]], known_mask=keep[box], **kw)
    assert torch.equal(got, hand)
    # refine_skip_steps: every stage starts from the canvas' window
    refined = UT.fused_level(lambda stage: pim, zoomed, geom, BLOCK, window=TOY_WINDOW, stages=(1, 2), device=device,
                             canvas=done.clone(), keep=keep, seed=22, refine_skip_steps={1: 2, 2: 5}, **kw)
    hand = done.clone()
    pim.sample_tiled(grid, present=present, cond_crops=_crops(zoomed, tiles), streamed=True, device=device, seed=22,
                     into=(hand, 48, 48), known_image=hand[:, :, box[0], box[1]], known_mask=keep[box],
                     init_canvas=hand[:, :, box[0], box[1]], init_skip_steps=(2, 5), **kw)
    assert torch.equal(refined, hand) and not torch.equal(refined, got)
    assert torch.equal(refined[:, :, keep.bool()], done[:, :, keep.bool()])


def test_fused_level_regeneration_matches_the_restatement(device, level):
    from ultra_res import grid as G
    from ultra_res import tiled as UT

    oim, pim, zoomed, done = level
    geom = _toy_geom()
    keep = UT.level_keep_mask(geom, [p for p in geom.positions if p not in BLOCK], device)
    nf = RS.generator_noise_fn(43)
    got = UT.fused_level(lambda stage: pim, zoomed, geom, BLOCK, window=TOY_WINDOW, stages=(1, 2), device=device,
                         canvas=done.clone(), keep=keep, sampler="dpmpp_2m", noise_fn=nf, known_resample_times=2).cpu()
    r0, c0, grid, present, tiles = UT.level_box(BLOCK)
    with FR.window_of(G, TOY_WINDOW):
        cond = G.cond_images_for_grid(zoomed, geom, tiles, fill_color=0.95, centre_crop_channels=False)
    box = (slice(48, 128), slice(48, 128))
    ref = KR.sample_tiled(oim, grid=grid, present=present, noise_fn=nf, sampler="dpmpp_2m", cond_images=cond,
                          known_image=done.cpu()[:, :, box[0], box[1]], known_mask=keep.cpu()[box], known_resample_times=2)
    want = done.cpu().clone()
    want[:, :, box[0], box[1]] = ref
    err = float((got - want).abs().max())
    print(f"fused_level regenerated 3x3 block vs the restatement: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
