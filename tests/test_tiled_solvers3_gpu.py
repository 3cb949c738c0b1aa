"""The canvas step with a second history on the MI355X: kd_tiles_fuse_update_hist2 against the fp64 expression and bit for
bit against kd_tiles_fuse_update_known; Imagen.sample_tiled with "dpmpp_3m", "dpmpp_2m_sde" and "dpmpp_3m_sde" on the 16 -> 32
cascade of tests/test_tiled_gpu.py against the restatement tests/tiled_solver3_ref.py, bit for bit against sample() on a
1 x 1 lattice, and over two shards."""
import ctypes as C

import pytest
import torch

import helpers as H
import tiled_known_ref as KR
import tiled_solver3_ref as T3
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

REL = 1e-6           # the solver-step bound (tests/test_tiled_gpu.py)
SAMPLE_ABS = 2e-3    # the project's sampler bound against the oracle on identical noise
N = 8
HOLE = [[True, True], [True, False], [True, True]]
NAN = float("nan")
NAMES3 = ("dpmpp_3m", "dpmpp_2m_sde", "dpmpp_3m_sde")


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


def _call(entry, x, hist, out, tiles, thr, lat, ramp, A, B, P, Sn, noise, *tail):
    E = H.engine()
    tile_of = torch.tensor(lat["tile_of"], dtype=torch.int32, device=x.device)
    E.check(getattr(E.load(), entry)(
        E.ptr(x), E.ptr(hist), E.ptr(out), E.ptr(tiles), E.ptr(thr), C.c_void_p(tile_of.data_ptr()), tiles.shape[0], tiles.shape[1],
        lat["S"], lat["st"], lat["ny"], lat["nx"], int(ramp), A, B, P, Sn, E.ptr(noise), 0, 0, 0, 0.0, 0.0, None, 0, None, None, 0.0,
        0.0, None, 0, *tail, E.current_stream()))


def _hist2(x, hist, hist2, out, tiles, thr, lat, ramp, A, B, P, P2, Sn, noise):
    _call("kd_tiles_fuse_update_hist2", x, hist, out, tiles, thr, lat, ramp, A, B, P, Sn, noise, H.engine().ptr(hist2), P2)


def _known(x, hist, out, tiles, thr, lat, ramp, A, B, P, Sn, noise):
    _call("kd_tiles_fuse_update_known", x, hist, out, tiles, thr, lat, ramp, A, B, P, Sn, noise)


def _fp64(x, hist, hist2, tiles, thr, lat, ramp, A, B, P, P2, Sn, z):
    """(x_next, x0bar, covered) of the canvas step in fp64 over the fp32 inputs and weights (tests/test_tiled_known_gpu.py)."""
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
    out = A * x.double() + B * xb + P * hist.double() + P2 * hist2.double() + Sn * z.double()
    return torch.where(covered, out, x.double()), xb, covered


@pytest.mark.parametrize("S,st,grid,present", [(16, 12, (2, 2), None), (16, 8, (3, 3), None), (20, 8, (3, 2), HOLE)])
def test_fuse_update_hist2_is_the_fp64_expression(device, S, st, grid, present):
    """Uniform and ramp weights, thresholds in [1, 3] and NULL.  x <- A x + B x0bar + P hist + P2 hist2 + Sn z within rel-L2
    1e-6 of fp64; the estimate written over the second history (x0bar_out == d_hist2) gives the bits of separate buffers;
    P2 = 0 over a NaN second history is kd_tiles_fuse_update_known bit for bit; the pixels no tile covers keep their bits
    in every buffer."""
    lat = _lattice(S, st, grid, present)
    Cn, n, Hc, Wc = 3, len(lat["origins"]), lat["Hc"], lat["Wc"]
    g = H.gen(S + st + n)
    dv = lambda t: None if t is None else t.to(device)
    bits = lambda t: t.view(torch.int32)
    x_in = torch.randn(Cn, Hc, Wc, generator=g) * 1.5
    h1_in, h2_in = (torch.rand(Cn, Hc, Wc, generator=g) * 2 - 1 for _ in range(2))
    tiles = torch.randn(n, Cn, S, S, generator=g) * 1.5
    z = torch.randn(Cn, Hc, Wc, generator=g)
    nan = torch.full_like(x_in, NAN)
    worst = 0.0
    for ramp in (0, 1):
        for thr in (torch.rand(n, generator=g) * 2 + 1, None):
            for A, B, P, P2, Sn in ((0.83, 0.21, -0.07, 0.05, 0.4), (0.83, 0.21, -0.07, 0.05, 0.0), (0.83, 0.21, 0.0, 0.05, 0.0)):
                want, xb64, covered = _fp64(x_in, h1_in, h2_in, tiles, thr, lat, ramp, A, B, P, P2, Sn, z)
                cov = covered.to(device)
                # separate buffers
                x, h1, h2, out = dv(x_in), dv(nan if P == 0 else h1_in), dv(h2_in), torch.full((Cn, Hc, Wc), 0.125, device=device)
                _hist2(x, h1, h2, out, dv(tiles), dv(thr), lat, ramp, A, B, P, P2, Sn, dv(z) if Sn else dv(nan))
                e = H.rel_l2(x[:, cov].cpu(), want[:, covered])
                worst = max(worst, e)
                assert e <= REL, (ramp, thr is None, P, P2, Sn, e)
                assert H.rel_l2(out[:, cov].cpu(), xb64[:, covered]) <= REL
                assert H.rel_l2(x[:, cov].cpu(), (want - P2 * h2_in.double())[:, covered]) > 20 * REL   # (the term is seen)
                assert torch.equal(bits(h2), bits(dv(h2_in)))   # the histories are read, never written
                assert torch.equal(bits(x[:, ~cov]), bits(dv(x_in)[:, ~cov])) and bool((out[:, ~cov] == 0.125).all())
                # the estimate over the second history
                x2, h2a = dv(x_in), dv(h2_in)
                _hist2(x2, h1, h2a, h2a, dv(tiles), dv(thr), lat, ramp, A, B, P, P2, Sn, dv(z) if Sn else dv(nan))
                assert torch.equal(bits(x2), bits(x)) and torch.equal(bits(h2a[:, cov]), bits(out[:, cov]))
                assert torch.equal(bits(h2a[:, ~cov]), bits(dv(h2_in)[:, ~cov]))
                # ... and over the first
                x3, h1a = dv(x_in), dv(h1_in)
                _hist2(x3, h1a, h2, h1a, dv(tiles), dv(thr), lat, ramp, A, B, P, P2, Sn, dv(z) if Sn else dv(nan))
                assert torch.equal(bits(x3), bits(x)) and torch.equal(bits(h1a[:, cov]), bits(out[:, cov]))
            # P2 = 0: the second history is not read, and the call is kd_tiles_fuse_update_known
            for A, B, P, Sn in ((0.83, 0.21, -0.07, 0.4), (0.83, 0.21, 0.0, 0.0)):
                xa, ha = dv(x_in), dv(h1_in)
                _known(xa, ha, ha, dv(tiles), dv(thr), lat, ramp, A, B, P, Sn, dv(z))
                xb_, hb = dv(x_in), dv(h1_in)
                _hist2(xb_, hb, dv(nan), hb, dv(tiles), dv(thr), lat, ramp, A, B, P, 0.0, Sn, dv(z))
                assert torch.equal(bits(xa), bits(xb_)) and torch.equal(bits(ha), bits(hb)) and bool(torch.isfinite(xb_).all())
                xc, hc = dv(x_in), dv(h1_in)
                E = H.engine()
                tile_of = torch.tensor(lat["tile_of"], dtype=torch.int32, device=device)
                tl, th, zd = dv(tiles), dv(thr), dv(z)   # (held over the launch)
                E.check(E.load().kd_tiles_fuse_update_hist2(
                    E.ptr(xc), E.ptr(hc), E.ptr(hc), E.ptr(tl), E.ptr(th), C.c_void_p(tile_of.data_ptr()), n, Cn, S, st,
                    lat["ny"], lat["nx"], ramp, A, B, P, Sn, E.ptr(zd), 0, 0, 0, 0.0, 0.0, None, 0, None, None, 0.0, 0.0, None, 0,
                    None, 0.0, E.current_stream()))   # (a NULL second history)
                assert torch.equal(bits(xa), bits(xc))
    print(f"fuse update hist2 S{S} st{st} {grid} {'hole' if present else 'full'}: worst rel-L2 {worst:.2e}")


def test_fuse_update_hist2_refuses_and_launches_nothing(device):
    E = H.engine()
    lat = _lattice(16, 12, (2, 2))
    x = torch.zeros(3, 28, 28, device=device)
    h1, h2, tiles = torch.zeros_like(x), torch.zeros_like(x), torch.zeros(4, 3, 16, 16, device=device)
    with pytest.raises(E.EngineError, match="null argument"):
        _call("kd_tiles_fuse_update_hist2", x, h1, h1, tiles, None, lat, 0, 0.9, 0.1, 0.0, 0.0, None, None, 0.25)
    with pytest.raises(E.EngineError, match="x must not be"):
        _hist2(x, h1, x, h1, tiles, None, lat, 0, 0.9, 0.1, 0.0, 0.25, 0.0, None)
    with pytest.raises(E.EngineError, match="16-byte aligned"):
        _call("kd_tiles_fuse_update_hist2", x, h1, h1, tiles, None, lat, 0, 0.9, 0.1, 0.0, 0.0, None,
              C.c_void_p(h2.data_ptr() + 4), 0.25)
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ whole sampler
CASCADE_KW = dict(image_sizes=(16, 32), timesteps=(N, N), pred_objectives=("noise", "v"), condition_on_text=False)


@pytest.fixture(scope="module")
def cascade(device):
    unets = [H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=3), H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=6, lowres_cond=True)]
    oim = RS.Imagen(unets, **CASCADE_KW)
    return oim, H.product_imagen(oim, "Imagen", device, **CASCADE_KW)


def _err(oim, pim, device, label, grid=(2, 2), **kw):
    nf = RS.generator_noise_fn(41)
    ref = T3.sample_tiled(oim, grid=grid, noise_fn=nf, **kw)
    dv = {k: v.to(device) if torch.is_tensor(v) else v for k, v in kw.items()}
    got = pim.sample_tiled(grid, noise_fn=nf, device=device, **dv).cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and float(got.std()) > 0.01
    err = float((got - ref).abs().max())
    print(f"tiled solvers3 {label}: canvas {tuple(got.shape[-2:])}, max|diff| {err:.2e}")
    return err


@pytest.mark.parametrize("sampler", NAMES3)
def test_canvas_matches_the_restatement(device, cascade, sampler):
    """2 x 2 lattice, canvases 28 and 56, T = 8."""
    oim, pim = cascade
    assert _err(oim, pim, device, f"{sampler} 2x2", sampler=sampler) < SAMPLE_ABS


def test_masked_canvas_with_resampling_matches_the_restatement(device, cascade):
    """known pixels, R = 2 under 3M: the ring advances in a step's last slot only (the mask of tests/test_tiled_known_gpu.py)."""
    oim, pim = cascade
    m = torch.zeros(56, 56, dtype=torch.bool)
    m[:, :20] = True
    m[30:40, 30:40] = True
    KR.assert_mask_condition(m, [KR.lattice(S, (2, 2), 0.25, None) for S in (16, 32)])
    kn = torch.rand(1, 3, 56, 56, generator=H.gen(31))
    err = _err(oim, pim, device, "dpmpp_3m R 2 2x2", sampler="dpmpp_3m", known_image=kn, known_mask=m, known_resample_times=2)
    assert err < SAMPLE_ABS


@pytest.mark.parametrize("sampler", NAMES3)
def test_one_tile_is_sample_at_batch_1(device, cascade, sampler):
    pim = cascade[1]
    kw = dict(seed=77, sampler=sampler, device=device)
    got = pim.sample_tiled((1, 1), **kw)
    want = pim.sample(batch_size=1, **kw)
    assert got.shape == want.shape == (1, 3, 32, 32) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


@pytest.mark.parametrize("sampler", ["dpmpp_3m", "dpmpp_3m_sde"])
def test_two_shards_on_one_device_are_the_single_canvas(device, cascade, sampler):
    """devices=[d, d]: each shard holds the second history like the first; tile_batch 2 divides the 4 tiles of the single
    canvas and the 2 of each shard, so every chunk of both calls has one batch size."""
    pim = cascade[1]
    kw = dict(seed=5, sampler=sampler, tile_batch=2)
    base = pim.sample_tiled((2, 2), device=device, **kw)
    assert torch.equal(pim.sample_tiled((2, 2), devices=[device, device], **kw), base)
    assert bool(torch.isfinite(base).all()) and float(base.std()) > 0.01
