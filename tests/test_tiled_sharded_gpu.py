"""A fused-tile canvas over several shards, on the MI355X: kd_tiles_rows_copy against slicing, its strip-buffer form, its
addressing past 2^31 elements and its refusals; kd_tiles_finalize_rows against kd_tiles_finalize_known; then
Imagen.sample_tiled(devices=[d, d]) and [d, d, d] - the shards of one canvas on one GPU, each with plans of its own -
against devices=None on the 16 -> 32 cascade of tests/test_tiled_gpu.py, bit for bit wherever every chunk of both calls has
one batch size; ultra_res.tiled.fused_level(devices=) on the 7 x 7 toy level; and two distinct devices where there are two."""
import ctypes as C

import pytest
import torch

import helpers as H
import self_cond_ref as SC
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

TWO_PLANS = 4e-3     # tests/test_seeds_gpu.py, tests/test_tiled_gpu.py: two plans of different batch, each within 2e-3 of the oracle
N = 8
HOLE = [[True, True], [True, False], [True, True]]
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ kd_tiles_rows_copy
def _rows_copy(src, dst, desc, S, Cn, thr_src=None, thr_dst=None, src_rows=None, dst_rows=None):
    E = H.engine()
    flat = (C.c_int * (4 * len(desc)))(*[int(v) for d in desc for v in d])
    return E.load().kd_tiles_rows_copy(E.ptr(src), src.shape[0], S if src_rows is None else src_rows, E.ptr(dst), dst.shape[0],
                                       S if dst_rows is None else dst_rows, E.ptr(thr_src), E.ptr(thr_dst), len(desc), Cn, S, flat,
                                       E.current_stream())


@pytest.mark.parametrize("S", [16, 20])
@pytest.mark.parametrize("Cn", [1, 3, 4])
def test_rows_copy_is_slicing(device, Cn, S):
    """Rows 4, 8 and S at every row0 that fits in steps of 4; 1, 5 and 33 descriptors (two launches); src = dst tile
    index in different buffers; with and without thresholds.  Untouched elements keep their bits."""
    E = H.engine()
    g = H.gen(Cn * 100 + S)
    src = torch.randn(9, Cn, S, S, generator=g).to(device)
    thr_src = torch.rand(9, generator=g).to(device)
    for rows in (4, 8, S):
        for n in (1, 5, 33):
            before = torch.randn(40, Cn, S, S, generator=g).to(device)
            thr_before = torch.rand(40, generator=g).to(device)
            # distinct destination tiles; descriptor i copies src tile i % 9 (the first: src = dst index)
            desc = [(i % 9, i if i < 9 else i + 3, (4 * i) % (S - rows + 4) if rows < S else 0, rows) for i in range(n)]
            assert desc[0][0] == desc[0][1] and all(r0 + r <= S for _, _, r0, r in desc)
            for with_thr in (False, True):
                dst, thr_dst = before.clone(), thr_before.clone()
                rc = _rows_copy(src, dst, desc, S, Cn, thr_src if with_thr else None, thr_dst if with_thr else None)
                E.check(rc)
                want, thr_want = before.clone(), thr_before.clone()
                for ts, td, r0, r in desc:
                    want[td, :, r0:r0 + r] = src[ts, :, r0:r0 + r]
                    if with_thr:
                        thr_want[td] = thr_src[ts]
                assert torch.equal(dst, want) and torch.equal(thr_dst, thr_want), (rows, n, with_thr)
    # rows = 0 moves nothing (the threshold still travels)
    dst, thr_dst = before.clone(), thr_before.clone()
    E.check(_rows_copy(src, dst, [(2, 5, 4, 0)], S, Cn, thr_src, thr_dst))
    assert torch.equal(dst, before) and float(thr_dst[5]) == float(thr_src[2])


@pytest.mark.parametrize("S,rows", [(16, 4), (20, 12)])
def test_rows_copy_packs_and_unpacks_a_strip_buffer(device, S, rows):
    """A side with fewer than S rows per tile is a strip buffer, the strip at its top: store -> buffer -> another store
    moves rows row0 .. row0 + r of every tile and its threshold, and nothing else; a shorter strip leaves the rest of its
    slot alone."""
    E = H.engine()
    g = H.gen(S + rows)
    Cn, n = 3, 6
    a, b = torch.randn(7, Cn, S, S, generator=g).to(device), torch.randn(8, Cn, S, S, generator=g).to(device)
    thr_a, thr_b = torch.rand(7, generator=g).to(device), torch.rand(8, generator=g).to(device)
    items = [(6 - m, m + 2, S - rows if m % 2 else 0, rows if m < 4 else rows - 4) for m in range(n)]   # (tile of a, tile of b, row0, r)
    flat = torch.full((n * Cn * rows * S + n,), NAN, device=device)
    buf, thr_buf = flat[:n * Cn * rows * S].view(n, Cn, rows, S), flat[n * Cn * rows * S:]
    E.check(_rows_copy(a, buf, [(ta, m, r0, r) for m, (ta, _, r0, r) in enumerate(items)], S, Cn, thr_a, thr_buf, dst_rows=rows))
    for m, (ta, _, r0, r) in enumerate(items):
        assert torch.equal(buf[m, :, :r], a[ta, :, r0:r0 + r]) and bool(torch.isnan(buf[m, :, r:]).all())
        assert float(thr_buf[m]) == float(thr_a[ta])
    other = torch.empty_like(flat)
    other.copy_(flat)
    want, thr_want = b.clone(), thr_b.clone()
    for m, (ta, tb, r0, r) in enumerate(items):
        want[tb, :, r0:r0 + r] = a[ta, :, r0:r0 + r]
        thr_want[tb] = thr_a[ta]
    E.check(_rows_copy(other[:n * Cn * rows * S].view(n, Cn, rows, S), b, [(m, tb, r0, r) for m, (_, tb, r0, r) in enumerate(items)],
                       S, Cn, other[n * Cn * rows * S:], thr_b, src_rows=rows))
    assert torch.equal(b, want) and torch.equal(thr_b, thr_want)


def test_rows_copy_offsets_are_64_bit(device):
    """Tile 2048 of a store of 2049 one-channel tiles of 1024^2 begins 2^31 elements in: read there, written there."""
    E = H.engine()
    S, last = 1024, 2048
    big = torch.empty(last + 1, 1, S, S, device=device)
    assert big.numel() > 2 ** 31
    big[last] = torch.randn(1, S, S, generator=H.gen(9)).to(device)
    small = torch.zeros(2, 1, S, S, device=device)
    E.check(_rows_copy(big, small, [(last, 1, 768, 256)], S, 1))
    assert torch.equal(small[1, :, 768:], big[last, :, 768:]) and not bool(small[1, :, :768].any()) and not bool(small[0].any())
    keep = big[last].clone()
    small[0] = torch.randn(1, S, S, generator=H.gen(10)).to(device)
    E.check(_rows_copy(small, big, [(0, last, 0, 256)], S, 1))
    assert torch.equal(big[last, :, :256], small[0, :, :256]) and torch.equal(big[last, :, 256:], keep[:, 256:])
    del big


def test_rows_copy_refuses_and_launches_nothing(device):
    E = H.engine()
    S, Cn = 16, 3
    src = torch.randn(4, Cn, S, S, generator=H.gen(1)).to(device)
    dst = torch.full((4, Cn, S, S), NAN, device=device)
    thr = torch.rand(4, generator=H.gen(2)).to(device)
    lib = E.load()
    ok = [(0, 1, 4, 8)]
    flat = lambda desc: (C.c_int * (4 * len(desc)))(*[v for d in desc for v in d])
    call = lambda s, d, desc, S_=S, sr=S, dr=S, ts=None, td=None, st=4, dt=4: lib.kd_tiles_rows_copy(
        s, st, sr, d, dt, dr, ts, td, len(desc), Cn, S_, flat(desc), E.current_stream())
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    refused = [
        ("null src", lambda: call(None, p(dst), ok)),
        ("null dst", lambda: call(p(src), None, ok)),
        ("one buffer", lambda: call(p(src), p(src), ok)),
        ("misaligned src", lambda: call(p(src, 4), p(dst), ok)),
        ("misaligned dst", lambda: call(p(src), p(dst, 8), ok)),
        ("S % 4", lambda: call(p(src), p(dst), ok, S_=18, sr=18, dr=18)),
        ("rows < 0", lambda: call(p(src), p(dst), [(0, 1, 4, -4)])),
        ("rows > S", lambda: call(p(src), p(dst), [(0, 1, 0, S + 4)])),
        ("row0 < 0", lambda: call(p(src), p(dst), [(0, 1, -4, 8)])),
        ("row0 + rows > S", lambda: call(p(src), p(dst), [(0, 1, 12, 8)])),
        ("a later descriptor", lambda: call(p(src), p(dst), ok * 40 + [(0, 1, 12, 8)])),
        ("src tile", lambda: call(p(src), p(dst), [(4, 1, 0, 8)])),
        ("dst tile", lambda: call(p(src), p(dst), [(0, -1, 0, 8)])),
        ("taller than the strip buffer", lambda: call(p(src), p(dst), [(0, 1, 0, 8)], dr=4)),
        ("a threshold without its twin", lambda: call(p(src), p(dst), ok, ts=p(thr))),
        ("no descriptor", lambda: lib.kd_tiles_rows_copy(p(src), 4, S, p(dst), 4, S, None, None, 0, Cn, S, flat(ok), E.current_stream())),
    ]
    for label, fn in refused:
        assert fn() != 0, label
        assert "tiles rows copy" in lib.kd_last_error().decode(), label
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all())   # nothing was launched
    assert call(p(src), p(dst), ok) == 0 and torch.equal(dst[1, :, 4:12], src[0, :, 4:12])


# ------------------------------------------------------------------------------------------------ kd_tiles_finalize_rows
@pytest.mark.parametrize("present", [None, HOLE])
def test_finalize_rows_is_finalize_known_on_those_rows(device, present):
    """The rows [y0, y1) written in place at an offset, and into a band that holds those rows alone (oy = -y0): the bits of
    kd_tiles_finalize_known there, every other element untouched."""
    E = H.engine()
    from imagen_pytorch.imagen_pytorch import normalize_tiling

    (geo,) = normalize_tiling((16,), (3, 2), present=present)
    Hc, Wc, n = geo["Hc"], geo["Wc"], len(geo["origins"])
    g = H.gen(77)
    x = (torch.randn(3, Hc, Wc, generator=g) * 1.5).to(device)
    kn, m = torch.rand(3, Hc, Wc, generator=g).to(device), (torch.rand(Hc, Wc, generator=g) > 0.6).to(device)
    tile_of = torch.tensor(geo["tile_of"], dtype=torch.int32, device=device)
    lib = E.load()
    args = (E.ptr(x), C.c_void_p(tile_of.data_ptr()), n, 3, 16, 12, 3, 2)
    for known in (False, True):
        ks, ms = (E.tiles_image(kn), E.tiles_mask(m)) if known else (None, None)
        before = torch.rand(3, Hc + 8, Wc + 12, generator=g).to(device)
        whole = before.clone()
        E.check(lib.kd_tiles_finalize_known(*args, E.ptr(whole), Hc + 8, Wc + 12, 4, 8, E.ref(ks), E.ref(ms), E.current_stream()))
        for y0, y1 in ((0, 12), (12, 24), (24, Hc), (0, Hc)):
            part = before.clone()
            E.check(lib.kd_tiles_finalize_rows(*args, E.ptr(part), Hc + 8, Wc + 12, 4, 8, E.ref(ks), E.ref(ms), y0, y1, E.current_stream()))
            want = before.clone()
            want[:, 4 + y0:4 + y1] = whole[:, 4 + y0:4 + y1]
            assert torch.equal(part, want), (known, y0, y1)
            band0 = torch.rand(3, y1 - y0, Wc, generator=g).to(device)
            band = band0.clone()
            E.check(lib.kd_tiles_finalize_rows(*args, E.ptr(band), y1 - y0, Wc, -y0, 0, E.ref(ks), E.ref(ms), y0, y1, E.current_stream()))
            covered = whole[:, 4 + y0:4 + y1, 8:8 + Wc] != before[:, 4 + y0:4 + y1, 8:8 + Wc]
            assert torch.equal(band, torch.where(covered, whole[:, 4 + y0:4 + y1, 8:8 + Wc], band0)), (known, y0, y1)
    out = torch.full((3, 12, Wc), NAN, device=device)
    for y0, y1, oy, Ho in ((12, 12, -12, 12), (-4, 8, 4, 12), (12, Hc + 4, -12, Hc), (12, 24, -8, 12), (12, 24, -12, 8)):
        assert lib.kd_tiles_finalize_rows(*args, E.ptr(out), Ho, Wc, oy, 0, None, None, y0, y1, E.current_stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ whole sampler
CASCADE_KW = dict(image_sizes=(16, 32), timesteps=(N, N), pred_objectives=("noise", "v"), condition_on_text=False)


def _unets(channels=3, **extra):
    return [H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=3, channels=channels, **extra),
            H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=6, channels=channels, lowres_cond=True, **extra)]


def _product(device, unets=None, **over):
    kw = dict(CASCADE_KW, **over)
    return H.product_imagen(RS.Imagen(unets or _unets(kw.get("channels", 3)), **kw), "Imagen", device, **kw)


@pytest.fixture(scope="module")
def cascade(device):
    return _product(device)


def _known(grid, channels=3):
    """The known image and mask at the last canvas' size: columns [0, 20), and rows that cross the seam between the
    first two lattice rows (and so between the first two shards)."""
    Hc, Wc = (grid[0] - 1) * 24 + 32, (grid[1] - 1) * 24 + 32
    m = torch.zeros(Hc, Wc, dtype=torch.bool)
    m[:, :20] = True
    m[20:30, :] = True
    return torch.rand(1, channels, Hc, Wc, generator=H.gen(31)), m


LATTICES = {"4x2": ((4, 2), None), "3x2-hole": ((3, 2), HOLE)}


def _sharded_equals_unsharded(pim, device, grid, present, tile_batch, shards=(2, 3), **kw):
    base = pim.sample_tiled(grid, present=present, tile_batch=tile_batch, device=device, **kw)
    assert bool(torch.isfinite(base).all()) and float(base.std()) > 0.01
    for n in shards:
        got = pim.sample_tiled(grid, present=present, tile_batch=tile_batch, devices=[device] * n, **kw)
        assert got.device == base.device and got.shape == base.shape
        assert torch.equal(got, base), (n, float((got - base).abs().max()))
    return base


@pytest.mark.parametrize("lattice,tile_batch", [("4x2", 1), ("4x2", 2), ("3x2-hole", 1)])
@pytest.mark.parametrize("sampler,eta,weights", [("ddpm", 0.0, "uniform"), ("ddim", 0.5, "uniform"), ("dpmpp_2m", 0.0, "uniform"),
                                                 ("dpmpp_2m", 0.0, "ramp")])
def test_shards_on_one_device_keep_the_bits(device, cascade, lattice, tile_batch, sampler, eta, weights):
    """Both stages of the cascade (the second with low-res conditioning) under a seed: [d, d] and [d, d, d] against
    devices=None.  tile_batch 1, and on the full lattice tile_batch = nx - every chunk of every run one batch size."""
    grid, present = LATTICES[lattice]
    _sharded_equals_unsharded(cascade, device, grid, present, tile_batch, seed=11, sampler=sampler, sampler_eta=eta,
                              tile_weights=weights)


@pytest.mark.parametrize("lattice,tile_batch", [("4x2", 2), ("3x2-hole", 1)])
def test_shards_keep_known_pixels_and_an_image_start(device, cascade, lattice, tile_batch):
    """known image at R = 2 (2M: the history and the slot's estimate apart), and init_canvas with skip 3."""
    grid, present = LATTICES[lattice]
    kn, m = (t.to(device) for t in _known(grid))
    base = _sharded_equals_unsharded(cascade, device, grid, present, tile_batch, seed=12, sampler="dpmpp_2m", known_image=kn,
                                     known_mask=m, known_resample_times=2)
    covered = base[0].abs().sum(0) > 0
    assert torch.equal(base[0, :, m & covered], kn[0, :, m & covered])
    _sharded_equals_unsharded(cascade, device, grid, present, tile_batch, seed=13, sampler="ddim", sampler_eta=0.5, init_canvas=kn,
                              init_skip_steps=3)
    _sharded_equals_unsharded(cascade, device, grid, present, tile_batch, seed=14, known_image=kn, known_mask=m,
                              known_resample_times=2, init_canvas=kn, init_skip_steps=3, streamed=True)


def test_shards_carry_the_self_conditioning(device):
    ou = H.ref_unet(SC.Unet, H.UNET_KW["small1"], seed=21, self_cond=True)
    kw = dict(image_sizes=(16,), timesteps=(N,), pred_objectives=("noise",), condition_on_text=False)
    pim = H.product_imagen(RS.Imagen([ou], **kw), "Imagen", device, **kw)
    assert pim.unets[0].self_cond
    kn, m = _known((4, 2))
    kn, m = kn[:, :, ::2, ::2].contiguous().to(device), m[::2, ::2].contiguous().to(device)
    _sharded_equals_unsharded(pim, device, (4, 2), None, 2, seed=15, sampler="dpmpp_2m")
    _sharded_equals_unsharded(pim, device, (3, 2), HOLE, 1, seed=16, sampler="dpmpp_2m", known_image=kn[:, :, :40], known_mask=m[:40],
                              known_resample_times=2)


def test_shards_under_text_guidance(device):
    ou = H.ref_unet(R.Unet, dict(H.UNET_KW["small1"], cond_dim=64, text_embed_dim=3), seed=17, text=True)
    kw = dict(image_sizes=(16,), timesteps=(N,), text_embed_dim=3)
    pim = H.product_imagen(RS.Imagen([ou], **kw), "Imagen", device, **kw)
    text = torch.randn(1, 2, 3, generator=H.gen(4)).to(device)
    _sharded_equals_unsharded(pim, device, (4, 2), None, 2, seed=17, sampler="dpmpp_2m", text_embeds=text, cond_scale=3.0)


def test_shards_of_a_one_channel_canvas(device):
    pim = _product(device, channels=1)
    _sharded_equals_unsharded(pim, device, (4, 2), None, 2, seed=18, sampler="ddim", sampler_eta=0.5)
    _sharded_equals_unsharded(pim, device, (3, 2), HOLE, 1, seed=18, sample_steps=(4, 6))   # and a shorter schedule per stage


def test_graph_on_is_graph_off_and_cond_images_follow_their_tiles(device):
    pim = _product(device, _unets(cond_images_channels=3))
    cond = torch.rand(8, 3, 16, 16, generator=H.gen(8)).to(device)
    kw = dict(seed=19, sampler="dpmpp_2m", cond_images=cond)
    base = _sharded_equals_unsharded(pim, device, (4, 2), None, 2, **kw)
    for n in (2, 3):
        assert torch.equal(pim.sample_tiled((4, 2), tile_batch=2, devices=[device] * n, use_graph=False, **kw), base)
    assert not torch.equal(pim.sample_tiled((4, 2), tile_batch=2, devices=[device] * 2, **dict(kw, cond_images=cond.flip(0))), base)


def test_ragged_chunks_stay_within_the_bound_of_two_plans(device, cascade):
    """tile_batch = 3 on 8 tiles: the unsharded call runs chunks of 3, 3, 2, two shards 3, 1 each, three shards 3, 1 / 2 / 2 -
    plans of different batch sizes round differently, the project's bound for that is 4e-3 (tests/test_tiled_gpu.py).
    Observed on the MI355X: 3.3e-7 (2 shards) and 3.6e-7 (3 shards)."""
    kw = dict(seed=20, sampler="dpmpp_2m", tile_batch=3)
    base = cascade.sample_tiled((4, 2), device=device, **kw)
    for n in (2, 3):
        err = float((cascade.sample_tiled((4, 2), devices=[device] * n, **kw) - base).abs().max())
        print(f"sharded ragged chunks, {n} shards, tile_batch 3: max|diff| {err:.2e}")
        assert err < TWO_PLANS


def test_nothing_outside_a_received_strip_reaches_an_owned_pixel(device, cascade, monkeypatch):
    """`_tiled_stage(_poison_halo=True)`, the stage loop's keyword for this test: every halo slot of every shard's store (and
    its threshold) is NaN before every slot, so only the received strips hold numbers; the canvas is finite and the canvas
    of devices=None all the same."""
    import functools

    kn, m = (t.to(device) for t in _known((4, 2)))
    kw = dict(seed=21, sampler="dpmpp_2m", tile_batch=2, tile_weights="ramp", known_image=kn, known_mask=m, known_resample_times=2)
    base = cascade.sample_tiled((4, 2), device=device, **kw)
    hole = cascade.sample_tiled((3, 2), present=HOLE, tile_batch=1, device=device, seed=21, streamed=True)
    monkeypatch.setattr(cascade, "_tiled_stage", functools.partial(cascade._tiled_stage, _poison_halo=True))
    for n in (2, 3):
        got = cascade.sample_tiled((4, 2), devices=[device] * n, **kw)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, base), n
    got = cascade.sample_tiled((3, 2), present=HOLE, tile_batch=1, devices=[device] * 3, seed=21, streamed=True)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, hole)


# ------------------------------------------------------------------------------------------------ streamed, cond_crops, into
TOY_W, TOY_WINDOW = 44, 24


def _toy_geom():
    from ultra_res import grid as G

    return G.GridGeometry(8, 6, 7, 24, 176)


@pytest.fixture(scope="module")
def level_imagen(device):
    unets = [H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=3, cond_images_channels=3),
             H.ref_unet(R.Unet, H.UNET_KW["small1"], seed=6, cond_images_channels=3, lowres_cond=True)]
    return H.product_imagen(RS.Imagen(unets, **CASCADE_KW), "Imagen", device, **CASCADE_KW)


@pytest.mark.parametrize("lattice,tile_batch", [("4x2", 2), ("3x2-hole", 1)])
def test_shards_stream_into_a_canvas_at_an_offset(device, level_imagen, lattice, tile_batch):
    """streamed + cond_crops + into at (8, 12): the window equals devices=None, the rest of `into` - and, under the hole,
    the pixels no tile covers - keep their bits."""
    import fused_level_ref as FR
    import imagen_pytorch as ip

    grid, present = LATTICES[lattice]
    pim = level_imagen
    zoomed = torch.rand(1, 3, TOY_W, TOY_W, generator=H.gen(44))
    pos = [(i, j) for i in range(grid[0]) for j in range(grid[1]) if present is None or present[i][j]]
    crops = lambda: ip.TileCondCrops(zoomed, FR.shifts_of(TOY_W, _toy_geom(), pos), TOY_WINDOW, 0.95)
    Hc, Wc = (grid[0] - 1) * 24 + 32, (grid[1] - 1) * 24 + 32
    before = torch.rand(1, 3, Hc + 20, Wc + 24, generator=H.gen(2)).to(device)
    kw = dict(present=present, tile_batch=tile_batch, seed=23, sampler="dpmpp_2m", streamed=True)
    want = before.clone()
    pim.sample_tiled(grid, cond_crops=crops(), into=(want, 8, 12), device=device, **kw)
    assert not torch.equal(want, before)
    for n in (2, 3):
        got = before.clone()
        out = pim.sample_tiled(grid, cond_crops=crops(), into=(got, 8, 12), devices=[device] * n, **kw)
        assert out is got and torch.equal(got, want), n
    rest = want.clone()
    rest[:, :, 8:8 + Hc, 12:12 + Wc] = before[:, :, 8:8 + Hc, 12:12 + Wc]
    assert torch.equal(rest, before)
    if present is not None:   # the hole: rows [32, 48) x columns [32, 56) of the window are covered by no tile
        assert torch.equal(want[:, :, 8 + 32:8 + 48, 12 + 32:12 + 56], before[:, :, 8 + 32:8 + 48, 12 + 32:12 + 56])
    # the known image as the window of `into` itself, every kept pixel keeping its bits
    m = torch.zeros(Hc, Wc, dtype=torch.bool, device=device)
    m[:, :20] = True
    m[20:30, :] = True
    res = []
    for devs in (None, [device] * 2, [device] * 3):
        canvas = before.clone()
        pim.sample_tiled(grid, cond_crops=crops(), into=(canvas, 8, 12), known_image=canvas[:, :, 8:8 + Hc, 12:12 + Wc], known_mask=m,
                         known_resample_times=2, devices=devs, **dict(kw, **({} if devs else dict(device=device))))
        res.append(canvas)
    assert torch.equal(res[1], res[0]) and torch.equal(res[2], res[0])
    assert torch.equal(res[0][:, :, 8:8 + Hc, 12:12 + Wc][:, :, m], before[:, :, 8:8 + Hc, 12:12 + Wc][:, :, m])


def test_fused_level_over_two_shards_is_the_level(device, level_imagen):
    from ultra_res import tiled as UT

    pim = level_imagen
    zoomed = torch.rand(1, 3, TOY_W, TOY_W, generator=H.gen(44))
    geom = _toy_geom()
    kw = dict(window=TOY_WINDOW, stages=(1, 2), sampler="dpmpp_2m", seed=21, tile_batch=7)
    want = UT.fused_level(lambda stage: pim, zoomed, geom, geom.positions, device=device, **kw)
    got = UT.fused_level(lambda stage: pim, zoomed, geom, geom.positions, devices=[device, device], **kw)
    assert got.shape == (1, 3, 176, 176) and got.device == want.device and torch.equal(got, want)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_two_distinct_devices(cascade):
    d0, d1 = torch.device("cuda", 0), torch.device("cuda", 1)
    kn, m = (t.to(d0) for t in _known((4, 2)))
    kw = dict(seed=25, sampler="dpmpp_2m", tile_batch=2, known_image=kn, known_mask=m, known_resample_times=2)
    base = cascade.sample_tiled((4, 2), device=d0, **kw)
    got = cascade.sample_tiled((4, 2), devices=[d0, d1], **kw)
    assert got.device == d0 and torch.equal(got, base)
    canvas = torch.rand(1, 3, 120, 80, generator=H.gen(3)).to(d0)
    want = canvas.clone()
    cascade.sample_tiled((3, 2), present=HOLE, tile_batch=1, seed=26, streamed=True, into=(want, 8, 12), device=d0)
    cascade.sample_tiled((3, 2), present=HOLE, tile_batch=1, seed=26, streamed=True, into=(canvas, 8, 12), devices=[d0, d1])
    assert torch.equal(canvas, want)
    with pytest.raises(ValueError, match=r"devices\[0\]"):   # refused before any forward
        cascade.sample_tiled((3, 2), present=HOLE, tile_batch=1, seed=26, streamed=True, into=(canvas, 8, 12), devices=[d1, d0])
