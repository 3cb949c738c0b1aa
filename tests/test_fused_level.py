"""The fused level without a GPU: cond_crop_maps through the pure-torch restatement of kd_tiles_cond_gather
(tests/fused_level_ref.py) against the materialised conditioning images, bit for bit, at a toy lattice and at the pipeline's
real numbers; the argument rules of sample_tiled(streamed=, cond_crops=, into=); the box of a sparse position set; and the
refusals and the empty level of ultra_res.tiled.fused_level."""
import pytest
import torch

import fused_level_ref as FR


def _G():
    from ultra_res import grid as G

    return G


def _maps(*a, **k):
    from imagen_pytorch import cond_crop_maps

    return cond_crop_maps(*a, **k)


# ------------------------------------------------------------------------------------------------ the maps
def test_maps_are_torchs_own_rounding():
    win, centre = _maps(24, 24)
    assert centre is None and win.dtype == torch.int32 and win.tolist() == list(range(24))
    win, centre = _maps(24, 16, centre_width=8)
    assert win.tolist() == [int(p * 1.5) for p in range(16)]              # floor(p 24 / 16)
    assert centre.tolist() == [8 + int(p * 1.5) // 3 for p in range(16)]   # crop at round(16 / 2) = 8, 8 -> 24 -> 16
    win, centre = _maps(1024, 1024, centre_width=161)
    assert centre[0] == 432 and centre[-1] == 432 + 160   # an odd margin, 863 / 2, rounds half to even
    with pytest.raises(ValueError, match="centre_width"):
        _maps(24, 16, centre_width=25)


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("v2", [False, True], ids=["3ch", "6ch"])
def test_restated_cond_gather_is_the_materialised_images(case, v2):
    """W 44 (shift 0 in row and column 3 fills everything) and W 45 (offset 10.5 -> 10), all 7 x 7 positions, S 24 / 16 / 8;
    mag 1 (W 1024, 166 / 124) and mag 2 (W 6400, 161 / 120) at a few positions, corners included."""
    G = _G()
    label, W, window, geom, pos, sizes = FR.cond_cases(G)[case]
    zoomed = torch.rand(1, 3, W, W, generator=torch.Generator().manual_seed(W))
    top = G.center_crop_offset(W, window)
    for S in sizes:
        want = FR.materialised(G, zoomed, geom, pos, window, S, 0.95, v2)
        win, centre = _maps(window, S, centre_width=geom.patch_width if v2 else None)
        assert int(win.min()) >= 0 and int(win.max()) < W - top
        got = FR.cond_gather(zoomed[0], FR.shifts_of(W, geom, pos), top, win, centre, 0.95)
        assert got.shape == want.shape == (len(pos), 6 if v2 else 3, S, S)
        assert torch.equal(got, want), (label, S)
        if case < 2:   # the quirk itself: a tile of row 3 is all fill, its neighbours are not
            assert bool((got[pos.index((3, 1))] == 0.95).all()) and not bool((got[pos.index((2, 1))] == 0.95).all())


# ------------------------------------------------------------------------------------------------ the argument rules
def _imagen(**kw):
    import imagen_pytorch as ip

    unets = [ip.Unet(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False,
                     cond_images_channels=3)]
    return ip.Imagen(unets, image_sizes=(16,), condition_on_text=False, timesteps=8, **kw)


def test_sample_tiled_refuses_the_new_arguments_by_name_before_it_needs_a_gpu():
    import imagen_pytorch as ip

    im = _imagen()
    img = torch.zeros(1, 3, 44, 44)
    four = [(0, 0)] * 4
    ok = ip.TileCondCrops(img, four, 24, 0.95)
    canvas = torch.zeros(1, 3, 40, 40)
    for kw, match in [
            (dict(cond_crops=ok, cond_images=torch.zeros(4, 3, 24, 24)), "cond_images or cond_crops"),
            (dict(cond_crops=(img, four, 24, 0.95)), "must be a TileCondCrops"),
            (dict(cond_crops=ip.TileCondCrops(torch.zeros(1, 3, 20, 20), four, 24, 0.95)), "narrower than window=24"),
            (dict(cond_crops=ip.TileCondCrops(torch.zeros(1, 3, 44, 40), four, 24, 0.95)), "one square image"),
            (dict(cond_crops=ip.TileCondCrops(img, four[:3], 24, 0.95)), r"shifts must be \[tiles 4\]\[2\]"),
            (dict(cond_crops=ip.TileCondCrops(img, [(0, 0, 0)] * 4, 24, 0.95)), r"shifts must be \[tiles 4\]\[2\]"),
            (dict(cond_crops=ip.TileCondCrops(img, [(0.5, 0)] * 4, 24, 0.95)), r"shifts must be \[tiles 4\]\[2\]"),
            (dict(cond_crops=ip.TileCondCrops(img, [(44, 0)] * 4, 24, 0.95)), "shifts must lie inside"),
            (dict(cond_crops=ip.TileCondCrops(img, four, 24, 0.95, centre_width=30)), "centre_width"),
            (dict(into=(canvas, 0, 0)), "needs streamed=True"),
            (dict(streamed=True, into=canvas), r"into must be \(canvas"),
            (dict(streamed=True, into=(canvas.double(), 0, 0)), "must be float32"),
            (dict(streamed=True, into=(canvas[0], 0, 0)), r"contiguous \[1, 3, Ho, Wo\]"),
            (dict(streamed=True, into=(torch.zeros(1, 4, 40, 40), 0, 0)), r"contiguous \[1, 3, Ho, Wo\]"),
            (dict(streamed=True, into=(canvas, 0, 2)), "multiples of 4"),
            (dict(streamed=True, into=(canvas, 2, 0)), "multiples of 4"),
            (dict(streamed=True, into=(torch.zeros(1, 3, 40, 42), 0, 0)), "multiples of 4"),
            (dict(streamed=True, into=(canvas, 16, 0)), "out of bounds"),    # the 28 x 28 canvas ends at row 44
            (dict(streamed=True, into=(canvas, 0, -4)), "out of bounds"),
            (dict(streamed=True, into=(canvas, 12, 12)), "must live on the device"),   # in bounds: only the place is wrong
    ]:
        with pytest.raises(ValueError, match=match):
            im.sample_tiled((2, 2), **kw)
    if not torch.cuda.is_available():   # what passes the checks reaches the engine: there is no CPU path
        for kw in (dict(streamed=True), dict(cond_crops=ok), dict(cond_crops=ok, streamed=True)):
            with pytest.raises(ip._engine.EngineUnavailable):
                im.sample_tiled((2, 2), seed=3, **kw)


def test_normalize_into_is_a_function_of_its_arguments():
    """The rules of `into` by themselves, in their order: None passes whatever `streamed` is, `streamed` is asked for
    before the triple is looked at, and the place is the last rule - a host canvas that meets every other one."""
    from imagen_pytorch.imagen_pytorch import normalize_into

    size = dict(channels=3, Hc=28, Wc=28, unet=1)
    canvas = torch.zeros(1, 3, 40, 40)
    assert normalize_into(None, streamed=False, **size) is None and normalize_into(None, streamed=True, **size) is None
    with pytest.raises(ValueError, match="needs streamed=True"):
        normalize_into("not a triple", streamed=False, **size)
    with pytest.raises(ValueError, match=r"the offset \(oy, ox\) must be two ints, got \(4, 4.0\)"):
        normalize_into((canvas, 4, 4.0), streamed=True, **size)
    with pytest.raises(ValueError, match="the 28 x 28 canvas of unet 1 at \\(16, 0\\) is out of bounds of the 40 x 40 canvas"):
        normalize_into((canvas, 16, 0), streamed=True, **size)
    with pytest.raises(ValueError, match="must live on the device, got cpu"):
        normalize_into([canvas, 12, 12], streamed=True, **size)
    if torch.cuda.is_available():
        dst = canvas.cuda()
        got = normalize_into((dst, torch.tensor(12).item(), 8), streamed=True, **size)
        assert got[0] is dst and got[1:] == (12, 8) and all(type(v) is int for v in got[1:])


# ------------------------------------------------------------------------------------------------ the level driver
def test_the_box_of_a_sparse_position_set():
    from ultra_res import tiled as UT

    r0, c0, grid, present, tiles = UT.level_box([(3, 3), (2, 4), (2, 3), (2, 4)])
    assert (r0, c0, grid) == (2, 3, (2, 2)) and present == [[True, True], [True, False]]
    assert tiles == [(2, 3), (2, 4), (3, 3)]   # row-major, no repeats: the numbering of normalize_tiling
    r0, c0, grid, present, tiles = UT.level_box([(30, 7), (28, 9)])
    assert (r0, c0, grid) == (28, 7, (3, 3)) and sum(map(sum, present)) == 2 and present[0][2] and present[2][0]
    assert UT.level_box([(5, 5)])[:4] == (5, 5, (1, 1), [[True]])
    with pytest.raises(ValueError, match="no positions"):
        UT.level_box([])


def _no_model(stage):
    raise AssertionError("no model may be loaded for this call")


def test_a_level_without_positions_is_the_enlarged_background_and_never_reaches_the_engine(monkeypatch):
    from imagen_pytorch import _engine
    from ultra_res import tiled as UT

    for name in ("load", "require_gpu"):
        monkeypatch.setattr(_engine, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError(f"_engine.{name} was called")))
    G = _G()
    geom = G.GridGeometry(8, 6, 7, 24, 176)
    zoomed = torch.rand(1, 3, 44, 44, generator=torch.Generator().manual_seed(2))
    got = UT.fused_level(_no_model, zoomed, geom, [], window=24, device="cpu")
    want = torch.nn.functional.interpolate(zoomed, size=(176, 176), mode="bilinear", align_corners=False)
    assert torch.equal(got, want)
    assert torch.equal(UT.fused_level(_no_model, zoomed, geom, [], window=24, device="cpu", background=False), torch.zeros_like(want))


def test_fused_level_refuses_by_name_before_it_needs_a_gpu():
    from ultra_res import tiled as UT

    G = _G()
    zoomed = torch.rand(1, 3, 44, 44)
    cpu = []

    def one(stage):   # the geometry is refused before the model moves to a device
        cpu.append(_imagen())
        return cpu[-1]

    pos = [(2, 3), (2, 4), (3, 3)]
    with pytest.raises(ValueError, match="stages"):
        UT.fused_level(_no_model, zoomed, G.GridGeometry(8, 6, 7, 12, 88), pos, stages=(2,), window=24)
    with pytest.raises(ValueError, match="inside the 7 x 7 grid"):
        UT.fused_level(_no_model, zoomed, G.GridGeometry(8, 6, 7, 12, 88), [(2, 7)], stages=(1,), window=24)
    with pytest.raises(ValueError, match="one square image"):
        UT.fused_level(_no_model, zoomed[0], G.GridGeometry(8, 6, 7, 12, 88), pos, stages=(1,), window=24)
    # a tile of 16 at overlap 0.25 strides 12: seven of them span 6 * 12 + 16 = 88
    for geom, match in ((G.GridGeometry(8, 6, 7, 24, 176), "out_patch_dist=24"), (G.GridGeometry(8, 6, 7, 12, 100), "canvas_width=100"),
                        (G.GridGeometry(8, 6, 8, 12, 88), "8 patches wide")):
        with pytest.raises(ValueError, match=f"geom .*{match}.* is not the lattice of unet 1: stride st=12"):
            UT.fused_level(one, zoomed, geom, pos, stages=(1,), window=24)
    with pytest.raises(ValueError, match="the Imagen holds 1"):
        UT.fused_level(one, zoomed, G.GridGeometry(8, 6, 7, 12, 88), pos, stages=(1, 2), window=24)
    with pytest.raises(ValueError, match="narrower than window=64"):
        UT.fused_level(one, zoomed, G.GridGeometry(8, 6, 7, 12, 88), pos, stages=(1,), window=64)
    assert cpu and all(p.device.type == "cpu" for im in cpu for p in im.parameters())
