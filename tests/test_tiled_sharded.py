"""A fused-tile canvas over several shards, without a GPU: the decomposition (normalize_shards) against a brute-force cover
computation, its refusals and those of normalize_devices, the real mag-2 geometry, and the restatement
tests/tiled_sharded_ref.py - every shard seeing NaN wherever the decomposition promises it nothing - against the unsharded
restatement tests/tiled_known_ref.py, bit for bit."""
import pytest
import torch

import tiled_known_ref as KR
import tiled_sharded_ref as SR
from oracle import sampler_ref as RS
from test_tiled import _gauss_denoiser

HOLE = [[True, True], [True, False], [True, True]]
EMPTY_ROW = [[True, True, True], [True, False, True], [False, False, False], [True, True, False], [False, True, True]]


def _np():
    from imagen_pytorch.imagen_pytorch import normalize_devices, normalize_shards, normalize_tiling

    return normalize_tiling, normalize_shards, normalize_devices


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_decomposition_names_what_it_refuses():
    tiling_of, shards_of, devices_of = _np()
    t = tiling_of((16,), (3, 2), present=HOLE)
    with pytest.raises(ValueError, match="4 shards are more than the 3 lattice rows that hold a present tile"):
        shards_of(t, 4)
    with pytest.raises(ValueError, match="3 shards are more than the 2 lattice rows that hold a present tile"):
        shards_of(tiling_of((16,), (3, 2), present=[[True, True], [False, False], [True, True]]), 3)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="n_shards must be an int >= 1"):
            shards_of(t, bad)
    e = tiling_of((16,), (5, 3), present=EMPTY_ROW)
    with pytest.raises(ValueError, match=r"the band of lattice rows \[2, 3\) holds no present tile"):
        shards_of(e, 3, bands=[(0, 2), (2, 3), (3, 5)])
    with pytest.raises(ValueError, match="bands must be 2 ranges"):
        shards_of(e, 2, bands=[(0, 2), (3, 5)])
    with pytest.raises(ValueError, match="is not a CUDA device"):
        devices_of(["cuda:0", "cpu"])
    with pytest.raises(ValueError, match="is not a CUDA device"):
        devices_of([torch.device("cpu")])
    for bad in (["cuda:0", 1.5], [None], ["cuda:0", "gpu-zero"], [True], [object()]):
        with pytest.raises(ValueError, match="is not a device"):
            devices_of(bad)
    for bad in ("cuda:0", torch.device("cuda:0"), [], 3):
        with pytest.raises(ValueError, match="devices must be a non-empty sequence"):
            devices_of(bad)
    with pytest.raises(ValueError, match="devices or noise_fn, one of them"):
        devices_of(["cuda:0", "cuda:0"], noise_fn=lambda tag, shape: None)
    assert devices_of(None) is None and devices_of(["cuda:0"], noise_fn=print) == [torch.device("cuda:0")]
    assert devices_of(["cuda:1", 0, torch.device("cuda", 2)]) == [torch.device("cuda", i) for i in (1, 0, 2)]


def _imagen():
    import imagen_pytorch as ip

    unets = [ip.Unet(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False)]
    return ip.Imagen(unets, image_sizes=(16,), condition_on_text=False, timesteps=8)


def test_sample_tiled_takes_devices_and_refuses_them_by_name_before_it_needs_a_gpu():
    """`devices=` is the new argument: on the code before it this call is a TypeError."""
    import imagen_pytorch as ip
    from ultra_res import tiled as UT

    im = _imagen()
    for kw, match in [
            (dict(devices=["cuda:0", "cpu"]), "is not a CUDA device"),
            (dict(devices=["cuda:0", 2.5]), "is not a device"),
            (dict(devices="cuda:0"), "devices must be a non-empty sequence"),
            (dict(devices=["cuda:0"] * 3), "3 shards are more than the 2 lattice rows"),
            (dict(devices=["cuda:0"] * 2, noise_fn=RS.generator_noise_fn(1)), "devices or noise_fn"),
    ]:
        with pytest.raises(ValueError, match=match):
            im.sample_tiled((2, 2), **kw)
    with pytest.raises(ValueError, match="3 shards are more than the 2 lattice rows"):
        UT.fused_canvas(lambda stage: im, num_patches_width=2, stages=(1,), devices=["cuda:0"] * 3)
    if not torch.cuda.is_available():   # what passes the checks reaches the engine: there is no CPU path
        with pytest.raises(ip._engine.EngineUnavailable):
            im.sample_tiled((2, 2), seed=3, devices=["cuda:0", "cuda:0"])


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("S,overlap,d", [(16, 0.25, 1), (16, 0.5, 1), (20, 0.6, 2)])
def test_halo_depth(S, overlap, d):
    tiling_of, shards_of, _ = _np()
    plan = shards_of(tiling_of((S,), (5, 2), overlap=overlap), 2)[0]
    assert plan["d"] == d


def _check_plan(geo, plan, n):
    S, st, ny, Hc = geo["S"], geo["st"], geo["ny"], geo["Hc"]
    shards = plan["shards"]
    assert len(shards) == n
    bands = [sh["band"] for sh in shards]
    assert bands[0][0] == 0 and bands[-1][1] == ny and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
    owned = [sh["owned"] for sh in shards]
    assert owned[0][0] == 0 and owned[-1][1] == Hc and all(a[1] == b[0] for a, b in zip(owned, owned[1:]))
    present = sorted(t for row in geo["tile_of"] for t in row if t >= 0)
    assert sorted(t for sh in shards for t in sh["own"]) == present   # every present tile is owned once
    owner = {t: i for i, sh in enumerate(shards) for t in sh["own"]}
    sent = {}
    for e in plan["exchange"]:
        for t, row0, rows in e["items"]:
            assert owner[t] == e["src"] and e["src"] != e["dst"] and (e["dst"], t) not in sent
            sent[(e["dst"], t)] = (row0, rows)
    for i, sh in enumerate(shards):
        r0, r1 = sh["band"]
        assert sh["own"] and sh["own"] == [t for r in range(r0, r1) for t in geo["tile_of"][r] if t >= 0]
        assert sh["extent"] == (r0 * st, (r1 - 1) * st + S) and sh["owned"][0] == r0 * st
        assert sh["extent"][0] <= sh["owned"][0] and sh["owned"][1] <= sh["extent"][1]
        extent, need = SR.brute_cover(geo, sh["band"])
        assert extent == sh["extent"]
        assert sorted(need) == sh["halo"] and not set(sh["halo"]) & set(sh["own"])
        for t, local in need.items():   # the strip is exactly the rows of the tile that lie inside the extent
            row0, rows = sh["strips"][t]
            assert local == list(range(row0, row0 + rows)) and sent[(i, t)] == (row0, rows)
        assert sum(1 for (dst, _) in sent if dst == i) == len(sh["halo"])
        # the store: own and halo in canvas order, the own tiles contiguous from `base`, tile_of for exactly that set
        assert sh["tiles"] == sorted(sh["own"] + sh["halo"])
        assert sh["tiles"][sh["base"]:sh["base"] + len(sh["own"])] == sh["own"]
        for r in range(ny):
            for q, t in enumerate(geo["tile_of"][r]):
                assert sh["tile_of"][r][q] == (sh["tiles"].index(t) if t in sh["tiles"] else -1)


@pytest.mark.parametrize("grid,present,overlap,shards", [
    ((2, 2), None, 0.25, (1, 2)), ((3, 2), HOLE, 0.25, (1, 2, 3)), ((5, 3), None, 0.25, (1, 2, 3, 5)),
    ((5, 3), None, 0.5, (2, 4)), ((5, 3), EMPTY_ROW, 0.25, (1, 2, 3, 4)), ((5, 2), None, 0.6, (2, 3, 5)),
    ((5, 3), EMPTY_ROW, 0.6, (2, 4))])
def test_bands_halos_and_strips_against_the_brute_force_cover(grid, present, overlap, shards):
    tiling_of, shards_of, _ = _np()
    S = 20 if overlap == 0.6 else 16
    tiling = tiling_of((S, 2 * S), grid, overlap=overlap, present=present)
    for n in shards:
        plans = shards_of(tiling, n)
        assert len(plans) == 2
        for geo, plan in zip(tiling, plans):
            _check_plan(geo, plan, n)
        assert [sh["band"] for sh in plans[0]["shards"]] == [sh["band"] for sh in plans[1]["shards"]]


def test_bands_are_balanced_by_present_tiles():
    tiling_of, shards_of, _ = _np()
    present = [[True] * 6, [True] + [False] * 5, [True] + [False] * 5, [True] + [False] * 5, [True] * 3 + [False] * 3]
    plan = shards_of(tiling_of((16,), (5, 6), present=present), 2)[0]
    assert [sh["band"] for sh in plan["shards"]] == [(0, 1), (1, 5)] and [len(sh["own"]) for sh in plan["shards"]] == [6, 6]
    plan = shards_of(tiling_of((16,), (5, 3), present=EMPTY_ROW), 4)[0]
    assert all(sh["own"] for sh in plan["shards"]) and max(len(sh["own"]) for sh in plan["shards"]) == 3


SCATTERED = [[(3 * r + 5 * q) % 7 not in (0, 3) for q in range(7)] for r in range(5)]   # 5 x 7, two holes in every row


@pytest.mark.parametrize("grid,present", [((4, 2), None), ((3, 2), HOLE), ((1, 1), None), ((5, 7), SCATTERED)])
def test_one_shard_is_the_whole_lattice(grid, present):
    """What sample_tiled(devices=None) rests on: at every stage, the one shard of normalize_shards(tiling, 1) owns every
    tile in canvas order from slot 0 of its store, has no halo and nothing to trade, ends every canvas row, and its
    `tile_of` is the tiling's own."""
    tiling_of, shards_of, _ = _np()
    if present is SCATTERED:
        assert all(sum(row) == 5 for row in SCATTERED) and len({tuple(row) for row in SCATTERED}) == 5
    tiling = tiling_of((16, 32, 64), grid, present=present)
    plans = shards_of(tiling, 1)
    assert len(plans) == len(tiling) == 3
    for geo, plan in zip(tiling, plans):
        (sh,) = plan["shards"]
        every = list(range(len(geo["origins"])))
        assert sh["own"] == every and sh["tiles"] == every and sh["base"] == 0 and sh["halo"] == []
        assert sh["owned"] == (0, geo["Hc"])
        assert sh["tile_of"] == geo["tile_of"]
        assert plan["exchange"] == []


def test_the_mag_2_level_over_8_shards():
    """53 x 53 slots of 1024^2 at stride 768 (the last stage of a mag-2 level), every slot present and a disc of tissue, over
    8 shards: every present tile is owned once, the bands hold 6 or 7 rows of the full lattice, the halo is one lattice row
    deep and every strip is the 256 rows of the overlap.  What a shard RECEIVES per schedule step on the full lattice at
    C = 3: 53 strips of 3 x 256 x 1024 fp32 and 53 thresholds from either neighbour - 166.7 MB for the first and the last
    shard, 333.4 MB for the six between them (the disc: 116.4 MB to 302.0 MB) - against 7 x 53 x 3 x 1024 x 1024 x 4 B =
    4.7 GB of tile estimates the shard's own forwards write in that step."""
    tiling_of, shards_of, _ = _np()
    disc = [[(r - 26) ** 2 + (q - 26) ** 2 <= 24 ** 2 for q in range(53)] for r in range(53)]
    seen = {}
    for name, present in (("full", None), ("disc", disc)):
        tiling = tiling_of((64, 256, 1024), (53, 53), overlap=0.25, present=present)
        geo, plan = tiling[2], shards_of(tiling, 8)[2]
        assert (geo["S"], geo["st"], geo["Hc"]) == (1024, 768, 40960) and plan["d"] == 1
        _check_plan(geo, plan, 8)
        assert all(rows == 256 for sh in plan["shards"] for _, rows in sh["strips"].values())
        got = [0] * 8
        for e in plan["exchange"]:
            assert abs(e["src"] - e["dst"]) == 1
            got[e["dst"]] += sum(3 * rows * 1024 * 4 + 4 for _, _, rows in e["items"])
        seen[name] = got
        loads = [len(sh["own"]) for sh in plan["shards"]]
        print(f"mag-2 {name}: bands {[sh['band'] for sh in plan['shards']]}, tiles {loads}, received MB/step "
              f"{[round(b / 1e6, 1) for b in got]}")
        if present is None:
            assert sorted(set(loads)) == [6 * 53, 7 * 53]
        else:
            assert max(loads) - min(loads) <= 53 and max(loads) <= -(-sum(loads) // 8) + 53
    assert seen["full"][0] == seen["full"][7] == 53 * (3 * 256 * 1024 * 4 + 4) and seen["full"][3] == 2 * seen["full"][0]
    assert round(seen["full"][0] / 1e6, 1) == 166.7 and round(seen["full"][3] / 1e6, 1) == 333.4
    assert (round(min(seen["disc"]) / 1e6, 1), round(max(seen["disc"]) / 1e6, 1)) == (116.4, 302.0)


# ------------------------------------------------------------------------------------------------ the restatement
CASES = [
    dict(name="ddpm"), dict(name="ddim", eta=0.5), dict(name="dpmpp_2m"),
    dict(name="dpmpp_2m", weights="ramp"), dict(name="ddim", eta=0.5, weights="ramp"),
    dict(name="dpmpp_2m", known=True, R=2), dict(name="ddpm", known=True, R=2), dict(name="ddim", eta=0.5, known=True, R=2),
    dict(name="dpmpp_2m", skip=3), dict(name="ddim", eta=0.5, skip=3, known=True, R=2, weights="ramp"),
]
_ids = lambda c: "-".join(f"{k}={v}" for k, v in c.items())


@pytest.fixture(scope="module")
def unsharded():
    """The unsharded restatement of every (case, lattice), computed once."""
    return {}


@pytest.mark.parametrize("grid,present,overlap", [((4, 2), None, 0.25), ((3, 2), HOLE, 0.25), ((4, 2), None, 0.6)],
                         ids=["4x2", "3x2-hole", "4x2-halo-2"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_sharded_restatement_is_the_unsharded_one(unsharded, case, grid, present, overlap):
    """1, 2 and 3 shards: the canvas assembled from the owned rows is torch.equal to tiled_known_ref.run_canvas with the
    pointwise Gaussian denoiser of tests/test_tiled.py; every shard's canvas is exact on its whole band extent and NaN
    outside it, so nothing outside a received strip reached an owned pixel."""
    tiling_of, shards_of, _ = _np()
    S = 20 if overlap == 0.6 else 16
    name, eta, weights = case["name"], case.get("eta", 0.0), case.get("weights", "uniform")
    R, skip = case.get("R", 1), case.get("skip", 0)
    sched = RS.GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=8)
    lat = KR.lattice(S, grid, overlap, present)
    tiling = tiling_of((S,), grid, overlap=overlap, present=present, tile_weights=weights)
    assert tiling[0]["origins"] == lat["origins"]
    nf = RS.generator_noise_fn(7)
    den = _gauss_denoiser(sched)
    denoise = lambda k, t, tn, tiles, prev: den(t, tiles)
    shape = (1, 3, lat["Hc"], lat["Wc"])
    x_T = nf(("init", 1), shape)
    if skip:
        x_T = x_T + (torch.rand(shape, generator=torch.Generator().manual_seed(3)) * 2 - 1)
    known = mask = None
    if case.get("known"):
        known = torch.rand(shape, generator=torch.Generator().manual_seed(5))
        mask = torch.zeros(shape[2:], dtype=torch.bool)
        mask[:, :10] = True
        mask[lat["st"] - 2:lat["st"] + 6, :] = True   # across the first seam between lattice rows
    key = (_ids(case), grid, overlap)
    if key not in unsharded:
        unsharded[key] = KR.run_canvas(denoise, x_T, lat, sched, name, eta, nf, 1, weights, known, mask, R, skip)
    want, covered = unsharded[key]
    assert bool(torch.isfinite(want).all()) and float(want.std()) > 0.1
    for n in (1, 2, 3):
        plan = shards_of(tiling, n)[0]
        got, cov, xs = SR.run_canvas_sharded(denoise, x_T, lat, plan, sched, name, eta, nf, 1, weights, known, mask, R, skip)
        assert torch.equal(cov, covered) and torch.equal(got, want), (n, float((got - want).abs().nan_to_num(9.0).max()))
        for sh, xi in zip(plan["shards"], xs):
            e0, e1 = sh["extent"]
            assert torch.equal(xi[:, :, e0:e1], want[:, :, e0:e1])
            assert bool(torch.isnan(xi[:, :, :e0]).all()) and bool(torch.isnan(xi[:, :, e1:]).all())
