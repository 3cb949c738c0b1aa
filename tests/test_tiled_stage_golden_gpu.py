"""Imagen.sample_tiled pinned to bits: one SHA-256 of the returned canvas per case of CASES, recorded on the MI355X by
tests/golden/make_tiled_stage_digests.py at the commit before the stage driver moved out of Imagen._tiled_stage into
imagen_pytorch/_canvas.py (tests/golden/tiled_stage_digests.json).  tests/golden/tiled_seed5_2x2.pt pins plain calls
only; known pixels, image starts, the third-order ring, streamed stages, cond_crops, `into`, injected noise and shards are
otherwise held to restatements within a tolerance or to "sharded equals unsharded", which holds as well when both sides
change together.

The models are the smallest of tests/test_tiled_sharded_gpu.py: its 16 -> 32 `small1` cascade (tiles 16 and 32, strides
12 and 24), the same with cond_images_channels=3, the self-conditioned and the text model.  Arguments are public ones
only, rebuilt here from seeds; the file holds results alone."""
import hashlib
import json
import pathlib

import pytest
import torch

import helpers as H
import self_cond_ref as SC
import test_tiled_sharded_gpu as TS
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).parent / "golden" / "tiled_stage_digests.json"
INTO_AT = (8, 12)

# name: model, lattice of TS.LATTICES, tile_batch, sample_tiled keywords, and what run_case builds from seeds:
# known = R (known image and mask, known_resample_times=R), init = init_skip_steps (init_canvas), text, cond_images,
# crops (cond_crops, streamed, into at INTO_AT; the known image is then the written window of `into`), noise_fn
CASES = {
    "a_4x2_batch2_2m_ramp_known": dict(model="cascade", lattice="4x2", tile_batch=2, known=2,
                                       kw=dict(sampler="dpmpp_2m", tile_weights="ramp")),
    "b_hole_batch1_ddpm_known_init_streamed": dict(model="cascade", lattice="3x2-hole", tile_batch=1, known=2, init=3,
                                                   kw=dict(streamed=True)),
    "c_hole_batch3_ragged_3m": dict(model="cascade", lattice="3x2-hole", tile_batch=3, kw=dict(sampler="dpmpp_3m")),
    "d_4x2_3m_sde_known": dict(model="cascade", lattice="4x2", tile_batch=2, known=2, kw=dict(sampler="dpmpp_3m_sde")),
    "e_self_cond_2m_known": dict(model="self_cond", lattice="4x2", tile_batch=2, known=2, kw=dict(sampler="dpmpp_2m")),
    "f_text_ddim_eta_guidance": dict(model="text", lattice="4x2", tile_batch=2, text=True,
                                     kw=dict(sampler="ddim", sampler_eta=0.5, cond_scale=3.0)),
    "g_crops_streamed_into_known_window": dict(model="level", lattice="4x2", tile_batch=2, known=2, crops=True,
                                               kw=dict(sampler="dpmpp_2m", streamed=True)),
    "h_cond_images_no_graph": dict(model="level", lattice="4x2", tile_batch=2, cond_images=True,
                                   kw=dict(sampler="dpmpp_2m", use_graph=False)),
    "i_case_b_with_noise_fn": dict(model="cascade", lattice="3x2-hole", tile_batch=1, known=2, init=3, noise_fn=True,
                                   kw=dict(streamed=True)),
}
SHARDED = {"j_case_a_three_shards": "a_4x2_batch2_2m_ramp_known", "j_case_g_three_shards": "g_crops_streamed_into_known_window"}
SEED = 41


def build_model(kind, device):
    if kind == "cascade":
        return TS._product(device)
    if kind == "level":
        return TS._product(device, TS._unets(cond_images_channels=3))
    single = dict(image_sizes=(16,), timesteps=(TS.N,))
    if kind == "self_cond":
        kw = dict(single, pred_objectives=("noise",), condition_on_text=False)
        ou = H.ref_unet(SC.Unet, H.UNET_KW["small1"], seed=21, self_cond=True)
    else:
        kw = dict(single, text_embed_dim=3)
        ou = H.ref_unet(R.Unet, dict(H.UNET_KW["small1"], cond_dim=64, text_embed_dim=3), seed=17, text=True)
    return H.product_imagen(RS.Imagen([ou], **kw), "Imagen", device, **kw)


def run_case(name, pim, device, shards=None):
    """The canvas the case returns (with crops: the whole `into` canvas)."""
    import fused_level_ref as FR
    import imagen_pytorch as ip

    case = CASES[name]
    grid, present = TS.LATTICES[case["lattice"]]
    kw = dict(case["kw"], present=present, tile_batch=case["tile_batch"], seed=SEED)
    kw.update(dict(device=device) if shards is None else dict(devices=[device] * shards))
    S = pim.image_sizes[-1]
    Hc, Wc = ((n - 1) * (S * 3 // 4) + S for n in grid)
    kn, m = TS._known(grid)
    kn, m = (kn[:, :, :Hc, :Wc], m[:Hc, :Wc]) if S == 32 else (kn[:, :, ::2, ::2][:, :, :Hc, :Wc], m[::2, ::2][:Hc, :Wc])
    kn, m = kn.contiguous().to(device), m.contiguous().to(device)
    assert tuple(kn.shape[-2:]) == (Hc, Wc) == tuple(m.shape)
    if case.get("crops"):
        pos = [(i, j) for i in range(grid[0]) for j in range(grid[1]) if present is None or present[i][j]]
        zoomed = torch.rand(1, 3, TS.TOY_W, TS.TOY_W, generator=H.gen(44))
        canvas = torch.rand(1, 3, Hc + 20, Wc + 24, generator=H.gen(2)).to(device)
        oy, ox = INTO_AT
        kn = canvas[:, :, oy:oy + Hc, ox:ox + Wc]
        kw.update(cond_crops=ip.TileCondCrops(zoomed, FR.shifts_of(TS.TOY_W, TS._toy_geom(), pos), TS.TOY_WINDOW, 0.95),
                  into=(canvas, oy, ox))
    if case.get("known"):
        kw.update(known_image=kn, known_mask=m, known_resample_times=case["known"])
    if case.get("init"):
        kw.update(init_canvas=torch.rand(1, 3, Hc, Wc, generator=H.gen(32)).to(device), init_skip_steps=case["init"])
    if case.get("text"):
        kw.update(text_embeds=torch.randn(1, 2, 3, generator=H.gen(4)).to(device))
    if case.get("cond_images"):
        n_tiles = sum(1 for i in range(grid[0]) for j in range(grid[1]) if present is None or present[i][j])
        kw.update(cond_images=torch.rand(n_tiles, 3, 16, 16, generator=H.gen(8)).to(device))
    if case.get("noise_fn"):
        kw.update(noise_fn=RS.generator_noise_fn(SEED))   # a generator per tag: init, lowres, inpaint, renoise, step
    out = pim.sample_tiled(grid, **kw)
    if case.get("crops"):
        assert out is canvas
    assert bool(torch.isfinite(out).all()) and float(out.std()) > 0.01
    return out


def digest(t):
    assert t.dtype == torch.float32
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def models(device):
    return {kind: build_model(kind, device) for kind in sorted({c["model"] for c in CASES.values()})}


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("name", list(CASES))
def test_canvas_keeps_the_recorded_bits(device, models, golden, name):
    got = digest(run_case(name, models[CASES[name]["model"]], device))
    assert got == golden[name], f"{name}: the canvas is not the recorded one ({got} != {golden[name]})"


@pytest.mark.parametrize("name", list(SHARDED))
def test_three_shards_give_the_unsharded_digest(device, models, golden, name):
    base = SHARDED[name]
    got = digest(run_case(base, models[CASES[base]["model"]], device, shards=3))
    assert golden[name] == golden[base], f"{name}: recorded apart from {base}"
    assert got == golden[base], f"{name}: three shards do not give the canvas of {base} ({got} != {golden[base]})"
