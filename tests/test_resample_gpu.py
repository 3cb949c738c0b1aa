"""The library's other resampling layers on the MI355X: the nearest-x2 + conv3x3 kernel of kernels_resample.hip against fp64
torch, the UNet forward and both samplers with `cross_embed_downsample=True` / `pixel_shuffle_upsample=False` against the
restatement in tests/resample_ref.py, graph / eager bit identity, a default UNet's plan through the extended
kd_unet_ext_t, and a strict ImagenTrainer.load."""
import functools

import pytest
import torch
import torch.nn.functional as F

import elucidated_ref as ER
import helpers as H
import resample_ref as RR
import self_cond_ref as SR
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

CONV_REL = 2e-6      # tests/test_kernels_gpu.py: the fp32 direct conv against fp64, relative L2
FWD_REL_L2 = 2e-5
SAMPLE_ABS = 2e-3
SWITCHES = {"cross_embed": dict(cross_embed_downsample=True), "nearest": dict(pixel_shuffle_upsample=False),
            "both": dict(cross_embed_downsample=True, pixel_shuffle_upsample=False)}


# ------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("B,Hh,Ww,Cin,Cout", [(2, 8, 8, 32, 64), (1, 4, 12, 96, 32), (3, 16, 16, 64, 128)])
def test_upsample_nearest_conv3x3_matches_fp64(device, B, Hh, Ww, Cin, Cout):
    """Dense, and into channels [0, Cout) and [32, 32 + Cout) of rows of Cout + 32 floats whose other channels must stay as
    they were.  (2, 8, 8): half a tile in x, the border taps of every phase; (1, 4, 12): half a tile in y, a partial one in
    x, three k-steps per input pixel row, one column tile; (3, 16, 16): two row tiles per image, two column tiles."""
    E = H.engine()
    lib = E.load()
    g = H.gen(Hh * Ww + Cin)
    x = torch.randn(B, Hh, Ww, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    bias = torch.randn(Cout, generator=g)
    ref = F.conv2d(F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), w.double(), bias.double(),
                   padding=1).permute(0, 2, 3, 1)
    xd, wd, bd = x.to(device), w.to(device), bias.to(device)
    y = torch.full((B, 2 * Hh, 2 * Ww, Cout), float("nan"), device=device)
    E.check(lib.kd_upsample_nearest_conv3x3_nhwc(E.ptr(xd), E.ptr(wd), E.ptr(bd), E.ptr(y), 0, 0, B, Hh, Ww, Cin, Cout,
                                                 E.current_stream()))
    e = H.rel_l2(y.cpu(), ref)
    print(f"upsample nearest conv3x3 {(B, Hh, Ww, Cin, Cout)}: rel-L2 {e:.2e}")
    assert e < CONV_REL
    ld = Cout + 32
    for off in (0, 32):
        fill = torch.randn(B, 2 * Hh, 2 * Ww, ld, generator=g)
        buf = fill.to(device)
        E.check(lib.kd_upsample_nearest_conv3x3_nhwc(E.ptr(xd), E.ptr(wd), E.ptr(bd), E.ptr(buf), ld, off, B, Hh, Ww, Cin, Cout,
                                                     E.current_stream()))
        got = buf.cpu()
        assert torch.equal(got[..., off:off + Cout], y.cpu()), off   # the same values as the dense run
        rest = [c for c in range(ld) if not off <= c < off + Cout]
        assert torch.equal(got[..., rest], fill[..., rest]), off
    # shapes the kernel does not take are refused, not run
    assert lib.kd_upsample_nearest_conv3x3_nhwc(E.ptr(xd), E.ptr(wd), E.ptr(bd), E.ptr(y), 0, 0, B, Hh, Ww, Cin - 4, Cout,
                                                E.current_stream()) != 0
    assert "multiple of 8" in lib.kd_last_error().decode()


# ------------------------------------------------------------------------------- the UNet forward
SMALL = dict(dim=32, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
             layer_cross_attns=(False, False, True))
WIDE = dict(dim=128, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
            layer_cross_attns=(False, False, True))
TEXT = dict(dim=32, dim_mults=(1, 2, 4), cond_dim=64, text_embed_dim=3, num_resnet_blocks=1, layer_attns=(False, True, True),
            layer_cross_attns=(False, True, True))


_ref_unet = functools.partial(H.ref_unet, RR.Unet)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mem", [False, True])
@pytest.mark.parametrize("sw", list(SWITCHES))
def test_unet_forward_matches_the_restatement(device, sw, mem, B):
    """memory_efficient adds the pre-downsample position (downs.L.0, three CrossEmbedLayers) and the last level's upsample
    (into the first half of the concat in front of final_res_block when init_conv_to_final_conv_residual is on)."""
    ou = _ref_unet(SMALL, seed=11, memory_efficient=mem, init_conv_to_final_conv_residual=mem, **SWITCHES[sw])
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, B, 32, seed=3))
    print(f"resample forward {sw} mem={mem} B={B}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_csv(pu, B, 32, device)
    n_up = 3 if mem else 2
    assert labels.count("upsample nearest conv3") == (n_up if "pixel_shuffle_upsample" in SWITCHES[sw] else 0)
    if "cross_embed_downsample" in SWITCHES[sw]:
        assert labels.count("conv k4 s2") == (3 if mem else 2)


def test_unet_forward_dim128_runs_the_2x2_half_where_the_plan_says(device):
    """dim 128, 64 px, batch 4.  The 2 x 2 halves have Cout / 2 = 64 and 128 columns over M = 4096 and 1024 output pixels:
    below the 64 whole tiles of 256 x 128 the bf16x3 kernel's epilogue form asks for, so the plan must have taken the generic
    conv for both (rows "conv k2 s2"), and none of the bf16x3 downsample rows ("conv k2 x3")."""
    ou = _ref_unet(WIDE, seed=12, **SWITCHES["both"])
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, 4, 64, seed=3))
    print(f"resample forward dim128 both B=4: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_csv(pu, 4, 64, device)
    assert labels.count("conv k2 s2") == 2 and labels.count("conv k4 s2") == 2 and "conv k2 x3" not in labels
    assert labels.count("upsample nearest conv3") == 2


@pytest.mark.parametrize("case", ["lowres", "self_cond", "text"])
def test_unet_forward_with_conditioning_matches_the_restatement(device, case):
    both = SWITCHES["both"]
    if case == "lowres":
        ou = _ref_unet(SMALL, lowres_cond=True, seed=13, memory_efficient=True, **both)
    elif case == "self_cond":
        ou = _ref_unet(SMALL, seed=14, self_cond=True, **both)
    else:
        ou = _ref_unet(TEXT, seed=15, text=True, **both)
    e, _ = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 32, seed=3))
    print(f"resample forward both + {case}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2


def test_default_unet_through_the_extended_ext_keeps_its_plan(device):
    """A default UNet built through kd_unet_create_ext with the two new fields zero has the launches and the bits of the
    plan kd_unet_create_shared builds."""
    lib = H.engine().load()
    ou = _ref_unet(H.UNET_KW["small2"], seed=4, lowres_cond=True)
    a, b = H.product_like(ou, device), H.product_like(ou, device)
    g = H.gen(5)
    x, t = torch.randn(2, 3, 32, 32, generator=g), torch.randn(2, generator=g)
    kw = dict(lowres_cond_img=torch.randn(2, 3, 32, 32, generator=g), lowres_noise_times=torch.full((2,), 1.5),
              cond_images=torch.rand(2, 3, 32, 32, generator=g))
    dv = {k: v.to(device) for k, v in kw.items()}
    ha = a.engine(2, 32, device, with_text=False)
    orig = lib.kd_unet_create_ext
    lib.kd_unet_create_ext = lambda cfg, arr, n, share, ext, out: lib.kd_unet_create_shared(cfg, arr, n, share, out)
    try:
        hb = b.engine(2, 32, device, with_text=False)
    finally:
        lib.kd_unet_create_ext = orig
    assert lib.kd_unet_num_launches(ha) == lib.kd_unet_num_launches(hb)
    assert torch.equal(a(x.to(device), t.to(device), **dv), b(x.to(device), t.to(device), **dv))
    assert "upsample nearest" not in H.plan_csv(a, 2, 32, device) and "conv k4 s2" not in H.plan_csv(a, 2, 32, device)


# ------------------------------------------------------------------------------- sampling
BASE = dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True), layer_cross_attns=(False, True))
SR2 = dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, memory_efficient=True, layer_attns=(False, True),
           layer_cross_attns=(False, True), init_conv_to_final_conv_residual=True)


def _cascade(device, cls_o, cls_p, seed, **kw):
    ous = [_ref_unet(BASE, seed=seed, **SWITCHES["both"]), _ref_unet(SR2, lowres_cond=True, seed=seed + 1, **SWITCHES["both"])]
    return H.imagen_pair(device, cls_o, cls_p, ous, image_sizes=(32, 64), condition_on_text=False, **kw)


def _inpaint(B, seed):
    g = H.gen(seed)
    inp = torch.rand(B, 3, 64, 64, generator=g)
    mask = torch.zeros(B, 64, 64, dtype=torch.bool)
    mask[:, 8:40, 12:60] = True
    return inp, mask


def test_ddpm_cascade_with_inpainting_matches_the_restatement(device):
    oim, pim = _cascade(device, SR.Imagen, "Imagen", 21, timesteps=(4, 4), pred_objectives=("noise", "v"))
    B = 2
    inp, mask = _inpaint(B, 3)
    nf = RS.generator_noise_fn(5)
    kw = dict(batch_size=B, inpaint_resample_times=2)
    ref = oim.sample(noise_fn=nf, inpaint_images=inp, inpaint_masks=mask, **kw)
    got = pim.sample(noise_fn=nf, inpaint_images=inp.to(device), inpaint_masks=mask.to(device), device=device, **kw).cpu()
    assert got.shape == (B, 3, 64, 64)
    err = float((got - ref).abs().max())
    print(f"resample DDPM cascade 32 -> 64, T=4, inpainting R=2: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_edm_cascade_matches_the_restatement(device):
    oim, pim = _cascade(device, ER.ElucidatedImagen, "ElucidatedImagen", 23, num_sample_steps=3)
    nf = RS.generator_noise_fn(13)
    ref = oim.sample(noise_fn=nf, batch_size=2)
    got = pim.sample(noise_fn=nf, batch_size=2, device=device).cpu()
    err = float((got - ref).abs().max())
    print(f"resample EDM cascade 32 -> 64, N=3: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_graph_equals_eager_and_table_on_equals_off(device):
    _, pim = _cascade(device, SR.Imagen, "Imagen", 25, timesteps=(4, 4), pred_objectives=("noise", "v"))
    nf = RS.generator_noise_fn(7)
    runs = {}
    for use_graph in (True, False):
        for table in (0, -1):
            pim.cond_table = table
            runs[use_graph, table] = pim.sample(noise_fn=nf, batch_size=2, use_graph=use_graph, device=device)
    base = runs[True, 0]
    for key, v in runs.items():
        assert torch.equal(v, base), key


# ------------------------------------------------------------------------------- the trainer
def test_trainer_loads_a_resample_checkpoint_strictly_and_samples_from_it(device, tmp_path, capsys):
    import imagen_pytorch as ip

    kw = dict(image_sizes=(32,), timesteps=(4,), condition_on_text=False)
    online, ema_u = _ref_unet(BASE, seed=31, **SWITCHES["both"]), _ref_unet(BASE, seed=32, **SWITCHES["both"])
    oim_online, oim_ema = RS.Imagen([online], **kw), RS.Imagen([ema_u], **kw)
    ema = {f"0.ema_model.{k}": v for k, v in ema_u.state_dict().items()}
    path = tmp_path / "ckpt.pt"
    torch.save({"model": oim_online.state_dict(), "ema": ema, "version": ip.__version__, "steps": torch.tensor([3])}, path)
    pim = ip.Imagen([ip.Unet(**online._locals)], **kw).to(device)
    trainer = ip.ImagenTrainer(imagen=pim)
    capsys.readouterr()
    trainer.load(str(path), strict=True)
    out = capsys.readouterr().out
    assert "Trying partial load" not in out and "library fork" not in out, out
    nf = RS.generator_noise_fn(11)
    ref = oim_ema.sample(noise_fn=nf, batch_size=2)
    got = trainer.sample(batch_size=2, noise_fn=nf).cpu()
    err = float((got - ref).abs().max())
    print(f"resample trainer.sample from the EMA weights: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
    assert float((ref - oim_online.sample(noise_fn=nf, batch_size=2)).abs().max()) > 10 * SAMPLE_ABS
