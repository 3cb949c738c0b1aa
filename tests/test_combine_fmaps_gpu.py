"""`Unet(combine_upsample_fmaps=True)` on the MI355X: the nearest-x-s + [GroupNorm affine + SiLU] + conv3x3 kernel of
kernels_upcombine.hip against fp64 torch, the UNet forward and both samplers against the restatement in
tests/combine_fmaps_ref.py, graph / eager bit identity, a default UNet's plan through kd_unet_create_ext2, and a strict
ImagenTrainer.load."""
import functools

import pytest
import torch
import torch.nn.functional as F

import combine_fmaps_ref as CR
import elucidated_ref as ER
import helpers as H
import self_cond_ref as SR
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

CONV_REL = 2e-6      # tests/test_kernels_gpu.py: the fp32 direct conv against fp64, relative L2
FWD_REL_L2 = 2e-5
SAMPLE_ABS = 2e-3
COMBINE = dict(combine_upsample_fmaps=True)


# ------------------------------------------------------------------------------- the kernel
SHAPES = [(2, 3, 5, 32, 64, 4),     # partial tile both ways; every border class
          (1, 1, 1, 16, 32, 4),     # every neighbour tap is padding
          (1, 8, 16, 64, 32, 8),    # exactly one tile; one column tile
          (3, 9, 17, 40, 96, 2),    # empty interior classes; two tiles each way; three column tiles; five k-steps
          (2, 2, 3, 16, 32, 16)]    # largest scale


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("B,Hh,Ww,Cin,Cout,s", SHAPES)
def test_upsample_nearest_gn_conv3x3_matches_fp64(device, B, Hh, Ww, Cin, Cout, s, affine):
    """Against F.conv2d(F.silu(F.group_norm(F.interpolate(x, scale_factor=s)))) in fp64.  With the affine the kernel gets the
    raw map and [B][Cin][2] = (A, B) kd_wf_ab_scale() of GroupNorm(8) from the LOW-RES statistics (kd_gn_fold_seg's form);
    without it, the map already activated at low resolution.  beta is random, so SiLU(B) != 0 where a tap is padding.
    Dense, and into channels [0, Cout) and [32, 32 + Cout) of rows of Cout + 32 floats whose other channels must stay."""
    E = H.engine()
    lib = E.load()
    g = H.gen(Hh * Ww + Cin + s)
    x = torch.randn(B, Hh, Ww, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    bias = torch.randn(Cout, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(Cin, generator=g), torch.randn(Cin, generator=g)
    x64 = x.double().permute(0, 3, 1, 2)
    up = F.interpolate(x64, scale_factor=s, mode="nearest")
    ref = F.conv2d(F.silu(F.group_norm(up, 8, gamma.double(), beta.double())), w.double(), bias.double(),
                   padding=1).permute(0, 2, 3, 1)
    if affine:
        xg = x64.reshape(B, 8, -1)
        mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
        rstd = (var + 1e-5).rsqrt()
        a = rstd.repeat_interleave(Cin // 8, 1) * gamma.double()                  # [B][Cin]
        b = beta.double() - mean.repeat_interleave(Cin // 8, 1) * a
        ab = (torch.stack((a, b), -1) * float(lib.kd_wf_ab_scale())).float().contiguous().to(device)
        src, abp = x.to(device), E.ptr(ab)
    else:
        src = F.silu(F.group_norm(x64, 8, gamma.double(), beta.double())).permute(0, 2, 3, 1).float().contiguous().to(device)
        abp = None
    wd, bd = w.to(device), bias.to(device)
    y = torch.full((B, s * Hh, s * Ww, Cout), float("nan"), device=device)
    E.check(lib.kd_upsample_nearest_gn_conv3x3_nhwc(E.ptr(src), 0, abp, E.ptr(wd), E.ptr(bd), E.ptr(y), 0, 0, B, Hh, Ww, Cin, Cout, s,
                                                    E.current_stream()))
    e = H.rel_l2(y.cpu(), ref)
    print(f"upsample nearest gn conv3x3 {(B, Hh, Ww, Cin, Cout, s)} affine={affine}: rel-L2 {e:.2e}")
    assert e < CONV_REL
    ld = Cout + 32
    for off in (0, 32):
        fill = torch.randn(B, s * Hh, s * Ww, ld, generator=g)
        buf = fill.to(device)
        E.check(lib.kd_upsample_nearest_gn_conv3x3_nhwc(E.ptr(src), 0, abp, E.ptr(wd), E.ptr(bd), E.ptr(buf), ld, off, B, Hh, Ww, Cin,
                                                        Cout, s, E.current_stream()))
        got = buf.cpu()
        assert torch.equal(got[..., off:off + Cout], y.cpu()), off   # the same values as the dense run
        rest = [c for c in range(ld) if not off <= c < off + Cout]
        assert torch.equal(got[..., rest], fill[..., rest]), off
    # shapes the kernel does not take are refused, not run
    assert lib.kd_upsample_nearest_gn_conv3x3_nhwc(E.ptr(src), 0, abp, E.ptr(wd), E.ptr(bd), E.ptr(y), 0, 0, B, Hh, Ww, Cin - 4, Cout, s,
                                                   E.current_stream()) != 0
    assert "multiple of 8" in lib.kd_last_error().decode()
    assert lib.kd_upsample_nearest_gn_conv3x3_nhwc(E.ptr(src), 0, abp, E.ptr(wd), E.ptr(bd), E.ptr(y), 0, 0, B, Hh, Ww, Cin, Cout, 1,
                                                   E.current_stream()) != 0
    assert "scale" in lib.kd_last_error().decode()


# ------------------------------------------------------------------------------- the UNet forward
SMALL = dict(dim=32, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
             layer_cross_attns=(False, False, True))
WIDE = dict(dim=128, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
            layer_cross_attns=(False, False, True))
TEXT = dict(dim=32, dim_mults=(1, 2, 4), cond_dim=64, text_embed_dim=3, num_resnet_blocks=1, layer_attns=(False, True, True),
            layer_cross_attns=(False, True, True))


_ref_unet = functools.partial(H.ref_unet, CR.Unet, **COMBINE)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("mem", [False, True])
def test_unet_forward_matches_the_restatement(device, mem, B):
    """Three levels at 32 px.  Not memory_efficient: the maps are at 8, 16 and 32 px - scales 4, 2 and a plain Block at scale 1;
    memory_efficient (with the init conv residual behind the combiner's slices): 4, 8, 16 px - scales 8, 4, 2, and the last
    upsample writes x's channels of the concat in place."""
    ou = _ref_unet(SMALL, seed=11, memory_efficient=mem, init_conv_to_final_conv_residual=mem)
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, B, 32, seed=3))
    print(f"combine forward mem={mem} B={B}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_csv(pu, B, 32, device)
    assert labels.count("upsample combine s=") == (3 if mem else 2)
    for s in ((8, 4, 2) if mem else (4, 2)):
        assert labels.count(f"upsample combine s={s} ") == 1
    assert "combine head" not in labels   # x's channels of the concat were written in place, not copied


@pytest.mark.parametrize("outer", ["attention", "linear_attention"])
def test_unet_forward_with_an_attention_block_as_the_last_producer(device, outer):
    """Not memory_efficient, with (linear) attention at the outermost level: the block's last GEMM writes x's channels of
    the concat in place, and the plain Block at scale 1 reads them from there."""
    kw = dict(SMALL, layer_attns=(outer == "attention", False, True))
    extra = dict(use_linear_attn=(True, False, False)) if outer == "linear_attention" else {}
    ou = _ref_unet(kw, seed=17, init_conv_to_final_conv_residual=True, **extra)
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 32, seed=3))
    print(f"combine forward, {outer} at the outermost level: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_csv(pu, 2, 32, device)
    assert labels.count("upsample combine s=") == 2 and "combine head" not in labels


def test_unet_forward_dim128_folds_the_partials_to_the_affine(device):
    """dim 128, memory_efficient, 64 px: the maps of the two levels without attention (256 channels at 16 px, 128 at 32 px)
    come from a ResnetBlock whose skip conv leaves GroupNorm partials over groups of 32 and 16 channels: their combiner
    launches take the gn_fold_seg affine (rows ending in "affine"); the attention level's map (512 channels, a token GEMM's
    output without partials) goes through GroupNorm + SiLU at low resolution."""
    ou = _ref_unet(WIDE, seed=12, memory_efficient=True)
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 64, seed=3))
    print(f"combine forward dim128 mem B=2: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_csv(pu, 2, 64, device)
    rows = [r for r in labels.splitlines() if "upsample combine s=" in r]
    print("\n".join(rows))
    assert len(rows) == 3
    assert sum("affine" in r for r in rows) == 2
    assert not any("affine" in r for r in rows if "Cin512" in r)


def test_unet_forward_with_text_lowres_and_self_cond_matches_the_restatement(device):
    ou = _ref_unet(TEXT, lowres_cond=True, seed=15, text=True, self_cond=True)
    e, _ = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 32, seed=3))
    print(f"combine forward text + lowres + self_cond: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2


def test_unet_forward_with_both_resampling_switches_and_linear_attention(device):
    ou = _ref_unet(SMALL, seed=16, memory_efficient=True, init_conv_to_final_conv_residual=True, cross_embed_downsample=True,
                   pixel_shuffle_upsample=False, use_linear_attn=True)
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 32, seed=3))
    print(f"combine forward cross-embed + nearest upsample + linear attention: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_csv(pu, 2, 32, device)
    assert labels.count("upsample combine s=") == 3 and labels.count("upsample nearest conv3") == 3


def test_default_unet_through_create_ext2_keeps_its_plan(device):
    """A default UNet built through kd_unet_create_ext2 with a zero ext2 has the launches and the bits of the plan
    kd_unet_create_ext builds."""
    lib = H.engine().load()
    from oracle import imagen_ref as R

    ou = H.ref_unet(R.Unet, H.UNET_KW["small2"], seed=4, lowres_cond=True)
    a, b = H.product_like(ou, device), H.product_like(ou, device)
    g = H.gen(5)
    x, t = torch.randn(2, 3, 32, 32, generator=g), torch.randn(2, generator=g)
    kw = dict(lowres_cond_img=torch.randn(2, 3, 32, 32, generator=g), lowres_noise_times=torch.full((2,), 1.5),
              cond_images=torch.rand(2, 3, 32, 32, generator=g))
    dv = {k: v.to(device) for k, v in kw.items()}
    ha = a.engine(2, 32, device, with_text=False)
    orig = lib.kd_unet_create_ext2
    called = []
    lib.kd_unet_create_ext2 = lambda cfg, arr, n, share, ext, ext2, out: (called.append(1), lib.kd_unet_create_ext(cfg, arr, n, share, ext, out))[1]
    try:
        hb = b.engine(2, 32, device, with_text=False)
    finally:
        lib.kd_unet_create_ext2 = orig
    assert called
    assert lib.kd_unet_num_launches(ha) == lib.kd_unet_num_launches(hb)
    assert torch.equal(a(x.to(device), t.to(device), **dv), b(x.to(device), t.to(device), **dv))
    assert "upsample combine" not in H.plan_csv(a, 2, 32, device)


# ------------------------------------------------------------------------------- sampling
BASE = dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True), layer_cross_attns=(False, True))
SR2 = dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, memory_efficient=True, layer_attns=(False, True),
           layer_cross_attns=(False, True), init_conv_to_final_conv_residual=True)


def _cascade(device, cls_o, cls_p, seed, **kw):
    ous = [_ref_unet(BASE, seed=seed), _ref_unet(SR2, lowres_cond=True, seed=seed + 1)]
    oim, pim = H.imagen_pair(device, cls_o, cls_p, ous, image_sizes=(32, 64), condition_on_text=False, **kw)
    assert all(u.combine_upsample_fmaps for u in pim.unets)
    return oim, pim


def test_ddpm_cascade_with_inpainting_matches_the_restatement(device):
    oim, pim = _cascade(device, SR.Imagen, "Imagen", 21, timesteps=(4, 4), pred_objectives=("noise", "v"))
    B = 2
    g = H.gen(3)
    inp = torch.rand(B, 3, 64, 64, generator=g)
    mask = torch.zeros(B, 64, 64, dtype=torch.bool)
    mask[:, 8:40, 12:60] = True
    nf = RS.generator_noise_fn(5)
    kw = dict(batch_size=B, inpaint_resample_times=2)
    ref = oim.sample(noise_fn=nf, inpaint_images=inp, inpaint_masks=mask, **kw)
    got = pim.sample(noise_fn=nf, inpaint_images=inp.to(device), inpaint_masks=mask.to(device), device=device, **kw).cpu()
    assert got.shape == (B, 3, 64, 64)
    err = float((got - ref).abs().max())
    print(f"combine DDPM cascade 32 -> 64, T=4, inpainting R=2: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_edm_cascade_matches_the_restatement(device):
    oim, pim = _cascade(device, ER.ElucidatedImagen, "ElucidatedImagen", 23, num_sample_steps=3)
    nf = RS.generator_noise_fn(13)
    ref = oim.sample(noise_fn=nf, batch_size=2)
    got = pim.sample(noise_fn=nf, batch_size=2, device=device).cpu()
    err = float((got - ref).abs().max())
    print(f"combine EDM cascade 32 -> 64, N=3: max|diff| {err:.2e}")
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
def test_trainer_loads_a_combine_checkpoint_strictly_and_samples_from_it(device, tmp_path, capsys):
    import imagen_pytorch as ip

    kw = dict(image_sizes=(32,), timesteps=(4,), condition_on_text=False)
    online, ema_u = _ref_unet(BASE, seed=31), _ref_unet(BASE, seed=32)
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
    print(f"combine trainer.sample from the EMA weights: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
    assert float((ref - oim_online.sample(noise_fn=nf, batch_size=2)).abs().max()) > 10 * SAMPLE_ABS
