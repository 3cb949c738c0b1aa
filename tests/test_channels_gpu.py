"""Images of 1, 2 or 4 channels (`Unet(channels=C)`, `Imagen(channels=C)`) on the MI355X: the init conv kernel at
NP = C | 2 C planes and the final conv at 9 C columns against fp64, the UNet forward against the oracle (and the
self-conditioning restatement), launch counts, and both samplers against their CPU restatements."""
import ctypes as C_

import pytest
import torch
import torch.nn.functional as F

import elucidated_ref as ER
import helpers as H
import self_cond_ref as SR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

CONV_REL = 2e-6      # as test_kernels_gpu.py / test_self_cond_gpu.py
FWD_REL_L2 = 2e-5
SAMPLE_ABS = 2e-3


# ------------------------------------------------------------------------------- the init conv kernel
INIT_SHAPES = [
    (1, 32, 16, 8, 8),        # dim 32: partial 32-row tiles
    (3, 96, 32, 16, 16),      # dim 64, S not a power of two, tiles cross image borders on every side
    (2, 64, 64, 32, 32),      # dim 128: two 32-row tiles for the k = 3 conv; 4 planes run the k = 15 ring
]
# (C, self-conditioning planes): NP = 1, 2, 4 (x alone), 2, 4 (x | self_cond); 8 planes where the kernel's LDS holds them
INIT_PLANES = [(1, False), (2, False), (4, False), (1, True), (2, True), (4, True)]


def _init_conv_case(device, B, S, n3, n7, n15, Cx, with_sc, with_res):
    """(rc, got NCHW on the CPU, fp64 reference, its three parts, the added term, fp32 CPU error)"""
    E = H.engine()
    lib = E.load()
    NP = 2 * Cx if with_sc else Cx
    c0, C_out = 2, n3 + n7 + n15
    Itot = c0 + NP + Cx          # cond (2) | x | (self_cond) | lowres: the planes sit at channel offset 2
    x = torch.randn(B, Cx, S, S, generator=H.gen(1))
    sc = torch.rand(B, Cx, S, S, generator=H.gen(2)) * 2 - 1 if with_sc else None
    ws = [torch.randn(n, Itot, k, k, generator=H.gen(10 + k)) * (NP * k * k) ** -0.5 for n, k in ((n3, 3), (n7, 7), (n15, 15))]
    inp = torch.cat((x, sc), 1) if with_sc else x
    res = torch.randn(B, S, S, C_out, generator=H.gen(5)) if with_res else None
    b = None if with_res else torch.randn(C_out, generator=H.gen(4))
    add = (res.permute(0, 3, 1, 2) if with_res else b[None, :, None, None])
    parts64 = [F.conv2d(inp.double(), w[:, c0:c0 + NP].double(), padding=w.shape[-1] // 2) for w in ws]
    ref = torch.cat(parts64, 1) + add.double()
    ref32 = torch.cat([F.conv2d(inp, w[:, c0:c0 + NP], padding=w.shape[-1] // 2) for w in ws], 1) + add
    err_cpu = float((ref32.double() - ref).norm() / ref.norm())
    dv = lambda t: None if t is None else t.to(device)
    xd, scd, wd, bd, rd = dv(x), dv(sc), [dv(w) for w in ws], dv(b), dv(res)
    y = torch.full((B, S, S, C_out), float("nan"), device=device)
    rc = lib.kd_init_conv_planes_c_nchw(E.ptr(xd), E.ptr(scd), E.ptr(wd[0]), E.ptr(wd[1]), E.ptr(wd[2]), Itot, c0,
                                        E.ptr(bd), E.ptr(rd), E.ptr(y), B, S, n3, n7, n15, 1, None, Cx, E.current_stream())
    torch.cuda.synchronize()
    return rc, y.permute(0, 3, 1, 2).cpu(), ref, parts64, add, err_cpu


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("Cx,with_sc", INIT_PLANES)
@pytest.mark.parametrize("B,S,n3,n7,n15", INIT_SHAPES)
def test_init_conv_c_planes(device, B, S, n3, n7, n15, Cx, with_sc, with_res):
    """The per-step share of the init convs over C | 2 C planes at input channels 2 .. of wider weights, + bias or + a
    step-invariant residual, in one launch, against torch conv2d in fp64.  8 planes at dim 128 do not fit the kernel's
    LDS even as a ring (161.3 KiB): the entry refuses them before any launch, as the plan does (generic path)."""
    E = H.engine()
    rc, got, ref, parts64, add, err_cpu = _init_conv_case(device, B, S, n3, n7, n15, Cx, with_sc, with_res)
    if Cx == 4 and with_sc and n3 == 64:
        assert rc != 0 and b"LDS" in E.load().kd_last_error()
        assert torch.isnan(got).all()   # nothing was launched
        return
    E.check(rc)
    assert torch.isfinite(got).all()
    err = float((got.double() - ref).norm() / ref.norm())
    print(f"init conv C={Cx} self_cond={with_sc} S={S} dim={n3 + n7 + n15}: rel-L2 {err:.2e} (fp32 CPU {err_cpu:.2e})")
    assert err <= max(3 * err_cpu, CONV_REL), (err, err_cpu)
    for sl, p64 in zip((slice(0, n3), slice(n3, n3 + n7), slice(n3 + n7, None)), parts64):
        e = float((got[:, sl].double() - (p64 + add[:, sl].double())).norm() / p64.norm())
        assert e <= max(3 * err_cpu, CONV_REL), (sl, e)


def test_init_conv_old_entry_is_the_three_channel_form(device):
    """kd_init_conv_planes_nchw (signature unchanged) == kd_init_conv_planes_c_nchw with channels = 3, bit for bit."""
    E = H.engine()
    lib = E.load()
    B, S, n3, n7, n15, Itot, c0 = 1, 32, 16, 8, 8, 8, 2
    x = torch.randn(B, 3, S, S, generator=H.gen(1)).to(device)
    ws = [(torch.randn(n, Itot, k, k, generator=H.gen(k)) * (3 * k * k) ** -0.5).to(device) for n, k in ((n3, 3), (n7, 7), (n15, 15))]
    b = torch.randn(n3 + n7 + n15, generator=H.gen(4)).to(device)
    ys = [torch.full((B, S, S, n3 + n7 + n15), float("nan"), device=device) for _ in range(2)]
    E.check(lib.kd_init_conv_planes_nchw(E.ptr(x), None, E.ptr(ws[0]), E.ptr(ws[1]), E.ptr(ws[2]), Itot, c0, E.ptr(b), None,
                                         E.ptr(ys[0]), B, S, n3, n7, n15, 1, None, E.current_stream()))
    E.check(lib.kd_init_conv_planes_c_nchw(E.ptr(x), None, E.ptr(ws[0]), E.ptr(ws[1]), E.ptr(ws[2]), Itot, c0, E.ptr(b), None,
                                           E.ptr(ys[1]), B, S, n3, n7, n15, 1, None, 3, E.current_stream()))
    assert torch.isfinite(ys[0]).all() and torch.equal(ys[0], ys[1])


@pytest.mark.parametrize("Cx", [1, 4])
def test_init_conv_generic_path_sees_c_planes(device, Cx):
    """48 px: a size the fused kernel refuses (S % 32 != 0) - its entry says so - and the plan's generic path (the C planes
    packed to 4-channel pixels, three implicit-GEMM convs with their biases) carries the forward of a base UNet."""
    E = H.engine()
    rc, got, *_ = _init_conv_case(device, 1, 48, 16, 8, 8, Cx, False, False)
    assert rc != 0 and b"init conv kernel" in E.load().kd_last_error() and torch.isnan(got).all()
    e = _forward_err(device, "small1", Cx, False, 2, 48, seed=31)
    assert e < FWD_REL_L2


# ------------------------------------------------------------------------------- the final conv
_FINAL_REF = {}


def _final_inputs(B, H_, W, Cfeat):
    """One set of inputs per shape, shared by the channel cases (4 channels, the narrower cases take the first C)."""
    key = (B, H_, W, Cfeat)
    if key not in _FINAL_REF:
        g = H.gen(7)
        _FINAL_REF[key] = dict(feat=torch.randn(B, H_, W, Cfeat, generator=g), lowres=torch.randn(B, 4, H_, W, generator=g),
                               w=torch.randn(4, Cfeat + 4, 3, 3, generator=g) * (9 * Cfeat) ** -0.5,
                               bias=torch.randn(4, generator=g))
    return _FINAL_REF[key]


@pytest.mark.parametrize("with_lowres", [False, True])
@pytest.mark.parametrize("Cx", [1, 2, 3, 4])
@pytest.mark.parametrize("B,H_,W,Cfeat", [
    (2, 10, 70, 32),      # H not a multiple of the 4-row blocks, W crosses a 64-pixel segment
    (1, 32, 32, 128),
])
def test_final_conv(device, B, H_, W, Cfeat, Cx, with_lowres):
    """kd_final_conv_nchw: the plan's launches (pack, 1x1 GEMM to 9 C columns, the low-res planes' share, gather)
    against torch conv2d over cat(feat, lowres) in fp64."""
    E = H.engine()
    lib = E.load()
    d = _final_inputs(B, H_, W, Cfeat)
    feat, bias = d["feat"], d["bias"][:Cx].contiguous()
    lowres = d["lowres"][:, :Cx].contiguous() if with_lowres else None
    cin = Cfeat + (Cx if with_lowres else 0)
    w = d["w"][:Cx, :cin].contiguous()
    inp = feat.permute(0, 3, 1, 2)
    if with_lowres:
        inp = torch.cat((inp, lowres), 1)
    ref = F.conv2d(inp.double(), w.double(), bias.double(), padding=1)
    ref32 = F.conv2d(inp, w, bias, padding=1)
    err_cpu = float((ref32.double() - ref).norm() / ref.norm())
    dv = lambda t: None if t is None else t.to(device)
    fd, wd, bd, ld = dv(feat), dv(w), dv(bias), dv(lowres)
    out = torch.full((B, Cx, H_, W), float("nan"), device=device)
    E.check(lib.kd_final_conv_nchw(E.ptr(fd), E.ptr(wd), E.ptr(bd), E.ptr(ld), E.ptr(out), B, H_, W, Cfeat, Cx,
                                   E.current_stream()))
    got = out.cpu()
    assert torch.isfinite(got).all()
    err = float((got.double() - ref).norm() / ref.norm())
    print(f"final conv C={Cx} lowres={with_lowres} {B}x{H_}x{W}x{Cfeat}: rel-L2 {err:.2e} (fp32 CPU {err_cpu:.2e})")
    assert err <= max(3 * err_cpu, CONV_REL), (err, err_cpu)


# ------------------------------------------------------------------------------- the UNet forward
ULTRA2 = dict(dim=128, dim_mults=(1, 2, 4, 8), num_resnet_blocks=2, memory_efficient=True,
              layer_attns=(False, False, False, True), layer_cross_attns=(False, False, True, True),
              init_conv_to_final_conv_residual=True, cond_images_channels=3)   # train_ultra_res.py:39-48


def _forward_err(device, name, Cx, lowres, B, S, seed, self_cond=False, fast=False):
    kw = ULTRA2 if name == "ultra2_full" else H.UNET_KW[name]
    cls = SR.Unet if self_cond else R.Unet
    extra = dict(self_cond=True) if self_cond else {}
    ou = H.ref_unet(cls, kw, seed=seed, channels=Cx, lowres_cond=lowres, **extra)
    if fast:
        ou = H.fast_oracle(ou)
    x, t, kw_in = H.unet_inputs(ou, B, S, seed=3)
    e, pu = H.forward_err(ou, device, x, t, kw_in)
    # (the bits forward_err compared: its two runs were identical)
    got = pu(x.to(device), t.to(device), **{k: v.to(device) for k, v in kw_in.items()}).cpu()
    assert got.shape == (B, Cx, S, S) and torch.isfinite(got).all()
    print(f"forward {name} C={Cx} S={S} self_cond={self_cond}: rel-L2 {e:.2e}")
    return e


@pytest.mark.parametrize("Cx", [1, 2, 4])
@pytest.mark.parametrize("name,lowres,S", [("small1", False, 32), ("small2", True, 32), ("small2", True, 48)])
def test_unet_forward_of_c_channels_matches_the_oracle(device, name, lowres, S, Cx):
    """Base UNet, and the SR UNet (lowres + cond images + memory_efficient + init -> final residual) on the fused init
    conv (32 px) and on the generic path (48 px)."""
    assert _forward_err(device, name, Cx, lowres, 2, S, seed=11) < FWD_REL_L2


@pytest.mark.parametrize("Cx", [1, 4])
def test_self_cond_unet_forward_of_c_channels_matches_the_restatement(device, Cx):
    assert _forward_err(device, "small2", Cx, True, 2, 32, seed=12, self_cond=True) < FWD_REL_L2


def test_full_width_unet_forward_of_four_channels_matches_the_oracle(device):
    """dim 128: the ring-form init conv (4 planes) and the 48-column final conv inside a plan."""
    assert _forward_err(device, "ultra2_full", 4, True, 2, 64, seed=13, fast=True) < FWD_REL_L2


@pytest.mark.parametrize("S", [32, 48])
def test_plans_of_every_channel_count_have_the_same_launches(device, S):
    """A channel count that fell to the generic init conv (three convs + a pack) at 32 px would show here; at 48 px every
    count runs the generic path."""
    lib = H.engine().load()
    counts = {}
    for Cx in (3, 1, 2, 4):
        ou = R.Unet(**H.UNET_KW["small2"], channels=Cx, lowres_cond=True, **H.NOTEXT)
        h = H.product_like(ou, device).engine(2, S, device, with_text=False)
        counts[Cx] = lib.kd_unet_num_launches(h)
    assert counts[1] == counts[2] == counts[4] == counts[3], counts


# ------------------------------------------------------------------------------- sampling
def _pair(device, names, sizes, channels, cls=(RS.Imagen, "Imagen"), seed=5, **kw):
    ous = [R.NullUnet() if n is None else H.randomize_(
        R.Unet(**H.UNET_KW[n], channels=channels, lowres_cond=i > 0, **H.NOTEXT), seed + i) for i, n in enumerate(names)]
    return H.imagen_pair(device, *cls, ous, image_sizes=sizes, channels=channels, condition_on_text=False, **kw)


def test_grayscale_cascade_with_dynamic_thresholding_matches_the_oracle(device):
    """C = 1, small1 -> small2 at (32, 64), T = 4, batch 2, dynamic thresholding in both stages: the quantile runs over
    C H W = H W values.  The thresholds of one step (kd_sample_last, which = 2) against the oracle's own: the sample is
    x0 / s, so the relative error of s is held to the bound of the samples."""
    E = H.engine()
    lib = E.load()
    oim, pim = _pair(device, ["small1", "small2"], (32, 64), 1, timesteps=(4, 4), pred_objectives=("noise", "v"),
                     dynamic_thresholding=(True, True))
    B = 2
    nf = RS.generator_noise_fn(21)
    ref1 = oim.sample(noise_fn=nf, batch_size=B, stop_at_unet_number=1)
    got1 = pim.sample(noise_fn=nf, batch_size=B, stop_at_unet_number=1, device=device).cpu()
    assert got1.shape == (B, 1, 32, 32)
    e1 = float((got1 - ref1).abs().max())
    cond = torch.rand(B, 3, 64, 64, generator=H.gen(2))
    kw = dict(batch_size=B, start_at_unet_number=2)
    ref2 = oim.sample(noise_fn=nf, start_image_or_video=ref1, cond_images=cond, **kw)
    got2 = pim.sample(noise_fn=nf, start_image_or_video=ref1.to(device), cond_images=cond.to(device), device=device, **kw).cpu()
    assert got2.shape == (B, 1, 64, 64)
    e2 = float((got2 - ref2).abs().max())
    print(f"C=1 cascade, dynamic thresholding: max|diff| base {e1:.2e}, SR {e2:.2e}")
    assert e1 < SAMPLE_ABS and e2 < SAMPLE_ABS
    # one step of the base stage from a wide x: thresholds well above the clamp at 1
    S, T, k = 32, 4, 1
    pu, ou, sched = pim.unets[0], oim.unets[0], oim.noise_schedulers[0]
    h = pu.engine(B, S, device, with_text=False)
    tables = pim.noise_schedulers[0].step_tables()
    sc = E.kd_schedule_t()
    sc.T = T
    for name, v in tables.items():
        setattr(sc, name, v.numpy().ctypes.data_as(C_.POINTER(C_.c_float)))
    x = torch.randn(B, 1, S, S, generator=H.gen(6)) * 1.5
    sa = E.kd_sample_args_t()
    sa.objective, sa.dynamic_threshold, sa.percentile, sa.resample_times, sa.seed, sa.use_graph = 0, 1, 0.95, 1, 9, 1
    xd = x.to(device)
    E.check(lib.kd_sample_steps(h, C_.byref(sc), C_.byref(sa), E.ptr(xd), k, k + 1, E.current_stream()))
    thr = torch.empty(B, device=device)
    E.check(lib.kd_sample_last(h, 2, E.ptr(thr), E.current_stream()))
    times, _ = sched.get_sampling_timesteps(B)[k]
    with torch.no_grad():
        x0 = sched.predict_start_from_noise(x, times, ou(x, sched.log_snr(times)))
    want = torch.quantile(x0.flatten(1).abs(), 0.95, dim=-1).clamp(min=1.0)
    assert (want > 1.0).all(), want
    rel = float(((thr.cpu() - want).abs() / want).max())
    print(f"C=1 thresholds {thr.cpu().tolist()} against {want.tolist()}: rel {rel:.2e}")
    assert rel < SAMPLE_ABS


def test_four_channel_sr_stage_with_inpainting_matches_the_oracle(device):
    """C = 4, SR stage at 64 px with cond images and inpainting, inpaint_resample_times = 2: the [B, H, W] mask is
    broadcast over the 4 channels, whose known pixels come back bit-exact."""
    oim, pim = _pair(device, [None, "small2"], (32, 64), 4, timesteps=(4, 4), pred_objectives=("noise", "v"))
    B = 2
    g = H.gen(8)
    start = torch.rand(B, 4, 32, 32, generator=g)
    cond = torch.rand(B, 3, 64, 64, generator=g)
    inp = torch.rand(B, 4, 64, 64, generator=g)
    mask = torch.zeros(B, 64, 64, dtype=torch.bool)
    mask[:, 4:40, 6:60] = True
    nf = RS.generator_noise_fn(12)
    kw = dict(batch_size=B, start_at_unet_number=2, inpaint_resample_times=2)
    ref = oim.sample(noise_fn=nf, start_image_or_video=start, cond_images=cond, inpaint_images=inp, inpaint_masks=mask, **kw)
    dv = lambda v: v.to(device)
    got = pim.sample(noise_fn=nf, start_image_or_video=dv(start), cond_images=dv(cond), inpaint_images=dv(inp),
                     inpaint_masks=dv(mask), device=device, **kw).cpu()
    assert got.shape == (B, 4, 64, 64)
    m = mask[:, None].expand_as(got)
    assert torch.equal(got[m], ref[m]), "known pixels"
    err = float((got - ref).abs().max())
    print(f"C=4 SR + inpainting (R=2): max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_two_channel_elucidated_sampling_matches_the_restatement(device):
    oim, pim = _pair(device, ["small1"], (32,), 2, cls=(ER.ElucidatedImagen, "ElucidatedImagen"), num_sample_steps=3)
    nf = RS.generator_noise_fn(13)
    ref = oim.sample(noise_fn=nf, batch_size=2)
    got = pim.sample(noise_fn=nf, batch_size=2, device=device).cpu()
    assert got.shape == (2, 2, 32, 32)
    err = float((got - ref).abs().max())
    print(f"C=2 EDM base, N=3: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_grayscale_graph_replay_equals_eager_launches(device):
    _, pim = _pair(device, [None, "small2"], (16, 32), 1, timesteps=(4, 4))
    start = torch.rand(2, 1, 16, 16, generator=H.gen(1)).to(device)
    kw = dict(noise_fn=RS.generator_noise_fn(7), batch_size=2, start_at_unet_number=2, start_image_or_video=start,
              cond_images=torch.rand(2, 3, 32, 32, generator=H.gen(2)).to(device), device=device)
    a = pim.sample(use_graph=True, **kw)
    b = pim.sample(use_graph=False, **kw)
    assert a.shape == (2, 1, 32, 32) and torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("Cx,mode", [(1, "L"), (2, "LA"), (4, "RGBA")])
def test_return_pil_images_by_channel_count(device, Cx, mode):
    """The library's ToPILImage: mode by channel count, values mul(255).byte() (truncation)."""
    import numpy as np

    _, pim = _pair(device, ["small1"], (32,), Cx, timesteps=(2,))
    ten = pim.sample(batch_size=2, seed=3, device=device)
    pil = pim.sample(batch_size=2, seed=3, device=device, return_pil_images=True)
    assert len(pil) == 2 and all(p.size == (32, 32) and p.mode == mode for p in pil)
    want = ten.clamp(0, 1).mul(255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    got = np.stack([np.asarray(p) for p in pil]).reshape(want.shape)
    assert np.array_equal(got, want)
