"""The structural switches of the UNet's first and last layer on the MI355X (`Unet(init_cross_embed=False,
init_conv_kernel_size=k, init_cross_embed_kernel_sizes=..., final_conv_kernel_size=k, final_resnet_block=False,
scale_skip_connection=False)`): the k x k final conv (kernels_final.hip) and the plain init conv's one-kernel form
(kernels_init.hip) against fp64 torch through the C ABI, the UNet forward and the samplers against the restatement in
tests/structure_ref.py, the plans' launch labels, a default UNet through kd_unet_create_ext4, and poisoned scratch."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import elucidated_ref as ER
import helpers as H
import solver_ref as SV
import structure_ref as SR
import test_poisoned_scratch_gpu as TPS
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

CONV_REL = 2e-6      # the bound the resample and combiner kernels are held to: fp32 against fp64, relative L2
FWD_REL_L2 = 2e-5
SAMPLE_ABS = 2e-3
# a GroupNorm partial sums 16 channels x 32 pixels = 512 fp32 values (and their squares): an fp32 accumulation of 512 terms is
# off by at most 512 * 2^-24 of the sum of the magnitudes
SEG_REL = 512 * 2.0 ** -24


# ------------------------------------------------------------------------------- the k x k final conv
@functools.lru_cache(maxsize=None)
def _final_inputs(H_, W, Cfeat, k):
    g = H.gen(H_ * W + Cfeat + k)
    return dict(feat=torch.randn(2, H_, W, Cfeat, generator=g), lowres=torch.randn(2, 4, H_, W, generator=g),
                w=torch.randn(4, Cfeat + 4, k, k, generator=g) * (k * k * Cfeat) ** -0.5, bias=torch.randn(4, generator=g))


def _ring(t, r):
    """The border ring of width r of [.., H, W] maps, flattened."""
    m = torch.ones(t.shape[-2:], dtype=torch.bool)
    if r > 0 and t.shape[-2] > 2 * r and t.shape[-1] > 2 * r:
        m[r:-r, r:-r] = False
    return t[..., m]


def _final_case(device, H_, W, Cfeat, k, Cx, with_lowres, entry="kd_final_conv_k_nchw"):
    E = H.engine()
    lib = E.load()
    d = _final_inputs(H_, W, Cfeat, k)
    feat, bias = d["feat"], d["bias"][:Cx].contiguous()
    lowres = d["lowres"][:, :Cx].contiguous() if with_lowres else None
    cin = Cfeat + (Cx if with_lowres else 0)
    w = d["w"][:Cx, :cin].contiguous()
    inp = feat.permute(0, 3, 1, 2)
    if with_lowres:
        inp = torch.cat((inp, lowres), 1)
    ref = F.conv2d(inp.double(), w.double(), bias.double(), padding=k // 2)
    dv = lambda t: None if t is None else t.to(device)
    fd, wd, bd, ld = dv(feat), dv(w), dv(bias), dv(lowres)
    out = torch.full((2, Cx, H_, W), float("nan"), device=device)
    if entry == "kd_final_conv_nchw":
        E.check(lib.kd_final_conv_nchw(E.ptr(fd), E.ptr(wd), E.ptr(bd), E.ptr(ld), E.ptr(out), 2, H_, W, Cfeat, Cx, E.current_stream()))
    else:
        E.check(lib.kd_final_conv_k_nchw(E.ptr(fd), E.ptr(wd), E.ptr(bd), E.ptr(ld), E.ptr(out), 2, H_, W, Cfeat, Cx, k,
                                         E.current_stream()))
    return out.cpu(), ref


@pytest.mark.parametrize("Cx", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [1, 5, 7])
@pytest.mark.parametrize("H_,W", [(5, 7), (37, 50), (64, 64)])   # smaller than a tile; partial tiles both ways; whole tiles
def test_final_conv_k_matches_fp64(device, H_, W, k, Cx):
    """kd_final_conv_k_nchw: the plan's launches (pack, 1x1 GEMM to the k^2 C columns, the low-res planes' share, the k x k
    gather) against torch conv2d over cat(feat, lowres) in fp64, B = 2, Cfeat 32 and 36, with and without low-res planes.  The
    border ring of width k // 2 is compared on its own, so that a padding error cannot hide in the mean."""
    for Cfeat in (32, 36):
        for with_lowres in (False, True):
            got, ref = _final_case(device, H_, W, Cfeat, k, Cx, with_lowres)
            assert torch.isfinite(got).all()
            err = H.rel_l2(got, ref)
            ring = H.rel_l2(_ring(got, k // 2), _ring(ref, k // 2))
            print(f"final conv k={k} C={Cx} lowres={with_lowres} 2x{H_}x{W}x{Cfeat}: rel-L2 {err:.2e}, border ring {ring:.2e}")
            assert err < CONV_REL and ring < CONV_REL, (Cfeat, with_lowres, err, ring)


@pytest.mark.parametrize("Cx", [1, 4])
def test_final_conv_k3_through_the_new_entry_is_the_old_entry(device, Cx):
    for with_lowres in (False, True):
        a, _ = _final_case(device, 37, 50, 36, 3, Cx, with_lowres)
        b, _ = _final_case(device, 37, 50, 36, 3, Cx, with_lowres, entry="kd_final_conv_nchw")
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_final_conv_k_refuses_other_sizes(device):
    E = H.engine()
    lib = E.load()
    t = torch.zeros(2 * 8 * 8 * 32, device=device)
    for k in (0, 2, 9):
        assert lib.kd_final_conv_k_nchw(E.ptr(t), E.ptr(t), E.ptr(t), None, E.ptr(t), 2, 8, 8, 32, 3, k, E.current_stream()) != 0
        assert b"kernel size" in lib.kd_last_error()


# ------------------------------------------------------------------------------- the plain init conv
PLANES = {1: (1, False), 3: (3, False), 4: (4, False), 6: (3, True)}   # NP -> (image channels, self_cond planes)


@functools.lru_cache(maxsize=None)
def _init_inputs(S, NP, k, dim):
    g = H.gen(S + 7 * NP + 31 * k + dim)
    Cx, with_sc = PLANES[NP]
    Itot = NP + 5   # the per-step planes sit at input channels 2 .. of wider weights
    return dict(x=torch.randn(2, Cx, S, S, generator=g), sc=torch.randn(2, Cx, S, S, generator=g) if with_sc else None,
                w=torch.randn(dim, Itot, k, k, generator=g) * (NP * k * k) ** -0.5, bias=torch.randn(dim, generator=g),
                res=torch.randn(2, S, S, dim, generator=g))


def _init_plain(device, S, NP, k, dim, *, res, ld=0, off=0, seg=False, fill=None):
    """(rc, y as the kernel left it [2][S][S][ld or dim], the partials or None)"""
    E = H.engine()
    lib = E.load()
    d = _init_inputs(S, NP, k, dim)
    Cx, _ = PLANES[NP]
    dv = lambda t: None if t is None else t.to(device)
    xd, scd, wd = dv(d["x"]), dv(d["sc"]), dv(d["w"])
    bd, rd = (None, dv(d["res"])) if res else (dv(d["bias"]), None)
    ldy = ld or dim
    y = torch.full((2, S, S, ldy), float("nan"), device=device) if fill is None else fill.to(device)
    sg = torch.full((2, dim // 16, S * S // 32, 2), float("nan"), dtype=torch.float64, device=device) if seg else None
    rc = lib.kd_init_conv_plain_nchw(E.ptr(xd), E.ptr(scd), E.ptr(wd), NP + 5, 2, E.ptr(bd), E.ptr(rd),
                                     y.data_ptr() + 4 * off, ldy, None if sg is None else sg.data_ptr(), 2, S, dim, k, Cx, 1, None,
                                     E.current_stream())
    torch.cuda.synchronize()
    return rc, y.cpu(), None if sg is None else sg.cpu()


def _init_ref(S, NP, k, dim, res):
    d = _init_inputs(S, NP, k, dim)
    inp = d["x"] if d["sc"] is None else torch.cat((d["x"], d["sc"]), 1)
    add = d["res"].permute(0, 3, 1, 2) if res else d["bias"][None, :, None, None]
    return (F.conv2d(inp.double(), d["w"][:, 2:2 + NP].double(), padding=k // 2) + add.double()).permute(0, 2, 3, 1)


@pytest.mark.parametrize("dim", [32, 128])
@pytest.mark.parametrize("NP", [1, 3, 4, 6])
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("S", [32, 64])
def test_init_conv_plain_matches_fp64(device, S, k, NP, dim):
    """kd_init_conv_plain_nchw, B = 2: + bias into a dense map, and + a step-invariant residual into channels [32, 32 + dim) of
    rows of dim + 64 floats whose other channels must stay; the GroupNorm partials against sums over the kernel's own output.
    dim 128 at k = 7 with 6 planes does not fit the kernel's LDS: the entry refuses it before any launch, as the plan's
    predicate does."""
    lib = H.engine().load()
    if (dim, k, NP) == (128, 7, 6):
        rc, y, _ = _init_plain(device, S, NP, k, dim, res=False)
        assert rc != 0 and b"plain init conv kernel" in lib.kd_last_error() and torch.isnan(y).all()
        return
    rc, y, sg = _init_plain(device, S, NP, k, dim, res=False, seg=True)
    assert rc == 0, lib.kd_last_error()
    ref = _init_ref(S, NP, k, dim, False)
    err = H.rel_l2(y, ref)
    ring = H.rel_l2(_ring(y.permute(0, 3, 1, 2), k // 2), _ring(ref.permute(0, 3, 1, 2), k // 2))
    print(f"plain init conv k={k} NP={NP} dim={dim} S={S} + bias: rel-L2 {err:.2e}, border ring {ring:.2e}")
    assert torch.isfinite(y).all() and err < CONV_REL and ring < CONV_REL
    # partials [B][dim / 16][S S / 32][2]: (sum, sum of squares) of 16 channels x one run of 32 pixels in raster order
    v = y.double().reshape(2, S * S // 32, 32, dim // 16, 16).permute(0, 3, 1, 2, 4)
    s1, s2, sa = v.sum((-1, -2)), (v * v).sum((-1, -2)), v.abs().sum((-1, -2))
    assert torch.isfinite(sg).all()
    e1, e2 = float(((sg[..., 0] - s1).abs() / sa).max()), float(((sg[..., 1] - s2).abs() / s2).max())
    print(f"  partials: sum off by {e1:.2e} of the magnitudes, sum of squares by {e2:.2e}")
    assert e1 <= SEG_REL and e2 <= SEG_REL
    fill = torch.randn(2, S, S, dim + 64, generator=H.gen(9))
    rc, buf, _ = _init_plain(device, S, NP, k, dim, res=True, ld=dim + 64, off=32, fill=fill)
    assert rc == 0, lib.kd_last_error()
    err = H.rel_l2(buf[..., 32:32 + dim], _init_ref(S, NP, k, dim, True))
    print(f"  + residual into a channel slice: rel-L2 {err:.2e}")
    assert err < CONV_REL
    rest = [c for c in range(dim + 64) if not 32 <= c < 32 + dim]
    assert torch.equal(buf[..., rest], fill[..., rest])


def test_init_conv_plain_refuses_what_its_predicate_refuses(device):
    lib = H.engine().load()
    for S, NP, k, dim in ((40, 3, 7, 32), (32, 3, 9, 32), (32, 3, 1, 32), (32, 3, 7, 160)):
        d = _init_inputs(32, NP, k, dim)   # (never read: refused before any launch)
        E = H.engine()
        t = d["w"].to(device)
        y = torch.full((4,), float("nan"), device=device)
        rc = lib.kd_init_conv_plain_nchw(E.ptr(t), None, E.ptr(t), NP + 5, 2, None, None, E.ptr(y), dim, None, 2, S, dim, k, NP, 1, None,
                                         E.current_stream())
        assert rc != 0 and b"plain init conv kernel" in lib.kd_last_error(), (S, NP, k, dim)
        assert torch.isnan(y).all()


# ------------------------------------------------------------------------------- the UNet forward
NARROW = dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True), layer_cross_attns=(False, True))
WIDE = dict(dim=128, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
            layer_cross_attns=(False, False, True))
RES = dict(init_conv_to_final_conv_residual=True)
FORWARD = {
    "plain_init_k3": dict(init_cross_embed=False, init_conv_kernel_size=3),
    "plain_init_k7": dict(init_cross_embed=False),
    "plain_init_k9_generic": dict(init_cross_embed=False, init_conv_kernel_size=9),
    "plain_init_k1_generic": dict(init_cross_embed=False, init_conv_kernel_size=1),      # the bounds of what is planned
    "plain_init_k15_generic": dict(init_cross_embed=False, init_conv_kernel_size=15, lowres_cond=True),
    "sizes_1_13": dict(init_cross_embed_kernel_sizes=(13, 1)),
    "sizes_3_5": dict(init_cross_embed_kernel_sizes=(3, 5)),
    "sizes_7": dict(init_cross_embed_kernel_sizes=(7,)),
    "sizes_3_7_15_5": dict(init_cross_embed_kernel_sizes=(3, 7, 15, 5)),
    "final_k1": dict(final_conv_kernel_size=1),
    "final_k5": dict(final_conv_kernel_size=5),
    "final_k7": dict(final_conv_kernel_size=7),
    "no_final_block": dict(final_resnet_block=False),
    "no_final_block_residual": dict(final_resnet_block=False, **RES),
    "no_final_block_combine": dict(final_resnet_block=False, combine_upsample_fmaps=True),
    "no_final_block_combine_residual": dict(final_resnet_block=False, combine_upsample_fmaps=True, **RES),
    "no_skip_scale": dict(scale_skip_connection=False),
    "all_five": dict(SR.FIVE, init_cross_embed_kernel_sizes=(3, 5), lowres_cond=True, cond_images_channels=3,
                     memory_efficient=True, **RES),
    "plain_init_self_cond": dict(init_cross_embed=False, init_conv_kernel_size=5, self_cond=True),
    "plain_init_self_cond_lowres": dict(init_cross_embed=False, self_cond=True, lowres_cond=True, channels=1),
}
_ref_unet = functools.partial(H.ref_unet, SR.Unet)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("name", sorted(FORWARD))
def test_unet_forward_matches_the_restatement(device, name, B):
    ou = _ref_unet(NARROW, seed=11, **FORWARD[name])
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, B, 32, seed=3))
    print(f"structure forward {name} B={B}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_labels(pu, B, 32, device)
    plain = not FORWARD[name].get("init_cross_embed", True)
    k = FORWARD[name].get("init_conv_kernel_size", 7)
    assert H.count_labels(labels, "init conv plain fused") == int(plain and k in (3, 5, 7)), labels[:8]
    fk = FORWARD[name].get("final_conv_kernel_size", 3)
    assert H.count_labels(labels, "final gather") == 1 and labels[-1] == ("final gather" if fk == 3 else f"final gather k{fk}")


def test_unet_forward_dim128_on_the_default_fast_plan(device):
    """dim 128 at 64 px, batch 4: the F(4x4,3x3) layers and the partials take the skip halves unscaled; the plain init conv
    (k = 7, 3 planes, 128 channels: 77.5 KiB of weights) runs in its one kernel; final conv 5 x 5 over the concat."""
    ou = _ref_unet(WIDE, seed=12, scale_skip_connection=False, init_cross_embed=False, final_conv_kernel_size=5,
                   final_resnet_block=False, **RES)
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, 4, 64, seed=3))
    print(f"structure forward dim128 S=64 B=4: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_labels(pu, 4, 64, device)
    assert H.count_labels(labels, "init conv plain fused k7 S64 C128") == 1
    assert H.count_labels(labels, "scale slice") == 0 and labels[-1] == "final gather k5"


# ------------------------------------------------------------------------------- plan labels
def test_plain_init_takes_the_generic_conv_where_its_predicate_fails(device):
    """40 px is no multiple of the kernel's 32-pixel tiles: one generic k = 7 conv over the packed planes."""
    ou = _ref_unet(NARROW, seed=13, init_cross_embed=False)
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 40, seed=3))
    print(f"structure forward plain init at 40 px: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_labels(pu, 2, 40, device)
    assert H.count_labels(labels, "init conv") == 0 and H.count_labels(labels, "conv k7 s1 M3200 Cin4 Cout32") == 1, labels[:8]


@pytest.mark.parametrize("over", [dict(init_cross_embed=False), {}], ids=["plain", "cross_embed"])
def test_init_conv_generic_knob_takes_the_generic_path_at_a_shape_the_kernels_take(device, over):
    """`unet.init_conv_generic = 1` (engine extension, the A/B of profiles/structure_step_c3.py): the generic convs at 32 px."""
    ou = _ref_unet(NARROW, seed=15, **over)
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 32, seed=3), init_conv_generic=1)
    print(f"structure forward init_conv_generic=1 {over}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_labels(pu, 2, 32, device)
    assert H.count_labels(labels, "init conv") == 0 and H.count_labels(labels, "conv k7 s1 M2048 Cin4") == 1, labels[:8]
    pu.init_conv_generic = 0
    x, t, _ = H.unet_inputs(ou, 2, 32, seed=3)
    pu(x.to(device), t.to(device))
    assert H.count_labels(H.plan_labels(pu, 2, 32, device), "init conv") == 1   # another plan: the knob is part of the key


def test_no_scale_launch_without_scale_skip_connection(device):
    ous = [_ref_unet(NARROW, seed=14, scale_skip_connection=s) for s in (True, False)]
    labels = []
    for ou in ous:
        pu = H.product_like(ou, device)
        x, t, kw = H.unet_inputs(ou, 2, 32, seed=3)
        pu(x.to(device), t.to(device))
        labels.append(H.plan_labels(pu, 2, 32, device))
    n = H.count_labels(labels[0], "scale slice")
    assert n > 0 and H.count_labels(labels[1], "scale slice") == 0
    assert [l for l in labels[0] if not l.startswith("scale slice")] == labels[1]


def test_default_unet_through_create_ext4_keeps_its_plan(device):
    """A default UNet built through kd_unet_create_ext4 with a zeroed ext4 has the launches, the labels and the bits of the
    plan kd_unet_create_ext3 builds."""
    E = H.engine()
    lib = E.load()
    from oracle import imagen_ref as R

    ou = H.ref_unet(R.Unet, H.UNET_KW["small2"], seed=4, lowres_cond=True)
    a, b = H.product_like(ou, device), H.product_like(ou, device)
    x, t, kw = H.unet_inputs(ou, 2, 32, seed=5)
    dv = {k: v.to(device) for k, v in kw.items()}
    ha = a.engine(2, 32, device, with_text=False)
    orig = lib.kd_unet_create_ext2
    called = []

    def through_ext4(cfg, arr, n, share, ext, ext2, out):
        called.append(1)
        return lib.kd_unet_create_ext4(cfg, arr, n, share, ext, ext2, None, C.byref(E.kd_unet_ext4_t()), out)

    lib.kd_unet_create_ext2 = through_ext4
    try:
        hb = b.engine(2, 32, device, with_text=False)
    finally:
        lib.kd_unet_create_ext2 = orig
    assert called
    assert lib.kd_unet_num_launches(ha) == lib.kd_unet_num_launches(hb)
    assert torch.equal(a(x.to(device), t.to(device), **dv), b(x.to(device), t.to(device), **dv))
    assert H.plan_labels(a, 2, 32, device) == H.plan_labels(b, 2, 32, device)


# ------------------------------------------------------------------------------- sampling
B = 3


def _cascade(device, cls_o, cls_p, seed, **kw):
    ous = [_ref_unet(NARROW, seed=seed, **SR.FIVE), _ref_unet(NARROW, seed=seed + 1, lowres_cond=True, **SR.FIVE, **RES)]
    oim, pim = H.imagen_pair(device, cls_o, cls_p, ous, image_sizes=(16, 32), condition_on_text=False, **kw)
    assert all(u.final_res_block is None and not u._plan["scale_skip_connection"] for u in pim.unets)
    return oim, pim


DDPM = dict(timesteps=(4, 4), pred_objectives=("noise", "v"))


def test_ddpm_cascade_with_inpainting_matches_the_restatement(device):
    oim, pim = _cascade(device, SV.Imagen, "Imagen", 21, **DDPM)
    g = H.gen(3)
    inp = torch.rand(B, 3, 32, 32, generator=g)
    mask = torch.zeros(B, 32, 32, dtype=torch.bool)
    mask[:, 4:20, 6:30] = True
    nf = RS.generator_noise_fn(5)
    kw = dict(batch_size=B, inpaint_resample_times=2)
    ref = oim.sample(noise_fn=nf, inpaint_images=inp, inpaint_masks=mask, **kw)
    got = pim.sample(noise_fn=nf, inpaint_images=inp.to(device), inpaint_masks=mask.to(device), device=device, **kw).cpu()
    assert got.shape == (B, 3, 32, 32)
    err = float((got - ref).abs().max())
    print(f"structure DDPM cascade 16 -> 32, T=4, inpainting R=2: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_edm_cascade_matches_the_restatement(device):
    oim, pim = _cascade(device, ER.ElucidatedImagen, "ElucidatedImagen", 23, num_sample_steps=3)
    nf = RS.generator_noise_fn(13)
    ref = oim.sample(noise_fn=nf, batch_size=B)
    got = pim.sample(noise_fn=nf, batch_size=B, device=device).cpu()
    err = float((got - ref).abs().max())
    print(f"structure EDM cascade 16 -> 32, N=3: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_dpmpp_2m_cascade_matches_the_restatement(device):
    oim, pim = _cascade(device, SV.Imagen, "Imagen", 25, timesteps=(8, 8), pred_objectives=("noise", "v"))
    nf = SV.never_step_noise(RS.generator_noise_fn(41))
    kw = dict(batch_size=B, sampler="dpmpp_2m", sample_steps=4)
    ref = oim.sample(noise_fn=nf, **kw)
    got = pim.sample(noise_fn=nf, device=device, **kw).cpu()
    err = float((got - ref).abs().max())
    print(f"structure DPM-Solver++(2M) cascade 16 -> 32, 4 of 8 steps: max|diff| {err:.2e}")
    assert bool(torch.isfinite(got).all()) and err < SAMPLE_ABS


def test_graph_equals_eager_and_table_on_equals_off(device):
    _, pim = _cascade(device, SV.Imagen, "Imagen", 27, **DDPM)
    nf = RS.generator_noise_fn(7)
    runs = {}
    for use_graph in (True, False):
        for table in (0, -1):
            pim.cond_table = table
            runs[use_graph, table] = pim.sample(noise_fn=nf, batch_size=B, use_graph=use_graph, device=device)
    base = runs[True, 0]
    assert bool(torch.isfinite(base).all())
    for key, v in runs.items():
        assert torch.equal(v, base), key


# ------------------------------------------------------------------------------- poisoned scratch
@pytest.mark.parametrize("name", ["all_five", "no_final_block_combine_residual"])
def test_forward_under_poisoned_scratch(device, name):
    ou = _ref_unet(NARROW, seed=31, **FORWARD[name])
    pu = H.product_like(ou, device)
    x, t, kw = H.unet_inputs(ou, 2, 32, seed=3)
    x, t, kw = x.to(device), t.to(device), {k: v.to(device) for k, v in kw.items()}
    TPS._check_forward(pu, lambda: pu(x, t, **kw), lambda: pu.engine(2, 32, device, with_text=False), f"structure {name}")


def test_sampling_under_poisoned_scratch(device):
    _, pim = _cascade(device, SV.Imagen, "Imagen", 33, **DDPM)
    TPS._check_sampler(pim, lambda: pim.sample(batch_size=B, seed=7, device=device), "structure DDPM cascade T=4", 2)
