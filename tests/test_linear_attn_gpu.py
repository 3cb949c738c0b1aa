"""Linear attention (library `Unet(use_linear_attn=..., use_linear_cross_attn=...)`) on the MI355X: the three kernels of
kernels_linattn.hip against fp64 torch, the UNet forward and both samplers against the restatement in
tests/linear_attn_ref.py, graph / eager and run-to-run bit identity, and the plan of a UNet without linear attention
through kd_unet_create_ext."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import elucidated_ref as ER
import helpers as H
import linear_attn_ref as LR
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

KERNEL_REL = 2e-6
FWD_REL_L2 = 2e-5
SAMPLE_ABS = 2e-3


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _at(t, floats):   # device pointer of a column slice (the kernels take row strides)
    return C.c_void_p(t.data_ptr() + 4 * floats)


# ------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("B,Hh,Ww,heads", [(2, 13, 21, 2), (1, 9, 8, 1), (3, 24, 40, 8)])
def test_dwconv_and_k_partials(device, B, Hh, Ww, heads):
    """Maps that are not powers of two, H W not a multiple of the chunk."""
    E = H.engine()
    lib = E.load()
    inner = 64 * heads
    x = torch.randn(B, Hh, Ww, 3 * inner, generator=H.gen(1))
    ws = [torch.randn(inner, 1, 3, 3, generator=H.gen(2 + i)) / 3 for i in range(3)]
    chunk = lib.kd_linattn_chunk_tokens()
    HW = Hh * Ww
    nch = (HW + chunk - 1) // chunk
    xd, wd = x.to(device), [w.to(device) for w in ws]
    y = torch.full_like(xd, float("nan"))
    part = torch.full((B, nch, inner, 2), float("nan"), device=device)
    E.check(lib.kd_linattn_dwconv_nhwc(E.ptr(xd), E.ptr(wd[0]), E.ptr(wd[1]), E.ptr(wd[2]), E.ptr(y), E.ptr(part), B, Hh, Ww,
                                       heads, E.current_stream()))
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), torch.cat(ws).double(), padding=1, groups=3 * inner).permute(0, 2, 3, 1)
    got = y.cpu()
    assert _rel(got, ref) < KERNEL_REL
    k = got.double()[..., inner:2 * inner].reshape(B, HW, inner)
    kp = F.pad(k, (0, 0, 0, nch * chunk - HW), value=float("-inf")).reshape(B, nch, chunk, inner)
    m = kp.amax(2)
    s = torch.exp(kp - m[:, :, None]).sum(2)
    p = part.cpu().double()
    assert torch.equal(p[..., 0], m)
    assert _rel(p[..., 1], s) < KERNEL_REL


def _partials(k, chunk):   # [B, HW, inner] -> the dwconv kernel's (max, sum exp) per chunk, fp32
    B, HW, inner = k.shape
    nch = (HW + chunk - 1) // chunk
    kp = F.pad(k.double(), (0, 0, 0, nch * chunk - HW), value=float("-inf")).reshape(B, nch, chunk, inner)
    m = kp.amax(2)
    return torch.stack((m, torch.exp(kp - m[:, :, None]).sum(2)), -1).float().contiguous()


@pytest.mark.parametrize("HW,m,null", [(273, 0, False), (273, 5, False), (4113, 37, False), (100, 3, True), (0, 7, True),
                                       (0, 37, False)])
def test_context_reduction(device, HW, m, null):
    E = H.engine()
    lib = E.load()
    B, heads = 2, 3
    inner = 64 * heads
    g = H.gen(HW + m)
    qkv = torch.randn(B, max(HW, 1), 3 * inner, generator=g) * 2
    ckv = torch.randn(B, max(m, 1), 2 * inner, generator=g) * 2
    nkv = torch.randn(2, 64, generator=g)
    k, v = qkv[:, :HW, inner:2 * inner], qkv[:, :HW, 2 * inner:]
    ck, cv = ckv[:, :m, :inner], ckv[:, :m, inner:]
    heads_ = lambda t: t.double().reshape(B, t.shape[1], heads, 64).transpose(1, 2)
    kk = [heads_(k)]
    vv = [heads_(v)]
    if null:
        kk.append(nkv[0].double().expand(B, heads, 1, 64))
        vv.append(nkv[1].double().expand(B, heads, 1, 64))
    kk.append(heads_(ck))
    vv.append(heads_(cv))
    ref = torch.einsum("bhnd,bhne->bhde", torch.cat(kk, 2).softmax(2), torch.cat(vv, 2))
    chunk = lib.kd_linattn_chunk_tokens()
    part = _partials(k, chunk).to(device) if HW else None
    qd, cd, nd = qkv.to(device), ckv.to(device), nkv.to(device)
    ctx = torch.full((B, heads, 64, 64), float("nan"), device=device)
    E.check(lib.kd_linattn_context(_at(qd, inner) if HW else None, _at(qd, 2 * inner) if HW else None, 3 * inner,
                                   E.ptr(part), HW, _at(cd, 0) if m else None, _at(cd, inner) if m else None, 2 * inner, m,
                                   _at(nd, 0) if null else None, _at(nd, 64) if null else None, E.ptr(ctx), B, heads,
                                   E.current_stream()))
    assert _rel(ctx.cpu(), ref) < KERNEL_REL


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("N", [1, 100, 192])
def test_apply(device, N, silu):
    E = H.engine()
    lib = E.load()
    B, heads = 2, 3
    inner = 64 * heads
    g = H.gen(N)
    q = torch.randn(B, N, 3 * inner, generator=g) * 3   # q = columns [0, inner) of a q | k | v map
    ctx = torch.randn(B, heads, 64, 64, generator=g) * 0.1
    qs = q[..., :inner].double().reshape(B, N, heads, 64).softmax(-1) * 0.125
    ref = torch.einsum("bnhd,bhde->bnhe", qs, ctx.double()).reshape(B, N, inner)
    if silu:
        ref = F.silu(ref)
    qd, cd = q.to(device), ctx.to(device)
    out = torch.full((B, N, inner), float("nan"), device=device)
    E.check(lib.kd_linattn_apply(E.ptr(qd), 3 * inner, E.ptr(cd), E.ptr(out), inner, B, N, heads, 0.125, silu,
                                 E.current_stream()))
    assert _rel(out.cpu(), ref) < KERNEL_REL


# ------------------------------------------------------------------------------- the UNet forward
SMALL = dict(dim=32, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
             layer_cross_attns=(False, False, True), use_linear_attn=True, use_linear_cross_attn=(False, True, False))
ULTRA2 = dict(dim=128, dim_mults=(1, 2, 4, 8), num_resnet_blocks=2, memory_efficient=True,
              layer_attns=(False, False, False, True), layer_cross_attns=(False, False, True, True),
              init_conv_to_final_conv_residual=True, cond_images_channels=3,
              use_linear_attn=True, use_linear_cross_attn=True)   # train_ultra_res.py:39-48 + linear attention
SEG = dict(dim=32, dim_mults=(1, 2, 3, 4), cond_dim=64, text_embed_dim=3, num_resnet_blocks=2,
           layer_attns=(False, False, True, True), layer_cross_attns=(False, True, True, True),
           cond_images_channels=4, use_linear_attn=True, use_linear_cross_attn=(True, False, True, False))


_ref_unet = functools.partial(H.ref_unet, LR.Unet)


@pytest.mark.parametrize("case", ["small_b2", "small_b5", "small_self_cond", "ultra2_256_b2", "ultra2_256_b16"])
def test_unet_forward_matches_the_restatement(device, case):
    """ultra2_256_b16: the plan's F(4x4,3x3) layers and bf16x3 1x1 convs in their whole-batch / image-set forms around the
    linear blocks of the 128 x 128 .. 32 x 32 levels (the first one: q | k | v maps of 1.6 GB)."""
    sc = None
    if case.startswith("small"):
        B, S = (5, 32) if case == "small_b5" else (2, 32)
        if case == "small_self_cond":
            ou = H.ref_unet(LR.SelfCondUnet, SMALL, seed=11, self_cond=True)
            sc = torch.rand(B, 3, S, S, generator=H.gen(9)) * 2 - 1
        else:
            ou = _ref_unet(SMALL, seed=11)
    else:
        B, S = (16 if case.endswith("b16") else 2), 256
        ou = H.fast_oracle(_ref_unet(ULTRA2, lowres_cond=True, seed=12))
    x, t, kw = H.unet_inputs(ou, B, S, seed=3)
    if sc is not None:
        kw["self_cond"] = sc   # (drawn last and from a generator of its own: x, t and the other planes are as without it)
    e, _ = H.forward_err(ou, device, x, t, kw)   # (asserts that a second run gives the same bits)
    print(f"linear-attention forward {case}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2


def test_plain_unet_through_the_new_export_keeps_its_plan(device):
    """A UNet without linear attention built through kd_unet_create_ext has the launches and the bits of the plan
    kd_unet_create_shared (= kd_unet_create) builds."""
    E = H.engine()
    lib = E.load()
    ou = _ref_unet(H.UNET_KW["small2"], seed=4, lowres_cond=True)
    a, b = H.product_like(ou, device), H.product_like(ou, device)
    x, t, kw = H.unet_inputs(ou, 2, 32, seed=5)
    dv = {k: v.to(device) for k, v in kw.items()}
    ha = a.engine(2, 32, device, with_text=False)
    orig = lib.kd_unet_create_ext
    lib.kd_unet_create_ext = lambda cfg, arr, n, share, ext, out: lib.kd_unet_create_shared(cfg, arr, n, share, out)
    try:
        hb = b.engine(2, 32, device, with_text=False)
    finally:
        lib.kd_unet_create_ext = orig
    assert lib.kd_unet_num_launches(ha) == lib.kd_unet_num_launches(hb)
    ya = a(x.to(device), t.to(device), **dv)
    yb = b(x.to(device), t.to(device), **dv)
    assert torch.equal(ya, yb)
    ol = _ref_unet(SMALL, seed=6)
    lin = H.product_like(ol, device)
    xl, tl, _ = H.unet_inputs(ol, 2, 32, seed=7)
    lin(xl.to(device), tl.to(device))   # (the profile replays the inputs of the last forward)
    labels = H.plan_csv(lin, 2, 32, device)
    # 2 levels x 2 paths of linear blocks, one LinearCrossAttention on each path of level 1
    assert labels.count("linattn dwconv") == 4 and labels.count("linattn apply") == 4, labels.count("linattn dwconv")
    assert labels.count("linattn xapply") == 2


# ------------------------------------------------------------------------------- sampling
def test_ddpm_text_guided_inpainting_matches_the_restatement(device):
    """T = 4, inpainting with 2 resamples, cond_scale = 3 on a text UNet with linear attention and linear
    cross-attention."""
    ou = _ref_unet(SEG, seed=17, text=True)
    oim, pim = H.imagen_pair(device, RS.Imagen, "Imagen", [ou], image_sizes=(32,), timesteps=(4,), text_embed_dim=3)
    B = 2
    g = H.gen(3)
    text = torch.tensor([0.0, 0.5, 0.2]).reshape(1, 1, 3).repeat_interleave(B, dim=0)
    labels = F.one_hot(torch.randint(0, 4, (B, 32, 32), generator=g), 4).permute(0, 3, 1, 2).float()
    inp = torch.rand(B, 3, 32, 32, generator=g)
    mask = torch.zeros(B, 32, 32, dtype=torch.bool)
    mask[:, 4:20, 6:30] = True
    nf = RS.generator_noise_fn(5)
    kw = dict(cond_scale=3.0, inpaint_resample_times=2)
    ref = oim.sample(noise_fn=nf, text_embeds=text, cond_images=labels, inpaint_images=inp, inpaint_masks=mask, **kw)
    dv = lambda v: v.to(device)
    got = pim.sample(noise_fn=nf, text_embeds=dv(text), cond_images=dv(labels), inpaint_images=dv(inp),
                     inpaint_masks=dv(mask), device=device, **kw).cpu()
    err = float((got - ref).abs().max())
    print(f"linear-attention DDPM text, cond_scale 3, inpainting R=2: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_edm_sampling_matches_the_restatement(device):
    ou = _ref_unet(SMALL, seed=23)
    oim, pim = H.imagen_pair(device, ER.ElucidatedImagen, "ElucidatedImagen", [ou], image_sizes=(32,), condition_on_text=False,
                             num_sample_steps=4)
    nf = RS.generator_noise_fn(13)
    ref = oim.sample(noise_fn=nf, batch_size=2)
    got = pim.sample(noise_fn=nf, batch_size=2, device=device).cpu()
    err = float((got - ref).abs().max())
    print(f"linear-attention EDM, N=4: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_graph_equals_eager_and_table_on_equals_off(device):
    ou = _ref_unet(SMALL, seed=25)
    _, pim = H.imagen_pair(device, RS.Imagen, "Imagen", [ou], image_sizes=(32,), timesteps=(4,), condition_on_text=False)
    nf = RS.generator_noise_fn(7)
    runs = {}
    for use_graph in (True, False):
        for table in (0, -1):
            pim.cond_table = table
            runs[use_graph, table] = pim.sample(noise_fn=nf, batch_size=2, use_graph=use_graph, device=device)
    base = runs[True, 0]
    for key, v in runs.items():
        assert torch.equal(v, base), key
    pim.cond_table = 0
    assert torch.equal(pim.sample(noise_fn=nf, batch_size=2, device=device), base)
