"""Self-conditioned UNets (library `Unet(self_cond=True)`) on the MI355X: the 6-plane init conv kernel against fp64, the
UNet forward and both samplers against the restatement in tests/self_cond_ref.py, and the engine's carried estimate
(graph / eager, conditioning table, split step ranges, kd_sample_set_self_cond, launch counts)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import helpers as H
import self_cond_ref as SR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

CONV_REL = 2e-6      # as test_kernels_gpu.py
FWD_REL_L2 = 2e-5
SAMPLE_ABS = 2e-3
DDPM, EDM = (SR.Imagen, "Imagen"), (SR.ElucidatedImagen, "ElucidatedImagen")   # (restatement, product class) of H.imagen_pair


# ------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("B,S,n3,n7,n15", [
    (2, 64, 64, 32, 32),      # dim 128: the SR UNets' init conv (two 32-row tiles for the k = 3 conv)
    (1, 32, 16, 8, 8),        # dim 32 (test UNets): partial 32-row tiles
    (3, 96, 32, 16, 16),      # dim 64, S not a power of two, tiles cross image borders on every side
])
def test_init_conv_six_planes(device, B, S, n3, n7, n15, with_res):
    """The per-step share of a self-conditioned UNet's init convs: planes x | self_cond (input channels c0 .. c0 + 5 of
    weights over 8 channels) in one launch, + bias or + a step-invariant residual, against torch conv2d in fp64."""
    E = H.engine()
    lib = E.load()
    Itot, c0, C_ = 8, 2, n3 + n7 + n15
    x = torch.randn(B, 3, S, S, generator=H.gen(1))
    sc = torch.rand(B, 3, S, S, generator=H.gen(2)) * 2 - 1
    ws = [torch.randn(n, Itot, k, k, generator=H.gen(10 + k)) * (6 * k * k) ** -0.5 for n, k in ((n3, 3), (n7, 7), (n15, 15))]
    inp = torch.cat((x, sc), 1)
    res = torch.randn(B, S, S, C_, generator=H.gen(5)) if with_res else None
    b = None if with_res else torch.randn(C_, generator=H.gen(4))
    add = (res.permute(0, 3, 1, 2) if with_res else b[None, :, None, None])
    parts64 = [F.conv2d(inp.double(), w[:, c0:c0 + 6].double(), padding=w.shape[-1] // 2) for w in ws]
    ref = torch.cat(parts64, 1) + add.double()
    ref32 = torch.cat([F.conv2d(inp, w[:, c0:c0 + 6], padding=w.shape[-1] // 2) for w in ws], 1) + add
    xd, scd = x.to(device), sc.to(device)
    wd = [w.to(device) for w in ws]
    bd = None if b is None else b.to(device)
    rd = None if res is None else res.to(device)
    y = torch.full((B, S, S, C_), float("nan"), device=device)
    E.check(lib.kd_init_conv_planes_nchw(E.ptr(xd), E.ptr(scd), E.ptr(wd[0]), E.ptr(wd[1]), E.ptr(wd[2]), Itot, c0,
                                         E.ptr(bd), E.ptr(rd), E.ptr(y), B, S, n3, n7, n15, 1, None, E.current_stream()))
    got = y.permute(0, 3, 1, 2).cpu()
    assert torch.isfinite(got).all()
    err = float((got.double() - ref).norm() / ref.norm())
    err_cpu = float((ref32.double() - ref).norm() / ref.norm())
    assert err <= max(3 * err_cpu, CONV_REL), (err, err_cpu)
    for sl, p64 in zip((slice(0, n3), slice(n3, n3 + n7), slice(n3 + n7, None)), parts64):
        e = float((got[:, sl].double() - (p64 + add[:, sl].double())).norm() / p64.norm())
        assert e <= max(3 * err_cpu, CONV_REL), (sl, e)


# ------------------------------------------------------------------------------- the UNet forward
_ref_unet = functools.partial(H.ref_unet, SR.Unet, self_cond=True)
ULTRA2 = dict(dim=128, dim_mults=(1, 2, 4, 8), num_resnet_blocks=2, memory_efficient=True,
              layer_attns=(False, False, False, True), layer_cross_attns=(False, False, True, True),
              init_conv_to_final_conv_residual=True, cond_images_channels=3)   # train_ultra_res.py:39-48


@pytest.mark.parametrize("case", ["base", "sr", "sr_generic", "ultra2_b16"])
def test_unet_forward_with_self_cond_matches_the_restatement(device, case):
    """sr_generic: 48 px, a size the fused kernel refuses (S % 32 != 0): the generic path (6 planes + 2 zero channels,
    three implicit-GEMM convs)."""
    if case == "base":
        kw, lowres, B, S = H.UNET_KW["small1"], False, 2, 32
    elif case == "ultra2_b16":
        kw, lowres, B, S = ULTRA2, True, 16, 64
    else:
        kw, lowres, B, S = H.UNET_KW["small2"], True, 2, 48 if case == "sr_generic" else 32
    ou = _ref_unet(kw, lowres_cond=lowres, seed=11)
    if case == "ultra2_b16":
        ou = H.fast_oracle(ou)
    pu = H.product_like(ou, device)
    g = H.gen(3)
    x = torch.randn(B, 3, S, S, generator=g)
    sc = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    t = torch.randn(B, generator=g) * 3
    kw_in = {}
    if lowres:
        kw_in.update(lowres_cond_img=torch.randn(B, 3, S, S, generator=g), lowres_noise_times=torch.full((B,), 1.5))
    if ou.has_cond_image:
        kw_in["cond_images"] = torch.rand(B, 3, S, S, generator=g)
    with torch.no_grad():
        ref = ou(x, t, self_cond=sc, **kw_in)
        ref0 = ou(x, t, **kw_in)
    dv = {k: v.to(device) for k, v in kw_in.items()}
    got = pu(x.to(device), t.to(device), self_cond=sc.to(device), **dv).cpu()
    got0 = pu(x.to(device), t.to(device), **dv).cpu()
    e, e0 = H.rel_l2(got, ref), H.rel_l2(got0, ref0)
    print(f"self-cond forward {case}: rel-L2 {e:.2e} (self_cond None: {e0:.2e})")
    assert e < FWD_REL_L2 and e0 < FWD_REL_L2
    assert H.rel_l2(ref, ref0) > 1e-3   # the self_cond planes matter


def test_fused_plan_has_the_plain_plans_launch_count(device):
    E = H.engine()
    lib = E.load()
    counts = []
    for self_cond in (False, True):
        pu = H.product_like(_ref_unet(H.UNET_KW["small2"], lowres_cond=True, seed=2, self_cond=self_cond), device)
        h = pu.engine(2, 32, device, with_text=False)
        counts.append(lib.kd_unet_num_launches(h))
    assert counts[0] == counts[1]


# ------------------------------------------------------------------------------- DDPM sampling
@pytest.mark.parametrize("objective,dyn", [("noise", True), ("v", False), ("v", True)])
def test_ddpm_base_sampling_matches_the_restatement(device, objective, dyn):
    oim, pim = H.imagen_pair(device, *DDPM, [_ref_unet(H.UNET_KW["small1"], seed=21)], image_sizes=(32,),
                             timesteps=(4,), pred_objectives=(objective,), dynamic_thresholding=(dyn,), condition_on_text=False)
    nf = RS.generator_noise_fn(31)
    ref = oim.sample(noise_fn=nf, batch_size=2)
    got = pim.sample(noise_fn=nf, batch_size=2, device=device).cpu()
    err = float((got - ref).abs().max())
    print(f"self-cond DDPM base {objective} dyn={dyn}: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_ddpm_sr_stage_with_inpainting_matches_the_restatement(device):
    """Mixed cascade (only unet2 self-conditioned), SR + cond images + inpainting with R = 2: x_start carries across
    resamples."""
    u2 = _ref_unet(H.UNET_KW["small2"], lowres_cond=True, seed=22)
    oim, pim = H.imagen_pair(device, *DDPM, [R.NullUnet(), u2], image_sizes=(16, 32), timesteps=(3, 3),
                             condition_on_text=False)
    assert pim.unets[1].self_cond
    g = H.gen(8)
    B = 2
    start = torch.rand(B, 3, 16, 16, generator=g)
    cond = torch.rand(B, 3, 32, 32, generator=g)
    inp = torch.rand(B, 3, 32, 32, generator=g)
    mask = torch.zeros(B, 32, 32, dtype=torch.bool)
    mask[:, 4:20, 6:30] = True
    nf = RS.generator_noise_fn(12)
    kw = dict(batch_size=B, start_at_unet_number=2, inpaint_resample_times=2)
    ref = oim.sample(noise_fn=nf, start_image_or_video=start, cond_images=cond, inpaint_images=inp, inpaint_masks=mask, **kw)
    dv = lambda v: v.to(device)
    got = pim.sample(noise_fn=nf, start_image_or_video=dv(start), cond_images=dv(cond), inpaint_images=dv(inp),
                     inpaint_masks=dv(mask), device=device, **kw).cpu()
    err = float((got - ref).abs().max())
    print(f"self-cond DDPM SR + inpainting (R=2): max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


SEG_KW = dict(dim=32, dim_mults=(1, 2, 3, 4), cond_dim=64, text_embed_dim=3, num_resnet_blocks=2,
              layer_attns=(False, True, True, True), layer_cross_attns=(False, True, True, True),
              cond_images_channels=4)   # train.py:30-39 at reduced dim


def test_ddpm_text_guided_sampling_matches_the_restatement(device):
    ou = _ref_unet(SEG_KW, seed=17, text=True)
    oim, pim = H.imagen_pair(device, *DDPM, [ou], image_sizes=(32,), timesteps=(3,), text_embed_dim=3)
    B = 2
    g = H.gen(3)
    text = torch.tensor([0.0, 0.5, 0.2]).reshape(1, 1, 3).repeat_interleave(B, dim=0)
    labels = F.one_hot(torch.randint(0, 4, (B, 32, 32), generator=g), 4).permute(0, 3, 1, 2).float()
    nf = RS.generator_noise_fn(5)
    ref = oim.sample(noise_fn=nf, text_embeds=text, cond_images=labels, cond_scale=2.5)
    got = pim.sample(noise_fn=nf, text_embeds=text.to(device), cond_images=labels.to(device), cond_scale=2.5,
                     device=device).cpu()
    err = float((got - ref).abs().max())
    print(f"self-cond DDPM text, cond_scale 2.5: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


# ------------------------------------------------------------------------------- EDM sampling
def test_edm_base_sampling_matches_the_restatement(device):
    oim, pim = H.imagen_pair(device, *EDM, [_ref_unet(H.UNET_KW["small1"], seed=23)],
                             image_sizes=(32,), condition_on_text=False, num_sample_steps=4)
    nf = RS.generator_noise_fn(13)
    ref = oim.sample(noise_fn=nf, batch_size=2)
    got = pim.sample(noise_fn=nf, batch_size=2, device=device).cpu()
    err = float((got - ref).abs().max())
    print(f"self-cond EDM base, N=4: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_edm_sr_stage_with_inpainting_matches_the_restatement(device):
    u2 = _ref_unet(H.UNET_KW["small2"], lowres_cond=True, seed=24)
    oim, pim = H.imagen_pair(device, *EDM, [R.NullUnet(), u2], image_sizes=(16, 32),
                             condition_on_text=False, num_sample_steps=3, sigma_max=(80, 320))
    g = H.gen(9)
    B = 2
    start = torch.rand(B, 3, 16, 16, generator=g)
    cond = torch.rand(B, 3, 32, 32, generator=g)
    inp = torch.rand(B, 3, 32, 32, generator=g)
    mask = torch.zeros(B, 32, 32, dtype=torch.bool)
    mask[:, 4:20, 6:30] = True
    nf = RS.generator_noise_fn(14)
    kw = dict(batch_size=B, start_at_unet_number=2, inpaint_resample_times=2)
    ref = oim.sample(noise_fn=nf, start_image_or_video=start, cond_images=cond, inpaint_images=inp, inpaint_masks=mask, **kw)
    dv = lambda v: v.to(device)
    got = pim.sample(noise_fn=nf, start_image_or_video=dv(start), cond_images=dv(cond), inpaint_images=dv(inp),
                     inpaint_masks=dv(mask), device=device, **kw).cpu()
    err = float((got - ref).abs().max())
    print(f"self-cond EDM SR + inpainting (R=2): max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


# ------------------------------------------------------------------------------- the carried estimate in the engine
def test_graph_equals_eager_table_on_equals_off_and_split_ranges_equal_one_call(device):
    """Bit for bit: captured graph against eager launches, the conditioning table on against off, and per-step calls
    (trace: kd_sample_steps(k, k + 1), continuing from the estimate the plan holds) against one kd_sample_loop; for the
    DDPM and the EDM sampler."""
    u = _ref_unet(H.UNET_KW["small2"], lowres_cond=True, seed=25)
    ikw = dict(image_sizes=(16, 32), condition_on_text=False)
    for make in (lambda: H.imagen_pair(device, *DDPM, [R.NullUnet(), u], timesteps=(4, 4), **ikw),
                 lambda: H.imagen_pair(device, *EDM, [R.NullUnet(), u], num_sample_steps=4, **ikw)):
        _, pim = make()
        start = torch.rand(2, 3, 16, 16, generator=H.gen(1)).to(device)
        nf = RS.generator_noise_fn(7)
        kw = dict(noise_fn=nf, batch_size=2, start_at_unet_number=2, start_image_or_video=start,
                  cond_images=torch.rand(2, 3, 32, 32, generator=H.gen(2)).to(device), device=device)
        runs = {}
        for use_graph in (True, False):
            for table in (0, -1):
                pim.cond_table = table
                runs[use_graph, table] = pim.sample(use_graph=use_graph, **kw)
        base = runs[True, 0]
        for key, v in runs.items():
            assert torch.equal(v, base), (type(pim).__name__, key)
        pim.cond_table = 0
        assert torch.equal(pim.sample(trace=[], **kw), base), type(pim).__name__


def test_set_self_cond_then_one_step_matches_one_restated_step(device):
    E = H.engine()
    lib = E.load()
    ou = _ref_unet(H.UNET_KW["small1"], seed=26)
    oim, pim = H.imagen_pair(device, *DDPM, [ou], image_sizes=(32,), timesteps=(5,), condition_on_text=False)
    pu = pim.unets[0]
    B, S, T, k = 2, 32, 5, 2
    h = pu.engine(B, S, device, with_text=False)
    tables = pim.noise_schedulers[0].step_tables()
    sc = E.kd_schedule_t()
    sc.T = T
    for name, v in tables.items():
        setattr(sc, name, v.numpy().ctypes.data_as(C.POINTER(C.c_float)))
    g = H.gen(6)
    noise = torch.randn(T, B, 3, S, S, generator=g)
    x = torch.randn(B, 3, S, S, generator=g)
    xs = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    args = E.kd_sample_args_t()
    args.objective, args.dynamic_threshold, args.percentile, args.resample_times = 0, 1, 0.95, 1
    nd = noise.to(device)
    args.d_noise_step = E.ptr(nd)
    args.use_graph = 1
    xd, xsd = x.to(device), xs.to(device)
    E.check(lib.kd_sample_set_self_cond(h, E.ptr(xsd), E.current_stream()))
    E.check(lib.kd_sample_steps(h, C.byref(sc), C.byref(args), E.ptr(xd), k, k + 1, E.current_stream()))
    carried = torch.empty(B, 3, S, S, device=device)
    E.check(lib.kd_sample_last(h, 5, E.ptr(carried), E.current_stream()))
    sched = oim.noise_schedulers[0]
    times, times_next = sched.get_sampling_timesteps(B)[k]
    with torch.no_grad():
        want, want_xs = RS.Imagen.p_sample(
            oim, SR._SelfCondCall(ou, xs), x, times, noise[k], noise_scheduler=sched, t_next=times_next, text_embeds=None,
            text_mask=None, cond_images=None, lowres_cond_img=None, lowres_noise_times=None, cond_scale=1.0,
            pred_objective="noise", dynamic_threshold=True)
    err = float((xd.cpu() - want).abs().max())
    print(f"one restated step from a seeded x_start: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
    assert H.rel_l2(carried, want_xs) < 1e-4


def test_zeroed_self_cond_weights_sample_like_the_plain_unet(device):
    """A self-cond UNet whose self_cond input weights are zero samples within fp32 rounding of the same UNet without
    self_cond (fused kernel at 32 px, DDPM and EDM).  The init conv sums in another order; EDM starts at sigma = 80, so
    its rounding reaches the sample at the 1e-4 level (the engine against the fp32 CPU restatement: 7e-5 above)."""
    ou = _ref_unet(H.UNET_KW["small1"], seed=27)
    with torch.no_grad():
        for i in range(3):
            ou.init_conv.convs[i].weight[:, SR.self_cond_channels(ou)] = 0.0
    plain = R.Unet(**H.UNET_KW["small1"], **H.NOTEXT).eval()
    plain.load_state_dict(SR.plain_state_dict(ou.state_dict(), ou), strict=True)
    nf = RS.generator_noise_fn(15)
    for cls, tol in ((DDPM, 1e-5), (EDM, 5e-4)):
        kw = dict(timesteps=(4,)) if cls is DDPM else dict(num_sample_steps=4)
        _, a = H.imagen_pair(device, *cls, [ou], image_sizes=(32,), condition_on_text=False, **kw)
        _, b = H.imagen_pair(device, *cls, [plain], image_sizes=(32,), condition_on_text=False, **kw)
        assert a.unets[0].self_cond and not b.unets[0].self_cond
        sa = a.sample(noise_fn=nf, batch_size=2, device=device).cpu()
        sb = b.sample(noise_fn=nf, batch_size=2, device=device).cpu()
        err = float((sa - sb).abs().max())
        print(f"{cls[1]}: zeroed self-cond weights vs plain: max|diff| {err:.2e}")
        assert err < tol
