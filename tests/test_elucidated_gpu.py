"""ElucidatedImagen on the MI355X: the EDM Heun sampler of the engine (kd_edm_sample_loop / _steps) against the CPU
restatement in tests/elucidated_ref.py, its kernels against fp64 expressions, and its graph / conditioning-table paths."""
import ctypes as C

import pytest
import torch

import elucidated_ref as ER
import helpers as H
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

SAMPLE_ABS = 2e-3
TRACE_REL_L2 = 2e-3
EDM = (ER.ElucidatedImagen, "ElucidatedImagen")   # (restatement, product class) of H.imagen_pair


def _base(device, N=5):
    return H.imagen_pair(device, *EDM, [H.oracle_unet("small1", seed=3)], image_sizes=(16,), condition_on_text=False,
                         num_sample_steps=N)


def test_base_unet_trace_and_sample_match_the_restatement(device):
    oim, pim = _base(device, N=5)
    nf = RS.generator_noise_fn(11)
    rtrace, ptrace = [], []
    ref = oim.sample(noise_fn=nf, batch_size=2, trace=rtrace)
    got = pim.sample(noise_fn=nf, batch_size=2, trace=ptrace, device=device)
    assert len(ptrace) == len(rtrace) == 5
    for k, (a, b) in enumerate(zip(ptrace, rtrace)):
        assert H.rel_l2(a, b) < TRACE_REL_L2, (k, H.rel_l2(a, b))
    err = float((got.cpu() - ref).abs().max())
    print(f"EDM base, N=5: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_sr_stage_with_cond_images_and_inpainting_matches_the_restatement(device):
    ou = H.oracle_unet("small2", lowres_cond=True, seed=5)
    oim, pim = H.imagen_pair(device, *EDM, [R.NullUnet(), ou], image_sizes=(16, 32), condition_on_text=False, num_sample_steps=3,
                                 sigma_max=(80, 320))
    g = torch.Generator().manual_seed(8)
    B = 2
    start = torch.rand(B, 3, 16, 16, generator=g)
    cond = torch.rand(B, 3, 32, 32, generator=g)
    inp = torch.rand(B, 3, 32, 32, generator=g)
    mask = torch.zeros(B, 32, 32, dtype=torch.bool)
    mask[:, 4:20, 6:30] = True
    nf = RS.generator_noise_fn(12)
    kw = dict(batch_size=B, start_at_unet_number=2, inpaint_resample_times=3)
    ref = oim.sample(noise_fn=nf, start_image_or_video=start, cond_images=cond, inpaint_images=inp, inpaint_masks=mask, **kw)
    dv = lambda v: v.to(device)
    got = pim.sample(noise_fn=nf, start_image_or_video=dv(start), cond_images=dv(cond), inpaint_images=dv(inp),
                     inpaint_masks=dv(mask), device=device, **kw).cpu()
    m = mask[:, None].expand_as(got)
    assert torch.equal(got[m], ref[m]), "known pixels"
    err = float((got - ref).abs().max())
    print(f"EDM SR stage + inpainting (R=3): max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


SEG_KW = dict(dim=32, dim_mults=(1, 2, 3, 4), cond_dim=64, text_embed_dim=3, num_resnet_blocks=2,
              layer_attns=(False, True, True, True), layer_cross_attns=(False, True, True, True),
              cond_images_channels=4)   # train.py:30-39 at reduced dim


@pytest.mark.parametrize("cond_scale,tokens", [pytest.param(1.0, 1, id="1.0"), pytest.param(3.0, 1, id="3.0"),
                                               pytest.param(2.5, 3, id="2.5-three-tokens")])
def test_text_conditioned_sampling_with_guidance_matches_the_restatement(device, cond_scale, tokens):
    """tokens = 3: three embedding rows per sample, the middle one all zero (a false entry in sample()'s default mask): the
    conditioning table and the replayed graphs carry K / V of more than one text token."""
    ou = H.randomize_(R.Unet(**SEG_KW, cond_on_text=True), 17)
    oim, pim = H.imagen_pair(device, *EDM, [ou], image_sizes=(16,), text_embed_dim=3, num_sample_steps=3)
    B = 2
    g = torch.Generator().manual_seed(3)
    text = torch.tensor([0.0, 0.5, 0.2]).reshape(1, 1, 3).repeat_interleave(B, dim=0)
    if tokens == 3:
        text = torch.cat((text, torch.zeros(B, 1, 3), torch.tensor([[[0.3, -0.2, 1.0]], [[-0.6, 0.1, 0.4]]])), dim=1)
        assert torch.any(text != 0.0, dim=-1).tolist() == [[True, False, True]] * B
    labels = torch.nn.functional.one_hot(torch.randint(0, 4, (B, 16, 16), generator=g), 4).permute(0, 3, 1, 2).float()
    nf = RS.generator_noise_fn(5)
    ref = oim.sample(noise_fn=nf, text_embeds=text, cond_images=labels, cond_scale=cond_scale)
    got = pim.sample(noise_fn=nf, text_embeds=text.to(device), cond_images=labels.to(device), cond_scale=cond_scale,
                     device=device)
    err = float((got.cpu() - ref).abs().max())
    print(f"EDM text-conditioned, cond_scale {cond_scale}: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_graph_replay_equals_eager_and_cond_table_on_equals_off(device):
    """Bit for bit: the captured step graphs against eager launches, and the 2N-row conditioning table against the
    conditioning computed in the step; then DDPM sampling on the same UNet still matches its oracle."""
    import imagen_pytorch as ip

    oim, pim = _base(device, N=4)
    nf = RS.generator_noise_fn(21)
    runs = {}
    for use_graph in (True, False):
        for table in (0, -1):
            pim.cond_table = table
            runs[use_graph, table] = pim.sample(noise_fn=nf, batch_size=2, use_graph=use_graph, device=device)
    base = runs[True, 0]
    for key, v in runs.items():
        assert torch.equal(v, base), key
    pu = pim.unets[0]
    h = pu.engine(2, 16, device, with_text=False)
    rows, runs_ = C.c_int(-1), C.c_int(-1)
    assert ip._engine.load().kd_unet_cond_table_build_ms(h, C.byref(rows), C.byref(runs_)) >= 0 and rows.value > 0
    # the same Unet under the DDPM sampler, after the EDM graphs and table rows: re-captures, matches its oracle
    ddpm_o = RS.Imagen([oim.unets[0]], image_sizes=(16,), timesteps=(3,), pred_objectives=("noise",),
                       condition_on_text=False)
    ddpm_p = ip.Imagen([pu], image_sizes=(16,), timesteps=(3,), pred_objectives=("noise",), condition_on_text=False)
    ref = ddpm_o.sample(noise_fn=nf, batch_size=2)
    got = ddpm_p.to(device).sample(noise_fn=nf, batch_size=2, device=device)
    assert float((got.cpu() - ref).abs().max()) < SAMPLE_ABS
    again = pim.sample(noise_fn=nf, batch_size=2, device=device)
    assert torch.equal(again, base)


@pytest.mark.parametrize("sampler", ["ddpm", "edm"])
def test_schedule_length_changing_on_a_live_plan_equals_a_fresh_plan(device, sampler):
    """One SR UNet, one plan, sampled with 3, then 5, then 3 steps through two sampler objects that share the UNet: the
    schedule tables on the device regrow and shrink, the captured iteration and the conditioning table are rebuilt.  Each
    result must be bit-equal to the same call on a plan made fresh by invalidate_engine(): same kernels, same inputs,
    same order."""
    import imagen_pytorch as ip

    pu = H.product_unet_like(H.oracle_unet("small2", lowres_cond=True, seed=5)).to(device)

    def make(steps):
        if sampler == "ddpm":
            return ip.Imagen([ip.NullUnet(), pu], image_sizes=(16, 32), timesteps=(steps, steps), pred_objectives=("noise", "v"),
                             condition_on_text=False).to(device)
        return ip.ElucidatedImagen([ip.NullUnet(), pu], image_sizes=(16, 32), num_sample_steps=steps, sigma_max=(80, 320),
                                   condition_on_text=False).to(device)

    ims = {3: make(3), 5: make(5)}   # (made before the first call: .to() drops the plans)
    g = torch.Generator().manual_seed(14)
    low = torch.rand(2, 3, 16, 16, generator=g).to(device)
    cond = torch.rand(2, 3, 32, 32, generator=g).to(device)
    nf = RS.generator_noise_fn(31)

    def run(steps):
        return ims[steps].sample(noise_fn=nf, batch_size=2, start_at_unet_number=2, start_image_or_video=low, cond_images=cond,
                                 use_graph=True, device=device)

    lengths = (3, 5, 3)
    live = [run(n) for n in lengths]
    assert len(pu._engines) == 1, "the three calls must share one plan"
    for i, n in enumerate(lengths):
        pu.invalidate_engine()
        fresh = run(n)
        assert torch.isfinite(fresh).all() and torch.equal(live[i], fresh), (i, n, float((live[i] - fresh).abs().max()))
    assert not torch.equal(live[0], live[1]), "the schedule length must matter"


def test_seeded_sampling_is_reproducible_and_in_range(device):
    _, pim = _base(device, N=3)
    a = pim.sample(batch_size=2, seed=1234, device=device)
    b = pim.sample(batch_size=2, seed=1234, device=device)
    c = pim.sample(batch_size=2, seed=1235, device=device)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0


# ------------------------------------------------------------------------------- the kernels, through the C ABI
def _abi_setup(device, N=3, B=2, S=16):
    from imagen_pytorch import _engine as E
    from imagen_pytorch.imagen_pytorch import edm_step_tables

    _, pim = _base(device, N=N)
    pu = pim.unets[0]
    h = pu.engine(B, S, device, with_text=False)
    tab = edm_step_tables(**pim.hparams[0])
    sc = E.kd_edm_schedule_t()
    sc.N, sc.S_noise = N, float(pim.hparams[0]["S_noise"])
    for name, _ in E.kd_edm_schedule_t._fields_[2:]:
        setattr(sc, name, tab[name].numpy().ctypes.data_as(C.POINTER(C.c_float)))
    g = torch.Generator().manual_seed(31)
    noise = torch.randn(N, B, 3, S, S, generator=g).to(device)
    args = E.kd_sample_args_t()
    args.dynamic_threshold, args.percentile, args.resample_times = 1, 0.95, 1
    args.d_noise_step = E.ptr(noise)
    args.use_graph = 1
    return E, pu, h, tab, sc, args, noise, g


def _thr(den, s):
    s = s.clamp(min=1.0)[:, None, None, None]
    return torch.maximum(torch.minimum(den, s), -s) / s


def test_edm_kernels_match_fp64_expressions(device):
    """The last step (churn, precondition-out, Euler) and a Heun step (plus the second precondition-out) of
    kd_edm_sample_steps, each output read back through kd_sample_last and recomputed in fp64 from its inputs."""
    E, pu, h, tab, sc, args, noise, g = _abi_setup(device)
    lib, N, B, S = E.load(), 3, 2, 16
    shp = (B, 3, S, S)
    f = lambda name, k: float(tab[name][k])
    for k in (N - 1, 0):
        x0 = (torch.randn(shp, generator=g) * 3).to(device)
        x = x0.clone()
        E.check(lib.kd_edm_sample_steps(h, C.byref(sc), C.byref(args), E.ptr(x), k, k + 1, E.current_stream()))
        net, den, s = H.sample_last(h, 0, shp, device), H.sample_last(h, 1, shp, device), H.sample_last(h, 2, (B,), device)
        xh, d = H.sample_last(h, 3, shp, device), H.sample_last(h, 4, shp, device)
        x0d, z = x0.double().cpu(), noise[k].double().cpu()
        # churn: x_hat = x + churn * (S_noise * z)
        assert H.rel_l2(xh, x0d + f("churn", k) * (float(sc.S_noise) * z)) < 1e-6, k
        # the first forward saw c_in(sigma_hat) x_hat at time c_noise(sigma_hat) (the last step has no second one)
        if k == N - 1:
            t = torch.full((B,), f("c_noise_hat", k), device=device)
            ref_net = pu(torch.tensor(f("c_in_hat", k)) * xh.float().to(device), t)
            assert H.rel_l2(net, ref_net) < 1e-6
            assert H.rel_l2(den, f("c_skip_hat", k) * xh + f("c_out_hat", k) * net) < 1e-6   # precondition-out
            q = torch.quantile(den.flatten(1).abs().float(), 0.95, dim=-1).double()
            assert torch.allclose(s, q.clamp(min=1.0), rtol=1e-6)
            want_d = (xh - _thr(den, s)) / f("sigma_hat", k)   # Euler
            assert H.rel_l2(d, want_d) < 1e-6
            assert H.rel_l2(x, xh + f("euler_step", k) * d) < 1e-6
        else:
            x_next = xh + f("euler_step", k) * d   # Heun: den / s / net are the second forward's
            assert H.rel_l2(den, f("c_skip_next", k) * x_next + f("c_out_next", k) * net) < 1e-5
            d2 = (x_next - _thr(den, s)) / f("sigma_next", k)
            assert H.rel_l2(x, xh + f("heun_step", k) * (d + d2)) < 1e-5


def test_edm_renoise_between_resamples(device):
    """Inpainting with R = 2 on a non-last step: x = Heun(x) + (sigma - sigma_next) z after the first resample only, and
    the known pixels of x_hat are inp + the added churn noise."""
    E, pu, h, tab, sc, args, noise, g = _abi_setup(device)
    lib, N, B, S, Rr = E.load(), 3, 2, 16, 2
    shp = (B, 3, S, S)
    churn = torch.randn(N * Rr, *shp, generator=g).to(device)
    ren = torch.randn(N * Rr, *shp, generator=g).to(device)
    inp = (torch.rand(shp, generator=g) * 2 - 1).to(device)
    mask = torch.zeros(B, 1, S, S)
    mask[:, :, 2:9, 3:14] = 1
    mask = mask.to(device)
    args.resample_times, args.d_noise_step, args.d_noise_renoise = Rr, E.ptr(churn), E.ptr(ren)
    args.d_inpaint_images, args.d_inpaint_masks = E.ptr(inp), E.ptr(mask)
    f = lambda name: float(tab[name][0])
    x = (torch.randn(shp, generator=g) * 3).to(device)
    x_start = x.clone()
    # step k = 0: iteration r = 1 (churn[0], then re-noise ren[0]), then r = 0 (churn[1], no re-noise)
    E.check(lib.kd_edm_sample_steps(h, C.byref(sc), C.byref(args), E.ptr(x), 0, 1, E.current_stream()))
    xh = H.sample_last(h, 3, shp, device)
    m = mask.bool().expand(shp).cpu()
    want_known = inp.double().cpu() + f("churn") * (float(sc.S_noise) * churn[1].double().cpu())
    assert H.rel_l2(xh[m], want_known[m]) < 1e-6
    # the second iteration's x_hat = (first iteration's result incl. re-noise) + churn: recover that result
    x1 = xh - f("churn") * (float(sc.S_noise) * churn[1].double().cpu())
    # the first iteration alone (R = 1 reads churn slot 0 as well): Heun(x) without the re-noise
    args2 = E.kd_sample_args_t.from_buffer_copy(args)
    args2.resample_times = 1
    args2.d_noise_renoise = None
    y = x_start.clone()
    E.check(lib.kd_edm_sample_steps(h, C.byref(sc), C.byref(args2), E.ptr(y), 0, 1, E.current_stream()))
    want = y.double().cpu() + f("renoise") * ren[0].double().cpu()
    assert H.rel_l2(x1[~m], want[~m]) < 1e-5


# ------------------------------------------------------------------------------- full dims (train_ultra_res.py:39-48)
ULTRA2 = dict(dim=128, dim_mults=(1, 2, 4, 8), num_resnet_blocks=2, memory_efficient=True,
              layer_attns=(False, False, False, True), layer_cross_attns=(False, False, True, True),
              init_conv_to_final_conv_residual=True, cond_images_channels=3)


def test_ultra_res_unet2_full_dims_matches_the_restatement(device):
    ou = H.fast_oracle(H.randomize_(R.Unet(**ULTRA2, lowres_cond=True, **H.NOTEXT), 82).eval())
    oim, pim = H.imagen_pair(device, *EDM, [R.NullUnet(), ou], image_sizes=(64, 256), condition_on_text=False, num_sample_steps=3,
                                 sigma_max=(80, 320))
    g = torch.Generator().manual_seed(9)
    B = 2
    start = torch.rand(B, 3, 64, 64, generator=g)
    cond = torch.rand(B, 3, 256, 256, generator=g)
    nf = RS.generator_noise_fn(41)
    rtrace, ptrace = [], []
    ref = oim.sample(noise_fn=nf, batch_size=B, start_image_or_video=start, cond_images=cond, start_at_unet_number=2,
                     trace=rtrace)
    got = pim.sample(noise_fn=nf, batch_size=B, start_image_or_video=start.to(device), cond_images=cond.to(device),
                     start_at_unet_number=2, trace=ptrace, device=device)
    for k, (a, b) in enumerate(zip(ptrace, rtrace)):
        assert H.rel_l2(a, b) < TRACE_REL_L2, (k, H.rel_l2(a, b))
    err = float((got.cpu() - ref).abs().max())
    print(f"EDM ultra-res unet2 full dims, B=2, N=3: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
