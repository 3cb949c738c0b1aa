"""The UNet's scalar constructor options on the MI355X against the oracle: num_time_tokens, learned_sinu_pos_emb_dim,
resnet_groups, ff_mult, attn_heads, attend_at_middle, use_global_context_attn, cond_dim, attn_pool_num_latents and
max_text_len, each at values no other suite runs (tests/unet_options_cases.py) - the forward of a narrow model and of the
smallest model the default fast plan engages on (also under the fp32-MFMA and the direct-conv plans), the plans the
structural options must build (kd_unet_profile labels, launch counts), both samplers over a cascade of such UNets, graph /
eager / conditioning-table bit identity, and a strict ImagenTrainer.load.  Bounds: the project's own (tests/test_unet_gpu.py).

What the engine refuses is decided in Unet.__init__ and tested in tests/test_unet_options.py, never here."""
import functools

import pytest
import torch

import elucidated_ref as ER
import helpers as H
import self_cond_ref as SR
import unet_options_cases as OC
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

FWD_REL_L2 = 2e-5
SAMPLE_ABS = 2e-3
PLANS = {"default": {}, "fp32_mfma": dict(gemm_bf16x3=-1), "direct": dict(conv_algo=1)}


@pytest.fixture(scope="module")
def oracle():
    """case name -> (oracle UNet, inputs, oracle output): computed once, shared unchanged by the plan variants of a case."""
    done = {}

    def get(name):
        if name not in done:
            ou = OC.oracle_unet(name)
            x, t, kw = OC.inputs(ou, OC.ALL[name])
            with torch.no_grad():
                done[name] = (ou, (x, t, kw), ou(x, t, **kw))
        return done[name]

    return get


def _forward_err(oracle, name, device, **plan):
    ou, (x, t, kw), ref = oracle(name)
    return H.forward_err(ou, device, x, t, kw, ref=ref, **plan)


def _handle(pu, case, device):
    return pu.engine(case["B"], case["S"], device, with_text=bool(case["text"]))


def _case_labels(pu, case, device):
    return H.plan_labels(_handle(pu, case, device))


_count = H.count_labels


def _check_gca_rows(pu, labels):
    """One GlobalContext launch (rows "gca_gate" / "gca_pool") per ResnetBlock that has the module; its gate is applied by
    "gate_add" where the block has no 1x1 skip conv and by that conv's epilogue where it has one.  final_res_block has the
    module whatever use_global_context_attn says (the library builds it with use_gca=True)."""
    blocks = [n[:-4] for n, _ in pu.named_modules() if n.endswith(".gca")]
    plain = [b for b in blocks if not hasattr(pu.get_submodule(b), "res_conv")]
    assert _count(labels, "gca_gate", "gca_pool") == len(blocks), (labels, blocks)
    assert _count(labels, "gate_add") == len(plain), (labels, plain)
    return blocks


# ------------------------------------------------------------------------------- a. forward, narrow model
@pytest.mark.parametrize("name", list(OC.FORWARD))
def test_forward_matches_the_oracle(device, oracle, name):
    e, _ = _forward_err(oracle, name, device)
    print(f"options forward {name} B={OC.ALL[name]['B']}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2


@pytest.mark.parametrize("name", ["no_gca", "no_gca_mem_eff", "mults_113_no_gca", "everything"])
def test_without_global_context_only_final_res_block_is_gated(device, oracle, name):
    """use_global_context_attn=False: the ResnetBlocks end in block2's conv with the residual in its epilogue (no skip conv)
    or in the skip conv with block2's output as its residual - no GlobalContext launch and no gate_add but final_res_block's."""
    case = OC.ALL[name]
    ou, (x, t, kw), _ = oracle(name)
    pu = H.product_like(ou, device)
    pu(x.to(device), t.to(device), **{k: v.to(device) for k, v in kw.items()})
    labels = _case_labels(pu, case, device)
    assert _check_gca_rows(pu, labels) == ["final_res_block"]
    assert _count(labels, "gate_add") == (0 if case["kw"].get("init_conv_to_final_conv_residual") else 1)
    # the same model with GlobalContext on has a gated launch per inner ResnetBlock more
    on = H.product_like(SR.Unet(**{**ou._locals, "use_global_context_attn": True}), device)
    on(x.to(device), t.to(device), **{k: v.to(device) for k, v in kw.items()})
    assert len(_check_gca_rows(on, _case_labels(on, case, device))) > 1


def test_attend_at_middle_off_drops_the_middle_transformer(device, oracle):
    case = OC.ALL["no_mid_attn"]
    ou, (x, t, kw), _ = oracle("no_mid_attn")
    lib = H.engine().load()
    off = H.product_like(ou, device)
    on = H.product_like(SR.Unet(**{**ou._locals, "attend_at_middle": True}), device)
    n_off, n_on = (lib.kd_unet_num_launches(_handle(u, case, device)) for u in (off, on))
    print(f"options attend_at_middle: {n_on} launches with the middle TransformerBlock, {n_off} without")
    assert n_off < n_on
    rows = {}
    for key, u in (("off", off), ("on", on)):
        u(x.to(device), t.to(device))
        rows[key] = _count(_case_labels(u, case, device), "attn N")
    # self-attention launches: a TransformerBlock on the down and the up path of levels 1 and 2, and the middle one
    assert rows == {"off": 4, "on": 5}


# ------------------------------------------------------------------------------- b. forward, fast plan
def _gn_rows(labels):
    """The plan's GroupNorm statistics launches in order: ("fold" | "stats", channels)."""
    return [("fold" if l.startswith("gn fold seg") else "stats", int(l.rsplit(" C", 1)[1]))
            for l in labels if l.startswith(("gn stats", "gn fold seg"))]


@pytest.fixture(scope="module")
def default_gn_rows(device):
    """_gn_rows of trajectory_ref.MODEL_A's plan with the default resnet_groups = 8 (product only, built once)."""
    done = []

    def get(case, inputs):
        if not done:
            x, t, _ = inputs
            p8 = H.product_like(SR.Unet(**case["base"], **H.NOTEXT), device)
            p8(x.to(device), t.to(device))
            done.append(_gn_rows(_case_labels(p8, case, device)))
        return done[0]

    return get


@pytest.mark.parametrize("name", list(OC.FAST))
def test_fast_plan_forward_matches_the_oracle(device, oracle, default_gn_rows, name):
    case = OC.ALL[name]
    e, pu = _forward_err(oracle, name, device)
    print(f"options forward {name} B={case['B']}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = _case_labels(pu, case, device)
    n_stats, n_fold = _count(labels, "gn stats"), _count(labels, "gn fold seg")
    print(f"  {n_stats} 'gn stats' rows, {n_fold} 'gn fold seg' rows, {_count(labels, 'wino4_in')} F(4x4,3x3) layers, "
          f"{len(labels)} launches")
    assert _count(labels, "wino4_in") >= 1 and _count(labels, "wino4 gemm bf16x3") >= 1   # the fast plan engaged
    G = case["kw"].get("resnet_groups")
    if G:
        # Builder::seg_sources: a GroupNorm folds its statistics from its producer's 16-channel partials (row "gn fold seg")
        # where its groups are 16 n channels wide AND a producer left partials for all its channels, else it takes a pass
        # over the map (row "gn stats").  Which producers leave partials does not depend on the groups, so against the plan of
        # the same model with the default 8 groups (group widths 16 n at every layer of it): a layer that takes the pass
        # there takes it here, and one that folds there folds here exactly where C / G is a multiple of 16
        rows8 = default_gn_rows(OC.ALL[name], oracle(name)[1])
        want = [(kind if kind == "stats" or (c // G) % 16 == 0 else "stats", c) for kind, c in rows8]
        assert all((c // 8) % 16 == 0 for _, c in rows8)
        assert _gn_rows(labels) == want, (_gn_rows(labels), want)
        if G == 32:    # 128- and 256-wide layers and the 384- and 768-wide concats take the pass, 512 and 1024 fold
            assert n_stats > _count([k for k, _ in rows8], "stats") and n_fold >= 1
        if G == 4:     # the same layers fold as with 8 groups
            assert _gn_rows(labels) == rows8 and n_fold >= 1
    if name == "fast_no_gca":
        assert _check_gca_rows(pu, labels) == ["final_res_block"]


@pytest.mark.parametrize("plan", ["fp32_mfma", "direct"])
@pytest.mark.parametrize("name", ["fast_groups_32", "fast_no_gca"])
def test_fast_model_forward_on_the_other_plans(device, oracle, name, plan):
    case = OC.ALL[name]
    e, pu = _forward_err(oracle, name, device, **PLANS[plan])
    print(f"options forward {name} plan {plan}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = _case_labels(pu, case, device)
    if plan == "fp32_mfma":
        assert not any("x3" in l for l in labels), [l for l in labels if "x3" in l]
    else:
        assert not any("wino" in l or "x3" in l for l in labels), [l for l in labels if "wino" in l or "x3" in l]


# ------------------------------------------------------------------------------- c. sampling
_ref_unet = functools.partial(H.ref_unet, SR.Unet)


def _cascade(device, cls_o, cls_p, seed, **kw):
    ous = [_ref_unet(OC.BASE, seed=seed), _ref_unet(OC.SR2, seed=seed + 1, lowres_cond=True)]
    return H.imagen_pair(device, cls_o, cls_p, ous, image_sizes=(32, 64), condition_on_text=False, **kw)


def test_ddpm_cascade_with_inpainting_matches_the_oracle(device):
    oim, pim = _cascade(device, SR.Imagen, "Imagen", 51, **OC.DDPM_KW)
    B = 2
    g = torch.Generator().manual_seed(3)
    inp = torch.rand(B, 3, 64, 64, generator=g)
    mask = torch.zeros(B, 64, 64, dtype=torch.bool)
    mask[:, 8:40, 12:60] = True
    nf = RS.generator_noise_fn(5)
    kw = dict(batch_size=B, inpaint_resample_times=2)
    ref = oim.sample(noise_fn=nf, inpaint_images=inp, inpaint_masks=mask, **kw)
    got = pim.sample(noise_fn=nf, inpaint_images=inp.to(device), inpaint_masks=mask.to(device), device=device, **kw).cpu()
    assert got.shape == (B, 3, 64, 64)
    err = float((got - ref).abs().max())
    print(f"options DDPM cascade 32 -> 64, T=4, linear / cosine, inpainting R=2: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_edm_cascade_matches_the_oracle(device):
    oim, pim = _cascade(device, ER.ElucidatedImagen, "ElucidatedImagen", 53, num_sample_steps=3)
    nf = RS.generator_noise_fn(13)
    ref = oim.sample(noise_fn=nf, batch_size=2)
    got = pim.sample(noise_fn=nf, batch_size=2, device=device).cpu()
    err = float((got - ref).abs().max())
    print(f"options EDM cascade 32 -> 64, N=3: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS


def test_graph_equals_eager_and_table_on_equals_off(device):
    _, pim = _cascade(device, SR.Imagen, "Imagen", 55, **OC.DDPM_KW)
    nf = RS.generator_noise_fn(7)
    runs = {}
    for use_graph in (True, False):
        for table in (0, -1):
            pim.cond_table = table
            runs[use_graph, table] = pim.sample(noise_fn=nf, batch_size=2, use_graph=use_graph, device=device)
    base = runs[True, 0]
    for key, v in runs.items():
        assert torch.equal(v, base), key


def test_trainer_loads_a_checkpoint_of_the_base_unet_strictly_and_samples_from_it(device, tmp_path, capsys):
    import imagen_pytorch as ip

    kw = dict(image_sizes=(32,), timesteps=(4,), condition_on_text=False)
    online, ema_u = _ref_unet(OC.BASE, seed=61), _ref_unet(OC.BASE, seed=62)
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
    print(f"options trainer.sample from the EMA weights: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
    assert float((ref - oim_online.sample(noise_fn=nf, batch_size=2)).abs().max()) > 10 * SAMPLE_ABS
