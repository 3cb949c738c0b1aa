"""Self-conditioned UNets (library `Unet(self_cond=True)`) without a GPU: the constructor and init-conv shape, the
checkpoint layout and strict loading through ImagenTrainer, and the restatement in tests/self_cond_ref.py."""
import pytest
import torch

import helpers as H
import self_cond_ref as SR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS


def _product(name, self_cond, lowres_cond=False, seed=0):
    import imagen_pytorch as ip

    kw = dict(H.UNET_KW[name])
    return H.randomize_(ip.Unet(**kw, lowres_cond=lowres_cond, cond_on_text=False, text_embed_dim=None,
                                self_cond=self_cond), seed)


@pytest.mark.parametrize("name,lowres", [("small1", False), ("small2", True), ("ultra1", False)])
def test_self_cond_unet_constructs_with_wider_init_conv(name, lowres):
    u = _product(name, True, lowres_cond=lowres)
    cond = H.UNET_KW[name].get("cond_images_channels", 0)
    want = 3 * (2 + int(lowres)) + cond
    for i in range(3):
        assert u.init_conv.convs[i].weight.shape[1] == want, i
    assert u.self_cond


def test_state_dict_keys_equal_the_plain_unets():
    a, b = _product("small2", True, lowres_cond=True), _product("small2", False, lowres_cond=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    diff = [k for k in sa if sa[k].shape != sb[k].shape]
    assert sorted(diff) == [f"init_conv.convs.{i}.weight" for i in range(3)]


def test_cast_model_parameters_keeps_self_cond():
    import imagen_pytorch as ip

    u1, u2 = _product("small1", True), _product("small2", False)
    im = ip.Imagen([u1, u2], image_sizes=(16, 32), timesteps=(2, 2), condition_on_text=False)
    assert im.unets[0].self_cond and not im.unets[1].self_cond
    assert im.unets[1].lowres_cond
    # a self-cond UNet recast as an SR stage keeps self_cond and gets the low-res channels too
    im2 = ip.Imagen([_product("small1", False), _product("small2", True)], image_sizes=(16, 32), timesteps=(2, 2),
                    condition_on_text=False)
    assert im2.unets[1].self_cond and im2.unets[1].init_conv.convs[0].weight.shape[1] == 3 * 3 + 3
    el = ip.ElucidatedImagen([_product("small1", True)], image_sizes=(16,), num_sample_steps=2, condition_on_text=False)
    assert el.unets[0].self_cond


def _imagens(self_cond_src, self_cond_dst, seed_dst=9):
    import imagen_pytorch as ip

    kw = dict(image_sizes=(16, 32), timesteps=(3, 3), condition_on_text=False)
    src = ip.Imagen([_product("small1", self_cond_src), _product("small2", self_cond_src, lowres_cond=True)], **kw)
    dst = ip.Imagen([_product("small1", self_cond_dst, seed=seed_dst),
                     _product("small2", self_cond_dst, lowres_cond=True, seed=seed_dst)], **kw)
    return src, dst


def test_self_cond_checkpoint_loads_strictly_through_the_trainer(tmp_path, monkeypatch):
    import imagen_pytorch as ip
    import imagen_pytorch.trainer as T

    src, dst = _imagens(True, True)
    with torch.no_grad():
        for i, p in enumerate(src.parameters()):
            p.add_(0.01 * (i + 1))
    ema = {f"{i}.ema_model.{k}": v + 1.0 for i, u in enumerate(src.unets) for k, v in u.state_dict().items()}
    path = tmp_path / "ckpt.pt"
    torch.save({"model": src.state_dict(), "ema": ema, "version": ip.__version__, "steps": torch.tensor([2, 5])}, path)

    def no_partial(*a, **k):
        raise AssertionError("the partial-load fallback ran")

    monkeypatch.setattr(T, "restore_parts", no_partial)
    trainer = ip.ImagenTrainer(imagen=dst)
    trainer.load(str(path))
    got, want = dst.state_dict(), src.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    for i, e in enumerate(trainer.ema_unets):
        for k, v in e.state_dict().items():
            assert torch.equal(v, ema[f"{i}.ema_model.{k}"]), (i, k)
    # the constructor decides: a plain Imagen refuses the checkpoint on a strict load
    _, plain = _imagens(True, False)
    with pytest.raises(RuntimeError):
        plain.load_state_dict(src.state_dict(), strict=True)
    # and restore_parts, the partial path, reports the init-conv shape mismatch
    lines = []
    ip.restore_parts(plain.state_dict(), src.state_dict(), report=lines.append)
    assert any("init_conv.convs.0.weight" in ln for ln in lines), lines


# ------------------------------------------------------------------------------- the restatement
def _ref_unet(name, lowres=False, seed=0, self_cond=True):
    kw = dict(H.UNET_KW[name])
    return H.randomize_(SR.Unet(**kw, lowres_cond=lowres, cond_on_text=False, text_embed_dim=None, self_cond=self_cond),
                        seed)


def test_restated_self_cond_none_equals_zeros():
    u = _ref_unet("small2", lowres=True, seed=2).eval()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 16, 16, generator=g)
    lr = torch.randn(2, 3, 16, 16, generator=g)
    cond = torch.rand(2, 3, 16, 16, generator=g)
    t, lt = torch.tensor([0.3, -1.0]), torch.tensor([2.0, 2.0])
    kw = dict(lowres_cond_img=lr, lowres_noise_times=lt, cond_images=cond)
    with torch.no_grad():
        a = u(x, t, **kw)
        b = u(x, t, self_cond=torch.zeros_like(x), **kw)
        c = u(x, t, self_cond=torch.randn(x.shape, generator=g), **kw)
    assert torch.equal(a, b)
    assert not torch.allclose(a, c)


def test_restated_unet_with_zeroed_self_cond_weights_equals_the_plain_oracle():
    u = _ref_unet("small2", lowres=True, seed=3).eval()
    with torch.no_grad():
        for i in range(3):
            u.init_conv.convs[i].weight[:, SR.self_cond_channels(u)] = 0.0
    plain = R.Unet(**H.UNET_KW["small2"], lowres_cond=True, cond_on_text=False, text_embed_dim=None).eval()
    plain.load_state_dict(SR.plain_state_dict(u.state_dict(), u), strict=True)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 16, 16, generator=g)
    kw = dict(lowres_cond_img=torch.randn(2, 3, 16, 16, generator=g), lowres_noise_times=torch.tensor([2.0, 2.0]),
              cond_images=torch.rand(2, 3, 16, 16, generator=g))
    with torch.no_grad():
        a = u(x, torch.tensor([0.5, 0.1]), self_cond=torch.randn(x.shape, generator=g), **kw)
        b = plain(x, torch.tensor([0.5, 0.1]), **kw)
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), float((a - b).abs().max())


def test_restated_ddpm_carries_x_start_across_resamples_and_steps():
    """2 timesteps x R = 2 resamples: the first iteration of a stage is fed zeros (None), every later one the previous
    iteration's thresholded x_start; a plain stage in the same cascade is fed nothing."""
    u1 = _ref_unet("small2", seed=5, self_cond=False)
    u2 = _ref_unet("small2", lowres=True, seed=6)
    im = SR.Imagen([u1, u2], image_sizes=(8, 16), timesteps=(2, 2), condition_on_text=False)
    im.x_start_log = log = []
    B = 1
    g = torch.Generator().manual_seed(4)
    inp = torch.rand(B, 3, 16, 16, generator=g)
    mask = torch.zeros(B, 16, 16, dtype=torch.bool)
    mask[:, 2:9, 3:12] = True
    im.sample(noise_fn=RS.generator_noise_fn(3), batch_size=B, cond_images=torch.rand(B, 3, 16, 16, generator=g),
              inpaint_images=inp, inpaint_masks=mask, inpaint_resample_times=2)
    assert len(log) == 2 * 2   # only the self-cond stage: T = 2 steps x R = 2
    assert log[0][0] is None
    for (fed, _), (_, prev) in zip(log[1:], log[:-1]):
        assert fed is prev
    for _, xs in log:
        assert float(xs.abs().max()) <= 1.0


def test_restated_edm_feeds_the_first_estimate_to_the_heun_forward():
    u = _ref_unet("small1", seed=7)
    im = SR.ElucidatedImagen([u], image_sizes=(8,), num_sample_steps=3, condition_on_text=False)
    fed = []
    orig = u.forward

    def spy(x, time, *, self_cond=None, **kw):
        fed.append(self_cond)
        return orig(x, time, self_cond=self_cond, **kw)

    u.forward = spy
    outs = []
    base = SR.ElucidatedImagen.preconditioned

    def record(self, *a, **k):
        o = base(self, *a, **k)
        outs.append(o)
        return o

    SR.ElucidatedImagen.preconditioned = record
    try:
        im.sample(noise_fn=RS.generator_noise_fn(8), batch_size=1)
    finally:
        SR.ElucidatedImagen.preconditioned = base
    # 3 steps: two forwards on steps 0 and 1, one on the last
    assert len(fed) == len(outs) == 5
    assert fed[0] is None
    for i in range(1, 5):
        assert fed[i] is outs[i - 1]
