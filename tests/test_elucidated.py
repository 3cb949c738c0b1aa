"""ElucidatedImagen without a GPU: the host tables of the EDM sampler against the restatement (tests/elucidated_ref.py),
the reference's constructor (train.py:97-110), and the checkpoint layout shared with Imagen."""
import math

import pytest
import torch
from torch import nn

import elucidated_ref as ER
import helpers as H


def _fixed_null_unet_cls():   # train.py:70-80
    import imagen_pytorch as ip

    class FixedNullUnet(ip.NullUnet):
        def __init__(self, lowres_cond=False, *args, **kwargs):
            super().__init__()
            self.lowres_cond = lowres_cond
            self.dummy_parameter = nn.Parameter(torch.tensor([0.]))

        def cast_model_parameters(self, *args, **kwargs):
            return self

        def forward(self, x, *args, **kwargs):
            return x

    return FixedNullUnet


@pytest.mark.parametrize("hp", [dict(), dict(num_sample_steps=5, sigma_max=320), dict(num_sample_steps=3, sigma_max=1280,
                                                                                       S_churn=0.0)])
def test_step_tables_equal_the_restatement(hp):
    import imagen_pytorch.imagen_pytorch as P

    full = {**ER.HPARAM_DEFAULTS, **hp}
    tab = P.edm_step_tables(**full)
    ref = ER.ElucidatedImagen([H.oracle_unet("small1")], image_sizes=(16,), condition_on_text=False)
    sigmas, gammas = ref.sample_schedule(full)
    N, sd = full["num_sample_steps"], full["sigma_data"]
    assert torch.equal(tab["init_sigma"], sigmas[0])
    for k in range(N):
        sigma, sigma_next, gamma = (t.item() for t in (sigmas[k], sigmas[k + 1], gammas[k]))
        sigma_hat = sigma + gamma * sigma
        want = dict(sigma=sigma, sigma_hat=sigma_hat, sigma_next=sigma_next,
                    churn=math.sqrt(sigma_hat ** 2 - sigma ** 2), euler_step=sigma_next - sigma_hat,
                    heun_step=0.5 * (sigma_next - sigma_hat), renoise=sigma - sigma_next)
        for name, v in want.items():
            assert tab[name][k].item() == torch.tensor(v, dtype=torch.float32).item(), (name, k)
        for tag, sg in (("hat", sigma_hat), ("next", sigma_next)):
            s1 = torch.full((1,), sg, dtype=torch.float32)
            assert tab[f"c_in_{tag}"][k] == ref.c_in(sd, s1)[0], (tag, k)
            assert tab[f"c_skip_{tag}"][k] == ref.c_skip(sd, s1)[0], (tag, k)
            assert tab[f"c_out_{tag}"][k] == ref.c_out(sd, s1)[0], (tag, k)
            assert tab[f"c_noise_{tag}"][k] == ref.c_noise(s1)[0], (tag, k)
    assert tab["sigma_next"][N - 1] == 0 and bool((tab["sigma_next"][: N - 1] > 0).all())


def _unet(kind):
    return H.product_unet_like(H.oracle_unet(kind, lowres_cond=kind == "small2", seed=4))


def test_reference_constructor_builds():
    """train.py:97-110 as written (unet 2 real, the others FixedNullUnet), at reduced UNet dims."""
    import imagen_pytorch as ip

    FixedNullUnet = _fixed_null_unet_cls()
    unet = ip.Unet(dim=32, cond_dim=64, text_embed_dim=3, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True),
                   layer_cross_attns=(False, True), memory_efficient=True, init_conv_to_final_conv_residual=True,
                   cond_images_channels=4)
    imagen = ip.ElucidatedImagen(
        unets=(FixedNullUnet(), unet, FixedNullUnet(lowres_cond=True)),
        image_sizes=(64, 256, 1024),
        cond_drop_prob=0.1,
        num_sample_steps=(32, 128, 128),
        text_embed_dim=3,
        random_crop_sizes=(None, None, 256),
        sigma_min=0.002,
        sigma_max=(80, 320, 1280),
    )
    assert isinstance(imagen, ip.Imagen) and len(imagen.unets) == 3
    assert [h["num_sample_steps"] for h in imagen.hparams] == [32, 128, 128]
    assert [h["sigma_max"] for h in imagen.hparams] == [80, 320, 1280]
    assert all(h["sigma_min"] == 0.002 and h["S_noise"] == 1.003 for h in imagen.hparams)
    assert imagen.step_tables(3)["sigma"].shape == (128,)
    assert float(imagen.step_tables(2)["init_sigma"]) == pytest.approx(320.0)
    with pytest.raises(NotImplementedError):
        imagen(torch.zeros(1, 3, 64, 64))


def test_state_dict_keys_equal_imagens():
    import imagen_pytorch as ip

    kw = dict(image_sizes=(16, 32), condition_on_text=False)
    a = ip.Imagen([_unet("small1"), _unet("small2")], timesteps=(3, 3), **kw)
    b = ip.ElucidatedImagen([_unet("small1"), _unet("small2")], num_sample_steps=(3, 4), **kw)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].shape == sb[k].shape for k in sa)


def test_imagen_checkpoint_loads_strictly_through_the_trainer(tmp_path):
    import imagen_pytorch as ip

    kw = dict(image_sizes=(16, 32), condition_on_text=False)
    src = ip.Imagen([_unet("small1"), _unet("small2")], timesteps=(3, 3), **kw)
    with torch.no_grad():
        for i, p in enumerate(src.parameters()):
            p.add_(0.01 * (i + 1))
    ema = {f"{i}.ema_model.{k}": v + 1.0 for i, u in enumerate(src.unets) for k, v in u.state_dict().items()}
    path = tmp_path / "ckpt.pt"
    torch.save({"model": src.state_dict(), "ema": ema, "version": ip.__version__, "steps": torch.tensor([2, 5])}, path)
    dst = ip.ElucidatedImagen([H.product_unet_like(H.oracle_unet("small1", seed=9)),
                               H.product_unet_like(H.oracle_unet("small2", lowres_cond=True, seed=9))],
                              num_sample_steps=3, **kw)
    trainer = ip.ImagenTrainer(imagen=dst)
    trainer.load(str(path))
    got, want = dst.state_dict(), src.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    for i, e in enumerate(trainer.ema_unets):
        for k, v in e.state_dict().items():
            assert torch.equal(v, ema[f"{i}.ema_model.{k}"]), (i, k)
    assert trainer.steps.tolist() == [2, 5]
    # restore_parts (the partial path of ImagenTrainer.load) maps an Imagen checkpoint onto the same keys
    assert set(ip.restore_parts(dst.state_dict(), src.state_dict())) == set(want)
