"""Images of 1, 2 or 4 channels (`Unet(channels=C)`): what the constructor accepts and refuses, and the parameter layout
against the oracle's.  No GPU."""
import pytest
import torch

import helpers as H
import self_cond_ref as SR
from oracle import imagen_ref as R

KW = dict(lowres_cond=True, cond_on_text=False, text_embed_dim=None)


def _same_layout_and_strict_load(pu, ou):
    ps, os_ = pu.state_dict(), ou.state_dict()
    assert list(ps.keys()) == list(os_.keys())
    assert {k: tuple(v.shape) for k, v in ps.items()} == {k: tuple(v.shape) for k, v in os_.items()}
    pu.load_state_dict(os_, strict=True)
    for k, v in pu.state_dict().items():
        assert torch.equal(v, os_[k]), k


@pytest.mark.parametrize("C", [1, 2, 4])
def test_unet_of_c_channels_has_the_oracles_parameters(C):
    import imagen_pytorch as ip

    pu = ip.Unet(**H.UNET_KW["small2"], channels=C, **KW)
    ou = H.randomize_(R.Unet(**H.UNET_KW["small2"], channels=C, **KW), 3)
    assert pu.channels == C and pu.channels_out == C
    # cond_images (3) | x (C) | lowres (C) in, C out
    assert pu.init_conv.convs[0].weight.shape[1] == 3 + 2 * C
    assert pu.final_conv.weight.shape[:2] == (C, 32 + C)
    _same_layout_and_strict_load(pu, ou)


@pytest.mark.parametrize("C", [1, 2, 4])
def test_self_cond_unet_of_c_channels_has_the_restatements_parameters(C):
    import imagen_pytorch as ip

    pu = ip.Unet(**H.UNET_KW["small2"], channels=C, self_cond=True, **KW)
    ou = H.randomize_(SR.Unet(**H.UNET_KW["small2"], channels=C, self_cond=True, **KW), 4)
    assert pu.init_conv.convs[0].weight.shape[1] == 3 + 3 * C   # cond_images | x | self_cond | lowres
    _same_layout_and_strict_load(pu, ou)


@pytest.mark.parametrize("kw", [dict(channels=5), dict(channels=0), dict(channels=1, channels_out=2)])
def test_other_channel_counts_stay_refused(kw):
    import imagen_pytorch as ip

    with pytest.raises(NotImplementedError):
        ip.Unet(**H.UNET_KW["small2"], **kw, **KW)


def test_imagen_casts_its_unets_to_its_channels():
    """Imagen(channels=C) re-creates a default (3-channel) UNet with C channels, as the library does."""
    import imagen_pytorch as ip

    u1 = ip.Unet(**H.UNET_KW["small1"], cond_on_text=False, text_embed_dim=None)
    u2 = ip.Unet(**H.UNET_KW["small2"], cond_on_text=False, text_embed_dim=None)
    im = ip.Imagen([u1, u2], image_sizes=(16, 32), channels=1, condition_on_text=False)
    assert [u.channels for u in im.unets] == [1, 1] and [u.channels_out for u in im.unets] == [1, 1]
    assert im.unets[1].lowres_cond and im.unets[1].final_conv.weight.shape[:2] == (1, 33)
