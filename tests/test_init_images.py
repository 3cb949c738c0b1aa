"""sample(init_images=..., skip_steps=...) without a GPU: the restatement tests/init_images_ref.py held to the oracle, the
argument rules of normalize_init_images, torch's nearest index rule as the start kernel states it, and the trainer's chunks."""
import pytest
import torch
import torch.nn.functional as F

import elucidated_ref as ER
import helpers as H
import init_images_ref as IR
from oracle import sampler_ref as RS


# ------------------------------------------------------------------------------------------------ the restatement
def _unets():
    return [H.oracle_unet("small1", seed=3), H.oracle_unet("small1", lowres_cond=True, seed=6)]


@pytest.mark.parametrize("sampler", ["ddpm", "edm"])
def test_restatement_with_a_zero_image_and_no_skip_is_the_oracle(sampler):
    """init_images = 0.5 normalises to exactly 0 and skip_steps = 0 walks every step: the oracle's sample, bit for bit."""
    if sampler == "ddpm":
        kw = dict(image_sizes=(16, 32), timesteps=(3, 2), pred_objectives=("noise", "noise"), condition_on_text=False)
        oim, rim = RS.Imagen(_unets(), **kw), IR.Imagen(_unets(), **kw)
    else:
        kw = dict(image_sizes=(16,), condition_on_text=False, num_sample_steps=3)
        oim, rim = ER.ElucidatedImagen(_unets()[:1], **kw), IR.ElucidatedImagen(_unets()[:1], **kw)
    nf = RS.generator_noise_fn(11)
    want = oim.sample(noise_fn=nf, batch_size=2)
    assert torch.equal(rim.sample(noise_fn=nf, batch_size=2), want)                       # no arguments: the parent's loop
    half = torch.full((2, 3, 24, 20), 0.5)
    got = rim.sample(noise_fn=nf, batch_size=2, init_images=half, skip_steps=0)
    assert torch.equal(got, want)
    # ... and both arguments do something: another image, fewer steps, one trace entry per step walked
    g = torch.Generator().manual_seed(2)
    init = torch.rand(2, 3, 16, 16, generator=g)
    trace = []
    moved = rim.sample(noise_fn=nf, batch_size=2, init_images=init, skip_steps=1, trace=trace, stop_at_unet_number=1)
    assert len(trace) == 2 and not torch.equal(moved, oim.sample(noise_fn=nf, batch_size=2, stop_at_unet_number=1))


# ------------------------------------------------------------------------------------------------ the argument rules
def _norm(*a, **k):
    from imagen_pytorch.imagen_pytorch import normalize_init_images

    return normalize_init_images(*a, **{**dict(steps=[8, 5], batch_size=3, channels=3), **k})


def test_arguments_are_cast_per_unet():
    t = torch.rand(3, 3, 16, 16)
    t2 = torch.rand(3, 3, 37, 50, dtype=torch.float64)
    assert _norm(None, None) == [(None, 0), (None, 0)]
    out = _norm(t, 4)
    assert [s for _, s in out] == [4, 4] and out[0][0] is t and out[1][0] is t
    out = _norm((None, t2), (3, None))
    assert out[0] == (None, 3) and out[1][0] is t2 and out[1][1] == 0
    out = _norm([t, None], [0, 4])                                                       # lists as tuples
    assert out[0][0] is t and out[0][1] == 0 and out[1] == (None, 4)


def test_entries_of_unets_not_sampled_are_ignored():
    t = torch.rand(3, 3, 16, 16)
    bad = torch.rand(2, 1, 4)                                                            # no image at all
    # skip 7 fits unet 1 (T = 8) alone: a call that stops at unet 1 takes it, one that samples unet 2 does not
    out = _norm(t, 7, stop_at_unet_number=1)
    assert out[0][0] is t and out[0][1] == 7 and out[1] == (None, 0)
    with pytest.raises(ValueError, match="skip_steps=7 of unet 2"):
        _norm(t, 7)
    out = _norm((bad, t), (99, 2), start_at_unet_number=2)
    assert out[0] == (None, 0) and out[1][0] is t and out[1][1] == 2
    out = _norm((t, bad), (1, -5), stop_at_unet_number=1)
    assert out[0][0] is t and out[0][1] == 1 and out[1] == (None, 0)


def test_every_refusal_is_a_value_error():
    t = torch.rand(3, 3, 16, 16)
    for skip in (-1, 8, (0, 5), (8, 0)):                                                 # outside 0 .. T-1 (N-1) of its unet
        with pytest.raises(ValueError, match="outside 0"):
            _norm(t, skip)
    assert [s for _, s in _norm(t, (7, 4))] == [7, 4]                                    # the last step of each is in range
    for skip in (1.0, "2", True):
        with pytest.raises(ValueError, match="must be an int"):
            _norm(t, skip)
    with pytest.raises(ValueError, match="one per unet"):
        _norm(t, (1, 2, 3))
    with pytest.raises(ValueError, match="one per unet"):
        _norm((t,), 0)
    for bad in (torch.rand(3, 16, 16), torch.rand(2, 3, 16, 16), torch.rand(3, 1, 16, 16), torch.rand(3, 3, 16, 0),
                torch.rand(3, 3, 4, 4, 4)):
        with pytest.raises(ValueError, match=r"must be \[batch 3, channels 3, H, W\]"):
            _norm(bad, 0)
    for dtype in (torch.int32, torch.int64, torch.bool):
        with pytest.raises(ValueError, match="floating dtype or uint8"):
            _norm(torch.ones(3, 3, 8, 8, dtype=dtype), 0)
    with pytest.raises(ValueError, match="tensor or None"):
        _norm([[1.0]], 0, steps=[8])


def test_uint8_images_are_divided_by_255():
    u8 = torch.randint(0, 256, (3, 3, 9, 11), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    (got, skip), _ = _norm((u8, None), 2)
    assert skip == 2 and got.dtype == torch.float32 and torch.equal(got, u8.float() / 255.0)


def test_sample_refuses_bad_arguments_before_it_asks_for_a_gpu():
    import imagen_pytorch as ip

    im = ip.Imagen([ip.Unet(dim=32, dim_mults=(1, 2), cond_on_text=False)], image_sizes=(16,), timesteps=4,
                   condition_on_text=False)
    with pytest.raises(ValueError, match="outside 0"):
        im.sample(batch_size=2, skip_steps=4)
    with pytest.raises(ValueError, match="must be"):
        im.sample(batch_size=2, init_images=torch.rand(3, 3, 16, 16))
    el = ip.ElucidatedImagen([ip.Unet(dim=32, dim_mults=(1, 2), cond_on_text=False)], image_sizes=(16,), num_sample_steps=5,
                             condition_on_text=False)
    with pytest.raises(ValueError, match="skip_steps=5 of unet 1 is outside 0 .. 4"):
        el.sample(batch_size=1, skip_steps=5)
    for name in ("texts", "video_frames"):                                               # what stays refused
        with pytest.raises(NotImplementedError):
            im.sample(batch_size=1, **{name: ["x"]})


# ------------------------------------------------------------------------------------------------ the index rule
@pytest.mark.parametrize("n_out", [16, 32, 48, 64])
def test_index_rule_equals_f_interpolate(n_out):
    """src = min(int(floor(fp32(dst) * (fp32(in) / fp32(out)))), in - 1), what kd_sample_start computes on both axes."""
    for n_in in range(1, 300):
        src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
        want = F.interpolate(src, (1, n_out), mode="nearest").flatten().long().tolist()
        assert [IR.nearest_index(d, n_in, n_out) for d in range(n_out)] == want, n_in


# ------------------------------------------------------------------------------------------------ the trainer's chunks
class _Recorder:
    unconditional = True
    unets = ()
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def sample(self, *args, **kw):
        self.calls.append((args, kw))
        return torch.zeros(kw["batch_size"], 3, 4, 4)


@pytest.mark.parametrize("form", ["tensor", "tuple", "list"])
def test_trainer_chunks_cut_init_images_like_the_batch(form):
    from imagen_pytorch import ImagenTrainer

    tr = ImagenTrainer.__new__(ImagenTrainer)
    torch.nn.Module.__init__(tr)
    tr.imagen = _Recorder()
    a, b = torch.arange(5.0).reshape(5, 1, 1, 1).expand(5, 3, 8, 8), torch.arange(5.0, 10.0).reshape(5, 1, 1, 1).expand(5, 3, 6, 7)
    init = {"tensor": a, "tuple": (a, None, b), "list": [None, b, a]}[form]
    out = tr._sample_in_chunks(2, batch_size=5, init_images=init, skip_steps=(3, 5, 1), seed=[1, 2, 3, 4, 5])
    assert tuple(out.shape) == (5, 3, 4, 4)
    assert [kw["batch_size"] for _, kw in tr.imagen.calls] == [2, 2, 1]
    n0 = 0
    for _, kw in tr.imagen.calls:
        n1 = n0 + kw["batch_size"]
        got = kw["init_images"]
        assert kw["skip_steps"] == (3, 5, 1) and kw["seed"] == [1, 2, 3, 4, 5][n0:n1]
        if form == "tensor":
            assert torch.equal(got, a[n0:n1])
        else:
            assert type(got) is type(init) and len(got) == 3
            for g, w in zip(got, init):
                assert (g is None and w is None) or torch.equal(g, w[n0:n1])
        n0 = n1
