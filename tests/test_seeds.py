"""Per-image seeds on the host side (no GPU): what `Imagen.sample` accepts as `seed`, how `ImagenTrainer.sample` cuts a
seed list alongside the batch, and which seed every patch of a grid gets from `imagen_sample_fn`."""
import pytest
import torch

import helpers as H
from ultra_res import distributed as D


def _imagen():
    import imagen_pytorch as ip

    u = ip.Unet(**H.UNET_KW["small1"], cond_on_text=False, text_embed_dim=None)
    return ip.Imagen([u], image_sizes=(16,), timesteps=2, condition_on_text=False)


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("seed", [[1, 2], [1, -2, 3], torch.tensor([[1, 2, 3]]), torch.zeros(3, 1, dtype=torch.int64),
                                  [1, 2, 2 ** 64], [1.0, 2.0, 3.0], torch.tensor([1.0, 2.0, 3.0]), "123", [1, 2, True]],
                         ids=["short", "negative", "2d", "2d-column", "2^64", "floats", "float-tensor", "str", "bool"])
def test_sample_refuses_bad_per_image_seeds_before_it_asks_for_a_gpu(seed):
    """A wrong length, a value outside [0, 2^64), a 2-D tensor and non-integers raise ValueError - before
    E.require_gpu(), so also where there is no device (EngineUnavailable is a RuntimeError, not a ValueError)."""
    with pytest.raises(ValueError):
        _imagen().sample(batch_size=3, seed=seed)


def test_normalize_seed_accepts_ints_sequences_and_1d_integer_tensors():
    import numpy as np

    from imagen_pytorch.imagen_pytorch import normalize_seed

    assert normalize_seed(None, 3) is None and normalize_seed(7, 3) == 7 and normalize_seed(-5, 3) == -5   # ints: as before
    top = 2 ** 64 - 1
    assert normalize_seed([0, top, 5], 3) == [0, top, 5]
    assert normalize_seed((4, 5), 2) == [4, 5]
    assert normalize_seed(torch.tensor([9, 8, 7]), 3) == [9, 8, 7]
    assert normalize_seed(torch.tensor([9, 8], dtype=torch.int32), 2) == [9, 8]
    assert normalize_seed(np.array([3, 2 ** 40], dtype=np.uint64), 2) == [3, 2 ** 40]
    assert all(type(s) is int for s in normalize_seed(np.array([3, 4]), 2))
    # the batch the seeds are counted against is the one sample() settles on: the inpaint images' for an unconditional model
    im = _imagen()
    with pytest.raises(ValueError, match="2 values for a batch of 3"):
        im.sample(inpaint_images=torch.zeros(3, 3, 16, 16), inpaint_masks=torch.zeros(3, 16, 16, dtype=torch.bool), seed=[1, 2])


# ------------------------------------------------------------------------------------------------ trainer chunks
def _recording_trainer():
    """An ImagenTrainer whose imagen.sample is a stub that records the kwargs of every chunk."""
    from imagen_pytorch import ImagenTrainer

    tr = ImagenTrainer(_imagen(), use_ema=False)
    calls = []

    def sample(*args, **kw):
        calls.append(kw)
        return torch.zeros(kw["batch_size"], 3, 4, 4)

    tr.imagen.sample = sample
    return tr, calls


@pytest.mark.parametrize("as_tensor", [False, True])
def test_trainer_cuts_a_seed_list_alongside_the_batch_and_keeps_the_int_rule(as_tensor):
    tr, calls = _recording_trainer()
    seeds = [1, 2, 3, 4, 5]
    out = tr.sample(batch_size=5, max_batch_size=2, seed=torch.tensor(seeds) if as_tensor else seeds)
    assert out.shape[0] == 5
    assert [c["batch_size"] for c in calls] == [2, 2, 1]
    assert [c["seed"] for c in calls] == [[1, 2], [3, 4], [5]]
    with pytest.raises(ValueError):
        tr.sample(batch_size=5, max_batch_size=2, seed=[1, 2, 3])
    # an int seed: chunk k draws under seed + 1000003 k, as before; no seed: none is handed on
    calls.clear()
    tr.sample(batch_size=5, max_batch_size=2, seed=7)
    assert [c["seed"] for c in calls] == [7, 7 + 1000003, 7 + 2 * 1000003]
    calls.clear()
    tr.sample(batch_size=5, max_batch_size=2)
    assert len(calls) == 3 and all("seed" not in c for c in calls)


# ------------------------------------------------------------------------------------------------ grid seeds
class _SeedImagen:
    """Stub Imagen for imagen_sample_fn: records (batch_size, seed) of every sample() call."""

    def __init__(self):
        self.calls = []

    def to(self, device):
        return self

    def sample(self, **kw):
        self.calls.append((kw["batch_size"], kw.get("seed")))
        return torch.zeros(kw["batch_size"], 3, 4, 4)


def _run_waves(max_batch, per_patch, split=False, seed=5, stage=2):
    """task -> seed over the waves of a 3 x 3 grid; split: every wave's tasks reach the function in two calls (two ranks)."""
    fake = _SeedImagen()
    fn = D.imagen_sample_fn(lambda st: fake, inpaint_resample=2, device=torch.device("cpu"), seed=seed, max_batch=max_batch,
                            per_patch_seeds=per_patch)
    pos = [(i, j) for i in range(3) for j in range(3)]
    got, calls = {}, []
    for wave in D.merged_waves([pos], [-1]):
        parts = [wave[0::2], wave[1::2]] if split else [wave]
        for tasks in (p for p in parts if p):
            n = len(tasks)
            fake.calls.clear()
            fn(stage, tasks, [torch.zeros(3, 2, 2)] * n, [None] * n, [torch.zeros(3, 4, 4)] * n, [torch.zeros(4, 4)] * n)
            calls += fake.calls
            n0 = 0
            for b, s in fake.calls:
                for i in range(b):
                    got[tasks[n0 + i]] = s[i] if isinstance(s, list) else s
                n0 += b
    return got, calls


def _todays_seed(seed, stage, task):
    return seed + 7919 * stage + 104729 * hash(task) % (2 ** 31)


def test_per_patch_seeds_do_not_depend_on_how_a_wave_is_batched_or_split():
    want, calls1 = _run_waves(1, True)
    assert len(want) == 9 and len(set(want.values())) == 9
    assert all(isinstance(s, list) and len(s) == b for b, s in calls1)
    assert want == {t: _todays_seed(5, 2, t) for t in want}   # today's formula, on the patch's own task
    for max_batch in (2, 8):
        got, calls = _run_waves(max_batch, True)
        assert got == want and max(b for b, _ in calls) == min(max_batch, 3)
    assert _run_waves(8, True, split=True)[0] == want
    assert _run_waves({2: 2}, True, split=True)[0] == want
    other, _ = _run_waves(8, True, stage=3)
    assert all(other[t] != want[t] for t in want)   # (the stage is part of the seed)


def test_default_grid_seeds_are_those_of_the_first_task_of_each_call():
    for max_batch in (1, 2, 8):
        fake = _SeedImagen()
        fn = D.imagen_sample_fn(lambda st: fake, inpaint_resample=2, device=torch.device("cpu"), seed=5, max_batch=max_batch)
        pos = [(i, j) for i in range(3) for j in range(3)]
        for wave in D.merged_waves([pos], [-1]):
            n = len(wave)
            fake.calls.clear()
            fn(2, wave, [torch.zeros(3, 2, 2)] * n, [None] * n, [torch.zeros(3, 4, 4)] * n, [torch.zeros(4, 4)] * n)
            firsts = [wave[n0] for n0 in range(0, n, max_batch)]
            assert [s for _, s in fake.calls] == [5 + 7919 * 2 + 104729 * hash(t) % (2 ** 31) for t in firsts]
            assert all(isinstance(s, int) for _, s in fake.calls)
    # and without a seed the scheduler's base_seed path is untouched by the flag
    fake = _SeedImagen()
    fn = D.imagen_sample_fn(lambda st: fake, inpaint_resample=2, device=torch.device("cpu"), max_batch=2, per_patch_seeds=True)
    assert fn.takes_base_seed
    tasks = [(0, 0, k) for k in range(3)]
    fn(2, tasks, [torch.zeros(3, 2, 2)] * 3, [None] * 3, [torch.zeros(3, 4, 4)] * 3, [torch.zeros(4, 4)] * 3, base_seed=100)
    assert fake.calls == [(2, 100), (1, 102)]
