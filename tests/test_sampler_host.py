"""The host side that Imagen.sample and Imagen.sample_tiled share, without a GPU: the schedule object that owns the arrays
its ctypes struct points into, the iterator over the stages of a call, and the stage bookkeeping of ultra_res.tiled."""
import gc

import pytest
import torch


def _read(struct, name, n):
    return torch.tensor([getattr(struct, name)[i] for i in range(n)], dtype=torch.float32)


def _churn():
    """Freed table memory, if any, is handed out again and overwritten."""
    gc.collect()
    return [torch.full((6,), float("nan")) for _ in range(256)]


@pytest.mark.parametrize("sampler,eta,skip", [("ddpm", 0.0, 0), ("ddim", 0.5, 0), ("dpmpp_2m", 0.0, 2)])
def test_step_schedule_owns_the_arrays_of_its_struct(sampler, eta, skip):
    from imagen_pytorch import _engine as E
    from imagen_pytorch import imagen_pytorch as M

    sched = M.GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=6)
    tables = sched.step_tables()
    sc = M._StepSchedule(tables, sampler, eta, skip)
    del tables
    junk = _churn()
    want = sched.step_tables()
    if sampler == "ddpm":
        assert isinstance(sc.struct, E.kd_schedule_t) and (sc.steps, sc.loop) == ("kd_sample_steps", "kd_sample_loop")
    else:
        want.update(M.solver_tables(sched.step_tables(), sampler, eta=eta, skip=skip))
        assert isinstance(sc.struct, E.kd_solver_schedule_t)
        assert (sc.steps, sc.loop) == ("kd_solver_sample_steps", "kd_solver_sample_loop")
    assert sc.T == sc.struct.T == 6
    names = [n for n, _ in sc.struct._fields_[1:]]
    assert len(names) == 9 and set(names) <= set(want)
    for n in names:
        assert torch.equal(_read(sc.struct, n, 6), want[n]), n
    assert sc.steps in E.SIGNATURES and sc.loop in E.SIGNATURES
    del junk


def test_edm_schedule_owns_the_arrays_of_its_struct():
    from imagen_pytorch import _engine as E
    from imagen_pytorch import imagen_pytorch as M

    tables = M.edm_step_tables(num_sample_steps=5)
    sc = M._StepSchedule.edm(tables, 1.003)
    del tables
    junk = _churn()
    want = M.edm_step_tables(num_sample_steps=5)
    assert isinstance(sc.struct, E.kd_edm_schedule_t) and (sc.steps, sc.loop) == ("kd_edm_sample_steps", "kd_edm_sample_loop")
    assert sc.steps in E.SIGNATURES and sc.loop in E.SIGNATURES
    assert sc.T == sc.struct.N == 5 and sc.struct.S_noise == pytest.approx(1.003, rel=1e-7)
    names = [n for n, _ in sc.struct._fields_[2:]]
    assert len(names) == 15
    for n in names:
        assert torch.equal(_read(sc.struct, n, 5), want[n]), n
    del junk


def _cascade(**kw):
    import imagen_pytorch as ip

    unet = lambda: ip.Unet(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False)
    return ip.Imagen([ip.NullUnet(), unet(), unet()], image_sizes=(8, 16, 32), timesteps=(8, 8, 6), condition_on_text=False,
                     pred_objectives=("noise", "v", "x_start"), dynamic_thresholding=(True, False, True), **kw)


def test_stage_iterator_walks_start_to_stop_on_the_stage_steps():
    im = _cascade()
    ones = (1.0, 1.0, 1.0)
    solvers = im._solver_args(("ddpm", "ddim", "dpmpp_2m"), (0.0, 0.5, 0.0), (None, 4, None))
    got = list(im._stages(solvers, ones, 2))
    assert [g[0] for g in got] == [2, 3] and [g[1] for g in got] == [im.unets[1], im.unets[2]]
    assert [g[2].num_timesteps for g in got] == [4, 6] and got[1][2] is im.noise_schedulers[2]
    assert got[0][2].noise_schedule == im.noise_schedulers[1].noise_schedule
    assert [g[3:] for g in got] == [("v", False, 1.0, ("ddim", 0.5)), ("x_start", True, 1.0, ("dpmpp_2m", 0.0))]
    assert [g[0] for g in im._stages(solvers, ones, 2, 2)] == [2]
    assert [g[0] for g in im._stages(solvers, ones, 3, 3)] == [3]
    assert [g[0] for g in im._stages(solvers, ones, 3)] == [3]


def test_stage_iterator_owns_the_two_asserts():
    im = _cascade()
    solvers = im._solver_args(None, 0.0, None)
    with pytest.raises(AssertionError, match="one cannot sample from null / placeholder unets"):
        next(im._stages(solvers, (1.0, 1.0, 1.0)))
    stages = im._stages(solvers, (1.0, 1.0, 3.0), 2)
    assert next(stages)[0] == 2   # a stage is refused when it is reached, as in the loop it replaces
    with pytest.raises(AssertionError, match="one cannot use classifier free guidance"):
        next(stages)


def test_tiled_stage_bookkeeping():
    from ultra_res import tiled as UT

    assert UT._check_stages([1, 2, 3], True) == (1, 2, 3) and UT._check_stages((2.0, 3), False) == (2, 3)
    assert UT._check_stages((1,), True) == (1,)
    for stages, from_one, match in (((), False, "in ascending order, got \\(\\)"), ((0, 1), False, "consecutive unet numbers in"),
                                    ((1, 3), False, "consecutive"), ((2, 1), False, "consecutive"),
                                    ((2, 3), True, "consecutive unet numbers from 1 in ascending order, got \\(2, 3\\)"),
                                    ((), True, "from 1")):
        with pytest.raises(ValueError, match=match):
            UT._check_stages(stages, from_one)
    assert UT._per_unet({2: "ddim"}, None, 3) == (None, "ddim", None)
    assert UT._per_unet({1: 0.5, 3: 1.0, 4: 0.1}, 0.0, 3) == (0.5, 0.0, 1.0)
    assert UT._per_unet("ddim", None, 3) == "ddim" and UT._per_unet(None, None, 2) is None
    assert UT._per_unet((4, None), None, 2) == (4, None)
