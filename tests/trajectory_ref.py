"""TEST INFRASTRUCTURE ONLY: long sampling trajectories of the CPU oracle, and what a forward error of the size the suite
tolerates (FWD_REL_L2 of tests/test_unet_gpu.py) does to them.  No product imports.

* ``CONFIGS``: the trajectory configurations - the smallest shapes at which the engine's default plan leaves the direct
  convolutions (dim 128, batch 4, 64 x 64: Winograd F(4x4,3x3) on bf16x3 at the 64 x 64 level, the batched F(2x2,3x3) GEMMs
  below it, matrix-core attention over 256 queries), one per sampler feedback path: plain DDPM, the SR call shape with
  inpainting resampling, EDM Heun, self-conditioning.
* ``PLANS``: the plan variants (attributes of the product UNet) the GPU test runs a configuration under.
* ``perturbed``: the oracle UNet with an error of relative size eps added to every output.
* ``deviation``: per-step rel-L2 / max-abs of a trajectory against another.
* ``envelope``: per step, the largest deviation the three perturbation modes cause - the tolerance of
  tests/test_trajectory_gpu.py, stored by tests/golden/make_trajectory_envelopes.py.
"""
from __future__ import annotations

import contextlib

import torch

import elucidated_ref as ER
import helpers as H
import self_cond_ref as SR
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

FWD_REL_L2 = 2e-5      # restated from tests/test_unet_gpu.py (test_trajectory.py holds the two equal)
MODES = ("rand", "fixed", "scale")

MODEL_A = dict(dim=128, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
               layer_cross_attns=(False, False, True))
MODEL_B = dict(H.UNET_KW["ultra2"], dim=128)

# attributes set on the product UNet before its plan is built (the plan options of kd_unet_config_t)
PLANS = {
    "default": {},
    "x3_planes": dict(gemm_bf16x3=1),        # V of the bf16x3 position GEMMs written as bf16 planes
    "x3_fp32v": dict(gemm_bf16x3=2),         # ... as fp32, split by the GEMM's loaders
    "x3_linear128": dict(x3_linear=128),     # token GEMMs / 1x1 convs on bf16x3 from K = 128
    "wino_fused": dict(conv_algo=3),         # the fused F(2x2,3x3) kernel wherever its shape rule allows
    "wino4_all": dict(conv_algo=4),          # F(4x4,3x3) wherever it fits
    # F(4x4,3x3) layers in two launch sets of 2 images.  On conv_algo = 4: under the default rule a set of 2 of the 4 images no
    # longer fills 256 CUs (wino4_whole_ok), and wino4_max_images alone would drop the layers instead of cutting them
    "wino4_sets2": dict(conv_algo=4, wino4_max_images=2),
    "plain": dict(conv_algo=1, gemm_bf16x3=-1, x3_linear=-1),   # direct convs, fp32 MFMA: tells a sampler bug from a fast-kernel bug
}
_ALL = list(PLANS)
_TWO = ["default", "plain"]

CONFIGS = {
    # T = 24 at batch 4: the conditioning table's chunks of B schedule steps include full ones and a repeated one in a traced run
    "base128": dict(unet=MODEL_A, sampler="ddpm", self_cond=False, batch=4, size=64, T=24, objective="noise",
                    inpaint_resample_times=0, weight_seed=29, noise_seed=101, input_seed=0, perturb_seed=7, plans=_ALL),
    # the ultra-res SR call: start at unet 2, low-res + cond image, inpainting with two resamples (24 forwards, a re-noise between)
    "sr128": dict(unet=MODEL_B, sampler="ddpm", self_cond=False, batch=4, size=64, T=12, objective="v",
                  inpaint_resample_times=2, weight_seed=31, noise_seed=102, input_seed=9, perturb_seed=8, plans=_TWO),
    # EDM Heun: two forwards per step but the last (23 forwards)
    "edm128": dict(unet=MODEL_A, sampler="edm", self_cond=False, batch=4, size=64, T=12, objective="noise",
                   inpaint_resample_times=0, weight_seed=29, noise_seed=103, input_seed=0, perturb_seed=9, plans=_TWO),
    # self-conditioning: the thresholded x0 of step k is an input of step k + 1
    "selfcond128": dict(unet=MODEL_A, sampler="ddpm", self_cond=True, batch=4, size=64, T=16, objective="noise",
                        inpaint_resample_times=0, weight_seed=33, noise_seed=104, input_seed=0, perturb_seed=10, plans=_TWO),
}


class Case:
    """One configuration's oracle: `imagen` (its sampled UNet is `unet`, stage `stage`), `imagen_kw` its constructor kwargs
    (the product's are the same) and `sample_kw` the arguments of sample() besides noise_fn / trace."""

    def __init__(self, name, T=None, fast=False):
        c = self.cfg = CONFIGS[name]
        self.name, self.T = name, int(T or c["T"])
        sr = bool(c["unet"].get("cond_images_channels", 0))     # configuration B: the second stage of a cascade
        plain = dict(cond_on_text=False, text_embed_dim=None)
        if c["self_cond"]:
            u = SR.Unet(**c["unet"], lowres_cond=sr, self_cond=True, **plain)
        else:
            u = R.Unet(**c["unet"], lowres_cond=sr, **plain)
        u = H.randomize_(u, c["weight_seed"]).eval()
        if fast:
            u = H.fast_oracle(u)
        S = c["size"]
        unets, sizes, objectives = ([R.NullUnet(), u], (S // 2, S), ("noise", c["objective"])) if sr else ([u], (S,), (c["objective"],))
        self.imagen_kw = dict(image_sizes=sizes, condition_on_text=False)
        if c["sampler"] == "edm":
            cls = ER.ElucidatedImagen
            self.imagen_kw.update(num_sample_steps=self.T)
        else:
            cls = SR.Imagen if c["self_cond"] else RS.Imagen
            self.imagen_kw.update(timesteps=self.T, pred_objectives=objectives)
        self.imagen = cls(unets, **self.imagen_kw)
        self.stage = len(unets)
        self.unet = self.imagen.unets[-1]
        B = c["batch"]
        self.sample_kw = dict(batch_size=B)
        self.mask = None
        if sr:
            g = torch.Generator().manual_seed(c["input_seed"])
            mask = torch.zeros(B, S, S)
            mask[:, :S // 4, :] = 1      # the overlap strips of an ultra-res patch: top and left quarter known
            mask[:, :, :S // 4] = 1
            self.mask = mask.bool()
            self.sample_kw.update(start_at_unet_number=2, start_image_or_video=torch.rand(B, 3, S // 2, S // 2, generator=g),
                                  cond_images=torch.rand(B, 3, S, S, generator=g),
                                  inpaint_images=torch.rand(B, 3, S, S, generator=g), inpaint_masks=mask,
                                  inpaint_resample_times=c["inpaint_resample_times"])

    def noise_fn(self):
        return RS.generator_noise_fn(self.cfg["noise_seed"])

    def run(self, perturb=None):
        """(trace, final image); perturb = (mode, eps) runs the UNet under `perturbed`."""
        trace = []
        ctx = perturbed(self.unet, perturb[0], perturb[1], self.cfg["perturb_seed"]) if perturb else contextlib.nullcontext()
        with ctx:
            final = self.imagen.sample(noise_fn=self.noise_fn(), trace=trace, **self.sample_kw)
        assert len(trace) == self.T
        return trace, final


@contextlib.contextmanager
def perturbed(unet, mode, eps, seed):
    """`unet.forward_with_cond_scale` (the one entry every sampler of the oracle calls) with an error of norm eps * ||y||
    added to each output y: 'rand' a fresh random direction per call, 'fixed' one random direction for the whole run,
    'scale' the output times (1 + eps)."""
    assert mode in MODES
    g = torch.Generator().manual_seed(seed)
    inner = unet.forward_with_cond_scale
    state = {}

    def fwd(*a, **k):
        y = inner(*a, **k)
        if mode == "scale":
            return y * (1.0 + eps)
        if mode == "rand" or "d" not in state:
            d = torch.randn(y.shape, generator=g, dtype=torch.float64)
            state["d"] = d / d.norm()
        return (y.double() + eps * y.double().norm() * state["d"]).to(y.dtype)

    unet.forward_with_cond_scale = fwd    # an instance attribute over the class's method
    try:
        yield unet
    finally:
        del unet.forward_with_cond_scale


def deviation(trace, ref_trace, final=None, ref_final=None):
    """Per step k: rel-L2 and max-abs of trace[k] against ref_trace[k]; and the final images' max-abs (None without them)."""
    assert len(trace) == len(ref_trace)
    rel = [H.rel_l2(a, b) for a, b in zip(trace, ref_trace)]
    mx = [float((a.double().cpu() - b.double().cpu()).abs().max()) for a, b in zip(trace, ref_trace)]
    fin = None if final is None else float((final.double().cpu() - ref_final.double().cpu()).abs().max())
    return dict(rel=rel, maxabs=mx, final=fin)


def envelope(name, eps, T=None, base=None):
    """The element-wise maximum over the three modes of the deviation from the unperturbed oracle run `base` (made here
    when None): dict(rel=[T], final=float, modes={mode: deviation})."""
    case = Case(name, T=T)
    base = base or case.run()
    modes = {}
    for m in MODES:
        tr, fin = case.run(perturb=(m, eps))
        modes[m] = deviation(tr, base[0], fin, base[1])
    return dict(rel=[max(modes[m]["rel"][k] for m in MODES) for k in range(case.T)],
                final=max(modes[m]["final"] for m in MODES), modes=modes)


def floor(name, T=None, base=None):
    """The oracle's own fp32 resolution: the default layout against helpers.fast_oracle's channels_last layout (the same
    arithmetic in another summation order)."""
    base = base or Case(name, T=T).run()
    tr, fin = Case(name, T=T, fast=True).run()
    return deviation(tr, base[0], fin, base[1])


def json_cfg(name):
    """CONFIGS[name] as JSON holds it (tuples as lists)."""
    import json

    return json.loads(json.dumps(CONFIGS[name]))
