"""TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED** (see oracle/imagen_ref.py): the restatement of fused-tile canvas sampling
(tests/tiled_ref.py, tests/tiled_known_ref.py) with the canvas step of DPM-Solver++(3M) and of the SDE forms of 2M and 3M, in
the divided-difference form of tests/solver3_ref.py with the FUSED estimate in the place of the estimate.  Everything but
the canvas step - lattice, cut, fuse, known pixels, the image start, the walk over the stages - is those files'.

``CanvasSolver3`` is ``tiled_ref.CanvasSolver`` for the names that one knows.  For the new names its history - the fused
estimates of the last two steps walked, newest first - lives in ``x0_prev``, the attribute the resample loop of
tiled_known_ref.run_canvas saves and puts back around every slot but a step's last: the history follows the schedule, not
the resample loop.  The order of a step is ``min(cap, estimates kept + 1, T - k)``: first order on the first step walked.
``sampler_eta`` None is 1 for the ``_sde`` names.  Noise: tag ("step", stage, k, r) of the canvas' shape, asked for in
every step of an ``_sde`` name but the last.
"""
from __future__ import annotations

import math

import torch

import tiled_known_ref as KR
import tiled_ref as TR
from oracle import sampler_ref as RS
from solver3_ref import CAPS


class CanvasSolver3(TR.CanvasSolver):
    def __init__(self, noise_scheduler, name, eta=0.0):
        if name not in CAPS:
            super().__init__(noise_scheduler, name, eta)
            return
        self.sched, self.name, self.eta = noise_scheduler, name, float(eta)
        assert (self.eta > 0) == name.endswith("_sde")
        self.steps = noise_scheduler.get_sampling_timesteps(1)
        f64 = lambda t: float(t.double().flatten()[0])
        self.lam = [(f64(noise_scheduler.log_snr(t)) / 2, f64(noise_scheduler.log_snr(tn)) / 2) for t, tn in self.steps]
        self.x0_prev = self.h_prev = None   # x0_prev: (x0bar of step k - 1[, of step k - 2])

    def wants_noise(self, k):
        if self.name not in CAPS:
            return super().wants_noise(k)
        return self.eta > 0 and k < len(self.steps) - 1

    def step(self, k, x, x0bar, noise=None):
        if self.name not in CAPS:
            return super().step(k, x, x0bar, noise)
        T, eta = len(self.steps), self.eta
        times, times_next = self.steps[k]
        f64 = lambda t: float(t.double().flatten()[0])
        a, s = (f64(v) for v in RS.log_snr_to_alpha_sigma(self.sched.log_snr(times)))
        a_next, s_next = (f64(v) for v in RS.log_snr_to_alpha_sigma(self.sched.log_snr(times_next)))
        hs = [b - a_ for a_, b in self.lam]
        h = hs[k]
        he = h * (1 + eta)
        A = (s_next / s) * math.exp(-eta * h)
        b = -a_next * math.expm1(-he)
        phi2 = math.expm1(-he) / he + 1
        phi3 = phi2 / he - 0.5
        kept = self.x0_prev or ()
        order = min(CAPS[self.name], len(kept) + 1, T - k)
        out = A * x + b * x0bar
        if order == 2:
            out = out + a_next * phi2 * ((x0bar - kept[0]) / (hs[k - 1] / h))
        elif order == 3:
            r0, r1 = hs[k - 1] / h, hs[k - 2] / h
            D1_0, D1_1 = (x0bar - kept[0]) / r0, (kept[0] - kept[1]) / r1
            out = out + a_next * phi2 * (D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)) - a_next * phi3 * ((D1_0 - D1_1) / (r0 + r1))
        if self.wants_noise(k):
            out = out + s_next * math.sqrt(-math.expm1(-2 * eta * h)) * noise
        self.x0_prev = ((x0bar,) + tuple(kept))[:2]
        return out


def sample_tiled(oim, *, sampler=None, sampler_eta=None, **kw):
    """tiled_known_ref.sample_tiled with CanvasSolver3 as the canvas step."""
    n = len(oim.unets)
    per = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * n
    etas = tuple((1.0 if str(nm).endswith("_sde") else 0.0) if e is None else float(e) for nm, e in zip(per(sampler), per(sampler_eta)))
    kept = KR.CanvasSolver
    KR.CanvasSolver = CanvasSolver3   # (run_canvas looks the class up in its module when it is called)
    try:
        return KR.sample_tiled(oim, sampler=sampler, sampler_eta=etas, **kw)
    finally:
        KR.CanvasSolver = kept
