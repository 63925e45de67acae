"""Test restatement of diffusers' LCMScheduler [3P] (latent consistency sampling, epsilon prediction), written from its
published algorithm in float64 and sharing no code with `diffsensei_amd.schedulers`.  The per-step noise is the device
generator's, restated in tests/_philox_ref.py (one int64 seed per panel, counter (pixel, 0, step, 0)).

    betas      = linspace(sqrt(b0), sqrt(b1), T)^2, abar = cumprod(1 - betas)            (scaled_linear)
    origin     = (1 .. N0) * (T // N0) - 1, descending                                   (N0 = original_inference_steps)
    timesteps  = origin[floor(linspace(0, N0, n, endpoint=False))]
    s          = t * timestep_scaling,  c_skip = 0.25 / (s^2 + 0.25),  c_out = s / sqrt(s^2 + 0.25)
    x0         = (x - sqrt(1 - abar_t) eps) / sqrt(abar_t)
    d          = c_out x0 + c_skip x
    x_next     = sqrt(abar_prev) d + sqrt(1 - abar_prev) z,   t_prev = the next timestep;   x_next = d on the last step

Everything is float64 - the betas included - so the fp32 tables of the code under test are compared with what they
approximate, and the update has no rounding of its own.  It follows the protocol of oracle/scheduler_ref.py
(`set_timesteps(n)`, `.timesteps`, `.init_noise_sigma`, `scale_model_input(x, i)`, `step(eps, i, x)`), so
`oracle.pipeline_ref.sample_loop` drives it unchanged.
"""
from __future__ import annotations

import numpy as np
import torch

from tests._philox_ref import philox_normal


class LCMOracle:
    init_noise_sigma = 1.0

    def __init__(self, seeds=None, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                 original_inference_steps=50, timestep_scaling=10.0):
        self.seeds = None if seeds is None else [int(s) for s in seeds]
        self.T, self.N0, self.scaling = int(num_train_timesteps), int(original_inference_steps), float(timestep_scaling)
        betas = np.linspace(np.sqrt(np.float64(beta_start)), np.sqrt(np.float64(beta_end)), self.T) ** 2
        self.abar = np.cumprod(1.0 - betas)

    def set_timesteps(self, n: int):
        if n > self.N0 or n > self.T:
            raise ValueError(n)
        origin = [j * (self.T // self.N0) - 1 for j in range(self.N0, 0, -1)]
        self.timesteps = np.array([origin[(m * self.N0) // n] for m in range(n)], dtype=np.int64)   # floor(m N0 / n), exactly
        self.n = n
        return self

    # ---- the six scalars of a row
    def scalars(self, i: int):
        """(sqrt(abar_t), sqrt(1 - abar_t), c_out, c_skip, sqrt(abar_prev), sqrt(1 - abar_prev)); the last row's pair is (1, 0)."""
        t = int(self.timesteps[i])
        s = t * self.scaling
        a = self.abar[t]
        last = i == self.n - 1
        ap = 1.0 if last else self.abar[int(self.timesteps[i + 1])]
        return (np.sqrt(a), np.sqrt(1 - a), s / np.sqrt(s * s + 0.25), 0.25 / (s * s + 0.25), np.sqrt(ap), np.sqrt(1 - ap))

    def tables(self, guidance: float):
        """(coef [n,8], solver [n,8], renoise [n+1,2]) in float64, in the layout of include/diffsensei_hip.h."""
        coef, solver, renoise = np.zeros((self.n, 8)), np.zeros((self.n, 8)), np.zeros((self.n + 1, 2))
        for i in range(self.n):
            sa, sb, c_out, c_skip, pa, pb = self.scalars(i)
            coef[i] = [self.timesteps[i], 1.0, sa, sb, c_out, c_skip, 1.0, guidance]
            solver[i, :2] = [pa, pb]
            renoise[i] = [sa, sb]
        renoise[self.n] = [1.0, 0.0]
        return coef, solver, renoise

    # ---- protocol of oracle/scheduler_ref.py
    def scale_model_input(self, x: torch.Tensor, i: int) -> torch.Tensor:
        return x

    def noise(self, i: int, shape) -> torch.Tensor:
        ns, c, h, w = shape
        assert c == 4 and self.seeds is not None and len(self.seeds) == ns, (shape, self.seeds)
        return torch.from_numpy(philox_normal(self.seeds, i, 0, h * w).reshape(ns, 4, h, w)).double()

    def step(self, eps: torch.Tensor, i: int, x: torch.Tensor) -> torch.Tensor:
        """float64 whatever comes in; the result is returned in x's dtype when that is float64, else float32."""
        sa, sb, c_out, c_skip, pa, pb = self.scalars(i)
        x64, e64 = x.double(), eps.double()
        x0 = (x64 - sb * e64) / sa
        d = c_out * x0 + c_skip * x64
        out = d if i == self.n - 1 else pa * d + pb * self.noise(i, x.shape)
        return out if x.dtype == torch.float64 else out.float()
