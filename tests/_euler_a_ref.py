"""Test restatement of diffusers' EulerAncestralDiscreteScheduler [3P] ("Euler a", epsilon prediction), written from its
published algorithm independently of `diffsensei_amd.schedulers`, with the per-step noise of the device generator
restated in tests/_philox_ref.py (one int64 seed per panel, counter (pixel, 0, step, 0)).

The schedule is numpy: float64 where diffusers uses float64 numpy, np.float32 scalar arithmetic in diffusers' order
where it uses 0-dim fp32 tensors (sigma_up, sigma_down, sqrt(sigma^2 + 1)).  The update is torch at diffusers' rounding
points for an fp16 pipeline: sample upcast to fp32, the noise drawn in the model output's dtype (fp16), `noise *
sigma_up` an fp16 tensor, the sum fp32.  It follows the protocol of oracle/scheduler_ref.py (`set_timesteps(n)`,
`.timesteps`, `.init_noise_sigma`, `scale_model_input(x, i)`, `step(eps, i, x)`) and uses the step index for the noise,
so `oracle.pipeline_ref.sample_loop` drives it unchanged.
"""
from __future__ import annotations

import numpy as np
import torch

from tests._philox_ref import philox_normal


def _alphas_cumprod(T=1000, beta_start=0.00085, beta_end=0.012) -> np.ndarray:
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).numpy()


class EulerAncestralOracle:
    def __init__(self, seeds=None, timestep_spacing="leading", steps_offset=1, num_train_timesteps=1000,
                 beta_start=0.00085, beta_end=0.012, exact=False):
        """exact: no fp16 rounding of the noise or of `noise * sigma_up`, and a float64 sample stays float64 - the update
        the rounded one approximates (the free-running float64 loops of tests/_loop_cases.py)."""
        self.exact = bool(exact)
        self.seeds = None if seeds is None else [int(s) for s in seeds]
        self.spacing, self.offset, self.T = timestep_spacing, steps_offset, num_train_timesteps
        self.ac = _alphas_cumprod(num_train_timesteps, beta_start, beta_end)

    # ---- schedule
    def set_timesteps(self, n: int):
        T = self.T
        if self.spacing == "linspace":
            ts = np.linspace(0.0, T - 1.0, n)[::-1]
        elif self.spacing == "leading":
            ts = np.round(np.arange(n) * (T // n))[::-1] + self.offset
        elif self.spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / n)) - 1
        else:
            raise ValueError(self.spacing)
        ts = np.ascontiguousarray(ts, dtype=np.float32)
        train_sig = np.sqrt((1 - self.ac) / self.ac)            # fp32, like diffusers' array of fp32 alphas_cumprod
        sig = np.interp(ts, np.arange(T), train_sig)
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps = ts
        self.n = n
        smax = self.sigmas.max()
        self.init_noise_sigma = float(smax) if self.spacing in ("linspace", "trailing") \
            else float(np.sqrt(smax * smax + np.float32(1)))
        return self

    def up_down(self, i: int):
        """(sigma_up, sigma_down) in fp32 scalar arithmetic, diffusers' order of operations."""
        f, t = np.float32(self.sigmas[i]), np.float32(self.sigmas[i + 1])
        up = np.sqrt(t * t * (f * f - t * t) / (f * f))
        down = np.sqrt(t * t - up * up)
        assert up.dtype == np.float32 and down.dtype == np.float32
        return up, down

    def up_down_exact(self, i: int):
        """The same two scalars in float64 from the fp32 sigmas (what the fp32 values approximate)."""
        f, t = float(self.sigmas[i]), float(self.sigmas[i + 1])
        up = np.sqrt(t * t * (f * f - t * t) / (f * f))
        return up, np.sqrt(t * t - up * up)

    def c_in_div(self, i: int) -> np.float32:
        s = np.float32(self.sigmas[i])
        return np.sqrt(s * s + np.float32(1))

    # ---- protocol of oracle/scheduler_ref.py
    def scale_model_input(self, x: torch.Tensor, i: int) -> torch.Tensor:
        return x / float(self.c_in_div(i))

    def noise(self, i: int, shape) -> torch.Tensor:
        """fp16 noise of step i for panels [ns,4,H,W]: the float64 restatement rounded to the model output's dtype."""
        ns, c, h, w = shape
        assert c == 4 and self.seeds is not None and len(self.seeds) == ns, (shape, self.seeds)
        z = torch.from_numpy(philox_normal(self.seeds, i, 0, h * w).reshape(ns, 4, h, w))
        return z if self.exact else z.to(torch.float16)

    def step(self, eps: torch.Tensor, i: int, x: torch.Tensor) -> torch.Tensor:
        s = torch.tensor(self.sigmas[i], dtype=torch.float32)
        up, down = self.up_down(i)
        up64 = lambda t: t if t.dtype == torch.float64 else t.float()
        x32 = up64(x)
        pred_x0 = x32 - s * up64(eps)
        derivative = (x32 - pred_x0) / s
        out = x32 + derivative * (torch.tensor(down) - s)
        return out + (self.noise(i, x.shape) * torch.tensor(up)).to(out.dtype)   # fp16 tensor * 0-dim fp32 -> fp16
