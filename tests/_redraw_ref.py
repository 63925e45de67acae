"""Test restatements for region redraw (masked, strength-based sampling from kept latents), written from the published
algorithms independently of `diffsensei_amd`: diffusers' img2img `get_timesteps` and 4-channel inpainting blend [3P].

* `renoise_rows(kind, ...)`: what a kept latent looks like at the noise level of every state, float64 numpy.
* `blend(...)`: the per-step blend at the kernel's rounding points, fp32 torch.
* `RedrawOracle`: wraps a scheduler oracle of the oracle/scheduler_ref.py protocol so that
  `oracle.pipeline_ref.sample_loop` runs the shortened, masked schedule.
* `mask_from_boxes`: the centre-in-half-open-box rule, in plain Python.
* `ulp16`: distance of two fp16 tensors in units in the last place.
"""
from __future__ import annotations

import numpy as np
import torch

hq = lambda t: t.half().float()


def alphas_cumprod(T=1000, beta_start=0.00085, beta_end=0.012) -> np.ndarray:
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).numpy().astype(np.float64)


def start_index(n: int, strength: float) -> int:
    init = min(int(n * strength), n)
    return max(n - init, 0)


def renoise_rows(kind: str, timesteps, sigmas=None) -> np.ndarray:
    """float64 [n + 1, 2].  kind "sigma" (Euler, Euler Ancestral): x0 + sigma * noise; "ddim": diffusers add_noise,
    sqrt(a_t) * x0 + sqrt(1 - a_t) * noise; "dpm": alpha * x0 + sigma * alpha * noise with alpha = 1 / sqrt(sigma^2 + 1).
    `sigmas`: the n (or n + 1) sigmas of the schedule; the final state is {1, 0} whatever the last sigma is."""
    n = len(timesteps)
    rows = np.zeros((n + 1, 2), dtype=np.float64)
    rows[n] = (1.0, 0.0)
    for i in range(n):
        if kind == "sigma":
            rows[i] = (1.0, float(sigmas[i]))
        elif kind == "ddim":
            a = alphas_cumprod()[int(timesteps[i])]
            rows[i] = (np.sqrt(a), np.sqrt(1.0 - a))
        elif kind == "dpm":
            s = float(sigmas[i])
            alpha = 1.0 / np.sqrt(s * s + 1.0)
            rows[i] = (alpha, s * alpha)
        else:
            raise ValueError(kind)
    return rows


def known(x0: torch.Tensor, noise: torch.Tensor, ka: float, kb: float) -> torch.Tensor:
    """half(ka * x0 + kb * noise), fp32 arithmetic without contraction (the kernel may contract: <= 1 fp16 ulp apart)."""
    ka, kb = torch.tensor(ka, dtype=torch.float32), torch.tensor(kb, dtype=torch.float32)
    return hq(ka * x0.float() + kb * noise.float())


def blend(xn_half: torch.Tensor, x0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor, ka: float, kb: float):
    """half(m * half(xn) + (1 - m) * half(known)); mask [ns,H,W] broadcast over the 4 channels."""
    m = mask.float()[:, None]
    return hq(m * xn_half.float() + (1.0 - m) * known(x0, noise, ka, kb))


def mask_from_boxes(boxes, h: int, w: int) -> torch.Tensor:
    m = torch.zeros(h, w)
    for y in range(h):
        for x in range(w):
            cx, cy = (x + 0.5) / w, (y + 0.5) / h
            if any(b[0] <= cx < b[2] and b[1] <= cy < b[3] for b in boxes):
                m[y, x] = 1.0
    return m


def ulp16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """|a - b| in fp16 units in the last place (finite inputs): the bit patterns mapped to a monotonic integer line."""
    def line(t):
        v = t.detach().cpu().contiguous().to(torch.float16).view(torch.int16).to(torch.int32)
        return torch.where(v < 0, -(v & 0x7FFF), v)
    return (line(a) - line(b)).abs()


class RedrawOracle:
    """`inner` (oracle/scheduler_ref.py protocol) run from step `t_start` of `n_total`, every step followed by the
    blend.  rows: [n_total + 1, 2] of the whole schedule.  `first_order_at_start`: DPMSolverOracle - a run that starts
    mid-schedule has no previous x0, so its first step is first order."""

    def __init__(self, inner, n_total: int, t_start: int, x0, noise, mask, rows, first_order_at_start=False):
        self.inner, self.n_total, self.t = inner, n_total, t_start
        self.x0, self.noise, self.mask, self.rows = x0.float(), noise.float(), mask.float(), rows
        self.first_order = first_order_at_start

    def set_timesteps(self, n_run: int):
        assert n_run == self.n_total - self.t
        self.inner.set_timesteps(self.n_total)
        if self.first_order:
            self.inner.orders[self.t] = 1
        self.timesteps = self.inner.timesteps[self.t:]
        self.init_noise_sigma = self.inner.init_noise_sigma
        return self

    def start_latents(self) -> torch.Tensor:
        ka, kb = self.rows[self.t]
        return known(self.x0, self.noise, float(ka), float(kb))

    def scale_model_input(self, x, i):
        return self.inner.scale_model_input(x, i + self.t)

    def step(self, eps, i, x):
        xn = hq(self.inner.step(eps, i + self.t, x))
        ka, kb = self.rows[self.t + i + 1]
        return blend(xn, self.x0, self.noise, self.mask, float(ka), float(kb))
