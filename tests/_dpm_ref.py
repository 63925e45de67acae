"""Test restatement of diffusers' DPMSolverMultistepScheduler [3P] (DPM-Solver++, multistep, order 1|2, epsilon
prediction, deterministic), written from its published algorithm independently of `diffsensei_amd.schedulers`.

Tables in float64 numpy (from the fp32 torch `alphas_cumprod` diffusers builds); the update in torch at diffusers'
rounding points for an fp16 pipeline: `convert_model_output` sees the fp16 sample, every scalar * fp16-tensor product is
fp16, the update itself runs on the sample upcast to fp32 and is cast back to fp16.  It follows the protocol of
oracle/scheduler_ref.py (`set_timesteps(n)`, `.timesteps`, `.init_noise_sigma`, `scale_model_input(x, i)`,
`step(eps, i, x)`), so `oracle.pipeline_ref.sample_loop` can drive it.
"""
from __future__ import annotations

import numpy as np
import torch

_h = lambda t: t.half().float()


def _alphas_cumprod(T=1000, beta_start=0.00085, beta_end=0.012) -> np.ndarray:
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).numpy().astype(np.float64)


class DPMSolverOracle:
    def __init__(self, solver_order=2, solver_type="midpoint", use_karras_sigmas=False, timestep_spacing="leading",
                 steps_offset=1, final_sigmas_type="zero", lower_order_final=True, euler_at_final=False,
                 num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, q=_h, q_out=None):
        """q: the rounding at diffusers' fp16 points (default: an fp16 round trip).  The identity gives the update the
        rounded one approximates, in the sample's own dtype (the free-running float64 loops of tests/_loop_cases.py).
        q_out: the rounding of the stored sample alone (default: q)."""
        self.q, self.q_out = q, (q if q_out is None else q_out)
        self.solver_order, self.solver_type = solver_order, solver_type
        self.karras, self.spacing, self.offset = use_karras_sigmas, timestep_spacing, steps_offset
        self.final, self.lower_order_final, self.euler_at_final = final_sigmas_type, lower_order_final, euler_at_final
        self.T = num_train_timesteps
        self.ac = _alphas_cumprod(num_train_timesteps, beta_start, beta_end)
        self.init_noise_sigma = 1.0

    # ---- schedule
    def set_timesteps(self, n: int):
        T = self.T
        if self.spacing == "linspace":
            ts = np.round(np.linspace(0, T - 1, n + 1))[::-1][:-1].astype(np.int64)
        elif self.spacing == "leading":
            ratio = T // (n + 1)
            ts = np.round(np.arange(n + 1) * ratio)[::-1][:-1].astype(np.int64) + self.offset
        elif self.spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1
        else:
            raise ValueError(self.spacing)
        train_sig = np.sqrt((1 - self.ac) / self.ac)
        if self.karras:
            lo, hi, rho = train_sig[0], train_sig[-1], 7.0
            ramp = np.linspace(0, 1, n)
            sig = (hi ** (1 / rho) + ramp * (lo ** (1 / rho) - hi ** (1 / rho))) ** rho
            ts = np.round(np.array([self._t_of_sigma(s, np.log(train_sig)) for s in sig])).astype(np.int64)
        else:
            sig = np.interp(ts, np.arange(T), train_sig)
        last = train_sig[0] if self.final == "sigma_min" else 0.0
        self.sigmas = np.concatenate([sig, [last]])
        self.timesteps = ts
        self.n = len(ts)
        # which steps run first order: diffusers' `step` with its lower_order_nums counter
        self.orders, lon = [], 0
        for i in range(self.n):
            final = i == self.n - 1 and (self.euler_at_final or (self.lower_order_final and self.n < 15)
                                         or self.final == "zero")
            self.orders.append(1 if (self.solver_order == 1 or lon < 1 or final) else 2)
            lon = min(lon + 1, self.solver_order)
        self.prev_x0 = None
        return self

    @staticmethod
    def _t_of_sigma(s: float, log_sigmas: np.ndarray) -> float:
        """Piecewise-linear inverse of log sigma(t) over the training timesteps (diffusers `_sigma_to_t`)."""
        ls = np.log(max(s, 1e-10))
        k = int(np.clip(np.sum(log_sigmas <= ls) - 1, 0, len(log_sigmas) - 2))
        w = np.clip((log_sigmas[k] - ls) / (log_sigmas[k] - log_sigmas[k + 1]), 0.0, 1.0)
        return (1 - w) * k + w * (k + 1)

    # ---- per-step scalars (float64)
    @staticmethod
    def alpha_sigma(s: float):
        a = 1.0 / np.sqrt(s * s + 1.0)
        return a, s * a

    def coefficients(self, i: int, order: int):
        """(sigma_s, alpha_s, a, b, 1/r0, c) of step i; c is the weight diffusers ADDS for heun and SUBTRACTS for
        midpoint."""
        a_t, s_t = self.alpha_sigma(self.sigmas[i + 1])
        a_s, s_s = self.alpha_sigma(self.sigmas[i])
        with np.errstate(divide="ignore"):
            lam_t = np.log(a_t) - np.log(s_t)            # +inf on a final sigma of 0
        h = lam_t - (np.log(a_s) - np.log(s_s))
        b = a_t * (np.exp(-h) - 1.0)
        inv_r0 = c = 0.0
        if order == 2:
            a_1, s_1 = self.alpha_sigma(self.sigmas[i - 1])
            inv_r0 = h / ((np.log(a_s) - np.log(s_s)) - (np.log(a_1) - np.log(s_1)))
            c = 0.5 * b if self.solver_type == "midpoint" else a_t * ((np.exp(-h) - 1.0) / h + 1.0)
        return s_s, a_s, s_t / s_s, b, inv_r0, c

    # ---- protocol of oracle/scheduler_ref.py
    def scale_model_input(self, x: torch.Tensor, i: int) -> torch.Tensor:
        return x

    def step(self, eps: torch.Tensor, i: int, x: torch.Tensor) -> torch.Tensor:
        order = self.orders[i]
        s_s, a_s, a, b, inv_r0, c = self.coefficients(i, order)
        q = self.q
        up = lambda t: t if t.dtype == torch.float64 else t.float()
        x16, e = q(up(x)), q(up(eps))
        x0 = q(q(x16 - q(s_s * e)) / a_s)
        out = a * x16 - q(b * x0)
        if order == 2:
            d1 = q(q(x0 - self.prev_x0) * inv_r0)
            out = out - q(c * d1) if self.solver_type == "midpoint" else out + q(c * d1)
        self.prev_x0 = x0
        return self.q_out(out)
