"""A denoiser with a closed-form answer, and the sampling loops run FREE over it (a plain module, not a conftest).

Data model: every latent pixel is Gaussian, x0 ~ N(mu, s^2).  In the variance-exploding form x = x0 + sigma * n the ideal
noise prediction, as a function of the scaled model input x_in = x / sqrt(1 + sigma^2), is

    eps(x_in, sigma) = sigma * (x_in * sqrt(1 + sigma^2) - mu) / (s^2 + sigma^2)

and the probability-flow ODE dx/dsigma = eps has the solution

    x(sigma) = mu + (x(sigma_0) - mu) * sqrt((s^2 + sigma^2) / (s^2 + sigma_0^2))

(divide by sqrt(1 + sigma^2) for the variance-preserving latents of DDIM and DPM-Solver++).  All four samplers hand the model
the same scaled quantity, so one denoiser serves them all.  Under classifier-free guidance the rows [uncond | cond] use mu_u
and mu_c; u + g (c - u) is linear in mu, so the guided loop solves the same ODE with mu_u + g (mu_c - mu_u) and the same s.

sigma of step i is read from each restatement's OWN table (`model_sigmas`), never recomputed from a rounded timestep.

Three drivers over one case (`Case`: ns panels of 8 x 12 latents, mu = 0.5 N(0, 1), s = 0.8, guidance 5.0):
  * `run_loop(..)`                 the restatement (oracle/scheduler_ref.py, tests/_dpm_ref.py, tests/_euler_a_ref.py) in float64;
  * `run_loop(.., emulate=True)`   the same with `half().double()` wherever the kernels store fp16: the latents, the model input,
                                   eps, the three roundings of the CFG combine (oracle/pipeline_ref.sample_loop) and, for
                                   DPM-Solver++ and Euler Ancestral, the restatements' own fp16 points; `q_lat` replaces the
                                   rounding of the stored latents alone (the truncation probe);
  * `closed_form(..)`              the exact end state.
`run_table_loop` interprets the rows of `diffsensei_amd.schedulers` (`coef_table`, `solver_table`) in float64 the way
include/diffsensei_hip.h documents them - the project's own host tables against the same closed form.
`d_emul(kind, cfg, n)` = rel-L2(emulation, float64 loop): the yardstick every free-running GPU gate is a multiple of.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle.scheduler_ref import DDIMOracle, EulerDiscreteOracle
from tests._dpm_ref import DPMSolverOracle
from tests._euler_a_ref import EulerAncestralOracle
from tests._philox_ref import philox_normal

KINDS = {0: "euler", 1: "ddim", 2: "dpm", 3: "euler_a"}
VP = (1, 2)                      # kinds whose latents are variance preserving (model input = latents)
NS, H, W = 2, 8, 12
S = 0.8
GUIDANCE = 5.0
STEPS = 50
NOISE_SEEDS = (20260101, 2 ** 40 + 3, 7919, 11)      # Euler Ancestral: the Philox seed of panel k derives from entry k % 4
SDXL = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, timestep_spacing="leading")

ident = lambda t: t
h16 = lambda t: t.half().double()


def trunc16(t: torch.Tensor) -> torch.Tensor:
    """fp16 conversion that truncates toward zero (the faulty conversion the 2 * D_emul gate has to catch)."""
    t = t.double()
    h = t.half()
    over = h.double().abs() > t.abs()                 # round-to-nearest went away from zero: one step back
    bits = h.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(torch.float16).double()


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def eps_ideal(x_in: torch.Tensor, sigma, mu: torch.Tensor) -> torch.Tensor:
    """The ideal noise prediction (float64, any device and layout as long as x_in and mu agree).  sigma: one number, or a
    float64 tensor that broadcasts against x_in (one sigma per batch row: panels at different steps)."""
    if torch.is_tensor(sigma):
        sigma = sigma.to(x_in.device, torch.float64)
        return sigma * (x_in.double() * torch.sqrt(1.0 + sigma * sigma) - mu) / (S * S + sigma * sigma)
    sigma = float(sigma)
    return sigma * (x_in.double() * math.sqrt(1.0 + sigma * sigma) - mu) / (S * S + sigma * sigma)


class Case:
    """ns panels: the two means and the unit noise the start state is drawn with (float64, NCHW)."""

    def __init__(self, ns: int = NS, seed: int = 1234):
        g = torch.Generator().manual_seed(seed)
        self.ns, self.seed = ns, seed
        self.mu_u = 0.5 * torch.randn(ns, 4, H, W, generator=g, dtype=torch.float64)
        self.mu_c = 0.5 * torch.randn(ns, 4, H, W, generator=g, dtype=torch.float64)
        self.z = torch.randn(ns, 4, H, W, generator=g, dtype=torch.float64)
        self.noise_seeds = [NOISE_SEEDS[k % len(NOISE_SEEDS)] + 977 * seed + k for k in range(ns)]

    def mu(self, do_cfg: bool) -> torch.Tensor:
        return self.mu_u + GUIDANCE * (self.mu_c - self.mu_u) if do_cfg else self.mu_c

    def start(self, kind: int, sigma0: float, do_cfg: bool) -> torch.Tensor:
        """A draw from the marginal at sigma0, in the sampler's own latent scaling, rounded to fp16 once: every loop
        (float64, emulation, device) and the closed form start from these very values."""
        x = self.mu(do_cfg) + math.sqrt(S * S + sigma0 * sigma0) * self.z
        if kind in VP:
            x = x / math.sqrt(1.0 + sigma0 * sigma0)
        return h16(x)


@functools.lru_cache(maxsize=None)
def case(ns: int = NS, seed: int = 1234) -> Case:
    return Case(ns, seed)


def make_oracle(kind: int, n: int, exact: bool, seeds=None, q_out=None):
    """The restatement of `kind` with its n-step schedule set.  exact: no fp16 point of its own."""
    if kind == 0:
        orc = EulerDiscreteOracle()
    elif kind == 1:
        orc = DDIMOracle()
    elif kind == 2:
        orc = DPMSolverOracle(q=ident if exact else h16, q_out=q_out)
    else:
        orc = EulerAncestralOracle(seeds=seeds, exact=exact)
    return orc.set_timesteps(n)


def model_sigmas(kind: int, orc) -> np.ndarray:
    """float64 [n + 1]: the variance-exploding sigma of the state entering every step and of the end state, from the
    restatement's own table (DDIM: its own alphas_cumprod at its own timesteps; it ends at alphas_cumprod[0], not at 0)."""
    if kind == 1:
        ac = orc.alphas_cumprod.double().numpy()
        a = np.concatenate([ac[np.asarray(orc.timesteps, dtype=np.int64)], [float(orc.final_alpha_cumprod)]])
        return np.sqrt((1.0 - a) / a)
    return np.asarray(orc.sigmas, dtype=np.float64)


def run_loop(kind: int, n: int = STEPS, do_cfg: bool = True, c: Case = None, emulate: bool = False, q_lat=None,
             t_start: int = 0, x_start: torch.Tensor = None, record=()):
    """The restatement's loop, free-running from step t_start.  Returns (end state, {k: state after k steps for k in
    record}).  q_lat: the rounding of the stored latents (default: that of the mode)."""
    c = c or case()
    q = h16 if emulate else ident
    q_lat = q if q_lat is None else q_lat
    assert t_start == 0 or kind != 2, "DPM-Solver++ from mid-schedule needs a first-order first row"
    orc = make_oracle(kind, n, exact=not emulate, seeds=c.noise_seeds, q_out=q_lat)
    sig = model_sigmas(kind, orc)
    x = c.start(kind, sig[t_start], do_cfg) if x_start is None else x_start.double()
    snaps = {}
    for i in range(t_start, n):
        xin = q(orc.scale_model_input(x, i))
        if do_cfg:
            u, cc = q(eps_ideal(xin, sig[i], c.mu_u)), q(eps_ideal(xin, sig[i], c.mu_c))
            e = q(u + q(GUIDANCE * q(cc - u)))
        else:
            e = q(eps_ideal(xin, sig[i], c.mu_c))
        x = orc.step(e, i, x)
        if kind != 2:                       # DPM-Solver++ rounds its result itself (q_out)
            x = q_lat(x)
        if i + 1 - t_start in record:
            snaps[i + 1 - t_start] = x.clone()
    return x, snaps


def closed_form(kind: int, n: int = STEPS, do_cfg: bool = True, c: Case = None, t_start: int = 0,
                x_start: torch.Tensor = None) -> torch.Tensor:
    """The exact end state of the probability-flow ODE from the loop's start state, in the sampler's latent scaling."""
    assert kind != 3, "Euler Ancestral is stochastic: no closed form is claimed"
    c = c or case()
    sig = model_sigmas(kind, make_oracle(kind, n, exact=True))
    s0, s1 = float(sig[t_start]), float(sig[n])
    x = c.start(kind, s0, do_cfg) if x_start is None else x_start.double()
    if kind in VP:
        x = x * math.sqrt(1.0 + s0 * s0)
    mu = c.mu(do_cfg)
    x = mu + (x - mu) * math.sqrt((S * S + s1 * s1) / (S * S + s0 * s0))
    return x / math.sqrt(1.0 + s1 * s1) if kind in VP else x


def host_scheduler(kind: int, n: int):
    from diffsensei_amd import schedulers as Sch
    cls = [Sch.EulerDiscreteScheduler, Sch.DDIMScheduler, Sch.DPMSolverMultistepScheduler,
           Sch.EulerAncestralDiscreteScheduler][kind]
    sch = cls(**SDXL)
    sch.set_timesteps(n)
    return sch


def run_table_loop(kind: int, n: int = STEPS, do_cfg: bool = True, c: Case = None) -> torch.Tensor:
    """The project's host tables (`coef_table`, `solver_table`) through a float64 interpreter of their rows as
    include/diffsensei_hip.h documents them: row {t, c_in_div, k0..k3, c_in_div_next, guidance}, solver row {order, sigma_s,
    alpha_s, a, b, 1/r0, c, 0}.  The first model input divides by column 1 of row 0, every later one by column 6 of the row
    before it; the guidance scale is column 7.  The denoiser's sigma is the restatement's, as in `run_loop`."""
    c = c or case()
    sch = host_scheduler(kind, n)
    tab = sch.coef_table(GUIDANCE).astype(np.float64)
    sol = sch.solver_table().astype(np.float64) if kind == 2 else None
    assert tab.shape == (n, 8)
    sig = model_sigmas(kind, make_oracle(kind, n, exact=True, seeds=c.noise_seeds))
    x = c.start(kind, sig[0], do_cfg)
    xin = x / tab[0, 1]
    prev = None
    for i in range(n):
        r = tab[i]
        if do_cfg:
            u, cc = eps_ideal(xin, sig[i], c.mu_u), eps_ideal(xin, sig[i], c.mu_c)
            e = u + r[7] * (cc - u)
        else:
            e = eps_ideal(xin, sig[i], c.mu_c)
        if kind == 0:
            x = x + ((x - (x - r[2] * e)) / r[2]) * (r[3] - r[2])
        elif kind == 1:
            x = r[4] * ((x - r[3] * e) / r[2]) + r[5] * e
        elif kind == 3:
            z = torch.from_numpy(philox_normal(c.noise_seeds, i, 0, H * W).reshape(c.ns, 4, H, W))
            x = x + ((x - (x - r[2] * e)) / r[2]) * (r[3] - r[2]) + r[4] * z
        else:
            sv = sol[i]
            x0 = (x - sv[1] * e) / sv[2]
            xn = sv[3] * x - sv[4] * x0
            if sv[0] == 2.0:
                xn = xn - sv[6] * ((x0 - prev) * sv[5])
            prev, x = x0, xn
        xin = x / r[6]
    return x


@functools.lru_cache(maxsize=None)
def f64_loop(kind: int, do_cfg: bool, n: int = STEPS, ns: int = NS, seed: int = 1234) -> torch.Tensor:
    return run_loop(kind, n, do_cfg, case(ns, seed))[0]


@functools.lru_cache(maxsize=None)
def d_emul(kind: int, do_cfg: bool, n: int = STEPS, ns: int = NS, seed: int = 1234) -> float:
    """rel-L2(fp16-storage emulation, float64 loop) after n free-running steps: computed, never typed in."""
    return rel(run_loop(kind, n, do_cfg, case(ns, seed), emulate=True)[0], f64_loop(kind, do_cfg, n, ns, seed))


@functools.lru_cache(maxsize=None)
def d_closed(kind: int, do_cfg: bool, n: int = STEPS, ns: int = NS, seed: int = 1234) -> float:
    """rel-L2(float64 loop, closed form): the restatement's own discretisation error at n steps."""
    return rel(f64_loop(kind, do_cfg, n, ns, seed), closed_form(kind, n, do_cfg, case(ns, seed)))
