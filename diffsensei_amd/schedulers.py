"""Scheduler objects with the diffusers protocol the reference pipeline drives
(`set_timesteps(n, device)`, `.timesteps`, `.init_noise_sigma`, `scale_model_input(x, t)`,
`step(eps, t, x, return_dict=False)[0]`; reference src/pipelines/pipeline_diffsensei.py:248-249, :317, :337).

Host side = the schedule tables only (a few hundred scalars computed once per `set_timesteps`, in numpy exactly
where diffusers uses numpy).  All per-element arithmetic (CFG combine, the update, the next step's input scaling)
runs in ONE HIP kernel (`sampler_step_kernel`, switched by `kind`) reading a per-step scalar table the engine indexes
with a device-side step counter — the reference issues 5+ elementwise launches per step here.

`_Scheduler` is the whole host protocol: config handling (`.config`, `from_config(config, **overrides)`, so the usual
swap `pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, use_karras_sigmas=True)` works),
the training sigmas and their interpolation, the timestep -> row lookup and the stand-alone `scale_model_input` /
`step`.  A sampler is a subclass with its `kind`, its config keys as class data, `set_timesteps` and `coef_table`
(DPM-Solver++ adds `solver_table`); tests/golden/scheduler_tables.npz pins every table and every refusal
(tools/dump_scheduler_tables.py).

`EulerAncestralDiscreteScheduler` and `LCMScheduler` are the stochastic samplers: their per-step noise is drawn inside the
step kernel from one int64 seed per panel, `draw_noise_seeds`.  `LCMScheduler` is the few-step consistency sampler; its
tables are pinned by tests/golden/lcm_tables.npz (tools/dump_lcm_tables.py), not by the matrix above.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import ops

KIND_EULER, KIND_DDIM, KIND_DPM, KIND_EULER_ANCESTRAL, KIND_LCM = 0, 1, 2, 3, 4
SOLVER_KINDS = (KIND_DPM, KIND_LCM)                 # read a second per-step table, the solver rows
NOISE_KINDS = (KIND_EULER_ANCESTRAL, KIND_LCM)      # draw Philox noise inside the step kernel: one seed per panel


class _Config(dict):
    """diffusers' FrozenDict stand-in: item and attribute access."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key) from None


def _timestep_grid(spacing: str, T: int, n: int, steps_offset: int) -> np.ndarray:
    """diffusers' n-point fp32 grid of EulerDiscrete / EulerAncestral / DDIM [3P] (DDIM casts it to int64)."""
    if spacing == "linspace":
        return np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
    if spacing == "leading":
        return (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + steps_offset
    return np.arange(T, 0, -T / n).round().copy().astype(np.float32) - 1   # trailing


class _Scheduler:
    kind = -1
    order = 1
    stochastic = False   # True: the pipeline draws one Philox seed per panel (`draw_noise_seeds`) for `load_schedule`
    # scheduler_config.json handling, as class data.  `_DEFAULTS`: the constructor arguments of the diffusers class [3P]
    # that are kept in `.config`, with their defaults; every other key is another class's and is ignored.  `_SUPPORTED`:
    # the keys that CHANGE the schedule or the update rule, with the values the device kernel implements - anything else
    # would sample on a different schedule than the reference's scheduler without a word, so it is refused.  A
    # `_SUPPORTED` key outside `_DEFAULTS` is refused by the constructor and dropped by `from_config`.
    _DEFAULTS: dict = {}
    _SUPPORTED: dict = {}

    def __init__(self, **kwargs):
        cfg = _Config(self._DEFAULTS)
        cfg.update({k: v for k, v in kwargs.items() if k in cfg})
        for key, ok in self._SUPPORTED.items():
            value = cfg[key] if key in cfg else kwargs.get(key, ok[0])
            if isinstance(value, (list, tuple)) or value not in ok:
                raise NotImplementedError(f"scheduler config {key}={value!r}: the MI355X sampler kernel implements "
                                          f"{type(self).__name__} with {key} in {ok} only")
        self.config = cfg
        self.T = int(cfg.num_train_timesteps)
        self.steps_offset = cfg.steps_offset
        betas = torch.linspace(cfg.beta_start ** 0.5, cfg.beta_end ** 0.5, self.T, dtype=torch.float32) ** 2  # scaled_linear
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.timesteps = None
        self.num_inference_steps = None
        self._step_index = 0

    @classmethod
    def from_config(cls, config=None, **overrides):
        """diffusers `SchedulerMixin.from_config`: keys the class does not take are ignored (another class's config)."""
        merged = dict(config or {})
        merged.update(overrides)
        return cls(**{k: v for k, v in merged.items() if k in cls._DEFAULTS})

    # -- pieces of `set_timesteps`
    def _train_sigmas(self) -> np.ndarray:
        ac = self.alphas_cumprod.numpy()
        return ((1 - ac) / ac) ** 0.5

    def _interp_sigmas(self, ts: np.ndarray) -> np.ndarray:
        sig = self._train_sigmas()
        return np.interp(ts, np.arange(0, len(sig)), sig)

    def _set_grid(self, ts: np.ndarray, device):
        self.timesteps_np = ts
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self.num_inference_steps = len(ts)
        self._step_index = 0

    # -- table for the engine: rows [n_steps, 8] = {t, c_in_div, k0..k3, c_in_div_next, guidance}
    def coef_table(self, guidance_scale: float) -> np.ndarray:
        raise NotImplementedError

    def _coef_frame(self, guidance_scale: float, sigmas: Optional[np.ndarray] = None) -> np.ndarray:
        """The table with k1..k3 left 0.  `sigmas` (fp32, n + 1): k0 = sigma and the model input is x / sqrt(sigma^2 + 1)
        (fp32 like the 0-dim sigma tensor arithmetic in diffusers); without them the model input is x."""
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        n = self.num_inference_steps
        tab = np.zeros((n, 8), dtype=np.float32)
        div = np.ones(n + 1, dtype=np.float32) if sigmas is None else ((sigmas ** 2 + 1) ** 0.5).astype(np.float32)
        tab[:, 0] = self.timesteps_np
        tab[:, 1] = div[:n]
        if sigmas is not None:
            tab[:, 2] = sigmas[:n]
        tab[:, 6] = div[1:n + 1]
        tab[:, 7] = guidance_scale
        return tab

    # -- second per-step table (DPM-Solver++ only; see include/diffsensei_hip.h)
    def solver_table(self, start: int = 0) -> Optional[np.ndarray]:
        return None

    # -- region redraw (include/diffsensei_hip.h, "Region redraw"): where a shortened run starts, and what a kept latent
    #    looks like at the noise level of every state
    def start_index(self, strength: float) -> int:
        """diffusers' img2img `get_timesteps` [3P]: a run of `strength` in (0, 1] skips the first `t_start` of the n
        steps, init = min(int(n * strength), n), t_start = max(n - init, 0).  ValueError outside (0, 1] or when no step
        would run."""
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        if not _is_real(strength) or not 0.0 < float(strength) <= 1.0:
            raise ValueError(f"`strength` has to be in (0, 1], got {strength!r}")
        n = self.num_inference_steps
        t_start = max(n - min(int(n * float(strength)), n), 0)
        if t_start >= n:
            raise ValueError(f"strength {strength} of {n} steps runs no step at all (int({n} * {strength}) = 0)")
        return t_start

    def renoise_table(self) -> np.ndarray:
        """fp32 [n + 1, 2]: row i = {ka, kb} with ka * x0 + kb * noise the kept latents x0 at the noise level of the
        state that enters step i; row n, the final state, is {1, 0} for every sampler."""
        raise NotImplementedError

    def _renoise_rows(self, ka, kb) -> np.ndarray:
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        n = self.num_inference_steps
        rows = np.zeros((n + 1, 2), dtype=np.float32)
        rows[:n, 0], rows[:n, 1] = np.asarray(ka, dtype=np.float32)[:n], np.asarray(kb, dtype=np.float32)[:n]
        rows[n] = (1.0, 0.0)
        return rows

    # -- panel schedules (continuous batching): everything ONE panel needs, without touching this object's state
    def panel_schedule(self, num_inference_steps: int, strength: float = 1.0, guidance_scale: float = 1.0) -> dict:
        """The schedule of one panel that runs `num_inference_steps` steps at `strength` (1.0: all of them; < 1: a region
        redraw that starts at `start_index(strength)`): {"t_start", "steps" (rows it runs), "rows" = coef_table[t_start:],
        "solver_rows" = solver_table(start=t_start) (None unless DPM-Solver++), "renoise_rows" = renoise_table[t_start:]
        (steps + 1 rows), "init_noise_sigma", "timesteps" (numpy, the run's own)}.  Computed on a copy: requests with
        other step counts are in flight, so this scheduler's `set_timesteps` state stays what it was."""
        import copy
        s = copy.copy(self)             # `set_timesteps` only rebinds attributes, so a shallow copy shares nothing it writes
        s.set_timesteps(int(num_inference_steps))
        t0 = s.start_index(strength)
        solver = s.solver_table(start=t0) if t0 else s.solver_table()
        return {"t_start": t0, "steps": s.num_inference_steps - t0, "rows": s.coef_table(guidance_scale)[t0:],
                "solver_rows": solver, "renoise_rows": s.renoise_table()[t0:],
                "init_noise_sigma": float(s.init_noise_sigma), "timesteps": np.array(s.timesteps_np[t0:])}

    # -- stand-alone protocol (one kernel launch each; the pipeline's fused loop does not go through these)
    def _index_of(self, timestep, default: int) -> int:
        """diffusers `index_for_timestep`: the row of `timestep` - the second one when a timestep repeats (a Karras grid
        rounded to integers can) - or `default` when there is none."""
        idx = np.nonzero(np.isclose(np.asarray(self.timesteps_np, dtype=np.float64), float(timestep)))[0]
        if len(idx) == 0:
            return default
        return int(idx[1] if len(idx) > 1 else idx[0])

    def _step_row(self, timestep) -> int:
        return self._index_of(timestep, self._step_index)

    def scale_model_input(self, sample: torch.Tensor, timestep) -> torch.Tensor:
        div = float(self.coef_table(1.0)[self._step_row(timestep), 1])
        if div == 1.0:
            return sample
        ns, c, h, w = sample.shape
        table = torch.tensor([[0, div, 0, 0, 0, 0, 1, 1]], dtype=torch.float32, device=sample.device)
        tmp = torch.empty((ns, h * w, c), dtype=torch.float16, device=sample.device)
        ops.prepare_model_input(sample.contiguous(), tmp, table, do_cfg=False)
        return ops.nhwc_to_nchw(tmp).reshape(ns, c, h, w)

    def _step_extras(self, i: int, lat: torch.Tensor, generator) -> dict:
        """What row i of this sampler reads besides the table: `solver` + `prev_x0` (DPM-Solver++), `seeds`
        (Euler Ancestral) or `solver` + `seeds` (LCM), on `lat`'s device.  Both tables are indexed with the step counter, here i."""
        return {}

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, *, generator=None,
             return_dict: bool = True, **kw):
        """model_output: the (already CFG-combined) noise prediction, NCHW like `sample`.  Computes in fp16 like the
        pipeline's fused loop.  `generator`: where a stochastic sampler draws its per-panel seeds from."""
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        i = self._step_row(timestep)
        ns, c, h, w = sample.shape
        dev = sample.device
        eps = ops.nchw_to_nhwc(model_output.to(torch.float16).reshape(ns, c, h * w).contiguous())
        lat = sample.to(torch.float16).contiguous().clone()
        scratch = torch.empty((ns, h * w, c), dtype=torch.float16, device=dev)
        table = torch.from_numpy(self.coef_table(1.0)).to(dev)
        ctr = torch.tensor([i], dtype=torch.int32, device=dev)
        _launch_step(eps, lat, scratch, table, self.kind, ctr, **self._step_extras(i, lat, generator))
        self._step_index = i + 1
        return (lat,) if not return_dict else {"prev_sample": lat}


def _is_real(v) -> bool:
    import numbers
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _launch_step(eps, lat, scratch, table, kind, ctr, solver=None, prev_x0=None, seeds=None):
    """One `sampler_step_kernel` launch through the C entry point that carries the given extras."""
    if solver is not None and seeds is not None:
        ops.cfg_lcm_step(eps, lat, scratch, table, solver, seeds, do_cfg=False, ctr=ctr)
    elif solver is not None:
        ops.cfg_dpm_step(eps, lat, scratch, table, solver, prev_x0, do_cfg=False, ctr=ctr)
    elif seeds is not None:
        ops.cfg_sampler_step_noise(eps, lat, scratch, table, seeds, kind, do_cfg=False, ctr=ctr)
    else:
        ops.cfg_sampler_step(eps, lat, scratch, table, kind, do_cfg=False, ctr=ctr)


# Euler / DDIM: the SDXL configuration as defaults, and nothing but it accepted
_SDXL = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
             timestep_spacing="leading", prediction_type="epsilon")
_SDXL_ONLY = {"beta_schedule": ("scaled_linear",), "timestep_spacing": ("leading",), "prediction_type": ("epsilon",),
              "trained_betas": (None,), "rescale_betas_zero_snr": (False,), "use_karras_sigmas": (False,),
              "use_exponential_sigmas": (False,), "use_beta_sigmas": (False,), "interpolation_type": ("linear",),
              "final_sigmas_type": ("zero",), "timestep_type": ("discrete",), "sigma_min": (None,), "sigma_max": (None,),
              "clip_sample": (False,), "set_alpha_to_one": (False,), "thresholding": (False,)}


class EulerDiscreteScheduler(_Scheduler):
    """diffusers EulerDiscreteScheduler [3P] (deterministic: s_churn = 0, final sigma 0, linear interpolation)."""
    kind = KIND_EULER
    _DEFAULTS = dict(_SDXL, trained_betas=None, use_karras_sigmas=False, use_exponential_sigmas=False,
                     use_beta_sigmas=False, interpolation_type="linear", sigma_min=None, sigma_max=None,
                     timestep_type="discrete", rescale_betas_zero_snr=False, final_sigmas_type="zero")
    _SUPPORTED = _SDXL_ONLY

    def set_timesteps(self, num_inference_steps: int, device=None):
        ts = _timestep_grid("leading", self.T, num_inference_steps, self.steps_offset)
        self.sigmas = np.concatenate([self._interp_sigmas(ts), [0.0]]).astype(np.float32)
        self.init_noise_sigma = float((self.sigmas.max() ** 2 + 1) ** 0.5)
        self._set_grid(ts, device)

    def coef_table(self, guidance_scale: float) -> np.ndarray:
        tab = self._coef_frame(guidance_scale, self.sigmas)
        tab[:, 3] = self.sigmas[1:]
        return tab

    def renoise_table(self) -> np.ndarray:
        return self._renoise_rows(np.ones_like(self.sigmas), self.sigmas)      # x0 + sigma_i * noise


class DDIMScheduler(_Scheduler):
    """diffusers DDIMScheduler [3P], eta = 0, clip_sample False, set_alpha_to_one False."""
    kind = KIND_DDIM
    init_noise_sigma = 1.0
    _DEFAULTS = dict(_SDXL, trained_betas=None, clip_sample=False, set_alpha_to_one=False, thresholding=False,
                     rescale_betas_zero_snr=False)
    _SUPPORTED = _SDXL_ONLY

    def set_timesteps(self, num_inference_steps: int, device=None):
        ts = _timestep_grid("leading", self.T, num_inference_steps, self.steps_offset)
        self._set_grid(ts.astype(np.int64), device)

    def coef_table(self, guidance_scale: float) -> np.ndarray:
        n = self.num_inference_steps
        tab = np.zeros((n, 8), dtype=np.float32)
        ac = self.alphas_cumprod.numpy().astype(np.float32)
        for i, t in enumerate(self.timesteps_np):
            prev = int(t) - self.T // n
            a_t = ac[int(t)]
            a_p = ac[prev] if prev >= 0 else ac[0]
            tab[i] = [float(t), 1.0, a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5, 1.0, guidance_scale]
        return tab

    def renoise_table(self) -> np.ndarray:
        a = self.alphas_cumprod.numpy().astype(np.float32)[np.asarray(self.timesteps_np, dtype=np.int64)]
        return self._renoise_rows(a ** 0.5, (1 - a) ** 0.5)                    # diffusers `add_noise` [3P]


# DPM-Solver++ / Euler Ancestral: diffusers' own constructor defaults (linear betas: NOT the SDXL schedule, so a bare config
# is refused; the usual way in is `from_config` of the pipeline's scheduler), and any of the three spacings
_DIFFUSERS = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                  prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0, rescale_betas_zero_snr=False)
_DIFFUSERS_SUPPORTED = {"beta_schedule": ("scaled_linear",), "trained_betas": (None,), "prediction_type": ("epsilon",),
                        "timestep_spacing": ("leading", "linspace", "trailing"), "rescale_betas_zero_snr": (False,)}


class DPMSolverMultistepScheduler(_Scheduler):
    """diffusers DPMSolverMultistepScheduler [3P]: DPM-Solver++ (algorithm_type "dpmsolver++"), multistep, solver_order
    1 or 2, solver_type "midpoint" or "heun", epsilon prediction, deterministic.

    Per step the engine reads the shared table row {t, 1, 0, 0, 0, 0, 1, guidance} (init_noise_sigma = 1 and
    scale_model_input is the identity) plus one solver row {order, sigma_s, alpha_s, a, b, 1/r0, c, 0}
    (include/diffsensei_hip.h).  Which rows run first order (diffusers' `lower_order_nums` / `lower_order_final` rules)
    is decided here, per row, so a captured step graph needs no host logic.  Scalars are 0-dim fp32 torch values
    computed in diffusers' order; the last row of a zero final sigma gives a = 0, b = -1 (lambda_t = +inf, no NaN)."""
    kind = KIND_DPM
    init_noise_sigma = 1.0
    _DEFAULTS = dict(_DIFFUSERS, solver_order=2, thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                     algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, euler_at_final=False,
                     use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False, use_lu_lambdas=False,
                     use_flow_sigmas=False, flow_shift=1.0, final_sigmas_type="zero", lambda_min_clipped=-float("inf"),
                     variance_type=None)
    _SUPPORTED = dict(_DIFFUSERS_SUPPORTED, solver_order=(1, 2), thresholding=(False,), algorithm_type=("dpmsolver++",),
                      solver_type=("midpoint", "heun"), use_exponential_sigmas=(False,), use_beta_sigmas=(False,),
                      use_lu_lambdas=(False,), use_flow_sigmas=(False,), final_sigmas_type=("zero", "sigma_min"),
                      variance_type=(None,))

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        # the one key judged by value, not by membership: whatever `float` reads as -inf (JSON's -Infinity included)
        lmc = float(self.config["lambda_min_clipped"])
        if not (math.isinf(lmc) and lmc < 0):
            raise NotImplementedError(f"scheduler config lambda_min_clipped={lmc!r}: only -inf (no clipping)")
        self.sigmas = None
        self.lower_order_nums = 0
        self._prev_x0 = None

    def _train_sigmas(self) -> np.ndarray:
        ac = self.alphas_cumprod    # torch arithmetic, where diffusers' class has it: an ulp from numpy's at a few t
        return np.array(((1 - ac) / ac) ** 0.5)

    def set_timesteps(self, num_inference_steps: int, device=None):
        """diffusers `set_timesteps` (lambda_min_clipped = -inf, so the last usable timestep is num_train_timesteps).
        This class's grid is its own: n + 1 points with the last dropped, and rounding AFTER the Karras map."""
        cfg, n, T = self.config, int(num_inference_steps), self.T
        if cfg.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif cfg.timestep_spacing == "leading":
            step_ratio = T // (n + 1)
            ts = (np.arange(0, n + 1) * step_ratio).round()[::-1][:-1].copy().astype(np.int64)
            ts += cfg.steps_offset
        else:  # trailing
            ts = np.arange(T, 0, -T / n).round().copy().astype(np.int64)
            ts -= 1
        train = self._train_sigmas()
        if cfg.use_karras_sigmas:
            rho, s_min, s_max = 7.0, train[0].item(), train[-1].item()
            ramp = np.linspace(0, 1, n)
            sigmas = (s_max ** (1 / rho) + ramp * (s_min ** (1 / rho) - s_max ** (1 / rho))) ** rho
            ts = _sigma_to_t(sigmas, np.log(train)).round().astype(np.int64)
        else:
            sigmas = self._interp_sigmas(ts)
        last = float(train[0]) if cfg.final_sigmas_type == "sigma_min" else 0.0
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [last]]).astype(np.float32))
        self._set_grid(ts, device)
        self.lower_order_nums = 0
        self._step_index = None     # diffusers: looked up at the first `step`, then counted

    # -- which rows run first order (diffusers `step`: lower_order_nums < 1, lower_order_final)
    def _order(self, i: int, lower_order_nums: int) -> int:
        cfg, n = self.config, self.num_inference_steps
        final = i == n - 1 and (cfg.euler_at_final or (cfg.lower_order_final and n < 15)
                                or cfg.final_sigmas_type == "zero")
        return 1 if (cfg.solver_order == 1 or lower_order_nums < 1 or final) else 2

    def step_orders(self) -> np.ndarray:
        """Order of every row when the whole schedule runs from step 0 (what the device table encodes)."""
        return np.array([self._order(i, min(i, self.config.solver_order)) for i in range(self.num_inference_steps)])

    def _solver_row(self, i: int, order: int) -> np.ndarray:
        def alpha_sigma(sig):
            alpha = 1 / ((sig ** 2 + 1) ** 0.5)
            return alpha, sig * alpha

        s = self.sigmas
        alpha_t, sigma_t = alpha_sigma(s[i + 1])
        alpha_s0, sigma_s0 = alpha_sigma(s[i])
        lambda_t = torch.log(alpha_t) - torch.log(sigma_t)
        lambda_s0 = torch.log(alpha_s0) - torch.log(sigma_s0)
        h = lambda_t - lambda_s0
        b = alpha_t * (torch.exp(-h) - 1.0)
        row = [float(order), sigma_s0, alpha_s0, sigma_t / sigma_s0, b, 0.0, 0.0, 0.0]
        if order == 2:
            alpha_s1, sigma_s1 = alpha_sigma(s[i - 1])
            lambda_s1 = torch.log(alpha_s1) - torch.log(sigma_s1)
            r0 = (lambda_s0 - lambda_s1) / h
            row[5] = 1.0 / r0
            # the kernel subtracts c*D1: midpoint's "- 0.5*b*D1", heun's "+ alpha_t*((e^-h - 1)/h + 1)*D1"
            row[6] = 0.5 * b if self.config.solver_type == "midpoint" else -(alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0))
        return np.array([float(v) for v in row], dtype=np.float32)

    def solver_table(self, start: int = 0) -> np.ndarray:
        """fp32 [n_steps - start, 8] solver rows {order, sigma_s, alpha_s, a, b, 1/r0, c, 0} (include/diffsensei_hip.h)
        of a run that begins at step `start` (region redraw with strength < 1): its first row is first order - there is
        no previous x0 yet - and the later ones are the rows of the whole schedule."""
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        n = self.num_inference_steps
        if not 0 <= int(start) < n:
            raise ValueError(f"solver_table: start {start} outside the {n} steps")
        if start == 0:
            orders = self.step_orders()
        else:
            orders = [self._order(i, min(i - start, self.config.solver_order)) for i in range(start, n)]
        return np.stack([self._solver_row(start + k, int(o)) for k, o in enumerate(orders)])

    def renoise_table(self) -> np.ndarray:
        alpha = 1 / ((self.sigmas ** 2 + 1) ** 0.5)                              # the arithmetic of `_solver_row`
        return self._renoise_rows(alpha.numpy(), (self.sigmas * alpha).numpy())

    def coef_table(self, guidance_scale: float) -> np.ndarray:
        return self._coef_frame(guidance_scale)

    # -- stand-alone protocol
    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def _step_row(self, timestep) -> int:
        if self._step_index is None:
            self._step_index = self._index_of(timestep, self.num_inference_steps - 1)
        return self._step_index

    def _step_extras(self, i: int, lat: torch.Tensor, generator) -> dict:
        """Row i at the order the run so far allows (a run may start mid-schedule; this step is counted here), and the
        previous x0, which stays on the device between calls."""
        rows = np.zeros((self.num_inference_steps, 8), dtype=np.float32)
        rows[i] = self._solver_row(i, self._order(i, self.lower_order_nums))
        if self._prev_x0 is None or self._prev_x0.shape != lat.shape or self._prev_x0.device != lat.device:
            self._prev_x0 = torch.empty_like(lat)
        self.lower_order_nums = min(self.lower_order_nums + 1, self.config.solver_order)
        return dict(solver=torch.from_numpy(rows).to(lat.device), prev_x0=self._prev_x0)


def draw_noise_seeds(num_samples: int, generator=None) -> list:
    """One non-negative int64 Philox seed per panel for a stochastic sampler: `torch.randint(0, 2**63 - 1, (n,),
    generator=generator)` on the generator's device for one generator, one draw from each of a list of generators (a
    panel's seed then depends on its own generator only), the global torch generator when `generator` is None."""
    hi = 2 ** 63 - 1
    if isinstance(generator, (list, tuple)):
        if len(generator) != num_samples:
            raise ValueError(f"{len(generator)} generators for {num_samples} samples")
        return [int(torch.randint(0, hi, (1,), generator=g, device=g.device).item()) for g in generator]
    if generator is None:
        return [int(v) for v in torch.randint(0, hi, (num_samples,)).tolist()]
    return [int(v) for v in torch.randint(0, hi, (num_samples,), generator=generator, device=generator.device).tolist()]


class EulerAncestralDiscreteScheduler(_Scheduler):
    """diffusers EulerAncestralDiscreteScheduler [3P] ("Euler a"), epsilon prediction: an Euler step from sigma_from down
    to sigma_down, then fresh noise of std sigma_up, with sigma_up^2 + sigma_down^2 = sigma_to^2.

    Per step the engine reads the table row {t, c_in_div, sigma, sigma_down, sigma_up, 0, c_in_div_next, guidance}; the
    noise is drawn inside the step kernel from a Philox counter keyed by one int64 seed per panel and indexed by the
    device step counter (include/diffsensei_hip.h, "device noise"), so a captured step graph needs no host work between
    replays and a panel's noise does not depend on the batch it runs in.  Scalars are 0-dim fp32 torch values computed
    in diffusers' order; the last row (sigma_to = 0) has sigma_up = sigma_down = 0."""
    kind = KIND_EULER_ANCESTRAL
    stochastic = True
    _DEFAULTS = _DIFFUSERS
    _SUPPORTED = _DIFFUSERS_SUPPORTED

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        # like diffusers, the training sigmas until `set_timesteps`: `init_noise_sigma` is read before it
        self.sigmas = torch.from_numpy(np.concatenate([self._train_sigmas()[::-1], [0.0]]).astype(np.float32))
        self._seeds = None

    @property
    def init_noise_sigma(self) -> float:
        smax = self.sigmas.max()
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return float(smax)
        return float((smax ** 2 + 1) ** 0.5)

    def set_timesteps(self, num_inference_steps: int, device=None):
        cfg = self.config
        ts = _timestep_grid(cfg.timestep_spacing, self.T, int(num_inference_steps), cfg.steps_offset)
        self.sigmas = torch.from_numpy(np.concatenate([self._interp_sigmas(ts), [0.0]]).astype(np.float32))
        self._set_grid(ts, device)
        self._seeds = None      # the stand-alone `step` draws new seeds for a new run

    def sigma_up_down(self, i: int):
        """(sigma_up, sigma_down) of row i, 0-dim fp32 tensors in diffusers' order of operations."""
        sigma_from, sigma_to = self.sigmas[i], self.sigmas[i + 1]
        sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
        sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
        return sigma_up, sigma_down

    def coef_table(self, guidance_scale: float) -> np.ndarray:
        tab = self._coef_frame(guidance_scale, self.sigmas.numpy())
        for i in range(len(tab)):
            up, down = self.sigma_up_down(i)
            tab[i, 3], tab[i, 4] = float(down), float(up)
        return tab

    def renoise_table(self) -> np.ndarray:
        sig = self.sigmas.numpy()
        return self._renoise_rows(np.ones_like(sig), sig)                       # x0 + sigma_i * noise

    # -- stand-alone protocol
    def _step_extras(self, i: int, lat: torch.Tensor, generator) -> dict:
        """The per-panel seeds, drawn once per run (`draw_noise_seeds(batch, generator)` at the first step after
        `set_timesteps`, kept in `noise_seeds`); the noise of step i is the device's Philox draw for (seed, pixel, i)."""
        if self._seeds is None or len(self._seeds) != lat.shape[0]:
            self._seeds = draw_noise_seeds(lat.shape[0], generator)
        return dict(seeds=torch.tensor(self._seeds, dtype=torch.int64, device=lat.device))

    @property
    def noise_seeds(self):
        """The seeds of the current stand-alone run (None before its first `step`)."""
        return None if self._seeds is None else list(self._seeds)


class LCMScheduler(_Scheduler):
    """diffusers LCMScheduler [3P], epsilon prediction: the consistency sampler a latent-consistency distillation (an LCM
    adapter merged into the UNet, or a distilled UNet) is run with, in 1 - 8 steps.  Per step: x0 from the prediction, the
    boundary condition denoised = c_out * x0 + c_skip * x, then the denoised value re-noised to the NEXT timestep,
    sqrt(a_prev) * denoised + sqrt(1 - a_prev) * z; the last step returns the denoised value itself.

    The timesteps are a subset of the `original_inference_steps` grid the distillation was trained on (`set_timesteps`),
    not of this project's other grids; `timestep_spacing`, `steps_offset` and `set_alpha_to_one` are kept in the config and
    never reach the arithmetic, as in diffusers.  Per step the engine reads the table row {t, 1, sqrt(a_t), sqrt(1 - a_t),
    c_out, c_skip, 1, guidance} (init_noise_sigma = 1, the model input is unscaled) plus one solver row {sqrt(a_prev),
    sqrt(1 - a_prev), 0, ...}, which is {1, 0} on the last row (include/diffsensei_hip.h).  The noise z is Euler Ancestral's
    source unchanged: Philox stream 0, one int64 seed per panel, indexed by the device step counter.  Scalars are 0-dim
    fp32 torch values computed in diffusers' order.

    Region redraw and strength runs truncate the n-step grid with this project's own `start_index` rule (skip the first
    n - int(n * strength) rows).  That is NOT diffusers' LCM img2img rule, which re-derives the grid from
    original_inference_steps * strength."""
    kind = KIND_LCM
    stochastic = True
    init_noise_sigma = 1.0
    SIGMA_DATA = 0.5
    _DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                     trained_betas=None, original_inference_steps=50, clip_sample=False, clip_sample_range=1.0,
                     set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon", thresholding=False,
                     dynamic_thresholding_ratio=0.995, sample_max_value=1.0, timestep_spacing="leading", timestep_scaling=10.0,
                     rescale_betas_zero_snr=False)
    _SUPPORTED = {"beta_schedule": ("scaled_linear",), "prediction_type": ("epsilon",), "clip_sample": (False,),
                  "thresholding": (False,), "rescale_betas_zero_snr": (False,), "trained_betas": (None,)}

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        orig = self.config.original_inference_steps
        if not _is_real(orig) or int(orig) != orig or not 1 <= int(orig) <= self.T:
            raise ValueError(f"original_inference_steps={orig!r} must be an integer in 1..{self.T}")
        if not _is_real(self.config.timestep_scaling):
            raise ValueError(f"timestep_scaling={self.config.timestep_scaling!r} must be a number")
        self._seeds = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        """diffusers `set_timesteps` (no `timesteps=` / `strength=`): the training grid of the distillation is
        origin = (1 .. original_inference_steps) * k - 1 with k = T // original_inference_steps, descending, and the run
        takes the n entries at floor(linspace(0, len(origin), n, endpoint=False))."""
        n, orig = int(num_inference_steps), int(self.config.original_inference_steps)
        if n < 1:
            raise ValueError(f"num_inference_steps={num_inference_steps!r} must be at least 1")
        if n > self.T:
            raise ValueError(f"num_inference_steps={n} cannot exceed num_train_timesteps={self.T}")
        if n > orig:
            raise ValueError(f"num_inference_steps={n} cannot exceed original_inference_steps={orig}: the distillation "
                             f"knows no finer grid")
        k = self.T // orig
        origin = (np.arange(1, orig + 1) * k - 1)[::-1].copy()
        idx = np.floor(np.linspace(0, len(origin), num=n, endpoint=False)).astype(np.int64)
        self._set_grid(origin[idx].astype(np.int64), device)
        self._seeds = None      # the stand-alone `step` draws new seeds for a new run

    def _alpha_pairs(self):
        """(sqrt(a_t), sqrt(1 - a_t)) of every row, 0-dim fp32 tensors."""
        return [(self.alphas_cumprod[int(t)].sqrt(), (1 - self.alphas_cumprod[int(t)]).sqrt()) for t in self.timesteps_np]

    def boundary_scalings(self, t: int):
        """(c_skip, c_out) of diffusers' `get_scalings_for_boundary_condition_discrete`, 0-dim fp32 tensors."""
        s = torch.tensor(int(t)) * float(self.config.timestep_scaling)
        c_skip = self.SIGMA_DATA ** 2 / (s ** 2 + self.SIGMA_DATA ** 2)
        c_out = s / (s ** 2 + self.SIGMA_DATA ** 2) ** 0.5
        return c_skip, c_out

    def coef_table(self, guidance_scale: float) -> np.ndarray:
        tab = self._coef_frame(guidance_scale)
        for i, (sa, sb) in enumerate(self._alpha_pairs()):
            c_skip, c_out = self.boundary_scalings(self.timesteps_np[i])
            tab[i, 2:6] = [float(sa), float(sb), float(c_out), float(c_skip)]
        return tab

    def solver_table(self, start: int = 0) -> np.ndarray:
        """fp32 [n_steps - start, 8] rows {sqrt(a_prev), sqrt(1 - a_prev), 0 x 6}: the noise level of the NEXT row's
        timestep, which the step re-noises its denoised value to; the last row is {1, 0} - the denoised value, no noise."""
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        n = self.num_inference_steps
        if not 0 <= int(start) < n:
            raise ValueError(f"solver_table: start {start} outside the {n} steps")
        rows = np.zeros((n, 8), dtype=np.float32)
        pairs = self._alpha_pairs()
        for i in range(n - 1):
            rows[i, 0], rows[i, 1] = float(pairs[i + 1][0]), float(pairs[i + 1][1])
        rows[n - 1, 0] = 1.0
        return rows[int(start):]

    def renoise_table(self) -> np.ndarray:
        pairs = self._alpha_pairs()                                             # diffusers `add_noise` [3P]
        return self._renoise_rows([float(a) for a, _ in pairs], [float(b) for _, b in pairs])

    # -- stand-alone protocol
    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def _step_extras(self, i: int, lat: torch.Tensor, generator) -> dict:
        if self._seeds is None or len(self._seeds) != lat.shape[0]:
            self._seeds = draw_noise_seeds(lat.shape[0], generator)
        return dict(solver=torch.from_numpy(self.solver_table()).to(lat.device),
                    seeds=torch.tensor(self._seeds, dtype=torch.int64, device=lat.device))

    @property
    def noise_seeds(self):
        """The seeds of the current stand-alone run (None before its first `step`)."""
        return None if self._seeds is None else list(self._seeds)


# scheduler_config.json `_class_name` -> class
SCHEDULERS = {c.__name__: c for c in (EulerDiscreteScheduler, DDIMScheduler, DPMSolverMultistepScheduler,
                                      EulerAncestralDiscreteScheduler, LCMScheduler)}


def _sigma_to_t(sigmas: np.ndarray, log_sigmas: np.ndarray) -> np.ndarray:
    """diffusers `_sigma_to_t` [3P]: piecewise-linear interpolation of log-sigma back to (fractional) timesteps."""
    log_sigma = np.log(np.maximum(sigmas, 1e-10))
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return (1 - w) * low_idx + w * high_idx
