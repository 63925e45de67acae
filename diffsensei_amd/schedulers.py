"""Scheduler objects with the diffusers protocol the reference pipeline drives
(`set_timesteps(n, device)`, `.timesteps`, `.init_noise_sigma`, `scale_model_input(x, t)`,
`step(eps, t, x, return_dict=False)[0]`; reference src/pipelines/pipeline_diffsensei.py:248-249, :317, :337).

Host side = the schedule tables only (a few hundred scalars computed once per `set_timesteps`, in numpy exactly
where diffusers uses numpy).  All per-element arithmetic (CFG combine, the update, the next step's input scaling)
runs in ONE HIP kernel (`ds_cfg_sampler_step_f16`, `ds_cfg_dpm_step_f16`) reading a per-step scalar table the engine
indexes with a device-side step counter — the reference issues 5+ elementwise launches per step here.

Every class has diffusers' `.config` and `from_config(config, **overrides)`, so the usual scheduler swap
`pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, use_karras_sigmas=True)` works.

`EulerAncestralDiscreteScheduler` is the one stochastic sampler: its per-step noise is drawn inside the step kernel
(`ds_cfg_sampler_step_noise_f16`) from one int64 seed per panel, `draw_noise_seeds`.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import ops

KIND_EULER, KIND_DDIM, KIND_DPM, KIND_EULER_ANCESTRAL = 0, 1, 2, 3


class _Config(dict):
    """diffusers' FrozenDict stand-in: item and attribute access."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key) from None


class _ConfigMixin:
    @classmethod
    def _config_keys(cls):
        raise NotImplementedError

    @classmethod
    def from_config(cls, config=None, **overrides):
        """diffusers `SchedulerMixin.from_config`: keys the class does not take are ignored (another class's config)."""
        merged = dict(config or {})
        merged.update(overrides)
        keys = cls._config_keys()
        return cls(**{k: v for k, v in merged.items() if k in keys})


def _alphas_cumprod(T: int, beta_start: float, beta_end: float) -> torch.Tensor:
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2  # scaled_linear
    return torch.cumprod(1.0 - betas, dim=0)


class _SchedulerBase(_ConfigMixin):
    kind = -1
    order = 1
    _CONFIG_FIXED = ()  # the `_FIXED` keys that are constructor arguments of the diffusers class (kept in `.config`)
    _FIXED = {"trained_betas": (None,), "rescale_betas_zero_snr": (False,), "use_karras_sigmas": (False,),
              "use_exponential_sigmas": (False,), "use_beta_sigmas": (False,), "interpolation_type": ("linear",),
              "final_sigmas_type": ("zero",), "timestep_type": ("discrete",), "sigma_min": (None,), "sigma_max": (None,),
              "clip_sample": (False,), "set_alpha_to_one": (False,), "thresholding": (False,)}

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 steps_offset=1, timestep_spacing="leading", prediction_type="epsilon", **unused):
        if beta_schedule != "scaled_linear" or timestep_spacing != "leading" or prediction_type != "epsilon":
            raise NotImplementedError("only the SDXL scheduler configuration (scaled_linear / leading / epsilon)")
        # scheduler_config.json keys of diffusers' Euler / DDIM classes [3P] that CHANGE the sigma schedule or the update
        # rule: only the value the device kernel implements is accepted - anything else would sample on a different
        # schedule than the reference's scheduler without a word.  Keys that do not touch the arithmetic are ignored.
        for key, ok in self._FIXED.items():
            if key in unused and unused[key] not in ok:
                raise NotImplementedError(f"scheduler config {key}={unused[key]!r}: the MI355X sampler kernel implements "
                                          f"{key} in {ok} only")
        self.config = _Config(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                              beta_schedule=beta_schedule, steps_offset=steps_offset, timestep_spacing=timestep_spacing,
                              prediction_type=prediction_type,
                              **{k: unused.get(k, self._FIXED[k][0]) for k in self._CONFIG_FIXED})
        self.T = num_train_timesteps
        self.steps_offset = steps_offset
        self.alphas_cumprod = _alphas_cumprod(num_train_timesteps, beta_start, beta_end)
        self.timesteps = None
        self.num_inference_steps = None
        self._step_index = 0
        self._dev_table = None

    @classmethod
    def _config_keys(cls):
        return ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "steps_offset", "timestep_spacing",
                "prediction_type") + cls._CONFIG_FIXED

    # -- table for the engine: rows [n_steps, 8] = {t, c_in_div, k0..k3, c_in_div_next, guidance}
    def coef_table(self, guidance_scale: float) -> np.ndarray:
        raise NotImplementedError

    # -- second per-step table (DPM-Solver++ only; see include/diffsensei_hip.h)
    def solver_table(self) -> Optional[np.ndarray]:
        return None

    def _table_on(self, device, guidance: float) -> torch.Tensor:
        return torch.from_numpy(self.coef_table(guidance)).to(device)

    def _index_of(self, t) -> int:
        tv = float(t)
        idx = np.nonzero(np.isclose(np.asarray(self.timesteps_np, dtype=np.float64), tv))[0]
        return int(idx[0]) if len(idx) else self._step_index

    # -- stand-alone protocol (one kernel launch each; the pipeline's fused loop does not go through these)
    def scale_model_input(self, sample: torch.Tensor, timestep) -> torch.Tensor:
        i = self._index_of(timestep)
        div = float(self.coef_table(1.0)[i, 1])
        if div == 1.0:
            return sample
        ns, c, h, w = sample.shape
        table = torch.tensor([[0, div, 0, 0, 0, 0, 1, 1]], dtype=torch.float32, device=sample.device)
        tmp = torch.empty((ns, h * w, c), dtype=torch.float16, device=sample.device)
        ops.prepare_model_input(sample.contiguous(), tmp, table, do_cfg=False)
        return ops.nhwc_to_nchw(tmp).reshape(ns, c, h, w)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True, **kw):
        """model_output: the (already CFG-combined) noise prediction, NCHW like `sample`."""
        i = self._index_of(timestep)
        row = self.coef_table(1.0)[i:i + 1].copy()
        table = torch.from_numpy(row).to(sample.device)
        ns, c, h, w = sample.shape
        eps = ops.nchw_to_nhwc(model_output.to(torch.float16).reshape(ns, c, h * w).contiguous())
        lat = sample.to(torch.float16).contiguous().clone()
        scratch = torch.empty((ns, h * w, c), dtype=torch.float16, device=sample.device)
        ops.cfg_sampler_step(eps, lat, scratch, table, self.kind, do_cfg=False)
        self._step_index = i + 1
        return (lat,) if not return_dict else {"prev_sample": lat}


class EulerDiscreteScheduler(_SchedulerBase):
    """diffusers EulerDiscreteScheduler [3P] (deterministic: s_churn = 0, final sigma 0, linear interpolation)."""
    kind = KIND_EULER
    _CONFIG_FIXED = ("trained_betas", "use_karras_sigmas", "use_exponential_sigmas", "use_beta_sigmas",
                     "interpolation_type", "sigma_min", "sigma_max", "timestep_type", "rescale_betas_zero_snr",
                     "final_sigmas_type")

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = num_inference_steps
        step_ratio = self.T // n
        ts = (np.arange(0, n) * step_ratio).round()[::-1].copy().astype(np.float32) + self.steps_offset
        ac = self.alphas_cumprod.numpy()
        sig = np.array(((1 - ac) / ac) ** 0.5)
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps_np = ts
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self.num_inference_steps = n
        self.init_noise_sigma = float((self.sigmas.max() ** 2 + 1) ** 0.5)
        self._step_index = 0

    def coef_table(self, guidance_scale: float) -> np.ndarray:
        n = self.num_inference_steps
        tab = np.zeros((n, 8), dtype=np.float32)
        s = self.sigmas.astype(np.float32)
        div = ((s ** 2 + 1) ** 0.5).astype(np.float32)   # fp32 like the 0-dim sigma tensor arithmetic in diffusers
        tab[:, 0] = self.timesteps_np
        tab[:, 1] = div[:n]
        tab[:, 2] = s[:n]
        tab[:, 3] = s[1:n + 1]
        tab[:, 6] = div[1:n + 1]
        tab[:, 7] = guidance_scale
        return tab


class DDIMScheduler(_SchedulerBase):
    """diffusers DDIMScheduler [3P], eta = 0, clip_sample False, set_alpha_to_one False."""
    kind = KIND_DDIM
    _CONFIG_FIXED = ("trained_betas", "clip_sample", "set_alpha_to_one", "thresholding", "rescale_betas_zero_snr")
    init_noise_sigma = 1.0

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = num_inference_steps
        step_ratio = self.T // n
        ts = (np.arange(0, n) * step_ratio).round()[::-1].copy().astype(np.int64) + self.steps_offset
        self.timesteps_np = ts
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self.num_inference_steps = n
        self._step_index = 0

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


class DPMSolverMultistepScheduler(_ConfigMixin):
    """diffusers DPMSolverMultistepScheduler [3P]: DPM-Solver++ (algorithm_type "dpmsolver++"), multistep, solver_order
    1 or 2, solver_type "midpoint" or "heun", epsilon prediction, deterministic.

    Per step the engine reads the shared table row {t, 1, 0, 0, 0, 0, 1, guidance} (init_noise_sigma = 1 and
    scale_model_input is the identity) plus one solver row {order, sigma_s, alpha_s, a, b, 1/r0, c, 0}
    (include/diffsensei_hip.h).  Which rows run first order (diffusers' `lower_order_nums` / `lower_order_final` rules)
    is decided here, per row, so a captured step graph needs no host logic.  Scalars are 0-dim fp32 torch values
    computed in diffusers' order; the last row of a zero final sigma gives a = 0, b = -1 (lambda_t = +inf, no NaN)."""
    kind = KIND_DPM
    order = 1
    init_noise_sigma = 1.0
    # diffusers' constructor defaults for this class (linear betas: NOT the SDXL schedule, so a bare config is refused)
    _DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                     dynamic_thresholding_ratio=0.995, sample_max_value=1.0, algorithm_type="dpmsolver++",
                     solver_type="midpoint", lower_order_final=True, euler_at_final=False, use_karras_sigmas=False,
                     use_exponential_sigmas=False, use_beta_sigmas=False, use_lu_lambdas=False, use_flow_sigmas=False,
                     flow_shift=1.0, final_sigmas_type="zero", lambda_min_clipped=-float("inf"), variance_type=None,
                     timestep_spacing="linspace", steps_offset=0, rescale_betas_zero_snr=False)
    # keys whose other values change the schedule or the update rule: only what the device kernel implements is accepted
    _SUPPORTED = {"beta_schedule": ("scaled_linear",), "trained_betas": (None,), "solver_order": (1, 2),
                  "prediction_type": ("epsilon",), "thresholding": (False,), "algorithm_type": ("dpmsolver++",),
                  "solver_type": ("midpoint", "heun"), "use_exponential_sigmas": (False,), "use_beta_sigmas": (False,),
                  "use_lu_lambdas": (False,), "use_flow_sigmas": (False,), "final_sigmas_type": ("zero", "sigma_min"),
                  "variance_type": (None,), "timestep_spacing": ("leading", "linspace", "trailing"),
                  "rescale_betas_zero_snr": (False,)}

    def __init__(self, **kwargs):
        cfg = _Config(self._DEFAULTS)
        cfg.update({k: v for k, v in kwargs.items() if k in self._DEFAULTS})   # other keys: not this class's (ignored)
        for key, ok in self._SUPPORTED.items():
            if isinstance(cfg[key], (list, tuple)) or cfg[key] not in ok:
                raise NotImplementedError(f"scheduler config {key}={cfg[key]!r}: the MI355X DPM-Solver++ kernel "
                                          f"implements {key} in {ok} only")
        lmc = float(cfg["lambda_min_clipped"])
        if not (math.isinf(lmc) and lmc < 0):
            raise NotImplementedError(f"scheduler config lambda_min_clipped={lmc!r}: only -inf (no clipping)")
        self.config = cfg
        self.T = int(cfg["num_train_timesteps"])
        self.alphas_cumprod = _alphas_cumprod(self.T, cfg["beta_start"], cfg["beta_end"])
        self.timesteps = None
        self.sigmas = None
        self.num_inference_steps = None
        self.lower_order_nums = 0
        self._step_index = None
        self._prev_x0 = None

    @classmethod
    def _config_keys(cls):
        return tuple(cls._DEFAULTS)

    def set_timesteps(self, num_inference_steps: int, device=None):
        """diffusers `set_timesteps` (lambda_min_clipped = -inf, so the last usable timestep is num_train_timesteps)."""
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
        ac = self.alphas_cumprod
        sigmas = np.array(((1 - ac) / ac) ** 0.5)
        log_sigmas = np.log(sigmas)
        if cfg.use_karras_sigmas:
            sigmas = np.flip(sigmas).copy()
            rho, s_min, s_max = 7.0, sigmas[-1].item(), sigmas[0].item()
            ramp = np.linspace(0, 1, n)
            sigmas = (s_max ** (1 / rho) + ramp * (s_min ** (1 / rho) - s_max ** (1 / rho))) ** rho
            ts = _sigma_to_t(sigmas, log_sigmas).round()
        else:
            sigmas = np.interp(ts, np.arange(0, len(sigmas)), sigmas)
        last = float(((1 - ac[0]) / ac[0]) ** 0.5) if cfg.final_sigmas_type == "sigma_min" else 0.0
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [last]]).astype(np.float32))
        self.timesteps_np = np.asarray(ts).astype(np.int64)
        self.timesteps = torch.from_numpy(self.timesteps_np.copy())
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self.num_inference_steps = len(self.timesteps_np)
        self.lower_order_nums = 0
        self._step_index = None

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

    def solver_table(self) -> np.ndarray:
        """fp32 [n_steps, 8] solver rows {order, sigma_s, alpha_s, a, b, 1/r0, c, 0} (include/diffsensei_hip.h)."""
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        orders = self.step_orders()
        return np.stack([self._solver_row(i, int(o)) for i, o in enumerate(orders)])

    def coef_table(self, guidance_scale: float) -> np.ndarray:
        n = self.num_inference_steps
        tab = np.zeros((n, 8), dtype=np.float32)
        tab[:, 0] = self.timesteps_np
        tab[:, 1] = 1.0
        tab[:, 6] = 1.0
        tab[:, 7] = guidance_scale
        return tab

    # -- stand-alone protocol (one kernel launch per step; the pipeline's fused loop does not go through these)
    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def _index_for_timestep(self, timestep) -> int:
        """diffusers `index_for_timestep`: the second match when a timestep repeats, the last row when none matches."""
        idx = np.nonzero(self.timesteps_np == int(round(float(timestep))))[0]
        if len(idx) == 0:
            return self.num_inference_steps - 1
        return int(idx[1] if len(idx) > 1 else idx[0])

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True, **kw):
        """model_output: the (already CFG-combined) noise prediction, NCHW like `sample`; keeps the previous x0 on the
        device between calls.  Computes in fp16 like the pipeline's fused loop."""
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        if self._step_index is None:
            self._step_index = self._index_for_timestep(timestep)
        i = self._step_index
        order = self._order(i, self.lower_order_nums)
        dev = sample.device
        solver = torch.from_numpy(self._solver_row(i, order)[None]).to(dev)
        table = torch.tensor([[0, 1, 0, 0, 0, 0, 1, 1]], dtype=torch.float32, device=dev)
        ns, c, h, w = sample.shape
        eps = ops.nchw_to_nhwc(model_output.to(torch.float16).reshape(ns, c, h * w).contiguous())
        lat = sample.to(torch.float16).contiguous().clone()
        if self._prev_x0 is None or self._prev_x0.shape != lat.shape or self._prev_x0.device != lat.device:
            self._prev_x0 = torch.empty_like(lat)
        scratch = torch.empty((ns, h * w, c), dtype=torch.float16, device=dev)
        ops.cfg_dpm_step(eps, lat, scratch, table, solver, self._prev_x0, do_cfg=False)
        self.lower_order_nums = min(self.lower_order_nums + 1, self.config.solver_order)
        self._step_index = i + 1
        return (lat,) if not return_dict else {"prev_sample": lat}


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


class EulerAncestralDiscreteScheduler(_ConfigMixin):
    """diffusers EulerAncestralDiscreteScheduler [3P] ("Euler a"), epsilon prediction: an Euler step from sigma_from down
    to sigma_down, then fresh noise of std sigma_up, with sigma_up^2 + sigma_down^2 = sigma_to^2.

    Per step the engine reads the table row {t, c_in_div, sigma, sigma_down, sigma_up, 0, c_in_div_next, guidance}; the
    noise is drawn inside the step kernel from a Philox counter keyed by one int64 seed per panel and indexed by the
    device step counter (include/diffsensei_hip.h, "device noise"), so a captured step graph needs no host work between
    replays and a panel's noise does not depend on the batch it runs in.  Scalars are 0-dim fp32 torch values computed
    in diffusers' order; the last row (sigma_to = 0) has sigma_up = sigma_down = 0."""
    kind = KIND_EULER_ANCESTRAL
    order = 1
    stochastic = True   # the pipeline draws `noise_seeds` for such a scheduler (after the initial latents)
    # diffusers' constructor defaults for this class (linear betas: NOT the SDXL schedule, so a bare config is refused)
    _DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0,
                     rescale_betas_zero_snr=False)
    # keys whose other values change the schedule or the update rule: only what the device kernel implements is accepted
    _SUPPORTED = {"beta_schedule": ("scaled_linear",), "trained_betas": (None,), "prediction_type": ("epsilon",),
                  "timestep_spacing": ("leading", "linspace", "trailing"), "rescale_betas_zero_snr": (False,)}

    def __init__(self, **kwargs):
        cfg = _Config(self._DEFAULTS)
        cfg.update({k: v for k, v in kwargs.items() if k in self._DEFAULTS})   # other keys: not this class's (ignored)
        for key, ok in self._SUPPORTED.items():
            if isinstance(cfg[key], (list, tuple)) or cfg[key] not in ok:
                raise NotImplementedError(f"scheduler config {key}={cfg[key]!r}: the MI355X Euler Ancestral kernel "
                                          f"implements {key} in {ok} only")
        self.config = cfg
        self.T = int(cfg["num_train_timesteps"])
        self.alphas_cumprod = _alphas_cumprod(self.T, cfg["beta_start"], cfg["beta_end"])
        ac = self.alphas_cumprod.numpy()
        self.sigmas = torch.from_numpy(np.concatenate([np.array(((1 - ac) / ac) ** 0.5)[::-1], [0.0]]).astype(np.float32))
        self.timesteps = None
        self.num_inference_steps = None
        self._step_index = 0
        self._seeds = None
        self._dev = None

    @classmethod
    def _config_keys(cls):
        return tuple(cls._DEFAULTS)

    @property
    def init_noise_sigma(self) -> float:
        smax = self.sigmas.max()
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return float(smax)
        return float((smax ** 2 + 1) ** 0.5)

    def set_timesteps(self, num_inference_steps: int, device=None):
        cfg, n, T = self.config, int(num_inference_steps), self.T
        if cfg.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif cfg.timestep_spacing == "leading":
            step_ratio = T // n
            ts = (np.arange(0, n) * step_ratio).round()[::-1].copy().astype(np.float32)
            ts += cfg.steps_offset
        else:  # trailing
            step_ratio = T / n
            ts = (np.arange(T, 0, -step_ratio)).round().copy().astype(np.float32)
            ts -= 1
        ac = self.alphas_cumprod.numpy()
        sig = np.array(((1 - ac) / ac) ** 0.5)
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps_np = ts
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self.num_inference_steps = n
        self._step_index = 0
        self._seeds = None      # the stand-alone `step` draws new seeds for a new run
        self._dev = None

    def sigma_up_down(self, i: int):
        """(sigma_up, sigma_down) of row i, 0-dim fp32 tensors in diffusers' order of operations."""
        sigma_from, sigma_to = self.sigmas[i], self.sigmas[i + 1]
        sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
        sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
        return sigma_up, sigma_down

    def coef_table(self, guidance_scale: float) -> np.ndarray:
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        n = self.num_inference_steps
        tab = np.zeros((n, 8), dtype=np.float32)
        s = self.sigmas.numpy()
        div = ((s ** 2 + 1) ** 0.5).astype(np.float32)   # fp32 like the 0-dim sigma tensor arithmetic in diffusers
        tab[:, 0] = self.timesteps_np
        tab[:, 1] = div[:n]
        tab[:, 2] = s[:n]
        for i in range(n):
            up, down = self.sigma_up_down(i)
            tab[i, 3], tab[i, 4] = float(down), float(up)
        tab[:, 6] = div[1:n + 1]
        tab[:, 7] = guidance_scale
        return tab

    def solver_table(self) -> Optional[np.ndarray]:
        return None

    # -- stand-alone protocol (one kernel launch each; the pipeline's fused loop does not go through these)
    def _index_of(self, t) -> int:
        idx = np.nonzero(np.isclose(np.asarray(self.timesteps_np, dtype=np.float64), float(t)))[0]
        return int(idx[0]) if len(idx) else self._step_index

    def scale_model_input(self, sample: torch.Tensor, timestep) -> torch.Tensor:
        i = self._index_of(timestep)
        div = float(self.coef_table(1.0)[i, 1])
        ns, c, h, w = sample.shape
        table = torch.tensor([[0, div, 0, 0, 0, 0, 1, 1]], dtype=torch.float32, device=sample.device)
        tmp = torch.empty((ns, h * w, c), dtype=torch.float16, device=sample.device)
        ops.prepare_model_input(sample.contiguous(), tmp, table, do_cfg=False)
        return ops.nhwc_to_nchw(tmp).reshape(ns, c, h, w)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None,
             return_dict: bool = True, **kw):
        """model_output: the (already CFG-combined) noise prediction, NCHW like `sample`.  The per-panel seeds are drawn
        once per run (`draw_noise_seeds(batch, generator)` at the first step after `set_timesteps`, kept in
        `noise_seeds`); the noise of step i is the device's Philox draw for (seed, pixel, i)."""
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps first")
        i = self._index_of(timestep)
        ns, c, h, w = sample.shape
        dev = sample.device
        if self._seeds is None or len(self._seeds) != ns:
            self._seeds = draw_noise_seeds(ns, generator)
            self._dev = None
        if self._dev is None or self._dev[0].device != dev:
            self._dev = (torch.from_numpy(self.coef_table(1.0)).to(dev),
                         torch.tensor(self._seeds, dtype=torch.int64, device=dev))
        table, seeds = self._dev
        ctr = torch.tensor([i], dtype=torch.int32, device=dev)
        eps = ops.nchw_to_nhwc(model_output.to(torch.float16).reshape(ns, c, h * w).contiguous())
        lat = sample.to(torch.float16).contiguous().clone()
        scratch = torch.empty((ns, h * w, c), dtype=torch.float16, device=dev)
        ops.cfg_sampler_step_noise(eps, lat, scratch, table, seeds, self.kind, do_cfg=False, ctr=ctr)
        self._step_index = i + 1
        return (lat,) if not return_dict else {"prev_sample": lat}

    @property
    def noise_seeds(self):
        """The seeds of the current stand-alone run (None before its first `step`)."""
        return None if self._seeds is None else list(self._seeds)


def _sigma_to_t(sigmas: np.ndarray, log_sigmas: np.ndarray) -> np.ndarray:
    """diffusers `_sigma_to_t` [3P]: piecewise-linear interpolation of log-sigma back to (fractional) timesteps."""
    log_sigma = np.log(np.maximum(sigmas, 1e-10))
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return (1 - w) * low_idx + w * high_idx
