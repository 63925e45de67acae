"""LCMScheduler host side, CPU only: the timestep grid, the three tables against the golden file (bit for bit) and against
the float64 restatement of tests/_lcm_ref.py (derived bounds), config handling, and panel schedules.

Bounds of the restatement check.  The code under test keeps diffusers' fp32 `alphas_cumprod`: a cumulative product of
t + 1 factors 1 - beta_j, each correct to about half an ulp (beta <= 0.012 is itself a few ulps off, which 1 - beta shrinks
a hundredfold), each product rounded once - a relative error of at most (t + 1) 2^-24 in abar_t, held here at
    |d abar| <= (3 (t + 1) + 8) 2^-24 abar          (three times the textbook forward bound, so no seed of luck is needed)
which the square roots pass on as d sqrt(a) = da / (2 sqrt(a)), d sqrt(1 - a) = da / (2 sqrt(1 - a)), plus one ulp for the
root and the store.  c_out and c_skip are four fp32 operations on the exact integer-valued s = 10 t: 4 ulps.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests._lcm_ref import LCMOracle

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "lcm_tables.npz")
U = 2.0 ** -24


def _lcm(**kw):
    from diffsensei_amd.schedulers import LCMScheduler
    return LCMScheduler(**kw)


# ---------------------------------------------------------------- 1. the grid
GRIDS = {4: [999, 759, 499, 259], 8: [999, 879, 759, 639, 499, 379, 259, 139], 3: [999, 679, 339], 1: [999],
         50: list(range(999, 0, -20))}


@pytest.mark.parametrize("n", sorted(GRIDS))
def test_timesteps(n):
    s = _lcm()
    s.set_timesteps(n)
    assert s.timesteps.tolist() == GRIDS[n] and s.timesteps.dtype == torch.int64 and s.num_inference_steps == n
    assert GRIDS[50][-1] == 19 and len(GRIDS[50]) == 50
    assert s.init_noise_sigma == 1.0
    assert LCMOracle().set_timesteps(n).timesteps.tolist() == GRIDS[n]


def test_too_many_steps_raise():
    s = _lcm()
    with pytest.raises(ValueError):
        s.set_timesteps(51)
    with pytest.raises(ValueError):
        s.set_timesteps(0)
    with pytest.raises(ValueError):
        _lcm(original_inference_steps=2000)                                   # more than the training timesteps
    s2 = _lcm(num_train_timesteps=40, original_inference_steps=40)
    with pytest.raises(ValueError):
        s2.set_timesteps(41)
    with pytest.raises(RuntimeError):
        _lcm().coef_table(1.0)
    with pytest.raises(RuntimeError):
        _lcm().solver_table()


# ---------------------------------------------------------------- 2. the tables
def test_tables_match_the_golden_file_bit_for_bit():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "dump_lcm_tables", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "dump_lcm_tables.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    now = tool.dump()
    with np.load(GOLDEN) as gold:
        assert sorted(gold.files) == sorted(now)
        for k in gold.files:
            a, b = gold[k], now[k]
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert a.tobytes() == b.tobytes(), f"{k}: the table moved"
    assert len(now) == 4 * len(tool.STEPS) * len(tool.CONFIGS)


@pytest.mark.parametrize("kw", [{}, dict(original_inference_steps=100, timestep_scaling=5.0)])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 50])
def test_tables_match_the_float64_restatement(n, kw):
    s = _lcm(**kw)
    s.set_timesteps(n)
    ref = LCMOracle(**kw).set_timesteps(n)
    coef, solver, renoise = ref.tables(2.5)
    tab, sol, ren = s.coef_table(2.5), s.solver_table(), s.renoise_table()
    assert tab.shape == (n, 8) and sol.shape == (n, 8) and ren.shape == (n + 1, 2)
    assert tab.dtype == sol.dtype == ren.dtype == np.float32
    assert np.array_equal(tab[:, 0], ref.timesteps) and (tab[:, 1] == 1).all() and (tab[:, 6] == 1).all() and (tab[:, 7] == 2.5).all()
    assert (sol[:, 2:] == 0).all() and tuple(sol[-1, :2]) == (1.0, 0.0) and tuple(ren[-1]) == (1.0, 0.0)

    def sqrt_bounds(t):
        a = ref.abar[t]
        da = (3 * (t + 1) + 8) * U * a
        return da / (2 * np.sqrt(a)) + 2 * U * np.sqrt(a), da / (2 * np.sqrt(1 - a)) + 2 * U * np.sqrt(1 - a)

    for i in range(n):
        t = int(ref.timesteps[i])
        ba, bb = sqrt_bounds(t)
        assert abs(float(tab[i, 2]) - coef[i, 2]) <= ba and abs(float(tab[i, 3]) - coef[i, 3]) <= bb, (n, i)
        assert abs(float(ren[i, 0]) - renoise[i, 0]) <= ba and abs(float(ren[i, 1]) - renoise[i, 1]) <= bb, (n, i)
        assert abs(float(tab[i, 4]) - coef[i, 4]) <= 4 * U * coef[i, 4] and abs(float(tab[i, 5]) - coef[i, 5]) <= 4 * U * coef[i, 5]
        if i < n - 1:
            pa, pb = sqrt_bounds(int(ref.timesteps[i + 1]))
            assert abs(float(sol[i, 0]) - solver[i, 0]) <= pa and abs(float(sol[i, 1]) - solver[i, 1]) <= pb, (n, i)
            assert sol[i, 0] == tab[i + 1, 2] and sol[i, 1] == tab[i + 1, 3]    # the next row's own pair, the same bits
    # the boundary condition: c_skip -> 0, c_out -> 1 away from t = 0, which no grid holds (the smallest s of these grids is
    # 5 * 9 = 45: c_skip = 0.25 / 2025.25 = 1.2e-4, c_out = 0.99994)
    assert (tab[:, 4] > 0.9999).all() and (tab[:, 5] < 2e-4).all() and (tab[:, 5] > 0).all()
    # a shortened run's solver rows are the tail of the whole run's
    for start in range(n):
        assert np.array_equal(s.solver_table(start=start), sol[start:])
    with pytest.raises(ValueError):
        s.solver_table(start=n)


def test_one_step_on_exact_data_returns_the_data():
    """x = sqrt(a) x0 + sqrt(1 - a) eps with the true eps: every row's denoised value is x0 up to c_skip (1e-9 at t = 999)."""
    ref = LCMOracle(seeds=[3]).set_timesteps(4)
    g = torch.Generator().manual_seed(0)
    x0, eps = torch.randn(1, 4, 8, 8, generator=g, dtype=torch.float64), torch.randn(1, 4, 8, 8, generator=g, dtype=torch.float64)
    for i in range(4):
        sa, sb, c_out, c_skip, pa, pb = ref.scalars(i)
        x = sa * x0 + sb * eps
        out = ref.step(eps, i, x)
        want = x0 if i == 3 else pa * x0 + pb * ref.noise(i, x.shape)
        assert float((out - want).abs().max()) <= 1e-4
    assert pa == 1.0 and pb == 0.0


# ---------------------------------------------------------------- 3. config behaviour
DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                original_inference_steps=50, timestep_scaling=10.0, steps_offset=0, timestep_spacing="leading",
                prediction_type="epsilon", clip_sample=False, thresholding=False, set_alpha_to_one=True,
                rescale_betas_zero_snr=False, trained_betas=None)


def test_defaults():
    s = _lcm()
    for k, v in DEFAULTS.items():
        assert s.config[k] == v, k
    assert s.kind == 4 and s.order == 1 and s.stochastic and s.init_noise_sigma == 1.0
    assert _lcm(set_alpha_to_one=False).config.set_alpha_to_one is False    # accepted, never reaches the arithmetic
    a, b = _lcm(set_alpha_to_one=False), _lcm()
    a.set_timesteps(4), b.set_timesteps(4)
    assert np.array_equal(a.coef_table(1.0), b.coef_table(1.0)) and np.array_equal(a.solver_table(), b.solver_table())
    from diffsensei_amd.schedulers import NOISE_KINDS, SOLVER_KINDS
    assert 4 in NOISE_KINDS and 4 in SOLVER_KINDS


REFUSED = [("beta_schedule", "linear"), ("beta_schedule", "squaredcos_cap_v2"), ("prediction_type", "v_prediction"),
           ("prediction_type", "sample"), ("clip_sample", True), ("thresholding", True), ("rescale_betas_zero_snr", True),
           ("trained_betas", [0.1, 0.2])]


@pytest.mark.parametrize("key,bad", REFUSED)
def test_refused_config_keys(key, bad):
    from diffsensei_amd.schedulers import LCMScheduler
    with pytest.raises(NotImplementedError):
        _lcm(**{key: bad})
    with pytest.raises(NotImplementedError):
        LCMScheduler.from_config(_lcm().config, **{key: bad})


def test_from_config_round_trips_with_the_four_existing_classes():
    from diffsensei_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,
                                           EulerDiscreteScheduler, LCMScheduler)
    euler = EulerDiscreteScheduler()
    olds = [euler, DDIMScheduler(), DPMSolverMultistepScheduler.from_config(euler.config, use_karras_sigmas=True),
            EulerAncestralDiscreteScheduler.from_config(euler.config)]
    for old in olds:
        before = dict(old.config)
        lcm = LCMScheduler.from_config(old.config)
        assert dict(old.config) == before                                     # the source config is not written to
        c = lcm.config
        assert (c.beta_start, c.beta_end, c.beta_schedule, c.prediction_type) == (0.00085, 0.012, "scaled_linear", "epsilon")
        assert c.original_inference_steps == 50 and c.timestep_scaling == 10.0
        assert torch.equal(lcm.alphas_cumprod, euler.alphas_cumprod)
        assert "use_karras_sigmas" not in c and "solver_order" not in c and "interpolation_type" not in c
        lcm.set_timesteps(4)
        assert lcm.timesteps.tolist() == GRIDS[4]                             # steps_offset = 1 of the SDXL config changes nothing
        # ... and back: the class and its config are what they were
        back = type(old).from_config(dict(c, **{k: v for k, v in old.config.items() if k not in c}))
        assert back.config == old.config and type(back) is type(old)
    # straight back from the LCM config alone: what the other class does not find there is its own default
    c = LCMScheduler.from_config(euler.config).config
    assert EulerDiscreteScheduler.from_config(c).config == euler.config
    assert DPMSolverMultistepScheduler.from_config(c).config == DPMSolverMultistepScheduler.from_config(euler.config).config
    assert EulerAncestralDiscreteScheduler.from_config(c).config == EulerAncestralDiscreteScheduler.from_config(euler.config).config
    assert DDIMScheduler.from_config(LCMScheduler.from_config(DDIMScheduler().config).config).config == DDIMScheduler().config
    # an LCM config that says set_alpha_to_one = True is a DDIM this project does not run: refused, not reinterpreted
    with pytest.raises(NotImplementedError):
        DDIMScheduler.from_config(c)
    again = LCMScheduler.from_config(c, original_inference_steps=100)
    assert again.config.original_inference_steps == 100 and c.original_inference_steps == 50


LCM_JSON = {"_class_name": "LCMScheduler", "_diffusers_version": "0.27.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
            "beta_start": 0.00085, "clip_sample": False, "clip_sample_range": 1.0, "dynamic_thresholding_ratio": 0.995,
            "num_train_timesteps": 1000, "original_inference_steps": 50, "prediction_type": "epsilon",
            "rescale_betas_zero_snr": False, "sample_max_value": 1.0, "set_alpha_to_one": True, "steps_offset": 1,
            "thresholding": False, "timestep_scaling": 10.0, "timestep_spacing": "leading", "trained_betas": None}


def test_scheduler_config_loads_through_from_pretrained(tmp_path):
    from diffsensei_amd.loading import load_scheduler
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.schedulers import SCHEDULERS, LCMScheduler
    from tests.test_euler_ancestral_scheduler import _checkpoint_pipe
    assert SCHEDULERS["LCMScheduler"] is LCMScheduler and len(SCHEDULERS) == 5
    pipe, root, unet, path = _checkpoint_pipe(tmp_path, LCM_JSON)
    s = pipe.scheduler
    assert isinstance(s, LCMScheduler) and s.kind == 4 and s.config.steps_offset == 1
    s.set_timesteps(8)
    assert s.timesteps.tolist() == GRIDS[8]
    assert isinstance(load_scheduler(os.path.dirname(path)), LCMScheduler)
    json.dump(dict(LCM_JSON, prediction_type="v_prediction"), open(path, "w"))
    with pytest.raises(NotImplementedError):
        DiffSenseiPipeline.from_pretrained(root, unet=unet)


# ---------------------------------------------------------------- 4. panel schedules and strength
def test_panel_schedule_full_and_half_strength():
    s = _lcm()
    s.set_timesteps(6)                                                        # the object's own state: stays what it is
    full = s.panel_schedule(4, 1.0, 1.25)
    assert s.num_inference_steps == 6 and len(s.timesteps) == 6
    ref = _lcm()
    ref.set_timesteps(4)
    assert full["t_start"] == 0 and full["steps"] == 4 and full["init_noise_sigma"] == 1.0
    assert np.array_equal(full["rows"], ref.coef_table(1.25)) and np.array_equal(full["solver_rows"], ref.solver_table())
    assert np.array_equal(full["renoise_rows"], ref.renoise_table()) and full["timesteps"].tolist() == GRIDS[4]
    # strength 0.5 of 4 steps: this project's start_index rule - the LAST two rows of the 4-step grid (not diffusers' LCM
    # img2img grid, which would re-derive the timesteps from original_inference_steps * strength)
    half = s.panel_schedule(4, 0.5, 1.25)
    assert half["t_start"] == 2 and half["steps"] == 2 and half["timesteps"].tolist() == GRIDS[4][2:]
    assert np.array_equal(half["rows"], ref.coef_table(1.25)[2:]) and np.array_equal(half["solver_rows"], ref.solver_table()[2:])
    assert half["renoise_rows"].shape == (3, 2) and np.array_equal(half["renoise_rows"], ref.renoise_table()[2:])
    assert tuple(half["solver_rows"][-1, :2]) == (1.0, 0.0)
    with pytest.raises(ValueError):
        s.panel_schedule(4, 0.1)                                              # int(4 * 0.1) = 0 steps
    with pytest.raises(ValueError):
        s.panel_schedule(51)
