"""DPMSolverMultistepScheduler (DPM-Solver++ 2M) host side, CPU only: the schedule and the per-step solver rows against
the test restatement (tests/_dpm_ref.py), config handling (refusals, `.config`, `from_config`, loading from a checkpoint
directory), and an analytic check of the solver math on Gaussian data, where the probability-flow ODE and the
epsilon-predictor are exact."""
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

from tests._dpm_ref import DPMSolverOracle
from tests._sampler_common import SDXL



def _dpm(**kw):
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**dict(SDXL, **kw))


@pytest.mark.parametrize("spacing,karras,final,lof",
                         list(itertools.product(("leading", "linspace", "trailing"), (False, True),
                                                ("zero", "sigma_min"), (True, False))))
def test_schedule_matches_restatement(spacing, karras, final, lof):
    for n in (1, 2, 3, 5, 14, 15, 25, 50):
        kw = dict(timestep_spacing=spacing, use_karras_sigmas=karras, final_sigmas_type=final, lower_order_final=lof)
        sch = _dpm(**kw)
        sch.set_timesteps(n)
        ref = DPMSolverOracle(**kw).set_timesteps(n)
        what = f"{kw} n={n}"
        assert np.array_equal(sch.timesteps.numpy(), ref.timesteps), what
        assert sch.timesteps.dtype == torch.int64
        sig = sch.sigmas.numpy().astype(np.float64)
        assert sig.shape == ref.sigmas.shape, what
        assert np.allclose(sig, ref.sigmas, rtol=1e-6, atol=0), what
        assert sch.step_orders().tolist() == ref.orders, what
        coef = sch.coef_table(7.5)
        assert np.array_equal(coef[:, 0], ref.timesteps.astype(np.float32))
        assert (coef[:, 1] == 1).all() and (coef[:, 6] == 1).all() and (coef[:, 7] == 7.5).all()
        assert (coef[:, 2:6] == 0).all()
        rows = sch.solver_table()
        assert rows.shape == (len(ref.timesteps), 8) and rows.dtype == np.float32
        assert np.isfinite(rows).all(), what
        assert rows[:, 0].tolist() == [float(o) for o in ref.orders]
        for i, o in enumerate(ref.orders):
            s_s, a_s, a, b, inv_r0, c = ref.coefficients(i, o)
            c = c if sch.config.solver_type == "midpoint" else -c
            want = np.array([s_s, a_s, a, b, inv_r0, c])
            assert np.allclose(rows[i, 1:7], want, rtol=2e-5, atol=2e-6), (what, i, rows[i], want)


def test_final_row_of_a_zero_final_sigma():
    for karras, solver_type in itertools.product((False, True), ("midpoint", "heun")):
        sch = _dpm(use_karras_sigmas=karras, solver_type=solver_type)
        sch.set_timesteps(25)
        last = sch.solver_table()[-1]
        assert last[0] == 1 and last[3] == 0 and last[4] == -1 and np.isfinite(last).all()


def test_heun_rows_and_first_order_solver():
    sch = _dpm(solver_type="heun", use_karras_sigmas=True)
    sch.set_timesteps(10)
    ref = DPMSolverOracle(solver_type="heun", use_karras_sigmas=True).set_timesteps(10)
    rows = sch.solver_table()
    for i in range(1, 9):
        c = ref.coefficients(i, 2)[5]
        assert rows[i, 6] == pytest.approx(-c, rel=2e-5)
    one = _dpm(solver_order=1)
    one.set_timesteps(20)
    assert (one.step_orders() == 1).all() and (one.solver_table()[:, 5:7] == 0).all()
    # euler_at_final and lower_order_final with a sigma_min final sigma
    for eaf, lof, n, last in ((True, False, 20, 1), (False, False, 20, 2), (False, True, 14, 1), (False, True, 15, 2)):
        s = _dpm(final_sigmas_type="sigma_min", euler_at_final=eaf, lower_order_final=lof)
        s.set_timesteps(n)
        assert s.step_orders()[-1] == last and s.step_orders()[0] == 1


REFUSED = [("algorithm_type", "dpmsolver"), ("algorithm_type", "sde-dpmsolver++"), ("algorithm_type", "sde-dpmsolver"),
           ("solver_order", 3), ("thresholding", True), ("use_lu_lambdas", True), ("use_exponential_sigmas", True),
           ("use_beta_sigmas", True), ("use_flow_sigmas", True), ("variance_type", "learned_range"),
           ("lambda_min_clipped", -5.1), ("rescale_betas_zero_snr", True), ("trained_betas", [0.1, 0.2]),
           ("prediction_type", "v_prediction"), ("prediction_type", "sample"), ("beta_schedule", "linear"),
           ("solver_type", "bh2"), ("final_sigmas_type", "denoise_to_zero"), ("timestep_spacing", "karras")]


@pytest.mark.parametrize("key,bad", REFUSED)
def test_refused_config_keys(key, bad):
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler
    with pytest.raises(NotImplementedError):
        _dpm(**{key: bad})
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler.from_config(_dpm().config, **{key: bad})


def test_defaults_are_diffusers_and_refused_without_sdxl_betas():
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler()                      # linear betas: not the SDXL schedule
    s = DPMSolverMultistepScheduler(beta_schedule="scaled_linear")
    c = s.config
    assert (c.beta_start, c.beta_end, c.timestep_spacing, c.steps_offset, c.solver_order) == (1e-4, 0.02, "linspace", 0, 2)
    assert (c.lower_order_final, c.euler_at_final, c.final_sigmas_type, c.solver_type) == (True, False, "zero", "midpoint")
    assert c["lambda_min_clipped"] == -math.inf and c.use_karras_sigmas is False
    assert s.init_noise_sigma == 1.0
    s.set_timesteps(4)
    x = torch.randn(1, 4, 2, 2)
    assert s.scale_model_input(x, s.timesteps[0]) is x
    # lambda_min_clipped = -inf accepted as written to JSON by diffusers
    DPMSolverMultistepScheduler(beta_schedule="scaled_linear", lambda_min_clipped=float("-inf"))


def test_from_config_swap_and_round_trips():
    from diffsensei_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler
    d = DPMSolverMultistepScheduler.from_config(EulerDiscreteScheduler().config, use_karras_sigmas=True)
    c = d.config
    assert (c.beta_start, c.beta_end, c.beta_schedule) == (0.00085, 0.012, "scaled_linear")
    assert (c.timestep_spacing, c.steps_offset, c.use_karras_sigmas) == ("leading", 1, True)
    assert torch.equal(d.alphas_cumprod, EulerDiscreteScheduler().alphas_cumprod)
    assert "interpolation_type" not in c and "clip_sample" not in c      # Euler-only keys are ignored
    DPMSolverMultistepScheduler.from_config(DDIMScheduler().config)
    for obj in (EulerDiscreteScheduler(), DDIMScheduler(), d, _dpm(solver_type="heun", final_sigmas_type="sigma_min")):
        again = type(obj).from_config(obj.config)
        assert again.config == obj.config and type(again) is type(obj)
        assert again.config is not obj.config
    # and back: the DPM config of an SDXL checkpoint builds Euler / DDIM again
    assert EulerDiscreteScheduler.from_config(DPMSolverMultistepScheduler.from_config(
        EulerDiscreteScheduler().config).config).config == EulerDiscreteScheduler().config
    assert DDIMScheduler.from_config(d.config, use_karras_sigmas=False).config == DDIMScheduler().config
    with pytest.raises(NotImplementedError):   # Karras stays refused by Euler, also through from_config
        EulerDiscreteScheduler.from_config(d.config)
    e = EulerDiscreteScheduler().config
    assert e.use_karras_sigmas is False and e["final_sigmas_type"] == "zero" and e.timestep_spacing == "leading"
    with pytest.raises(AttributeError):
        e.solver_order


def test_full_dpm_scheduler_config_loads_through_from_pretrained(tmp_path):
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler
    from diffsensei_amd.unet import UNetMangaModel
    from tests.test_from_pretrained import make_checkpoint_dir
    root = str(tmp_path / "image_generator")
    make_checkpoint_dir(root)
    unet = UNetMangaModel.from_config(root, subfolder="unet", torch_dtype=torch.float16, device="cpu")
    path = os.path.join(root, "scheduler", "scheduler_config.json")
    # an SDXL scheduler_config.json as diffusers writes it after `DPMSolverMultistepScheduler.from_config(...)`
    json.dump({"_class_name": "DPMSolverMultistepScheduler", "_diffusers_version": "0.27.0", "algorithm_type": "dpmsolver++",
               "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
               "dynamic_thresholding_ratio": 0.995, "euler_at_final": False, "final_sigmas_type": "zero",
               "lambda_min_clipped": -math.inf, "lower_order_final": True, "num_train_timesteps": 1000,
               "prediction_type": "epsilon", "sample_max_value": 1.0, "solver_order": 2, "solver_type": "midpoint",
               "steps_offset": 1, "thresholding": False, "timestep_spacing": "leading", "trained_betas": None,
               "use_karras_sigmas": True, "use_lu_lambdas": False, "variance_type": None, "clip_sample": False,
               "interpolation_type": "linear", "set_alpha_to_one": False, "skip_prk_steps": True},
              open(path, "w"))
    pipe = DiffSenseiPipeline.from_pretrained(root, unet=unet)
    s = pipe.scheduler
    assert isinstance(s, DPMSolverMultistepScheduler) and s.kind == 2
    assert s.config.use_karras_sigmas and s.config.timestep_spacing == "leading" and s.config.steps_offset == 1
    s.set_timesteps(25)
    ref = DPMSolverOracle(use_karras_sigmas=True).set_timesteps(25)
    assert np.array_equal(s.timesteps.numpy(), ref.timesteps)
    cfg = json.load(open(path))
    cfg["solver_order"] = 3
    json.dump(cfg, open(path, "w"))
    with pytest.raises(NotImplementedError):
        DiffSenseiPipeline.from_pretrained(root, unet=unet)


# ---- analytic check: x0 ~ N(0, S^2) has the exact epsilon-predictor sigma*x/(alpha^2 S^2 + sigma^2) (VP) and an exact
# probability-flow solution x_u = x_t * std_u / std_t; the emitted fp32 tables are run in float64 with that predictor.
S2 = 0.5 ** 2


def _dpm_error(n: int, order: int, karras: bool = True) -> float:
    sch = _dpm(solver_order=order, use_karras_sigmas=karras)
    sch.set_timesteps(n)
    rows = sch.solver_table().astype(np.float64)
    std = lambda r: math.sqrt(r[2] ** 2 * S2 + r[1] ** 2)      # VP marginal std at the row's sigma_s

    def run(x, rs, prev=float("nan")):
        for r in rs:
            o, s_s, a_s, a, b, inv_r0, c = r[:7]
            x0 = (x - s_s * (s_s * x / (a_s ** 2 * S2 + s_s ** 2))) / a_s
            x = a * x - b * x0 - (c * (x0 - prev) * inv_r0 if o == 2 else 0.0)
            prev = x0
        return x

    x_init = std(rows[0])
    got = run(x_init, rows)
    ref = run(x_init * std(rows[-1]) / std(rows[0]), rows[-1:])   # exact state at the last nonzero sigma + final step
    assert rows[-1][0] == 1 and rows[-1][3] == 0
    return abs(got - ref) / abs(ref)


def _euler_error(n: int) -> float:
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(n)
    tab = sch.coef_table(1.0).astype(np.float64)
    std = lambda s: math.sqrt(S2 + s ** 2)                     # VE marginal std

    def run(x, rs):
        for r in rs:
            s, sn = r[2], r[3]
            x0 = x - s * (s * x / (S2 + s ** 2))
            x = x + (x - x0) / s * (sn - s)
        return x

    x_init = std(tab[0, 2])
    got = run(x_init, tab)
    ref = run(x_init * std(tab[-1, 2]) / std(tab[0, 2]), tab[-1:])
    return abs(got - ref) / abs(ref)


@pytest.mark.parametrize("order,gate", [(1, 0.8), (2, 1.6)])
def test_observed_order_of_convergence_on_gaussian_data(order, gate):
    """log2 of the error ratio as n doubles 10 -> 20 -> 40 (measured on CPU, Karras sigmas: order 1 1.01 / 1.01, order 2 1.87 / 2.13);
    the Euler table's error at the same n is printed for comparison only."""
    errs = {n: _dpm_error(n, order) for n in (10, 20, 40)}
    rates = [math.log2(errs[10] / errs[20]), math.log2(errs[20] / errs[40])]
    print(f"[dpm order {order}] rel errors {errs} observed orders {rates}; "
          f"euler {({n: _euler_error(n) for n in (10, 20, 40)})}")
    assert all(r >= gate for r in rates), (errs, rates)
    assert errs[40] < errs[20] < errs[10]
