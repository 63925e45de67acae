"""EulerAncestralDiscreteScheduler host side and the restated device noise, CPU only: the Philox restatement against the
Random123 known answers, moments of the restated normals, the schedule against tests/_euler_a_ref.py, an analytic check
of the update on Gaussian data, config handling, and where the per-panel seeds come from."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests._euler_a_ref import EulerAncestralOracle
from tests._philox_ref import MOMENT_HW, MOMENT_SEEDS, moment_conditions, philox4x32_10, philox_normal, philox_u32, uniforms
from tests._sampler_common import SDXL

SPACINGS = ("leading", "linspace", "trailing")


def _ea(**kw):
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler
    return EulerAncestralDiscreteScheduler(**dict(SDXL, **kw))


# ---------------------------------------------------------------- 1. the generator
# philox4x32-10 rows of Random123's known-answer file (counter, key -> output).  All three were run against this
# restatement and against a second, separately written pure-integer Philox: both give these words.
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _philox_ints(c, k):
    """A second Philox4x32-10, plain Python integers, to cross-check the vectorised restatement."""
    c, k = list(c), list(k)
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) % 2 ** 32, (k[1] + 0xBB67AE85) % 2 ** 32]
        a, b = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(b >> 32) ^ c[1] ^ k[0], b % 2 ** 32, (a >> 32) ^ c[3] ^ k[1], a % 2 ** 32]
    return tuple(c)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = tuple(int(v) for v in philox4x32_10(counter, key))
    assert got == want, " ".join(f"{v:08x}" for v in got)
    assert _philox_ints(counter, key) == want


def test_philox_counter_layout_and_uniforms():
    """key = (seed lo, seed hi), counter = (pixel, 0, step, stream); u = x 2^-32 + 2^-33 in fp32, in (0, 1]."""
    seed, step, stream, HW = 0x123456789ABCDEF, 7, 0, 5
    x = philox_u32([seed], step, stream, HW)
    assert x.shape == (1, HW, 4) and x.dtype == np.uint32
    for pix in range(HW):
        assert tuple(int(v) for v in x[0, pix]) == _philox_ints((pix, 0, step, stream), (0x89ABCDEF, 0x01234567))
    assert not np.array_equal(philox_u32([seed], step, 1, HW), x)            # the reserved streams are other streams
    u = uniforms(np.array([0, 1, 0x7fffffff, 0xffffffff], dtype=np.uint32))
    assert u.dtype == np.float32 and u[0] == np.float32(2.0 ** -33) and u[-1] == 1.0 and (u > 0).all()
    z = philox_normal([seed, seed + 1], step, stream, HW)
    assert z.shape == (2, 4, HW) and np.isfinite(z).all()
    # a panel's noise does not depend on the panels beside it
    assert np.array_equal(philox_normal([seed + 1], step, stream, HW)[0], z[1])


@pytest.mark.parametrize("step", (0, 1, 49))
def test_restated_normals_moments(step):
    """4-sigma conditions on 2^20 restated normals (16 seeds x 128 x 128 x 4) - the seeds and steps the GPU test uses."""
    z = philox_normal(MOMENT_SEEDS, step, 0, MOMENT_HW)
    assert z.size == 2 ** 20
    cond = moment_conditions(z, philox_normal(MOMENT_SEEDS, step + 1, 0, MOMENT_HW))
    print({k: f"{v:.3g} (<= {b:.3g})" for k, (v, b) in cond.items()})
    bad = {k: vb for k, vb in cond.items() if not vb[0] <= vb[1]}
    assert not bad, bad


# ---------------------------------------------------------------- 3. the schedule
def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("spacing", SPACINGS)
def test_schedule_matches_restatement(spacing):
    for n in (1, 2, 5, 30, 50):
        offset = 1 if spacing == "leading" else 0
        sch = _ea(timestep_spacing=spacing, steps_offset=offset)
        sch.set_timesteps(n)
        ref = EulerAncestralOracle(timestep_spacing=spacing, steps_offset=offset).set_timesteps(n)
        what = f"{spacing} n={n}"
        assert sch.timesteps.dtype == torch.float32 and np.array_equal(sch.timesteps.numpy(), ref.timesteps), what
        assert sch.num_inference_steps == n and sch.sigmas.dtype == torch.float32
        assert sch.init_noise_sigma == pytest.approx(ref.init_noise_sigma, rel=1e-6), what
        tab = sch.coef_table(7.5)
        assert tab.shape == (n, 8) and tab.dtype == np.float32 and np.isfinite(tab).all(), what
        assert np.array_equal(tab[:, 0], ref.timesteps) and (tab[:, 5] == 0).all() and (tab[:, 7] == 7.5).all()
        want = np.zeros((n, 8), dtype=np.float32)
        for i in range(n):
            up, down = ref.up_down(i)
            want[i, 1:5] = [ref.c_in_div(i), ref.sigmas[i], down, up]
            want[i, 6] = ref.c_in_div(i + 1)
            # the fp32 scalars against their float64 values: sigma_up goes through 6 roundings and one subtraction of
            # squares (amplified by sigma_from^2 / (sigma_from^2 - sigma_to^2) < 8 on these schedules, halved by the
            # root): 1e-5 relative holds with room.  sigma_down^2 = sigma_to^2 - sigma_up^2 cancels almost completely
            # when sigma_to << sigma_from (sigma_down = sigma_to^2 / sigma_from), in diffusers' fp32 as here, so it is
            # held in absolute terms: 2e-5 sigma_to^2 from sigma_up's bound, twice that with the other roundings
            up64, down64 = ref.up_down_exact(i)
            assert tab[i, 4] == pytest.approx(up64, rel=1e-5, abs=0), what
            assert abs(float(tab[i, 3]) ** 2 - down64 ** 2) <= 4e-5 * float(ref.sigmas[i + 1]) ** 2, what
            assert tab[i, 4] ** 2 + tab[i, 3] ** 2 == pytest.approx(float(ref.sigmas[i + 1]) ** 2, rel=1e-5, abs=0), what
        assert (_ulps(tab[:, 1:7], want[:, 1:7]) <= 1).all(), (what, tab, want)
        assert tab[-1, 3] == 0 and tab[-1, 4] == 0 and tab[-1, 6] == 1, what      # sigma_to = 0: no noise, no NaN
        assert (tab[:-1, 4] > 0).all() and (tab[:-1, 3] > 0).all()


# ---------------------------------------------------------------- 4. analytic check on Gaussian data
def _gaussian_run(spacing, S, n=30, zero_up=False, seed=20260101, HW=128 * 128):
    """The emitted fp32 table run in float64 on 2^16 scalars x0 ~ N(0, S^2) with the exact predictor
    eps = sigma x / (S^2 + sigma^2) and restated noise; returns (sample std, the std the recursion below predicts)."""
    sch = _ea(timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0)
    sch.set_timesteps(n)
    tab = sch.coef_table(1.0).astype(np.float64)
    ref = EulerAncestralOracle(timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0).set_timesteps(n)
    rng = np.random.default_rng(7)
    x = rng.standard_normal(4 * HW) * math.sqrt(S * S + tab[0, 2] ** 2)
    var = S * S + float(ref.sigmas[0]) ** 2
    for i in range(n):
        s, down, up = tab[i, 2], tab[i, 3], 0.0 if zero_up else tab[i, 4]
        eps = s * x / (S * S + s * s)
        x = x + (x - (x - s * eps)) / s * (down - s) + up * philox_normal([seed], i, 0, HW).ravel()
        # what the published algorithm does to the variance, from the restatement's float64 scalars: the Euler part
        # scales x by (S^2 + sigma_to^2) / (S^2 + sigma_from^2) (sigma_from * sigma_down = sigma_to^2), then sigma_up^2
        f2, t2 = float(ref.sigmas[i]) ** 2, float(ref.sigmas[i + 1]) ** 2
        var = var * ((S * S + t2) / (S * S + f2)) ** 2 + ref.up_down_exact(i)[0] ** 2
    return x.std(), math.sqrt(var)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_ancestral_step_on_gaussian_data(spacing):
    """For x0 ~ N(0, S^2) the predictor eps = sigma x / (S^2 + sigma^2) is exact and every step is linear in x, so the
    variance after a step is known in closed form:
        var' = var * ((S^2 + sigma_to^2) / (S^2 + sigma_from^2))^2 + sigma_up^2
             = (S^2 + sigma_to^2) - S^2 (sigma_from^2 - sigma_to^2)^2 / (sigma_from^2 (S^2 + sigma_from^2))   on the marginal.
    The second term is the Euler step's own discretisation error: an ancestral Euler step does NOT map
    N(0, S^2 + sigma_from^2) exactly onto N(0, S^2 + sigma_to^2) (only for S = 0), and over 30 SDXL steps the final std
    is 14 % (S = 0.5) below S.  The check is therefore against the propagated closed form, at the statistical bound
    4 std / sqrt(2 N) of a sample std over N = 2^16 scalars; with sigma_up zeroed the same run must miss it."""
    S, N = 0.5, 2 ** 16
    got, want = _gaussian_run(spacing, S)
    print(f"[{spacing}] final std {got:.5f}, propagated {want:.5f}, S {S}")
    assert abs(got - want) <= 4 * want / math.sqrt(2 * N), (got, want)
    assert 0.5 * S < want < S                       # the known shrinkage of Euler a, not a broken schedule
    no_noise, _ = _gaussian_run(spacing, S, zero_up=True)
    assert abs(no_noise - want) > 4 * want / math.sqrt(2 * N), (no_noise, want)


# ---------------------------------------------------------------- 5. config behaviour
def test_defaults_are_diffusers_and_refused_without_sdxl_betas():
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler
    with pytest.raises(NotImplementedError):
        EulerAncestralDiscreteScheduler()                      # linear betas: not the SDXL schedule
    s = EulerAncestralDiscreteScheduler(beta_schedule="scaled_linear")
    c = s.config
    assert dict(c) == dict(num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="scaled_linear",
                           trained_betas=None, prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0,
                           rescale_betas_zero_snr=False)
    assert s.kind == 3 and s.order == 1 and s.stochastic and s.solver_table() is None
    assert _ea().config.timestep_spacing == "leading" and _ea().config.steps_offset == 1
    # before set_timesteps init_noise_sigma is taken from the training sigmas, like diffusers
    e = _ea()
    smax = float(e.sigmas.max())
    assert e.init_noise_sigma == pytest.approx(math.sqrt(smax ** 2 + 1), rel=1e-6)
    assert _ea(timestep_spacing="trailing", steps_offset=0).init_noise_sigma == pytest.approx(smax, rel=1e-6)
    with pytest.raises(RuntimeError):
        e.coef_table(1.0)


REFUSED = [("trained_betas", [0.1, 0.2]), ("prediction_type", "v_prediction"), ("prediction_type", "sample"),
           ("rescale_betas_zero_snr", True), ("beta_schedule", "linear"), ("beta_schedule", "squaredcos_cap_v2"),
           ("timestep_spacing", "karras")]


@pytest.mark.parametrize("key,bad", REFUSED)
def test_refused_config_keys(key, bad):
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler
    with pytest.raises(NotImplementedError):
        _ea(**{key: bad})
    with pytest.raises(NotImplementedError):
        EulerAncestralDiscreteScheduler.from_config(_ea().config, **{key: bad})


def test_from_config_swap_and_round_trips():
    from diffsensei_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,
                                           EulerDiscreteScheduler)
    a = EulerAncestralDiscreteScheduler.from_config(EulerDiscreteScheduler().config)
    c = a.config
    assert (c.beta_start, c.beta_end, c.beta_schedule) == (0.00085, 0.012, "scaled_linear")
    assert (c.timestep_spacing, c.steps_offset, c.prediction_type) == ("leading", 1, "epsilon")
    assert torch.equal(a.alphas_cumprod, EulerDiscreteScheduler().alphas_cumprod)
    assert "interpolation_type" not in c and "use_karras_sigmas" not in c      # Euler-only keys are ignored
    EulerAncestralDiscreteScheduler.from_config(DDIMScheduler().config)
    d = DPMSolverMultistepScheduler.from_config(EulerDiscreteScheduler().config, use_karras_sigmas=True)
    assert EulerAncestralDiscreteScheduler.from_config(d.config).config == c
    again = EulerAncestralDiscreteScheduler.from_config(c)
    assert again.config == c and again.config is not c and type(again) is EulerAncestralDiscreteScheduler
    # and back: the existing classes and their configs are what they were
    assert EulerDiscreteScheduler.from_config(c).config == EulerDiscreteScheduler().config
    assert DDIMScheduler.from_config(c).config == DDIMScheduler().config
    assert DPMSolverMultistepScheduler.from_config(c).config == \
        DPMSolverMultistepScheduler.from_config(EulerDiscreteScheduler().config).config
    # Euler a's leading schedule is Euler's: same timesteps, same sigmas, same model-input scaling
    e = EulerDiscreteScheduler()
    e.set_timesteps(20)
    a.set_timesteps(20)
    assert np.array_equal(a.timesteps.numpy(), e.timesteps.numpy()) and np.array_equal(a.sigmas.numpy(), e.sigmas)
    assert a.init_noise_sigma == e.init_noise_sigma
    ta, te = a.coef_table(5.0), e.coef_table(5.0)
    assert np.array_equal(ta[:, [0, 1, 2, 6, 7]], te[:, [0, 1, 2, 6, 7]])
    for existing in (EulerDiscreteScheduler, DDIMScheduler, DPMSolverMultistepScheduler):
        assert not getattr(existing, "stochastic", False)


def _checkpoint_pipe(tmp_path, scheduler_json):
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.unet import UNetMangaModel
    from tests.test_from_pretrained import make_checkpoint_dir
    root = str(tmp_path / "image_generator")
    make_checkpoint_dir(root)
    unet = UNetMangaModel.from_config(root, subfolder="unet", torch_dtype=torch.float16, device="cpu")
    path = os.path.join(root, "scheduler", "scheduler_config.json")
    json.dump(scheduler_json, open(path, "w"))
    return DiffSenseiPipeline.from_pretrained(root, unet=unet), root, unet, path


# an SDXL scheduler_config.json as diffusers writes it after `EulerAncestralDiscreteScheduler.from_config(...)`
EA_JSON = {"_class_name": "EulerAncestralDiscreteScheduler", "_diffusers_version": "0.27.0", "beta_end": 0.012,
           "beta_schedule": "scaled_linear", "beta_start": 0.00085, "num_train_timesteps": 1000,
           "prediction_type": "epsilon", "rescale_betas_zero_snr": False, "steps_offset": 1,
           "timestep_spacing": "leading", "trained_betas": None, "clip_sample": False, "interpolation_type": "linear",
           "set_alpha_to_one": False, "skip_prk_steps": True, "use_karras_sigmas": False}


def test_scheduler_config_loads_through_from_pretrained(tmp_path):
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler
    pipe, root, unet, path = _checkpoint_pipe(tmp_path, EA_JSON)
    s = pipe.scheduler
    assert isinstance(s, EulerAncestralDiscreteScheduler) and s.kind == 3
    assert s.config.timestep_spacing == "leading" and s.config.steps_offset == 1
    s.set_timesteps(30)
    assert np.array_equal(s.timesteps.numpy(), EulerAncestralOracle().set_timesteps(30).timesteps)
    json.dump(dict(EA_JSON, prediction_type="v_prediction"), open(path, "w"))
    with pytest.raises(NotImplementedError):
        DiffSenseiPipeline.from_pretrained(root, unet=unet)


# ---------------------------------------------------------------- 5b. where the seeds come from
def test_draw_noise_seeds():
    from diffsensei_amd.schedulers import draw_noise_seeds
    g = torch.Generator().manual_seed(11)
    a = draw_noise_seeds(3, g)
    want = torch.randint(0, 2 ** 63 - 1, (3,), generator=torch.Generator().manual_seed(11)).tolist()
    assert a == want and all(isinstance(v, int) and 0 <= v < 2 ** 63 - 1 for v in a)
    assert draw_noise_seeds(3, torch.Generator().manual_seed(11)) == a          # same generator state -> same seeds
    assert draw_noise_seeds(3, g) != a                                          # the generator has moved on
    # a list of generators: one draw from each, so a panel's seed depends on its own generator only
    gens = lambda seeds: [torch.Generator().manual_seed(s) for s in seeds]
    x, y = draw_noise_seeds(3, gens([1, 2, 3])), draw_noise_seeds(3, gens([9, 2, 8]))
    assert x[1] == y[1] and x[0] != y[0] and x[2] != y[2]
    assert x[1] == int(torch.randint(0, 2 ** 63 - 1, (1,), generator=torch.Generator().manual_seed(2)))
    with pytest.raises(ValueError):
        draw_noise_seeds(2, gens([1, 2, 3]))
    torch.manual_seed(5)
    b = draw_noise_seeds(2)
    torch.manual_seed(5)
    assert b == torch.randint(0, 2 ** 63 - 1, (2,)).tolist()                    # generator None: the global generator


def test_conditioning_draws_seeds_after_the_initial_latents(tmp_path):
    """`_conditioning` on a CPU pipeline (the reference-image branch stubbed out: it needs the GPU): a stochastic
    scheduler takes its seeds from the generator AFTER prepare_latents, a deterministic one does not touch it."""
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    pipe, *_ = _checkpoint_pipe(tmp_path, EA_JSON)
    cfg = pipe.unet.config
    z = torch.zeros(2, 1, 4)
    pipe.prepare_ip_image_embeds = lambda *a, **k: (z, z, z, z)
    pe = torch.zeros(1, 77, cfg.cross_attention_dim)
    pooled = torch.zeros(1, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim)

    def cond(seed, **kw):
        g = None if seed is None else torch.Generator().manual_seed(seed)
        names = dict(prompt="p", prompt_2=None, height=64, width=64, num_inference_steps=4, guidance_scale=5.0,
                     negative_prompt=None, negative_prompt_2=None, num_samples=2, generator=g, original_size=None,
                     crops_coords_top_left=(0, 0), target_size=None, ip_images=[], ip_image_embeds=None, ip_bbox=[],
                     ip_scale=1.0, dialog_bbox=[], latents=None, prompt_embeds=pe, negative_prompt_embeds=None,
                     pooled_prompt_embeds=pooled, negative_pooled_prompt_embeds=None)
        return pipe._conditioning(*names.values(), **kw), g

    assert isinstance(pipe.scheduler, EulerAncestralDiscreteScheduler)
    (a, ga), (b, _) = cond(3), cond(3)
    assert a["noise_seeds"] == b["noise_seeds"] and len(a["noise_seeds"]) == 2 and torch.equal(a["lat"], b["lat"])
    assert cond(4)[0]["noise_seeds"] != a["noise_seeds"]
    # the documented derivation: randn for the latents first, then randint for the seeds, from the same generator
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float16)
    assert a["noise_seeds"] == torch.randint(0, 2 ** 63 - 1, (2,), generator=g).tolist()
    assert torch.equal(ga.get_state(), g.get_state())
    over, go = cond(3, noise_seeds=[5, 2 ** 63 - 2])
    assert over["noise_seeds"] == [5, 2 ** 63 - 2] and torch.equal(over["lat"], a["lat"])
    for bad in ([5], [5, -1], [5, 2 ** 63]):
        with pytest.raises(ValueError):
            cond(3, noise_seeds=bad)
    # Euler on the same generator: the same initial latents, no seeds, and the generator consumed by the latents only
    pipe.scheduler = EulerDiscreteScheduler.from_config(pipe.scheduler.config)
    e, ge = cond(3)
    assert e["noise_seeds"] is None
    assert torch.equal(e["lat"], a["lat"]) and torch.equal(e["lat"], lat * pipe.scheduler.init_noise_sigma)
    g2 = torch.Generator().manual_seed(3)
    torch.randn(2, 4, 8, 8, generator=g2, dtype=torch.float16)
    assert torch.equal(ge.get_state(), g2.get_state())
    with pytest.raises(ValueError):
        cond(3, noise_seeds=[1, 2])
