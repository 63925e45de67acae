"""GPU: the device noise source (Philox4x32-10 + Box-Muller, keyed per panel) and Euler Ancestral (kind 3 of
sampler_step_kernel) against the test restatements tests/_philox_ref.py and tests/_euler_a_ref.py - the generator bit
for bit, whole n-step kernel sequences, batch invariance, the stand-alone `scheduler.step` loop and the whole
`DiffSenseiPipeline.__call__` / `generate_batch` (eager == graph, seeds, vs the oracle sampling loop, scheduler swaps).

Kernel tolerance: the 1.5e-3 of test_gpu_ops.py::test_cfg_sampler_step per step.  Model-level gates: <= 3x the value
measured on MI355X (logged by tests/_gates.gate)."""
import itertools

import numpy as np
import pytest
import torch

from tests._euler_a_ref import EulerAncestralOracle
from tests._gates import gate
from tests._philox_ref import MOMENT_HW, MOMENT_SEEDS, moment_conditions, philox_normal, philox_u32
from tests._sampler_common import DEV, DIALOG, IP_BBOX, SDXL, _close, _nhwc, _pipe, _rel, hq
from tests._sampler_common import parts  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
SEEDS3 = [0, 2 ** 63 - 2, 0x0123456789ABCDEF]


def _spacing_kw(spacing):
    return dict(timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0)


def _ea(**kw):
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler
    return EulerAncestralDiscreteScheduler(**dict(SDXL, **kw))


def _seeds_dev(seeds):
    return torch.tensor([int(s) for s in seeds], dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------- 6. the generator
@pytest.mark.parametrize("ns,H,W", [(3, 8, 12), (32, 128, 128)])
def test_philox_u32_bit_exact(hip_lib, ns, H, W):
    from diffsensei_amd import ops
    seeds = (SEEDS3 + [1000003 * k + 17 for k in range(ns)])[:ns]
    for step in (0, 1, 49):
        got = ops.philox_u32(_seeds_dev(seeds), step, H * W).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, philox_u32(seeds, step, 0, H * W)), (ns, step)
    assert np.array_equal(ops.philox_u32(_seeds_dev(seeds), 3, H * W, stream_id=1).cpu().numpy().view(np.uint32),
                          philox_u32(seeds, 3, 1, H * W))


def test_philox_normal_vs_restatement_and_moments(hip_lib):
    """fp32 Box-Muller on the device vs float64 on the same fp32 uniforms; hard condition 1e-3 (above it, sigma_up *
    error at late steps would eat the 1.5e-3 per-step kernel tolerance)."""
    from diffsensei_amd import ops
    worst = 0.0
    for seeds, hw in ((SEEDS3, 8 * 12), (MOMENT_SEEDS, MOMENT_HW)):
        for step in (0, 1, 49):
            got = ops.philox_normal(_seeds_dev(seeds), step, hw).cpu().numpy()
            assert got.shape == (len(seeds), 4, hw) and got.dtype == np.float32 and np.isfinite(got).all()
            worst = max(worst, float(np.abs(got - philox_normal(seeds, step, 0, hw)).max()))
    assert worst <= 1e-3, worst
    gate("test_gpu_euler_ancestral:1 max|z_dev - z_ref|", worst, 2.0e-6)   # measured 7.1e-7 (v_log / v_sin / v_cos in fp32)
    for step in (0, 1, 49):
        z, zn = (ops.philox_normal(_seeds_dev(MOMENT_SEEDS), s, MOMENT_HW).cpu().numpy() for s in (step, step + 1))
        bad = {k: vb for k, vb in moment_conditions(z, zn).items() if not vb[0] <= vb[1]}
        assert not bad, (step, bad)


# ---------------------------------------------------------------- 7. kernel sequences
def _sequence(ns, H, W, n, do_cfg, seed, spacing):
    """n steps of ds_cfg_sampler_step_noise_f16 (kind 3) with the device step counter, each checked against the
    restatement started from the kernel's own previous latents (see test_gpu_dpm._sequence)."""
    from diffsensei_amd import ops
    sch = _ea(**_spacing_kw(spacing))
    sch.set_timesteps(n)
    seeds = (SEEDS3 + [7919 * k + 5 for k in range(ns)])[:ns]
    orc = EulerAncestralOracle(seeds=seeds, **_spacing_kw(spacing)).set_timesteps(n)
    g = torch.Generator().manual_seed(seed)
    gs = 5.0
    tab_h = sch.coef_table(gs)
    table = torch.from_numpy(tab_h).to(DEV)
    lat_d = (torch.randn(ns, 4, H, W, generator=g) * sch.init_noise_sigma).half().to(DEV)
    rows = 2 * ns if do_cfg else ns
    xin = torch.empty(rows, H * W, 4, dtype=torch.float16, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    seeds_d = _seeds_dev(seeds)
    for i in range(n):
        eps = (torch.randn(rows, 4, H, W, generator=g) * 0.5).half()
        x_in = lat_d.float().cpu()
        ctr.fill_(i)
        ops.cfg_sampler_step_noise(_nhwc(eps).to(DEV), lat_d, xin, table, seeds_d, 3, do_cfg, ctr)
        if do_cfg:
            u, c = eps.float().chunk(2)
            e = hq(u + hq(gs * hq(c - u)))
        else:
            e = eps.float()
        what = f"{spacing} cfg={do_cfg} n={n} step {i}"
        _close(lat_d, hq(orc.step(e, i, x_in)), what=what)
        got = xin.view(rows, H, W, 4).permute(0, 3, 1, 2)
        _close(got[:ns], hq(lat_d.float().cpu() / float(tab_h[i, 6])), what=what + " model_in")
        if do_cfg:
            assert torch.equal(got[ns:], got[:ns]), "model_in (cond half) != model_in (uncond half)"
        if i == n - 1:   # sigma_to = 0: the last step adds no noise - it is the plain Euler step to sigma 0
            _close(lat_d, hq(x_in - float(tab_h[i, 2]) * e), what=what + " (last row: x0, no noise)")
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,do_cfg,spacing", list(itertools.product((5, 30), (True, False),
                                                                    ("leading", "linspace", "trailing"))))
def test_euler_a_kernel_sequence_vs_restatement(hip_lib, n, do_cfg, spacing):
    _sequence(3, 8, 12, n, do_cfg, seed=n * 3 + int(do_cfg), spacing=spacing)


def test_euler_a_kernel_sequence_batch64_shape(hip_lib):
    """UNet batch 64 at 1024^2: ns 32 samples of 128 x 128 latents, CFG on."""
    _sequence(32, 128, 128, 5, True, seed=3, spacing="leading")


# ---------------------------------------------------------------- 8. batch invariance, bit exact at kernel level
def test_noise_depends_on_seed_and_step_only(hip_lib):
    H, W, n, s = 8, 12, 6, 0x5EED5EED5EED
    g = torch.Generator().manual_seed(77)
    eps1 = [(torch.randn(1, 4, H, W, generator=g) * 0.5).half() for _ in range(n)]
    # the panel with seed s as row 0 of ns 1 and as row 2 of ns 4 with other seeds (and other latents, other eps)
    # around it: one step from the same inputs, at every step index
    from diffsensei_amd import ops
    sch = _ea()
    sch.set_timesteps(n)
    table = torch.from_numpy(sch.coef_table(1.0)).to(DEV)
    x0 = (torch.randn(1, 4, H, W, generator=g) * sch.init_noise_sigma).half()
    outs = {}
    for i in range(n):
        ctr = torch.tensor([i], dtype=torch.int32, device=DEV)
        for name, ns, row, seeds in (("alone", 1, 0, [s]), ("in batch", 4, 2, [11, 2 ** 63 - 2, s, 0]),
                                     ("again", 1, 0, [s]), ("other seed", 1, 0, [s + 1])):
            lat = (torch.randn(ns, 4, H, W, generator=torch.Generator().manual_seed(5)) * 3).half()
            lat[row] = x0[0]
            eps = (torch.randn(ns, 4, H, W, generator=torch.Generator().manual_seed(6)) * 0.5).half()
            eps[row] = eps1[i][0]
            lat_d = lat.to(DEV)
            xin = torch.empty(ns, H * W, 4, dtype=torch.float16, device=DEV)
            ops.cfg_sampler_step_noise(_nhwc(eps).to(DEV), lat_d, xin, table, _seeds_dev(seeds), 3, False, ctr)
            outs[name, i] = lat_d[row].cpu()
        assert torch.equal(outs["alone", i], outs["in batch", i]), f"step {i}: noise depends on the batch"
        assert torch.equal(outs["alone", i], outs["again", i]), f"step {i}: same (seed, step) twice differs"
        if i < n - 1:
            assert not torch.equal(outs["alone", i], outs["other seed", i])
    # different steps give different noise: the same inputs at step 0 and step 1 of a two-row table with equal rows
    row = sch.coef_table(1.0)[:1]
    tab2 = torch.from_numpy(np.concatenate([row, row])).to(DEV)
    res = []
    for i in (0, 1):
        lat_d = x0.to(DEV).clone()
        xin = torch.empty(1, H * W, 4, dtype=torch.float16, device=DEV)
        ops.cfg_sampler_step_noise(_nhwc(eps1[0]).to(DEV), lat_d, xin, tab2, _seeds_dev([s]), 3, False,
                                   torch.tensor([i], dtype=torch.int32, device=DEV))
        res.append(lat_d.cpu())
    assert not torch.equal(res[0], res[1])


# ---------------------------------------------------------------- 9. launch checks
def test_euler_a_kernel_launch_checks(hip_lib):
    from diffsensei_amd import _lib, ops
    lat = torch.zeros(1, 4, 4, 4, dtype=torch.float16, device=DEV)
    xin = torch.empty(1, 16, 4, dtype=torch.float16, device=DEV)
    eps = torch.zeros_like(xin)
    table = torch.ones(1, 8, device=DEV)
    seeds = _seeds_dev([1])
    with pytest.raises(_lib.DiffSenseiHipError):          # kind 3 without seeds, through both entry points
        ops.cfg_sampler_step(eps, lat, xin, table, 3, do_cfg=False)
    with pytest.raises(_lib.DiffSenseiHipError):
        ops.cfg_sampler_step_noise(eps, lat, xin, table, None, 3, do_cfg=False)
    with pytest.raises(_lib.DiffSenseiHipError):          # kind 4
        ops.cfg_sampler_step_noise(eps, lat, xin, table, seeds, 4, do_cfg=False)
    with pytest.raises(_lib.DiffSenseiHipError):          # kind 2 still needs its own buffers
        ops.cfg_sampler_step_noise(eps, lat, xin, table, seeds, 2, do_cfg=False)
    with pytest.raises(ValueError):                       # one seed per panel
        ops.cfg_sampler_step_noise(eps, lat, xin, table, _seeds_dev([1, 2]), 3, do_cfg=False)
    with pytest.raises(_lib.DiffSenseiHipError):
        ops.cfg_sampler_step_noise(eps, lat, xin, table, seeds.to(torch.int32), 3, do_cfg=False)
    ops.cfg_sampler_step_noise(eps, lat, xin, table, seeds, 3, do_cfg=False)
    ops.cfg_sampler_step_noise(eps, lat, xin, table, None, 0, do_cfg=False)      # Euler needs no seeds
    torch.cuda.synchronize()
    assert hip_lib.ds_version() >= 102


# ---------------------------------------------------------------- 10. the stand-alone protocol
def test_standalone_scheduler_step_loop(hip_lib):
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    sch = EulerAncestralDiscreteScheduler.from_config(EulerDiscreteScheduler().config)
    n, ns = 10, 2
    for run in range(2):                                   # a second run on the same object draws new seeds
        sch.set_timesteps(n, device=DEV)
        assert sch.noise_seeds is None
        gen = torch.Generator().manual_seed(31 + run)
        seeds = torch.randint(0, 2 ** 63 - 1, (ns,), generator=torch.Generator().manual_seed(31 + run)).tolist()
        orc = EulerAncestralOracle(seeds=seeds).set_timesteps(n)
        g = torch.Generator().manual_seed(32)
        x = (torch.randn(ns, 4, 8, 8, generator=g) * sch.init_noise_sigma).half().to(DEV)
        for i, t in enumerate(sch.timesteps):
            xin = sch.scale_model_input(x, t)
            _close(xin, hq(orc.scale_model_input(x.float().cpu(), i)), what=f"scale_model_input {i}")
            e = (torch.randn(ns, 4, 8, 8, generator=g) * 0.5).half()
            x_prev = x.float().cpu()
            out = sch.step(e.to(DEV), t, x, generator=gen, return_dict=(i % 2 == 0))
            x = out["prev_sample"] if i % 2 == 0 else out[0]
            _close(x, hq(orc.step(e.float(), i, x_prev)), what=f"scheduler.step run {run} step {i}")
        assert sch._step_index == n and sch.noise_seeds == seeds


# ---------------------------------------------------------------- 11-13. the whole pipeline
def _euler_a():
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    return EulerAncestralDiscreteScheduler.from_config(EulerDiscreteScheduler().config)


def _kwargs(parts, steps, **kw):
    return dict(dict(prompt="a manga panel", height=128, width=128, num_inference_steps=steps, guidance_scale=7.5,
                     num_samples=2, ip_images=list(parts["imgs"]), ip_bbox=[list(b) for b in IP_BBOX], ip_scale=0.6,
                     dialog_bbox=[list(b) for b in DIALOG], latents=parts["lat0"].clone(), prompt_embeds=parts["pe"],
                     pooled_prompt_embeds=parts["pooled"]), **kw)


def _call(pipe, parts, steps, **kw):
    return pipe(output_type="latent", **_kwargs(parts, steps, **kw)).images.clone()


def test_pipeline_euler_a_vs_oracle(parts):
    from PIL import Image
    from oracle.pipeline_ref import sample_loop
    from oracle.resampler_ref import resampler_forward
    from oracle.unet_ref import UNetOracle
    pipe = _pipe(parts, _euler_a())
    steps, ns, size = 5, 2, 128
    gen = lambda s: torch.Generator().manual_seed(s)
    results = []
    for use_graph in (False, True):
        pipe.use_graph = use_graph
        results.append(_call(pipe, parts, steps, generator=gen(9)))
        assert pipe.last_run_info["graph"] == use_graph
        # the documented derivation: the initial latents are given, so the generator's first draw is the seeds
        seeds = torch.randint(0, 2 ** 63 - 1, (ns,), generator=gen(9)).tolist()
        assert pipe.last_run_info["noise_seeds"] == seeds
    assert torch.equal(results[0], results[1])                                  # eager == hipGraph, same seeds
    assert torch.equal(_call(pipe, parts, steps, generator=gen(9)), results[0])  # same generator seed: same panel
    other = _call(pipe, parts, steps, generator=gen(10))
    assert torch.isfinite(other).all() and not torch.equal(other, results[0])
    assert torch.equal(_call(pipe, parts, steps, noise_seeds=seeds), results[0])  # explicit seeds override the draw
    # without `latents=`: randn for the initial latents first, then the seeds, from the same generator
    g = gen(12)
    torch.randn(ns, 4, size // 8, size // 8, generator=g, dtype=torch.float16)
    kw = _kwargs(parts, 2, generator=gen(12))
    del kw["latents"]
    pipe(output_type="latent", **kw)
    assert pipe.last_run_info["noise_seeds"] == torch.randint(0, 2 ** 63 - 1, (ns,), generator=g).tolist()
    # oracle pipeline, as in tests/test_gpu_dpm.py::test_pipeline_dpm_karras_vs_oracle, with the Euler a restatement
    clip, mae, rs, cfg, pe, pooled = parts["clip"], parts["mae"], parts["rs"], parts["cfg"], parts["pe"], parts["pooled"]
    imgs = parts["imgs"]
    clip_px = pipe._processors()[0](images=imgs + [Image.new("RGB", (224, 224))] * 2, return_tensors="pt").pixel_values
    magi_px = pipe._processors()[1](images=imgs + [Image.new("RGB", (224, 224))] * 2, return_tensors="pt").pixel_values
    with torch.no_grad():
        ce = clip(clip_px, output_hidden_states=True).hidden_states[-2].unsqueeze(0)
        me = mae(magi_px).last_hidden_state[:, 0].unsqueeze(0)
        ce[0, 2:], me[0, 2:] = 0, 0
        rsd = {k: v.float().cpu() for k, v in rs.state_dict().items()}
        img = resampler_forward(rsd, ce, me, 2, 64)
        neg = resampler_forward(rsd, torch.zeros_like(ce), torch.zeros_like(me), 2, 64)
        enc = torch.cat([torch.cat([torch.zeros_like(pe.float()).repeat(ns, 1, 1), pe.float().repeat(ns, 1, 1)]),
                         torch.cat([neg.repeat(ns, 1, 1), img.repeat(ns, 1, 1)])], dim=1)
        te = torch.cat([torch.zeros(ns, pooled.shape[1]), pooled.float().repeat(ns, 1)])
        tid = torch.tensor([[size, size, 0, 0, size, size]] * (2 * ns), dtype=torch.float32)
        bbox = torch.zeros(2 * ns, 4, 4)
        bbox[ns:, 0], bbox[ns:, 1] = torch.tensor(IP_BBOX[0]), torch.tensor(IP_BBOX[1])
        db = torch.zeros(2 * ns, 8, 4, dtype=torch.float16)
        db[ns:, 0], db[ns:, 1] = torch.tensor(DIALOG[0]).half(), torch.tensor(DIALOG[1]).half()
        orc = EulerAncestralOracle(seeds=seeds).set_timesteps(steps)
        ref = sample_loop(UNetOracle(cfg, parts["sd"], q=hq), orc, hq(parts["lat0"].float() * orc.init_noise_sigma),
                          hq(enc), hq(te), tid, bbox, db, 7.5, steps, 0.6, q=hq)
    # measured 3.8e-3 (5 Euler a steps at guidance 7.5; the DPM and Euler pipeline tests measure 3.6e-3 / 3.7e-3), so
    # 3x the measurement is above the 1.0e-2 those tests hold: that figure is the gate
    gate("test_gpu_euler_ancestral:2 " + '_rel(results[0], ref)', _rel(results[0], ref), 1.0e-2)


def test_request_alone_vs_inside_a_batch(parts):
    """The same request alone and between two other requests in one `generate_batch`: its noise is the same (its own
    seeds), so its latents differ only by what the batch-size-dependent kernel choice rounds differently - the figure
    plain Euler shows on the same requests.  A noise stream that depended on the batch position would be off by ~1."""
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    steps = 5
    g = torch.Generator().manual_seed(21)
    lat = lambda n: torch.randn(n, 4, 16, 16, generator=g).half()
    mine = lambda: _kwargs(parts, steps, generator=torch.Generator().manual_seed(3))
    before = lambda: _kwargs(parts, steps, num_samples=1, latents=lat(1), generator=torch.Generator().manual_seed(4),
                             prompt_embeds=parts["pe"] * 0.5)
    after = lambda: _kwargs(parts, steps, num_samples=1, latents=lat(1), generator=torch.Generator().manual_seed(5),
                            ip_scale=0.6, dialog_bbox=[])
    figures = {}
    for name, sch in (("euler", EulerDiscreteScheduler()), ("euler_a", _euler_a())):
        pipe = _pipe(parts, sch)
        alone = pipe(output_type="latent", **mine()).images.clone()
        seeds_alone = pipe.last_run_info["noise_seeds"]
        out = pipe.generate_batch([before(), mine(), after()], output_type="latent")
        assert [o.shape[0] for o in out] == [1, 2, 1]
        if name == "euler_a":
            assert pipe.last_run_info["noise_seeds"][1:3] == seeds_alone and len(pipe.last_run_info["noise_seeds"]) == 4
        else:
            assert seeds_alone is None and pipe.last_run_info["noise_seeds"] is None
        figures[name] = _rel(out[1], alone)
        print(f"[alone vs in batch] {name}: rel-L2 {figures[name]:.4g}")
    # measured 0 / 0: at this tiny shape the plans of UNet batch 4 and 8 pick the same kernels, so the panels are equal
    # bit for bit under both samplers; at shapes where the plans differ, Euler's own figure is the yardstick
    gate("test_gpu_euler_ancestral:3 euler alone-vs-batch rel-L2", figures["euler"], 1.0e-2)
    gate("test_gpu_euler_ancestral:4 euler_a alone-vs-batch rel-L2 (<= 2x euler's)", figures["euler_a"],
         2 * figures["euler"])


def test_pipeline_scheduler_swaps_leave_no_state(parts):
    """Euler -> Euler a -> DPM++ 2M -> Euler on one pipeline object (mirror of test_gpu_dpm's)."""
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    pipe = _pipe(parts, EulerDiscreteScheduler())
    e1 = _call(pipe, parts, 4)
    assert pipe.last_run_info["noise_seeds"] is None
    pipe.scheduler = _euler_a()
    a1 = _call(pipe, parts, 5, noise_seeds=[7, 8])
    a2 = _call(pipe, parts, 5, noise_seeds=[7, 8])
    a3 = _call(pipe, parts, 5, noise_seeds=[7, 9])         # the seed buffer is reloaded on every call
    assert pipe.last_run_info["noise_seeds"] == [7, 9]
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, use_karras_sigmas=True)
    d1 = _call(pipe, parts, 5)
    pipe.scheduler = EulerDiscreteScheduler.from_config(pipe.scheduler.config, use_karras_sigmas=False)
    e2 = _call(pipe, parts, 4)
    fresh_a = _call(_pipe(parts, _euler_a()), parts, 5, noise_seeds=[7, 8])
    fresh_d = _call(_pipe(parts, DPMSolverMultistepScheduler.from_config(EulerDiscreteScheduler().config,
                                                                         use_karras_sigmas=True)), parts, 5)
    assert torch.isfinite(a1).all() and not torch.equal(e1, a1) and not torch.equal(a1, d1)
    assert torch.equal(e1, e2)
    assert torch.equal(a1, a2) and torch.equal(a1, fresh_a)
    assert torch.equal(a1[0], a3[0]) and not torch.equal(a1[1], a3[1])     # panel 0 kept its seed, panel 1 did not
    assert torch.equal(d1, fresh_d)
    with pytest.raises(ValueError):
        _call(pipe, parts, 4, noise_seeds=[1, 2])          # Euler draws no noise
