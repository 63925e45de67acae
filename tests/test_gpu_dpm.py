"""GPU: DPM-Solver++ (DPMSolverMultistepScheduler, kind 2 of sampler_step_kernel) against the test restatement
tests/_dpm_ref.py - whole n-step sequences through `ds_cfg_dpm_step_f16`, the stand-alone `scheduler.step` loop, and the
whole `DiffSenseiPipeline.__call__` (eager == graph, vs the oracle sampling loop, scheduler swaps on one pipeline).

Kernel tolerance: the 1.5e-3 of test_gpu_ops.py::test_cfg_sampler_step per step.  Pipeline gate: <= 3x the value measured
on MI355X (logged by tests/_gates.gate)."""
import itertools

import pytest
import torch

from tests._dpm_ref import DPMSolverOracle
from tests._gates import gate
from tests._sampler_common import DEV, DIALOG, IP_BBOX, SDXL, _close, _nhwc, _pipe, _rel, hq
from tests._sampler_common import parts  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _sequence(ns, H, W, n, do_cfg, seed, prev_fill=0.0, check=True, **kw):
    """n steps of ds_cfg_dpm_step_f16 with the device step counter, each checked against the restatement; returns the
    final latents.  Each restatement step starts from the kernel's latents (its previous x0 is its own): one rounding
    flip of an fp32 intermediate is one fp16 ulp, and two free-running sequences would compound those flips."""
    from diffsensei_amd import ops
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler
    sch = DPMSolverMultistepScheduler(**dict(SDXL, **kw))
    sch.set_timesteps(n)
    orc = DPMSolverOracle(**kw).set_timesteps(n)
    g = torch.Generator().manual_seed(seed)
    gs = 5.0
    table = torch.from_numpy(sch.coef_table(gs)).to(DEV)
    solver = torch.from_numpy(sch.solver_table()).to(DEV)
    lat = torch.randn(ns, 4, H, W, generator=g).half()
    lat_d = lat.to(DEV)
    prev = torch.full_like(lat_d, prev_fill)
    rows = 2 * ns if do_cfg else ns
    xin = torch.empty(rows, H * W, 4, dtype=torch.float16, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for i in range(n):
        eps = (torch.randn(rows, 4, H, W, generator=g) * 0.5).half()
        x_in = lat_d.float().cpu()
        ctr.fill_(i)
        ops.cfg_dpm_step(_nhwc(eps).to(DEV), lat_d, xin, table, solver, prev, do_cfg, ctr)
        if not check:
            continue
        if do_cfg:
            u, c = eps.float().chunk(2)
            e = hq(u + hq(gs * hq(c - u)))
        else:
            e = eps.float()
        x_ref = orc.step(e, i, x_in)
        _close(lat_d, x_ref, what=f"{kw} cfg={do_cfg} n={n} step {i} (order {orc.orders[i]})")
        got = xin.view(rows, H, W, 4).permute(0, 3, 1, 2)
        assert torch.equal(got[:ns], lat_d), "model_in != new latents"
        if do_cfg:
            assert torch.equal(got[ns:], lat_d), "model_in (cond half) != new latents"
    torch.cuda.synchronize()
    return lat_d


@pytest.mark.parametrize("n,do_cfg,solver_type,order,karras",
                         list(itertools.product((5, 14, 15, 25), (True, False), ("midpoint", "heun"), (1, 2),
                                                (False, True))))
def test_dpm_kernel_sequence_vs_restatement(hip_lib, n, do_cfg, solver_type, order, karras):
    _sequence(2, 8, 12, n, do_cfg, seed=n * 7 + order, solver_type=solver_type, solver_order=order,
              use_karras_sigmas=karras)


def test_dpm_kernel_sequence_batch64_shape(hip_lib):
    """UNet batch 64 at 1024^2: ns 32 samples of 128 x 128 latents, CFG on."""
    _sequence(32, 128, 128, 6, True, seed=3, use_karras_sigmas=True)


def test_dpm_kernel_sigma_min_and_trailing(hip_lib):
    _sequence(2, 8, 12, 16, True, seed=11, final_sigmas_type="sigma_min", timestep_spacing="trailing",
              lower_order_final=False)
    _sequence(2, 8, 12, 20, False, seed=12, timestep_spacing="linspace", steps_offset=0, euler_at_final=True)


def test_dpm_first_step_ignores_prev_x0(hip_lib):
    """prev_x0 holds garbage (or the previous request's x0) before step 0: order-1 rows must not read it."""
    a = _sequence(2, 8, 12, 5, True, seed=21, prev_fill=float("nan"), check=False, use_karras_sigmas=True)
    b = _sequence(2, 8, 12, 5, True, seed=21, prev_fill=0.0, check=False, use_karras_sigmas=True)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_dpm_kernel_launch_checks(hip_lib):
    from diffsensei_amd import _lib, ops
    lat = torch.zeros(1, 4, 4, 4, dtype=torch.float16, device=DEV)
    xin = torch.empty(1, 16, 4, dtype=torch.float16, device=DEV)
    eps = torch.zeros_like(xin)
    table = torch.zeros(1, 8, device=DEV)
    with pytest.raises(_lib.DiffSenseiHipError):          # kind 2 without prev_x0 / solver rows
        ops.cfg_sampler_step(eps, lat, xin, table, 2, do_cfg=False)
    with pytest.raises(_lib.DiffSenseiHipError):
        ops.cfg_sampler_step(eps, lat, xin, table, 3, do_cfg=False)
    assert hip_lib.ds_version() >= 101


def test_standalone_scheduler_step_loop(hip_lib):
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    g = torch.Generator().manual_seed(31)
    for solver_type in ("midpoint", "heun"):
        sch = DPMSolverMultistepScheduler.from_config(EulerDiscreteScheduler().config, use_karras_sigmas=True,
                                                      solver_type=solver_type)
        n = 10
        sch.set_timesteps(n, device=DEV)
        orc = DPMSolverOracle(use_karras_sigmas=True, solver_type=solver_type).set_timesteps(n)
        x = (torch.randn(2, 4, 8, 8, generator=g) * sch.init_noise_sigma).half().to(DEV)
        x_ref = x.float().cpu()
        for i, t in enumerate(sch.timesteps):
            xin = sch.scale_model_input(x, t)
            assert xin is x
            e = (torch.randn(2, 4, 8, 8, generator=g) * 0.5).half()
            out = sch.step(e.to(DEV), t, xin, return_dict=(i % 2 == 0))
            x = out["prev_sample"] if i % 2 == 0 else out[0]
            x_ref = orc.step(e.float(), i, x_ref)
            _close(x, x_ref, what=f"scheduler.step {solver_type} {i}")
        assert sch._step_index == n and sch.lower_order_nums == 2


# ---------------------------------------------------------------- the whole pipeline
def _call(pipe, parts, steps):
    return pipe(prompt="a manga panel", height=128, width=128, num_inference_steps=steps, guidance_scale=7.5,
                num_samples=2, ip_images=list(parts["imgs"]), ip_bbox=[list(b) for b in IP_BBOX], ip_scale=0.6,
                dialog_bbox=[list(b) for b in DIALOG], latents=parts["lat0"].clone(), prompt_embeds=parts["pe"],
                pooled_prompt_embeds=parts["pooled"], output_type="latent").images.clone()


def _dpm_karras():
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    return DPMSolverMultistepScheduler.from_config(EulerDiscreteScheduler().config, use_karras_sigmas=True)


def test_pipeline_dpm_karras_vs_oracle(parts):
    from PIL import Image
    from oracle.pipeline_ref import sample_loop
    from oracle.resampler_ref import resampler_forward
    from oracle.unet_ref import UNetOracle
    pipe = _pipe(parts, _dpm_karras())
    steps, ns, size = 5, 2, 128
    results = []
    for use_graph in (False, True):
        pipe.use_graph = use_graph
        results.append(_call(pipe, parts, steps))
        assert pipe.last_run_info["graph"] == use_graph
    assert torch.equal(results[0], results[1])
    # oracle pipeline, as in tests/test_gpu_pipeline.py::test_pipeline_call_vs_oracle, with the DPM restatement
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
        orc = DPMSolverOracle(use_karras_sigmas=True)
        ref = sample_loop(UNetOracle(cfg, parts["sd"], q=hq), orc, hq(parts["lat0"].float() * orc.init_noise_sigma),
                          hq(enc), hq(te), tid, bbox, db, 7.5, steps, 0.6, q=hq)
    # measured 3.6e-3 (5 DPM++ 2M steps at guidance 7.5; tests/test_gpu_pipeline.py measures 3.7e-3 after 3 Euler steps)
    gate("test_gpu_dpm:1 " + '_rel(results[0], ref)', _rel(results[0], ref), 1.0e-2)


def test_pipeline_scheduler_swaps_leave_no_state(parts):
    """Euler -> DPM++ 2M -> Euler on one pipeline object: the two Euler panels are identical and the DPM panel equals a
    fresh pipeline's (no stale step plan, no solver rows or previous x0 leaking between calls)."""
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    pipe = _pipe(parts, EulerDiscreteScheduler())
    e1 = _call(pipe, parts, 4)
    pipe.scheduler = _dpm_karras()
    d1 = _call(pipe, parts, 5)
    d2 = _call(pipe, parts, 5)                      # same engine, prev_x0 now holds the first call's x0
    pipe.scheduler = EulerDiscreteScheduler.from_config(pipe.scheduler.config, use_karras_sigmas=False)
    e2 = _call(pipe, parts, 4)
    fresh = _call(_pipe(parts, _dpm_karras()), parts, 5)
    assert torch.isfinite(d1).all() and not torch.equal(e1, d1)
    assert torch.equal(e1, e2)
    assert torch.equal(d1, d2) and torch.equal(d1, fresh)
