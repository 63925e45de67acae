"""GPU: region redraw - `sampler_step_kernel<GV, RD = true>` and `redraw_start_kernel` against the torch restatement of
tests/_redraw_ref.py (exact where the mask is 1, 1 fp16 ulp where it is 0, the fp32 blend in between), the launch checks,
and the whole `DiffSenseiPipeline.__call__` / `generate_batch` (kept region exact, vs the oracle sampling loop, full
strength == the plain call for the four samplers, eager == graph, no stale state, DPM-Solver++ from mid-schedule).

Model-level gates: <= 3x the value measured on MI355X (logged by tests/_gates.gate)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _redraw_ref as R
from tests._dpm_ref import DPMSolverOracle
from tests._gates import gate
from tests._sampler_common import DEV, DIALOG, IP_BBOX, SDXL, _nhwc, _pipe, _rel, hq
from tests._sampler_common import parts  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
KINDS = {0: "euler", 1: "ddim", 2: "dpm", 3: "euler_a"}


def _scheduler(kind, **kw):
    from diffsensei_amd import schedulers as S
    cls = {0: S.EulerDiscreteScheduler, 1: S.DDIMScheduler, 2: S.DPMSolverMultistepScheduler,
           3: S.EulerAncestralDiscreteScheduler}[kind]
    return cls(**dict(SDXL, **kw))


def _masks(ns, H, W, which):
    """One mask per panel, cycling: a box, all ones, a soft ramp (values 0 and 1 included); or all zeros."""
    m = torch.zeros(ns, H, W)
    if which == "zeros":
        return m
    for n in range(ns):
        if n % 3 == 0:
            m[n] = R.mask_from_boxes([[0.25, 0.25, 0.8, 1.0]], H, W)
        elif n % 3 == 1:
            m[n] = 1.0
        else:
            m[n] = torch.linspace(0, 1, H * W).reshape(H, W).half().float()
    return m


def _sequence(kind, do_cfg, ns, H, W, which="mixed", n=5, per_panel=False, check_soft=True):
    """n redraw steps; after each, the same step through the existing non-redraw op from the SAME inputs (the redraw
    run's own previous latents and prev_x0).  Returns the worst soft-pixel error relative to max|ref|."""
    from diffsensei_amd import ops
    sch = _scheduler(kind)
    sch.set_timesteps(n)
    g = torch.Generator().manual_seed(11 * kind + int(do_cfg) + ns)
    gs = 5.0
    table = torch.from_numpy(sch.coef_table(gs)).to(DEV)
    solver = torch.from_numpy(sch.solver_table()).to(DEV) if kind == 2 else None
    seeds = torch.tensor([7919 * k + 5 for k in range(ns)], dtype=torch.int64, device=DEV) if kind == 3 else None
    guidance = torch.tensor([3.0 + 0.5 * k for k in range(ns)], device=DEV) if per_panel else None
    rows = sch.renoise_table()
    x0 = torch.randn(ns, 4, H, W, generator=g).half()
    noise = torch.randn(ns, 4, H, W, generator=g).half()
    mask = _masks(ns, H, W, which)
    buf = ops.redraw_buffer(ns, H, W, DEV)
    ops.redraw_load(buf, x0, noise, mask, torch.from_numpy(rows))
    lat = torch.empty(ns, 4, H, W, dtype=torch.float16, device=DEV)
    ops.redraw_start(buf, lat)
    assert int(R.ulp16(lat, R.known(x0, noise, *rows[0])).max()) <= 1
    prev = torch.zeros_like(lat) if kind == 2 else None
    B = 2 * ns if do_cfg else ns
    xin = torch.empty(B, H * W, 4, dtype=torch.float16, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    m4 = mask[:, None].expand(ns, 4, H, W)
    one, zero, soft = m4 == 1, m4 == 0, (m4 > 0) & (m4 < 1)
    worst = 0.0
    for i in range(n):
        eps = _nhwc((torch.randn(B, 4, H, W, generator=g) * 0.5).half()).to(DEV)
        ctr.fill_(i)
        lat_p, prev_p, xin_p = lat.clone(), None if prev is None else prev.clone(), torch.empty_like(xin)
        if kind == 2:
            ops.cfg_dpm_step(eps, lat_p, xin_p, table, solver, prev_p, do_cfg, ctr, guidance=guidance)
        elif kind == 3:
            ops.cfg_sampler_step_noise(eps, lat_p, xin_p, table, seeds, 3, do_cfg, ctr, guidance=guidance)
        else:
            ops.cfg_sampler_step(eps, lat_p, xin_p, table, kind, do_cfg, ctr, guidance=guidance)
        ops.cfg_sampler_step_redraw(eps, lat, xin, table, buf, kind, do_cfg, ctr, guidance=guidance, solver=solver,
                                    prev_x0=prev, seeds=seeds)
        what = f"{KINDS[kind]} cfg={do_cfg} step {i}"
        got, plain = lat.cpu(), lat_p.cpu()
        assert torch.isfinite(got.float()).all(), what
        unhwc = lambda t: t.view(B, H, W, 4).permute(0, 3, 1, 2).cpu()
        xi, xi_p = unhwc(xin), unhwc(xin_p)
        # m == 1: the bits of the non-redraw kernel - latents, model_in (both CFG halves), prev_x0 (everywhere: the
        # blend does not touch it)
        assert torch.equal(got[one], plain[one]), what
        assert torch.equal(xi[:ns][one], xi_p[:ns][one]), what
        if do_cfg:
            assert torch.equal(xi[ns:], xi[:ns]), what
        if kind == 2:
            assert torch.equal(prev.cpu(), prev_p.cpu()), what
        # m == 0: the kept latents at the next state's noise level, one contraction away from the fp32 restatement
        kn = R.known(x0, noise, *rows[i + 1])
        assert int(R.ulp16(got, kn)[zero].max() if zero.any() else 0) <= 1, what
        # model_in is formed from the blended value
        div = float(table[i, 6])
        assert int(R.ulp16(xi[:ns], (got.float() / div).half()).max()) <= 1, what      # x * (1 / div) or x / div
        if check_soft and soft.any():
            ref = R.blend(plain.float(), x0, noise, mask, *rows[i + 1])
            worst = max(worst, float((got.float() - ref)[soft].abs().max() / ref[soft].abs().max()))
    # the last renoise row is {1, 0}: the kept region is the kept latents, bit for bit
    if zero.any():
        assert torch.equal(lat.cpu()[zero], x0[zero])
    torch.cuda.synchronize()
    return worst


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("do_cfg", [True, False])
def test_redraw_kernel_sequence(hip_lib, kind, do_cfg):
    worst = _sequence(kind, do_cfg, 3, 8, 12)
    # soft pixels vs the fp32 restatement, max |err| / max |ref|: the restatement's `known` is computed without the kernel's
    # fma contraction, so a pixel can sit 1 fp16 ulp away.  Measured 0 for seven of the eight cases and 7.9e-6 (one ulp of
    # one small value) for DPM-Solver++ without CFG
    gate(f"test_gpu_redraw:1 soft-mask blend, {KINDS[kind]} cfg={do_cfg}", worst, 2.0e-5)


@pytest.mark.parametrize("kind", [0, 2])
def test_redraw_kernel_all_zeros_mask(hip_lib, kind):
    """Nothing is repainted: every state is the kept latents at that state's noise level, whatever eps says."""
    _sequence(kind, True, 3, 8, 12, which="zeros")


def test_redraw_kernel_per_panel_guidance(hip_lib):
    """The GV instantiation of the redraw kernel (<true, true>): one guidance scale per panel."""
    _sequence(0, True, 3, 8, 12, per_panel=True)
    _sequence(3, True, 3, 8, 12, per_panel=True)


def test_redraw_kernel_batch64_shape(hip_lib):
    """UNet batch 64 at 1024^2: ns 32 panels of 128 x 128 latents, CFG on; finiteness and the two exactness properties."""
    _sequence(0, True, 32, 128, 128, n=2, check_soft=False)


def test_redraw_start(hip_lib):
    from diffsensei_amd import ops
    ns, H, W = 3, 8, 12
    g = torch.Generator().manual_seed(3)
    x0, noise = torch.randn(ns, 4, H, W, generator=g).half(), torch.randn(ns, 4, H, W, generator=g).half()
    sch = _scheduler(0)
    sch.set_timesteps(10)
    rows = sch.renoise_table()[4:]
    buf = ops.redraw_buffer(ns, H, W, DEV)
    lat = torch.zeros(ns, 4, H, W, dtype=torch.float16, device=DEV)
    ops.redraw_load(buf, x0, noise, torch.ones(ns, H, W), torch.from_numpy(rows), False, sch.init_noise_sigma)
    ops.redraw_start(buf, lat)
    assert int(R.ulp16(lat, R.known(x0, noise, *rows[0])).max()) <= 1       # strength < 1: one contraction
    assert not torch.equal(lat.cpu(), x0)
    ops.redraw_load(buf, x0, noise, torch.ones(ns, H, W), torch.from_numpy(rows), True, sch.init_noise_sigma)
    ops.redraw_start(buf, lat)
    assert torch.equal(lat, noise.to(DEV).half() * sch.init_noise_sigma)    # full strength: `prepare_latents`' product
    ops.redraw_load(buf, x0, noise, torch.ones(ns, H, W), torch.tensor([[1.0, 0.0], [1.0, 0.0]]), False)
    ops.redraw_start(buf, lat)
    assert torch.equal(lat.cpu(), x0)


def test_redraw_launch_checks(hip_lib):
    """A refused launch returns an error code and launches nothing: the latents keep their bits."""
    from diffsensei_amd import _lib, ops
    from diffsensei_amd.engine import make_op
    ns, H, W = 1, 4, 4
    lat = torch.full((ns, 4, H, W), 3.0, dtype=torch.float16, device=DEV)
    xin = torch.zeros(ns, H * W, 4, dtype=torch.float16, device=DEV)
    eps = torch.ones_like(xin)
    table = torch.ones(1, 8, device=DEV)
    with pytest.raises(_lib.DiffSenseiHipError, match="redraw"):
        ops.cfg_sampler_step_redraw(eps, lat, xin, table, None, 0, do_cfg=False)         # the flag without the buffer
    op = make_op("SAMPLER_STEP", i=(ns, H * W, 0, 0, 1), p=(eps, lat, xin, table, None, None, None, None, None, None))
    assert hip_lib.ds_op_run(ctypes.byref(op), None) != 0
    assert b"redraw" in hip_lib.ds_last_error()
    assert hip_lib.ds_redraw_start_f16(None, lat.data_ptr(), ns, H * W, None) != 0
    buf = ops.redraw_buffer(ns, H, W, DEV)
    x0 = torch.zeros(ns, 4, H, W)
    rows = torch.tensor([[1.0, 1.0], [1.0, 0.0]])
    for bad in (1.5, -0.25, float("nan")):                                               # the mask range, host-side
        m = torch.ones(ns, H, W)
        m[0, 1, 2] = bad
        with pytest.raises(_lib.DiffSenseiHipError, match="mask"):
            ops.redraw_load(buf, x0, x0, m, rows)
    with pytest.raises(ValueError):
        ops.redraw_load(buf, x0, x0, torch.ones(ns, H, W + 1), rows)
    with pytest.raises(ValueError):
        ops.redraw_load(buf, x0, x0, torch.ones(ns, H, W), torch.ones(ops.REDRAW_MAX_ROWS + 1, 2))
    with pytest.raises(_lib.DiffSenseiHipError):                                         # a buffer of another shape
        ops.cfg_sampler_step_redraw(eps, lat, xin, table, ops.redraw_buffer(2, H, W, DEV), 0, do_cfg=False)
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and bool((lat == 3.0).all()) and bool((xin == 0).all())
    # a flag of 0 ignores p[9]: the plain kernel
    op = make_op("SAMPLER_STEP", i=(ns, H * W, 0, 0, 0), p=(eps, lat, xin, table, None, None, None, None, None, buf))
    assert hip_lib.ds_op_run(ctypes.byref(op), None) == 0
    torch.cuda.synchronize()
    assert hip_lib.ds_version() >= 104


# ---------------------------------------------------------------- the whole pipeline
def _kwargs(parts, steps, **kw):
    return dict(dict(prompt="a manga panel", height=128, width=128, num_inference_steps=steps, guidance_scale=7.5,
                     num_samples=2, ip_images=list(parts["imgs"]), ip_bbox=[list(b) for b in IP_BBOX], ip_scale=0.6,
                     dialog_bbox=[list(b) for b in DIALOG], latents=parts["lat0"].clone(), prompt_embeds=parts["pe"],
                     pooled_prompt_embeds=parts["pooled"]), **kw)


def _call(pipe, parts, steps, **kw):
    return pipe(output_type="latent", **_kwargs(parts, steps, **kw)).images.clone()


def _euler():
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    return EulerDiscreteScheduler()


def _dpm():
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(_euler().config)


RIGHT = [[0.5, 0, 1, 1]]
NOISE_SEED = 41


def _noise():
    return torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(NOISE_SEED)).half()


@pytest.fixture(scope="module")
def base(parts):
    """Call A: the panels that the redraws keep.  Computed once, never written."""
    return _call(_pipe(parts, _euler()), parts, 10).cpu()


@pytest.fixture(scope="module")
def oracle_inputs(parts):
    """The oracle UNet and its CFG-concatenated conditioning for `_kwargs` (as tests/test_gpu_euler_ancestral.py)."""
    from PIL import Image
    from oracle.resampler_ref import resampler_forward
    from oracle.unet_ref import UNetOracle
    from transformers import CLIPImageProcessor, ViTImageProcessor
    clip, mae, rs, cfg, pe, pooled = parts["clip"], parts["mae"], parts["rs"], parts["cfg"], parts["pe"], parts["pooled"]
    imgs, ns, size = parts["imgs"], 2, 128
    black = [Image.new("RGB", (224, 224))] * 2
    clip_px = CLIPImageProcessor()(images=imgs + black, return_tensors="pt").pixel_values
    magi_px = ViTImageProcessor()(images=imgs + black, return_tensors="pt").pixel_values
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
    return dict(unet=UNetOracle(cfg, parts["sd"], q=hq), args=(hq(enc), hq(te), tid, bbox, db))


def _oracle_run(oracle_inputs, wrapped, steps_run):
    from oracle.pipeline_ref import sample_loop
    with torch.no_grad():
        return sample_loop(oracle_inputs["unet"], wrapped, wrapped.start_latents(), *oracle_inputs["args"], 7.5,
                           steps_run, 0.6, q=hq)


def test_pipeline_redraw_box_vs_oracle(parts, base, oracle_inputs):
    from oracle.scheduler_ref import EulerDiscreteOracle
    pipe = _pipe(parts, _euler())
    steps, strength = 10, 0.6
    seen = []
    out = _call(pipe, parts, steps, latents=_noise(), redraw_latents=base, redraw_bbox=RIGHT, strength=strength,
                callback_on_step_end=lambda p, i, t, kw: seen.append((i, float(t)))).cpu()
    info = pipe.last_run_info["redraw"]
    assert info == {"t_start": 4, "steps_run": 6, "repaint_fraction": 0.5}
    ts = pipe.scheduler.timesteps.cpu().tolist()
    assert seen == [(i, ts[4 + i]) for i in range(6)]                 # run-relative index, true timestep
    assert torch.isfinite(out).all()
    assert torch.equal(out[..., :8], base[..., :8])                   # the kept half: bit for bit
    assert not torch.equal(out[..., 8:], base[..., 8:])               # the repainted half: drawn again
    assert (out[..., 8:] - base[..., 8:]).abs().mean() > 0.05
    _call(pipe, parts, 2)
    assert "redraw" not in pipe.last_run_info                         # only on redraw calls
    # the oracle sampling loop under a wrapper scheduler that offsets the step index and applies the blend
    inner = EulerDiscreteOracle().set_timesteps(steps)
    mask = R.mask_from_boxes(RIGHT, 16, 16)[None].expand(2, 16, 16)
    rows = R.renoise_rows("sigma", inner.timesteps, inner.sigmas)
    ref = _oracle_run(oracle_inputs, R.RedrawOracle(inner, steps, 4, base, _noise(), mask, rows), 6)
    assert torch.equal(ref[..., :8], base[..., :8].float())
    # measured 3.95e-4 over the panel and 5.34e-4 over the repainted half (the last 6 of 10 Euler steps at guidance 7.5);
    # both gates are far inside the 1.0e-2 of test_gpu_euler_ancestral.py::test_pipeline_euler_a_vs_oracle at this size
    gate("test_gpu_redraw:2 _rel(out, ref)", _rel(out, ref), 1.2e-3)
    gate("test_gpu_redraw:3 _rel(out[repainted], ref[repainted])", _rel(out[..., 8:], ref[..., 8:]), 1.6e-3)


def test_pipeline_full_strength_all_ones_is_the_plain_call(parts, base):
    """strength 1, everything repainted, `latents=noise`: the plain call with the same `latents`, bit for bit, for each
    of the four samplers (Euler Ancestral: the same seeds from the same generator)."""
    from diffsensei_amd.schedulers import DDIMScheduler, EulerAncestralDiscreteScheduler
    cfgd = _euler().config
    for sch in (_euler(), DDIMScheduler(), _dpm(), EulerAncestralDiscreteScheduler.from_config(cfgd)):
        pipe = _pipe(parts, sch)
        gen = lambda: torch.Generator().manual_seed(9)
        plain = _call(pipe, parts, 4, latents=_noise(), generator=gen())
        seeds = pipe.last_run_info["noise_seeds"]
        rd = _call(pipe, parts, 4, latents=_noise(), generator=gen(), redraw_latents=base[:1],
                   redraw_mask=torch.ones(16, 16), strength=1.0)
        assert pipe.last_run_info["noise_seeds"] == seeds
        assert pipe.last_run_info["redraw"] == {"t_start": 0, "steps_run": 4, "repaint_fraction": 1.0}
        assert torch.equal(rd, plain), type(sch).__name__
        assert torch.equal(_call(pipe, parts, 4, latents=_noise(), generator=gen()), plain)   # and back: nothing stale


def test_pipeline_graph_equals_eager_and_no_stale_state(parts, base):
    kw1 = dict(latents=_noise(), redraw_latents=base, redraw_bbox=RIGHT, strength=0.6)
    soft = torch.linspace(-0.5, 1, 256).clamp(0, 1).reshape(16, 16)           # zeros, a ramp, a one
    kw2 = dict(latents=_noise() * 0.5, redraw_latents=base[1:], redraw_mask=torch.stack([soft, soft.t()]),
               redraw_bbox=[[0.75, 0.75, 1, 1]], strength=0.3)
    outs = {}
    for use_graph in (False, True):
        pipe = _pipe(parts, _euler())
        pipe.use_graph = use_graph
        a = _call(pipe, parts, 10, **kw1)
        assert pipe.last_run_info["graph"] == use_graph and pipe.last_run_info["redraw"]["steps_run"] == 6
        b = _call(pipe, parts, 10, **kw2)            # another mask, another x0, fewer steps, on the same engine
        assert pipe.last_run_info["redraw"]["steps_run"] == 3 and pipe.last_run_info["redraw"]["t_start"] == 7
        plain = _call(pipe, parts, 10)               # a plain sampler afterwards sees nothing of it
        outs[use_graph] = (a, b, plain)
    for x, y in zip(outs[False], outs[True]):
        assert torch.equal(x, y)                                                  # eager == hipGraph
    fresh = _pipe(parts, _euler())
    assert torch.equal(_call(fresh, parts, 10, **kw2), outs[True][1])             # second redraw == a fresh pipeline's
    assert torch.equal(outs[True][2].cpu(), base)                                 # plain after redraw == call A
    # kept exactly where the combined mask is 0; one row of `redraw_latents` serves both panels
    m = torch.maximum(torch.stack([soft, soft.t()]), R.mask_from_boxes([[0.75, 0.75, 1, 1]], 16, 16)[None])
    zero = (m == 0)[:, None].expand(2, 4, 16, 16)
    assert zero.any() and torch.equal(outs[True][1].cpu()[zero], base[1:].repeat(2, 1, 1, 1)[zero])


def test_generate_batch_redraws_vs_each_alone(parts, base):
    pipe = _pipe(parts, _euler())
    r1 = _kwargs(parts, 10, latents=_noise(), redraw_latents=base, redraw_bbox=RIGHT, strength=0.6)
    r2 = _kwargs(parts, 10, num_samples=1, latents=_noise()[:1] * 0.7, redraw_latents=base[1:],
                 redraw_bbox=[[0, 0.5, 1, 1]], strength=0.6, prompt_embeds=parts["pe"] * 0.5)
    alone = [pipe(output_type="latent", **dict(r)).images.clone().cpu() for r in (r1, r2)]
    out = [o.cpu() for o in pipe.generate_batch([dict(r1), dict(r2)], output_type="latent")]
    assert [o.shape[0] for o in out] == [2, 1]
    assert pipe.last_run_info["redraw"] == {"t_start": 4, "steps_run": 6, "repaint_fraction": 0.5}
    assert torch.equal(out[0][..., :8], base[..., :8]) and torch.equal(alone[0][..., :8], base[..., :8])
    assert torch.equal(out[1][:, :, :8], base[1:, :, :8]) and torch.equal(alone[1][:, :, :8], base[1:, :, :8])
    assert not torch.equal(out[1][:, :, 8:], base[1:, :, 8:])
    # repainted regions: the figure test_gpu_euler_ancestral.py::test_request_alone_vs_inside_a_batch holds for Euler
    # (measured 0 / 0 here as there: at this tiny shape UNet batches 4 and 6 pick the same kernels)
    gate("test_gpu_redraw:4 request 1 alone-vs-batch rel-L2", _rel(out[0][..., 8:], alone[0][..., 8:]), 1.0e-2)
    gate("test_gpu_redraw:5 request 2 alone-vs-batch rel-L2", _rel(out[1][:, :, 8:], alone[1][:, :, 8:]), 1.0e-2)
    with pytest.raises(ValueError):
        pipe.generate_batch([dict(r1), _kwargs(parts, 10)], output_type="latent")
    with pytest.raises(ValueError):
        pipe.generate_batch([dict(r1), dict(r2, strength=0.3)], output_type="latent")


def test_pipeline_dpm_from_mid_schedule_vs_oracle(parts, base, oracle_inputs):
    pipe = _pipe(parts, _dpm())
    steps = 10
    out = _call(pipe, parts, steps, latents=_noise(), redraw_latents=base, redraw_bbox=RIGHT, strength=0.5).cpu()
    assert pipe.last_run_info["redraw"] == {"t_start": 5, "steps_run": 5, "repaint_fraction": 0.5}
    assert torch.equal(out[..., :8], base[..., :8]) and not torch.equal(out[..., 8:], base[..., 8:])
    inner = DPMSolverOracle().set_timesteps(steps)
    mask = R.mask_from_boxes(RIGHT, 16, 16)[None].expand(2, 16, 16)
    rows = R.renoise_rows("dpm", inner.timesteps, inner.sigmas)
    ref = _oracle_run(oracle_inputs, R.RedrawOracle(inner, steps, 5, base, _noise(), mask, rows, first_order_at_start=True), 5)
    # measured 4.60e-4 over the panel and 6.25e-4 over the repainted half (the last 5 of 10 DPM-Solver++ steps); the DPM
    # pipeline test of tests/test_gpu_dpm.py holds 1.0e-2 at this size
    gate("test_gpu_redraw:6 dpm _rel(out, ref)", _rel(out, ref), 1.3e-3)
    gate("test_gpu_redraw:7 dpm _rel(out[repainted], ref[repainted])", _rel(out[..., 8:], ref[..., 8:]), 1.8e-3)


def test_decode_latents_is_postprocess(parts, base):
    pipe = _pipe(parts, _euler())
    x = base.to(DEV)
    assert pipe.decode_latents(x, output_type="latent") is pipe._postprocess(x, "latent")

    class Vae:                                   # any object with the `decode` protocol is used as is
        config = None

        def decode(self, z, return_dict=False):
            return (z[:, :3].repeat_interleave(2, 2).repeat_interleave(2, 3).tanh(),)
    pipe.vae = Vae()
    for ot in ("pt", "np"):
        a, b = pipe.decode_latents(x, output_type=ot), pipe._postprocess(x, ot)
        assert (torch.equal(a, b) if ot == "pt" else np.array_equal(a, b)) and a.shape[0] == 2
    a, b = pipe.decode_latents(x), pipe._postprocess(x, "pil")
    assert len(a) == 2 and all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b))
