"""GPU: LCM sampling (kind 4 of `sampler_step_kernel`, csrc/elementwise.hip) against the float64 restatement of
tests/_lcm_ref.py fed the device generator's restated normals (tests/_philox_ref.py), and the whole pipeline with
`LCMScheduler`.

Kernel sequences: ns 2, 16 x 16 latents, n in {1, 2, 4, 8} steps, with and without CFG, with and without the region-redraw
blend; every step is checked against the restatement started from the kernel's own previous latents.  The figure is
max |got - ref| / max |ref| per step.  It cannot be derived (fp16 storage of the state, an fp16 noise tensor times an fp32
scalar, fp32 tables against float64 ones), so it is measured on the MI355X against the restatement and gated at no more than
3x the measurement; the pipeline figure likewise, against the oracle loop.  Both are logged by tests/_gates.gate.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests._gates import gate
from tests._lcm_ref import LCMOracle
from tests._sampler_common import DEV, DIALOG, IP_BBOX, _nhwc, _pipe, _rel, hq
from tests._sampler_common import parts  # noqa: F401  (the fixture)
from tests.test_gpu_per_panel_scales import _clone, pipe  # noqa: F401  (`pipe`: the fixture of the continuous-batching test)

pytestmark = pytest.mark.gpu
NS, H, W = 2, 16, 16
SEEDS = [0x0123456789ABCDEF, 2 ** 63 - 2]
# Measured on MI355X against the restatement / the oracle (profiles/lcm_measured_gates.jsonl), each gate <= 3x its measurement:
#   plain sequences 2.6e-4 .. 3.9e-4 (16 x 16, the largest entries a few units: about one fp16 rounding of the state),
#   redraw sequences 4.3e-4 .. 7.1e-4 (the blend adds the rounding of the re-noised kept latents),
#   the stand-alone scheduler.step loop 2.4e-4 / 4.5e-4, the 4-step pipeline 4.1e-3 (Euler a measures 3.8e-3 on 5 steps)
SEQUENCE_GATE = {False: 1.1e-3, True: 1.5e-3}     # by `redraw`
STANDALONE_GATE = 1.2e-3
PIPELINE_GATE = 1.0e-2


def _lcm(**kw):
    from diffsensei_amd.schedulers import LCMScheduler
    return LCMScheduler(**kw)


def _seeds_dev(seeds):
    return torch.tensor([int(s) for s in seeds], dtype=torch.int64, device=DEV)


def _cfg_combine(eps, gs, do_cfg):
    if not do_cfg:
        return eps.float()
    u, c = eps.float().chunk(2)
    return hq(u + hq(gs * hq(c - u)))


def _mask():
    m = torch.zeros(NS, H, W)
    m[0, 4:12, 2:10] = 1.0                                                    # a box: zeros and ones
    m[1] = torch.linspace(0, 1, H * W).reshape(H, W).half().float()           # a soft ramp, 0 and 1 included
    return m


def _sequence(n, do_cfg, redraw, seeds=SEEDS, seed=0):
    """n steps with the device step counter.  Returns (worst per-step figure, [latents after every step])."""
    from diffsensei_amd import ops
    sch = _lcm()
    sch.set_timesteps(n)
    orc = LCMOracle(seeds=seeds).set_timesteps(n)
    gs = 5.0
    table = torch.from_numpy(sch.coef_table(gs)).to(DEV)
    solver = torch.from_numpy(sch.solver_table()).to(DEV)
    g = torch.Generator().manual_seed(100 * n + 10 * int(do_cfg) + int(redraw) + seed)
    rows = 2 * NS if do_cfg else NS
    xin = torch.empty(rows, H * W, 4, dtype=torch.float16, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    seeds_d = _seeds_dev(seeds)
    if redraw:
        x0k, nz, mask = torch.randn(NS, 4, H, W, generator=g).half(), torch.randn(NS, 4, H, W, generator=g).half(), _mask()
        ren = sch.renoise_table()
        buf = ops.redraw_buffer(NS, H, W, DEV)
        ops.redraw_load(buf, x0k, nz, mask, torch.from_numpy(ren))
        lat_d = torch.empty(NS, 4, H, W, dtype=torch.float16, device=DEV)
        ops.redraw_start(buf, lat_d)
        m4 = mask[:, None].double()
        _, _, ren64 = orc.tables(gs)
    else:
        lat_d = torch.randn(NS, 4, H, W, generator=g).half().to(DEV)
    worst, states = 0.0, []
    for i in range(n):
        eps = (torch.randn(rows, 4, H, W, generator=g) * 0.5).half()
        x_in = lat_d.float().cpu()
        ctr.fill_(i)
        if redraw:
            ops.cfg_sampler_step_redraw(_nhwc(eps).to(DEV), lat_d, xin, table, buf, 4, do_cfg, ctr, solver=solver, seeds=seeds_d)
        else:
            ops.cfg_lcm_step(_nhwc(eps).to(DEV), lat_d, xin, table, solver, seeds_d, do_cfg, ctr)
        ref = orc.step(_cfg_combine(eps, gs, do_cfg).double(), i, x_in.double())
        if redraw:
            known = ren64[i + 1, 0] * x0k.double() + ren64[i + 1, 1] * nz.double()
            ref = m4 * ref + (1 - m4) * known
        got = lat_d.double().cpu()
        assert torch.isfinite(got).all(), (n, do_cfg, redraw, i)
        worst = max(worst, float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-3)))
        mi = xin.view(rows, H, W, 4).permute(0, 3, 1, 2).cpu()
        assert torch.equal(mi[:NS], lat_d.cpu()), "the model input is the unscaled latent"
        if do_cfg:
            assert torch.equal(mi[NS:], mi[:NS])
        states.append(lat_d.cpu().clone())
    if redraw:                                                                 # the last renoise row is {1, 0}
        zero = (mask == 0)[:, None].expand(NS, 4, H, W)
        assert torch.equal(states[-1][zero], x0k[zero])
    torch.cuda.synchronize()
    return worst, states


@pytest.mark.parametrize("n,do_cfg,redraw", list(itertools.product((1, 2, 4, 8), (True, False), (False, True))))
def test_lcm_kernel_sequence_vs_restatement(hip_lib, n, do_cfg, redraw):
    worst, _ = _sequence(n, do_cfg, redraw)
    print(f"[lcm sequence n={n} cfg={do_cfg} redraw={redraw}] worst per-step max|err| / max|ref| = {worst:.4g}")
    gate(f"test_gpu_lcm:1 kernel sequence n={n} cfg={do_cfg} redraw={redraw}", worst, SEQUENCE_GATE[redraw])


def test_last_step_adds_no_noise_and_seeds_matter_before_it(hip_lib):
    """Two seed pairs: every intermediate state differs, the last step - from identical inputs - is identical."""
    from diffsensei_amd import ops
    n = 4
    _, a = _sequence(n, False, False, seeds=SEEDS)
    _, b = _sequence(n, False, False, seeds=[5, 6])
    for i in range(n - 1):
        assert not torch.equal(a[i], b[i]), f"state {i} does not depend on the seeds"
    sch = _lcm()
    sch.set_timesteps(n)
    table, solver = torch.from_numpy(sch.coef_table(1.0)).to(DEV), torch.from_numpy(sch.solver_table()).to(DEV)
    g = torch.Generator().manual_seed(3)
    x, eps = torch.randn(NS, 4, H, W, generator=g).half(), (torch.randn(NS, 4, H, W, generator=g) * 0.5).half()
    outs = []
    for seeds in (SEEDS, [5, 6]):
        for i in (n - 2, n - 1):
            lat = x.to(DEV).clone()
            xin = torch.empty(NS, H * W, 4, dtype=torch.float16, device=DEV)
            ops.cfg_lcm_step(_nhwc(eps).to(DEV), lat, xin, table, solver, _seeds_dev(seeds), False,
                             torch.tensor([i], dtype=torch.int32, device=DEV))
            outs.append(lat.cpu())
    assert not torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    # ... and it is the denoised value: c_out x0 + c_skip x
    orc = LCMOracle(seeds=SEEDS).set_timesteps(n)
    sa, sb, c_out, c_skip, _, _ = orc.scalars(n - 1)
    want = c_out * (x.double() - sb * eps.double()) / sa + c_skip * x.double()
    assert float((outs[1].double() - want).abs().max() / want.abs().max()) <= 2.0 ** -10


def test_noise_depends_on_seed_and_step_only(hip_lib):
    """A panel alone, inside a batch of other seeds, and run twice: equal bits at every step index."""
    from diffsensei_amd import ops
    n, s = 4, 0x5EED5EED5EED
    sch = _lcm()
    sch.set_timesteps(n)
    table, solver = torch.from_numpy(sch.coef_table(1.0)).to(DEV), torch.from_numpy(sch.solver_table()).to(DEV)
    g = torch.Generator().manual_seed(77)
    x0 = torch.randn(1, 4, H, W, generator=g).half()
    eps1 = (torch.randn(1, 4, H, W, generator=g) * 0.5).half()
    for i in range(n):
        ctr = torch.tensor([i], dtype=torch.int32, device=DEV)
        outs = {}
        for name, ns, row, seeds in (("alone", 1, 0, [s]), ("in batch", 4, 2, [11, 2 ** 63 - 2, s, 0]), ("again", 1, 0, [s]),
                                     ("other seed", 1, 0, [s + 1])):
            lat = (torch.randn(ns, 4, H, W, generator=torch.Generator().manual_seed(5)) * 3).half()
            eps = (torch.randn(ns, 4, H, W, generator=torch.Generator().manual_seed(6)) * 0.5).half()
            lat[row], eps[row] = x0[0], eps1[0]
            lat_d = lat.to(DEV)
            xin = torch.empty(ns, H * W, 4, dtype=torch.float16, device=DEV)
            ops.cfg_lcm_step(_nhwc(eps).to(DEV), lat_d, xin, table, solver, _seeds_dev(seeds), False, ctr)
            outs[name] = lat_d[row].cpu()
        assert torch.equal(outs["alone"], outs["in batch"]), f"step {i}: noise depends on the batch"
        assert torch.equal(outs["alone"], outs["again"]), f"step {i}: same (seed, step) twice differs"
        assert torch.equal(outs["alone"], outs["other seed"]) == (i == n - 1)


def test_lcm_launch_checks(hip_lib):
    """Kind 4 without its solver rows or without its seeds is refused by every entry point, and nothing is launched."""
    from diffsensei_amd import _lib, ops
    from diffsensei_amd.engine import make_op
    lat = torch.full((1, 4, 4, 4), 3.0, dtype=torch.float16, device=DEV)
    xin = torch.zeros(1, 16, 4, dtype=torch.float16, device=DEV)
    eps = torch.ones_like(xin)
    table, solver, seeds = torch.ones(1, 8, device=DEV), torch.ones(1, 8, device=DEV), _seeds_dev([1])
    with pytest.raises(_lib.DiffSenseiHipError, match="solver"):
        ops.cfg_lcm_step(eps, lat, xin, table, None, seeds, do_cfg=False)
    with pytest.raises(_lib.DiffSenseiHipError, match="seeds"):
        ops.cfg_lcm_step(eps, lat, xin, table, solver, None, do_cfg=False)
    with pytest.raises(_lib.DiffSenseiHipError):          # the entry points that cannot carry both
        ops.cfg_sampler_step(eps, lat, xin, table, 4, do_cfg=False)
    with pytest.raises(_lib.DiffSenseiHipError):
        ops.cfg_sampler_step_noise(eps, lat, xin, table, seeds, 4, do_cfg=False)
    buf = ops.redraw_buffer(1, 4, 4, DEV)
    with pytest.raises(_lib.DiffSenseiHipError, match="solver"):
        ops.cfg_sampler_step_redraw(eps, lat, xin, table, buf, 4, do_cfg=False, seeds=seeds)
    with pytest.raises(_lib.DiffSenseiHipError, match="seeds"):
        ops.cfg_sampler_step_redraw(eps, lat, xin, table, buf, 4, do_cfg=False, solver=solver)
    with pytest.raises(_lib.DiffSenseiHipError):          # kind 5
        ops._step_panels(eps, lat, xin, table, None, solver, None, seeds, None, 1, 16, 5, False)
    for p in ((eps, lat, xin, table, None, None, None, seeds, None, None), (eps, lat, xin, table, None, None, solver, None, None, None)):
        op = make_op("SAMPLER_STEP", i=(1, 16, 4, 0, 0), p=p)
        assert hip_lib.ds_op_run(ctypes.byref(op), None) != 0
    panel = ops.panel_schedule_buffer(1, DEV)             # panel schedules: the solver rows live in the buffer, the seeds do not
    with pytest.raises(_lib.DiffSenseiHipError, match="seeds"):
        _lib.check(hip_lib.ds_cfg_sampler_step_slots_f16(eps.data_ptr(), lat.data_ptr(), xin.data_ptr(), panel.data_ptr(), None, None,
                                                         None, None, torch.zeros(1, dtype=torch.int32, device=DEV).data_ptr(), 1, 16, 4,
                                                         0, None), "ds_cfg_sampler_step_slots_f16")
    torch.cuda.synchronize()
    assert bool((lat == 3.0).all()) and bool((xin == 0).all())
    ops.cfg_lcm_step(eps, lat, xin, table, solver, seeds, do_cfg=False)
    torch.cuda.synchronize()
    assert not bool((lat == 3.0).all())


def test_standalone_scheduler_step_loop(hip_lib):
    from diffsensei_amd.schedulers import EulerDiscreteScheduler, LCMScheduler
    sch = LCMScheduler.from_config(EulerDiscreteScheduler().config)
    n, ns = 4, 2
    for run in range(2):                                   # a second run on the same object draws new seeds
        sch.set_timesteps(n, device=DEV)
        assert sch.noise_seeds is None
        gen = torch.Generator().manual_seed(31 + run)
        seeds = torch.randint(0, 2 ** 63 - 1, (ns,), generator=torch.Generator().manual_seed(31 + run)).tolist()
        orc = LCMOracle(seeds=seeds).set_timesteps(n)
        g = torch.Generator().manual_seed(32)
        x = torch.randn(ns, 4, 8, 8, generator=g).half().to(DEV)
        worst = 0.0
        for i, t in enumerate(sch.timesteps):
            assert sch.scale_model_input(x, t) is x
            e = (torch.randn(ns, 4, 8, 8, generator=g) * 0.5).half()
            ref = orc.step(e.double(), i, x.double().cpu())
            out = sch.step(e.to(DEV), t, x, generator=gen, return_dict=(i % 2 == 0))
            x = out["prev_sample"] if i % 2 == 0 else out[0]
            worst = max(worst, float((x.double().cpu() - ref).abs().max() / ref.abs().max()))
        assert sch._step_index == n and sch.noise_seeds == seeds
        gate(f"test_gpu_lcm:2 stand-alone scheduler.step loop, run {run}", worst, STANDALONE_GATE)


# ---------------------------------------------------------------- the whole pipeline
def _kwargs(parts, steps, **kw):
    return dict(dict(prompt="a manga panel", height=128, width=128, num_inference_steps=steps, guidance_scale=7.5,
                     num_samples=2, ip_images=list(parts["imgs"]), ip_bbox=[list(b) for b in IP_BBOX], ip_scale=0.6,
                     dialog_bbox=[list(b) for b in DIALOG], latents=parts["lat0"].clone(), prompt_embeds=parts["pe"],
                     pooled_prompt_embeds=parts["pooled"]), **kw)


def _call(pipe, parts, steps, **kw):
    return pipe(output_type="latent", **_kwargs(parts, steps, **kw)).images.clone()


def test_pipeline_lcm_vs_oracle(parts):
    from PIL import Image
    from oracle.pipeline_ref import sample_loop
    from oracle.resampler_ref import resampler_forward
    from oracle.unet_ref import UNetOracle
    pipe = _pipe(parts, _lcm())
    steps, ns, size = 4, 2, 128
    gen = lambda s: torch.Generator().manual_seed(s)
    results = []
    for use_graph in (False, True):
        pipe.use_graph = use_graph
        results.append(_call(pipe, parts, steps, generator=gen(9)))
        assert pipe.last_run_info["graph"] == use_graph
        seeds = torch.randint(0, 2 ** 63 - 1, (ns,), generator=gen(9)).tolist()   # the latents are given: the first draw is the seeds
        assert pipe.last_run_info["noise_seeds"] == seeds
    assert torch.equal(results[0], results[1])                                   # eager == hipGraph, same seeds
    assert torch.equal(_call(pipe, parts, steps, generator=gen(9)), results[0])
    other = _call(pipe, parts, steps, generator=gen(10))
    assert torch.isfinite(other).all() and not torch.equal(other, results[0])
    assert torch.equal(_call(pipe, parts, steps, noise_seeds=seeds), results[0])  # explicit seeds override the draw
    # guidance 1: the unconditional half is dropped (UNet batch = ns), which is where a distillation adapter is run
    one = _call(pipe, parts, steps, noise_seeds=seeds, guidance_scale=1.0)
    assert pipe.last_run_info["batch"] == ns and torch.isfinite(one).all() and not torch.equal(one, results[0])
    with pytest.raises(ValueError):
        _call(pipe, parts, 51, noise_seeds=seeds)
    # the oracle pipeline, as in tests/test_gpu_euler_ancestral.py, with the LCM restatement
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
        orc = LCMOracle(seeds=seeds)
        ref = sample_loop(UNetOracle(cfg, parts["sd"], q=hq), orc, hq(parts["lat0"].float()), hq(enc), hq(te), tid, bbox, db,
                          7.5, steps, 0.6, q=hq)
    fig = _rel(results[0], ref)
    print(f"[lcm pipeline] 4 steps, guidance 7.5, vs the oracle loop: rel-L2 {fig:.4g}")
    gate("test_gpu_lcm:3 4-step LCM pipeline vs the oracle loop driven by the restated scheduler", fig, PIPELINE_GATE)


def test_pipeline_scheduler_swaps_leave_no_state(parts):
    """Euler -> LCM -> Euler a -> LCM -> Euler on one pipeline object."""
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, LCMScheduler
    pipe = _pipe(parts, EulerDiscreteScheduler())
    e1 = _call(pipe, parts, 4)
    pipe.scheduler = LCMScheduler.from_config(pipe.scheduler.config)
    l1 = _call(pipe, parts, 4, noise_seeds=[7, 8])
    l2 = _call(pipe, parts, 4, noise_seeds=[7, 9])         # the seed buffer is reloaded on every call
    assert pipe.last_run_info["noise_seeds"] == [7, 9]
    pipe.scheduler = EulerAncestralDiscreteScheduler.from_config(pipe.scheduler.config, steps_offset=1)
    a1 = _call(pipe, parts, 5, noise_seeds=[7, 8])
    pipe.scheduler = LCMScheduler.from_config(pipe.scheduler.config)
    l3 = _call(pipe, parts, 4, noise_seeds=[7, 8])
    l8 = _call(pipe, parts, 8, noise_seeds=[7, 8])
    pipe.scheduler = EulerDiscreteScheduler.from_config(pipe.scheduler.config)
    e2 = _call(pipe, parts, 4)
    fresh_l = _call(_pipe(parts, _lcm()), parts, 4, noise_seeds=[7, 8])
    fresh_a = _call(_pipe(parts, EulerAncestralDiscreteScheduler.from_config(EulerDiscreteScheduler().config)), parts, 5,
                    noise_seeds=[7, 8])
    assert torch.isfinite(l1).all() and not torch.equal(e1, l1) and not torch.equal(l1, a1) and not torch.equal(l1, l8)
    assert torch.equal(e1, e2) and torch.equal(a1, fresh_a)
    assert torch.equal(l1, l3) and torch.equal(l1, fresh_l)
    assert torch.equal(l1[0], l2[0]) and not torch.equal(l1[1], l2[1])     # panel 0 kept its seed, panel 1 did not
    with pytest.raises(ValueError):
        _call(pipe, parts, 4, noise_seeds=[1, 2])          # Euler draws no noise


def test_request_alone_vs_inside_a_batch(parts):
    steps = 4
    g = torch.Generator().manual_seed(21)
    lat = lambda n: torch.randn(n, 4, 16, 16, generator=g).half()
    mine = lambda: _kwargs(parts, steps, generator=torch.Generator().manual_seed(3))
    before = lambda: _kwargs(parts, steps, num_samples=1, latents=lat(1), generator=torch.Generator().manual_seed(4),
                             prompt_embeds=parts["pe"] * 0.5)
    after = lambda: _kwargs(parts, steps, num_samples=1, latents=lat(1), generator=torch.Generator().manual_seed(5), dialog_bbox=[])
    pipe = _pipe(parts, _lcm())
    alone = pipe(output_type="latent", **mine()).images.clone()
    seeds_alone = pipe.last_run_info["noise_seeds"]
    out = pipe.generate_batch([before(), mine(), after()], output_type="latent")
    assert [o.shape[0] for o in out] == [1, 2, 1]
    assert pipe.last_run_info["noise_seeds"][1:3] == seeds_alone and len(pipe.last_run_info["noise_seeds"]) == 4
    # the rule of tests/test_gpu_euler_ancestral.py: the panel's noise is its own, so what is left is what the
    # batch-size-dependent kernel choice rounds differently - 0 at this shape (the plans of UNet batch 4 and 8 pick the same
    # kernels), held at the gate the plain samplers' alone-vs-batch figures have
    gate("test_gpu_lcm:4 LCM request alone vs inside a batch, rel-L2", _rel(out[1], alone), 1.0e-2)


def test_continuous_batching_requests_equal_their_uniform_batches(pipe):
    """Requests of 4, 2 and 2 LCM steps through two slots, the third admitted into the slot the second left: each equals row q
    of a uniform `generate_batch` of its own step count, `torch.equal` - the rule of tests/test_gpu_continuous.py."""
    from tests.test_gpu_continuous import _queue, _references
    p, cfg, sd, rs, clip, mae, A, B = pipe
    old = p.scheduler
    try:
        p.scheduler = _lcm()
        want = _references(p, "LCMScheduler", A, B, cfg)
        out = p.generate_continuous([_clone(r) for r in _queue(p, A, B, cfg)], slots=2, output_type="latent")
        info = dict(p.last_run_info)
    finally:
        p.scheduler = old
    assert info["continuous"]["admissions"] == [(0, 0, [0]), (0, 1, [1]), (2, 2, [1])] and info["continuous"]["forwards"] == 4
    assert info["noise_seeds"] == [[5], [6], [7]]
    for tag, o, w in zip("ABC", out, want):
        assert o.shape == (1, 4, 16, 16) and torch.isfinite(o).all()
        assert torch.equal(o, w), f"request {tag} differs from its uniform batch"
    assert not torch.equal(out[1], out[2])
