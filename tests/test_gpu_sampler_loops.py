"""GPU: the sampler-step kernels run FREE for the benchmarked 50 steps over the closed-form denoiser of tests/_loop_cases.py.

The lock-step tests (tests/test_gpu_ops.py::test_cfg_sampler_step, tests/test_gpu_dpm.py::_sequence, the Euler Ancestral twin)
restart every reference step from the kernel's own latents and fill the step counter from the host.  Here nothing is re-seeded:
the counter lives on the device and is advanced there, eps of step i is the ideal prediction for the device's OWN model input
(float64 torch on the device, rounded to fp16 once), and what one step hands the next - latents, model input, previous x0, the
Philox step index, a panel slot's rows - is whatever the kernels left.

Gates, all from the references on the CPU (tests/test_sampler_loops_host.py shows that they hold for the references alone and
that a truncating latent store leaves them):
  rel-L2(device, float64 loop)  <= 2 * D_emul(kind, cfg)   D_emul = rel-L2(fp16-storage emulation, float64 loop).  The device
                                                            loop and the emulation are two realisations of the same rounding
                                                            noise (fp32 intermediates, flips of single fp16 ulps); a
                                                            systematic error grows linearly over 50 steps and leaves the band.
  rel-L2(device, closed form)   <= 1.25 * rel-L2(float64 loop, closed form)          (not for Euler Ancestral: no claim)
  model_in == new latents / c_in_div_next after every step: bit for bit where the divisor is 1 (DDIM, DPM-Solver++, every
  last row), within 1 fp16 ulp of the fp32 quotient elsewhere (as tests/test_gpu_redraw.py); the final counter is 50.
"""
import numpy as np
import pytest
import torch

from tests import _loop_cases as L
from tests import _redraw_ref as R
from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, HW = L.H, L.W, L.H * L.W


def _nhwc(x):
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).contiguous()


def _mu_rows(cases, do_cfg):
    """float64 [rows, HW, 4] on the device: the mean every model_in row is denoised towards ([uncond | cond] under CFG)."""
    mu_u, mu_c = torch.cat([c.mu_u for c in cases]), torch.cat([c.mu_c for c in cases])
    return (torch.cat([_nhwc(mu_u), _nhwc(mu_c)]) if do_cfg else _nhwc(mu_c)).to(DEV)


def _check_model_in(xin, lat, div, do_cfg, what):
    ns = lat.shape[0]
    got = xin.view(xin.shape[0], H, W, 4).permute(0, 3, 1, 2)
    if div == 1.0:
        assert torch.equal(got[:ns], lat), f"{what}: model_in != new latents"
    else:
        want = (lat.float() / div).half()
        assert int(R.ulp16(got[:ns], want).max()) <= 1, f"{what}: model_in != new latents / c_in_div_next ({div})"
    if do_cfg:
        assert torch.equal(got[ns:], got[:ns]), f"{what}: the CFG halves of model_in differ"


def _counter():
    """(device step counter, the launch that advances it): the project's own counter kernel - the op the engine's step plan
    ends with - so the counter is never written from the host after it is zeroed."""
    from diffsensei_amd.engine import Plan, make_op
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    return ctr, Plan([make_op("ADVANCE", p=(ctr,))], [ctr])


def _table(rows):
    """The rows on the device with two NaN rows behind them: a counter that ran ahead reads NaN, not another allocation."""
    t = torch.as_tensor(rows, dtype=torch.float32)
    return torch.cat([t, torch.full((2, t.shape[1]), float("nan"))]).to(DEV)


def _schedule(kind, n):
    """(host scheduler, float64 model sigmas of the restatement's own table) for an n-step run."""
    return L.host_scheduler(kind, n), L.model_sigmas(kind, L.make_oracle(kind, n, exact=True))


def _device_loop(kind, do_cfg, path, c, n=L.STEPS):
    """n free-running steps of `c` through the single-table entry points (path "table") or the panel-schedule path (path
    "slots", every slot the same schedule).  Returns the final latents."""
    from diffsensei_amd import ops
    ns = c.ns
    sch, sig = _schedule(kind, n)
    coef = sch.coef_table(L.GUIDANCE)
    table = _table(coef)
    solver = _table(sch.solver_table()) if kind == 2 else None
    seeds = torch.tensor(c.noise_seeds, dtype=torch.int64, device=DEV) if kind == 3 else None
    lat = c.start(kind, sig[0], do_cfg).half().to(DEV)
    prev = torch.full_like(lat, float("nan")) if kind == 2 else None          # the first row is first order: never read
    rows = 2 * ns if do_cfg else ns
    xin = torch.empty(rows, HW, 4, dtype=torch.float16, device=DEV)
    ctr, advance = _counter()
    mu = _mu_rows([c], do_cfg)
    if path == "table":
        ops.prepare_model_input(lat, xin, table, do_cfg, ctr)
    else:
        ps = sch.panel_schedule(n, 1.0, L.GUIDANCE)
        assert ps["t_start"] == 0 and ps["steps"] == n
        panel = ops.panel_schedule_buffer(ns, DEV)
        for slot in range(ns):
            ops.panel_slot_load(panel, ns, slot, 0, torch.from_numpy(ps["rows"]),
                                None if kind != 2 else torch.from_numpy(ps["solver_rows"]))
        ops.panel_slot_start(panel, None, lat, xin, 0, ns, do_cfg)
        guidance = torch.full((ns,), L.GUIDANCE, dtype=torch.float32, device=DEV) if do_cfg else None
    _check_model_in(xin, lat, float(coef[0, 1]), do_cfg, "start")
    for i in range(n):
        eps = L.eps_ideal(xin, sig[i], mu).half()
        if path == "slots":
            ops.cfg_sampler_step_slots(eps, lat, xin, panel, kind, ctr, guidance, do_cfg, prev, seeds, None)
        elif kind == 2:
            ops.cfg_dpm_step(eps, lat, xin, table, solver, prev, do_cfg, ctr)
        elif kind == 3:
            ops.cfg_sampler_step_noise(eps, lat, xin, table, seeds, 3, do_cfg, ctr)
        else:
            ops.cfg_sampler_step(eps, lat, xin, table, kind, do_cfg, ctr)
        _check_model_in(xin, lat, float(coef[i, 6]), do_cfg, f"{L.KINDS[kind]} cfg={do_cfg} {path} step {i}")
        advance.run()                                                         # on the device, never re-filled from the host
    assert int(ctr.item()) == n
    assert torch.isfinite(lat).all()
    return lat.cpu()


def _gates(name, got, kind, do_cfg, n, ns, seed):
    c = L.case(ns, seed)
    d_loop, d_emul = L.rel(got, L.f64_loop(kind, do_cfg, n, ns, seed)), L.d_emul(kind, do_cfg, n, ns, seed)
    d_cf = None if kind == 3 else L.rel(got, L.closed_form(kind, n, do_cfg, c))
    print(f"{name}: vs float64 loop {d_loop:.3e} (D_emul {d_emul:.3e}), vs closed form {d_cf}")     # figures, then assertions
    gate(f"{name}: rel-L2 vs the float64 loop (2 x D_emul)", d_loop, 2 * d_emul)
    if kind != 3:
        gate(f"{name}: rel-L2 vs the closed form (1.25 x the float64 loop's own)", d_cf,
             1.25 * L.d_closed(kind, do_cfg, n, ns, seed))


@pytest.mark.parametrize("path", ["table", "slots"])
@pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_fifty_free_running_steps(hip_lib, kind, do_cfg, path):
    c = L.case()
    assert L.d_emul(kind, do_cfg) <= 5e-3
    got = _device_loop(kind, do_cfg, path, c)
    _gates(f"{L.KINDS[kind]} cfg={do_cfg} {path}, 50 free steps", got, kind, do_cfg, L.STEPS, c.ns, c.seed)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_panels_of_different_length_with_a_refill(hip_lib, kind):
    """Two slots under CFG: a 50-step panel beside a 20-step one; when the short one has finished (counter 20) its slot is
    refilled with a 30-step panel that starts at that step.  Every panel ends with the bits of that panel run alone through
    the single-table entry points, and passes the 2 * D_emul gate of its own length."""
    from diffsensei_amd import ops
    ns, do_cfg = 2, True
    runs = {"A": (L.case(1, 11), 50), "B": (L.case(1, 12), 20), "C": (L.case(1, 13), 30)}
    alone = {k: _device_loop(kind, do_cfg, "table", c, n) for k, (c, n) in runs.items()}
    sched = {k: _schedule(kind, n) for k, (c, n) in runs.items()}
    ps = {k: sched[k][0].panel_schedule(runs[k][1], 1.0, L.GUIDANCE) for k in runs}
    start = lambda k: runs[k][0].start(kind, sched[k][1][0], do_cfg).half().to(DEV)
    lat = torch.cat([start("A"), start("B")])
    prev = torch.full_like(lat, float("nan")) if kind == 2 else None
    seeds = torch.tensor([runs["A"][0].noise_seeds[0], runs["B"][0].noise_seeds[0]], dtype=torch.int64, device=DEV) \
        if kind == 3 else None
    xin = torch.empty(2 * ns, HW, 4, dtype=torch.float16, device=DEV)
    ctr, advance = _counter()
    guidance = torch.full((ns,), L.GUIDANCE, dtype=torch.float32, device=DEV)
    panel = ops.panel_schedule_buffer(ns, DEV)

    def load(slot, k, at):
        ops.panel_slot_load(panel, ns, slot, at, torch.from_numpy(ps[k]["rows"]),
                            None if kind != 2 else torch.from_numpy(ps[k]["solver_rows"]))

    load(0, "A", 0)
    load(1, "B", 0)
    ops.panel_slot_start(panel, None, lat, xin, 0, ns, do_cfg)
    slots = [("A", 0), ("B", 0)]                    # (occupant, the counter value its schedule began at)
    final = {}
    for s in range(50):
        if s == 20:                                 # B has run its 20 rows: hand its slot to C
            final["B"] = lat[1].cpu().clone()
            lat[1] = start("C")[0]
            if kind == 3:
                seeds[1] = runs["C"][0].noise_seeds[0]
            load(1, "C", 20)
            ops.panel_slot_start(panel, None, lat, xin, 1, 1, do_cfg)
            slots[1] = ("C", 20)
        sig = torch.tensor([sched[k][1][s - at] for k, at in slots] * 2, dtype=torch.float64).view(2 * ns, 1, 1)
        mu = _mu_rows([runs[k][0] for k, _ in slots], do_cfg)
        eps = L.eps_ideal(xin, sig, mu).half()
        ops.cfg_sampler_step_slots(eps, lat, xin, panel, kind, ctr, guidance, do_cfg, prev, seeds, None)
        advance.run()
    assert int(ctr.item()) == 50
    final["A"], final["C"] = lat[0].cpu(), lat[1].cpu()
    for k, (c, n) in runs.items():
        assert torch.equal(final[k], alone[k][0]), f"{L.KINDS[kind]}: panel {k} ({n} steps) differs from that panel run alone"
        _gates(f"{L.KINDS[kind]} mixed-length slots, panel {k} ({n} steps)", final[k][None], kind, do_cfg, n, 1, c.seed)


def test_redraw_fifty_nominal_steps_at_strength_06(hip_lib):
    """Euler under CFG through `cfg_sampler_step_redraw`: the right half of every panel is kept, strength 0.6 of 50 nominal
    steps (30 run, from row 20).  The kept half is the kept latents re-noised to the state's noise level after every step (<= 1
    fp16 ulp from tests/_redraw_ref.known, the kernel may contract) and the kept latents bit for bit at the end; the free half
    is a free-running Euler loop from row 20 and passes the gates of that loop."""
    from diffsensei_amd import ops
    kind, do_cfg, n, c = 0, True, L.STEPS, L.case()
    ns = c.ns
    sch, sig = _schedule(kind, n)
    ps = sch.panel_schedule(n, 0.6, L.GUIDANCE)
    t0, run = ps["t_start"], ps["steps"]
    assert (t0, run) == (R.start_index(n, 0.6), n - R.start_index(n, 0.6)) == (20, 30)
    want_rows = R.renoise_rows("sigma", ps["timesteps"], sig[t0:])
    assert np.allclose(ps["renoise_rows"], want_rows, rtol=1e-6, atol=0)
    x0k = L.closed_form(kind, n, do_cfg, c).half()              # what an earlier run ended on
    noise = c.z.half()
    mask = torch.zeros(ns, H, W)
    mask[:, :, :W // 2] = 1.0
    free = (mask[:, None] == 1).expand(ns, 4, H, W)
    buf = ops.redraw_buffer(ns, H, W, DEV)
    ops.redraw_load(buf, x0k, noise, mask, torch.from_numpy(ps["renoise_rows"]))
    lat = torch.empty(ns, 4, H, W, dtype=torch.float16, device=DEV)
    ops.redraw_start(buf, lat)
    assert int(R.ulp16(lat, R.known(x0k, noise, *ps["renoise_rows"][0])).max()) <= 1
    x_start = lat.cpu().double()
    table = _table(ps["rows"])
    xin = torch.empty(2 * ns, HW, 4, dtype=torch.float16, device=DEV)
    ctr, advance = _counter()
    ops.prepare_model_input(lat, xin, table, do_cfg, ctr)
    mu = _mu_rows([c], do_cfg)
    for i in range(run):
        eps = L.eps_ideal(xin, sig[t0 + i], mu).half()
        ops.cfg_sampler_step_redraw(eps, lat, xin, table, buf, kind, do_cfg, ctr)
        kept = R.known(x0k, noise, *ps["renoise_rows"][i + 1])
        assert int(R.ulp16(lat, kept)[~free].max()) <= 1, f"step {i}: the kept half is not the re-noised kept latents"
        _check_model_in(xin, lat, float(ps["rows"][i, 6]), do_cfg, f"redraw step {i}")
        advance.run()
    assert int(ctr.item()) == run
    got = lat.cpu()
    assert torch.equal(got[~free], x0k[~free])
    ref = L.run_loop(kind, n, do_cfg, c, t_start=t0, x_start=x_start)[0]
    emu = L.run_loop(kind, n, do_cfg, c, emulate=True, t_start=t0, x_start=x_start)[0]
    closed = L.closed_form(kind, n, do_cfg, c, t_start=t0, x_start=x_start)
    d_emul = L.rel(emu[free], ref[free])
    assert 0.0 < d_emul <= 5e-3
    gate("euler redraw 0.6 x 50, free half: rel-L2 vs the float64 loop (2 x D_emul)", L.rel(got[free], ref[free]), 2 * d_emul)
    gate("euler redraw 0.6 x 50, free half: rel-L2 vs the closed form (1.25 x the float64 loop's own)",
         L.rel(got[free], closed[free]), 1.25 * L.rel(ref[free], closed[free]))
