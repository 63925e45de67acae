"""GPU: the panel-schedule entry points inside poisoned memory, with the cases, helpers and references of
tests/test_gpu_poisoned_memory.py (see its docstring for what a case asserts).

The cases are appended to that module's CASES list when this module is imported, which pytest does for every test module
before it runs a test: `test_every_entry_point_has_a_case` there then finds the new entry points covered.  They RUN here,
through that module's own test function.

The panel-schedule buffer is built on the host from the layout documented in include/diffsensei_hip.h, not through the
library's loader, and every row no panel runs holds the run's poison: a result that moves with the fill has read a row
that is not the panel's own."""
import functools
import importlib

import pytest
import torch

# the module object pytest itself runs (test modules are imported under their base names): its CASES is the list the
# completeness test reads
try:
    PM = importlib.import_module("test_gpu_poisoned_memory")
except ImportError:                                             # imported as part of the `tests` package instead
    PM = importlib.import_module("tests.test_gpu_poisoned_memory")

NS_, SH, SW, NSTEP = PM.NS_, PM.SH, PM.SW, PM.NSTEP
R = 1024
STEP = 3                    # both panels are at row 3 of the 10-step schedule: panel 0 started at counter 0, panel 1 at 2
FIRST = len(PM.CASES)


def _panel_host(ns, fill):
    """(uint8 host buffer pre-filled with `fill` in every fp32 row, its views) per include/diffsensei_hip.h"""
    F = (8 * ns + 15) & ~15
    buf = torch.zeros(F + 4 * ns * (4 + 16 * R + 2 * (R + 1)), dtype=torch.uint8)
    assert buf.numel() == int(PM._lib().ds_panel_schedule_bytes(ns))
    i32, f32 = buf[:8 * ns].view(torch.int32), buf[F:].view(torch.float32)
    f32.copy_(fill.expand(f32.numel()))
    a, b, c = 4 * ns, 4 * ns + 8 * R * ns, 4 * ns + 16 * R * ns
    return buf, (i32[:ns], i32[ns:], f32[:a].view(ns, 4), f32[a:b].view(ns, R, 8), f32[b:c].view(ns, R, 8), f32[c:].view(ns, R + 1, 2))


def _panel(m, h, renoise=None, modes=(2, 2), sigma=1.0, starts=(0, 2)):
    """Panel 0 runs the whole schedule from counter 0, panel 1 the rows [2:] from counter 2: at counter 3 both are at row 3."""
    buf, (start, steps, mode, coef, solver, rn) = _panel_host(NS_, m.poison((1,), torch.float32))
    for n, t0 in enumerate(starts):
        k = NSTEP - t0
        start[n], steps[n] = t0, k
        mode[n] = torch.tensor([float(modes[n]), sigma, 0.0, 0.0])
        coef[n, :k] = h.table[t0:]
        if h.solver is not None:
            solver[n, :k] = h.solver[t0:]
        if renoise is not None:
            rn[n, :k + 1] = renoise[t0:]
    return m.place(buf)


def _step_run(m, h):
    eps, lat = m.place(h.eps), m.place(h.lat)
    xin = m.out((2 * NS_, SH * SW, 4))
    ctr = m.place(torch.tensor([STEP], dtype=torch.int32))
    prev = m.place(h.prev) if h.kind == 2 else None
    seeds = m.place(h.seeds) if h.kind == 3 else None
    rd = hasattr(h, "rd")
    # Euler Ancestral draws its noise for the panel's OWN step index: the reference of `_step_data` draws for step 3, so
    # there both panels run the whole schedule from counter 0
    panel = _panel(m, h, h.rd.rows.float() if rd else None, starts=(0, 0) if h.kind == 3 else (0, 2))
    m.ops.cfg_sampler_step_slots(eps, lat, xin, panel, h.kind, ctr, m.place(h.guidance), True, prev, seeds,
                                 PM._redraw_buffer(m, h) if rd else None)
    return (lat, xin) + ((prev,) if h.kind == 2 else ())


for kind in (0, 1, 2, 3):
    for redraw in (False, True):
        PM._add(f"panel-step-kind{kind}{'-redraw' if redraw else ''}", ["ds_cfg_sampler_step_slots_f16", "ds_panel_schedule_bytes"],
                functools.partial(PM._step_data, kind, STEP, True, redraw), _step_run, PM._step_check)


def _frozen_run(m, h):
    """counter 0: panel 1 (start 2) has not begun - nothing of it may be stored, nothing of its rows read"""
    eps, lat, xin = m.place(h.eps), m.place(h.lat), m.place(h.eps)
    panel = _panel(m, h)
    m.ops.cfg_sampler_step_slots(eps, lat, xin, panel, h.kind, m.place(torch.zeros(1, dtype=torch.int32)), m.place(h.guidance), True)
    return (lat, xin)


def _frozen_check(o, h):
    assert torch.equal(o[0][1], h.lat[1]) and not torch.equal(o[0][0], h.lat[0])
    assert torch.equal(o[1][1], h.eps[1]) and torch.equal(o[1][NS_ + 1], h.eps[NS_ + 1]) and not torch.equal(o[1][0], h.eps[0])


PM._add("panel-step-kind0-one-panel-not-started", ["ds_cfg_sampler_step_slots_f16"], functools.partial(PM._step_data, 0, 0, True),
        _frozen_run, _frozen_check)


def _temb_run(m, h):
    """rows 0 / 2 / 4: panel 0 at its row 1 (t = 41), rows 1 / 3 / 5: an empty slot (t = 0) whose rows are poison"""
    buf, (start, steps, mode, coef, solver, rn) = _panel_host(2, m.poison((1,), torch.float32))
    start[0], steps[0], start[1], steps[1] = 2, 2, 0, 0
    coef[0, :2] = h.table
    return (m.ops.timestep_embed_slots(m.place(buf), 2, 6, 320, m.place(torch.tensor([3], dtype=torch.int32))),)


def _temb_check(o, h):
    from oracle.unet_ref import timestep_sinusoid
    PM._close(o[0][0::2], h.ref, 2e-3, "sinusoid, panel rows")
    PM._close(o[0][1::2], timestep_sinusoid(torch.zeros(3), 320), 2e-3, "sinusoid, empty slot")


PM._add("panel-timestep-embed-6x320", ["ds_timestep_embed_slots_f16"], PM._time_data, _temb_run, _temb_check)


def _start_run(m, h):
    """slot 1 alone, from its own renoise row 0 (the schedule's row 2); slot 0's latents and model input stay as placed"""
    lat, xin = m.place(h.lat), m.place(h.eps)
    panel = _panel(m, h, h.rd.rows.float(), modes=(1, 0), sigma=h.rd.init_sigma)
    m.ops.panel_slot_start(panel, PM._redraw_buffer(m, h), lat, xin, 1, 1, True)
    return (lat, xin)


def _start_check(o, h):
    from tests import _redraw_ref as RR
    want = RR.known(h.rd.x0, h.rd.noise, *h.rd.rows[2].tolist())
    assert int(RR.ulp16(o[0][1:], want[1:]).max()) <= 1        # tests/test_gpu_redraw.py::test_redraw_start: one contraction
    assert torch.equal(o[0][0], h.lat[0]) and torch.equal(o[1][0], h.eps[0]) and torch.equal(o[1][NS_], h.eps[NS_])
    got = o[1].view(2 * NS_, SH, SW, 4).permute(0, 3, 1, 2)
    PM._close(got[1], PM.hq(o[0][1].float() / float(h.table[2, 1])), 1.5e-3, "model input of the started slot")
    assert torch.equal(got[NS_ + 1], got[1])


PM._add("panel-slot-start-one-slot", ["ds_panel_slot_start_f16"], functools.partial(PM._step_data, 0, 3, False, True), _start_run,
        _start_check)


def _load_run(m, h):
    """slot 1 of 2 into a zeroed buffer out of device rows that sit between poison; slot 0 stays zero"""
    panel = m.place(torch.zeros(int(PM._lib().ds_panel_schedule_bytes(NS_)), dtype=torch.uint8))
    m.ops.panel_slot_load(panel, NS_, 1, 5, m.place(h.table[2:]), m.place(h.solver[2:]), m.place(h.rd.rows.float()[2:]), 1, 0.75)
    return (panel,)


def _load_check(o, h):
    buf, (start, steps, mode, coef, solver, rn) = _panel_host(NS_, torch.zeros(1))
    k = NSTEP - 2
    start[1], steps[1] = 5, k
    mode[1] = torch.tensor([1.0, 0.75, 0.0, 0.0])
    coef[1, :k], solver[1, :k], rn[1, :k + 1] = h.table[2:], h.solver[2:], h.rd.rows.float()[2:]
    assert torch.equal(o[0], buf), "the loaded slot is not the documented layout, or another slot changed"


PM._add("panel-slot-load", ["ds_panel_slot_load", "ds_panel_schedule_bytes"], functools.partial(PM._step_data, 2, 3, False, True), _load_run,
        _load_check)

OURS = PM.CASES[FIRST:]


def test_the_panel_entry_points_are_covered():
    """host only: the completeness test of tests/test_gpu_poisoned_memory.py, run with these cases registered"""
    PM.test_every_entry_point_has_a_case()
    named = {e for c in OURS for e in c.entry}
    assert named == {"ds_cfg_sampler_step_slots_f16", "ds_timestep_embed_slots_f16", "ds_panel_slot_start_f16", "ds_panel_slot_load",
                     "ds_panel_schedule_bytes"}


@pytest.mark.gpu
@pytest.mark.parametrize("case", OURS, ids=lambda c: c.id)
def test_panel_result_depends_on_nothing_but_the_operands(hip_lib, case):
    PM.test_result_depends_on_nothing_but_the_operands(hip_lib, case)
