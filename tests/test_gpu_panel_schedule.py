"""GPU: the panel-schedule kernels (include/diffsensei_hip.h, "Panel schedules") against the kernels they extend.

Per panel the panel-mode step is the same instruction sequence on the same operands as the single-table step, so every
comparison is `torch.equal`: a panel of the batched launch against the existing kernel run on that panel ALONE with its
own rows and its own counter (tests/test_gpu_per_panel_scales.py holds mixed batches to the same standard)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests._sampler_common import SDXL

DEV = "cuda"
CLOCKS = [(0, 3), (1, 2), (0, 1)]          # (start, steps) per panel; five global steps cover before / during / after
GUIDANCE = [2.0, 5.0, 7.5]
SEEDS = [11, 2 ** 40 + 3, 7]


def _scheduler(kind):
    from diffsensei_amd import schedulers as S
    return [S.EulerDiscreteScheduler, S.DDIMScheduler, S.DPMSolverMultistepScheduler, S.EulerAncestralDiscreteScheduler][kind](**SDXL)


def _schedules(kind, clocks=CLOCKS):
    sch = _scheduler(kind)
    return [sch.panel_schedule(steps, 1.0, 1.0) for _, steps in clocks]


def _load_panel(ns, clocks, schedules, modes=None, sigma=None):
    from diffsensei_amd import ops
    panel = ops.panel_schedule_buffer(ns, DEV)
    for v in ops.panel_schedule_views(panel, ns)[2:]:
        v.fill_(float("nan"))                                  # rows nobody loaded must never reach a result
    for n, ((start, _), s) in enumerate(zip(clocks, schedules)):
        ops.panel_slot_load(panel, ns, n, start, torch.from_numpy(s["rows"]),
                            None if s["solver_rows"] is None else torch.from_numpy(s["solver_rows"]),
                            torch.from_numpy(s["renoise_rows"]), (modes or [2] * ns)[n],
                            s["init_noise_sigma"] if sigma is None else sigma[n])
    return panel


def _reference_step(kind, do_cfg, n, j, sched, eps, lat, prev, xin, redraw_parts):
    """The EXISTING kernel on panel n alone: its rows as the table, its local step j as the counter."""
    from diffsensei_amd import ops
    ns = lat.shape[0]
    H, W = lat.shape[2], lat.shape[3]
    e1 = torch.cat([eps[n:n + 1], eps[ns + n:ns + n + 1]]) if do_cfg else eps[n:n + 1].clone()
    l1, p1 = lat[n:n + 1].clone(), prev[n:n + 1].clone()
    x1 = torch.cat([xin[n:n + 1], xin[ns + n:ns + n + 1]]) if do_cfg else xin[n:n + 1].clone()
    table = torch.from_numpy(sched["rows"]).to(DEV)
    solver = None if sched["solver_rows"] is None else torch.from_numpy(sched["solver_rows"]).to(DEV)
    ctr = torch.tensor([j], dtype=torch.int32, device=DEV)
    g = torch.tensor([GUIDANCE[n]], dtype=torch.float32, device=DEV)
    seeds = torch.tensor([SEEDS[n]], dtype=torch.int64, device=DEV) if kind == 3 else None
    if redraw_parts is not None:
        x0, nz, mask = redraw_parts
        buf = ops.redraw_buffer(1, H, W, DEV)
        ops.redraw_load(buf, x0[n:n + 1], nz[n:n + 1], mask[n:n + 1], torch.from_numpy(sched["renoise_rows"]))
        ops.cfg_sampler_step_redraw(e1, l1, x1, table, buf, kind, do_cfg, ctr, guidance=g, solver=solver,
                                    prev_x0=p1 if kind == 2 else None, seeds=seeds)
    elif kind == 2:
        ops.cfg_dpm_step(e1, l1, x1, table, solver, p1, do_cfg, ctr, guidance=g)
    elif kind == 3:
        ops.cfg_sampler_step_noise(e1, l1, x1, table, seeds, kind, do_cfg, ctr, guidance=g)
    else:
        ops.cfg_sampler_step(e1, l1, x1, table, kind, do_cfg, ctr, guidance=g)
    return l1, p1, x1


@pytest.mark.gpu
@pytest.mark.parametrize("redraw", [False, True], ids=["plain", "redraw"])
@pytest.mark.parametrize("hw", [(10, 12), (16, 16)], ids=["hw120", "hw256"])
@pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_panel_step_equals_the_single_table_kernel_per_panel(hip_lib, kind, do_cfg, hw, redraw):
    """ns = 3; HW = 120 leaves a tail block (360 threads) and puts both panel boundaries inside a wavefront.  After every one of
    five global steps each panel's latents, prev_x0 and both model_in halves equal the existing kernel run on that panel alone;
    a panel before its start or after its end keeps the bits of the step before."""
    from diffsensei_amd import ops
    ns, (H, W) = 3, hw
    HW = H * W
    g = torch.Generator().manual_seed(100 * kind + 10 * do_cfg + H)
    rnd = lambda *s: torch.randn(*s, generator=g).half().to(DEV)
    schedules = _schedules(kind)
    panel = _load_panel(ns, CLOCKS, schedules)
    rows_b = 2 * ns if do_cfg else ns
    lat, prev, xin = rnd(ns, 4, H, W), rnd(ns, 4, H, W), rnd(rows_b, HW, 4)
    guidance = torch.tensor(GUIDANCE, dtype=torch.float32, device=DEV)
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device=DEV) if kind == 3 else None
    parts = rd = None
    if redraw:
        mask = torch.tensor([0.0, 1.0, 0.25, 0.6])[torch.randint(0, 4, (ns, H, W), generator=g)]
        parts = (rnd(ns, 4, H, W), rnd(ns, 4, H, W), mask.to(DEV))
        rd = ops.redraw_buffer(ns, H, W, DEV)
        # the buffer's own header and renoise rows are NOT read on panel schedules: NaN there must not show
        ops.redraw_load(rd, parts[0], parts[1], parts[2], torch.full((3, 2), float("nan")), False, float("nan"))
        assert {0.0, 1.0} <= set(mask.unique().tolist()) and len(mask.unique()) == 4
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s in range(5):
        eps = rnd(rows_b, HW, 4)
        ctr.fill_(s)
        want_l, want_p, want_x = lat.clone(), prev.clone(), xin.clone()
        active = []
        for n, (start, steps) in enumerate(CLOCKS):
            j = s - start
            if 0 <= j < steps:
                active.append(n)
                l1, p1, x1 = _reference_step(kind, do_cfg, n, j, schedules[n], eps, lat, prev, xin, parts)
                want_l[n], want_p[n], want_x[n] = l1[0], p1[0], x1[0]
                if do_cfg:
                    want_x[ns + n] = x1[1]
        ops.cfg_sampler_step_slots(eps, lat, xin, panel, kind, ctr, guidance if do_cfg else None, do_cfg,
                                   prev if kind == 2 else None, seeds, rd)
        assert active == [[0, 2], [0, 1], [0, 1], [], []][s]
        for n in range(ns):
            what = f"kind {kind} step {s} panel {n} ({'active' if n in active else 'frozen'})"
            assert torch.equal(lat[n], want_l[n]), f"{what}: latents"
            assert torch.equal(prev[n], want_p[n]), f"{what}: prev_x0"
            assert torch.equal(xin[n], want_x[n]), f"{what}: model_in"
            if do_cfg:
                assert torch.equal(xin[ns + n], want_x[ns + n]), f"{what}: model_in, conditional half"
        assert torch.isfinite(lat).all() and torch.isfinite(xin).all()


@pytest.mark.gpu
@pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "nocfg"])
def test_euler_ancestral_noise_does_not_depend_on_the_admission_step(hip_lib, do_cfg):
    """Two panels with one seed, one schedule, one start state and the same eps per LOCAL step, admitted at global steps 0
    and 1: the Philox step index is the local step, so they end bit-identical (and the noise is really there)."""
    from diffsensei_amd import ops
    ns, H, W, steps = 2, 10, 12, 3
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).half()
    sched = _scheduler(3).panel_schedule(steps, 1.0, 1.0)
    panel = _load_panel(ns, [(0, steps), (1, steps)], [sched, sched])
    one = rnd(1, 4, H, W)
    lat = one.repeat(2, 1, 1, 1).to(DEV)
    xin = torch.zeros(2 * ns if do_cfg else ns, H * W, 4, dtype=torch.float16, device=DEV)
    local = [[rnd(1, H * W, 4) for _ in range(2)] for _ in range(steps)]         # [local step][uncond, cond]
    seeds = torch.tensor([99, 99], dtype=torch.int64, device=DEV)
    guidance = torch.tensor([4.0, 4.0], device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    after_first = None
    for s in range(steps + 1):
        pick = lambda n, half: local[min(max(s - n, 0), steps - 1)][half]
        eps = torch.cat([pick(0, 0), pick(1, 0)] + ([pick(0, 1), pick(1, 1)] if do_cfg else [])).to(DEV)
        ctr.fill_(s)
        ops.cfg_sampler_step_slots(eps, lat, xin, panel, 3, ctr, guidance if do_cfg else None, do_cfg, None, seeds, None)
        if s == 0:
            after_first = lat[0].clone()
            assert torch.equal(lat[1].cpu(), one[0]), "panel 1 has not started"
        if s == 1:
            assert torch.equal(lat[1], after_first), "local step 0 at global step 1 draws the noise of step 0"
    assert torch.equal(lat[0], lat[1])
    other = torch.tensor([99, 100], dtype=torch.int64, device=DEV)
    lat2 = one.repeat(2, 1, 1, 1).to(DEV)
    ctr.fill_(0)
    ops.panel_slot_load(panel, ns, 1, 0, torch.from_numpy(sched["rows"]))
    ops.cfg_sampler_step_slots(torch.cat([local[0][0]] * 2 + ([local[0][1]] * 2 if do_cfg else [])).to(DEV), lat2, xin, panel, 3,
                               ctr, guidance if do_cfg else None, do_cfg, None, other, None)
    assert not torch.equal(lat2[0], lat2[1]), "another seed is another noise"


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [32, 320])
def test_panel_time_embedding_equals_the_scalar_kernel_row_by_row(hip_lib, dim):
    """ns = 4 with an empty slot whose rows hold NaN: row b embeds the timestep of panel b % ns at clamp(j, 0, steps - 1),
    the empty slot embeds 0 - every row equals the scalar kernel's row for that timestep, so every row is finite."""
    from diffsensei_amd import ops
    ns, B = 4, 8
    clocks = CLOCKS + [(2, 0)]
    schedules = _schedules(0)
    panel = ops.panel_schedule_buffer(ns, DEV)
    for v in ops.panel_schedule_views(panel, ns)[2:]:
        v.fill_(float("nan"))
    for n, ((start, _), s) in enumerate(zip(CLOCKS, schedules)):
        ops.panel_slot_load(panel, ns, n, start, torch.from_numpy(s["rows"]))
    ops.panel_slot_load(panel, ns, 3, 2, None)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    seen = set()
    for s in range(5):
        ctr.fill_(s)
        got = ops.timestep_embed_slots(panel, ns, B, dim, ctr, flip=True, freq_shift=0.0)
        assert got.shape == (B, dim) and torch.isfinite(got).all()
        for b in range(B):
            n = b % ns
            start, steps = clocks[n]
            t = 0.0 if steps == 0 else float(schedules[n]["rows"][min(max(s - start, 0), steps - 1), 0])
            seen.add(t)
            table = torch.tensor([[t, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.float32, device=DEV)
            assert torch.equal(got[b], ops.timestep_embed(table, 1, dim, True, 0.0)[0]), f"step {s} row {b} (t = {t})"
    assert len(seen) >= 5


@pytest.mark.gpu
@pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "nocfg"])
def test_slot_start_writes_the_named_slots_only(hip_lib, do_cfg):
    """Slot 0 starts from its own renoise row 0, slot 1 at full strength, slot 2 is a plain panel (latents given): each equals
    redraw_start + prepare_model_input on that panel alone, and a launch over one slot leaves every other slot's bits alone."""
    from diffsensei_amd import ops
    ns, H, W = 3, 10, 12
    HW = H * W
    g = torch.Generator().manual_seed(8)
    rnd = lambda *s: torch.randn(*s, generator=g).half().to(DEV)
    sch = _scheduler(0)
    schedules = [sch.panel_schedule(6, 0.5, 1.0), sch.panel_schedule(4, 1.0, 1.0), sch.panel_schedule(3, 1.0, 1.0)]
    assert schedules[0]["t_start"] == 3
    sigma = [float("nan"), schedules[1]["init_noise_sigma"], float("nan")]
    panel = _load_panel(ns, [(0, 3), (0, 4), (5, 3)], schedules, modes=[0, 1, 2], sigma=sigma)
    x0, nz = rnd(ns, 4, H, W), rnd(ns, 4, H, W)
    rd = ops.redraw_buffer(ns, H, W, DEV)
    ops.redraw_load(rd, x0, nz, torch.ones(ns, H, W), torch.full((2, 2), float("nan")), False, float("nan"))
    rows_b = 2 * ns if do_cfg else ns
    lat, xin = rnd(ns, 4, H, W), rnd(rows_b, HW, 4)

    def reference(n):
        l1 = lat[n:n + 1].clone()
        if n < 2:
            buf = ops.redraw_buffer(1, H, W, DEV)
            ops.redraw_load(buf, x0[n:n + 1], nz[n:n + 1], torch.ones(1, H, W), torch.from_numpy(schedules[n]["renoise_rows"]),
                            full_strength=n == 1, init_noise_sigma=schedules[n]["init_noise_sigma"])
            ops.redraw_start(buf, l1)
        x1 = torch.empty(2 if do_cfg else 1, HW, 4, dtype=torch.float16, device=DEV)
        ops.prepare_model_input(l1, x1, torch.from_numpy(schedules[n]["rows"]).to(DEV), do_cfg)
        return l1[0], x1

    for order in ([1], [0], [2]):
        n = order[0]
        before_l, before_x = lat.clone(), xin.clone()
        want_l, want_x = reference(n)
        ops.panel_slot_start(panel, rd, lat, xin, n, 1, do_cfg)
        assert torch.equal(lat[n], want_l) and torch.equal(xin[n], want_x[0])
        if do_cfg:
            assert torch.equal(xin[ns + n], want_x[1])
        if n == 2:
            assert torch.equal(lat[2], before_l[2]), "a plain panel's latents are the host's"
        else:
            assert not torch.equal(lat[n], before_l[n])
        for k in range(ns):
            if k != n:
                assert torch.equal(lat[k], before_l[k]) and torch.equal(xin[k], before_x[k]), f"slot {k} was touched"
                assert not do_cfg or torch.equal(xin[ns + k], before_x[ns + k])
    # a range of slots, and no redraw buffer at all: every slot keeps its latents
    lat2, xin2 = lat.clone(), torch.zeros_like(xin)
    ops.panel_slot_start(panel, None, lat2, xin2, 0, 3, do_cfg)
    assert torch.equal(lat2, lat) and torch.equal(xin2, xin)
    # an empty slot inside the range has no row 0 to divide by: nothing of it is written
    ops.panel_slot_load(panel, ns, 1, 0, None)
    lat3, xin3 = rnd(ns, 4, H, W), rnd(rows_b, HW, 4)
    keep_l, keep_x = lat3.clone(), xin3.clone()
    ops.panel_slot_start(panel, rd, lat3, xin3, 0, 3, do_cfg)
    assert torch.equal(lat3[1], keep_l[1]) and torch.equal(xin3[1], keep_x[1]) and not torch.equal(xin3[0], keep_x[0])
    assert not do_cfg or torch.equal(xin3[ns + 1], keep_x[ns + 1])
    assert torch.isfinite(lat3).all() and torch.isfinite(xin3).all()


@pytest.mark.gpu
def test_bad_arguments_return_an_error_and_launch_nothing(hip_lib):
    from diffsensei_amd import ops
    lib = hip_lib
    ns, H, W = 2, 4, 4
    panel = ops.panel_schedule_buffer(ns, DEV)
    rows = torch.ones(4, 8, device=DEV)
    ops.panel_slot_load(panel, ns, 0, 0, rows)
    ops.panel_slot_load(panel, ns, 1, 0, rows)
    big = torch.ones(ops.PANEL_MAX_ROWS + 1, 8, device=DEV)
    lat = torch.ones(ns, 4, H, W, dtype=torch.float16, device=DEV)
    xin = torch.ones(2 * ns, H * W, 4, dtype=torch.float16, device=DEV)
    eps = torch.ones(2 * ns, H * W, 4, dtype=torch.float16, device=DEV)
    out = torch.ones(2 * ns, 32, dtype=torch.float16, device=DEV)
    gd = torch.ones(ns, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    keep = panel.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, L, X, E, O, G, T, R = (t.data_ptr() for t in (panel, lat, xin, eps, out, gd, ctr, rows))
    bad = [
        ("steps above the row capacity", lambda: lib.ds_panel_slot_load(P, ns, 0, 0, ops.PANEL_MAX_ROWS + 1, big.data_ptr(), None, None, 2, 1.0, st)),
        ("null buffer", lambda: lib.ds_panel_slot_load(None, ns, 0, 0, 4, R, None, None, 2, 1.0, st)),
        ("misaligned buffer", lambda: lib.ds_panel_slot_load(P + 4, ns, 0, 0, 4, R, None, None, 2, 1.0, st)),
        ("slot outside", lambda: lib.ds_panel_slot_load(P, ns, ns, 0, 4, R, None, None, 2, 1.0, st)),
        ("renoise start without rows", lambda: lib.ds_panel_slot_load(P, ns, 0, 0, 4, R, None, None, 0, 1.0, st)),
        ("step: null buffer", lambda: lib.ds_cfg_sampler_step_slots_f16(E, L, X, None, G, None, None, None, T, ns, H * W, 0, 1, st)),
        ("step: misaligned buffer", lambda: lib.ds_cfg_sampler_step_slots_f16(E, L, X, P + 8, G, None, None, None, T, ns, H * W, 0, 1, st)),
        ("step: no counter", lambda: lib.ds_cfg_sampler_step_slots_f16(E, L, X, P, G, None, None, None, None, ns, H * W, 0, 1, st)),
        ("step: no guidance under cfg", lambda: lib.ds_cfg_sampler_step_slots_f16(E, L, X, P, None, None, None, None, T, ns, H * W, 0, 1, st)),
        ("step: kind 2 without prev_x0", lambda: lib.ds_cfg_sampler_step_slots_f16(E, L, X, P, G, None, None, None, T, ns, H * W, 2, 1, st)),
        ("step: kind 3 without seeds", lambda: lib.ds_cfg_sampler_step_slots_f16(E, L, X, P, G, None, None, None, T, ns, H * W, 3, 1, st)),
        ("step: misaligned redraw buffer", lambda: lib.ds_cfg_sampler_step_slots_f16(E, L, X, P, G, None, None, P + 4, T, ns, H * W, 0, 1, st)),
        ("temb: null buffer", lambda: lib.ds_timestep_embed_slots_f16(None, T, O, 2 * ns, 32, 1, 0.0, ns, st)),
        ("temb: misaligned buffer", lambda: lib.ds_timestep_embed_slots_f16(P + 4, T, O, 2 * ns, 32, 1, 0.0, ns, st)),
        ("temb: rows not whole groups", lambda: lib.ds_timestep_embed_slots_f16(P, T, O, 3, 32, 1, 0.0, ns, st)),
        ("start: null buffer", lambda: lib.ds_panel_slot_start_f16(None, None, L, X, ns, H * W, 1, 0, 1, st)),
        ("start: misaligned buffer", lambda: lib.ds_panel_slot_start_f16(P + 4, None, L, X, ns, H * W, 1, 0, 1, st)),
        ("start: slots outside", lambda: lib.ds_panel_slot_start_f16(P, None, L, X, ns, H * W, 1, 1, 2, st)),
    ]
    for what, call in bad:
        assert call() != 0, f"{what}: accepted"
        assert lib.ds_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(panel, keep)
    for t in (lat, xin, out):
        assert bool((t == 1).all()), "a refused call launched something"
    assert int(lib.ds_panel_schedule_bytes(ns)) == panel.numel() == ((8 * ns + 15) & ~15) + 4 * ns * (4 + 16 * 1024 + 2 * 1025)
    with pytest.raises(ValueError):
        ops.panel_slot_load(panel, ns, 0, 0, torch.ones(4, 7))
    with pytest.raises(Exception, match="capacity"):
        ops.panel_slot_load(panel, ns, 0, 0, big)
