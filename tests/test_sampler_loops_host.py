"""CPU: the sampling loops run free over a denoiser whose answer is known in closed form (tests/_loop_cases.py).

* The float64 loops of the scheduler restatements (oracle/scheduler_ref.py, tests/_dpm_ref.py) converge to the closed form at
  their order - the first pin on the restatements that is not itself a restatement - and the project's own host tables
  (`coef_table`, `solver_table`), interpreted in float64, land on the same loop.
* D_emul(kind, cfg) = rel-L2(fp16-storage emulation, float64 loop) after 50 free steps is the yardstick of the GPU gates in
  tests/test_gpu_sampler_loops.py (<= 2 * D_emul).  It is computed here, bounded (<= 5e-3: otherwise the input is badly chosen
  and a gate built on it says nothing) and shown to be sensitive: a truncating conversion of the stored latents - inside the
  lock-step tolerance 1.5e-3 * max|x| at every single step - leaves the 2 * D_emul band over 50 steps.
"""
import pytest
import torch

from tests import _loop_cases as L

CFG = pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "nocfg"])
LOCK_STEP_TOL = 1.5e-3          # tests/_sampler_common._close, per step


@CFG
@pytest.mark.parametrize("kind", [0, 1])
def test_euler_and_ddim_restatements_are_first_order(kind, do_cfg):
    err = {n: L.d_closed(kind, do_cfg, n) for n in (25, 50, 100)}
    print(f"{L.KINDS[kind]} cfg={do_cfg}: float64 loop vs closed form {err}")
    for n in (25, 50):
        ratio = err[n] / err[2 * n]
        assert 1.6 <= ratio <= 2.4, f"{L.KINDS[kind]}: err({n}) / err({2 * n}) = {ratio:.3f}"


@CFG
def test_dpm_restatement_converges_and_beats_euler(do_cfg):
    dpm = {n: L.d_closed(2, do_cfg, n) for n in (25, 50, 100)}
    euler = {n: L.d_closed(0, do_cfg, n) for n in (25, 50, 100)}
    print(f"cfg={do_cfg}: DPM-Solver++ 2M {dpm}, Euler {euler}")
    assert dpm[25] > dpm[50] > dpm[100]
    for n in (25, 50, 100):
        assert dpm[n] < euler[n], (n, dpm[n], euler[n])


@CFG
@pytest.mark.parametrize("n", [25, 50, 100])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_host_scheduler_tables_run_the_restatements_loop(kind, n, do_cfg):
    """`coef_table` / `solver_table` through the float64 row interpreter vs the restatement's float64 loop: 1e-6 relative.
    All n rows, both c_in_div columns, the guidance column, the solver rows and (kind 3) the per-step noise index enter."""
    d = L.rel(L.run_table_loop(kind, n, do_cfg), L.f64_loop(kind, do_cfg, n))
    print(f"{L.KINDS[kind]} n={n} cfg={do_cfg}: host tables vs restatement {d:.3e}")
    assert d <= 1e-6


@CFG
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_fp16_storage_emulation_stays_near_the_float64_loop(kind, do_cfg):
    d = L.d_emul(kind, do_cfg)
    print(f"D_emul({L.KINDS[kind]}, cfg={do_cfg}) = {d:.3e}")
    assert 0.0 < d <= 5e-3


@CFG
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_truncated_latents_leave_the_gate_but_not_the_lock_step_tolerance(kind, do_cfg):
    """The latents' rounding hook swapped for truncation toward zero: every single step stays inside the lock-step tolerance,
    the 50-step distance to the float64 loop exceeds the 2 * D_emul gate of the GPU tests."""
    per_step = []

    def q_lat(y):
        t, h = L.trunc16(y), L.h16(y)
        per_step.append(float((t - h).abs().max() / h.abs().max()))
        return t

    x = L.run_loop(kind, L.STEPS, do_cfg, emulate=True, q_lat=q_lat)[0]
    d, gate = L.rel(x, L.f64_loop(kind, do_cfg)), 2 * L.d_emul(kind, do_cfg)
    print(f"{L.KINDS[kind]} cfg={do_cfg}: truncated latents {d:.3e} = {d / gate * 2:.1f} x D_emul; worst single step "
          f"{max(per_step):.3e} of max|x|")
    assert len(per_step) == L.STEPS and max(per_step) <= LOCK_STEP_TOL
    assert d > gate


def test_trunc16_truncates():
    x = torch.tensor([1.0 + 2.0 ** -10 * 0.75, -(1.0 + 2.0 ** -10 * 0.75), 0.1, -0.1, 3.0, 0.0], dtype=torch.float64)
    t = L.trunc16(x)
    assert t[0] == 1.0 and t[1] == -1.0 and t[4] == 3.0 and t[5] == 0.0
    assert (t.abs() <= x.abs()).all() and ((t - x).abs() < 2.0 ** -10 * x.abs().clamp_min(1e-30) + 1e-30).all()
    assert torch.equal(t, t.half().double())


def test_closed_form_is_the_ode_solution():
    """The closed form against the denoiser itself: d x / d sigma = eps at an interior sigma (central difference), so the
    two formulas of tests/_loop_cases.py pin each other."""
    c = L.case()
    mu, s0, sg, dh = c.mu(True), 14.0, 2.5, 1e-5
    x0 = c.start(0, s0, True)
    xs = lambda s: mu + (x0 - mu) * ((L.S ** 2 + s * s) / (L.S ** 2 + s0 * s0)) ** 0.5
    dxds = (xs(sg + dh) - xs(sg - dh)) / (2 * dh)
    eps = L.eps_ideal(xs(sg) / (1 + sg * sg) ** 0.5, sg, mu)
    assert L.rel(dxds, eps) <= 1e-8
