"""CPU: the per-panel flag belongs to the launch plan (engine.UNetEngine.per_panel).  Built over CPU buffers, nothing is
launched: a fresh engine's plans are op for op the one-scalar plans (IP_ATTN i[10] = 0 reading the first of B equal
floats, SAMPLER_STEP with a null guidance pointer), and `enable_per_panel` flips exactly those two things, once."""
import pytest
import torch


@pytest.fixture(scope="module")
def packed(hip_lib):
    from diffsensei_amd.engine import PackedUNet
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    cfg = tiny_config()
    return PackedUNet(cfg, random_state_dict(cfg, 0), torch.device("cpu"))


def _fields(op):
    return (op.code, list(op.i), list(op.f), list(op.l), list(op.p))


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_uniform_plan_is_unchanged_and_the_switch_touches_two_fields(packed, kind):
    from diffsensei_amd._lib import OP
    from diffsensei_amd.engine import UNetEngine
    eng = UNetEngine(packed, 4, 16, 16)
    assert tuple(eng.ip_scale.shape) == (4,) and not eng.per_panel and eng.guidance is None
    ip = [op for op in eng.forward_ops if op.code == OP["IP_ATTN"]]
    assert ip and all(op.i[10] == 0 and op.p[7] == eng.ip_scale.data_ptr() for op in ip)
    eng.build_sampler(2, kind, True)
    before = [_fields(op) for op in eng.forward_ops]
    n_step = eng.step_plan.n
    assert n_step == len(eng.forward_ops) + 2
    eng.latents.fill_(0.25)
    buffers = (eng.latents, eng.guidance, eng.prev_x0, eng.noise_seeds)
    eng.enable_per_panel()
    assert eng.per_panel and tuple(eng.guidance.shape) == (2,) and eng.guidance.dtype == torch.float32
    # the switch allocates nothing: what the host wrote before it (the latents, say) is what the new step plan reads
    assert all(a is b for a, b in zip(buffers, (eng.latents, eng.guidance, eng.prev_x0, eng.noise_seeds)))
    assert (eng.latents == 0.25).all()
    assert eng.step_plan.n == n_step and eng.forward_plan.n == len(eng.forward_ops) and not eng.step_plan.captured
    for b, op in zip(before, eng.forward_ops):
        if op.code == OP["IP_ATTN"]:
            assert op.i[10] == 1 and op.p[7] == eng.ip_scale.data_ptr()
            b[1][10] = 1
        assert _fields(op) == b
    plan = eng.step_plan
    eng.enable_per_panel()                                   # sticky and idempotent: nothing is rebuilt
    eng.build_sampler(2, kind, True)
    assert eng.step_plan is plan


def test_scale_values_are_a_number_or_exactly_n(packed):
    from diffsensei_amd.engine import UNetEngine
    f = UNetEngine._scale_values
    assert f(0.6, 4, "x") is None and f(1, 4, "x") is None and f(torch.tensor(0.5), 4, "x") is None
    assert f([0.4, 1.0], 2, "x") == [0.4, 1.0] and f(torch.tensor([0.5, 2.0]), 2, "x") == [0.5, 2.0]
    with pytest.raises(ValueError):
        f([0.4, 1.0, 2.0], 2, "x")


def test_load_schedule_guidance_on_both_kinds_of_plan(packed):
    """`load_schedule(guidance=)`: equal values on a uniform plan go to column 7; differing values switch the plans and
    land in the vector - after everything else was checked, so a refused call changes nothing; on per-panel plans a call
    WITHOUT a vector writes column 7's value for every panel, because the step no longer reads the column."""
    import numpy as np
    from diffsensei_amd.engine import UNetEngine
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(3)
    table = torch.from_numpy(sch.coef_table(7.5))
    eng = UNetEngine(packed, 4, 16, 16)
    eng.load_schedule(table)                                  # no sampler built, no vector: as before
    with pytest.raises(ValueError):
        eng.load_schedule(table, guidance=[3.0, 5.0])         # a vector needs the sampler's panel count
    eng.build_sampler(2, 0, True)
    eng.latents.fill_(0.5)
    eng.load_schedule(table, guidance=[3.0, 3.0])
    assert not eng.per_panel and (eng.table[:3, 7] == 3.0).all()
    eng.load_schedule(table, guidance=np.float32(4.0))
    assert not eng.per_panel and (eng.table[:3, 7] == 4.0).all()
    for bad in (dict(solver_rows=table), dict(noise_seeds=[1, 2]), dict(guidance=[3.0, 5.0, 7.0])):
        with pytest.raises(ValueError):
            eng.load_schedule(table, **dict(dict(guidance=[3.0, 5.0]), **bad))
        assert not eng.per_panel and (eng.table[:3, 7] == 4.0).all()
    eng.load_schedule(table, guidance=[3.0, 5.0])
    assert eng.per_panel and eng.guidance.tolist() == [3.0, 5.0] and (eng.latents == 0.5).all()
    eng.load_schedule(table)
    assert eng.guidance.tolist() == [7.5, 7.5]
    eng.load_schedule(table, guidance=2.0)
    assert eng.guidance.tolist() == [2.0, 2.0]
