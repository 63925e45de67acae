"""CPU: the host side of continuous batching - `serving.plan_continuous` (the admission timeline `generate_continuous`
executes), the per-panel scheduler tables (`_Scheduler.panel_schedule`) and `BucketBatcher(continuous=True)`."""
import math
import random

import numpy as np
import pytest
import torch

from tests._sampler_common import SDXL


def _schedulers():
    from diffsensei_amd import schedulers as S
    return [S.EulerDiscreteScheduler(**SDXL), S.DDIMScheduler(**SDXL), S.DPMSolverMultistepScheduler(**SDXL),
            S.EulerAncestralDiscreteScheduler(**SDXL)]


def test_plan_continuous_hand_checked_case():
    """slots 2, one panel each, steps [4, 2, 2]: A and B start at step 0, C takes B's slot at step 2; 4 forwards, no idle slot
    step - where the bucketed plan (one batch per step count) needs 4 + 2 = 6 forwards."""
    from diffsensei_amd.serving import plan_batches, plan_continuous
    plan = plan_continuous([4, 2, 2], [1, 1, 1], 2)
    assert plan["admissions"] == [(0, 0, [0]), (0, 1, [1]), (2, 2, [1])]
    assert plan["forwards"] == 4 and plan["idle_slot_steps"] == 0 and plan["slot_steps"] == 8
    assert plan["finish"] == [4, 2, 4]
    reqs = [dict(height=128, width=128, num_inference_steps=n) for n in (4, 2, 2)]
    batches = plan_batches(reqs, 2)
    assert sorted(map(sorted, batches)) == [[0], [1, 2]]
    assert sum(reqs[b[0]]["num_inference_steps"] for b in batches) == 6


@pytest.mark.parametrize("seed", range(8))
def test_plan_continuous_random_queues(seed):
    from diffsensei_amd.serving import plan_continuous
    rng = random.Random(seed)
    slots = rng.randint(3, 9)
    n = rng.randint(1, 24)
    steps = [rng.randint(1, 12) for _ in range(n)]
    panels = [rng.randint(1, 3) for _ in range(n)]
    plan = plan_continuous(steps, panels, slots)
    adm = plan["admissions"]
    assert [r for _, r, _ in adm] == list(range(n)), "admission order is submission order"
    assert [s for s, _, _ in adm] == sorted(s for s, _, _ in adm)
    owner = {}                                                   # (slot, global step) -> request
    for s, r, sl in adm:
        assert len(sl) == panels[r] == len(set(sl)) and all(0 <= q < slots for q in sl)
        assert plan["finish"][r] == s + steps[r], "exactly its steps, consecutively, from its admission on"
        for q in sl:
            for t in range(s, s + steps[r]):
                assert (q, t) not in owner, f"slot {q} holds requests {owner.get((q, t))} and {r} at step {t}"
                owner[(q, t)] = r
    assert plan["forwards"] == max(plan["finish"])
    assert plan["slot_steps"] == sum(a * b for a, b in zip(steps, panels)) == len(owner)
    assert plan["forwards"] >= math.ceil(plan["slot_steps"] / slots)
    assert plan["idle_slot_steps"] == plan["forwards"] * slots - plan["slot_steps"] >= 0
    # the head of the queue is admitted at the FIRST boundary with enough free slots: one boundary earlier it did not fit
    for k, (s, r, sl) in enumerate(adm):
        lo = adm[k - 1][0] if k else 0                           # it cannot overtake the request in front of it
        for t in range(lo, s):
            busy = {q for (q, tt), rr in owner.items() if tt == t and rr < r}
            assert slots - len(busy) < panels[r], f"request {r} would have fitted at step {t}, was admitted at {s}"


def test_plan_continuous_refusals():
    from diffsensei_amd.serving import plan_continuous
    with pytest.raises(ValueError, match="exceeds"):
        plan_continuous([3, 3], [1, 3], 2)
    with pytest.raises(ValueError):
        plan_continuous([0], [1], 2)
    with pytest.raises(ValueError):
        plan_continuous([1], [1], 0)
    assert plan_continuous([], [], 4)["forwards"] == 0


@pytest.mark.parametrize("steps", [5, 8])
@pytest.mark.parametrize("strength", [1.0, 0.5])
@pytest.mark.parametrize("which", range(4))
def test_panel_schedule_is_the_sliced_tables_and_leaves_the_scheduler_alone(which, steps, strength):
    sch = _schedulers()[which]
    sch.set_timesteps(7)                                         # another request's schedule is "in flight"
    before = {k: (v.clone() if torch.is_tensor(v) else np.array(v, copy=True) if isinstance(v, np.ndarray) else v)
              for k, v in vars(sch).items()}
    got = sch.panel_schedule(steps, strength, guidance_scale=3.5)
    for k, v in before.items():                                  # timesteps, sigmas, num_inference_steps, counters: all as found
        now = getattr(sch, k)
        same = torch.equal(now, v) if torch.is_tensor(v) else (np.array_equal(now, v) if isinstance(v, np.ndarray) else now == v)
        assert same, f"panel_schedule changed the scheduler's `{k}`"
    assert set(vars(sch)) == set(before)
    ref = _schedulers()[which]
    ref.set_timesteps(steps)
    t0 = ref.start_index(strength)
    assert got["t_start"] == t0 and got["steps"] == steps - t0 >= 1
    assert np.array_equal(got["rows"], ref.coef_table(3.5)[t0:])
    solver = ref.solver_table(start=t0) if t0 else ref.solver_table()
    assert (got["solver_rows"] is None) == (solver is None)
    if solver is not None:
        assert np.array_equal(got["solver_rows"], solver) and got["solver_rows"][0, 0] == 1.0
    assert np.array_equal(got["renoise_rows"], ref.renoise_table()[t0:]) and got["renoise_rows"].shape == (steps - t0 + 1, 2)
    assert got["init_noise_sigma"] == float(ref.init_noise_sigma)
    assert np.array_equal(got["timesteps"], np.asarray(ref.timesteps_np)[t0:])


class _FakePipe:
    def __init__(self):
        self.calls = []

    def generate_batch(self, requests, output_type="pil"):
        self.calls.append(("batch", [r["tag"] for r in requests]))
        return [[r["tag"]] for r in requests]

    def generate_continuous(self, requests, slots, output_type="pil"):
        self.calls.append(("continuous", [r["tag"] for r in requests], slots))
        return [[r["tag"]] for r in requests]

    def hold_adapters(self):
        import contextlib
        return contextlib.nullcontext()


def _queue():
    q = []
    for k, (hw, steps, g, extra) in enumerate([
            ((1024, 1024), 20, 5.0, {}), ((512, 512), 30, 5.0, {}), ((1024, 1024), 50, 7.0, {}),
            ((1024, 1024), 30, 1.0, {}), ((512, 512), 20, 3.0, {"num_samples": 3}),
            ((1024, 1024), 30, 5.0, {"redraw_latents": torch.zeros(1, 4, 128, 128), "redraw_bbox": [[0, 0, 1, 1]], "strength": 0.5}),
            ((1024, 1024), 20, 5.0, {"lora": {"a": 1.0}})]):
        q.append(dict(tag=k, prompt="p", height=hw[0], width=hw[1], num_inference_steps=steps, guidance_scale=g, **extra))
    return q


def test_bucket_batcher_continuous_groups_and_slots():
    """Groups by (height, width, guidance side, lora), largest resolution first, submission order inside a group; `slots` is
    the cap `plan_batches` computes from max_panels and max_pixels."""
    from diffsensei_amd.serving import BucketBatcher
    pipe = _FakePipe()
    b = BucketBatcher(pipe, max_panels=16, max_pixels=8 * 1024 * 1024, continuous=True)
    tickets = [b.submit(**r) for r in _queue()]
    res = b.run(output_type="latent")
    assert [r[0] for r in res] == tickets
    assert all(c[0] == "continuous" for c in pipe.calls)
    got = [(c[1], c[2]) for c in pipe.calls]
    # 1024^2: cap = min(16, 8 Mpx / 1 Mpx) = 8 slots; steps 20 / 50 / 30 and the strength-0.5 redraw share one run
    assert ([0, 2, 5], 8) in got and ([3], 8) in got and ([6], 8) in got
    assert ([1, 4], 16) in got                                  # 512^2: 32 would fit the pixels, max_panels caps at 16
    assert len(got) == 4 and [c[1] for c in pipe.calls][-1] == [1, 4], "largest resolution first"
    assert b.last_plan == [c[1] for c in pipe.calls] and b.last_slots == [c[2] for c in pipe.calls]
    with pytest.raises(ValueError, match="max_panels"):
        b2 = BucketBatcher(pipe, max_panels=2, continuous=True)
        b2.submit(tag=0, prompt="p", height=512, width=512, num_samples=3)
        b2.run()


def test_bucket_batcher_default_is_todays_plan():
    from diffsensei_amd.serving import BucketBatcher, plan_batches
    reqs = [r for r in _queue() if "lora" not in r]
    pipe = _FakePipe()
    b = BucketBatcher(pipe, max_panels=16, max_pixels=8 * 1024 * 1024)
    assert b.continuous is False
    for r in reqs:
        b.submit(**r)
    b.run()
    assert b.last_plan == plan_batches(reqs, 16, 8 * 1024 * 1024, False)
    assert [c[0] for c in pipe.calls] == ["batch"] * len(b.last_plan) and [c[1] for c in pipe.calls] == b.last_plan
