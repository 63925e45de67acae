"""CPU: `mix_scales` of the request front-end (diffsensei_amd/serving.py) - requests that differ only in guidance_scale /
ip_scale share a UNet batch, classifier-free guidance on / off still separates them, the default key and the
max_panels / max_pixels packing are what they were, and every request reaches the pipeline with its own values."""
import pytest

from diffsensei_amd.serving import BucketBatcher, bucket_key, plan_batches

PAIRS = [(3.0, 0.4), (5.0, 0.6), (7.5, 1.0), (9.0, 0.0)]


def _req(size=1024, n=1, g=5.0, s=1.0, steps=20, **kw):
    return dict(prompt="p", height=size, width=size, num_inference_steps=steps, num_samples=n, guidance_scale=g, ip_scale=s, **kw)


def _queue():
    return [_req(g=PAIRS[i % 4][0], s=PAIRS[i % 4][1]) for i in range(8)]


def test_eight_requests_with_four_slider_pairs_share_one_batch():
    reqs = _queue()
    assert plan_batches(reqs, max_panels=32, mix_scales=True) == [list(range(8))]
    assert plan_batches(reqs, max_panels=32) == [[0, 4], [1, 5], [2, 6], [3, 7]]          # the default: one bucket per pair
    assert plan_batches(reqs, max_panels=32, mix_scales=False) == plan_batches(reqs, max_panels=32)
    assert bucket_key(reqs[0]) == (1024, 1024, 20, 3.0, 0.4)                                # the default key is unchanged
    assert bucket_key(reqs[0], mix_scales=True) == (1024, 1024, 20, True)
    assert {bucket_key(r, True) for r in reqs} == {(1024, 1024, 20, True)}


def test_cfg_off_is_never_batched_with_cfg_on():
    reqs = [_req(g=5.0), _req(g=1.0), _req(g=7.5), _req(g=0.5), _req(g=1.0001), _req(g=[0.5, 1.0], n=2)]   # the last: both off
    plan = plan_batches(reqs, max_panels=32, mix_scales=True)
    assert sorted(plan) == [[0, 2, 4], [1, 3, 5]]
    for b in plan:
        assert len({max(r["guidance_scale"]) > 1 if isinstance(r["guidance_scale"], list) else r["guidance_scale"] > 1
                    for r in (reqs[i] for i in b)}) == 1
    assert bucket_key(_req(g=[3.0, 7.5], n=2), True) == bucket_key(_req(g=5.0), True)       # a sweep request mixes in too
    assert bucket_key(_req(g=[3.0, 7.5], s=(0.4, 1.0), n=2)) == (1024, 1024, 20, (3.0, 7.5), (0.4, 1.0))   # hashable by default


def test_size_and_steps_still_separate_and_packing_is_unchanged():
    reqs = [_req(512, g=3.0), _req(1024, g=5.0), _req(512, g=7.5), _req(1024, g=7.5, steps=30), _req(1024, g=9.0)]
    assert plan_batches(reqs, max_panels=32, mix_scales=True) == [[1, 4], [3], [0, 2]]      # largest first, steps apart
    # max_panels: 8 mixed requests of 3 panels, at most 8 panels per batch -> 2 + 2 + 2 + 2, submission order kept
    reqs = [_req(n=3, g=PAIRS[i % 4][0], s=PAIRS[i % 4][1]) for i in range(8)]
    assert plan_batches(reqs, max_panels=8, mix_scales=True) == [[0, 1], [2, 3], [4, 5], [6, 7]]
    same = [_req(n=3) for _ in range(8)]
    assert plan_batches(reqs, max_panels=8, mix_scales=True) == plan_batches(same, max_panels=8)
    # max_pixels: 2048^2 requests under a 32 Mpx cap -> 8 panels per batch, whatever their sliders
    reqs = [_req(2048, n=2, g=PAIRS[i % 4][0], s=PAIRS[i % 4][1]) for i in range(6)]
    same = [_req(2048, n=2) for _ in range(6)]
    want = [[0, 1, 2, 3], [4, 5]]
    assert plan_batches(reqs, 32, 32 * 1024 * 1024, mix_scales=True) == want == plan_batches(same, 32, 32 * 1024 * 1024)
    with pytest.raises(ValueError):
        plan_batches([_req(n=9)], max_panels=8, mix_scales=True)


def test_batcher_hands_each_request_its_own_values():
    class Stub:
        def __init__(self):
            self.calls = []

        def generate_batch(self, requests, output_type="pil"):
            self.calls.append([(r["guidance_scale"], r["ip_scale"]) for r in requests])
            return [(r["tag"], r["guidance_scale"], r["ip_scale"]) for r in requests]

    class Pipe(Stub):
        def generate_batch(self, requests, output_type="pil"):
            return Stub.generate_batch(self, [dict(r, tag=r.pop("prompt")) for r in map(dict, requests)], output_type)

    pipe = Pipe()
    b = BucketBatcher(pipe, max_panels=32, mix_scales=True)
    tickets = [b.submit(**dict(r, prompt=f"r{i}")) for i, r in enumerate(_queue())]
    out = b.run(output_type="latent")
    assert b.last_plan == [list(range(8))] and len(pipe.calls) == 1
    assert pipe.calls[0] == [PAIRS[i % 4] for i in range(8)]
    for t in tickets:
        assert out[t] == (f"r{t}", *PAIRS[t % 4])
    pipe2 = Pipe()
    b = BucketBatcher(pipe2, max_panels=32)                                                 # default: four batches, as today
    for i, r in enumerate(_queue()):
        b.submit(**dict(r, prompt=f"r{i}"))
    out = b.run()
    assert len(pipe2.calls) == 4 and all(len(set(c)) == 1 for c in pipe2.calls)
    assert [o[1:] for o in out] == [PAIRS[i % 4] for i in range(8)]


def test_slider_values_of_any_real_type_and_requests_no_batch_can_hold():
    import numpy as np
    import torch
    assert bucket_key(_req(g=np.float32(5.0), s=torch.tensor(0.5))) == (1024, 1024, 20, 5.0, 0.5)
    assert bucket_key(_req(g=np.float64(7.5)), mix_scales=True) == (1024, 1024, 20, True)
    with pytest.raises(ValueError):
        bucket_key(_req(g=[0.5, 5.0], n=2), mix_scales=True)
    b = BucketBatcher(object(), mix_scales=True)
    b.submit(**_req(g=3.0))
    with pytest.raises(ValueError):
        b.submit(**_req(g=[0.5, 5.0], n=2))          # refused alone, at submit: the queued request is not taken down with it
    assert len(b) == 1
