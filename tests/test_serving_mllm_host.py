"""CPU: MLLM-conditioned requests in the request front-end (diffsensei_amd/serving.py) with recording stand-ins for the
pipeline, the agent and the pre-pass: they are decoded in groups of at most `agent.llm.max_sequences`, replaced by
`ip_image_embeds` requests before the UNet batches are planned, and everything else takes the path it took before."""
import pytest

from diffsensei_amd.serving import BucketBatcher, plan_batches


class _Llm:
    max_sequences = 4


class _Agent:
    llm = _Llm()


class _Pipe:
    def __init__(self):
        self.calls = []

    def generate_batch(self, requests, output_type="pil"):
        self.calls.append([dict(r) for r in requests])
        return [f"{r['tag']}:{output_type}" for r in requests]


def _req(size, tag, **kw):
    return dict(prompt="p", height=size, width=size, num_inference_steps=50, guidance_scale=7.5, num_samples=1, tag=tag, **kw)


def _mllm(tag, **kw):
    return dict(input_ids=f"ids-{tag}", ids_cmp_mask=f"mask-{tag}", mllm_scale=0.5, **kw)


def _batcher(**kw):
    pipe, seen = _Pipe(), []

    def prepass(p, agent, requests, **shared):
        assert p is pipe and isinstance(agent, _Agent)
        seen.append(([r["input_ids"] for r in requests], shared))
        assert all(set(r) == {"input_ids", "ids_cmp_mask", "mllm_scale", "ip_images"} for r in requests)
        return [f"emb-{r['input_ids'][4:]}" for r in requests]

    return BucketBatcher(pipe, agent=_Agent(), prepass=prepass, **kw), pipe, seen


def test_mllm_requests_are_grouped_and_replaced_before_planning():
    b, pipe, seen = _batcher(max_panels=4)
    tags = "abcdefghij"
    tickets = []
    for k, t in enumerate(tags):
        if k in (1, 5):                                                         # two plain requests in between
            tickets.append(b.submit(**_req(512, t, ip_images=[f"img-{t}"])))
        else:
            tickets.append(b.submit(**_req(512 if k % 2 else 1024, t, ip_images=[f"img-{t}"], mllm=_mllm(t))))
    assert tickets == list(range(10))
    out = b.run(output_type="pt")
    assert out == [f"{t}:pt" for t in tags], "tickets keep their order"
    assert [ids for ids, _ in seen] == [["ids-a", "ids-c", "ids-d", "ids-e"], ["ids-g", "ids-h", "ids-i", "ids-j"]]
    assert b.last_prepass == [[0, 2, 3, 4], [6, 7, 8, 9]] and all(len(g) <= _Llm.max_sequences for g in b.last_prepass)
    served = {r["tag"]: r for call in pipe.calls for r in call}
    for k, t in enumerate(tags):
        r = served[t]
        assert "mllm" not in r
        if k in (1, 5):
            assert r["ip_images"] == [f"img-{t}"] and "ip_image_embeds" not in r
        else:
            assert r["ip_images"] == [] and r["ip_image_embeds"] == f"emb-{t}"
    # the UNet plan is the plan of the replaced requests
    flat = [dict(_req(512 if (k % 2 or k in (1, 5)) else 1024, t)) for k, t in enumerate(tags)]
    assert b.last_plan == plan_batches(flat, 4, 32 * 1024 * 1024, False)
    assert all(len(call) <= 4 for call in pipe.calls)


def test_shared_decode_arguments_split_groups():
    b, pipe, seen = _batcher()
    for t, kw in zip("abcd", [dict(eos_token_id=2), dict(eos_token_id=2), dict(eos_token_id=9), dict(eos_token_id=2)]):
        b.submit(**_req(512, t, ip_images=[t], mllm=_mllm(t, img_ids_list=[5, 6, 7], **kw)))
    assert b.run() == [f"{t}:pil" for t in "abcd"]
    assert [(ids, sh["eos_token_id"], sh["img_ids_list"]) for ids, sh in seen] == \
        [(["ids-a", "ids-b", "ids-d"], 2, [5, 6, 7]), (["ids-c"], 9, [5, 6, 7])]


def test_mllm_needs_an_agent_and_its_fields():
    with pytest.raises(ValueError):
        BucketBatcher(_Pipe()).submit(**_req(512, "a", ip_images=["x"], mllm=_mllm("a")))
    b, _, _ = _batcher()
    with pytest.raises(ValueError):
        b.submit(**_req(512, "a", ip_images=["x"], mllm=dict(input_ids="i", ids_cmp_mask="m")))
    with pytest.raises(ValueError):
        b.submit(**_req(512, "a", ip_image_embeds="e", mllm=_mllm("a")))
    assert len(b) == 0


def test_queue_without_mllm_is_planned_as_before():
    reqs = [_req(512, "a"), _req(1024, "b"), _req(512, "c"), _req(512, "d")]
    plain, with_agent = BucketBatcher(_Pipe(), max_panels=2), _batcher(max_panels=2)
    b, pipe, seen = with_agent
    for r in reqs:
        plain.submit(**r)
        b.submit(**r)
    assert plain.run() == b.run()
    assert b.last_plan == plain.last_plan == [[1], [0, 2], [3]]
    assert seen == [] and b.last_prepass == []
    assert pipe.calls == plain.pipe.calls
