"""GPU: `DiffSenseiPipeline.generate_continuous` - per-panel schedules, slots refilled in flight - on the tiny pipeline of
tests/test_gpu_per_panel_scales.py (latents 16 x 16, UNet batch 4 at slots = 2).

A request that ran in slot q of a continuous run equals row q of a uniform `generate_batch` of its own step count,
`torch.equal`: per panel the arithmetic is the same instruction sequence on the same operands, whatever the other slot is
doing and whenever the request was admitted."""
import pytest
import torch

from tests._gates import gate
from tests._sampler_common import SDXL
from tests.test_gpu_per_panel_scales import _clone, _oracle, _rel, pipe  # noqa: F401  (`pipe` is the fixture)

SCHEDULERS = ["EulerDiscreteScheduler", "DDIMScheduler", "DPMSolverMultistepScheduler", "EulerAncestralDiscreteScheduler"]
_REFS = {}


def _set_scheduler(p, name):
    from diffsensei_amd import schedulers as S
    p.scheduler = getattr(S, name)() if name in ("EulerDiscreteScheduler", "DDIMScheduler") else getattr(S, name)(**SDXL)


def _third(A, cfg):
    """request C: its own embeddings, latents, boxes, guidance and IP scale"""
    g = torch.Generator().manual_seed(77)
    return _clone(A, prompt_embeds=torch.randn(1, 77, cfg.cross_attention_dim, generator=g).half(),
                  pooled_prompt_embeds=torch.randn(1, 128, generator=g).half(), latents=torch.randn(1, 4, 16, 16, generator=g).half(),
                  ip_bbox=[[0.3, 0.2, 0.9, 0.8]], dialog_bbox=[[0.5, 0.6, 0.9, 0.9]], guidance_scale=4.5, ip_scale=0.7)


def _queue(p, A, B, cfg):
    seeds = (lambda k: dict(noise_seeds=[k])) if p.scheduler.stochastic else (lambda k: {})
    a = _clone(A, num_inference_steps=4, **seeds(5))
    b = _clone(B, num_inference_steps=2, **seeds(6))
    c = dict(_third(A, cfg), num_inference_steps=2, **seeds(7))
    return a, b, c


def _references(p, name, A, B, cfg):
    """X equals row q of generate_batch over two requests of X's step count; X' is the OTHER kind of request at X's steps."""
    if name not in _REFS:
        a, b, c = _queue(p, A, B, cfg)
        ref = lambda first, second: p.generate_batch([_clone(first), _clone(second)], output_type="latent")
        _REFS[name] = (ref(a, dict(b, num_inference_steps=4))[0], ref(dict(a, num_inference_steps=2), b)[1],
                       ref(dict(a, num_inference_steps=2), c)[1])
    return _REFS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", SCHEDULERS)
def test_refilled_slots_equal_uniform_batches(pipe, name, use_graph):
    """slots = 2: A (4 steps) and B (2) start at step 0, C (2) takes B's slot at step 2."""
    from diffsensei_amd.engine import Plan
    from diffsensei_amd.serving import plan_continuous
    p, cfg, sd, rs, clip, mae, A, B = pipe
    old, old_graph = p.scheduler, p.use_graph
    captures = []
    capture = Plan.capture
    try:
        _set_scheduler(p, name)
        want = _references(p, name, A, B, cfg)
        p.use_graph = use_graph
        Plan.capture = lambda self, stream: (captures.append(self), capture(self, stream))[1]
        out = p.generate_continuous([_clone(r) for r in _queue(p, A, B, cfg)], slots=2, output_type="latent")
        info = dict(p.last_run_info)
    finally:
        Plan.capture = capture
        p.scheduler, p.use_graph = old, old_graph
    assert info["continuous"] == plan_continuous([4, 2, 2], [1, 1, 1], 2)
    assert info["continuous"]["admissions"] == [(0, 0, [0]), (0, 1, [1]), (2, 2, [1])]
    assert info["continuous"]["forwards"] == 4 and info["continuous"]["idle_slot_steps"] == 0 and info["batch"] == 4
    assert info["graph"] == use_graph
    eng = p.unet.engine(4, 16, 16, 1.0)
    assert [c for c in captures if c is eng.step_plan] == ([eng.step_plan] if use_graph else []), "one capture serves the whole run"
    for tag, o, w in zip("ABC", out, want):
        assert o.shape == (1, 4, 16, 16) and torch.isfinite(o).all()
        assert torch.equal(o, w), f"{name}: request {tag} differs from its uniform batch (max |d| {float((o.float() - w.float()).abs().max()):.3g})"
    assert not torch.equal(out[1], out[2])


@pytest.mark.gpu
def test_plain_and_redraw_share_the_slots(pipe):
    """A plain 4-step request and a redraw of strength 0.5 over 4 steps (2 run) in one run: each equals its own uniform
    generate_batch, and what the redraw keeps are the bits of its `redraw_latents`."""
    p, cfg, sd, rs, clip, mae, A, B = pipe
    g = torch.Generator().manual_seed(21)
    kept = torch.randn(1, 4, 16, 16, generator=g).half()
    box = [[0.25, 0.25, 0.75, 0.75]]
    plain = _clone(A, num_inference_steps=4)
    redraw = _clone(B, num_inference_steps=4, redraw_latents=kept, redraw_bbox=box, strength=0.5)
    out = p.generate_continuous([_clone(plain), _clone(redraw)], slots=2, output_type="latent")
    info = p.last_run_info["continuous"]
    assert info["admissions"] == [(0, 0, [0]), (0, 1, [1])] and info["forwards"] == 4 and info["idle_slot_steps"] == 2
    want_plain = p.generate_batch([_clone(plain), _clone(B, num_inference_steps=4)], output_type="latent")[0]
    other = _clone(A, num_inference_steps=4, redraw_latents=kept.flip(-1), redraw_bbox=[[0.0, 0.0, 0.5, 0.5]], strength=0.5)
    want_redraw = p.generate_batch([other, _clone(redraw)], output_type="latent")[1]
    assert torch.equal(out[0], want_plain), "the plain request inside the redraw sampler"
    assert torch.equal(out[1], want_redraw), "the redraw request beside a plain one"
    from diffsensei_amd.pipeline import redraw_mask_from_boxes
    keep = (redraw_mask_from_boxes(box, 16, 16) == 0)[None, None].expand(1, 4, 16, 16)
    assert 0 < int(keep.sum()) < keep.numel()
    assert torch.equal(out[1].cpu()[keep], kept[keep]), "the kept region is bit for bit the latents given"
    assert not torch.equal(out[1].cpu()[~keep], kept[~keep])


@pytest.mark.gpu
def test_a_refilled_request_against_its_own_oracle_loop(pipe):
    """B (3 steps) is admitted at step 1 into the slot a 1-step request left: against the oracle loop of
    tests/test_gpu_per_panel_scales.py run for B alone, at that test's gate."""
    p, cfg, sd, rs, clip, mae, A, B = pipe
    out = p.generate_continuous([_clone(A), _clone(A, num_inference_steps=1), _clone(B)], slots=2, output_type="latent")
    assert p.last_run_info["continuous"]["admissions"] == [(0, 0, [0]), (0, 1, [1]), (1, 2, [1])]
    ref = _oracle(cfg, sd, rs, clip, mae, B, B["guidance_scale"], B["ip_scale"])
    gate("test_gpu_continuous: request admitted at step 1 into a freed slot vs its own oracle loop", _rel(out[2], ref), 1.2e-2)


@pytest.mark.gpu
def test_refusals_come_before_anything_runs(pipe):
    p, cfg, sd, rs, clip, mae, A, B = pipe
    before = dict(p.last_run_info)
    run = lambda reqs, slots=2: p.generate_continuous(reqs, slots=slots, output_type="latent")
    with pytest.raises(ValueError, match="height"):
        run([_clone(A), _clone(B, height=256, width=256, latents=torch.zeros(1, 4, 32, 32).half())])
    with pytest.raises(ValueError, match="guidance"):
        run([_clone(A), _clone(B, guidance_scale=1.0)])
    with pytest.raises(ValueError, match="slots"):
        run([_clone(A), _clone(B, num_samples=3, latents=None)])
    with pytest.raises(ValueError, match="lora"):
        run([_clone(A, lora={}), _clone(B, lora={"x": 1.0})])
    with pytest.raises(ValueError):
        run([_clone(A), _clone(B, strength=0.5)])                 # a strength without anything to keep
    with pytest.raises(TypeError):
        run([_clone(A, callback_on_step_end=lambda *a: None)])
    # what a request's conditioning would only find at its admission, with other requests' steps already run: C waits for a slot
    for bad in (dict(noise_seeds=[3]),                               # Euler draws no noise
                dict(latents=torch.zeros(1, 4, 8, 8).half()), dict(ip_bbox=[]), dict(ip_scale=[0.5, 0.6]), dict(prompt=None),
                dict(pooled_prompt_embeds=None), dict(generator=[torch.Generator(), torch.Generator()])):
        with pytest.raises(ValueError):
            run([_clone(A), _clone(B), _clone(A, **bad)])
    assert p.last_run_info == before, "a refused run ran something"
    assert run([]) == []


@pytest.mark.gpu
def test_conditioning_survives_a_sampling_stream_that_lags_behind_the_host(pipe):
    """Three admissions, two of them refills of one slot by requests whose conditioning tensors have the same sizes, while the
    sampling stream is held back by a device-side delay so that the host runs ahead of it: each request still equals its own
    uniform batch.  This pins the result under a lagging stream; it is NOT a detector of a conditioning tensor freed too
    early - on the tiny pipeline it also passed with the hand-over in `_generate_continuous` disabled, the allocator did not
    happen to reuse the memory in time.  That lifetime is held by construction there (`hand_over`)."""
    p, cfg, sd, rs, clip, mae, A, B = pipe
    a = _clone(A, num_inference_steps=3)
    b = _clone(B, num_inference_steps=1)
    c = dict(_third(A, cfg), num_inference_steps=1)
    d = _clone(B, num_inference_steps=1, guidance_scale=6.0, ip_scale=0.3, latents=B["latents"].flip(-1),
               prompt_embeds=B["prompt_embeds"].flip(1), ip_bbox=[[0.1, 0.0, 0.4, 1.0], [0.6, 0.0, 0.9, 1.0]])
    ref = lambda second: p.generate_batch([_clone(A, num_inference_steps=1), _clone(second)], output_type="latent")[1]
    want = [ref(b), ref(c), ref(d)]
    if p._stream is None:
        p._stream = torch.cuda.Stream()
    with torch.cuda.stream(p._stream):
        torch.cuda._sleep(200_000_000)
    out = p.generate_continuous([_clone(r) for r in (a, b, c, d)], slots=2, output_type="latent")
    assert p.last_run_info["continuous"]["admissions"] == [(0, 0, [0]), (0, 1, [1]), (1, 2, [1]), (2, 3, [1])]
    for tag, o, w in zip("BCD", out[1:], want):
        assert torch.equal(o, w), f"request {tag} was served with something else's conditioning"
    assert not torch.equal(out[2], out[3])
