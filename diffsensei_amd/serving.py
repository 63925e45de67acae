"""Request front-end: resolution-bucketed batching of panel requests.

The reference serves one panel request at a time from a Gradio callback (scripts/demo/gradio_wo_mllm.py:45, the
`pipeline(...)` call inside `result_generation`), and its training side groups images by size with a bucket sampler
(src/datasets/dataset_size_bucket.py:488-544: items are binned by (height, width) and a batch never mixes bins).
Here the same idea is applied to inference, because one UNet launch plan / hipGraph exists per
(batch, height, width) and the kernels only reach their throughput on large batches:

    batcher = BucketBatcher(pipe)                              # up to 32 panels per UNet batch at 1024 x 1024
    tickets = [batcher.submit(**request_kwargs) for ...]      # the keyword arguments of DiffSenseiPipeline.__call__
    results = batcher.run(output_type="pil")                   # results[ticket] = that request's images

Requests that share (height, width, steps, guidance_scale, ip_scale) - and, for region-redraw requests
(`redraw_latents` or `redraw_image`), `strength`; a redraw never shares a batch with a plain request - are concatenated into one UNet batch
of at most `max_panels` panels (`DiffSenseiPipeline.generate_batch`: per-request prompts, character references, boxes, seeds);
buckets run largest-resolution first.

`mix_scales=True` (`bucket_key`, `plan_batches`, `BucketBatcher`) drops the two sliders from that key: guidance and IP
scale are per-panel vectors in the kernels, so requests that differ only in them share a batch, a launch plan and a
captured hipGraph, and every panel still gets its own values.  What stays in the key is which side of 1 the guidance is
on: classifier-free guidance doubles the UNet batch, so it is on or off for a whole batch.  The default, False, is the
five-value key above.  Multi-GPU: shard the request list with `distributed.shard_requests` (LPT by
pixel count, no data-path collective) and run one batcher per rank.

`continuous=True` (`BucketBatcher`; `plan_continuous`, `continuous_key`) takes step count, strength and plain / redraw out
of the key as well: every panel slot of `DiffSenseiPipeline.generate_continuous` runs its own schedule, and a finished
panel's slot is handed to the next request of the queue while the others keep going, so a queue of mixed step counts
keeps one UNet batch full instead of falling apart into one small bucket per step count.  The default, False, plans
the static batches described above.

Long prompts: a request with `max_prompt_chunks` (or direct `prompt_embeds` of another length than 77) carries the chunk
count it results in as one more key element (`_chunks_key`): the UNet engine is sized by its text length, so requests with
different chunk counts never share a UNet batch.  Requests without the field are keyed as before.

MLLM-conditioned requests: `BucketBatcher(pipe, agent=agent)` and `submit(..., ip_images=[...], mllm={"input_ids",
"ids_cmp_mask", "mllm_scale", ...})`.  `run()` first turns every such request into an `ip_image_embeds` request through
`mllm.mllm_prepass_batch`, in groups of at most `agent.llm.max_sequences` (one decode loop per group: a token step for 16
sequences reads the weights once), then plans the UNet batches as above.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple


def _scale_key(v):
    """A slider value as a hashable: a float (anything `float()` takes, as before), or a tuple of floats for the
    one-value-per-sample form."""
    try:
        return float(v)
    except (TypeError, ValueError):
        return tuple(float(x) for x in v)


def _chunks_key(request: dict, chunks=None) -> Tuple:
    """(("chunks", k),) for a request that carries `max_prompt_chunks` or direct `prompt_embeds` of another length than 77,
    () for every other request: its key is what it was.  k is the chunk count the request RESULTS in - the UNet engine is
    sized by it -: `chunks(request)` (`DiffSenseiPipeline.prompt_chunk_count`, which tokenizes the prompts) or, for direct
    embeddings, ceil(length / 77).  A text prompt with `max_prompt_chunks` > 1 cannot be counted without the tokenizers."""
    pe = request.get("prompt_embeds")
    if "max_prompt_chunks" not in request and (pe is None or int(pe.shape[-2]) == 77):
        return ()
    if pe is not None:
        return (("chunks", -(-int(pe.shape[-2]) // 77)),)
    mc = request["max_prompt_chunks"]
    if isinstance(mc, bool) or not isinstance(mc, int) or not 1 <= mc <= 4:
        raise ValueError(f"`max_prompt_chunks` must be an integer in 1..4, got {mc!r}")
    if mc == 1:
        return (("chunks", 1),)
    if chunks is None:
        raise ValueError("the chunk count of a text prompt with max_prompt_chunks > 1 needs the tokenizers: pass "
                         "chunks=pipe.prompt_chunk_count")
    return (("chunks", int(chunks(request))),)


def bucket_key(request: dict, mix_scales: bool = False, chunks=None) -> Tuple:
    """What must agree for two requests to share a UNet batch.  mix_scales: (height, width, steps, guidance > 1) - the
    sliders travel per panel, only classifier-free guidance on / off is a property of the batch.  A request whose own
    guidance values lie on both sides of 1 fits no batch and is a ValueError here, so that it cannot take the requests
    bucketed with it down (`BucketBatcher.submit` checks every request this way).  `chunks`: see `_chunks_key` - requests
    whose prompts result in different chunk counts never share a batch."""
    g = _scale_key(request.get("guidance_scale", 5.0))
    # a region-redraw request (`redraw_latents` or `redraw_image`) runs a shortened schedule with another step kernel: it shares a batch
    # only with redraws of the same strength.  A plain request's key is what it was.
    is_redraw = request.get("redraw_latents") is not None or request.get("redraw_image") is not None
    redraw = (("redraw", float(request.get("strength", 1.0))),) if is_redraw else ()
    # `lora={name: weight}`: the merged UNet weights are one state per batch.  Only a request that carries the field gets the
    # element, so every other key is what it was; {} (no adapter) is a state of its own, distinct from "whatever is set"
    if "lora" in request:
        redraw = redraw + (("lora", tuple(sorted((str(k), float(v)) for k, v in dict(request["lora"] or {}).items()))),)
    redraw = redraw + _chunks_key(request, chunks)
    if mix_scales:
        on = {x > 1 for x in (g if isinstance(g, tuple) else (g,))}
        if len(on) != 1:
            raise ValueError(f"guidance_scale {list(g)} mixes classifier-free guidance on (> 1) and off (<= 1) in one request")
        return (request.get("height"), request.get("width"), request.get("num_inference_steps", 40), on.pop()) + redraw
    return (request.get("height"), request.get("width"), request.get("num_inference_steps", 40), g,
            _scale_key(request.get("ip_scale", 1.0))) + redraw


def plan_batches(requests: List[dict], max_panels: int, max_pixels: Optional[int] = None,
                 mix_scales: bool = False, chunks=None) -> List[List[int]]:
    """Indices of `requests` grouped into batches: same bucket, at most `max_panels` panels (sum of num_samples) per
    batch - and at most `max_pixels` output pixels if given, so small resolutions get proportionally larger batches (a
    single request above the pixel cap but within `max_panels` runs alone; only `num_samples > max_panels` is an error) -
    submission order kept inside a bucket, buckets ordered by decreasing pixel count (the long jobs first)."""
    if max_panels < 1:
        raise ValueError("max_panels must be >= 1")
    buckets: Dict[Tuple, List[int]] = {}
    for i, r in enumerate(requests):
        buckets.setdefault(bucket_key(r, mix_scales, chunks), []).append(i)
    order = sorted(buckets, key=lambda k: -((k[0] or 0) * (k[1] or 0)))
    batches: List[List[int]] = []
    for k in order:
        cap = max_panels
        if max_pixels is not None and k[0] and k[1]:
            cap = max(1, min(max_panels, max_pixels // (k[0] * k[1])))
        cur, panels = [], 0
        for i in buckets[k]:
            n = int(requests[i].get("num_samples", 1) or 1)
            if n > max_panels:
                raise ValueError(f"request {i}: num_samples {n} exceeds max_panels {max_panels}")
            if n > cap:
                # the pixel cap only shapes how requests are PACKED: a single request that is larger than it (2048 x 2048 with
                # num_samples 9..16 under the 32 Mpx default) is still served, in a batch of its own, as before the cap existed
                if cur:
                    batches.append(cur)
                    cur, panels = [], 0
                batches.append([i])
                continue
            if cur and panels + n > cap:
                batches.append(cur)
                cur, panels = [], 0
            cur.append(i)
            panels += n
        if cur:
            batches.append(cur)
    return batches


def plan_continuous(steps_run: List[int], panels: List[int], slots: int) -> dict:
    """The timeline of a continuous-batching run over `slots` panel slots, from the step counts alone (pure host code: which
    panel finishes at which step needs no look at the device).  Request r runs `steps_run[r]` consecutive steps on
    `panels[r]` slots.  Requests are admitted strictly in order: the head of the queue is admitted at the first step
    boundary at which `panels[head]` slots are free (the lowest-numbered free ones), and several may be admitted at one
    boundary.  Returns {"forwards": UNet forwards of the run, "slot_steps": sum of steps x panels, "idle_slot_steps":
    forwards x slots - slot_steps, "admissions": [(global_step, request, [slots])] in admission order, "finish":
    [global step after which request r is done]}.  `DiffSenseiPipeline.generate_continuous` executes exactly this plan."""
    if slots < 1:
        raise ValueError("slots must be >= 1")
    if len(steps_run) != len(panels):
        raise ValueError(f"{len(steps_run)} step counts for {len(panels)} panel counts")
    for r, (n, k) in enumerate(zip(steps_run, panels)):
        if int(n) < 1 or int(k) < 1:
            raise ValueError(f"request {r}: steps {n} and panels {k} must both be >= 1")
        if int(k) > slots:
            raise ValueError(f"request {r}: num_samples {k} exceeds the {slots} slots")
    free = list(range(slots))
    busy: Dict[int, int] = {}              # slot -> global step at which it is free again
    admissions, finish = [], [0] * len(steps_run)
    head, s = 0, 0
    while True:
        for slot in [q for q, end in busy.items() if end == s]:
            del busy[slot]
            free.append(slot)
        free.sort()
        while head < len(steps_run) and int(panels[head]) <= len(free):
            take, free = free[:int(panels[head])], free[int(panels[head]):]
            for slot in take:
                busy[slot] = s + int(steps_run[head])
            finish[head] = s + int(steps_run[head])
            admissions.append((s, head, take))
            head += 1
        if not busy:
            break
        s += 1
    slot_steps = sum(int(n) * int(k) for n, k in zip(steps_run, panels))
    return {"forwards": s, "slot_steps": slot_steps, "idle_slot_steps": s * slots - slot_steps, "admissions": admissions,
            "finish": finish}


def continuous_key(request: dict, chunks=None) -> Tuple:
    """What must agree for requests to share a continuous-batching run: (height, width, guidance > 1, lora state) and, for
    a request with `max_prompt_chunks` or long `prompt_embeds`, its chunk count (`_chunks_key`).  Step counts, strengths,
    plain vs redraw and both sliders are per panel there."""
    g = _scale_key(request.get("guidance_scale", 5.0))
    on = {x > 1 for x in (g if isinstance(g, tuple) else (g,))}
    if len(on) != 1:
        raise ValueError(f"guidance_scale {list(g)} mixes classifier-free guidance on (> 1) and off (<= 1) in one request")
    lora = None
    if "lora" in request:
        lora = tuple(sorted((str(k), float(v)) for k, v in dict(request["lora"] or {}).items()))
    return (request.get("height"), request.get("width"), on.pop(), lora) + _chunks_key(request, chunks)


class BucketBatcher:
    """Collects requests, then runs them bucket by bucket through `pipe.generate_batch` - or, with `continuous=True`, group
    by group (`continuous_key`, largest resolution first) through `pipe.generate_continuous` on as many panel slots as
    `plan_batches` would put panels into a batch: requests of any step count, strength and mode keep those slots full."""

    def __init__(self, pipe, max_panels: int = 32, max_pixels: Optional[int] = 32 * 1024 * 1024,
                 mix_scales: bool = False, agent=None, prepass=None, continuous: bool = False):
        # defaults = the benchmark's operating point (bench.py: 32 panels of 1024 x 1024 per call = UNet batch 64, where every
        # projection of the level-2 transformers is a whole number of 256-tile rounds); the pixel cap scales the panel count
        # down for larger images and lets smaller ones use the full 32
        self.pipe = pipe
        self.max_panels = max_panels
        self.max_pixels = max_pixels
        self.mix_scales = mix_scales         # requests that differ only in guidance_scale / ip_scale share a batch
        self.agent = agent                   # mllm.ContinuousLVLM: resolves requests submitted with `mllm=...`
        self.prepass = prepass               # what decodes one group (None: mllm.mllm_prepass_batch)
        self._pending: List[dict] = []
        self.last_plan: List[List[int]] = []
        self.last_prepass: List[List[int]] = []   # tickets of each MLLM pre-pass batch of the last run()
        self.continuous = continuous         # slots refilled in flight instead of one static batch per bucket
        self.last_slots: List[int] = []      # continuous: the slot count of each group of the last run()
        self._chunks = getattr(pipe, "prompt_chunk_count", None)   # resolves `max_prompt_chunks` to a chunk count (tokenizers)

    def submit(self, **request) -> int:
        """Queue one request (keyword arguments of `DiffSenseiPipeline.__call__`, without `output_type`); returns its ticket."""
        if "output_type" in request:
            raise TypeError("output_type is chosen per run(), not per request")
        bucket_key(request, True, self._chunks)   # a request no batch can hold is refused here, not when its batch runs
        m = request.get("mllm")
        if m is not None:
            if self.agent is None:
                raise ValueError("a request with `mllm` needs a BucketBatcher built with `agent=`")
            missing = [k for k in ("input_ids", "ids_cmp_mask", "mllm_scale") if k not in m]
            if missing:
                raise ValueError(f"mllm: {missing} missing (input_ids, ids_cmp_mask and mllm_scale are needed)")
            if request.get("ip_image_embeds") is not None:
                raise ValueError("`mllm` produces ip_image_embeds; pass one or the other")
        self._pending.append(request)
        return len(self._pending) - 1

    def __len__(self) -> int:
        return len(self._pending)

    _MLLM_SHARED = ("tokenizer", "img_ids_list", "eos_token_id", "max_new_tokens")   # one value per pre-pass batch

    def _resolve_mllm(self, reqs: List[dict]) -> List[dict]:
        """Requests with `mllm` -> the same requests with `ip_image_embeds` (and no `ip_images`), decoded in groups of at
        most `agent.llm.max_sequences` that agree on the shared decode arguments; the others are passed through."""
        self.last_prepass = []
        groups: Dict[Tuple, List[int]] = {}
        for i, r in enumerate(reqs):
            m = r.get("mllm")
            if m is not None:
                shared = tuple((k, id(m[k]) if k == "tokenizer" else (tuple(m[k]) if k == "img_ids_list" else m[k]))
                               for k in self._MLLM_SHARED if m.get(k) is not None)
                groups.setdefault(shared, []).append(i)
        if not groups:
            return reqs
        prepass = self.prepass
        if prepass is None:
            from .mllm import mllm_prepass_batch as prepass
        out = list(reqs)
        cap = max(1, int(self.agent.llm.max_sequences))
        for idx in groups.values():
            m0 = reqs[idx[0]]["mllm"]
            kw = {k: m0[k] for k in self._MLLM_SHARED if m0.get(k) is not None}
            for c0 in range(0, len(idx), cap):
                part = idx[c0:c0 + cap]
                embeds = prepass(self.pipe, self.agent,
                                 [dict(input_ids=reqs[i]["mllm"]["input_ids"], ids_cmp_mask=reqs[i]["mllm"]["ids_cmp_mask"],
                                       mllm_scale=reqs[i]["mllm"]["mllm_scale"], ip_images=reqs[i].get("ip_images", []))
                                  for i in part], **kw)
                self.last_prepass.append(part)
                for i, e in zip(part, embeds):
                    r = {k: v for k, v in reqs[i].items() if k != "mllm"}
                    r["ip_images"], r["ip_image_embeds"] = [], e
                    out[i] = r
        return out

    def run(self, output_type: str = "pil") -> List[Any]:
        """Run everything queued; returns the per-request outputs indexed by ticket and empties the queue."""
        reqs, self._pending = self._pending, []
        reqs = self._resolve_mllm(reqs)
        if self.continuous:
            return self._run_continuous(reqs, output_type)
        self.last_plan = plan_batches(reqs, self.max_panels, self.max_pixels, self.mix_scales, self._chunks)
        results: List[Any] = [None] * len(reqs)
        import contextlib
        # requests with `lora`: a batch leaves its adapters set, so consecutive batches of one state switch once, and the state
        # from before the run comes back once, at the end
        hold = self.pipe.hold_adapters() if any("lora" in r for r in reqs) else contextlib.nullcontext()
        with hold:
            for batch in self.last_plan:
                outs = self.pipe.generate_batch([reqs[i] for i in batch], output_type=output_type)
                for i, o in zip(batch, outs):
                    results[i] = o
        return results

    def _run_continuous(self, reqs: List[dict], output_type: str) -> List[Any]:
        groups: Dict[Tuple, List[int]] = {}
        for i, r in enumerate(reqs):
            groups.setdefault(continuous_key(r, self._chunks), []).append(i)
        order = sorted(groups, key=lambda k: -((k[0] or 0) * (k[1] or 0)))
        self.last_plan, self.last_slots = [], []
        for k in order:
            cap = self.max_panels
            if self.max_pixels is not None and k[0] and k[1]:
                cap = max(1, min(self.max_panels, self.max_pixels // (k[0] * k[1])))
            ns = [int(reqs[i].get("num_samples", 1) or 1) for i in groups[k]]
            for i, n in zip(groups[k], ns):
                if n > self.max_panels:
                    raise ValueError(f"request {i}: num_samples {n} exceeds max_panels {self.max_panels}")
            # like `plan_batches`, the pixel cap shapes the packing only: a request larger than it is still served
            self.last_plan.append(groups[k])
            self.last_slots.append(max(cap, max(ns)))
        results: List[Any] = [None] * len(reqs)
        import contextlib
        hold = self.pipe.hold_adapters() if any("lora" in r for r in reqs) else contextlib.nullcontext()
        with hold:
            for idx, slots in zip(self.last_plan, self.last_slots):
                outs = self.pipe.generate_continuous([reqs[i] for i in idx], slots=slots, output_type=output_type)
                for i, o in zip(idx, outs):
                    results[i] = o
        return results
