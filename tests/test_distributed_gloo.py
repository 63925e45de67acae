"""CPU, world_size 2 over gloo: the N>1 path of the serving layer — bucketed weight broadcast from rank 0,
deterministic request sharding with no data-path collective, result gather."""
import os
import socket
import sys

import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The ranks of these tests run on the host.  Where a GPU is visible, init_from_env() selects device LOCAL_RANK, which a
# 1-GPU box does not have for ranks 1..7: its test hook DS_FORCE_DEVICE puts every rank on device 0 instead (no effect
# without a GPU), and DS_DIST_BACKEND keeps bench.py's ranks on gloo, whose collectives need no device per rank.
HOST_RANK_ENV = {"DS_FORCE_DEVICE": "0"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), **HOST_RANK_ENV)
    import torch.distributed as dist
    from diffsensei_amd.distributed import PanelRequest, broadcast_tensors, init_from_env, run_sharded
    r, w, _ = init_from_env("gloo")
    assert (r, w) == (rank, world)
    # weights: rank 0 holds the seeded values, everyone else garbage -> identical after the broadcast
    g = torch.Generator().manual_seed(0)
    shapes = [(320, 4, 3, 3), (1280,), (640, 640), (10240, 1280), (17,)]
    ws = [torch.randn(s, generator=g).half() if rank == 0 else torch.full(s, float(rank)).half() for s in shapes]
    ws.append(torch.arange(6, dtype=torch.float32) if rank == 0 else torch.zeros(6))
    stats = broadcast_tensors(ws, src=0, bucket_bytes=1 << 20)
    g2 = torch.Generator().manual_seed(0)
    ok = all(torch.equal(t, torch.randn(s, generator=g2).half()) for t, s in zip(ws[:-1], shapes))
    ok = ok and torch.equal(ws[-1], torch.arange(6, dtype=torch.float32)) and stats["buckets"] >= 2
    reqs = [PanelRequest(i, s, s, 50, 1 + (i % 2)) for i, s in enumerate([512, 768, 1024, 1536, 1024, 512, 768, 1024])]
    seen = []

    def work(req):
        seen.append(req.request_id)
        return (rank, req.height)

    out = run_sharded(reqs, work, gather=True)
    dist.barrier()
    q.put((rank, ok, seen, out))
    dist.destroy_process_group()


def test_broadcast_and_sharding_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, ok0, seen0, out0), (r1, ok1, seen1, out1) = res
    assert ok0 and ok1
    assert sorted(seen0 + seen1) == list(range(8)) and not set(seen0) & set(seen1)
    assert out1 is None and sorted(out0) == list(range(8))
    assert all(out0[i][0] == (0 if i in seen0 else 1) for i in range(8))


def test_shard_requests_balanced_and_deterministic():
    from diffsensei_amd.distributed import PanelRequest, shard_requests
    reqs = [PanelRequest(i, s, s) for i, s in enumerate([512, 768, 1024, 1536] * 8)]
    a = shard_requests(reqs, 8)
    b = shard_requests(list(reversed(reqs)), 8)
    assert [[r.request_id for r in s] for s in a] == [[r.request_id for r in s] for s in b]
    loads = [sum(r.cost() for r in s) for s in a]
    assert max(loads) / min(loads) < 1.25
    assert sum(len(s) for s in a) == 32
    for s in a:
        assert [(r.height, r.width) for r in s] == sorted((r.height, r.width) for r in s)
    assert shard_requests([], 4) == [[], [], [], []]


def _worker_batched(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), **HOST_RANK_ENV)
    import torch.distributed as dist
    from diffsensei_amd.distributed import PanelRequest, init_from_env, run_sharded_batched
    init_from_env("gloo")
    calls = []

    class FakePipe:  # records the UNet batches the front-end forms on this rank
        def generate_batch(self, requests, output_type="pil"):
            calls.append([(r["height"], r["prompt"]) for r in requests])
            return [f"{r['prompt']}@{rank}" for r in requests]

    sizes = [512, 768, 1024, 1536, 1024, 512, 768, 1024, 512, 512]
    reqs = [PanelRequest(i, s, s, 50, 1, payload={"prompt": f"p{i}", "guidance_scale": 7.5}) for i, s in enumerate(sizes)]
    out = run_sharded_batched(reqs, FakePipe(), max_panels=4, output_type="pt", gather=True)
    dist.barrier()
    q.put((rank, calls, out))
    dist.destroy_process_group()


def test_sharded_bucketed_serving_world2():
    """configs[3] control flow: a mixed-resolution queue is sharded over 2 ranks (no data-path collective), each rank
    batches its shard per resolution bucket, rank 0 gathers every request's result exactly once."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_batched, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    (_, calls0, out0), (_, calls1, out1) = res
    assert out1 is None and sorted(out0) == list(range(10))
    served = [pr for c in calls0 + calls1 for b in [c] for (_, pr) in b]
    assert sorted(served) == sorted(f"p{i}" for i in range(10))              # every request on exactly one rank
    for c in calls0 + calls1:
        assert len({h for h, _ in c}) == 1 and len(c) <= 4                   # a batch never mixes buckets, panel cap
    assert calls0 and calls1                                                 # both ranks got work
    for i in range(10):
        assert out0[i].startswith(f"p{i}@")


def _mllm_worker(rank, world, port, q):
    """The MLLM engine's packed weights (stacked q|k|v / gate|up, o, down, the RMSNorm gains, embeddings, lm_head) are what the
    N > 1 start-up broadcast must cover: rank 1 starts from different seeds and must end bit-identical to rank 0."""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), **HOST_RANK_ENV)
    import torch.distributed as dist
    from diffsensei_amd.distributed import broadcast_tensors, init_from_env
    from diffsensei_amd.mllm import LlamaConfig, LlamaDecodeEngine, llama_param_shapes
    init_from_env("gloo")
    cfg = LlamaConfig(vocab_size=96, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1)
    g = torch.Generator().manual_seed(100 + rank)
    sd = {k: torch.randn(s, generator=g) * 0.05 for k, s in llama_param_shapes(cfg).items()}
    eng = LlamaDecodeEngine(cfg, sd, "cpu", max_positions=16, max_new_tokens=4)
    ts = eng.tensors()
    n_param = sum(t.numel() for t in ts)
    before = torch.cat([t.flatten().float() for t in ts]).sum().item()
    broadcast_tensors(ts, src=0, bucket_bytes=1 << 16)
    after = torch.cat([t.flatten().float() for t in eng.tensors()])
    dist.barrier()
    q.put((rank, n_param, before, after.sum().item(), after[::97].tolist()))
    dist.destroy_process_group()


def test_mllm_weight_broadcast_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mllm_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, n0, before0, after0, sample0), (_, n1, before1, after1, sample1) = res
    # every tensor of the model is in the list: 2 layers x ((3+1+2+1) H-by-* blocks + 2 RMSNorm gains) + embeddings + lm_head
    # + final gain
    assert n0 == n1 == 2 * (3 * 128 * 128 + 128 * 128 + 2 * 256 * 128 + 128 * 256 + 2 * 128) + 2 * 96 * 128 + 128
    assert before0 != before1 and after0 == before0 and after1 == after0 and sample0 == sample1


def _pipeline_bcast_worker(rank, world, port, q):
    """`broadcast_pipeline` over a pipeline-shaped object: every engine's tensors() + the extra (MLLM-agent-like) module,
    rank 1 starts from other values, `weights_changed()` is called, and the cross-rank checksum passes; a replica that is
    then perturbed on one rank makes `verify_replicas` raise on EVERY rank."""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), **HOST_RANK_ENV)
    import torch.distributed as dist
    from diffsensei_amd.distributed import broadcast_pipeline, init_from_env, tensors_checksum, verify_replicas
    init_from_env("gloo")
    g = torch.Generator().manual_seed(5 + 100 * rank)

    class Engine:
        def __init__(self, shapes, dtype):
            self.ts = [torch.randn(s, generator=g).to(dtype) for s in shapes]

        changed = 0

        def tensors(self):
            return self.ts

        def weights_changed(self):
            self.changed += 1

    class UNet(Engine):
        pass

    class Pipe:
        def __init__(self):
            self.unet = UNet([(64, 4, 3, 3), (640, 320), (77,)], torch.float16)
            self.enc = Engine([(128, 128), (5,)], torch.float16)
            self.vae = Engine([(32, 32, 3, 3)], torch.bfloat16)

        def tensors(self):
            return self.unet.tensors() + self.enc.tensors() + self.vae.tensors()

    pipe, agent = Pipe(), Engine([(96, 128), (7,)], torch.float32)
    before = int(tensors_checksum(pipe.tensors() + agent.tensors())[0])
    stats = broadcast_pipeline(pipe, extra=[agent], bucket_bytes=1 << 14)
    after = int(tensors_checksum(pipe.tensors() + agent.tensors())[0])
    ok = stats["tensors"] == 8 and stats["checksum"] == after and stats["buckets"] >= 3
    ok = ok and [m.changed for m in (pipe.unet, pipe.vae, agent)] == [1, 1, 1]      # every engine the pipeline names + the extra
    raised = False
    if rank == 1:
        pipe.enc.ts[0][3, 3] += 1.0                      # one value differs on one rank
    try:
        verify_replicas(pipe.tensors())
    except RuntimeError:
        raised = True
    dist.barrier()
    q.put((rank, before, after, ok, raised))
    dist.destroy_process_group()


def test_broadcast_pipeline_and_replica_check_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_pipeline_bcast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, b0, a0, ok0, r0), (_, b1, a1, ok1, r1) = res
    assert b0 != b1 and a0 == a1 == b0 and ok0 and ok1
    assert r0 and r1, "a perturbed replica must be detected on both ranks"


def test_weight_arena_rehomes_tensors_in_place():
    """`WeightArena` (the no-staging weight broadcast): every tensor keeps its identity, shape and values but ends up as a
    256-byte-aligned slice of a flat segment per dtype; memory listed twice - also under another shape - is re-homed once and
    keeps aliasing; a view of a LISTED tensor follows it into its slot; a non-contiguous tensor and a view of unlisted storage
    are left alone (`loose`) and go through the staging buffer of `broadcast_arena`."""
    from diffsensei_amd.distributed import WeightArena
    g = torch.Generator().manual_seed(0)
    ts = [torch.randn(s, generator=g).half() for s in [(7, 3), (640, 640), (5,), (33, 2, 2)]]
    ts += [torch.arange(6, dtype=torch.float32), torch.randn(3, 3, generator=g)]
    shared = ts[1]
    flat_alias = ts[1].view(-1)                                   # the same storage under another shape
    odd = torch.randn(8, 6, generator=g).half().t()               # not contiguous, base not listed
    base = torch.randn(3, 16, 16, generator=g).half()             # a packed weight that is NOT listed ...
    view = base[1]                                                # ... and a slice of it that an engine lists: must keep aliasing
    packed = torch.randn(4, 8, 8, generator=g).half()             # a packed weight that IS listed ...
    window, tview = packed[2], packed[1].t()                      # ... with a contiguous and a transposed window onto it
    lst = ts + [shared, flat_alias, odd, view, packed, window, tview]
    before = [t.clone() for t in lst]
    ids = [id(t) for t in lst]
    arena = WeightArena(lst)
    assert [id(t) for t in lst] == ids and all(torch.equal(a, b) for a, b in zip(lst, before))
    assert set(k[1] for k in arena.buffers) == {torch.float16, torch.float32}
    assert len(arena.loose) == 2 and arena.loose[0] is odd and arena.loose[1] is view and view.data_ptr() == base[1].data_ptr()
    view.fill_(7.0)
    assert float(base[1].float().mean()) == 7.0                   # still a window onto the unlisted packed weight
    (f16,) = arena.buffers[(torch.device("cpu"), torch.float16)]
    lo, hi = f16.data_ptr(), f16.data_ptr() + f16.numel() * 2
    for t in ts[:4] + [packed]:
        assert lo <= t.data_ptr() < hi and (t.data_ptr() - lo) % 256 == 0 and t.is_contiguous()
    # aliases and windows moved WITH their owners
    assert flat_alias.data_ptr() == ts[1].data_ptr() and flat_alias.shape == (640 * 640,)
    assert window.data_ptr() == packed[2].data_ptr() and tview.data_ptr() == packed[1].data_ptr() and not tview.is_contiguous()
    packed[2].fill_(3.0)
    packed[1].copy_(torch.arange(64).view(8, 8).half())
    assert float(window.float().mean()) == 3.0 and torch.equal(tview, torch.arange(64).view(8, 8).half().t())
    ts[1].view(-1)[5] = 9.0
    assert float(flat_alias[5]) == 9.0
    # distinct memory is counted once
    unique = ts + [odd, view, packed]
    assert arena.payload_bytes == sum(t.numel() * t.element_size() for t in unique)
    assert arena.bytes >= sum(t.numel() * t.element_size() for t in ts + [packed])
    # writing through the arena IS writing the tensors (what the in-place broadcast relies on)
    f16.zero_()
    assert all(float(t.abs().sum()) == 0 for t in ts[:4]) and float(ts[4].sum()) == 15.0 and float(window.abs().sum()) == 0
    sl = arena.slices(1 << 10)
    assert sum(x.numel() * x.element_size() for x in sl) == arena.bytes and all(x.is_contiguous() for x in sl)


def test_weight_arena_keeps_aliases_of_another_element_type():
    """a tensor that shares a listed owner's storage under a DIFFERENT dtype (the int16 / uint8 reinterpretation of a
    packed f16 weight) used to go to `loose` with its old storage while the owner was re-homed - the aliasing broke silently.
    It now follows the owner into its slot and costs no message of its own."""
    from diffsensei_amd.distributed import WeightArena
    w = torch.arange(96, dtype=torch.float32).half().view(8, 12)
    first = torch.randn(5, 3).half()                              # pushes w's slot to a non-zero offset of the segment
    as_i16, as_u8 = w.view(torch.int16), w.view(-1).view(torch.uint8)
    bits = as_i16.clone()
    arena = WeightArena([first, w, as_i16, as_u8])
    assert arena.loose == [] and arena.payload_bytes == (15 + 96) * 2
    assert as_i16.data_ptr() == w.data_ptr() == as_u8.data_ptr() and w.storage_offset() > 0
    assert torch.equal(as_i16, bits) and as_u8.shape == (192,) and as_i16.shape == (8, 12)
    w[3, 4] = 1.0
    assert int(as_i16[3, 4]) == 0x3C00 and int(as_u8[2 * (3 * 12 + 4) + 1]) == 0x3C


def test_weight_arena_segments_bound_the_transient_copy():
    """Segments: the arena is filled in pieces of at most `segment_bytes` (1 GiB in production), so re-homing never holds a
    second copy of all weights; a tensor larger than a segment gets a segment of its own."""
    from diffsensei_amd.distributed import WeightArena
    ts = [torch.full((1000,), float(i)).half() for i in range(10)] + [torch.ones(5000).half()]
    arena = WeightArena(ts, segment_bytes=4096)                   # 2 x 2048-byte slots per segment
    segs = arena.buffers[(torch.device("cpu"), torch.float16)]
    assert len(segs) == 6 and [s.numel() * 2 for s in segs[:5]] == [4096] * 5 and segs[5].numel() >= 5000
    assert all(float(t[0]) == float(i) for i, t in enumerate(ts[:10])) and float(ts[10].sum()) == 5000
    assert sum(x.numel() for x in arena.slices(1 << 20)) * 2 == arena.bytes


def _loose_worker(rank, world, port, q):
    """A non-contiguous tensor, a view of unlisted storage, a view of a LISTED tensor and a re-shaped alias all arrive
    intact on rank 1 (RCCL / NCCL raise "Tensors must be contiguous" for the first one if it is sent as it is)."""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), **HOST_RANK_ENV)
    import torch.distributed as dist
    from diffsensei_amd.distributed import broadcast_tensors, init_from_env
    init_from_env("gloo")
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g).half() if rank == 0 else torch.full(s, -1.0).half()
    plain = mk(33, 7)
    odd = mk(8, 6).t()                                            # not contiguous
    hidden_base = mk(3, 16, 16)
    view = hidden_base[1]                                         # base not listed
    packed = mk(4, 8, 8)
    window, alias = packed[2].t(), packed.view(-1)                # base listed
    f32odd = (torch.randn(5, 4, generator=g) if rank == 0 else torch.zeros(5, 4)).t()
    lst = [plain, odd, view, packed, window, alias, f32odd]
    stats = broadcast_tensors(lst, src=0, bucket_bytes=1 << 10)
    g2 = torch.Generator().manual_seed(3)
    exp = lambda *s: torch.randn(*s, generator=g2).half()
    e_plain, e_odd, e_base, e_packed = exp(33, 7), exp(8, 6).t(), exp(3, 16, 16), exp(4, 8, 8)
    e_f32 = torch.randn(5, 4, generator=g2).t()
    ok = torch.equal(plain, e_plain) and torch.equal(odd, e_odd) and torch.equal(view, e_base[1]) and torch.equal(packed, e_packed)
    ok = ok and torch.equal(window, e_packed[2].t()) and torch.equal(alias, e_packed.view(-1)) and torch.equal(f32odd, e_f32)
    ok = ok and torch.equal(hidden_base[1], e_base[1]) and window.data_ptr() == packed[2].data_ptr()
    if rank == 1:
        ok = ok and float(hidden_base[0].float().mean()) == -1.0   # only the listed window of the hidden base was written
    dist.barrier()
    q.put((rank, ok, stats["buckets"], stats["bytes"]))
    dist.destroy_process_group()


def test_broadcast_non_contiguous_and_views_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_loose_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, ok0, nb0, by0), (_, ok1, nb1, by1) = res
    assert ok0 and ok1 and nb0 == nb1 and nb0 >= 3
    # payload: plain + odd + view + packed + f32odd, the window / alias of `packed` counted once with it
    assert by0 == by1 == (33 * 7 + 48 + 256 + 256) * 2 + 20 * 4


def test_broadcast_pipeline_requires_weights_changed_of_every_engine():
    """an engine that lists `tensors()` but has no `weights_changed()` would keep stale raw-pointer caches silently
    after the re-homing broadcast - `broadcast_pipeline` refuses it (no process group needed for the check); every engine of
    the package defines the hook."""
    import pytest
    from diffsensei_amd.distributed import broadcast_pipeline
    from diffsensei_amd import encoders, mllm, resampler, unet, vae

    class NoHook:
        def tensors(self):
            return [torch.zeros(3)]

    class Pipe:
        unet = NoHook()

        def tensors(self):
            return self.unet.tensors()

    with pytest.raises(TypeError, match="weights_changed"):
        broadcast_pipeline(Pipe())
    for cls in (encoders.ViTEncoderEngine, encoders.ClipTextEngine, resampler.Resampler, unet.UNetMangaModel,
                vae.VaeDecoderEngine, mllm.LlamaDecodeEngine, mllm.QwenResampler, mllm.ContinuousLVLM):
        assert callable(getattr(cls, "weights_changed", None)) and callable(getattr(cls, "tensors", None)), cls


def _run_bench(args, env_extra=None, drop=("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")):
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(HOST_RANK_ENV, DS_DIST_BACKEND="gloo")
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *args], env=env, capture_output=True, text=True,
                       timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, [json.loads(ln) for ln in lines]


def test_bench_gpus2_without_torchrun_spawns_its_own_ranks():
    """`python bench.py --gpus 2` with NO torchrun environment (the form the driver uses at N = 1) used to
    die on `assert world == args.gpus`; it now re-launches itself under torch.distributed.run on a free 127.0.0.1 port.
    `--dry-run` keeps the launcher, the process group (gloo here: no GPU), both barriers, the max-over-ranks reduction and the
    one JSON line from rank 0, and replaces the step by a sleep."""
    r, lines = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1, r.stdout            # ONE line, from rank 0 only
    ln = lines[0]
    assert ln["n_gpus"] == 2 and ln["steps"] == 3 and ln["warmup"] == 1 and ln["dry_run"] is True
    assert ln["ms_per_step"] >= 10.0 and ln["scaling"] == "weak"


def test_bench_under_torchrun_env_mismatch_is_an_error_not_a_hang():
    """Under a launcher whose WORLD_SIZE disagrees with --gpus the script exits with a message (no spawn, no assert)."""
    r, lines = _run_bench(["--gpus", "2", "--dry-run"], env_extra={"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}, drop=())
    assert r.returncode != 0 and not lines
    assert "WORLD_SIZE=1" in r.stderr


# ------------------------------------------------------------------------------------------ world size 8
def _worker_c3_world8(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), **HOST_RANK_ENV)
    import torch.distributed as dist
    from diffsensei_amd.distributed import PanelRequest, init_from_env, run_sharded_batched
    init_from_env("gloo")
    calls = []

    class StubPipe:   # stands for DiffSenseiPipeline.generate_batch: one "image" per request, tagged with the serving rank
        def generate_batch(self, requests, output_type="pil"):
            calls.append([(r["height"], r["prompt"]) for r in requests])
            return [torch.full((2, 2), float(rank)) for _ in requests]

    sizes = [512, 768, 1024, 1536] * 8      # BASELINE.json configs[3]: mixed-resolution bucket, 32 requests, 8 GPUs
    reqs = [PanelRequest(i, s, s, 50, 1, payload={"prompt": f"p{i}", "guidance_scale": 7.5}) for i, s in enumerate(sizes)]
    out = run_sharded_batched(reqs, StubPipe(), max_panels=16, output_type="pt", gather=True)
    dist.barrier()
    mine = sum(PanelRequest(0, h, h, 50, 1).cost() for c in calls for (h, _) in c)
    q.put((rank, calls, mine, None if out is None else {k: float(v[0][0]) for k, v in out.items()}))
    dist.destroy_process_group()


def test_configs3_queue_over_8_ranks_every_request_once_and_balanced():
    """BASELINE.json configs[3] - 32 requests over the buckets {512, 768, 1024, 1536}^2 on 8 ranks - through the real
    `run_sharded_batched` (LPT sharding, per-rank BucketBatcher, uint8 / array gather to rank 0) with a stub pipeline on 8 gloo
    processes: every request is served exactly once, by the rank the result says, never in a mixed-bucket batch, and the LPT
    shards are within 10 % of each other in modelled cost.  (The N = 2 / 4 / 8 CURVE stays unmeasured: no multi-GPU box in reach.)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_c3_world8, args=(r, 8, port, q)) for r in range(8)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    served = {}
    for rank, calls, _, out in res:
        assert (out is None) == (rank != 0)
        for batch in calls:
            assert len({h for h, _ in batch}) == 1 and len(batch) <= 16
            for _, pr in batch:
                assert pr not in served, f"{pr} served twice"
                served[pr] = rank
    assert sorted(served) == sorted(f"p{i}" for i in range(32))
    out0 = res[0][3]
    assert sorted(out0) == list(range(32))
    assert all(int(out0[i]) == served[f"p{i}"] for i in range(32))       # the gathered result comes from the rank that served it
    loads = [m for _, _, m, _ in res]
    assert min(loads) > 0 and max(loads) / min(loads) <= 1.10, loads


def test_bench_gpus8_dry_run_one_line_from_rank0():
    """`python bench.py --gpus 8 --dry-run` with no torchrun environment: the script starts its own 8 ranks (gloo here), runs the
    barrier-bracketed timing with the MAX over ranks and prints ONE JSON line with n_gpus 8 from rank 0."""
    r, lines = _run_bench(["--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1, r.stdout
    ln = lines[0]
    assert ln["n_gpus"] == 8 and ln["steps"] == 2 and ln["warmup"] == 1 and ln["dry_run"] is True and ln["scaling"] == "weak"
