"""Multi-GPU serving layer: one process per GPU, frozen weights broadcast once over RCCL/xGMI, panel requests
sharded with NO data-path collective (each panel is independent: reference
src/pipelines/pipeline_diffsensei.py:180-372 keeps no cross-sample state).

The reference itself has no inference parallelism (demos pin 'cuda:0'); the only collective this path needs is
the start-up weight broadcast, plus an optional gather of results to rank 0.  `torch.distributed` backend "nccl"
IS RCCL on ROCm; the same code runs on gloo for the CPU tests.

xGMI is point-to-point (7 links x ~153 GB/s per GPU): a ring broadcast is per-link bound, so the weights are re-homed
into one flat arena per dtype (`WeightArena`) and the arena itself is sent in a few LARGE slices (default 512 MiB),
issued asynchronously with one final wait — no per-tensor messages, no staging copies; ~9 GB of weights ~= 60-70 ms.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

Tensor = torch.Tensor


def init_from_env(backend: Optional[str] = None) -> Tuple[int, int, int]:
    """(rank, world_size, local_rank) from the torchrun environment; initialises the default process group."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # RCCL shares device buffers between the ranks of a node through dmabuf IPC; the legacy IPC mode fails on hosts whose
    # driver only supports dmabuf (hipIpcGetMemHandle: invalid argument).  Read when the HSA runtime starts, i.e. at the
    # first device call below - a value the launcher already exported is left alone.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # test hooks (a 1-GPU box can still drive the N > 1 control flow): DS_DIST_BACKEND overrides the backend (gloo moves
    # CUDA tensors through the host), DS_FORCE_DEVICE pins every rank to one device index
    backend = os.environ.get("DS_DIST_BACKEND", backend)
    if "DS_FORCE_DEVICE" in os.environ:
        local = int(os.environ["DS_FORCE_DEVICE"])
    if torch.cuda.is_available():
        torch.cuda.set_device(local)   # every launch resolves "the current stream" on this rank's own GPU
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


class WeightArena:
    """Every frozen weight of a serving process in a few flat buffers ("segments", <= 1 GiB each) per (device, dtype).

    `WeightArena(tensors)` re-homes the given tensors: each keeps its Python identity, shape and values, but its storage
    becomes a 256-byte-aligned slice of a segment (`Tensor.set_`), after ONE device-to-device copy per tensor at start-up.
    The weight broadcast then runs on slices of the segments themselves - no `torch.cat` staging buffer, no copy-back (the
    round-2 path moved every byte three times), and the slices are issued as asynchronous collectives with a single wait at
    the end, so RCCL pipelines them over the xGMI ring.  Segments are filled one after the other and every tensor's old
    storage is released as soon as it has moved, so the transient peak is the weights + ONE segment (a single flat buffer per
    dtype held ~2x the weights while it was being filled).

    Aliasing is preserved: the same memory listed twice - under the same or under different shapes (`w` and `w.view(-1)`) -
    occupies one slot; a view into a LISTED tensor's storage (a slice of a packed weight, a transposed view) is re-pointed
    into that tensor's new slot with its offset and strides.  What is left over - non-contiguous tensors and views whose base
    is not listed - stays where it is (`loose`) and goes through one contiguous staging buffer per dtype in
    `broadcast_arena` (RCCL / NCCL refuse non-contiguous tensors).
    Data pointers change: callers must drop launch plans / packed copies derived from the old storage
    (`weights_changed()` of the engines - `broadcast_pipeline` calls it on every engine)."""
    ALIGN = 256
    SEGMENT_BYTES = 1 << 30

    def __init__(self, tensors: Sequence[Tensor], segment_bytes: Optional[int] = None):
        seg_bytes = int(segment_bytes or self.SEGMENT_BYTES)
        self.buffers: Dict[Tuple[torch.device, torch.dtype], List[Tensor]] = {}   # the segments, in fill order
        self.loose: List[Tensor] = []
        groups: Dict[Tuple[torch.device, torch.dtype], List[Tensor]] = {}
        owner_of: Dict[Tuple[int, int], Tensor] = {}     # (storage address, storage bytes) -> the listed tensor that owns it
        seen_ids = set()
        aliases: List[Tuple[Tensor, Tensor]] = []
        views: List[Tuple[Tensor, Tuple[int, int], int]] = []
        self.payload_bytes = 0                  # bytes of distinct weight memory (an alias or a view of a listed tensor counts once)
        for t in tensors:
            if id(t) in seen_ids:               # the same Python object listed twice
                continue
            seen_ids.add(id(t))
            st = t.untyped_storage()
            skey = (st.data_ptr(), st.nbytes())
            owns = t.storage_offset() == 0 and st.nbytes() == t.numel() * t.element_size() and t.is_contiguous()
            if owns and t.numel():
                first = owner_of.get(skey)
                if first is None:
                    owner_of[skey] = t
                    groups.setdefault((t.device, t.dtype), []).append(t)
                    self.payload_bytes += t.numel() * t.element_size()
                else:
                    # same memory, maybe another shape - or another element type (a uint8 / int32 reinterpretation of a
                    # packed weight, ADVICE r4: sent "loose" it kept the OLD storage and the aliasing broke silently): one
                    # slot, re-pointed below through the owner's new storage
                    aliases.append((t, first))
            elif owns:                          # empty tensor: nothing to move or send
                continue
            else:
                views.append((t, skey, t.storage_offset()))
        self.bytes = 0                          # arena size (with alignment padding)
        for (dev, dtype), lst in groups.items():
            esz = lst[0].element_size()
            step = max(1, self.ALIGN // esz)
            cap = max(step, seg_bytes // esz // step * step)
            segs: List[Tensor] = []
            i = 0
            while i < len(lst):
                # one segment: as many tensors as fit (a tensor larger than a segment gets one of its own)
                offs, n, j = [], 0, i
                while j < len(lst):
                    need = (lst[j].numel() + step - 1) // step * step
                    if j > i and n + need > cap:
                        break
                    offs.append(n)
                    n += need
                    j += 1
                flat = torch.zeros(n, dtype=dtype, device=dev)
                for t, off in zip(lst[i:j], offs):
                    view = flat[off:off + t.numel()].view(t.shape)
                    view.copy_(t)
                    t.set_(view)                # the old storage is released here (unless a loose view still holds it)
                segs.append(flat)
                self.bytes += n * esz
                i = j
                if dev.type == "cuda" and i < len(lst):
                    torch.cuda.empty_cache()    # hand the freed originals back before the next segment is allocated
            self.buffers[(dev, dtype)] = segs
        for t, first in aliases:
            # storage offsets count ELEMENTS of the aliasing tensor's own type: the owner's byte offset (a multiple of ALIGN)
            # divides by any element size
            off_bytes = first.storage_offset() * first.element_size()
            assert off_bytes % t.element_size() == 0
            t.set_(first.untyped_storage(), off_bytes // t.element_size(), t.size(), t.stride())
        for t, skey, off in views:
            base = owner_of.get(skey)
            if base is not None and base.dtype == t.dtype:
                # a window onto a listed tensor: follows it into its slot (offset and strides kept), needs no message of its own
                t.set_(base.untyped_storage(), base.storage_offset() + off, t.size(), t.stride())
            else:
                self.loose.append(t)
                self.payload_bytes += t.numel() * t.element_size()

    def segments(self) -> List[Tensor]:
        return [f for segs in self.buffers.values() for f in segs]

    def slices(self, bucket_bytes: int) -> List[Tensor]:
        """Contiguous slices of the segments, <= bucket_bytes each (the `loose` tensors are handled by `broadcast_arena`)."""
        out = []
        for flat in self.segments():
            m = max(1, bucket_bytes // flat.element_size())
            out += [flat[o:o + m] for o in range(0, flat.numel(), m)]
        return out


def broadcast_arena(arena: WeightArena, src: int = 0, bucket_bytes: int = 512 << 20, force: bool = False) -> Dict[str, float]:
    """Broadcast the arena's segments from `src` in `bucket_bytes` slices: all collectives issued asynchronously, one wait.
    Loose tensors (non-contiguous, or views of unlisted storage) travel through ONE contiguous staging buffer per
    (device, dtype) and are copied back after the wait."""
    stats = {"bytes": 0, "buckets": 0, "seconds": 0.0}
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not force):
        return stats
    t0 = time.perf_counter()
    work = []
    for sl in arena.slices(bucket_bytes):
        work.append(dist.broadcast(sl, src=src, async_op=True))
        stats["bytes"] += sl.numel() * sl.element_size()
        stats["buckets"] += 1
    staged: List[Tuple[Tensor, List[Tensor]]] = []
    by_type: Dict[Tuple[torch.device, torch.dtype], List[Tensor]] = {}
    for t in arena.loose:
        if t.numel():
            by_type.setdefault((t.device, t.dtype), []).append(t)
    for lst in by_type.values():
        stage = torch.cat([t.reshape(-1) for t in lst])
        work.append(dist.broadcast(stage, src=src, async_op=True))
        staged.append((stage, lst))
        stats["bytes"] += stage.numel() * stage.element_size()
        stats["buckets"] += 1
    for w in work:
        w.wait()
    for stage, lst in staged:
        o = 0
        for t in lst:
            t.copy_(stage[o:o + t.numel()].view(t.shape))
            o += t.numel()
    if any(dev.type == "cuda" for dev, _ in arena.buffers) or any(t.is_cuda for t in arena.loose):
        torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    return stats


def broadcast_tensors(tensors: Sequence[Tensor], src: int = 0, bucket_bytes: int = 512 << 20,
                      force: bool = False) -> Dict[str, float]:
    """In-place broadcast of tensors from `src`: they are re-homed into a `WeightArena` (their data pointers change!) and
    the arena is broadcast in large asynchronous slices.  `force`: issue the collectives even in a 1-rank group (the RCCL
    bring-up test on a single GPU).  Returns {"bytes", "buckets", "seconds", "consolidate_s"}."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not force):
        return {"bytes": 0, "buckets": 0, "seconds": 0.0, "consolidate_s": 0.0}
    t0 = time.perf_counter()
    arena = WeightArena(tensors)
    if any(dev.type == "cuda" for dev, _ in arena.buffers):
        torch.cuda.synchronize()
    t_cons = time.perf_counter() - t0
    stats = broadcast_arena(arena, src=src, bucket_bytes=bucket_bytes, force=force)
    stats["arena_bytes"], stats["bytes"] = stats["bytes"], arena.payload_bytes   # "bytes": the tensors' own; arena: + padding
    stats["consolidate_s"] = t_cons
    return stats


def tensors_checksum(tensors: Sequence[Tensor]) -> Tensor:
    """int64 [2] = (wrapping sum of every tensor's bit pattern weighted by its position, total element count), computed
    on the tensors' device.  Exact (integer arithmetic), so equal weights <=> equal checksums across ranks up to
    collisions; used to verify the weight broadcast."""
    dev = tensors[0].device if tensors else torch.device("cpu")
    acc = torch.zeros(2, dtype=torch.int64, device=dev)
    for k, t in enumerate(tensors):
        flat = t.detach().reshape(-1)
        if flat.element_size() == 2:
            bits = flat.view(torch.int16).to(torch.int64)
        elif flat.element_size() == 4:
            bits = flat.view(torch.int32).to(torch.int64)
        elif flat.element_size() == 1:
            bits = flat.view(torch.uint8).to(torch.int64)
        else:
            bits = flat.view(torch.int64)
        # position weights keep permutations of equal tensors from cancelling; the sum wraps mod 2^64 by construction
        w = torch.arange(1, bits.numel() + 1, dtype=torch.int64, device=dev) % 8191 + 1
        acc[0] += (bits * w).sum() * (2 * k + 1)
        acc[1] += bits.numel()
    return acc


def verify_replicas(tensors: Sequence[Tensor]) -> Dict[str, int]:
    """All ranks must hold bit-identical `tensors`: all-reduce MIN and MAX of the checksum and compare.  Raises on any
    rank if they differ.  Returns {"checksum", "elements"}; a no-op outside a process group."""
    cs = tensors_checksum(tensors)
    if dist.is_initialized():
        lo, hi = cs.clone(), cs.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        if not torch.equal(lo, hi):
            raise RuntimeError(f"weight replicas differ across ranks after the broadcast: checksum min {lo.tolist()} "
                               f"max {hi.tolist()} (this rank {cs.tolist()})")
    return {"checksum": int(cs[0].item()), "elements": int(cs[1].item())}


def broadcast_pipeline(pipe, extra: Sequence = (), src: int = 0, bucket_bytes: int = 512 << 20,
                       force: bool = False) -> Dict[str, float]:
    """Start-up weight distribution of one serving process group: broadcast `pipe.tensors()` (+ the `tensors()` of every
    object in `extra`, e.g. the MLLM agent) from rank `src`, drop the UNet's derived packed weights, and verify that all
    ranks ended up bit-identical.  Returns the broadcast stats + {"verify_ms", "checksum", "elements"}."""
    tensors = list(pipe.tensors())
    for m in extra:
        if m is not None:
            tensors += list(m.tensors())
    stats = broadcast_tensors(tensors, src=src, bucket_bytes=bucket_bytes, force=force)
    # the tensors now live in the weight arena (new data pointers) and, on ranks != src, hold new values: every engine
    # drops what it derived from the old storage (packed copies, launch plans with raw pointers)
    names = ("unet", "text_encoder", "text_encoder_2", "image_encoder", "magi_image_encoder", "image_proj_model", "vae")
    for m in [getattr(pipe, n, None) for n in names] + list(extra):
        if m is None or not hasattr(m, "tensors"):
            continue            # not one of this package's engines (e.g. a user-supplied torch module): nothing was re-homed
        if not hasattr(m, "weights_changed"):
            raise TypeError(f"{type(m).__name__} lists tensors() for the weight broadcast but has no weights_changed(): a "
                            f"raw-pointer cache inside it would go stale silently")
        m.weights_changed()
    t0 = time.perf_counter()
    ver = verify_replicas(tensors) if (dist.is_initialized() and (dist.get_world_size() > 1 or force)) else \
        {"checksum": None, "elements": sum(t.numel() for t in tensors)}
    if tensors and tensors[0].is_cuda:
        torch.cuda.synchronize()
    stats.update(ver)
    stats["verify_ms"] = (time.perf_counter() - t0) * 1e3
    stats["tensors"] = len(tensors)
    return stats


@dataclass
class PanelRequest:
    """One `DiffSenseiPipeline.__call__` worth of work."""
    request_id: int
    height: int
    width: int
    num_inference_steps: int = 50
    num_samples: int = 1
    payload: dict = field(default_factory=dict)

    def cost(self) -> float:
        # UNet FLOPs scale ~ linearly in latent pixels below 1024^2 and faster above (self-attention); good enough
        px = self.height * self.width
        return px * (1.0 + px / (2048.0 * 2048.0)) * self.num_inference_steps * self.num_samples


def shard_requests(requests: Sequence[PanelRequest], world_size: int) -> List[List[PanelRequest]]:
    """Deterministic static partition: longest-processing-time-first over ranks; within a rank requests are grouped
    by (height, width) bucket so same-shape panels run back to back on one launch plan (the bucket idea of reference
    src/datasets/dataset_size_bucket.py:488-544, applied to serving)."""
    shards: List[List[PanelRequest]] = [[] for _ in range(world_size)]
    load = [0.0] * world_size
    for r in sorted(requests, key=lambda r: (-r.cost(), r.request_id)):
        k = min(range(world_size), key=lambda i: (load[i], i))
        shards[k].append(r)
        load[k] += r.cost()
    for s in shards:
        s.sort(key=lambda r: (r.height, r.width, r.request_id))
    return shards


class _WirePil:
    """A PIL image on the wire: its pixels as ONE contiguous uint8 array (3 bytes per pixel) instead of a pickled PIL object."""
    __slots__ = ("px",)

    def __init__(self, px):
        self.px = px


def _to_wire(x):
    """What crosses the process boundary in a result gather: uint8 / float arrays, not pickled PIL objects; what was a PIL
    image stays marked as one so that rank 0 can hand back the worker's own types."""
    import numpy as np
    if isinstance(x, (list, tuple)):
        return [_to_wire(v) for v in x]
    if isinstance(x, Tensor):
        return x.detach().cpu().numpy()
    if hasattr(x, "mode") and hasattr(x, "size") and hasattr(x, "tobytes"):   # a PIL image
        return _WirePil(np.ascontiguousarray(np.asarray(x)))
    return x


def _from_wire(x, as_pil: Optional[bool]):
    """`as_pil` None: what the worker produced (PIL stays PIL, arrays stay arrays); True: every uint8 [H,W,1|3|4] array
    becomes a PIL image; False: every image is a uint8 array."""
    import numpy as np
    if isinstance(x, list):
        return [_from_wire(v, as_pil) for v in x]
    was_pil = isinstance(x, _WirePil)
    if was_pil:
        x = x.px
    img_like = isinstance(x, np.ndarray) and x.dtype == np.uint8 and (x.ndim == 2 or (x.ndim == 3 and x.shape[2] in (1, 3, 4)))
    if img_like and (as_pil is True or (as_pil is None and was_pil)):
        from PIL import Image
        return Image.fromarray(x[:, :, 0] if x.ndim == 3 and x.shape[2] == 1 else x)
    return x


def _normalise_local(results: dict, as_pil: Optional[bool]) -> dict:
    """The world_size-1 / gather=False path returns the same TYPES a gather would (the result type used to
    depend on the world size): every result takes the wire round trip without the wire - torch tensors come back as numpy
    arrays, tuples as lists, PIL images as PIL images (or as `as_pil` asks) - exactly what rank 0 receives from eight ranks."""
    return {k: _from_wire(_to_wire(v), as_pil) for k, v in results.items()}


def _gather_results(results: dict, rank: int, world: int, as_pil: Optional[bool]):
    wire = {k: _to_wire(v) for k, v in results.items()}
    gathered: List[Optional[dict]] = [None] * world if rank == 0 else None
    dist.gather_object(wire, gathered, dst=0)
    if rank != 0:
        return None
    out = {}
    for d in gathered:
        out.update({k: _from_wire(v, as_pil) for k, v in d.items()})
    return out


def run_sharded(requests: Sequence[PanelRequest], worker: Callable[[PanelRequest], object], gather: bool = True,
                as_pil: Optional[bool] = None):
    """Every rank runs `worker` on its shard; rank 0 optionally receives all results keyed by request_id.  Gathered images
    travel as uint8 arrays ([H,W,3]); by default (`as_pil` None) rank 0 gets back what the workers produced - PIL images
    stay PIL images - whatever the world size; `as_pil` False asks for the uint8 arrays, True for PIL everywhere."""
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    mine = shard_requests(requests, world)[rank]
    results = {r.request_id: worker(r) for r in mine}
    if not gather or world == 1:
        return _normalise_local(results, as_pil)
    return _gather_results(results, rank, world, as_pil)


def run_sharded_batched(requests: Sequence[PanelRequest], pipe, max_panels: int = 16, max_pixels: Optional[int] = None,
                        output_type: str = "pil", gather: bool = True, as_pil: Optional[bool] = None,
                        mix_scales: bool = False):
    """`run_sharded` for a whole queue: every rank pushes its shard through a `serving.BucketBatcher`, so requests of
    one (size, steps, guidance) bucket share UNet batches on that rank (BASELINE.json configs[3]: mixed-resolution
    queue over the GPUs of a node).  `PanelRequest.payload` holds the other `__call__` keyword arguments.  With
    `gather`, rank 0 receives every request's images (moved as uint8 arrays; `as_pil` as in `run_sharded`: by default the
    result has the types `output_type` asked for, on one rank or on eight).  `mix_scales`: as in `serving.BucketBatcher` -
    requests that differ only in guidance_scale / ip_scale share a batch."""
    from .serving import BucketBatcher
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    mine = shard_requests(requests, world)[rank]
    batcher = BucketBatcher(pipe, max_panels=max_panels, max_pixels=max_pixels, mix_scales=mix_scales)
    for r in mine:
        batcher.submit(height=r.height, width=r.width, num_inference_steps=r.num_inference_steps,
                       num_samples=r.num_samples, **r.payload)
    outs = batcher.run(output_type=output_type)
    results = {r.request_id: o for r, o in zip(mine, outs)}
    if not gather or world == 1:
        return _normalise_local(results, as_pil)
    return _gather_results(results, rank, world, as_pil)
