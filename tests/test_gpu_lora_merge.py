"""GPU: `lora_merge_kernel` (csrc/lora.hip) through `ops.lora_merge` / DS_OP_LORA_MERGE.

Test 1 compares with fp64 on the f16 operands.  Per element
    |out - ref| <= max(2^-11 |ref|, 2^-25) + (R + 2) 2^-24 T,     T = |W| + sum_i |s_i| (|B_i| |A_i|)
- half an f16 ulp (2^-25: half the f16 subnormal spacing) for the one rounding of the result, plus the textbook forward bound
of an fp32 sum of R + 1 exact products (f16 x f16 is exact in fp32; the strength and the add onto f32(W) are two more
roundings).  The bound is derived, not measured: "within one ulp" would be wrong near cancellation.  The share of elements
that differ from f16(ref) at all is gated at 0.5 % (an fp32 emulation on the CPU gives 0 - 0.04 % on these inputs).

Inputs: seeded normal, W std 0.03, A / B std 0.02.  Shapes are the smallest that take every path of the kernel: ragged tile
edges in both dimensions, a rank below one MFMA k-step, a segment boundary off the k-step, a negative strength, the largest
rank at the cross-attention width, many small segments with an empty one, the GEGLU row map with the fused-LayerNorm second
output and a wide leading dimension.

Case "d" has eight ranks and an empty segment between them: nine segments, which is why the launcher takes up to 16 (the
host never merges more than 8 adapters).  Case "e" is case "b" with the `pack_geglu` permutation; that permutation needs
the half to be a multiple of 64, which N = 320 is not, so "e" keeps K, the ranks and the strengths of "b" at N = 384, the
next size it exists for (three 128-row groups, still ragged against the kernel's 64-row tiles through the map).  Ranks
12 + 128 make rows of B that are not 16-byte aligned (element-wise reads), 256 aligned ones (16-byte reads), "d" both in
one matrix.

Test 2 is the rule of tests/test_gpu_poisoned_memory.py for the new op, which has no exported entry point of its own.
"""
import pytest
import torch

from tests._arena import Arena, Plain
from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(N, K, ranks, s=None, seed=0, empty_at=None, geglu=False, ld_extra=0):
    g = torch.Generator().manual_seed(seed)
    R = sum(ranks)
    W = (torch.randn(N, K, generator=g) * 0.03).half()
    A = (torch.randn(R, K, generator=g) * 0.02).half()
    B = (torch.randn(N, R, generator=g) * 0.02).half()
    seg = [0]
    for r in ranks:
        seg.append(seg[-1] + r)
    s = list(s) if s is not None else [1.0] * len(ranks)
    if empty_at is not None:
        seg.insert(empty_at, seg[empty_at])
        s.insert(empty_at, 3.0)
    c = dict(W=W, A=A, B=B, seg=torch.tensor(seg, dtype=torch.int32), s=torch.tensor(s, dtype=torch.float32), map=None,
             colscale=None, ld=K + ld_extra)
    if geglu:
        from diffsensei_amd.engine import pack_geglu
        idx = torch.arange(N, dtype=torch.int32)
        c["map"] = pack_geglu(idx[:, None], idx)[1].contiguous()
        c["colscale"] = (1.0 + 0.1 * torch.randn(K, generator=g)).half()
        c["beta"] = (0.05 * torch.randn(K, generator=g)).half()
    return c


CASES = {
    "a": lambda: _case(136, 72, [4], seed=1),
    "b": lambda: _case(320, 264, [12, 128], [0.75, -0.5], seed=2),
    "c": lambda: _case(256, 2048, [256], seed=3),
    "d": lambda: _case(64, 64, [1, 3, 8, 16, 33, 64, 100, 31], [1.0, -2.0, 0.5, 1.5, -0.25, 0.75, 1.25, -1.0], seed=4, empty_at=4),
    "e": lambda: _case(384, 264, [12, 128], [0.75, -0.5], seed=5, geglu=True, ld_extra=8),
}


def _reference(c):
    """(ref, T) in fp64 from the f16 operands."""
    W, A, B = c["W"].double(), c["A"].double(), c["B"].double()
    if c["map"] is not None:
        W, B = W[c["map"].long()], B[c["map"].long()]
    ref, T = W.clone(), W.abs()
    seg, s = c["seg"].tolist(), c["s"].double().tolist()
    for i in range(len(s)):
        lo, hi = seg[i], seg[i + 1]
        if hi > lo:
            ref += s[i] * (B[:, lo:hi] @ A[lo:hi])
            T += abs(s[i]) * (B[:, lo:hi].abs() @ A[lo:hi].abs())
    return ref, T


def _run(mem, c):
    """The case on `mem` (an Arena or Plain): returns (out, out2 or None)."""
    N, K = c["W"].shape
    W, A, B = mem.place(c["W"]), mem.place(c["A"]), mem.place(c["B"])
    seg, s = mem.place(c["seg"]), mem.place(c["s"])
    mp = None if c["map"] is None else mem.place(c["map"])
    cs = None if c["colscale"] is None else mem.place(c["colscale"])
    out = mem.out((N, K), ld=c["ld"])
    out2 = None if cs is None else mem.out((N, K), ld=c["ld"])
    mem.ops.lora_merge(W, A, B, seg, s, out=out, map=mp, colscale=cs, out2=out2)
    torch.cuda.synchronize()
    return out, out2


@pytest.mark.parametrize("name", list(CASES))
def test_merge_vs_fp64(hip_lib, name):
    c = CASES[name]()
    out, out2 = _run(Plain(DEV), c)
    ref, T = _reference(c)
    R = c["A"].shape[0]
    got = out.double().cpu()
    bound = torch.maximum(ref.abs() * 2.0 ** -11, torch.full_like(ref, 2.0 ** -25)) + (R + 2) * 2.0 ** -24 * T
    err = (got - ref).abs()
    worst = float((err / bound).max())
    differ = float((out.cpu() != ref.half()).double().mean())
    print(f"[lora_merge {name}] max err / bound = {worst:.4g}, share of elements != f16(ref) = {differ:.3e}")
    assert torch.isfinite(got).all()
    assert worst <= 1.0, f"case {name}: error is {worst:.4g} x the derived bound"
    gate(f"lora_merge {name}: share of elements that differ from f16(fp64 reference)", differ, 5e-3)
    assert float((got - c["W"].double()[c["map"].long()] if c["map"] is not None else got - c["W"].double()).abs().max()) > 1e-4, \
        "the adapters left no trace"
    if out2 is not None:
        # the second output equals pack_ln_fused's gamma (.) W copy of the kernel's OWN out, bit for bit
        from diffsensei_amd.engine import pack_ln_fused
        gw = pack_ln_fused(out.contiguous().cpu(), None, c["colscale"], c["beta"])[0]
        assert torch.equal(out2.cpu().view(torch.int16), gw.view(torch.int16))


def test_no_adapter_and_zero_strength_copy_the_base(hip_lib):
    from diffsensei_amd import ops
    c = CASES["b"]()
    W, A, B = c["W"].to(DEV), c["A"].to(DEV), c["B"].to(DEV)
    out = ops.lora_merge(W)                                   # n = 0
    assert torch.equal(out.view(torch.int16), W.view(torch.int16))
    out = ops.lora_merge(W, A[:12].contiguous(), B[:, :12].contiguous(), [0, 12], [0.0])
    assert torch.equal(out, W) and torch.equal(out.view(torch.int16), W.view(torch.int16))
    mp = torch.arange(W.shape[0] - 1, -1, -1, dtype=torch.int32, device=DEV)
    out = ops.lora_merge(W, map=mp)
    assert torch.equal(out, W.flip(0))


def test_aliasing_the_base_is_refused(hip_lib):
    from diffsensei_amd import _lib, ops
    c = CASES["a"]()
    W, A, B = c["W"].to(DEV), c["A"].to(DEV), c["B"].to(DEV)
    before = W.clone()
    with pytest.raises(_lib.DiffSenseiHipError, match="read only"):
        ops.lora_merge(W, A, B, [0, 4], [1.0], out=W)
    cs = torch.ones(W.shape[1], dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.DiffSenseiHipError, match="read only"):
        ops.lora_merge(W, A, B, [0, 4], [1.0], colscale=cs, out2=W)
    torch.cuda.synchronize()
    assert torch.equal(W, before)                             # nothing was launched
    with pytest.raises(_lib.DiffSenseiHipError):
        ops.lora_merge(W.cpu(), A, B, [0, 4], [1.0])


@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_merge_inside_poisoned_memory(hip_lib, name):
    c = CASES[name]()
    results = []
    for mem in (Plain(DEV), Arena(DEV, "nan", capacity=24 << 20), Arena(DEV, "loud", capacity=24 << 20)):
        out, out2 = _run(mem, c)
        mem.check()
        assert torch.isfinite(out).all() and (out2 is None or torch.isfinite(out2).all()), mem.fill
        results.append((out.contiguous().cpu(), None if out2 is None else out2.contiguous().cpu()))
    for out, out2 in results[1:]:
        assert torch.equal(out.view(torch.int16), results[0][0].view(torch.int16))
        if out2 is not None:
            assert torch.equal(out2.view(torch.int16), results[0][1].view(torch.int16))


def test_op_describe(hip_lib):
    import ctypes as C
    from diffsensei_amd import ops
    c = CASES["e"]()
    N, K = c["W"].shape
    t = {k: c[k].to(DEV) for k in ("W", "A", "B", "seg", "s", "map", "colscale")}
    out, out2 = torch.empty(N, K, dtype=torch.float16, device=DEV), torch.empty(N, K, dtype=torch.float16, device=DEV)
    op = ops.lora_merge_op(t["W"], out, t["A"], t["B"], t["seg"], t["s"], t["map"], t["colscale"], out2)
    name, fl, by = C.create_string_buffer(64), C.c_double(), C.c_double()
    assert hip_lib.ds_op_describe(C.byref(op), name, 64, C.byref(fl), C.byref(by)) == 0
    R = c["A"].shape[0]
    assert name.value == b"lora_merge_kernel"
    assert fl.value == 2.0 * N * K * R and by.value == 2.0 * (3.0 * N * K + R * (N + K))
