"""GPU: the MLLM decode kernels (csrc/llm.hip) at the context lengths, widths and vocabulary of the real model.

The other MLLM test files keep every loop of these kernels at one or two iterations (T <= 24, H = 512, V = 3000).  Here
the key-group loop of llm_attn_body (16 wavefronts x KPW keys per iteration: 64 keys at D = 128, 128 at D = 64) and its
softmax loop (1024 keys per iteration) run at, and either side of, their boundaries and up to the launcher's largest cache
(T_max = 8192); llm_rmsnorm_row runs 1, 1 + 8 elements and 2.5 iterations (H = 2048, 2056, 5120); llm_select_body scans
the agent's vocabulary (32330: configs/train/diffsensei/mllm.yaml of the reference, LlamaConfig.vocab_size here) with the
image ids at its end and ties the lowest id of which sits in a higher wavefront, a higher lane or a later scan step.

Attention compares with tests/_llm_attn_ref.py (fp32, same fp16 inputs, the reference model's rounding points) on inputs
whose boundary keys carry a mark; tests/test_llm_attn_ref_host.py shows on the CPU that this reference is exact to 1e-4
and that losing any one boundary key moves the output by >= 10x the gate.  Every comparison is max|err| / max|ref| and
goes through gate(): the bound is min(starting bound, 2.9 x the value measured on MI355X and rounded to 3 digits), the
starting bounds being the per-op bounds of tests/test_gpu_mllm.py (4e-3: fp16 output rounding + accumulation order; 2e-3
for the rotated keys, RMSNorm, SwiGLU and blend, whose sums are short or absent; 3e-2 for hidden states after two fp16
layers).  MEASURED holds the measured value of every gate by name; the kernels use no atomics, so the values repeat.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _llm_attn_ref as A
from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"

# measured on MI355X (gfx950), one entry per gate: max|err| / max|ref|, rounded to 3 digits (0 = bit-identical)
MEASURED = {
    'D128 3/3 row at 63: output': 0.000276,
    'D128 3/3 row at 63: appended keys': 0,
    'D128 3/3 row at 64: output': 0.000227,
    'D128 3/3 row at 64: appended keys': 0,
    'D128 3/3 row at 65: output': 0.000252,
    'D128 3/3 row at 65: appended keys': 0,
    'D128 3/3 row at 1023: output': 0.000193,
    'D128 3/3 row at 1023: appended keys': 0,
    'D128 3/3 row at 1024: output': 0.000221,
    'D128 3/3 row at 1024: appended keys': 0,
    'D128 3/3 chunk over the key-loop boundary: output': 0.00022,
    'D128 3/3 chunk over the key-loop boundary: appended keys': 0,
    'D128 3/3 chunk over the softmax-loop boundary: output': 0.000316,
    'D128 3/3 chunk over the softmax-loop boundary: appended keys': 0,
    'D128 3/3 5 rows ending at T_max: output': 0.000234,
    'D128 3/3 5 rows ending at T_max: appended keys': 0,
    'D128 3/3 chunk at the end of an 8192 cache: output': 0.00034,
    'D128 3/3 chunk at the end of an 8192 cache: appended keys': 0,
    'D128 4/2 row at 63: output': 0.000185,
    'D128 4/2 row at 63: appended keys': 0,
    'D128 4/2 row at 64: output': 0.000247,
    'D128 4/2 row at 64: appended keys': 0,
    'D128 4/2 row at 65: output': 0.000344,
    'D128 4/2 row at 65: appended keys': 0,
    'D128 4/2 row at 1023: output': 0.000342,
    'D128 4/2 row at 1023: appended keys': 0,
    'D128 4/2 row at 1024: output': 0.000173,
    'D128 4/2 row at 1024: appended keys': 0,
    'D128 4/2 chunk over the key-loop boundary: output': 0.00036,
    'D128 4/2 chunk over the key-loop boundary: appended keys': 0,
    'D128 4/2 chunk over the softmax-loop boundary: output': 0.000376,
    'D128 4/2 chunk over the softmax-loop boundary: appended keys': 0,
    'D128 4/2 5 rows ending at T_max: output': 0.000392,
    'D128 4/2 5 rows ending at T_max: appended keys': 7.4e-08,
    'D128 4/2 chunk at the end of an 8192 cache: output': 0.000414,
    'D128 4/2 chunk at the end of an 8192 cache: appended keys': 1.73e-06,
    'D64 4/2 row at 127: output': 0.000247,
    'D64 4/2 row at 127: appended keys': 0,
    'D64 4/2 row at 128: output': 0.000256,
    'D64 4/2 row at 128: appended keys': 0,
    'D64 4/2 row at 129: output': 0.000274,
    'D64 4/2 row at 129: appended keys': 0,
    'D64 4/2 row at 1023: output': 0.000254,
    'D64 4/2 row at 1023: appended keys': 0,
    'D64 4/2 row at 1024: output': 0.000335,
    'D64 4/2 row at 1024: appended keys': 0,
    'D64 4/2 chunk over the key-loop boundary: output': 0.000388,
    'D64 4/2 chunk over the key-loop boundary: appended keys': 0,
    'D64 4/2 chunk over the softmax-loop boundary: output': 0.000199,
    'D64 4/2 chunk over the softmax-loop boundary: appended keys': 0,
    'D64 4/2 5 rows ending at T_max: output': 0.000416,
    'D64 4/2 5 rows ending at T_max: appended keys': 0,
    'D64 8/1 row at 127: output': 0.000314,
    'D64 8/1 row at 127: appended keys': 0,
    'D64 8/1 row at 128: output': 0.00028,
    'D64 8/1 row at 128: appended keys': 0,
    'D64 8/1 row at 129: output': 0.000264,
    'D64 8/1 row at 129: appended keys': 0,
    'D64 8/1 row at 1023: output': 0.000427,
    'D64 8/1 row at 1023: appended keys': 0,
    'D64 8/1 row at 1024: output': 0.000286,
    'D64 8/1 row at 1024: appended keys': 0,
    'D64 8/1 chunk over the key-loop boundary: output': 0.000246,
    'D64 8/1 chunk over the key-loop boundary: appended keys': 0,
    'D64 8/1 chunk over the softmax-loop boundary: output': 0.000351,
    'D64 8/1 chunk over the softmax-loop boundary: appended keys': 0,
    'D64 8/1 5 rows ending at T_max: output': 0.000278,
    'D64 8/1 5 rows ending at T_max: appended keys': 0,
    'D128 3/3 kernel-filled: output, worst launch': 0.000403,
    'D128 3/3 kernel-filled: rotated key cache': 0.000108,
    'D128 4/2 kernel-filled: output, worst launch': 0.000403,
    'D128 4/2 kernel-filled: rotated key cache': 0.000197,
    'D128 3/3 guard: rows inside the cache': 0.000291,
    'D128 3/3 guard: appended keys': 1e-06,
    'D128 4/2 guard: rows inside the cache': 0.000444,
    'D128 4/2 guard: appended keys': 0,
    'D64 4/2 guard: rows inside the cache': 0.000242,
    'D64 4/2 guard: appended keys': 0,
    'D64 8/1 guard: rows inside the cache': 0.000278,
    'D64 8/1 guard: appended keys': 0,
    'D128 3/3 slots: output at length 0': 0,
    'D128 3/3 slots: appended key at length 0': 0,
    'D128 3/3 slots: output at length 64': 0.000227,
    'D128 3/3 slots: appended key at length 64': 0,
    'D128 3/3 slots: output at length 1030': 0.000303,
    'D128 3/3 slots: appended key at length 1030': 0,
    'D128 4/2 slots: output at length 0': 0,
    'D128 4/2 slots: appended key at length 0': 0,
    'D128 4/2 slots: output at length 64': 0.000247,
    'D128 4/2 slots: appended key at length 64': 0,
    'D128 4/2 slots: output at length 1030': 0.000201,
    'D128 4/2 slots: appended key at length 1030': 0,
    'D64 4/2 slots: output at length 0': 0,
    'D64 4/2 slots: appended key at length 0': 0,
    'D64 4/2 slots: output at length 128': 0.000256,
    'D64 4/2 slots: appended key at length 128': 0,
    'D64 4/2 slots: output at length 1030': 0.000412,
    'D64 4/2 slots: appended key at length 1030': 0,
    'D64 8/1 slots: output at length 0': 0,
    'D64 8/1 slots: appended key at length 0': 0,
    'D64 8/1 slots: output at length 128': 0.00028,
    'D64 8/1 slots: appended key at length 128': 0,
    'D64 8/1 slots: output at length 1030': 0.000437,
    'D64 8/1 slots: appended key at length 1030': 0,
    'rmsnorm H=2048 M=1': 0.000284,
    'rmsnorm H=2048 M=5': 0.00038,
    'rmsnorm H=2048 M=37': 0.00037,
    'rmsnorm H=2056 M=1': 0.000287,
    'rmsnorm H=2056 M=5': 0.000253,
    'rmsnorm H=2056 M=37': 0.000407,
    'rmsnorm H=5120 M=1': 0.000276,
    'rmsnorm H=5120 M=5': 0.000349,
    'rmsnorm H=5120 M=37': 0.000385,
    'swiglu I=13824 M=1': 0.000467,
    'swiglu I=13824 M=37': 0.000622,
    'blend n=8': 0.000182,
    'blend n=4392': 0.000454,
    'fed-back hidden states, mfma, graph=True, call 0': 0.00156,
    'fed-back hidden states, mfma, graph=True, call 1': 0.00156,
    'fed-back hidden states, chunks, graph=True, call 0': 0.00115,
    'fed-back hidden states, chunks, graph=True, call 1': 0.00115,
    'fed-back hidden states, mfma, graph=False, call 0': 0.00156,
    'fed-back hidden states, mfma, graph=False, call 1': 0.00156,
    'fed-back hidden states, chunks, graph=False, call 0': 0.00115,
    'fed-back hidden states, chunks, graph=False, call 1': 0.00115,
}


def _g(name, value, start):
    """gate at min(starting bound, 2.9 x the rounded measured value): under 3 x what was measured"""
    return gate(name, value, min(start, 2.9 * MEASURED[name]))


def _h(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).half()


_TABLES = {}


def _rope(D, T_max):
    from oracle import llama_ref as R
    if (D, T_max) not in _TABLES:
        cos, sin = R.rope_tables(D, T_max)
        _TABLES[(D, T_max)] = (cos.to(DEV).contiguous(), sin.to(DEV).contiguous())
    return _TABLES[(D, T_max)]


def _state(pos0):
    return torch.tensor([pos0, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)


def _cache(kr, qkv, n, T_max, D, heads, kv_heads):
    """caches [T_max, kv_heads*D] whose first n rows are the reference's rotated fp16 keys and the raw values"""
    W = kv_heads * D
    kc = torch.zeros(T_max, W, dtype=torch.float16, device=DEV)
    vc = torch.zeros_like(kc)
    kc[:n] = kr[:n].half().reshape(n, W).to(DEV)
    vc[:n] = qkv[:n, (heads + kv_heads) * D:].to(DEV)
    return kc, vc


# ------------------------------------------------------------------------------------------------ attention
ONE_SEQ = [(D, h, kv) + c for D, h, kv in A.CONFIGS for c in A.one_sequence_cases(D)]


@pytest.mark.parametrize("D,heads,kv_heads,name,pos0,M,T_max", ONE_SEQ,
                         ids=[f"D{c[0]}-h{c[1]}kv{c[2]}-pos{c[4]}-M{c[5]}-Tmax{c[6]}" for c in ONE_SEQ])
def test_attention_one_sequence_at_the_loop_boundaries(hip_lib, D, heads, kv_heads, name, pos0, M, T_max):
    """Rows pos0 .. pos0+M-1 on a cache written from the reference: T = pos0+r+1 sits at and either side of the
    key-group loop's boundary (16 KPW keys) and the softmax loop's (1024), inside chunks that straddle them (in-chunk
    keys come from qkv, the others from the cache), at the last row of the cache and at the end of the largest cache."""
    from diffsensei_amd import ops
    tag = f"D{D} {heads}/{kv_heads} {name}"
    T, vcol = pos0 + M, (heads + kv_heads) * D
    qkv = A.planted_qkv(D, heads, kv_heads, T, pos0, A.case_seed(D, heads, kv_heads, pos0, M))
    ref, kr = A.attention_ref(qkv, D, heads, kv_heads, pos0, M)
    kc, vc = _cache(kr, qkv, pos0, T_max, D, heads, kv_heads)
    kc0, vc0 = kc.clone(), vc.clone()
    cos, sin = _rope(D, T_max)
    state = _state(pos0)
    out = ops.llm_attention(qkv[pos0:T].to(DEV).contiguous(), kc, vc, cos, sin, state, heads, kv_heads, 1.0 / math.sqrt(D))
    _g(f"{tag}: output", A.rel_err(out, ref), 4e-3)
    _g(f"{tag}: appended keys", A.rel_err(kc[pos0:T].view(M, kv_heads, D), kr[pos0:T]), 2e-3)
    assert torch.equal(vc[pos0:T].cpu(), qkv[pos0:T, vcol:]), "appended values must be a bit copy"
    assert torch.equal(kc[:pos0], kc0[:pos0]) and torch.equal(vc[:pos0], vc0[:pos0]), "cache rows before pos0 were rewritten"
    assert not kc[T:].any() and not vc[T:].any(), "rows past the cache length were written"
    assert state.tolist() == [pos0, 0, 0, 0, 0, 0, 0, 0], "attention must not move the counters"


@pytest.mark.parametrize("D,heads,kv_heads", [c for c in A.CONFIGS if c[0] == 128])
def test_attention_cache_filled_by_the_kernel(hip_lib, D, heads, kv_heads):
    """300 prompt rows in chunks of 16 + 12, then 3 single tokens, on a cache the kernel itself fills: five key-loop
    iterations, the cache-write path at large pos0.  Every row is compared, each launch against its own max|ref|."""
    from diffsensei_amd import ops
    tag = f"D{D} {heads}/{kv_heads} kernel-filled"
    T, T_max, vcol = sum(A.FILL_ROWS), 320, (heads + kv_heads) * D
    qkv = A.planted_qkv(D, heads, kv_heads, T, 300, A.case_seed(D, heads, kv_heads, 0, T))
    ref, kr = A.attention_ref(qkv, D, heads, kv_heads, 0, T)
    kc = torch.zeros(T_max, kv_heads * D, dtype=torch.float16, device=DEV)
    vc = torch.zeros_like(kc)
    cos, sin = _rope(D, T_max)
    state, qd = _state(0), qkv.to(DEV)
    err, r0 = 0.0, 0
    for m in A.FILL_ROWS:
        out = ops.llm_attention(qd[r0:r0 + m].contiguous(), kc, vc, cos, sin, state, heads, kv_heads, 1.0 / math.sqrt(D))
        ops.llm_advance(state, m)
        err = max(err, A.rel_err(out, ref[r0:r0 + m]))
        r0 += m
    assert int(state[0]) == T
    _g(f"{tag}: output, worst launch", err, 4e-3)
    _g(f"{tag}: rotated key cache", A.rel_err(kc[:T].view(T, kv_heads, D), kr), 2e-3)
    assert torch.equal(vc[:T].cpu(), qkv[:, vcol:]), "value cache must be a bit copy"
    assert not kc[T:].any() and not vc[T:].any(), "rows past the cache length were written"


@pytest.mark.parametrize("D,heads,kv_heads", A.CONFIGS)
def test_attention_rows_past_the_cache_are_left_alone(hip_lib, D, heads, kv_heads):
    """`if (T > p.T_max) return;`: 16 rows at pos0 = 32 on a 40-row cache - rows 0..7 are computed and appended, rows
    8..15 write neither the output nor anything else."""
    from diffsensei_amd import ops
    tag = f"D{D} {heads}/{kv_heads} guard"
    pos0, M, T_max = A.GUARD
    live, vcol = T_max - pos0, (heads + kv_heads) * D
    qkv = A.planted_qkv(D, heads, kv_heads, T_max, pos0, A.case_seed(D, heads, kv_heads, pos0, live))
    ref, kr = A.attention_ref(qkv, D, heads, kv_heads, pos0, live)
    rows = torch.cat([qkv[pos0:], _h((M - live, qkv.shape[1]), torch.Generator().manual_seed(D + heads))])
    kc, vc = _cache(kr, qkv, pos0, T_max, D, heads, kv_heads)
    kc0, vc0 = kc.clone(), vc.clone()
    cos, sin = _rope(D, T_max)
    out = torch.full((M, heads * D), 7.0, dtype=torch.float16, device=DEV)
    ops.llm_attention(rows.to(DEV).contiguous(), kc, vc, cos, sin, _state(pos0), heads, kv_heads, 1.0 / math.sqrt(D), out=out)
    _g(f"{tag}: rows inside the cache", A.rel_err(out[:live], ref), 4e-3)
    assert bool((out[live:] == 7.0).all()), "a row past the cache wrote its output"
    assert torch.equal(kc[:pos0], kc0[:pos0]) and torch.equal(vc[:pos0], vc0[:pos0]), "cache rows 0..31 changed"
    _g(f"{tag}: appended keys", A.rel_err(kc[pos0:].view(live, kv_heads, D), kr[pos0:]), 2e-3)
    assert torch.equal(vc[pos0:].cpu(), qkv[pos0:, vcol:])


@pytest.mark.parametrize("D,heads,kv_heads", A.CONFIGS)
def test_attention_slots_at_the_loop_boundaries(hip_lib, D, heads, kv_heads):
    """Four slots at cache lengths 0, 16 KPW - 1 (finished), 16 KPW and 1030, three padding rows between the slots'
    caches (slot_stride > T_max * ldc): the assertions of test_attention_slots, and every live slot bit-identical to the
    one-sequence kernel on that slot's cache alone."""
    from diffsensei_amd import ops
    from diffsensei_amd._lib import check
    tag = f"D{D} {heads}/{kv_heads} slots"
    lens, fin = A.slot_lengths(D), [0, 1, 0, 0]
    S, T_max, PAD, W, vcol = 4, 1100, 3, kv_heads * D, (heads + kv_heads) * D
    scale = 1.0 / math.sqrt(D)
    cos, sin = _rope(D, T_max)
    kc = torch.full((S, T_max + PAD, W), 5.0, dtype=torch.float16, device=DEV)
    vc = torch.full_like(kc, 5.0)
    hist, refs = [], []
    for s, n in enumerate(lens):
        h = A.planted_qkv(D, heads, kv_heads, n + 1, n, A.case_seed(D, heads, kv_heads, n, 1))
        ref, kr = A.attention_ref(h, D, heads, kv_heads, n, 1)
        kc[s, :T_max], vc[s, :T_max] = _cache(kr, h, n, T_max, D, heads, kv_heads)
        hist.append(h)
        refs.append((ref, kr))
    kc0, vc0 = kc.clone(), vc.clone()
    state = torch.tensor([[lens[s], 1, fin[s], 0, 9, 2, 0, 0] for s in range(S)], dtype=torch.int32, device=DEV)
    state0 = state.clone()
    qkv = torch.stack([hist[s][-1] for s in range(S)]).to(DEV)
    out = torch.full((S, heads * D), 7.0, dtype=torch.float16, device=DEV)
    check(hip_lib.ds_llm_attn_slots_f16(qkv.data_ptr(), qkv.shape[1], kc.data_ptr(), vc.data_ptr(), W, kc.stride(0),
                                        cos.data_ptr(), sin.data_ptr(), out.data_ptr(), heads * D, state.data_ptr(), S,
                                        heads, kv_heads, D, T_max, scale, torch.cuda.current_stream().cuda_stream),
          "ds_llm_attn_slots_f16")
    assert torch.equal(state, state0), "attention must not move the counters"
    assert torch.equal(kc[:, T_max:], kc0[:, T_max:]) and torch.equal(vc[:, T_max:], vc0[:, T_max:]), "padding written"
    for s in range(S):
        T = lens[s] + 1
        if fin[s]:
            assert torch.equal(kc[s], kc0[s]) and torch.equal(vc[s], vc0[s]), "a finished slot's cache was written"
            assert bool((out[s] == 7.0).all()), "a finished slot's output row was written"
            continue
        ref, kr = refs[s]
        _g(f"{tag}: output at length {lens[s]}", A.rel_err(out[s:s + 1], ref), 4e-3)
        _g(f"{tag}: appended key at length {lens[s]}", A.rel_err(kc[s, T - 1:T].view(1, kv_heads, D), kr[T - 1:T]), 2e-3)
        assert torch.equal(vc[s, :T].cpu(), hist[s][:, vcol:]), "value cache must be a bit copy"
        assert torch.equal(kc[s, :T - 1], kc0[s, :T - 1]), "rows before the new one were rewritten"
        assert not kc[s, T:T_max].any() and not vc[s, T:T_max].any(), "rows past the slot's length were written"
        k1, v1 = kc0[s, :T_max].clone(), vc0[s, :T_max].clone()
        o1 = ops.llm_attention(qkv[s:s + 1].contiguous(), k1, v1, cos, sin, _state(lens[s]), heads, kv_heads, scale)
        assert torch.equal(out[s], o1[0]), f"slot {s} differs from the one-sequence kernel"
        assert torch.equal(kc[s, :T_max], k1) and torch.equal(vc[s, :T_max], v1), f"slot {s}: caches differ"


# ------------------------------------------------------------------------------------------------ width loops
def _rms_ref(x, gam, eps):
    return gam.float() * (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)).half().float()


@pytest.mark.parametrize("M", [1, 5, 37])
@pytest.mark.parametrize("H", [2048, 2056, 5120])
def test_rmsnorm_at_model_widths(hip_lib, H, M):
    """llm_rmsnorm_row strides by 2048: exactly one iteration, one and 8 elements, 2.5 (the 13B width)."""
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(H + M)
    x, gam = _h((M, H), g, 3.0), (1 + 0.1 * torch.randn(H, generator=g)).half()
    y = ops.llm_rmsnorm(x.to(DEV), gam.to(DEV), 1e-6)
    _g(f"rmsnorm H={H} M={M}", A.rel_err(y, _rms_ref(x, gam, 1e-6)), 2e-3)
    assert torch.equal(ops.llm_rmsnorm_slots(x.to(DEV), gam.to(DEV), 1e-6), y), "slots: same rows as the one-sequence kernel"


def test_rmsnorm_feature_tap_at_the_13b_width(hip_lib):
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(11)
    S, H, cap = 5, 5120, 4
    x, gam = _h((S, H), g, 3.0).to(DEV), (1 + 0.1 * torch.randn(H, generator=g)).half().to(DEV)
    y = ops.llm_rmsnorm(x, gam, 1e-6)
    feat = torch.zeros(cap, H, dtype=torch.float16, device=DEV)
    state = torch.tensor([0, 3, 0, 0, 9, 2, 0, 0], dtype=torch.int32, device=DEV)       # 3 ids out -> feature row 2
    y0 = ops.llm_rmsnorm(x[:1], gam, 1e-6, feat=feat, state=state)
    assert torch.equal(y0[0], y[0]) and torch.equal(feat[2], y[0]) and not feat[[0, 1, 3]].any()
    feats = torch.zeros(S, cap, H, dtype=torch.float16, device=DEV)
    rows = [[0, 3, 0, 0, 9, 2, 0, 0], [5, 1, 0, 0, 9, 2, 0, 0], [2, 2, 1, 0, 9, 2, 0, 0], [7, 4, 0, 0, 9, 2, 0, 0],
            [1, 0, 0, 0, 9, 2, 0, 0]]                                                   # slot 2 finished, slot 4: no id yet
    ys = ops.llm_rmsnorm_slots(x, gam, 1e-6, feat=feats, state=torch.tensor(rows, dtype=torch.int32, device=DEV))
    assert torch.equal(ys, y)
    for s, row in ((0, 2), (1, 0), (3, 3)):
        others = [r for r in range(cap) if r != row]
        assert torch.equal(feats[s, row], y[s]) and not feats[s, others].any(), f"slot {s}"
    assert not feats[2].any() and not feats[4].any(), "a finished slot / a slot without an id writes no feature row"


@pytest.mark.parametrize("M", [1, 37])
def test_swiglu_at_the_13b_width(hip_lib, M):
    from diffsensei_amd import ops
    I = 13824
    gu = _h((M, 2 * I), torch.Generator().manual_seed(M), 2.0)
    _g(f"swiglu I={I} M={M}", A.rel_err(ops.llm_swiglu(gu.to(DEV)), F.silu(gu[:, :I].float()) * gu[:, I:].float()), 2e-3)


def test_embed_at_the_13b_width(hip_lib):
    from diffsensei_amd import ops
    H, V = 5120, 1031
    table = _h((V, H), torch.Generator().manual_seed(2)).to(DEV)
    toks = [0, V - 1, 517]
    for tok in toks:
        out = torch.full((H,), 7.0, dtype=torch.float16, device=DEV)
        ops.llm_embed(table, torch.tensor([0, 0, 0, tok, 0, 0, 0, 0], dtype=torch.int32, device=DEV), out)
        assert torch.equal(out, table[tok]), f"row {tok} must be a bit copy"
    state = torch.tensor([[s, 0, 0, tok, 9, 2, 0, 0] for s, tok in enumerate(toks)], dtype=torch.int32, device=DEV)
    out = torch.full((len(toks), H), 7.0, dtype=torch.float16, device=DEV)
    ops.llm_embed_slots(table, state, out)
    assert torch.equal(out, table[toks]), "row s is embed[state[s][3]]"


@pytest.mark.parametrize("n", [8, 2 * 2048 + 8 * 37])      # one thread; two full 256 x 8 blocks and 37 threads of a third
def test_blend_one_vector_and_a_ragged_last_block(hip_lib, n):
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(n)
    a, b = _h((n,), g), _h((n,), g)
    _g(f"blend n={n}", A.rel_err(ops.blend(a.to(DEV), b.to(DEV), 0.3), a.float() * 0.3 + b.float() * 0.7), 2e-3)


# ------------------------------------------------------------------------------------------------ selection
N_CHAIN = 18            # <img>, 16 image ids, </img>: the last ids of the vocabulary, where the real ones are


def _select_cases(V):
    """(name, logits fp16 [V], prev, use_chain, expected id or None = whatever the reference says)"""
    g = torch.Generator().manual_seed(V)
    base = -torch.rand(V, generator=g) - 0.5                                            # everything negative
    chain = list(range(V - N_CHAIN, V))
    cases = []
    for i in (0, V - 1, 1023, 1024):
        if i < V:
            lg = base.clone(); lg[i] = 3.0
            cases.append((f"maximum alone at {i}", lg, 5, False, i))
            cases.append((f"maximum at {i}, processor on", lg, 5, True, None))
    for lo, hi, why in ((1500, 2050, "lower id in a higher wavefront"), (5, 1025, "lower id in the higher lane"),
                        (7, 1031, "same thread, two scan steps")):
        if hi < V:
            lg = base.clone(); lg[lo] = 3.0; lg[hi] = 3.0
            cases.append((f"tie {lo}/{hi}: {why}", lg, 5, False, lo))
            cases.append((f"tie {lo}/{hi}, processor on", lg, 5, True, lo))
    big = base.clone(); big[700] = 4.0; big[chain[3]] = 9.0
    for q in (0, 7, N_CHAIN - 2):
        cases.append((f"forced chain step {q}", big, chain[q], True, chain[q + 1]))
    cases.append(("image ids zeroed, all else negative", base, 5, True, chain[1]))
    cases.append(("a large image-id logit is zeroed", big, 5, True, 700))
    cases.append(("</img> forces nothing", big, chain[-1], True, 700))
    cases.append(("no processor: plain argmax", big, 5, False, chain[3]))
    ninf = torch.full((V,), float("-inf")); ninf[V - 1] = -2.5
    cases.append(("-inf everywhere but the last id", ninf, 5, False, V - 1))
    ninf = torch.full((V,), float("-inf")); ninf[300] = -1.0
    cases.append(("-inf row, processor on", ninf, 5, True, None))
    return chain, [(n, lg.half(), p, c, e) for n, lg, p, c, e in cases]


@pytest.mark.parametrize("V", [1024, 1025, 32330])
def test_select_over_the_agent_vocabulary(hip_lib, V):
    """llm_select and llm_select_slots (ldl > V, the row padding holds a huge logit) against
    oracle.llama_ref.image_token_processor + argmax on the same fp16 logits; ties go to the lowest id wherever it sits."""
    from diffsensei_amd import ops
    from diffsensei_amd._lib import check
    from oracle import llama_ref as R
    chain_ids, cases = _select_cases(V)
    chain = torch.tensor(chain_ids, dtype=torch.int32, device=DEV)
    S, cap, ldl, adv = len(cases), 4, V + 13, 1
    want_state, want_ids = [], []
    logits_b = torch.full((S, ldl), 60000.0, dtype=torch.float16, device=DEV)
    state_b = torch.zeros(S, 8, dtype=torch.int32, device=DEV)
    for s, (name, lg, prev, use_chain, expect) in enumerate(cases):
        scores = lg.float()
        want = int((R.image_token_processor(prev, scores, chain_ids) if use_chain else scores).argmax())
        assert expect is None or want == expect, (name, want, expect)
        assert 0 <= want < V
        n_out = s % 3
        row = [10 + s, n_out, 0, prev, 8, 2, 0, 0]
        want_state.append([10 + s + adv, n_out + 1, 0, want, 8, 2, 0, 0])
        want_ids.append([want if i == n_out else -1 for i in range(cap)])
        logits_b[s, :V] = lg.to(DEV)
        state_b[s] = torch.tensor(row, dtype=torch.int32)
    for use_chain in (True, False):                         # the one-slot kernel, case by case
        for s, (name, lg, prev, uc, _) in enumerate(cases):
            if uc != use_chain:
                continue
            buf = torch.full((ldl,), 60000.0, dtype=torch.float16, device=DEV)
            buf[:V] = lg.to(DEV)
            st = state_b[s].clone()
            ids = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
            ops.llm_select(buf[:V], chain if use_chain else None, adv, st, ids)
            assert st.tolist() == want_state[s], (V, name, st.tolist(), want_state[s])
            assert ids.tolist() == want_ids[s], (V, name, ids.tolist())
    for use_chain in (True, False):                         # the same cases, one per slot, one launch per chain setting
        idx = [s for s, c in enumerate(cases) if c[3] == use_chain]
        lb, sb = logits_b[idx].contiguous(), state_b[idx].contiguous()
        ids = torch.full((len(idx), cap), -1, dtype=torch.int32, device=DEV)
        check(hip_lib.ds_llm_select_slots_f16(lb.data_ptr(), ldl, V, chain.data_ptr() if use_chain else None,
                                              N_CHAIN if use_chain else 0, cap, adv, sb.data_ptr(), ids.data_ptr(),
                                              len(idx), torch.cuda.current_stream().cuda_stream), "ds_llm_select_slots_f16")
        assert sb.tolist() == [want_state[s] for s in idx], (V, use_chain, sb.tolist())
        assert ids.tolist() == [want_ids[s] for s in idx], (V, use_chain, ids.tolist())


# ------------------------------------------------------------------------------------------------ engine
PROMPT_ROWS, MAX_NEW, EOS = 300, 24, 2
PROMPT_SEEDS = {300: 43, 130: 51, 17: 52}


def _prompt_ids(n):
    return torch.randint(3, 590, (n,), generator=torch.Generator().manual_seed(PROMPT_SEEDS[n]))


@pytest.fixture(scope="module")
def tiny(hip_lib):
    from oracle import llama_ref as R
    from oracle import make_golden_mllm as G
    from diffsensei_amd.mllm import LlamaConfig, LlamaDecodeEngine
    cfg = LlamaConfig(vocab_size=G.TINY["vocab_size"], hidden_size=G.TINY["hidden_size"],
                      intermediate_size=G.TINY["intermediate_size"], num_hidden_layers=G.TINY["num_hidden_layers"],
                      num_attention_heads=G.TINY["num_attention_heads"], rms_norm_eps=G.TINY["rms_norm_eps"])
    sd = G.tiny_weights()

    def mk(graph, path="mfma", sequences=1):
        eng = LlamaDecodeEngine(cfg, sd, DEV, max_positions=384, max_new_tokens=MAX_NEW, use_graph=graph, poll_every=4,
                                prompt_path=path, max_sequences=sequences)
        eng.set_image_token_chain(G.IMG_IDS)
        return eng

    ids = _prompt_ids(PROMPT_ROWS)
    emb = sd["model.embed_tokens.weight"].half()[ids]                                     # the engine's table rows
    ref = R.greedy_generate(sd, R.LlamaRefConfig(**G.TINY), emb.float(), int(ids[-1]), G.IMG_IDS, EOS, MAX_NEW)
    return {"mk": mk, "ids": ids, "ref": ref}


@pytest.mark.parametrize("path", ["mfma", "chunks"])
@pytest.mark.parametrize("graph", [True, False])
def test_generate_after_a_300_row_prompt(tiny, graph, path):
    """Tiny model (D = 128), 300 prompt rows, 24 new tokens: five and six key-loop iterations in the prompt chunks and in
    the token loop.  Every oracle margin of this prompt is above the fp16 logit noise (minimum 0.174), so all ids match."""
    ids, ref = tiny["ids"], tiny["ref"]
    assert float(ref["margins"].min()) >= 5e-2 and len(ref["ids"]) == MAX_NEW, float(ref["margins"].min())
    eng = tiny["mk"](graph, path)
    for rep in range(2):                                                                  # 2nd call replays the graph
        out = eng.generate(eng.embed_tokens(ids), int(ids[-1]), EOS, MAX_NEW)
        got, want, margins = out["ids"].tolist(), ref["ids"].tolist(), ref["margins"].tolist()
        for i, (a, b) in enumerate(zip(got, want)):                                       # the rule of _check_ids
            assert a == b or margins[i] < 5e-2, f"id {i} is {a}, oracle {b} (margin {margins[i]:.3g})"
        assert got == want
        info = eng.last_run_info
        assert info["prompt_tokens"] == PROMPT_ROWS and info["graph"] == graph
        _g(f"fed-back hidden states, {path}, graph={graph}, call {rep}", A.rel_err(out["hidden"], ref["hidden"]), 3e-2)


def test_batch_of_long_and_short_prompts_equals_each_alone(tiny):
    """Prompts of 17, 130 and 300 rows in one generate_batch call: every sequence bit for bit what the engine returns for
    it alone, in another slot and among other neighbours (the equality of
    test_a_sequence_does_not_depend_on_its_slot_or_its_neighbours)."""
    eng = tiny["mk"](True, sequences=4)
    prompts = [_prompt_ids(n) for n in (17, 130, 300)]
    embs = lambda which: [eng.embed_tokens(prompts[k]) for k in which]
    last = lambda which: [int(prompts[k][-1]) for k in which]
    first = eng.generate_batch(embs([0, 1, 2]), last([0, 1, 2]), EOS, MAX_NEW)
    assert eng.last_run_info["sequences"] == 3 and eng.last_run_info["prompt_tokens"] == [17, 130, 300]
    assert first[2]["ids"].tolist() == tiny["ref"]["ids"].tolist(), "the 300-row prompt decodes to the oracle's ids"
    for k in range(3):
        alone = eng.generate_batch(embs([k]), last([k]), EOS, MAX_NEW)[0]
        assert eng.last_run_info["sequences"] == 1
        other = eng.generate_batch(embs([k]), last([k]), EOS, MAX_NEW, slots=[3])[0]
        for what, got in (("alone in slot 0", alone), ("alone in slot 3", other)):
            assert torch.equal(got["ids"], first[k]["ids"]), (k, what)
            assert torch.equal(got["hidden"], first[k]["hidden"]), (k, what)
    order = [2, 0, 1]
    mixed = eng.generate_batch(embs(order), last(order), EOS, MAX_NEW)
    for pos, k in enumerate(order):
        assert torch.equal(mixed[pos]["ids"], first[k]["ids"]) and torch.equal(mixed[pos]["hidden"], first[k]["hidden"])
