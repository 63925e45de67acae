"""GPU: the fp8-cache form of the MLLM decode attention (csrc/llm.hip: llm_attn_body<D, true>; ds_llm_attn_kv8 and
ds_llm_attn_slots_kv8) at the op level.

The format's reference is `diffsensei_amd.mllm.quantize_kv_fp8` (pinned on the CPU by tests/test_mllm_kv8_host.py) and the
mode's reference is attention over the dequantised cache (tests/_kv8_ref.attention_over_cache_ref).  The kernel reads 8
codes per lane, so its loop constants and seams are those of the fp16 kernel: the shapes, planted inputs and case lists are
tests/_llm_attn_ref.py's, with T_max <= 1100.

1. exact quantiser  - rotary tables cos = 1, sin = 0 (the rotation is then exact): K and V codes and exponent bytes in the cache
                      equal quantize_kv_fp8 of the input bit for bit.
2. real tables      - V still bit for bit; every K exponent byte equal; at most 1e-4 of the K codes differ from quantize_kv_fp8
                      of the reference's rotated fp16 keys, each by one code (a condition, not a measurement: two CPU
                      restatements of the rotation disagree on 0 to 2e-6 of the codes and on no exponent).  `_check_kv` applies
                      it to every launch of this file.
3. outputs          - against attention_over_cache_ref over the cache bytes read back after the launch and dequantised on the
                      host, on planted inputs at the seams of the kernel's loops, through gate() at min(4e-3, 2.9 x measured)
                      (the fp16 kernel's starting bound; MEASURED holds the table, the convention of
                      test_gpu_llm_long_context.py).
4. chunking         - the 300 + 3 rows of _llm_attn_ref.FILL_ROWS fed so and as 43 chunks of 7 and one of 2: the same cache bytes, and
                      outputs that are BIT-IDENTICAL (asserted; measured so on MI355X): a chunk's own rows go through the
                      quantiser in registers and then through the arithmetic of a cached row.
5. guards           - rows that would pass T_max write nothing (sentinel bytes behind codes and exponents intact); a finished
                      slot's codes, exponents and output row are untouched; the state counters do not move.
6. poisoned memory  - both entry points inside the arena of tests/_arena.py (the cases join tests/test_gpu_poisoned_memory.py's
                      list, whose completeness test asks every entry of _lib.SIGNATURES for one).  The arena's uint8 fills are
                      loud here: 0xFF is e4m3's NaN as a code and 2^128 as an exponent byte; 0x01 is a code of 2^-9 and a scale
                      of 2^-126, a key whose score is 0 and takes a share of the softmax - and the three runs must agree bit
                      for bit.
"""
import functools
import math
import types

import pytest
import torch

from tests import _kv8_ref as K8
from tests import _llm_attn_ref as A
from tests._gates import gate

try:
    import test_gpu_poisoned_memory as P          # the module object pytest itself collects (tests/ is on sys.path)
except ImportError:                               # collected under another import mode
    from tests import test_gpu_poisoned_memory as P

DEV = "cuda"
NS = types.SimpleNamespace
CONFIGS = A.CONFIGS
SENTINEL = 0xA5
CODE_MISMATCH_CAP = 1e-4

# measured on MI355X (gfx950): max|err| / max|ref| of every output gate, rounded to 3 digits
MEASURED = {
    'D128 3/3 row at 63: output': 0.000293,
    'D128 3/3 row at 64: output': 0.000297,
    'D128 3/3 row at 65: output': 0.000267,
    'D128 3/3 row at 1023: output': 0.000315,
    'D128 3/3 row at 1024: output': 0.000179,
    'D128 3/3 chunk over the key-loop boundary: output': 0.000221,
    'D128 3/3 chunk over the softmax-loop boundary: output': 0.000322,
    'D128 3/3 5 rows ending at T_max: output': 0.000353,
    'D128 4/2 row at 63: output': 0.000209,
    'D128 4/2 row at 64: output': 0.000263,
    'D128 4/2 row at 65: output': 0.000338,
    'D128 4/2 row at 1023: output': 0.000196,
    'D128 4/2 row at 1024: output': 0.000223,
    'D128 4/2 chunk over the key-loop boundary: output': 0.000432,
    'D128 4/2 chunk over the softmax-loop boundary: output': 0.000384,
    'D128 4/2 5 rows ending at T_max: output': 0.000309,
    'D64 4/2 row at 127: output': 0.000259,
    'D64 4/2 row at 128: output': 0.00026,
    'D64 4/2 row at 129: output': 0.000268,
    'D64 4/2 row at 1023: output': 0.000252,
    'D64 4/2 row at 1024: output': 0.000293,
    'D64 4/2 chunk over the key-loop boundary: output': 0.00042,
    'D64 4/2 chunk over the softmax-loop boundary: output': 0.000349,
    'D64 4/2 5 rows ending at T_max: output': 0.000333,
    'D64 8/1 row at 127: output': 0.000295,
    'D64 8/1 row at 128: output': 0.000334,
    'D64 8/1 row at 129: output': 0.000259,
    'D64 8/1 row at 1023: output': 0.000432,
    'D64 8/1 row at 1024: output': 0.000209,
    'D64 8/1 chunk over the key-loop boundary: output': 0.000248,
    'D64 8/1 chunk over the softmax-loop boundary: output': 0.000314,
    'D64 8/1 5 rows ending at T_max: output': 0.000344,
    'D128 3/3 slots: output at length 0': 0.0,
    'D128 3/3 slots: output at length 64': 0.000297,
    'D128 3/3 slots: output at length 1030': 0.000373,
    'D128 4/2 slots: output at length 0': 0.0,
    'D128 4/2 slots: output at length 64': 0.000263,
    'D128 4/2 slots: output at length 1030': 0.000259,
    'D64 4/2 slots: output at length 0': 0.0,
    'D64 4/2 slots: output at length 128': 0.00026,
    'D64 4/2 slots: output at length 1030': 0.000214,
    'D64 8/1 slots: output at length 0': 0.0,
    'D64 8/1 slots: output at length 128': 0.000334,
    'D64 8/1 slots: output at length 1030': 0.000291,
    'D128 3/3 kernel-filled: output, worst launch': 0.000506,
    'D128 3/3 kernel-filled: the other chunking against the first': 0.0,
    'D128 4/2 kernel-filled: output, worst launch': 0.000368,
    'D128 4/2 kernel-filled: the other chunking against the first': 0.0,
    'D128 3/3 guard: output': 0.000302,
    'D128 4/2 guard: output': 0.000242,
    'D64 4/2 guard: output': 0.000257,
    'D64 8/1 guard: output': 0.000278,
}


def _g(name, value):
    """gate at min(4e-3, 2.9 x the rounded measured value); 4e-3 is the fp16 kernel's starting bound"""
    return gate(name, value, min(4e-3, 2.9 * MEASURED[name]) if name in MEASURED else 4e-3)


_TABLES = {}


def _rope(D, T_max, identity=False):
    from oracle import llama_ref as R
    key = (D, T_max, identity)
    if key not in _TABLES:
        cos, sin = R.rope_tables(D, T_max)
        if identity:
            cos, sin = torch.ones_like(cos), torch.zeros_like(sin)
        _TABLES[key] = (cos.to(DEV).contiguous(), sin.to(DEV).contiguous())
    return _TABLES[key]


def _state(pos0):
    return torch.tensor([pos0, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)


def _cache(kr, v, n, T_max, pad=0):
    """(kc, vc, ke, ve) on the device: [T_max + pad] rows, the first n hold quantize_kv_fp8 of the rotated fp16 keys kr and of
    the values v ([>= n, kv_heads, D]), the rows up to T_max are zero, the pad rows hold the sentinel"""
    from diffsensei_amd.mllm import quantize_kv_fp8
    Hkv, D = kr.shape[1], kr.shape[2]
    kc = torch.zeros(T_max + pad, Hkv * D, dtype=torch.uint8)
    ke = torch.zeros(T_max + pad, Hkv, dtype=torch.uint8)
    vc, ve = kc.clone(), ke.clone()
    if n:
        (c, e), (c2, e2) = quantize_kv_fp8(kr[:n]), quantize_kv_fp8(v[:n])
        kc[:n], ke[:n], vc[:n], ve[:n] = c.view(n, -1), e, c2.view(n, -1), e2
    for t in (kc, vc, ke, ve):
        t[T_max:] = SENTINEL
    return [t.to(DEV) for t in (kc, vc, ke, ve)]


def _check_kv(what, kc, ke, vc, ve, kr, v):
    """Cases 1 / 2 on rows of the cache (CPU uint8 [n, kv*D] / [n, kv]) against the rotated fp16 keys kr and values v
    [n, kv, D]: V bit for bit, K exponents equal, K codes within the cap and one code apart.  Returns the mismatches."""
    from diffsensei_amd.mllm import quantize_kv_fp8
    n, Hkv, D = kr.shape
    (wk, wke), (wv, wve) = quantize_kv_fp8(kr), quantize_kv_fp8(v)
    assert torch.equal(vc.view(n, Hkv, D), wv) and torch.equal(ve, wve), f"{what}: V codes / exponents are not the host quantiser's"
    assert torch.equal(ke, wke), f"{what}: a K exponent byte differs from the reference's"
    got = kc.view(n, Hkv, D)
    bad = got != wk
    nbad = int(bad.sum())
    print(f"[kv8] {what}: {nbad} of {bad.numel()} K codes differ")
    assert nbad <= CODE_MISMATCH_CAP * bad.numel(), f"{what}: {nbad} of {bad.numel()} K codes differ from the reference's"
    if nbad:                                      # sign + magnitude codes: the neighbour is +-1 on the byte, same sign
        a, b = got[bad].to(torch.int32), wk[bad].to(torch.int32)
        assert bool(((a - b).abs() == 1).all()) and bool(((a ^ b) & 0x80 == 0).all()), f"{what}: a K code is more than one code away"
    return nbad


def _deq(kc, ke, vc, ve, Hkv, D):
    from diffsensei_amd.mllm import dequantize_kv_fp8
    n = kc.shape[0]
    return dequantize_kv_fp8(kc.view(n, Hkv, D), ke), dequantize_kv_fp8(vc.view(n, Hkv, D), ve)


def _spread_rows(T, W, D, seed):
    """fp16 [T, W]: Gaussian heads whose magnitudes are spread over fp16's range, an all-zero head, heads with fp16's largest
    and smallest values"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, W, generator=g) * torch.pow(2.0, torch.randint(-20, 13, (T, W // D), generator=g).float()).repeat_interleave(D, 1)
    x = x.clamp(-65504, 65504).half()
    x[1, :D] = 0
    x[2, :D] = 0
    x[2, 5] = 65504.0
    x[3, :D] = 0
    x[3, 7] = -(2.0 ** -24)
    x[4, 3] = 65504.0
    return x


# ------------------------------------------------------------------------------------------------ 1. exact quantiser
@pytest.mark.gpu
@pytest.mark.parametrize("D,heads,kv_heads", CONFIGS)
def test_appended_codes_and_exponents_are_the_host_quantisers_bit_for_bit(hip_lib, D, heads, kv_heads):
    """cos = 1, sin = 0: the rotation is exact, so K as well as V must come out as quantize_kv_fp8 of the input, bit for bit:
    a 16-row chunk into an empty cache, one behind 40 cached rows, and the slot form at lengths (0, 40)."""
    from diffsensei_amd import ops
    T_max, W, scale = 64, kv_heads * D, 1.0 / math.sqrt(D)
    cos, sin = _rope(D, T_max, identity=True)
    qkv = _spread_rows(56, (heads + 2 * kv_heads) * D, D, D + heads)
    qkv[:, :heads * D] = (qkv[:, :heads * D].float().clamp(-4, 4) * 0.25).half()         # q stays small: finite scores
    # The rotation k cos + rotate_half(k) sin is exact with these tables except for the sign of a zero: -0 * 1 + (+0) is +0.  K
    # therefore carries no negative zero here (12 of the first 16 rows' zeros were, 5 of them came back positive from the
    # device, as the same expression does on the CPU); V, a bit copy, keeps its negative zeros and must store them as 0x80.
    kcols = qkv[:, heads * D:(heads + kv_heads) * D]
    kcols[kcols == 0] = 0.0
    assert bool(((qkv[:, (heads + kv_heads) * D:] == 0) & torch.signbit(qkv[:, (heads + kv_heads) * D:])).any())
    _, k, v = A.split_qkv(qkv, D, heads, kv_heads)
    for pos0 in (0, 40):
        kc, vc, ke, ve = _cache(k, v, pos0, T_max)
        state = _state(pos0)
        ops.llm_attention_kv8(qkv[pos0:pos0 + 16].to(DEV).contiguous(), kc, vc, ke, ve, cos, sin, state, heads, kv_heads, scale)
        rows = slice(pos0, pos0 + 16)
        n = _check_kv(f"D{D} {heads}/{kv_heads} exact, pos0 {pos0}", kc[rows].cpu(), ke[rows].cpu(), vc[rows].cpu(), ve[rows].cpu(),
                      k[rows], v[rows])
        assert n == 0, "with an exact rotation no K code may differ"
        assert not kc[pos0 + 16:].any() and not ke[pos0 + 16:].any() and not vc[pos0 + 16:].any() and not ve[pos0 + 16:].any()
        assert state.tolist() == [pos0, 0, 0, 0, 0, 0, 0, 0]
    lens = (0, 40)
    cs = [_cache(k, v, n, T_max) for n in lens]
    kc, vc, ke, ve = [torch.stack([c[i] for c in cs]).contiguous() for i in range(4)]
    state = torch.tensor([[n, 1, 0, 0, 9, 2, 0, 0] for n in lens], dtype=torch.int32, device=DEV)
    rows = torch.stack([qkv[n] for n in lens]).to(DEV)
    ops.llm_attention_slots_kv8(rows, kc, vc, ke, ve, cos, sin, state, heads, kv_heads, scale)
    for s, n in enumerate(lens):
        r = slice(n, n + 1)
        assert _check_kv(f"D{D} {heads}/{kv_heads} exact, slot at {n}", kc[s, r].cpu(), ke[s, r].cpu(), vc[s, r].cpu(), ve[s, r].cpu(),
                         k[r], v[r]) == 0
        assert not kc[s, n + 1:].any() and not ke[s, n + 1:].any()


# ------------------------------------------------------------------------------------------------ 2 + 3. real tables, outputs
def _one_sequence(tag, D, heads, kv_heads, pos0, M, T_max, pad=0, M_launch=None):
    """One launch of M_launch (default M) rows at pos0 on a cache holding the quantised reference rows 0 .. pos0-1; checks 2,
    3 and the write guards on the M rows that fit.  Returns (out, caches)."""
    from diffsensei_amd import ops
    T = pos0 + M
    qkv = A.planted_qkv(D, heads, kv_heads, T, pos0, A.case_seed(D, heads, kv_heads, pos0, M))
    q, k, v = A.split_qkv(qkv, D, heads, kv_heads)
    kr = K8.rotated_keys_ref(k)
    kc, vc, ke, ve = _cache(kr, v, pos0, T_max, pad)
    before = [t.clone() for t in (kc, vc, ke, ve)]
    cos, sin = _rope(D, T_max)
    state = _state(pos0)
    rows = qkv[pos0:T]
    if M_launch and M_launch > M:                                   # rows that would pass the end of the cache
        rows = torch.cat([rows, (torch.randn(M_launch - M, qkv.shape[1], generator=torch.Generator().manual_seed(D + heads))).half()])
    out = torch.full((rows.shape[0], heads * D), 7.0, dtype=torch.float16, device=DEV)
    ops.llm_attention_kv8(rows.to(DEV).contiguous(), kc[:T_max], vc[:T_max], ke[:T_max], ve[:T_max], cos, sin, state, heads, kv_heads,
                          1.0 / math.sqrt(D), out=out)
    got = [t.cpu() for t in (kc, vc, ke, ve)]
    _check_kv(tag, got[0][pos0:T], got[2][pos0:T], got[1][pos0:T], got[3][pos0:T], kr[pos0:T], v[pos0:T])
    kd, vd = _deq(got[0][:T], got[2][:T], got[1][:T], got[3][:T], kv_heads, D)
    _g(f"{tag}: output", A.rel_err(out[:M], K8.attention_over_cache_ref(q[pos0:T], kd, vd, pos0)))
    for t, b in zip((kc, vc, ke, ve), before):
        assert torch.equal(t[:pos0], b[:pos0]), f"{tag}: cache rows before pos0 were rewritten"
        assert torch.equal(t[T:], b[T:]), f"{tag}: rows past the appended ones were written"
    assert bool((out[M:] == 7.0).all()), f"{tag}: a row past the cache wrote its output"
    assert state.tolist() == [pos0, 0, 0, 0, 0, 0, 0, 0], "attention must not move the counters"
    return out


ONE_SEQ = [(D, h, kv) + c for D, h, kv in CONFIGS for c in A.one_sequence_cases(D) if c[3] <= 1100]


@pytest.mark.gpu
@pytest.mark.parametrize("D,heads,kv_heads,name,pos0,M,T_max", ONE_SEQ,
                         ids=[f"D{c[0]}-h{c[1]}kv{c[2]}-pos{c[4]}-M{c[5]}" for c in ONE_SEQ])
def test_attention_over_the_dequantised_cache_at_the_loop_boundaries(hip_lib, D, heads, kv_heads, name, pos0, M, T_max):
    """Rows at and around one key-loop iteration (16 KPW keys) and the softmax stride (1024), a chunk over each boundary (its
    own keys quantised in registers, the others read from the cache), 5 rows ending at T_max."""
    _one_sequence(f"D{D} {heads}/{kv_heads} {name}", D, heads, kv_heads, pos0, M, T_max)


@pytest.mark.gpu
@pytest.mark.parametrize("D,heads,kv_heads", CONFIGS)
def test_slots_at_the_loop_boundaries_and_a_finished_slot(hip_lib, D, heads, kv_heads):
    """Slot lengths (0, G-1 finished, G, 1030) with three sentinel rows between the slots' caches and exponent arrays: every
    live slot against its own dequantised cache and bit-identical to the one-sequence kernel on that slot alone; the finished
    slot's codes, exponents and output row untouched; the state block unchanged."""
    from diffsensei_amd import ops
    from diffsensei_amd._lib import check
    tag = f"D{D} {heads}/{kv_heads} slots"
    lens, fin = A.slot_lengths(D), [0, 1, 0, 0]
    S, T_max, PAD, W, scale = 4, 1100, 3, kv_heads * D, 1.0 / math.sqrt(D)
    cos, sin = _rope(D, T_max)
    hist, cs = [], []
    for n in lens:
        h = A.planted_qkv(D, heads, kv_heads, n + 1, n, A.case_seed(D, heads, kv_heads, n, 1))
        _, k, v = A.split_qkv(h, D, heads, kv_heads)
        hist.append(h)
        cs.append(_cache(K8.rotated_keys_ref(k), v, n, T_max, PAD))
    kc, vc, ke, ve = [torch.stack([c[i] for c in cs]).contiguous() for i in range(4)]
    before = [t.clone() for t in (kc, vc, ke, ve)]
    state = torch.tensor([[lens[s], 1, fin[s], 0, 9, 2, 0, 0] for s in range(S)], dtype=torch.int32, device=DEV)
    state0 = state.clone()
    qkv = torch.stack([h[-1] for h in hist]).to(DEV)
    out = torch.full((S, heads * D), 7.0, dtype=torch.float16, device=DEV)
    check(hip_lib.ds_llm_attn_slots_kv8(qkv.data_ptr(), qkv.shape[1], kc.data_ptr(), vc.data_ptr(), W, kc.stride(0), ke.data_ptr(),
                                        ve.data_ptr(), kv_heads, ke.stride(0), cos.data_ptr(), sin.data_ptr(), out.data_ptr(),
                                        heads * D, state.data_ptr(), S, heads, kv_heads, D, T_max, scale,
                                        torch.cuda.current_stream().cuda_stream), "ds_llm_attn_slots_kv8")
    assert torch.equal(state, state0), "attention must not move the counters"
    for s in range(S):
        n, T = lens[s], lens[s] + 1
        if fin[s]:
            for t, b in zip((kc, vc, ke, ve), before):
                assert torch.equal(t[s], b[s]), "a finished slot's codes / exponents were written"
            assert bool((out[s] == 7.0).all()), "a finished slot's output row was written"
            continue
        q, k, v = A.split_qkv(hist[s], D, heads, kv_heads)
        kr = K8.rotated_keys_ref(k)
        got = [t[s].cpu() for t in (kc, vc, ke, ve)]
        _check_kv(f"{tag} at length {n}", got[0][n:T], got[2][n:T], got[1][n:T], got[3][n:T], kr[n:T], v[n:T])
        kd, vd = _deq(got[0][:T], got[2][:T], got[1][:T], got[3][:T], kv_heads, D)
        _g(f"{tag}: output at length {n}", A.rel_err(out[s:s + 1], K8.attention_over_cache_ref(q[n:T], kd, vd, n)))
        for t, b in zip((kc, vc, ke, ve), before):
            assert torch.equal(t[s, :n], b[s, :n]) and torch.equal(t[s, T:], b[s, T:]), "rows other than the new one were written"
        one = [b[s, :T_max].clone() for b in before]
        o1 = ops.llm_attention_kv8(qkv[s:s + 1].contiguous(), one[0], one[1], one[2], one[3], cos, sin, _state(n), heads, kv_heads, scale)
        assert torch.equal(out[s], o1[0]), f"slot {s} differs from the one-sequence kernel"
        for t, o in zip((kc, vc, ke, ve), one):
            assert torch.equal(t[s, :T_max], o), f"slot {s}: caches differ from the one-sequence kernel's"


# ------------------------------------------------------------------------------------------------ 4. chunking
OTHER_ROWS = (7,) * 43 + (2,)


@pytest.mark.gpu
@pytest.mark.parametrize("D,heads,kv_heads", [c for c in CONFIGS if c[0] == 128])
def test_result_does_not_depend_on_how_the_rows_are_cut_into_chunks(hip_lib, D, heads, kv_heads):
    """303 rows (300 prompt rows and 3 tokens) into an empty cache as 18 x 16 + 12 + 1 + 1 + 1 and as 43 x 7 + 2: equal cache
    bytes, bit-identical outputs, every launch within the output gate of its own max|ref|, the K codes within case 2's cap
    over all rows."""
    from diffsensei_amd import ops
    tag = f"D{D} {heads}/{kv_heads} kernel-filled"
    T, T_max = sum(A.FILL_ROWS), 320
    assert sum(OTHER_ROWS) == T
    qkv = A.planted_qkv(D, heads, kv_heads, T, 300, A.case_seed(D, heads, kv_heads, 0, T))
    q, k, v = A.split_qkv(qkv, D, heads, kv_heads)
    kr = K8.rotated_keys_ref(k)
    cos, sin = _rope(D, T_max)
    qd = qkv.to(DEV)
    runs = []
    for chunks in (A.FILL_ROWS, OTHER_ROWS):
        kc, vc, ke, ve = _cache(kr, v, 0, T_max)
        state, outs, r0 = _state(0), [], 0
        for m in chunks:
            outs.append(ops.llm_attention_kv8(qd[r0:r0 + m].contiguous(), kc, vc, ke, ve, cos, sin, state, heads, kv_heads,
                                              1.0 / math.sqrt(D)))
            ops.llm_advance(state, m)
            r0 += m
        assert int(state[0]) == T
        runs.append((torch.cat(outs).cpu(), [t.cpu() for t in (kc, vc, ke, ve)]))
    (out_a, ca), (out_b, cb) = runs
    for a, b in zip(ca, cb):
        assert torch.equal(a, b), "the cache bytes depend on the chunking"
    assert not ca[0][T:].any() and not ca[2][T:].any(), "rows past the cache length were written"
    _check_kv(tag, ca[0][:T], ca[2][:T], ca[1][:T], ca[3][:T], kr, v)
    kd, vd = _deq(ca[0][:T], ca[2][:T], ca[1][:T], ca[3][:T], kv_heads, D)
    ref = K8.attention_over_cache_ref(q, kd, vd, 0)
    err, r0 = 0.0, 0
    for m in A.FILL_ROWS:
        err = max(err, A.rel_err(out_a[r0:r0 + m], ref[r0:r0 + m]))
        r0 += m
    _g(f"{tag}: output, worst launch", err)
    _g(f"{tag}: the other chunking against the first", A.rel_err(out_b, out_a.float()))
    assert torch.equal(out_a, out_b), "the outputs depend on the chunking"


# ------------------------------------------------------------------------------------------------ 5. guards
@pytest.mark.gpu
@pytest.mark.parametrize("D,heads,kv_heads", CONFIGS)
def test_rows_past_the_cache_write_neither_codes_nor_exponents(hip_lib, D, heads, kv_heads):
    """pos0 = 32, 16 rows, T_max = 40: rows 0..7 are computed and appended, rows 8..15 write nothing - the sentinel rows behind
    the codes and behind the exponent bytes are intact, their output rows too."""
    pos0, M, T_max = A.GUARD
    _one_sequence(f"D{D} {heads}/{kv_heads} guard", D, heads, kv_heads, pos0, T_max - pos0, T_max, pad=24, M_launch=M)


@pytest.mark.gpu
def test_launch_checks(hip_lib):
    """Exponent pointers present, ldc % 8 == 0, the exponent arrays' slot stride: refused at the launch, nothing runs."""
    D, heads, kv = 64, 4, 2
    T_max, W = 16, kv * D
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device=DEV)
    qkv, out = z(2, (heads + 2 * kv) * D, dt=torch.float16), z(2, heads * D, dt=torch.float16)
    kc, vc, ke, ve, cos = z(2, T_max, W), z(2, T_max, W), z(2, T_max, kv), z(2, T_max, kv), z(T_max, D // 2, dt=torch.float32)
    st = torch.tensor([[0, 0, 0, 0, 0, 0, 0, 0]] * 2, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    one = lambda ke_ptr, ldc, lde: hip_lib.ds_llm_attn_kv8(qkv.data_ptr(), qkv.shape[1], kc.data_ptr(), vc.data_ptr(), ldc, ke_ptr,
                                                           ve.data_ptr(), lde, cos.data_ptr(), cos.data_ptr(), out.data_ptr(),
                                                           heads * D, st.data_ptr(), 1, heads, kv, D, T_max, 0.125, s)
    assert one(ke.data_ptr(), W, kv) == 0
    assert one(None, W, kv) != 0 and b"exponent" in hip_lib.ds_last_error()
    assert one(ke.data_ptr(), W + 4, kv) != 0
    assert one(ke.data_ptr(), W, kv - 1) != 0
    slots = lambda es: hip_lib.ds_llm_attn_slots_kv8(qkv.data_ptr(), qkv.shape[1], kc.data_ptr(), vc.data_ptr(), W, T_max * W,
                                                     ke.data_ptr(), ve.data_ptr(), kv, es, cos.data_ptr(), cos.data_ptr(),
                                                     out.data_ptr(), heads * D, st.data_ptr(), 2, heads, kv, D, T_max, 0.125, s)
    assert slots(T_max * kv) == 0
    assert slots(T_max * kv - 1) != 0 and b"exponent slot stride" in hip_lib.ds_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. poisoned memory
def _untouched(m, *tails):
    """cache rows past the sequence belong to the placed operand: they must still hold what `m.poison` put there"""
    torch.cuda.synchronize()
    want = 0 if m.plain else m.pattern(torch.uint8)
    for t in tails:
        assert bool((t == want).all()), "rows past the cache length were written"


@functools.lru_cache(maxsize=None)
def _p_data(D, heads, kv, lens, M, T_max=40):
    """per sequence: fused rows [n + M], rotated fp16 keys, values"""
    g = torch.Generator().manual_seed(D * 5 + heads + M)
    seqs = []
    for n in lens:
        qkv = (torch.randn(n + M, (heads + 2 * kv) * D, generator=g)).half()
        q, k, v = A.split_qkv(qkv, D, heads, kv)
        seqs.append(NS(qkv=qkv, q=q, kr=K8.rotated_keys_ref(k), v=v, n=n))
    from oracle import llama_ref as R
    cos, sin = R.rope_tables(D, T_max)
    return NS(seqs=seqs, cos=cos.contiguous(), sin=sin.contiguous(), dims=(D, heads, kv, M, T_max))


def _p_caches(m, h, S):
    from diffsensei_amd.mllm import quantize_kv_fp8
    D, heads, kv, M, T_max = h.dims
    kc, vc = m.poison((S, T_max, kv * D), torch.uint8), m.poison((S, T_max, kv * D), torch.uint8)
    ke, ve = m.poison((S, T_max, kv), torch.uint8), m.poison((S, T_max, kv), torch.uint8)
    for s, q in enumerate(h.seqs):
        if q.n:
            (c, e), (c2, e2) = quantize_kv_fp8(q.kr[:q.n]), quantize_kv_fp8(q.v[:q.n])
            kc[s, :q.n], ke[s, :q.n], vc[s, :q.n], ve[s, :q.n] = c.view(q.n, -1), e, c2.view(q.n, -1), e2
    return kc, vc, ke, ve


def _p_run_one(m, h):
    D, heads, kv, M, T_max = h.dims
    q = h.seqs[0]
    kc, vc, ke, ve = [m.place(t[0]) for t in _p_caches(m, h, 1)]
    state = m.place(torch.tensor([q.n, 0, 0, 0, 9, 2, 0, 0], dtype=torch.int32))
    out = m.ops.llm_attention_kv8(m.place(q.qkv[q.n:]), kc, vc, ke, ve, m.place(h.cos), m.place(h.sin), state, heads, kv,
                                  1.0 / math.sqrt(D))
    T = q.n + M
    _untouched(m, kc[T:], vc[T:], ke[T:], ve[T:])
    return (out, kc[:T], vc[:T], ke[:T], ve[:T], state)


def _p_check_seq(what, h, q, out, kc, vc, ke, ve, M):
    D, heads, kv = h.dims[:3]
    T = q.n + M
    _check_kv(what, kc[q.n:T], ke[q.n:T], vc[q.n:T], ve[q.n:T], q.kr[q.n:T], q.v[q.n:T])
    kd, vd = _deq(kc[:T], ke[:T], vc[:T], ve[:T], kv, D)
    P._close_rel(out, K8.attention_over_cache_ref(q.q[q.n:T], kd, vd, q.n), 4e-3, what)


def _p_check_one(o, h):
    q, M = h.seqs[0], h.dims[3]
    _p_check_seq("kv8 attention rows", h, q, o[0], o[1], o[2], o[3], o[4], M)
    assert o[5].tolist() == [q.n, 0, 0, 0, 9, 2, 0, 0]


P_LENS, P_FIN = (0, 7, 23), (0, 1, 0)


def _p_run_slots(m, h):
    D, heads, kv, M, T_max = h.dims
    S = len(P_LENS)
    kc, vc, ke, ve = [m.place(t) for t in _p_caches(m, h, S)]
    state = m.place(torch.tensor([[P_LENS[s], 1, P_FIN[s], 0, 9, 2, 0, 0] for s in range(S)], dtype=torch.int32))
    out = m.place(torch.full((S, heads * D), 7.0, dtype=torch.float16))       # a finished slot's row is left alone
    m.ops.llm_attention_slots_kv8(m.place(torch.stack([q.qkv[-1] for q in h.seqs])), kc, vc, ke, ve, m.place(h.cos), m.place(h.sin),
                                  state, heads, kv, 1.0 / math.sqrt(D), out=out)
    rows = [n + (0 if P_FIN[s] else 1) for s, n in enumerate(P_LENS)]
    _untouched(m, *[c[s, r:] for c in (kc, vc, ke, ve) for s, r in enumerate(rows)])
    return (out, state) + tuple(c[s, :r] for c in (kc, vc, ke, ve) for s, r in enumerate(rows))


def _p_check_slots(o, h):
    S = len(P_LENS)
    out, state = o[0], o[1]
    kcs, vcs, kes, ves = o[2:2 + S], o[2 + S:2 + 2 * S], o[2 + 2 * S:2 + 3 * S], o[2 + 3 * S:]
    for s, q in enumerate(h.seqs):
        if P_FIN[s]:
            assert bool((out[s] == 7.0).all()) and kcs[s].shape[0] == q.n, "a finished slot's output row was written"
            continue
        _p_check_seq(f"kv8 attention slot {s}", h, q, out[s:s + 1], kcs[s], vcs[s], kes[s], ves[s], 1)
    assert state.tolist() == [[P_LENS[s], 1, P_FIN[s], 0, 9, 2, 0, 0] for s in range(S)]


KV8_CASES = [P.Case("llm-attn-kv8-D128-h3-kv3-pos19-M5", ["ds_llm_attn_kv8"], functools.partial(_p_data, 128, 3, 3, (19,), 5),
                    _p_run_one, _p_check_one),
             P.Case("llm-attn-slots-kv8-D64-h4-kv2", ["ds_llm_attn_slots_kv8"], functools.partial(_p_data, 64, 4, 2, P_LENS, 1),
                    _p_run_slots, _p_check_slots)]
P.CASES.extend(KV8_CASES)     # on import, which pytest does for every test module before it runs a test (as test_gpu_llm_fp4_poisoned.py)


def test_the_kv8_entry_points_have_their_cases():
    """Host only: what tests/test_gpu_poisoned_memory.py::test_every_entry_point_has_a_case needs from this file."""
    from diffsensei_amd._lib import SIGNATURES
    ours = {e for c in KV8_CASES for e in c.entry}
    assert ours == {"ds_llm_attn_kv8", "ds_llm_attn_slots_kv8"} and ours <= set(SIGNATURES)
    assert all(any(c is k for k in P.CASES) for c in KV8_CASES) and len({c.id for c in P.CASES}) == len(P.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", KV8_CASES, ids=lambda c: c.id)
def test_kv8_result_depends_on_nothing_but_the_operands(hip_lib, case):
    P.test_result_depends_on_nothing_but_the_operands(hip_lib, case)
