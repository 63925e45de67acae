"""GPU: `llm_attn_rows_kernel` (csrc/llm.hip) through `ops.llm_attention_rows` / DS_OP_LLM_ATTN_ROWS[_KV8]: ragged attention
over the rows of several slots in one launch, against the existing kernel fed the same rows per slot in chunks of <= 16
(`ops.llm_attention` / `ops.llm_attention_kv8` with the cursor set to the slot's start length).

Both run `llm_attn_body` on the same row with the same keys, so everything is compared bit for bit - no tolerance anywhere in
this file: outputs, cache bytes and exponent bytes.  All buffers are poisoned first: the unused slot, every cache row at or
past a slot's new length, the rows of `out` outside the table and the state block must come back byte for byte.

4 slots of T_max 64, three in use: segments of 1, 17 and 5 rows at cache lengths 0, 13 and 40 (the 17-row one is longer than
a launch of the existing kernel may be and crosses the key-group seams of tests/_llm_attn_ref.py: 4 keys per wavefront at
D = 128, 8 at D = 64); heads / kv heads 4 / 2."""
import math

import pytest
import torch

from tests._llm_attn_ref import kpw

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEADS, KV_HEADS, T_MAX, SLOTS = 4, 2, 64, 4
SEGMENTS = [(2, 0, 1), (0, 13, 17), (3, 40, 5)]             # (slot, cache length at the start, rows); slot 1 is unused
POISON = 0xA5


def _poisoned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(POISON)
    return t


def _rope(D):
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    fr = torch.outer(torch.arange(T_MAX, dtype=torch.float32), inv_freq)
    return fr.cos().to(DEV).contiguous(), fr.sin().to(DEV).contiguous()


class Caches:
    """k / v caches [SLOTS, T_MAX, kv_heads * D] (fp16, or e4m3 codes with exponent planes [SLOTS, T_MAX, kv_heads]), poisoned"""

    def __init__(self, D, kv8):
        self.kv8 = kv8
        dt = torch.uint8 if kv8 else torch.float16
        self.k, self.v = _poisoned((SLOTS, T_MAX, KV_HEADS * D), dt), _poisoned((SLOTS, T_MAX, KV_HEADS * D), dt)
        self.ke = _poisoned((SLOTS, T_MAX, KV_HEADS), torch.uint8) if kv8 else None
        self.ve = _poisoned((SLOTS, T_MAX, KV_HEADS), torch.uint8) if kv8 else None

    def planes(self):
        return [t for t in (self.k, self.v, self.ke, self.ve) if t is not None]

    def clone(self):
        c = Caches.__new__(Caches)
        c.kv8 = self.kv8
        c.k, c.v = self.k.clone(), self.v.clone()
        c.ke, c.ve = (self.ke.clone(), self.ve.clone()) if self.kv8 else (None, None)
        return c


def _chunks(ops, qkv, c, slot, start, cos, sin, out):
    """the existing kernel: the rows of qkv appended to slot `slot` from length `start` on, in chunks of at most 16"""
    D = qkv.shape[1] // (HEADS + 2 * KV_HEADS)
    pf = torch.zeros(8, dtype=torch.int32, device=DEV)
    pf[0] = start
    for r0 in range(0, qkv.shape[0], 16):
        m = min(16, qkv.shape[0] - r0)
        if c.kv8:
            ops.llm_attention_kv8(qkv[r0:r0 + m], c.k[slot], c.v[slot], c.ke[slot], c.ve[slot], cos, sin, pf, HEADS, KV_HEADS,
                                  1.0 / math.sqrt(D), out=out[r0:r0 + m])
        else:
            ops.llm_attention(qkv[r0:r0 + m], c.k[slot], c.v[slot], cos, sin, pf, HEADS, KV_HEADS, 1.0 / math.sqrt(D),
                              out=out[r0:r0 + m])
        ops.llm_advance(pf, m)


def _setup(ops, D, kv8, segments, seed):
    """caches filled up to every segment's start length by the existing kernel (the rest poison), the segments' qkv rows, the
    row table, the state block (a paused slot carries flag 2, the unused one 1) and the rope tables"""
    g = torch.Generator().manual_seed(seed)
    width = (HEADS + 2 * KV_HEADS) * D
    cos, sin = _rope(D)
    base = Caches(D, kv8)
    for slot, start, _ in segments:
        if start:
            fill = torch.randn(start, width, generator=g).half().to(DEV)
            _chunks(ops, fill, base, slot, 0, cos, sin, torch.empty(start, HEADS * D, dtype=torch.float16, device=DEV))
    R = sum(m for _, _, m in segments)
    qkv = torch.randn(R, width, generator=g).half().to(DEV)
    table = torch.tensor([[slot, r] for slot, _, m in segments for r in range(m)], dtype=torch.int32, device=DEV)
    state = torch.zeros(SLOTS, 8, dtype=torch.int32)
    state[:, 2] = 1
    for slot, start, _ in segments:
        state[slot, 0], state[slot, 2], state[slot, 3] = start, 2, 7
    return base, qkv, table, state.to(DEV), cos, sin


def _run_rows(ops, D, c, qkv, table, state, cos, sin):
    """one launch; `out` sits between two guard rows"""
    R = qkv.shape[0]
    full = _poisoned((R + 2, HEADS * D), torch.float16)
    ops.llm_attention_rows(qkv, c.k, c.v, cos, sin, state, table, HEADS, KV_HEADS, 1.0 / math.sqrt(D), out=full[1:R + 1],
                           k_exp=c.ke, v_exp=c.ve)
    torch.cuda.synchronize()
    return full


def _is_poison(t):
    return bool((t.contiguous().view(torch.uint8) == POISON).all())


@pytest.mark.parametrize("kv8", [False, True], ids=["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_rows_launch_equals_the_existing_kernel_in_chunks(hip_lib, D, kv8):
    from diffsensei_amd import ops
    assert 13 // kpw(D) != (13 + 16) // kpw(D)              # the long segment crosses key-group seams
    base, qkv, table, state, cos, sin = _setup(ops, D, kv8, SEGMENTS, seed=D + kv8)
    got_c, ref_c = base.clone(), base.clone()
    state0 = state.clone()
    full = _run_rows(ops, D, got_c, qkv, table, state, cos, sin)
    R = qkv.shape[0]
    ref = _poisoned((R, HEADS * D), torch.float16)
    a = 0
    for slot, start, m in SEGMENTS:
        _chunks(ops, qkv[a:a + m], ref_c, slot, start, cos, sin, ref[a:a + m])
        a += m
    torch.cuda.synchronize()
    assert not _is_poison(ref) and torch.isfinite(ref.float()).all()
    assert torch.equal(full[1:R + 1], ref), "outputs differ from the existing kernel's"
    assert _is_poison(full[0]) and _is_poison(full[R + 1]), "a row of `out` outside the table was written"
    assert torch.equal(state, state0), "the state block was written"
    for got, want, orig in zip(got_c.planes(), ref_c.planes(), base.planes()):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), "cache / exponent bytes differ"
        assert torch.equal(got[1], orig[1]) and _is_poison(got[1]), "the unused slot was written"
        for slot, start, m in SEGMENTS:
            assert torch.equal(got[slot, :start], orig[slot, :start]), "rows below the start length were rewritten"
            assert not _is_poison(got[slot, start:start + m])
            assert _is_poison(got[slot, start + m:]), "a cache row at or past the new length was written"


@pytest.mark.parametrize("kv8", [False, True], ids=["fp16", "fp8"])
def test_segment_order_and_cut_do_not_matter(hip_lib, kv8):
    """the same rows with the segments in another order, and the 17-row segment alone in a launch of its own: same bits"""
    from diffsensei_amd import ops
    D = 128
    base, qkv, table, state, cos, sin = _setup(ops, D, kv8, SEGMENTS, seed=5)
    c1 = base.clone()
    full = _run_rows(ops, D, c1, qkv, table, state, cos, sin)
    order = [1, 2, 0]
    offs = [0, 1, 18]
    rows = torch.cat([torch.arange(offs[i], offs[i] + SEGMENTS[i][2]) for i in order]).to(DEV)
    c2 = base.clone()
    full2 = _run_rows(ops, D, c2, qkv[rows].contiguous(), table[rows].contiguous(), state, cos, sin)
    assert torch.equal(full2[1:-1], full[1:-1][rows])
    for x, y in zip(c1.planes(), c2.planes()):
        assert torch.equal(x, y)
    c3 = base.clone()
    alone = _run_rows(ops, D, c3, qkv[1:18].contiguous(), table[1:18].contiguous(), state, cos, sin)
    assert torch.equal(alone[1:-1], full[2:19])
    for x, y in zip(c1.planes(), c3.planes()):
        assert torch.equal(x[0], y[0])


@pytest.mark.parametrize("kv8", [False, True], ids=["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_a_segment_that_would_pass_t_max_writes_nothing_there(hip_lib, D, kv8):
    """8 rows from length 60 in slot 0 of a 64-row cache: rows 0..3 are rows 60..63, rows 4..7 have no place - their blocks
    write no output, no cache row (slot 1, which follows slot 0 in memory, stays poison) and no exponent."""
    from diffsensei_amd import ops
    segments = [(0, T_MAX - 4, 8), (2, 3, 2)]
    base, qkv, table, state, cos, sin = _setup(ops, D, kv8, segments, seed=11)
    got_c, ref_c = base.clone(), base.clone()
    full = _run_rows(ops, D, got_c, qkv, table, state, cos, sin)
    ref = _poisoned((10, HEADS * D), torch.float16)
    _chunks(ops, qkv[0:4], ref_c, 0, T_MAX - 4, cos, sin, ref[0:4])
    _chunks(ops, qkv[8:10], ref_c, 2, 3, cos, sin, ref[8:10])
    torch.cuda.synchronize()
    assert torch.equal(full[1:11], ref) and _is_poison(full[5:9]) and _is_poison(full[0]) and _is_poison(full[11])
    for got, want in zip(got_c.planes(), ref_c.planes()):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
        assert _is_poison(got[1]) and _is_poison(got[3]) and _is_poison(got[2, 5:])


def test_argument_checks(hip_lib):
    from diffsensei_amd import _lib, ops
    D = 64
    base, qkv, table, state, cos, sin = _setup(ops, D, False, [(2, 0, 1)], seed=1)
    with pytest.raises(ValueError):
        ops.llm_attention_rows(qkv, base.k, base.v, cos, sin, state, table[:, :1].contiguous(), HEADS, KV_HEADS, 0.125)
    with pytest.raises(_lib.DiffSenseiHipError):            # T_max past what the kernel's score buffer is sized for
        big = torch.zeros(1, 8200, KV_HEADS * D, dtype=torch.float16, device=DEV)
        ops.llm_attention_rows(qkv, big, big.clone(), torch.zeros(8200, D // 2, device=DEV), torch.zeros(8200, D // 2, device=DEV),
                               state[:1].contiguous(), table, HEADS, KV_HEADS, 0.125)
