"""CPU: host side of MXFP4 weight-only decoding (W4A16) in diffsensei_amd/mllm.py - the quantiser (`quantize_rows_mxfp4`:
packed e2m1 elements, one E8M0 exponent per block of 32, one fp32 scale per row), what the engine holds, lists and prices
with `weight_dtype="mxfp4"`, and the LDS bank model's verdict on the order in which `llm_gemv_pipe_kernel` keeps x for the
fp4 form.  No kernel runs here; the numerics are covered on the GPU by tests/test_gpu_llm_fp4.py, test_gpu_llm_fp4_poisoned.py
and test_gpu_mllm_fp4.py."""
import importlib.util
import os

import pytest
import torch

from diffsensei_amd import _lib
from diffsensei_amd import mllm as M

CFG = dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1)
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _sd(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(s, generator=g) * 0.05 for k, s in M.llama_param_shapes(cfg).items()}


def _engine(weight_dtype=None, **over):
    cfg = M.LlamaConfig(**dict(CFG, **over))
    kw = {} if weight_dtype is None else {"weight_dtype": weight_dtype}
    return cfg, M.LlamaDecodeEngine(cfg, _sd(cfg), "cpu", max_positions=32, max_new_tokens=8, **kw)


def _nibbles(q):
    """[N, K] codes: element 2i from the low nibble of byte i, element 2i + 1 from the high one"""
    return torch.stack([q & 15, q >> 4], dim=2).view(q.shape[0], -1)


def test_quantiser_properties():
    g = torch.Generator().manual_seed(1)
    N, K = 37, 160
    w = torch.randn(N, K, generator=g) * torch.logspace(-3, 1, N)[:, None]
    w[:, 32:64] *= 2.0 ** -6                                            # a small block, a tiny one and one the clamp flushes
    w[:, 64:96] *= 2.0 ** -11
    w[:, 96:128] *= 2.0 ** -20
    w[5] = 0.0                                                          # an all-zero row
    w[9, 3] = 7.0                                                       # a row with one outlier
    w[11, 128:160] = 0.0                                                # an all-zero block in a live row
    q, e, s = M.quantize_rows_mxfp4(w)
    assert q.dtype == torch.uint8 and q.shape == (N, K // 2) and q.is_contiguous()
    assert e.dtype == torch.uint8 and e.shape == (N, K // 32) and e.is_contiguous()
    assert s.dtype == torch.float32 and s.shape == (N,) and bool((s > 0).all())
    assert int(e.min()) >= 114 and int(e.max()) <= 127
    assert int(e[11, 4]) == 114, "an all-zero block stores the smallest exponent"
    w16 = w.half().float()                                              # the quantiser starts from the fp16 weights
    deq = M.dequantize_rows_mxfp4(q, e, s)
    assert deq.dtype == torch.float32 and deq.shape == (N, K)
    rows = [n for n in range(N) if n != 5]
    assert torch.equal(s[rows], w16[rows].abs().amax(1) / 6.0)
    assert float(s[5]) == 1.0 and not q[5].any()
    # each row's largest |w| maps to +-6 at exponent 0
    top = w16.abs().argmax(dim=1)
    codes = _nibbles(q)
    assert (codes[rows, top[rows]] & 7).tolist() == [7] * (N - 1)
    assert torch.equal((codes[rows, top[rows]] >> 3).bool(), w16[rows, top[rows]] < 0)
    assert e[rows, top[rows] // 32].tolist() == [127] * (N - 1)
    # |w16 - deq| <= half the local e2m1 step * block scale * row scale.  Two things the format itself does are outside "half a
    # step" and are checked on their own below: the OCP exponent rule leaves elements of up to 8 units in a block whose unit
    # can only express 6 - those saturate - and the clamp of the exponent flushes what is below a quarter of 2^-13.
    bs = torch.ldexp(torch.ones(()), e.to(torch.int32) - 127).repeat_interleave(32, dim=1) * s[:, None]     # one unit of the block
    mag = E2M1[(codes & 7).long()]                                      # |element| in block units
    assert torch.equal(deq, torch.where(codes > 7, -mag, mag) * torch.ldexp(torch.ones(()), e.to(torch.int32) - 127)
                       .repeat_interleave(32, dim=1) * s[:, None])
    step = torch.where(mag < 2, 0.5, torch.where(mag < 4, 1.0, 2.0))    # spacing of e2m1 above |code| (the wider neighbour)
    err = (w16 - deq).abs()
    # a block whose own exponent floor(log2 amax) - 2 is below -13 keeps 114: its elements are coarser than "half a step" says
    # only in one way - everything under a quarter unit is flushed to zero, and a quarter unit is half the step at zero anyway
    sat = w16.abs() > 7.0 * bs                                          # beyond 6 + half the last step: saturated, never above 8 units
    assert bool(sat.any()) and bool((mag[sat] == 6).all()) and bool((w16[sat].abs() < 8.0 * bs[sat] * (1 + 1e-6)).all())
    assert bool((err <= 0.5 * step * bs * (1 + 1e-6))[~sat].all())
    flushed = (e == 114).repeat_interleave(32, dim=1) & (deq == 0) & (w16 != 0)
    assert bool(flushed.any()), "the case must reach the clamp"
    assert bool((w16[flushed].abs() <= 0.25 * bs[flushed]).all())
    assert bool((w16[flushed].abs() <= 2.0 ** -15 * 6 * s[:, None].expand(N, K)[flushed] * (1 + 1e-6)).all())


def test_quantiser_known_answers_ties_and_nibble_order():
    # row maximum 6 -> s = 1; block 0 has exponent 0 (its elements are the values themselves), ties go to the even mantissa:
    # 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4, 7 saturates to 6 (block 1, after the fp16 rounding
    # the quantiser would see 7 as the row maximum, so the saturation is shown on a value between 6 and 7 in a second row)
    vals = [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -6.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0,
            4.0, 0.3, 0.7, 1.3, 1.7, 2.4, 2.6, 3.4, 3.6, 5.1]
    want = [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0, -6.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0,
            4.0, 0.5, 0.5, 1.5, 1.5, 2.0, 3.0, 3.0, 4.0, 6.0]
    w = torch.tensor([vals])
    q, e, s = M.quantize_rows_mxfp4(w)
    assert float(s[0]) == 1.0 and e.tolist() == [[127]]
    assert M.dequantize_rows_mxfp4(q, e, s)[0].tolist() == want
    codes = _nibbles(q)[0].tolist()
    assert codes[:8] == [7, 0, 2, 2, 4, 4, 6, 6] and codes[8:16] == [0, 10, 10, 12, 12, 14, 14, 15]
    # the low nibble holds the even element
    assert int(q[0, 0]) == 7 | (0 << 4) and int(q[0, 1]) == 2 | (2 << 4) and int(q[0, 7]) == 14 | (15 << 4)
    # a second block two powers of two down (unit 0.25): 0.625 = 2.5 units -> 2, 0.875 = 3.5 units -> 4, 1.25 = 5 units -> 4
    w2 = torch.tensor([[6.0] + [0.0] * 31 + [1.5, 0.125, 0.375, 0.625, 0.875, 1.25] + [0.0] * 26])
    q2, e2, s2 = M.quantize_rows_mxfp4(w2)
    assert e2.tolist() == [[127, 125]], "block maximum 1.5: floor(log2 1.5) - 2 = -2"
    assert M.dequantize_rows_mxfp4(q2, e2, s2)[0, 32:38].tolist() == [1.5, 0.125, 0.375, 0.5, 1.0, 1.0]
    # saturation: with s = 7 / 6 the element 7 is 6 units (exact or one ulp off) and lands on code 7, exponent 0
    q3, e3, s3 = M.quantize_rows_mxfp4(torch.tensor([[7.0] + [0.0] * 31]))
    assert int(q3[0, 0]) == 7 and int(e3[0, 0]) == 127 and float(s3[0]) == pytest.approx(7.0 / 6.0)


def test_quantiser_commutes_with_stacking_and_refuses_bad_shapes():
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(24, 96, generator=g), torch.randn(40, 96, generator=g) * 3
    qa, ea, sa = M.quantize_rows_mxfp4(a)
    qb, eb, sb = M.quantize_rows_mxfp4(b)
    qc, ec, sc = M.quantize_rows_mxfp4(torch.cat([a, b]))
    assert torch.equal(qc, torch.cat([qa, qb])) and torch.equal(ec, torch.cat([ea, eb])) and torch.equal(sc, torch.cat([sa, sb]))
    with pytest.raises(ValueError):
        M.quantize_rows_mxfp4(torch.zeros(64))                          # 1-D
    with pytest.raises(ValueError):
        M.quantize_rows_mxfp4(torch.zeros(4, 48))                       # K % 32


def test_mxfp4_engine_tensors_and_bytes():
    cfg, eng = _engine("mxfp4")
    L, H, I, V = cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    assert eng.weight_dtype == "mxfp4"
    for ws, es, ss, rows, K in ((eng.wqkv, eng.eqkv, eng.sqkv, 3 * H, H), (eng.wo, eng.eo, eng.so, H, H),
                                (eng.wgu, eng.egu, eng.sgu, 2 * I, H), (eng.wdown, eng.edown, eng.sdown, H, I)):
        assert len(ws) == len(es) == len(ss) == L
        for w, e, s in zip(ws, es, ss):
            assert w.dtype == torch.uint8 and w.shape == (rows, K // 2)
            assert e.dtype == torch.uint8 and e.shape == (rows, K // 32)
            assert s.dtype == torch.float32 and s.shape == (rows,)
    assert eng.embed.dtype == eng.lm_head.dtype == eng.norm_g.dtype == torch.float16
    assert all(g.dtype == torch.float16 for g in eng.g_in + eng.g_post)
    ts = eng.tensors()
    assert len(ts) == 3 + 14 * L
    by = lambda dt: sum(1 for t in ts if t.dtype == dt)
    assert (by(torch.uint8), by(torch.float32), by(torch.float16)) == (8 * L, 4 * L, 3 + 2 * L)
    held = eng.wqkv + eng.wo + eng.wgu + eng.wdown + eng.eqkv + eng.eo + eng.egu + eng.edown + eng.sqkv + eng.so + eng.sgu + eng.sdown
    assert all(any(t is w for t in ts) for w in held)
    n_w = L * (3 * H * H + H * H + 2 * I * H + H * I)
    n_rows = L * (3 * H + H + 2 * I + H)
    assert eng.weight_bytes_per_token() == n_w // 2 + n_w // 32 + 4 * n_rows + 2 * (V * H + H)
    # the engine quantises what the fp16 engine holds, group by group
    _, ref = _engine()
    q, e, s = M.quantize_rows_mxfp4(ref.wgu[1])
    assert torch.equal(eng.wgu[1], q) and torch.equal(eng.egu[1], e) and torch.equal(eng.sgu[1], s)


def test_mxfp4_engine_op_lists_use_the_fp4_ops_except_for_lm_head():
    cfg, eng = _engine("mxfp4")
    L = cfg.num_hidden_layers
    code = lambda ops_: [int(o.code) for o in ops_]
    assert (_lib.OP["LLM_GEMV_FP4"], _lib.OP["LLM_GEMM16_FP4"]) == (38, 39)
    tok = eng._token_ops(1)
    assert code(tok).count(_lib.OP["LLM_GEMV_FP4"]) == 4 * L
    assert code(tok).count(_lib.OP["LLM_GEMV"]) == 1, "lm_head stays fp16"
    assert _lib.OP["LLM_GEMV_W8"] not in code(tok)
    f4 = [o for o in tok if int(o.code) == _lib.OP["LLM_GEMV_FP4"]]
    assert f4[0].p[1] == eng.wqkv[0].data_ptr() and f4[0].p[5] == eng.sqkv[0].data_ptr() and f4[0].p[6] == eng.eqkv[0].data_ptr()
    assert f4[0].p[4] == eng.g_in[0].data_ptr()
    assert f4[1].p[1] == eng.wo[0].data_ptr() and f4[1].p[5] == eng.so[0].data_ptr() and f4[1].p[6] == eng.eo[0].data_ptr()
    assert f4[2].p[1] == eng.wgu[0].data_ptr() and f4[2].p[5] == eng.sgu[0].data_ptr() and f4[2].p[6] == eng.egu[0].data_ptr()
    assert f4[2].p[4] == eng.g_post[0].data_ptr()
    assert f4[3].p[1] == eng.wdown[0].data_ptr() and f4[3].p[5] == eng.sdown[0].data_ptr() and f4[3].p[6] == eng.edown[0].data_ptr()
    assert not f4[3].p[4]
    assert f4[7].p[1] == eng.wdown[1].data_ptr() and f4[7].p[6] == eng.edown[1].data_ptr()
    chunk = eng._chunk_ops(16, "chunk")
    assert code(chunk).count(_lib.OP["LLM_GEMV_FP4"]) == 4 * L and _lib.OP["LLM_GEMV"] not in code(chunk)
    cfg1 = M.LlamaConfig(**dict(CFG, num_hidden_layers=1))
    eng4 = M.LlamaDecodeEngine(cfg1, _sd(cfg1), "cpu", max_positions=32, max_new_tokens=8, max_sequences=4, weight_dtype="mxfp4")
    batch = eng4._token_ops(4)
    assert code(batch).count(_lib.OP["LLM_GEMM16_FP4"]) == 4 and code(batch).count(_lib.OP["LLM_GEMM16"]) == 1
    g16 = [o for o in batch if int(o.code) == _lib.OP["LLM_GEMM16_FP4"]]
    assert g16[2].p[5] == eng4.sgu[0].data_ptr() and g16[2].p[6] == eng4.egu[0].data_ptr() and g16[2].i[0] == 4


def test_mxfp4_engine_argument_checks():
    with pytest.raises(ValueError):
        _engine("int4")
    with pytest.raises(ValueError):                                     # hidden 144: a multiple of 16, not of 32
        _engine("mxfp4", hidden_size=144)
    with pytest.raises(ValueError):                                     # the same for the intermediate size (K of down)
        _engine("mxfp4", intermediate_size=272)
    _engine("int8", intermediate_size=272)                              # a multiple of 16: fine for int8 and fp16
    _engine(None, intermediate_size=272)


def test_checksum_sees_a_changed_nibble_and_a_changed_exponent():
    from diffsensei_amd.distributed import tensors_checksum
    _, eng = _engine("mxfp4")
    before = tensors_checksum(eng.tensors())
    assert torch.equal(tensors_checksum(eng.tensors()), before)
    eng.wo[1][17, 5] ^= 0x10                                            # one bit of one high nibble
    after = tensors_checksum(eng.tensors())
    assert int(after[0]) != int(before[0]) and int(after[1]) == int(before[1])
    eng.wo[1][17, 5] ^= 0x10
    assert torch.equal(tensors_checksum(eng.tensors()), before)
    eng.edown[0][3, 2] -= 1                                             # one block exponent
    after = tensors_checksum(eng.tensors())
    assert int(after[0]) != int(before[0]) and int(after[1]) == int(before[1])


def test_fp16_and_int8_engines_are_unchanged():
    cfg, eng = _engine()
    L = cfg.num_hidden_layers
    assert eng.weight_dtype == "float16"
    assert len(eng.tensors()) == 3 + 6 * L and all(t.dtype == torch.float16 for t in eng.tensors())
    codes = [int(o.code) for o in eng._token_ops(1)]
    assert not {_lib.OP["LLM_GEMV_FP4"], _lib.OP["LLM_GEMM16_FP4"], _lib.OP["LLM_GEMV_W8"]} & set(codes)
    assert codes.count(_lib.OP["LLM_GEMV"]) == 4 * L + 1
    first = eng._token_ops(1)[1]
    assert first.p[1] == eng.wqkv[0].data_ptr() and first.p[4] == eng.g_in[0].data_ptr() and not first.p[5] and not first.p[6]
    assert not (eng.eqkv or eng.eo or eng.egu or eng.edown or eng.sqkv)
    _, e8 = _engine("int8")
    assert len(e8.tensors()) == 3 + 10 * L and not (e8.eqkv or e8.eo or e8.egu or e8.edown)
    t8 = e8._token_ops(1)
    codes8 = [int(o.code) for o in t8]
    assert codes8.count(_lib.OP["LLM_GEMV_W8"]) == 4 * L and _lib.OP["LLM_GEMV_FP4"] not in codes8
    w8 = [o for o in t8 if int(o.code) == _lib.OP["LLM_GEMV_W8"]]
    assert w8[0].p[5] == e8.sqkv[0].data_ptr() and not w8[0].p[6]
    q, s = M.quantize_rows_int8(eng.wo[1])
    assert torch.equal(e8.wo[1], q) and torch.equal(e8.so[1], s)


# ---- the LDS bank model on the order in which llm_gemv_pipe_kernel keeps x for the fp4 form (csrc/llm.hip: WLoad<fp4x2_t>::xpos)
def _bank_model():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "lds_bank_model.py")
    spec = importlib.util.spec_from_file_location("lds_bank_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("K", [5120, 13824, 2048, 736, 256])
def test_fp4_x_layout_in_lds_is_a_permutation_without_bank_conflicts(K):
    B = _bank_model()
    # a permutation of the row's K halves in units of 8: nothing leaves the row, nothing collides
    assert sorted(B.fp4_xpos(k, K) for k in range(0, K, 8)) == list(range(0, K, 8))
    for m in range(4):                                                  # row m of the staged block starts at m * K halves
        for chunk in range(0, K, 2048):                                 # one load of a wavefront: lane l covers chunk + 32 l .. + 32
            for j in range(4):                                          # its four 16-byte x reads
                addr = B.fp4_x_read(K, m, chunk, j)
                groups = B.active_groups(addr)
                assert groups >= 1
                assert B.read_cycles(addr) == groups, f"K={K} row {m} chunk {chunk} read {j}: bank conflict in the permuted layout"
                if K - chunk >= 2048:
                    assert B.read_cycles(B.fp4_x_read(K, m, chunk, j, permuted=False)) == 16, \
                        "the natural layout is the 4-way conflict the permutation removes"
