"""CPU: host side of int8 weight-only decoding (W8A16) in diffsensei_amd/mllm.py - the per-row quantiser and what the
engine holds, lists and prices with `weight_dtype="int8"`.  No kernel runs here; the numerics are covered on the GPU by
tests/test_gpu_llm_w8.py and tests/test_gpu_mllm_w8.py."""
import pytest
import torch

from diffsensei_amd import _lib
from diffsensei_amd import mllm as M

CFG = dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1)


def _sd(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(s, generator=g) * 0.05 for k, s in M.llama_param_shapes(cfg).items()}


def _engine(weight_dtype=None, **over):
    cfg = M.LlamaConfig(**dict(CFG, **over))
    kw = {} if weight_dtype is None else {"weight_dtype": weight_dtype}
    return cfg, M.LlamaDecodeEngine(cfg, _sd(cfg), "cpu", max_positions=32, max_new_tokens=8, **kw)


def test_quantiser_properties():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(37, 80, generator=g) * torch.logspace(-3, 1, 37)[:, None]
    w[5] = 0.0                                                          # an all-zero row
    w[9, 3] = 7.0                                                       # a row with one outlier
    q, s = M.quantize_rows_int8(w)
    assert q.dtype == torch.int8 and q.shape == w.shape and q.is_contiguous()
    assert s.dtype == torch.float32 and s.shape == (37,) and bool((s > 0).all())
    assert int(q.to(torch.int32).abs().max()) <= 127
    w16 = w.half().float()                                              # the quantiser starts from the fp16 weights
    deq = M.dequantize_rows_int8(q, s)
    assert deq.dtype == torch.float32
    assert bool(((w16 - deq).abs() <= 0.5 * s[:, None] * (1 + 1e-6)).all())
    top = w16.abs().argmax(dim=1)
    rows = [n for n in range(37) if n != 5]
    assert q[rows, top[rows]].to(torch.int32).abs().tolist() == [127] * 36, "each row's largest |w| maps to +-127"
    assert torch.equal(torch.sign(q[rows, top[rows]].float()), torch.sign(w16[rows, top[rows]]))
    assert float(s[5]) == 1.0 and not q[5].any()
    assert torch.equal(s[rows], w16[rows].abs().amax(1) / 127.0)


def test_quantiser_rounds_half_to_even_and_commutes_with_stacking():
    # s = 1 exactly (row maximum 127): 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0, -1.5 -> -2
    w = torch.tensor([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5]])
    q, s = M.quantize_rows_int8(w)
    assert float(s[0]) == 1.0 and q[0].tolist() == [127, 0, 2, 2, 0, -2, -2, 4]
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(24, 48, generator=g), torch.randn(40, 48, generator=g) * 3
    qa, sa = M.quantize_rows_int8(a)
    qb, sb = M.quantize_rows_int8(b)
    qc, sc = M.quantize_rows_int8(torch.cat([a, b]))
    assert torch.equal(qc, torch.cat([qa, qb])) and torch.equal(sc, torch.cat([sa, sb]))
    with pytest.raises(ValueError):
        M.quantize_rows_int8(torch.zeros(8))


def test_int8_engine_tensors_and_bytes():
    cfg, eng = _engine("int8")
    L, H, I, V = cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    assert eng.weight_dtype == "int8"
    for ws, ss, rows, K in ((eng.wqkv, eng.sqkv, 3 * H, H), (eng.wo, eng.so, H, H), (eng.wgu, eng.sgu, 2 * I, H),
                            (eng.wdown, eng.sdown, H, I)):
        assert len(ws) == len(ss) == L
        for w, s in zip(ws, ss):
            assert w.dtype == torch.int8 and w.shape == (rows, K) and s.dtype == torch.float32 and s.shape == (rows,)
    assert eng.embed.dtype == eng.lm_head.dtype == eng.norm_g.dtype == torch.float16
    assert all(g.dtype == torch.float16 for g in eng.g_in + eng.g_post)
    ts = eng.tensors()
    assert len(ts) == 3 + 10 * L
    by = lambda dt: sum(1 for t in ts if t.dtype == dt)
    assert (by(torch.int8), by(torch.float32), by(torch.float16)) == (4 * L, 4 * L, 3 + 2 * L)
    assert all(any(t is w for t in ts) for w in eng.wqkv + eng.wo + eng.wgu + eng.wdown + eng.sqkv + eng.so + eng.sgu + eng.sdown)
    n_q = L * (3 * H * H + H * H + 2 * I * H + H * I)
    n_s = L * (3 * H + H + 2 * I + H)
    assert eng.weight_bytes_per_token() == n_q + 4 * n_s + 2 * (V * H + H)
    # the engine quantises what the fp16 engine holds, group by group
    _, ref = _engine()
    q, s = M.quantize_rows_int8(ref.wgu[1])
    assert torch.equal(eng.wgu[1], q) and torch.equal(eng.sgu[1], s)


def test_int8_engine_op_lists_use_the_w8_ops_except_for_lm_head():
    cfg, eng = _engine("int8")
    L = cfg.num_hidden_layers
    code = lambda ops_: [int(o.code) for o in ops_]
    tok = eng._token_ops(1)
    assert code(tok).count(_lib.OP["LLM_GEMV_W8"]) == 4 * L
    assert code(tok).count(_lib.OP["LLM_GEMV"]) == 1, "lm_head stays fp16"
    w8 = [o for o in tok if int(o.code) == _lib.OP["LLM_GEMV_W8"]]
    assert w8[0].p[1] == eng.wqkv[0].data_ptr() and w8[0].p[5] == eng.sqkv[0].data_ptr()
    assert w8[2].p[1] == eng.wgu[0].data_ptr() and w8[2].p[5] == eng.sgu[0].data_ptr() and w8[2].p[4] == eng.g_post[0].data_ptr()
    assert w8[3].p[1] == eng.wdown[0].data_ptr() and w8[3].p[5] == eng.sdown[0].data_ptr() and not w8[3].p[4]
    chunk = eng._chunk_ops(16, "chunk")
    assert code(chunk).count(_lib.OP["LLM_GEMV_W8"]) == 4 * L and _lib.OP["LLM_GEMV"] not in code(chunk)
    _, eng4 = _engine("int8", num_hidden_layers=1)
    eng4 = M.LlamaDecodeEngine(eng4.cfg, _sd(eng4.cfg), "cpu", max_positions=32, max_new_tokens=8, max_sequences=4,
                               weight_dtype="int8")
    batch = eng4._token_ops(4)
    assert code(batch).count(_lib.OP["LLM_GEMM16_W8"]) == 4 and code(batch).count(_lib.OP["LLM_GEMM16"]) == 1


def test_int8_engine_argument_checks():
    with pytest.raises(ValueError):
        _engine("int4")
    with pytest.raises(ValueError):                                     # hidden 136: a multiple of 8, not of 16
        _engine("int8", hidden_size=136, num_attention_heads=1, intermediate_size=256)
    with pytest.raises(ValueError):                                     # the same for the intermediate size (K of down)
        _engine("int8", intermediate_size=264)
    cfg = M.LlamaConfig(**dict(CFG, intermediate_size=264))
    M.LlamaDecodeEngine(cfg, _sd(cfg), "cpu", max_positions=32, max_new_tokens=8)   # fine with fp16 weights


def test_checksum_sees_a_changed_int8_element():
    from diffsensei_amd.distributed import tensors_checksum
    _, eng = _engine("int8")
    before = tensors_checksum(eng.tensors())
    assert torch.equal(tensors_checksum(eng.tensors()), before)
    eng.wo[1][17, 5] += 1
    after = tensors_checksum(eng.tensors())
    assert int(after[0]) != int(before[0]) and int(after[1]) == int(before[1])


def test_fp16_engine_is_unchanged():
    cfg, eng = _engine()
    assert eng.weight_dtype == "float16"
    assert len(eng.tensors()) == 3 + 6 * cfg.num_hidden_layers and all(t.dtype == torch.float16 for t in eng.tensors())
    codes = [int(o.code) for o in eng._token_ops(1)]
    assert _lib.OP["LLM_GEMV_W8"] not in codes and _lib.OP["LLM_GEMM16_W8"] not in codes
    assert codes.count(_lib.OP["LLM_GEMV"]) == 4 * cfg.num_hidden_layers + 1
    first = eng._token_ops(1)[1]
    assert first.p[1] == eng.wqkv[0].data_ptr() and first.p[4] == eng.g_in[0].data_ptr() and not first.p[5]
    _, explicit = _engine("float16")
    assert torch.equal(explicit.wqkv[0], eng.wqkv[0])
