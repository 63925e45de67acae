"""CPU: host side of the fp8 KV cache in diffsensei_amd/mllm.py - the quantiser (`quantize_kv_fp8`: OCP e4m3 codes, one
power-of-two exponent byte per head), what the engine holds, lists and prices with `kv_dtype="fp8"`, and the preconditions
of the GPU model tests (tests/test_gpu_mllm_kv8.py), asserted here where no GPU time is spent.  No kernel runs here."""
import os

import numpy as np
import pytest
import torch

from diffsensei_amd import _lib
from diffsensei_amd import mllm as M
from tests import _kv8_ref as K8

CFG = dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1)
GOLD = os.path.join(os.path.dirname(__file__), "golden", "mllm_tiny.npz")


def _sd(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(s, generator=g) * 0.05 for k, s in M.llama_param_shapes(cfg).items()}


def _engine(kv_dtype=None, S=1, **over):
    cfg = M.LlamaConfig(**dict(CFG, **over))
    kw = {} if kv_dtype is None else {"kv_dtype": kv_dtype}
    return cfg, M.LlamaDecodeEngine(cfg, _sd(cfg), "cpu", max_positions=32, max_new_tokens=8, max_sequences=S, **kw)


def _heads(D=128):
    """[N, D] fp16: Gaussian heads whose magnitudes are spread over fp16's range, an all-zero head, heads holding fp16's
    largest and smallest values, exact powers of two either side of the exponent rule's 0.875"""
    g = torch.Generator().manual_seed(3)
    N = 64
    x = torch.randn(N, D, generator=g) * torch.logspace(-7, 4, N, base=10.0)[:, None]
    x = x.clamp(-65504.0, 65504.0).half()
    x[5] = 0.0
    x[6] = 0.0
    x[6, 9] = 65504.0                                   # fp16's largest value
    x[7, 3] = -65504.0
    x[8] = 0.0
    x[8, 0] = 2.0 ** -24                                # fp16's smallest subnormal, alone
    x[9, 1] = 2.0 ** -24                                # and beside ordinary values
    x[10] = 0.0
    x[10, 5] = 2.0 ** -14                               # fp16's smallest normal
    x[11] = 0.0
    x[11, :4] = torch.tensor([448.0, 449.0, -0.875, 0.874])
    x[12] = 0.0
    x[12, :3] = torch.tensor([0.875, 0.5, -0.25])       # m = 0.875 exactly: the lower exponent
    x[13] = 0.0
    x[13, :3] = torch.tensor([0.8755, 0.5, -0.25])      # just above
    x[14] = 0.0
    x[14, 7] = -0.0
    return x


def test_quantiser_properties():
    x = _heads()
    codes, exps = M.quantize_kv_fp8(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and codes.is_contiguous()
    assert exps.dtype == torch.uint8 and exps.shape == x.shape[:-1] and exps.is_contiguous()
    assert not bool(((codes & 0x7F) == 0x7F).any()), "0x7F / 0xFF are e4m3fn's NaN"
    ex = exps.to(torch.int32) - 127
    assert int(ex.min()) >= -33 and int(ex.max()) <= 8
    amax = x.double().abs().amax(-1)
    live = amax > 0
    assert (~live).nonzero().view(-1).tolist() == [5, 14]
    assert ex[~live].tolist() == [0, 0] and not codes[5].any(), "an all-zero head stores ex = 0 and zero codes"
    assert int(ex[8]) == -32 and int(ex[6]) == 8 and int(ex[12]) == -9 and int(ex[13]) == -8
    # ex is the smallest integer with amax / 2^ex <= 448
    sc = torch.ldexp(torch.ones_like(amax), ex)
    assert bool((amax[live] / sc[live] <= 448.0).all()) and bool((amax[live] / (sc[live] / 2) > 448.0).all())
    # element error: at most half an e4m3 step at the element's own exponent (step 2^(floor(log2 |y|) - 3), 2^-9 for subnormals)
    deq = M.dequantize_kv_fp8(codes, exps)
    assert deq.dtype == torch.float32 and deq.shape == x.shape
    y = x.double() / sc[:, None]
    e = torch.frexp(y.abs().float()).exponent.to(torch.float64) - 1               # floor(log2 |y|), garbage at 0 (clamped below)
    step = torch.pow(2.0, torch.clamp(e, min=-6.0) - 3.0)
    err = (deq.double() / sc[:, None] - y).abs()
    assert bool((err <= step / 2).all()), float((err / step).max())
    # amax / 2^ex lies in (224, 448], and rounding is monotone: each head's largest code lies in [224, 448]
    top = (deq.double().abs().amax(-1) / sc)[live]
    assert bool((top >= 224.0).all()) and bool((top <= 448.0).all())
    # idempotence, and the sign of zero survives
    # (the map x -> dequantise(quantise(x)) is idempotent bit for bit; the codes repeat too, except for a head whose largest
    # value was rounded down to exactly 224 2^ex = 448 2^(ex-1): the rule then picks ex - 1 and every code moves up a binade)
    # Heads 6 and 7 are left out: 65504 = 255.875 2^8 rounds up to 256 2^8 = 65536, a finite fp32 number that is no fp16 one,
    # so it cannot be fed to the quantiser again - the kernels use it as the fp32 number it is.)
    assert deq[6, 9] == 65536.0 and deq[7, 3] == -65536.0
    rest = torch.tensor([n for n in range(x.shape[0]) if n not in (6, 7)])
    c2, e2 = M.quantize_kv_fp8(deq[rest])
    assert torch.equal(M.dequantize_kv_fp8(c2, e2), deq[rest])
    down = (deq.double().abs().amax(-1) / sc == 224.0)[rest]
    assert bool(down.any()) and bool((~down).any())
    assert torch.equal(c2[~down], codes[rest][~down]) and torch.equal(e2[~down], exps[rest][~down])
    assert torch.equal(e2[down], exps[rest][down] - 1)
    assert int(codes[14, 7]) == 0x80
    # stacking heads equals quantising them stacked; any leading shape
    a, b = M.quantize_kv_fp8(x.view(4, 16, -1))
    assert torch.equal(a.view_as(codes), codes) and torch.equal(b.view_as(exps), exps)
    a, b = M.quantize_kv_fp8(x[17])
    assert torch.equal(a, codes[17]) and int(b) == int(exps[17])
    for k in range(0, 64, 7):
        a, b = M.quantize_kv_fp8(x[k:k + 3])
        assert torch.equal(a, codes[k:k + 3]) and torch.equal(b, exps[k:k + 3])


def test_quantiser_rounds_to_fp16_first_and_to_nearest_even():
    x = torch.zeros(2, 64)
    x[0, :5] = torch.tensor([448.0, 17.0, 19.0, 21.0, 1.0 + 2.0 ** -12])   # 17 / 19 / 21: ties between codes at step 2 (binade 16..32)
    x[1, :4] = torch.tensor([256.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -11])   # ties at the subnormal step 2^-9
    codes, exps = M.quantize_kv_fp8(x)
    assert exps.tolist() == [127, 127]
    deq = M.dequantize_kv_fp8(codes, exps)
    assert deq[0, :5].tolist() == [448.0, 16.0, 20.0, 20.0, 1.0]           # 1 + 2^-12 is 1 in fp16 already
    assert deq[1, :4].tolist() == [256.0, 0.0, 2.0 ** -8, 0.0]


def test_gaussian_error_is_what_the_documents_say():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, 128, generator=g).half()
    d = K8.qdq(x)
    rel = float((d - x.float()).pow(2).mean().sqrt() / x.float().pow(2).mean().sqrt())
    assert 0.02 < rel < 0.032, rel                                         # "2.6 %" in README / DESIGN / the docstrings


def test_fp8_engine_holds_byte_caches_and_prices_them():
    cfg, e16 = _engine(S=3)
    _, e8 = _engine("fp8", S=3)
    L, D, Hkv = cfg.num_hidden_layers, cfg.head_dim, cfg.kv_heads
    assert e16.kv_dtype == "float16" and e8.kv_dtype == "fp8"
    assert not e16.kes and not e16.ves and all(t.dtype == torch.float16 for t in e16.kcs + e16.vcs)
    assert len(e8.kcs) == len(e8.vcs) == len(e8.kes) == len(e8.ves) == L
    for kc, vc, ke, ve in zip(e8.kcs, e8.vcs, e8.kes, e8.ves):
        assert kc.dtype == vc.dtype == ke.dtype == ve.dtype == torch.uint8
        assert kc.shape == vc.shape == (3, 32, Hkv * D) and ke.shape == ve.shape == (3, 32, Hkv)
    assert e16.kv_cache_bytes() == 2 * L * 3 * 32 * Hkv * D * 2
    assert e8.kv_cache_bytes() == 2 * L * 3 * 32 * Hkv * (D + 1)
    assert e8.kv_cache_bytes() * 2 * D == e16.kv_cache_bytes() * (D + 1)
    assert len(e8.tensors()) == len(e16.tensors()), "the cache is no weight"
    assert e8.weight_bytes_per_token() == e16.weight_bytes_per_token()


def test_fp8_engine_op_lists_carry_the_new_opcodes_and_pointers():
    cfg, eng = _engine("fp8", S=4)
    L, D = cfg.num_hidden_layers, cfg.head_dim
    code = lambda ops_: [int(o.code) for o in ops_]
    assert (_lib.OP["LLM_ATTN_KV8"], _lib.OP["LLM_ATTN_SLOTS_KV8"]) == (40, 41)
    for width in (1, 4):
        tok = eng._token_ops(width)
        assert code(tok).count(_lib.OP["LLM_ATTN_SLOTS_KV8"]) == L
        assert not {_lib.OP["LLM_ATTN"], _lib.OP["LLM_ATTN_SLOTS"], _lib.OP["LLM_ATTN_KV8"]} & set(code(tok))
        at = [o for o in tok if int(o.code) == _lib.OP["LLM_ATTN_SLOTS_KV8"]]
        for l, o in enumerate(at):
            assert o.p[1] == eng.kcs[l].data_ptr() and o.p[2] == eng.vcs[l].data_ptr()
            assert o.p[7] == eng.kes[l].data_ptr() and o.p[8] == eng.ves[l].data_ptr()
            assert o.p[0] == eng.qkv.data_ptr() and o.p[5] == eng.att.data_ptr() and o.p[6] == eng.state.data_ptr()
            assert list(o.i[:5]) == [width, 1, 1, D, 32]
            assert list(o.l[:6]) == [3 * D, D, D, 32 * D, 1, 32], "ldqkv ldc ldo slot_stride (bytes) lde exp_slot_stride"
    chunk = eng._chunk_ops(16, "chunk")
    assert code(chunk).count(_lib.OP["LLM_ATTN_KV8"]) == L and _lib.OP["LLM_ATTN_SLOTS_KV8"] not in code(chunk)
    o = [o for o in chunk if int(o.code) == _lib.OP["LLM_ATTN_KV8"]][1]
    assert o.p[1] == eng.kcs[1].data_ptr() and o.p[7] == eng.kes[1].data_ptr() and o.p[8] == eng.ves[1].data_ptr()
    assert list(o.l[:6]) == [3 * D, D, D, 0, 1, 0] and list(o.i[:5]) == [16, 1, 1, D, 32]
    # independent of weight_dtype: the projections keep their own opcodes
    for wd, proj in (("int8", "LLM_GEMV_W8"), ("mxfp4", "LLM_GEMV_FP4")):
        e = M.LlamaDecodeEngine(cfg, _sd(cfg), "cpu", max_positions=32, max_new_tokens=8, weight_dtype=wd, kv_dtype="fp8")
        c = code(e._token_ops(1))
        assert c.count(_lib.OP[proj]) == 4 * L and c.count(_lib.OP["LLM_ATTN_SLOTS_KV8"]) == L


def test_default_engine_is_unchanged_and_other_values_are_refused():
    cfg, eng = _engine()
    _, same = _engine("float16")
    for e in (eng, same):
        c = [int(o.code) for o in e._token_ops(1) + e._chunk_ops(5, "last")]
        assert not {_lib.OP["LLM_ATTN_KV8"], _lib.OP["LLM_ATTN_SLOTS_KV8"]} & set(c)
        assert c.count(_lib.OP["LLM_ATTN_SLOTS"]) == c.count(_lib.OP["LLM_ATTN"]) == cfg.num_hidden_layers
        at = [o for o in e._token_ops(1) if int(o.code) == _lib.OP["LLM_ATTN_SLOTS"]][0]
        assert not at.p[7] and not at.p[8] and list(at.l[3:6]) == [e.kcs[0].stride(0), 0, 0]
    for bad in ("fp16", "e4m3", "int8", None, 8):
        with pytest.raises(ValueError):
            _engine(bad) if bad is not None else M.LlamaDecodeEngine(cfg, _sd(cfg), "cpu", kv_dtype=None)


# ---- preconditions of tests/test_gpu_mllm_kv8.py
def test_the_batch_prompts_leave_no_room_for_a_flipped_id():
    """The fp8-cache oracle runs all 28 ids on the three batch prompts with every top-2 margin >= 5e-2 (minimum margins
    0.213, 0.145 and 0.086), so the GPU test may ask for equal ids."""
    from oracle import make_golden_mllm as G
    from tests.test_gpu_mllm_fp4 import make_prompt
    assert G.MAX_NEW == 28
    for p in K8.BATCH_PROMPTS:
        ref = K8.tiny_oracle(("kv8", p), make_prompt(G, *p), 2)
        m = ref["margins"].tolist()
        print(p, "minimum margin", min(m))
        assert len(ref["output_ids"]) == len(m) == G.MAX_NEW, (p, len(m))
        assert min(m) >= K8.MARGIN, (p, m)


def test_the_two_oracles_are_further_apart_than_twice_the_hidden_state_gate():
    """Golden prompt a: the hidden states of the fp8-cache oracle differ from the plain oracle's by at least twice the GPU
    test's starting gate (2.26e-2 of max|ref| measured, the gate starts at 1e-2): a kernel that skipped the quantisation
    cannot pass that gate."""
    from oracle import make_golden_mllm as G
    eos = int(dict(np.load(GOLD))["a_eos"])
    plain = K8.tiny_oracle(("plain", "a"), G.tiny_prompt(), eos, kv8=False)
    kv8 = K8.tiny_oracle(("kv8", "a"), G.tiny_prompt(), eos)
    n = min(len(plain["hidden"]), len(kv8["hidden"]))
    assert n >= G.N_IMG
    d = (kv8["hidden"][:n] - plain["hidden"][:n]).abs().max().item() / kv8["hidden"][:n].abs().max().item()
    print("distance between the oracles", d)
    assert d >= 2 * K8.HIDDEN_GATE_START, d
