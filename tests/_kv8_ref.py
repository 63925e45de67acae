"""References of the fp8 KV cache (`LlamaDecodeEngine(kv_dtype="fp8")`, csrc/llm.hip: llm_attn_body<D, true>), plain PyTorch
on the CPU.

The quantiser's reference is `diffsensei_amd.mllm.quantize_kv_fp8` itself: tests/test_mllm_kv8_host.py pins it (no NaN code,
the exponent rule, idempotence, half a step of error).  The mode's reference is "attention over the dequantised cache":

* `attention_over_cache_ref` - tests/_llm_attn_ref.causal_attention_ref with the keys taken as already rotated (the cache
  holds rotated keys; the q rows are rotated here): same rounding points (fp16 probabilities), fp32;
* `llama_forward_kv8` - oracle.llama_ref.llama_forward with k (after the rotation) and v passed through quantise /
  dequantise before they are used and before they enter the cache.  `kv8_oracle()` swaps it in for the duration of a
  `with` block, so `oracle.llama_ref.lvlm_generate` / `greedy_generate` run the fp8-cache model; oracle/ is not edited.

The fp8 kernel reads 8 codes per lane, so its loop constants are the fp16 kernel's: `kpw`, `boundary_keys` and the case
lists of tests/_llm_attn_ref.py hold for it unchanged and are re-exported here.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from diffsensei_amd.mllm import dequantize_kv_fp8, quantize_kv_fp8
from oracle import llama_ref as R
from tests import _llm_attn_ref as A

ATT_WAVES, SOFTMAX_STRIDE = A.ATT_WAVES, A.SOFTMAX_STRIDE
kpw = A.kpw                                     # keys per wavefront and iteration of the fp8 form: 64 / (D / 8), as fp16
boundary_keys = A.boundary_keys


def qdq(x: torch.Tensor) -> torch.Tensor:
    """x [..., D] seen through the cache: fp32"""
    return dequantize_kv_fp8(*quantize_kv_fp8(x))


def attention_over_cache_ref(q, k_deq, v_deq, pos0: int, theta: float = 10000.0):
    """q [M, heads, D] un-rotated rows at positions pos0 .. pos0+M-1; k_deq (rotated), v_deq [T >= pos0+M, kv_heads, D]: the
    dequantised cache rows 0 .. T-1.  Row r sees keys 0 .. pos0+r.  Returns out [M, heads*D] fp32."""
    M, Hh, D = q.shape
    T, Hkv, _ = k_deq.shape
    assert T >= pos0 + M and Hh % Hkv == 0
    rep = Hh // Hkv
    cos, sin = R.rope_tables(D, T, theta)
    qr = R.apply_rope(q.float(), cos[pos0:pos0 + M], sin[pos0:pos0 + M])
    s = torch.einsum("thd,shd->hts", qr, k_deq.float().repeat_interleave(rep, 1)) / math.sqrt(D)
    keep = torch.arange(T)[None, :] <= (pos0 + torch.arange(M))[:, None]
    p = s.masked_fill(~keep[None], float("-inf")).softmax(-1).half().float()     # the reference casts P to fp16
    return torch.einsum("hts,shd->thd", p, v_deq.float().repeat_interleave(rep, 1)).reshape(M, Hh * D)


def rotated_keys_ref(k, theta: float = 10000.0):
    """k [T, kv_heads, D] un-rotated fp16 -> the fp16 rotated keys the fp16 cache would hold (fp32 rotation, one rounding)"""
    T, _, D = k.shape
    cos, sin = R.rope_tables(D, T, theta)
    return R.apply_rope(k.float(), cos, sin).half()


def llama_forward_kv8(sd, cfg, x, cache):
    """oracle.llama_ref.llama_forward, every new k and v seen through the fp8 cache format"""
    T = x.shape[0]
    Hh, D = cfg.num_attention_heads, cfg.head_dim
    pos0 = cache.length
    cos, sin = R.rope_tables(D, pos0 + T, cfg.rope_theta)
    cos, sin = cos[pos0:], sin[pos0:]
    h = x.float()
    for li in range(cfg.num_hidden_layers):
        p = f"model.layers.{li}."
        xn = R.rms_norm(h, sd[p + "input_layernorm.weight"].float(), cfg.rms_norm_eps)
        q = (xn @ sd[p + "self_attn.q_proj.weight"].float().T).view(T, Hh, D)
        k = (xn @ sd[p + "self_attn.k_proj.weight"].float().T).view(T, Hh, D)
        v = (xn @ sd[p + "self_attn.v_proj.weight"].float().T).view(T, Hh, D)
        q, k = R.apply_rope(q, cos, sin), qdq(R.apply_rope(k, cos, sin))
        v = qdq(v)
        if cache.k[li] is not None:
            k = torch.cat([cache.k[li], k], 0)
            v = torch.cat([cache.v[li], v], 0)
        cache.k[li], cache.v[li] = k, v
        s = torch.einsum("thd,shd->hts", q, k) / math.sqrt(D)
        keep = torch.arange(pos0 + T)[None, :] <= (pos0 + torch.arange(T))[:, None]
        s = s.masked_fill(~keep[None], float("-inf"))
        a = torch.einsum("hts,shd->thd", s.softmax(-1), v).reshape(T, Hh * D)
        h = h + a @ sd[p + "self_attn.o_proj.weight"].float().T
        xn = R.rms_norm(h, sd[p + "post_attention_layernorm.weight"].float(), cfg.rms_norm_eps)
        g = xn @ sd[p + "mlp.gate_proj.weight"].float().T
        u = xn @ sd[p + "mlp.up_proj.weight"].float().T
        h = h + (F.silu(g) * u) @ sd[p + "mlp.down_proj.weight"].float().T
    cache.length = pos0 + T
    hn = R.rms_norm(h, sd["model.norm.weight"].float(), cfg.rms_norm_eps)
    return hn, hn @ sd["lm_head.weight"].float().T


@contextlib.contextmanager
def kv8_oracle():
    """oracle.llama_ref with `llama_forward` replaced by `llama_forward_kv8` inside the block"""
    saved = R.llama_forward
    R.llama_forward = llama_forward_kv8
    try:
        yield R
    finally:
        R.llama_forward = saved


# ---- the tiny-model cases shared by tests/test_mllm_kv8_host.py (preconditions, CPU) and tests/test_gpu_mllm_kv8.py
BATCH_PROMPTS = [(22, 17, 3), (29, 20, 3), (24, 30, 2)]     # (seed, n1, n2) of test_gpu_mllm_fp4.make_prompt
FP4_PROMPT = (26, 14, 2)                                    # the mxfp4 + fp8-cache case (margins: test_gpu_mllm_kv8.py)
MARGIN = 5e-2                                               # the id rule of test_gpu_mllm.py: below it a pick may flip
HIDDEN_GATE_START = 1e-2                                    # starting bound of the hidden-state / img_gen_feat gates

_ORACLE = {}


def tiny_oracle(key, prompt, eos, kv8=True, sd=None):
    """`oracle.llama_ref.lvlm_generate` of the tiny model on `prompt` = (ids, mask, image_embeds), computed once per `key`
    and shared by every test that needs it (never modified)."""
    if key not in _ORACLE:
        from oracle import make_golden_mllm as G
        sd = G.tiny_weights() if sd is None else sd
        sd_in, sd_out = G.tiny_resampler(G.RES_IN, 11), G.tiny_resampler(G.RES_OUT, 12)
        heads = (G.RES_IN["num_heads"], G.RES_OUT["num_heads"])
        ids, mask, img = prompt
        with (kv8_oracle() if kv8 else contextlib.nullcontext()):
            _ORACLE[key] = R.lvlm_generate(sd, R.LlamaRefConfig(**G.TINY), sd_in, sd_out, heads, ids, img, mask, G.IMG_IDS,
                                           eos, G.MAX_NEW, G.N_IMG)
    return _ORACLE[key]
