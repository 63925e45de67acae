"""MLLM pre-pass on MI355X: the producer of `ip_image_embeds` for the sampler.

Mirrors, for batch 1 and greedy decoding (the only mode the reference uses: `do_sample=False`, `num_beams=1`):
  * `ContinuousLVLM.generate`           reference src/models/mllm/seed_x.py:90-171
  * `LlamaForCausalLM` + KV cache       reference src/models/mllm/modeling_llama_xformer.py:97-314, 428-610
  * `AutoImageTokenGenerationProcessor` reference src/models/mllm/generation.py:19-30 (folded into the pick kernel)
  * `QwenResampler`                     reference src/models/qwen_resampler.py:87-145
  * the hand-off into the sampler       reference scripts/demo/gradio.py:85-109  (`mllm_prepass`)

Execution model: every weight is read once per generated token, so decoding is HBM-bound; one token step is a static
list of `DS_OP_LLM_*` launches (csrc/llm.hip) whose step-varying scalars live in a device-side state block, captured
once into a hipGraph and replayed per token.  The host looks at the device only every `poll_every` tokens (one 32-byte
copy) to see whether EOS was produced.  The prompt is one pass per layer: projections through the MFMA GEMMs
(`ops.gemm`), attention through the decode kernel in 16-row chunks (`prompt_path="mfma"`, 22 ms for 96 tokens at 13B
dims); `prompt_path="chunks"` runs it through the token kernels 16 rows at a time instead (166 ms; kept for A/B).

Host-side packing (once): q|k|v and gate|up projections stacked; the two RMSNorm gains of each layer stay vectors and are
applied in the GEMV prologue at the reference's rounding points (normalise in fp32, round to fp16, times the fp16 gain -
folding them into the fp16 weights would round once instead of twice and can flip greedy near-ties); QwenResampler: the constant query projection and the position-embedding contribution to the keys are
precomputed (they depend on weights only).  There is no CPU/PyTorch execution path: without the HIP library every call
raises.

Batched decode (`LlamaDecodeEngine(max_sequences=S)`, `generate_batch`, `ContinuousLVLM.generate_batch`,
`mllm_prepass_batch`): the token loop is HBM-bound on the weights, and a step for up to 16 sequences reads the same
weights as a step for one.  The engine owns S cache slots, an int32 [S][8] state block, and per-slot id and feature
buffers; a sequence is a batch of one slot, so both entries are one decode loop (`_decode`) over one token plan built at
a width: width 1 for `generate` (slot 0, projections on the `llm_gemv` kernels), width S for `generate_batch` (one static
launch list over all S rows, `llm_gemm16_kernel` for every projection, whatever number of slots is in use); embed,
attention, final norm and pick are the slot-form ops in both.  A sequence's ids and hidden states do not depend on what
the other slots hold or on the slot it sits in.  A finished or unused slot is skipped by every kernel that writes
per-slot state.  KV memory: a slot is 2 x layers x T_max x kv_heads x head_dim fp16 = 0.84 GB at
13B dimensions and T_max 1024 (13.4 GB for 16 slots, next to 26 GB of weights).

int8 weight-only decoding (`LlamaDecodeEngine(weight_dtype="int8")`, W8A16): the four projection groups of every layer
are stored as int8 with one fp32 scale per output row (`quantize_rows_int8`), activations stay fp16, and the token step
runs the int8 forms of the same kernels (`DS_OP_LLM_GEMV_W8` / `DS_OP_LLM_GEMM16_W8`: exact int8 -> f16 unpack in
registers, fp32 accumulation, the row scale in the epilogue), so a step streams about half the bytes.  The embedding,
`lm_head` and every RMSNorm gain stay fp16.  The prompt pass dequantises one matrix at a time into a reusable fp16
scratch (`llm_dequant_w8_kernel`) and keeps the MFMA GEMMs.  Opt-in: the default stays fp16, bit for bit.

MXFP4 weight-only decoding (`LlamaDecodeEngine(weight_dtype="mxfp4")`, W4A16): the same four groups in the OCP MX fp4
format plus one fp32 scale per row (`quantize_rows_mxfp4`: packed e2m1 elements, one E8M0 exponent per 32-element block),
a quarter of the fp16 bytes plus 1/32 for the block exponents.  The token step runs `DS_OP_LLM_GEMV_FP4` /
`DS_OP_LLM_GEMM16_FP4` (gfx950's `v_cvt_scalef32_pk_f16_fp4` unpacks a byte into two f16 values times the block scale,
exactly); the prompt pass dequantises through `llm_dequant_fp4_kernel`.  Everything else is as for int8, opt-in included.
On Gaussian weights the format's relative rms error is 11 % (int8 per row: 0.9 %); no parity figure for a trained 13B
checkpoint can be produced offline, so what the mode does to the agent's output quality is not measured.

FP8 KV cache (`LlamaDecodeEngine(kv_dtype="fp8")`, independent of `weight_dtype`): every cache row and kv head is stored as
head_dim OCP e4m3 codes and one exponent byte (`quantize_kv_fp8`: value = f32(e4m3) * 2^(e - 127), the exponent the smallest
that brings the head's largest magnitude to <= 448, so the scaling is exact and the one rounding is fp32 -> e4m3), K after
the rotation and its rounding to fp16, V as projected.  A slot then costs 2 x layers x T_max x kv_heads x (head_dim + 1)
bytes, (head_dim + 1) / (2 head_dim) = 0.504 of the fp16 cache at head_dim 128: 0.42 GB per slot and 6.8 GB for 16 slots at
13B dimensions and T_max 1024 (`kv_cache_bytes()`).  The token step and the prompt pass run the fp8-cache forms of the
attention op (`DS_OP_LLM_ATTN_KV8` / `DS_OP_LLM_ATTN_SLOTS_KV8`: `v_cvt_pk_f32_fp8` unpacks two codes per instruction, the
power of two multiplies the finished score or the probability); every key and value, the launch's own rows included, is
seen through the quantiser, so the result is attention over the dequantised cache whatever the chunking.  Opt-in: the
default stays fp16, bit for bit.  A quantised mode with its own error (2.6 % relative rms on Gaussian heads; on the tiny test
model the fed-back hidden states move by 2.2e-2 of max|ref| and the greedy ids stay the same); what it does to a trained 13B
checkpoint's output cannot be measured offline and is not measured.  Decode rate: `profiles/mllm_kv8_decode.txt`.

Chain fast-forward (`LlamaDecodeEngine(chain_fast_forward=True)`, independent of `weight_dtype`, `kv_dtype`, `use_graph`,
`prompt_path` and `max_sequences`): the image-token processor folded into the pick kernel forces the successor of any id in
chain[:-1], so once a sequence's current token lies in the chain every following id up to and including </img> is known
before a weight is read (`forced_run`, pure host arithmetic).  With the mode on the pick kernel marks such a slot
(state[2] = 2, "paused": every per-slot kernel leaves it alone, as it does a finished one); the host, which reads the state
block after the prompt pass and after every burst, then runs the forced rows of all paused slots in ONE pass - the embeddings
of [cur] + f[:-1] at the slot's next positions through `_layers_mfma`, the layer loop of the prompt pass (MFMA GEMMs, int8 /
mxfp4 from the dequantised scratch) with one launch of the ragged attention kernel per layer (`DS_OP_LLM_ATTN_ROWS[_KV8]`,
`llm_attn_rows_kernel`: a row table (slot, row), every slot at its own cache length, segments of any length) - stores the
final norm of every row as the fed-back hidden state of its id, writes the ids and rewrites the slot's state row; no lm_head,
no pick.  The token loop then goes on with </img> as the current token.  Teacher forcing with the ids the pick kernel would
have produced: the same ids; the hidden states differ from the default's by fp16 rounding (other GEMM kernels), which can flip
a free near-tie after </img>.  What that does to a trained 13B checkpoint cannot be measured offline.  The first forced id
after an <img>-ending prompt is still the prompt pass's own pick.  At 13B dimensions, 96-row prompt ending in <img>, 64 image
tokens, 120 new ids: 628 -> 314 ms for one sequence, 1255 -> 702 ms for 16 (`profiles/mllm_chain_ff.txt`).
A chain with a repeated id is refused in this mode.  Opt-in: the default stays as it is, bit for bit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib, ops
from .engine import Plan, make_op

Tensor = torch.Tensor
CHUNK = 16  # prompt rows per pass (llm.hip: M <= 16)


@dataclass
class LlamaConfig:
    vocab_size: int = 32330            # LLaMA-2 vocabulary + the MLLM's added image/box tokens
    hidden_size: int = 5120            # LLaMA-2-13B dims (the SEED-X agent the reference loads, gradio.py:256-257)
    intermediate_size: int = 13824
    num_hidden_layers: int = 40
    num_attention_heads: int = 40
    num_key_value_heads: Optional[int] = None
    rms_norm_eps: float = 1e-5
    rope_theta: float = 10000.0

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @property
    def kv_heads(self) -> int:
        return self.num_key_value_heads or self.num_attention_heads

    @classmethod
    def from_hf(cls, c) -> "LlamaConfig":
        g = lambda k, d=None: getattr(c, k, d) if not isinstance(c, dict) else c.get(k, d)
        return cls(g("vocab_size"), g("hidden_size"), g("intermediate_size"), g("num_hidden_layers"),
                   g("num_attention_heads"), g("num_key_value_heads"), g("rms_norm_eps", 1e-6),
                   g("rope_theta", 10000.0) or 10000.0)


def llama_param_shapes(cfg: LlamaConfig) -> Dict[str, tuple]:
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    kv = cfg.kv_heads * cfg.head_dim
    s = {"model.embed_tokens.weight": (V, H), "model.norm.weight": (H,), "lm_head.weight": (V, H)}
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        s[p + "self_attn.q_proj.weight"] = (H, H)
        s[p + "self_attn.k_proj.weight"] = (kv, H)
        s[p + "self_attn.v_proj.weight"] = (kv, H)
        s[p + "self_attn.o_proj.weight"] = (H, H)
        s[p + "mlp.gate_proj.weight"] = (I, H)
        s[p + "mlp.up_proj.weight"] = (I, H)
        s[p + "mlp.down_proj.weight"] = (H, I)
        s[p + "input_layernorm.weight"] = (H,)
        s[p + "post_attention_layernorm.weight"] = (H,)
    return s


def random_llama_state_dict(cfg: LlamaConfig, device, seed: int = 0) -> Dict[str, Tensor]:
    """Seeded fp16 weights at the real shapes, generated on the device (no checkpoints exist offline)."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in llama_param_shapes(cfg).items():
        if len(shape) == 1:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g, device=device)
        else:
            std = 0.5 if "embed_tokens" in name else 1.0 / math.sqrt(shape[1])
            t = torch.randn(shape, generator=g, device=device, dtype=torch.float16).float() * std
        sd[name] = t.to(torch.float16)
    return sd


def quantize_rows_int8(w: Tensor):
    """Per-row symmetric int8 of a weight matrix [N, K] -> (q int8 [N, K], s fp32 [N]) with w ~ q * s[:, None].
    `w` is first rounded to fp16 (what the engine holds today), then: s[n] = max_k |w[n, k]| / 127 in fp32 (1 for an
    all-zero row), q = clamp(round_half_even(w / s), -127, 127).  Works on host and device tensors; the scales are per
    output row, so quantising stacked matrices (q|k|v, gate|up) equals stacking the quantised ones."""
    if w.dim() != 2:
        raise ValueError(f"quantize_rows_int8 takes a matrix [N, K], got {tuple(w.shape)}")
    w = w.detach().to(torch.float16).to(torch.float32)
    amax = w.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.clamp(torch.round(w / s[:, None]), -127, 127).to(torch.int8)      # torch.round: half to even
    return q.contiguous(), s.contiguous()


def dequantize_rows_int8(q: Tensor, s: Tensor) -> Tensor:
    """fp32 [N, K] = q * s[:, None] (one fp32 multiply per element: what the int8 kernels compute with)."""
    return q.to(torch.float32) * s.to(torch.float32)[:, None]


E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # code 0..7 of an fp4 e2m1 magnitude (bit 3 of the nibble: sign)
MX_BLOCK = 32                                                # elements along K that share one E8M0 exponent
MX_MIN_EXP = -13                                             # stored exponents lie in [114, 127]


def quantize_rows_mxfp4(w: Tensor):
    """MXFP4 with one extra fp32 scale per row, of a weight matrix [N, K] (K % 32 == 0) ->
    (q uint8 [N, K/2], e uint8 [N, K/32], s fp32 [N]) with w ~ e2m1(q) * 2^(e - 127) * s[:, None].
    `w` is first rounded to fp16 (what the engine holds today), then: s[n] = max_k |w[n, k]| / 6 in fp32 (1 for an all-zero
    row); the row / s[n] is cut into blocks of 32 along K; a block whose largest magnitude is a gets the exponent
    floor(log2 a) - 2 (the OCP MX rule for an element format whose largest exponent is 2), clamped to [-13, 0] - never above
    0 because a normalised row does not exceed 6 - and stored biased, e = exponent + 127 (an all-zero block stores 114); the
    elements are x / 2^exponent, saturated to +-6 and rounded to the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the
    even mantissa (0.25 -> 0, 0.75 -> 1, 2.5 -> 2, 5 -> 4), as sign + 3 bits, two per byte with element 2i in the low nibble.
    The clamp at -13: every e2m1 * 2^exponent is then a NORMAL f16 number (the smallest, 0.5 * 2^-13 = 2^-14, is f16's
    smallest normal), so the kernels' in-register conversion to f16 is exact and no fdot2 / MFMA operand is subnormal.  What
    the clamp flushes to zero lies below 0.25 * 2^-13 = 2^-15 of the normalised row, i.e. below 2^-15 * 6 of the row's
    largest weight.  Works on host and device tensors; scales are per row and per block, so quantising stacked matrices
    (q|k|v, gate|up) equals stacking the quantised ones."""
    if w.dim() != 2:
        raise ValueError(f"quantize_rows_mxfp4 takes a matrix [N, K], got {tuple(w.shape)}")
    N, K = w.shape
    if K % MX_BLOCK:
        raise ValueError(f"quantize_rows_mxfp4: K = {K} is not a multiple of {MX_BLOCK}")
    w = w.detach().to(torch.float16).to(torch.float32)
    amax = w.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / 6.0, torch.ones_like(amax))
    x = (w / s[:, None]).view(N, K // MX_BLOCK, MX_BLOCK)
    a = x.abs().amax(dim=2)
    ex = torch.frexp(a).exponent.to(torch.int32) - 1 - 2            # a = m 2^k, m in [0.5, 1): floor(log2 a) = k - 1
    ex = torch.where(a > 0, ex, torch.full_like(ex, MX_MIN_EXP)).clamp_(MX_MIN_EXP, 0)
    y = torch.ldexp(x, -ex[:, :, None]).view(N, K)                  # exact: a power of two
    mag = y.abs().clamp_(max=6.0)
    code = torch.zeros_like(mag, dtype=torch.uint8)
    for i in range(7):                                              # midpoint i lies between codes i and i + 1; a tie goes to the
        mid = 0.5 * (E2M1_VALUES[i] + E2M1_VALUES[i + 1])           # even code (mantissa bit 0): up when i is odd
        code += ((mag >= mid) if i % 2 else (mag > mid)).to(torch.uint8)
    code |= ((y < 0) & (code > 0)).to(torch.uint8) << 3
    q = code[:, 0::2] | (code[:, 1::2] << 4)
    return q.contiguous(), (ex + 127).to(torch.uint8).contiguous(), s.contiguous()


def dequantize_rows_mxfp4(q: Tensor, e: Tensor, s: Tensor) -> Tensor:
    """fp32 [N, K] = f32(e2m1) * 2^(e - 127) * s[:, None]: the block product is exact, the row scale is one fp32 multiply per
    element (what the MXFP4 kernels compute with)."""
    N, K = q.shape[0], 2 * q.shape[1]
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=q.device)
    v = torch.stack([lut[(q & 15).long()], lut[(q >> 4).long()]], dim=2).view(N, K // MX_BLOCK, MX_BLOCK)
    v = torch.ldexp(v, (e.to(torch.int32) - 127)[:, :, None]).view(N, K)
    return v * s.to(torch.float32)[:, None]


KV8_MAX = 448.0                                              # largest finite OCP e4m3fn value


def quantize_kv_fp8(x: Tensor):
    """The fp8 KV-cache format of heads [..., D] -> (codes uint8 [..., D], exponents uint8 [...]) with
    x ~ f32(e4m3(codes)) * 2^(exponents - 127).  `x` is first rounded to fp16 (what the fp16 cache holds: the rotated key,
    the value as projected), then per head: amax = its largest magnitude = m 2^k with m in [0.5, 1); ex = k - 9 if m <= 0.875
    else k - 8 - the smallest integer with amax / 2^ex <= 448 - and 0 for an all-zero head (for fp16 input ex lies in
    [-33, 8]: no clamp); the codes are x / 2^ex (exact: a power of two) rounded once, fp32 -> OCP e4m3fn, to nearest even with
    subnormals kept.  Nothing saturates, since no scaled value exceeds 448 (`to(torch.float8_e4m3fn)` would return NaN above
    464).  The exponent is stored biased, e = ex + 127.  Works on host and device tensors; everything is per head, so
    quantising stacked heads equals stacking the quantised ones.  The kernels compute the same bits (csrc/llm.hip:
    kv8_quantize).  On Gaussian heads the relative rms error is 2.6 %; what the format does to a trained 13B checkpoint's
    output cannot be measured offline."""
    if x.dim() < 1:
        raise ValueError("quantize_kv_fp8 takes heads [..., D]")
    x = x.detach().to(torch.float16).to(torch.float32)
    amax = x.abs().amax(dim=-1)
    m, k = torch.frexp(amax)
    ex = k.to(torch.int32) - torch.where(m <= 0.875, 9, 8).to(torch.int32)
    ex = torch.where(amax > 0, ex, torch.zeros_like(ex))
    y = torch.ldexp(x, -ex[..., None])                              # exact: a power of two
    codes = y.to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.contiguous(), (ex + 127).to(torch.uint8).contiguous()


def dequantize_kv_fp8(codes: Tensor, exps: Tensor) -> Tensor:
    """fp32 [..., D] = f32(e4m3(codes)) * 2^(exps - 127): exact (what the fp8-cache attention computes with)."""
    v = codes.contiguous().view(torch.float8_e4m3fn).to(torch.float32)
    return torch.ldexp(v, (exps.to(torch.int32) - 127)[..., None])


def forced_run(chain: Sequence[int], cur: int, n_out: int, max_new: int, eos: int) -> List[int]:
    """The ids the pick kernel (`llm_select_body`, csrc/llm.hip) would append one by one without looking at a logit, starting
    with current token `cur` and `n_out` ids already out: while `cur` lies in chain[:-1] and fewer than `max_new` ids are out,
    the successor of `cur` in the chain is appended and becomes `cur`; the run ends after `eos` was appended (the kernel
    finishes the sequence there) and when `max_new` ids are out.  Pure host arithmetic on a chain without repeated ids (with
    repeats the kernel's rule and the reference's `.index()` rule differ: `set_image_token_chain` refuses them in this mode)."""
    succ = {int(a): int(b) for a, b in zip(chain[:-1], chain[1:])}
    out: List[int] = []
    cur, n_out = int(cur), int(n_out)
    while cur in succ and n_out < max_new:
        cur = succ[cur]
        out.append(cur)
        n_out += 1
        if cur == eos:
            break
    return out


class LlamaDecodeEngine:
    """Device-resident LLaMA decoder + KV cache + the captured one-token launch plan."""

    def __init__(self, cfg: LlamaConfig, sd: Dict[str, Tensor], device, max_positions: int = 1024,
                 max_new_tokens: int = 512, use_graph: bool = True, poll_every: int = 8, prompt_path: str = "mfma",
                 max_sequences: int = 1, weight_dtype: str = "float16", kv_dtype: str = "float16",
                 chain_fast_forward: bool = False):
        """max_sequences S > 1: `generate_batch` decodes up to S sequences per weight pass; the engine then holds S KV-cache
        slots (each 2 x layers x max_positions x kv_heads x head_dim fp16: 0.84 GB at 13B dimensions and 1024 positions)
        and [S] state / id / feature / logits rows.  `generate` is one sequence in slot 0, whatever S is.
        prompt_path applies to `generate` only: `generate_batch` always takes the MFMA prompt pass.
        weight_dtype "int8": the q|k|v, o, gate|up and down matrices are held as int8 with fp32 row scales (W8A16, see
        `quantize_rows_int8`); the embedding, lm_head and the RMSNorm gains stay fp16.
        weight_dtype "mxfp4": the same matrices as MXFP4 (W4A16, see `quantize_rows_mxfp4`): packed e2m1 [N, K/2], block
        exponents [N, K/32] and fp32 row scales.  Its effect on a trained checkpoint's output is not measured.
        kv_dtype "fp8": the KV cache holds OCP e4m3 codes and one power-of-two exponent byte per (row, kv head) (see
        `quantize_kv_fp8`): (head_dim + 1) / (2 head_dim) of the fp16 cache's bytes, and attention over the dequantised
        cache.  Independent of weight_dtype.  Its effect on a trained checkpoint's output is not measured either.
        chain_fast_forward: once the current token of a sequence lies in the image-token chain, every following id up to
        </img> is known; the decoder then runs those rows in one pass through the prompt pass's MFMA GEMMs and one ragged
        attention launch per layer instead of one token step each (see the module docstring).  Teacher forcing with the ids
        the pick kernel would have produced: the same ids, hidden states that differ by fp16 rounding (other GEMM kernels).
        Independent of every other argument; needs a chain without repeated ids."""
        _lib.load()
        self.chain_fast_forward = bool(chain_fast_forward)
        if kv_dtype not in ("float16", "fp8"):
            raise ValueError(f"kv_dtype {kv_dtype!r}: 'float16' or 'fp8'")
        self.kv_dtype = kv_dtype
        if weight_dtype not in ("float16", "int8", "mxfp4"):
            raise ValueError(f"weight_dtype {weight_dtype!r}: 'float16', 'int8' or 'mxfp4'")
        self.weight_dtype = weight_dtype
        kmul = {"float16": 8, "int8": 16, "mxfp4": MX_BLOCK}[weight_dtype]     # weights per 16-byte load: K is a multiple
        quantised = weight_dtype != "float16"
        if not 1 <= int(max_sequences) <= CHUNK:
            raise ValueError(f"max_sequences {max_sequences} outside [1, {CHUNK}] (rows of one weight pass)")
        self.max_sequences = S = int(max_sequences)
        if prompt_path not in ("mfma", "chunks"):
            raise ValueError("prompt_path: 'mfma' (GEMM projections) or 'chunks' (16-row passes of the token kernels)")
        self.cfg, self.dev = cfg, torch.device(device)
        self.T_max, self.cap = int(max_positions), int(max_new_tokens)
        self.use_graph, self.poll_every = use_graph, max(1, int(poll_every))
        H, I, V, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
        D, Hq, Hkv = cfg.head_dim, cfg.num_attention_heads, cfg.kv_heads
        if D not in (64, 128):
            raise ValueError(f"head_dim {D}: the decode attention kernel is built for 64 and 128")
        if H % 8 or I % 8:
            raise ValueError("hidden and intermediate sizes must be multiples of 8")
        if quantised and (H % kmul or I % kmul or (Hq * D) % kmul):
            raise ValueError(f"weight_dtype={weight_dtype!r}: K of every quantised matrix (hidden, heads * head_dim, intermediate "
                             f"size) must be a multiple of {kmul}")
        dev = self.dev
        f16 = lambda t: t.detach().to(device=dev, dtype=torch.float16).contiguous()

        stack = lambda ws: torch.cat([t.detach().to(dev) for t in ws], 0).to(torch.float16).contiguous()

        self.embed = f16(sd["model.embed_tokens.weight"])
        self.lm_head = f16(sd["lm_head.weight"])
        self.norm_g = f16(sd["model.norm.weight"])
        # q|k|v and gate|up are stacked (one weight stream per projection group); the RMSNorm gains stay separate vectors
        # applied in the GEMV prologue with the reference's rounding points (normalise, round to fp16, times the fp16 gain)
        self.wqkv, self.wo, self.wgu, self.wdown, self.g_in, self.g_post = [], [], [], [], [], []
        # int8 / mxfp4: the fp32 row scales of the four groups; mxfp4: their block exponents (empty lists otherwise)
        self.sqkv, self.so, self.sgu, self.sdown = [], [], [], []
        self.eqkv, self.eo, self.egu, self.edown = [], [], [], []

        def put(ws: list, ss: list, es: list, w16: Tensor) -> None:
            """one matrix at a time: its fp16 copy is dropped as soon as it is quantised"""
            if weight_dtype == "float16":
                ws.append(w16)
            elif weight_dtype == "int8":
                q, s = quantize_rows_int8(w16)
                ws.append(q)
                ss.append(s)
            else:
                q, e, s = quantize_rows_mxfp4(w16)
                ws.append(q)
                ss.append(s)
                es.append(e)

        for i in range(L):
            p = f"model.layers.{i}."
            put(self.wqkv, self.sqkv, self.eqkv, stack([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"]))
            self.g_in.append(f16(sd[p + "input_layernorm.weight"]))
            put(self.wo, self.so, self.eo, f16(sd[p + "self_attn.o_proj.weight"]))
            put(self.wgu, self.sgu, self.egu, stack([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]]))
            self.g_post.append(f16(sd[p + "post_attention_layernorm.weight"]))
            put(self.wdown, self.sdown, self.edown, f16(sd[p + "mlp.down_proj.weight"]))
        self._w16: Optional[Tensor] = None                  # int8 / mxfp4: fp16 scratch of the prompt pass (largest group), on first use
        E = lambda *s, dtype=torch.float16: torch.zeros(s, dtype=dtype, device=dev)
        self.qkv_dim = (Hq + 2 * Hkv) * D
        self.h, self.qkv, self.att = E(CHUNK, H), E(CHUNK, self.qkv_dim), E(CHUNK, Hq * D)
        self.act = E(CHUNK, I)
        # per slot: KV cache [S, T_max, kv_heads*D] per layer, state block, generated ids, fed-back hidden states, final-norm
        # row and logits.  `generate` uses slot 0.
        # kv_dtype "fp8": the caches hold code bytes, and kes / ves [S, T_max, kv_heads] the exponent byte of every head
        kv_t = torch.uint8 if kv_dtype == "fp8" else torch.float16
        self.kcs = [E(S, self.T_max, Hkv * D, dtype=kv_t) for _ in range(L)]
        self.vcs = [E(S, self.T_max, Hkv * D, dtype=kv_t) for _ in range(L)]
        self.kes = [E(S, self.T_max, Hkv, dtype=torch.uint8) for _ in range(L)] if kv_dtype == "fp8" else []
        self.ves = [E(S, self.T_max, Hkv, dtype=torch.uint8) for _ in range(L)] if kv_dtype == "fp8" else []
        self.state = E(S, 8, dtype=torch.int32)
        self.state[:, 2] = 1                                # no slot started: every per-slot kernel skips it
        self.out_ids, self.feats = E(S, self.cap, dtype=torch.int32), E(S, self.cap, H)
        self.feat = self.feats[0]                           # slot 0's rows: what `generate` fills
        self.hn, self.logits = E(S, H), E(S, V)
        inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
        fr = torch.outer(torch.arange(self.T_max, dtype=torch.float32), inv_freq)      # rotary table (weights-like)
        self.rope_cos, self.rope_sin = fr.cos().to(dev).contiguous(), fr.sin().to(dev).contiguous()
        self.state_pf = E(8, dtype=torch.int32)             # prompt pass: per-layer chunk cursor (see _prompt_mfma)
        self.prompt_path = prompt_path
        self.chain = E(1, dtype=torch.int32)
        self.n_chain = 0
        self._plans: Dict[tuple, Plan] = {}
        self._stream: Optional[torch.cuda.Stream] = None
        self.last_run_info: dict = {}

    @classmethod
    def from_pretrained_module(cls, llm, device, **kw) -> "LlamaDecodeEngine":
        """`llm`: a transformers/reference LlamaForCausalLM (anything with `.config` and `.state_dict()`)."""
        return cls(LlamaConfig.from_hf(llm.config), llm.state_dict(), device, **kw)

    def weight_bytes_per_token(self) -> int:
        """Algorithmic HBM bytes of one decode step: every layer matrix + lm_head once (+ one embedding row)."""
        n = sum(w.numel() for ws in (self.wqkv, self.wo, self.wgu, self.wdown) for w in ws)
        if self.weight_dtype != "float16":                  # the quantised bytes (int8: 1 per weight; mxfp4: 0.5 per weight + 1
            ns = sum(s.numel() for ss in (self.sqkv, self.so, self.sgu, self.sdown) for s in ss)     # per block) + 4 per row
            ne = sum(e.numel() for es in (self.eqkv, self.eo, self.egu, self.edown) for e in es)     # scale; lm_head is fp16
            return n + ne + 4 * ns + 2 * (self.lm_head.numel() + self.cfg.hidden_size)
        return 2 * (n + self.lm_head.numel() + self.cfg.hidden_size)

    def kv_cache_bytes(self) -> int:
        """Bytes of the KV cache over all slots and layers: 2 x layers x S x T_max x kv_heads x head_dim fp16 values, or -
        kv_dtype "fp8" - (head_dim + 1) bytes per (row, kv head) for K and for V: the codes and the exponent byte."""
        return sum(t.numel() * t.element_size() for ts in (self.kcs, self.vcs, self.kes, self.ves) for t in ts)

    def tensors(self) -> List[Tensor]:
        """Frozen weights in kernel layout (the multi-GPU weight broadcast list)."""
        return ([self.embed, self.lm_head, self.norm_g] + self.wqkv + self.wo + self.wgu + self.wdown + self.g_in + self.g_post
                + self.sqkv + self.so + self.sgu + self.sdown + self.eqkv + self.eo + self.egu + self.edown)

    # ---- launch lists ------------------------------------------------------------------------------------
    def _proj(self, code: str, w: Tensor, scales: tuple, i, l, p) -> object:
        """One projection launch: `code` (LLM_GEMV / LLM_GEMM16) as it is with fp16 weights (`scales` empty), its _W8 form
        with p[5] = the row scales for an int8 matrix, its _FP4 form with p[5] = the row scales and p[6] = the block
        exponents for an MXFP4 one.  p = (x, y, residual, gain)."""
        x, y, residual, gain = p
        if not scales:
            return make_op(code, i=i, f=(self.cfg.rms_norm_eps,), l=l, p=(x, w, y, residual) + ((gain,) if gain is not None else ()))
        return make_op(code + ("_W8", "_FP4")[len(scales) - 1], i=i, f=(self.cfg.rms_norm_eps,), l=l,
                       p=(x, w, y, residual, gain) + scales)

    def _scales(self, l: int):
        """What the (qkv, o, gate|up, down) matrices of layer l come with: nothing (fp16), the row scales (int8), the row
        scales and the block exponents (mxfp4)."""
        groups = ((self.sqkv, self.eqkv), (self.so, self.eo), (self.sgu, self.egu), (self.sdown, self.edown))
        return [tuple(t[l] for t in g if t) for g in groups]

    def _layer_ops(self, l: int, M: int, proj: str, slots: bool) -> list:
        """The five launches of layer l over M rows.  slots: every row is its own sequence (slot-form attention on the
        row's cache slot and state row); otherwise the rows are M positions of the sequence in slot 0."""
        c = self.cfg
        H, I, D, Hq, Hkv = c.hidden_size, c.intermediate_size, c.head_dim, c.num_attention_heads, c.kv_heads
        sq, so, sg, sd_ = self._scales(l)
        kv8 = self.kv_dtype == "fp8"
        al = (self.qkv_dim, Hkv * D, Hq * D)                                  # ldqkv, ldc, ldo; then the slot stride
        if kv8:                                                               # fp8 cache: l[4] = lde, l[5] = the exponents' slot stride
            al += (self.kcs[l].stride(0) if slots else 0, Hkv) + ((self.kes[l].stride(0),) if slots else ())
        elif slots:
            al += (self.kcs[l].stride(0),)
        return [
            self._proj(proj, self.wqkv[l], sq, (M, self.qkv_dim, H, 1, 0), (H, self.qkv_dim, 0),
                       (self.h, self.qkv, None, self.g_in[l])),
            make_op(("LLM_ATTN_SLOTS" if slots else "LLM_ATTN") + ("_KV8" if kv8 else ""), i=(M, Hq, Hkv, D, self.T_max),
                    f=(1.0 / math.sqrt(D),), l=al,
                    p=(self.qkv, self.kcs[l], self.vcs[l], self.rope_cos, self.rope_sin, self.att, self.state)
                    + ((self.kes[l], self.ves[l]) if kv8 else ())),
            self._proj(proj, self.wo[l], so, (M, H, Hq * D, 0, 0), (Hq * D, H, H), (self.att, self.h, self.h, None)),
            self._proj(proj, self.wgu[l], sg, (M, I, H, 1, 1), (H, I, 0), (self.h, self.act, None, self.g_post[l])),
            self._proj(proj, self.wdown[l], sd_, (M, H, I, 0, 0), (I, H, H), (self.act, self.h, self.h, None)),
        ]

    def _token_ops(self, width: int) -> list:
        """One token step for the first `width` slots, one row each: slot-form embed / attention / final norm with tap /
        pick, and every projection on `llm_gemv` kernels at width 1 (`generate`), on `llm_gemm16_kernel` at the engine's
        width S (`generate_batch`, whatever number of slots is in use)."""
        c = self.cfg
        H, V, eps = c.hidden_size, c.vocab_size, c.rms_norm_eps
        proj = "LLM_GEMV" if width == 1 else "LLM_GEMM16"
        ops_ = [make_op("LLM_EMBED_SLOTS", i=(width, H, V), l=(H,), p=(self.embed, self.state, self.h))]
        for l in range(c.num_hidden_layers):
            ops_ += self._layer_ops(l, width, proj, slots=True)
        ops_.append(make_op("LLM_RMSNORM_SLOTS", i=(width, H, self.cap), f=(eps,), l=(H, H),
                            p=(self.h, self.norm_g, self.hn, self.feats, self.state)))
        ops_.append(make_op(proj, i=(width, V, H, 0, 0), f=(eps,), l=(H, V, 0), p=(self.hn, self.lm_head, self.logits, None)))
        ops_.append(make_op("LLM_SELECT_SLOTS", i=(V, self.n_chain, self.cap, 1, width, int(self.chain_fast_forward)),
                            l=(V,),
                            p=(self.logits, self.chain if self.n_chain else None, self.state, self.out_ids)))
        return ops_

    def _chunk_ops(self, M: int, kind: str) -> list:
        """M <= 16 prompt rows of the sequence in slot 0 through the token kernels.  kind: 'chunk' (more rows follow),
        'last' (final prompt chunk -> first token)."""
        c = self.cfg
        H, V, eps = c.hidden_size, c.vocab_size, c.rms_norm_eps
        ops_ = []
        for l in range(c.num_hidden_layers):
            ops_ += self._layer_ops(l, M, "LLM_GEMV", slots=False)
        if kind == "chunk":
            ops_.append(make_op("LLM_ADVANCE", i=(M,), p=(self.state,)))
            return ops_
        last_row = self.h.data_ptr() + (M - 1) * H * 2
        ops_.append(make_op("LLM_RMSNORM", i=(1, H, self.cap), f=(eps,), l=(H, H),
                            p=(last_row, self.norm_g, self.hn, None, self.state)))
        ops_.append(make_op("LLM_GEMV", i=(1, V, H, 0, 0), f=(eps,), l=(H, V, 0),
                            p=(self.hn, self.lm_head, self.logits, None)))
        ops_.append(make_op("LLM_SELECT", i=(V, self.n_chain, self.cap, M, int(self.chain_fast_forward)),
                            p=(self.logits, self.chain if self.n_chain else None, self.state, self.out_ids)))
        return ops_

    def weights_changed(self) -> None:
        """The weight tensors moved or changed (multi-GPU broadcast into the weight arena): cached launch plans hold raw
        pointers and are rebuilt on next use."""
        self._plans.clear()

    def _plan(self, M: int, kind: str) -> Plan:
        """kind 'token': the token step at width M; 'chunk' / 'last': M prompt rows"""
        key = (M, kind, self.n_chain, self.chain.data_ptr(), self.chain_fast_forward)
        pl = self._plans.get(key)
        if pl is None:
            pl = Plan(self._token_ops(M) if kind == "token" else self._chunk_ops(M, kind), keep=[self])
            self._plans[key] = pl
        return pl

    def set_image_token_chain(self, img_ids_list: Optional[Sequence[int]]) -> None:
        """[<img>, <img_00000> .. <img_{n-1}>, </img>] of the logits processor (None/empty = plain greedy)."""
        ids = [int(v) for v in (img_ids_list or [])]
        if self.chain_fast_forward and len(set(ids)) != len(ids):
            raise ValueError("chain_fast_forward: the image-token chain repeats an id; the successor of a repeated id is not "
                             "defined the same way by the pick kernel and by the reference")
        if ids == getattr(self, "_chain_ids", None):
            return
        self._chain_ids = ids
        self.n_chain = len(ids)
        self.chain = torch.tensor(ids or [0], dtype=torch.int32, device=self.dev)
        self._plans.clear()

    # ---- generation --------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, inputs_embeds: Tensor, last_prompt_id: int, eos_token_id: int, max_new_tokens: int) -> dict:
        """Greedy decoding from prompt embeddings [T0, hidden] (fp16, device).  Returns the new ids [n] (int64, device)
        and `hidden` [n-1, hidden]: the post-final-norm state of every generated token that was fed back."""
        out = self._decode([inputs_embeds], [int(last_prompt_id)], [int(eos_token_id)], [int(max_new_tokens)], [0], width=1)
        info = self.last_run_info
        self.last_run_info = {"graph": info["graph"], "prompt_tokens": info["prompt_tokens"][0], "new_tokens": info["new_tokens"][0],
                              "token_steps_launched": info["token_steps_launched"], "ops_per_token": info["ops_per_token"],
                              "kv_dtype": info["kv_dtype"], "fast_forward_rows": info["fast_forward_rows"][0],
                              "fast_forward_passes": info["fast_forward_passes"]}
        return out[0]

    @torch.no_grad()
    def generate_batch(self, inputs_embeds: Sequence[Tensor], last_prompt_ids: Sequence[int], eos_token_ids,
                       max_new_tokens, slots: Optional[Sequence[int]] = None) -> List[dict]:
        """`generate` for 1 <= n <= max_sequences sequences of different prompt lengths in one decode loop.
        `eos_token_ids` / `max_new_tokens`: one value for all, or one per sequence.  `slots`: the cache slot of each
        sequence (default 0..n-1); results do not depend on it.  Returns one {"ids", "hidden"} per sequence."""
        S = self.max_sequences
        embs = list(inputs_embeds)
        n = len(embs)
        if S < 2:
            raise ValueError("generate_batch needs an engine built with max_sequences > 1")
        if not 1 <= n <= S:
            raise ValueError(f"{n} sequences: the engine has {S} slots")
        per = lambda v: [int(x) for x in v] if isinstance(v, (list, tuple)) else [int(v)] * n
        last, eos, max_new = per(list(last_prompt_ids)), per(eos_token_ids), per(max_new_tokens)
        slots = list(range(n)) if slots is None else [int(x) for x in slots]
        if not len(last) == len(eos) == len(max_new) == len(slots) == n:
            raise ValueError("one last_prompt_id / eos / max_new_tokens / slot per sequence is needed")
        if len(set(slots)) != n or min(slots) < 0 or max(slots) >= S:
            raise ValueError(f"slots {slots}: {n} different values in [0, {S}) are needed")
        return self._decode(embs, last, eos, max_new, slots, width=S)

    def _decode(self, embs: List[Tensor], last: List[int], eos: List[int], max_new: List[int], slots: List[int],
                width: int) -> List[dict]:
        """The decode loop of both entries: sequence i in cache slot slots[i], the token step over the first `width` slots
        (1: `generate`, slot 0; S: `generate_batch`).  Writes the state rows, runs the prompt pass, runs and captures the
        token plan, replays it in bursts of `poll_every`, polls the finished flags and reads back per slot."""
        S, H = self.max_sequences, self.cfg.hidden_size
        T0s = []
        for e, mn in zip(embs, max_new):
            if e.dim() != 2 or e.shape[1] != H or e.dtype != torch.float16 or not e.is_cuda:
                raise ValueError("inputs_embeds must be fp16 device tensors [T, hidden]")
            if not 0 < mn <= self.cap:
                raise ValueError(f"max_new_tokens {mn} outside (0, {self.cap}] (engine capacity)")
            T0 = int(e.shape[0])
            if T0 < 1 or T0 + mn > self.T_max:
                raise ValueError(f"prompt {T0} + max_new_tokens {mn} exceeds the KV cache ({self.T_max} positions)")
            T0s.append(T0)
        # which kernels compute the prompt decides its bits: one sequence of at most one chunk, or prompt_path "chunks",
        # goes through the token kernels 16 rows at a time; everything else (every batch) takes the MFMA pass
        chunks = width == 1 and (T0s[0] <= CHUNK or self.prompt_path == "chunks")
        dev = self.dev
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=dev)
        st = self._stream
        st.wait_stream(torch.cuda.current_stream(dev))
        graph, steps = False, 0
        rows = [[0, 0, 1, 0, 0, 0, 0, 0] for _ in range(S)]      # unused slots: finished
        for i, s in enumerate(slots):     # cache length: the chunk lists advance it, the MFMA pass leaves it to us (its pick adds 0)
            rows[s] = [0 if chunks else T0s[i], 0, 0, last[i], max_new[i], eos[i], 0, 0]
        with torch.cuda.stream(st):
            self.state.copy_(torch.tensor(rows, dtype=torch.int32), non_blocking=False)
            if chunks:
                for r0 in range(0, T0s[0], CHUNK):
                    m = min(CHUNK, T0s[0] - r0)
                    self.h[:m].copy_(embs[0][r0:r0 + m])
                    self._plan(m, "last" if r0 + m == T0s[0] else "chunk").run(st.cuda_stream)
            else:
                self._prompt_mfma(embs, slots, width)
            tok = self._plan(width, "token")
            done, most = False, max(max_new) - 1
            ff = self.chain_fast_forward and self.n_chain > 1
            ff_rows, ff_passes = {s: 0 for s in slots}, 0
            state = self.state.cpu() if ff else None      # fast-forward: the prompt pass's pick may already have paused a slot
            while True:
                if ff:      # paused slots (flag 2) go through one pass; what is left follows from the rows the host now holds
                    ff_passes += self._fast_forward(state, slots, ff_rows)
                    done = bool(state[:, 2].all())
                    left = max([int(state[s, 4] - state[s, 1]) for s in slots if not int(state[s, 2])], default=0)
                else:
                    left = most - steps
                if done or left <= 0:
                    break
                burst = min(self.poll_every, left)
                for _ in range(burst):
                    if self.use_graph and not tok.captured:
                        tok.run(st.cuda_stream)       # first step eager, then capture the launch list once
                        tok.capture(st.cuda_stream)
                    elif self.use_graph:
                        tok.replay(st.cuda_stream)
                        graph = True
                    else:
                        tok.run(st.cuda_stream)
                steps += burst
                # the only host<->device sync of the loop (every `poll_every` steps): every slot's flag in one copy
                state = self.state.cpu()
                done = bool(state[:, 2].all())
            state = self.state.cpu()
            out = []
            for s in slots:
                k = int(state[s, 1])
                out.append({"ids": self.out_ids[s, :k].to(torch.int64), "hidden": self.feats[s, :max(k - 1, 0)].clone()})
        torch.cuda.current_stream(dev).wait_stream(st)
        self.last_run_info = {"graph": graph, "sequences": len(embs), "prompt_tokens": T0s, "new_tokens": [len(o["ids"]) for o in out],
                              "token_steps_launched": steps, "ops_per_token": tok.n, "kv_dtype": self.kv_dtype,
                              "fast_forward_rows": [ff_rows[s] for s in slots], "fast_forward_passes": ff_passes}
        return out

    def _fast_forward(self, state: Tensor, slots: List[int], ff_rows: Dict[int, int]) -> int:
        """Chain fast-forward: every slot the pick kernel paused (flag 2 in `state`, the host copy of the state block) has a
        current token inside the image-token chain, so its next ids are `forced_run`'s.  One pass over the concatenated rows
        of all paused slots - slot s: the embeddings of [cur] + f[:-1] at positions len .. len + m - 1 - through
        `_layers_mfma` with one ragged attention launch per layer; the final norm of row r is the fed-back hidden state of id
        n_out - 1 + r; then f goes into out_ids and the slot's state row is rewritten (length + m, count + m, current token
        f[-1], finished if f[-1] is the eos or the count reached max_new).  No lm_head, no pick.  The other slots' rows are
        not touched; `state` is updated in place.  Returns the number of passes run (0 or 1)."""
        segs = []                                               # (slot, ids fed, ids out)
        for s in slots:
            if int(state[s, 2]) != 2:
                continue
            ln, n_out, _, cur, mx, eos = (int(v) for v in state[s, :6])
            f = forced_run(self._chain_ids, cur, n_out, mx, eos)
            assert f and ln + len(f) <= self.T_max and n_out + len(f) <= self.cap, (s, ln, n_out, len(f))
            segs.append((s, [cur] + f[:-1], f))
        if not segs:
            return 0
        dev, eps = self.dev, self.cfg.rms_norm_eps
        fed = torch.tensor([t for _, ids, _ in segs for t in ids], dtype=torch.long).to(dev)
        table = torch.tensor([[s, r] for s, ids, _ in segs for r in range(len(ids))], dtype=torch.int32).to(dev)
        starts = [0]
        for _, ids, _ in segs:
            starts.append(starts[-1] + len(ids))
        h = self._layers_mfma(self.embed.index_select(0, fed), [s for s, _, _ in segs], starts, table)
        for (s, _, f), a in zip(segs, starts):
            m, n_out = len(f), int(state[s, 1])
            ops.llm_rmsnorm(h[a:a + m], self.norm_g, eps, out=self.feats[s, n_out - 1:n_out - 1 + m])
            self.out_ids[s, n_out:n_out + m].copy_(torch.tensor(f, dtype=torch.int32))
            state[s, 0] += m
            state[s, 1] += m
            state[s, 3] = f[-1]
            state[s, 2] = int(f[-1] == int(state[s, 5]) or n_out + m >= int(state[s, 4]))
            self.state[s].copy_(state[s])
            ff_rows[s] += m
        return 1

    def _w(self, ws: list, ss: list, l: int, es: Sequence[Tensor] = ()) -> Tensor:
        """The fp16 matrix a prompt-pass GEMM reads: the weight itself, or - int8 / mxfp4 - its dequantised copy in the one
        reusable scratch (sized for the largest group, gate|up; stream order keeps the previous user ahead of the rewrite)."""
        if self.weight_dtype == "float16":
            return ws[l]
        if self._w16 is None:
            per = 2 if self.weight_dtype == "mxfp4" else 1          # weights per stored byte
            n = max(per * w.numel() for group in (self.wqkv, self.wo, self.wgu, self.wdown) for w in group[:1])
            self._w16 = torch.empty(n, dtype=torch.float16, device=self.dev)
        if self.weight_dtype == "int8":
            return ops.llm_dequant_w8(ws[l], ss[l], out=self._w16)
        return ops.llm_dequant_fp4(ws[l], es[l], ss[l], out=self._w16)

    def _prompt_mfma(self, embs: List[Tensor], slots: List[int], width: int) -> None:
        """The prompts of n >= 1 sequences in one pass per layer over their concatenated rows: the projections are
        [rows,K] x [N,K]^T MFMA GEMMs (weights streamed once per layer for the whole batch instead of once per 16-row
        chunk); only the attention walks each sequence's rows in chunks of 16 (causal inside a chunk, cache rows before
        it) into that sequence's slot.  Ends like the chunked path, per slot: final norm of each sequence's last row,
        lm_head (`llm_gemv` at width 1, `llm_gemm16_kernel` over all S rows otherwise) and the first pick."""
        eps = self.cfg.rms_norm_eps
        h = torch.cat([e.contiguous() for e in embs], 0) if width > 1 else embs[0].contiguous().clone()
        starts = [0]
        for e in embs:
            starts.append(starts[-1] + int(e.shape[0]))
        h = self._layers_mfma(h, slots, starts)
        if width == 1:
            last_rows = h[-1:]
        else:                                                                # row s = the last prompt row of the sequence in slot s
            idx = torch.tensor([starts[i + 1] - 1 for i in range(len(embs))], dtype=torch.long, device=self.dev)
            self.h.zero_()
            self.h[torch.tensor(slots, dtype=torch.long, device=self.dev)] = h.index_select(0, idx)
            last_rows = self.h[:width]
        ops.llm_rmsnorm(last_rows, self.norm_g, eps, out=self.hn[:width])
        (ops.llm_gemv if width == 1 else ops.llm_gemm16)(self.hn[:width], self.lm_head, out=self.logits[:width])
        ops.llm_select_slots(self.logits[:width], self.chain if self.n_chain else None, 0, self.state[:width],
                             self.out_ids[:width], pause=self.chain_fast_forward)

    def _layers_mfma(self, h: Tensor, slots: List[int], starts: List[int], table: Optional[Tensor] = None) -> Tensor:
        """Every decoder layer over known-token rows: h [rows, hidden], rows starts[i] .. starts[i + 1] - 1 are consecutive
        positions of the sequence in slots[i].  RMSNorm, the MFMA GEMMs (int8 / mxfp4: from the dequantised scratch), attention,
        o-proj, SwiGLU, down-proj; returns the last layer's residual stream.  Where a sequence's rows start decides the
        attention: `table` None - the prompt pass, every sequence at position 0 - walks each sequence in chunks of 16 with the
        one-sequence kernel and a cursor of its own; with `table` (int32 [rows][2] = (slot, row of the segment), the
        fast-forward pass) sequence i starts at the length in its state row, state[slots[i]][0], and all rows of all
        sequences are one launch of `llm_attn_rows_kernel`."""
        c = self.cfg
        Hq, Hkv, eps = c.num_attention_heads, c.kv_heads, c.rms_norm_eps
        scale = 1.0 / math.sqrt(c.head_dim)
        pf = self.state_pf
        kv8 = self.kv_dtype == "fp8"
        att = torch.empty((starts[-1], Hq * c.head_dim), dtype=torch.float16, device=self.dev)
        for l in range(c.num_hidden_layers):
            xn = ops.llm_rmsnorm(h, self.g_in[l], eps)                       # LlamaRMSNorm incl. its gain, then the plain GEMM
            qkv = ops.gemm(xn, self._w(self.wqkv, self.sqkv, l, self.eqkv))
            if table is not None:
                ops.llm_attention_rows(qkv, self.kcs[l], self.vcs[l], self.rope_cos, self.rope_sin, self.state, table, Hq, Hkv,
                                       scale, out=att, k_exp=self.kes[l] if kv8 else None, v_exp=self.ves[l] if kv8 else None)
            for i, s in enumerate(slots if table is None else ()):
                pf.zero_()                                                   # chunk cursor of this slot's cache
                for r0 in range(starts[i], starts[i + 1], CHUNK):
                    m = min(CHUNK, starts[i + 1] - r0)
                    if kv8:
                        ops.llm_attention_kv8(qkv[r0:r0 + m], self.kcs[l][s], self.vcs[l][s], self.kes[l][s], self.ves[l][s],
                                              self.rope_cos, self.rope_sin, pf, Hq, Hkv, scale, out=att[r0:r0 + m])
                    else:
                        ops.llm_attention(qkv[r0:r0 + m], self.kcs[l][s], self.vcs[l][s], self.rope_cos, self.rope_sin, pf,
                                          Hq, Hkv, scale, out=att[r0:r0 + m])
                    ops.llm_advance(pf, m)
            h = ops.gemm(att, self._w(self.wo, self.so, l, self.eo), residual=h)
            xn = ops.llm_rmsnorm(h, self.g_post[l], eps)
            act = ops.llm_swiglu(ops.gemm(xn, self._w(self.wgu, self.sgu, l, self.egu)))
            h = ops.gemm(act, self._w(self.wdown, self.sdown, l, self.edown), residual=h)
        return h

    def embed_tokens(self, input_ids: Tensor) -> Tensor:
        """Row gather from the embedding table (data movement only)."""
        return self.embed.index_select(0, input_ids.to(self.dev).view(-1).long())


def sincos_pos_embed_2d(embed_dim: int, grid_size: int) -> Tensor:
    """The fixed 2-D sin/cos table `QwenResampler.pos_embed` is initialised with (qwen_resampler.py:37-86): first half
    of the channels encodes the column index, second half the row index, each as [sin | cos] over 10000^(-2i/d)."""
    def one(dim, pos):
        omega = 1.0 / 10000 ** (torch.arange(dim // 2, dtype=torch.float32) / (dim / 2.0))
        out = pos.reshape(-1)[:, None] * omega[None]
        return torch.cat([out.sin(), out.cos()], 1)
    r = torch.arange(grid_size, dtype=torch.float32)
    gh, gw = torch.meshgrid(r, r, indexing="ij")
    return torch.cat([one(embed_dim // 2, gw), one(embed_dim // 2, gh)], 1)


def random_qwen_resampler_state_dict(grid_size: int, embed_dim: int, kv_dim: int, device, seed: int = 0) -> Dict[str, Tensor]:
    """Seeded weights with the reference module's key names (benchmarks / tests; no checkpoints exist offline)."""
    g = torch.Generator(device=device).manual_seed(seed)
    E, Q = embed_dim, grid_size ** 2
    R = lambda *s, std=0.02: torch.randn(*s, generator=g, device=device) * std
    return {"pos_embed": sincos_pos_embed_2d(E, grid_size).to(device), "query": R(Q, E),
            "kv_proj.weight": R(E, kv_dim, std=1.0 / math.sqrt(kv_dim)),
            "attn.in_proj_weight": R(3 * E, E, std=1.0 / math.sqrt(E)), "attn.in_proj_bias": R(3 * E),
            "attn.out_proj.weight": R(E, E, std=1.0 / math.sqrt(E)), "attn.out_proj.bias": R(E),
            "ln_q.weight": 1.0 + R(E), "ln_q.bias": R(E), "ln_kv.weight": 1.0 + R(E), "ln_kv.bias": R(E)}


class QwenResampler:
    """Single cross-attention resampler (reference src/models/qwen_resampler.py:87-145) on the HIP ops.
    Weight-only terms are folded at construction: q = (ln_q(query)+pos) Wq^T + bq is a constant, and the position
    embedding enters the keys as a per-token additive term pos Wk^T + bk."""

    def __init__(self, sd: Dict[str, Tensor], num_heads: int, device):
        _lib.load()
        dev = torch.device(device)
        f32 = lambda k: sd[k].detach().to(dev).float()
        self.dev, self.heads = dev, int(num_heads)
        query, pos = f32("query"), f32("pos_embed")
        self.num_queries, E = query.shape
        self.embed_dim = E
        wi, bi = f32("attn.in_proj_weight"), f32("attn.in_proj_bias")
        q = torch.nn.functional.layer_norm(query, (E,), f32("ln_q.weight"), f32("ln_q.bias")) + pos
        half = lambda t: t.to(torch.float16).contiguous()
        self.q = half(q @ wi[:E].T + bi[:E])[None]                                   # [1,Q,E]
        self.kv_proj = half(f32("kv_proj.weight")) if "kv_proj.weight" in sd else None
        self.ln_g, self.ln_b = half(f32("ln_kv.weight")), half(f32("ln_kv.bias"))
        self.w_kv = half(wi[E:])                                                     # [2E,E]: k rows then v rows
        self.pos = pos
        self._wk, self._bk, self._bv = wi[E:2 * E], bi[E:2 * E], bi[2 * E:]
        self._add: Dict[int, Tensor] = {}
        self.w_out, self.b_out = half(f32("attn.out_proj.weight")), half(f32("attn.out_proj.bias"))

    def weights_changed(self) -> None:
        """Drop the per-length key addends derived from the (rewritten) weights."""
        self._add.clear()

    def tensors(self) -> List[Tensor]:
        """Frozen (folded) weights (the multi-GPU weight broadcast list); the per-length key addends are derived."""
        self._add.clear()
        return [t for t in (self.q, self.kv_proj, self.ln_g, self.ln_b, self.w_kv, self.pos, self._wk, self._bk, self._bv,
                            self.w_out, self.b_out) if t is not None]

    def _kv_addend(self, L: int) -> Tensor:
        """[L,2E] = [pos Wk^T + bk | bv] (pos interpolated like get_abs_pos when L differs from the query grid)."""
        a = self._add.get(L)
        if a is None:
            pos = self.pos
            if L != pos.shape[0]:
                s, t = int(math.sqrt(pos.shape[0])), int(math.sqrt(L))
                pos = torch.nn.functional.interpolate(pos.reshape(1, s, s, -1).permute(0, 3, 1, 2), size=(t, t),
                                                      mode="bicubic", align_corners=False)
                pos = pos.permute(0, 2, 3, 1).flatten(0, 2)
            a = torch.cat([pos @ self._wk.T + self._bk, self._bv[None].expand(pos.shape[0], -1)], 1)
            a = a.to(torch.float16).contiguous()
            self._add[L] = a
        return a

    @torch.no_grad()
    def __call__(self, x: Tensor) -> Tensor:
        """x: [B, L, kv_dim] -> [B, num_queries, embed_dim] (fp16)."""
        B, L, _ = x.shape
        E = self.embed_dim
        x = x.to(device=self.dev, dtype=torch.float16).reshape(B * L, -1).contiguous()
        if self.kv_proj is not None:
            x = ops.gemm(x, self.kv_proj)
        x = ops.layernorm(x, self.ln_g, self.ln_b, 1e-5)
        add = self._kv_addend(L)
        kv = ops.gemm(x, self.w_kv, residual=add if B == 1 else add.repeat(B, 1)).view(B, L, 2 * E)
        q = self.q if B == 1 else self.q.expand(B, -1, -1).contiguous()
        o = ops.small_attention(q, kv[:, :, :E], kv[:, :, E:], self.heads, 1.0 / math.sqrt(E // self.heads))
        return ops.gemm(o.view(B * self.num_queries, E), self.w_out, bias=self.b_out).view(B, self.num_queries, E)


BOI_TOKEN, EOI_TOKEN, IMG_TOKEN = "<img>", "</img>", "<img_{:05d}>"


def image_token_ids(tokenizer, num_img_gen_tokens: int, img_ids_list: Optional[Sequence[int]] = None):
    """(processor chain, </img> id, the `num_img_gen_tokens` <img_xxxxx> ids) the way the reference derives them.

    The LLaMA sentencepiece tokenizer prepends a '▁' id to whatever it encodes; the reference therefore takes
    `encode(EOI_TOKEN)[1]` and `encode(img tokens)[1:]` (seed_x.py:139-141, gradio.py:44-45) but keeps the FULL encoded
    list, prefix included, as the logits processor's chain (generation.py:15-17).  Same here: the chain is the list as
    encoded; </img> is its last id and the image ids are the `num_img_gen_tokens` ids before it, so a list with or
    without the prefix gives the same answer."""
    if img_ids_list is None:
        if tokenizer is None:
            raise ValueError("pass a tokenizer or `img_ids_list`")
        s = BOI_TOKEN + "".join(IMG_TOKEN.format(i) for i in range(num_img_gen_tokens)) + EOI_TOKEN
        img_ids_list = tokenizer.encode(s, add_special_tokens=False)
    chain = [int(v) for v in img_ids_list]
    if len(chain) < num_img_gen_tokens + 2:
        raise ValueError(f"image-token chain has {len(chain)} ids; needs <img> + {num_img_gen_tokens} image ids + </img>")
    return chain, chain[-1], chain[-(num_img_gen_tokens + 1):-1]


class ContinuousLVLM:
    """`ContinuousLVLM.generate` of the reference (seed_x.py:90-171) over the decode engine.

    `tokenizer` is only used the way the reference uses it: to turn the image-token strings into ids and to decode the
    result; callers without tokenizer files pass `img_ids_list=[<img>, <img_00000>.., </img>]` instead."""

    def __init__(self, llm: LlamaDecodeEngine, input_resampler: QwenResampler, output_resampler: QwenResampler):
        self.llm, self.input_resampler, self.output_resampler = llm, input_resampler, output_resampler

    def dtype(self):
        return torch.float16

    def tensors(self) -> List[Tensor]:
        """Frozen weights of the whole agent: LLaMA decode engine + both QwenResamplers (multi-GPU broadcast list)."""
        return self.llm.tensors() + self.input_resampler.tensors() + self.output_resampler.tensors()

    def weights_changed(self) -> None:
        self.llm.weights_changed()
        self.input_resampler.weights_changed()
        self.output_resampler.weights_changed()

    def _prepare(self, tokenizer=None, prompt=None, input_ids=None, image_embeds=None, ids_cmp_mask=None,
                 logits_processor=None, num_img_gen_tokens=64, temperature=0.7, num_beams=1, max_new_tokens=120,
                 top_p=0.5, img_ids_list: Optional[Sequence[int]] = None, eos_token_id: Optional[int] = None) -> dict:
        """Argument handling of `generate` up to the token ids (no device work)."""
        if logits_processor is not None:
            raise NotImplementedError("the image-token processor is built into the pick kernel; custom processors "
                                      "have no device implementation")
        if num_beams != 1:
            raise NotImplementedError("the reference decodes greedily (num_beams=1, do_sample=False)")
        img_ids_list, eoi_token_id, image_gen_id_list = image_token_ids(tokenizer, num_img_gen_tokens, img_ids_list)
        if eos_token_id is None:
            eos_token_id = getattr(tokenizer, "eos_token_id", None)
            if eos_token_id is None:
                raise ValueError("pass `eos_token_id` (or a tokenizer that has one)")
        if prompt is not None:
            input_ids = tokenizer(prompt, return_tensors="pt").input_ids
        if isinstance(input_ids, list):
            input_ids = torch.tensor(input_ids)
        if image_embeds is not None:
            assert ids_cmp_mask is not None
        return {"tokenizer": tokenizer, "ids": input_ids.view(-1), "image_embeds": image_embeds, "ids_cmp_mask": ids_cmp_mask,
                "chain": img_ids_list, "eoi": eoi_token_id, "gen_ids": image_gen_id_list, "eos": int(eos_token_id),
                "max_new": int(max_new_tokens), "n_img": int(num_img_gen_tokens)}

    @staticmethod
    def _image_blocks(q: dict, g: dict):
        """`generate`'s bookkeeping after decoding: ids with the image blocks rewritten, their mask, the hidden-state
        block of every complete <img> .. </img> run (seed_x.py:139-160)."""
        generate_ids, last_hidden_states = g["ids"].clone(), g["hidden"]
        n_img = q["n_img"]
        image_gen_ids = torch.tensor(q["gen_ids"], dtype=generate_ids.dtype, device=generate_ids.device)
        eoi_indices = torch.where(generate_ids == q["eoi"])[0].tolist()
        ids_gen_mask = torch.zeros_like(generate_ids, dtype=torch.bool)
        feats = []
        for e in eoi_indices:
            if e >= n_img:
                feats.append(last_hidden_states[e - n_img:e])
                generate_ids[e - n_img:e] = image_gen_ids
                ids_gen_mask[e - n_img:e] = True
        return generate_ids, ids_gen_mask, len(eoi_indices), feats

    @torch.no_grad()
    def generate(self, tokenizer=None, prompt=None, input_ids=None, image_embeds=None, ids_cmp_mask=None,
                 logits_processor=None, num_img_gen_tokens=64, temperature=0.7, num_beams=1, max_new_tokens=120,
                 top_p=0.5, img_ids_list: Optional[Sequence[int]] = None, eos_token_id: Optional[int] = None) -> dict:
        q = self._prepare(tokenizer, prompt, input_ids, image_embeds, ids_cmp_mask, logits_processor, num_img_gen_tokens,
                          temperature, num_beams, max_new_tokens, top_p, img_ids_list, eos_token_id)
        return self._generate([q], batch=False)[0]

    @torch.no_grad()
    def generate_batch(self, requests: Sequence[dict]) -> List[dict]:
        """`generate` for up to `llm.max_sequences` requests (each the keyword arguments of `generate`) in one decode
        loop: the input resampler runs once over the stacked `image_embeds`, the decoder once over all sequences, the
        output resampler once over all image blocks.  All requests must share `img_ids_list` (the processor chain is one
        per launch plan) and `num_img_gen_tokens`."""
        qs = [self._prepare(**r) for r in requests]
        return self._generate(qs, batch=True) if qs else []

    def _generate(self, qs: List[dict], batch: bool) -> List[dict]:
        """Both entries: input resampler, image-token chain, decode, image blocks, output resampler, result dicts.
        batch: the sequences go through `llm.generate_batch`; otherwise `qs` is one request for `llm.generate`."""
        if any(q["chain"] != qs[0]["chain"] or q["n_img"] != qs[0]["n_img"] for q in qs):
            raise ValueError("generate_batch: all requests must share img_ids_list and num_img_gen_tokens")
        llm = self.llm
        embs = [llm.embed_tokens(q["ids"]) for q in qs]
        with_img = [i for i, q in enumerate(qs) if q["image_embeds"] is not None]
        imgs = [qs[i]["image_embeds"] for i in with_img]
        if len(imgs) > 1 and len({tuple(t.shape[1:]) for t in imgs}) == 1:
            lm = self.input_resampler(torch.cat([t.to(llm.dev) for t in imgs], 0))
            parts = lm.split([int(t.shape[0]) for t in imgs], 0)
        else:                                      # one request, or different token grids: the position table is per length
            parts = [self.input_resampler(t) for t in imgs]
        for i, part in zip(with_img, parts):
            emb = embs[i]
            emb[qs[i]["ids_cmp_mask"].view(-1).to(emb.device)] = part.reshape(-1, emb.shape[-1])
        llm.set_image_token_chain(qs[0]["chain"])
        last, eos, max_new = [int(q["ids"][-1]) for q in qs], [q["eos"] for q in qs], [q["max_new"] for q in qs]
        gs = llm.generate_batch(embs, last, eos, max_new) if batch else [llm.generate(embs[0], last[0], eos[0], max_new[0])]
        blocks = [self._image_blocks(q, g) for q, g in zip(qs, gs)]
        all_feats = [f for b in blocks for f in b[3]]
        res = self.output_resampler(torch.stack(all_feats)).contiguous() if all_feats else None
        outs, at = [], 0
        for q, (generate_ids, ids_gen_mask, num_gen_imgs, feats) in zip(qs, blocks):
            img_gen_feat = None
            if num_gen_imgs > 0:
                if not feats:
                    raise RuntimeError("</img> was generated without a whole image block in front of it")
                img_gen_feat = res[at:at + len(feats)].contiguous()
                at += len(feats)
            tok = q["tokenizer"]
            text = tok.decode(generate_ids, skip_special_tokens=True) if tok is not None else None
            outs.append({"text": text, "output_ids": generate_ids, "img_gen_feat": img_gen_feat,
                         "num_gen_imgs": num_gen_imgs, "ids_gen_mask": ids_gen_mask})
        return outs


def _prepass(pipeline, agent: ContinuousLVLM, requests: Sequence[dict], batch: bool, tokenizer, img_ids_list, eos_token_id,
             max_new_tokens) -> List[Tensor]:
    """reference scripts/demo/gradio.py:85-109 for every request (`input_ids`, `ids_cmp_mask`, `ip_images`, `mllm_scale`):
    character tokens -> MLLM -> blended `ip_image_embeds`.  batch: one decode loop for all (`agent.generate_batch`)."""
    cfg = pipeline.unet.config
    nv, n_ip = cfg.num_vision_tokens, cfg.max_num_ips
    image_embeds = [pipeline.encode_ip_tokens(r["ip_images"])[:, nv:, :] for r in requests]      # each [1, n_ip*nv, dim]
    kws = [dict(tokenizer=tokenizer, input_ids=r["input_ids"].unsqueeze(0), image_embeds=e,
                ids_cmp_mask=r["ids_cmp_mask"].unsqueeze(0), max_new_tokens=max_new_tokens,
                num_img_gen_tokens=agent.output_resampler.num_queries, img_ids_list=img_ids_list, eos_token_id=eos_token_id)
           for r, e in zip(requests, image_embeds)]
    outs = agent.generate_batch(kws) if batch else [agent.generate(**kw) for kw in kws]
    blended = []
    for r, e, out in zip(requests, image_embeds, outs):
        if out["img_gen_feat"] is None:
            raise RuntimeError("the MLLM produced no image block")
        gen = out["img_gen_feat"].view(n_ip, nv, -1)
        blended.append(ops.blend(gen, e.reshape(n_ip, nv, -1).to(gen.dtype), float(r["mllm_scale"])))
    return blended


@torch.no_grad()
def mllm_prepass(pipeline, agent: ContinuousLVLM, input_ids: Tensor, ids_cmp_mask: Tensor, ip_images: list,
                 mllm_scale: float, tokenizer=None, img_ids_list: Optional[Sequence[int]] = None,
                 eos_token_id: Optional[int] = None, max_new_tokens: int = 500) -> Tensor:
    """reference scripts/demo/gradio.py:85-109: character tokens -> MLLM -> blended `ip_image_embeds`
    [max_num_ips, num_vision_tokens, dim] to pass to `pipeline(ip_images=[], ip_image_embeds=...)`."""
    request = dict(input_ids=input_ids, ids_cmp_mask=ids_cmp_mask, ip_images=ip_images, mllm_scale=mllm_scale)
    return _prepass(pipeline, agent, [request], False, tokenizer, img_ids_list, eos_token_id, max_new_tokens)[0]


@torch.no_grad()
def mllm_prepass_batch(pipeline, agent: ContinuousLVLM, requests: Sequence[dict], tokenizer=None,
                       img_ids_list: Optional[Sequence[int]] = None, eos_token_id: Optional[int] = None,
                       max_new_tokens: int = 500) -> List[Tensor]:
    """`mllm_prepass` for up to `agent.llm.max_sequences` requests in one decode loop.  Each request is a dict with
    `input_ids`, `ids_cmp_mask`, `ip_images` and `mllm_scale`; returns one blended `ip_image_embeds` per request."""
    return _prepass(pipeline, agent, requests, True, tokenizer, img_ids_list, eos_token_id, max_new_tokens)
