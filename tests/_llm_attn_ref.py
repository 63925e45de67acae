"""Reference and planted inputs for the MLLM decode attention (csrc/llm.hip: llm_attn_body), plain PyTorch on the CPU.

`causal_attention_ref` is the one statement of "rows pos0 .. pos0+M-1 attend causally to keys 0 .. pos0+r" that the GPU
tests of the long-context file compare with, at the rounding points of the reference model's fp16 attention:
rotate-half rotary (oracle.llama_ref.rope_tables / apply_rope), keys rounded to fp16 after the rotation (the cache holds
them so), probabilities rounded to fp16 before P.V.  `dtype=torch.float64` runs the same code in double; `drop=j` removes
key j from every softmax, which is how tests/test_llm_attn_ref_host.py shows that losing any one boundary key is visible.

`planted_qkv` builds the fused q|k|v rows: q is scaled by 0.25, so the scores are flat and no key is negligible; k, v are
N(0,1) in fp16; every key index of the boundary set gets +64 on one channel of v that belongs to that index alone, so a
kernel that skips, doubles or misplaces that key moves one output channel by 64 p_j.
"""
import math

import torch

from oracle import llama_ref as R

ATT_WAVES = 16                      # wavefronts of llm_attn_kernel; one key group per wavefront and loop iteration
SOFTMAX_STRIDE = 64 * ATT_WAVES     # keys per iteration of the kernel's exp / sum loop


def kpw(D: int) -> int:
    """keys per wavefront and iteration: a wavefront reads 64 / (D/8) whole key rows."""
    return 64 // (D // 8)


def boundary_keys(D: int, T: int, pos0: int) -> list:
    """first / last key of a wavefront's group, first key of the second key-loop iteration, both sides of the softmax
    loop's stride, both sides of the cache / in-chunk seam, the newest key - clipped to [0, T)."""
    K = kpw(D)
    cand = [0, K - 1, K, ATT_WAVES * K - 1, ATT_WAVES * K, SOFTMAX_STRIDE - 1, SOFTMAX_STRIDE, pos0 - 1, pos0, T - 2, T - 1]
    return sorted({j for j in cand if 0 <= j < T})


def planted_qkv(D: int, heads: int, kv_heads: int, T: int, pos0: int, seed: int) -> torch.Tensor:
    """fp16 [T, (heads + 2 kv_heads) D] rows q | k | v (un-rotated), marks planted in v as described above."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(T, heads * D, generator=g) * 0.25).half()
    k = torch.randn(T, kv_heads * D, generator=g).half()
    v = torch.randn(T, kv_heads, D, generator=g)
    for i, j in enumerate(boundary_keys(D, T, pos0)):
        v[j, :, (7 * i + 3) % D] += 64.0
    return torch.cat([q, k, v.half().view(T, kv_heads * D)], 1)


def split_qkv(qkv: torch.Tensor, D: int, heads: int, kv_heads: int):
    T = qkv.shape[0]
    q = qkv[:, :heads * D].view(T, heads, D)
    k = qkv[:, heads * D:(heads + kv_heads) * D].view(T, kv_heads, D)
    v = qkv[:, (heads + kv_heads) * D:].view(T, kv_heads, D)
    return q, k, v


def causal_attention_ref(q, k, v, pos0: int, dtype=torch.float32, drop=None, theta: float = 10000.0):
    """q [M, heads, D]: the rows at positions pos0 .. pos0+M-1; k, v [T >= pos0+M, kv_heads, D]: rows 0 .. T-1 (all
    un-rotated).  Row r sees keys 0 .. pos0+r.  Returns (out [M, heads*D], rotated fp16 keys [T, kv_heads, D]), both in
    `dtype`."""
    M, Hh, D = q.shape
    T, Hkv, _ = k.shape
    assert T >= pos0 + M and Hh % Hkv == 0
    rep = Hh // Hkv
    cos, sin = R.rope_tables(D, T, theta)                                        # the fp32 table the kernel is given
    cos, sin = cos.to(dtype), sin.to(dtype)
    kr = R.apply_rope(k.to(dtype), cos, sin).half().to(dtype)                    # the cache holds fp16 rotated keys
    qr = R.apply_rope(q.to(dtype), cos[pos0:pos0 + M], sin[pos0:pos0 + M])
    s = torch.einsum("thd,shd->hts", qr, kr.repeat_interleave(rep, 1)) / math.sqrt(D)
    keep = torch.arange(T)[None, :] <= (pos0 + torch.arange(M))[:, None]
    if drop is not None:
        keep = keep & (torch.arange(T) != int(drop))[None, :]
    p = s.masked_fill(~keep[None], float("-inf")).softmax(-1).half().to(dtype)   # the reference casts P to fp16
    out = torch.einsum("hts,shd->thd", p, v.to(dtype).repeat_interleave(rep, 1)).reshape(M, Hh * D)
    return out, kr


def attention_ref(qkv, D: int, heads: int, kv_heads: int, pos0: int, M: int, dtype=torch.float32, drop=None):
    """`causal_attention_ref` on fused rows: qkv [>= pos0+M, (heads + 2 kv_heads) D]."""
    q, k, v = split_qkv(qkv[:pos0 + M], D, heads, kv_heads)
    return causal_attention_ref(q[pos0:], k, v, pos0, dtype, drop)


def rel_err(got, ref) -> float:
    """max |err| / max |ref|: the normalisation of the MLLM kernel tests."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (got.shape, ref.shape)
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)


# ---- the shapes of tests/test_gpu_llm_long_context.py; tests/test_llm_attn_ref_host.py holds each to (a) and (b) ----
CONFIGS = [(128, 3, 3), (128, 4, 2), (64, 4, 2), (64, 8, 1)]                       # (D, heads, kv_heads)


def one_sequence_cases(D: int) -> list:
    """(name, pos0, M, T_max) of the one-sequence kernel with a directly written cache."""
    G = ATT_WAVES * kpw(D)                                                       # keys per key-loop iteration
    cases = [(f"row at {p}", p, 1, 1100) for p in (G - 1, G, G + 1, SOFTMAX_STRIDE - 1, SOFTMAX_STRIDE)]
    cases += [("chunk over the key-loop boundary", G - 8, 16, 1100),
              ("chunk over the softmax-loop boundary", SOFTMAX_STRIDE - 8, 16, 1100),
              ("5 rows ending at T_max", 1100 - 5, 5, 1100)]
    if D == 128:
        cases.append(("chunk at the end of an 8192 cache", 8192 - 16, 16, 8192))
    return cases


def slot_lengths(D: int) -> list:
    G = ATT_WAVES * kpw(D)
    return [0, G - 1, G, 1030]


FILL_ROWS = (16,) * 18 + (12, 1, 1, 1)          # kernel-filled case: 300 prompt rows in chunks, then 3 tokens
GUARD = (32, 16, 40)                            # pos0, M, T_max: rows 8..15 would pass the end of the cache


def case_seed(D: int, heads: int, kv_heads: int, pos0: int, M: int) -> int:
    return ((D * 131 + heads) * 131 + kv_heads) * 8209 + pos0 * 17 + M


def all_cases() -> list:
    """(D, heads, kv_heads, seam, pos0, launches) of every attention comparison of the GPU file: inputs are planted for
    the seam `seam`; the launches take launches[0], launches[1], .. rows from position pos0 on, and the rows of each
    launch are one comparison, normalised by their own max|ref| (the kernel-filled case walks all rows from 0, its
    planted seam is the first single token)."""
    out = []
    for D, heads, kv in CONFIGS:
        out += [(D, heads, kv, p, p, (m,)) for _, p, m, _ in one_sequence_cases(D)]
        out += [(D, heads, kv, n, n, (1,)) for n in slot_lengths(D)]
        out.append((D, heads, kv, GUARD[0], GUARD[0], (GUARD[2] - GUARD[0],)))
        if D == 128:
            out.append((D, heads, kv, 300, 0, FILL_ROWS))
    return out
