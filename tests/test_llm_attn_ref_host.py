"""CPU: the attention reference of tests/_llm_attn_ref.py is exact enough, and its planted inputs are sharp enough, for
the gates of tests/test_gpu_llm_long_context.py - shown on the reference alone, no wrong kernel is ever run.

For every (D, heads, kv_heads, pos0, M) the GPU file compares:
  (a) the fp32 reference agrees with the same code in fp64 to 1e-4 of max|ref|, 40x below the 4e-3 gate (what is left
      is an fp16 rounding of a key or a probability that falls the other way in fp32: one ulp of one term of thousands);
  (b) with any single key of the boundary set removed from the softmax, every row that sees this key moves by at least
      10 x 4e-3 of max|ref| - the normalisation of the GPU test - so a kernel that loses one of these keys cannot pass.
"""
import pytest
import torch

from tests import _llm_attn_ref as A

GPU_TOL = 4e-3          # the per-op bound of the MLLM kernel tests (tests/test_gpu_mllm.py)
CASES = A.all_cases()


@pytest.mark.parametrize("D,heads,kv_heads,seam,pos0,launches", CASES,
                         ids=[f"D{c[0]}-h{c[1]}kv{c[2]}-pos{c[4]}-M{sum(c[5])}" for c in CASES])
def test_reference_is_exact_and_every_boundary_key_counts(D, heads, kv_heads, seam, pos0, launches):
    M = sum(launches)
    T = pos0 + M
    qkv = A.planted_qkv(D, heads, kv_heads, T, seam, A.case_seed(D, heads, kv_heads, pos0, M))
    ref32, kr32 = A.attention_ref(qkv, D, heads, kv_heads, pos0, M)
    ref64, kr64 = A.attention_ref(qkv, D, heads, kv_heads, pos0, M, dtype=torch.float64)
    assert A.rel_err(kr32, kr64) <= 2.0 ** -10, "rotated keys differ by more than one fp16 ulp"
    keys = A.boundary_keys(D, T, seam)
    assert T == 1 or len(keys) >= 2
    dropped = {j: A.attention_ref(qkv, D, heads, kv_heads, pos0, M, dtype=torch.float64, drop=j)[0]
               for j in keys if T > 1}             # T == 1: the only key, nothing is left to attend to without it
    worst_a, worst_b, r0 = 0.0, float("inf"), 0
    for m in launches:                              # each launch is one comparison with its own max|ref|
        sl = slice(r0, r0 + m)
        den = ref64[sl].abs().max().item()
        a = A.rel_err(ref32[sl], ref64[sl])
        worst_a = max(worst_a, a)
        assert a <= 1e-4, f"rows {r0}..{r0 + m - 1}: the fp32 reference is {a:.3g} of max|ref| away from fp64"
        for j, out in dropped.items():
            rows = [r for r in range(r0, r0 + m) if pos0 + r >= max(j, 1)]       # rows that see key j and another one
            if not rows:
                continue
            move = (out[rows] - ref64[rows]).abs().max(1).values / den
            worst_b = min(worst_b, move.min().item())
            assert move.min().item() >= 10 * GPU_TOL, f"dropping key {j} moves row {rows[int(move.argmin())]} by " \
                                                       f"{move.min().item():.3g} of max|ref| only"
        r0 += m
    print(f"(a) fp32 vs fp64: {worst_a:.3g}   (b) smallest single-key effect: {worst_b:.3g} of max|ref| = "
          f"{worst_b / GPU_TOL:.1f} x the gate")
