"""GPU: the three MXFP4 entry points (ds_llm_gemv_fp4, ds_llm_gemm16_fp4, ds_llm_dequant_fp4) with poison around their operands.

The memory model is tests/_arena.py and the procedure is that of tests/test_gpu_poisoned_memory.py, whose case class and
test body are used as they are: every case runs on ordinary tensors, inside an arena filled with quiet NaN and inside one
filled with the "loud" patterns; the two poisoned results must be bit-equal to each other and to the plain run, finite, with
every guard and canary byte intact, and the plain run must meet the fp32 reference at the tolerances of
tests/test_gpu_llm_fp4.py.  The arena's uint8 fills make an over-read of an MXFP4 operand loud: 0xFF nibbles are -6, and an
exponent byte 0xFF is a scale of 2^128 (infinity or NaN after the conversion), 0x01 one of 2^-126.

Shapes: (520, 736) - 23 blocks, ragged last 4-column block and 16-column tile, a part-used 128-wide k-block - for the plain,
residual-in-place, rms and rms + gain epilogues, and (344, 512) for SwiGLU, both at M = 5 (the generic GEMV kernel and the
matrix-pipe kernel) and, for the GEMV entry, also at M = 1 (the pipelined token kernel, which stages x in LDS in its own order).

The cases are also appended to the case list of tests/test_gpu_poisoned_memory.py: its completeness test asks every entry of
`_lib.SIGNATURES` for a poisoned-memory case, and these are the cases of the three new entries."""
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

try:
    import test_gpu_poisoned_memory as P          # the module object pytest itself collects (tests/ is on sys.path)
except ImportError:                               # collected under another import mode
    from tests import test_gpu_poisoned_memory as P

NS = types.SimpleNamespace
N1, K1, N2, K2 = 520, 736, 344, 512


@functools.lru_cache(maxsize=None)
def _data():
    from diffsensei_amd.mllm import dequantize_rows_mxfp4, quantize_rows_mxfp4
    g = torch.Generator().manual_seed(N1 * 3 + K1)
    r = lambda shape, scale=1.0: (torch.randn(shape, generator=g) * scale).half()
    stag = lambda rows, K: (torch.pow(2.0, (torch.arange(rows) % 7 - 3).float())[:, None]
                            * torch.pow(2.0, -(torch.arange(K // 32) % 5).float()).repeat_interleave(32)[None, :])
    x, res, x2 = r((16, K1)), r((16, N1)), r((16, K2))
    gain = (1.0 + 0.3 * torch.randn(K1, generator=g)).half()
    q, e, s = quantize_rows_mxfp4(r((N1, K1), 1 / math.sqrt(K1)).float() * stag(N1, K1))
    wsw = r((2 * N2, K2), 2 / math.sqrt(K2) / 8).float() * stag(2 * N2, K2)
    wsw[N2:] *= 8.0
    qsw, esw, ssw = quantize_rows_mxfp4(wsw)
    wf, wswf = dequantize_rows_mxfp4(q, e, s), dequantize_rows_mxfp4(qsw, esw, ssw)
    xw = x.float() @ wf.T
    r5 = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    r6 = torch.rsqrt(x2.float().pow(2).mean(-1, keepdim=True) + 1e-6)
    xn = (gain.float() * (x.float() * r5).half().float()).half()
    ref = [xw, xw.half().float() + res.float(), xw * r5, xn.float() @ wf.T,
           F.silu((x2.float() @ wswf[:N2].T) * r6) * ((x2.float() @ wswf[N2:].T) * r6)]
    block = dequantize_rows_mxfp4(q, e, torch.ones(N1))
    return NS(x=x, x2=x2, res=res, gain=gain, q=q, e=e, s=s, qsw=qsw, esw=esw, ssw=ssw, ref=ref,
              deq=(block * s[:, None]).half())


def _run(kernel, M):
    def run(m, h):
        fn = m.ops.llm_gemv_fp4 if kernel == "gemv" else m.ops.llm_gemm16_fp4
        x, x2, gain = m.place(h.x[:M]), m.place(h.x2[:M]), m.place(h.gain)
        w = (m.place(h.q), m.place(h.e), m.place(h.s))
        wsw = (m.place(h.qsw), m.place(h.esw), m.place(h.ssw))
        y = m.place(h.res[:M])
        fn(x, *w, out=y, residual=y)                                                    # in place: h += x W^T
        return (fn(x, *w), y, fn(x, *w, rms=True, eps=1e-5), fn(x, *w, rms=True, eps=1e-5, gain=gain),
                fn(x2, *wsw, rms=True, swiglu=True, eps=1e-6))
    return run


def _check(M):
    def check(o, h):
        # tests/test_gpu_llm_fp4.py: 4e-3 plain, residual, rms; 1.5e-3 rms + gain; 6e-3 SwiGLU
        for got, ref, tol, what in zip(o, h.ref, (4e-3, 4e-3, 4e-3, 1.5e-3, 6e-3),
                                       ("plain", "residual in place", "rms", "rms + gain", "swiglu")):
            P._close_rel(got, ref[:M], tol, f"llm mxfp4 {what}")
    return check


FP4_CASES = [P.Case(f"llm-{kernel}-mxfp4-{M}x{N1}x{K1}+swiglu-{M}x{N2}x{K2}", [entry], _data, _run(kernel, M), _check(M))
             for kernel, entry, M in (("gemv", "ds_llm_gemv_fp4", 5), ("gemv", "ds_llm_gemv_fp4", 1),
                                      ("gemm16", "ds_llm_gemm16_fp4", 5))]
FP4_CASES.append(P.Case(f"llm-dequant-mxfp4-37x{K1}", ["ds_llm_dequant_fp4"], _data,
                        lambda m, h: (m.ops.llm_dequant_fp4(m.place(h.q[:37]), m.place(h.e[:37]), m.place(h.s[:37])),),
                        lambda o, h: torch.equal(o[0], h.deq[:37]) or pytest.fail("dequant is the host format, bit for bit")))
P.CASES.extend(FP4_CASES)     # on import, which pytest does for every test module before it runs a test (as test_gpu_panel_poisoned.py)


def test_the_fp4_entry_points_have_their_cases():
    """Host only: what tests/test_gpu_poisoned_memory.py::test_every_entry_point_has_a_case needs from this file (that test
    runs with every test module imported, tests/test_gpu_panel_poisoned.py's cases included)."""
    from diffsensei_amd._lib import SIGNATURES
    ours = {e for c in FP4_CASES for e in c.entry}
    assert ours == {"ds_llm_gemv_fp4", "ds_llm_gemm16_fp4", "ds_llm_dequant_fp4"} and ours <= set(SIGNATURES)
    assert all(any(c is k for k in P.CASES) for c in FP4_CASES) and len({c.id for c in P.CASES}) == len(P.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FP4_CASES, ids=lambda c: c.id)
def test_fp4_result_depends_on_nothing_but_the_operands(hip_lib, case):
    P.test_result_depends_on_nothing_but_the_operands(hip_lib, case)
