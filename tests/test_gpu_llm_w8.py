"""GPU: the int8-weight (W8A16) forms of the MLLM decode kernels (csrc/llm.hip) - `llm_gemv_pipe_kernel` (M <= 4),
`llm_gemv_kernel` (generic), `llm_gemm16_kernel` (matrix pipe) and `llm_dequant_w8_kernel`.

Reference: fp32 torch from the same operands, x.float() @ (q.float() * s[:, None]).T.  The weights come from
`quantize_rows_int8` of random fp16 matrices whose row n was first multiplied by 2 ** (n % 7 - 3) (SwiGLU: the up rows by
a further 8), so a scale taken from the wrong row is off by a factor of two or more.  Tolerances are those of
test_gpu_llm_gemm16.py / test_gpu_mllm.py for the same epilogues - the rounding points are the same and the integer
weights make every product exact: 4e-3 of max|ref| for plain, residual in place and rms, 1.5e-3 for rms + gain, 6e-3
for SwiGLU.  Shapes: (520, 704) ragged last 4-column block / 16-column tile and K not a whole wave iteration; (520, 720)
an odd number of 16-weight groups (the two-MFMA-steps-per-load pairing has a half-used tail); (260, 5120) several full
iterations at the model's K; (768, 256) K shorter than one iteration; (4096, 13824) one real-width case, gemm16 only."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
NK = [(520, 704), (520, 720), (260, 5120), (768, 256)]


def _h(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).half()


def _close(got, ref, tol, what):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    den = max(ref.abs().max().item(), 1e-3)
    gate(what, err / den, tol)


def _quantised(rows, K, g, std, swiglu=False):
    """int8 weights + scales (device) and their fp32 dequantised form (host) of a random matrix with staggered row sizes"""
    from diffsensei_amd.mllm import dequantize_rows_int8, quantize_rows_int8
    w = _h((rows, K), g, std).float() * torch.pow(2.0, (torch.arange(rows) % 7 - 3).float())[:, None]
    if swiglu:
        w[rows // 2:] *= 8.0
    q, s = quantize_rows_int8(w)
    return q.to(DEV), s.to(DEV), dequantize_rows_int8(q, s)


@functools.lru_cache(maxsize=None)
def _case(N, K):
    """Operands for 16 rows and their fp32 references, made once per (N, K); a test with M rows uses the first M."""
    g = torch.Generator().manual_seed(N * 3 + K)
    x, res = _h((16, K), g), _h((16, N), g)
    q, s, wd = _quantised(N, K, g, 1 / math.sqrt(K))
    gain = (1.0 + 0.3 * torch.randn(K, generator=g)).half()
    xw = x.float() @ wd.T
    r = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    xn = (gain.float() * (x.float() * r).half().float()).half()
    return {"x": x.to(DEV), "res": res.to(DEV), "q": q, "s": s, "gain": gain.to(DEV), "plain": xw,
            "residual": xw.half().float() + res.float(), "rms": xw * r, "rms_gain": xn.float() @ wd.T}


@functools.lru_cache(maxsize=None)
def _swiglu_case(N, K):
    g = torch.Generator().manual_seed(N + K)
    x = _h((16, K), g)
    q, s, wd = _quantised(2 * N, K, g, 2 / math.sqrt(K) / 8, swiglu=True)
    r = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)
    gate_, up = (x.float() @ wd[:N].T) * r, (x.float() @ wd[N:].T) * r
    gain = (1.0 + 0.3 * torch.randn(K, generator=g)).half()
    xn = (gain.float() * (x.float() * r).half().float()).half().float()
    gg, ug = (xn @ wd[:N].T).half().float(), (xn @ wd[N:].T).half().float()
    return {"x": x.to(DEV), "q": q, "s": s, "gain": gain.to(DEV), "swiglu": F.silu(gate_) * up,
            "swiglu_gain": F.silu(gg).half().float() * ug}


def _check_epilogues(fn, M, N, K, tag):
    c = _case(N, K)
    x = c["x"][:M].contiguous()
    _close(fn(x, c["q"], c["s"]), c["plain"][:M], 4e-3, f"{tag} plain")
    y = c["res"][:M].clone()
    fn(x, c["q"], c["s"], out=y, residual=y)                                  # in place: h += x W^T
    _close(y, c["residual"][:M], 4e-3, f"{tag} residual in place")
    _close(fn(x, c["q"], c["s"], rms=True, eps=1e-5), c["rms"][:M], 4e-3, f"{tag} rms")
    _close(fn(x, c["q"], c["s"], rms=True, eps=1e-5, gain=c["gain"]), c["rms_gain"][:M], 1.5e-3, f"{tag} rms + gain")


def _check_swiglu(fn, M, N, K, tag):
    c = _swiglu_case(N, K)
    x = c["x"][:M].contiguous()
    _close(fn(x, c["q"], c["s"], rms=True, swiglu=True, eps=1e-6), c["swiglu"][:M], 6e-3, f"{tag} swiglu")
    _close(fn(x, c["q"], c["s"], rms=True, swiglu=True, eps=1e-6, gain=c["gain"]), c["swiglu_gain"][:M], 6e-3,
           f"{tag} swiglu + gain")


@pytest.mark.parametrize("M", [1, 2, 4, 5, 16])          # 1, 2, 4: the pipelined token kernel; 5, 16: the generic kernel
@pytest.mark.parametrize("N,K", NK)
def test_gemv_w8_plain_residual_rms(hip_lib, M, N, K):
    from diffsensei_amd import ops
    _check_epilogues(ops.llm_gemv_w8, M, N, K, "gemv")


@pytest.mark.parametrize("M", [1, 2, 4, 5, 16])
@pytest.mark.parametrize("N,K", [(344, 512), (1024, 1024)])
def test_gemv_w8_swiglu(hip_lib, M, N, K):
    from diffsensei_amd import ops
    _check_swiglu(ops.llm_gemv_w8, M, N, K, "gemv")


def test_gemv_w8_variant_1_is_the_generic_kernel_and_variant_2_is_refused(hip_lib):
    from diffsensei_amd import _lib, ops
    L = _lib.load()
    c = _case(520, 720)
    try:
        assert L.ds_set_option(b"llm_gemv_variant", 1) == 0
        _check_epilogues(ops.llm_gemv_w8, 2, 520, 720, "gemv variant 1")
        assert L.ds_set_option(b"llm_gemv_variant", 2) == 0
        with pytest.raises(_lib.DiffSenseiHipError, match="int8"):
            ops.llm_gemv_w8(c["x"][:1].contiguous(), c["q"], c["s"])
    finally:
        assert L.ds_set_option(b"llm_gemv_variant", 0) == 0


@pytest.mark.parametrize("M,N,K", [(M, N, K) for (N, K) in NK for M in (1, 5, 8, 16)] + [(16, 4096, 13824)])
def test_gemm16_w8_plain_residual_rms(hip_lib, M, N, K):
    from diffsensei_amd import ops
    _check_epilogues(ops.llm_gemm16_w8, M, N, K, "gemm16")


@pytest.mark.parametrize("M", [1, 5, 8, 16])
@pytest.mark.parametrize("N,K", [(344, 512), (1024, 1024)])
def test_gemm16_w8_swiglu(hip_lib, M, N, K):
    from diffsensei_amd import ops
    _check_swiglu(ops.llm_gemm16_w8, M, N, K, "gemm16")


@pytest.mark.parametrize("N,K,swiglu", [(520, 704, False), (520, 720, False), (260, 5120, False), (344, 512, True)])
def test_gemm16_w8_rows_are_independent(hip_lib, N, K, swiglu):
    """Row r of an M = 16 call == the same row of an M = 5 call == the same row when every other row is scaled x100."""
    from diffsensei_amd import ops
    c = _swiglu_case(N, K) if swiglu else _case(N, K)
    x, q, s, gain = c["x"], c["q"], c["s"], c["gain"]
    for kw in (dict(), dict(rms=True, eps=1e-5), dict(rms=True, eps=1e-5, gain=gain)):
        if swiglu and not kw:
            continue
        kw = dict(kw, swiglu=swiglu)
        full = ops.llm_gemm16_w8(x, q, s, **kw)
        five = ops.llm_gemm16_w8(x[:5].contiguous(), q, s, **kw)
        assert torch.equal(full[:5], five), f"M = 16 vs M = 5 rows differ ({kw})"
        for r in (0, 7, 15):
            x2 = x * 100.0
            x2[r] = x[r]
            other = ops.llm_gemm16_w8(x2, q, s, **kw)
            assert torch.equal(other[r], full[r]), f"row {r} depends on the other rows ({kw})"


def test_gemm16_w8_in_place_residual_leaves_the_rest_of_the_buffer(hip_lib):
    """Columns past N and rows past M of an oversized output buffer are untouched (ragged last 16-column tile)."""
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(11)
    M, N, K = 5, 520, 720
    x = _h((16, K), g).to(DEV)
    q, s, wd = _quantised(N + 24, K, g, 1 / math.sqrt(K))
    buf = _h((16, N + 24), g).to(DEV)
    before = buf.clone()
    ops.llm_gemm16_w8(x, q, s, out=buf, residual=buf, M=M, N=N)
    ref = (x[:M].float().cpu() @ wd[:N].T).half().float() + before[:M, :N].float().cpu()
    _close(buf[:M, :N], ref, 4e-3, "gemm16 residual in place, oversized buffer")
    assert torch.equal(buf[M:], before[M:]), "rows past M were written"
    assert torch.equal(buf[:, N:], before[:, N:]), "columns past N were written"


@pytest.mark.parametrize("N,K", [(5, 48), (768, 704)])
def test_dequant_w8_is_one_multiply_and_one_rounding(hip_lib, N, K):
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(N + K)
    q, s, _ = _quantised(N, K, g, 0.05)
    got = ops.llm_dequant_w8(q, s)
    assert got.dtype == torch.float16 and got.shape == (N, K)
    assert torch.equal(got, (q.float() * s[:, None]).half())
    big = torch.full((N * K + 64,), 7.0, dtype=torch.float16, device=DEV)      # a larger scratch: the tail stays as it was
    view = ops.llm_dequant_w8(q, s, out=big)
    assert torch.equal(view, got) and bool((big[N * K:] == 7.0).all())


def test_w8_refusals(hip_lib):
    from diffsensei_amd import _lib, ops
    g = torch.Generator().manual_seed(5)
    x24 = _h((2, 24), g).to(DEV)
    q24 = torch.randint(-127, 128, (32, 24), dtype=torch.int8, generator=g).to(DEV)
    s32 = torch.rand(32, generator=g).to(DEV) + 0.1
    for fn in (ops.llm_gemv_w8, ops.llm_gemm16_w8):
        with pytest.raises(ValueError):
            fn(x24, q24, s32)                                                  # K = 24: not a multiple of 16
    with pytest.raises(ValueError):
        ops.llm_dequant_w8(q24, s32)
    x = _h((2, 32), g).to(DEV)
    q = torch.randint(-127, 128, (32, 32), dtype=torch.int8, generator=g).to(DEV)
    for fn in (ops.llm_gemv_w8, ops.llm_gemm16_w8):
        with pytest.raises(ValueError):
            fn(x, q, s32[:31].contiguous())                                    # one scale short
        with pytest.raises(ValueError):
            fn(x, q, s32[:16].contiguous(), swiglu=True)                       # SwiGLU needs [2N] scales
        with pytest.raises(_lib.DiffSenseiHipError):
            fn(x, q, s32.half())                                               # scales must be fp32
        with pytest.raises(_lib.DiffSenseiHipError):
            fn(x, q.half(), s32)                                               # weights must be int8
    L = _lib.load()                                                            # and below the Python checks: the C ABI itself
    y = torch.zeros(2, 32, dtype=torch.float16, device=DEV)
    for entry in (L.ds_llm_gemv_w8, L.ds_llm_gemm16_w8):
        assert entry(x24.data_ptr(), 24, q24.data_ptr(), y.data_ptr(), 32, None, 0, 2, 32, 24, 0, None, 0, 1e-6,
                     s32.data_ptr(), None) != 0 and b"K % 16" in L.ds_last_error()
        assert entry(x.data_ptr(), 32, q.data_ptr(), y.data_ptr(), 32, None, 0, 2, 32, 32, 0, None, 0, 1e-6, None, None) != 0
    assert not y.any()
