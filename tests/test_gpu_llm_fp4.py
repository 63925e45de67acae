"""GPU: the MXFP4-weight (W4A16) forms of the MLLM decode kernels (csrc/llm.hip) - `llm_gemv_pipe_kernel` (M <= 4),
`llm_gemv_kernel` (generic), `llm_gemm16_kernel` (matrix pipe) and `llm_dequant_fp4_kernel`.

Reference: fp32 torch from the same operands, x.float() @ dequantize_rows_mxfp4(q, e, s).T.  The weights come from
`quantize_rows_mxfp4` of random fp16 matrices whose row n was first multiplied by 2 ** (n % 7 - 3) (SwiGLU: the up rows by
a further 8) and whose block b of every row by 2 ** -(b % 5), so a row scale or a block exponent taken from the wrong place
is off by a factor of two or more.  Tolerances are those of test_gpu_llm_w8.py for the same epilogues - every weight
e2m1 * 2^exponent is exact in f16 and the rounding points are the same: 4e-3 of max|ref| for plain, residual in place and rms,
1.5e-3 for rms + gain, 6e-3 for SwiGLU.  Shapes: (520, 704) 22 blocks, ragged last 4-column block / 16-column tile, K shorter
than one 2048-wide wave iteration; (520, 736) 23 blocks - an odd count, so the four-MFMA-steps-per-load pairing has a part-used
128-wide k-block; (260, 5120) several full iterations at the model's K; (768, 256) K shorter than one iteration;
(4096, 13824) one real-width case, gemm16 only."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
NK = [(520, 704), (520, 736), (260, 5120), (768, 256)]


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
    """MXFP4 weights (q, e, s on the device) and their fp32 dequantised form (host) of a random matrix with staggered row
    and block sizes"""
    from diffsensei_amd.mllm import dequantize_rows_mxfp4, quantize_rows_mxfp4
    w = _h((rows, K), g, std).float() * torch.pow(2.0, (torch.arange(rows) % 7 - 3).float())[:, None]
    w = w * torch.pow(2.0, -(torch.arange(K // 32) % 5).float()).repeat_interleave(32)[None, :]
    if swiglu:
        w[rows // 2:] *= 8.0
    q, e, s = quantize_rows_mxfp4(w)
    return (q.to(DEV), e.to(DEV), s.to(DEV)), dequantize_rows_mxfp4(q, e, s)


@functools.lru_cache(maxsize=None)
def _case(N, K):
    """Operands for 16 rows and their fp32 references, made once per (N, K); a test with M rows uses the first M."""
    g = torch.Generator().manual_seed(N * 3 + K)
    x, res = _h((16, K), g), _h((16, N), g)
    qes, wd = _quantised(N, K, g, 1 / math.sqrt(K))
    gain = (1.0 + 0.3 * torch.randn(K, generator=g)).half()
    xw = x.float() @ wd.T
    r = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    xn = (gain.float() * (x.float() * r).half().float()).half()
    return {"x": x.to(DEV), "res": res.to(DEV), "qes": qes, "gain": gain.to(DEV), "plain": xw,
            "residual": xw.half().float() + res.float(), "rms": xw * r, "rms_gain": xn.float() @ wd.T}


@functools.lru_cache(maxsize=None)
def _swiglu_case(N, K):
    g = torch.Generator().manual_seed(N + K)
    x = _h((16, K), g)
    qes, wd = _quantised(2 * N, K, g, 2 / math.sqrt(K) / 8, swiglu=True)
    r = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)
    gate_, up = (x.float() @ wd[:N].T) * r, (x.float() @ wd[N:].T) * r
    gain = (1.0 + 0.3 * torch.randn(K, generator=g)).half()
    xn = (gain.float() * (x.float() * r).half().float()).half().float()
    gg, ug = (xn @ wd[:N].T).half().float(), (xn @ wd[N:].T).half().float()
    return {"x": x.to(DEV), "qes": qes, "gain": gain.to(DEV), "swiglu": F.silu(gate_) * up,
            "swiglu_gain": F.silu(gg).half().float() * ug}


def _check_epilogues(fn, M, N, K, tag):
    c = _case(N, K)
    x = c["x"][:M].contiguous()
    _close(fn(x, *c["qes"]), c["plain"][:M], 4e-3, f"{tag} plain")
    y = c["res"][:M].clone()
    fn(x, *c["qes"], out=y, residual=y)                                       # in place: h += x W^T
    _close(y, c["residual"][:M], 4e-3, f"{tag} residual in place")
    _close(fn(x, *c["qes"], rms=True, eps=1e-5), c["rms"][:M], 4e-3, f"{tag} rms")
    _close(fn(x, *c["qes"], rms=True, eps=1e-5, gain=c["gain"]), c["rms_gain"][:M], 1.5e-3, f"{tag} rms + gain")


def _check_swiglu(fn, M, N, K, tag):
    c = _swiglu_case(N, K)
    x = c["x"][:M].contiguous()
    _close(fn(x, *c["qes"], rms=True, swiglu=True, eps=1e-6), c["swiglu"][:M], 6e-3, f"{tag} swiglu")
    _close(fn(x, *c["qes"], rms=True, swiglu=True, eps=1e-6, gain=c["gain"]), c["swiglu_gain"][:M], 6e-3,
           f"{tag} swiglu + gain")


@pytest.mark.parametrize("M", [1, 2, 4, 5, 16])          # 1, 2, 4: the pipelined token kernel; 5, 16: the generic kernel
@pytest.mark.parametrize("N,K", NK)
def test_gemv_fp4_plain_residual_rms(hip_lib, M, N, K):
    from diffsensei_amd import ops
    _check_epilogues(ops.llm_gemv_fp4, M, N, K, "gemv")


@pytest.mark.parametrize("M", [1, 2, 4, 5, 16])
@pytest.mark.parametrize("N,K", [(344, 512), (1024, 1024)])
def test_gemv_fp4_swiglu(hip_lib, M, N, K):
    from diffsensei_amd import ops
    _check_swiglu(ops.llm_gemv_fp4, M, N, K, "gemv")


def test_gemv_fp4_variant_1_is_the_generic_kernel_and_variant_2_is_refused(hip_lib):
    from diffsensei_amd import _lib, ops
    L = _lib.load()
    c = _case(520, 736)
    try:
        assert L.ds_set_option(b"llm_gemv_variant", 1) == 0
        _check_epilogues(ops.llm_gemv_fp4, 2, 520, 736, "gemv variant 1")
        assert L.ds_set_option(b"llm_gemv_variant", 2) == 0
        with pytest.raises(_lib.DiffSenseiHipError, match="MXFP4"):
            ops.llm_gemv_fp4(c["x"][:1].contiguous(), *c["qes"])
    finally:
        assert L.ds_set_option(b"llm_gemv_variant", 0) == 0


@pytest.mark.parametrize("M,N,K", [(M, N, K) for (N, K) in NK for M in (1, 5, 8, 16)] + [(16, 4096, 13824)])
def test_gemm16_fp4_plain_residual_rms(hip_lib, M, N, K):
    from diffsensei_amd import ops
    _check_epilogues(ops.llm_gemm16_fp4, M, N, K, "gemm16")


@pytest.mark.parametrize("M", [1, 5, 8, 16])
@pytest.mark.parametrize("N,K", [(344, 512), (1024, 1024)])
def test_gemm16_fp4_swiglu(hip_lib, M, N, K):
    from diffsensei_amd import ops
    _check_swiglu(ops.llm_gemm16_fp4, M, N, K, "gemm16")


@pytest.mark.parametrize("N,K,swiglu", [(520, 704, False), (520, 736, False), (260, 5120, False), (344, 512, True)])
def test_gemm16_fp4_rows_are_independent(hip_lib, N, K, swiglu):
    """Row r of an M = 16 call == the same row of an M = 5 call == the same row when every other row is scaled x100."""
    from diffsensei_amd import ops
    c = _swiglu_case(N, K) if swiglu else _case(N, K)
    x, qes, gain = c["x"], c["qes"], c["gain"]
    for kw in (dict(), dict(rms=True, eps=1e-5), dict(rms=True, eps=1e-5, gain=gain)):
        if swiglu and not kw:
            continue
        kw = dict(kw, swiglu=swiglu)
        full = ops.llm_gemm16_fp4(x, *qes, **kw)
        five = ops.llm_gemm16_fp4(x[:5].contiguous(), *qes, **kw)
        assert torch.equal(full[:5], five), f"M = 16 vs M = 5 rows differ ({kw})"
        for r in (0, 7, 15):
            x2 = x * 100.0
            x2[r] = x[r]
            other = ops.llm_gemm16_fp4(x2, *qes, **kw)
            assert torch.equal(other[r], full[r]), f"row {r} depends on the other rows ({kw})"


def test_gemm16_fp4_in_place_residual_leaves_the_rest_of_the_buffer(hip_lib):
    """Columns past N and rows past M of an oversized output buffer are untouched (ragged last 16-column tile)."""
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(11)
    M, N, K = 5, 520, 736
    x = _h((16, K), g).to(DEV)
    qes, wd = _quantised(N + 24, K, g, 1 / math.sqrt(K))
    buf = _h((16, N + 24), g).to(DEV)
    before = buf.clone()
    ops.llm_gemm16_fp4(x, *qes, out=buf, residual=buf, M=M, N=N)
    ref = (x[:M].float().cpu() @ wd[:N].T).half().float() + before[:M, :N].float().cpu()
    _close(buf[:M, :N], ref, 4e-3, "gemm16 residual in place, oversized buffer")
    assert torch.equal(buf[M:], before[M:]), "rows past M were written"
    assert torch.equal(buf[:, N:], before[:, N:]), "columns past N were written"


def _all_codes(N, K):
    """A hand-made MXFP4 matrix: every one of the 16 nibble codes in both nibble positions of every byte position of a word,
    block exponents that cycle through 114 .. 127 (both ends included), row scales that are no powers of two."""
    i = torch.arange(N * (K // 2)).view(N, K // 2)
    lo, hi = (i + i // 16) % 16, (3 * i + 5 + i // 7) % 16
    q = (lo | (hi << 4)).to(torch.uint8)
    e = (114 + (torch.arange(N * (K // 32)).view(N, K // 32) * 13) % 14).to(torch.uint8)
    s = 0.37 * torch.pow(1.7, (torch.arange(N) % 9 - 4).float())
    return q, e, s


@pytest.mark.parametrize("N,K,made", [(5, 64, False), (768, 704, False), (5, 64, True), (768, 704, True)])
def test_dequant_fp4_is_the_host_format_bit_for_bit(hip_lib, N, K, made):
    """Pins the nibble order (low nibble = even element), the byte order of the conversion's byte select and its scale
    semantics: w16 = f16(f32(e2m1 * 2^(e-127)) * s[n]), one multiply and one rounding, equal to the host format bit for bit."""
    from diffsensei_amd import ops
    from diffsensei_amd.mllm import dequantize_rows_mxfp4
    if made:
        q, e, s = _all_codes(N, K)
        both = torch.stack([q & 15, q >> 4])
        assert all(len(set(both[p].flatten().tolist())) == 16 for p in range(2)), "all 16 codes in both nibble positions"
        assert int(e.min()) == 114 and int(e.max()) == 127
    else:
        (q, e, s), _ = _quantised(N, K, torch.Generator().manual_seed(N + K), 0.05)
        q, e, s = q.cpu(), e.cpu(), s.cpu()
    block = dequantize_rows_mxfp4(q, e, torch.ones(N))                          # e2m1 * 2^(e-127): exact
    want = (block.float() * s[:, None]).half()
    got = ops.llm_dequant_fp4(q.to(DEV), e.to(DEV), s.to(DEV))
    assert got.dtype == torch.float16 and got.shape == (N, K)
    assert torch.equal(got.cpu(), want), f"{int((got.cpu() != want).sum())} of {N * K} elements differ"
    big = torch.full((N * K + 64,), 7.0, dtype=torch.float16, device=DEV)      # a larger scratch: the tail stays as it was
    view = ops.llm_dequant_fp4(q.to(DEV), e.to(DEV), s.to(DEV), out=big)
    assert torch.equal(view, got) and bool((big[N * K:] == 7.0).all())


def test_fp4_refusals(hip_lib):
    from diffsensei_amd import _lib, ops
    g = torch.Generator().manual_seed(5)
    u8 = lambda *shape, lo=0, hi=256: torch.randint(lo, hi, shape, dtype=torch.uint8, generator=g).to(DEV)
    x48, q48, e48 = _h((2, 48), g).to(DEV), u8(32, 24), u8(32, 1, lo=114, hi=128)
    s32 = torch.rand(32, generator=g).to(DEV) + 0.1
    for fn in (ops.llm_gemv_fp4, ops.llm_gemm16_fp4):
        with pytest.raises(ValueError):
            fn(x48, q48, e48, s32)                                             # K = 48: not a multiple of 32
    with pytest.raises(ValueError):
        ops.llm_dequant_fp4(q48, e48, s32)
    x, q, e = _h((2, 64), g).to(DEV), u8(32, 32), u8(32, 2, lo=114, hi=128)
    for fn in (ops.llm_gemv_fp4, ops.llm_gemm16_fp4):
        with pytest.raises(ValueError):
            fn(x, q, e, s32[:31].contiguous())                                 # one row scale short
        with pytest.raises(ValueError):
            fn(x, q, e[:, :1].contiguous(), s32)                               # one exponent per block is needed
        with pytest.raises(ValueError):
            fn(x, q, e[:16].contiguous(), s32[:16].contiguous(), swiglu=True)  # SwiGLU needs [2N] rows of both
        with pytest.raises(_lib.DiffSenseiHipError):
            fn(x, q, e, s32.half())                                            # row scales must be fp32
        with pytest.raises(_lib.DiffSenseiHipError):
            fn(x, q.to(torch.int8), e, s32)                                    # weights must be uint8
        with pytest.raises(_lib.DiffSenseiHipError):
            fn(x, q, e.to(torch.int8), s32)                                    # exponents must be uint8
    L = _lib.load()                                                            # and below the Python checks: the C ABI itself
    y = torch.zeros(2, 32, dtype=torch.float16, device=DEV)
    for entry in (L.ds_llm_gemv_fp4, L.ds_llm_gemm16_fp4):
        assert entry(x48.data_ptr(), 48, q48.data_ptr(), y.data_ptr(), 32, None, 0, 2, 32, 48, 0, None, 0, 1e-6,
                     s32.data_ptr(), e48.data_ptr(), None) != 0 and b"K % 32" in L.ds_last_error()
        assert entry(x.data_ptr(), 64, q.data_ptr(), y.data_ptr(), 32, None, 0, 2, 32, 64, 0, None, 0, 1e-6, s32.data_ptr(),
                     None, None) != 0 and b"w_exp" in L.ds_last_error()          # no block exponents
        assert entry(x.data_ptr(), 64, q.data_ptr(), y.data_ptr(), 32, None, 0, 2, 32, 64, 0, None, 0, 1e-6, None,
                     e.data_ptr(), None) != 0 and b"w_scale" in L.ds_last_error()  # no row scales
    assert L.ds_llm_dequant_fp4(q48.data_ptr(), s32.data_ptr(), y.data_ptr(), 2, 48, e48.data_ptr(), None) != 0
    assert L.ds_llm_dequant_fp4(q.data_ptr(), s32.data_ptr(), y.data_ptr(), 1, 64, None, None) != 0
    torch.cuda.synchronize()
    assert not y.any()
