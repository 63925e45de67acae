"""GPU: `llm_gemm16_kernel` (csrc/llm.hip) - the M <= 16 weight-streaming GEMM of the batched MLLM decode.

Reference: fp32 torch from the same fp16 inputs.  Tolerances are those of test_gpu_mllm.py for the same epilogues (they
bound the fp16 output rounding and the accumulation order, which the MFMA kernel shares): 4e-3 of max|ref| for plain,
residual and rms, 1.5e-3 for rms + gain, 6e-3 for SwiGLU.  Row independence is checked bit for bit."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _h(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).half()


def _close(got, ref, tol, what):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    den = max(ref.abs().max().item(), 1e-3)
    gate(what, err / den, tol)


SHAPES = [(M, N, K) for (N, K) in [(520, 704), (260, 5120), (768, 256)] for M in (1, 5, 8, 16)] + [(16, 4096, 13824)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm16_plain_residual_rms(hip_lib, M, N, K):
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(M * 7 + N + K)
    x, w, res = _h((M, K), g), _h((N, K), g, 1 / math.sqrt(K)), _h((M, N), g)
    xd, wd = x.to(DEV), w.to(DEV)
    xw = x.float() @ w.float().T
    _close(ops.llm_gemm16(xd, wd), xw, 4e-3, "plain")
    y = res.to(DEV).clone()
    ops.llm_gemm16(xd, wd, out=y, residual=y)                                 # in place: h += x W^T
    _close(y, xw.half().float() + res.float(), 4e-3, "residual in place")
    r = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    _close(ops.llm_gemm16(xd, wd, rms=True, eps=1e-5), xw * r, 4e-3, "rms")
    gain = (1.0 + 0.3 * torch.randn(K, generator=g)).half()
    xn = (gain.float() * (x.float() * r).half().float()).half()
    _close(ops.llm_gemm16(xd, wd, rms=True, eps=1e-5, gain=gain.to(DEV)), xn.float() @ w.float().T, 1.5e-3, "rms + gain")


@pytest.mark.parametrize("M", [1, 5, 8, 16])
@pytest.mark.parametrize("N,K", [(344, 512), (1024, 1024)])
def test_gemm16_swiglu(hip_lib, M, N, K):
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    x, w = _h((M, K), g), _h((2 * N, K), g, 2 / math.sqrt(K))
    r = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)
    gate_, up = (x.float() @ w[:N].float().T) * r, (x.float() @ w[N:].float().T) * r
    _close(ops.llm_gemm16(x.to(DEV), w.to(DEV), rms=True, swiglu=True, eps=1e-6), F.silu(gate_) * up, 6e-3, "swiglu")
    gain = (1.0 + 0.3 * torch.randn(K, generator=g)).half()
    xn = (gain.float() * (x.float() * r).half().float()).half().float()
    gate_, up = (xn @ w[:N].float().T).half().float(), (xn @ w[N:].float().T).half().float()
    _close(ops.llm_gemm16(x.to(DEV), w.to(DEV), rms=True, swiglu=True, eps=1e-6, gain=gain.to(DEV)),
           F.silu(gate_).half().float() * up, 6e-3, "swiglu + gain")


@pytest.mark.parametrize("N,K,swiglu", [(520, 704, False), (260, 5120, False), (344, 512, True)])
def test_gemm16_rows_are_independent(hip_lib, N, K, swiglu):
    """Row r of an M = 16 call == the same row of an M = 5 call == the same row when every other row is scaled x100."""
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(N + K)
    x = _h((16, K), g).to(DEV)
    w = _h(((2 if swiglu else 1) * N, K), g, 1 / math.sqrt(K)).to(DEV)
    gain = (1.0 + 0.3 * torch.randn(K, generator=g)).half().to(DEV)
    for kw in (dict(), dict(rms=True, eps=1e-5), dict(rms=True, eps=1e-5, gain=gain)):
        if swiglu and not kw:
            continue
        kw = dict(kw, swiglu=swiglu)
        full = ops.llm_gemm16(x, w, **kw)
        five = ops.llm_gemm16(x[:5].contiguous(), w, **kw)
        assert torch.equal(full[:5], five), f"M = 16 vs M = 5 rows differ ({kw})"
        for r in (0, 7, 15):
            x2 = x * 100.0
            x2[r] = x[r]
            other = ops.llm_gemm16(x2, w, **kw)
            assert torch.equal(other[r], full[r]), f"row {r} depends on the other rows ({kw})"


def test_gemm16_in_place_residual_leaves_the_rest_of_the_buffer(hip_lib):
    """Columns past N and rows past M of an oversized output buffer are untouched (ragged last 16-column tile)."""
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(11)
    M, N, K = 5, 520, 704
    x, w = _h((16, K), g).to(DEV), _h((N + 24, K), g, 1 / math.sqrt(K)).to(DEV)
    buf = _h((16, N + 24), g).to(DEV)
    before = buf.clone()
    ops.llm_gemm16(x, w, out=buf, residual=buf, M=M, N=N)
    ref = (x[:M].float() @ w[:N].float().T).half().float() + before[:M, :N].float()
    _close(buf[:M, :N], ref, 4e-3, "residual in place, oversized buffer")
    assert torch.equal(buf[M:], before[M:]), "rows past M were written"
    assert torch.equal(buf[:, N:], before[:, N:]), "columns past N were written"
