"""GPU: the convolution mode of `lora_merge_kernel` (csrc/lora.hip) through `ops.lora_merge(..., conv_cin=Cin)`.

The base W is a 3x3 weight in checkpoint order [Cout, Cin, 3, 3]; A [R, 9 Cin] and the output are in the packed tap-major
order of `engine.pack_conv3x3`, k = (ky * 3 + kx) * Cin + ci.  The reference is fp64 on the f16 operands, formed in
CHECKPOINT order (dW[o,i,ky,kx] = sum_r B[o,r] A[r,i,ky,kx] on the 4-D down matrix) and packed afterwards, so a wrong tap or
channel index in the kernel cannot cancel against the same mistake in the test.

The bound is the derived one of tests/test_gpu_lora_merge.py, per element
    |out - ref| <= max(2^-11 |ref|, 2^-25) + (R + 2) 2^-24 T,     T = |W| + sum_i |s_i| (|B_i| |A_i|)
(half an f16 ulp for the one rounding of the result plus the forward bound of an fp32 sum of R + 1 exact products, the
strength and the add onto f32(W)); it is not measured.

Shapes (Cout, Cin): (72, 8) - nine taps inside one 64-column tile, a ragged row tile and a ragged last column tile;
(64, 40) - taps that start in the middle of a tile; (136, 64) - one tap per tile, three row tiles, the last ragged.  Ranks 1,
8 and 33 (below one MFMA k-step, one aligned piece of B, past one k-step and off its 8-rank pieces), each as the live segment
of two, the other at strength 0 - before it and behind it.
"""
import pytest
import torch

from tests._arena import Arena, Plain

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(72, 8), (64, 40), (136, 64)]
RANKS = [1, 8, 33]


def _case(Cout, Cin, r, dead_first, seed):
    """Two segments, one of them at strength 0: ranks (5, r) or (r, 5)."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.03).half()
    ranks = (5, r) if dead_first else (r, 5)
    A4 = (torch.randn(sum(ranks), Cin, 3, 3, generator=g) * 0.02).half()
    B = (torch.randn(Cout, sum(ranks), generator=g) * 0.02).half()
    s = [0.0, -0.75] if dead_first else [1.25, 0.0]
    return dict(W=W, A4=A4, B=B, seg=torch.tensor([0, ranks[0], sum(ranks)], dtype=torch.int32),
                s=torch.tensor(s, dtype=torch.float32), Cin=Cin)


def _packed_A(c):
    from diffsensei_amd.lora import pack_conv_down
    return pack_conv_down(c["A4"])


def _reference(c):
    """(ref, T) in fp64, packed order, from sums formed in checkpoint order."""
    from diffsensei_amd.engine import pack_conv3x3
    W, A4, B = c["W"].double(), c["A4"].double(), c["B"].double()
    ref, T = W.clone(), W.abs()
    seg, s = c["seg"].tolist(), c["s"].double().tolist()
    for i in range(len(s)):
        lo, hi = seg[i], seg[i + 1]
        ref += s[i] * torch.einsum("or,rikl->oikl", B[:, lo:hi], A4[lo:hi])
        T += abs(s[i]) * torch.einsum("or,rikl->oikl", B[:, lo:hi].abs(), A4[lo:hi].abs())
    return pack_conv3x3(ref), pack_conv3x3(T)


def _run(mem, c, ld_extra=0):
    Cout, K = c["W"].shape[0], 9 * c["Cin"]
    W, A, B = mem.place(c["W"].reshape(Cout, -1)), mem.place(_packed_A(c)), mem.place(c["B"])
    seg, s = mem.place(c["seg"]), mem.place(c["s"])
    out = mem.out((Cout, K), ld=K + ld_extra)
    mem.ops.lora_merge(W, A, B, seg, s, out=out, conv_cin=c["Cin"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dead_first", [False, True])
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("Cout,Cin", SHAPES)
def test_conv_merge_vs_fp64(hip_lib, Cout, Cin, r, dead_first):
    from diffsensei_amd.engine import pack_conv3x3
    c = _case(Cout, Cin, r, dead_first, seed=Cout + Cin + r)
    out = _run(Plain(DEV), c)
    ref, T = _reference(c)
    R = c["A4"].shape[0]
    got = out.double().cpu()
    bound = torch.maximum(ref.abs() * 2.0 ** -11, torch.full_like(ref, 2.0 ** -25)) + (R + 2) * 2.0 ** -24 * T
    worst = float(((got - ref).abs() / bound).max())
    print(f"[lora conv merge {Cout}x{Cin} r={r} dead_first={dead_first}] max err / bound = {worst:.4g}")
    assert torch.isfinite(got).all()
    assert worst <= 1.0, f"error is {worst:.4g} x the derived bound"
    base = pack_conv3x3(c["W"]).double()
    assert float((got - base).abs().max()) > 1e-4, "the live adapter left no trace"
    # every tap moved: a kernel that merged one tap's columns only would pass the line above
    moved = (got - base).abs().reshape(Cout, 9, Cin).amax(dim=(0, 2))
    assert bool((moved > 1e-5).all()), moved


@pytest.mark.parametrize("Cout,Cin", SHAPES)
def test_no_adapter_and_zero_strength_give_the_packed_base(hip_lib, Cout, Cin):
    from diffsensei_amd import ops
    from diffsensei_amd.engine import pack_conv3x3
    c = _case(Cout, Cin, 8, False, seed=5)
    W = c["W"].to(DEV)
    want = pack_conv3x3(c["W"]).view(torch.int16)
    out = ops.lora_merge(W, conv_cin=Cin)                                   # no adapter; the 4-D base as it lies
    assert out.shape == (Cout, 9 * Cin) and torch.equal(out.cpu().view(torch.int16), want)
    out = ops.lora_merge(W.reshape(Cout, -1), conv_cin=Cin)                 # ... and its [Cout, 9 Cin] view
    assert torch.equal(out.cpu().view(torch.int16), want)
    A, B = _packed_A(c).to(DEV), c["B"].to(DEV)
    out = ops.lora_merge(W, A, B, c["seg"].to(DEV), torch.zeros(2, device=DEV), conv_cin=Cin)
    assert torch.equal(out.cpu().view(torch.int16), want)
    out = ops.lora_merge(W, A, B, [0, 0, 0], [1.0, 2.0], conv_cin=Cin)      # empty segments
    assert torch.equal(out.cpu().view(torch.int16), want)


def test_aliasing_the_base_and_misfits_are_refused(hip_lib):
    from diffsensei_amd import _lib, ops
    c = _case(72, 8, 8, False, seed=6)
    W, A, B = c["W"].to(DEV).reshape(72, -1), _packed_A(c).to(DEV), c["B"].to(DEV)
    before = W.clone()
    with pytest.raises(_lib.DiffSenseiHipError, match="read only"):
        ops.lora_merge(W, A, B, c["seg"].to(DEV), c["s"].to(DEV), out=W, conv_cin=8)
    with pytest.raises(ValueError):                                          # K is not 9 Cin
        ops.lora_merge(W, A, B, c["seg"].to(DEV), c["s"].to(DEV), conv_cin=16)
    with pytest.raises(ValueError):                                          # a 4-D base without the mode
        ops.lora_merge(c["W"].to(DEV)[:, :, :, :2].contiguous(), conv_cin=8)
    wide = torch.zeros(72, 80, dtype=torch.float16, device=DEV)[:, :72]
    with pytest.raises(ValueError):                                          # the base must be contiguous
        ops.lora_merge(wide, conv_cin=8)
    torch.cuda.synchronize()
    assert torch.equal(W, before)                                            # nothing was launched


@pytest.mark.parametrize("Cout,Cin,r", [(72, 8, 33), (64, 40, 1), (136, 64, 8)])
def test_conv_merge_inside_poisoned_memory(hip_lib, Cout, Cin, r):
    """The rule of tests/test_gpu_poisoned_memory.py: operands between NaN (and 1000.0) guards, the output with canary columns
    behind a wide leading dimension - the result depends on nothing but the operands, and no guard byte changes."""
    c = _case(Cout, Cin, r, True, seed=7)
    results = []
    for mem in (Plain(DEV), Arena(DEV, "nan", capacity=24 << 20), Arena(DEV, "loud", capacity=24 << 20)):
        out = _run(mem, c, ld_extra=8)
        mem.check()
        assert torch.isfinite(out).all(), mem.fill
        results.append(out.contiguous().cpu())
    for out in results[1:]:
        assert torch.equal(out.view(torch.int16), results[0].view(torch.int16))


def test_op_describe_reports_the_packed_width(hip_lib):
    import ctypes as C
    from diffsensei_amd import ops
    c = _case(136, 64, 33, False, seed=8)
    N, K, R = 136, 9 * 64, 38
    out = torch.empty(N, K, dtype=torch.float16, device=DEV)
    op = ops.lora_merge_op(c["W"].to(DEV), out, _packed_A(c).to(DEV), c["B"].to(DEV), c["seg"].to(DEV), c["s"].to(DEV), conv_cin=64)
    assert op.i[1] == K and op.i[4] == 64
    name, fl, by = C.create_string_buffer(64), C.c_double(), C.c_double()
    assert hip_lib.ds_op_describe(C.byref(op), name, 64, C.byref(fl), C.byref(by)) == 0
    assert name.value == b"lora_merge_kernel"
    assert fl.value == 2.0 * N * K * R and by.value == 2.0 * (2.0 * N * K + R * (N + K))
