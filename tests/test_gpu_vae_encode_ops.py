"""GPU: the four ops the VAE encoder adds, each through its C-ABI wrapper against fp32 torch on fp16-rounded operands:
the pad-(0,1,0,1) stride-2 mode of the gather GEMM kernels (`ops.conv3x3_down`), `vae_enc_conv_in_kernel`,
`vae_enc_conv_out_kernel` (quant_conv folded in, logvar clamp) and `vae_latents_kernel` (mode bit for bit, sample within one
fp16 ulp of float64 arithmetic on the Philox restatement of tests/_philox_ref.py).

Gate: tests/test_gpu_ops.py's per-op 2e-3 of max|ref| (fp16 output rounding is 4.9e-4 relative, the rest is accumulation
order); the bf16 instantiation of the downsample gets tests/test_gpu_vae.py's per-op 1e-2 (bf16 rounds at 2^-9)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _redraw_ref as R
from tests._philox_ref import philox_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-3


def _close(got, ref, tol=TOL, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    den = max(ref.abs().max().item(), 1e-3)
    print(f"{what}: max err {err:.4g} vs max|ref| {den:.4g} ({err / den:.3g})")
    assert err <= tol * den, f"{what}: max err {err:.4g} vs max|ref| {den:.4g}"


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------- Downsample2D(padding=0)
DOWN_SHAPES = [(2, 16, 16, 128),      # the plain case
               (1, 34, 18, 256),      # Wo = 17 crosses a 16-wide tile
               (1, 9, 11, 128),       # odd sides: no pad row or column is read
               (1, 40, 72, 512)]      # the widest level


def _down_case(B, H, W, C, dt):
    g = torch.Generator().manual_seed(B * H + W + C)
    x = torch.randn(B, C, H, W, generator=g).to(dt)
    w = (torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)).to(dt)
    b = torch.randn(C, generator=g).to(dt)
    return x, w, b


@pytest.mark.parametrize("B,H,W,C", DOWN_SHAPES)
def test_conv3x3_down(hip_lib, B, H, W, C):
    from diffsensei_amd import ops
    x, w, b = _down_case(B, H, W, C, torch.float16)
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), b.float(), stride=2)
    assert ref.shape == (B, C, H // 2, W // 2)
    xn, wn = _nhwc(x).to(DEV), _nhwc(w).to(DEV)
    got = ops.conv3x3_down(xn, wn, b.to(DEV))
    assert got.shape == (B, H // 2, W // 2, C) and got.dtype == torch.float16
    _close(got.permute(0, 3, 1, 2), ref, what=f"conv3x3_down {(B, H, W, C)}")
    if (B, H, W, C) == DOWN_SHAPES[0]:
        # the UNet's stride-2 convolution pads 1 on every side: the same shape out, another function of the input
        sym = ops.conv3x3(xn, wn, b.to(DEV), stride=2)
        assert sym.shape == got.shape
        ref_sym = F.conv2d(x.float(), w.float(), b.float(), stride=2, padding=1)
        _close(sym.permute(0, 3, 1, 2), ref_sym, what="symmetric stride 2 (unchanged)")
        assert float((sym.float() - got.float()).abs().max()) > 0.5
        assert float((sym.permute(0, 3, 1, 2).float().cpu() - ref).abs().max()) > 100 * TOL * float(ref.abs().max())


@pytest.mark.parametrize("B,H,W,C", DOWN_SHAPES[:3])
def test_conv3x3_down_bf16(hip_lib, B, H, W, C):
    from diffsensei_amd import ops
    x, w, b = _down_case(B, H, W, C, torch.bfloat16)
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), b.float(), stride=2)
    got = ops.conv3x3_down(_nhwc(x).to(DEV), _nhwc(w).to(DEV), b.to(DEV))
    assert got.dtype == torch.bfloat16
    _close(got.permute(0, 3, 1, 2), ref, tol=1e-2, what=f"conv3x3_down bf16 {(B, H, W, C)}")


def test_conv3x3_down_refusals(hip_lib):
    from diffsensei_amd import _lib, ops
    x = torch.zeros(1, 1, 8, 128, dtype=torch.float16, device=DEV)
    w = torch.zeros(128, 3, 3, 128, dtype=torch.float16, device=DEV)
    b = torch.zeros(128, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError):
        ops.conv3x3_down(x, w, b)                                            # one row: no output row
    with pytest.raises(_lib.DiffSenseiHipError):
        ops.conv3x3_down(torch.zeros(1, 8, 8, 96, dtype=torch.float16, device=DEV),
                         torch.zeros(128, 3, 3, 96, dtype=torch.float16, device=DEV), b)     # Cin % 64


# ---------------------------------------------------------------- conv_in
def _conv_in_weights(C=128, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(C, 3, 3, 3, generator=g) / math.sqrt(27)).half(), (torch.randn(C, generator=g) * 0.3).half()


@pytest.mark.parametrize("B,H,W", [(2, 16, 24), (1, 9, 11)])
def test_enc_conv_in_forms(hip_lib, B, H, W):
    from diffsensei_amd import ops
    w, b = _conv_in_weights()
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(H), dtype=torch.uint8)
    xn = (u8.float() * 2.0 / 255.0 - 1.0).permute(0, 3, 1, 2).contiguous()          # fp32 NCHW in [-1, 1]
    ref = F.conv2d(xn, w.float(), b.float(), padding=1)
    wd, bd = _nhwc(w).to(DEV), b.to(DEV)
    got_u8 = ops.vae_enc_conv_in(u8.to(DEV), wd, bd).permute(0, 3, 1, 2)
    got_f = ops.vae_enc_conv_in(xn.to(DEV), wd, bd).permute(0, 3, 1, 2)
    assert got_u8.shape == (B, 128, H, W) and got_u8.dtype == torch.float16
    _close(got_u8, ref, what=f"enc conv_in uint8 {(B, H, W)}")
    _close(got_f, ref, what=f"enc conv_in fp32 {(B, H, W)}")
    _close(got_u8, got_f, what="uint8 vs fp32 form")
    got_bf = ops.vae_enc_conv_in(u8.to(DEV), wd.bfloat16(), bd.bfloat16()).permute(0, 3, 1, 2)
    _close(got_bf, ref, tol=1e-2, what="enc conv_in bf16")


def test_enc_conv_in_zero_bytes_border(hip_lib):
    """An all-zero-byte image is -1 everywhere inside; the padding is 0, not -1: the interior is one constant per channel
    (bias - sum of the weights), the border is not."""
    from diffsensei_amd import ops
    w, b = _conv_in_weights(seed=8)
    H, W = 8, 16
    u8 = torch.zeros(1, H, W, 3, dtype=torch.uint8)
    got = ops.vae_enc_conv_in(u8.to(DEV), _nhwc(w).to(DEV), b.to(DEV)).permute(0, 3, 1, 2).float().cpu()
    ref = F.conv2d(torch.full((1, 3, H, W), -1.0), w.float(), b.float(), padding=1)
    _close(got, ref, what="zero bytes")
    const = b.float() - w.float().sum(dim=(1, 2, 3))                                # what padding with -1 would give everywhere
    assert float((ref[0, :, 1:-1, 1:-1] - const[:, None, None]).abs().max()) < 1e-5
    border = torch.ones(H, W, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    gap = (ref[0][:, border] - const[:, None]).abs().max().item()
    assert gap > 0.3                                                                # the rule is visible ...
    assert float((got[0][:, border] - ref[0][:, border]).abs().max()) <= TOL * float(ref.abs().max())   # ... and the kernel follows it


# ---------------------------------------------------------------- conv_out + quant_conv
@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (1, 9, 11)])
def test_enc_conv_out_fold_and_clamps(hip_lib, B, H, W):
    from diffsensei_amd import ops
    from diffsensei_amd.vae import fold_quant_conv
    C = 512
    g = torch.Generator().manual_seed(B + H)
    x = torch.randn(B, C, H, W, generator=g).half()
    wc, bc = torch.randn(8, C, 3, 3, generator=g) / math.sqrt(9 * C), torch.randn(8, generator=g) * 0.1
    wq, bq = torch.randn(8, 8, 1, 1, generator=g) * 0.5, torch.randn(8, generator=g) * 0.1
    wq[4:] *= 25.0                                     # logvar rows: a standard deviation of ~ 35, so both clamp ends are reached
    w2, b2 = fold_quant_conv(wc, bc, wq, bq)
    w2 = w2.half()
    raw = F.conv2d(x.float(), w2.float(), b2, padding=1)
    assert float(raw[:, 4:].max()) > 25 and float(raw[:, 4:].min()) < -35, "the inputs must overshoot both clamp ends"
    ref = torch.cat([raw[:, :4], raw[:, 4:].clamp(-30.0, 20.0)], dim=1)
    got = ops.vae_enc_conv_out(_nhwc(x).to(DEV), _nhwc(w2).to(DEV), b2.to(DEV)).cpu()
    assert got.shape == (B, 8, H, W) and got.dtype == torch.float32
    _close(got[:, :4], ref[:, :4], what=f"mean {(B, H, W)}")
    _close(got[:, 4:], ref[:, 4:], what=f"logvar {(B, H, W)}")
    hi, lo = raw[:, 4:] > 20.5, raw[:, 4:] < -30.5
    assert hi.any() and lo.any()
    assert (got[:, 4:][hi] == 20.0).all() and (got[:, 4:][lo] == -30.0).all()
    assert float(got[:, 4:].max()) == 20.0 and float(got[:, 4:].min()) == -30.0
    assert float(got[:, :4].abs().max()) < 20.0 and float(raw[:, :4].abs().max()) > 2.0     # the mean is not clamped
    # the fold is the two convolutions: the unfolded fp32 pair agrees with the reference up to the fp16 rounding of W'
    two = F.conv2d(F.conv2d(x.float(), wc, bc, padding=1), wq, bq)
    assert float((two - raw).abs().max() / raw.abs().max()) < 1e-3


# ---------------------------------------------------------------- moments -> latents
SF = 0.13025
MEAN, STD = [0.3, -0.2, 0.05, 1.1], [1.2, 0.7, 2.0, 0.9]


def _affine(pair):
    sf = torch.tensor(SF, dtype=torch.float32)
    if not pair:
        return torch.zeros(4), sf.expand(4).clone()
    return torch.tensor(MEAN, dtype=torch.float32), sf / torch.tensor(STD, dtype=torch.float32)


def _moments(B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randn(B, 4, h, w, generator=g) * 3.0, torch.randn(B, 4, h, w, generator=g) - 1.0], dim=1)


@pytest.mark.parametrize("pair", [False, True])
def test_latents_mode_bit_for_bit(hip_lib, pair):
    from diffsensei_amd import ops
    shift, scale = _affine(pair)
    for B, h, w in ((2, 8, 8), (3, 9, 11), (1, 17, 15)):
        mom = _moments(B, h, w, 10 * B + h)
        got = ops.vae_latents(mom.to(DEV), scale.tolist(), shift.tolist() if pair else None).cpu()
        want = ((mom[:, :4] - shift.view(1, 4, 1, 1)) * scale.view(1, 4, 1, 1)).half()
        assert got.shape == (B, 4, h, w) and got.dtype == torch.float16
        assert torch.equal(got, want), (pair, B, h, w)
    if not pair:
        assert torch.equal(want, (mom[:, :4] * torch.tensor(SF, dtype=torch.float32)).half())      # fp16(mean * sf)


@pytest.mark.parametrize("pair", [False, True])
def test_latents_sample_vs_float64(hip_lib, pair):
    """float64 arithmetic on the device's own moments and the Philox restatement (step 0, stream_id 1).  The device normals are
    within 2e-6 of that restatement (tests/test_gpu_euler_ancestral.py's gate) and exp is fp32: one fp16 rounding flip is all
    that can differ."""
    from diffsensei_amd import ops
    shift, scale = _affine(pair)
    B, h, w = 3, 9, 11
    seeds = [12345, 2 ** 62 + 3, 12345]
    mom = _moments(B, h, w, 77)
    mom[2] = mom[0]                                     # the same picture at rows 0 and 2, with the same seed
    sd = torch.tensor(seeds, dtype=torch.int64, device=DEV)
    got = ops.vae_latents(mom.to(DEV), scale.tolist(), shift.tolist() if pair else None, seeds=sd).cpu()
    n = torch.from_numpy(philox_normal(seeds, 0, 1, h * w)).view(B, 4, h, w)
    m64 = mom.double()
    z = m64[:, :4] + torch.exp(0.5 * m64[:, 4:]) * n
    want = (z - shift.double().view(1, 4, 1, 1)) * scale.double().view(1, 4, 1, 1)
    d = R.ulp16(got, want.half())
    print(f"latents sample pair={pair}: fp16 ulp distance max {int(d.max())}, elements off by one {int((d == 1).sum())} of {d.numel()}")
    assert int(d.max()) <= 1
    assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[1])
    # the row in the batch does not matter: the first image alone, and behind another one
    alone = ops.vae_latents(mom[:1].to(DEV), scale.tolist(), shift.tolist() if pair else None, seeds=sd[:1]).cpu()
    assert torch.equal(alone[0], got[0])
    # another seed, another sample; no seeds, the mode
    other = ops.vae_latents(mom[:1].to(DEV), scale.tolist(), shift.tolist() if pair else None, seeds=sd[1:2]).cpu()
    assert not torch.equal(other, alone)
    with pytest.raises(ValueError):
        ops.vae_latents(mom.to(DEV), scale.tolist(), None, seeds=sd[:2])
