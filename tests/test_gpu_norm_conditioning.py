"""GPU: GroupNorm and fused-LayerNorm statistics over their stated range (csrc/norm.hip, `gn_emit` of csrc/conv_halo.hip, the
fused-LayerNorm epilogues of csrc/ds_epilogue.h) - diffusers' GroupNorm / LayerNorm of ResnetBlock2D, Transformer2DModel and
the VAE decoder [3P], reached from reference src/models/unet.py:244-338.  Every variance on those paths is one-pass,
var = E[x^2] - mean^2 from fp32 sums, which loses accuracy as 1 + (mean / sigma)^2 grows; large means are what a convolution
bias plus the per-image time-embedding bias put in front of norm2, and what the VAE decoder carries.

Cases, references (float64 on the CPU, from the ROUNDED inputs) and the emulation the asserted range comes from:
tests/_norm_cases.py; tests/test_norm_cases_host.py shows on the CPU that the kernels' arithmetic reaches every tolerance
asserted here with a factor of three in hand (the comparison of the two GroupNorm paths with each other, a difference of two
f16 tensors, to one f16 ulp of the largest output: half its tolerance).  Tolerances are the project's own for these kernels (max |y - ref| / max |ref|):
GroupNorm f16 3e-3, bf16 2e-2, convolution-partial path vs three-launch path 2e-3, LayerNorm 2e-3, fused LayerNorm 5e-3,
|y - beta| <= 3e-3 on an exactly constant group.

Asserted: GroupNorm f16 mean / sigma <= 64, bf16 <= 32, fused LayerNorm <= 32, and the families mixed, spike, flat, tiny, concat.
Beyond (GroupNorm 128, 256; bf16 64): finite output asserted, the error is written beside the emulation's figure to
norm_conditioning.txt in the directory of the gate log of tests/_gates.py (kept as profiles/norm_conditioning.txt).

What each family is there to catch (reasoned from the code, csrc/norm.hip):
  * flat - dropping the fmaxf(..., 0) clamp of the variance: the constant group at 11.0859375 has a sum of squares that
    rounds, its ss / n - mean^2 comes out a few fp32 ulps of mean^2 either side of zero and, at (1, 333, 128 + 64) and
    (1, 100, 512), below -1e-6 -> NaN at eps 1e-6 (tests/test_norm_cases_host.py::test_flat_family_needs_the_variance_clamp
    shows it on the emulation; the groups at 8.0 and -3.0 are exact in fp32, variance exactly 0: they pin y = beta, not the
    clamp).  tiny (variance 1e-6) pins the scale at which eps enters, it does not reach the clamp either;
  * mixed - indexing the finalize step's partials with cpg off by one: a group then takes a neighbour's channel, whose level
    differs by orders of magnitude (k = 64 | 0 | ~2e4 | ~1e-2 side by side);
  * concat - summing x2's partials with C1's stride (or reading x2 with x1's): the +64 / -64 seam inside a group moves;
  * the convolution cases - halving the chunks the finalize step reads on the partial path: 2, 3 and 8 pixel tiles per image.
"""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import _norm_cases as nc
from tests._gates import LOG as GATE_LOG, gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = os.path.join(os.path.dirname(GATE_LOG), "norm_conditioning.txt")     # beside the measured gates
_id = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)

GN_CASES = ([(s, f) for s in nc.GN_SHAPES_ALL for f in nc.GN_FAMILIES_ALL] +
            [(s, f) for s in nc.GN_SHAPES_REST for f in nc.GN_FAMILIES_REST])


def _record(line):
    print("[recorded] " + line)
    try:
        os.makedirs(os.path.dirname(RECORD), exist_ok=True)
        with open(RECORD, "a") as fh:
            fh.write(line + "\n")
    except OSError:
        pass


class _option:
    """`with _option(b"gn_variant", 1)`: the knob set on this thread, 0 again on exit."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        from diffsensei_amd import _lib
        self.lib = _lib.load()
        assert self.lib.ds_set_option(self.key, self.value) == 0
        return self.lib

    def __exit__(self, *exc):
        self.lib.ds_set_option(self.key, 0)


def _flat_abs(y, ref, info, Cc, groups=nc.GROUPS):
    cpg = Cc // groups
    y = y.double().cpu()
    return max((y[b, :, g * cpg:(g + 1) * cpg] - ref[b, :, g * cpg:(g + 1) * cpg]).abs().max().item() for b, g, _ in info["flat"])


# ---------------------------------------------------------------------------------------------- 1. three-launch GroupNorm, f16
@pytest.mark.parametrize("shape,family", GN_CASES, ids=_id)
def test_groupnorm_f16_three_launch(hip_lib, shape, family):
    """ops.groupnorm, 32 groups, with and without SiLU, eps 1e-5 and 1e-6, both gn_variant values (512-thread blocks with >= 64
    rows per block | 256-thread blocks with 8-row chunks), single- and two-source as the shape says."""
    from diffsensei_amd import ops
    B, HW, C1, C2 = shape
    Cc = C1 + C2
    x, info = nc.gn_case(family, B, HW, Cc)
    c1 = info["c1"] or C1
    x1 = x[..., :c1].contiguous().to(DEV)
    x2 = x[..., c1:].contiguous().to(DEV) if c1 < Cc else None
    gamma, beta = nc.affine(Cc, 0)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    k = nc.family_k(family)
    recorded = k in nc.K_RECORDED
    worst = 0.0
    for eps in (1e-5, 1e-6):
        ref = {silu: nc.gn_ref(x, gamma, beta, nc.GROUPS, eps, silu) for silu in (False, True)}
        for variant in (0, 1):
            with _option(b"gn_variant", variant):
                got = {silu: ops.groupnorm(x1, gd, bd, nc.GROUPS, eps, silu, x2) for silu in (False, True)}
            for silu in (False, True):
                e = nc.relmax(got[silu], ref[silu])
                what = f"groupnorm f16 {_id(shape)} {family} eps {eps:g} silu {int(silu)} gn_variant {variant}"
                if recorded:
                    worst = max(worst, e)
                    continue
                gate(what, e, nc.TOL_GN_F16)
                if info["flat"]:
                    gate(what + ": |y - beta| on the constant groups", _flat_abs(got[silu], ref[silu], info, Cc), nc.TOL_FLAT_ABS)
    if recorded:
        emu = 0.0
        for variant in (0, 1):
            s, ss = nc.emulate_gn_partials(x, *nc.kernel_chunks(B, HW, Cc, variant))
            for eps in (1e-5, 1e-6):
                tabA, tabS, _, _ = nc.emulate_gn_finalize(s, ss, HW, gamma, beta, nc.GROUPS, eps, contract=1)
                for silu in (False, True):
                    y = torch.from_numpy(nc.emulate_gn_apply(x, tabA, tabS, silu))
                    emu = max(emu, nc.relmax(y, nc.gn_ref(x, gamma, beta, nc.GROUPS, eps, silu)))
        _record(nc.fmt_record("groupnorm f16 three-launch", _id(shape), k, worst, emu))


# ---------------------------------------------------------------------------------------------- 2. GroupNorm from conv partials
_CONV_CACHE = {}


def _conv_inputs(B, H, W, Cin, Cout):
    """x, w and the fp32 convolution of the two (NHWC, no bias) - once per shape, shared by every k and kernel variant."""
    key = (B, H, W, Cin, Cout)
    if key not in _CONV_CACHE:
        g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cin + Cout + 7)
        x = torch.randn((B, H, W, Cin), generator=g).half()
        w = (torch.randn((Cout, 3, 3, Cin), generator=g) * (9 * Cin) ** -0.5).half()
        z = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).contiguous()
        _CONV_CACHE[key] = (x, w, z)
    return _CONV_CACHE[key]


def _biases_for_ratio(z, k, groups=nc.GROUPS):
    """conv bias [Cout] and per-image bias [B, Cout] (f16), constant inside a group, that put every (image, group) of
    z + bias + rowbias at mean / sigma = +-k (the sign alternating between groups): the level a convolution bias plus the
    time-embedding projection give conv1's output in front of norm2.  Half of the level comes from each."""
    B, H, W, Cout = z.shape
    cpg = Cout // groups
    zg = z.double().view(B, H * W, groups, cpg)
    mean, sigma = zg.mean(dim=(1, 3)), zg.var(dim=(1, 3), unbiased=False).sqrt()                  # [B, groups]
    sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(groups)], dtype=torch.float64)
    level = sign * k * sigma - mean
    bias = (0.5 * level.mean(0)).half()
    rowbias = (level - bias.double()).half()
    return bias.repeat_interleave(cpg), rowbias.repeat_interleave(cpg, dim=1)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [8, 32, 64])
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 16, 16, 64, 320), (1, 18, 13, 64, 64), (2, 32, 32, 320, 640)])
def test_groupnorm_from_conv_partials_at_large_means(hip_lib, B, H, W, Cin, Cout, k, variant):
    """CONV3X3 with a statistics workspace, then GROUPNORM with `pre_chunks` (the pattern of
    tests/test_gpu_gn_from_conv.py), on a convolution whose OUTPUT groups sit at mean / sigma k: vs the float64 GroupNorm + SiLU
    of the stored output (3e-3) and vs the three-launch path on the same tensor (2e-3); the convolution's output is
    bit-identical with and without the statistics."""
    from diffsensei_amd import ops
    from diffsensei_amd.engine import make_op
    x, w, z = _conv_inputs(B, H, W, Cin, Cout)
    b, rb = _biases_for_ratio(z, k)
    gamma, beta = nc.affine(Cout, 2)
    xd, wd, bd, rbd, gd, btd = (t.to(DEV) for t in (x, w, b, rb, gamma, beta))
    run = lambda lib, op: lib.ds_op_run(C.byref(op), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    with _option(b"conv_halo_variant", variant) as lib:
        nch = int(lib.ds_conv3x3_gn_chunks(B, H, W, Cin, Cout))
        assert nch > 0, "the halo-patch kernels take every stride-1 shape with Cin % 64 == 0"
        ws = torch.zeros(lib.ds_groupnorm_workspace_bytes(B, Cout), dtype=torch.uint8, device=DEV)
        y = torch.empty((B, H, W, Cout), dtype=torch.float16, device=DEV)
        assert run(lib, make_op("CONV3X3", i=(B, H, W, Cin, Cout, 1, 0, Cout, 0, 0), p=(xd, wd, y, bd, rbd, None, ws))) == 0, lib.ds_last_error().decode()
        plain = ops.conv3x3(xd, wd, bd, rowbias=rbd)
        out = torch.empty((B, H * W, Cout), dtype=torch.float16, device=DEV)
        assert run(lib, make_op("GROUPNORM", i=(B, H * W, Cout, 0, 32, 1, nch), f=(1e-5,), p=(y, None, out, gd, btd, ws))) == 0, lib.ds_last_error().decode()
    assert torch.equal(y, plain), "emitting the statistics changed the convolution's output"
    ys = y.cpu().view(B, H * W, Cout)
    ratio = nc.gn_ratio(ys)
    assert 0.95 * k <= ratio.min().item() and ratio.max().item() <= 1.05 * k, (k, ratio.min().item(), ratio.max().item())
    three = ops.groupnorm(y.view(B, H * W, Cout), gd, btd, 32, 1e-5, True)
    ref = nc.gn_ref(ys, gamma, beta, nc.GROUPS, 1e-5, True)
    what = f"groupnorm from conv partials {B}x{H}x{W} {Cin}->{Cout} mean/sigma {k} conv_halo_variant {variant} ({nch} chunks)"
    den = ref.abs().max().item()
    gate(what + ": vs three-launch", (out.double().cpu() - three.double().cpu()).abs().max().item() / den, nc.TOL_GN_CONV)
    gate(what + ": vs float64", nc.relmax(out, ref), nc.TOL_GN_F16)
    gate(what + ": three-launch vs float64", nc.relmax(three, ref), nc.TOL_GN_F16)


# ---------------------------------------------------------------------------------------------- 3. VAE forms
@pytest.mark.parametrize("family", [f"offset{k}" for k in nc.K_ASSERTED_BF16 + nc.K_RECORDED_BF16] + ["mixed", "flat"])
@pytest.mark.parametrize("shape", nc.VAE_SHAPES, ids=_id)
def test_groupnorm_bf16(hip_lib, shape, family):
    """ops.groupnorm_bf16, eps 1e-6, reference from the bf16-ROUNDED input.  Asserted through mean / sigma 32: bf16 carries 8
    mantissa bits, so at 64 sigma is two ulps of the data - the rounded input no longer is the distribution it is named after
    and its statistics hang on how the rounding fell; 64 is recorded.  `mixed` puts its offset group at 32 for the same reason."""
    from diffsensei_amd import ops
    B, HW, Cc = shape
    x, info = nc.gn_case(family, B, HW, Cc, torch.bfloat16, mixed_k=32)
    gamma, beta = nc.affine(Cc, 0, torch.bfloat16)
    k = nc.family_k(family)
    recorded = k in nc.K_RECORDED_BF16
    worst = emu = 0.0
    for silu in (False, True):
        ref = nc.gn_ref(x, gamma, beta, nc.GROUPS, 1e-6, silu)
        for variant in (0, 1):
            with _option(b"gn_variant", variant):
                y = ops.groupnorm_bf16(x.to(DEV), gamma.to(DEV), beta.to(DEV), nc.GROUPS, 1e-6, silu)
            e = nc.relmax(y, ref)
            what = f"groupnorm bf16 {_id(shape)} {family} silu {int(silu)} gn_variant {variant}"
            if recorded:
                worst = max(worst, e)
                emu = max(emu, nc.relmax(nc.emulate_groupnorm(x, gamma, beta, 1e-6, silu, *nc.kernel_chunks(B, HW, Cc, variant)), ref))
                continue
            gate(what, e, nc.TOL_GN_BF16)
            if info["flat"]:
                gate(what + ": |y - beta| on the constant groups", _flat_abs(y, ref, info, Cc), nc.TOL_FLAT_ABS)
    if recorded:
        _record(nc.fmt_record("groupnorm bf16 three-launch", _id(shape), k, worst, emu))


@pytest.mark.parametrize("family", [f"offset{k}" for k in nc.K_ASSERTED + nc.K_RECORDED] + ["mixed", "flat"])
@pytest.mark.parametrize("shape", nc.VAE_SHAPES, ids=_id)
def test_groupnorm_scaled_f16(hip_lib, shape, family):
    """ops.groupnorm_scaled (the decoder's scaled-f16 mode), out_scale 0.375, eps 1e-6: the f16 range and tolerance."""
    from diffsensei_amd import ops
    B, HW, Cc = shape
    x, info = nc.gn_case(family, B, HW, Cc)
    gamma, beta = nc.affine(Cc, 0)
    k = nc.family_k(family)
    recorded = k in nc.K_RECORDED
    worst = emu = 0.0
    for silu in (False, True):
        ref = nc.gn_ref(x, gamma, beta, nc.GROUPS, 1e-6, silu) * nc.OUT_SCALE
        for variant in (0, 1):
            with _option(b"gn_variant", variant):
                y = ops.groupnorm_scaled(x.to(DEV), gamma.to(DEV), beta.to(DEV), nc.GROUPS, 1e-6, silu, nc.OUT_SCALE)
            e = nc.relmax(y, ref)
            what = f"groupnorm scaled f16 {_id(shape)} {family} silu {int(silu)} gn_variant {variant}"
            if recorded:
                worst = max(worst, e)
                emu = max(emu, nc.relmax(nc.emulate_groupnorm(x, gamma, beta, 1e-6, silu, *nc.kernel_chunks(B, HW, Cc, variant),
                                                              out_scale=nc.OUT_SCALE), ref))
                continue
            gate(what, e, nc.TOL_GN_F16)
            if info["flat"]:
                gate(what + ": |y / scale - beta| on the constant groups", _flat_abs(y, ref, info, Cc) / nc.OUT_SCALE, nc.TOL_FLAT_ABS)
    if recorded:
        _record(nc.fmt_record("groupnorm scaled f16 three-launch", _id(shape), k, worst, emu))


# ---------------------------------------------------------------------------------------------- 4. LayerNorm
@pytest.mark.parametrize("family", [f"offset{k}" for k in nc.K_ASSERTED + nc.K_RECORDED] + ["spike", "flat", "tiny"])
@pytest.mark.parametrize("M,Cc", nc.LN_SHAPES)
def test_layernorm_two_pass_holds_at_every_mean(hip_lib, M, Cc, family):
    """The stand-alone kernel is two-pass (the row lives in registers): its 2e-3 holds at EVERY mean / sigma, 256 included."""
    from diffsensei_amd import ops
    x, info = nc.ln_case(family, M, Cc)
    gamma, beta = nc.affine(Cc, 1)
    ref = nc.ln_ref(x, gamma, beta, 1e-5)
    y = ops.layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-5)
    gate(f"layernorm {M}x{Cc} {family}", nc.relmax(y, ref), nc.TOL_LN)
    for row, _ in info["flat"]:
        gate(f"layernorm {M}x{Cc} flat row {row}: |y - beta|", (y[row].double().cpu() - ref[row]).abs().max().item(), nc.TOL_FLAT_ABS)


def _ln_problem(M, N, K, k, bias=True, seed=0):
    g = torch.Generator().manual_seed(nc._seed("fused", M, N, K, k, seed))
    x, _ = nc.ln_case(f"offset{k}", M, K)
    w = (torch.randn((N, K), generator=g) / math.sqrt(K)).half()
    b = (0.3 * torch.randn((N,), generator=g)).half() if bias else None
    gamma, beta = nc.affine(K, 4)
    return x, w, b, gamma, beta


def _cpu_partials(x, strip=64):
    """[K / strip, M, 2] fp32 (sum, sum of squares) per row and strip - what a producer would have emitted for x."""
    M, K = x.shape
    xs = x.float().view(M, K // strip, strip)
    return torch.stack([xs.sum(-1).t(), (xs * xs).sum(-1).t()], dim=-1).contiguous().to(DEV)


def _pack(w, b, gamma, beta):
    from diffsensei_amd.engine import pack_ln_fused
    return pack_ln_fused(w.to(DEV), None if b is None else b.to(DEV), gamma.to(DEV), beta.to(DEV))


@pytest.mark.parametrize("k", nc.K_FUSED_LN)
def test_fused_layernorm_256_kernel_plain_and_geglu(hip_lib, k):
    """Consumers on the 256 x 256 kernel, fed by the finalize launch: plain at (256, 256, 128), GEGLU at (512, 2048, 256) - the
    smallest shapes tests/test_gpu_ln_fusion.py runs those routes at."""
    from diffsensei_amd import ops
    from diffsensei_amd.engine import pack_geglu
    x, w, b, gamma, beta = _ln_problem(256, 256, 128, k, bias=False)
    gw, c2, b2 = _pack(w, None, gamma, beta)
    got = ops.gemm_ln(x.to(DEV), gw, b2, c2, ops.ln_finalize(_cpu_partials(x), 128, 1e-5))
    gate(f"fused layernorm -> linear, 256 x 256 kernel, mean/sigma {k}", nc.relmax(got, nc.ln_linear_ref(x, gamma, beta, 1e-5, w)), nc.TOL_LN_FUSED)
    M, Cc = 512, 256
    x, w, b, gamma, beta = _ln_problem(M, 8 * Cc, Cc, k)
    z = nc.ln_linear_ref(x, gamma, beta, 1e-5, w, b)
    ref = z[:, :4 * Cc].half().double() * F.gelu(z[:, 4 * Cc:].half().double())
    gw, c2, b2 = _pack(w, b, gamma, beta)
    gwp, b2p = pack_geglu(gw, b2)
    half = 4 * Cc
    c2p = torch.stack([c2[:half].reshape(-1, 64, 2), c2[half:].reshape(-1, 64, 2)], dim=1).reshape(-1, 2).contiguous()
    got = ops.gemm_ln(x.to(DEV), gwp, b2p, c2p, ops.ln_finalize(_cpu_partials(x), Cc, 1e-5), geglu=True)
    assert got.shape == (M, 4 * Cc)
    gate(f"fused layernorm -> GEGLU, 256 x 256 kernel, mean/sigma {k}", nc.relmax(got, ref), nc.TOL_LN_FUSED)


def _wide_cases():
    from tests.test_gpu_ln_fusion import _knob_cases
    return _knob_cases([(64, 128, 64, k) for k in nc.K_FUSED_LN] + [(96, 640, 1600, 32)],
                       [(272, 256, 128, k, v) for k in nc.K_FUSED_LN for v in (1, 3)])


@pytest.mark.parametrize("M,N,K,k,variant", _wide_cases())
def test_fused_layernorm_128_wide_kernels(hip_lib, M, N, K, k, variant):
    """Consumers that sum the partials of their own rows (no finalize launch): the automatic dispatch at the smallest shape
    and at the one with a second, ragged round of partial loads; the one-buffer 64-row kernel through the knob mechanism of
    tests/test_gpu_ln_fusion.py (`_knob_cases`, `_forced_route`)."""
    from diffsensei_amd import ops
    from tests.test_gpu_ln_fusion import _forced_route
    x, w, b, gamma, beta = _ln_problem(M, N, K, k)
    gw, c2, b2 = _pack(w, b, gamma, beta)
    with _forced_route(variant, M, N, K, ln_stats=4096, ln_c=4096, ln_partial=1):
        got = ops.gemm_ln_partial(x.to(DEV), gw, b2, c2, _cpu_partials(x))
    gate(f"fused layernorm -> linear, 128-wide kernels {M}x{N}x{K} gemm_variant {variant}, mean/sigma {k}",
         nc.relmax(got, nc.ln_linear_ref(x, gamma, beta, 1e-5, w, b)), nc.TOL_LN_FUSED)


@pytest.mark.parametrize("k", nc.K_FUSED_LN)
def test_fused_layernorm_t160_statistics_format(hip_lib, k):
    """gemm_t160_kernel's 160-column statistics format (entries of 64 | 64 | 32 columns) from a real producer whose OUTPUT rows
    sit at mean / sigma k (through the residual), consumed on gemm_t160_kernel and on the 128-wide kernels: (96, 320, 1920, 320),
    the smallest chain tests/test_gpu_gemm_t160.py runs."""
    from diffsensei_amd import _lib
    from diffsensei_amd.engine import pack_ln_fused
    from tests.test_gpu_gemm_t160 import _forced, _gemm_op
    lib = _lib.load()
    M, K, Cc, Nq = 96, 320, 1920, 320
    g = torch.Generator().manual_seed(160 + k)
    a = torch.randn((M, K), generator=g).half()
    wo, bo = (0.1 * torch.randn((Cc, K), generator=g) / math.sqrt(K)).half(), (0.1 * torch.randn((Cc,), generator=g)).half()
    h0, _ = nc.ln_case(f"offset{k}", M, Cc)
    wq = (torch.randn((Nq, Cc), generator=g) / math.sqrt(Cc)).half()
    gamma, beta = nc.affine(Cc, 4)
    dv = lambda t: t.to(DEV)
    h, part, name = _forced(lib, 11, lambda: _gemm_op(lib, dv(a), dv(wo), dv(bo), dv(h0), stats_strip=160))
    assert name == "gemm_t160_kernel" and part.shape == (3 * (Cc // 160), M, 2)
    hc = h.cpu()
    ratio = hc.double().mean(1).abs() / hc.double().std(1, unbiased=False)
    assert 0.85 * k <= ratio.min().item() and ratio.max().item() <= 1.15 * k, (ratio.min().item(), ratio.max().item())
    gw, c2, b2 = pack_ln_fused(dv(wq), None, dv(gamma), dv(beta))
    ref = nc.ln_linear_ref(hc, gamma, beta, 1e-5, wq)
    q_t160, _, nm = _forced(lib, 11, lambda: _gemm_op(lib, h, gw, b2, None, ln_partial=part, ln_c=c2, ln_nstrips=3 * (Cc // 160)))
    assert nm == "gemm_t160_kernel"
    with _option(b"gemm_t160", 1):
        q_wide, _, nm2 = _gemm_op(lib, h, gw, b2, None, ln_partial=part, ln_c=c2, ln_nstrips=3 * (Cc // 160))
    assert nm2.startswith("gemm_glds_kernel")
    gate(f"fused layernorm chain, 160-column statistics, consumer on gemm_t160, mean/sigma {k}", nc.relmax(q_t160, ref), nc.TOL_LN_FUSED)
    gate(f"fused layernorm chain, 160-column statistics, consumer on {nm2}, mean/sigma {k}", nc.relmax(q_wide, ref), nc.TOL_LN_FUSED)
    assert torch.equal(q_t160, q_wide), "the two consumer families sum the same partials to different bits"


@pytest.mark.parametrize("k", nc.K_FUSED_LN)
def test_fused_layernorm_swapped_forms(hip_lib, k):
    """norm1 -> attn1.to_v produced transposed: the 256 x 256 form at (3, 512, 256) and the 128-wide form at (1, 72, 128)."""
    from diffsensei_amd import ops
    for Z, N, Cc, wide in ((3, 512, 256, False), (1, 72, 128, True)):
        x, wv, _, gamma, beta = _ln_problem(Z * N, Cc, Cc, k, bias=False, seed=1)
        ref = nc.ln_ref(x, gamma, beta, 1e-5).view(Z, N, Cc)
        ref = torch.einsum("ck,znk->zcn", wv.double(), ref)
        gw, c2, _ = _pack(wv, None, gamma, beta)
        bf = (wv.double() @ beta.double()).float()
        bh = bf.half()
        cb = torch.cat([c2.cpu(), torch.stack([bh, (bf - bh.float()).half()], dim=1)], dim=1).contiguous().to(DEV)
        part = _cpu_partials(x)
        xd = x.view(Z, N, Cc).to(DEV)
        got = ops.gemm_ln_swapped_partial(gw, xd, part, cb) if wide else ops.gemm_ln_swapped(gw, xd, ops.ln_finalize(part, Cc, 1e-5), cb)
        assert got.shape == (Z, Cc, N)
        gate(f"fused layernorm -> V^T (swapped{', 128-wide kernels' if wide else ''}) Z={Z} N={N} C={Cc}, mean/sigma {k}",
             nc.relmax(got, ref), nc.TOL_LN_FUSED)


@pytest.mark.parametrize("k", [8, 16, 32])
@pytest.mark.parametrize("M,N,K,variant", [(512, 1280, 1280, 3), (1024, 256, 128, 3), (154, 1280, 1280, 0)])
def test_producer_row_statistics_at_large_means(hip_lib, M, N, K, variant, k):
    """A +residual projection whose OUTPUT rows sit at mean / sigma k (the level comes in through the residual): the partial
    sums are those of the stored f16 values, the output is bit-identical to the GEMM without statistics, and the finalize
    launch gives the mean to 1e-5 (the bounds of tests/test_gpu_ln_fusion.py::test_producer_row_statistics).  rstd to 1e-4
    relative is asserted at mean / sigma 8 and 16: var = ss / C - mean^2 in fp32 carries 0.5 (mean / sigma)^2 x a few 6e-8, which
    the emulation of tests/test_norm_cases_host.py::test_fused_layernorm_statistics_range puts at ~6e-6 | 2e-5...3e-5 |
    7e-5...1.3e-4 for 8 | 16 | 32 - at 32 the one-pass design sits AT the bound, not a factor of three inside it.  There the
    measured rstd error goes on record beside the emulation's; what it does to a consumer's output is gated by the tests
    above (5e-3)."""
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(M + N + K + k)
    x = torch.randn((M, K), generator=g).half()
    w, b = (0.1 * torch.randn((N, K), generator=g) / math.sqrt(K)).half(), (0.1 * torch.randn((N,), generator=g)).half()
    r, _ = nc.ln_case(f"offset{k}", M, N)
    dv = lambda t: t.to(DEV)
    with _option(b"gemm_variant", variant):
        y, part = ops.gemm_ln(dv(x), dv(w), dv(b), residual=dv(r), emit_stats=True)
        y0 = ops.gemm(dv(x), dv(w), dv(b), dv(r))
    assert part.shape == (N // 64, M, 2)
    assert torch.equal(y, y0), "statistics emission changed the stored output"
    yd = y.double().cpu()
    mean, var = yd.mean(1), yd.var(1, unbiased=False)
    ratio = mean.abs() / var.sqrt()      # (a 256-column row's sample sigma scatters by 1 / sqrt(512) = 4.4 %; 1024 rows reach 3.5 of those)
    assert 0.75 * k <= ratio.min().item() and ratio.max().item() <= 1.25 * k, (ratio.min().item(), ratio.max().item())
    strips = yd.view(M, N // 64, 64)
    assert torch.allclose(part[..., 0].t().double().cpu(), strips.sum(-1), rtol=1e-5, atol=1e-3)
    assert torch.allclose(part[..., 1].t().double().cpu(), (strips * strips).sum(-1), rtol=1e-5, atol=1e-3)
    st = ops.ln_finalize(part, N, 1e-5).double().cpu()
    assert torch.allclose(st[:, 0], mean, rtol=1e-5, atol=1e-5)
    e_rstd = ((st[:, 1] - torch.rsqrt(var + 1e-5)).abs() * torch.sqrt(var + 1e-5)).max().item()
    what = f"producer row statistics {M}x{N}x{K} gemm_variant {variant} mean/sigma {k}: rstd relative error"
    if k <= 16:
        gate(what, e_rstd, 1e-4)
    else:
        _, emu = nc.emulate_ln_stats(y.cpu(), 64, 1e-5)
        e_emu = ((torch.from_numpy(emu).double() - torch.rsqrt(var + 1e-5)).abs() * torch.sqrt(var + 1e-5)).max().item()
        _record(nc.fmt_record("fused layernorm rstd (relative)", f"{M}x{N}x{K} gemm_variant {variant}", k, e_rstd, e_emu))
