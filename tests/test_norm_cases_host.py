"""CPU: the shared normalisation cases of tests/_norm_cases.py - (a) their float64 references agree with torch's own
float64 GroupNorm / LayerNorm (this tests the helper, not the kernels); (b) an emulation of the kernels' one-pass arithmetic
(fp32 partial sums per row chunk and channel, fp32 finalize, fp32 scale/shift table, one rounding of the output) stays at or
below ONE THIRD of the tolerance the GPU tests assert, on every asserted case and at several chunk geometries - the asserted
range of tests/test_gpu_norm_conditioning.py is what the design reaches, derived here and not from the kernels' output;
(c) the same emulation beyond the range (mean / sigma 128, 256; bf16 64) is printed for the record (pytest -s).

Where the emulation says the design can NOT reach a bound the range is cut there, and the test says so:
test_fused_layernorm_statistics_range."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _norm_cases as nc

GN_CASES = ([(s, f) for s in nc.GN_SHAPES_ALL for f in nc.GN_FAMILIES_ALL] +
            [(s, f) for s in nc.GN_SHAPES_REST for f in nc.GN_FAMILIES_REST])
_id = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _geometries(B, HW, C):
    """Chunk geometries the emulation is run at: the launch's own under both gn_variant values, and half / twice the chunks of
    the default (what a change of the chunking rule would do)."""
    n0, l0 = nc.kernel_chunks(B, HW, C, 0)
    n1, l1 = nc.kernel_chunks(B, HW, C, 1)
    return {"gn_variant0": (n0, l0), "gn_variant1": (n1, l1), "half": (max(1, n0 // 2), l0), "twice": (min(HW, 2 * n0), l0)}


def _flat_abs(y, ref, info, C):
    cpg = C // nc.GROUPS
    return max([(y[b, :, g * cpg:(g + 1) * cpg] - ref[b, :, g * cpg:(g + 1) * cpg]).abs().max().item() for b, g, _ in info["flat"]],
               default=0.0)


@pytest.mark.parametrize("shape,family", GN_CASES, ids=_id)
def test_groupnorm_reference_is_torch_float64(shape, family):
    B, HW, C1, C2 = shape
    C = C1 + C2
    x, info = nc.gn_case(family, B, HW, C)
    assert x.dtype == torch.float16 and torch.isfinite(x).all()
    gamma, beta = nc.affine(C, 0)
    for eps in (1e-5, 1e-6):
        want = F.group_norm(x.double().permute(0, 2, 1), nc.GROUPS, gamma.double(), beta.double(), eps).permute(0, 2, 1)
        assert nc.relmax(nc.gn_ref(x, gamma, beta, nc.GROUPS, eps, False), want) <= 1e-9
        assert nc.relmax(nc.gn_ref(x, gamma, beta, nc.GROUPS, eps, True), F.silu(want)) <= 1e-9
    k = nc.family_k(family)
    if k:        # the generator delivers the ratio it is named after, after rounding to f16 (the smallest group has 128
        r = nc.gn_ratio(x)      # elements: its sample sigma scatters by 1 / sqrt(2 * 128) = 6 %, four of those over 64 groups)
        assert 0.75 * k <= r.min().item() and r.max().item() <= 1.25 * k, (r.min().item(), r.max().item())
    if family == "flat":
        ref = nc.gn_ref(x, gamma, beta, nc.GROUPS, 1e-6, False)
        cpg = C // nc.GROUPS
        for b, g, v in info["flat"]:
            assert bool((x[b, :, g * cpg:(g + 1) * cpg] == v).all())
            assert torch.equal(ref[b, :, g * cpg:(g + 1) * cpg], beta.double()[g * cpg:(g + 1) * cpg].expand(HW, cpg))
    if family == "concat":
        assert info["c1"] % 8 == 0 and (info["c1"] % (C // nc.GROUPS) != 0 or C // nc.GROUPS == 2)


@pytest.mark.parametrize("family", ["offset0", "offset32", "offset256", "spike", "flat", "tiny"])
@pytest.mark.parametrize("M,C", nc.LN_SHAPES)
def test_layernorm_reference_is_torch_float64(M, C, family):
    x, info = nc.ln_case(family, M, C)
    assert torch.isfinite(x).all()
    gamma, beta = nc.affine(C, 1)
    want = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    assert nc.relmax(nc.ln_ref(x, gamma, beta, 1e-5), want) <= 1e-9
    g = torch.Generator().manual_seed(C)
    w, b = torch.randn((24, C), generator=g).half(), torch.randn((24,), generator=g).half()
    assert nc.relmax(nc.ln_linear_ref(x, gamma, beta, 1e-5, w, b), F.linear(want, w.double(), b.double())) <= 1e-9
    for row, _ in info["flat"]:
        assert torch.equal(nc.ln_ref(x, gamma, beta, 1e-5)[row], beta.double())


@pytest.mark.parametrize("geometry", ["gn_variant0", "gn_variant1", "half", "twice"])
@pytest.mark.parametrize("shape,family", GN_CASES, ids=_id)
def test_groupnorm_f16_emulation_within_a_third(shape, family, geometry):
    """Asserted cases: emulated error <= TOL_GN_F16 / 3 (and |y - beta| <= TOL_FLAT_ABS / 3 on the constant groups), for both
    eps, with and without SiLU, and for each way the compiler may contract var = ss / n - mean^2.  Recorded cases: printed."""
    B, HW, C1, C2 = shape
    C = C1 + C2
    x, info = nc.gn_case(family, B, HW, C)
    gamma, beta = nc.affine(C, 0)
    nch, lanes = _geometries(B, HW, C)[geometry]
    s, ss = nc.emulate_gn_partials(x, nch, lanes)
    k = nc.family_k(family)
    recorded = k in nc.K_RECORDED
    worst = worst_flat = 0.0
    for eps in (1e-5, 1e-6):
        ref = {silu: nc.gn_ref(x, gamma, beta, nc.GROUPS, eps, silu) for silu in (False, True)}
        for contract in (0, 1, 2):
            tabA, tabS, _, _ = nc.emulate_gn_finalize(s, ss, HW, gamma, beta, nc.GROUPS, eps, contract)
            for silu in (False, True):
                y = torch.from_numpy(nc.emulate_gn_apply(x, tabA, tabS, silu))
                worst = max(worst, nc.relmax(y, ref[silu]))
                worst_flat = max(worst_flat, _flat_abs(y, ref[silu], info, C))
    print(f"[emulated] groupnorm f16 {_id(shape)} {family} {geometry} ({nch} chunks x {lanes} lanes): {worst:.2e}"
          + (f", constant groups |y - beta| {worst_flat:.2e}" if info["flat"] else "") + ("  (recorded only)" if recorded else ""))
    if not recorded:
        assert worst <= nc.TOL_GN_F16 / 3, worst
        assert worst_flat <= nc.TOL_FLAT_ABS / 3, worst_flat


@pytest.mark.parametrize("family", [f"offset{k}" for k in nc.K_ASSERTED_BF16 + nc.K_RECORDED_BF16] + ["mixed", "flat"])
@pytest.mark.parametrize("shape", nc.VAE_SHAPES, ids=_id)
def test_groupnorm_vae_forms_emulation_within_a_third(shape, family):
    """bf16 (reference from the bf16-rounded input; asserted through mean / sigma 32 - bf16 carries 8 mantissa bits, at 64
    sigma is two ulps of the data and the rounded input no longer has the ratio it is named after) and the scaled f16 form
    (out_scale 0.375: one more fp32 multiply before the rounding)."""
    B, HW, C = shape
    k = nc.family_k(family)
    for dtype, tol, recorded in ((torch.bfloat16, nc.TOL_GN_BF16, k in nc.K_RECORDED_BF16), (torch.float16, nc.TOL_GN_F16, False)):
        x, info = nc.gn_case(family, B, HW, C, dtype, mixed_k=32 if dtype == torch.bfloat16 else 64)
        gamma, beta = nc.affine(C, 0, dtype)
        scale = 1.0 if dtype == torch.bfloat16 else nc.OUT_SCALE
        worst = worst_flat = 0.0
        for variant in (0, 1):
            nch, lanes = nc.kernel_chunks(B, HW, C, variant)
            for silu in (False, True):
                y = nc.emulate_groupnorm(x, gamma, beta, 1e-6, silu, nch, lanes, out_scale=scale)
                ref = nc.gn_ref(x, gamma, beta, nc.GROUPS, 1e-6, silu) * scale
                worst = max(worst, nc.relmax(y, ref))
                worst_flat = max(worst_flat, _flat_abs(y, ref, info, C) / scale)
        print(f"[emulated] groupnorm {'bf16' if dtype == torch.bfloat16 else 'f16 scaled'} {_id(shape)} {family}: {worst:.2e}"
              + (f", constant groups {worst_flat:.2e}" if info["flat"] else "") + ("  (recorded only)" if recorded else ""))
        if not recorded:
            assert worst <= tol / 3, worst
            assert worst_flat <= nc.TOL_FLAT_ABS / 3, worst_flat


@pytest.mark.parametrize("k", [8, 32, 64])
@pytest.mark.parametrize("B,H,W,C", [(2, 16, 16, 320), (1, 18, 13, 64), (2, 32, 32, 640)])
def test_conv_partial_emulation_within_a_third(B, H, W, C, k):
    """The convolution epilogue's statistics (one partial pair per 8 x 16-pixel tile and channel) on a tensor whose groups sit
    at mean / sigma k: vs float64 <= TOL_GN_F16 / 3.  Vs the three-launch arithmetic on the same tensor the figure is a
    difference of two f16 tensors and comes in steps of one f16 ulp of the element that differs - for the largest output
    2^-11 ... 2^-10 of max|ref|, i.e. 4.9e-4 ... 9.8e-4 - so a third of TOL_GN_CONV (6.7e-4) is not a level that comparison can
    resolve (emulated at mean / sigma 64: 7.9e-4 on the first shape, one ulp).  What is asserted instead: the two paths never
    differ by more than ONE ulp of the largest output, 2^-10 - half of TOL_GN_CONV."""
    y, _ = nc.gn_case(f"offset{k}", B, H * W, C)
    gamma, beta = nc.affine(C, 2)
    s, ss = nc.emulate_tile_partials(y, H, W)
    tabA, tabS, _, _ = nc.emulate_gn_finalize(s, ss, H * W, gamma, beta, nc.GROUPS, 1e-5)
    got = torch.from_numpy(nc.emulate_gn_apply(y, tabA, tabS, True))
    ref = nc.gn_ref(y, gamma, beta, nc.GROUPS, 1e-5, True)
    three = nc.emulate_groupnorm(y, gamma, beta, 1e-5, True, *nc.kernel_chunks(B, H * W, C))
    e_ref, e_three = nc.relmax(got, ref), nc.relmax(got, three)
    print(f"[emulated] groupnorm from {s.shape[1]} tile partials {B}x{H}x{W}x{C} mean/sigma {k}: vs float64 {e_ref:.2e}, vs three-launch {e_three:.2e}")
    assert e_ref <= nc.TOL_GN_F16 / 3 and e_three <= 2.0 ** -10 <= nc.TOL_GN_CONV / 2, (e_ref, e_three)


def _emulate_fused_consumer(x, w, bias, gamma, beta, eps):
    """y = rstd (x gw^T - mean c) + b' with the statistics of emulate_ln_stats; the contraction itself in float64 rounded to
    fp32 (its accumulation error is far below the f16 rounding of the output), -c as the f16 (hi, lo) pair the kernels read."""
    from diffsensei_amd.engine import pack_ln_fused
    gw, c2, b2 = pack_ln_fused(w, bias, gamma, beta)
    mean, rstd = nc.emulate_ln_stats(x, 64, eps)
    acc = (x.double() @ gw.double().t()).numpy().astype(nc.F32)
    negc = (c2[:, 0].double() + c2[:, 1].double()).numpy().astype(nc.F32)
    y = rstd[:, None] * (acc + mean[:, None] * negc[None]) + b2.float().numpy()[None]
    return torch.from_numpy(y.astype(np.float16).astype(np.float64))


@pytest.mark.parametrize("M,C", [(256, 128), (64, 640), (256, 1280), (96, 1600)])
def test_fused_layernorm_statistics_range(M, C):
    """The fused LayerNorm's row statistics are fp32 sums of 64-column strips, var = fma(-mean, mean, ss / C).
    * consumer output vs float64 LayerNorm -> Linear: <= TOL_LN_FUSED / 3 through mean / sigma 32 (asserted on the GPU at 16, 32);
    * the row-statistics bounds of test_gpu_ln_fusion.py::test_producer_row_statistics (mean 1e-5, rstd 1e-4 relative) are
      reachable with a factor of three in hand through mean / sigma 16: the emulated rstd error is ~6e-6 at 8, 2e-5...3e-5 at 16
      and 7e-5...1.3e-4 at 32, i.e. ~0.5 (mean / sigma)^2 x a few fp32 ulps of ss / C - at 32 that IS the bound (past it at
      C = 1280).  The GPU test therefore asserts rstd at 8 and 16 and records it at 32 (the mean, the partial sums and the
      bit-identity of the output are asserted at all three)."""
    gamma, beta = nc.affine(C, 3)
    g = torch.Generator().manual_seed(M + C)
    w, b = (torch.randn((64, C), generator=g) / C ** 0.5).half(), (0.3 * torch.randn((64,), generator=g)).half()
    for k in (0, 8) + nc.K_FUSED_LN + (64,):
        x, _ = nc.ln_case(f"offset{k}", M, C)
        mean, rstd = nc.emulate_ln_stats(x, 64, 1e-5)
        xd = x.double()
        m64, r64 = xd.mean(1), 1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)
        e_mean = ((torch.from_numpy(mean).double() - m64).abs() / (1e-5 + 1e-5 * m64.abs())).max().item()
        e_rstd = ((torch.from_numpy(rstd).double() - r64).abs() / r64).max().item()
        e_out = nc.relmax(_emulate_fused_consumer(x, w, b, gamma, beta, 1e-5), nc.ln_linear_ref(x, gamma, beta, 1e-5, w, b))
        print(f"[emulated] fused layernorm M={M} C={C} mean/sigma {k}: mean err / bound {e_mean:.2f}, rstd rel {e_rstd:.2e}, consumer {e_out:.2e}")
        if k <= 32:
            assert e_out <= nc.TOL_LN_FUSED / 3, e_out
            assert e_mean <= 1.0, e_mean
        if k <= 16:
            assert e_rstd <= 1e-4 / 3, e_rstd
        if k == 32:
            assert e_rstd > 1e-4 / 3, "the design reaches rstd 1e-4 at mean / sigma 32 with room after all: assert it on the GPU"


def test_flat_family_needs_the_variance_clamp():
    """What `flat` is there for, shown on the emulation: with var = fma(-mean, mean, ss / n) (the form the compiler emits for
    gn_finalize_kernel) the groups at 8.0 and -3.0 have a variance of exactly 0 - every sum is exact - so they pin
    y = beta but never reach the clamp; the group at 11.0859375 comes out a few ulps of mean^2 BELOW zero at (1, 333, 128 + 64)
    and (1, 100, 512): without max(var, 0), rstd = rsqrt(var + 1e-6) is NaN there (asserted on the GPU by the eps 1e-6
    cases of those shapes: three-launch f16, scaled f16).  `tiny` (sigma 1e-3, var 1e-6) stays positive: it checks that eps
    enters the variance at the right scale, not the clamp."""
    needs = {}
    for B, HW, C in [(1, 333, 192), (1, 100, 512), (2, 1024, 320)]:
        x, info = nc.gn_case("flat", B, HW, C)
        gamma, beta = nc.affine(C, 0)
        s, ss = nc.emulate_gn_partials(x, *nc.kernel_chunks(B, HW, C))
        _, _, _, rstd = nc.emulate_gn_finalize(s, ss, HW, gamma, beta, nc.GROUPS, 1e-6, contract=1, clamp=False)
        _, _, _, clamped = nc.emulate_gn_finalize(s, ss, HW, gamma, beta, nc.GROUPS, 1e-6, contract=1)
        assert np.isfinite(clamped).all()
        for b, g, v in info["flat"]:
            if v in (8.0, -3.0):
                assert clamped[b, g] == np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-6)))), (B, HW, C, v)   # var == 0 exactly
        needs[(B, HW, C)] = [v for b, g, v in info["flat"] if not np.isfinite(rstd[b, g])]
        x, _ = nc.gn_case("tiny", B, HW, C)
        s, ss = nc.emulate_gn_partials(x, *nc.kernel_chunks(B, HW, C))
        _, _, _, rstd = nc.emulate_gn_finalize(s, ss, HW, gamma, beta, nc.GROUPS, 1e-6, contract=1, clamp=False)
        assert np.isfinite(rstd).all()
    assert needs[(1, 333, 192)] == [11.0859375] and needs[(1, 100, 512)] == [11.0859375], needs
