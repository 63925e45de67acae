"""Shared cases for the normalisation-conditioning tests (tests/test_norm_cases_host.py, tests/test_gpu_norm_conditioning.py).

Every GroupNorm on the hot path and the fused LayerNorm take their variance from one-pass fp32 sums, var = E[x^2] - mean^2
(csrc/norm.hip, `gn_emit` in csrc/conv_halo.hip, the GEMM epilogues of csrc/ds_epilogue.h), which loses accuracy as
1 + (mean / sigma)^2 grows.  This module holds

  * seeded generators of f16- (or bf16-) representable inputs in the regimes where that shows,
  * float64 references computed from the ROUNDED inputs,
  * an emulation of the kernels' arithmetic (fp32 partial sums per row chunk and channel, fp32 finalize, fp32 scale/shift
    table, one rounding of the output), from which the asserted range of the GPU tests is derived on the CPU - the GPU
    thresholds do not come from the code under test.

Data families (`k` = mean / sigma of a group or row):
  offset(k)  (randn + k) * s, s per group (row) from [0.5, 4], the sign of k alternating between groups (rows)
  mixed      neighbouring groups at very different levels: k | 0 | magnitude ~2e4 | magnitude ~1e-2, repeating
  spike      O(1) data with one element of 3e4 in one group (row): squares near the f16 maximum dominate the sum of squares
  flat       exactly constant groups (rows) - 8.0, -3.0 and 11.0859375 - among random ones: the reference output there is beta
  tiny       sigma = 1e-3 around 0: eps dominates the variance
  concat     two sources, x1 at level +k and x2 at level -k, the seam inside a group
"""
import math

import numpy as np
import torch

GROUPS = 32
TOL_GN_F16 = 3e-3        # tests/test_gpu_ops.py::test_groupnorm
TOL_GN_BF16 = 2e-2       # tests/test_gpu_vae.py::test_gemm_and_groupnorm_bf16
TOL_GN_CONV = 2e-3       # tests/test_gpu_gn_from_conv.py: partial path vs three-launch path
TOL_LN = 2e-3            # tests/test_gpu_ops.py::test_layernorm (_close's default)
TOL_LN_FUSED = 5e-3      # tests/test_gpu_ln_fusion.py, offset >= 1
TOL_FLAT_ABS = 3e-3      # |y - beta| on an exactly constant group

K_ASSERTED = (0, 8, 32, 64)       # f16 GroupNorm: inside the range the arithmetic holds (see the host test)
K_RECORDED = (128, 256)           # beyond it: finite output asserted, error recorded
K_ASSERTED_BF16 = (0, 8, 32)      # bf16 carries 8 mantissa bits: at k = 64 sigma is two ulps of the data
K_RECORDED_BF16 = (64,)
K_FUSED_LN = (16, 32)

# (B, HW, C1, C2): shapes picked for the kernels' geometry, not their size
GN_SHAPES_ALL = [(2, 64, 64, 0),         # cpg 2, one chunk
                 (1, 333, 128, 64),      # concat, cpg 6, row tail
                 (2, 1024, 320, 0)]      # cpg 10: 16-byte vectors straddle groups; finalize takes its 1024-stride loop
GN_SHAPES_REST = [(1, 4096, 640, 0),     # cpg 20
                  (1, 72, 1920, 0),      # W = 240, R = 2, cpg 60
                  (1, 130, 1280, 1280)]  # two slabs with different R
# where the `concat` family puts the seam: C1 a multiple of 8 (the kernels' vector) and, where the group size allows it, not of
# the group size (C = 64: cpg 2 divides every multiple of 8 - the seam then falls between two groups)
CONCAT_SPLIT = {64: (24, 40), 192: (128, 64), 320: (136, 184)}
GN_FAMILIES_ALL = ([f"offset{k}" for k in K_ASSERTED + K_RECORDED] + ["mixed", "spike", "flat", "tiny", "concat"])
GN_FAMILIES_REST = [f"offset{k}" for k in K_ASSERTED + K_RECORDED] + ["mixed"]
VAE_SHAPES = [(2, 768, 256), (1, 100, 512)]
LN_SHAPES = [(5, 768), (37, 128), (9, 8192), (64, 5120)]
# 8.0 and -3.0: sums, mean and E[x^2] of such a group are exact in fp32 and its variance comes out as exactly 0.  11.0859375
# (1419 / 128, an f16 value with a full mantissa): the sum of squares rounds, E[x^2] - mean^2 lands a few ulps of mean^2 either
# side of zero - at some shapes below -eps - and only the clamp of the variance keeps rstd finite.
FLAT_VALUES = (8.0, -3.0, 11.0859375)
OUT_SCALE = 0.375        # groupnorm_scaled: not a power of two, so the scaled output rounds on its own


def _seed(*parts):
    h = 0
    for p in parts:
        for ch in str(p):
            h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


def _round(x, dtype):
    return x.to(dtype)


def affine(C, seed, dtype=torch.float16):
    g = torch.Generator().manual_seed(_seed("affine", C, seed))
    gamma = _round(1 + 0.2 * torch.randn(C, generator=g), dtype)
    beta = _round(0.2 * torch.randn(C, generator=g), dtype)
    return gamma, beta


def family_k(family):
    """offsetK -> K; None for the other families."""
    return int(family[6:]) if family.startswith("offset") else None


def gn_case(family, B, HW, C, dtype=torch.float16, groups=GROUPS, mixed_k=64, c1=None):
    """-> (x [B, HW, C] of `dtype`, info).  info["flat"]: list of (b, group, value) of the exactly constant groups;
    info["c1"]: where a two-source launch splits the channels (None: wherever the caller likes)."""
    cpg = C // groups
    g = torch.Generator().manual_seed(_seed(family, B, HW, C, str(dtype)))
    z = torch.randn((B, HW, groups, cpg), generator=g, dtype=torch.float64)
    s = 0.5 + 3.5 * torch.rand((B, 1, groups, 1), generator=g, dtype=torch.float64)
    sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(groups)], dtype=torch.float64).view(1, 1, groups, 1)
    info = {"flat": [], "c1": c1}
    k = family_k(family)
    if k is not None:
        x = (z + sign * k) * s
    elif family == "mixed":
        lvl = torch.arange(groups).view(1, 1, groups, 1) % 4
        big = (z * 5e3).clamp(-3e4, 3e4)
        x = torch.where(lvl == 0, (z + sign * mixed_k) * s, torch.where(lvl == 1, z * s, torch.where(lvl == 2, big, z * 1e-2)))
    elif family == "spike":
        x = z.clone()
        x[0, HW // 2, 3 % groups, cpg - 1] = 3e4
    elif family == "flat":
        x = z * s
        for b in range(B):
            for j, v in enumerate(FLAT_VALUES):
                grp = (5 + 7 * b + 11 * j) % groups
                x[b, :, grp, :] = v
                info["flat"].append((b, grp, v))
    elif family == "tiny":
        x = z * 1e-3
    elif family == "concat":
        c1 = CONCAT_SPLIT[C][0]
        info["c1"] = c1
        ch = torch.arange(C).view(1, 1, groups, cpg)
        x = (z + torch.where(ch < c1, 64.0, -64.0)) * s
    else:
        raise ValueError(family)
    return _round(x.reshape(B, HW, C), dtype), info


def gn_ref(x, gamma, beta, groups, eps, silu):
    """float64 GroupNorm (+SiLU) of the rounded input: [B, HW, C] -> float64 [B, HW, C]."""
    B, HW, C = x.shape
    xg = x.double().view(B, HW, groups, C // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).view(B, HW, C) * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if silu else y


def gn_ratio(x, groups=GROUPS):
    """|mean| / sigma per (image, group) of a [B, HW, C] tensor, float64."""
    B, HW, C = x.shape
    xg = x.double().view(B, HW, groups, C // groups)
    return xg.mean(dim=(1, 3)).abs() / xg.var(dim=(1, 3), unbiased=False).sqrt().clamp_min(1e-300)


def ln_case(family, M, C, dtype=torch.float16):
    """-> (x [M, C], info); the LayerNorm twins of the GroupNorm families, one row = one group."""
    g = torch.Generator().manual_seed(_seed("ln", family, M, C))
    z = torch.randn((M, C), generator=g, dtype=torch.float64)
    s = 0.5 + 3.5 * torch.rand((M, 1), generator=g, dtype=torch.float64)
    sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(M)], dtype=torch.float64).view(M, 1)
    info = {"flat": []}
    k = family_k(family)
    if k is not None:
        x = (z + sign * k) * s
    elif family == "spike":
        x = z.clone()
        x[M // 2, C - 3] = 3e4
        x[0, 0] = -3e4
    elif family == "flat":
        x = z * s
        for j, v in enumerate(FLAT_VALUES):
            row = (1 + 2 * j) % M
            x[row] = v
            info["flat"].append((row, v))
    elif family == "tiny":
        x = z * 1e-3
    else:
        raise ValueError(family)
    return _round(x, dtype), info


def ln_ref(x, gamma, beta, eps):
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def ln_linear_ref(x, gamma, beta, eps, w, bias=None):
    y = ln_ref(x, gamma, beta, eps) @ w.double().t()
    return y if bias is None else y + bias.double()


def relmax(got, ref):
    """max |got - ref| / max |ref|, in float64 on the CPU; `got` must be finite and of ref's shape."""
    got, ref = got.detach().double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "non-finite output"
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------------------------
# Emulation of the one-pass arithmetic.  numpy float32 throughout: every +, * below rounds to fp32 as the kernels' do.
F32 = np.float32


def _round_out(y32, dtype):
    if dtype == torch.float16:
        return y32.astype(np.float16).astype(np.float64)
    assert dtype == torch.bfloat16
    bits = np.ascontiguousarray(y32, dtype=F32).view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16          # round to nearest even on the upper 16 bits
    return bits.astype(np.uint32).view(F32).astype(np.float64)


def _seq_sum(a, axis):
    """fp32 sum along `axis` in index order (what one lane's accumulator does)."""
    a = np.moveaxis(a, axis, 0)
    acc = np.zeros(a.shape[1:], dtype=F32)
    for i in range(a.shape[0]):
        acc = acc + a[i]
    return acc


def _tree_sum(a):
    """fp32 butterfly over the last axis (a power of two): wavefront shuffles, then the waves' partials in pairs."""
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def emulate_gn_partials(x, nchunks, lanes_per_column):
    """x [B, HW, C] (torch, f16 / bf16) -> (s, ss) fp32 [B, nchunks, C]: gn_stats_kernel's order - a chunk's rows are dealt
    round-robin to `lanes_per_column` lanes (R of gn_geom), each lane adds four rows at a time as (f0 + f1) + (f2 + f3) and
    fma(f0, f0, f1 * f1) + fma(f2, f2, f3 * f3) (squares of 11-bit mantissas are exact in fp32, so each fma is one rounding of
    f0^2 + f1^2), then the lanes are added in order.  Rows are padded with zeros to whole groups of four per lane: adding an
    exact zero changes no sum, it only moves a tail row from the kernel's one-at-a-time loop into a group of four."""
    B, HW, C = x.shape
    R = max(1, lanes_per_column)
    rpc = -(-HW // nchunks)
    J = -(-rpc // (4 * R)) * 4
    xp = np.zeros((B, nchunks * rpc, C), dtype=F32)
    xp[:, :HW] = x.float().numpy()
    xp = xp.reshape(B, nchunks, rpc, C)
    pad = np.zeros((B, nchunks, J * R, C), dtype=F32)
    pad[:, :, :rpc] = xp
    v = pad.reshape(B, nchunks, J // 4, 4, R, C)
    f0, f1, f2, f3 = v[:, :, :, 0], v[:, :, :, 1], v[:, :, :, 2], v[:, :, :, 3]
    s4 = (f0 + f1) + (f2 + f3)
    q4 = (f0 * f0 + f1 * f1) + (f2 * f2 + f3 * f3)
    s = _seq_sum(_seq_sum(s4, 2), 2)          # over a lane's groups of four, then over the lanes
    ss = _seq_sum(_seq_sum(q4, 2), 2)
    return s, ss


def emulate_tile_partials(y, H, W, th=8, tw=16):
    """y [B, H*W, C] -> (s, ss) fp32 [B, tiles, C]: the convolution epilogue's partials (gn_emit): one pair per channel and
    th x tw pixel tile; inside a tile a lane adds its 8 rows in order, four lanes meet in two shuffles, four waves in pairs."""
    B, HW, C = y.shape
    ty, tx = -(-H // th), -(-W // tw)
    yp = np.zeros((B, ty * th, tx * tw, C), dtype=F32)
    yp[:, :H, :W] = y.float().numpy().reshape(B, H, W, C)
    t = yp.reshape(B, ty, th, tx, tw, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, ty * tx, th * tw, C)
    # pixel p of the tile: thread (p & 15) + 16 * j for j < 8, lanes 16 apart in a wave, four waves
    v = t.reshape(B, ty * tx, 8, 16, C)
    s = _tree_sum(np.moveaxis(_seq_sum(v, 2), 2, -1))
    ss = _tree_sum(np.moveaxis(_seq_sum(v * v, 2), 2, -1))
    return s, ss


def emulate_gn_finalize(s, ss, HW, gamma, beta, groups, eps, contract=0, clamp=True):
    """(s, ss) fp32 [B, nchunks, C] -> (tabA, tabS) fp32 [B, C]: gn_finalize_kernel - 256 lanes walk a group's
    nchunks x cpg pairs four at a time, butterfly, mean = s / n, var = max(ss / n - mean^2, 0), a = rstd gamma,
    shift = beta - mean a.  `contract`: how the compiler may fuse var's multiply-subtract (0: not at all,
    1: fma(-mean, mean, ss / n) - what hipcc makes of it under -ffp-contract=fast, 2: fma(ss, 1 / n, -(mean * mean))).
    `clamp=False`: the same without the max(..., 0), to show which cases need it."""
    B, nch, C = s.shape
    cpg = C // groups
    items = nch * cpg
    J = -(-items // 1024)

    def total(p):
        a = p.reshape(B, nch, groups, cpg).transpose(0, 2, 1, 3).reshape(B, groups, items)
        pad = np.zeros((B, groups, J * 1024), dtype=F32)
        pad[..., :items] = a
        q = pad.reshape(B, groups, J, 4, 256)
        return _tree_sum(_seq_sum((q[:, :, :, 0] + q[:, :, :, 1]) + (q[:, :, :, 2] + q[:, :, :, 3]), 2))

    S, SS = total(s), total(ss)
    inv_n = F32(1.0) / (F32(cpg) * F32(HW))
    mean = S * inv_n
    if contract == 0:
        var = SS * inv_n - mean * mean
    elif contract == 1:
        var = (-(mean.astype(np.float64) ** 2) + (SS * inv_n).astype(np.float64)).astype(F32)
    else:
        var = (SS.astype(np.float64) * np.float64(inv_n) - (mean * mean).astype(np.float64)).astype(F32)
    if clamp:
        var = np.maximum(var, F32(0))
    with np.errstate(invalid="ignore"):
        rstd = (1.0 / np.sqrt((var + F32(eps)).astype(np.float64))).astype(F32)
    gam = np.repeat(rstd, cpg, axis=1) * gamma.float().numpy()[None]
    tabA = gam.astype(F32)
    tabS = beta.float().numpy()[None] - np.repeat(mean, cpg, axis=1) * tabA
    return tabA, tabS.astype(F32), mean, rstd


def emulate_gn_apply(x, tabA, tabS, silu, out_scale=1.0):
    """y = silu(fma(a, x, s)) * out_scale, rounded once to x's type -> float64 [B, HW, C]."""
    xf = x.float().numpy().astype(np.float64)
    f = (tabA[:, None].astype(np.float64) * xf + tabS[:, None].astype(np.float64)).astype(F32)
    if silu:
        f = (f.astype(np.float64) / (1.0 + np.exp(-f.astype(np.float64)))).astype(F32)
    return _round_out(f * F32(out_scale), x.dtype)


def kernel_chunks(B, HW, C, variant=0):
    """(row chunks, lanes per channel column) of ds_launch_groupnorm / gn_geom for a shape - restated from csrc/norm.hip so
    the emulation can be run at the launch's own geometry; the host test also runs it at other chunk counts."""
    nch = min(128, max(1, (HW + 7) // 8))
    threads = 256
    nslab = ((C // 8) + 255) // 256
    if variant != 1:
        want = (1024 + B * nslab - 1) // (B * nslab)
        nch = min(nch, max(want, (HW + 63) // 64))
        threads = 512
    return nch, max(1, threads // min(C // 8, 256))


def emulate_groupnorm(x, gamma, beta, eps, silu, nchunks, lanes=2, groups=GROUPS, contract=1, out_scale=1.0):
    """The three launches end to end -> float64 [B, HW, C] (values representable in x's type)."""
    s, ss = emulate_gn_partials(x, nchunks, lanes)
    tabA, tabS, _, _ = emulate_gn_finalize(s, ss, x.shape[1], gamma, beta, groups, eps, contract)
    return torch.from_numpy(emulate_gn_apply(x, tabA, tabS, silu, out_scale))


def emulate_ln_stats(x, strip=64, eps=1e-5):
    """x [M, C] f16 -> (mean, rstd) fp32 [M]: the fused LayerNorm's statistics - fp32 (sum, sum of squares) per row and
    `strip` columns (a lane adds its 8 adjacent values in order, the strip's lanes meet in a butterfly - the producers'
    epilogues, csrc/gemm_pp.hip), then four lanes per row take every fourth strip and meet in two shuffles
    (ln_finalize_kernel / ds_epilogue.h)."""
    M, C = x.shape
    xs = x.float().numpy().reshape(M, C // strip, strip // 8, 8)
    ps, pq = _tree_sum(_seq_sum(xs, 3)), _tree_sum(_seq_sum(xs * xs, 3))
    n = -(-ps.shape[1] // 4) * 4
    pad = np.zeros((2, M, n), dtype=F32)
    pad[0, :, :ps.shape[1]], pad[1, :, :ps.shape[1]] = ps, pq
    lanes = _seq_sum(pad.reshape(2, M, n // 4, 4), 2)
    tot = (lanes[..., 0] + lanes[..., 1]) + (lanes[..., 2] + lanes[..., 3])
    inv_c = F32(1.0) / F32(C)
    mean = tot[0] * inv_c
    var = np.maximum((-(mean.astype(np.float64) ** 2) + (tot[1] * inv_c).astype(np.float64)).astype(F32), F32(0))   # fmaf(-mean, mean, q / C)
    return mean,(1.0 / np.sqrt((var + F32(eps)).astype(np.float64))).astype(F32)


def fmt_record(path, what, k, measured, emulated=None):
    tail = "" if emulated is None else f"  emulated {emulated:.2e}"
    return f"{path:<34} {what:<44} mean/sigma {k:>4}  measured {measured:.2e}{tail}"
