// Epilogue arithmetic shared by the GEMM / convolution kernels: the cross-kernel BIT contracts live here.
// Kernels that may replace one another (gemm_glds_kernel, gemm_t160_kernel, gemm_g320_kernel, gemm_pp_kernel + ln_finalize_kernel,
// the halo convolutions) promise the same bits, and the tests hold them to it with torch.equal (tests/test_gpu_ln_fusion.py,
// test_gpu_gemm_t160.py, test_gpu_gemm_g320.py, test_gpu_gn_from_conv.py, test_gpu_ops.py).  Every summation order and rounding
// point that promise rests on is spelled ONCE below; a kernel's own file keeps its loads, its tile layout and the measured reasons
// for when it asks for what.  Sizes are template arguments; nothing here branches on the calling kernel.
// (gemm_pp_kernel's epilogues keep their own spelling of the residual add and of the row statistics - v_dot2c form -: its body sits
// at the register budget and is not touched for tidiness.)
#pragma once
#include "ds_common.h"
#include "ds_kernels.h"

// ---- fused LayerNorm, consumer of PARTIAL sums (GemmParams::ln_partial) ---------------------------------------------------------
// A producer left one (sum, sum of squares) pair per row and column strip, part[entry * M + row].  THE summation order, of
// ln_finalize_kernel (norm.hip) and of every consumer epilogue: four interleaved chains - chain q adds entries q, q + 4, q + 8, ... in
// that order - then (0 + 1) + (2 + 3); fp32 addition commutes, so who holds which chain is free.  (mean, rstd) of a row:
__device__ __forceinline__ f32x2 ln_mean_rstd(float s, float q, float inv_c, float eps) {
    const float mean = s * inv_c;
    const float var = fmaxf(fmaf(-mean, mean, q * inv_c), 0.f);
    return f32x2{mean, rsqrtf(var + eps)};
}

// Row form: the lane owns tile rows row0 + 32 mi (both half-waves hold the same rows).  Half-wave lhi takes chains 2 lhi and
// 2 lhi + 1, JJ entries per chain and round; one cross-half exchange then gives (0 + 1) + (2 + 3).  Three pieces, so that a kernel
// can put its k-loop between the request and the sum.
// One round of loads, entries base .. base + 4 JJ - 1 (clamped addresses: ln_part_add masks what lies past `strips`).
template <int MI, int JJ>
__device__ __forceinline__ void ln_part_load(f32x2 (&t)[MI][2][JJ], const float* stats, int row0, int M, int base, int lhi, int strips) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int m = min(row0 + mi * 32, M - 1);
        const f32x2* part = reinterpret_cast<const f32x2*>(stats) + m;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
#pragma unroll
            for (int jj = 0; jj < JJ; ++jj) {
                const int j = base + 2 * lhi + cc + 4 * jj;
                t[mi][cc][jj] = part[(long)min(j, strips - 1) * M];
            }
    }
}
template <int MI, int JJ>
__device__ __forceinline__ void ln_part_add(float (&sa)[MI][2], float (&qa)[MI][2], const f32x2 (&t)[MI][2][JJ], int base, int lhi, int strips) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
#pragma unroll
            for (int jj = 0; jj < JJ; ++jj) {
                const bool in = base + 2 * lhi + cc + 4 * jj < strips;
                sa[mi][cc] += in ? t[mi][cc][jj][0] : 0.f;
                qa[mi][cc] += in ? t[mi][cc][jj][1] : 0.f;
            }
}
template <int MI>
__device__ __forceinline__ void ln_part_finish(const float (&sa)[MI][2], const float (&qa)[MI][2], float inv_c, float eps, float* mean, float* rstd) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const float s2 = sa[mi][0] + sa[mi][1], q2 = qa[mi][0] + qa[mi][1];
        const f32x2 mr = ln_mean_rstd(s2 + __shfl_xor(s2, 32, 64), q2 + __shfl_xor(q2, 32, 64), inv_c, eps);
        mean[mi] = mr[0];
        rstd[mi] = mr[1];
    }
}

// ---- stage 1: one accumulator value x -> the fp32 value the caller rounds to f16 ------------------------------------------------------
// plain: x + b.  Fused-LayerNorm consumer: y = rstd (x - mean c) + b' where the bias add was, with -c as the f16 (hi, lo) pair of
// GemmParams::ln_c (column n: elements 2 n, 2 n + 1).
// (Per value, not per group of four: with the loop over a lane's four columns inside the helper gemm_g320_kernel and
// gemm_t160_kernel<4, 4> came out with other register counts - profiles/epilogue_header_resource_usage.txt.)
__device__ __forceinline__ float bias_apply(float x, half_t b) { return x + (float)b; }
__device__ __forceinline__ float ln_apply(float x, float mean, float rstd, half_t c_hi, half_t c_lo, half_t b) {
    const float nc = (float)c_hi + (float)c_lo;   // -c_n
    return fmaf(fmaf(mean, nc, x), rstd, (float)b);
}

// ---- stage 2: 16-byte pieces of f16 rows ------------------------------------------------------------------------------------------
// GEGLU: f16(h * f16(gelu(g))) - h and g arrive rounded to f16 (what nn.Linear hands to GEGLU in the reference)
__device__ __forceinline__ h8 geglu8(h8 hv, h8 gv) {
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const f32x2 ge = ds_gelu_erf2(f32x2{(float)gv[e], (float)gv[e + 1]});
        o[e] = (half_t)((float)hv[e] * (float)(half_t)ge[0]);
        o[e + 1] = (half_t)((float)hv[e + 1] * (float)(half_t)ge[1]);
    }
    return o;
}

// Residual add.  f16: one v_pk_add_f16 per two values - the same number as (f16)((float)a + (float)b), which never rounds twice
// (all pairs of finite f16: tests/test_f16_add_equivalence.py); bf16 (VAE) keeps the f32 form.
template <typename T>
__device__ __forceinline__ typename Elt<T>::v8 add_residual8(typename Elt<T>::v8 v, typename Elt<T>::v8 r) {
    if constexpr (__is_same(T, half_t)) return v + r;
    else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (T)((float)v[e] + (float)r[e]);
        return v;
    }
}

// Row statistics of a fused-LayerNorm PRODUCER: (sum, sum of squares) of the 8 f16 values a lane stores, in fp32, in element order;
// then the four lanes of a quad (lane ^ 1, lane ^ 2)
__device__ __forceinline__ void sum_sq8(h8 v, float& s, float& q) {
    s = 0.f, q = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float f = (float)v[e];
        s += f;
        q = fmaf(f, f, q);
    }
}
__device__ __forceinline__ void quad_sum2(float& s, float& q) {
    s += ds_dpp_f32<0xB1>(s);
    q += ds_dpp_f32<0xB1>(q);
    s += ds_dpp_f32<0x4E>(s);
    q += ds_dpp_f32<0x4E>(q);
}
