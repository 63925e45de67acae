// MLLM pre-pass: LLaMA greedy decoding with a KV cache for gfx950.
// Reference: src/models/mllm/seed_x.py:90-171 (generate), src/models/mllm/modeling_llama_xformer.py:97-314 (rotary
// embedding, attention with past_key_value, MLP, decoder layer), src/models/mllm/generation.py:19-30 (logits processor).
//
// Batch-1 greedy decoding streams every weight once per token: the path is HBM-bound (13 B parameters = 26 GB per
// token), so the kernels below are wide vector loads + fp32 dot products on the VALU, not MFMA tiles.  The same kernels
// take up to 16 rows (causal inside the chunk), which is how the attention of the prompt runs; the prompt's projections
// go through the MFMA GEMMs (mllm.py: _prompt_mfma; 16-row passes of these kernels remain as an A/B path).  The token
// loop is a static launch list whose only varying inputs live in a small device-side state block, so it replays as a
// hipGraph:
//     state[0] = tokens in the KV cache   state[1] = tokens generated   state[2] = finished   state[3] = current token
//     state[4] = max_new_tokens of this call   state[5] = eos token id                      (int32[8], two spare)
//
// HBM layout: weights [N,K] row-major fp16 (one wavefront streams one row); the RMSNorm gains are folded into the
// following projection on the host (W' = W diag(g)), so a projection only needs the row's 1/rms, which every wavefront
// recomputes from the x it reads anyway; KV cache [T_max, kv_heads*D] fp16 per layer, keys stored rotated.
// int8 weight-only decoding (W8A16): the projection weights may instead be int8 [N,K] with one fp32 scale per row; the
// GEMV / gemm16 kernels are templated on the weight element type (WLoad below) and share every line but the unpack and the
// row scale in the epilogue.  Activations, KV cache, embedding, lm_head and gains stay fp16.
// MXFP4 weight-only decoding (W4A16): the projection weights may also be packed e2m1 [N,K/2] (element 2i in the low nibble)
// with one biased E8M0 exponent per 32-element block ([N,K/32], values 114..127) and one fp32 scale per row; a 16-byte load
// is one block, unpacked by v_cvt_scalef32_pk_f16_fp4 with the block's scale - the third WLoad specialisation below.
#include <type_traits>

#include "ds_common.h"
#include "ds_kernels.h"

namespace {

__device__ __forceinline__ float dot8(const h8 a, const h8 b, float acc) {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        h2 x = {a[e], a[e + 1]}, y = {b[e], b[e + 1]};
        acc = __builtin_amdgcn_fdot2(x, y, acc, false);
    }
    return acc;
}

// LlamaRMSNorm output for 8 elements, with the reference's rounding points (modeling_llama_xformer.py:77-82):
// hidden = x(fp32) * r -> .to(fp16) -> weight(fp16) * hidden -> fp16
__device__ __forceinline__ h8 rms_gain8(const h8& x, const h8& g, float r) {
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)g[e] * (float)(half_t)((float)x[e] * r));
    return o;
}

// One 16-byte weight load per lane and what it holds: 8 fp16 weights, or 16 int8 weights (W8A16: int8 weights with one
// fp32 scale per output row, fp16 activations).  `halves` turns a load into NH fragments of 8 halves; int8 -> f16 is exact
// (|q| <= 127).  Per 32-bit word: q ^ 0x80 = q + 128 as an unsigned byte, v_perm_b32 puts it under the exponent byte 0x64
// (f16 0x6400 + u = 1024 + u, ulp 1 there), a packed subtract of 1152 leaves q: 5 VALU instructions per 4 weights.
// MXFP4: 32 e2m1 weights = one OCP MX block, so a load never mixes two block scales.  The block's biased E8M0 exponent e
// (114..127) becomes the f32 2^(e-127) = bit_cast(e << 23), and one v_cvt_scalef32_pk_f16_fp4 per byte gives f16(e2m1 * scale)
// for its two nibbles (low nibble = the even element; the byte of the word is the builtin's last argument): 16 conversions
// + one shift per 32 weights.  Every product e2m1 * 2^(e-127) is a normal f16 (>= 2^-14), so the conversion is exact.
// Common to the three: SH = log2(weights per WT storage unit) turns an element index into a WT index; ROW_SCALE = the sum is
// multiplied by p.w_scale[n] in the epilogue; BLOCK_SCALE = a load comes with its p.w_exp byte; xpos = where x[k] (k % 8 == 0)
// sits in the pipelined kernel's LDS copy of a row.
typedef int i32x4 __attribute__((ext_vector_type(4)));
struct fp4x2_t { uint8_t b; };   // two e2m1 weights
template <typename WT>
struct WLoad;
template <>
struct WLoad<half_t> {
    typedef h8 raw;
    static constexpr int E = 8, NH = 1, SH = 0;
    static constexpr bool ROW_SCALE = false, BLOCK_SCALE = false;
    static constexpr int PIPE_WAVES = 1;   // llm_gemv_pipe_kernel, M = 1: wavefronts per SIMD asked of the compiler (1 = no request)
    static constexpr int PIPE_BLOCKS = 5;  // llm_gemv_pipe_kernel: resident blocks per CU by registers (launch_gemv_stream)
    static __device__ __forceinline__ int xpos(int k, int) { return k; }
    static __device__ __forceinline__ void halves(const raw& r, unsigned, h8 (&o)[1]) { o[0] = r; }
};
template <>
struct WLoad<int8_t> {
    typedef i32x4 raw;
    static constexpr int E = 16, NH = 2, SH = 0;
    static constexpr bool ROW_SCALE = true, BLOCK_SCALE = false;
    static constexpr int PIPE_WAVES = 5;   // the unpack temporaries must not cost the fifth resident block (launch_gemv_stream)
    static constexpr int PIPE_BLOCKS = 5;
    static __device__ __forceinline__ int xpos(int k, int) { return k; }
    static __device__ __forceinline__ void halves(const raw& r, unsigned, h8 (&o)[2]) {
        const h2 bias = {(half_t)1152.0f, (half_t)1152.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned u = (unsigned)r[j] ^ 0x80808080u;
            const h2 lo = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, u, 0x04010400u)) - bias;
            const h2 hi = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, u, 0x04030402u)) - bias;
            h8& d = o[j >> 1];
            const int e = 4 * (j & 1);
            d[e] = lo[0];
            d[e + 1] = lo[1];
            d[e + 2] = hi[0];
            d[e + 3] = hi[1];
        }
    }
};
template <>
struct WLoad<fp4x2_t> {
    typedef i32x4 raw;
    static constexpr int E = 32, NH = 4, SH = 1;
    static constexpr bool ROW_SCALE = true, BLOCK_SCALE = true;
    static constexpr int PIPE_WAVES = 1;
    static constexpr int PIPE_BLOCKS = 4;  // two sets of 8 loads + 8 exponents and four h8 per load in flight: 125 VGPRs, four wavefronts per SIMD
    // A lane's load covers x[32 l .. 32 l + 32) of a 2048-wide chunk (64 lanes): four 16-byte reads which in the natural
    // layout sit at a 64-byte lane stride (a 4-way bank conflict).  The LDS copy of a row is therefore permuted inside every
    // chunk of CL = min(2048, K - chunk start) halves: quarter j of every lane's 32 is stored together, x[chunk + 32 l + 8 j + e]
    // at chunk + j * CL / 4 + 8 l + e.  Read j of lanes l .. l + 15 is then 256 consecutive bytes (tools/lds_bank_model.py:
    // conflict-free), a ragged last chunk (K % 32 == 0: CL / 4 is a multiple of 8) stays inside the row's K halves.
    static __device__ __forceinline__ int xpos(int k, int K) {
        const int c0 = k & ~2047, r = k & 2047, cl = min(2048, K - c0);
        return c0 + ((r >> 3) & 3) * (cl >> 2) + (r >> 5) * 8;
    }
    static __device__ __forceinline__ void halves(const raw& r, unsigned e, h8 (&o)[4]) {
        const float sc = __builtin_bit_cast(float, e << 23);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned u = (unsigned)r[j];
            const h2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(u, sc, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(u, sc, 1);
            const h2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(u, sc, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(u, sc, 3);
            o[j] = h8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
        }
    }
};

// The one weight load of the projection kernels: the 16 bytes of weight row `row` at element k and, under BLOCK_SCALE, the
// exponent byte of that block (e = 0 otherwise).  Each kernel has its own rule for which k (and, in gemm16, which row) a load
// past the end is clamped to; it clamps BEFORE the call, so the weights and the exponent of a clamped re-read are one block's.
template <typename WT>
__device__ __forceinline__ void wload(const LlmGemvParams& p, long row, int K, int k, typename WLoad<WT>::raw& v, unsigned& e) {
    typedef WLoad<WT> WL;
    const WT* wr = reinterpret_cast<const WT*>(p.w) + ((row * K) >> WL::SH);
    v = *reinterpret_cast<const typename WL::raw*>(wr + (k >> WL::SH));
    e = 0;
    if constexpr (WL::BLOCK_SCALE) e = p.w_exp[row * (K / WL::E) + k / WL::E];
}

// ---- What the four projection kernels promise - the same bits whatever the kernel, the row count or the chunking, and the
// reference's fp16 rounding points - rests on the three functions below; each is spelled here once.
// 1/rms of one row of x read from global memory by one whole wavefront (`valid` false: a row past M, the sum is 0)
__device__ __forceinline__ float llm_row_scale(const half_t* xr, bool valid, int K, float eps, int lane) {
    float ss = 0.f;
    if (valid) {
        for (int k = lane * 8; k < K; k += 512) {
            const h8 v = *reinterpret_cast<const h8*>(xr + k);
            ss = dot8(v, v, ss);
        }
    }
    return __builtin_amdgcn_rsqf(wave_sum(ss) / (float)K + eps);
}

// Row staging of the LDS kernels (256 threads, all of them call it): rows 0 .. MC-1 of x (zeros past M) go to xs[m][K] in the
// order WL::xpos gives, rs[m] becomes the row's 1/rms (1 without p.rms) from per-wavefront partial sums added in wavefront
// order (rs[MC ..] holds the [MC][4] partials); with a gain the staged rows become the RMSNorm OUTPUT (reference roundings,
// rms_gain8) and no scale is left for the dots: rs[m] = 1.  Ends behind a barrier.
template <typename WL, int MC>
__device__ __forceinline__ void llm_stage_rows(const LlmGemvParams& p, half_t* xs, float* rs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K;
    float ss[MC];
#pragma unroll
    for (int m = 0; m < MC; ++m) {
        ss[m] = 0.f;
        for (int k = tid * 8; k < K; k += 2048) {
            h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (m < p.M) v = *reinterpret_cast<const h8*>(p.x + (long)m * p.ldx + k);
            *reinterpret_cast<h8*>(xs + (long)m * K + WL::xpos(k, K)) = v;
            ss[m] = dot8(v, v, ss[m]);
        }
        ss[m] = wave_sum(ss[m]);
        if (lane == 0) rs[MC + m * 4 + wave] = ss[m];
    }
    __syncthreads();
    if (tid < MC) {
        const float s = rs[MC + tid * 4] + rs[MC + tid * 4 + 1] + rs[MC + tid * 4 + 2] + rs[MC + tid * 4 + 3];
        rs[tid] = p.rms ? __builtin_amdgcn_rsqf(s / (float)K + p.eps) : 1.0f;
    }
    __syncthreads();
    if (p.rms && p.gain) {
#pragma unroll
        for (int m = 0; m < MC; ++m) {
            const float r = rs[m];
            for (int k = tid * 8; k < K; k += 2048) {
                h8* xp = reinterpret_cast<h8*>(xs + (long)m * K + WL::xpos(k, K));
                *xp = rms_gain8(*xp, *reinterpret_cast<const h8*>(p.gain + k), r);
            }
        }
        __syncthreads();
        if (tid < MC) rs[tid] = 1.0f;
        __syncthreads();
    }
}

// The output element, from the wavefront's or tile's fp32 sum(s), in two steps because every lane of the GEMV kernels holds
// the sum and one lane stores.  llm_proj_scale, in every lane: times the row's 1/rms `rr` (1 when a gain was applied: the scale
// is already inside x'), then times the weight row's scale for ROW_SCALE formats (sg: row n, su: the up row n + N) - the
// order of the two products is part of the bits.  (One fused function called by the storing lane alone gives the same bits
// but other registers: it changed the occupancy of three instantiations.)
template <typename WL, int SWIGLU>
__device__ __forceinline__ void llm_proj_scale(float& g, float& u, float rr, float sg, float su) {
    g *= rr;
    if (SWIGLU) u *= rr;
    if constexpr (WL::ROW_SCALE) {
        g *= sg;
        if (SWIGLU) u *= su;
    }
}
// llm_proj_out, in the storing lane: the scaled sums meet their fp16 roundings HERE and nowhere else.  SwiGLU is the
// reference's act_fn(gate_proj(x)) * up_proj(x) with an fp16 tensor after every step, f16(f16(silu(f16 g)) * f16 u); plain is
// f16(f16(g) + residual) (`residual`: the element, null without one).
template <int SWIGLU>
__device__ __forceinline__ half_t llm_proj_out(float g, float u, const half_t* residual) {
    float o;
    if (SWIGLU) {
        o = (float)(half_t)ds_silu((float)(half_t)g) * (float)(half_t)u;
    } else {
        o = (float)(half_t)g;
        if (residual) o += (float)*residual;
    }
    return (half_t)o;
}

// ---------------------------------------------------------------------------------------------------------------
// y[m][n] = r_m * sum_k x[m][k] w[n][k]  (+ residual[m][n]),  r_m = rsqrt(mean_k x[m][k]^2 + eps) if rms else 1
// (with p.gain: y[m][n] = sum_k f16(gain[k] * f16(x[m][k] r_m)) w[n][k], the reference's RMSNorm roundings)
// SWIGLU:  y[m][n] = silu(r_m * x.w[n]) * (r_m * x.w[n+N])     (gate rows [0,N), up rows [N,2N))
// One wavefront per output column; MC rows of x per pass (x comes from L1/L2, it is MC*K*2 bytes).
// ---------------------------------------------------------------------------------------------------------------
// WT = int8_t: w is int8 [N,K] (K % 16 == 0) and the wave's sum is multiplied by p.w_scale[n] (SwiGLU: [n] for the gate
// row, [n + N] for the up row) before the fp16 rounding; every other rounding point is the fp16 kernel's.
// WT = fp4x2_t: w is packed e2m1 [N,K/2] (K % 32 == 0), a load's block exponent is p.w_exp[n * K/32 + k/32] (the clamped k of
// the load, so weights and scale of a re-read come from the same block), and the row scale is applied as for int8.
template <typename WT, int MC, int SWIGLU>
__global__ __launch_bounds__(256) void llm_gemv_kernel(LlmGemvParams p) {
    typedef WLoad<WT> WL;
    constexpr int E = WL::E, NH = WL::NH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + wave;
    const int m0 = blockIdx.y * MC;
    if (n >= p.N) return;
    const int K = p.K;
    float r[MC];
#pragma unroll
    for (int m = 0; m < MC; ++m) r[m] = 1.0f;
    if (p.rms) {
#pragma unroll
        for (int m = 0; m < MC; ++m) r[m] = llm_row_scale(p.x + (long)(m0 + m) * p.ldx, m0 + m < p.M, K, p.eps, lane);
    }
    float acc[MC], acu[MC];
#pragma unroll
    for (int m = 0; m < MC; ++m) acc[m] = acu[m] = 0.f;
    constexpr int U = (MC <= 4) ? 4 : 2;  // independent 16-byte loads in flight per lane
    for (int k0 = lane * E; k0 < K; k0 += 64 * E * U) {
        typename WL::raw wv[U], uv[U];
        unsigned we[U], ue[U];   // block exponents of the loads (BLOCK_SCALE only)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = min(k0 + 64 * E * u, K - E);  // clamped re-read past the end, masked below
            wload<WT>(p, n, K, k, wv[u], we[u]);
            ue[u] = 0;
            if (SWIGLU) wload<WT>(p, (long)n + p.N, K, k, uv[u], ue[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + 64 * E * u;
            if (k < K) {
                h8 wh[NH], uh[NH];
                WL::halves(wv[u], we[u], wh);
                if (SWIGLU) WL::halves(uv[u], ue[u], uh);
#pragma unroll
                for (int m = 0; m < MC; ++m) {
                    if (m0 + m < p.M) {
#pragma unroll
                        for (int j = 0; j < NH; ++j) {
                            h8 xv = *reinterpret_cast<const h8*>(p.x + (long)(m0 + m) * p.ldx + k + 8 * j);
                            if (p.gain) xv = rms_gain8(xv, *reinterpret_cast<const h8*>(p.gain + k + 8 * j), r[m]);
                            acc[m] = dot8(xv, wh[j], acc[m]);
                            if (SWIGLU) acu[m] = dot8(xv, uh[j], acu[m]);
                        }
                    }
                }
            }
        }
    }
    float sg = 1.0f, su = 1.0f;
    if constexpr (WL::ROW_SCALE) {
        sg = p.w_scale[n];
        if (SWIGLU) su = p.w_scale[n + p.N];
    }
#pragma unroll
    for (int m = 0; m < MC; ++m) {
        acc[m] = wave_sum(acc[m]);
        if (SWIGLU) acu[m] = wave_sum(acu[m]);
        llm_proj_scale<WL, SWIGLU>(acc[m], acu[m], p.gain ? 1.0f : r[m], sg, su);
    }
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < MC; ++m) {
            if (m0 + m < p.M)
                p.y[(long)(m0 + m) * p.ldy + n] = llm_proj_out<SWIGLU>(
                    acc[m], acu[m], p.residual ? p.residual + (long)(m0 + m) * p.ldr + n : nullptr);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Attention of chunk row r (absolute position pos0 + r) over keys 0 .. pos0 + r: cache rows for j < pos0, the chunk's
// own (still un-rotated) k/v rows of the fused qkv buffer for j >= pos0.  The block of (head h, row r) also appends
// its rotated key and its value to the cache, so one launch per layer does rope + append + attention.
// Lanes are laid out [64/LPK keys][LPK chunks of 8 dims]: a wavefront reads whole 2*D-byte key rows.
// ---------------------------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void rope_chunk(const half_t* row, int c, const float* cs, const float* sn, float out[8]) {
    constexpr int LPK = D / 8, HALF = D / 2;
    const h8 a = *reinterpret_cast<const h8*>(row + 8 * c);
    const h8 b = *reinterpret_cast<const h8*>(row + 8 * (c ^ (LPK / 2)));
    const int d0 = (8 * c) % HALF;
    const float sgn = (8 * c < HALF) ? -1.0f : 1.0f;  // rotate_half = cat(-x2, x1)
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = (float)a[e] * cs[d0 + e] + sgn * (float)b[e] * sn[d0 + e];
}

constexpr int ATT_WAVES = 16;  // one key group per wavefront per iteration: the loop is a chain of dependent loads

// ---- fp8 KV cache (LlmAttnParams::k_exp): OCP e4m3 codes and one biased power-of-two exponent per (row, kv head).
// 2^(e - 127) of an exponent byte: the quantiser stores 94 .. 135, always the exponent field of a normal float
__device__ __forceinline__ float kv8_scale(unsigned e) { return __uint_as_float(e << 23); }

// 8 codes (two dwords, element 0 in the lowest byte) -> their e4m3 values in fp32, unscaled
__device__ __forceinline__ void kv8_unpack(const uint2 c, float out[8]) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
    const f2 d = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false), e = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
    out[0] = a[0]; out[1] = a[1]; out[2] = b[0]; out[3] = b[1];
    out[4] = d[0]; out[5] = d[1]; out[6] = e[0]; out[7] = e[1];
}

// The quantiser (diffsensei_amd/mllm.py: quantize_kv_fp8) on a head whose D values (fp16 numbers held in fp32) lie 8 per
// lane over D/8 neighbouring lanes, all of them active: amax over the head with the score loop's shuffle pattern; the
// exponent from the bits of amax = 1.f 2^(E-127): ex = E - 135 if 1.f <= 1.75 (amax / 2^ex <= 448) else E - 134, so the
// stored byte ex + 127 is the exponent field of amax + 0x1FFFFF, minus 8 (127 for an all-zero head); x 2^-ex is exact and
// at most 448, so the one rounding is v_cvt_pk_fp8_f32's (nearest even, subnormals kept) and nothing saturates.
template <int D>
__device__ __forceinline__ unsigned kv8_quantize(const float x[8], uint2& codes) {
    constexpr int LPK = D / 8;
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a = fmaxf(a, fabsf(x[e]));
#pragma unroll
    for (int o = 1; o < LPK; o <<= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
    const unsigned bits = __float_as_uint(a);
    const unsigned eb = bits ? ((bits + 0x1FFFFFu) >> 23) - 8u : 127u;
    const float inv = __uint_as_float((254u - eb) << 23);     // 2^-ex
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv, x[3] * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] * inv, x[5] * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] * inv, x[7] * inv, hi, true);
    codes = make_uint2((unsigned)lo, (unsigned)hi);
    return eb;
}

// KV8: the fp8-cache form (ds_kernels.h).  Same score / softmax / P V loop; a key or value is 8 code bytes per lane and
// the exponent byte of its (row, kv head) - a load of its own, beside the codes' and not behind it - and the power of two
// multiplies the finished dot product (keys) or the probability (values), so the conversion adds nothing to the loop's
// chain of dependent loads.  The chunk's own rows go through kv8_quantize in registers and then through the same
// arithmetic as a cached row: a row's result does not depend on how the prompt was cut into chunks.
template <int D, bool KV8>
__device__ __forceinline__ void llm_attn_body(const LlmAttnParams& p, const int h, const int r) {
    constexpr int LPK = D / 8, KPW = 64 / LPK, HALF = D / 2;
    // The state row first: the length every block starts from and, beside it, the flag only the slot form uses - one round
    // trip for both.  The fence keeps the two loads in front of the index arithmetic below, which then hides their latency
    // (left to itself the scheduler issues them behind the first division and the block waits with nothing to do).
    const int pos0 = p.state[0], finished = p.state[2];
    __builtin_amdgcn_sched_barrier(0);
    extern __shared__ float sm[];
    float* sc = sm;                    // [T_max] scores, then probabilities
    float* red = sm + p.T_max;         // [ATT_WAVES][D]
    float* misc = red + ATT_WAVES * D;  // [2 * ATT_WAVES]
    const int hkv = h / (p.heads / p.kv_heads);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane % LPK, ks = lane / LPK;
    const int T = pos0 + r + 1;
    // never write past the cache (the host sizes it); slot form only: a finished (or never started) slot is left alone.
    // One branch for both: a branch on the flag in front of the length's load would make every launch of the token step
    // wait for the state row twice.
    if ((T > p.T_max) | ((p.state_stride != 0) & (finished != 0))) return;
    const long kcol = (long)(p.heads + hkv) * D, vcol = (long)(p.heads + p.kv_heads + hkv) * D;
    const half_t* qrow = p.qkv + (long)r * p.ldqkv;
    uint8_t* const kc8 = reinterpret_cast<uint8_t*>(p.kc);     // KV8: the caches hold bytes
    uint8_t* const vc8 = reinterpret_cast<uint8_t*>(p.vc);

    float qf[8];
    rope_chunk<D>(qrow + (long)h * D, c, p.rope_cos + (long)(pos0 + r) * HALF, p.rope_sin + (long)(pos0 + r) * HALF, qf);

    // ---- scores
    float mx = -3.0e38f;
    for (int g = wave; g * KPW < T; g += ATT_WAVES) {
        const int j = g * KPW + ks;
        float s = 0.f, ksc = 1.0f;
        if (j < T) {
            float kf[8];
            if (j < pos0) {
                if constexpr (KV8) {
                    const uint2 kv = *reinterpret_cast<const uint2*>(kc8 + (long)j * p.ldc + (long)hkv * D + 8 * c);
                    ksc = kv8_scale(p.k_exp[(long)j * p.lde + hkv]);
                    kv8_unpack(kv, kf);
                } else {
                    const h8 kv = *reinterpret_cast<const h8*>(p.kc + (long)j * p.ldc + (long)hkv * D + 8 * c);
#pragma unroll
                    for (int e = 0; e < 8; ++e) kf[e] = (float)kv[e];
                }
            } else {
                rope_chunk<D>(p.qkv + (long)(j - pos0) * p.ldqkv + kcol, c, p.rope_cos + (long)j * HALF,
                              p.rope_sin + (long)j * HALF, kf);
#pragma unroll
                for (int e = 0; e < 8; ++e) kf[e] = (float)(half_t)kf[e];  // same rounding as the cached copy
                if constexpr (KV8) {    // and the same codes: all LPK lanes of a key take this branch together
                    uint2 kv;
                    ksc = kv8_scale(kv8_quantize<D>(kf, kv));
                    kv8_unpack(kv, kf);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf(qf[e], kf[e], s);
        }
#pragma unroll
        for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o, 64);
        if constexpr (KV8) s *= ksc;
        s *= p.scale;
        if (j < T) {
            if (c == 0) sc[j] = s;
            mx = fmaxf(mx, s);
        }
    }
    mx = wave_max(mx);
    if (lane == 0) misc[wave] = mx;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < ATT_WAVES; ++w) mx = fmaxf(mx, misc[w]);
    float sum = 0.f;
    for (int j = tid; j < T; j += 64 * ATT_WAVES) {
        const float e = __expf(sc[j] - mx);
        sc[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) misc[ATT_WAVES + wave] = sum;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < ATT_WAVES; ++w) tot += misc[ATT_WAVES + w];
    const float inv = 1.0f / tot;

    // ---- P V
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int g = wave; g * KPW < T; g += ATT_WAVES) {
        const int j = g * KPW + ks;
        if (j < T) {
            float pj = (float)(half_t)(sc[j] * inv);  // the reference casts the probabilities to fp16
            if constexpr (KV8) {
                uint2 vv;
                unsigned eb;
                if (j < pos0) {
                    vv = *reinterpret_cast<const uint2*>(vc8 + (long)j * p.ldc + (long)hkv * D + 8 * c);
                    eb = p.v_exp[(long)j * p.lde + hkv];
                } else {
                    const h8 vh = *reinterpret_cast<const h8*>(p.qkv + (long)(j - pos0) * p.ldqkv + vcol + 8 * c);
                    float vx[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) vx[e] = (float)vh[e];
                    eb = kv8_quantize<D>(vx, vv);
                }
                float vf[8];
                kv8_unpack(vv, vf);
                pj *= kv8_scale(eb);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, vf[e], acc[e]);
            } else {
                const half_t* vp = (j < pos0) ? p.vc + (long)j * p.ldc + (long)hkv * D + 8 * c
                                              : p.qkv + (long)(j - pos0) * p.ldqkv + vcol + 8 * c;
                const h8 vv = *reinterpret_cast<const h8*>(vp);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, (float)vv[e], acc[e]);
            }
        }
    }
#pragma unroll
    for (int o = LPK; o < 64; o <<= 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
    }
    if (ks == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wave * D + 8 * c + e] = acc[e];
    }
    __syncthreads();
    if (tid < D) {
        float o = 0.f;
#pragma unroll
        for (int w = 0; w < ATT_WAVES; ++w) o += red[w * D + tid];
        p.out[(long)r * p.ldo + (long)h * D + tid] = (half_t)o;
    }
    // ---- append this row's rotated key and its value (one query head per kv head does it)
    if (h % (p.heads / p.kv_heads) == 0 && wave == 0 && ks == 0) {
        float kf[8];
        rope_chunk<D>(qrow + kcol, c, p.rope_cos + (long)(pos0 + r) * HALF, p.rope_sin + (long)(pos0 + r) * HALF, kf);
        h8 ko;
#pragma unroll
        for (int e = 0; e < 8; ++e) ko[e] = (half_t)kf[e];
        const long off = (long)(pos0 + r) * p.ldc + (long)hkv * D + 8 * c;
        if constexpr (KV8) {    // lanes 0 .. LPK-1 of wavefront 0 hold the head: codes with vector stores, one exponent byte each
            const h8 vo = *reinterpret_cast<const h8*>(qrow + vcol + 8 * c);
            float vf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                kf[e] = (float)ko[e];
                vf[e] = (float)vo[e];
            }
            uint2 k8, v8;
            const unsigned ek = kv8_quantize<D>(kf, k8), ev = kv8_quantize<D>(vf, v8);
            *reinterpret_cast<uint2*>(kc8 + off) = k8;
            *reinterpret_cast<uint2*>(vc8 + off) = v8;
            if (c == 0) {
                p.k_exp[(long)(pos0 + r) * p.lde + hkv] = (uint8_t)ek;
                p.v_exp[(long)(pos0 + r) * p.lde + hkv] = (uint8_t)ev;
            }
        } else {
            *reinterpret_cast<h8*>(p.kc + off) = ko;
            *reinterpret_cast<h8*>(p.vc + off) = *reinterpret_cast<const h8*>(qrow + vcol + 8 * c);
        }
    }
}

// Block (head h, row m), both row forms (ds_kernels.h).  One-sequence form (state_stride = 0): row m of the chunk, on the one
// cache and state block.  Slot form: the block moves to row m of qkv / out, to slot m's own cache (kc + m * slot_stride) and
// state row (state + 8 m) and runs the body on row 0 there, so the slot's length state[m][0] sets its rotary position.
// Only the slot form looks at the finished flag - a finished (or never started) slot returns before it touches anything;
// the one-sequence form never did (the prompt cursor has the flag at zero), hence the `state_stride != 0 &` in the body's
// early-out.
template <int D, bool KV8>
__global__ __launch_bounds__(64 * ATT_WAVES) void llm_attn_kernel(LlmAttnParams p) {
    const int s = p.state_stride ? blockIdx.y : 0;   // rows in front of this block's row that are other sequences
    p.state += p.state_stride * s;
    p.qkv += (long)s * p.ldqkv;
    p.out += (long)s * p.ldo;
    if constexpr (KV8) {                             // byte caches: the slot stride counts bytes
        p.kc = reinterpret_cast<half_t*>(reinterpret_cast<uint8_t*>(p.kc) + (long)s * p.slot_stride);
        p.vc = reinterpret_cast<half_t*>(reinterpret_cast<uint8_t*>(p.vc) + (long)s * p.slot_stride);
        p.k_exp += (long)s * p.exp_slot_stride;
        p.v_exp += (long)s * p.exp_slot_stride;
    } else {
        p.kc += (long)s * p.slot_stride;
        p.vc += (long)s * p.slot_stride;
    }
    llm_attn_body<D, KV8>(p, blockIdx.x, blockIdx.y - s);
}

// Ragged form: the rows of several slots in one launch (the chain fast-forward pass, diffsensei_amd/mllm.py).  Row R of qkv /
// out is row r of the segment of slot `slot`, table[R] = (slot, r); a segment's rows are consecutive, so its first row is
// R - r.  Block (head h, row R) moves to that slot's cache, exponent planes and state row and to the segment's first row, and
// runs the body on row r: keys below state[slot][0] come from the cache, the segment's own rows from qkv, rounded as a cached
// copy, and the block appends its own K and V - nothing here reads what another block of the launch writes, so the result
// does not depend on how the rows are cut into segments or launches.  Segments may be longer than 16 rows.  The finished
// flag is not looked at (state_stride = 0 for the body): a paused slot carries 2 there.  A table entry outside the launch
// (slot not in [0, n_slots), r not in [0, R]) is skipped; the body writes nothing at or past T_max.
template <int D, bool KV8>
__global__ __launch_bounds__(64 * ATT_WAVES) void llm_attn_rows_kernel(LlmAttnParams p, const int* __restrict__ table,
                                                                       int n_slots) {
    const int R = blockIdx.y;
    const int s = table[2 * R], r = table[2 * R + 1];
    if ((s < 0) | (s >= n_slots) | (r < 0) | (r > R)) return;
    p.state += 8 * s;
    p.qkv += (long)(R - r) * p.ldqkv;
    p.out += (long)(R - r) * p.ldo;
    if constexpr (KV8) {                             // byte caches: the slot stride counts bytes
        p.kc = reinterpret_cast<half_t*>(reinterpret_cast<uint8_t*>(p.kc) + (long)s * p.slot_stride);
        p.vc = reinterpret_cast<half_t*>(reinterpret_cast<uint8_t*>(p.vc) + (long)s * p.slot_stride);
        p.k_exp += (long)s * p.exp_slot_stride;
        p.v_exp += (long)s * p.exp_slot_stride;
    } else {
        p.kc += (long)s * p.slot_stride;
        p.vc += (long)s * p.slot_stride;
    }
    p.state_stride = 0;
    llm_attn_body<D, KV8>(p, blockIdx.x, r);
}

// ---------------------------------------------------------------------------------------------------------------
// y[m] = g * (x[m] / rms(x[m]))  (LlamaRMSNorm: normalise in fp32, cast to fp16, then multiply by the gain).
// `feat` (token loop only, M = 1): the same row is also stored as row state[1]-1 of the per-token feature buffer —
// the hidden state seed_x.py:143 collects for every generated token that was fed back.
// ---------------------------------------------------------------------------------------------------------------
// `fr` = the feature row this block also writes (null: none)
__device__ __forceinline__ void llm_rmsnorm_row(const half_t* __restrict__ xr, const half_t* __restrict__ gamma,
                                                half_t* __restrict__ yr, half_t* __restrict__ fr, int H, float eps) {
    __shared__ float part[4];
    const int tid = threadIdx.x;
    float ss = 0.f;
    for (int k = tid * 8; k < H; k += 2048) {
        const h8 v = *reinterpret_cast<const h8*>(xr + k);
        ss = dot8(v, v, ss);
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    const float r = __builtin_amdgcn_rsqf((part[0] + part[1] + part[2] + part[3]) / (float)H + eps);
    for (int k = tid * 8; k < H; k += 2048) {
        const h8 v = *reinterpret_cast<const h8*>(xr + k);
        const h8 g = *reinterpret_cast<const h8*>(gamma + k);
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)g[e] * (float)(half_t)((float)v[e] * r));
        *reinterpret_cast<h8*>(yr + k) = o;
        if (fr) *reinterpret_cast<h8*>(fr + k) = o;
    }
}

// Row m, both row forms.  The tap: one-sequence form (state_stride = 0) row state[1]-1+m of feat ([max_out][H]); slot form
// row state[m][1]-1 of feat[m] ([S][max_out][H]).
__global__ __launch_bounds__(256) void llm_rmsnorm_kernel(const half_t* __restrict__ x, long ldx,
                                                          const half_t* __restrict__ gamma, half_t* __restrict__ y,
                                                          long ldy, half_t* __restrict__ feat,
                                                          const int* __restrict__ state, int state_stride, int H,
                                                          int max_out, float eps) {
    const int m = blockIdx.x;
    half_t* fr = nullptr;
    if (feat) {
        const int s = state_stride ? m : 0;
        const int* st = state + state_stride * s;
        const int row = st[1] - 1 + (m - s);
        if (row >= 0 && row < max_out && !st[2]) fr = feat + ((long)s * max_out + row) * H;
    }
    llm_rmsnorm_row(x + (long)m * ldx, gamma, y + (long)m * ldy, fr, H, eps);
}

// h[m,:] = embed_tokens[state[m][3]]  (one-sequence form: one row, h[0,:] = embed_tokens[state[3]])
__global__ __launch_bounds__(256) void llm_embed_kernel(const half_t* __restrict__ table, const int* __restrict__ state,
                                                        int state_stride, half_t* __restrict__ out, long ldo, int H,
                                                        int vocab) {
    const int m = blockIdx.y;
    const int tok = min(max(state[state_stride * m + 3], 0), vocab - 1);
    const int k = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (k < H) *reinterpret_cast<h8*>(out + (long)m * ldo + k) = *reinterpret_cast<const h8*>(table + (long)tok * H + k);
}

// ---------------------------------------------------------------------------------------------------------------
// Greedy choice with the reference's AutoImageTokenGenerationProcessor folded in (generation.py:19-30):
//   chain = [<img>, <img_00000> .. <img_{n-1}>, </img>];  previous token in chain[:-1] -> the next chain id wins
//   (the reference lifts its score to max + 10); otherwise the scores of chain[1:] are set to exactly 0.0 first.
// argmax ties go to the lowest id (torch.argmax).  Then: append the id, make it the current token, advance the cache
// length by `adv` rows, and raise `finished` on EOS (state[5]) or when state[4] ids are out.  One block.
// PAUSE (chain fast-forward): a slot that did not finish and whose new token lies in chain[:-1] - every following id up to
// </img> is then known without reading a weight - gets state[2] = 2: every per-slot kernel leaves it alone until the host
// has run the forced rows in one pass and written the state row back.  Without PAUSE the code is what it was.
// ---------------------------------------------------------------------------------------------------------------
template <bool PAUSE>
__device__ __forceinline__ void llm_select_body(const half_t* __restrict__ logits, int V,
                                                const int* __restrict__ chain, int n_chain, int out_cap, int adv,
                                                int* __restrict__ state, int* __restrict__ out_ids) {
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ int forced, lo, hi;
    const int tid = threadIdx.x;
    if (state[2]) return;  // finished: replays of the captured step are no-ops
    const int prev = state[3];
    if (tid == 0) {
        forced = -1;
        lo = 0x7fffffff;
        hi = -1;
    }
    __syncthreads();
    if (tid < n_chain - 1 && chain[tid] == prev) atomicMax(&forced, chain[tid + 1]);
    if (tid >= 1 && tid < n_chain) {  // id range of chain[1:], so the membership scan below runs for few ids only
        atomicMin(&lo, chain[tid]);
        atomicMax(&hi, chain[tid]);
    }
    __syncthreads();
    const int zlo = lo, zhi = hi;
    float best = -3.0e38f;
    int idx = 0x7fffffff;
    for (int v = tid; v < V; v += 1024) {
        float s = (float)logits[v];
        if (v >= zlo && v <= zhi)
            for (int q = 1; q < n_chain; ++q)
                if (chain[q] == v) s = 0.0f;
        if (s > best) {  // strided ascending scan: the first maximum of this thread is its lowest id
            best = s;
            idx = v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ob > best || (ob == best && oi < idx)) {
            best = ob;
            idx = oi;
        }
    }
    if ((tid & 63) == 0) {
        bv[tid >> 6] = best;
        bi[tid >> 6] = idx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < idx)) {
                best = bv[w];
                idx = bi[w];
            }
        const int next = forced >= 0 ? forced : idx;
        const int n_out = state[1], max_new = state[4], eos = state[5];
        if (n_out < out_cap) out_ids[n_out] = next;
        state[1] = n_out + 1;
        state[3] = next;
        state[0] += adv;
        if (next == eos || n_out + 1 >= max_new) state[2] = 1;
        else if constexpr (PAUSE) {
            for (int q = 0; q < n_chain - 1; ++q)
                if (chain[q] == next) {
                    state[2] = 2;
                    break;
                }
        }
    }
}

// One block per row m over logits[m] (row stride ldl), with the row's own state (its eos and max_new live there) and its
// own out_ids[m] ([S][out_cap]).  The one-sequence form is one row.
template <bool PAUSE>
__global__ __launch_bounds__(1024) void llm_select_kernel(const half_t* __restrict__ logits, long ldl, int V,
                                                          const int* __restrict__ chain, int n_chain, int out_cap,
                                                          int adv, int* __restrict__ state, int state_stride,
                                                          int* __restrict__ out_ids) {
    const int m = blockIdx.x;
    llm_select_body<PAUSE>(logits + (long)m * ldl, V, chain, n_chain, out_cap, adv, state + state_stride * m,
                           out_ids + (long)m * out_cap);
}

// act[m][n] = silu(gu[m][n]) * gu[m][I+n]  (prompt pass: the gate|up projection comes out of the MFMA GEMM as [M,2I])
__global__ __launch_bounds__(256) void llm_swiglu_kernel(const half_t* __restrict__ gu, half_t* __restrict__ act,
                                                         int M, int I) {
    const long idx = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (idx >= (long)M * I) return;
    const long m = idx / I, n = idx - m * I;
    const h8 g = *reinterpret_cast<const h8*>(gu + m * 2 * I + n);
    const h8 u = *reinterpret_cast<const h8*>(gu + m * 2 * I + I + n);
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)(half_t)ds_silu((float)g[e]) * (float)u[e]);
    *reinterpret_cast<h8*>(act + idx) = o;
}

__global__ void llm_advance_kernel(int* state, int rows) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[0] += rows;
}

// out = a * s + b * (1 - s): the MLLM / encoder blend of scripts/demo/gradio.py:108-109 (n % 8 == 0)
__global__ __launch_bounds__(256) void blend_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b,
                                                    half_t* __restrict__ out, long n, float s) {
    const long k = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (k >= n) return;
    const h8 av = *reinterpret_cast<const h8*>(a + k), bv = *reinterpret_cast<const h8*>(b + k);
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)(half_t)((float)av[e] * s) + (float)(half_t)((float)bv[e] * (1.0f - s)));
    *reinterpret_cast<h8*>(out + k) = o;
}

// ---------------------------------------------------------------------------------------------------------------
// Token-loop variant (M <= 4): the kernel above keeps only ~4 KB of weights in flight per wavefront and spends a third
// of each wavefront's life on the x prologue - measured 3.9 TB/s on the 13 B model.  Here the block stages x (and the
// row scales) in LDS once, every wavefront walks several output columns, and each column iteration has 8 KB (plain) /
// 2 x 4 KB (SwiGLU) of independent 16-byte weight loads in flight before the first dot product.
// ---------------------------------------------------------------------------------------------------------------
template <int MC, int SWIGLU>
__global__ __launch_bounds__(256) void llm_gemv_stream_kernel(LlmGemvParams p) {
    extern __shared__ char smem_raw[];
    half_t* xs = reinterpret_cast<half_t*>(smem_raw);               // [MC][K]
    float* rs = reinterpret_cast<float*>(smem_raw + (size_t)MC * p.K * 2);  // [MC] row scales, then [MC][4] partials
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = p.K;
    llm_stage_rows<WLoad<half_t>, MC>(p, xs, rs);
    constexpr int U = SWIGLU ? 4 : 8;
    for (int n = blockIdx.x * 4 + wave; n < p.N; n += gridDim.x * 4) {
        float acc[MC], acu[MC];
#pragma unroll
        for (int m = 0; m < MC; ++m) acc[m] = acu[m] = 0.f;
        for (int k0 = lane * 8; k0 < K; k0 += 512 * U) {
            h8 wv[U], uv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = min(k0 + 512 * u, K - 8);
                unsigned none;
                wload<half_t>(p, n, K, k, wv[u], none);
                if (SWIGLU) wload<half_t>(p, (long)n + p.N, K, k, uv[u], none);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + 512 * u;
                if (k < K) {
#pragma unroll
                    for (int m = 0; m < MC; ++m) {
                        const h8 xv = *reinterpret_cast<const h8*>(xs + (long)m * K + k);
                        acc[m] = dot8(xv, wv[u], acc[m]);
                        if (SWIGLU) acu[m] = dot8(xv, uv[u], acu[m]);
                    }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < MC; ++m) {
            acc[m] = wave_sum(acc[m]);
            if (SWIGLU) acu[m] = wave_sum(acu[m]);
            llm_proj_scale<WLoad<half_t>, SWIGLU>(acc[m], acu[m], rs[m], 1.0f, 1.0f);
        }
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < MC; ++m) {
                if (m < p.M)
                    p.y[(long)m * p.ldy + n] = llm_proj_out<SWIGLU>(
                        acc[m], acu[m], p.residual ? p.residual + (long)m * p.ldr + n : nullptr);
            }
        }
    }
}

// Same data path, software-pipelined: the weight loads of the NEXT k-block (or of the next column's first k-block) are
// issued before the dot products of the current one, and the first block is requested before x is staged, so a
// wavefront always has 8 KB of weights in flight - no load bubble at block start, between k-blocks or between columns.
// WT = int8_t: 16 weights per load, so a lane's k-stride is 16 and a k-block is twice as long; x stays fp16 in LDS.
// WT = fp4x2_t: 32 weights per load with the load's block exponent beside it; x stays fp16 in LDS, in the order WLoad::xpos
// gives (the fp16 and int8 forms keep the natural order).
template <typename WT, int MC, int SWIGLU>
__global__ __launch_bounds__(256, MC == 1 ? WLoad<WT>::PIPE_WAVES : 1) void llm_gemv_pipe_kernel(LlmGemvParams p) {
    typedef WLoad<WT> WL;
    typedef typename WL::raw wraw;
    constexpr int E = WL::E, NH = WL::NH;
    extern __shared__ char smem_raw[];
    half_t* xs = reinterpret_cast<half_t*>(smem_raw);
    float* rs = reinterpret_cast<float*>(smem_raw + (size_t)MC * p.K * 2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = p.K, N = p.N;
    constexpr int U = SWIGLU ? 4 : 8;
    const int NIT = (K + 64 * E * U - 1) / (64 * E * U);
    const int stride = gridDim.x * 4;
    int n = blockIdx.x * 4 + wave;
    wraw wa[U], ua[U], wb[U], ub[U];
    unsigned ea[U], fa[U], eb[U], fb[U];   // block exponents of the loads (BLOCK_SCALE only): e* gate / plain, f* up
    auto issue = [&](int col, int it, wraw(&wv)[U], wraw(&uv)[U], unsigned(&ev)[U], unsigned(&fv)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = min(it * 64 * E * U + 64 * E * u + lane * E, K - E);
            wload<WT>(p, col, K, k, wv[u], ev[u]);
            fv[u] = 0;
            if (SWIGLU) wload<WT>(p, (long)col + N, K, k, uv[u], fv[u]);
        }
    };
    if (n < N) issue(n, 0, wa, ua, ea, fa);
    llm_stage_rows<WL, MC>(p, xs, rs);
    while (n < N) {
        float acc[MC], acu[MC];
#pragma unroll
        for (int m = 0; m < MC; ++m) acc[m] = acu[m] = 0.f;
        for (int it = 0; it < NIT; ++it) {
            const bool last = it + 1 == NIT;
            const int ncol = last ? n + stride : n;
            if (ncol < N) issue(ncol, last ? 0 : it + 1, wb, ub, eb, fb);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = it * 64 * E * U + 64 * E * u + lane * E;
                if (k < K) {
                    h8 wh[NH], uh[NH];
                    WL::halves(wa[u], ea[u], wh);
                    if (SWIGLU) WL::halves(ua[u], fa[u], uh);
#pragma unroll
                    for (int m = 0; m < MC; ++m) {
#pragma unroll
                        for (int j = 0; j < NH; ++j) {
                            const h8 xv = *reinterpret_cast<const h8*>(xs + (long)m * K + WL::xpos(k + 8 * j, K));
                            acc[m] = dot8(xv, wh[j], acc[m]);
                            if (SWIGLU) acu[m] = dot8(xv, uh[j], acu[m]);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                wa[u] = wb[u];
                if (SWIGLU) ua[u] = ub[u];
                if constexpr (WL::BLOCK_SCALE) {
                    ea[u] = eb[u];
                    if (SWIGLU) fa[u] = fb[u];
                }
            }
        }
        float sg = 1.0f, su = 1.0f;
        if constexpr (WL::ROW_SCALE) {
            sg = p.w_scale[n];
            if (SWIGLU) su = p.w_scale[n + N];
        }
#pragma unroll
        for (int m = 0; m < MC; ++m) {
            acc[m] = wave_sum(acc[m]);
            if (SWIGLU) acu[m] = wave_sum(acu[m]);
            llm_proj_scale<WL, SWIGLU>(acc[m], acu[m], rs[m], sg, su);
        }
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < MC; ++m) {
                if (m < p.M)
                    p.y[(long)m * p.ldy + n] = llm_proj_out<SWIGLU>(
                        acc[m], acu[m], p.residual ? p.residual + (long)m * p.ldr + n : nullptr);
            }
        }
        n += stride;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Batched decode (up to 16 sequences per weight pass): y[M <= 16, N] = x'[M, K] w[N, K]^T on the matrix pipe, same
// prologues / epilogues and fp16 rounding points as the kernels above.  At 16 rows the fdot2 form needs 64 fdot2 and
// 256 B of x per 16-byte weight load and lane, which a CU cannot feed at the HBM rate; one v_mfma_f32_16x16x32_f16 does
// the 16 rows x 16 columns x 32 k of a 1 KB weight fragment.
//   A operand = x, padded to 16 rows with zeros: lane l holds x[l & 15][k + 8 (l >> 4) .. + 8]
//   B operand = 16 weight rows:                  lane l holds w[n0 + (l & 15)][k + 8 (l >> 4) .. + 8]
//   C:                                           lane l holds y[4 (l >> 4) + reg][n0 + (l & 15)]
// Weights go HBM -> VGPR in that layout with 16-byte loads, no LDS.  A block owns one 16-column tile at a time; its
// four wavefronts split K in interleaved blocks of 32 U halves (U MFMA steps), so a wavefront consumes U / 2 whole
// 128-byte lines of each of its 16 weight rows per iteration and has U KB of weights in flight: the loads of the next
// k-block (or of the next tile's first one) are issued before the MFMAs of the current one.  The four partial tiles
// are added in wavefront order 0..3 through LDS (no atomics), by the thread that then writes the element.
// x: read from L2 in the fragment layout, prefetched with the weights (16 x 13824 x 2 B does not fit LDS).  Staging x
// in LDS by K chunks pays only when a staged chunk serves several column tiles; the o / down projections have 320
// tiles for 256 CUs, so a block has one tile and a staged chunk would move the same bytes from L2 as the fragments do,
// plus an LDS round trip and two barriers per chunk.  Only the RMSNorm gain [K] is kept in LDS (read per k-step).
// A row's result depends on that row of x alone: rows >= M are zero fragments, the k order is fixed by (K, lane), the
// row scale is computed by a fixed wavefront, and an MFMA output row takes nothing from other A rows.
// ---------------------------------------------------------------------------------------------------------------
// WT = int8_t: one 16-byte load holds 16 weights of a row and feeds two MFMA steps.  Lane l's load covers
// k + 16 (l >> 4) .. + 16 of a 64-wide k-block; step 2v takes its first 8 weights, step 2v + 1 the last 8, and the lane's x
// fragments of those two steps are read at the same k indices (any assignment of k to lanes is a valid MFMA as long as
// A and B agree).  K % 16 == 0, so a load is inside K or wholly past it: past it the x fragments are zero, whatever number
// of 16-weight groups the last block has.  The row scale w_scale[n] is applied in the epilogue by the writing thread.
// WT = fp4x2_t: the same argument with four steps per load.  Lane l's load covers k + 32 (l >> 4) .. + 32 of a 128-wide
// k-block (one MX block, converted with its exponent w_exp[n][k / 32]); step 4v + j takes its weights 8 j .. 8 j + 8 and the
// lane's x fragment of that step is read at the same k.  K % 32 == 0, so a load is inside K or wholly past it (23 blocks: the
// last 128-wide k-block has three loads inside K and one past it); U is 4 or 8, so a wavefront issues 1 or 2 loads per matrix.
template <typename WT, int SWIGLU>
__global__ __launch_bounds__(256) void llm_gemm16_kernel(LlmGemvParams p) {
    typedef WLoad<WT> WL;
    typedef typename WL::raw wraw;
    constexpr int E = WL::E, NH = WL::NH;
    constexpr int U = SWIGLU ? 4 : 8;   // MFMA steps per iteration
    constexpr int UL = U / NH;          // 16-byte weight loads per lane and matrix per iteration
    constexpr int KB = 32 * U;          // halves of K per wavefront iteration
    constexpr int NACC = SWIGLU ? 2 : 1;
    extern __shared__ char smem_raw[];
    float* red = reinterpret_cast<float*>(smem_raw);                   // [2 tiles in flight][NACC][4 wavefronts][256]
    float* rs = red + 2 * NACC * 4 * 256;                              // [16] row scales
    half_t* gl = reinterpret_cast<half_t*>(rs + 16);                   // [K] RMSNorm gain (with p.gain)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int K = p.K, N = p.N, M = p.M;
    const int NT = (N + 15) / 16, NIT = (K + 4 * KB - 1) / (4 * KB);
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    wraw wa[UL], ua[UL], wb[UL], ub[UL];
    unsigned ea[UL], fa[UL], eb[UL], fb[UL];   // block exponents of the loads (BLOCK_SCALE only): e* gate / plain, f* up
    h8 xa[U], xb[U];
    // first k of MFMA step u of this lane in iteration `it`: a load spans NH steps, 32 NH k per group of 4 lanes-by-16
    auto kof = [&](int it, int u) { return (it * 4 + wave) * KB + 32 * NH * (u / NH) + 8 * NH * g + 8 * (u % NH); };
    auto issue_w = [&](int tile, int it, wraw(&wv)[UL], wraw(&uv)[UL], unsigned(&ev)[UL], unsigned(&fv)[UL]) {
        const long col = min(tile * 16 + c, N - 1);   // ragged last tile: re-read the last row, never stored
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            const int k = min(kof(it, u * NH), K - E);   // ragged K: clamped (the scale index with it), x is zero there
            wload<WT>(p, col, K, k, wv[u], ev[u]);
            fv[u] = 0;
            if (SWIGLU) wload<WT>(p, col + N, K, k, uv[u], fv[u]);
        }
    };
    const half_t* xr = p.x + (long)min(c, M - 1) * p.ldx;
    auto issue_x = [&](int it, h8(&xv)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = kof(it, u);
            const h8 v = *reinterpret_cast<const h8*>(xr + min(k, K - 8));
            xv[u] = (c < M && k < K) ? v : zero;
        }
    };
    int tile = blockIdx.x;
    if (tile < NT) issue_w(tile, 0, wa, ua, ea, fa);
    // ---- row scales (wavefront w: rows 4w .. 4w+3) and the gain vector
    if (p.rms) {
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) {
            const int m = wave * 4 + mm;
            const float r = llm_row_scale(p.x + (long)m * p.ldx, m < M, K, p.eps, lane);
            if (lane == 0) rs[m] = m < M ? r : 1.0f;
        }
        if (p.gain)
            for (int k = tid * 8; k < K; k += 2048) *reinterpret_cast<h8*>(gl + k) = *reinterpret_cast<const h8*>(p.gain + k);
    } else if (tid < 16) {
        rs[tid] = 1.0f;
    }
    __syncthreads();
    const bool gain = p.rms && p.gain;
    const float ra = rs[c];
    if (tile < NT) issue_x(0, xa);
    int par = 0;
    while (tile < NT) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acu = {0.f, 0.f, 0.f, 0.f};
        for (int it = 0; it < NIT; ++it) {
            const bool last = it + 1 == NIT;
            const int ntile = last ? tile + (int)gridDim.x : tile, nit = last ? 0 : it + 1;
            if (ntile < NT) {
                issue_x(nit, xb);
                issue_w(ntile, nit, wb, ub, eb, fb);
            }
#pragma unroll
            for (int v = 0; v < UL; ++v) {
                h8 wh[NH], uh[NH];
                WL::halves(wa[v], ea[v], wh);
                if (SWIGLU) WL::halves(ua[v], fa[v], uh);
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int u = v * NH + j;
                    h8 a = xa[u];
                    if (gain) {   // the fragment becomes the RMSNorm OUTPUT at the reference's roundings (zero stays zero)
                        const int k = min(kof(it, u), K - 8);
                        a = rms_gain8(a, *reinterpret_cast<const h8*>(gl + k), ra);
                    }
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, wh[j], acc, 0, 0, 0);
                    if (SWIGLU) acu = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, uh[j], acu, 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) xa[u] = xb[u];
#pragma unroll
            for (int u = 0; u < UL; ++u) {
                wa[u] = wb[u];
                if (SWIGLU) ua[u] = ub[u];
                if constexpr (WL::BLOCK_SCALE) {
                    ea[u] = eb[u];
                    if (SWIGLU) fa[u] = fb[u];
                }
            }
        }
        // ---- split-K reduction in wavefront order, then the epilogue: thread (wave = reg, lane) owns one element
        float* rp = red + par * NACC * 1024;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            rp[wave * 256 + q * 64 + lane] = acc[q];
            if (SWIGLU) rp[1024 + wave * 256 + q * 64 + lane] = acu[q];
        }
        __syncthreads();   // one barrier per tile: the next tile writes the other half of `red`
        {
            const int m = 4 * g + wave, n = tile * 16 + c;
            float a = ((rp[tid] + rp[256 + tid]) + rp[512 + tid]) + rp[768 + tid];
            const float rr = gain ? 1.0f : rs[m];
            if (m < M && n < N) {
                float b = 0.f, sg = 1.0f, su = 1.0f;
                if (SWIGLU) b = ((rp[1024 + tid] + rp[1280 + tid]) + rp[1536 + tid]) + rp[1792 + tid];
                if constexpr (WL::ROW_SCALE) {
                    sg = p.w_scale[n];
                    if (SWIGLU) su = p.w_scale[n + N];
                }
                llm_proj_scale<WL, SWIGLU>(a, b, rr, sg, su);
                p.y[(long)m * p.ldy + n] = llm_proj_out<SWIGLU>(a, b, p.residual ? p.residual + (long)m * p.ldr + n : nullptr);
            }
        }
        par ^= 1;
        tile += gridDim.x;
    }
}

// w16[n][k] = f16(f32(q[n][k]) * s[n]): the prompt pass dequantises the matrix it is about to hand to the MFMA GEMMs.
// One thread per 16 weights (K % 16 == 0: all of one row); one fp32 multiply and one round-to-nearest-even per element.
__global__ __launch_bounds__(256) void llm_dequant_w8_kernel(const int8_t* __restrict__ q, const float* __restrict__ s,
                                                             half_t* __restrict__ w16, long groups, int K) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= groups) return;
    const long e0 = gi * 16;
    const float sc = s[e0 / K];
    const i32x4 v = *reinterpret_cast<const i32x4*>(q + e0);
    h8 o[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            float f = (float)(int8_t)(v[j] >> (8 * b)) * sc;
            asm("" : "+v"(f));   // the fp32 product stays a value of its own: the fp16 rounding is a second, separate step
            o[j >> 1][4 * (j & 1) + b] = (half_t)f;
        }
    }
    *reinterpret_cast<h8*>(w16 + e0) = o[0];
    *reinterpret_cast<h8*>(w16 + e0 + 8) = o[1];
}

// w16[n][k] = f16(f32(e2m1[n][k] * 2^(e[n][k/32] - 127)) * s[n]) for the prompt pass's MFMA GEMMs: one thread per MX block
// (16 bytes), the block product through the same hardware conversion as the decode kernels (exact in f16), then one fp32
// multiply by the row scale and one round-to-nearest-even per element.
__global__ __launch_bounds__(256) void llm_dequant_fp4_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ ex,
                                                              const float* __restrict__ s, half_t* __restrict__ w16,
                                                              long blocks, int K) {
    const long bi = (long)blockIdx.x * 256 + threadIdx.x;
    if (bi >= blocks) return;
    const float sc = s[bi / (K / 32)];
    const i32x4 v = *reinterpret_cast<const i32x4*>(q + bi * 16);
    h8 h[4];
    WLoad<fp4x2_t>::halves(v, ex[bi], h);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float f = (float)h[j][e] * sc;
            asm("" : "+v"(f));   // as in llm_dequant_w8_kernel: the fp32 product and the fp16 rounding stay two steps
            o[e] = (half_t)f;
        }
        *reinterpret_cast<h8*>(w16 + bi * 32 + 8 * j) = o;
    }
}

static thread_local int g_llm_gemv_variant = 0;  // 0 auto (pipelined), 1 one-column-per-wavefront kernel, 2 un-pipelined streaming kernel

// compute units of the device, asked once per process: the persistent kernels launch exactly their resident set
int cu_count(int& cus) {
    static int cached = 0;
    if (!cached) {
        int dev = 0;
        hipDeviceProp_t prop;
        DS_HIP(hipGetDevice(&dev));
        DS_HIP(hipGetDeviceProperties(&prop, dev));
        cached = prop.multiProcessorCount;
    }
    cus = cached;
    return 0;
}

template <typename WT, int MC, int SWIGLU>
int launch_gemv_stream(const LlmGemvParams& p, hipStream_t stream) {
    int cus;
    if (const int rc = cu_count(cus)) return rc;
    const size_t lds = (size_t)MC * p.K * 2 + (size_t)MC * 5 * sizeof(float);
    // resident blocks per CU: 8 x 4 wavefronts at <= 64 VGPRs (streaming kernel), 5 at ~90 VGPRs (pipelined kernel; 4 for
    // MXFP4 at ~125); launching exactly the resident set makes every wavefront walk the same number of columns (no tail round)
    const size_t by_regs = g_llm_gemv_variant == 2 ? 8 : WLoad<WT>::PIPE_BLOCKS;
    const int per_cu = (int)min(by_regs, (size_t)(160 * 1024) / (lds + 512));
    // (N = 5120 = exactly one column per resident wavefront for the o / down projections.  Fewer, longer-lived wavefronts
    // with 2-4 columns each to pipeline were measured and are slower: 5.03 -> 5.13 / 5.22 / 5.56 ms per token,
    // profiles/r02_mllm_min_cols_ab.jsonl - resident wavefronts matter more than per-wavefront prefetch here.)
    const int blocks = min((p.N + 3) / 4, cus * max(per_cu, 1));
    if constexpr (sizeof(WT) == 2) {
        if (g_llm_gemv_variant == 2) {
            hipLaunchKernelGGL((llm_gemv_stream_kernel<MC, SWIGLU>), dim3(blocks), dim3(256), lds, stream, p);
            DS_LAUNCH_CHECK();
            return 0;
        }
    }
    hipLaunchKernelGGL((llm_gemv_pipe_kernel<WT, MC, SWIGLU>), dim3(blocks), dim3(256), lds, stream, p);
    DS_LAUNCH_CHECK();
    return 0;
}

template <typename WT, int SWIGLU>
int launch_gemv(const LlmGemvParams& p, hipStream_t stream) {
    const int mcs = p.M == 1 ? 1 : p.M == 2 ? 2 : 4;  // LDS copy of x must fit the default 64 KiB dynamic limit
    if (p.M <= 4 && g_llm_gemv_variant != 1 && (size_t)mcs * p.K * 2 + 128 <= 64 * 1024) {
        if (p.M == 1) return launch_gemv_stream<WT, 1, SWIGLU>(p, stream);
        if (p.M == 2) return launch_gemv_stream<WT, 2, SWIGLU>(p, stream);
        return launch_gemv_stream<WT, 4, SWIGLU>(p, stream);
    }
    const int mc = p.M <= 1 ? 1 : p.M <= 2 ? 2 : p.M <= 4 ? 4 : p.M <= 8 ? 8 : 16;
    const dim3 grid((p.N + 3) / 4, (p.M + mc - 1) / mc);
    switch (mc) {
        case 1: hipLaunchKernelGGL((llm_gemv_kernel<WT, 1, SWIGLU>), grid, dim3(256), 0, stream, p); break;
        case 2: hipLaunchKernelGGL((llm_gemv_kernel<WT, 2, SWIGLU>), grid, dim3(256), 0, stream, p); break;
        case 4: hipLaunchKernelGGL((llm_gemv_kernel<WT, 4, SWIGLU>), grid, dim3(256), 0, stream, p); break;
        case 8: hipLaunchKernelGGL((llm_gemv_kernel<WT, 8, SWIGLU>), grid, dim3(256), 0, stream, p); break;
        default: hipLaunchKernelGGL((llm_gemv_kernel<WT, 16, SWIGLU>), grid, dim3(256), 0, stream, p); break;
    }
    DS_LAUNCH_CHECK();
    return 0;
}

constexpr int GEMM16_BLOCKS_PER_CU = 3;

template <typename WT>
int launch_gemm16(const LlmGemvParams& p, hipStream_t stream) {
    int cus;
    if (const int rc = cu_count(cus)) return rc;
    const size_t lds = (size_t)(2 * (p.swiglu ? 2 : 1) * 4 * 256 + 16) * sizeof(float) + (p.rms && p.gain ? (size_t)p.K * 2 : 0);
    // the resident set, as launch_gemv_stream sizes it: GEMM16_BLOCKS_PER_CU blocks of 4 wavefronts by registers
    const int per_cu = (int)min((size_t)GEMM16_BLOCKS_PER_CU, (size_t)(160 * 1024) / (lds + 512));
    const int blocks = min((p.N + 15) / 16, cus * max(per_cu, 1));
    if (p.swiglu) hipLaunchKernelGGL((llm_gemm16_kernel<WT, 1>), dim3(blocks), dim3(256), lds, stream, p);
    else hipLaunchKernelGGL((llm_gemm16_kernel<WT, 0>), dim3(blocks), dim3(256), lds, stream, p);
    DS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

void ds_llm_gemv_set_variant(int v) { g_llm_gemv_variant = v; }

// int8 weights (p.w_scale given): 16 weights per 16-byte load, so K % 16 == 0; the scale vector is fp32 [N] (SwiGLU [2N])
static int check_llm_w8(const LlmGemvParams& p, const char* what) {
    DS_REQUIRE(p.K >= 16 && p.K % 16 == 0, "%s: int8 weights need K %% 16 == 0 (K=%d)", what, p.K);
    return 0;
}

// MXFP4 weights (p.w_exp given): one 16-byte load is one 32-element block, so K % 32 == 0; the row scales are needed too
static int check_llm_fp4(const LlmGemvParams& p, const char* what) {
    DS_REQUIRE(p.w_scale, "%s: MXFP4 weights need their row scales (w_scale)", what);
    DS_REQUIRE(p.K >= 32 && p.K % 32 == 0, "%s: MXFP4 weights need K %% 32 == 0 (K=%d)", what, p.K);
    return 0;
}

// From the operands to the weight type: p.w_exp says MXFP4, p.w_scale alone int8, neither fp16.  Checks what the format asks
// of the shape, then calls f(a value of the WLoad element type, the format's name in messages - null for fp16).
template <typename F>
static int with_llm_weight_type(const LlmGemvParams& p, const char* what, F&& f) {
    if (p.w_exp) {
        if (const int rc = check_llm_fp4(p, what)) return rc;
        return f(fp4x2_t{}, "MXFP4");
    }
    if (p.w_scale) {
        if (const int rc = check_llm_w8(p, what)) return rc;
        return f(int8_t{}, "int8");
    }
    return f(half_t{}, nullptr);
}

int ds_launch_llm_gemv(const LlmGemvParams& p, hipStream_t stream) {
    DS_REQUIRE(p.M > 0 && p.N > 0 && p.K >= 8 && p.K % 8 == 0, "llm_gemv: bad shape M=%d N=%d K=%d", p.M, p.N, p.K);
    DS_REQUIRE(p.ldx % 8 == 0 && p.ldx >= p.K, "llm_gemv: ldx %ld must be a multiple of 8 and >= K", p.ldx);
    DS_REQUIRE(p.x && p.w && p.y, "llm_gemv: null operand");
    DS_REQUIRE(!(p.swiglu && p.residual), "llm_gemv: the SwiGLU epilogue takes no residual");
    return with_llm_weight_type(p, "llm_gemv", [&](auto wt, const char* quantised) {
        typedef decltype(wt) WT;
        DS_REQUIRE(!quantised || g_llm_gemv_variant != 2,
                   "llm_gemv: llm_gemv_variant 2 (un-pipelined streaming kernel) has no %s-weight form", quantised);
        return p.swiglu ? launch_gemv<WT, 1>(p, stream) : launch_gemv<WT, 0>(p, stream);
    });
}

int ds_launch_llm_gemm16(const LlmGemvParams& p, hipStream_t stream) {
    DS_REQUIRE(p.M > 0 && p.M <= 16 && p.N > 0 && p.K >= 8 && p.K % 8 == 0, "llm_gemm16: bad shape M=%d (1..16) N=%d K=%d",
               p.M, p.N, p.K);
    DS_REQUIRE(p.ldx % 8 == 0 && p.ldx >= p.K, "llm_gemm16: ldx %ld must be a multiple of 8 and >= K", p.ldx);
    DS_REQUIRE(p.x && p.w && p.y, "llm_gemm16: null operand");
    DS_REQUIRE(!(p.swiglu && p.residual), "llm_gemm16: the SwiGLU epilogue takes no residual");
    DS_REQUIRE(!(p.rms && p.gain) || p.K <= 20480, "llm_gemm16: K %d too long for the gain vector in LDS (20480)", p.K);
    return with_llm_weight_type(p, "llm_gemm16", [&](auto wt, const char*) { return launch_gemm16<decltype(wt)>(p, stream); });
}

int ds_launch_llm_dequant_w8(const int8_t* q, const float* scale, half_t* w16, long N, int K, hipStream_t stream) {
    DS_REQUIRE(N > 0 && K >= 16 && K % 16 == 0, "llm_dequant_w8: bad shape N=%ld K=%d (K %% 16 == 0)", N, K);
    DS_REQUIRE(q && scale && w16, "llm_dequant_w8: null operand");
    const long groups = N * (long)K / 16;
    DS_REQUIRE((groups + 255) / 256 <= 0x7fffffffL, "llm_dequant_w8: matrix too large");
    hipLaunchKernelGGL(llm_dequant_w8_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, stream, q, scale, w16,
                       groups, K);
    DS_LAUNCH_CHECK();
    return 0;
}

int ds_launch_llm_dequant_fp4(const uint8_t* q, const uint8_t* w_exp, const float* scale, half_t* w16, long N, int K,
                              hipStream_t stream) {
    DS_REQUIRE(N > 0 && K >= 32 && K % 32 == 0, "llm_dequant_fp4: bad shape N=%ld K=%d (K %% 32 == 0)", N, K);
    DS_REQUIRE(q && w_exp && scale && w16, "llm_dequant_fp4: null operand");
    const long blocks = N * (long)(K / 32);
    DS_REQUIRE((blocks + 255) / 256 <= 0x7fffffffL, "llm_dequant_fp4: matrix too large");
    hipLaunchKernelGGL(llm_dequant_fp4_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, stream, q, w_exp, scale,
                       w16, blocks, K);
    DS_LAUNCH_CHECK();
    return 0;
}

// ---- the four per-row kernels: one launcher and one argument check per kind, both row forms (ds_kernels.h; the callers in
// capi.hip pass state_stride 0 or 8, and one row to the one-sequence embed and pick)
// what both attention launchers ask of their operands (the row count is each launcher's own)
static int check_llm_attn(const LlmAttnParams& p) {
    DS_REQUIRE(p.D == 64 || p.D == 128, "llm_attn: head_dim %d unsupported (64 or 128)", p.D);
    DS_REQUIRE(p.heads > 0 && p.kv_heads > 0 && p.heads % p.kv_heads == 0, "llm_attn: heads %d / kv_heads %d", p.heads,
               p.kv_heads);
    DS_REQUIRE(p.T_max > 0 && p.T_max <= 8192, "llm_attn: cache length %d (max 8192)", p.T_max);
    DS_REQUIRE(p.ldqkv % 8 == 0 && p.ldc % 8 == 0, "llm_attn: row strides must be multiples of 8");
    DS_REQUIRE(p.qkv && p.kc && p.vc && p.rope_cos && p.rope_sin && p.out && p.state, "llm_attn: null operand");
    if (p.state_stride)   // a negative stride fails here too
        DS_REQUIRE(p.slot_stride % 8 == 0 && p.slot_stride >= (long)p.T_max * p.ldc, "llm_attn: slot stride %ld < T_max * ldc",
                   p.slot_stride);
    else DS_REQUIRE(p.slot_stride == 0, "llm_attn: the one-sequence form has one cache (slot stride %ld)", p.slot_stride);
    if (p.kv8) {
        DS_REQUIRE(p.k_exp && p.v_exp, "llm_attn: the fp8 cache needs both exponent arrays");
        DS_REQUIRE(p.ldc >= (long)p.kv_heads * p.D && p.lde >= p.kv_heads, "llm_attn: fp8 cache rows ldc %ld / lde %ld < kv_heads",
                   p.ldc, p.lde);
        if (p.state_stride)
            DS_REQUIRE(p.exp_slot_stride >= (long)p.T_max * p.lde, "llm_attn: exponent slot stride %ld < T_max * lde",
                       p.exp_slot_stride);
        else DS_REQUIRE(p.exp_slot_stride == 0, "llm_attn: the one-sequence form has one exponent array (slot stride %ld)",
                        p.exp_slot_stride);
    } else DS_REQUIRE(!p.k_exp && !p.v_exp, "llm_attn: exponent arrays belong to the fp8 cache form");
    return 0;
}

// Both attention kernel families have the same instantiations, block shape and LDS: one block of 1024 threads per (head, row),
// T_max + 16 D + 32 floats (at most 41 KB at T_max 8192).  Picks <D, KV8> and calls launch(D, KV8 as integral constants,
// grid, block, lds), which names the family and adds its own arguments.
template <typename F>
static int launch_llm_attn_form(const LlmAttnParams& p, F&& launch) {
    if (const int rc = check_llm_attn(p)) return rc;
    const size_t lds = (size_t)(p.T_max + ATT_WAVES * p.D + 2 * ATT_WAVES) * sizeof(float);
    const dim3 grid(p.heads, p.M);
    const dim3 block(64 * ATT_WAVES);
    typedef std::integral_constant<int, 128> D128;
    typedef std::integral_constant<int, 64> D64;
    if (p.D == 128 && p.kv8) launch(D128{}, std::true_type{}, grid, block, lds);
    else if (p.D == 128) launch(D128{}, std::false_type{}, grid, block, lds);
    else if (p.kv8) launch(D64{}, std::true_type{}, grid, block, lds);
    else launch(D64{}, std::false_type{}, grid, block, lds);
    DS_LAUNCH_CHECK();
    return 0;
}

int ds_launch_llm_attn(const LlmAttnParams& p, hipStream_t stream) {
    DS_REQUIRE(p.M > 0 && p.M <= 16, "llm_attn: %d rows per pass (1..16)", p.M);
    return launch_llm_attn_form(p, [&](auto d, auto kv8, dim3 grid, dim3 block, size_t lds) {
        hipLaunchKernelGGL((llm_attn_kernel<decltype(d)::value, decltype(kv8)::value>), grid, block, lds, stream, p);
    });
}

// p in the slot form (state_stride 8, the slot strides), p.M = rows of qkv / out = entries of `table` (device int32 [M][2]).
int ds_launch_llm_attn_rows(const LlmAttnParams& p, const int* table, int n_slots, hipStream_t stream) {
    DS_REQUIRE(p.M > 0 && p.M <= 65535, "llm_attn_rows: %d rows (1..65535)", p.M);
    DS_REQUIRE(table && n_slots > 0, "llm_attn_rows: the row table and the number of slots are needed");
    DS_REQUIRE(p.state_stride == 8, "llm_attn_rows: the slot form's state block is needed (stride %d)", p.state_stride);
    return launch_llm_attn_form(p, [&](auto d, auto kv8, dim3 grid, dim3 block, size_t lds) {
        hipLaunchKernelGGL((llm_attn_rows_kernel<decltype(d)::value, decltype(kv8)::value>), grid, block, lds, stream, p, table,
                           n_slots);
    });
}

int ds_launch_llm_rmsnorm(const half_t* x, long ldx, const half_t* gamma, half_t* y, long ldy, half_t* feat,
                          const int* state, int state_stride, int M, int H, int max_out, float eps, hipStream_t stream) {
    DS_REQUIRE(M > 0 && H >= 8 && H % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "llm_rmsnorm: bad shape M=%d H=%d", M, H);
    DS_REQUIRE(x && gamma && y && (!feat || state), "llm_rmsnorm: null operand");
    DS_REQUIRE(!feat || state_stride || M == 1, "llm_rmsnorm: the feature tap of one sequence is for the 1-row token loop");
    hipLaunchKernelGGL(llm_rmsnorm_kernel, dim3(M), dim3(256), 0, stream, x, ldx, gamma, y, ldy, feat, state, state_stride, H,
                       max_out, eps);
    DS_LAUNCH_CHECK();
    return 0;
}

int ds_launch_llm_embed(const half_t* table, const int* state, int state_stride, half_t* out, long ldo, int M, int H,
                        int vocab, hipStream_t stream) {
    DS_REQUIRE(M > 0 && H % 8 == 0 && vocab > 0 && ldo % 8 == 0 && ldo >= H, "llm_embed: bad shape M=%d H=%d vocab=%d", M, H,
               vocab);
    DS_REQUIRE(table && state && out, "llm_embed: null operand");
    hipLaunchKernelGGL(llm_embed_kernel, dim3((H / 8 + 255) / 256, M), dim3(256), 0, stream, table, state, state_stride, out,
                       ldo, H, vocab);
    DS_LAUNCH_CHECK();
    return 0;
}

int ds_launch_llm_select(const half_t* logits, long ldl, int V, const int* chain, int n_chain, int out_cap, int adv,
                         int* state, int state_stride, int* out_ids, int M, int pause, hipStream_t stream) {
    DS_REQUIRE(pause == 0 || pause == 1, "llm_select: pause flag %d (0 or 1)", pause);
    DS_REQUIRE(M > 0 && V > 0 && ldl >= V && n_chain >= 0 && n_chain <= 1024 && out_cap > 0 && adv >= 0,
               "llm_select: bad arguments");
    DS_REQUIRE(n_chain == 0 || chain, "llm_select: chain ids missing");
    DS_REQUIRE(logits && state && out_ids, "llm_select: null operand");
    if (pause)
        hipLaunchKernelGGL(llm_select_kernel<true>, dim3(M), dim3(1024), 0, stream, logits, ldl, V, chain, n_chain, out_cap,
                           adv, state, state_stride, out_ids);
    else
        hipLaunchKernelGGL(llm_select_kernel<false>, dim3(M), dim3(1024), 0, stream, logits, ldl, V, chain, n_chain, out_cap,
                           adv, state, state_stride, out_ids);
    DS_LAUNCH_CHECK();
    return 0;
}

int ds_launch_llm_swiglu(const half_t* gu, half_t* act, int M, int I, hipStream_t stream) {
    DS_REQUIRE(M > 0 && I >= 8 && I % 8 == 0 && gu && act, "llm_swiglu: bad shape M=%d I=%d", M, I);
    const long n8 = (long)M * I / 8;
    hipLaunchKernelGGL(llm_swiglu_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, gu, act, M, I);
    DS_LAUNCH_CHECK();
    return 0;
}

int ds_launch_blend(const half_t* a, const half_t* b, half_t* out, long n, float s, hipStream_t stream) {
    DS_REQUIRE(n > 0 && n % 8 == 0 && a && b && out, "blend: n (%ld) must be a positive multiple of 8", n);
    hipLaunchKernelGGL(blend_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, stream, a, b, out, n, s);
    DS_LAUNCH_CHECK();
    return 0;
}

int ds_launch_llm_advance(int* state, int rows, hipStream_t stream) {
    hipLaunchKernelGGL(llm_advance_kernel, dim3(1), dim3(64), 0, stream, state, rows);
    DS_LAUNCH_CHECK();
    return 0;
}
