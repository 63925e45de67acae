// C ABI (include/diffsensei_hip.h) over the kernel launchers, plus the plan executor: a flat launch list
// that replays one UNet forward (+CFG+scheduler step) with no host arithmetic, eagerly or as a hipGraph.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/diffsensei_hip.h"
#include "ds_common.h"
#include "ds_kernels.h"

static thread_local char g_err[512] = "";
void ds_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define H(x) reinterpret_cast<const half_t*>(x)
#define HM(x) reinterpret_cast<half_t*>(x)
#define S(x) reinterpret_cast<hipStream_t>(x)

extern "C" {

const char* ds_last_error(void) { return g_err; }
int ds_version(void) { return 108; }

int ds_device_info(int* cu_count, int* lds_bytes, char* arch_name, int arch_name_len) {
    int dev = 0;
    DS_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    DS_HIP(hipGetDeviceProperties(&prop, dev));
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = (int)prop.sharedMemPerBlock;
    if (arch_name && arch_name_len > 0) {
        strncpy(arch_name, prop.gcnArchName, arch_name_len - 1);
        arch_name[arch_name_len - 1] = 0;
    }
    return 0;
}

int ds_set_option(const char* key, int value) {
    DS_REQUIRE(key != nullptr, "ds_set_option: null key");
    if (strcmp(key, "gemm_variant") == 0) {
        DS_REQUIRE(value >= 0 && value <= 11, "gemm_variant must be 0..11");
        ds_gemm_set_variant(value);
        return 0;
    }
    if (strcmp(key, "ip_attn_min_blocks") == 0) {
        ds_ip_attn_set_min_blocks(value);
        return 0;
    }
    if (strcmp(key, "gn_variant") == 0) {
        DS_REQUIRE(value >= 0 && value <= 1, "gn_variant must be 0 (auto) or 1 (round-3 geometry)");
        ds_groupnorm_set_variant(value);
        return 0;
    }
    if (strcmp(key, "ip_attn_variant") == 0) {
        DS_REQUIRE(value >= 0 && value <= 3, "ip_attn_variant must be 0 (auto), 1 (register-staged), 2 (LDS-DMA ring) or 3 (register-staged, padding keys 80..95 not skipped)");
        ds_ip_attn_set_variant(value);
        return 0;
    }
    if (strcmp(key, "attn_variant") == 0) {
        DS_REQUIRE(value >= 0 && value <= 4, "attn_variant must be 0..4");
        ds_attn_set_variant(value);
        return 0;
    }
    if (strcmp(key, "conv_halo_variant") == 0) {
        DS_REQUIRE(value >= 0 && value <= 4, "conv_halo_variant must be 0..4");
        ds_conv_halo_set_variant(value);
        return 0;
    }
    if (strcmp(key, "conv_deep_blocks") == 0) {
        DS_REQUIRE(value >= 0 && value <= 8, "conv_deep_blocks must be 0..8");
        ds_conv_halo_set_deep_blocks(value);
        return 0;
    }
    if (strcmp(key, "llm_gemv_variant") == 0) {
        DS_REQUIRE(value >= 0 && value <= 2, "llm_gemv_variant must be 0..2");
        ds_llm_gemv_set_variant(value);
        return 0;
    }
    if (strcmp(key, "gemm_t160") == 0) {
        DS_REQUIRE(value >= 0 && value <= 3, "gemm_t160 must be 0 (auto), 1 (off), 2 (no 128-row tiles) or 3 (128-row tiles wherever it runs)");
        ds_gemm_set_t160(value);
        return 0;
    }
    if (strcmp(key, "gemm_g320") == 0) {
        DS_REQUIRE(value >= 0 && value <= 1, "gemm_g320 must be 0 (auto) or 1 (off)");
        ds_gemm_set_g320(value);
        return 0;
    }
    if (strcmp(key, "gemm_ring") == 0) {
        DS_REQUIRE(value >= 0 && value <= 1, "gemm_ring must be 0 (auto) or 1 (off)");
        ds_gemm_set_ring(value);
        return 0;
    }
    if (strcmp(key, "gemm_pp_narrow") == 0) {
        DS_REQUIRE(value >= 0 && value <= 1, "gemm_pp_narrow must be 0 (auto) or 1 (N, K <= 640 never on gemm_pp_kernel)");
        ds_gemm_set_pp_narrow(value);
        return 0;
    }
    if (strcmp(key, "gemm_pp_even") == 0) {
        ds_gemm_pp_set_even(value);
        return 0;
    }
    if (strcmp(key, "gemm_debug") == 0) {
        ds_gemm_set_debug(value);
        return 0;
    }
    ds_set_error("ds_set_option: unknown key '%s'", key);
    return -1;
}

int ds_gemm_t160_fits(int M, int N, int K, int batch) { return ds_gemm_t160_shape(M, N, K, batch) ? 1 : 0; }
int ds_gemm_g320_fits(int M, int N, int K, int batch) { return ds_gemm_g320_shape(M, N, K, batch) ? 1 : 0; }

int ds_debug_counter(const char* name, int reset, long long* value) {
    DS_REQUIRE(name != nullptr, "ds_debug_counter: null name");
    if (strcmp(name, "attn_sp_recentre") == 0) return ds_attn_sp_recentre_count(reset, value);
    ds_set_error("ds_debug_counter: unknown counter '%s'", name);
    return -1;
}

int ds_gemm_f16(const void* x, int64_t ldx, const void* x2, int64_t ldx2, int k1, const void* w, int64_t ldw,
                const void* bias, const void* residual, int64_t ldr, void* y, int64_t ldy, int M, int N, int K,
                int epilogue, void* stream) {
    GemmParams p;
    p.A = H(x); p.lda = ldx; p.A2 = H(x2); p.lda2 = ldx2; p.K1 = x2 ? k1 : K;
    p.W = H(w); p.ldw = ldw; p.bias = H(bias); p.residual = H(residual); p.ldr = ldr;
    p.C = HM(y); p.ldc = ldy; p.M = M; p.N = N; p.K = K; p.epi = epilogue;
    return ds_launch_gemm(p, 1, S(stream));
}

int ds_gemm_ln_f16(const void* x, int64_t ldx, const void* gw, int64_t ldw, const void* bias_ln, const float* ln_stats,
                   const void* ln_c, const void* residual, int64_t ldr, void* y, int64_t ldy, float* stats_out, int M, int N,
                   int K, int epilogue, void* stream) {
    GemmParams p;
    p.A = H(x); p.lda = ldx; p.K1 = K; p.W = H(gw); p.ldw = ldw; p.bias = H(bias_ln); p.residual = H(residual); p.ldr = ldr;
    p.C = HM(y); p.ldc = ldy; p.M = M; p.N = N; p.K = K; p.epi = epilogue;
    p.ln_stats = ln_stats; p.ln_c = H(ln_c); p.stats_out = stats_out;
    DS_REQUIRE(ln_stats || stats_out, "ds_gemm_ln_f16: neither row statistics to consume nor to emit - use ds_gemm_f16");
    return ds_launch_gemm(p, 1, S(stream));
}

int ds_gemm_ln_partial_f16(const void* x, int64_t ldx, const void* gw, int64_t ldw, const void* bias_ln, const float* ln_partial,
                           float eps, const void* ln_c, const void* residual, int64_t ldr, void* y, int64_t ldy, float* stats_out,
                           int M, int N, int K, int epilogue, void* stream) {
    GemmParams p;
    p.A = H(x); p.lda = ldx; p.K1 = K; p.W = H(gw); p.ldw = ldw; p.bias = H(bias_ln); p.residual = H(residual); p.ldr = ldr;
    p.C = HM(y); p.ldc = ldy; p.M = M; p.N = N; p.K = K; p.epi = epilogue;
    p.ln_stats = ln_partial; p.ln_partial = 1; p.ln_eps = eps; p.ln_c = H(ln_c); p.stats_out = stats_out;
    DS_REQUIRE(ln_partial && ln_c, "ds_gemm_ln_partial_f16: the partial sums and c are required");
    return ds_launch_gemm(p, 1, S(stream));
}

int ds_ln_finalize(const float* partial, float* stats, int M, int strips, int C, float eps, void* stream) {
    return ds_launch_ln_finalize(partial, stats, M, strips, C, eps, S(stream));
}

int ds_gemm_ln_swapped_f16(const void* a, int64_t lda, const void* x, int64_t ldx, int64_t sx, const float* ln_stats,
                           int64_t ln_bstride, const void* ln_cb, void* y, int64_t ldy, int64_t sy, int M, int N, int K,
                           int batch, void* stream) {
    GemmParams p;
    p.A = H(a); p.lda = lda; p.sA = 0; p.K1 = K; p.W = H(x); p.ldw = ldx; p.sW = sx;
    p.C = HM(y); p.ldc = ldy; p.sC = sy; p.M = M; p.N = N; p.K = K;
    p.ln_stats = ln_stats; p.ln_c = H(ln_cb); p.ln_swapped = 1; p.ln_bstride = ln_bstride;
    DS_REQUIRE(ln_stats && ln_cb, "ds_gemm_ln_swapped_f16: statistics and (c, b') are required");
    return ds_launch_gemm(p, batch, S(stream));
}

int ds_gemm_ln_swapped_partial_f16(const void* a, int64_t lda, const void* x, int64_t ldx, int64_t sx, const float* ln_partial,
                                   float eps, int64_t ln_rows, int64_t ln_bstride, const void* ln_cb, void* y, int64_t ldy,
                                   int64_t sy, int M, int N, int K, int batch, void* stream) {
    GemmParams p;
    p.A = H(a); p.lda = lda; p.sA = 0; p.K1 = K; p.W = H(x); p.ldw = ldx; p.sW = sx;
    p.C = HM(y); p.ldc = ldy; p.sC = sy; p.M = M; p.N = N; p.K = K;
    p.ln_stats = ln_partial; p.ln_partial = 1; p.ln_eps = eps; p.ln_rows = ln_rows; p.ln_c = H(ln_cb); p.ln_swapped = 1;
    p.ln_bstride = ln_bstride;
    DS_REQUIRE(ln_partial && ln_cb, "ds_gemm_ln_swapped_partial_f16: partial sums and (c, b') are required");
    return ds_launch_gemm(p, batch, S(stream));
}

int ds_gemm_ln_fusable(int M, int N, int K, int epilogue, int batch) { return ds_gemm_ln_kind(M, N, K, batch, epilogue); }

int ds_gemm_f16_batched(const void* x, int64_t ldx, int64_t sx, const void* w, int64_t ldw, int64_t sw, void* y,
                        int64_t ldy, int64_t sy, int M, int N, int K, int batch, void* stream) {
    GemmParams p;
    p.A = H(x); p.lda = ldx; p.sA = sx; p.K1 = K; p.W = H(w); p.ldw = ldw; p.sW = sw;
    p.C = HM(y); p.ldc = ldy; p.sC = sy; p.M = M; p.N = N; p.K = K;
    return ds_launch_gemm(p, batch, S(stream));
}

// The GemmParams of a 3x3 convolution: the one decode behind the ds_conv3x3_* entry points, the plan's CONV3X3 op (launch and
// ds_op_describe) and ds_conv3x3_gn_chunks.  `p` is filled even where an argument is refused (-1).
static int conv3x3_params(GemmParams& p, const void* x, const void* w, const void* bias, const void* rowbias, int64_t rowbias_ld,
                          const void* residual, void* y, int B, int H_, int W_, int Cin, int Cout, int stride, int upsample,
                          int dtype = DS_DTYPE_F16, int out_h = 0, int out_w = 0, float* gn_partial = nullptr,
                          int gn_chunks_planned = 0) {
    // upsample == 2: exact x2, `w` holds the four folded 2 x 2 phase weights [4][Cout][4 Cin] (ds_fold_upsample2x_f16)
    const bool fold = upsample == 2;
    p = GemmParams();
    p.conv = 1;
    p.A = H(x); p.W = H(w); p.ldw = (fold ? 4L : 9L) * Cin; p.bias = H(bias); p.rowbias = H(rowbias); p.rowbias_ld = (int)rowbias_ld;
    p.residual = H(residual); p.ldr = Cout; p.C = HM(y); p.ldc = Cout;
    p.Hin = H_; p.Win = W_; p.Cin = Cin; p.cstride = stride; p.upsample = upsample != 0; p.up_fold = fold;
    p.Hout = upsample ? (out_h ? out_h : 2 * H_) : (stride == 2 ? (H_ + 1) / 2 : H_);
    p.Wout = upsample ? (out_w ? out_w : 2 * W_) : (stride == 2 ? (W_ + 1) / 2 : W_);
    if (upsample) {  // ATen: scale = float(input_size) / output_size
        p.up_sy = (float)H_ / (float)p.Hout;
        p.up_sx = (float)W_ / (float)p.Wout;
    }
    p.M = B * p.Hout * p.Wout; p.N = Cout; p.K = 9 * Cin; p.K1 = p.K;
    p.rows_per_group = p.Hout * p.Wout;
    p.dtype = dtype;
    p.gn_partial = gn_partial;
    p.gn_chunks = gn_chunks_planned;   // checked against the kernel the launch picks (conv_halo.hip)
    DS_REQUIRE(stride == 1 || stride == 2, "conv3x3: stride must be 1 or 2");
    DS_REQUIRE(!(upsample && stride != 1), "conv3x3: upsample with stride 2 is not a thing");
    DS_REQUIRE(!fold || (dtype == DS_DTYPE_F16 && (out_h == 0 || out_h == 2 * H_) && (out_w == 0 || out_w == 2 * W_)),
               "conv3x3: folded upsample weights serve the exact x2 f16 case only");
    DS_REQUIRE((out_h == 0 && out_w == 0) || (upsample && out_h > 0 && out_w > 0),
               "conv3x3: an explicit output size needs the upsample flag");
    return 0;
}

static int conv3x3_params(GemmParams& p, const ds_op& o) {
    const int32_t* i = o.i;
    void* const* q = o.p;
    return conv3x3_params(p, q[0], q[1], q[3], q[4], i[7], q[5], q[2], i[0], i[1], i[2], i[3], i[4], i[5], i[6], DS_DTYPE_F16, i[8],
                          i[9], reinterpret_cast<float*>(q[6]), i[10]);
}

static int conv3x3_impl(const void* x, const void* w, const void* bias, const void* rowbias, int64_t rowbias_ld,
                        const void* residual, void* y, int B, int H_, int W_, int Cin, int Cout, int stride,
                        int upsample, hipStream_t stream, int dtype = DS_DTYPE_F16, int out_h = 0, int out_w = 0) {
    GemmParams p;
    if (conv3x3_params(p, x, w, bias, rowbias, rowbias_ld, residual, y, B, H_, W_, Cin, Cout, stride, upsample, dtype, out_h, out_w))
        return -1;
    return ds_launch_gemm(p, 1, stream);
}

int ds_conv3x3_gn_chunks(int B, int H_, int W_, int Cin, int Cout) {
    GemmParams p;
    if (B <= 0 || H_ <= 0 || W_ <= 0 || Cin <= 0 || Cout <= 0) return 0;
    if (conv3x3_params(p, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, B, H_, W_, Cin, Cout, 1, 0)) return 0;
    return ds_gemm_conv_gn_chunks(p);
}

int ds_conv3x3_f16(const void* x, const void* w, const void* bias, const void* rowbias, int64_t rowbias_ld,
                   const void* residual, void* y, int B, int H_, int W_, int Cin, int Cout, int stride, int upsample,
                   void* stream) {
    return conv3x3_impl(x, w, bias, rowbias, rowbias_ld, residual, y, B, H_, W_, Cin, Cout, stride, upsample != 0, S(stream));
}

int ds_conv3x3_up2fold_f16(const void* x, const void* wfold, const void* bias, const void* rowbias, int64_t rowbias_ld,
                           const void* residual, void* y, int B, int H_, int W_, int Cin, int Cout, void* stream) {
    return conv3x3_impl(x, wfold, bias, rowbias, rowbias_ld, residual, y, B, H_, W_, Cin, Cout, 1, 2, S(stream));
}

int ds_fold_upsample2x_f16(const void* w, void* wfold, int Cout, int Cin, void* stream) {
    return ds_launch_fold_upsample2x(H(w), HM(wfold), Cout, Cin, S(stream));
}

int ds_conv3x3_resize_f16(const void* x, const void* w, const void* bias, const void* rowbias, int64_t rowbias_ld,
                          const void* residual, void* y, int B, int H_, int W_, int Cin, int Cout, int Hout, int Wout,
                          void* stream) {
    return conv3x3_impl(x, w, bias, rowbias, rowbias_ld, residual, y, B, H_, W_, Cin, Cout, 1, 1, S(stream), DS_DTYPE_F16, Hout,
                        Wout);
}

// ---- bf16 entry points: the VAE decoder (fp16 overflows there; the reference runs it in fp32) ----------------------
int ds_conv3x3_bf16(const void* x, const void* w, const void* bias, const void* residual, void* y, int B, int H_,
                    int W_, int Cin, int Cout, int upsample, void* stream) {
    return conv3x3_impl(x, w, bias, nullptr, 0, residual, y, B, H_, W_, Cin, Cout, 1, upsample != 0, S(stream), DS_DTYPE_BF16);
}

int ds_gemm_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, const void* residual,
                 int64_t ldr, void* y, int64_t ldy, int M, int N, int K, void* stream) {
    GemmParams p;
    p.A = H(x); p.lda = ldx; p.K1 = K; p.W = H(w); p.ldw = ldw; p.bias = H(bias); p.residual = H(residual); p.ldr = ldr;
    p.C = HM(y); p.ldc = ldy; p.M = M; p.N = N; p.K = K; p.dtype = DS_DTYPE_BF16;
    return ds_launch_gemm(p, 1, S(stream));
}

int ds_gemm_bf16_batched(const void* x, int64_t ldx, int64_t sx, const void* w, int64_t ldw, int64_t sw, void* y,
                         int64_t ldy, int64_t sy, int M, int N, int K, int batch, void* stream) {
    GemmParams p;
    p.A = H(x); p.lda = ldx; p.sA = sx; p.K1 = K; p.W = H(w); p.ldw = ldw; p.sW = sw;
    p.C = HM(y); p.ldc = ldy; p.sC = sy; p.M = M; p.N = N; p.K = K; p.dtype = DS_DTYPE_BF16;
    return ds_launch_gemm(p, batch, S(stream));
}

int ds_groupnorm_bf16(const void* x, void* y, const void* gamma, const void* beta, void* ws, int B, int HW, int C,
                      int groups, float eps, int silu, void* stream) {
    GroupNormParams p;
    p.x1 = H(x); p.y = HM(y); p.gamma = H(gamma); p.beta = H(beta); p.ws = reinterpret_cast<float*>(ws);
    p.B = B; p.HW = HW; p.C1 = C; p.C2 = 0; p.groups = groups; p.eps = eps; p.silu = silu; p.dtype = DS_DTYPE_BF16;
    return ds_launch_groupnorm(p, S(stream));
}

int ds_wide_attn_bf16(const void* q, const void* k, const void* vt, void* o, int B, int N, int n_valid, float scale,
                      void* stream) {
    return ds_launch_wide_attn(q, k, vt, o, B, N, n_valid, DS_DTYPE_BF16, scale, S(stream));
}

int ds_vae_conv_in_bf16(const float* latents, const float* post_quant_w, const float* post_quant_b, const void* w,
                        const void* bias, void* y, int B, int H_, int W_, int C, float scaling_factor, void* stream) {
    return ds_launch_vae_conv_in(latents, post_quant_w, post_quant_b, w, bias, y, B, H_, W_, C, scaling_factor,
                                 DS_DTYPE_BF16, S(stream));
}

int ds_vae_conv_out_bf16(const void* x, const void* w, const void* bias, float* image, int B, int H_, int W_, int C,
                         int denormalize, void* stream) {
    return ds_launch_vae_conv_out(x, w, bias, image, B, H_, W_, C, denormalize, DS_DTYPE_BF16, S(stream));
}

// ---- f16 twins of the decoder entry points (the scaled-fp16 "upcast" mode of diffsensei_amd/vae.py)
int ds_groupnorm_scaled_f16(const void* x, void* y, const void* gamma, const void* beta, void* ws, int B, int HW, int C,
                            int groups, float eps, int silu, float out_scale, void* stream) {
    GroupNormParams p;
    p.x1 = H(x); p.y = HM(y); p.gamma = H(gamma); p.beta = H(beta); p.ws = reinterpret_cast<float*>(ws);
    p.B = B; p.HW = HW; p.C1 = C; p.C2 = 0; p.groups = groups; p.eps = eps; p.silu = silu; p.out_scale = out_scale;
    return ds_launch_groupnorm(p, S(stream));
}

int ds_wide_attn_f16(const void* q, const void* k, const void* vt, void* o, int B, int N, int n_valid, float scale,
                     void* stream) {
    return ds_launch_wide_attn(q, k, vt, o, B, N, n_valid, DS_DTYPE_F16, scale, S(stream));
}

int ds_vae_conv_in_f16(const float* latents, const float* post_quant_w, const float* post_quant_b, const void* w,
                       const void* bias, void* y, int B, int H_, int W_, int C, float scaling_factor, void* stream) {
    return ds_launch_vae_conv_in(latents, post_quant_w, post_quant_b, w, bias, y, B, H_, W_, C, scaling_factor,
                                 DS_DTYPE_F16, S(stream));
}

int ds_vae_conv_out_f16(const void* x, const void* w, const void* bias, float* image, int B, int H_, int W_, int C,
                        int denormalize, void* stream) {
    return ds_launch_vae_conv_out(x, w, bias, image, B, H_, W_, C, denormalize, DS_DTYPE_F16, S(stream));
}

// ---- VAE encoder (diffsensei_amd/vae.py VaeEncoderEngine)
static int conv3x3_down_impl(const void* x, const void* w, const void* bias, void* y, int B, int H_, int W_, int Cin, int Cout,
                             int dtype, hipStream_t stream) {
    DS_REQUIRE(B > 0 && H_ >= 2 && W_ >= 2, "conv3x3_down: B (%d) > 0 and H, W (%d, %d) >= 2 are needed", B, H_, W_);
    GemmParams p;
    p.conv = 1;
    p.A = H(x); p.W = H(w); p.ldw = 9L * Cin; p.bias = H(bias); p.C = HM(y); p.ldc = Cout;
    p.Hin = H_; p.Win = W_; p.Cin = Cin; p.cstride = 2; p.pad_lo = 0;
    p.Hout = H_ / 2; p.Wout = W_ / 2;
    DS_REQUIRE((long)B * H_ * W_ * Cin <= 2147483647L, "conv3x3_down: the input (%d x %d x %d x %d) exceeds 32-bit element offsets", B, H_, W_, Cin);
    p.M = B * p.Hout * p.Wout; p.N = Cout; p.K = 9 * Cin; p.K1 = p.K;
    p.rows_per_group = p.Hout * p.Wout;
    p.dtype = dtype;
    return ds_launch_gemm(p, 1, stream);
}

int ds_conv3x3_down_f16(const void* x, const void* w, const void* bias, void* y, int B, int H_, int W_, int Cin, int Cout,
                        void* stream) {
    return conv3x3_down_impl(x, w, bias, y, B, H_, W_, Cin, Cout, DS_DTYPE_F16, S(stream));
}

int ds_conv3x3_down_bf16(const void* x, const void* w, const void* bias, void* y, int B, int H_, int W_, int Cin, int Cout,
                         void* stream) {
    return conv3x3_down_impl(x, w, bias, y, B, H_, W_, Cin, Cout, DS_DTYPE_BF16, S(stream));
}

int ds_vae_enc_conv_in_f16(const void* image, int image_is_u8, const void* w, const void* bias, void* y, int B, int H_, int W_,
                           int C, void* stream) {
    return ds_launch_vae_enc_conv_in(image, image_is_u8, w, bias, y, B, H_, W_, C, DS_DTYPE_F16, S(stream));
}

int ds_vae_enc_conv_in_bf16(const void* image, int image_is_u8, const void* w, const void* bias, void* y, int B, int H_, int W_,
                            int C, void* stream) {
    return ds_launch_vae_enc_conv_in(image, image_is_u8, w, bias, y, B, H_, W_, C, DS_DTYPE_BF16, S(stream));
}

int ds_vae_enc_conv_out_f16(const void* x, const void* w, const float* bias, float* moments, int B, int H_, int W_, int C,
                            void* stream) {
    return ds_launch_vae_enc_conv_out(x, w, bias, moments, B, H_, W_, C, DS_DTYPE_F16, S(stream));
}

int ds_vae_enc_conv_out_bf16(const void* x, const void* w, const float* bias, float* moments, int B, int H_, int W_, int C,
                             void* stream) {
    return ds_launch_vae_enc_conv_out(x, w, bias, moments, B, H_, W_, C, DS_DTYPE_BF16, S(stream));
}

int ds_vae_latents_f16(const float* moments, const int64_t* seeds, const float* shift4, const float* scale4, void* latents,
                       int B, int HW, void* stream) {
    return ds_launch_vae_latents(moments, reinterpret_cast<const long long*>(seeds), shift4, scale4, HM(latents), B, HW,
                                 S(stream));
}

size_t ds_groupnorm_workspace_bytes(int B, int C) { return ds_groupnorm_ws_floats(B, C) * sizeof(float); }

int ds_groupnorm_f16(const void* x1, const void* x2, void* y, const void* gamma, const void* beta, void* ws, int B,
                     int HW, int C1, int C2, int groups, float eps, int silu, void* stream) {
    GroupNormParams p;
    p.x1 = H(x1); p.x2 = H(x2); p.y = HM(y); p.gamma = H(gamma); p.beta = H(beta); p.ws = reinterpret_cast<float*>(ws);
    p.B = B; p.HW = HW; p.C1 = C1; p.C2 = x2 ? C2 : 0; p.groups = groups; p.eps = eps; p.silu = silu;
    return ds_launch_groupnorm(p, S(stream));
}

int ds_layernorm_f16(const void* x, void* y, const void* gamma, const void* beta, int rows, int C, float eps,
                     void* stream) {
    return ds_launch_layernorm(H(x), HM(y), H(gamma), H(beta), rows, C, eps, S(stream));
}

int ds_self_attn_f16(const void* q, int64_t ldq, int64_t sq, const void* k, int64_t ldk, int64_t sk, const void* vt,
                     int64_t ldv, void* o, int64_t ldo, int64_t so, int B, int heads, int Nq, int Nk, float scale,
                     void* stream) {
    SelfAttnParams p;
    p.q = H(q); p.k = H(k); p.vt = H(vt); p.o = HM(o);
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.sq = sq; p.sk = sk; p.so = so;
    p.B = B; p.heads = heads; p.Nq = Nq; p.Nk = Nk; p.scale = scale;
    return ds_launch_self_attn(p, S(stream));
}

// THE filling of an IPAttnParams: the four entry points below and the DS_OP_IP_ATTN case.  ip_scale_rows 1: ip_scale_dev is [B].
static IPAttnParams ip_attn_params(const void* q, int64_t ldq, const void* kt, const void* vtt, const void* ki, const void* vti,
                                   const float* bbox, void* o, int64_t ldo, int B, int heads, int N, int Lt, int Li, int n_dummy,
                                   int tok_per_ip, int max_ips, int mask_h, int mask_w, float qk_scale, float ip_scale,
                                   const float* ip_scale_dev, int ip_scale_rows, int64_t ldk, int64_t sk, int64_t sv) {
    IPAttnParams p;
    p.ldk = ldk; p.sk = sk; p.sv = sv;
    p.q = H(q); p.kt = H(kt); p.vtt = H(vtt); p.ki = H(ki); p.vti = H(vti); p.bbox = bbox; p.o = HM(o);
    p.ldq = ldq; p.ldo = ldo; p.B = B; p.heads = heads; p.N = N; p.C = heads * 64;
    p.Lt = Lt; p.Li = Li; p.LP = 96; p.n_dummy = n_dummy; p.tok_per_ip = tok_per_ip; p.max_ips = max_ips;
    p.mask_h = mask_h; p.mask_w = mask_w; p.qk_scale = qk_scale;
    p.ip_scale = ip_scale; p.ip_scale_ptr = ip_scale_dev; p.ip_scale_rows = ip_scale_rows;
    return p;
}
// the long-prompt form: the same, and the text panels' count and strides
static IPAttnLongParams ip_attn_long_params(const IPAttnParams& a, int text_panels, int64_t ldkt, int64_t skt, int64_t svt) {
    IPAttnLongParams pl;
    pl.a = a; pl.T = text_panels; pl.ldkt = ldkt; pl.skt = skt; pl.svt = svt;
    return pl;
}

int ds_masked_ip_attn_f16(const void* q, int64_t ldq, const void* kt, const void* vtt, const void* ki,
                          const void* vti, const float* bbox, void* o, int64_t ldo, int B, int heads, int N, int Lt,
                          int Li, int n_dummy, int tok_per_ip, int max_ips, int mask_h, int mask_w, float qk_scale,
                          float ip_scale, const float* ip_scale_dev, int64_t ldk, int64_t sk, int64_t sv,
                          void* stream) {
    return ds_launch_ip_attn(ip_attn_params(q, ldq, kt, vtt, ki, vti, bbox, o, ldo, B, heads, N, Lt, Li, n_dummy, tok_per_ip, max_ips,
                                            mask_h, mask_w, qk_scale, ip_scale, ip_scale_dev, 0, ldk, sk, sv), S(stream));
}

int ds_masked_ip_attn_rows_f16(const void* q, int64_t ldq, const void* kt, const void* vtt, const void* ki,
                               const void* vti, const float* bbox, void* o, int64_t ldo, int B, int heads, int N, int Lt,
                               int Li, int n_dummy, int tok_per_ip, int max_ips, int mask_h, int mask_w, float qk_scale,
                               const float* ip_scale_rows_dev, int64_t ldk, int64_t sk, int64_t sv, void* stream) {
    return ds_launch_ip_attn(ip_attn_params(q, ldq, kt, vtt, ki, vti, bbox, o, ldo, B, heads, N, Lt, Li, n_dummy, tok_per_ip, max_ips,
                                            mask_h, mask_w, qk_scale, 1.0f, ip_scale_rows_dev, 1, ldk, sk, sv), S(stream));
}

int ds_masked_ip_attn_long_f16(const void* q, int64_t ldq, const void* kt, const void* vtt, const void* ki, const void* vti,
                               const float* bbox, void* o, int64_t ldo, int B, int heads, int N, int Lt, int text_panels, int Li,
                               int n_dummy, int tok_per_ip, int max_ips, int mask_h, int mask_w, float qk_scale, float ip_scale,
                               const float* ip_scale_dev, int64_t ldkt, int64_t skt, int64_t svt, int64_t ldk, int64_t sk,
                               int64_t sv, void* stream) {
    const IPAttnParams a = ip_attn_params(q, ldq, kt, vtt, ki, vti, bbox, o, ldo, B, heads, N, Lt, Li, n_dummy, tok_per_ip, max_ips,
                                          mask_h, mask_w, qk_scale, ip_scale, ip_scale_dev, 0, ldk, sk, sv);
    return ds_launch_ip_attn_long(ip_attn_long_params(a, text_panels, ldkt, skt, svt), S(stream));
}

int ds_masked_ip_attn_long_rows_f16(const void* q, int64_t ldq, const void* kt, const void* vtt, const void* ki, const void* vti,
                                    const float* bbox, void* o, int64_t ldo, int B, int heads, int N, int Lt, int text_panels,
                                    int Li, int n_dummy, int tok_per_ip, int max_ips, int mask_h, int mask_w, float qk_scale,
                                    const float* ip_scale_rows_dev, int64_t ldkt, int64_t skt, int64_t svt, int64_t ldk,
                                    int64_t sk, int64_t sv, void* stream) {
    const IPAttnParams a = ip_attn_params(q, ldq, kt, vtt, ki, vti, bbox, o, ldo, B, heads, N, Lt, Li, n_dummy, tok_per_ip, max_ips,
                                          mask_h, mask_w, qk_scale, 1.0f, ip_scale_rows_dev, 1, ldk, sk, sv);
    return ds_launch_ip_attn_long(ip_attn_long_params(a, text_panels, ldkt, skt, svt), S(stream));
}

int ds_ip_region_flags(const float* bbox, uint8_t* flags, int B, int N, int max_ips, int mask_h, int mask_w,
                       void* stream) {
    return ds_launch_ip_region_flags(bbox, flags, B, N, max_ips, mask_h, mask_w, S(stream));
}

int ds_small_attn_f16(const void* q, int64_t ldq, int64_t sq, const void* k, int64_t ldk, int64_t sk, const void* v,
                      int64_t ldv, int64_t sv, void* o, int64_t ldo, int64_t so, int B, int heads, int Nq, int Nk,
                      int D, float scale, void* stream) {
    return ds_launch_small_attn(H(q), H(k), H(v), HM(o), ldq, ldk, ldv, ldo, sq, sk, sv, so, B, heads, Nq, Nk, D, scale,
                                S(stream));
}

int ds_small_attn_causal_f16(const void* q, int64_t ldq, int64_t sq, const void* k, int64_t ldk, int64_t sk, const void* v,
                             int64_t ldv, int64_t sv, void* o, int64_t ldo, int64_t so, int B, int heads, int N, int D,
                             float scale, void* stream) {
    return ds_launch_small_attn(H(q), H(k), H(v), HM(o), ldq, ldk, ldv, ldo, sq, sk, sv, so, B, heads, N, N, D, scale,
                                S(stream), 1);
}

int ds_embed_tokens_f16(const int32_t* ids, const void* tok_emb, const void* pos_emb, void* out, int B, int T, int D,
                        int vocab, void* stream) {
    return ds_launch_embed_tokens(ids, H(tok_emb), H(pos_emb), HM(out), B, T, D, vocab, S(stream));
}

int ds_conv_in_dialog_f16(const void* x, const void* w, const void* bias, const int32_t* dialog_boxes,
                          const void* dialog_emb, void* y, int B, int H_, int W_, int Cin, int Cout, int ndialog,
                          void* stream) {
    return ds_launch_conv_in(H(x), H(w), H(bias), dialog_boxes, H(dialog_emb), HM(y), B, H_, W_, Cin, Cout, ndialog,
                             S(stream));
}

int ds_conv_out_f16(const void* x, const void* w, const void* bias, void* y, int B, int H_, int W_, int Cin, int Cout,
                    void* stream) {
    return ds_launch_conv_out(H(x), H(w), H(bias), HM(y), B, H_, W_, Cin, Cout, S(stream));
}

int ds_skinny_linear_f16(const void* x, const void* w, const void* bias, const void* addend, void* y, int M, int N,
                         int K, int silu_in, int silu_out, void* stream) {
    return ds_launch_skinny_linear(H(x), H(w), H(bias), H(addend), HM(y), M, N, K, silu_in, silu_out, S(stream));
}

// ---- MLLM pre-pass (llm.hip): LLaMA greedy decoding
// The six projection entry points and op codes are {gemv, gemm16} x the weight form: what the weights are made of and
// therefore which of w_scale / w_exp the call carries (the others are not read).
enum LlmWeights { LLM_W_F16, LLM_W_INT8, LLM_W_MXFP4 };
static LlmWeights llm_weights_of(int code) {
    return code == DS_OP_LLM_GEMV_FP4 || code == DS_OP_LLM_GEMM16_FP4 ? LLM_W_MXFP4
           : code == DS_OP_LLM_GEMV_W8 || code == DS_OP_LLM_GEMM16_W8 ? LLM_W_INT8 : LLM_W_F16;
}
static bool llm_is_gemm16(int code) {
    return code == DS_OP_LLM_GEMM16 || code == DS_OP_LLM_GEMM16_W8 || code == DS_OP_LLM_GEMM16_FP4;
}

static int llm_gemv_impl(bool gemm16, LlmWeights form, const void* x, int64_t ldx, const void* w, void* y, int64_t ldy,
                         const void* residual, int64_t ldr, int M, int N, int K, int rms, const void* rms_gain, int swiglu,
                         float eps, const void* w_scale, const void* w_exp, hipStream_t st) {
    DS_REQUIRE(form != LLM_W_INT8 || w_scale, "%s: int8 weights need their scale vector", gemm16 ? "llm_gemm16_w8" : "llm_gemv_w8");
    DS_REQUIRE(form != LLM_W_MXFP4 || (w_scale && w_exp),
               "%s: MXFP4 weights need their row scales (w_scale) and block exponents (w_exp)",
               gemm16 ? "llm_gemm16_fp4" : "llm_gemv_fp4");
    LlmGemvParams g;
    g.w_scale = form == LLM_W_F16 ? nullptr : reinterpret_cast<const float*>(w_scale);
    g.w_exp = form == LLM_W_MXFP4 ? reinterpret_cast<const uint8_t*>(w_exp) : nullptr;
    g.x = H(x); g.w = w; g.y = HM(y); g.residual = H(residual); g.gain = rms ? H(rms_gain) : nullptr;
    g.ldx = ldx; g.ldy = ldy; g.ldr = ldr; g.M = M; g.N = N; g.K = K; g.rms = rms; g.swiglu = swiglu; g.eps = eps;
    return gemm16 ? ds_launch_llm_gemm16(g, st) : ds_launch_llm_gemv(g, st);
}

// The four per-row kernels take both row forms (ds_kernels.h): SEQ for the one-sequence entry points and ops, SLOTS for
// the *_slots ones - the state stride is the only thing that tells the two families apart below.
constexpr int SEQ = 0, SLOTS = 8;

static int llm_attn_impl(const void* qkv, int64_t ldqkv, void* kc, void* vc, int64_t ldc, const float* rope_cos,
                         const float* rope_sin, void* out, int64_t ldo, const int32_t* state, int M, int heads,
                         int kv_heads, int D, int T_max, float scale, hipStream_t st, int state_stride = SEQ,
                         int64_t slot_stride = 0, bool kv8 = false, void* k_exp = nullptr, void* v_exp = nullptr,
                         int64_t lde = 0, int64_t exp_slot_stride = 0, const int32_t* row_table = nullptr, int n_slots = 0) {
    LlmAttnParams a;
    a.kv8 = kv8; a.k_exp = reinterpret_cast<uint8_t*>(k_exp); a.v_exp = reinterpret_cast<uint8_t*>(v_exp);
    a.lde = (long)lde; a.exp_slot_stride = (long)exp_slot_stride;
    a.qkv = H(qkv); a.kc = HM(kc); a.vc = HM(vc); a.rope_cos = rope_cos; a.rope_sin = rope_sin; a.out = HM(out);
    a.state = state; a.ldqkv = ldqkv; a.ldc = ldc; a.ldo = ldo;
    a.M = M; a.heads = heads; a.kv_heads = kv_heads; a.D = D; a.T_max = T_max; a.scale = scale;
    a.state_stride = state_stride; a.slot_stride = (long)slot_stride;
    if (row_table) return ds_launch_llm_attn_rows(a, row_table, n_slots, st);   // the ragged form: M rows of the table
    return ds_launch_llm_attn(a, st);
}

int ds_llm_gemv_f16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual,
                    int64_t ldr, int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, void* stream) {
    return llm_gemv_impl(false, LLM_W_F16, x, ldx, w, y, ldy, residual, ldr, M, N, K, rms, rms_gain, swiglu, eps, nullptr, nullptr,
                         S(stream));
}

int ds_llm_attn_f16(const void* qkv, int64_t ldqkv, void* k_cache, void* v_cache, int64_t ldc, const float* rope_cos,
                    const float* rope_sin, void* out, int64_t ldo, const int32_t* state, int M, int heads,
                    int kv_heads, int D, int T_max, float scale, void* stream) {
    return llm_attn_impl(qkv, ldqkv, k_cache, v_cache, ldc, rope_cos, rope_sin, out, ldo, state, M, heads, kv_heads, D,
                         T_max, scale, S(stream));
}

int ds_llm_rmsnorm_f16(const void* x, int64_t ldx, const void* gamma, void* y, int64_t ldy, void* feat,
                       const int32_t* state, int M, int Hd, int max_out, float eps, void* stream) {
    return ds_launch_llm_rmsnorm(H(x), ldx, H(gamma), HM(y), ldy, HM(feat), state, SEQ, M, Hd, max_out, eps, S(stream));
}

int ds_llm_embed_f16(const void* table, const int32_t* state, void* out, int Hd, int vocab, void* stream) {
    return ds_launch_llm_embed(H(table), state, SEQ, HM(out), Hd, 1, Hd, vocab, S(stream));
}

int ds_llm_select_f16(const void* logits, int V, const int32_t* chain, int n_chain, int out_cap, int adv,
                      int32_t* state, int32_t* out_ids, void* stream) {
    return ds_launch_llm_select(H(logits), V, V, chain, n_chain, out_cap, adv, state, SEQ, out_ids, 1, 0, S(stream));
}

int ds_llm_advance(int32_t* state, int rows, void* stream) { return ds_launch_llm_advance(state, rows, S(stream)); }

int ds_llm_swiglu_f16(const void* gate_up, void* act, int M, int I, void* stream) {
    return ds_launch_llm_swiglu(H(gate_up), HM(act), M, I, S(stream));
}

// ---- int8 weight-only (W8A16) forms: w int8 [N,K] (K % 16 == 0), w_scale fp32 [N] (SwiGLU [2N])
int ds_llm_gemv_w8(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                   int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, const float* w_scale,
                   void* stream) {
    return llm_gemv_impl(false, LLM_W_INT8, x, ldx, w, y, ldy, residual, ldr, M, N, K, rms, rms_gain, swiglu, eps, w_scale, nullptr,
                         S(stream));
}

int ds_llm_gemm16_w8(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                     int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, const float* w_scale,
                     void* stream) {
    return llm_gemv_impl(true, LLM_W_INT8, x, ldx, w, y, ldy, residual, ldr, M, N, K, rms, rms_gain, swiglu, eps, w_scale, nullptr,
                         S(stream));
}

int ds_llm_dequant_w8(const void* q, const float* w_scale, void* w16, int64_t N, int K, void* stream) {
    return ds_launch_llm_dequant_w8(reinterpret_cast<const int8_t*>(q), w_scale, HM(w16), (long)N, K, S(stream));
}

// ---- MXFP4 weight-only (W4A16) forms: w packed e2m1 [N,K/2] (K % 32 == 0), w_exp E8M0 [N,K/32], w_scale fp32 [N] (SwiGLU 2N rows)
int ds_llm_gemv_fp4(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                    int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, const float* w_scale,
                    const uint8_t* w_exp, void* stream) {
    return llm_gemv_impl(false, LLM_W_MXFP4, x, ldx, w, y, ldy, residual, ldr, M, N, K, rms, rms_gain, swiglu, eps, w_scale, w_exp,
                         S(stream));
}

int ds_llm_gemm16_fp4(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                      int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, const float* w_scale,
                      const uint8_t* w_exp, void* stream) {
    return llm_gemv_impl(true, LLM_W_MXFP4, x, ldx, w, y, ldy, residual, ldr, M, N, K, rms, rms_gain, swiglu, eps, w_scale, w_exp,
                         S(stream));
}

int ds_llm_dequant_fp4(const void* q, const float* w_scale, void* w16, int64_t N, int K, const uint8_t* w_exp, void* stream) {
    return ds_launch_llm_dequant_fp4(reinterpret_cast<const uint8_t*>(q), w_exp, w_scale, HM(w16), (long)N, K, S(stream));
}

// ---- batched decode: up to 16 sequences per weight pass
int ds_llm_gemm16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                  int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, void* stream) {
    return llm_gemv_impl(true, LLM_W_F16, x, ldx, w, y, ldy, residual, ldr, M, N, K, rms, rms_gain, swiglu, eps, nullptr, nullptr,
                         S(stream));
}

int ds_llm_attn_slots_f16(const void* qkv, int64_t ldqkv, void* k_cache, void* v_cache, int64_t ldc, int64_t slot_stride,
                          const float* rope_cos, const float* rope_sin, void* out, int64_t ldo, const int32_t* state,
                          int slots, int heads, int kv_heads, int D, int T_max, float scale, void* stream) {
    return llm_attn_impl(qkv, ldqkv, k_cache, v_cache, ldc, rope_cos, rope_sin, out, ldo, state, slots, heads, kv_heads, D,
                         T_max, scale, S(stream), SLOTS, slot_stride);
}

// ---- fp8 KV cache: uint8 e4m3 caches (ldc, slot_stride in bytes) + uint8 exponent arrays [T_max, kv_heads] rows (lde)
int ds_llm_attn_kv8(const void* qkv, int64_t ldqkv, void* k_cache, void* v_cache, int64_t ldc, void* k_exp, void* v_exp,
                    int64_t lde, const float* rope_cos, const float* rope_sin, void* out, int64_t ldo, const int32_t* state,
                    int M, int heads, int kv_heads, int D, int T_max, float scale, void* stream) {
    return llm_attn_impl(qkv, ldqkv, k_cache, v_cache, ldc, rope_cos, rope_sin, out, ldo, state, M, heads, kv_heads, D,
                         T_max, scale, S(stream), SEQ, 0, true, k_exp, v_exp, lde, 0);
}

int ds_llm_attn_slots_kv8(const void* qkv, int64_t ldqkv, void* k_cache, void* v_cache, int64_t ldc, int64_t slot_stride,
                          void* k_exp, void* v_exp, int64_t lde, int64_t exp_slot_stride, const float* rope_cos,
                          const float* rope_sin, void* out, int64_t ldo, const int32_t* state, int slots, int heads,
                          int kv_heads, int D, int T_max, float scale, void* stream) {
    return llm_attn_impl(qkv, ldqkv, k_cache, v_cache, ldc, rope_cos, rope_sin, out, ldo, state, slots, heads, kv_heads, D,
                         T_max, scale, S(stream), SLOTS, slot_stride, true, k_exp, v_exp, lde, exp_slot_stride);
}

int ds_llm_rmsnorm_slots_f16(const void* x, int64_t ldx, const void* gamma, void* y, int64_t ldy, void* feat,
                             const int32_t* state, int slots, int Hd, int max_out, float eps, void* stream) {
    return ds_launch_llm_rmsnorm(H(x), ldx, H(gamma), HM(y), ldy, HM(feat), state, SLOTS, slots, Hd, max_out, eps, S(stream));
}

int ds_llm_embed_slots_f16(const void* table, const int32_t* state, void* out, int64_t ldo, int slots, int Hd, int vocab,
                           void* stream) {
    return ds_launch_llm_embed(H(table), state, SLOTS, HM(out), ldo, slots, Hd, vocab, S(stream));
}

int ds_llm_select_slots_f16(const void* logits, int64_t ldl, int V, const int32_t* chain, int n_chain, int out_cap, int adv,
                            int32_t* state, int32_t* out_ids, int slots, void* stream) {
    return ds_launch_llm_select(H(logits), ldl, V, chain, n_chain, out_cap, adv, state, SLOTS, out_ids, slots, 0, S(stream));
}

int ds_resize_h_u8(const uint8_t* src, int H_, int W_, const int32_t* first, const int32_t* count, const int32_t* taps,
                   int ksize, int out_w, uint8_t* dst, void* stream) {
    return ds_launch_resize_h(src, H_, W_, first, count, taps, ksize, out_w, dst, S(stream));
}

int ds_resize_v_norm_u8(const uint8_t* tmp, int Ht, int Wt, const int32_t* first, const int32_t* count,
                        const int32_t* taps, int ksize, int top, int left, int out_h, int out_w, float scale,
                        const float* mean3, const float* std3, float* out_f32, uint8_t* out_u8, void* stream) {
    return ds_launch_resize_v_norm(tmp, Ht, Wt, first, count, taps, ksize, top, left, out_h, out_w, scale, mean3, std3,
                                   out_f32, out_u8, S(stream));
}

int ds_blend_f16(const void* a, const void* b, void* out, int64_t n, float scale, void* stream) {
    return ds_launch_blend(H(a), H(b), HM(out), (long)n, scale, S(stream));
}

int ds_timestep_embed_f16(const float* table, const int32_t* step_ctr, void* out, int B, int dim, int flip,
                          float freq_shift, void* stream) {
    return ds_launch_timestep_embed(table, step_ctr, HM(out), B, dim, flip, freq_shift, S(stream));
}

int ds_add_time_ids_f16(const void* text_embeds, const void* time_ids, void* out, int B, int pooled_dim, int n_ids,
                        int dim, int flip, float freq_shift, void* stream) {
    return ds_launch_add_time_ids(H(text_embeds), H(time_ids), HM(out), B, pooled_dim, n_ids, dim, flip, freq_shift,
                                  S(stream));
}

int ds_cfg_sampler_step_f16(const void* eps, void* latents, void* model_in, const float* table,
                            const int32_t* step_ctr, int ns, int HW, int kind, int do_cfg, void* stream) {
    SamplerStepParams p;
    p.eps = H(eps); p.latents = HM(latents); p.model_in = HM(model_in); p.coef = table;
    p.ns = ns; p.HW = HW; p.kind = kind; p.do_cfg = do_cfg;
    return ds_launch_sampler_step(p, step_ctr, S(stream));
}

int ds_cfg_dpm_step_f16(const void* eps, void* latents, void* model_in, const float* table, const float* solver,
                        void* prev_x0, const int32_t* step_ctr, int ns, int HW, int do_cfg, void* stream) {
    SamplerStepParams p;
    p.eps = H(eps); p.latents = HM(latents); p.model_in = HM(model_in); p.coef = table;
    p.solver = solver; p.prev_x0 = HM(prev_x0);
    p.ns = ns; p.HW = HW; p.kind = 2; p.do_cfg = do_cfg;
    return ds_launch_sampler_step(p, step_ctr, S(stream));
}

int ds_cfg_sampler_step_noise_f16(const void* eps, void* latents, void* model_in, const float* table,
                                  const int64_t* seeds, const int32_t* step_ctr, int ns, int HW, int kind, int do_cfg,
                                  void* stream) {
    SamplerStepParams p;
    p.eps = H(eps); p.latents = HM(latents); p.model_in = HM(model_in); p.coef = table;
    p.seeds = reinterpret_cast<const long long*>(seeds);
    p.ns = ns; p.HW = HW; p.kind = kind; p.do_cfg = do_cfg;
    return ds_launch_sampler_step(p, step_ctr, S(stream));
}

int ds_cfg_sampler_step_panels_f16(const void* eps, void* latents, void* model_in, const float* table,
                                   const float* guidance, const float* solver, void* prev_x0, const int64_t* seeds,
                                   const int32_t* step_ctr, int ns, int HW, int kind, int do_cfg, void* stream) {
    SamplerStepParams p;
    p.eps = H(eps); p.latents = HM(latents); p.model_in = HM(model_in); p.coef = table;
    p.guidance = guidance; p.solver = solver; p.prev_x0 = HM(prev_x0);
    p.seeds = reinterpret_cast<const long long*>(seeds);
    p.ns = ns; p.HW = HW; p.kind = kind; p.do_cfg = do_cfg;
    return ds_launch_sampler_step(p, step_ctr, S(stream));
}

int ds_cfg_sampler_step_redraw_f16(const void* eps, void* latents, void* model_in, const float* table,
                                   const float* guidance, const float* solver, void* prev_x0, const int64_t* seeds,
                                   const void* redraw, const int32_t* step_ctr, int ns, int HW, int kind, int do_cfg,
                                   void* stream) {
    SamplerStepParams p;
    p.eps = H(eps); p.latents = HM(latents); p.model_in = HM(model_in); p.coef = table;
    p.guidance = guidance; p.solver = solver; p.prev_x0 = HM(prev_x0);
    p.seeds = reinterpret_cast<const long long*>(seeds);
    p.redraw = redraw; p.redraw_on = 1;
    p.ns = ns; p.HW = HW; p.kind = kind; p.do_cfg = do_cfg;
    return ds_launch_sampler_step(p, step_ctr, S(stream));
}

int64_t ds_redraw_buffer_bytes(int ns, int HW) {
    return (int64_t)ds_redraw_f32_offset(ns, HW) + (int64_t)sizeof(float) * (4 + 2 * DS_REDRAW_MAX_ROWS);
}

int ds_redraw_start_f16(const void* redraw, void* latents, int ns, int HW, void* stream) {
    return ds_launch_redraw_start(redraw, HM(latents), ns, HW, S(stream));
}

// ---- panel schedules (continuous batching)
int64_t ds_panel_schedule_bytes(int ns) { return ns > 0 ? (int64_t)ds_panel_bytes(ns) : 0; }

int ds_panel_slot_load(void* panel, int ns, int slot, int start, int steps, const float* coef_rows, const float* solver_rows,
                       const float* renoise_rows, int start_mode, float init_noise_sigma, void* stream) {
    DS_REQUIRE(panel != nullptr, "panel_slot_load: null panel-schedule buffer");
    DS_REQUIRE(((uintptr_t)panel & 15) == 0, "panel_slot_load: the panel-schedule buffer must be 16-byte aligned");
    DS_REQUIRE(ns > 0 && slot >= 0 && slot < ns, "panel_slot_load: slot %d outside the %d panels", slot, ns);
    DS_REQUIRE(steps >= 0 && steps <= DS_PANEL_MAX_ROWS, "panel_slot_load: steps[%d] = %d exceeds the row capacity %d", slot, steps,
               DS_PANEL_MAX_ROWS);
    DS_REQUIRE(start >= 0, "panel_slot_load: start %d is negative", start);
    DS_REQUIRE((((uintptr_t)coef_rows | (uintptr_t)solver_rows | (uintptr_t)renoise_rows) & 3) == 0,
               "panel_slot_load: the rows are fp32 arrays, 4-byte aligned");
    DS_REQUIRE(steps == 0 || coef_rows, "panel_slot_load: %d steps without coefficient rows", steps);
    DS_REQUIRE(start_mode >= DS_PANEL_START_RENOISE && start_mode <= DS_PANEL_START_KEEP, "panel_slot_load: start mode %d", start_mode);
    DS_REQUIRE(start_mode != DS_PANEL_START_RENOISE || renoise_rows || steps == 0,
               "panel_slot_load: start mode 0 (renoise row 0) without renoise rows");
    return ds_launch_panel_slot_load(panel, ns, slot, start, steps, coef_rows, solver_rows, renoise_rows, start_mode,
                                     init_noise_sigma, S(stream));
}

int ds_cfg_sampler_step_slots_f16(const void* eps, void* latents, void* model_in, const void* panel, const float* guidance,
                                  void* prev_x0, const int64_t* seeds, const void* redraw, const int32_t* step_ctr, int ns,
                                  int HW, int kind, int do_cfg, void* stream) {
    SamplerStepParams p;
    p.eps = H(eps); p.latents = HM(latents); p.model_in = HM(model_in); p.coef = reinterpret_cast<const float*>(panel);
    p.guidance = guidance; p.prev_x0 = HM(prev_x0);
    p.seeds = reinterpret_cast<const long long*>(seeds);
    p.redraw = redraw; p.redraw_on = redraw != nullptr;
    p.ns = ns; p.HW = HW; p.kind = kind; p.do_cfg = do_cfg;
    return ds_launch_sampler_step_panels(p, step_ctr, S(stream));
}

int ds_timestep_embed_slots_f16(const void* panel, const int32_t* step_ctr, void* out, int B, int dim, int flip,
                                float freq_shift, int ns, void* stream) {
    return ds_launch_timestep_embed_panels(panel, step_ctr, HM(out), B, dim, flip, freq_shift, ns, S(stream));
}

int ds_panel_slot_start_f16(const void* panel, const void* redraw, void* latents, void* model_in, int ns, int HW, int do_cfg,
                            int slot0, int nslots, void* stream) {
    return ds_launch_panel_slot_start(panel, redraw, HM(latents), HM(model_in), ns, HW, do_cfg, slot0, nslots, S(stream));
}

int ds_philox_u32(const int64_t* seeds, int step, int stream_id, uint32_t* out, int ns, int HW, void* stream) {
    return ds_launch_philox_u32(reinterpret_cast<const long long*>(seeds), step, stream_id, out, ns, HW, S(stream));
}

int ds_philox_normal_f32(const int64_t* seeds, int step, int stream_id, float* out, int ns, int HW, void* stream) {
    return ds_launch_philox_normal(reinterpret_cast<const long long*>(seeds), step, stream_id, out, ns, HW, S(stream));
}

int ds_prepare_model_input_f16(const void* latents, void* model_in, const float* table, const int32_t* step_ctr,
                               int ns, int HW, int do_cfg, void* stream) {
    return ds_launch_prepare_model_input(H(latents), HM(model_in), table, step_ctr, ns, HW, 4, do_cfg, S(stream));
}

int ds_nhwc_to_nchw_f16(const void* x, void* y, int B, int HW, int C, void* stream) {
    return ds_launch_nhwc_to_nchw(H(x), HM(y), B, HW, C, S(stream));
}
int ds_nchw_to_nhwc_f16(const void* x, void* y, int B, int HW, int C, void* stream) {
    return ds_launch_nchw_to_nhwc(H(x), HM(y), B, HW, C, S(stream));
}
int ds_image_f32_to_u8_nhwc(const float* image, uint8_t* out, int B, int H_, int W_, void* stream) {
    return ds_launch_image_to_u8(image, out, B, H_, W_, S(stream));
}
int ds_pad_rows_f16(const void* x, void* y, int B, int rows_in, int rows_out, int row_off, int total_rows, int C,
                    void* stream) {
    return ds_launch_pad_rows(H(x), HM(y), B, rows_in, rows_out, row_off, total_rows, C, S(stream));
}

// ---------------------------------------------------------------------------------------- plan executor
static LoraMergeParams lora_merge_params(const ds_op& o) {
    const int32_t* i = o.i;
    const int64_t* l = o.l;
    void* const* p = o.p;
    LoraMergeParams m;
    m.W = H(p[0]); m.out = HM(p[1]); m.A = H(p[2]); m.B = H(p[3]);
    m.seg = reinterpret_cast<const int*>(p[4]); m.s = reinterpret_cast<const float*>(p[5]);
    m.map = reinterpret_cast<const int*>(p[6]); m.colscale = H(p[7]); m.out2 = HM(p[8]);
    m.N = i[0]; m.K = i[1]; m.R = i[2]; m.nseg = i[3]; m.cin = i[4];
    m.ldw = l[0]; m.ldo = l[1]; m.lda = l[2]; m.ldb = l[3]; m.ldo2 = l[4];
    return m;
}

// The GemmParams of a DS_OP_GEMM: the one decode of its slots (include/diffsensei_hip.h), for the launch and for ds_op_describe
static GemmParams gemm_params(const ds_op& o) {
    const int32_t* i = o.i;
    const int64_t* l = o.l;
    void* const* p = o.p;
    GemmParams g;
    g.A = H(p[0]); g.A2 = H(p[1]); g.W = H(p[2]); g.C = HM(p[3]); g.bias = H(p[4]); g.rowbias = H(p[5]);
    g.residual = H(p[6]);
    g.lda = l[0]; g.lda2 = l[1]; g.ldw = l[2]; g.ldc = l[3]; g.ldr = l[4];
    g.sA = l[5]; g.sA2 = l[6]; g.sW = l[7]; g.sC = l[8]; g.sR = l[9];
    g.M = i[0]; g.N = i[1]; g.K = i[2]; g.K1 = g.A2 ? i[3] : i[2];
    g.epi = i[4];
    g.rowbias_ld = i[6]; g.rows_per_group = i[7] > 0 ? i[7] : 1;
    g.ln_stats = reinterpret_cast<const float*>(p[7]); g.ln_c = H(p[8]); g.stats_out = reinterpret_cast<float*>(p[9]);
    g.ln_swapped = i[8]; g.ln_bstride = l[10];
    g.ln_partial = i[9]; g.ln_eps = i[9] ? o.f[0] : g.ln_eps; g.ln_rows = l[11];
    g.ln_nstrips = i[10]; g.stats_strip = i[11];
    return g;
}
static int gemm_batch(const ds_op& o) { return o.i[5] > 0 ? o.i[5] : 1; }

static int run_op(const ds_op& o, hipStream_t st) {
    const int32_t* i = o.i;
    const int64_t* l = o.l;
    void* const* p = o.p;
    switch (o.code) {
        case DS_OP_GEMM:
            return ds_launch_gemm(gemm_params(o), gemm_batch(o), st);
        case DS_OP_LN_FINALIZE:
            return ds_launch_ln_finalize(reinterpret_cast<const float*>(p[0]), reinterpret_cast<float*>(p[1]), i[0], i[1], i[2],
                                         o.f[0], st);
        case DS_OP_CONV3X3: {
            GemmParams g;
            if (conv3x3_params(g, o)) return -1;
            return ds_launch_gemm(g, 1, st);
        }
        case DS_OP_GROUPNORM: {
            GroupNormParams g;
            g.x1 = H(p[0]); g.x2 = H(p[1]); g.y = HM(p[2]); g.gamma = H(p[3]); g.beta = H(p[4]);
            g.ws = reinterpret_cast<float*>(p[5]);
            g.B = i[0]; g.HW = i[1]; g.C1 = i[2]; g.C2 = p[1] ? i[3] : 0; g.groups = i[4]; g.silu = i[5]; g.eps = o.f[0];
            g.pre_chunks = i[6];
            return ds_launch_groupnorm(g, st);
        }
        case DS_OP_LAYERNORM:
            return ds_launch_layernorm(H(p[0]), HM(p[1]), H(p[2]), H(p[3]), i[0], i[1], o.f[0], st);
        case DS_OP_SELF_ATTN: {
            SelfAttnParams a;
            a.q = H(p[0]); a.k = H(p[1]); a.vt = H(p[2]); a.o = HM(p[3]);
            a.ldq = l[0]; a.ldk = l[1]; a.ldv = l[2]; a.ldo = l[3]; a.sq = l[4]; a.sk = l[5]; a.so = l[6];
            a.B = i[0]; a.heads = i[1]; a.Nq = i[2]; a.Nk = i[3]; a.scale = o.f[0];
            return ds_launch_self_attn(a, st);
        }
        case DS_OP_IP_ATTN: {
            const IPAttnParams a = ip_attn_params(p[0], l[0], p[1], p[2], p[3], p[4], reinterpret_cast<const float*>(p[5]), p[6], l[1],
                                                  i[0], i[1], i[2], i[3], i[4], i[5], i[6], i[7], i[8], i[9], o.f[0], o.f[1],
                                                  reinterpret_cast<const float*>(p[7]), i[10], l[2], l[3], l[4]);
            if (i[11] > 1)   // long prompt: i[11] text panels with the strides l[5..7] of their own
                return ds_launch_ip_attn_long(ip_attn_long_params(a, i[11], l[5], l[6], l[7]), st);
            return ds_launch_ip_attn(a, st);
        }
        case DS_OP_CONV_IN:
            return ds_launch_conv_in(H(p[0]), H(p[1]), H(p[2]), reinterpret_cast<const int*>(p[3]), H(p[4]), HM(p[5]),
                                     i[0], i[1], i[2], i[3], i[4], i[5], st);
        case DS_OP_CONV_OUT:
            return ds_launch_conv_out(H(p[0]), H(p[1]), H(p[2]), HM(p[3]), i[0], i[1], i[2], i[3], i[4], st);
        case DS_OP_SKINNY:
            return ds_launch_skinny_linear(H(p[0]), H(p[1]), H(p[2]), H(p[3]), HM(p[4]), i[0], i[1], i[2], i[3], i[4], st);
        case DS_OP_TIMESTEP_EMBED:
            if (i[3] > 0)   // panel schedules: p[0] is the panel-schedule buffer, i[3] = ns
                return ds_launch_timestep_embed_panels(p[0], reinterpret_cast<const int*>(p[1]), HM(p[2]), i[0], i[1], i[2],
                                                       o.f[0], i[3], st);
            return ds_launch_timestep_embed(reinterpret_cast<const float*>(p[0]), reinterpret_cast<const int*>(p[1]),
                                            HM(p[2]), i[0], i[1], i[2], o.f[0], st);
        case DS_OP_ADD_TIME_IDS:
            return ds_launch_add_time_ids(H(p[0]), H(p[1]), HM(p[2]), i[0], i[1], i[2], i[3], i[4], o.f[0], st);
        case DS_OP_SAMPLER_STEP: {
            SamplerStepParams s;
            s.eps = H(p[0]); s.latents = HM(p[1]); s.model_in = HM(p[2]); s.coef = reinterpret_cast<const float*>(p[3]);
            s.prev_x0 = HM(p[5]); s.solver = reinterpret_cast<const float*>(p[6]);
            s.seeds = reinterpret_cast<const long long*>(p[7]);
            s.guidance = reinterpret_cast<const float*>(p[8]);
            s.redraw = p[9]; s.redraw_on = i[4];
            s.ns = i[0]; s.HW = i[1]; s.kind = i[2]; s.do_cfg = i[3];
            if (i[5]) {     // panel schedules: p[3] is the panel-schedule buffer, the solver rows live in it
                s.solver = nullptr;
                return ds_launch_sampler_step_panels(s, reinterpret_cast<const int*>(p[4]), st);
            }
            return ds_launch_sampler_step(s, reinterpret_cast<const int*>(p[4]), st);
        }
        case DS_OP_REDRAW_START:
            return ds_launch_redraw_start(p[0], HM(p[1]), i[0], i[1], st);
        case DS_OP_SLOT_START:
            return ds_launch_panel_slot_start(p[0], p[1], HM(p[2]), HM(p[3]), i[0], i[1], i[2], i[3], i[4], st);
        case DS_OP_PREP_INPUT:
            return ds_launch_prepare_model_input(H(p[0]), HM(p[1]), reinterpret_cast<const float*>(p[2]),
                                                 reinterpret_cast<const int*>(p[3]), i[0], i[1], 4, i[2], st);
        case DS_OP_ADVANCE:
            return ds_launch_advance_counter(reinterpret_cast<int*>(p[0]), st);
        case DS_OP_NHWC2NCHW:
            return ds_launch_nhwc_to_nchw(H(p[0]), HM(p[1]), i[0], i[1], i[2], st);
        case DS_OP_NCHW2NHWC:
            return ds_launch_nchw_to_nhwc(H(p[0]), HM(p[1]), i[0], i[1], i[2], st);
        case DS_OP_PAD_ROWS:
            return ds_launch_pad_rows(H(p[0]), HM(p[1]), i[0], i[1], i[2], i[3], i[4], i[5], st);
        case DS_OP_SMALL_ATTN:
            return ds_launch_small_attn(H(p[0]), H(p[1]), H(p[2]), HM(p[3]), l[0], l[1], l[2], l[3], l[4], l[5], l[6],
                                        l[7], i[0], i[1], i[2], i[3], i[4], o.f[0], st);
        case DS_OP_LLM_GEMV:
        case DS_OP_LLM_GEMM16:
        case DS_OP_LLM_GEMV_W8:
        case DS_OP_LLM_GEMM16_W8:
        case DS_OP_LLM_GEMV_FP4:
        case DS_OP_LLM_GEMM16_FP4: {   // one slot layout; p[5] (row scales) and p[6] (block exponents) by weight form
            const LlmWeights form = llm_weights_of(o.code);
            return llm_gemv_impl(llm_is_gemm16(o.code), form, p[0], l[0], p[1], p[2], l[1], p[3], l[2], i[0], i[1], i[2], i[3], p[4],
                                 i[4], o.f[0], form != LLM_W_F16 ? p[5] : nullptr, form == LLM_W_MXFP4 ? p[6] : nullptr, st);
        }
        case DS_OP_LLM_ATTN:
        case DS_OP_LLM_ATTN_SLOTS:
        case DS_OP_LLM_ATTN_KV8:
        case DS_OP_LLM_ATTN_SLOTS_KV8:
        case DS_OP_LLM_ATTN_ROWS:
        case DS_OP_LLM_ATTN_ROWS_KV8: {   // one slot layout; the slot strides, exponent planes and row table by form
            const bool rows = o.code == DS_OP_LLM_ATTN_ROWS || o.code == DS_OP_LLM_ATTN_ROWS_KV8;
            const bool kv8 = o.code == DS_OP_LLM_ATTN_KV8 || o.code == DS_OP_LLM_ATTN_SLOTS_KV8 || o.code == DS_OP_LLM_ATTN_ROWS_KV8;
            const bool slots = rows || o.code == DS_OP_LLM_ATTN_SLOTS || o.code == DS_OP_LLM_ATTN_SLOTS_KV8;
            // without a table the launch fails (never the slot form by accident)
            DS_REQUIRE(!rows || p[9], "%s: p[9], the row table, is missing", kv8 ? "DS_OP_LLM_ATTN_ROWS_KV8" : "DS_OP_LLM_ATTN_ROWS");
            return llm_attn_impl(p[0], l[0], p[1], p[2], l[1], reinterpret_cast<const float*>(p[3]),
                                 reinterpret_cast<const float*>(p[4]), p[5], l[2], reinterpret_cast<const int32_t*>(p[6]),
                                 i[0], i[1], i[2], i[3], i[4], o.f[0], st, slots ? SLOTS : SEQ, slots ? l[3] : 0, kv8,
                                 kv8 ? p[7] : nullptr, kv8 ? p[8] : nullptr, kv8 ? l[4] : 0, kv8 && slots ? l[5] : 0,
                                 rows ? reinterpret_cast<const int32_t*>(p[9]) : nullptr, rows ? i[5] : 0);
        }
        case DS_OP_LLM_RMSNORM:
            return ds_launch_llm_rmsnorm(H(p[0]), l[0], H(p[1]), HM(p[2]), l[1], HM(p[3]),
                                         reinterpret_cast<const int*>(p[4]), SEQ, i[0], i[1], i[2], o.f[0], st);
        case DS_OP_LLM_EMBED:
            return ds_launch_llm_embed(H(p[0]), reinterpret_cast<const int*>(p[1]), SEQ, HM(p[2]), i[0], 1, i[0], i[1], st);
        case DS_OP_LLM_SELECT:
            return ds_launch_llm_select(H(p[0]), i[0], i[0], reinterpret_cast<const int*>(p[1]), i[1], i[2], i[3],
                                        reinterpret_cast<int*>(p[2]), SEQ, reinterpret_cast<int*>(p[3]), 1, i[4], st);
        case DS_OP_LLM_ADVANCE:
            return ds_launch_llm_advance(reinterpret_cast<int*>(p[0]), i[0], st);
        case DS_OP_LLM_RMSNORM_SLOTS:
            return ds_launch_llm_rmsnorm(H(p[0]), l[0], H(p[1]), HM(p[2]), l[1], HM(p[3]),
                                         reinterpret_cast<const int*>(p[4]), SLOTS, i[0], i[1], i[2], o.f[0], st);
        case DS_OP_LLM_EMBED_SLOTS:
            return ds_launch_llm_embed(H(p[0]), reinterpret_cast<const int*>(p[1]), SLOTS, HM(p[2]), l[0], i[0], i[1], i[2], st);
        case DS_OP_LLM_SELECT_SLOTS:
            return ds_launch_llm_select(H(p[0]), l[0], i[0], reinterpret_cast<const int*>(p[1]), i[1], i[2], i[3],
                                        reinterpret_cast<int*>(p[2]), SLOTS, reinterpret_cast<int*>(p[3]), i[4], i[5], st);
        case DS_OP_LORA_MERGE:
            return ds_launch_lora_merge(lora_merge_params(o), st);
        default:
            ds_set_error("plan: unknown opcode %d", o.code);
            return -4;
    }
}

// Static description of one op for roofline accounting: the gfx950 kernel it dispatches to (same spelling as the
// rocprofv3 kernel trace), its ALGORITHMIC flops (2*MAC) and its algorithmic HBM bytes (each operand once).
int ds_op_describe(const ds_op* op, char* name, int name_len, double* flops, double* bytes) {
    DS_REQUIRE(op != nullptr, "ds_op_describe: null op");
    const int32_t* i = op->i;
    const char* nm = "other";
    double fl = 0, by = 0;
    switch (op->code) {
        case DS_OP_GEMM: {
            const int batch = gemm_batch(*op);
            nm = ds_gemm_kernel_name(gemm_params(*op), batch);
            fl = 2.0 * i[0] * (double)i[1] * i[2] * batch;
            by = 2.0 * batch * ((double)i[0] * i[2] + (double)i[1] * i[2] + (double)i[0] * (i[4] == 1 || i[4] == 4 ? i[1] / 2 : i[1]));
            break;
        }
        case DS_OP_CONV3X3: {
            GemmParams g;
            nm = conv3x3_params(g, *op) == 0 ? ds_gemm_kernel_name(g, 1) : "refused";
            // i[6] == 2 (folded x2 upsample, 4 taps executed): still the ALGORITHMIC work of the nearest x2 + 3 x 3 it replaces
            fl = 2.0 * g.M * (double)g.N * g.K;
            by = 2.0 * ((double)i[0] * i[1] * i[2] * i[3] + (double)g.N * g.K + (double)g.M * g.N);
            break;
        }
        case DS_OP_GROUPNORM: nm = "groupnorm(3 kernels)"; by = 2.0 * 2.0 * i[0] * (double)i[1] * (i[2] + i[3]); break;
        case DS_OP_LAYERNORM: nm = "layernorm_kernel"; by = 2.0 * 2.0 * i[0] * (double)i[1]; break;
        case DS_OP_LN_FINALIZE: nm = "ln_finalize_kernel"; by = 8.0 * i[0] * (double)(i[1] + 1); break;
        case DS_OP_SELF_ATTN:
            nm = ds_self_attn_kernel_name(i[0], i[1], i[2], i[3]);
            fl = 4.0 * i[0] * (double)i[1] * i[2] * (double)i[3] * 64;
            by = 2.0 * i[0] * (double)i[1] * 64 * (2.0 * i[2] + 2.0 * i[3]);
            break;
        case DS_OP_IP_ATTN:
            nm = i[11] > 1 ? "ip_attn_long_kernel" : "ip_attn_kernel";
            fl = 4.0 * i[0] * (double)i[1] * i[2] * (double)(i[3] + i[4]) * 64;
            by = 2.0 * i[0] * (double)i[1] * 64 * (2.0 * i[2] + 2.0 * (i[3] + i[4]));
            break;
        case DS_OP_SMALL_ATTN: nm = "small_attn_kernel"; fl = 4.0 * i[0] * (double)i[1] * i[2] * (double)i[3] * i[4]; break;
        case DS_OP_CONV_IN: nm = "conv_in_kernel"; fl = 2.0 * i[0] * (double)i[1] * i[2] * 9 * i[3] * i[4]; break;
        case DS_OP_CONV_OUT: nm = "conv_out_kernel"; fl = 2.0 * i[0] * (double)i[1] * i[2] * 9 * i[3] * i[4]; break;
        case DS_OP_SKINNY: nm = "skinny_linear_kernel"; fl = 2.0 * i[0] * (double)i[1] * i[2]; by = 2.0 * i[1] * (double)i[2]; break;
        case DS_OP_TIMESTEP_EMBED: nm = i[3] > 0 ? "timestep_embed_panels_kernel" : "other"; break;   // (the one-table launch keeps the name it had)
        case DS_OP_SAMPLER_STEP: nm = "sampler_step_kernel"; break;    // every instantiation, panel schedules (i[5]) included
        case DS_OP_SLOT_START: nm = "panel_slot_start_kernel"; by = 2.0 * 3.0 * i[4] * 4.0 * i[1]; break;
        case DS_OP_REDRAW_START: nm = "redraw_start_kernel"; by = 2.0 * 3.0 * i[0] * 4.0 * i[1]; break;
        case DS_OP_LLM_GEMV:
        case DS_OP_LLM_GEMM16:
        case DS_OP_LLM_GEMV_W8:
        case DS_OP_LLM_GEMM16_W8:
        case DS_OP_LLM_GEMV_FP4:
        case DS_OP_LLM_GEMM16_FP4: {   // W + x + y bytes: the weights are read once for all M rows; x and y fp16
            const LlmWeights form = llm_weights_of(op->code);
            const double rows = (double)i[1] * (i[4] ? 2 : 1), K = i[2];
            nm = llm_is_gemm16(op->code) ? "llm_gemm16_kernel" : "llm_gemv_kernel";
            fl = 2.0 * i[0] * (double)i[1] * i[2] * (i[4] ? 2 : 1);
            // per weight row: fp16 2 bytes per weight; int8 1 + the fp32 row scale; MXFP4 half a byte + one exponent byte per 32
            // + the row scale
            by = rows * (form == LLM_W_F16 ? 2.0 * K : form == LLM_W_INT8 ? K + 4.0 : K / 2.0 + K / 32.0 + 4.0) +
                 2.0 * ((double)i[0] * i[2] + (double)i[0] * i[1]);
            break;
        }
        case DS_OP_LLM_ATTN:
        case DS_OP_LLM_ATTN_SLOTS: nm = "llm_attn_kernel"; break;
        case DS_OP_LLM_ATTN_ROWS: nm = "llm_attn_rows_kernel"; break;
        case DS_OP_LLM_ATTN_ROWS_KV8:    // every slot's cache once at its full length, as for the slot form: an upper bound
            nm = "llm_attn_rows_kernel";
            by = 2.0 * i[5] * (double)i[4] * i[2] * (i[3] + 1.0);
            break;
        case DS_OP_LLM_ATTN_KV8:      // the fp8 cache read once at its full length (an upper bound: the length is device state):
        case DS_OP_LLM_ATTN_SLOTS_KV8:   // D code bytes + 1 exponent byte per (row, kv head), for K and for V, per sequence
            nm = "llm_attn_kernel";
            by = 2.0 * (op->code == DS_OP_LLM_ATTN_SLOTS_KV8 ? i[0] : 1) * (double)i[4] * i[2] * (i[3] + 1.0);
            break;
        case DS_OP_LLM_RMSNORM:
        case DS_OP_LLM_RMSNORM_SLOTS: nm = "llm_rmsnorm_kernel"; by = 4.0 * i[0] * (double)i[1]; break;
        case DS_OP_LLM_SELECT_SLOTS: nm = "llm_select_kernel"; by = 2.0 * i[0] * (double)i[4]; break;
        case DS_OP_LLM_SELECT: nm = "llm_select_kernel"; by = 2.0 * i[0]; break;
        case DS_OP_LORA_MERGE:   // W in, out (and out2) out, A and B once; the adapters' products (convolution mode: K = 9 Cin)
            nm = "lora_merge_kernel";
            fl = 2.0 * i[0] * (double)i[1] * i[2];
            by = 2.0 * ((op->p[8] ? 3.0 : 2.0) * i[0] * (double)i[1] + (double)i[2] * ((double)i[0] + i[1]));
            break;
        default: break;
    }
    if (name && name_len > 0) {
        strncpy(name, nm, name_len - 1);
        name[name_len - 1] = 0;
    }
    if (flops) *flops = fl;
    if (bytes) *bytes = by;
    return 0;
}

struct ds_plan {
    std::vector<ds_op> ops;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

int ds_op_run(const ds_op* op, void* stream) {
    DS_REQUIRE(op != nullptr, "ds_op_run: null op");
    return run_op(*op, S(stream));
}

int ds_plan_create(const ds_op* ops, int n_ops, ds_plan** out) {
    DS_REQUIRE(ops && n_ops > 0 && out, "ds_plan_create: bad arguments");
    ds_plan* pl = new ds_plan();
    pl->ops.assign(ops, ops + n_ops);
    *out = pl;
    return 0;
}

int ds_plan_num_ops(const ds_plan* plan) { return plan ? (int)plan->ops.size() : -1; }

int ds_plan_run(ds_plan* plan, void* stream) {
    DS_REQUIRE(plan, "ds_plan_run: null plan");
    for (size_t k = 0; k < plan->ops.size(); ++k) {
        int rc;
        if (plan->ops[k].code == DS_OP_LORA_MERGE) {
            // consecutive merges are independent (each writes its own matrix from read-only inputs): one launch per group
            LoraMergeParams grp[DS_LORA_GROUP];
            int n = 0;
            while (n < DS_LORA_GROUP && k + n < plan->ops.size() && plan->ops[k + n].code == DS_OP_LORA_MERGE) {
                grp[n] = lora_merge_params(plan->ops[k + n]);
                ++n;
            }
            rc = ds_launch_lora_merge_group(grp, n, S(stream));
            if (rc == 0) {
                k += n - 1;
                continue;
            }
        } else
            rc = run_op(plan->ops[k], S(stream));
        if (rc != 0) {
            char msg[600];
            snprintf(msg, sizeof(msg), "plan op %zu (code %d): %s", k, plan->ops[k].code, g_err);
            ds_set_error("%s", msg);
            return rc;
        }
    }
    return 0;
}

int ds_plan_capture(ds_plan* plan, void* stream) {
    DS_REQUIRE(plan, "ds_plan_capture: null plan");
    if (plan->exec) return 0;
    hipStream_t st = S(stream);
    DS_REQUIRE(st != nullptr, "ds_plan_capture: needs a non-default stream");
    DS_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = ds_plan_run(plan, stream);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(st, &g);
    if (rc != 0) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess) {
        ds_set_error("hipStreamEndCapture failed: %s", hipGetErrorString(e));
        return -2;
    }
    plan->graph = g;
    DS_HIP(hipGraphInstantiate(&plan->exec, g, nullptr, nullptr, 0));
    return 0;
}

int ds_plan_replay(ds_plan* plan, void* stream) {
    DS_REQUIRE(plan && plan->exec, "ds_plan_replay: plan not captured");
    DS_HIP(hipGraphLaunch(plan->exec, S(stream)));
    return 0;
}

int ds_plan_destroy(ds_plan* plan) {
    if (!plan) return 0;
    if (plan->exec) (void)hipGraphExecDestroy(plan->exec);
    if (plan->graph) (void)hipGraphDestroy(plan->graph);
    delete plan;
    return 0;
}

}  // extern "C"
