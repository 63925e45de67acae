// Internal launcher interface between the C-ABI layer / plan executor and the HIP kernels.
#pragma once
#include "ds_common.h"

// EPI_GEGLU320: GEGLU whose packed W rows come in groups of 320 (160 hidden + their 160 gates): gemm_g320_kernel only
enum { EPI_NONE = 0, EPI_GEGLU = 1, EPI_GELU = 2, EPI_QUICK_GELU = 3, EPI_GEGLU320 = 4 };

struct GemmParams {
    const half_t* A = nullptr;   // plain: [M,K] rows (lda);  conv: NHWC input [B,Hin,Win,Cin]
    const half_t* A2 = nullptr;  // plain only: second source for k >= K1 (channel concat without a copy)
    const half_t* W = nullptr;   // [N,K] rows (ldw), K contiguous; conv: K = (ky*3+kx)*Cin + ci
    half_t* C = nullptr;         // [M,N] rows (ldc)   (GEGLU: [M,N/2])
    const half_t* bias = nullptr;      // [N]
    const half_t* rowbias = nullptr;   // [M/rows_per_group, rowbias_ld]  (resnet time-embedding projection)
    const half_t* residual = nullptr;  // [M,N] rows (ldr), added after rounding to f16
    long lda = 0, lda2 = 0, ldw = 0, ldc = 0, ldr = 0;
    long sA = 0, sA2 = 0, sW = 0, sC = 0, sR = 0;  // batch strides (elements), grid.z
    int M = 0, N = 0, K = 0, K1 = 0;
    int rowbias_ld = 0, rows_per_group = 1;
    int epi = EPI_NONE;
    int conv = 0;
    int Hin = 0, Win = 0, Cin = 0, Hout = 0, Wout = 0, cstride = 1, upsample = 0;
    float up_sy = 0.5f, up_sx = 0.5f;  // upsample: nearest-resize scales float(Hin)/Hout, float(Win)/Wout (ATen's definition)
    int up_fold = 0;  // upsample, exactly 2Hin x 2Win, halo-patch kernels only: W holds the four 2 x 2 phase weights [4][N][4 Cin]
                      //   (ldw = 4 Cin, ds_launch_fold_upsample2x) instead of [N][9 Cin]; K stays 9 Cin, the work of the op it replaces
    int tiles_m = 0, tiles_n = 0;
    int nbatch = 1;  // gemm_pp_kernel only: batch items folded into the persistent tile walk (id -> item, tile); others use grid.z
    // ---- LayerNorm fused across a producer / consumer pair of gemm_pp_kernel launches (gemm_pp.hip header, "LayerNorm"):
    // producer: per-row partial sums of the STORED output, one (sum, sum of squares) pair per row and 64-column strip,
    //           laid out [N / 64][M] (float2); consumer: y = rstd_m * (x_m . gw_n - mu_m c_n) + b'_n with gw = gamma (.) W
    //           packed at load time, (mu, rstd) per row from ds_launch_ln_finalize, c_n = sum_k gw_nk as a NEGATED f16
    //           (hi, lo) pair per output column, b' = bias + W beta passed as `bias`.
    float* stats_out = nullptr;        // producer: [N/64][M] float2 partials (fast plain epilogue, nbatch 1)
    const float* ln_stats = nullptr;   // consumer: [M] float2 (mu, rstd)
    const half_t* ln_c = nullptr;      // consumer: [N][2] f16 (-c hi, -c lo), in the (packed) row order of W
    int ln_swapped = 0;                // consumer, operand-swapped form (V^T = Wv X_b^T): the normalised rows are the rows of W
                                       // (tile columns): ln_stats[b * ln_bstride + n], ln_c = [M][4] f16 (-c hi, -c lo, b' hi, b' lo)
    long ln_bstride = 0;               //   rows of the normalised matrix per batch item
    int ln_partial = 0;                // consumer on the 128-wide LDS-DMA kernels (gemm.hip, "Fused LayerNorm"): ln_stats points at the
    float ln_eps = 1e-5f;              //   producer's PARTIALS [K/64][rows] float2 and the epilogue finalises its own rows (eps = ln_eps)
    long ln_rows = 0;                  //   operand-swapped form only: rows of the normalised matrix over all batch items (stride of the partials)
    int ln_nstrips = 0;                // consumer of partials: entries per row to sum (0 = K / 64; 3 K / 160 behind a gemm_t160_kernel producer)
    int stats_strip = 0;               // producer: statistics format (0 = one entry per 64 columns).  160 is what gemm_t160_kernel emits - its
                                       //   160-column tiles hold no whole 64-column strips -: three entries per tile (columns 0..63, 64..127,
                                       //   128..159), [3 N / 160][M] float2; the launch planner requests it explicitly (and tells the
                                       //   consumers: ln_nstrips), a direct caller never gets it
    // ---- GroupNorm statistics out of the producing convolution (conv_halo.hip, round 6): the halo-patch kernels also write, per
    // (image, pixel tile, output channel), the (sum, sum of squares) of the f16 values they store - the partial-sum layout of
    // gn_stats_kernel, [B][gn_chunks][Cout] float2 - so the GroupNorm that follows skips its statistics pass (one read of x less)
    float* gn_partial = nullptr;
    int gn_chunks = 0;                 // chunks per image the plan expects (DsOp CONV3X3 i[10] = ds_conv3x3_gn_chunks at plan time); the
                                       //   launch requires it to equal ds_conv_halo_gn_chunks of the kernel it picks (0: not stated)
    int dtype = DS_DTYPE_F16;  // element type of A / W / C / bias / residual (the pointers are 2-byte opaque): bf16 = VAE path
    int debug = 0;  // ablation only (ds_set_option "gemm_debug"): 1 skip MFMA, 2 skip tile loads — results are garbage
    int pad_lo = 1;  // conv: zero padding on the top / left side.  0 (with cstride 2): diffusers' Downsample2D(padding=0), F.pad(x, (0,1,0,1)) +
                     //   stride 2 - output (Y, X) reads rows 2Y + ky, columns 2X + kx, Hout = Hin / 2 (ds_conv3x3_down_f16 / _bf16).
                     //   Host dispatch only (a template argument of the kernels); last, so that no other field moves
};
// gemm.hip's route() is the one authority on which kernel serves a GEMM / 3x3 convolution: the launch, the name and the two
// planner queries below all read its answer (a problem no kernel serves: the launch fails, the name is "refused")
int ds_launch_gemm(const GemmParams& p, int batch, hipStream_t stream);
int ds_gemm_conv_gn_chunks(const GemmParams& p);  // GroupNorm partial chunks per image the routed conv kernel would emit (0: none)
int ds_gemm_ln_kind(int M, int N, int K, int batch, int epi);  // fused LayerNorm, the role-free problem's route: 1 = gemm_pp_kernel, 2 = 128-wide kernels, 0 = none
bool ds_gemm_pp_applicable(const GemmParams& p);  // gemm_pp.hip: 256 x 256 ping-pong kernel takes this shape
bool ds_gemm_pp_fused_tiles(int M, int N, int epi, bool swapped, int debug);  // ... and its fused-LayerNorm epilogues these tiles
int ds_launch_gemm_pp(const GemmParams& p, int batch, hipStream_t stream);
bool ds_conv_halo_applicable(const GemmParams& p);  // conv_halo.hip: halo-patch 3x3 convolution takes this shape
int ds_launch_conv_halo(const GemmParams& p, hipStream_t stream);
const char* ds_conv_halo_kernel_name(const GemmParams& p);  // conv_halo_kernel | conv_halo256_kernel | conv_halo_deep_kernel: what ds_launch_conv_halo runs
int ds_conv_halo_gn_chunks(const GemmParams& p);  // pixel tiles per image of the variant ds_launch_conv_halo would run; 0: no statistics (too many tiles / not applicable)
int ds_launch_fold_upsample2x(const half_t* w, half_t* out, int Cout, int Cin, hipStream_t stream);  // [Cout][9 Cin] -> [4][Cout][4 Cin]
void ds_conv_halo_set_variant(int v);  // 0 auto, 1 8x16-pixel blocks, 2 16x16-pixel blocks, 3 ring-buffered 8x16 blocks, 4 auto without the ring-buffered kernel
void ds_conv_halo_set_deep_blocks(int v);  // the ring-buffered 8x16 kernel takes grids of <= v blocks per CU (default 1)
const char* ds_gemm_kernel_name(const GemmParams& p, int batch);  // route(p, batch).name: the instantiation ds_launch_gemm runs, or "refused"
void ds_gemm_set_debug(int v);
void ds_gemm_set_ring(int v);     // 0 auto (ring-buffered kernel for small grids), 1 never
void ds_gemm_set_pp_narrow(int v);  // 0 auto, 1: N, K <= 640 projections never on gemm_pp_kernel (A/B)
void ds_gemm_pp_set_even(int v);  // experiment: 1 = persistent grid shrunk so that every round of tiles is full
void ds_gemm_set_variant(int v);  // 0 auto, 1 register staging only, 2 glds (BM <= 128), 3 glds, BM = 256 when large
// gemm_t160.hip: 64 x 160 tiles, one block per CU, for the small-batch projections of the 1280-channel level
bool ds_gemm_t160_shape(int M, int N, int K, int batch);           // the automatic dispatch rule (host logic only)
int ds_gemm_t160_rows(int M, int N, int K, int batch);             // rows per tile the launcher uses there: 64 | 128 (0: the rule does not pick the kernel -> 64 when forced)
bool ds_gemm_t160_possible(const GemmParams& p, int batch);        // what the kernel can run at all (gemm_variant 11)
bool ds_gemm_t160_applicable(const GemmParams& p, int batch);      // possible && shape rule
int ds_launch_gemm_t160(const GemmParams& p, hipStream_t stream);
void ds_gemm_set_t160(int v);     // 0 auto, 1 never
// gemm_g320.hip: 256 x 320 tiles, one block per CU, for the GEGLU projection of a small-batch request (epi == EPI_GEGLU320)
bool ds_gemm_g320_shape(int M, int N, int K, int batch);           // the automatic dispatch rule (host logic only)
bool ds_gemm_g320_possible(const GemmParams& p, int batch);
bool ds_gemm_g320_plain_applicable(const GemmParams& p, int batch);   // the plain-epilogue form: possible && shape rule (q|k at M = 8192, N = 2560)
int ds_launch_gemm_g320(const GemmParams& p, hipStream_t stream);
void ds_gemm_set_g320(int v);     // 0 auto, 1 never

// ---- VAE decoder only (vae.hip) ---------------------------------------------------------------------
int ds_launch_wide_attn(const void* q, const void* k, const void* vt, void* o, int B, int N, int n_valid, int dtype,
                        float scale, hipStream_t stream);  // one head of dim 512: q,k,o [B,N,512]; vt [B,512,N]; keys >= n_valid masked
int ds_launch_vae_conv_in(const float* lat, const float* wpq, const float* bpq, const void* w, const void* bias, void* y,
                          int B, int H, int W, int C, float scaling_factor, int dtype, hipStream_t stream);
int ds_launch_vae_conv_out(const void* x, const void* w, const void* bias, float* img, int B, int H, int W, int C,
                           int denorm, int dtype, hipStream_t stream);
// ---- VAE encoder only (vae.hip) ---------------------------------------------------------------------
int ds_launch_vae_enc_conv_in(const void* img, int is_u8, const void* w, const void* bias, void* y, int B, int H, int W,
                              int C, int dtype, hipStream_t stream);   // img: uint8 NHWC [B,H,W,3] or fp32 NCHW [B,3,H,W] in [-1, 1]
int ds_launch_vae_enc_conv_out(const void* x, const void* w, const float* bias, float* moments, int B, int H, int W, int C,
                               int dtype, hipStream_t stream);         // w [8,3,3,C] (quant_conv folded in), bias fp32 [8]
int ds_launch_vae_latents(const float* moments, const long long* seeds, const float* shift4, const float* scale4,
                          half_t* out, int B, int HW, hipStream_t stream);   // shift4 / scale4: HOST floats (shift4 may be null)

// ---- normalisation ---------------------------------------------------------------------------------
struct GroupNormParams {
    const half_t* x1 = nullptr;  // [B,HW,C1]
    const half_t* x2 = nullptr;  // [B,HW,C2] or null  (channels C1..C1+C2)
    half_t* y = nullptr;         // [B,HW,C1+C2]
    const half_t* gamma = nullptr;
    const half_t* beta = nullptr;
    float* ws = nullptr;         // workspace, ds_groupnorm_ws_floats() floats
    int B = 0, HW = 0, C1 = 0, C2 = 0, groups = 32;
    float eps = 1e-5f;
    int silu = 0;
    int dtype = DS_DTYPE_F16;  // bf16: VAE decoder path (x, y, gamma, beta are 2-byte opaque pointers)
    float out_scale = 1.0f;    // y = act(norm(x)) * out_scale (the VAE decoder's scaled-fp16 mode; exact for powers of two)
    int pre_chunks = 0;        // > 0: ws already holds [B][pre_chunks][C] float2 partial sums (written by the producing convolution,
                               //      GemmParams::gn_partial): no statistics launch
};
size_t ds_groupnorm_ws_floats(int B, int C);
void ds_groupnorm_set_variant(int v);  // 0 auto (round-4 geometry), 1 round-3 geometry (A/B)
int ds_launch_groupnorm(const GroupNormParams& p, hipStream_t stream);
int ds_launch_layernorm(const half_t* x, half_t* y, const half_t* gamma, const half_t* beta, int rows, int C,
                        float eps, hipStream_t stream);
// row statistics of a fused LayerNorm: partial [strips][M] float2 (sum, sum of squares) -> stats [M] float2 (mean, rstd)
int ds_launch_ln_finalize(const float* partial, float* stats, int M, int strips, int C, float eps, hipStream_t stream);

// ---- attention -------------------------------------------------------------------------------------
struct SelfAttnParams {
    const half_t* q = nullptr;   // [B,N,*] rows (ldq), head h at column h*64
    const half_t* k = nullptr;   // [B,N,*] rows (ldk)
    const half_t* vt = nullptr;  // [B,heads,64,ldv]  (V transposed: keys contiguous)
    half_t* o = nullptr;         // [B,N,*] rows (ldo)
    long ldq = 0, ldk = 0, ldv = 0, ldo = 0;
    long sq = 0, sk = 0, so = 0;  // per-batch strides (elements)
    int B = 0, heads = 0, Nq = 0, Nk = 0;
    float scale = 0.125f;
    int xcd_map = 1;  // self_attn_sp_kernel: 1 = all query blocks of a head on one XCD (0: plain order, A/B via attn_variant 4)
};
int ds_launch_self_attn(const SelfAttnParams& p, hipStream_t stream);
int ds_launch_self_attn_sp(const SelfAttnParams& p, hipStream_t stream);
int ds_attn_sp_recentre_count(int reset, long long* value);   // debug counter of the rare re-centring branch (attention_sp.hip)
const char* ds_self_attn_kernel_name(int B, int heads, int Nq, int Nk);  // which kernel ds_launch_self_attn picks for this shape  // attention_sp.hip: software-pipelined variant
void ds_attn_set_variant(int v);  // 0 auto, 1 force 32 query rows per wave, 2 force 64 rows per wave, 3 force the software-pipelined kernel
void ds_ip_attn_set_min_blocks(int v);
void ds_ip_attn_set_variant(int v);  // 0 auto, 1 four-wave register-staged kernel, 2 eight-wave LDS-DMA ring kernel (N % 256 == 0), 3 four-wave without the T16 specialisation (A/B)

struct IPAttnParams {
    const half_t* q = nullptr;     // [B,N,C] rows (ldq)
    const half_t* kt = nullptr;    // text keys   [B,LP,C]      (rows >= Lt are padding)
    const half_t* vtt = nullptr;   // text values [B,C,LP]      (transposed)
    const half_t* ki = nullptr;    // ip keys     [B,LP,C]
    const half_t* vti = nullptr;   // ip values   [B,C,LP]
    const float* bbox = nullptr;   // [B,max_ips,4]
    half_t* o = nullptr;           // [B,N,C] rows (ldo)
    long ldq = 0, ldo = 0;
    long ldk = 0, sk = 0;          // key panels: row stride / batch stride (elements); 0 -> dense [B,LP,C]
    long sv = 0;                   // value panels: batch stride (elements); 0 -> dense [B,C,LP]
    int B = 0, heads = 0, N = 0, C = 0;
    int Lt = 77, Li = 80, LP = 96;
    int n_dummy = 16, tok_per_ip = 16, max_ips = 4;
    int mask_h = 0, mask_w = 0;    // grid the reference infers from (N, aspect_ratio)
    float step_x = 0.f, step_y = 0.f;   // 1/(mask_w-1), 1/(mask_h-1) correctly rounded: filled in by ds_launch_ip_attn
    float qk_scale = 0.125f, ip_scale = 1.0f;
    const float* ip_scale_ptr = nullptr;  // device scalar; overrides ip_scale when set (graph-replay safe)
    int ip_scale_rows = 0;         // 1: ip_scale_ptr is [B] floats, batch row b reads element b (under CFG rows n and ns + n
                                   // both belong to panel n: the caller writes that panel's scale into both)
};
int ds_launch_ip_attn(const IPAttnParams& p, hipStream_t stream);
// Long prompts (ip_attn_long_kernel): the text side is T panels of 96 rows, kt [B,96 T,C] / vtt [B,C,96 T] (value rows dense),
// with strides of their own; a.ldk / a.sk / a.sv describe the IP panels alone.  1 <= a.Lt <= 384, (T - 1) 96 < a.Lt <= 96 T.
struct IPAttnLongParams {
    IPAttnParams a;
    long ldkt = 0, skt = 0;        // text key panel: row stride / batch stride (elements); 0 -> dense [B,96 T,C]
    long svt = 0;                  // text value panel: batch stride (elements); 0 -> dense [B,C,96 T]
    int T = 0;                     // text panels
};
int ds_launch_ip_attn_long(const IPAttnLongParams& p, hipStream_t stream);
int ds_launch_small_attn(const half_t* q, const half_t* k, const half_t* v, half_t* o, long ldq, long ldk, long ldv,
                         long ldo, long sq, long sk, long sv, long so, int B, int heads, int Nq, int Nk, int D,
                         float scale, hipStream_t stream, int causal = 0);
int ds_launch_ip_region_flags(const float* bbox, uint8_t* flags, int B, int N, int max_ips, int mask_h, int mask_w,
                              hipStream_t stream);

// ---- small / elementwise ------------------------------------------------------------------------------
int ds_launch_conv_in(const half_t* x, const half_t* w, const half_t* bias, const int* dialog_boxes,
                      const half_t* dialog_emb, half_t* y, int B, int H, int W, int Cin, int Cout, int ndialog,
                      hipStream_t stream);
int ds_launch_conv_out(const half_t* x, const half_t* w, const half_t* bias, half_t* y, int B, int H, int W, int Cin,
                       int Cout, hipStream_t stream);
int ds_launch_skinny_linear(const half_t* x, const half_t* w, const half_t* bias, const half_t* addend, half_t* y,
                            int M, int N, int K, int act_in, int act_out, hipStream_t stream);
// Per-step scalar table: row i (8 floats) = {timestep, c_in_div, k0, k1, k2, k3, c_in_div_next, guidance};
// `ctr` is a device int selecting the row (null = row 0) so a captured hipGraph is step-independent.
int ds_launch_timestep_embed(const float* table, const int* ctr, half_t* out, int B, int dim, int flip,
                             float freq_shift, hipStream_t stream);
int ds_launch_add_time_ids(const half_t* text_embeds, const half_t* time_ids, half_t* out, int B, int pooled_dim,
                           int n_ids, int dim, int flip, float freq_shift, hipStream_t stream);

struct SamplerStepParams {
    const half_t* eps = nullptr;    // UNet output, NHWC [2*ns, HW, 4]: rows [0,ns) uncond, [ns,2ns) cond
    half_t* latents = nullptr;      // NCHW [ns,4,H,W], updated in place (fp16 between steps, like the reference)
    half_t* model_in = nullptr;     // NHWC [2*ns, HW, 4]: next step's scaled input (both CFG halves)
    const float* coef = nullptr;    // per-step scalar table (see elementwise.hip)
    half_t* prev_x0 = nullptr;      // kind 2: NCHW [ns,4,H,W] x0 of the previous step (read, then overwritten)
    const float* solver = nullptr;  // kind 2: per-step solver rows [n_steps,8] (include/diffsensei_hip.h)
    const long long* seeds = nullptr;  // kind 3: int64 [ns], one Philox key per panel (noise = f(seed, pixel, *ctr))
    const float* guidance = nullptr;   // fp32 [ns], one guidance scale per panel in place of column 7 (null: column 7)
    const void* redraw = nullptr;      // region redraw: the packed buffer below (read when redraw_on is set)
    int ns = 0, HW = 0, C = 4;
    int kind = 0;                   // 0 Euler, 1 DDIM, 2 DPM-Solver++ (multistep, order 1|2 per row), 3 Euler Ancestral
    int do_cfg = 1;
    int redraw_on = 0;              // 1: blend with the kept latents after the step (a launch without the buffer is refused)
};
int ds_launch_sampler_step(const SamplerStepParams& p, const int* ctr, hipStream_t stream);
// Region redraw: ONE device buffer (16-byte aligned) whose offsets follow from ns and HW (include/diffsensei_hip.h):
//   x0k fp16 [ns,4,HW] | noise fp16 [ns,4,HW] | mask fp16 [ns,HW] | pad to 16 bytes |
//   header fp32 [4] = {full strength, init_noise_sigma, 0, 0} | renoise rows fp32 [DS_REDRAW_MAX_ROWS][2] = {ka, kb}
constexpr int DS_REDRAW_MAX_ROWS = 1025;
struct RedrawView {
    const half_t *x0k, *noise, *mask;
    const float *hdr, *rows;
};
__host__ __device__ inline long ds_redraw_f32_offset(int ns, int HW) {   // bytes
    return ((long)ns * HW * 9 * 2 + 15) & ~15L;
}
__host__ __device__ inline RedrawView ds_redraw_view(const void* buf, int ns, int HW) {
    const half_t* h = static_cast<const half_t*>(buf);
    const float* f = reinterpret_cast<const float*>(static_cast<const char*>(buf) + ds_redraw_f32_offset(ns, HW));
    return RedrawView{h, h + (long)ns * 4 * HW, h + (long)ns * 8 * HW, f, f + 4};
}
int ds_launch_redraw_start(const void* redraw, half_t* latents, int ns, int HW, hipStream_t stream);
// Panel schedules (continuous batching): ONE device buffer (16-byte aligned) whose offsets follow from ns alone
// (include/diffsensei_hip.h, "Panel schedules"); R = DS_PANEL_MAX_ROWS:
//   start int32 [ns] | steps int32 [ns] | pad to 16 bytes | mode fp32 [ns][4] = {start mode, init_noise_sigma, 0, 0} |
//   coef fp32 [ns][R][8] | solver fp32 [ns][R][8] | renoise fp32 [ns][R + 1][2]
// With s = *ctr panel n is at its row j = s - start[n] and active iff 0 <= j < steps[n].
#ifndef DS_PANEL_MAX_ROWS
#define DS_PANEL_MAX_ROWS 1024   // include/diffsensei_hip.h states the same value
#endif
enum { DS_PANEL_START_RENOISE = 0, DS_PANEL_START_FULL = 1, DS_PANEL_START_KEEP = 2 };
struct PanelView {
    const int *start, *steps;
    const float *mode, *coef, *solver, *renoise;
};
__host__ __device__ inline long ds_panel_f32_offset(int ns) {   // bytes
    return ((long)ns * 8 + 15) & ~15L;
}
__host__ __device__ inline long ds_panel_bytes(int ns) {
    return ds_panel_f32_offset(ns) + (long)sizeof(float) * ns * (4 + 16L * DS_PANEL_MAX_ROWS + 2L * (DS_PANEL_MAX_ROWS + 1));
}
__host__ __device__ inline PanelView ds_panel_view(const void* buf, int ns) {
    const int* s = static_cast<const int*>(buf);
    const float* f = reinterpret_cast<const float*>(static_cast<const char*>(buf) + ds_panel_f32_offset(ns));
    const float* coef = f + (long)ns * 4;
    const float* solver = coef + (long)ns * DS_PANEL_MAX_ROWS * 8;
    return PanelView{s, s + ns, f, coef, solver, solver + (long)ns * DS_PANEL_MAX_ROWS * 8};
}
// `panel` = true: p.coef is the panel-schedule buffer (p.solver unused, p.guidance required under CFG), see sampler_step_kernel
int ds_launch_sampler_step_panels(const SamplerStepParams& p, const int* ctr, hipStream_t stream);
int ds_launch_panel_slot_load(void* panel, int ns, int slot, int start, int steps, const float* coef, const float* solver,
                              const float* renoise, int start_mode, float init_noise_sigma, hipStream_t stream);
int ds_launch_timestep_embed_panels(const void* panel, const int* ctr, half_t* out, int B, int dim, int flip,
                                    float freq_shift, int ns, hipStream_t stream);
int ds_launch_panel_slot_start(const void* panel, const void* redraw, half_t* latents, half_t* model_in, int ns, int HW,
                               int do_cfg, int slot0, int nslots, hipStream_t stream);
// Philox4x32-10 keyed per panel, counter (pixel, 0, step, stream_id): raw words [ns,HW,4] / Box-Muller normals [ns,4,HW]
int ds_launch_philox_u32(const long long* seeds, int step, int stream_id, unsigned* out, int ns, int HW,
                         hipStream_t stream);
int ds_launch_philox_normal(const long long* seeds, int step, int stream_id, float* out, int ns, int HW,
                            hipStream_t stream);
int ds_launch_prepare_model_input(const half_t* latents, half_t* model_in, const float* table, const int* ctr, int ns,
                                  int HW, int C, int do_cfg, hipStream_t stream);
int ds_launch_advance_counter(int* ctr, hipStream_t stream);
int ds_launch_nhwc_to_nchw(const half_t* x, half_t* y, int B, int HW, int C, hipStream_t stream);
int ds_launch_image_to_u8(const float* img, uint8_t* out, int B, int H, int W, hipStream_t stream);
int ds_launch_nchw_to_nhwc(const half_t* x, half_t* y, int B, int HW, int C, hipStream_t stream);
int ds_launch_embed_tokens(const int* ids, const half_t* tok_emb, const half_t* pos_emb, half_t* out, int B, int T,
                           int D, int vocab, hipStream_t stream);
int ds_launch_pad_rows(const half_t* x, half_t* y, int B, int rows_in, int rows_out, int row_off, int total_rows,
                       int C, hipStream_t stream);

// ---- LoRA merge into a packed weight buffer (lora.hip) ------------------------------------------------
#define DS_LORA_MAX_SEGMENTS 16   // the host merges at most 8 adapters at once (lora.py); empty segments may pad the list
struct LoraMergeParams {
    const half_t* W = nullptr;         // [N,K] base weight rows (ldw), read only: never `out` or `out2`
    half_t* out = nullptr;             // [N,K] rows (ldo): f16(f32(W[map(n)]) + sum_i s_i (B_i A_i)[map(n)])
    const half_t* A = nullptr;         // [R,K] rows (lda): the adapters' down matrices, concatenated along the rank
    const half_t* B = nullptr;         // [N,R] rows (ldb): the up matrices, same concatenation
    const int* seg = nullptr;          // device int32 [nseg + 1]: rank offsets, one segment per adapter (empty ones are legal)
    const float* s = nullptr;          // device fp32 [nseg]: strength of each adapter
    const int* map = nullptr;          // optional device int32 [N]: output row n reads row map[n] of W and B
    const half_t* colscale = nullptr;  // with out2: f16 [K]
    half_t* out2 = nullptr;            // optional [N,K] rows (ldo2): f16(f32(out) * f32(colscale[k]))
    long ldw = 0, ldo = 0, lda = 0, ldb = 0, ldo2 = 0;
    int N = 0, K = 0, R = 0, nseg = 0;
    int cin = 0;                       // > 0: convolution mode - W is [N][cin][3][3] (checkpoint order), out / A are tap-major, K = 9 cin
};
int ds_launch_lora_merge(const LoraMergeParams& p, hipStream_t stream);
#define DS_LORA_GROUP 24   // matrices per launch: 24 x 136 bytes of parameters fit the 4 KiB of kernel arguments
// `count` (1..DS_LORA_GROUP) independent merges in ONE launch; the plan executor groups consecutive DS_OP_LORA_MERGE ops
int ds_launch_lora_merge_group(const LoraMergeParams* ps, int count, hipStream_t stream);

// ---- MLLM pre-pass: LLaMA greedy decoding (llm.hip) ---------------------------------------------------
// device-side state block (int32[8]): {tokens in the KV cache, tokens generated, finished, current token,
//                                      max_new_tokens, eos id, spare, spare}
struct LlmGemvParams {
    const half_t* x = nullptr;         // [M,K] rows (ldx)
    const void* w = nullptr;           // [N,K] row-major fp16 (int8 with w_scale, MXFP4 with w_exp); SwiGLU: [2N,K] = gate rows then up rows
    half_t* y = nullptr;               // [M,N] rows (ldy)
    const half_t* residual = nullptr;  // [M,N] rows (ldr) added after the fp16 rounding; may alias y
    long ldx = 0, ldy = 0, ldr = 0;
    int M = 0, N = 0, K = 0;
    int rms = 0;                       // LlamaRMSNorm in front of the projection: row m is scaled by rsqrt(mean(x[m]^2) + eps)
    const half_t* gain = nullptr;      // [K] RMSNorm weight.  Given: x' = f16(gain * f16(x * r)) exactly like the reference
                                       // (normalise in fp32, round to fp16, multiply by the fp16 gain, round) is what meets
                                       // w; null: the caller folded the gain into w and only r is applied to the dot
    int swiglu = 0;                    // y = silu(x.w[n]) * (x.w[n+N])
    float eps = 1e-6f;
    const float* w_scale = nullptr;    // null: fp16 weights.  Given: w is int8 (K % 16 == 0) and w_scale fp32 [N] (SwiGLU [2N]),
                                       // one scale per weight row: y = (x' . q[n]) * w_scale[n], scaled in fp32 before the fp16 rounding
    const uint8_t* w_exp = nullptr;    // given (with w_scale): w is MXFP4 - packed e2m1 [N,K/2], element 2i in the low nibble (K % 32
                                       // == 0) - and w_exp [N,K/32] row-major (SwiGLU [2N,K/32]) holds one biased E8M0 exponent per
                                       // 32-element block: weight = e2m1 * 2^(w_exp - 127) * w_scale[n].  The natural layout is the
                                       // kernels' own: no permuted copy
};
int ds_launch_llm_gemv(const LlmGemvParams& p, hipStream_t stream);
void ds_llm_gemv_set_variant(int v);   // 0 auto (pipelined), 1 one column per wavefront, 2 streaming without pipelining

// Row forms of the four per-row kernels below (attention, RMSNorm with tap, embed, pick).  A launch is `rows` rows; row m
// reads its state at state + m * state_stride and its cache at kc / vc + m * slot_stride:
//   one-sequence form  state_stride = 0, slot_stride = 0: all rows belong to one sequence, row m sits at position
//                      state[0] + m and sees the rows before it in the same launch (prompt chunks, M <= 16)
//   slot form          state_stride = 8: every row is its own sequence - row m of qkv / out / logits, state row m of an
//                      int32 [S][8] block, cache slot m of [S][T_max][kv_heads*D], feat[m] of [S][max_out][H],
//                      out_ids[m] of [S][out_cap]; a finished (or never started) slot is skipped
struct LlmAttnParams {
    const half_t* qkv = nullptr;       // [M, (heads + 2 kv_heads) * D] rows (ldqkv): q | k | v, not yet rotated
    half_t* kc = nullptr;              // key cache   [T_max, kv_heads*D] rows (ldc), rotated keys
    half_t* vc = nullptr;              // value cache [T_max, kv_heads*D]
    const float* rope_cos = nullptr;   // [T_max, D/2]
    const float* rope_sin = nullptr;
    half_t* out = nullptr;             // [M, heads*D] rows (ldo)
    const int* state = nullptr;        // state[0] = rows already in the cache
    long ldqkv = 0, ldc = 0, ldo = 0;
    int M = 0, heads = 0, kv_heads = 0, D = 0, T_max = 0;
    float scale = 1.0f;
    long slot_stride = 0;              // elements between the caches of two rows (slot form; 0 in the one-sequence form)
    int state_stride = 0;              // 0 | 8, see above
    int kv8 = 0;
    // fp8 KV cache (kv8 = 1): kc / vc point at uint8 caches of OCP e4m3 codes with the same [T_max, kv_heads*D] rows (ldc
    // and slot_stride then count bytes), k_exp / v_exp at uint8 [T_max, kv_heads] rows (lde) of one biased exponent per (row,
    // kv head): value = f32(e4m3) * 2^(exp - 127), exp - 127 the smallest integer that brings the head's largest magnitude to
    // <= 448 (0 for an all-zero head).  Every key and value, the chunk's own rows included, is seen through that quantiser.
    uint8_t* k_exp = nullptr;
    uint8_t* v_exp = nullptr;
    long lde = 0;
    long exp_slot_stride = 0;          // bytes between the exponent arrays of two rows (slot form)
};
int ds_launch_llm_attn(const LlmAttnParams& p, hipStream_t stream);
// Ragged form (llm_attn_rows_kernel): p as in the slot form, p.M rows; table = device int32 [M][2] = (slot, row in the slot's
// segment) - a segment's rows are consecutive in qkv / out and may be more than 16; slot in [0, n_slots).  The finished flag of
// the state rows is not looked at.
int ds_launch_llm_attn_rows(const LlmAttnParams& p, const int* table, int n_slots, hipStream_t stream);
int ds_launch_llm_rmsnorm(const half_t* x, long ldx, const half_t* gamma, half_t* y, long ldy, half_t* feat,
                          const int* state, int state_stride, int M, int H, int max_out, float eps, hipStream_t stream);
int ds_launch_llm_embed(const half_t* table, const int* state, int state_stride, half_t* out, long ldo, int M, int H,
                        int vocab, hipStream_t stream);
int ds_launch_llm_select(const half_t* logits, long ldl, int V, const int* chain, int n_chain, int out_cap, int adv,
                         int* state, int state_stride, int* out_ids, int M, int pause, hipStream_t stream);
// pause = 1 (chain fast-forward): a row that did not finish and whose new id lies in chain[:-1] gets state[2] = 2; 0: as ever
int ds_launch_llm_advance(int* state, int rows, hipStream_t stream);
int ds_launch_blend(const half_t* a, const half_t* b, half_t* out, long n, float s, hipStream_t stream);
int ds_launch_llm_swiglu(const half_t* gu, half_t* act, int M, int I, hipStream_t stream);
// batched decode: M <= 16 sequences per weight pass (matrix pipe)
int ds_launch_llm_gemm16(const LlmGemvParams& p, hipStream_t stream);
// w16[n][k] = f16(f32(q[n][k]) * scale[n]): an int8 weight matrix back to fp16 for the prompt pass's MFMA GEMMs
int ds_launch_llm_dequant_w8(const int8_t* q, const float* scale, half_t* w16, long N, int K, hipStream_t stream);
// w16[n][k] = f16(f32(e2m1[n][k] * 2^(w_exp[n][k/32] - 127)) * scale[n]): the same for an MXFP4 matrix (q [N,K/2], K % 32 == 0)
int ds_launch_llm_dequant_fp4(const uint8_t* q, const uint8_t* w_exp, const float* scale, half_t* w16, long N, int K,
                              hipStream_t stream);

// ---- character-reference pre-processing (preprocess.hip): Pillow's 8-bit separable resize + crop + normalise ----
int ds_launch_resize_h(const uint8_t* src, int H, int W, const int* first, const int* count, const int* taps, int ksize,
                       int out_w, uint8_t* dst, hipStream_t stream);
int ds_launch_resize_v_norm(const uint8_t* tmp, int Ht, int Wt, const int* first, const int* count, const int* taps,
                            int ksize, int top, int left, int out_h, int out_w, float scale, const float* mean3,
                            const float* std3, float* out_f32, uint8_t* out_u8, hipStream_t stream);
