/* diffsensei_hip.h — C ABI of the MI355X (gfx950) DiffSensei sampling kernels.
 *
 * This is the drop-in boundary for ONE path of jianzongwu/DiffSensei: the SDXL-UNet denoising loop with
 * region-masked IP-Adapter cross-attention (reference src/pipelines/pipeline_diffsensei.py:310-337,
 * src/models/unet.py:116-347, src/models/attention_processor.py, src/models/resampler.py).
 * The reference has no FFI of its own (pure Python over torch/diffusers); these entry points are what a
 * ctypes binding for that path binds (see INTEGRATION.md for the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch.Tensor.data_ptr()); the library never
 *     allocates or frees device memory and keeps no reference after the call returns (plans excepted: a plan
 *     borrows every pointer baked into its ops until ds_plan_destroy);
 *   - activations are fp16, channels-last: images [B, H*W, C], token matrices [rows, C];
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work is
 *     asynchronous on it, no hidden synchronisation;
 *   - return value: 0 = ok, negative = error (message via ds_last_error()); nothing throws or aborts.
 */
#ifndef DIFFSENSEI_HIP_H
#define DIFFSENSEI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* ds_last_error(void);
int ds_version(void);
/* number of HIP devices visible / properties of the current one (sanity for loaders) */
int ds_device_info(int* cu_count, int* lds_bytes, char* arch_name, int arch_name_len);
/* Tuning / test knobs.  THREAD-LOCAL since round 5 (no global mutable state beside the last-error slot - which is
 * thread-local too): a value set here changes only the launches the CALLING THREAD issues afterwards; other threads, and so
 * other serving handles of the process, keep the automatic dispatch.  Every knob defaults to 0 = automatic, which is what
 * production runs.
 * They exist so that A/B runs and the parity tests can force a kernel variant the automatic rule would only pick at
 * large problem sizes.  Variants of one operator that share their arithmetic are bit-identical and the tests assert torch.equal
 * between them (GEMM families, conv block sizes, flash attention <1> / <2>, ip_attn variants, hipGraph vs eager); the ones that
 * re-associate a sum - self_attn_sp_kernel vs the flash kernels, gn_variant 1's chunking - are compared at a stated tolerance.
 *   "gemm_variant"       0 auto | 1 register-staged only | 2, 7 two-buffer LDS-DMA | 8, 9 one-buffer LDS-DMA |
 *                        3 256x256 ping-pong (gemm_pp_kernel) | 10 halo-patch conv | 11 64x160 tiles (gemm_t160_kernel)
 *   "gemm_t160"          0 (default) small-batch projections whose 64x160 (or, failing that, 128x160) grid is one block per CU
 *                        run gemm_t160_kernel | 1 never (A/B) | 2 never its 128-row tile | 3 128-row tiles wherever it runs (tests)
 *   "gemm_g320"          0 (default) ds_gemm_g320_fits follows its shape rule | 1 it answers 0 (A/B: planners then keep the
 *                        128-row GEGLU packing and the 128 x 128 / 256 x 256 kernels)
 *   "gemm_pp_even"       1 (default) gemm_pp_kernel's persistent grid = ceil(tiles / rounds) blocks, every round full |
 *                        0 one block per CU with a partial last round
 *   "gemm_ring"          0 (default) grids of <= 512 64x128 blocks (num_samples 1) use the ring-buffered
 *                        gemm_glds_kernel<64,false,3|4> | 1 never (A/B: profiles/r02_ring_in_pipeline_ab.txt)
 *   "gemm_pp_narrow"     0 (default) the N, K <= 640 projections run gemm_pp_kernel where its ragged last tile column takes the
 *                        branch-free epilogue (plain epilogue, N % 64 == 0, M % 256 == 0) | 1 never: the 128x128 kernels, the
 *                        rule of rounds 1-5 (A/B: profiles/r06_pp_narrow_ab.txt)
 *   "conv_halo_variant"  0 auto (16x16-pixel blocks from 1024 blocks on; the ring-buffered 8x16 kernel for grids of at most
 *                        "conv_deep_blocks" blocks per CU) | 1 force conv_halo_kernel (8x16 pixels) | 2 force conv_halo256_kernel
 *                        (16x16 pixels) | 3 force conv_halo_deep_kernel (8x16 pixels, W ring of three buffers: small grids) |
 *                        4 auto without conv_halo_deep_kernel (A/B)
 *   "conv_deep_blocks"   grids of <= this many 8x16 blocks per CU run conv_halo_deep_kernel (default 1; 0 = never)
 *   "attn_variant"       0 auto (>= 128 blocks of 256 query rows: the software-pipelined self_attn_sp_kernel - every UNet shape
 *                        at every batch; smaller grids: self_attn_kernel<1>) | 1 force self_attn_kernel<1> (32 rows per wave) |
 *                        2 force self_attn_kernel<2> (64 rows per wave) | 3 force self_attn_sp_kernel | 4 the same with the
 *                        plain block order instead of the per-XCD head grouping (A/B: profiles/r03_self_attn_sp.txt)
 *   "ip_attn_min_blocks" grid size below which ip_attn_kernel stops doubling its query tiles per block (default 1024)
 *   "ip_attn_variant"    0 / 1 the register-staged ip_attn_kernel<4,false> | 2 force the 8-wave LDS-DMA ring kernel
 *                        ip_attn_kernel<8,true> where N % 256 == 0 - bit-identical results; faster back to back, slower inside the
 *                        UNet forward, so never automatic (A/B: profiles/r04_ipattn_ring_ab.txt, r04_forward_option_ab.txt) |
 *                        3 the register-staged kernel WITHOUT the round-6 specialisation that never issues the work of the padding
 *                        keys 80..95 (taken automatically when both key counts lie in (64, 80]; bit-identical; A/B)
 *   "gn_variant"         0 (default) GroupNorm on 512-thread blocks with >= 64 rows per block | 1 the round-3 geometry
 *                        (256 threads, 8-row chunks; A/B: profiles/r04_gn_geometry_ab.txt)
 *   "llm_gemv_variant"   0 auto (software-pipelined persistent GEMV) | 1 one column per wavefront | 2 un-pipelined streaming GEMV
 *   "gemm_debug"         bits 0..7: ablation builds of gemm_pp_kernel (only in a library built with -DDS_ABLATION; 0 otherwise) |
 *                        bit 8 (256): gemm_pp_kernel drains a tile's C stores before the next tile's first k-tile instead of
 *                        letting them retire under it - same bits out (tests/test_gpu_ops.py::test_gemm_pingpong_tile_handover) |
 *                        bit 10 (1024): halo-patch convs use the row-index patch swizzle (2-way LDS bank conflicts; A/B only)
 * returns 0, or -1 (ds_last_error()) for an unknown key / out-of-range value */
int ds_set_option(const char* key, int value);
/* Debug counters kept by the kernels on the current device (test instrumentation; SYNCHRONISES the device - never on a serving path).
 *   "attn_sp_recentre"  how many times self_attn_sp_kernel's rare re-centring branch ran (per wave and query block) since the
 *                       last reset: lets a model-level test prove that its logits crossed the 2^14 threshold
 *                       (tests/test_gpu_outlier_magnitudes.py).
 * *value receives the count; reset != 0 clears it afterwards.  Returns 0, or -1 for an unknown name. */
int ds_debug_counter(const char* name, int reset, long long* value);
/* Host-side query of the dispatch rule (no GPU work): 1 when a plain f16 GEMM of this shape runs gemm_t160_kernel (64 x 160
 * tiles, one block per CU: the M = 2048, N = 1280 projections of a batch-1 request at 1024 x 1024).  A launch planner asks
 * before it requests that kernel's LayerNorm statistics format (DsOp GEMM i[11] = 160: three partial pairs per row and
 * 160-column tile - columns 0..63, 64..127, 128..159) and tells the consumers to add 3 N / 160 entries (i[10]); a direct
 * ds_gemm_ln_* call always gets the 64-column format. */
int ds_gemm_t160_fits(int M, int N, int K, int batch);
/* Host-side query of the dispatch rule (no GPU work): 1 when the GEGLU projection [M, N packed] x K of a small-batch request
 * should run gemm_g320_kernel (256 x 320 tiles, exactly one block per CU: M = 2048, N = 10240, K = 1280 at UNet batch 2,
 * 1024 x 1024 - diffusers' GEGLU [3P] reached from reference src/models/unet.py:244-338).  That kernel reads W / bias / c
 * packed in groups of 320 rows (160 hidden rows, then their 160 gate rows) and is selected by epilogue code 4 (below);
 * a planner asks BEFORE packing.  Epilogue codes of the GEMM entry points: 0 none, 1 GEGLU (128-row groups: 64 hidden + 64
 * gates), 2 GELU, 3 QuickGELU, 4 GEGLU in 320-row groups. */
int ds_gemm_g320_fits(int M, int N, int K, int batch);
/* Host-side query: partial-sum chunks per image that a stride-1 3x3 convolution of this shape writes for the GroupNorm behind
 * it (DsOp CONV3X3 p[6] = the GroupNorm workspace; DsOp GROUPNORM i[6] = this number: the GroupNorm then skips its statistics
 * pass).  0: this convolution cannot (not a halo-patch kernel shape, or more than 128 pixel tiles per image).  Replaces the
 * first read of conv1's output by diffusers' ResnetBlock2D.norm2 [3P], reached from reference src/models/unet.py:244-338. */
int ds_conv3x3_gn_chunks(int B, int H, int W, int Cin, int Cout);

/* ------------------------------------------------------------------------------------------------
 * Operators.  Each replaces the torch call(s) named in its comment.
 * ---------------------------------------------------------------------------------------------- */

/* y[M,N] = act(x[M,K] @ w[N,K]^T + bias[N]) (+residual[M,N]).  epilogue: 0 none, 2 GELU(erf), 3 quick-GELU,
 * 1 GEGLU: w rows are packed per 128-row tile as 64 "hidden" + 64 "gate" rows and y[M,N/2] = hidden * gelu(gate).
 * replaces nn.Linear at reference src/models/attention_processor.py:56,63,64,84,207,225,226,245,246,261 and the
 * diffusers GEGLU/FeedForward/proj_in/proj_out linears reached from src/models/unet.py:244-338.
 * x2/k1: optional second A source for columns k >= k1 (channel concat of two tensors without a copy). */
int ds_gemm_f16(const void* x, int64_t ldx, const void* x2, int64_t ldx2, int k1, const void* w, int64_t ldw,
                const void* bias, const void* residual, int64_t ldr, void* y, int64_t ldy, int M, int N, int K,
                int epilogue, void* stream);

/* LayerNorm fused into the GEMM pair around it (round 4).  Replaces the three `nn.LayerNorm` passes of diffusers'
 * BasicTransformerBlock [3P] that the reference reaches from src/models/unet.py:244-338 (norm2 -> attn2.to_q,
 * norm3 -> ff.net.0 GEGLU; attention_processor.py:209 takes the normalised hidden states as its query input):
 *   producer  y = x w^T + bias (+ residual), and `stats_out` [N/64][M] float2 receives the (sum, sum of squares) of every
 *             stored row per 64-column strip;
 *   ds_ln_finalize: partial sums -> stats [M] float2 (mean, rstd = rsqrt(var + eps));
 *   consumer  y = rstd_m (x_m . gw_n - mean_m c_n) + b'_n on the RAW x, with gw = gamma (.) w (f16), ln_c [N][2] f16 =
 *             (-c hi, -c lo), c_n = sum_k gw_nk, bias_ln = bias + w beta - all packed once at load time (GEGLU: in the packed
 *             row order).  epilogue 0 or 1 (GEGLU).  Either role may be absent (null pointers), both may be combined.
 * Two implementations, one statistics format.  ds_gemm_ln_fusable(M, N, K, epilogue, batch) says which one ds_gemm_f16's
 * dispatch gives the shape: 1 = the 256 x 256 persistent kernel (M, N multiples of 256, K of 128; consumers take the
 * finalised ln_stats of ds_ln_finalize through ds_gemm_ln_f16), 2 = the 128-wide kernels of small batches and of the
 * 640-channel level (N a multiple of 128, K of 64; producers through ds_gemm_ln_f16 with ln_stats = NULL, consumers through
 * ds_gemm_ln_partial_f16, which sums the K/64 partials of its own rows in the epilogue - no finalize launch), 0 = neither
 * (callers keep ds_layernorm_f16 + ds_gemm_f16).  Producers and consumers of either kind combine. */
int ds_gemm_ln_f16(const void* x, int64_t ldx, const void* gw, int64_t ldw, const void* bias_ln, const float* ln_stats,
                   const void* ln_c, const void* residual, int64_t ldr, void* y, int64_t ldy, float* stats_out, int M, int N,
                   int K, int epilogue, void* stream);
int ds_gemm_ln_partial_f16(const void* x, int64_t ldx, const void* gw, int64_t ldw, const void* bias_ln, const float* ln_partial,
                           float eps, const void* ln_c, const void* residual, int64_t ldr, void* y, int64_t ldy, float* stats_out,
                           int M, int N, int K, int epilogue, void* stream);
int ds_ln_finalize(const float* partial, float* stats, int M, int strips, int C, float eps, void* stream);
/* operand-swapped consumer (norm1 -> attn1.to_v, produced transposed: y[b] = a @ LN(x[b])^T, a = gamma (.) Wv [M,K] shared,
 * x[b] the raw rows [N,K] of batch item b): the normalised rows index the OUTPUT COLUMNS, so ln_stats is read at
 * [b * ln_bstride + n] and ln_cb is [M][4] f16 = (-c hi, -c lo, b' hi, b' lo) per output row. */
int ds_gemm_ln_swapped_f16(const void* a, int64_t lda, const void* x, int64_t ldx, int64_t sx, const float* ln_stats,
                           int64_t ln_bstride, const void* ln_cb, void* y, int64_t ldy, int64_t sy, int M, int N, int K,
                           int batch, void* stream);
/* the same on the 128-wide kernels: ln_partial = the producer's partial sums [K/64][ln_rows] float2 (ln_rows = rows of the
 * normalised matrix over all batch items); every block finalises the statistics of its 128 output columns itself. */
int ds_gemm_ln_swapped_partial_f16(const void* a, int64_t lda, const void* x, int64_t ldx, int64_t sx, const float* ln_partial,
                                   float eps, int64_t ln_rows, int64_t ln_bstride, const void* ln_cb, void* y, int64_t ldy,
                                   int64_t sy, int M, int N, int K, int batch, void* stream);
int ds_gemm_ln_fusable(int M, int N, int K, int epilogue, int batch);

/* batched variant: grid.z = batch with element strides (0 = shared operand); used for V^T = Wv @ X_b^T */
int ds_gemm_f16_batched(const void* x, int64_t ldx, int64_t sx, const void* w, int64_t ldw, int64_t sw, void* y,
                        int64_t ldy, int64_t sy, int M, int N, int K, int batch, void* stream);

/* ---- VAE decoder (bf16 storage, fp32 accumulate): replaces AutoencoderKL.decode reached from reference
 * src/pipelines/pipeline_diffsensei.py:339-367 (the reference upcasts the VAE to fp32 because fp16 overflows).
 * Same layouts as the f16 entry points; all tensors bf16 unless noted. */
/* y = conv3x3(x[B,H,W,Cin], w[Cout,3,3,Cin]) + bias (+ residual); stride 1; upsample != 0 = nearest x2 in front.
 * Cin % 64 == 0.  ResnetBlock2D.conv1/conv2, Upsample2D.conv of the decoder. */
int ds_conv3x3_bf16(const void* x, const void* w, const void* bias, const void* residual, void* y, int B, int H,
                    int W, int Cin, int Cout, int upsample, void* stream);
/* y[M,N] = x[M,K] @ w[N,K]^T + bias (+ residual); M, N % 16 == 0, K % 128 == 0: conv_shortcut (1x1), to_q/k/out */
int ds_gemm_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, const void* residual,
                 int64_t ldr, void* y, int64_t ldy, int M, int N, int K, void* stream);
/* batched (element strides, 0 = shared operand): V^T[b] = Wv @ X_b^T */
int ds_gemm_bf16_batched(const void* x, int64_t ldx, int64_t sx, const void* w, int64_t ldw, int64_t sw, void* y,
                         int64_t ldy, int64_t sy, int M, int N, int K, int batch, void* stream);
/* GroupNorm (+SiLU) over [B,HW,C]; ws: ds_groupnorm_workspace_bytes(B, C) */
int ds_groupnorm_bf16(const void* x, void* y, const void* gamma, const void* beta, void* ws, int B, int HW, int C,
                      int groups, float eps, int silu, void* stream);
/* single-head attention, head dim 512: q,k,o [B,N,512], vt [B,512,N]; N % 8 == 0.  Decoder mid_block.attentions.0.
 * n_valid (0 = N): only keys [0, n_valid) take part - rows [n_valid, N) are the caller's padding (latent sizes whose
 * token count is not a multiple of 16 are padded on the host side of the VAE engine). */
int ds_wide_attn_bf16(const void* q, const void* k, const void* vt, void* o, int B, int N, int n_valid, float scale,
                      void* stream);
/* y[B,H,W,C] = conv_in(post_quant_conv(latents / scaling_factor)); latents fp32 NCHW [B,4,H,W]; post_quant_w [4,4],
 * post_quant_b [4] fp32; w [C,3,3,4], bias [C] bf16 */
int ds_vae_conv_in_bf16(const float* latents, const float* post_quant_w, const float* post_quant_b, const void* w,
                        const void* bias, void* y, int B, int H, int W, int C, float scaling_factor, void* stream);
/* image fp32 NCHW [B,3,H,W] = conv_out(x[B,H,W,C]); w [3,3,3,C], bias [3] bf16; denormalize != 0 also applies
 * VaeImageProcessor.denormalize, (x / 2 + 0.5).clamp(0, 1) (pipeline_diffsensei.py:367 postprocess) */
int ds_vae_conv_out_bf16(const void* x, const void* w, const void* bias, float* image, int B, int H, int W, int C,
                         int denormalize, void* stream);

/* ---- the same decoder in scaled fp16 (diffsensei_amd/vae.py, precision "fp16-scaled": what runs when the VAE config has
 * force_upcast, i.e. where the reference upcasts the VAE to fp32 "as it overflows in float16", pipeline_diffsensei.py:339-344).
 * All tensors f16.  Conv outputs and the residual stream are stored multiplied by S = 2^-6 (range 4.2e6, fp16's 11-bit
 * mantissa instead of bf16's 8), conv INPUTS are O(1): GroupNorm+SiLU outputs, pre-multiplied by S through `out_scale` so
 * that every accumulator already carries the factor; biases are pre-scaled on the host; GroupNorm of a scaled tensor is
 * exact with eps * S^2.  The 3x3 convs and linears go through ds_conv3x3_f16 / ds_gemm_f16 / ds_gemm_f16_batched. */
/* GroupNorm (+SiLU) over x[B,HW,C], y = act(norm(x)) * out_scale; ws: ds_groupnorm_workspace_bytes(B, C) */
int ds_groupnorm_scaled_f16(const void* x, void* y, const void* gamma, const void* beta, void* ws, int B, int HW, int C,
                            int groups, float eps, int silu, float out_scale, void* stream);
/* ds_wide_attn_bf16 / ds_vae_conv_in_bf16 / ds_vae_conv_out_bf16 with f16 tensors (same arguments) */
int ds_wide_attn_f16(const void* q, const void* k, const void* vt, void* o, int B, int N, int n_valid, float scale,
                     void* stream);
int ds_vae_conv_in_f16(const float* latents, const float* post_quant_w, const float* post_quant_b, const void* w,
                       const void* bias, void* y, int B, int H, int W, int C, float scaling_factor, void* stream);
int ds_vae_conv_out_f16(const void* x, const void* w, const void* bias, float* image, int B, int H, int W, int C,
                        int denormalize, void* stream);

/* ---- VAE encoder: replaces AutoencoderKL.encode (diffusers [3P]) so that region redraw can start from a picture
 * (diffsensei_amd/vae.py VaeEncoderEngine).  Resnets, GroupNorms, the 1x1 shortcuts and the dim-512 attention are the decoder's
 * entry points above, in either storage mode; these are the four ops that have no decoder counterpart. */
/* Downsample2D(padding=0): F.pad(x, (0,1,0,1)) then a 3x3 convolution with stride 2 and no padding.  x [B,H,W,Cin] NHWC,
 * w [Cout,3,3,Cin], y [B,H/2,W/2,Cout] (floor): output (Y, X) reads rows 2Y + ky, columns 2X + kx; rows >= H and columns >= W
 * read as zero.  Cin % 64 == 0.  ds_conv3x3_f16 with stride 2 pads 1 on every side instead (the UNet's downsamplers). */
int ds_conv3x3_down_f16(const void* x, const void* w, const void* bias, void* y, int B, int H, int W, int Cin, int Cout,
                        void* stream);
int ds_conv3x3_down_bf16(const void* x, const void* w, const void* bias, void* y, int B, int H, int W, int Cin, int Cout,
                         void* stream);
/* y[B,H,W,C] = conv_in(image), 3x3, 3 -> C, pad 1 (zero padding of the NORMALISED image).  image_is_u8 != 0: image is uint8
 * NHWC [B,H,W,3] and the kernel computes fma(u, 2/255, -1) in fp32; else fp32 NCHW [B,3,H,W] already in [-1, 1].
 * w [C,3,3,3], bias [C] in the storage type (f16 / bf16), as is y. */
int ds_vae_enc_conv_in_f16(const void* image, int image_is_u8, const void* w, const void* bias, void* y, int B, int H, int W,
                           int C, void* stream);
int ds_vae_enc_conv_in_bf16(const void* image, int image_is_u8, const void* w, const void* bias, void* y, int B, int H, int W,
                            int C, void* stream);
/* moments fp32 NCHW [B,8,H,W] = quant_conv(conv_out(x[B,H,W,C])): w [8,3,3,C] in the storage type with quant_conv folded in
 * (W' = Wq Wc), bias fp32 [8] (b' = Wq bc + bq); channels 0..3 = mean, 4..7 = logvar clamped to [-30, 20]. */
int ds_vae_enc_conv_out_f16(const void* x, const void* w, const float* bias, float* moments, int B, int H, int W, int C,
                            void* stream);
int ds_vae_enc_conv_out_bf16(const void* x, const void* w, const float* bias, float* moments, int B, int H, int W, int C,
                             void* stream);
/* latents fp16 NCHW [B,4,HW] = fp16((z - shift[c]) * scale[c]) with z = mean (seeds == NULL: the mode) or
 * z = mean + exp(0.5 logvar) * n, n = the device noise below for (seeds[b], pixel, step 0, stream_id 1); seeds: device int64 [B].
 * shift4 (may be NULL = 0) and scale4 are HOST pointers to 4 floats: latents_mean and scaling_factor / latents_std, or 0 and
 * scaling_factor. */
int ds_vae_latents_f16(const float* moments, const int64_t* seeds, const float* shift4, const float* scale4, void* latents,
                       int B, int HW, void* stream);

/* 3x3 convolution, pad 1, NHWC: y[B,Ho,Wo,Cout] = conv(x[B,H,W,Cin], w[Cout,3,3,Cin]) + bias
 * (+ rowbias[b, :] per image — the resnet time_emb_proj term) (+ residual).  stride in {1,2};
 * upsample != 0 fuses a nearest x2 upsample in front (diffusers Upsample2D).  Cin % 64 == 0.
 * replaces ResnetBlock2D.conv1/conv2, Downsample2D.conv, Upsample2D.conv reached from src/models/unet.py:244-332. */
int ds_conv3x3_f16(const void* x, const void* w, const void* bias, const void* rowbias, int64_t rowbias_ld,
                   const void* residual, void* y, int B, int H, int W, int Cin, int Cout, int stride, int upsample,
                   void* stream);
/* Upsample2D with an explicit output size (diffusers resizes to the skip tensor's size when a latent side is not a
 * multiple of 4 - `forward_upsample_size` [3P]): nearest resize of x [B,H,W,Cin] to Hout x Wout exactly as
 * F.interpolate(size=..., mode="nearest") indexes it (src = min(floor(dst * float(in)/out), in-1)), then the 3x3 conv.
 * The resized tensor never exists in HBM. */
int ds_conv3x3_resize_f16(const void* x, const void* w, const void* bias, const void* rowbias, int64_t rowbias_ld,
                          const void* residual, void* y, int B, int H, int W, int Cin, int Cout, int Hout, int Wout,
                          void* stream);
/* Upsample2D at exactly x2 without the arithmetic the nearest resize makes redundant: every 2x2 block of the upsampled
 * image is one input pixel, so output pixel (2Y+py, 2X+px) is a 2x2 convolution of the INPUT with sums of the 3x3 taps
 * (rows: py = 0 -> {0} | {1,2}, py = 1 -> {0,1} | {2}; columns alike) - 4 taps per pixel instead of 9.
 * ds_fold_upsample2x_f16: packed w [Cout, 9*Cin] (k = (ky*3+kx)*Cin + ci) -> wfold [4][Cout, 4*Cin] (phase py*2+px,
 * k = (a*2+b)*Cin + ci), summed in fp32 in (ky, kx) order and rounded to f16 once; done once per weight load.
 * ds_conv3x3_up2fold_f16: y[B,2H,2W,Cout] from x[B,H,W,Cin] and wfold; same epilogue as ds_conv3x3_f16.  Cin % 64 == 0.
 * Agrees with ds_conv3x3_f16(upsample = 1) to the extra f16 rounding of the folded weights, not bit for bit. */
int ds_fold_upsample2x_f16(const void* w, void* wfold, int Cout, int Cin, void* stream);
int ds_conv3x3_up2fold_f16(const void* x, const void* wfold, const void* bias, const void* rowbias, int64_t rowbias_ld,
                           const void* residual, void* y, int B, int H, int W, int Cin, int Cout, void* stream);

/* GroupNorm (+SiLU) over NHWC; x2 (may be NULL) supplies channels C1..C1+C2 (skip concat).  ws: device scratch
 * of ds_groupnorm_workspace_bytes(B, C1+C2) bytes. */
size_t ds_groupnorm_workspace_bytes(int B, int C);
int ds_groupnorm_f16(const void* x1, const void* x2, void* y, const void* gamma, const void* beta, void* ws, int B,
                     int HW, int C1, int C2, int groups, float eps, int silu, void* stream);
int ds_layernorm_f16(const void* x, void* y, const void* gamma, const void* beta, int rows, int C, float eps,
                     void* stream);

/* Flash self-attention, head_dim 64.  q,k: [B,N,ld] with head h at column h*64; vt: [B,heads,64,ldv] (V stored
 * key-contiguous); o: [B,N,ldo].  replaces F.scaled_dot_product_attention at
 * reference src/models/attention_processor.py:76-78. */
int ds_self_attn_f16(const void* q, int64_t ldq, int64_t sq, const void* k, int64_t ldk, int64_t sk, const void* vt,
                     int64_t ldv, void* o, int64_t ldo, int64_t so, int B, int heads, int Nq, int Nk, float scale,
                     void* stream);

/* (Rounds 2-5 carried an OCP e4m3 variant of this call for BASELINE.json configs[4] - ds_quantize_fp8_e4m3_f16 /
 * ds_self_attn_fp8_f16 on v_mfma_f32_32x32x64_f8f6f4.  Removed in round 6: 5.4e-2 per-op error on white noise - 25x the fp16
 * kernels' - for +3.7 % at 2048 x 2048, and the fp16 Q K^T / fp8 P V hybrid cannot go below 3.7e-2
 * (tests/test_fp8_error_floor.py).  configs[4] is served by the fp16 kernels.) */

/* Fused text + region-masked IP cross-attention core of MaskedIPAttnProcessor2_0
 * (reference src/models/attention_processor.py:235-258 incl. prepare_attention_mask_ip :115-169):
 *   o = softmax(q kt^T * s) vt  +  ip_scale * softmax(q ki^T * s + M(bbox)) vi
 * kt/ki: [B,96,C] key panels (rows >= Lt / Li are padding), vtt/vti: [B,C,96] transposed value panels (columns >= Lt / Li
 * are padding).  The padding may hold anything finite: those keys get probability exactly 0 and never reach the output
 * (Inf / NaN there would, as 0 * Inf).  q / o: [B,N,ldq] / [B,N,ldo] with head h at column h*64 (batch stride N rows).
 * bbox: [B,max_ips,4] fp32 relative boxes, (mask_h, mask_w): the grid the reference infers from (N, aspect_ratio).
 * ip_scale_dev: optional device float overriding ip_scale (lets a captured graph follow set_ip_scale).
 * ldk/sk: row / batch stride of the key panels, sv: batch stride of the value panels (elements; 0 = dense) —
 * the engine projects the text/IP tokens for all 70 layers with one stacked GEMM and hands out column slices. */
int ds_masked_ip_attn_f16(const void* q, int64_t ldq, const void* kt, const void* vtt, const void* ki,
                          const void* vti, const float* bbox, void* o, int64_t ldo, int B, int heads, int N, int Lt,
                          int Li, int n_dummy, int tok_per_ip, int max_ips, int mask_h, int mask_w, float qk_scale,
                          float ip_scale, const float* ip_scale_dev, int64_t ldk, int64_t sk, int64_t sv,
                          void* stream);
/* ds_masked_ip_attn_f16 with one IP scale per batch row: ip_scale_rows_dev is a device fp32 vector [B] and row b uses
 * element b,  w = (ip part ? ip_scale_rows_dev[b] : 1) / sum  - the scalar call's arithmetic with that row's value.
 * Panel <-> row rule: a classifier-free-guidance batch of ns panels is B = 2 ns rows, all negative rows first, so rows n
 * and ns + n both belong to panel n and the caller writes that panel's scale into both elements.  The vector is read at
 * launch time by every block (a captured graph follows what was last written to it). */
int ds_masked_ip_attn_rows_f16(const void* q, int64_t ldq, const void* kt, const void* vtt, const void* ki,
                               const void* vti, const float* bbox, void* o, int64_t ldo, int B, int heads, int N, int Lt,
                               int Li, int n_dummy, int tok_per_ip, int max_ips, int mask_h, int mask_w, float qk_scale,
                               const float* ip_scale_rows_dev, int64_t ldk, int64_t sk, int64_t sv, void* stream);
/* Long prompts: the same core with 1 <= Lt <= 384 text keys in text_panels = ceil(Lt / 96) panels of 96 rows (at most 4) -
 * kt [B, 96 text_panels, C] with row / batch strides ldkt / skt, vtt [B, C, 96 text_panels] (rows dense) with batch stride svt
 * (elements; 0 = dense).  ki / vti stay one 96-row panel with ldk / sk / sv.  The text softmax runs over all Lt keys (online
 * over the panels: fp32 scores, exp(s - running max) packed to fp16 for the P V product, fp32 accumulation, one division by
 * the row sum at the end); keys >= Lt get probability exactly 0 whatever finite values their rows hold.  The IP side, the
 * output and ip_scale_dev are ds_masked_ip_attn_f16's.  Lt > 384, Lt <= 0, a panel count that does not match Lt and strides
 * that are no multiples of 8 are refused before any launch. */
int ds_masked_ip_attn_long_f16(const void* q, int64_t ldq, const void* kt, const void* vtt, const void* ki, const void* vti,
                               const float* bbox, void* o, int64_t ldo, int B, int heads, int N, int Lt, int text_panels, int Li,
                               int n_dummy, int tok_per_ip, int max_ips, int mask_h, int mask_w, float qk_scale, float ip_scale,
                               const float* ip_scale_dev, int64_t ldkt, int64_t skt, int64_t svt, int64_t ldk, int64_t sk,
                               int64_t sv, void* stream);
/* ds_masked_ip_attn_long_f16 with one IP scale per batch row (see ds_masked_ip_attn_rows_f16) */
int ds_masked_ip_attn_long_rows_f16(const void* q, int64_t ldq, const void* kt, const void* vtt, const void* ki, const void* vti,
                                    const float* bbox, void* o, int64_t ldo, int B, int heads, int N, int Lt, int text_panels,
                                    int Li, int n_dummy, int tok_per_ip, int max_ips, int mask_h, int mask_w, float qk_scale,
                                    const float* ip_scale_rows_dev, int64_t ldkt, int64_t skt, int64_t svt, int64_t ldk,
                                    int64_t sk, int64_t sv, void* stream);
/* debug/test hook: bit k of flags[b*N+i] = token i inside box k (the reference's inside_bbox_mask) */
int ds_ip_region_flags(const float* bbox, uint8_t* flags, int B, int N, int max_ips, int mask_h, int mask_w,
                       void* stream);

/* generic small attention (head_dim <= 256, arbitrary lengths): encoders + perceiver resampler
 * (reference src/models/resampler.py:67-72).  q/k/v/o: [B,N,ld] with head h at column h*D. */
int ds_small_attn_f16(const void* q, int64_t ldq, int64_t sq, const void* k, int64_t ldk, int64_t sk, const void* v,
                      int64_t ldv, int64_t sv, void* o, int64_t ldo, int64_t so, int B, int heads, int Nq, int Nk,
                      int D, float scale, void* stream);

/* causal variant (token t attends to tokens <= t): the SDXL CLIP text encoders reached through `encode_prompt`
 * (reference src/pipelines/pipeline_diffsensei.py:237-245 -> transformers CLIPTextModel [3P]) */
int ds_small_attn_causal_f16(const void* q, int64_t ldq, int64_t sq, const void* k, int64_t ldk, int64_t sk, const void* v,
                             int64_t ldv, int64_t sv, void* o, int64_t ldo, int64_t so, int B, int heads, int N, int D,
                             float scale, void* stream);
/* out[b,t,:] = tok_emb[ids[b,t],:] + pos_emb[t,:]  (CLIPTextEmbeddings [3P]); ids int32 [B,T] */
int ds_embed_tokens_f16(const int32_t* ids, const void* tok_emb, const void* pos_emb, void* out, int B, int T, int D,
                        int vocab, void* stream);

/* conv_in (Cin=4) fused with UNetMangaModel.encode_dialog_bbox (reference src/models/unet.py:206-210, :88-114).
 * dialog_boxes: int32 [B,ndialog,4] pixel boxes (x1,y1,x2,y2), already truncated/clamped like the reference. */
int ds_conv_in_dialog_f16(const void* x, const void* w, const void* bias, const int32_t* dialog_boxes,
                          const void* dialog_emb, void* y, int B, int H, int W, int Cin, int Cout, int ndialog,
                          void* stream);
/* conv_out (Cout=4) on an already GroupNorm+SiLU'd input (reference src/models/unet.py:335-338) */
int ds_conv_out_f16(const void* x, const void* w, const void* bias, void* y, int B, int H, int W, int Cin, int Cout,
                    void* stream);

/* y[M,N] = act_out(act_in(x)[M,K] @ w[N,K]^T + bias + addend), M small (time-embedding MLPs, time_emb_proj) */
int ds_skinny_linear_f16(const void* x, const void* w, const void* bias, const void* addend, void* y, int M, int N,
                         int K, int silu_in, int silu_out, void* stream);

/* Per-step scalar table (device, fp32, 8 floats per row):
 *   {timestep, c_in_div, k0, k1, k2, k3, c_in_div_next, guidance_scale}
 *   Euler: k0 = sigma_i, k1 = sigma_{i+1};  DDIM: k0..k3 = sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)
 * `step_ctr` (device int32, may be NULL = row 0) selects the row. */
int ds_timestep_embed_f16(const float* table, const int32_t* step_ctr, void* out, int B, int dim, int flip_sin_to_cos,
                          float freq_shift, void* stream);
int ds_add_time_ids_f16(const void* text_embeds, const void* time_ids, void* out, int B, int pooled_dim, int n_ids,
                        int dim, int flip_sin_to_cos, float freq_shift, void* stream);
/* classifier-free guidance + scheduler.step + next scale_model_input in one launch
 * (reference src/pipelines/pipeline_diffsensei.py:315-317, :333-337).  eps: NHWC [2ns,HW,4] (uncond first);
 * latents: NCHW [ns,4,HW] updated in place; model_in: NHWC [2ns,HW,4].  kind: 0 Euler, 1 DDIM (2 and 3 need more
 * arguments: ds_cfg_dpm_step_f16, ds_cfg_sampler_step_noise_f16). */
int ds_cfg_sampler_step_f16(const void* eps, void* latents, void* model_in, const float* table,
                            const int32_t* step_ctr, int ns, int HW, int kind, int do_cfg, void* stream);
/* DPM-Solver++ (diffusers DPMSolverMultistepScheduler, algorithm_type "dpmsolver++", epsilon prediction, order 1|2):
 * CFG + the multistep update + the next model input (= the new latents) in one launch, on the same layouts as above.
 * The per-step table carries {t, 1, 0, 0, 0, 0, 1, guidance}; `solver` (device, fp32, 8 floats per row, the same
 * step_ctr) carries the update:
 *   {order, sigma_s, alpha_s, a, b, 1/r0, c, 0}   with alpha = 1/sqrt(1+sigma_ve^2), sigma = sigma_ve*alpha,
 *   lambda = log(alpha) - log(sigma), h = lambda_t - lambda_s, r0 = (lambda_s - lambda_s1) / h,
 *   a = sigma_t/sigma_s, b = alpha_t*(exp(-h)-1), c = 0.5*b (midpoint) or -alpha_t*((exp(-h)-1)/h+1) (heun)
 *   x0 = fp16(fp16(x - fp16(sigma_s*eps)) / alpha_s);  x' = fp16(a*x - fp16(b*x0) [- fp16(c*D1)]) with
 *   D1 = fp16(fp16(x0 - prev_x0) * (1/r0)), the bracket only on rows with order 2.
 * prev_x0: NCHW [ns,4,HW] fp16, read by order-2 rows and overwritten with x0 on every row (never read on order 1). */
int ds_cfg_dpm_step_f16(const void* eps, void* latents, void* model_in, const float* table, const float* solver,
                        void* prev_x0, const int32_t* step_ctr, int ns, int HW, int do_cfg, void* stream);
/* Device noise: Philox4x32-10 (Salmon et al., Random123; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants
 * 0x9E3779B9 / 0xBB67AE85) + Box-Muller, keyed per panel so that what a panel sees depends on its own seed and the step
 * only - not on its row in the batch, the rows beside it or the rank it runs on:
 *   key     = (seed & 0xffffffff, seed >> 32)            seeds: device int64 [ns], one per panel
 *   counter = (pixel, 0, step, stream_id)                pixel = 0 .. HW-1 inside the panel
 *   x0..x3  = the four latent channels of that pixel;  u_k = x_k * 2^-32 + 2^-33 in fp32 (never 0)
 *   channels 0,1 = sqrt(-2 ln u0) * {cos, sin}(2 pi u1);  channels 2,3 the same from (u2, u3)
 * stream_id 0 = sampler-step noise; 1 = the VAE encoder's posterior sample (ds_vae_latents_f16, step 0); 2.. are reserved
 * (initial latents, other samplers) and unused so far.
 * ds_philox_u32: the raw words, uint32 [ns,HW,4].  ds_philox_normal_f32: the normals, fp32 NCHW [ns,4,HW]. */
int ds_philox_u32(const int64_t* seeds, int step, int stream_id, uint32_t* out, int ns, int HW, void* stream);
int ds_philox_normal_f32(const int64_t* seeds, int step, int stream_id, float* out, int ns, int HW, void* stream);
/* ds_cfg_sampler_step_f16 with a noise source: kind 0 / 1 as above (seeds unused, may be NULL) and
 * kind 3 = Euler Ancestral (diffusers EulerAncestralDiscreteScheduler, epsilon prediction), table row
 *   {t, c_in_div, sigma, sigma_down, sigma_up, 0, c_in_div_next, guidance}
 *   x' = fp16( x + ((x - (x - sigma*eps)) / sigma) * (sigma_down - sigma) + fp16(sigma_up * fp16(z)) ),  x upcast to fp32,
 *   z = the normals above for (seeds[n], pixel, step = *step_ctr (0 when NULL), stream_id 0).
 * The last row has sigma_down = sigma_up = 0: no noise.  kind 3 needs `seeds`; ds_cfg_sampler_step_f16 has none to give
 * and refuses it. */
int ds_cfg_sampler_step_noise_f16(const void* eps, void* latents, void* model_in, const float* table,
                                  const int64_t* seeds, const int32_t* step_ctr, int ns, int HW, int kind, int do_cfg,
                                  void* stream);
/* The sampler step with one guidance scale per panel, for every kind (0 Euler, 1 DDIM, 2 DPM-Solver++, 3 Euler
 * Ancestral, 4 LCM): the superset of the three calls above.  guidance: device fp32 [ns]; panel n - eps rows n (negative) and
 * ns + n (conditional), latents / prev_x0 / seeds element n - uses guidance[n] where the calls above use column 7 of the
 * table row:  gd = fp16(guidance[n] * fp16(ec - eu)),  e = fp16(eu + gd).  NULL = column 7, i.e. exactly the calls above.
 * Not read when do_cfg = 0.  solver: kinds 2 and 4, prev_x0: kind 2, seeds: kinds 3 and 4 (NULL otherwise).
 * kind 4 = LCM (diffusers LCMScheduler, epsilon prediction), the few-step consistency sampler.  Six scalars per step: four
 * in the table row, two in the solver row of the same step_ctr -
 *   table  {t, 1, sqrt(a_t), sqrt(1 - a_t), c_out, c_skip, 1, guidance}     solver  {sqrt(a_prev), sqrt(1 - a_prev), 0 x 6}
 *   with s = t * timestep_scaling, c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25), a = alphas_cumprod, prev = the
 *   NEXT row's timestep; the last row's solver pair is {1, 0}
 *   x0 = (x - sqrt(1 - a_t) * eps) / sqrt(a_t);  d = c_out * x0 + c_skip * x                                (fp32, x upcast)
 *   x' = fp16( sqrt(a_prev) * d + fp16(sqrt(1 - a_prev) * fp16(z)) ),  z = the normals of kind 3: same stream, same counter
 * so the last row stores the denoised value d itself, without noise.  The model input is the latent (c_in_div = 1).  kind 4
 * needs `solver` AND `seeds`: this call, the redraw call and the slots call carry both; ds_cfg_sampler_step_f16,
 * ds_cfg_dpm_step_f16 and ds_cfg_sampler_step_noise_f16 cannot and refuse it. */
int ds_cfg_sampler_step_panels_f16(const void* eps, void* latents, void* model_in, const float* table,
                                   const float* guidance, const float* solver, void* prev_x0, const int64_t* seeds,
                                   const int32_t* step_ctr, int ns, int HW, int kind, int do_cfg, void* stream);
/* Region redraw: masked, strength-based sampling from kept latents.  The step of ds_cfg_sampler_step_panels_f16 (all its
 * arguments, same meaning) followed, in the same launch, by the blend of diffusers' 4-channel inpainting loop [3P]: the
 * kept region is reset to the original latents re-noised to the noise level of the state the step produced.
 * `redraw`: ONE device buffer, 16-byte aligned, ds_redraw_buffer_bytes(ns, HW) bytes, offsets from ns and HW alone:
 *   x0k    fp16 NCHW [ns,4,HW]   the kept latents (the final latents of an earlier run)          at byte 0
 *   noise  fp16 NCHW [ns,4,HW]   the fixed start noise, unit variance                            at byte 8*ns*HW
 *   mask   fp16 [ns,HW]          one value per panel and pixel in [0, 1]; 1 = repaint            at byte 16*ns*HW
 *   (pad to the next multiple of 16 bytes: F = (18*ns*HW + 15) & ~15)
 *   header fp32 [4]              {full strength (0 | 1), init_noise_sigma, 0, 0}                 at byte F
 *   rows   fp32 [1025][2]        the renoise table, row r = {ka, kb} of STATE r                  at byte F + 16
 * Renoise table: state r is what enters step r of the run (r = 0: the start) and state n_run is the result; a kept
 * latent at the noise level of state r is ka * x0k + kb * noise:
 *   Euler, Euler Ancestral  {1, sigma_r}                     DDIM, LCM  {sqrt(a_r), sqrt(1 - a_r)}
 *   DPM-Solver++            {alpha_r, sigma_r * alpha_r}, alpha = 1 / sqrt(sigma^2 + 1)      final state, every kind  {1, 0}
 * The table does not depend on `kind` inside the kernel.  A run that starts mid-schedule (strength < 1) loads the rows
 * of its own states: row 0 is its start state, and step_ctr counts from 0 (kind 3 therefore draws its Philox noise for
 * the run-relative step).  Per pixel (one thread, 4 channels), with m = mask[n][pix], xn the step's result in fp32:
 *   m == 1:  latent = fp16(xn)                              bit for bit the call above; x0k / noise are not read
 *   else     known  = fp16(ka * x0k + kb * noise)           fp32 arithmetic (one contraction), {ka, kb} = row *step_ctr + 1
 *   m == 0:  latent = known                                 on the last row {1, 0}: x0k bit for bit
 *   else     latent = fp16(m * fp16(xn) + (1 - m) * known)  fp32 arithmetic
 * prev_x0 (kind 2) receives the step's own x0, before the blend; model_in is formed from the blended latent for both
 * CFG halves.  The mask's range is the caller's to check (no kernel reads it twice); a NULL `redraw` is refused. */
int ds_cfg_sampler_step_redraw_f16(const void* eps, void* latents, void* model_in, const float* table,
                                   const float* guidance, const float* solver, void* prev_x0, const int64_t* seeds,
                                   const void* redraw, const int32_t* step_ctr, int ns, int HW, int kind, int do_cfg,
                                   void* stream);
int64_t ds_redraw_buffer_bytes(int ns, int HW);
/* The state a redraw run starts from, out of the same buffer: latents[ns,4,HW] = fp16(ka0 * x0k + kb0 * noise) with
 * {ka0, kb0} = renoise row 0 (fp32, one rounding); with the header's full-strength flag set, fp16(noise *
 * init_noise_sigma) instead - the product a plain run starts from, so strength 1 with an all-ones mask IS the plain run. */
int ds_redraw_start_f16(const void* redraw, void* latents, int ns, int HW, void* stream);
int ds_prepare_model_input_f16(const void* latents, void* model_in, const float* table, const int32_t* step_ctr,
                               int ns, int HW, int do_cfg, void* stream);
/* Panel schedules (continuous batching): every panel slot of a sampling batch runs its own schedule, so requests with
 * different step counts, strengths and plain / redraw modes share one UNet batch and a finished panel's slot is handed to
 * the next request while the others keep going.  `panel`: ONE device buffer, 16-byte aligned,
 * ds_panel_schedule_bytes(ns) bytes, offsets from ns alone; R = DS_PANEL_MAX_ROWS, the row capacity of a slot:
 *   start    int32 [ns]          value of the global step counter at which the panel's schedule begins     at byte 0
 *   steps    int32 [ns]          rows the panel runs; 0 = an empty slot                                    at byte 4*ns
 *   (pad to the next multiple of 16 bytes: F = (8*ns + 15) & ~15)
 *   mode     fp32 [ns][4]        {start mode, init_noise_sigma, 0, 0}; start mode 0 = renoise row 0,       at byte F
 *                                1 = full strength (noise * init_noise_sigma), 2 = keep the latents (a plain panel)
 *   coef     fp32 [ns][R][8]     the panel's rows of the per-step scalar table (column 7 is not read)      at byte F + 16*ns
 *   solver   fp32 [ns][R][8]     its DPM-Solver++ or LCM rows (kinds 2, 4)                                 at byte F + 16*ns + 32*R*ns
 *   renoise  fp32 [ns][R+1][2]   its renoise rows {ka, kb}, state r of ITS run (region redraw)             at byte F + 16*ns + 64*R*ns
 * With s = *step_ctr panel n is at its row j = s - start[n]; it is active iff 0 <= j < steps[n] (steps above R count as R).
 * ds_panel_slot_load writes one slot from DEVICE rows - coef_rows [steps][8], solver_rows [steps][8] (NULL: kept),
 * renoise_rows [steps+1][2] (NULL: kept; start mode 0 needs them) - plus its clock and start mode, in one launch; no other
 * slot's bytes change.  steps above DS_PANEL_MAX_ROWS, a slot outside [0, ns), a NULL or misaligned buffer fail. */
#define DS_PANEL_MAX_ROWS 1024
int64_t ds_panel_schedule_bytes(int ns);
int ds_panel_slot_load(void* panel, int ns, int slot, int start, int steps, const float* coef_rows, const float* solver_rows,
                       const float* renoise_rows, int start_mode, float init_noise_sigma, void* stream);
/* ds_cfg_sampler_step_redraw_f16 on panel schedules: panel n takes row j of its own coefficient / solver / renoise rows
 * where that call takes row *step_ctr of the shared tables; guidance is always the per-panel vector (needed when do_cfg);
 * kinds 3 and 4 draw their Philox noise for step j, so a panel's noise depends on neither its slot nor when it was admitted.
 * An inactive panel (empty, not yet started, finished) has nothing stored: its latents, prev_x0 and both model_in rows keep
 * their bits.  `redraw` NULL: no blend (every panel plain); given: the x0k | noise | mask parts of the redraw buffer above
 * are read (its header and renoise rows are not), and a plain panel carries an all-ones mask.  step_ctr is required. */
int ds_cfg_sampler_step_slots_f16(const void* eps, void* latents, void* model_in, const void* panel, const float* guidance,
                                  void* prev_x0, const int64_t* seeds, const void* redraw, const int32_t* step_ctr, int ns,
                                  int HW, int kind, int do_cfg, void* stream);
/* ds_timestep_embed_f16 with one timestep per row: row b belongs to panel b % ns (B a multiple of ns) and embeds column 0
 * of that panel's row clamp(j, 0, steps - 1); an empty slot embeds 0.  Always finite. */
int ds_timestep_embed_slots_f16(const void* panel, const int32_t* step_ctr, void* out, int B, int dim, int flip_sin_to_cos,
                                float freq_shift, int ns, void* stream);
/* The state slots [slot0, slot0 + nslots) start from: ds_redraw_start_f16 + ds_prepare_model_input_f16 for those panels
 * alone.  By start mode: 0 latents = fp16(ka0 * x0k + kb0 * noise), {ka0, kb0} = the panel's own renoise row 0; 1 latents =
 * fp16(noise * init_noise_sigma); 2, or `redraw` NULL: the latents are the caller's.  Then model_in = fp16(latents /
 * c_in_div) of the panel's coefficient row 0 into rows n and (do_cfg) ns + n.  Nothing of another slot is written, and
 * nothing of an empty slot (steps = 0) in the range. */
int ds_panel_slot_start_f16(const void* panel, const void* redraw, void* latents, void* model_in, int ns, int HW, int do_cfg,
                            int slot0, int nslots, void* stream);
int ds_nhwc_to_nchw_f16(const void* x, void* y, int B, int HW, int C, void* stream);
int ds_nchw_to_nhwc_f16(const void* x, void* y, int B, int HW, int C, void* stream);
int ds_pad_rows_f16(const void* x, void* y, int B, int rows_in, int rows_out, int row_off, int total_rows, int C,
                    void* stream);
/* tail of `image_processor.postprocess(image, output_type="pil")` (reference src/pipelines/pipeline_diffsensei.py:367;
 * diffusers pt_to_numpy + numpy_to_pil [3P]): image fp32 NCHW [B,3,H,W] in [0,1] -> out uint8 NHWC [B,H,W,3] =
 * (x * 255).round() with numpy's round-half-to-even.  H*W must be a multiple of 4. */
int ds_image_f32_to_u8_nhwc(const float* image, uint8_t* out, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MLLM pre-pass: LLaMA greedy decoding with a KV cache.
 * Replaces, for batch 1, `self.llm.generate(...)` as driven by reference src/models/mllm/seed_x.py:121-136
 * (LlamaForCausalLM of src/models/mllm/modeling_llama_xformer.py:612-, logits processor of
 * src/models/mllm/generation.py:19-30).  All kernels read the step-varying scalars from a device-side state block
 *     int32 state[8] = {rows in the KV cache, tokens generated, finished flag, current token id,
 *                       max_new_tokens of this call, eos token id, spare, spare}
 * so one token step is a static launch list (DS_OP_LLM_* above) that replays as a hipGraph.
 * ---------------------------------------------------------------------------------------------- */
/* y[M,N] = x'[M,K] @ w[N,K]^T (+ residual).  `rms` != 0 puts a LlamaRMSNorm in front of the projection
 * (modeling_llama_xformer.py:77-82 + the q/k/v or gate/up projections :277-296): r_m = rsqrt(mean(x_m^2)+eps) and
 *   rms_gain [K] given:  x'[m][k] = f16(rms_gain[k] * f16(x[m][k] * r_m))   - the reference's rounding points exactly;
 *   rms_gain NULL:       y = r_m * (x @ w^T)                                  - for a caller that folded the gain into w.
 * `swiglu`: w is [2N,K] (gate rows, then up rows) and y = silu(x'.w_gate) * (x'.w_up) (LlamaMLP.forward :166-167).
 * M <= 16 rows per pass internally; HBM-bound weight streaming, one wavefront per output column. */
int ds_llm_gemv_f16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual,
                    int64_t ldr, int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, void* stream);
/* rotary embedding + KV-cache append + attention for M (<= 16) new rows at positions state[0] .. state[0]+M-1
 * (LlamaAttention.forward :192-244: causal inside the prompt chunk, every cached key for a single new token).
 * qkv: [M,(heads+2*kv_heads)*D] un-rotated q|k|v; caches [T_max,kv_heads*D]; rope tables fp32 [T_max,D/2];
 * D in {64,128}.  Does NOT advance state[0] (ds_llm_select_f16 / ds_llm_advance do, once per step). */
int ds_llm_attn_f16(const void* qkv, int64_t ldqkv, void* k_cache, void* v_cache, int64_t ldc, const float* rope_cos,
                    const float* rope_sin, void* out, int64_t ldo, const int32_t* state, int M, int heads,
                    int kv_heads, int D, int T_max, float scale, void* stream);
/* LlamaRMSNorm with its gain (the final `model.norm`, :595).  `feat` (may be NULL; M == 1): the row is also stored as
 * row state[1]-1 of a [max_out,H] buffer - the per-token hidden states seed_x.py:143 gathers. */
int ds_llm_rmsnorm_f16(const void* x, int64_t ldx, const void* gamma, void* y, int64_t ldy, void* feat,
                       const int32_t* state, int M, int H, int max_out, float eps, void* stream);
/* out[0,:] = embed_tokens[state[3]] */
int ds_llm_embed_f16(const void* table, const int32_t* state, void* out, int H, int vocab, void* stream);
/* greedy choice with AutoImageTokenGenerationProcessor (generation.py:19-30) folded in; chain = [<img>, <img_0> ..
 * <img_{n-1}>, </img>] (n_chain ids, 0 = no processor).  Appends to out_ids[state[1]++] (capacity out_cap), sets
 * state[3], adds `adv` to state[0], raises state[2] on the eos id (state[5]) or after state[4] ids.  A no-op once
 * state[2] is set. */
int ds_llm_select_f16(const void* logits, int V, const int32_t* chain, int n_chain, int out_cap, int adv,
                      int32_t* state, int32_t* out_ids, void* stream);
int ds_llm_advance(int32_t* state, int rows, void* stream); /* state[0] += rows (prompt chunks before the last) */
/* out = a*scale + b*(1-scale), n elements (multiple of 8): `img_gen_feat * mllm_scale + image_embeds * (1 - mllm_scale)`
 * (reference scripts/demo/gradio.py:108-109) */
int ds_blend_f16(const void* a, const void* b, void* out, int64_t n, float scale, void* stream);
/* act[M,I] = silu(gate_up[:, :I]) * gate_up[:, I:] - the prompt pass, where gate|up comes out of ds_gemm_f16 as [M,2I]
 * (LlamaMLP.forward, modeling_llama_xformer.py:166-167) */
int ds_llm_swiglu_f16(const void* gate_up, void* act, int M, int I, void* stream);

/* Batched decode: up to 16 sequences share one pass over the weights.  The state block becomes int32 [S][8], one row
 * per sequence slot with the eight fields above; every slot has its own KV cache ([S][T_max][kv_heads*D] per layer),
 * feature buffer ([S][max_out][H]) and id list ([S][out_cap]).  A slot whose finished flag is set (a sequence that
 * ended, or a slot that was never started: the host sets the flag) has nothing written to its cache, ids, features or
 * counters; its rows of the projections still compute (finite, unused) values. */
/* ds_llm_gemv_f16 for M <= 16 on the matrix pipe (llm_gemm16_kernel: v_mfma_f32_16x16x32_f16, x = A padded to 16
 * rows, 16 weight rows = B, weights streamed HBM -> VGPR once for all rows).  Same prologues, epilogues and fp16
 * rounding points; any N, K % 8 == 0 (with rms_gain: K <= 20480).  A row of y depends on that row of x only - not on M,
 * on the other rows or on the padding - and the K split inside a block is reduced in a fixed order (no atomics). */
int ds_llm_gemm16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                  int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, void* stream);
/* int8 weight-only decoding (W8A16): ds_llm_gemv_f16 / ds_llm_gemm16 with w as int8 [N,K] (two's complement, row-major;
 * SwiGLU [2N,K]) and w_scale fp32 [N] (SwiGLU [2N]: gate scales, then up scales), one scale per weight row:
 *   y[m][n] = f16( (sum_k x'[m][k] q[n][k]) * r_m * w_scale[n] )  - the int8 -> f16 unpack is exact, the sum is fp32, the
 * scale is applied in fp32 before the one fp16 rounding; every other rounding point is that of the fp16 form.
 * K % 16 == 0 (a 16-byte load holds 16 weights).  ds_llm_gemv_w8 runs llm_gemv_pipe_kernel (M <= 4) or llm_gemv_kernel;
 * with the option "llm_gemv_variant" = 2 it fails (that kernel has no int8 form). */
int ds_llm_gemv_w8(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                   int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, const float* w_scale,
                   void* stream);
int ds_llm_gemm16_w8(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                     int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, const float* w_scale,
                     void* stream);
/* w16[n][k] = f16(f32(q[n][k]) * w_scale[n]) for q int8 [N,K], K % 16 == 0 (one fp32 multiply, one round to nearest even):
 * the prompt pass hands the result to ds_gemm_f16 */
int ds_llm_dequant_w8(const void* q, const float* w_scale, void* w16, int64_t N, int K, void* stream);
/* MXFP4 weight-only decoding (W4A16): the _w8 entry points with w in the OCP MX fp4 format plus one fp32 scale per row.
 *   w        uint8 [N,K/2] row-major (SwiGLU [2N,K/2]): two e2m1 elements per byte (sign + 3 bits, values +-{0, 0.5, 1, 1.5, 2,
 *            3, 4, 6}), element 2i in the low nibble, element 2i+1 in the high nibble
 *   w_exp    uint8 [N,K/32] row-major (SwiGLU [2N,K/32]): one biased E8M0 exponent per block of 32 elements along K,
 *            block scale = 2^(w_exp - 127); the quantiser stores 114..127 (exponents -13..0), so every e2m1 * block scale is a
 *            normal f16 number and the in-register conversion (v_cvt_scalef32_pk_f16_fp4) is exact
 *   w_scale  fp32 [N] (SwiGLU [2N]): one scale per weight row
 *   weight[n][k] = e2m1(w[n][k]) * 2^(w_exp[n][k/32] - 127) * w_scale[n]
 *   y[m][n] = f16( (sum_k x'[m][k] * f16(e2m1 * 2^(w_exp-127))) * r_m * w_scale[n] )  - fp32 sum, the row scale in fp32 before
 * the one fp16 rounding; every other rounding point is that of the fp16 form.  K % 32 == 0 (a 16-byte load is one block).
 * ds_llm_gemv_fp4 runs llm_gemv_pipe_kernel (M <= 4) or llm_gemv_kernel; with the option "llm_gemv_variant" = 2 it fails
 * (that kernel has no MXFP4 form).  Both w_scale and w_exp are required.  No parity figure exists for a trained checkpoint. */
int ds_llm_gemv_fp4(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                    int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, const float* w_scale,
                    const uint8_t* w_exp, void* stream);
int ds_llm_gemm16_fp4(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, const void* residual, int64_t ldr,
                      int M, int N, int K, int rms, const void* rms_gain, int swiglu, float eps, const float* w_scale,
                      const uint8_t* w_exp, void* stream);
/* w16[n][k] = f16(f32(e2m1 * 2^(w_exp - 127)) * w_scale[n]) for an MXFP4 matrix (one fp32 multiply, one round to nearest even):
 * the prompt pass hands the result to ds_gemm_f16 */
int ds_llm_dequant_fp4(const void* q, const float* w_scale, void* w16, int64_t N, int K, const uint8_t* w_exp, void* stream);
/* The slot forms of ds_llm_attn_f16 / _rmsnorm_ / _embed_ / _select_: the same four kernels with every row a sequence of
 * its own (state row s of an int32 [S][8] block) instead of the next position of one sequence.  The attention, the feature
 * tap and the pick leave a slot with state[s][2] set (finished, or never started) alone.
 * ds_llm_attn_f16 for one new row per slot: row s of qkv / out belongs to slot s, its caches start slot_stride
 * elements after slot s-1's, its position is state[s][0]. */
int ds_llm_attn_slots_f16(const void* qkv, int64_t ldqkv, void* k_cache, void* v_cache, int64_t ldc, int64_t slot_stride,
                          const float* rope_cos, const float* rope_sin, void* out, int64_t ldo, const int32_t* state,
                          int slots, int heads, int kv_heads, int D, int T_max, float scale, void* stream);
/* FP8 KV cache: ds_llm_attn_f16 / ds_llm_attn_slots_f16 on a cache of OCP e4m3 codes with one power-of-two exponent per
 * (row, kv head).  For every cache row and kv head the D values are stored as
 *   k_cache / v_cache  uint8 [T_max, kv_heads*D] rows (ldc BYTES; slot form: slot_stride BYTES between two slots): D e4m3fn
 *                      codes (largest finite 448, subnormals down to 2^-9)
 *   k_exp / v_exp      uint8 [T_max, kv_heads] rows (lde; slot form: exp_slot_stride between two slots): e = ex + 127 with ex
 *                      the smallest integer such that amax / 2^ex <= 448, amax the head's largest fp16 magnitude (ex = 0 for an
 *                      all-zero head; for fp16 input ex lies in [-33, 8])
 *   value = f32(e4m3) * 2^(e - 127); x / 2^ex is exact, the one rounding is fp32 -> e4m3 to nearest even, nothing saturates.
 * K is quantised after the rotation and its rounding to fp16, V as it is.  Scores, softmax and P.V as in the fp16 form (fp32
 * accumulation, probabilities rounded to fp16): score_j = dot(q, f32(k8_j)) * 2^exk_j * scale, P.V term = (p_j * 2^exv_j) *
 * f32(v8_j).  Every key and value - the chunk's own rows and the row's own key included - is seen through the quantiser, so the
 * result is attention over the dequantised cache and does not depend on how the rows were cut into launches.  The guards of the
 * fp16 form hold for codes and exponent bytes alike.  ldc % 8 == 0, 8-byte aligned caches.  A quantised mode with its own error
 * (2.6 % relative rms on Gaussian heads); no parity figure exists for a trained checkpoint. */
int ds_llm_attn_kv8(const void* qkv, int64_t ldqkv, void* k_cache, void* v_cache, int64_t ldc, void* k_exp, void* v_exp,
                    int64_t lde, const float* rope_cos, const float* rope_sin, void* out, int64_t ldo, const int32_t* state,
                    int M, int heads, int kv_heads, int D, int T_max, float scale, void* stream);
int ds_llm_attn_slots_kv8(const void* qkv, int64_t ldqkv, void* k_cache, void* v_cache, int64_t ldc, int64_t slot_stride,
                          void* k_exp, void* v_exp, int64_t lde, int64_t exp_slot_stride, const float* rope_cos,
                          const float* rope_sin, void* out, int64_t ldo, const int32_t* state, int slots, int heads,
                          int kv_heads, int D, int T_max, float scale, void* stream);
/* row s normalised as ds_llm_rmsnorm_f16 does; `feat` (may be NULL): also stored as row state[s][1]-1 of feat[s] */
int ds_llm_rmsnorm_slots_f16(const void* x, int64_t ldx, const void* gamma, void* y, int64_t ldy, void* feat,
                             const int32_t* state, int slots, int H, int max_out, float eps, void* stream);
/* out[s,:] = embed_tokens[state[s][3]] */
int ds_llm_embed_slots_f16(const void* table, const int32_t* state, void* out, int64_t ldo, int slots, int H, int vocab,
                           void* stream);
/* ds_llm_select_f16 per slot: logits row s (stride ldl), state row s (with its own eos and max_new), out_ids[s] */
int ds_llm_select_slots_f16(const void* logits, int64_t ldl, int V, const int32_t* chain, int n_chain, int out_cap, int adv,
                            int32_t* state, int32_t* out_ids, int slots, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Character-reference pre-processing on the device.  Replaces the Pillow resize that
 * `CLIPImageProcessor()` / `ViTImageProcessor()` run on the host (reference src/pipelines/pipeline_diffsensei.py:125-126)
 * bit for bit: 8-bit separable resample with 22-bit fixed-point taps (libImaging Resample.c), horizontal pass, 8-bit
 * intermediate, vertical pass; then centre crop, * rescale, (x - mean) / std, CHW fp32.
 * Tables (device int32, built once per (in, out, filter) by the host with Pillow's double arithmetic):
 *   first[o] = first source index of output o, count[o] = taps used, taps[o*ksize + k] = round(w * 2^22).
 * Images: RGB uint8, HWC, device.  mean3 / std3: HOST arrays of 3 floats.
 * ---------------------------------------------------------------------------------------------- */
/* dst[H,out_w,3] = horizontal pass of src[H,W,3] */
int ds_resize_h_u8(const uint8_t* src, int H, int W, const int32_t* first, const int32_t* count, const int32_t* taps,
                   int ksize, int out_w, uint8_t* dst, void* stream);
/* vertical pass of tmp[Ht,Wt,3] restricted to the crop window rows [top, top+out_h) x columns [left, left+out_w),
 * then out_f32[3,out_h,out_w] = (u8 * scale - mean) / std; out_u8 (may be NULL) receives the cropped bytes [out_h,out_w,3] */
int ds_resize_v_norm_u8(const uint8_t* tmp, int Ht, int Wt, const int32_t* first, const int32_t* count,
                        const int32_t* taps, int ksize, int top, int left, int out_h, int out_w, float scale,
                        const float* mean3, const float* std3, float* out_f32, uint8_t* out_u8, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Plans: a static launch list (one UNet forward, or forward + CFG + scheduler step) built once by the host
 * and replayed with zero host arithmetic — optionally as a captured hipGraph.
 * ---------------------------------------------------------------------------------------------- */
enum ds_opcode {
    DS_OP_GEMM = 1,          /* p: x, x2, w, y, bias, rowbias, residual, ln_stats, ln_c, stats_out (fused LayerNorm, see ds_gemm_ln_f16; i[8] = operand-swapped form, l[10] = ln_bstride; i[9] = ln_stats holds PARTIAL sums, f[0] = eps, l[11] = ln_rows: ds_gemm_ln_partial_f16 / ds_gemm_ln_swapped_partial_f16)   l: ldx ldx2 ldw ldy ldr sx sx2 sw sy sr
                                i: M N K K1 epilogue (0 none, 1 GEGLU in 128-row groups, 2 GELU, 3 QuickGELU, 4 GEGLU in 320-row groups: ds_gemm_g320_fits)
                                batch rowbias_ld rows_per_group; i[10] = strips a consumer of partial sums adds per
                                row (0 = K / 64), i[11] = statistics format a producer emits (0 = one entry per 64 columns; 160: ds_gemm_t160_fits;
                                the launch fails if the kernel it picks does not emit that format, e.g. 160 off gemm_t160_kernel) */
    DS_OP_CONV3X3 = 2,       /* p: x, w, y, bias, rowbias, residual, gn_partial (optional: GroupNorm workspace, see ds_conv3x3_gn_chunks)
                                i: B H W Cin Cout stride upsample rowbias_ld Hout Wout (upsample only; 0 0 = 2H x 2W);
                                   upsample == 2: exact x2 with the folded weights of ds_fold_upsample2x_f16 in p[1];
                                i[10] = GroupNorm partial-sum chunks per image the plan expects (with p[6]: ds_conv3x3_gn_chunks at plan
                                time, the GROUPNORM op's i[6]); the launch fails unless the kernel it picks writes exactly that many.
                                0 = no count stated: the launch writes what its kernel writes (the caller asked ds_conv3x3_gn_chunks
                                on the launching thread); a launch plan always states it */
    DS_OP_GROUPNORM = 3,     /* p: x1, x2, y, gamma, beta, ws             i: B HW C1 C2 groups silu pre_chunks (0, or the number of
                                partial-sum chunks per image the producing convolution left in ws)   f: eps */
    DS_OP_LAYERNORM = 4,     /* p: x, y, gamma, beta                      i: rows C                   f: eps */
    DS_OP_SELF_ATTN = 5,     /* p: q, k, vt, o   l: ldq ldk ldv ldo sq sk so   i: B heads Nq Nk       f: scale */
    DS_OP_IP_ATTN = 6,       /* p: q, kt, vtt, ki, vti, bbox, o, ip_scale_dev   l: ldq ldo ldk sk sv
                                i: B heads N Lt Li n_dummy tok_per_ip max_ips mask_h mask_w; i[10] = 1: ip_scale_dev is a
                                   [B] vector, one scale per batch row (ds_masked_ip_attn_rows_f16); 0: one device scalar
                                   i[11] = T > 1: long prompt (ds_masked_ip_attn_long_f16) - kt / vtt are T panels of 96 rows
                                   with the strides l[5] ldkt, l[6] skt, l[7] svt; 0 or 1: one text panel sharing ldk sk sv
                                f: qk_scale ip_scale */
    DS_OP_CONV_IN = 7,       /* p: x, w, bias, boxes, demb, y             i: B H W Cin Cout ndialog */
    DS_OP_CONV_OUT = 8,      /* p: x, w, bias, y                          i: B H W Cin Cout */
    DS_OP_SKINNY = 9,        /* p: x, w, bias, addend, y                  i: M N K silu_in silu_out */
    DS_OP_TIMESTEP_EMBED = 10, /* p: table, ctr, out                      i: B dim flip               f: freq_shift
                                  i[3] = ns > 0: panel schedules - p[0] is the panel-schedule buffer, row b reads panel b % ns
                                  (ds_timestep_embed_slots_f16) */
    DS_OP_ADD_TIME_IDS = 11, /* p: text_embeds, time_ids, out             i: B pooled n_ids dim flip  f: freq_shift */
    DS_OP_SAMPLER_STEP = 12, /* p: eps, latents, model_in, table, ctr, prev_x0 (kind 2), solver (kinds 2 and 4),
                                   seeds (kinds 3 and 4), guidance (p[8]: fp32 [ns], one per panel; NULL = column 7 of the table)
                                   p[9]: the region-redraw buffer (ds_cfg_sampler_step_redraw_f16), read when i[4] = 1
                                i: ns HW kind (0 Euler, 1 DDIM, 2 DPM-Solver++, 3 Euler Ancestral, 4 LCM) do_cfg redraw (i[4]: 0 | 1;
                                   1 without p[9] fails the launch)
                                   i[5] = 1: panel schedules (ds_cfg_sampler_step_slots_f16) - p[3] is the panel-schedule buffer in
                                   the table's place, p[6] is not read (the solver rows live in the buffer), p[8] is required */
    DS_OP_PREP_INPUT = 13,   /* p: latents, model_in, table, ctr          i: ns HW do_cfg */
    DS_OP_ADVANCE = 14,      /* p: ctr */
    DS_OP_NHWC2NCHW = 15,    /* p: x, y                                   i: B HW C */
    DS_OP_NCHW2NHWC = 16,    /* p: x, y                                   i: B HW C */
    DS_OP_PAD_ROWS = 17,     /* p: x, y                                   i: B rows_in rows_out row_off total_rows C */
    DS_OP_SMALL_ATTN = 18,   /* p: q, k, v, o   l: ldq ldk ldv ldo sq sk sv so   i: B heads Nq Nk D   f: scale */
    DS_OP_LLM_GEMV = 19,     /* p: x, w, y, residual, rms_gain   l: ldx ldy ldr   i: M N K rms swiglu  f: eps */
    DS_OP_LLM_ATTN = 20,     /* p: qkv, k_cache, v_cache, rope_cos, rope_sin, out, state   l: ldqkv ldc ldo
                                i: M heads kv_heads D T_max                                           f: scale */
    DS_OP_LLM_RMSNORM = 21,  /* p: x, gamma, y, feat, state l: ldx ldy       i: M H max_out           f: eps */
    DS_OP_LLM_EMBED = 22,    /* p: table, state, out                         i: H vocab */
    DS_OP_LLM_SELECT = 23,   /* p: logits, chain, state, out_ids             i: V n_chain out_cap adv pause
                                pause (i[4]; 0 | 1, chain fast-forward): 1 = a sequence that did not finish and whose new id lies in
                                chain[:-1] gets state[2] = 2 - every per-slot kernel then leaves it alone until the host has decoded
                                the forced ids in one pass and rewritten the state row; 0 = the pick as it always was */
    DS_OP_LLM_ADVANCE = 24,  /* p: state                                     i: rows */
    /* 25, 26: retired (fp8 attention, rounds 2-5) */
    DS_OP_LN_FINALIZE = 27,  /* p: partial, stats                            i: M strips C               f: eps */
    DS_OP_LLM_GEMM16 = 28,   /* as DS_OP_LLM_GEMV, M <= 16, on the matrix pipe (ds_llm_gemm16) */
    DS_OP_LLM_ATTN_SLOTS = 29,    /* as DS_OP_LLM_ATTN with i[0] = slots and l[3] = slot_stride (ds_llm_attn_slots_f16) */
    DS_OP_LLM_RMSNORM_SLOTS = 30, /* p: x, gamma, y, feat, state l: ldx ldy     i: slots H max_out       f: eps */
    DS_OP_LLM_EMBED_SLOTS = 31,   /* p: table, state, out        l: ldo         i: slots H vocab */
    DS_OP_LLM_SELECT_SLOTS = 32,  /* p: logits, chain, state, out_ids  l: ldl   i: V n_chain out_cap adv slots pause (i[5], as i[4]
                                     of DS_OP_LLM_SELECT) */
    DS_OP_REDRAW_START = 33,      /* p: redraw buffer, latents                  i: ns HW   (ds_redraw_start_f16) */
    DS_OP_LLM_GEMV_W8 = 34,       /* DS_OP_LLM_GEMV with int8 weights in p[1] and p[5] = w_scale (ds_llm_gemv_w8) */
    DS_OP_LLM_GEMM16_W8 = 35,     /* DS_OP_LLM_GEMM16 with int8 weights in p[1] and p[5] = w_scale (ds_llm_gemm16_w8) */
    DS_OP_LORA_MERGE = 36,        /* p: W, out, A, B, seg, s, map, colscale, out2   l: ldw ldo lda ldb ldo2   i: N K R nseg cin
                                     i[4] = cin > 0: convolution mode - W is a 3x3 weight in checkpoint order [N][cin][3][3] (contiguous,
                                     ldw = K = 9 cin) while out and A are in the packed tap-major order k = (ky*3 + kx)*cin + ci, so
                                     nseg = 0 gives the packed base; cin a multiple of 8.  cin = 0, a plain matrix:
                                     out[n,k] = f16(f32(W[map(n),k]) + sum_i s[i] * sum_{r in [seg[i], seg[i+1])} B[map(n),r] A[r,k]):
                                     W [N,K] f16 is the base weight, read only - the launch fails when it is out or out2; A [R,K]
                                     and B [N,R] f16 hold the adapters concatenated along the rank (any rank, any boundary; nseg <= 16, empty segments legal);
                                     seg int32 [nseg+1] and s fp32 [nseg] are DEVICE arrays, so a plan is replayed with new
                                     strengths after a host write; nseg = 0 copies W.  Each adapter is accumulated in fp32, scaled in
                                     fp32, added in order, rounded once.  map (optional int32 [N]) permutes the rows of W and B alike;
                                     out2 (optional, with colscale f16 [K]) = f16(f32(out) * f32(colscale[k])), the fused-LayerNorm
                                     copy.  N, K multiples of 8; ldw, ldo, lda, ldo2 multiples of 8; no exported entry point */
    DS_OP_SLOT_START = 37,        /* p: panel-schedule buffer, redraw buffer (or NULL), latents, model_in
                                     i: ns HW do_cfg slot0 nslots   (ds_panel_slot_start_f16) */
    DS_OP_LLM_GEMV_FP4 = 38,      /* DS_OP_LLM_GEMV with MXFP4 weights in p[1], p[5] = w_scale, p[6] = w_exp (ds_llm_gemv_fp4) */
    DS_OP_LLM_GEMM16_FP4 = 39,    /* DS_OP_LLM_GEMM16 with MXFP4 weights in p[1], p[5] = w_scale, p[6] = w_exp (ds_llm_gemm16_fp4) */
    DS_OP_LLM_ATTN_KV8 = 40,      /* DS_OP_LLM_ATTN on the fp8 cache: p[1], p[2] = uint8 e4m3 caches (l[1] = ldc in bytes), p[7] = k_exp,
                                     p[8] = v_exp, l[4] = lde (ds_llm_attn_kv8) */
    DS_OP_LLM_ATTN_SLOTS_KV8 = 41, /* DS_OP_LLM_ATTN_SLOTS likewise: l[3] = slot_stride in bytes, p[7] = k_exp, p[8] = v_exp, l[4] = lde,
                                     l[5] = exp_slot_stride (ds_llm_attn_slots_kv8) */
    DS_OP_LLM_ATTN_ROWS = 42,     /* ragged attention over the rows of several slots in one launch (llm_attn_rows_kernel; the chain
                                     fast-forward pass): p, l, f as DS_OP_LLM_ATTN_SLOTS plus p[9] = row table, device int32 [rows][2] =
                                     (slot, row r inside the slot's segment); i: rows heads kv_heads D T_max slots.  A segment is a
                                     run of consecutive rows of qkv / out with r = 0, 1, ..; it may be longer than 16 rows.  Row r sits
                                     at position state[slot][0] + r, sees the slot's cache below state[slot][0] and the segment's rows
                                     up to itself, and appends its K and V; state[slot][2] is not looked at, the state is not
                                     written, nothing is written at or past T_max, a table entry with slot outside [0, slots) or r
                                     outside [0, row] is skipped.  No exported entry point */
    DS_OP_LLM_ATTN_ROWS_KV8 = 43  /* DS_OP_LLM_ATTN_ROWS on the fp8 cache: operands as DS_OP_LLM_ATTN_SLOTS_KV8 plus p[9] and i[5] */
};

typedef struct ds_op {
    int32_t code;
    int32_t i[16];
    float f[4];
    int64_t l[12];
    void* p[10];
} ds_op;

typedef struct ds_plan ds_plan;
int ds_op_run(const ds_op* op, void* stream); /* run one op immediately */
/* roofline accounting: kernel the op's launch runs under the calling thread's options (rocprofv3 spelling), algorithmic flops
 * (2*MAC) and HBM bytes.  A GEMM / CONV3X3 op that no kernel serves (ds_op_run of it fails) is named "refused"; the call still
 * returns 0 with the op's flops and bytes. */
int ds_op_describe(const ds_op* op, char* name, int name_len, double* flops, double* bytes);
int ds_plan_create(const ds_op* ops, int n_ops, ds_plan** out);
int ds_plan_num_ops(const ds_plan* plan);
int ds_plan_run(ds_plan* plan, void* stream);            /* eager: one launch per op */
int ds_plan_capture(ds_plan* plan, void* stream);        /* capture the launch list into a hipGraph (once) */
int ds_plan_replay(ds_plan* plan, void* stream);         /* hipGraphLaunch of the captured graph */
int ds_plan_destroy(ds_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSENSEI_HIP_H */
