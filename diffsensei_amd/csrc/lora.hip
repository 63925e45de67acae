// LoRA merge: a packed weight buffer rewritten in place of a re-pack.
//
//   out[n, k]  = f16( f32(W[map(n), k]) + sum_i s_i * ( sum_{r in seg_i} B[map(n), r] * A[r, k] ) )
//   out2[n, k] = f16( f32(out[n, k]) * f32(colscale[k]) )                                   (optional)
//
// W is the untouched base weight (never the buffer being written), A [R, K] / B [N, R] are the active adapters concatenated
// along the rank, seg (int32 [nseg + 1]) and s (fp32 [nseg]) live on the device, so a captured or cached plan is replayed with
// new strengths after one small host write - the idiom of the per-step table.  Each adapter is accumulated in fp32 on the
// matrix pipe, scaled in fp32, the adapters are added in order onto f32(W), and the sum is rounded to f16 once.  A segment
// that is empty or has strength exactly 0 adds nothing, so nseg = 0 and s = [0] both give the bits of W.
//
// out2 is the gamma (.) W' copy of the fused LayerNorms (engine.pack_ln_fused): both factors are f16 values, their product has
// at most 22 significant bits and is exact in fp32, so the one rounding below gives the bits of the double-precision host
// path applied to the kernel's own `out`.
//
// The op is HBM-bound (W in, out and out2 out; A and B are re-read out of L2), so the shape is chosen for the stores, not the
// MFMA rate.  One block = 64 rows x 64 columns, one wave = 16 rows x 64 columns = whole 128-byte lines of W / out in
// 16-byte accesses.  v_mfma_f32_16x16x32_f16 leaves lane l with D[4 (l >> 4) + reg][l & 15]: the MFMA's row index is made the
// output COLUMN k and its column index the output row n, and the four 16-column tiles of a wave interleave their rows
// (tile t, MFMA row 4 q + j  ->  column 32 (t >> 1) + 8 q + 4 (t & 1) + j) so that lane l ends up with 8 consecutive columns
// 8 (l >> 4) .. + 8 of each 32-column half of row l & 15.
//   A operand: lane l holds At[column(t, l & 15)][8 (l >> 4) .. + 8]   (A staged TRANSPOSED in LDS, [k][r])
//   B operand: lane l holds Bt[row l & 15][8 (l >> 4) .. + 8]          (B staged as it lies, [n][r])
// Ranks and segment boundaries are arbitrary: a 32-rank step that crosses the end of its segment is padded with zeros as it
// is staged, and B - whose rows are R elements long, any R - is read in 16-byte pieces where a piece lies inside its segment
// and is aligned (R and the segment start multiples of 8: the usual ranks), element by element otherwise, never past its end.
// W, out, out2 and A move in 16-byte accesses throughout; the transposed staging of A writes single halves to LDS (4-way bank
// conflicts at this pitch), which the global traffic hides.
// No atomics: every output element is written by one lane.
//
// Convolution mode (cin > 0): W is a 3x3 weight as the checkpoint has it, [N][Cin][3][3], and out / A / K are in the packed
// tap-major order of engine.pack_conv3x3, k = (ky * 3 + kx) * Cin + ci, K = 9 Cin:
//   out[n, tap * Cin + ci] = f16( f32(W[n][ci][tap]) + sum_i s_i * (B_i A_i)[n, tap * Cin + ci] )
// Only the read of W differs: Cin is a multiple of 8, so an 8-column piece never straddles a tap (a 64-column tile may, when
// Cin < 64: tap and channel are found per piece), and the piece is 8 halves 18 bytes apart.  The nine tap tiles of one
// (row block, channel range) read the same lines of W, eight of the nine times out of L2; the stores stay whole 16-byte
// pieces.  No adapter gives the bits of pack_conv3x3(W): the base of the state dict is the only base there is.
#include "ds_common.h"
#include "ds_kernels.h"

#define LM_TILE 64  // rows and columns per block
#define LM_RC 32    // ranks per MFMA
#define LM_LD 40    // LDS row pitch in halves: 80 bytes keeps 16-byte alignment off the 64-byte power of two

// One launch serves up to DS_LORA_GROUP matrices (a merge plan has hundreds of them, most a few hundred tiles large: launched
// one by one they run one after the other, each too small to fill the chip).  The group travels by value in the kernel
// arguments; a block finds its matrix by its tile number.
struct LoraMergeGroup {
    LoraMergeParams e[DS_LORA_GROUP];
    int tile_start[DS_LORA_GROUP + 1];   // first tile of each matrix in the 1-D grid; [count] = all tiles
    int count;
};

__global__ __launch_bounds__(256) void lora_merge_kernel(LoraMergeGroup grp) {
    __shared__ __attribute__((aligned(16))) half_t At[LM_TILE * LM_LD];
    __shared__ __attribute__((aligned(16))) half_t Bt[LM_TILE * LM_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int which = 0;
    for (int e = 1; e < grp.count; ++e) which = (int)blockIdx.x >= grp.tile_start[e] ? e : which;   // uniform over the block
    const LoraMergeParams p = grp.e[which];
    const int tile = (int)blockIdx.x - grp.tile_start[which];
    const int tiles_n = (p.N + LM_TILE - 1) / LM_TILE;
    const int n0 = (tile % tiles_n) * LM_TILE, k0 = (tile / tiles_n) * LM_TILE;
    const int g = lane >> 4, m = lane & 15;
    const int n = n0 + wave * 16 + m;
    const bool n_ok = n < p.N;
    const long src = n_ok ? (p.map ? (long)p.map[n] : (long)n) : 0;

    // f32(W) first: the loads are in flight while the adapters are staged
    float tot[2][8];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const int kk = k0 + 32 * hh + 8 * g;
        h8 w = {0, 0, 0, 0, 0, 0, 0, 0};
        if (n_ok && kk < p.K) {
            if (p.cin > 0) {   // checkpoint order [ci][tap]: 8 channels of one tap, 18 bytes apart; the other taps' blocks hit the same lines in L2
                const int tap = kk / p.cin, ci = kk - tap * p.cin;
                const half_t* wr = p.W + src * p.ldw + (long)ci * 9 + tap;
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = wr[9 * j];
            } else {
                w = *reinterpret_cast<const h8*>(p.W + src * p.ldw + kk);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) tot[hh][j] = (float)w[j];
    }

    // staging roles: A - rank tid >> 3 of the step, 8 columns; B - row tid >> 2 of the block, 8 ranks
    const int a_r = tid >> 3, a_c = (tid & 7) * 8;
    const int b_n = tid >> 2, b_q = (tid & 3) * 8;
    const bool b_ok = n0 + b_n < p.N;
    const long b_src = b_ok ? (p.map ? (long)p.map[n0 + b_n] : (long)(n0 + b_n)) : 0;
    const bool b_vec = (((uintptr_t)p.B & 15) | (p.ldb & 7)) == 0;   // rows of B start 16-byte aligned: whole 8-rank pieces in one load

    for (int i = 0; i < p.nseg; ++i) {
        const int beg = max(p.seg[i], 0), end = min(p.seg[i + 1], p.R);
        const float sc = p.s[i];
        if (end <= beg || sc == 0.0f) continue;   // uniform over the block
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4{0, 0, 0, 0};
        for (int r0 = beg; r0 < end; r0 += LM_RC) {
            __syncthreads();
            {
                h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                const int r = r0 + a_r;
                if (r < end && k0 + a_c < p.K) v = *reinterpret_cast<const h8*>(p.A + (long)r * p.lda + k0 + a_c);
#pragma unroll
                for (int j = 0; j < 8; ++j) At[(a_c + j) * LM_LD + a_r] = v[j];
            }
            {
                h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (b_ok) {
                    const half_t* row = p.B + b_src * p.ldb;
                    const int rb = r0 + b_q;
                    if (b_vec && (rb & 7) == 0 && rb + 8 <= end) {
                        v = *reinterpret_cast<const h8*>(row + rb);
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (rb + j < end) v[j] = row[rb + j];
                    }
                }
                *reinterpret_cast<h8*>(&Bt[b_n * LM_LD + b_q]) = v;
            }
            __syncthreads();
            const h8 bf = *reinterpret_cast<const h8*>(&Bt[(wave * 16 + m) * LM_LD + 8 * g]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = 32 * (t >> 1) + 8 * (m >> 2) + 4 * (t & 1) + (m & 3);
                const h8 af = *reinterpret_cast<const h8*>(&At[col * LM_LD + 8 * g]);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) tot[t >> 1][4 * (t & 1) + j] += sc * acc[t][j];
    }

#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const int kk = k0 + 32 * hh + 8 * g;
        if (!n_ok || kk >= p.K) continue;
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)tot[hh][j];
        *reinterpret_cast<h8*>(p.out + (long)n * p.ldo + kk) = o;
        if (p.out2) {
            const h8 cs = *reinterpret_cast<const h8*>(p.colscale + kk);
            h8 o2;
#pragma unroll
            for (int j = 0; j < 8; ++j) o2[j] = (half_t)((float)o[j] * (float)cs[j]);   // exact product, one rounding
            *reinterpret_cast<h8*>(p.out2 + (long)n * p.ldo2 + kk) = o2;
        }
    }
}

static int lora_merge_check(const LoraMergeParams& p) {
    DS_REQUIRE(p.W && p.out, "lora_merge: W and out are needed");
    DS_REQUIRE(p.N > 0 && p.K > 0 && p.N % 8 == 0 && p.K % 8 == 0, "lora_merge: N (%d) and K (%d) must be positive multiples of 8",
               p.N, p.K);
    DS_REQUIRE(p.nseg >= 0 && p.nseg <= DS_LORA_MAX_SEGMENTS, "lora_merge: %d segments (at most %d)", p.nseg, DS_LORA_MAX_SEGMENTS);
    DS_REQUIRE(p.R >= 0, "lora_merge: negative rank total");
    DS_REQUIRE(p.nseg == 0 || (p.A && p.B && p.seg && p.s && p.R > 0), "lora_merge: adapters need A, B, seg, s and R > 0");
    DS_REQUIRE(p.cin == 0 || (p.cin > 0 && p.cin % 8 == 0 && p.K == 9 * p.cin && p.ldw == (long)p.K),
               "lora_merge: convolution mode needs Cin (%d) a positive multiple of 8, K (%d) = 9 Cin and a contiguous base", p.cin, p.K);
    DS_REQUIRE((const void*)p.W != (const void*)p.out &&(const void*)p.W != (const void*)p.out2,
               "lora_merge: the base weight W is read only and must not be an output (merge from the base, not in place)");
    DS_REQUIRE((p.out2 != nullptr) == (p.colscale != nullptr), "lora_merge: out2 and colscale come together");
    DS_REQUIRE(p.out2 != p.out, "lora_merge: out2 must not be out");
    DS_REQUIRE(p.ldw >= p.K && p.ldo >= p.K && p.ldw % 8 == 0 && p.ldo % 8 == 0, "lora_merge: ldw / ldo must be multiples of 8, >= K");
    DS_REQUIRE(!p.out2 || (p.ldo2 >= p.K && p.ldo2 % 8 == 0), "lora_merge: ldo2 must be a multiple of 8, >= K");
    DS_REQUIRE(p.nseg == 0 || (p.lda >= p.K && p.lda % 8 == 0 && p.ldb >= p.R), "lora_merge: lda (multiple of 8, >= K) / ldb (>= R)");
    DS_REQUIRE((((uintptr_t)p.W | (uintptr_t)p.out | (uintptr_t)p.out2 | (uintptr_t)p.A | (uintptr_t)p.colscale) & 15) == 0,
               "lora_merge: W, out, out2, A and colscale must be 16-byte aligned");
    DS_REQUIRE((((uintptr_t)p.seg | (uintptr_t)p.s | (uintptr_t)p.map) & 3) == 0 && ((uintptr_t)p.B & 1) == 0,
               "lora_merge: misaligned seg / s / map / B");
    return 0;
}

int ds_launch_lora_merge_group(const LoraMergeParams* ps, int count, hipStream_t stream) {
    DS_REQUIRE(ps && count >= 1 && count <= DS_LORA_GROUP, "lora_merge: a group holds 1..%d matrices, got %d", DS_LORA_GROUP, count);
    LoraMergeGroup grp;
    long tiles = 0;
    for (int e = 0; e < count; ++e) {
        const int rc = lora_merge_check(ps[e]);
        if (rc != 0) return rc;
        grp.e[e] = ps[e];
        grp.tile_start[e] = (int)tiles;
        tiles += (long)((ps[e].N + LM_TILE - 1) / LM_TILE) * ((ps[e].K + LM_TILE - 1) / LM_TILE);
        DS_REQUIRE(tiles < (1l << 30), "lora_merge: too many tiles in one launch");
    }
    for (int e = count; e <= DS_LORA_GROUP; ++e) grp.tile_start[e] = (int)tiles;
    grp.count = count;
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, grp);
    DS_LAUNCH_CHECK();
    return 0;
}

int ds_launch_lora_merge(const LoraMergeParams& p, hipStream_t stream) { return ds_launch_lora_merge_group(&p, 1, stream); }
