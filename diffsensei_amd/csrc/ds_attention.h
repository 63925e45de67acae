// What the flash / fused cross-attention kernels of attention.hip and attention_sp.hip share: the constants, the one-instruction
// exponential, the f16 packing of a score block, the two softmax passes over a score block and the 16-byte row store.
// Every function is forced inline.  What is held per kernel is its bits (tests/test_gpu_attention_bits.py), its registers,
// scratch and occupancy (profiles/attention_refactor_resource_usage.txt) and its time (profiles/attention_refactor_ab.jsonl) -
// not its instruction stream: the IP kernels' changed by hundreds of instructions, self_attn_sp_kernel's by one, and
// self_attn_kernel, held to the parent's assembly, keeps its own marked text of the exp2 pass and the store.
#pragma once
#include "ds_common.h"

constexpr float LOG2E = 1.4426950408889634f;
constexpr float NEG_BIG = -1.0e30f;

// 2^x as ONE v_exp_f32.  exp2f() adds a denormal-range rescue (compare, select, ldexp: five more VALU slots per score);
// softmax arguments are <= 0 and anything below 2^-126 may flush to zero.  The softmax of the flash kernels is VALU
// bound (32 scores per lane per 16 MFMAs), so every slot per score shows up in the kernel time.
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ h8 pack8(const f32x16& s, int base) {
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)s[base + e];
    return o;
}

// Registers 0 .. NR-1 of one score block: s = exp2(s * a + b), psum2 += s.  Two scores per VALU slot where the ISA allows it:
// v_pk_fma_f32 for the scale-and-shift, v_pk_add_f32 for the row sum (the exponential itself has no packed form).  The two
// lanes of psum2 are two chains of adds in register order: the order IS the result (tests/test_gpu_attention_bits.py).
template <int NR>
__device__ __forceinline__ void exp2_sum_block(f32x16& s, const f32x2 a, const f32x2 b, f32x2& psum2) {
#pragma unroll
    for (int r = 0; r < NR; r += 2) {
        f32x2 v = {s[r], s[r + 1]};
        v = __builtin_elementwise_fma(v, a, b);
        const f32x2 e = {fast_exp2(v[0]), fast_exp2(v[1])};
        s[r] = e[0];
        s[r + 1] = e[1];
        psum2 += e;
    }
}

// Registers 0 .. NR-1 of one score block: s *= w (v_pk_mul_f32)
template <int NR>
__device__ __forceinline__ void scale_block(f32x16& s, const f32x2 w2) {
#pragma unroll
    for (int r = 0; r < NR; r += 2) {
        f32x2 v = {s[r], s[r + 1]};
        v *= w2;
        s[r] = v[0];
        s[r + 1] = v[1];
    }
}

// One query row's 64 output columns (O^T blocks ot[0], ot[1] of the 32x32 MFMA layout), as 16-byte stores.  A lane holds columns
// 8g + 4 lhi + {0..3} of its query row; its partner lane ^ 32 the other four of every group of eight.  One v_permlane32_swap per
// dword and group pair leaves the lower lane with columns 16j .. 16j+7 and the upper one with 16j+8 .. 16j+15: four stores per
// wave and 32-column block instead of eight 8-byte ones (the hand-over of gemm_pp_kernel's GEGLU epilogue; round 6, the store shape
// was measured on ip_attn_kernel).  `op`: the row's first column + 8 lhi, the row index clamped
// by the caller: the swaps run on every lane (rows past the end included), only the stores are masked by row_ok.
// SCALE: the columns are multiplied by inv on the way (the flash kernels' 1 / row sum); the IP kernels normalise earlier and
// have no multiply here.
template <bool SCALE>
__device__ __forceinline__ void store_rows16(half_t* op, bool row_ok, const f32x16 (&ot)[2], float inv = 1.0f) {
#pragma unroll
    for (int db = 0; db < 2; ++db) {
        unsigned og[4][2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            h4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (SCALE) o[e] = (half_t)(ot[db][4 * g + e] * inv);
                else o[e] = (half_t)ot[db][4 * g + e];
            }
            const u32x2 t2 = __builtin_bit_cast(u32x2, o);
            og[g][0] = t2[0], og[g][1] = t2[1];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            swap32(og[2 * j][0], og[2 * j + 1][0]);
            swap32(og[2 * j][1], og[2 * j + 1][1]);
            const u32x4 v = {og[2 * j][0], og[2 * j][1], og[2 * j + 1][0], og[2 * j + 1][1]};
            if (row_ok) *reinterpret_cast<u32x4*>(op + db * 32 + j * 16) = v;
        }
    }
}
