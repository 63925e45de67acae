// Device noise shared by the sampler step (elementwise.hip) and the VAE encoder's posterior sample (vae.hip).
#pragma once
#include "ds_common.h"

namespace {

// ---------------------------------------------------------------- device noise: Philox4x32-10 + Box-Muller
// Counter-based generator of Salmon et al. (Random123), so a captured step graph draws fresh noise on every replay with
// no host work between replays.  Key = the panel's 64-bit seed, counter = (pixel in the panel, 0, step, stream): what a
// panel sees depends on its own seed and the step only, never on its row in the batch.  One call = the four latent
// channels of one pixel, i.e. the sampler kernel's own work split (include/diffsensei_hip.h, "device noise").
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ void panel_philox(long long seed, int pix, int step, int stream_id, unsigned out[4]) {
    const unsigned long long s = (unsigned long long)seed;
    philox4x32_10((unsigned)pix, 0u, (unsigned)step, (unsigned)stream_id, (unsigned)s, (unsigned)(s >> 32), out);
}

// u = x * 2^-32 + 2^-33 in (0, 1] (the product is exact, so an fma contraction rounds the same); v_sin_f32 / v_cos_f32
// take revolutions, which is what u1 is.
__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float& z0, float& z1) {
    const float u0 = (float)a * 0x1p-32f + 0x1p-33f;
    const float u1 = (float)b * 0x1p-32f + 0x1p-33f;
    const float r = sqrtf(-2.0f * __logf(u0));
    z0 = r * __builtin_amdgcn_cosf(u1);
    z1 = r * __builtin_amdgcn_sinf(u1);
}

__device__ __forceinline__ void panel_normals(long long seed, int pix, int step, int stream_id, float z[4]) {
    unsigned x[4];
    panel_philox(seed, pix, step, stream_id, x);
    box_muller(x[0], x[1], z[0], z[1]);
    box_muller(x[2], x[3], z[2], z[3]);
}

}  // namespace
