"""Test restatement of the device noise source (include/diffsensei_hip.h, "device noise"): Philox4x32-10 as published
by Salmon et al. (Random123), keyed per panel, plus Box-Muller - written from the published algorithm in numpy,
independently of the HIP kernel.

  key     = (seed & 0xffffffff, seed >> 32)          one 64-bit seed per panel
  counter = (pixel, 0, step, stream)                 pixel = 0 .. HW-1 inside the panel
  output  = x0..x3 = the four latent channels of that pixel
  u_k     = x_k * 2^-32 + 2^-33 in fp32              (never 0)
  channels 0,1 = sqrt(-2 ln u0) * {cos, sin}(2 pi u1); channels 2,3 the same from (u2, u3)

The uniforms are rounded to fp32 exactly like the kernel's; Box-Muller itself runs in float64, so the result is the
value the fp32 device arithmetic approximates.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32 values, key: 2 -> 4 uint32 arrays.  Everything broadcasts."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _MASK for v in key]
    shape = np.broadcast(*c, *k).shape
    c = [np.broadcast_to(v, shape).copy() for v in c]
    k = [np.broadcast_to(v, shape).copy() for v in k]
    for r in range(10):
        if r:
            k[0] = (k[0] + np.uint64(W0)) & _MASK
            k[1] = (k[1] + np.uint64(W1)) & _MASK
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bit products: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
    return [v.astype(np.uint32) for v in c]


def philox_u32(seeds, step: int, stream: int, HW: int) -> np.ndarray:
    """uint32 [ns, HW, 4]: the raw generator output for every (panel, pixel)."""
    seeds = np.array([int(s) for s in seeds], dtype=np.uint64)
    k0 = (seeds & _MASK)[:, None]
    k1 = (seeds >> np.uint64(32))[:, None]
    pix = np.arange(HW, dtype=np.uint64)[None, :]
    out = philox4x32_10((pix, 0, int(step), int(stream)), (k0, k1))
    return np.stack(out, axis=-1)


def uniforms(x: np.ndarray) -> np.ndarray:
    """fp32 u = x * 2^-32 + 2^-33 with fp32 rounding of the conversion and of the sum (the product is exact)."""
    xf = x.astype(np.float32)
    return (xf * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)).astype(np.float32)


def philox_normal(seeds, step: int, stream: int, HW: int) -> np.ndarray:
    """float64 [ns, 4, HW]: Box-Muller in float64 on the fp32-rounded uniforms."""
    u = uniforms(philox_u32(seeds, step, stream, HW)).astype(np.float64)
    out = np.empty((u.shape[0], 4, HW), dtype=np.float64)
    for pair in (0, 1):
        r = np.sqrt(-2.0 * np.log(u[..., 2 * pair]))
        th = 2.0 * np.pi * u[..., 2 * pair + 1]
        out[:, 2 * pair] = r * np.cos(th)
        out[:, 2 * pair + 1] = r * np.sin(th)
    return out


# ---- the 4-sigma moment conditions the CPU and the GPU tests share
# 16 panels x 128 x 128 pixels x 4 channels = 2^20 normals per step; the extremes of the seed range are among them
MOMENT_SEEDS = [0, 2 ** 63 - 2, 1, 2, 3, 0x9E3779B97F4A7C15 >> 1, 20260101, 1 << 32, (1 << 32) - 1, 42, 1234567890123,
                7, 8, 9, 10, 11]
MOMENT_HW = 128 * 128


def _corr(a: np.ndarray, b: np.ndarray) -> float:
    a, b = a.ravel().astype(np.float64), b.ravel().astype(np.float64)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def moment_conditions(z: np.ndarray, z_next: np.ndarray) -> dict:
    """z, z_next: [ns, 4, HW] normals of steps s and s + 1 for the same seeds.  name -> (|statistic|, 4-sigma bound of
    that statistic for independent standard normals: std of the sample mean 1/sqrt(N), of the sample variance
    sqrt(2/N), of the sample kurtosis sqrt(24/N), of a sample correlation 1/sqrt(N))."""
    x = z.astype(np.float64).ravel()
    N = x.size
    m, v = x.mean(), x.var()
    out = {"mean": (abs(m), 4 / np.sqrt(N)), "var": (abs(v - 1), 4 * np.sqrt(2 / N)),
           "kurtosis": (abs(((x - m) ** 4).mean() / v ** 2 - 3), 4 * np.sqrt(24 / N)),
           "corr step/step+1": (abs(_corr(z, z_next)), 4 / np.sqrt(N)),
           "corr seed k/k+1": (abs(_corr(z[:-1], z[1:])), 4 / np.sqrt(z[1:].size))}
    for a in range(4):
        for b in range(a + 1, 4):
            out[f"corr channel {a}/{b}"] = (abs(_corr(z[:, a], z[:, b])), 4 / np.sqrt(z[:, a].size))
    return out
