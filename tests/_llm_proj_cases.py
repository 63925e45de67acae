"""The cases of test_gpu_llm_proj_bits.py: the four LLM projection kernels of csrc/llm.hip (`llm_gemv_kernel`,
`llm_gemv_stream_kernel`, `llm_gemv_pipe_kernel`, `llm_gemm16_kernel`) at the smallest shapes that reach every loop seam, and the
sha256 of every output as the kernels gave it BEFORE their prologue, loads and epilogue were moved into shared functions
(tests/golden/llm_proj_bits.json).  The tolerance tests of these kernels pass a changed summation order; this one does not.

No random generator and no quantiser: every operand is an integer formula whose values are exact in its format - x, residual,
gain and the fp16 weights as multiples of a power of two, int8 codes, MXFP4 bytes, block exponents 114..127 and row scales
2^-a (1 + j/8) directly.  Magnitudes are chosen so that an fp32 evaluation of every case stays finite and below 1000, which
`operands` asserts on the host.

    python -m tests._llm_proj_cases [path]     # writes the fixture: run on the build whose bits are to be the record

Shapes (N, K): A (520, 736) - 23 blocks of 32, so the K tail is a clamped re-read in all three formats; B (72, 8928) - more
than one k-iteration in the pipelined and the gemm16 kernel; C (12408, 736) - more columns than resident wavefronts and more
16-column tiles than resident blocks (the prefetch of the next column's / tile's first k-block, both halves of gemm16's
reduction buffer) with a ragged last tile."""
import functools
import hashlib
import json
import os
import sys

import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llm_proj_bits.json")
SHAPES = {"A": (520, 736), "B": (72, 8928), "C": (12408, 736)}
FORMATS = ("f16", "w8", "fp4")
# name: (residual in place, rms, gain, swiglu)
EPILOGUES = {"plain": (0, 0, 0, 0), "residual": (1, 0, 0, 0), "rms": (0, 1, 0, 0), "rms_gain": (0, 1, 1, 0),
             "swiglu_rms": (0, 1, 0, 1), "swiglu_rms_gain": (0, 1, 1, 1)}
VARIANT = {"pipe": 0, "generic": 1, "stream": 2, "gemm16": 0}   # llm_gemv_variant of the kernel (gemm16 does not read it)
EPS = 1e-5
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _groups():
    """(kernel, format, shape) -> [(epilogue, M)], in the order the fixture lists them"""
    g = {}
    every = list(EPILOGUES)
    for fmt in FORMATS:
        g["generic", fmt, "A"] = [(e, M) for e in every for M in (1, 5, 16)]
        g["pipe", fmt, "A"] = [(e, M) for e in every for M in (1, 2, 3, 4)]       # M = 3: MC = 4 with a masked row
        g["gemm16", fmt, "A"] = [(e, M) for e in every for M in (1, 5, 16)]
        g["pipe", fmt, "B"] = [(e, M) for e in (("swiglu_rms", "swiglu_rms_gain") + (() if fmt == "fp4" else ("plain",)))
                               for M in (1, 2)]
        g["gemm16", fmt, "B"] = [(e, 16) for e in ("plain", "rms_gain", "swiglu_rms")]
        g["pipe", fmt, "C"] = [(e, 1) for e in ("plain", "swiglu_rms")]
        g["gemm16", fmt, "C"] = [(e, 16) for e in ("plain", "swiglu_rms")]
    g["stream", "f16", "A"] = [(e, M) for e in every for M in (1, 3)]
    g["stream", "f16", "C"] = [(e, 1) for e in ("plain", "swiglu_rms")]
    return g


GROUPS = _groups()


def case_name(kernel, fmt, shape, epilogue, M):
    return f"{kernel}-{fmt}-{shape}-{epilogue}-M{M}"


def _weights(fmt, rows, K):
    """the operands of `rows` weight rows after x, in the order ops.llm_*_{w8,fp4} take them, and their fp32 values"""
    n = torch.arange(rows, dtype=torch.int64)[:, None]
    j8 = 1.0 + (n[:, 0] % 8).float() / 8                                       # 1 + j/8
    if fmt == "f16":
        k = torch.arange(K, dtype=torch.int64)[None, :]
        w = (((n * 37 + k * 11 + 3) % 129 - 64).float() / 1024).half()
        return (w,), w.float()
    if fmt == "w8":
        k = torch.arange(K, dtype=torch.int64)[None, :]
        q = ((n * 53 + k * 17 + 5) % 255 - 127).to(torch.int8)
        s = j8 * torch.pow(2.0, -(12 + n[:, 0] % 3).float())
        return (q, s), q.float() * s[:, None]
    kb = torch.arange(K // 2, dtype=torch.int64)[None, :]
    q = ((n * 29 + kb * 13 + 1) % 256).to(torch.uint8)                         # element 2i in the low nibble
    b = torch.arange(K // 32, dtype=torch.int64)[None, :]
    e = (114 + (n * 5 + b * 3) % 14).to(torch.uint8)
    s = j8 * torch.pow(2.0, -(7 + n[:, 0] % 3).float())
    nib = torch.stack((q & 15, q >> 4), dim=-1).reshape(rows, K).long()
    val = torch.tensor(E2M1)[nib & 7] * (1.0 - 2.0 * (nib >> 3).float())
    wd = val * torch.pow(2.0, e.float() - 127).repeat_interleave(32, dim=1) * s[:, None]
    return (q, e, s), wd


@functools.lru_cache(maxsize=None)
def operands(fmt, shape, swiglu):
    """host operands of 16 rows (a case with M rows takes the first M), checked against the magnitude bound"""
    N, K = SHAPES[shape]
    m = torch.arange(16, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :]
    x = (((m * 131 + k * 29 + 7) % 257 - 128).float() / 64).half()
    res = (((m * 17 + torch.arange(N, dtype=torch.int64)[None, :] * 7) % 65 - 32).float() / 16).half()
    gain = (1.0 + ((k[0] * 5) % 9 - 4).float() / 16).half()
    w, wd = _weights(fmt, 2 * N if swiglu else N, K)
    r = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + EPS)
    for xs in (x.float(), x.float() * r, x.float() * r * gain.float()):
        y = xs @ wd.T
        y = torch.nn.functional.silu(y[:, :N]) * y[:, N:] if swiglu else y.abs() + res.float().abs()
        assert torch.isfinite(y).all() and y.abs().max().item() < 1000.0, (fmt, shape, swiglu, y.abs().max().item())
    return {"x": x, "res": res, "gain": gain, "w": w}


@functools.lru_cache(maxsize=None)
def _on_device(fmt, shape, swiglu):
    return {k: tuple(t.cuda() for t in v) if k == "w" else v.cuda() for k, v in operands(fmt, shape, swiglu).items()}


def run_group(kernel, fmt, shape):
    """{case name: sha256 of the output's bytes} of one (kernel, format, shape) group"""
    from diffsensei_amd import _lib, ops
    fam = "llm_gemm16" if kernel == "gemm16" else "llm_gemv"
    fn = getattr(ops, fam + {"f16": "", "w8": "_w8", "fp4": "_fp4"}[fmt])
    L = _lib.load()
    out = {}
    try:
        assert L.ds_set_option(b"llm_gemv_variant", VARIANT[kernel]) == 0
        for epilogue, M in GROUPS[kernel, fmt, shape]:
            residual, rms, gain, swiglu = EPILOGUES[epilogue]
            c = _on_device(fmt, shape, bool(swiglu))
            x = c["x"][:M].contiguous()
            kw = dict(rms=bool(rms), swiglu=bool(swiglu), eps=EPS, gain=c["gain"] if gain else None)
            if residual:
                y = c["res"][:M].clone()
                fn(x, *c["w"], out=y, residual=y, **kw)                          # in place: h += x W^T
            else:
                y = fn(x, *c["w"], **kw)
            assert y.shape == (M, SHAPES[shape][0])
            out[case_name(kernel, fmt, shape, epilogue, M)] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()
    finally:
        assert L.ds_set_option(b"llm_gemv_variant", 0) == 0
    return out


def main():
    digests = {}
    for key in GROUPS:
        digests.update(run_group(*key))
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as fh:
        json.dump(digests, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(digests)} cases -> {path}")


if __name__ == "__main__":
    main()
