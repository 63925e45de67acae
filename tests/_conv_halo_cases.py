"""The cases of test_gpu_conv_halo_bits.py: the three halo-patch 3x3 convolution kernels of csrc/conv_halo.hip
(`conv_halo_kernel`, `conv_halo_deep_kernel`, `conv_halo256_kernel`) in all eight instantiations (f16, f16 phase mode, bf16) at
the smallest shapes that cross every seam of their staging, k-loops and epilogue, and the sha256 of every output as the kernels
gave it BEFORE their tile decode, descriptors, fragment walk and epilogue were moved into shared device functions
(tests/golden/conv_halo_bits.json).  The family's other tests compare the three kernels with one another, which a change that
moves all three together passes; this one does not.

No random generator: every operand is an integer formula, k / 2^a with a per-channel power-of-two scale, exact in f16 and in
bf16.  The scales differ between channels so that the fp32 accumulation is NOT exact: a changed order of adds shows.  The "full"
epilogue carries, on half of the columns, a bias of about +2048 and a per-image bias of about -2047: (acc + bias) keeps acc to
2^-12, (acc + per-image bias) to 2^-13, so the two orders of the adds round differently in about one stored value in thirty.

    python -m tests._conv_halo_cases [path]     # writes the fixture: run on the build whose bits are to be the record

Seams.  Cin 64 / 128 / 192 / 320 = 1 / 2 / 3 / 5 channel slices (the deep kernel's patch double buffer uses both parities and its
W ring wraps from 3 slices up; the 256 kernel's two W buffers alternate from 2 k-tiles).  B x H x W of 2 x 9 x 13 (one ragged
tile of the 16 x 16 kernel, two of the 8 x 16 ones), 1 x 20 x 24 and 3 x 17 x 33 (ragged both ways, several tiles, batch stride).
Cout 128 (full tile), 192 (second tile of 64 columns: the 256 kernel's TAIL body; once more under gemm_debug bit 11, which runs
it as a full tile), 72 (ragged inside a tile), 320 (tail as third tile).  Every instantiation meets every slice count on a ragged
shape with a tail tile and the full epilogue."""
import functools
import hashlib
import json
import os
import sys

import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_halo_bits.json")
VARIANT = {"k8": 1, "k256": 2, "deep": 3}          # conv_halo_variant that forces the kernel
S1, S2, S3 = (2, 9, 13), (1, 20, 24), (3, 17, 33)
SLICES = (64, 128, 192, 320)


def _groups():
    """(kernel, instantiation) -> [(mode, (B, H, W), Cin, Cout, epilogue, extra)], in the order the fixture lists them.
    mode: conv | gn (CONV3X3 op with GroupNorm partials) | up (gather x2) | resize (extra = (Ho, Wo)) | fold (phase mode);
    extra of conv: the gemm_debug value."""
    g = {}
    for k in VARIANT:
        g[k, "f16"] = ([("conv", S1, cin, 192, "full", 0) for cin in SLICES] +
                       [("conv", S2, 128, 128, "bias", 0), ("conv", S3, 128, 128, "plain", 0),
                        ("conv", S1, 64, 72, "bias", 0), ("conv", S2, 64, 320, "full", 0), ("conv", S1, 128, 192, "full", 2048),
                        ("gn", S3, 64, 192, "gn", 0),
                        ("up", (2, 5, 7), 128, 128, "full", 0), ("resize", (2, 5, 4), 128, 64, "bias", (9, 7))])
        g[k, "fold"] = ([("fold", (2, 5, 7), cin, 192, "full", 0) for cin in SLICES] + [("fold", S2, 64, 128, "plain", 0)])
    for k in ("k8", "k256"):
        g[k, "bf16"] = ([("conv", S1, cin, 192, "full", 0) for cin in SLICES] +
                        [("conv", S3, 128, 128, "bias", 0), ("up", (1, 5, 7), 64, 72, "bias", 0)])
    return g


GROUPS = _groups()


def case_name(kernel, inst, mode, shape, cin, cout, epilogue, extra):
    tail = "" if not extra else "-" + ("x".join(map(str, extra)) if isinstance(extra, tuple) else f"dbg{extra}")
    return f"{kernel}-{inst}-{mode}-{'x'.join(map(str, shape))}-{cin}-{cout}-{epilogue}{tail}"


def _ar(n):
    return torch.arange(n, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def operands(bf16, shape, cin, cout, out_hw):
    """host operands of one problem: x [B,H,W,Cin], w [Cout,3,3,Cin], gentle and cancelling biases, residual [B,Ho,Wo,Cout]"""
    dt = torch.bfloat16 if bf16 else torch.float16
    half = 128 if bf16 else 1024                      # k / half, |k| < half: 8 or 11 significant bits
    B, H, W = shape
    Ho, Wo = out_hw
    b, y, x_, c = _ar(B)[:, None, None, None], _ar(H)[None, :, None, None], _ar(W)[None, None, :, None], _ar(cin)[None, None, None, :]
    x = ((b * 977 + y * 131 + x_ * 61 + c * 29 + 7) % (2 * half - 1) - (half - 1)).float() / half * torch.pow(2.0, -(c % 3).float())
    n, t, ci = _ar(cout)[:, None, None], _ar(9)[None, :, None], _ar(cin)[None, None, :]
    w = ((n * 337 + t * 113 + ci * 43 + 3) % (2 * half - 1) - (half - 1)).float() / (16 * half) * torch.pow(2.0, -((n + ci) % 2).float())
    n1 = _ar(cout)
    bias = ((n1 * 37 + 5) % 257 - 128).float() / 64
    rowbias = ((n1[None, :] * 11 + _ar(B)[:, None] * 29) % 129 - 64).float() / 32
    # these columns: bias ~ +2048, per-image bias ~ -2047, sum 1 .. 4 (f16 only: the bf16 entry point has no per-image bias)
    cancel = ((n1 % 8) < 4) & (not bf16)
    bias_full = torch.where(cancel, 2048.0 + 2 * (n1 % 2), bias)
    rowbias_full = torch.where(cancel[None, :], -2047.0 + ((n1[None, :] >> 1) + _ar(B)[:, None]) % 2, rowbias)
    ob, oy, ox, on = _ar(B)[:, None, None, None], _ar(Ho)[None, :, None, None], _ar(Wo)[None, None, :, None], n1[None, None, None, :]
    res = ((ob * 211 + oy * 89 + ox * 53 + on * 17 + 1) % 255 - 127).float() / 64
    ops = {"x": x, "w": w.view(cout, 3, 3, cin), "bias": bias, "rowbias": rowbias, "bias_full": bias_full,
           "rowbias_full": rowbias_full, "res": res}
    for k, v in ops.items():
        assert torch.equal(v.to(dt).float(), v), (k, "not exact in", dt)
    return {k: v.to(dt).contiguous() for k, v in ops.items()}


def _out_hw(mode, shape, extra):
    _, H, W = shape
    return {"up": (2 * H, 2 * W), "fold": (2 * H, 2 * W), "resize": extra}.get(mode, (H, W))


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        assert torch.isfinite(t.float()).all()
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_case(kernel, inst, mode, shape, cin, cout, epilogue, extra):
    """sha256 of the output's bytes (mode gn: and of the fp32 partial sums) of one case; conv_halo_variant is the caller's"""
    import ctypes as C
    from diffsensei_amd import _lib, ops
    from diffsensei_amd.engine import make_op
    L = _lib.load()
    bf16 = inst == "bf16"
    o = {k: v.cuda() for k, v in operands(bf16, shape, cin, cout, _out_hw(mode, shape, extra)).items()}
    bias = {"plain": None, "bias": o["bias"], "gn": o["bias"], "full": o["bias_full"]}[epilogue]
    rowbias = {"gn": o["rowbias"], "full": o["rowbias_full"]}.get(epilogue)
    res = o["res"] if epilogue == "full" else None
    B, H, W = shape
    if mode == "gn":
        nch = int(L.ds_conv3x3_gn_chunks(B, H, W, cin, cout))
        assert nch > 0
        ws = torch.zeros(L.ds_groupnorm_workspace_bytes(B, cout), dtype=torch.uint8, device="cuda")
        y = torch.empty((B, H, W, cout), dtype=torch.float16, device="cuda")
        op = make_op("CONV3X3", i=(B, H, W, cin, cout, 1, 0, cout, 0, 0), p=(o["x"], o["w"], y, bias, rowbias, None, ws))
        rc = L.ds_op_run(C.byref(op), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.ds_last_error().decode()
        return _digest(y, ws[: B * nch * cout * 8])
    if bf16:                                            # the bf16 entry point has no per-image bias
        return _digest(ops.conv3x3_bf16(o["x"], o["w"], bias if bias is not None else torch.zeros_like(o["bias"]),
                                        upsample=mode == "up", residual=res))
    if mode == "fold":
        return _digest(ops.conv3x3_up2fold(o["x"], ops.fold_upsample2x(o["w"]), bias, rowbias=rowbias, residual=res))
    if mode == "resize":
        return _digest(ops.conv3x3(o["x"], o["w"], bias, rowbias=rowbias, residual=res, out_size=extra))
    assert L.ds_set_option(b"gemm_debug", int(extra)) == 0
    try:
        return _digest(ops.conv3x3(o["x"], o["w"], bias, upsample=mode == "up", rowbias=rowbias, residual=res))
    finally:
        assert L.ds_set_option(b"gemm_debug", 0) == 0


def run_group(kernel, inst):
    """{case name: sha256} of one (kernel, instantiation) group, the kernel forced with conv_halo_variant"""
    from diffsensei_amd import _lib
    L = _lib.load()
    out = {}
    try:
        assert L.ds_set_option(b"conv_halo_variant", VARIANT[kernel]) == 0
        for case in GROUPS[kernel, inst]:
            out[case_name(kernel, inst, *case)] = run_case(kernel, inst, *case)
    finally:
        assert L.ds_set_option(b"conv_halo_variant", 0) == 0
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
