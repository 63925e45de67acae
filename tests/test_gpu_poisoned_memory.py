"""GPU: every launching entry point of include/diffsensei_hip.h with poison around its operands (tests/_arena.py), plus the
GEMM shapes with K % 64 != 0 that no op-level test had (the register-staged kernel's predicated k tail; the CLIP ViT-H/14
patch embedding, K = 592, runs it in production).

Every case runs three times - on ordinary tensors, inside an arena filled with quiet NaN and inside one filled with 1000.0
(integer operands: two different in-range patterns) - and asserts:
  1. the NaN-fill result is bit-identical to the 1000.0-fill result,
  2. both are bit-identical to the plain call (the library is deterministic: no atomics),
  3. the plain call meets the fp32 / fp64 reference at the tolerance the existing test of that op uses (named per case),
  4. the result is finite,
  5. no guard or canary byte changed.
A result that moves with the fill has read something that is not its operand; a changed guard byte is a stray store.

Padding that a documented contract makes the caller's is part of the operand and holds 1000.0 in all three runs: V^T
columns Nk..ceil8(Nk) of self-attention, key-panel rows / value-panel columns Lt..96 of the IP attention, rows
n_valid..N of the wide attention.  ds_llm_gemm16's header promises that a row of y depends on that row of x alone, "not on
the padding": x holds exactly M rows here and what follows is poison.  Index operands (token ids, the state block's current
token) are surrounded by the in-range values 1 / 2, and rows 1 and 2 of the tables they index hold NaN.

`test_every_entry_point_has_a_case` (host only) keeps the list complete: a new entry of `_lib.SIGNATURES` needs a case, or a
line in EXEMPT saying why it launches nothing of its own.

The last two tests poison what the two engines with persistent buffers keep between calls.
"""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._arena import Arena, Plain, options

DEV = "cuda"
BF = torch.bfloat16
NS = types.SimpleNamespace
LOUD = 1000.0


# ------------------------------------------------------------------------------------------------ helpers
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _r(shape, g, scale=1.0, dtype=torch.float16):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _close(got, ref, tol=2e-3, what=""):
    """tests/test_gpu_ops.py's rule: max |err| <= tol * max(max|ref|, 1e-3) + 1e-3 * tol"""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    den = max(ref.abs().max().item(), 1e-3)
    assert err <= tol * den + 1e-3 * tol, f"{what}: max err {err:.4g} vs max|ref| {den:.4g} (tol {tol:g})"


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _lib():
    from diffsensei_amd import _lib as L
    return L.load()


def _kernel_name(code, ints):
    """the kernel the dispatch gives this op under the calling thread's knobs (ds_op_describe: host only)"""
    from diffsensei_amd.engine import make_op
    lib = _lib()
    name = C.create_string_buffer(128)
    fl, by = C.c_double(), C.c_double()
    op = make_op(code, i=ints, l=(ints[2], 0, ints[2], ints[1], ints[1]) if code == "GEMM" else ())
    assert lib.ds_op_describe(C.byref(op), name, 128, C.byref(fl), C.byref(by)) == 0
    return name.value.decode()


def _op_run(op):
    lib = _lib()
    rc = lib.ds_op_run(C.byref(op), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ds_last_error().decode()


class Case:
    """id; entry: the C entry points the case must be seen calling; build() -> host data with references (cached);
    run(m, h) -> tuple of device tensors (m: Arena or Plain); check(outs, h): the reference assertions on the plain run's
    outputs (CPU tensors); opts: ((knob, value), ...); kernel: (op code, ints, expected ds_op_describe name)."""

    def __init__(self, id, entry, build, run, check, opts=(), kernel=None, capacity=96 << 20):
        self.id, self.entry, self.build, self.run, self.check = id, tuple(entry), build, run, check
        self.opts, self.kernel, self.capacity = tuple(opts), kernel, capacity


CASES = []


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


def _oid(opts):
    return "-".join(f"{k}{v}" for k, v in opts) or "auto"


# ------------------------------------------------------------------------------------------------ GEMM
K_TAIL = [(200, 136, 72), (77, 96, 200), (260, 128, 328), (130, 72, 8), (4, 1280, 592)]
GEMM_MODES = ("plain", "bias", "res", "inplace", "gelu", "quick_gelu")


@functools.lru_cache(maxsize=None)
def _gemm_data(M, N, K):
    g = _g(M + N + K)
    x, w, b, r = _r((M, K), g), _r((N, K), g, 1 / math.sqrt(K)), _r((N,), g), _r((M, N), g)
    y = x.float() @ w.float().t()
    yb = y + b.float()
    ybh = yb.half().float()
    ref = {"plain": y, "bias": yb, "res": ybh + r.float(), "inplace": ybh + r.float(), "gelu": F.gelu(ybh),
           "quick_gelu": ybh * torch.sigmoid(1.702 * ybh)}
    return NS(x=x, w=w, b=b, r=r, ref=ref)


def _gemm_run(mode):
    def run(m, h):
        x, w = m.place(h.x), m.place(h.w)
        if mode == "plain":
            return (m.ops.gemm(x, w),)
        b = m.place(h.b)
        if mode == "bias":
            return (m.ops.gemm(x, w, b),)
        if mode == "res":
            return (m.ops.gemm(x, w, b, m.place(h.r)),)
        if mode == "inplace":
            r = m.place(h.r)
            return (m.ops.gemm(x, w, b, residual=r, out=r),)
        return (m.ops.gemm(x, w, b, act=mode),)
    return run


def _gemm_check(mode):
    # tests/test_gpu_ops.py::test_gemm_bias_residual / test_gemm_activation: 2e-3 of max|ref|
    return lambda o, h: _close(o[0], h.ref[mode], 2e-3, f"gemm {mode}")


for (M, N, K) in K_TAIL:
    for mode in GEMM_MODES:
        _add(f"gemm-ktail-{M}x{N}x{K}-{mode}", ["ds_gemm_f16"], functools.partial(_gemm_data, M, N, K), _gemm_run(mode),
             _gemm_check(mode), kernel=("GEMM", (M, N, K, K, {"gelu": 2, "quick_gelu": 3}.get(mode, 0), 1, 0, 1), "gemm_f16_kernel<64,false>"))

# forced families on K % 64 == 0 shapes with M and N tails: what ds_op_describe answers under each knob (asserted).  Only knob
# values that change the kernel are listed: gemm_ring 1 replaces the ring kernel the automatic dispatch gives the two K >= 256
# shapes (<64,false,4>); gemm_t160 1 / gemm_g320 1 mean "never" and leave these shapes where they are - gemm_t160_kernel runs
# through gemm_variant 11 (also with its 128-row tiles, gemm_t160 3), gemm_g320_kernel through its 320-row GEGLU packing below
_GLDS = "gemm_glds_kernel<64,false,%d>"
GEMM_FAMILIES = {
    (200, 136, 192): [((), _GLDS % 1), ((("gemm_variant", 1),), "gemm_f16_kernel<64,false>"), ((("gemm_variant", 2),), _GLDS % 2),
                      ((("gemm_variant", 3),), _GLDS % 2), ((("gemm_variant", 7),), _GLDS % 2), ((("gemm_variant", 8),), _GLDS % 1),
                      ((("gemm_variant", 9),), _GLDS % 1), ((("gemm_variant", 11),), _GLDS % 2)],     # (K < 256: no ring kernel to switch off)
    (64, 128, 320): [((), _GLDS % 4), ((("gemm_variant", 1),), "gemm_f16_kernel<64,false>"), ((("gemm_variant", 2),), _GLDS % 2),
                     ((("gemm_variant", 3),), _GLDS % 2), ((("gemm_variant", 7),), _GLDS % 2), ((("gemm_variant", 8),), _GLDS % 1),
                     ((("gemm_variant", 9),), _GLDS % 1), ((("gemm_variant", 11),), _GLDS % 2), ((("gemm_ring", 1),), _GLDS % 1)],
    (272, 640, 256): [((), _GLDS % 4), ((("gemm_variant", 1),), "gemm_f16_kernel<64,false>"), ((("gemm_variant", 2),), _GLDS % 2),
                      ((("gemm_variant", 3),), "gemm_pp_kernel<0,0>"), ((("gemm_variant", 7),), _GLDS % 2),
                      ((("gemm_variant", 8),), _GLDS % 1), ((("gemm_variant", 9),), _GLDS % 1),
                      ((("gemm_variant", 11),), "gemm_t160_kernel"), ((("gemm_variant", 11), ("gemm_t160", 3)), None),
                      ((("gemm_ring", 1),), _GLDS % 1)],
}
for (M, N, K), fams in GEMM_FAMILIES.items():
    for opts, kern in fams:
        for mode in ("res", "gelu"):
            _add(f"gemm-{M}x{N}x{K}-{_oid(opts)}-{mode}", ["ds_gemm_f16"], functools.partial(_gemm_data, M, N, K), _gemm_run(mode),
                 _gemm_check(mode), opts=opts,
                 kernel=None if kern is None or mode == "gelu" else ("GEMM", (M, N, K, K, 0, 1, 0, 1), kern))


# split A (K1 = 64 + a 72-wide x2) and ldc > N with a canary behind the columns
@functools.lru_cache(maxsize=None)
def _split_data(M, N, K1, K2):
    g = _g(M + N + K1 + K2)
    x1, x2, w = _r((M, K1), g), _r((M, K2), g), _r((N, K1 + K2), g, 1 / math.sqrt(K1 + K2))
    return NS(x1=x1, x2=x2, w=w, ref=torch.cat([x1, x2], 1).float() @ w.float().t())


_add("gemm-split-a-200x136x64+72", ["ds_gemm_f16"], functools.partial(_split_data, 200, 136, 64, 72),
     lambda m, h: (m.ops.gemm(m.place(h.x1), m.place(h.w), x2=m.place(h.x2)),),
     lambda o, h: _close(o[0], h.ref, 2e-3, "split A"))          # test_gemm_split_a: 2e-3


def _gemm_wide_run(extra):
    def run(m, h):
        from diffsensei_amd import _lib as L, ops
        M, K = h.x.shape
        N = h.w.shape[0]
        x, w, b, r = m.place(h.x), m.place(h.w), m.place(h.b), m.place(h.r)
        y = m.out((M, N), ld=N + extra)
        L.check(_lib().ds_gemm_f16(x.data_ptr(), K, None, 0, K, w.data_ptr(), K, b.data_ptr(), r.data_ptr(), N, y.data_ptr(),
                                   N + extra, M, N, K, 0, ops._stream()), "ds_gemm_f16 (ldy > N)")
        return (y,)
    return run


for (M, N, K), opts in [((200, 136, 72), ()), ((260, 128, 328), ()), ((272, 640, 256), ()), ((272, 640, 256), (("gemm_variant", 3),)),
                        ((272, 640, 256), (("gemm_variant", 11),)), ((200, 136, 192), (("gemm_variant", 2),))]:
    _add(f"gemm-ldc-{M}x{N}x{K}-{_oid(opts)}", ["ds_gemm_f16"], functools.partial(_gemm_data, M, N, K), _gemm_wide_run(24),
         _gemm_check("res"), opts=opts)


# GEGLU at M = 777 (128-row packing) and on gemm_g320_kernel (320-row packing)
@functools.lru_cache(maxsize=None)
def _geglu_data(M, Ch, K, pack):
    from diffsensei_amd.engine import pack_geglu, pack_geglu320
    g = _g(M + Ch + K)
    x, w, b = _r((M, K), g), _r((2 * Ch, K), g, 1 / math.sqrt(K)), _r((2 * Ch,), g)
    p = (x.float() @ w.float().t() + b.float()).half().float()
    ref = p[:, :Ch] * F.gelu(p[:, Ch:]).half().float()
    wp, bp = pack_geglu(w, b) if pack == 128 else (pack_geglu320(w), pack_geglu320(b))
    return NS(x=x, wp=wp, bp=bp, ref=ref)


_add("gemm-geglu-777", ["ds_gemm_f16"], functools.partial(_geglu_data, 777, 512, 128, 128),
     lambda m, h: (m.ops.gemm(m.place(h.x), m.place(h.wp), m.place(h.bp), geglu=True),),
     lambda o, h: _close(o[0], h.ref, 2e-3, "geglu"))            # test_gemm_geglu: 2e-3
_add("gemm-geglu320-300x640x192", ["ds_gemm_f16"], functools.partial(_geglu_data, 300, 320, 192, 320),
     lambda m, h: (m.ops.gemm(m.place(h.x), m.place(h.wp), m.place(h.bp), geglu=320),),
     lambda o, h: _close(o[0], h.ref, 3e-3, "geglu320"),         # test_gpu_gemm_g320.py: 3e-3
     kernel=("GEMM", (300, 640, 192, 192, 4, 1, 0, 1), "gemm_g320_kernel"))


# batched V^T form
@functools.lru_cache(maxsize=None)
def _vt_data(B, N, Cc, dtype=torch.float16):
    g = _g(B + N + Cc)
    x, wv = _r((B, N, Cc), g, dtype=dtype), _r((Cc, Cc), g, 1 / math.sqrt(Cc), dtype=dtype)
    return NS(x=x, wv=wv, ref=torch.einsum("ck,bnk->bcn", wv.float(), x.float()))


for (B, N, Cc), opts, kern in [((3, 272, 384), (), _GLDS % 4), ((3, 272, 384), (("gemm_variant", 1),), "gemm_f16_kernel<64,false>"),
                               ((3, 272, 384), (("gemm_variant", 3),), "gemm_pp_kernel<0,0>"),
                               ((5, 1000, 1280), (), "gemm_glds_kernel<128,false,1>"),
                               ((5, 1000, 1280), (("gemm_variant", 1),), "gemm_f16_kernel<128,false>")]:
    _add(f"gemm-batched-vt-{B}x{N}x{Cc}-{_oid(opts)}", ["ds_gemm_f16_batched"], functools.partial(_vt_data, B, N, Cc),
         lambda m, h: (m.ops.gemm_batched_nt(m.place(h.wv), m.place(h.x)),),
         lambda o, h: _close(o[0], h.ref, 2e-3, "V^T"), opts=opts,          # test_gemm_batched_vt: 2e-3
         kernel=("GEMM", (Cc, N, Cc, Cc, 0, B, 0, 1), kern))


# fused LayerNorm: producers and consumers of tests/test_gpu_ln_fusion.py at their smallest shapes, statistics in the arena
def _relmax_ok(got, ref, tol, what):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    e = ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()
    assert e <= tol, f"{what}: {e:.3g} > {tol:g}"


@functools.lru_cache(maxsize=None)
def _ln_producer_data(M, N, K):
    g = _g(M + N + K + 1)
    x, w, b = _r((M, K), g), _r((N, K), g, 1 / math.sqrt(K)), _r((N,), g)
    r = (_r((M, N), g) * 3 + 1.5).half()
    ref = (x.float() @ w.float().t() + b.float()).half().float() + r.float()
    return NS(x=x, w=w, b=b, r=r, ref=ref, N=N)


def _ln_producer_run(finalize):
    def run(m, h):
        y, part = m.ops.gemm_ln(m.place(h.x), m.place(h.w), m.place(h.b), residual=m.place(h.r), emit_stats=True)
        return (y, part, m.ops.ln_finalize(part, h.N, 1e-5)) if finalize else (y, part)
    return run


def _ln_producer_check(o, h):
    # test_producer_row_statistics / test_wide_producer_row_statistics: sums rtol 1e-5 atol 1e-3; mean 1e-5, rstd 1e-4
    _close(o[0], h.ref, 2e-3, "producer output")
    yf = o[0].float()
    M, N = yf.shape
    strips = yf.view(M, N // 64, 64)
    assert torch.allclose(o[1][..., 0].t(), strips.sum(-1), rtol=1e-5, atol=1e-3)
    assert torch.allclose(o[1][..., 1].t(), (strips * strips).sum(-1), rtol=1e-5, atol=1e-3)
    if len(o) > 2:
        assert torch.allclose(o[2][:, 0], yf.mean(1), rtol=1e-5, atol=1e-5)
        assert torch.allclose(o[2][:, 1], torch.rsqrt(yf.var(1, unbiased=False) + 1e-5), rtol=1e-4, atol=0)


_add("gemm-ln-producer-pp-1024x256x128", ["ds_gemm_ln_f16", "ds_ln_finalize"], functools.partial(_ln_producer_data, 1024, 256, 128),
     _ln_producer_run(True), _ln_producer_check, opts=(("gemm_variant", 3),))
_add("gemm-ln-producer-wide-154x1280x1280", ["ds_gemm_ln_f16"], functools.partial(_ln_producer_data, 154, 1280, 1280),
     _ln_producer_run(False), _ln_producer_check)


@functools.lru_cache(maxsize=None)
def _ln_consumer_data(M, N, K, geglu=False):
    from diffsensei_amd.engine import pack_geglu, pack_ln_fused
    g = _g(M + N + K + 3)
    x = ((torch.randn((M, K), generator=g) + 0.3) * (1.0 + torch.rand((M, 1), generator=g) * 3)).half()
    w, b = _r((N, K), g, 1 / math.sqrt(K)), _r((N,), g, 0.3)
    gamma, beta = (1 + 0.2 * torch.randn(K, generator=g)).half(), _r((K,), g, 0.2)
    z = F.linear(F.layer_norm(x.float(), (K,), gamma.float(), beta.float(), 1e-5), w.float(), b.float())
    gw, c2, b2 = pack_ln_fused(w, b, gamma, beta)
    if geglu:
        half = N // 2
        ref = z[:, :half].half().float() * F.gelu(z[:, half:].half().float())
        gw, b2 = pack_geglu(gw, b2)
        c2 = torch.stack([c2[:half].reshape(-1, 64, 2), c2[half:].reshape(-1, 64, 2)], dim=1).reshape(-1, 2).contiguous()
    else:
        ref = z
    xs = x.float().view(M, K // 64, 64)
    part = torch.stack([xs.sum(-1).t(), (xs * xs).sum(-1).t()], dim=-1).contiguous()
    return NS(x=x, gw=gw, c2=c2, b2=b2, part=part, ref=ref, K=K)


def _ln_consumer_run(form, geglu):
    def run(m, h):
        x, gw, b2, c2, part = m.place(h.x), m.place(h.gw), m.place(h.b2), m.place(h.c2), m.place(h.part)
        if form == "partial":
            return (m.ops.gemm_ln_partial(x, gw, b2, c2, part, geglu=geglu),)
        return (m.ops.gemm_ln(x, gw, b2, c2, m.ops.ln_finalize(part, h.K, 1e-5), geglu=geglu),)
    return run


# test_consumer_plain_vs_layernorm_linear / test_wide_consumer_plain_vs_layernorm_linear: 3e-3; the GEGLU forms: 4e-3
_add("gemm-ln-consumer-pp-256x256x128", ["ds_gemm_ln_f16", "ds_ln_finalize"], functools.partial(_ln_consumer_data, 256, 256, 128),
     _ln_consumer_run("final", False), lambda o, h: _relmax_ok(o[0], h.ref, 3e-3, "LN consumer"), opts=(("gemm_variant", 3),))
_add("gemm-ln-consumer-pp-geglu-512x2048x256", ["ds_gemm_ln_f16"], functools.partial(_ln_consumer_data, 512, 2048, 256, True),
     _ln_consumer_run("final", True), lambda o, h: _relmax_ok(o[0], h.ref, 4e-3, "LN GEGLU consumer"), opts=(("gemm_variant", 3),))
_add("gemm-ln-consumer-wide-64x128x64", ["ds_gemm_ln_partial_f16"], functools.partial(_ln_consumer_data, 64, 128, 64),
     _ln_consumer_run("partial", False), lambda o, h: _relmax_ok(o[0], h.ref, 3e-3, "LN consumer (partial sums)"))
_add("gemm-ln-consumer-wide-geglu-192x1024x128", ["ds_gemm_ln_partial_f16"], functools.partial(_ln_consumer_data, 192, 1024, 128, True),
     _ln_consumer_run("partial", True), lambda o, h: _relmax_ok(o[0], h.ref, 4e-3, "LN GEGLU consumer (partial sums)"))


@functools.lru_cache(maxsize=None)
def _ln_swapped_data(Z, N, Cc):
    from diffsensei_amd.engine import pack_ln_fused
    g = _g(21 + Cc + Z * 7 + N)
    x = ((torch.randn((Z, N, Cc), generator=g) + 0.4) * (1.0 + torch.rand((Z, N, 1), generator=g) * 3)).half()
    wv, gamma, beta = _r((Cc, Cc), g, 1 / math.sqrt(Cc)), (1 + 0.2 * torch.randn(Cc, generator=g)).half(), _r((Cc,), g, 0.3)
    ref = torch.einsum("ck,znk->zcn", wv.float(), F.layer_norm(x.float(), (Cc,), gamma.float(), beta.float(), 1e-5))
    gw, c2, _ = pack_ln_fused(wv, None, gamma, beta)
    bf = (wv.double() @ beta.double()).float()
    bh = bf.half()
    cb = torch.cat([c2, torch.stack([bh, (bf - bh.float()).half()], dim=1)], dim=1).contiguous()
    xs = x.float().view(Z * N, Cc // 64, 64)
    part = torch.stack([xs.sum(-1).t(), (xs * xs).sum(-1).t()], dim=-1).contiguous()
    return NS(x=x, gw=gw, cb=cb, part=part, ref=ref, C=Cc)


# test_consumer_swapped_vs_layernorm_linear / test_wide_consumer_swapped_vs_layernorm_linear: 3e-3
_add("gemm-ln-swapped-pp-3x512x256", ["ds_gemm_ln_swapped_f16", "ds_ln_finalize"], functools.partial(_ln_swapped_data, 3, 512, 256),
     lambda m, h: (m.ops.gemm_ln_swapped(m.place(h.gw), m.place(h.x), m.ops.ln_finalize(m.place(h.part), h.C, 1e-5), m.place(h.cb)),),
     lambda o, h: _relmax_ok(o[0], h.ref, 3e-3, "LN swapped consumer"), opts=(("gemm_variant", 3),))
for (Z, N, Cc) in [(1, 72, 128), (3, 296, 640)]:
    _add(f"gemm-ln-swapped-wide-{Z}x{N}x{Cc}", ["ds_gemm_ln_swapped_partial_f16"], functools.partial(_ln_swapped_data, Z, N, Cc),
         lambda m, h: (m.ops.gemm_ln_swapped_partial(m.place(h.gw), m.place(h.x), m.place(h.part), m.place(h.cb)),),
         lambda o, h: _relmax_ok(o[0], h.ref, 3e-3, "LN swapped consumer (partial sums)"))


# bf16 GEMM and its batched form (tests/test_gpu_vae.py::test_gemm_and_groupnorm_bf16: 1e-2 of max|ref|)
def _close_rel(got, ref, tol, what):
    """tests/test_gpu_vae.py / test_gpu_mllm.py's rule: max |err| <= tol * max(max|ref|, 1e-3)"""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    den = max(ref.abs().max().item(), 1e-3)
    assert err <= tol * den, f"{what}: max err {err:.4g} vs max|ref| {den:.4g} (tol {tol:g})"


@functools.lru_cache(maxsize=None)
def _gemm_bf16_data(M, N, K):
    g = _g(M + N + K)
    x, w, b, r = _r((M, K), g, dtype=BF), _r((N, K), g, 1 / math.sqrt(K), dtype=BF), _r((N,), g, dtype=BF), _r((M, N), g, dtype=BF)
    return NS(x=x, w=w, b=b, r=r, ref=(x.float() @ w.float().t() + b.float()).to(BF).float() + r.float())


for (M, N, K) in [(272, 144, 128), (1040, 256, 512)]:
    _add(f"gemm-bf16-{M}x{N}x{K}", ["ds_gemm_bf16"], functools.partial(_gemm_bf16_data, M, N, K),
         lambda m, h: (m.ops.gemm_bf16(m.place(h.x), m.place(h.w), m.place(h.b), m.place(h.r)),),
         lambda o, h: _close_rel(o[0], h.ref, 1e-2, "gemm bf16"))
_add("gemm-bf16-batched-2x272x512", ["ds_gemm_bf16_batched"], functools.partial(_vt_data, 2, 272, 512, BF),
     lambda m, h: (m.ops.gemm_batched_nt_bf16(m.place(h.wv), m.place(h.x)),),
     lambda o, h: _close_rel(o[0], h.ref, 1e-2, "V^T bf16"))


# ------------------------------------------------------------------------------------------------ convolution
@functools.lru_cache(maxsize=None)
def _conv_data(B, H, W, Cin, Cout, form, out_hw=None, dtype=torch.float16):
    g = _g(B * H + W + Cin + Cout + len(form))
    x = torch.randn((B, Cin, H, W), generator=g).to(dtype)
    w = (torch.randn((Cout, Cin, 3, 3), generator=g) / math.sqrt(9 * Cin)).to(dtype)
    b = torch.randn((Cout,), generator=g).to(dtype)
    xf = x.float()
    if form in ("up", "fold"):
        ref = F.conv2d(F.interpolate(xf, scale_factor=2.0, mode="nearest"), w.float(), b.float(), padding=1)
    elif form == "resize":
        ref = F.conv2d(F.interpolate(xf, size=out_hw, mode="nearest"), w.float(), b.float(), padding=1)
    elif form == "s2":
        ref = F.conv2d(xf, w.float(), b.float(), stride=2, padding=1)
    elif form == "down":
        ref = F.conv2d(F.pad(xf, (0, 1, 0, 1)), w.float(), b.float(), stride=2)
    else:
        ref = F.conv2d(xf, w.float(), b.float(), padding=1)
    rb, res = _r((B, Cout), g, dtype=dtype), _r(tuple(ref.shape), g, dtype=dtype)
    if dtype == torch.float16:
        ref2 = (ref + rb.float()[:, :, None, None]).half().float() + res.float()
    else:
        ref2 = ref.to(BF).float() + res.float()
    return NS(x=_nhwc(x), w=_nhwc(w), b=b, rb=rb, res=_nhwc(res), ref=ref, ref2=ref2, w_nchw=w)


def _conv_run(form, out_hw=None):
    def run(m, h):
        x, w, b, rb, res = m.place(h.x), m.place(h.w), m.place(h.b), m.place(h.rb), m.place(h.res)
        kw = {"s1": {}, "s2": {"stride": 2}, "up": {"upsample": True}, "resize": {"out_size": out_hw}}[form]
        return (m.ops.conv3x3(x, w, b, **kw), m.ops.conv3x3(x, w, b, rowbias=rb, residual=res, **kw))
    return run


def _conv_check(o, h):
    # tests/test_gpu_ops.py::test_conv3x3 and its forced-variant twins: 2e-3 of max|ref|
    _close(_nchw(o[0]), h.ref, 2e-3, "conv")
    _close(_nchw(o[1]), h.ref2, 2e-3, "conv + rowbias + residual")


HALO = {1: "conv_halo_kernel", 2: "conv_halo256_kernel", 3: "conv_halo_deep_kernel"}
SIZES = [(9, 13), (20, 24)]
CHANNELS = [(64, 128), (192, 64), (128, 192)]
_conv_fams = [((("conv_halo_variant", v),), HALO[v]) for v in (1, 2, 3)] + \
             [((("gemm_variant", 1),), "gemm_f16_kernel<64,true>"), ((("gemm_variant", 2),), "gemm_glds_kernel<64,true,2>")]
for (H, W) in SIZES:
    for (Cin, Cout) in CHANNELS:
        for opts, kern in _conv_fams:
            _add(f"conv-s1-{H}x{W}-{Cin}to{Cout}-{_oid(opts)}", ["ds_conv3x3_f16"], functools.partial(_conv_data, 2, H, W, Cin, Cout, "s1"),
                 _conv_run("s1"), _conv_check, opts=opts, kernel=("CONV3X3", (2, H, W, Cin, Cout, 1, 0, 0, 0, 0, 0), kern))
    for (Cin, Cout) in CHANNELS[:2]:
        for opts, kern in _conv_fams:
            _add(f"conv-up2-{H}x{W}-{Cin}to{Cout}-{_oid(opts)}", ["ds_conv3x3_f16"], functools.partial(_conv_data, 2, H, W, Cin, Cout, "up"),
                 _conv_run("up"), _conv_check, opts=opts, kernel=("CONV3X3", (2, H, W, Cin, Cout, 1, 1, 0, 0, 0, 0), kern))
        for opts, kern in [((), "gemm_glds_kernel<64,true,1>")] + _conv_fams[3:]:
            _add(f"conv-s2-{H}x{W}-{Cin}to{Cout}-{_oid(opts)}", ["ds_conv3x3_f16"], functools.partial(_conv_data, 2, H, W, Cin, Cout, "s2"),
                 _conv_run("s2"), _conv_check, opts=opts, kernel=("CONV3X3", (2, H, W, Cin, Cout, 2, 0, 0, 0, 0, 0), kern))
    out_hw = (2 * H - 1, 2 * W + 1)
    for opts, kern in _conv_fams:
        _add(f"conv-resize-{H}x{W}-to-{out_hw[0]}x{out_hw[1]}-{_oid(opts)}", ["ds_conv3x3_resize_f16"],
             functools.partial(_conv_data, 2, H, W, 64, 128, "resize", out_hw), _conv_run("resize", out_hw), _conv_check, opts=opts,
             kernel=("CONV3X3", (2, H, W, 64, 128, 1, 1, 0, out_hw[0], out_hw[1], 0), kern))


def _fold_run(m, h):
    x, w, b, rb, res = m.place(h.x), m.place(h.w), m.place(h.b), m.place(h.rb), m.place(h.res)
    wf = m.ops.fold_upsample2x(w)
    return (wf, m.ops.conv3x3_up2fold(x, wf, b), m.ops.conv3x3_up2fold(x, wf, b, rowbias=rb, residual=res))


def _fold_check(o, h):
    # tests/test_gpu_upsample_fold.py: the native fold bit for bit; the phase mode at 2e-3 of max|ref|
    from diffsensei_amd.engine import fold_upsample2x_reference
    assert torch.equal(o[0], fold_upsample2x_reference(h.w.reshape(h.w.shape[0], -1)))
    _close(_nchw(o[1]), h.ref, 2e-3, "phase mode")
    _close(_nchw(o[2]), h.ref2, 2e-3, "phase mode + rowbias + residual")


for (H, W) in SIZES:
    for v in (1, 2, 3):
        _add(f"conv-fold-{H}x{W}-64to192-halo{v}", ["ds_fold_upsample2x_f16", "ds_conv3x3_up2fold_f16"],
             functools.partial(_conv_data, 2, H, W, 64, 192, "fold"), _fold_run, _fold_check, opts=(("conv_halo_variant", v),),
             kernel=("CONV3X3", (2, H, W, 64, 192, 1, 2, 0, 0, 0, 0), HALO[v]))

for (H, W) in SIZES:
    for dt, entry, tol in ((torch.float16, "ds_conv3x3_down_f16", 2e-3), (BF, "ds_conv3x3_down_bf16", 1e-2)):
        # tests/test_gpu_vae_encode_ops.py: 2e-3 (f16), 1e-2 (bf16) of max|ref|
        _add(f"conv-down-{H}x{W}-{'bf16' if dt == BF else 'f16'}", [entry], functools.partial(_conv_data, 2, H, W, 128, 128, "down", None, dt),
             lambda m, h: (m.ops.conv3x3_down(m.place(h.x), m.place(h.w), m.place(h.b)),),
             lambda o, h, tol=tol: _close_rel(_nchw(o[0]), h.ref, tol, "conv3x3_down"))
    for up in (False, True):
        for v in (1, 2):
            # tests/test_gpu_vae.py::test_conv3x3_bf16: 1e-2 of max|ref|
            _add(f"conv-bf16-{H}x{W}-{'up' if up else 's1'}-halo{v}", ["ds_conv3x3_bf16"],
                 functools.partial(_conv_data, 2, H, W, 128, 192, "up" if up else "s1", None, BF),
                 lambda m, h, up=up: (m.ops.conv3x3_bf16(m.place(h.x), m.place(h.w), m.place(h.b), upsample=up),
                                      m.ops.conv3x3_bf16(m.place(h.x), m.place(h.w), m.place(h.b), upsample=up, residual=m.place(h.res))),
                 lambda o, h: (_close_rel(_nchw(o[0]), h.ref, 1e-2, "conv bf16"), _close_rel(_nchw(o[1]), h.ref2, 1e-2, "conv bf16 + residual")),
                 opts=(("conv_halo_variant", v),))


# GroupNorm statistics out of the convolution's epilogue into a poisoned workspace, then the GroupNorm that reads them
@functools.lru_cache(maxsize=None)
def _gn_conv_data(B, H, W, Cin, Cout):
    h = _conv_data(B, H, W, Cin, Cout, "s1")
    g = _g(B + H + Cin + Cout)
    gamma, beta = (1 + 0.2 * torch.randn(Cout, generator=g)).half(), _r((Cout,), g, 0.2)
    return NS(x=h.x, w=h.w, b=h.b, rb=h.rb, gamma=gamma, beta=beta, ref=(h.ref + h.rb.float()[:, :, None, None]), dims=(B, H, W, Cin, Cout))


def _gn_conv_run(m, h):
    from diffsensei_amd.engine import make_op
    lib = _lib()
    B, H, W, Cin, Cout = h.dims
    x, w, b, rb, gamma, beta = (m.place(t) for t in (h.x, h.w, h.b, h.rb, h.gamma, h.beta))
    nch = int(lib.ds_conv3x3_gn_chunks(B, H, W, Cin, Cout))
    assert nch > 0
    ws = m.out((int(lib.ds_groupnorm_workspace_bytes(B, Cout)),), dtype=torch.uint8)       # poisoned before the call
    y = m.out((B, H, W, Cout))
    _op_run(make_op("CONV3X3", i=(B, H, W, Cin, Cout, 1, 0, Cout, 0, 0, nch), p=(x, w, y, b, rb, None, ws)))
    out = m.out((B, H * W, Cout))
    _op_run(make_op("GROUPNORM", i=(B, H * W, Cout, 0, 32, 1, nch), f=(1e-5,), p=(y, None, out, gamma, beta, ws)))
    return (y, out)


def _gn_conv_check(o, h):
    # tests/test_gpu_gn_from_conv.py: conv output at the conv tolerance; GroupNorm + SiLU of the stored tensor at 3e-3
    _close(_nchw(o[0]), h.ref, 2e-3, "conv + rowbias (emitting statistics)")
    B, H, W, Cin, Cout = h.dims
    yf = o[0].float().view(B, H * W, Cout)
    ref = F.silu(F.group_norm(yf.transpose(1, 2), 32, h.gamma.float(), h.beta.float(), 1e-5)).transpose(1, 2)
    _relmax_ok(o[1], ref, 3e-3, "GroupNorm from conv partials")


# (pre_chunks needs one f16 source, so the two-source (1, 333, 128 + 64) shape below cannot take it: the pre_chunks path runs
# here, under both GroupNorm geometries)
for (H, W), (Cin, Cout) in [((9, 13), (64, 128)), ((20, 24), (128, 192))]:
    for v in (1, 2, 3):
        for gv in (0, 1):
            _add(f"conv-gn-partial-{H}x{W}-{Cin}to{Cout}-halo{v}-gn{gv}", ["ds_op_run", "ds_conv3x3_gn_chunks", "ds_groupnorm_workspace_bytes"],
                 functools.partial(_gn_conv_data, 2, H, W, Cin, Cout), _gn_conv_run, _gn_conv_check,
                 opts=(("conv_halo_variant", v), ("gn_variant", gv)))


# ------------------------------------------------------------------------------------------------ normalisation
@functools.lru_cache(maxsize=None)
def _gn_data(B, HW, C1, C2, dtype=torch.float16, silu=True, eps=1e-5):
    g = _g(HW + C1 + C2)
    x1 = (_r((B, HW, C1), g, 2.0).float() + 0.5).to(dtype)
    x2 = _r((B, HW, C2), g, dtype=dtype) if C2 else None
    Cc = C1 + C2
    gamma, beta = (1 + 0.1 * torch.randn(Cc, generator=g)).to(dtype), (0.1 * torch.randn(Cc, generator=g)).to(dtype)
    xc = torch.cat([x1, x2], -1) if C2 else x1
    ref = F.group_norm(xc.float().permute(0, 2, 1), 32, gamma.float(), beta.float(), eps).permute(0, 2, 1)
    return NS(x1=x1, x2=x2, gamma=gamma, beta=beta, ref=F.silu(ref) if silu else ref, eps=eps, silu=silu)


def _gn_run(kind):
    def run(m, h):
        x1, gamma, beta = m.place(h.x1), m.place(h.gamma), m.place(h.beta)
        if kind == "f16":
            return (m.ops.groupnorm(x1, gamma, beta, 32, h.eps, h.silu, None if h.x2 is None else m.place(h.x2)),)
        if kind == "bf16":
            return (m.ops.groupnorm_bf16(x1, gamma, beta, 32, h.eps, h.silu),)
        return (m.ops.groupnorm_scaled(x1, gamma, beta, 32, h.eps, h.silu, 2.0 ** -6),)
    return run


for v in (0, 1):
    for (B, HW, C1, C2) in [(1, 333, 128, 64), (2, 64, 1920, 0)]:
        # tests/test_gpu_ops.py::test_groupnorm: 3e-3
        _add(f"groupnorm-f16-{B}x{HW}x{C1}+{C2}-gn{v}", ["ds_groupnorm_f16", "ds_groupnorm_workspace_bytes"],
             functools.partial(_gn_data, B, HW, C1, C2), _gn_run("f16"), lambda o, h: _close(o[0], h.ref, 3e-3, "groupnorm"),
             opts=(("gn_variant", v),))
        # the scaled form is the same kernel with one more multiply (2^-6: exact): test_groupnorm's 3e-3 on ref * 2^-6
        _add(f"groupnorm-scaled-{B}x{HW}x{C1 + C2}-gn{v}", ["ds_groupnorm_scaled_f16"], functools.partial(_gn_data, B, HW, C1 + C2, 0),
             _gn_run("scaled"), lambda o, h: _close(o[0], h.ref * 2.0 ** -6, 3e-3, "groupnorm scaled"), opts=(("gn_variant", v),))
        # tests/test_gpu_vae.py::test_gemm_and_groupnorm_bf16: 2e-2 of max|ref|
        _add(f"groupnorm-bf16-{B}x{HW}x{C1 + C2}-gn{v}", ["ds_groupnorm_bf16"], functools.partial(_gn_data, B, HW, C1 + C2, 0, BF, v == 0, 1e-6),
             _gn_run("bf16"), lambda o, h: _close_rel(o[0], h.ref, 2e-2, "groupnorm bf16"), opts=(("gn_variant", v),))


@functools.lru_cache(maxsize=None)
def _lnorm_data(rows, Cc):
    g = _g(rows + Cc)
    x = (_r((rows, Cc), g, 3.0).float() + 1.0).half()
    gamma, beta = (1 + 0.1 * torch.randn(Cc, generator=g)).half(), (0.1 * torch.randn(Cc, generator=g)).half()
    return NS(x=x, gamma=gamma, beta=beta, ref=F.layer_norm(x.float(), (Cc,), gamma.float(), beta.float(), 1e-5))


for rows, Cc in [(5, 768), (37, 128), (9, 8192)]:
    _add(f"layernorm-{rows}x{Cc}", ["ds_layernorm_f16"], functools.partial(_lnorm_data, rows, Cc),
         lambda m, h: (m.ops.layernorm(m.place(h.x), m.place(h.gamma), m.place(h.beta)),),
         lambda o, h: _close(o[0], h.ref, 2e-3, "layernorm"))     # test_layernorm: 2e-3


# ------------------------------------------------------------------------------------------------ attention
@functools.lru_cache(maxsize=None)
def _self_attn_data(B, heads, N):
    g = _g(B + heads + N)
    Cc = heads * 64
    q, k, v = _r((B, N, Cc), g), _r((B, N, Cc), g), _r((B, N, Cc), g)
    hs = lambda t: t.float().view(B, N, heads, 64).transpose(1, 2)
    ref = F.scaled_dot_product_attention(hs(q), hs(k), hs(v)).transpose(1, 2).reshape(B, N, Cc)
    Np = (N + 7) // 8 * 8
    vt = torch.full((B, heads, 64, Np), LOUD, dtype=torch.float16)            # the caller's padding: part of the operand
    vt[..., :N] = v.view(B, N, heads, 64).permute(0, 2, 3, 1)
    return NS(q=q, k=k, vt=vt, ref=ref, heads=heads)


ATTN_KERNELS = {1: "self_attn_kernel<1>", 2: "self_attn_kernel<2>", 3: "self_attn_sp_kernel"}
for (B, heads, N) in [(2, 2, 63), (1, 4, 99), (2, 1, 20), (1, 2, 1001)]:
    for v in (1, 2, 3):
        # test_self_attention_any_token_count / test_self_attention_sp_any_token_count: 3e-3
        _add(f"self-attn-{B}x{heads}x{N}-attn{v}", ["ds_self_attn_f16"], functools.partial(_self_attn_data, B, heads, N),
             lambda m, h: (m.ops.self_attention(m.place(h.q), m.place(h.k), m.place(h.vt), h.heads),),
             lambda o, h: _close(o[0], h.ref, 3e-3, "self-attn"), opts=(("attn_variant", v),),
             kernel=("SELF_ATTN", (B, heads, N, N), ATTN_KERNELS[v]))


# masked IP attention in the column-slice layout of tests/test_gpu_masked_ip_attn.py::test_stacked_panels_and_column_slices
IP_LAYOUT = (16, 16, 4)
IP_SCALES = (0.6, -0.35, 0.9)


@functools.lru_cache(maxsize=None)
def _ip_data(B, heads, hw):
    from tests.test_gpu_masked_ip_attn import _case
    operands, bbox, t, i = _case(B, heads, hw, 77, IP_LAYOUT)
    q, kt, vtt, ki, vti = (x.clone() for x in operands)
    kt[:, 77:], vtt[:, :, 77:], ki[:, 80:], vti[:, :, 80:] = LOUD, LOUD, LOUD, LOUD      # the caller's padding (header: anything finite)
    scales = torch.tensor(IP_SCALES[:B], dtype=torch.float32)
    return NS(q=q, kt=kt, vtt=vtt, ki=ki, vti=vti, bbox=bbox, ref=t + 0.6 * i, ref_rows=t + scales.double().view(B, 1, 1) * i,
              scales=scales, heads=heads, hw=hw)


def _ip_run(rows):
    def run(m, h):
        from tests.test_gpu_masked_ip_attn import LP
        nd, tpi, K = IP_LAYOUT
        kw = dict(Lt=77, Li=nd + K * tpi, n_dummy=nd, tok_per_ip=tpi)
        bbox = m.place(h.bbox)
        sd = m.place(h.scales) if rows else None
        if m.plain:
            return (m.ops.masked_ip_attention(m.place(h.q), m.place(h.kt), m.place(h.vtt), m.place(h.ki), m.place(h.vti), bbox, h.heads,
                                              h.hw, 0.6, ip_scale_dev=sd, **kw),)
        B, N, Cc = h.q.shape
        Wd, off, ldq, qo, ldo = Cc + 128, 64, Cc + 64, 32, Cc + 24

        def stacked(shape, sl, t):                  # the operand inside a wider buffer whose other columns / rows are poison
            host = m.poison(shape, torch.float16)
            host[sl] = t
            return m.place(host)[sl]
        ks, vs = (slice(None), slice(None), slice(off, off + Cc)), (slice(None), slice(off, off + Cc))
        kt, ki = stacked((B, LP, Wd), ks, h.kt), stacked((B, LP, Wd), ks, h.ki)
        vtt, vti = stacked((B, Wd, LP), vs, h.vtt), stacked((B, Wd, LP), vs, h.vti)
        q = stacked((B, N, ldq), (slice(None), slice(None), slice(qo, qo + Cc)), h.q)
        o = m.out((B * N, Cc), ld=ldo).unflatten(0, (B, N))
        return (m.ops.masked_ip_attention(q, kt, vtt, ki, vti, bbox, h.heads, h.hw, 0.6, out=o, ip_scale_dev=sd, **kw),)
    return run


def _ip_check(rows):
    def check(o, h):
        from tests.test_gpu_masked_ip_attn import TOL, _err
        e = _err(o[0], h.ref_rows if rows else h.ref)
        assert e <= TOL, f"masked ip attn vs fp64 reference: {e:.3g} > {TOL}"       # that file's gate: 4e-3
    return check


for (B, heads, hw) in [(3, 3, (18, 13)), (1, 3, (16, 16))]:
    for v in (1, 2, 3):
        _add(f"ip-attn-B{B}-{hw[0]}x{hw[1]}-ip{v}", ["ds_masked_ip_attn_f16"], functools.partial(_ip_data, B, heads, hw), _ip_run(False),
             _ip_check(False), opts=(("ip_attn_variant", v),))
        if B > 1:
            _add(f"ip-attn-rows-B{B}-{hw[0]}x{hw[1]}-ip{v}", ["ds_masked_ip_attn_rows_f16"], functools.partial(_ip_data, B, heads, hw),
                 _ip_run(True), _ip_check(True), opts=(("ip_attn_variant", v),))
_add("ip-attn-rows-B3-16x16-ip2", ["ds_masked_ip_attn_rows_f16"], functools.partial(_ip_data, 3, 1, (16, 16)), _ip_run(True), _ip_check(True),
     opts=(("ip_attn_variant", 2),))


@functools.lru_cache(maxsize=None)
def _flags_data(hw, max_ips):
    from oracle.attention_ref import ip_region_mask
    from oracle.ip_box_cases import box_cases
    bbox = box_cases(hw[0], hw[1], max_ips, 3)
    mask = ip_region_mask(bbox, hw[0] * hw[1], 1, hw[0] / hw[1], max_ips, 1)[:, 0]
    return NS(bbox=bbox, mask=mask, hw=hw, K=max_ips)


def _flags_check(o, h):
    inside = torch.stack([(o[0] >> k) & 1 for k in range(h.K)], -1).bool()          # test_region_flags_vs_oracle: bit for bit
    assert torch.equal(inside, h.mask[:, :, 1:] == 0) and torch.equal(h.mask[:, :, 0] == 0, ~inside.any(-1))


for hw, K in [((18, 13), 4), ((7, 9), 8)]:
    _add(f"ip-region-flags-{hw[0]}x{hw[1]}-k{K}", ["ds_ip_region_flags"], functools.partial(_flags_data, hw, K),
         lambda m, h: (m.ops.ip_region_flags(m.place(h.bbox), h.hw[0] * h.hw[1], h.hw),), _flags_check)


@functools.lru_cache(maxsize=None)
def _small_attn_data(B, heads, Nq, Nk, D, causal):
    g = _g(B + heads + Nq + Nk + D)
    q, k, v = _r((B, Nq, heads * D), g), _r((B, Nk, heads * D), g), _r((B, Nk, heads * D), g)
    hs = lambda t, n: t.float().view(B, n, heads, D).transpose(1, 2)
    ref = F.scaled_dot_product_attention(hs(q, Nq), hs(k, Nk), hs(v, Nk), is_causal=causal).transpose(1, 2).reshape(B, Nq, heads * D)
    return NS(q=q, k=k, v=v, kv=torch.cat([k, v], -1), ref=ref, heads=heads, D=D)


def _small_attn_run(causal, halves):
    def run(m, h):
        q = m.place(h.q)
        if halves:                                   # k and v are the two column halves of one buffer
            kv = m.place(h.kv)
            k, v = kv[:, :, :h.k.shape[2]], kv[:, :, h.k.shape[2]:]
        else:
            k, v = m.place(h.k), m.place(h.v)
        fn = m.ops.causal_attention if causal else m.ops.small_attention
        return (fn(q, k, v, h.heads, h.D ** -0.5),)
    return run


# tests/test_gpu_ops.py::test_small_attention: 3e-3 (the causal kernel is the same loop with a key limit per row).  The causal
# entry point takes one N for queries and keys, so the (5, 77) pair runs non-causal and the causal form at N = 5 and N = 77.
for (B, heads, Nq, Nk, D), causal, halves in [((2, 4, 5, 77, 64), False, False), ((2, 4, 77, 77, 64), True, False), ((2, 4, 5, 5, 64), True, False),
                                              ((1, 2, 16, 274, 160), False, True), ((1, 2, 274, 274, 160), True, True)]:
    _add(f"small-attn-{B}x{heads}x{Nq}x{Nk}x{D}{'-causal' if causal else ''}{'-kv-halves' if halves else ''}",
         ["ds_small_attn_causal_f16" if causal else "ds_small_attn_f16"], functools.partial(_small_attn_data, B, heads, Nq, Nk, D, causal),
         _small_attn_run(causal, halves), lambda o, h: _close(o[0], h.ref, 3e-3, "small attn"))


@functools.lru_cache(maxsize=None)
def _wide_attn_data(N, n_valid, dtype):
    g = _g(N)
    q, k, v = _r((1, N, 512), g, dtype=dtype), _r((1, N, 512), g, dtype=dtype), _r((1, N, 512), g, dtype=dtype)
    scale = 1 / math.sqrt(512)
    nv = n_valid
    ref = torch.softmax(q[:, :nv].float() @ k[:, :nv].float().transpose(1, 2) * scale, -1) @ v[:, :nv].float()
    q[:, nv:], k[:, nv:], v[:, nv:] = LOUD, LOUD, LOUD                        # rows n_valid..N: the caller's padding
    return NS(q=q, k=k, vt=v.transpose(1, 2).contiguous(), ref=ref, scale=scale, nv=nv)


for dt, fn, entry, tol in ((BF, "wide_attention_bf16", "ds_wide_attn_bf16", 2e-2), (torch.float16, "wide_attention_f16", "ds_wide_attn_f16", 1e-2)):
    # tests/test_gpu_vae.py: 2e-2 (bf16), 1e-2 (f16) of max|ref|; only the rows of real queries are compared
    _add(f"wide-attn-{'bf16' if dt == BF else 'f16'}-1000-valid997", [entry], functools.partial(_wide_attn_data, 1000, 997, dt),
         lambda m, h, fn=fn: (getattr(m.ops, fn)(m.place(h.q), m.place(h.k), m.place(h.vt), h.scale, n_valid=h.nv)[:, :h.nv],),
         lambda o, h, tol=tol: _close_rel(o[0], h.ref, tol, "wide attention"))


# ------------------------------------------------------------------------------------------------ LLM decode kernels
@functools.lru_cache(maxsize=None)
def _llm_data(N, K):
    from diffsensei_amd.mllm import dequantize_rows_int8, quantize_rows_int8
    g = _g(N * 3 + K)
    x, res = _r((16, K), g), _r((16, N), g)
    w, wsw = _r((N, K), g, 1 / math.sqrt(K)), _r((2 * N, K), g, 2 / math.sqrt(K))
    gain = (1.0 + 0.3 * torch.randn(K, generator=g)).half()
    stag = lambda rows: torch.pow(2.0, (torch.arange(rows) % 7 - 3).float())[:, None]
    q, s = quantize_rows_int8(w.float() * stag(N))
    qsw, ssw = quantize_rows_int8(wsw.float() * stag(2 * N) / 8)
    out = NS(x=x, res=res, gain=gain, f16=NS(w=w, wsw=wsw, wf=w.float(), wswf=wsw.float()),
             int8=NS(w=q, s=s, wsw=qsw, ssw=ssw, wf=dequantize_rows_int8(q, s), wswf=dequantize_rows_int8(qsw, ssw)))
    for t in (out.f16, out.int8):
        xw = x.float() @ t.wf.T
        r5 = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
        r6 = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)
        xn = (gain.float() * (x.float() * r5).half().float()).half()
        t.ref = [xw, xw.half().float() + res.float(), xw * r5, xn.float() @ t.wf.T,
                 F.silu((x.float() @ t.wswf[:N].T) * r6) * ((x.float() @ t.wswf[N:].T) * r6)]
    return out


def _llm_run(kernel, wt, M):
    def run(m, h):
        t = getattr(h, wt)
        x, w, wsw, gain = m.place(h.x[:M]), m.place(t.w), m.place(t.wsw), m.place(h.gain)
        if wt == "int8":
            fn = m.ops.llm_gemv_w8 if kernel == "gemv" else m.ops.llm_gemm16_w8
            s, ssw = m.place(t.s), m.place(t.ssw)
            call = lambda wgt, sc, **kw: fn(x, wgt, sc, **kw)
        else:
            fn = m.ops.llm_gemv if kernel == "gemv" else m.ops.llm_gemm16
            s = ssw = None
            call = lambda wgt, sc, **kw: fn(x, wgt, **kw)
        y = m.place(h.res[:M])
        call(w, s, out=y, residual=y)                                                   # in place: h += x W^T
        return (call(w, s), y, call(w, s, rms=True, eps=1e-5), call(w, s, rms=True, eps=1e-5, gain=gain),
                call(wsw, ssw, rms=True, swiglu=True, eps=1e-6))
    return run


def _llm_check(wt, M):
    def check(o, h):
        # tests/test_gpu_mllm.py / test_gpu_llm_gemm16.py / test_gpu_llm_w8.py: 4e-3 plain, residual, rms; 1.5e-3 rms + gain; 6e-3 SwiGLU
        for got, ref, tol, what in zip(o, getattr(h, wt).ref, (4e-3, 4e-3, 4e-3, 1.5e-3, 6e-3),
                                       ("plain", "residual in place", "rms", "rms + gain", "swiglu")):
            _close_rel(got, ref[:M], tol, f"llm {wt} {what}")
    return check


LLM_ENTRY = {("gemv", "f16"): "ds_llm_gemv_f16", ("gemv", "int8"): "ds_llm_gemv_w8", ("gemm16", "f16"): "ds_llm_gemm16",
             ("gemm16", "int8"): "ds_llm_gemm16_w8"}
for (N, K) in [(520, 704), (520, 720)]:
    for M in (1, 5, 16):
        for (kernel, wt), entry in LLM_ENTRY.items():
            variants = ((0, 1, 2) if wt == "f16" else (0, 1)) if kernel == "gemv" else (0,)
            for v in variants:
                _add(f"llm-{kernel}-{wt}-{M}x{N}x{K}-v{v}", [entry], functools.partial(_llm_data, N, K), _llm_run(kernel, wt, M),
                     _llm_check(wt, M), opts=(("llm_gemv_variant", v),) if v else ())

_add("llm-dequant-w8-37x720", ["ds_llm_dequant_w8"], functools.partial(_llm_data, 520, 720),
     lambda m, h: (m.ops.llm_dequant_w8(m.place(h.int8.w[:37]), m.place(h.int8.s[:37])),),
     lambda o, h: torch.equal(o[0], (h.int8.w[:37].float() * h.int8.s[:37, None]).half()) or pytest.fail("dequant is one multiply, one rounding"))


def _rope(T_max, D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(T_max).float(), inv)
    return fr.cos().contiguous(), fr.sin().contiguous()


@functools.lru_cache(maxsize=None)
def _llm_attn_data(D, heads, kv, pos0, M, T_max=40):
    from tests._llm_attn_ref import attention_ref, split_qkv
    g = _g(D + heads + pos0 + M)
    qkv = _r((pos0 + M, (heads + 2 * kv) * D), g)
    ref, kr = attention_ref(qkv, D, heads, kv, pos0, M)
    cos, sin = _rope(T_max, D)
    _, _, v = split_qkv(qkv, D, heads, kv)
    return NS(qkv=qkv, ref=ref, kr=kr.reshape(pos0 + M, kv * D), v=v.reshape(pos0 + M, kv * D), cos=cos, sin=sin,
              dims=(D, heads, kv, pos0, M, T_max))


def _untouched(m, *tails):
    """cache rows past the sequence are part of the placed operand, so `check()` does not see them: they must still hold
    what `m.poison` put there (zeros on ordinary tensors), compared through an integer view"""
    torch.cuda.synchronize()
    for t in tails:
        want = 0 if m.plain else m.pattern(torch.float16)
        assert bool((t.contiguous().view(torch.int16) == want).all()), "rows past the cache length were written"


def _llm_attn_run(m, h):
    D, heads, kv, pos0, M, T_max = h.dims
    kc, vc = m.poison((T_max, kv * D), torch.float16), m.poison((T_max, kv * D), torch.float16)   # rows >= pos0: unwritten memory
    kc[:pos0], vc[:pos0] = h.kr[:pos0].half(), h.v[:pos0]
    kc, vc = m.place(kc), m.place(vc)
    state = m.place(torch.tensor([pos0, 0, 0, 0, 9, 2, 0, 0], dtype=torch.int32))
    out = m.ops.llm_attention(m.place(h.qkv[pos0:]), kc, vc, m.place(h.cos), m.place(h.sin), state, heads, kv, 1.0 / math.sqrt(D))
    m.ops.llm_advance(state, M)
    _untouched(m, kc[pos0 + M:], vc[pos0 + M:])
    return (out, kc[:pos0 + M], vc[:pos0 + M], state)


def _llm_attn_check(o, h):
    # tests/test_gpu_mllm.py::test_llm_attention_chunks_and_tokens: rows 4e-3, rotated keys 2e-3, values a bit copy
    D, heads, kv, pos0, M, T_max = h.dims
    _close_rel(o[0], h.ref, 4e-3, "llm attention rows")
    _close_rel(o[1], h.kr, 2e-3, "rotated key cache")
    assert torch.equal(o[2], h.v), "value cache must be a bit copy"
    assert o[3].tolist() == [pos0 + M, 0, 0, 0, 9, 2, 0, 0]


for (D, heads, kv, pos0, M) in [(128, 3, 3, 19, 5), (64, 4, 2, 23, 1), (128, 3, 3, 0, 16)]:
    _add(f"llm-attn-D{D}-h{heads}-kv{kv}-pos{pos0}-M{M}", ["ds_llm_attn_f16", "ds_llm_advance"],
         functools.partial(_llm_attn_data, D, heads, kv, pos0, M), _llm_attn_run, _llm_attn_check)

SLOT_LENS, SLOT_FIN = (0, 7, 23), (0, 1, 0)


@functools.lru_cache(maxsize=None)
def _llm_attn_slots_data(D, heads, kv, T_max=40):
    from tests._llm_attn_ref import attention_ref, split_qkv
    g = _g(D * 3 + heads)
    hist, refs, krs, vs = [], [], [], []
    for n in SLOT_LENS:
        qkv = _r((n + 1, (heads + 2 * kv) * D), g)
        ref, kr = attention_ref(qkv, D, heads, kv, n, 1)
        hist.append(qkv), refs.append(ref[0]), krs.append(kr.reshape(n + 1, kv * D)), vs.append(split_qkv(qkv, D, heads, kv)[2].reshape(n + 1, kv * D))
    cos, sin = _rope(T_max, D)
    return NS(hist=hist, refs=refs, krs=krs, vs=vs, cos=cos, sin=sin, dims=(D, heads, kv, T_max))


def _llm_attn_slots_run(m, h):
    D, heads, kv, T_max = h.dims
    S = len(SLOT_LENS)
    kc, vc = m.poison((S, T_max, kv * D), torch.float16), m.poison((S, T_max, kv * D), torch.float16)
    for s, n in enumerate(SLOT_LENS):
        kc[s, :n], vc[s, :n] = h.krs[s][:n].half(), h.vs[s][:n]
    kc, vc = m.place(kc), m.place(vc)
    state = m.place(torch.tensor([[SLOT_LENS[s], 1, SLOT_FIN[s], 0, 9, 2, 0, 0] for s in range(S)], dtype=torch.int32))
    out = m.place(torch.full((S, heads * D), 7.0, dtype=torch.float16))       # a finished slot's row is left alone
    m.ops.llm_attention_slots(m.place(torch.stack([q[-1] for q in h.hist])), kc, vc, m.place(h.cos), m.place(h.sin), state, heads, kv,
                              1.0 / math.sqrt(D), out=out)
    rows = [n + (0 if SLOT_FIN[s] else 1) for s, n in enumerate(SLOT_LENS)]
    _untouched(m, *[c[s, r:] for c in (kc, vc) for s, r in enumerate(rows)])
    return (out, state) + tuple(c[s, :r] for c in (kc, vc) for s, r in enumerate(rows))      # views: each slot's live cache rows


def _llm_attn_slots_check(o, h):
    # tests/test_gpu_llm_batch_kernels.py::test_attention_slots: rows 4e-3, rotated keys 2e-3, values a bit copy, finished slot untouched
    S = len(SLOT_LENS)
    out, state, kcs, vcs = o[0], o[1], o[2:2 + S], o[2 + S:]
    for s, n in enumerate(SLOT_LENS):
        rows = n + (0 if SLOT_FIN[s] else 1)
        if SLOT_FIN[s]:
            assert bool((out[s] == 7.0).all()), "a finished slot's output row was written"
        else:
            _close_rel(out[s], h.refs[s], 4e-3, f"attention slot {s}")
            _close_rel(kcs[s], h.krs[s], 2e-3, f"rotated key cache slot {s}")
        assert kcs[s].shape[0] == rows and torch.equal(vcs[s], h.vs[s][:rows]), "value cache must be a bit copy"
    assert state.tolist() == [[SLOT_LENS[s], 1, SLOT_FIN[s], 0, 9, 2, 0, 0] for s in range(S)]


for (D, heads, kv) in [(128, 3, 3), (64, 4, 2)]:
    _add(f"llm-attn-slots-D{D}-h{heads}-kv{kv}", ["ds_llm_attn_slots_f16"], functools.partial(_llm_attn_slots_data, D, heads, kv),
         _llm_attn_slots_run, _llm_attn_slots_check)


@functools.lru_cache(maxsize=None)
def _rms_data(S, H):
    g = _g(3 + S + H)
    x, gam = _r((S, H), g, 3.0), (1 + 0.1 * torch.randn(H, generator=g)).half()
    ref = gam.float() * (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)).half().float()
    table = _r((640, H), g)
    table[1], table[2] = float("nan"), float("nan")          # the rows the in-range poison around the state block points at
    return NS(x=x, gam=gam, ref=ref, table=table, H=H)


def _rms_run(m, h):
    x, gam = m.place(h.x), m.place(h.gam)
    feat = m.place(torch.zeros(4, h.H, dtype=torch.float16))
    state = m.place(torch.tensor([0, 3, 0, 17, 9, 2, 0, 0], dtype=torch.int32))             # 3 ids out -> feature row 2
    y1 = m.ops.llm_rmsnorm(x[:1], gam, 1e-6, feat=feat, state=state)
    emb = m.place(torch.zeros(1, h.H, dtype=torch.float16))
    m.ops.llm_embed(m.place(h.table), state, emb)
    return (m.ops.llm_rmsnorm(x, gam, 1e-6), y1, feat, emb)


def _rms_check(o, h):
    # tests/test_gpu_mllm.py::test_llm_rmsnorm_and_feature_tap: 2e-3; the tap and the embedding are bit copies
    _close_rel(o[0], h.ref, 2e-3, "rmsnorm")
    assert torch.equal(o[1], o[0][:1]) and torch.equal(o[2][2], o[1][0]) and not o[2][[0, 1, 3]].any()
    assert torch.equal(o[3][0], h.table[17])


_add("llm-rmsnorm-embed-5x512", ["ds_llm_rmsnorm_f16", "ds_llm_embed_f16"], functools.partial(_rms_data, 5, 512), _rms_run, _rms_check)

RMS_SLOT_STATE = [[0, 3, 0, 4, 9, 2, 0, 0], [5, 1, 0, 17, 9, 2, 0, 0], [2, 2, 1, 600, 9, 2, 0, 0]]


def _rms_slots_run(m, h):
    x, gam = m.place(h.x), m.place(h.gam)
    feat = m.place(torch.zeros(3, 4, h.H, dtype=torch.float16))
    state = m.place(torch.tensor(RMS_SLOT_STATE, dtype=torch.int32))
    y = m.ops.llm_rmsnorm_slots(x, gam, 1e-6, feat=feat, state=state)
    emb = m.place(torch.zeros(3, h.H, dtype=torch.float16))
    m.ops.llm_embed_slots(m.place(h.table), state, emb)
    return (y, feat, emb)


def _rms_slots_check(o, h):
    # tests/test_gpu_llm_batch_kernels.py::test_rmsnorm_slots_feature_tap_and_embed: 2e-3; taps and embeddings bit copies
    _close_rel(o[0], h.ref, 2e-3, "rmsnorm slots")
    assert torch.equal(o[1][0, 2], o[0][0]) and not o[1][0, [0, 1, 3]].any() and torch.equal(o[1][1, 0], o[0][1]) and not o[1][1, 1:].any()
    assert not o[1][2].any(), "a finished slot writes no feature row"
    assert torch.equal(o[2][:2], h.table[[4, 17]])


_add("llm-rmsnorm-embed-slots-3x512", ["ds_llm_rmsnorm_slots_f16", "ds_llm_embed_slots_f16"], functools.partial(_rms_data, 3, 512),
     _rms_slots_run, _rms_slots_check)


@functools.lru_cache(maxsize=None)
def _select_data():
    g = _g(0)
    V = 3000
    base = -torch.rand(V, generator=g) - 0.5
    tie = base.clone(); tie[1234] = 0.0; tie[77] = 0.0
    lg = base.clone(); lg[2000] = 4.0; lg[2902] = 9.0
    return NS(logits=torch.stack([base, tie, lg]).half(), chain=torch.tensor([2900, 2901, 2902, 2903], dtype=torch.int32), V=V)


SELECT_STATE = [[10, 0, 0, 5, 8, 2, 0, 0], [11, 0, 0, 5, 8, 2, 0, 0], [12, 4, 1, 5, 8, 2, 0, 0]]


def _select_run(slots):
    def run(m, h):
        chain = m.place(h.chain)
        if slots:                                     # ldl > V: the columns behind each row are poison
            ldl = h.V + 40
            wide = m.poison((3, ldl), torch.float16)
            wide[:, :h.V] = h.logits
            logits = m.place(wide)[:, :h.V]
            state = m.place(torch.tensor(SELECT_STATE, dtype=torch.int32))
            ids = m.place(torch.full((3, 8), -1, dtype=torch.int32))
            from diffsensei_amd import _lib as L, ops
            L.check(_lib().ds_llm_select_slots_f16(logits.data_ptr(), ldl, h.V, chain.data_ptr(), 4, 8, 1, state.data_ptr(), ids.data_ptr(),
                                                   3, ops._stream()), "ds_llm_select_slots_f16")
            return (state, ids)
        outs = []
        for s in range(3):
            state = m.place(torch.tensor(SELECT_STATE[s], dtype=torch.int32))
            ids = m.place(torch.full((8,), -1, dtype=torch.int32))
            m.ops.llm_select(m.place(h.logits[s]), chain, 1, state, ids)
            outs += [state, ids]
        return tuple(outs)
    return run


def _select_check(slots):
    def check(o, h):
        # the semantics asserted by test_select_slots_match_the_one_slot_kernel: image ids zeroed -> lowest wins; ties -> lowest id
        state = o[0] if slots else torch.stack(list(o[0::2]))
        ids = o[1] if slots else torch.stack(list(o[1::2]))
        assert state.tolist() == [[11, 1, 0, 2901, 8, 2, 0, 0], [12, 1, 0, 77, 8, 2, 0, 0], [12, 4, 1, 5, 8, 2, 0, 0]]
        assert ids[0, 0] == 2901 and ids[1, 0] == 77 and bool((ids[2] == -1).all()) and bool((ids[:2, 1:] == -1).all())
    return check


_add("llm-select", ["ds_llm_select_f16"], _select_data, _select_run(False), _select_check(False))
_add("llm-select-slots-ldl", ["ds_llm_select_slots_f16"], _select_data, _select_run(True), _select_check(True))


@functools.lru_cache(maxsize=None)
def _swiglu_blend_data():
    g = _g(5)
    return NS(gu=_r((7, 2 * 704), g, 2.0), a=_r((4, 16, 64), g), b=_r((4, 16, 64), g))


# tests/test_gpu_mllm.py::test_llm_swiglu / test_blend: 2e-3
_add("llm-swiglu-7x704", ["ds_llm_swiglu_f16"], _swiglu_blend_data, lambda m, h: (m.ops.llm_swiglu(m.place(h.gu)),),
     lambda o, h: _close_rel(o[0], F.silu(h.gu[:, :704].float()) * h.gu[:, 704:].float(), 2e-3, "swiglu"))
_add("blend-4x16x64", ["ds_blend_f16"], _swiglu_blend_data, lambda m, h: (m.ops.blend(m.place(h.a), m.place(h.b), 0.3),),
     lambda o, h: _close_rel(o[0], h.a.float() * 0.3 + h.b.float() * 0.7, 2e-3, "blend"))


# ------------------------------------------------------------------------------------------------ UNet head, tail, embeddings
@functools.lru_cache(maxsize=None)
def _conv_in_out_data(B=2, H=9, W=13, Cc=64):
    g = _g(11)
    x, w, b, emb = _r((B, 4, H, W), g), _r((Cc, 4, 3, 3), g, 1 / 6), _r((Cc,), g), _r((Cc,), g)
    boxes = torch.tensor([[[1, 2, 9, 7], [5, 5, 13, 9], [0, 0, 0, 0]], [[0, 0, 0, 0]] * 3], dtype=torch.int32)
    ref = F.conv2d(x.float(), w.float(), b.float(), padding=1).half().float()
    mask = torch.zeros(B, 1, H, W)
    for i in range(B):
        for (x1, y1, x2, y2) in boxes[i].tolist():
            mask[i, :, y1:y2, x1:x2] = 1
    ref = ref + mask * emb.float()[None, :, None, None]
    xo, wo, bo = _r((B, Cc, H, W), g), _r((4, Cc, 3, 3), g, 1 / math.sqrt(9 * Cc)), _r((4,), g)
    return NS(x=_nhwc(x), w=_nhwc(w), b=b, emb=emb, boxes=boxes, ref=ref, xo=_nhwc(xo), wo=_nhwc(wo), bo=bo,
              refo=F.conv2d(xo.float(), wo.float(), bo.float(), padding=1))


# tests/test_gpu_ops.py::test_conv_in_dialog_and_conv_out: 1e-3 (conv_in + dialog), 2e-3 (conv_out)
_add("conv-in-dialog-2x9x13", ["ds_conv_in_dialog_f16"], _conv_in_out_data,
     lambda m, h: (m.ops.conv_in_dialog(m.place(h.x), m.place(h.w), m.place(h.b), m.place(h.boxes), m.place(h.emb)),),
     lambda o, h: _close(_nchw(o[0]), h.ref, 1e-3, "conv_in + dialog"))
_add("conv-out-2x9x13", ["ds_conv_out_f16"], _conv_in_out_data, lambda m, h: (m.ops.conv_out(m.place(h.xo), m.place(h.wo), m.place(h.bo)),),
     lambda o, h: _close(_nchw(o[0]), h.refo, 2e-3, "conv_out"))


@functools.lru_cache(maxsize=None)
def _skinny_data(M=5, N=13, K=72):
    g = _g(31)
    x, w, b, add = _r((M, K), g), _r((N, K), g, 1 / math.sqrt(K)), _r((N,), g), _r((M, N), g)
    return NS(x=x, w=w, b=b, add=add, ref=(F.silu(x.float()).half().float() @ w.float().t() + b.float()).half().float() + add.float(),
              ref2=F.silu((x.float() @ w.float().t() + b.float()).half().float()))


# tests/test_gpu_ops.py::test_time_embedding_chain: 2e-3 for every piece
_add("skinny-linear-5x13x72", ["ds_skinny_linear_f16"], _skinny_data,
     lambda m, h: (m.ops.skinny_linear(m.place(h.x), m.place(h.w), m.place(h.b), m.place(h.add), silu_in=True),
                   m.ops.skinny_linear(m.place(h.x), m.place(h.w), m.place(h.b), silu_out=True)),
     lambda o, h: (_close(o[0], h.ref, 2e-3, "skinny linear"), _close(o[1], h.ref2, 2e-3, "skinny silu_out")))


@functools.lru_cache(maxsize=None)
def _time_data(B=3):
    from oracle.unet_ref import timestep_sinusoid
    g = _g(31)
    table = torch.zeros(2, 8)
    table[0, 0], table[1, 0] = 981.0, 41.0
    te, tid = _r((B, 1280), g), torch.tensor([[1024, 768, 0, 0, 1024, 768]] * B).half()
    return NS(table=table, te=te, tid=tid, B=B, ref=timestep_sinusoid(torch.full((B,), 41.0), 320),
              ref_ids=torch.cat([te.float(), timestep_sinusoid(tid.float().flatten(), 256).reshape(B, -1)], -1))


_add("timestep-embed-3x320", ["ds_timestep_embed_f16"], _time_data,
     lambda m, h: (m.ops.timestep_embed(m.place(h.table), h.B, 320, ctr=m.place(torch.tensor([1], dtype=torch.int32))),),
     lambda o, h: _close(o[0], h.ref, 2e-3, "sinusoid"))
_add("add-time-ids-3", ["ds_add_time_ids_f16"], _time_data, lambda m, h: (m.ops.add_time_ids(m.place(h.te), m.place(h.tid), 256),),
     lambda o, h: _close(o[0], h.ref_ids, 2e-3, "add_time_ids"))


# ------------------------------------------------------------------------------------------------ sampler steps (ns = 2, HW = 35)
NS_, SH, SW, NSTEP, GS = 2, 5, 7, 10, 5.0
SDXL = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, timestep_spacing="leading")
SEEDS = [12345, 2 ** 62 + 3]
hq = lambda t: t.half().float()


@functools.lru_cache(maxsize=None)
def _step_data(kind, step, per_panel=False, redraw=False):
    """One step of sampler `kind` at row `step` of a 10-step schedule against the restatements the sampler tests use
    (oracle/scheduler_ref.py, tests/_dpm_ref.py, tests/_euler_a_ref.py, tests/_redraw_ref.py)."""
    from diffsensei_amd import schedulers as S
    from oracle.scheduler_ref import DDIMOracle, EulerDiscreteOracle
    from tests import _redraw_ref as R
    from tests._dpm_ref import DPMSolverOracle
    from tests._euler_a_ref import EulerAncestralOracle
    cls = {0: S.EulerDiscreteScheduler, 1: S.DDIMScheduler, 2: S.DPMSolverMultistepScheduler, 3: S.EulerAncestralDiscreteScheduler}[kind]
    sch = cls(**SDXL)
    sch.set_timesteps(NSTEP)
    orc = {0: EulerDiscreteOracle, 1: DDIMOracle, 2: DPMSolverOracle, 3: lambda: EulerAncestralOracle(seeds=SEEDS)}[kind]().set_timesteps(NSTEP)
    g = _g(41 + kind + step)
    lat = (_r((NS_, 4, SH, SW), g) * 3).contiguous()
    eps = _r((2 * NS_, 4, SH, SW), g, 0.5)
    prev = _r((NS_, 4, SH, SW), g)
    guidance = torch.tensor([3.0, 6.5]) if per_panel else None
    u, c = eps.float().chunk(2)
    gs = guidance.view(NS_, 1, 1, 1) if per_panel else GS
    e = hq(u + hq(gs * hq(c - u)))
    if kind == 2:
        orc.prev_x0 = prev.float()
    x_new = hq(orc.step(e, step, lat.float()))
    table = torch.from_numpy(sch.coef_table(GS)).float()
    out = NS(kind=kind, step=step, lat=lat, eps=eps.permute(0, 2, 3, 1).reshape(2 * NS_, SH * SW, 4).contiguous(), prev=prev, table=table,
             solver=torch.from_numpy(sch.solver_table()).float() if kind == 2 else None, guidance=guidance,
             seeds=torch.tensor(SEEDS, dtype=torch.int64), ref=x_new, prev_ref=orc.prev_x0 if kind == 2 else None)
    if redraw:
        rows = sch.renoise_table()
        x0, noise = _r((NS_, 4, SH, SW), g), _r((NS_, 4, SH, SW), g)
        mask = torch.stack([R.mask_from_boxes([[0.25, 0.25, 0.8, 1.0]], SH, SW), torch.linspace(0, 1, SH * SW).reshape(SH, SW).half().float()])
        out.rd = NS(x0=x0, noise=noise, mask=mask, rows=torch.from_numpy(rows), init_sigma=float(sch.init_noise_sigma))
        out.ref = R.blend(x_new, x0, noise, mask, *rows[step + 1])
        out.start_ref = R.known(x0, noise, *rows[0])
    out.model_in_ref = hq(out.ref / float(table[step, 6]))
    return out


def _redraw_buffer(m, h):
    """the packed redraw buffer (include/diffsensei_hip.h "Region redraw") built on the host, then placed as one operand"""
    from diffsensei_amd import ops
    n = int(_lib().ds_redraw_buffer_bytes(NS_, SH * SW))
    host = torch.zeros(n, dtype=torch.uint8)
    vx, vn, vm, hdr, vr = _redraw_views_host(host)
    vx.copy_(h.rd.x0), vn.copy_(h.rd.noise), vm.copy_(h.rd.mask.half())
    hdr.copy_(torch.tensor([0.0, h.rd.init_sigma, 0.0, 0.0]))
    vr[:h.rd.rows.shape[0]].copy_(h.rd.rows.float())
    assert ops.REDRAW_MAX_ROWS == vr.shape[0]
    return m.place(host)


def _redraw_views_host(buf):
    n4, HW = NS_ * 4 * SH * SW, SH * SW
    off = (18 * NS_ * HW + 15) & ~15
    half, f32 = buf[:18 * NS_ * HW].view(torch.float16), buf[off:].view(torch.float32)
    return half[:n4].view(NS_, 4, SH, SW), half[n4:2 * n4].view(NS_, 4, SH, SW), half[2 * n4:].view(NS_, SH, SW), f32[:4], f32[4:].view(-1, 2)


def _step_run(entry):
    def run(m, h):
        eps, lat, table = m.place(h.eps), m.place(h.lat), m.place(h.table)
        xin = m.out((2 * NS_, SH * SW, 4))
        ctr = m.place(torch.tensor([h.step], dtype=torch.int32))
        guidance = None if h.guidance is None else m.place(h.guidance)
        solver, prev = (m.place(h.solver), m.place(h.prev)) if h.kind == 2 else (None, None)
        seeds = m.place(h.seeds) if h.kind == 3 else None
        if entry == "ds_cfg_sampler_step_f16":
            m.ops.cfg_sampler_step(eps, lat, xin, table, h.kind, True, ctr)
        elif entry == "ds_cfg_dpm_step_f16":
            m.ops.cfg_dpm_step(eps, lat, xin, table, solver, prev, True, ctr)
        elif entry == "ds_cfg_sampler_step_noise_f16":
            m.ops.cfg_sampler_step_noise(eps, lat, xin, table, seeds, h.kind, True, ctr)
        elif entry == "ds_cfg_sampler_step_panels_f16":
            if h.kind == 2:
                m.ops.cfg_dpm_step(eps, lat, xin, table, solver, prev, True, ctr, guidance=guidance)
            elif h.kind == 3:
                m.ops.cfg_sampler_step_noise(eps, lat, xin, table, seeds, 3, True, ctr, guidance=guidance)
            else:
                m.ops.cfg_sampler_step(eps, lat, xin, table, h.kind, True, ctr, guidance=guidance)
        else:
            m.ops.cfg_sampler_step_redraw(eps, lat, xin, table, _redraw_buffer(m, h), h.kind, True, ctr, guidance=guidance, solver=solver,
                                          prev_x0=prev, seeds=seeds)
        return (lat, xin) + ((prev,) if h.kind == 2 else ())
    return run


def _step_check(o, h):
    # tests/test_gpu_ops.py::test_cfg_sampler_step, tests/test_gpu_dpm.py, tests/test_gpu_euler_ancestral.py: 1.5e-3 per step
    _close(o[0], h.ref, 1.5e-3, f"kind {h.kind} step {h.step}")
    got = o[1].view(2 * NS_, SH, SW, 4).permute(0, 3, 1, 2)
    if h.step + 1 < NSTEP:                                     # (the last row has no next model input to scale for)
        _close(got[:NS_], h.model_in_ref, 1.5e-3, "next model input")
    assert torch.equal(got[NS_:], got[:NS_])
    if h.kind == 2:
        _close(o[2], h.prev_ref, 1.5e-3, "prev_x0")


for entry, combos in [("ds_cfg_sampler_step_f16", [(0, 4), (1, 4), (0, NSTEP - 1)]), ("ds_cfg_dpm_step_f16", [(2, 0), (2, 3)]),
                      ("ds_cfg_sampler_step_noise_f16", [(3, 4), (0, 4)])]:
    for kind, step in combos:
        _add(f"sampler-{entry[3:-4]}-kind{kind}-step{step}", [entry], functools.partial(_step_data, kind, step), _step_run(entry), _step_check)
for kind in (0, 1, 2, 3):
    _add(f"sampler-panels-kind{kind}", ["ds_cfg_sampler_step_panels_f16"], functools.partial(_step_data, kind, 3, True),
         _step_run("ds_cfg_sampler_step_panels_f16"), _step_check)
    for per_panel in (False, True):
        _add(f"sampler-redraw-kind{kind}{'-panels' if per_panel else ''}", ["ds_cfg_sampler_step_redraw_f16", "ds_redraw_buffer_bytes"],
             functools.partial(_step_data, kind, 3, per_panel, True), _step_run("ds_cfg_sampler_step_redraw_f16"), _step_check)


def _redraw_start_check(o, h):
    from tests import _redraw_ref as R
    assert int(R.ulp16(o[0], h.start_ref).max()) <= 1          # tests/test_gpu_redraw.py::test_redraw_start: one contraction


_add("redraw-start", ["ds_redraw_start_f16"], functools.partial(_step_data, 0, 3, False, True),
     lambda m, h: (lambda lat: (m.ops.redraw_start(_redraw_buffer(m, h), lat), lat)[1:])(m.out((NS_, 4, SH, SW))), _redraw_start_check)
_add("prepare-model-input", ["ds_prepare_model_input_f16"], functools.partial(_step_data, 0, 4),
     lambda m, h: (lambda xin: (m.ops.prepare_model_input(m.place(h.lat), xin, m.place(h.table), True,
                                                          m.place(torch.tensor([h.step], dtype=torch.int32))), xin)[1:])(m.out((2 * NS_, SH * SW, 4))),
     lambda o, h: (_close(o[0].view(2 * NS_, SH, SW, 4).permute(0, 3, 1, 2)[:NS_], hq(h.lat.float() / float(h.table[h.step, 1])), 1.5e-3,
                          "scale_model_input"), None)[1])


def _philox_check_u32(o, h):
    from tests._philox_ref import philox_u32
    assert np.array_equal(o[0].numpy().view(np.uint32), philox_u32(SEEDS, 3, 0, 35))     # test_philox_u32_bit_exact


def _philox_check_normal(o, h):
    from tests._philox_ref import philox_normal
    # tests/test_gpu_euler_ancestral.py::test_philox_normal_vs_restatement_and_moments: the hard condition 1e-3, its gate 2e-6
    assert float(np.abs(o[0].numpy() - philox_normal(SEEDS, 3, 0, 35)).max()) <= 2.0e-6


_seeds = lambda: NS(seeds=torch.tensor(SEEDS, dtype=torch.int64))
_add("philox-u32", ["ds_philox_u32"], _seeds, lambda m, h: (m.ops.philox_u32(m.place(h.seeds), 3, 35),), _philox_check_u32)
_add("philox-normal", ["ds_philox_normal_f32"], _seeds, lambda m, h: (m.ops.philox_normal(m.place(h.seeds), 3, 35),), _philox_check_normal)


# ------------------------------------------------------------------------------------------------ layout helpers, embeddings, images
@functools.lru_cache(maxsize=None)
def _layout_data():
    g = _g(51)
    tok = _r((90, 72), g)
    tok[1], tok[2] = float("nan"), float("nan")              # what the poison around the ids points at
    ids = torch.randint(3, 90, (2, 11), generator=g, dtype=torch.int32)
    img = torch.rand((2, 3, 6, 10), generator=g)
    img[0, 0, 0, :10] = (torch.arange(10, dtype=torch.float32) + 0.5) / 255.0            # .5 ties
    return NS(x=_r((3, 35, 4), g), wide=_r((2, 50, 72), g), e=_r((2, 157, 64), g), tok=tok, pos=_r((16, 72), g), ids=ids, img=img)


_add("nhwc-to-nchw-3x35x4", ["ds_nhwc_to_nchw_f16"], _layout_data, lambda m, h: (m.ops.nhwc_to_nchw(m.place(h.x)),),
     lambda o, h: torch.equal(o[0], h.x.permute(0, 2, 1).contiguous()) or pytest.fail("nhwc -> nchw"))
_add("nhwc-to-nchw-2x50x72", ["ds_nhwc_to_nchw_f16"], _layout_data, lambda m, h: (m.ops.nhwc_to_nchw(m.place(h.wide)),),
     lambda o, h: torch.equal(o[0], h.wide.permute(0, 2, 1).contiguous()) or pytest.fail("nhwc -> nchw"))
_add("nchw-to-nhwc-3x4x35", ["ds_nchw_to_nhwc_f16"], _layout_data, lambda m, h: (m.ops.nchw_to_nhwc(m.place(h.x.permute(0, 2, 1))),),
     lambda o, h: torch.equal(o[0], h.x) or pytest.fail("nchw -> nhwc"))
_add("nchw-to-nhwc-2x72x50", ["ds_nchw_to_nhwc_f16"], _layout_data, lambda m, h: (m.ops.nchw_to_nhwc(m.place(h.wide.permute(0, 2, 1))),),
     lambda o, h: torch.equal(o[0], h.wide) or pytest.fail("nchw -> nhwc"))
_add("pad-rows-157-to-96", ["ds_pad_rows_f16"], _layout_data, lambda m, h: (m.ops.pad_rows(m.place(h.e), 77, 80, 96),),
     lambda o, h: (torch.equal(o[0][:, :80], h.e[:, 77:]) and not o[0][:, 80:].any()) or pytest.fail("pad_rows"))
# out = tok[ids] + pos: one fp16 rounding of an exact fp32 sum (4.9e-4 relative) -> the 2e-3 rule of tests/test_gpu_ops.py
_add("embed-tokens-2x11x72", ["ds_embed_tokens_f16"], _layout_data,
     lambda m, h: (m.ops.embed_tokens(m.place(h.ids), m.place(h.tok), m.place(h.pos)),),
     lambda o, h: _close(o[0], h.tok[h.ids.long()].float() + h.pos[:11].float(), 2e-3, "embed_tokens"))
_add("image-to-u8-6x10", ["ds_image_f32_to_u8_nhwc"], _layout_data, lambda m, h: (m.ops.image_to_u8(m.place(h.img)),),
     lambda o, h: (o[0].numpy() == (h.img.permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")).all() or pytest.fail("image -> u8"))


# ------------------------------------------------------------------------------------------------ VAE stem and head kernels
@functools.lru_cache(maxsize=None)
def _vae_data(dtype, B=2, H=9, W=13, Cc=128):
    from diffsensei_amd.vae import fold_quant_conv
    g = _g(9)
    lat = torch.randn(B, 4, H, W, generator=g)
    pqw, pqb = torch.randn(4, 4, generator=g) * 0.5, torch.randn(4, generator=g) * 0.1
    w, b = _r((Cc, 4, 3, 3), g, 1 / 6.0, dtype), _r((Cc,), g, dtype=dtype)
    sf = 0.13025
    ref_in = F.conv2d(F.conv2d(lat / sf, pqw.view(4, 4, 1, 1), pqb), w.float(), b.float(), padding=1)
    x = _r((B, Cc, H, W), g, dtype=dtype)
    wo, bo = _r((3, Cc, 3, 3), g, 1 / math.sqrt(9 * Cc), dtype), _r((3,), g, dtype=dtype)
    ref_out = F.conv2d(x.float(), wo.float(), bo.float(), padding=1)
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    xn = (u8.float() * 2.0 / 255.0 - 1.0).permute(0, 3, 1, 2).contiguous()
    we, be = (torch.randn(Cc, 3, 3, 3, generator=g) / math.sqrt(27)).to(dtype), (torch.randn(Cc, generator=g) * 0.3).to(dtype)
    ref_enc_in = F.conv2d(xn, we.float(), be.float(), padding=1)
    wc, bc = torch.randn(8, Cc, 3, 3, generator=g) / math.sqrt(9 * Cc), torch.randn(8, generator=g) * 0.1
    wq, bq = torch.randn(8, 8, 1, 1, generator=g) * 0.5, torch.randn(8, generator=g) * 0.1
    wq[4:] *= 25.0
    w2, b2 = fold_quant_conv(wc, bc, wq, bq)
    w2 = w2.to(dtype)
    raw = F.conv2d(x.float(), w2.float(), b2, padding=1)
    ref_enc_out = torch.cat([raw[:, :4], raw[:, 4:].clamp(-30.0, 20.0)], dim=1)
    return NS(lat=lat, pqw=pqw, pqb=pqb, w=_nhwc(w), b=b, sf=sf, ref_in=ref_in, x=_nhwc(x), wo=_nhwc(wo), bo=bo, ref_out=ref_out, u8=u8, xn=xn,
              we=_nhwc(we), be=be, ref_enc_in=ref_enc_in, w2=_nhwc(w2), b2=b2.float(), ref_enc_out=ref_enc_out)


for dt, tag, tol in ((torch.float16, "f16", 2e-3), (BF, "bf16", 1e-2)):
    # tests/test_gpu_vae.py::test_vae_conv_in_out (bf16 output: 1e-2; fp32 image out of conv_out: 2e-3), tests/test_gpu_vae_encode_ops.py
    # (2e-3 f16, 1e-2 bf16); the f16 twins of the decoder's stem round to f16, the 2e-3 of tests/test_gpu_ops.py
    _add(f"vae-conv-in-{tag}", [f"ds_vae_conv_in_{tag}"], functools.partial(_vae_data, dt),
         lambda m, h: (m.ops.vae_conv_in(m.place(h.lat), m.place(h.pqw), m.place(h.pqb), m.place(h.w), m.place(h.b), h.sf),),
         lambda o, h, tol=tol: _close_rel(_nchw(o[0]), h.ref_in, tol, "post_quant + conv_in"))
    _add(f"vae-conv-out-{tag}", [f"ds_vae_conv_out_{tag}"], functools.partial(_vae_data, dt),
         lambda m, h: (m.ops.vae_conv_out(m.place(h.x), m.place(h.wo), m.place(h.bo)),
                       m.ops.vae_conv_out(m.place(h.x), m.place(h.wo), m.place(h.bo), denormalize=True)),
         lambda o, h: (_close_rel(o[0], h.ref_out, 2e-3, "conv_out"), _close_rel(o[1], (h.ref_out / 2 + 0.5).clamp(0, 1), 2e-3, "denorm")))
    _add(f"vae-enc-conv-in-{tag}", [f"ds_vae_enc_conv_in_{tag}"], functools.partial(_vae_data, dt),
         lambda m, h: (m.ops.vae_enc_conv_in(m.place(h.u8), m.place(h.we), m.place(h.be)),
                       m.ops.vae_enc_conv_in(m.place(h.xn), m.place(h.we), m.place(h.be))),
         lambda o, h, tol=tol: (_close_rel(_nchw(o[0]), h.ref_enc_in, tol, "enc conv_in uint8"),
                                _close_rel(_nchw(o[1]), h.ref_enc_in, tol, "enc conv_in fp32")))
    _add(f"vae-enc-conv-out-{tag}", [f"ds_vae_enc_conv_out_{tag}"], functools.partial(_vae_data, dt),
         lambda m, h: (m.ops.vae_enc_conv_out(m.place(h.x), m.place(h.w2), m.place(h.b2)),),
         lambda o, h, tol=tol: (_close_rel(o[0][:, :4], h.ref_enc_out[:, :4], tol, "mean"),
                                _close_rel(o[0][:, 4:], h.ref_enc_out[:, 4:], tol, "logvar")))


@functools.lru_cache(maxsize=None)
def _latents_data(B=2, H=9, W=13):
    from tests._philox_ref import philox_normal
    g = _g(77)
    mom = torch.cat([torch.randn(B, 4, H, W, generator=g) * 3.0, torch.randn(B, 4, H, W, generator=g) - 1.0], dim=1)
    shift = torch.tensor([0.3, -0.2, 0.05, 1.1])
    scale = torch.tensor(0.13025) / torch.tensor([1.2, 0.7, 2.0, 0.9])
    mode = ((mom[:, :4] - shift.view(1, 4, 1, 1)) * scale.view(1, 4, 1, 1)).half()
    n = torch.from_numpy(philox_normal(SEEDS, 0, 1, H * W)).view(B, 4, H, W)
    z = mom.double()[:, :4] + torch.exp(0.5 * mom.double()[:, 4:]) * n
    sample = ((z - shift.double().view(1, 4, 1, 1)) * scale.double().view(1, 4, 1, 1)).half()
    return NS(mom=mom, shift=shift.tolist(), scale=scale.tolist(), mode=mode, sample=sample, seeds=torch.tensor(SEEDS, dtype=torch.int64))


def _latents_check(o, h):
    from tests import _redraw_ref as R
    # tests/test_gpu_vae_encode_ops.py: the mode bit for bit, the sample within one fp16 ulp of float64 arithmetic
    assert torch.equal(o[0], h.mode) and int(R.ulp16(o[1], h.sample).max()) <= 1


_add("vae-latents-9x13", ["ds_vae_latents_f16"], _latents_data,
     lambda m, h: (m.ops.vae_latents(m.place(h.mom), h.scale, h.shift), m.ops.vae_latents(m.place(h.mom), h.scale, h.shift, seeds=m.place(h.seeds))),
     _latents_check)


# ------------------------------------------------------------------------------------------------ image pre-processing
@functools.lru_cache(maxsize=None)
def _resize_data(h_in=10, w_in=14, nh=7, nw=9, top=1, left=2, oh=5, ow=6):
    """Expected bytes and floats from the oracle that is pinned bit-exact to Pillow (oracle/image_preprocess_ref.py): its
    horizontal pass, its two-pass resize, its fp32 normalisation on the cropped window.  The tables the kernels are handed are
    the product's host tables, as in production."""
    from diffsensei_amd.preprocess import resample_tables
    from oracle import image_preprocess_ref as P
    src = np.random.RandomState(3).randint(0, 256, (h_in, w_in, 3)).astype(np.uint8)
    src[: h_in // 3] = 255                                   # saturated area: the bicubic lobes clamp
    tmp = P.pil_resize_u8(src, h_in, nw, "bicubic")          # height unchanged: the horizontal pass alone
    crop = P.pil_resize_u8(src, nh, nw, "bicubic")[top:top + oh, left:left + ow]
    x = crop.astype(np.float32) * np.float32(1 / 255)
    out = np.ascontiguousarray(((x - np.asarray(P.CLIP_MEAN, np.float32)) / np.asarray(P.CLIP_STD, np.float32)).transpose(2, 0, 1))
    T = lambda t: tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in t)
    return NS(src=torch.from_numpy(src), th=T(resample_tables(w_in, nw, "bicubic")), tv=T(resample_tables(h_in, nh, "bicubic")),
              tmp=torch.from_numpy(tmp), crop=torch.from_numpy(np.ascontiguousarray(crop)), out=torch.from_numpy(out),
              dims=(h_in, w_in, nh, nw, top, left, oh, ow), mean=P.CLIP_MEAN, std=P.CLIP_STD)


def _resize_run(m, h):
    from diffsensei_amd import _lib as L, ops
    lib = _lib()
    h_in, w_in, nh, nw, top, left, oh, ow = h.dims
    src = m.place(h.src)
    fh, ch, th = (m.place(t) for t in h.th)
    fv, cv, tv = (m.place(t) for t in h.tv)
    tmp = m.out((h_in, nw, 3), dtype=torch.uint8)
    L.check(lib.ds_resize_h_u8(src.data_ptr(), h_in, w_in, fh.data_ptr(), ch.data_ptr(), th.data_ptr(), th.shape[1], nw, tmp.data_ptr(),
                               ops._stream()), "ds_resize_h_u8")
    out, by = m.out((3, oh, ow), dtype=torch.float32), m.out((oh, ow, 3), dtype=torch.uint8)
    m3, s3 = (C.c_float * 3)(*h.mean), (C.c_float * 3)(*h.std)
    L.check(lib.ds_resize_v_norm_u8(tmp.data_ptr(), h_in, nw, fv.data_ptr(), cv.data_ptr(), tv.data_ptr(), tv.shape[1], top, left, oh, ow,
                                    1.0 / 255.0, m3, s3, out.data_ptr(), by.data_ptr(), ops._stream()), "ds_resize_v_norm_u8")
    return (tmp, by, out)


def _resize_check(o, h):
    # tests/test_gpu_preprocess.py: the bytes are the oracle's (= Pillow's); the normalised fp32 pixels agree to 1e-6
    assert torch.equal(o[0], h.tmp) and torch.equal(o[1], h.crop)
    err = float((o[2] - h.out).abs().max())
    print(f"resize: max |normalised - oracle| {err:.3g}")
    assert err <= 1e-6, err


_add("resize-u8-10x14-to-7x9-crop-5x6", ["ds_resize_h_u8", "ds_resize_v_norm_u8"], _resize_data, _resize_run, _resize_check)


# ------------------------------------------------------------------------------------------------ completeness (host only)
EXEMPT = {
    "ds_last_error": "host query: the thread's last error string",
    "ds_version": "host query",
    "ds_device_info": "host query of the device properties",
    "ds_set_option": "host: sets a thread-local knob (used by the cases)",
    "ds_debug_counter": "test instrumentation: reads one device counter, takes no operand",
    "ds_gemm_t160_fits": "host query of the dispatch rule",
    "ds_gemm_g320_fits": "host query of the dispatch rule",
    "ds_gemm_ln_fusable": "host query of the dispatch rule",
    "ds_conv3x3_gn_chunks": "host query of the dispatch rule (asked by the conv-gn-partial cases)",
    "ds_groupnorm_workspace_bytes": "host query (asked by the GroupNorm cases)",
    "ds_redraw_buffer_bytes": "host query (asked by the redraw cases)",
    "ds_op_describe": "host query: kernel name and roofline figures of an op",
    "ds_op_run": "plan executor: runs the launchers covered above (used by the conv-gn-partial cases)",
    "ds_plan_create": "plan executor: host bookkeeping",
    "ds_plan_num_ops": "plan executor: host query",
    "ds_plan_run": "plan executor: runs the launchers covered above",
    "ds_plan_capture": "plan executor: the same launches captured into a hipGraph",
    "ds_plan_replay": "plan executor: replays the captured launches",
    "ds_plan_destroy": "plan executor: host bookkeeping",
}


def test_every_entry_point_has_a_case():
    """Every symbol of the C ABI is named by a case above or exempted with a reason; nothing is named that does not exist."""
    from diffsensei_amd._lib import SIGNATURES
    named = {e for c in CASES for e in c.entry}
    assert not named - set(SIGNATURES), f"cases name entry points that do not exist: {sorted(named - set(SIGNATURES))}"
    assert not set(EXEMPT) - set(SIGNATURES), f"exemptions for entry points that do not exist: {sorted(set(EXEMPT) - set(SIGNATURES))}"
    missing = set(SIGNATURES) - named - set(EXEMPT)
    assert not missing, f"entry points without a poisoned-memory case (add one, or an EXEMPT line saying why not): {sorted(missing)}"
    assert all(r.strip() for r in EXEMPT.values())
    assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"


def test_arena_names_the_region_a_stray_store_hit():
    """The net itself, on the host: alignment (16 bytes, never 256), guard sizes, and `check()` finding one changed byte in front
    of an operand, behind one, and in the canary columns of a wide output - for both fills."""
    from tests._arena import GUARD_MIN_BYTES, GUARD_ROWS
    for fill in ("nan", "loud"):
        a = Arena("cpu", fill, capacity=8 << 20)
        x = a.place(torch.randn(7, 72).half())
        w = a.place(torch.randint(-5, 5, (9, 48), dtype=torch.int8))
        ids = a.place(torch.arange(6, dtype=torch.int32))
        y = a.out((5, 13), ld=24)
        z = a.out((3, 4, 8), dtype=torch.float32)
        for t in (x, w, ids, y, z):
            assert t.data_ptr() % 16 == 0 and t.data_ptr() % 256 != 0
        assert w.data_ptr() - (x.data_ptr() + x.numel() * 2) >= max(GUARD_ROWS * 72 * 2, GUARD_MIN_BYTES) + max(GUARD_ROWS * 48, GUARD_MIN_BYTES)
        assert y.stride() == (24, 1) and z.is_contiguous()
        assert bool(torch.isnan(y).all()) == (fill == "nan") and (fill == "nan" or bool((y == 1000.0).all()))
        a.check()
        x.fill_(1.0), y.fill_(2.0), z.fill_(3.0), ids.fill_(4)                 # writing operands and outputs is fine
        a.check()
        for poke, where in ((lambda: a.buf.__setitem__(x.data_ptr() - a.base - 1, 9), "guard in front of"),
                            (lambda: a.buf.__setitem__(w.data_ptr() - a.base + w.numel(), 9), "guard behind"),
                            (lambda: y.as_strided((5, 14), (24, 1)).__setitem__((2, 13), 1.5), "canary columns 13..24")):
            saved = a.buf.clone()
            poke()
            with pytest.raises(AssertionError, match=where):
                a.check()
            a.buf.copy_(saved)
            a.check()


# ------------------------------------------------------------------------------------------------ the cases on the GPU
class _Recorder:
    """Counts calls of the named entry points of the loaded library for the duration of a `with` block."""

    def __init__(self, lib, names):
        self.lib, self.names, self.called, self.saved = lib, names, set(), {}

    def __enter__(self):
        for n in self.names:
            fn = getattr(self.lib, n)
            self.saved[n] = fn

            def wrapped(*a, _fn=fn, _n=n):
                self.called.add(_n)
                return _fn(*a)
            setattr(self.lib, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.lib, n, fn)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_result_depends_on_nothing_but_the_operands(hip_lib, case):
    lib = hip_lib
    h = case.build()
    res = {}
    for mode in ("plain", "nan", "loud"):
        m = Plain(DEV) if mode == "plain" else Arena(DEV, mode, case.capacity)
        with options(lib, case.opts), _Recorder(lib, case.entry) as rec:
            if case.kernel is not None:
                code, ints, want = case.kernel
                assert _kernel_name(code, ints) == want, f"{case.id}: the knobs select {_kernel_name(code, ints)}, not {want}"
            outs = case.run(m, h)
            torch.cuda.synchronize()
        assert rec.called == set(case.entry), f"{case.id}: expected calls of {case.entry}, saw {sorted(rec.called)}"
        m.check()
        if not m.plain:      # a wrapper that allocated past the arena's hooks would hand back an output without canaries
            lo, hi = m.buf.data_ptr(), m.buf.data_ptr() + m.buf.numel()
            assert all(lo <= o.data_ptr() < hi for o in outs), f"{case.id}: an output was allocated outside the arena"
        res[mode] = [o.detach().clone().cpu() for o in outs]
        del m
    for k, (a, b, p) in enumerate(zip(res["nan"], res["loud"], res["plain"])):
        assert a.shape == b.shape == p.shape and a.dtype == p.dtype
        if a.is_floating_point():
            assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all(), \
                f"{case.id}: output {k} is not finite with poison around the operands"
        assert torch.equal(_bytes(a), _bytes(b)), \
            f"{case.id}: output {k} differs between the NaN fill and the 1000.0 fill: the kernel read something that is not its operand"
        assert torch.equal(_bytes(a), _bytes(p)), f"{case.id}: output {k} inside the arena differs from the plain call"
    case.check(res["plain"], h)


# ------------------------------------------------------------------------------------------------ engine scratch
def _poison_(t):
    if t.is_floating_point():
        t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(255)
    else:
        t.fill_(1)                                  # a wrong value that is in range wherever an integer buffer is an index


@pytest.mark.gpu
def test_unet_engine_scratch_carries_nothing_between_forwards(hip_lib):
    """Tiny config at 18 x 26 (level 1: 9 x 13 = 117 tokens, not a multiple of 8).  After one forward every tensor the engine keeps
    is filled with NaN except the whitelist below - what legitimately carries state across calls - and the same call must give
    the same bits.  A new persistent buffer has to be put on the whitelist deliberately."""
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    from tests.test_gpu_unet import _inputs
    cfg = tiny_config()
    model = UNetMangaModel(cfg, device=DEV)
    model.load_state_dict({k: v.half() for k, v in random_state_dict(cfg, 0).items()})
    model._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    B, H, W = 2, 18, 26
    x, enc, te, tid, bbox, db = _inputs(cfg, B, H, W, seed=7)
    call = lambda: model(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": H / W},
                         added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample.clone()
    first = call()
    eng = model.engine(B, H, W, H / W)
    assert eng.hw[1] == (9, 13) and (9 * 13) % 8 != 0
    # what carries state across forwards: the per-step scalar table and its row counter (written by the sampler set-up, read by
    # every forward), the IP scale vector and the dialog boxes (request state that set_request may leave as it is)
    whitelist = {"table": eng.table, "ctr": eng.ctr, "ip_scale": eng.ip_scale, "dialog_boxes": eng.dialog_boxes}
    keep_ids = {id(t) for t in whitelist.values()}
    # ... and the eight zeroed slack rows behind the scratch the operand-swapped V^T GEMM reads past the last image
    assert eng.zero_scratch and {k[0] for k in eng.zero_scratch} == {"t_norm", "t_hidden"}
    slack = {}
    for key in eng.zero_scratch:
        h_, w_ = eng.hw[key[1]]
        t = eng.scratch[key]
        M = B * h_ * w_
        assert t.numel() % (M + 8) == 0
        slack[id(t)] = M * (t.numel() // (M + 8))                # the first M rows are poisoned too
    n = 0
    for t in eng.keep:
        if not isinstance(t, torch.Tensor) or id(t) in keep_ids:
            continue
        _poison_(t.view(-1)[:slack[id(t)]] if id(t) in slack else t)
        n += 1
    assert n > 20
    again = call()
    assert torch.isfinite(again).all(), "a forward read a buffer it had not written (NaN left by the poison)"
    assert torch.equal(_bytes(again.cpu()), _bytes(first.cpu())), "the second forward depends on what the first left in the scratch"


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["mfma", "chunks"])
@pytest.mark.parametrize("weights", ["float16", "int8"])
def test_llama_engine_buffers_carry_nothing_into_a_run(hip_lib, weights, path):
    """Tiny oracle model.  A fresh engine whose activation buffers, KV caches, id lists, feature buffers and dequant scratch are
    filled with NaN (integers: a wrong in-range id) right after construction - the state blocks and the chain are left alone -
    must produce, for `generate` and for the 4-slot batched decode, the ids and features of an untouched fresh engine."""
    from oracle import make_golden_mllm as G
    from diffsensei_amd.mllm import LlamaConfig, LlamaDecodeEngine
    from tests.test_gpu_mllm_batch import PROMPTS, make_prompt
    cfg = LlamaConfig(vocab_size=G.TINY["vocab_size"], hidden_size=G.TINY["hidden_size"], intermediate_size=G.TINY["intermediate_size"],
                      num_hidden_layers=G.TINY["num_hidden_layers"], num_attention_heads=G.TINY["num_attention_heads"],
                      rms_norm_eps=G.TINY["rms_norm_eps"])
    sd = G.tiny_weights()
    prompts = [make_prompt(G, *p)[0] for p in PROMPTS]
    assert min(len(p) for p in prompts) > 16

    def run(poison):
        eng = LlamaDecodeEngine(cfg, sd, DEV, max_positions=96, max_new_tokens=40, use_graph=True, poll_every=4, prompt_path=path,
                                max_sequences=4, weight_dtype=weights)
        eng.set_image_token_chain(G.IMG_IDS)
        if poison:
            if weights == "int8":
                eng._w(eng.wqkv, eng.sqkv, 0)                     # the prompt pass's dequant scratch: allocated on first use
                assert eng._w16 is not None
            bufs = [eng.h, eng.qkv, eng.att, eng.act, eng.hn, eng.logits, eng.feats, eng.out_ids] + eng.kcs + eng.vcs + (
                [eng._w16] if eng._w16 is not None else [])
            for t in bufs:
                _poison_(t)
        one = eng.generate(eng.embed_tokens(prompts[3]), int(prompts[3][-1]), 2, G.MAX_NEW)
        outs = [(one["ids"].cpu(), one["hidden"].cpu())]
        batch = eng.generate_batch([eng.embed_tokens(p) for p in prompts], [int(p[-1]) for p in prompts], 2, G.MAX_NEW)
        outs += [(o["ids"].cpu(), o["hidden"].cpu()) for o in batch]
        return outs

    want, got = run(False), run(True)
    for k, ((ids0, hid0), (ids1, hid1)) in enumerate(zip(want, got)):
        what = "generate" if k == 0 else f"generate_batch sequence {k - 1}"
        assert len(ids0) > G.N_IMG and torch.isfinite(hid1.float()).all(), what
        assert torch.equal(ids1, ids0), f"{what}: the ids depend on what the buffers held before the run"
        assert torch.equal(_bytes(hid1), _bytes(hid0)), f"{what}: the features depend on what the buffers held before the run"
