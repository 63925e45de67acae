"""Thin torch-tensor wrappers over the C ABI (one function per entry point of include/diffsensei_hip.h).

PyTorch is plumbing here: device memory and the current HIP stream.  No arithmetic happens in this file;
every function checks devices/dtypes, hands raw pointers to the library and raises on a non-zero status.
Layouts: activations fp16 channels-last — images [B, H*W, C] (or [B,H,W,C]), token matrices [rows, C].
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check

Tensor = torch.Tensor


def bind_device(dev: torch.device) -> None:
    """One process drives one GPU.  The library launches on "the current stream", which HIP resolves per
    CURRENT device, so before a launch the tensors' device is made the current one (a no-op in the normal case where
    `init_from_env` / the caller already selected it).  NOTE: this changes process-global state (torch's current device) and
    does not restore it - deliberate under the one-process-one-GPU design; the library's per-device one-off set-up
    (`ds_first_on_device`, csrc/ds_common.h) is keyed by device, so a process that does touch a second GPU stays correct."""
    if dev.type == "cuda" and dev.index is not None and dev.index != torch.cuda.current_device():
        torch.cuda.set_device(dev)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(*ts: Optional[Tensor], dtype=torch.float16) -> None:
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.DiffSenseiHipError("diffsensei_amd ops need CUDA(HIP) tensors — there is no CPU path")
        bind_device(t.device)
        if dtype is not None and t.dtype != dtype:
            raise _lib.DiffSenseiHipError(f"expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise _lib.DiffSenseiHipError("tensor must be contiguous")


_EPILOGUES = {None: 0, "geglu": 1, "gelu": 2, "quick_gelu": 3}


def _geglu_code(geglu) -> int:
    """`geglu` argument of the GEMM wrappers -> epilogue code: False 0, True 1 (w / bias packed by `engine.pack_geglu`, 128-row
    groups), 320 -> 4 (packed by `engine.pack_geglu320`: gemm_g320_kernel)."""
    if geglu is True or geglu == 1:
        return 1
    if geglu == 320:
        return 4
    assert not geglu, geglu
    return 0


def gemm(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
         geglu: bool = False, out: Optional[Tensor] = None, x2: Optional[Tensor] = None,
         act: Optional[str] = None) -> Tensor:
    """y = act(cat([x, x2], -1) @ w.T + bias) (+residual);  geglu: w/bias packed by `pack_geglu`, y = h*gelu(g)."""
    _chk(x, w, bias, residual, x2)
    epi = _geglu_code(geglu) if geglu else _EPILOGUES[act]
    M, K1 = x.shape
    K = K1 + (x2.shape[1] if x2 is not None else 0)
    N = w.shape[0]
    assert w.shape[1] == K
    n_out = N // 2 if geglu else N
    if out is None:
        out = torch.empty((M, n_out), dtype=torch.float16, device=x.device)
    L = _lib.load()
    check(L.ds_gemm_f16(_p(x), K1, _p(x2), 0 if x2 is None else x2.shape[1], K1, _p(w), K, _p(bias), _p(residual),
                        n_out, _p(out), n_out, M, N, K, epi, _stream()), "ds_gemm_f16")
    return out


def gemm_ln(x: Tensor, gw: Tensor, bias_ln: Optional[Tensor] = None, ln_c: Optional[Tensor] = None,
            ln_stats: Optional[Tensor] = None, residual: Optional[Tensor] = None, geglu: bool = False,
            emit_stats: bool = False, out: Optional[Tensor] = None):
    """The two roles of a fused LayerNorm (include/diffsensei_hip.h, ds_gemm_ln_f16):
    consumer (`ln_stats` [M,2] fp32 (mean, rstd), `ln_c` [N,2] f16, `gw`, `bias_ln` from `engine.pack_ln_fused`):
        y = rstd (x gw^T - mean c) + b' on the RAW x;
    producer (`emit_stats`): y = x gw^T + bias (+ residual) and the [N/64, M, 2] fp32 partial (sum, sum of squares) of the stored
        rows -> returns (y, partial)."""
    _chk(x, gw, bias_ln, ln_c, residual)
    _chk(ln_stats, dtype=torch.float32)
    M, K = x.shape
    N = gw.shape[0]
    n_out = N // 2 if geglu else N
    if out is None:
        out = torch.empty((M, n_out), dtype=torch.float16, device=x.device)
    part = torch.empty((N // 64, M, 2), dtype=torch.float32, device=x.device) if emit_stats else None
    L = _lib.load()
    check(L.ds_gemm_ln_f16(_p(x), K, _p(gw), K, _p(bias_ln), _p(ln_stats), _p(ln_c), _p(residual), n_out, _p(out), n_out,
                           _p(part), M, N, K, _geglu_code(geglu), _stream()), "ds_gemm_ln_f16")
    return (out, part) if emit_stats else out


def ln_finalize(partial: Tensor, C: int, eps: float = 1e-5) -> Tensor:
    """[strips, M, 2] fp32 partial sums of a producer GEMM -> [M, 2] fp32 (mean, rstd) over C columns."""
    _chk(partial, dtype=torch.float32)
    strips, M, _ = partial.shape
    st = torch.empty((M, 2), dtype=torch.float32, device=partial.device)
    check(_lib.load().ds_ln_finalize(_p(partial), _p(st), M, strips, C, eps, _stream()), "ds_ln_finalize")
    return st


def gemm_ln_fusable(M: int, N: int, K: int, geglu: bool = False, batch: int = 1) -> int:
    """Which fused-LayerNorm form the dispatch gives this GEMM: 1 = the 256 x 256 kernel (`gemm_ln` with finalised statistics),
    2 = the 128-wide kernels (`gemm_ln_partial` consumers, `gemm_ln` producers), 0 = none."""
    return int(_lib.load().ds_gemm_ln_fusable(M, N, K, _geglu_code(geglu), batch))


def gemm_ln_partial(x: Tensor, gw: Tensor, bias_ln: Optional[Tensor], ln_c: Tensor, partial: Tensor, eps: float = 1e-5,
                    residual: Optional[Tensor] = None, geglu: bool = False, emit_stats: bool = False,
                    out: Optional[Tensor] = None):
    """Consumer of a fused LayerNorm on the 128-wide kernels (ds_gemm_ln_partial_f16): `partial` [K/64, M, 2] fp32 is what a
    producer emitted; every block sums the partials of its own rows, no finalize launch.  y = rstd (x gw^T - mean c) + b'."""
    _chk(x, gw, bias_ln, ln_c, residual)
    _chk(partial, dtype=torch.float32)
    M, K = x.shape
    N = gw.shape[0]
    assert tuple(partial.shape) == (K // 64, M, 2), (tuple(partial.shape), (K // 64, M, 2))
    n_out = N // 2 if geglu else N
    if out is None:
        out = torch.empty((M, n_out), dtype=torch.float16, device=x.device)
    part = torch.empty((N // 64, M, 2), dtype=torch.float32, device=x.device) if emit_stats else None
    check(_lib.load().ds_gemm_ln_partial_f16(_p(x), K, _p(gw), K, _p(bias_ln), _p(partial), eps, _p(ln_c), _p(residual), n_out,
                                             _p(out), n_out, _p(part), M, N, K, _geglu_code(geglu), _stream()),
          "ds_gemm_ln_partial_f16")
    return (out, part) if emit_stats else out


def gemm_ln_swapped_partial(a: Tensor, x: Tensor, partial: Tensor, ln_cb: Tensor, eps: float = 1e-5,
                            out: Optional[Tensor] = None) -> Tensor:
    """`gemm_ln_swapped` on the 128-wide kernels (ds_gemm_ln_swapped_partial_f16): partial [K/64, Z*N, 2] fp32 as a producer
    emitted them for the rows of x.view(Z*N, K); no finalize launch."""
    _chk(a, x, ln_cb)
    _chk(partial, dtype=torch.float32)
    Z, N, K = x.shape
    M = a.shape[0]
    assert tuple(partial.shape) == (K // 64, Z * N, 2), tuple(partial.shape)
    if out is None:
        out = torch.empty((Z, M, N), dtype=torch.float16, device=x.device)
    check(_lib.load().ds_gemm_ln_swapped_partial_f16(_p(a), K, _p(x), K, N * K, _p(partial), eps, Z * N, N, _p(ln_cb), _p(out), N,
                                                     M * N, M, N, K, Z, _stream()), "ds_gemm_ln_swapped_partial_f16")
    return out


def gemm_ln_swapped(a: Tensor, x: Tensor, ln_stats: Tensor, ln_cb: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """out[z] = a @ LN(x[z])^T with the LayerNorm folded in (ds_gemm_ln_swapped_f16): a = gamma (.) W [M,K], x [Z,N,K] raw,
    ln_stats [Z*N,2] fp32 (mean, rstd), ln_cb [M,4] f16 (-c hi, -c lo, b' hi, b' lo) -> [Z,M,N]."""
    _chk(a, x, ln_cb)
    _chk(ln_stats, dtype=torch.float32)
    Z, N, K = x.shape
    M = a.shape[0]
    if out is None:
        out = torch.empty((Z, M, N), dtype=torch.float16, device=x.device)
    check(_lib.load().ds_gemm_ln_swapped_f16(_p(a), K, _p(x), K, N * K, _p(ln_stats), N, _p(ln_cb), _p(out), N, M * N, M, N, K,
                                             Z, _stream()), "ds_gemm_ln_swapped_f16")
    return out


def gemm_batched_nt(a: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """out[z] = a[z or shared] @ b[z].T ; a: [M,K] or [Z,M,K], b: [Z,N,K] -> [Z,M,N]."""
    _chk(a, b)
    Z, N, K = b.shape
    M = a.shape[-2]
    sa = 0 if a.dim() == 2 else M * K
    if out is None:
        out = torch.empty((Z, M, N), dtype=torch.float16, device=b.device)
    L = _lib.load()
    check(L.ds_gemm_f16_batched(_p(a), K, sa, _p(b), K, N * K, _p(out), N, M * N, M, N, K, Z, _stream()),
          "ds_gemm_f16_batched")
    return out


def conv3x3(x: Tensor, w: Tensor, bias: Optional[Tensor], stride: int = 1, upsample: bool = False,
            rowbias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
            out_size: Optional[Tuple[int, int]] = None) -> Tensor:
    """x: [B,H,W,Cin] NHWC, w: [Cout,3,3,Cin] -> [B,Ho,Wo,Cout]; rowbias: [B,Cout] per-image bias.  `out_size` (Ho, Wo):
    nearest-resize to that size first (F.interpolate(size=...) indexing), then the conv (Upsample2D with output_size)."""
    _chk(x, w, bias, rowbias, residual)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    L = _lib.load()
    if out_size is not None:
        Ho, Wo = int(out_size[0]), int(out_size[1])
        y = torch.empty((B, Ho, Wo, Cout), dtype=torch.float16, device=x.device)
        check(L.ds_conv3x3_resize_f16(_p(x), _p(w), _p(bias), _p(rowbias), 0 if rowbias is None else rowbias.shape[1],
                                      _p(residual), _p(y), B, H, W, Cin, Cout, Ho, Wo, _stream()), "ds_conv3x3_resize_f16")
        return y
    Ho, Wo = (2 * H, 2 * W) if upsample else ((H + stride - 1) // stride, (W + stride - 1) // stride)
    y = torch.empty((B, Ho, Wo, Cout), dtype=torch.float16, device=x.device)
    check(L.ds_conv3x3_f16(_p(x), _p(w), _p(bias), _p(rowbias), 0 if rowbias is None else rowbias.shape[1],
                           _p(residual), _p(y), B, H, W, Cin, Cout, stride, int(upsample), _stream()),
          "ds_conv3x3_f16")
    return y


def fold_upsample2x(w: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """w: [Cout,3,3,Cin] (= packed [Cout, 9*Cin]) -> [4, Cout, 4*Cin]: the four 2x2 phase weights of nearest x2 + conv3x3
    (ds_fold_upsample2x_f16; torch model: `engine.fold_upsample2x_reference`).  `out`: existing storage to fold into (after a
    LoRA merge rewrote `w` in place)."""
    _chk(w, out)
    Cout, Cin = w.shape[0], w.numel() // (9 * w.shape[0])
    if out is None:
        out = torch.empty((4, Cout, 4 * Cin), dtype=torch.float16, device=w.device)
    elif tuple(out.shape) != (4, Cout, 4 * Cin):
        raise ValueError(f"fold_upsample2x: out must be [4, {Cout}, {4 * Cin}]")
    check(_lib.load().ds_fold_upsample2x_f16(_p(w), _p(out), Cout, Cin, _stream()), "ds_fold_upsample2x_f16")
    return out


def conv3x3_up2fold(x: Tensor, wfold: Tensor, bias: Optional[Tensor], rowbias: Optional[Tensor] = None,
                    residual: Optional[Tensor] = None) -> Tensor:
    """x: [B,H,W,Cin] NHWC, wfold: [4,Cout,4*Cin] from `fold_upsample2x` -> [B,2H,2W,Cout]: Upsample2D (nearest x2 + conv3x3)
    as four 2x2 phase convolutions of x."""
    _chk(x, wfold, bias, rowbias, residual)
    B, H, W, Cin = x.shape
    Cout = wfold.shape[1]
    assert wfold.shape == (4, Cout, 4 * Cin), (tuple(wfold.shape), Cin)
    y = torch.empty((B, 2 * H, 2 * W, Cout), dtype=torch.float16, device=x.device)
    check(_lib.load().ds_conv3x3_up2fold_f16(_p(x), _p(wfold), _p(bias), _p(rowbias), 0 if rowbias is None else rowbias.shape[1],
                                             _p(residual), _p(y), B, H, W, Cin, Cout, _stream()), "ds_conv3x3_up2fold_f16")
    return y


def groupnorm(x: Tensor, gamma: Tensor, beta: Tensor, groups: int, eps: float, silu: bool,
              x2: Optional[Tensor] = None) -> Tensor:
    """x: [B,HW,C1] (+ x2 [B,HW,C2] concatenated on channels) -> [B,HW,C1+C2]."""
    _chk(x, gamma, beta, x2)
    B, HW, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[2]
    L = _lib.load()
    ws = torch.empty(L.ds_groupnorm_workspace_bytes(B, C1 + C2), dtype=torch.uint8, device=x.device)
    y = torch.empty((B, HW, C1 + C2), dtype=torch.float16, device=x.device)
    check(L.ds_groupnorm_f16(_p(x), _p(x2), _p(y), _p(gamma), _p(beta), _p(ws), B, HW, C1, C2, groups, eps, int(silu),
                             _stream()), "ds_groupnorm_f16")
    return y


def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = 1e-5) -> Tensor:
    _chk(x, gamma, beta)
    C = x.shape[-1]
    y = torch.empty_like(x)
    check(_lib.load().ds_layernorm_f16(_p(x), _p(y), _p(gamma), _p(beta), x.numel() // C, C, eps, _stream()),
          "ds_layernorm_f16")
    return y


def self_attention(q: Tensor, k: Tensor, vt: Tensor, heads: int, scale: Optional[float] = None) -> Tensor:
    """q,k: [B,N,heads*64]; vt: [B,heads,64,Nk] (V transposed) -> [B,N,heads*64]."""
    _chk(q, k, vt)
    B, Nq, Cc = q.shape
    Nk = k.shape[1]
    o = torch.empty_like(q)
    check(_lib.load().ds_self_attn_f16(_p(q), Cc, Nq * Cc, _p(k), Cc, Nk * Cc, _p(vt), vt.shape[-1], _p(o), Cc, Nq * Cc,
                                       B, heads, Nq, Nk, scale if scale is not None else 0.125, _stream()),
          "ds_self_attn_f16")
    return o


def masked_ip_attention(q: Tensor, kt: Tensor, vtt: Tensor, ki: Tensor, vti: Tensor, bbox: Tensor, heads: int,
                        mask_hw: Tuple[int, int], ip_scale: float, Lt: int = 77, Li: int = 80, n_dummy: int = 16,
                        tok_per_ip: int = 16, qk_scale: float = 0.125, out: Optional[Tensor] = None,
                        ldq: Optional[int] = None, ldo: Optional[int] = None, ldk: Optional[int] = None,
                        sk: Optional[int] = None, sv: Optional[int] = None,
                        ip_scale_dev: Optional[Tensor] = None) -> Tensor:
    """q: [B,N,C]; kt/ki: [B,96,C]; vtt/vti: [B,C,96]; bbox: [B,max_ips,4] fp32.

    The strides of the C ABI (include/diffsensei_hip.h) are taken from the tensors, so column slices of wider buffers work as
    they are: q / out `buf[:, :, c0:c0+C]` (row stride ldq / ldo, batch stride N rows), key panels `stacked[:, :, c0:c0+C]`
    (ldk, sk), value panels `stacked_t[:, c0:c0+C, :]` (sv).  `ldq, ldo, ldk, sk, sv` override what the tensors say;
    `ip_scale_dev` (fp32 on the device) replaces `ip_scale`: shape [1] is one scale for the batch, shape [B] one per batch
    row (under CFG rows n and ns + n belong to panel n and carry the same value).  With B = 1 the two mean the same.

    Long prompts: kt [B,96 T,C] / vtt [B,C,96 T] with T = ceil(Lt / 96) in 2..4 (Lt up to 384) take the long-prompt kernel
    (ds_masked_ip_attn_long_f16 / ..._rows_f16); the text panels then have strides of their own, taken from the tensors."""
    for t in (q, kt, vtt, ki, vti, out):
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.DiffSenseiHipError("diffsensei_amd ops need CUDA(HIP) tensors — there is no CPU path")
        bind_device(t.device)
        if t.dtype != torch.float16 or t.dim() != 3 or t.stride(2) != 1:
            raise _lib.DiffSenseiHipError("masked_ip_attention: fp16 [*,*,*] tensors with unit stride in the last dimension")
    _chk(bbox, dtype=torch.float32)
    _chk(ip_scale_dev, dtype=torch.float32)
    B, N, Cc = q.shape
    if ip_scale_dev is not None and (ip_scale_dev.device != q.device or tuple(ip_scale_dev.shape) not in ((1,), (B,))):
        raise _lib.DiffSenseiHipError(f"masked_ip_attention: ip_scale_dev {tuple(ip_scale_dev.shape)} on {ip_scale_dev.device}: "
                                      f"(1,) or ({B},) on {q.device} is needed")
    if out is None:
        out = torch.empty((B, N, Cc), dtype=torch.float16, device=q.device)
    if out.shape != q.shape:
        raise _lib.DiffSenseiHipError(f"masked_ip_attention: out {tuple(out.shape)} != q {tuple(q.shape)}")
    ldq = q.stride(1) if ldq is None else ldq
    ldo = out.stride(1) if ldo is None else ldo
    if B > 1 and (q.stride(0) != N * ldq or out.stride(0) != N * ldo):
        raise _lib.DiffSenseiHipError("masked_ip_attention: q / out batch stride must be N rows")
    if kt.shape[1] != 96:
        # long prompt: T text panels of 96 rows with strides of their own (ds_masked_ip_attn_long_f16); one panel stays below
        T = kt.shape[1] // 96
        if kt.shape[1] % 96 or vtt.shape[2] != kt.shape[1] or vtt.stride(1) != vtt.shape[2] or vti.stride(1) != vti.shape[2]:
            raise _lib.DiffSenseiHipError(f"masked_ip_attention: text panels [B,96 T,C] / [B,C,96 T] with dense value rows are needed "
                                          f"(kt {tuple(kt.shape)}, vtt {tuple(vtt.shape)})")
        if ldk is not None or sk is not None or sv is not None:
            raise _lib.DiffSenseiHipError("masked_ip_attention: ldk / sk / sv overrides are for the one-panel form")
        strides = (kt.stride(1), kt.stride(0), vtt.stride(0), ki.stride(1), ki.stride(0), vti.stride(0))
        if ip_scale_dev is not None and ip_scale_dev.shape[0] > 1:
            check(_lib.load().ds_masked_ip_attn_long_rows_f16(_p(q), ldq, _p(kt), _p(vtt), _p(ki), _p(vti), _p(bbox), _p(out), ldo,
                                                              B, heads, N, Lt, T, Li, n_dummy, tok_per_ip, bbox.shape[1],
                                                              mask_hw[0], mask_hw[1], qk_scale, _p(ip_scale_dev), *strides,
                                                              _stream()),
                  "ds_masked_ip_attn_long_rows_f16")
            return out
        check(_lib.load().ds_masked_ip_attn_long_f16(_p(q), ldq, _p(kt), _p(vtt), _p(ki), _p(vti), _p(bbox), _p(out), ldo, B, heads,
                                                     N, Lt, T, Li, n_dummy, tok_per_ip, bbox.shape[1], mask_hw[0], mask_hw[1],
                                                     qk_scale, ip_scale, _p(ip_scale_dev), *strides, _stream()),
              "ds_masked_ip_attn_long_f16")
        return out
    if kt.stride() != ki.stride() or vtt.stride() != vti.stride() or vtt.stride(1) != vtt.shape[2]:
        raise _lib.DiffSenseiHipError("masked_ip_attention: text and IP panels must share strides; value rows are dense")
    ldk = kt.stride(1) if ldk is None else ldk
    sk = kt.stride(0) if sk is None else sk
    sv = vtt.stride(0) if sv is None else sv
    if ip_scale_dev is not None and ip_scale_dev.shape[0] > 1:
        check(_lib.load().ds_masked_ip_attn_rows_f16(_p(q), ldq, _p(kt), _p(vtt), _p(ki), _p(vti), _p(bbox), _p(out), ldo, B,
                                                     heads, N, Lt, Li, n_dummy, tok_per_ip, bbox.shape[1], mask_hw[0],
                                                     mask_hw[1], qk_scale, _p(ip_scale_dev), ldk, sk, sv, _stream()),
              "ds_masked_ip_attn_rows_f16")
        return out
    check(_lib.load().ds_masked_ip_attn_f16(_p(q), ldq, _p(kt), _p(vtt), _p(ki), _p(vti), _p(bbox), _p(out), ldo, B, heads,
                                            N, Lt, Li, n_dummy, tok_per_ip, bbox.shape[1], mask_hw[0], mask_hw[1],
                                            qk_scale, ip_scale, _p(ip_scale_dev), ldk, sk, sv, _stream()),
          "ds_masked_ip_attn_f16")
    return out


def ip_region_flags(bbox: Tensor, N: int, mask_hw: Tuple[int, int]) -> Tensor:
    _chk(bbox, dtype=torch.float32)
    B = bbox.shape[0]
    flags = torch.empty((B, N), dtype=torch.uint8, device=bbox.device)
    check(_lib.load().ds_ip_region_flags(_p(bbox), _p(flags), B, N, bbox.shape[1], mask_hw[0], mask_hw[1], _stream()),
          "ds_ip_region_flags")
    return flags


def embed_tokens(ids: Tensor, tok_emb: Tensor, pos_emb: Tensor) -> Tensor:
    """ids: int32 [B,T]; tok_emb: [vocab,D]; pos_emb: [>=T,D] -> [B,T,D] = tok_emb[ids] + pos_emb[:T]."""
    _chk(tok_emb, pos_emb)
    _chk(ids, dtype=torch.int32)
    B, T = ids.shape
    D = tok_emb.shape[1]
    out = torch.empty((B, T, D), dtype=torch.float16, device=ids.device)
    check(_lib.load().ds_embed_tokens_f16(_p(ids), _p(tok_emb), _p(pos_emb), _p(out), B, T, D, tok_emb.shape[0],
                                          _stream()), "ds_embed_tokens_f16")
    return out


def causal_attention(q: Tensor, k: Tensor, v: Tensor, heads: int, scale: float) -> Tensor:
    """Causal self-attention over [B,N,heads*D] (k/v may be column-slice views): the CLIP text encoders."""
    _chk(q)
    for t in (k, v):
        if not t.is_cuda or t.dtype != torch.float16 or t.stride(2) != 1:
            raise _lib.DiffSenseiHipError("causal_attention: k/v must be fp16 device tensors with unit inner stride")
    B, N, Cc = q.shape
    o = torch.empty_like(q)
    check(_lib.load().ds_small_attn_causal_f16(_p(q), Cc, N * Cc, _p(k), k.stride(1), k.stride(0), _p(v), v.stride(1),
                                               v.stride(0), _p(o), Cc, N * Cc, B, heads, N, Cc // heads, scale,
                                               _stream()), "ds_small_attn_causal_f16")
    return o


def small_attention(q: Tensor, k: Tensor, v: Tensor, heads: int, scale: float) -> Tensor:
    """q: [B,Nq,heads*D], k/v: [B,Nk,heads*D] (any D<=256 multiple of 8); k/v may be column-slice views."""
    _chk(q)
    for t in (k, v):
        if not t.is_cuda or t.dtype != torch.float16 or t.stride(2) != 1:
            raise _lib.DiffSenseiHipError("small_attention: k/v must be fp16 device tensors with unit inner stride")
    B, Nq, Cc = q.shape
    Nk = k.shape[1]
    o = torch.empty_like(q)
    check(_lib.load().ds_small_attn_f16(_p(q), Cc, Nq * Cc, _p(k), k.stride(1), k.stride(0), _p(v), v.stride(1),
                                        v.stride(0), _p(o), Cc, Nq * Cc, B, heads, Nq, Nk, Cc // heads, scale,
                                        _stream()), "ds_small_attn_f16")
    return o


def conv_in_dialog(x: Tensor, w: Tensor, bias: Tensor, boxes: Optional[Tensor], demb: Optional[Tensor]) -> Tensor:
    """x: [B,H,W,4]; w: [Cout,3,3,4]; boxes: int32 [B,nd,4] pixel boxes or None."""
    _chk(x, w, bias, demb)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    nd = 0 if boxes is None else boxes.shape[1]
    if boxes is not None:
        _chk(boxes, dtype=torch.int32)
    y = torch.empty((B, H, W, Cout), dtype=torch.float16, device=x.device)
    check(_lib.load().ds_conv_in_dialog_f16(_p(x), _p(w), _p(bias), _p(boxes), _p(demb), _p(y), B, H, W, Cin, Cout, nd,
                                            _stream()), "ds_conv_in_dialog_f16")
    return y


def conv_out(x: Tensor, w: Tensor, bias: Tensor) -> Tensor:
    _chk(x, w, bias)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    y = torch.empty((B, H, W, Cout), dtype=torch.float16, device=x.device)
    check(_lib.load().ds_conv_out_f16(_p(x), _p(w), _p(bias), _p(y), B, H, W, Cin, Cout, _stream()), "ds_conv_out_f16")
    return y


def skinny_linear(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, addend: Optional[Tensor] = None,
                  silu_in: bool = False, silu_out: bool = False) -> Tensor:
    _chk(x, w, bias, addend)
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float16, device=x.device)
    check(_lib.load().ds_skinny_linear_f16(_p(x), _p(w), _p(bias), _p(addend), _p(y), M, N, K, int(silu_in),
                                           int(silu_out), _stream()), "ds_skinny_linear_f16")
    return y


def timestep_embed(table: Tensor, B: int, dim: int, flip: bool = True, freq_shift: float = 0.0,
                   ctr: Optional[Tensor] = None) -> Tensor:
    _chk(table, dtype=torch.float32)
    out = torch.empty((B, dim), dtype=torch.float16, device=table.device)
    check(_lib.load().ds_timestep_embed_f16(_p(table), _p(ctr), _p(out), B, dim, int(flip), freq_shift, _stream()),
          "ds_timestep_embed_f16")
    return out


def add_time_ids(text_embeds: Tensor, time_ids: Tensor, dim: int, flip: bool = True, freq_shift: float = 0.0) -> Tensor:
    _chk(text_embeds, time_ids)
    B, P = text_embeds.shape
    n = time_ids.shape[1]
    out = torch.empty((B, P + n * dim), dtype=torch.float16, device=text_embeds.device)
    check(_lib.load().ds_add_time_ids_f16(_p(text_embeds), _p(time_ids), _p(out), B, P, n, dim, int(flip), freq_shift,
                                          _stream()), "ds_add_time_ids_f16")
    return out


def _chk_seeds(seeds: Optional[Tensor], ns: int) -> None:
    _chk(seeds, dtype=torch.int64)
    if seeds is not None and tuple(seeds.shape) != (ns,):
        raise ValueError(f"seeds {tuple(seeds.shape)}: one int64 per panel, ({ns},), is needed")


def _sampler_step_dims(eps: Tensor, latents: Tensor, model_in: Tensor, table: Tensor, solver: Optional[Tensor] = None,
                       prev_x0: Optional[Tensor] = None, seeds: Optional[Tensor] = None,
                       guidance: Optional[Tensor] = None) -> Tuple[int, int]:
    """The checks the entry points of `sampler_step_kernel` share; returns (ns, HW)."""
    _chk(eps, latents, model_in, prev_x0)
    _chk(table, solver, guidance, dtype=torch.float32)
    if guidance is not None and (tuple(guidance.shape) != (latents.shape[0],) or guidance.device != latents.device):
        raise _lib.DiffSenseiHipError(f"guidance {tuple(guidance.shape)} on {guidance.device}: one fp32 per panel, "
                                      f"({latents.shape[0]},), on {latents.device} is needed")
    if prev_x0 is not None and prev_x0.shape != latents.shape:
        raise ValueError(f"prev_x0 {tuple(prev_x0.shape)} must have the latents' shape {tuple(latents.shape)}")
    ns = latents.shape[0]
    _chk_seeds(seeds, ns)
    return ns, latents.shape[2] * latents.shape[3]


def _step_panels(eps, latents, model_in, table, guidance, solver, prev_x0, seeds, ctr, ns, HW, kind, do_cfg) -> None:
    """Every kind with one guidance scale per panel (`guidance`: fp32 [ns] in place of column 7 of the table)."""
    check(_lib.load().ds_cfg_sampler_step_panels_f16(_p(eps), _p(latents), _p(model_in), _p(table), _p(guidance), _p(solver),
                                                     _p(prev_x0), _p(seeds), _p(ctr), ns, HW, kind, int(do_cfg), _stream()),
          "ds_cfg_sampler_step_panels_f16")


def cfg_sampler_step(eps: Tensor, latents: Tensor, model_in: Tensor, table: Tensor, kind: int, do_cfg: bool = True,
                     ctr: Optional[Tensor] = None, guidance: Optional[Tensor] = None) -> None:
    """eps: [2ns,HW,4] NHWC; latents: [ns,4,H,W] NCHW (in place); model_in: [2ns,HW,4].  `guidance`: fp32 [ns], one
    scale per panel (rows n and ns + n of eps) in place of column 7 of the table; None: column 7."""
    ns, HW = _sampler_step_dims(eps, latents, model_in, table, guidance=guidance)
    if guidance is not None:
        if kind not in (0, 1):
            raise _lib.DiffSenseiHipError("cfg_sampler_step: kind 0 or 1 (2: cfg_dpm_step, 3: cfg_sampler_step_noise)")
        return _step_panels(eps, latents, model_in, table, guidance, None, None, None, ctr, ns, HW, kind, do_cfg)
    check(_lib.load().ds_cfg_sampler_step_f16(_p(eps), _p(latents), _p(model_in), _p(table), _p(ctr), ns, HW, kind,
                                              int(do_cfg), _stream()), "ds_cfg_sampler_step_f16")


def cfg_dpm_step(eps: Tensor, latents: Tensor, model_in: Tensor, table: Tensor, solver: Tensor, prev_x0: Tensor,
                 do_cfg: bool = True, ctr: Optional[Tensor] = None, guidance: Optional[Tensor] = None) -> None:
    """DPM-Solver++ step: eps [2ns,HW,4] NHWC; latents, prev_x0: [ns,4,H,W] NCHW (both in place); model_in: [2ns,HW,4];
    solver: fp32 rows [n,8] (include/diffsensei_hip.h); `guidance`: as in `cfg_sampler_step`."""
    ns, HW = _sampler_step_dims(eps, latents, model_in, table, solver=solver, prev_x0=prev_x0, guidance=guidance)
    if guidance is not None:
        return _step_panels(eps, latents, model_in, table, guidance, solver, prev_x0, None, ctr, ns, HW, 2, do_cfg)
    check(_lib.load().ds_cfg_dpm_step_f16(_p(eps), _p(latents), _p(model_in), _p(table), _p(solver), _p(prev_x0),
                                          _p(ctr), ns, HW, int(do_cfg), _stream()), "ds_cfg_dpm_step_f16")


def cfg_sampler_step_noise(eps: Tensor, latents: Tensor, model_in: Tensor, table: Tensor, seeds: Optional[Tensor],
                           kind: int, do_cfg: bool = True, ctr: Optional[Tensor] = None,
                           guidance: Optional[Tensor] = None) -> None:
    """`cfg_sampler_step` with the per-panel Philox seeds (int64 [ns]) that kind 3, Euler Ancestral, draws its noise
    from: the noise of panel n at this launch is a function of (seeds[n], pixel, *ctr) only."""
    ns, HW = _sampler_step_dims(eps, latents, model_in, table, seeds=seeds, guidance=guidance)
    if guidance is not None:
        if kind == 2:
            raise _lib.DiffSenseiHipError("cfg_sampler_step_noise: kind 2 needs solver rows and prev_x0 (cfg_dpm_step)")
        return _step_panels(eps, latents, model_in, table, guidance, None, None, seeds, ctr, ns, HW, kind, do_cfg)
    check(_lib.load().ds_cfg_sampler_step_noise_f16(_p(eps), _p(latents), _p(model_in), _p(table), _p(seeds), _p(ctr),
                                                    ns, HW, kind, int(do_cfg), _stream()),
          "ds_cfg_sampler_step_noise_f16")


def cfg_lcm_step(eps: Tensor, latents: Tensor, model_in: Tensor, table: Tensor, solver: Optional[Tensor],
                 seeds: Optional[Tensor], do_cfg: bool = True, ctr: Optional[Tensor] = None,
                 guidance: Optional[Tensor] = None) -> None:
    """LCM step (kind 4): `cfg_sampler_step_noise` plus the solver rows fp32 [n,8] = {sqrt(a_prev), sqrt(1-a_prev), 0...} that
    carry the row's fifth and sixth scalar (include/diffsensei_hip.h).  It goes through the per-panel entry point, the one
    that takes table, solver rows and seeds together; `guidance` None keeps column 7 of the table."""
    ns, HW = _sampler_step_dims(eps, latents, model_in, table, solver=solver, seeds=seeds, guidance=guidance)
    _step_panels(eps, latents, model_in, table, guidance, solver, None, seeds, ctr, ns, HW, 4, do_cfg)


# ---- region redraw: the packed buffer of include/diffsensei_hip.h ("Region redraw") and the two launches that read it
REDRAW_MAX_ROWS = 1025


def redraw_buffer(ns: int, H: int, W: int, device) -> Tensor:
    """The zeroed uint8 device buffer `x0k | noise | mask | header | renoise rows` for `ns` panels of H x W latents."""
    n = int(_lib.load().ds_redraw_buffer_bytes(int(ns), int(H) * int(W)))
    return torch.zeros(n, dtype=torch.uint8, device=device)


def redraw_views(buf: Tensor, ns: int, H: int, W: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Views of a redraw buffer: x0k fp16 [ns,4,H,W], noise fp16 [ns,4,H,W], mask fp16 [ns,H,W], header fp32 [4]
    ({full strength, init_noise_sigma, 0, 0}), renoise rows fp32 [REDRAW_MAX_ROWS, 2]."""
    HW = H * W
    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() or buf.data_ptr() % 16:
        raise _lib.DiffSenseiHipError("redraw buffer: a contiguous, 16-byte aligned uint8 vector is needed")
    if buf.numel() != int(_lib.load().ds_redraw_buffer_bytes(ns, HW)):
        raise _lib.DiffSenseiHipError(f"redraw buffer: {buf.numel()} bytes do not fit ns={ns}, HW={HW}")
    n4 = ns * 4 * HW
    off = (18 * ns * HW + 15) & ~15
    half = buf[:18 * ns * HW].view(torch.float16)
    f32 = buf[off:].view(torch.float32)
    return (half[:n4].view(ns, 4, H, W), half[n4:2 * n4].view(ns, 4, H, W), half[2 * n4:].view(ns, H, W), f32[:4],
            f32[4:].view(REDRAW_MAX_ROWS, 2))


def redraw_load(buf: Tensor, x0: Tensor, noise: Tensor, mask: Tensor, renoise_rows: Tensor, full_strength: bool = False,
                init_noise_sigma: float = 1.0) -> None:
    """Fill a redraw buffer.  x0, noise: [ns,4,H,W]; mask: [ns,H,W] in [0, 1] (1 = repaint; checked here, on the host -
    the kernel takes it as given); renoise_rows: fp32 [n_run + 1, 2], one {ka, kb} per state of the run."""
    if x0.dim() != 4 or x0.shape[1] != 4 or noise.shape != x0.shape:
        raise ValueError(f"redraw: x0 {tuple(x0.shape)} and noise {tuple(noise.shape)} must both be [ns,4,H,W]")
    ns, _, H, W = x0.shape
    if tuple(mask.shape) != (ns, H, W):
        raise ValueError(f"redraw: mask {tuple(mask.shape)}, ({ns}, {H}, {W}) is needed")
    rows = torch.as_tensor(renoise_rows, dtype=torch.float32)
    if rows.dim() != 2 or rows.shape[1] != 2 or not 2 <= rows.shape[0] <= REDRAW_MAX_ROWS:
        raise ValueError(f"redraw: renoise rows {tuple(rows.shape)}, [n_run + 1, 2] with n_run + 1 <= {REDRAW_MAX_ROWS} is needed")
    mh = mask.to(torch.float16)
    lo, hi = float(mh.min()), float(mh.max())
    if not (lo >= 0.0 and hi <= 1.0):      # also refuses NaN
        raise _lib.DiffSenseiHipError(f"redraw: mask values must lie in [0, 1], got [{lo}, {hi}]")
    vx, vn, vm, hdr, vr = redraw_views(buf, ns, H, W)
    vx.copy_(x0.to(torch.float16))
    vn.copy_(noise.to(torch.float16))
    vm.copy_(mh)
    hdr.copy_(torch.tensor([1.0 if full_strength else 0.0, float(init_noise_sigma), 0.0, 0.0], dtype=torch.float32))
    vr[:rows.shape[0]].copy_(rows)


def cfg_sampler_step_redraw(eps: Tensor, latents: Tensor, model_in: Tensor, table: Tensor, redraw: Optional[Tensor],
                            kind: int, do_cfg: bool = True, ctr: Optional[Tensor] = None,
                            guidance: Optional[Tensor] = None, solver: Optional[Tensor] = None,
                            prev_x0: Optional[Tensor] = None, seeds: Optional[Tensor] = None) -> None:
    """The sampler step of any kind (`solver` + `prev_x0`: kind 2, `seeds`: kind 3, `guidance`: per panel) followed in
    the same launch by the region-redraw blend out of `redraw` (`redraw_buffer` / `redraw_load`): pixels whose mask is
    1 get exactly the step's result, the others are pulled to the kept latents re-noised with renoise row *ctr + 1."""
    ns, HW = _sampler_step_dims(eps, latents, model_in, table, solver=solver, prev_x0=prev_x0, seeds=seeds,
                                guidance=guidance)
    if redraw is not None:
        _chk(redraw, dtype=torch.uint8)
        redraw_views(redraw, ns, latents.shape[2], latents.shape[3])
    check(_lib.load().ds_cfg_sampler_step_redraw_f16(_p(eps), _p(latents), _p(model_in), _p(table), _p(guidance), _p(solver),
                                                     _p(prev_x0), _p(seeds), _p(redraw), _p(ctr), ns, HW, kind, int(do_cfg),
                                                     _stream()), "ds_cfg_sampler_step_redraw_f16")


def redraw_start(redraw: Tensor, latents: Tensor) -> None:
    """latents [ns,4,H,W] = the start state of a redraw run out of `redraw`: half(ka0 * x0k + kb0 * noise), or
    half(noise * init_noise_sigma) when the buffer's header says full strength."""
    _chk(latents)
    _chk(redraw, dtype=torch.uint8)
    ns, _, H, W = latents.shape
    redraw_views(redraw, ns, H, W)
    check(_lib.load().ds_redraw_start_f16(_p(redraw), _p(latents), ns, H * W, _stream()), "ds_redraw_start_f16")


# ---- panel schedules: the per-slot buffer of include/diffsensei_hip.h ("Panel schedules") and the launches that read it
PANEL_MAX_ROWS = 1024
PANEL_START_RENOISE, PANEL_START_FULL, PANEL_START_KEEP = 0, 1, 2


def panel_schedule_buffer(ns: int, device) -> Tensor:
    """The zeroed uint8 device buffer `start | steps | mode | coef | solver | renoise` for `ns` panel slots, all empty."""
    return torch.zeros(int(_lib.load().ds_panel_schedule_bytes(int(ns))), dtype=torch.uint8, device=device)


def _chk_panel(buf: Tensor, ns: int) -> None:
    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() or buf.data_ptr() % 16:
        raise _lib.DiffSenseiHipError("panel-schedule buffer: a contiguous, 16-byte aligned uint8 vector is needed")
    if buf.numel() != int(_lib.load().ds_panel_schedule_bytes(ns)):
        raise _lib.DiffSenseiHipError(f"panel-schedule buffer: {buf.numel()} bytes do not fit ns={ns}")


def panel_schedule_views(buf: Tensor, ns: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Views of a panel-schedule buffer: start int32 [ns], steps int32 [ns], mode fp32 [ns,4], coef fp32 [ns,R,8], solver
    fp32 [ns,R,8], renoise fp32 [ns,R+1,2] with R = PANEL_MAX_ROWS."""
    _chk_panel(buf, ns)
    R = PANEL_MAX_ROWS
    off = (8 * ns + 15) & ~15
    i32 = buf[:8 * ns].view(torch.int32)
    f32 = buf[off:].view(torch.float32)
    a, b, c = 4 * ns, 4 * ns + 8 * R * ns, 4 * ns + 16 * R * ns
    return (i32[:ns], i32[ns:], f32[:a].view(ns, 4), f32[a:b].view(ns, R, 8), f32[b:c].view(ns, R, 8),
            f32[c:].view(ns, R + 1, 2))


def panel_slot_load(buf: Tensor, ns: int, slot: int, start: int, rows: Optional[Tensor], solver_rows: Optional[Tensor] = None,
                    renoise_rows: Optional[Tensor] = None, start_mode: int = PANEL_START_KEEP,
                    init_noise_sigma: float = 1.0) -> None:
    """Write slot `slot` of a panel-schedule buffer: its schedule begins when the step counter reads `start` and runs
    `rows.shape[0]` rows.  rows: fp32 [steps, 8]; solver_rows: fp32 [steps, 8] (DPM-Solver++); renoise_rows: fp32
    [steps + 1, 2] (region redraw).  Host tensors are copied to the device first; the launch is stream-ordered.
    rows = None empties the slot."""
    _chk(buf, dtype=torch.uint8)
    _chk_panel(buf, ns)
    dev = buf.device
    f = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32).to(dev, non_blocking=True).contiguous()
    rows, solver_rows, renoise_rows = f(rows), f(solver_rows), f(renoise_rows)
    steps = 0 if rows is None else int(rows.shape[0])
    if rows is not None and (rows.dim() != 2 or rows.shape[1] != 8):
        raise ValueError(f"panel_slot_load: rows {tuple(rows.shape)}, [steps, 8] is needed")
    if solver_rows is not None and tuple(solver_rows.shape) != (steps, 8):
        raise ValueError(f"panel_slot_load: solver rows {tuple(solver_rows.shape)} do not match the {steps} rows")
    if renoise_rows is not None and tuple(renoise_rows.shape) != (steps + 1, 2):
        raise ValueError(f"panel_slot_load: renoise rows {tuple(renoise_rows.shape)}, ({steps + 1}, 2) is needed")
    check(_lib.load().ds_panel_slot_load(_p(buf), int(ns), int(slot), int(start), steps, _p(rows), _p(solver_rows),
                                         _p(renoise_rows), int(start_mode), float(init_noise_sigma), _stream()),
          "ds_panel_slot_load")


def cfg_sampler_step_slots(eps: Tensor, latents: Tensor, model_in: Tensor, panel: Tensor, kind: int, ctr: Tensor,
                           guidance: Optional[Tensor], do_cfg: bool = True, prev_x0: Optional[Tensor] = None,
                           seeds: Optional[Tensor] = None, redraw: Optional[Tensor] = None) -> None:
    """The sampler step on panel schedules: panel n runs row `ctr - start[n]` of its own rows in `panel`
    (`panel_schedule_buffer` / `panel_slot_load`) and an inactive panel is left alone.  `redraw`: the region-redraw
    buffer (its kept latents, noise and masks; the renoise rows come from `panel`), None for no blend."""
    ns = latents.shape[0]
    _chk(eps, latents, model_in, prev_x0)
    _chk(guidance, dtype=torch.float32)
    _chk(ctr, dtype=torch.int32)
    _chk(panel, dtype=torch.uint8)
    _chk_panel(panel, ns)
    if guidance is not None and tuple(guidance.shape) != (ns,):
        raise _lib.DiffSenseiHipError(f"guidance {tuple(guidance.shape)}: one fp32 per panel, ({ns},), is needed")
    if prev_x0 is not None and prev_x0.shape != latents.shape:
        raise ValueError(f"prev_x0 {tuple(prev_x0.shape)} must have the latents' shape {tuple(latents.shape)}")
    _chk_seeds(seeds, ns)
    if redraw is not None:
        _chk(redraw, dtype=torch.uint8)
        redraw_views(redraw, ns, latents.shape[2], latents.shape[3])
    check(_lib.load().ds_cfg_sampler_step_slots_f16(_p(eps), _p(latents), _p(model_in), _p(panel), _p(guidance), _p(prev_x0),
                                                    _p(seeds), _p(redraw), _p(ctr), ns, latents.shape[2] * latents.shape[3],
                                                    int(kind), int(do_cfg), _stream()), "ds_cfg_sampler_step_slots_f16")


def timestep_embed_slots(panel: Tensor, ns: int, B: int, dim: int, ctr: Tensor, flip: bool = True,
                         freq_shift: float = 0.0) -> Tensor:
    """[B, dim] sinusoidal embeddings, row b of the timestep panel b % ns is at (0 for an empty slot)."""
    _chk(panel, dtype=torch.uint8)
    _chk_panel(panel, ns)
    _chk(ctr, dtype=torch.int32)
    out = torch.empty((B, dim), dtype=torch.float16, device=panel.device)
    check(_lib.load().ds_timestep_embed_slots_f16(_p(panel), _p(ctr), _p(out), B, dim, int(flip), freq_shift, int(ns),
                                                  _stream()), "ds_timestep_embed_slots_f16")
    return out


def panel_slot_start(panel: Tensor, redraw: Optional[Tensor], latents: Tensor, model_in: Tensor, slot0: int, nslots: int,
                     do_cfg: bool = True) -> None:
    """Start state and first model input of slots [slot0, slot0 + nslots): see `ds_panel_slot_start_f16`."""
    _chk(latents, model_in)
    ns, _, H, W = latents.shape
    _chk(panel, dtype=torch.uint8)
    _chk_panel(panel, ns)
    if redraw is not None:
        _chk(redraw, dtype=torch.uint8)
        redraw_views(redraw, ns, H, W)
    check(_lib.load().ds_panel_slot_start_f16(_p(panel), _p(redraw), _p(latents), _p(model_in), ns, H * W, int(do_cfg),
                                              int(slot0), int(nslots), _stream()), "ds_panel_slot_start_f16")


def philox_u32(seeds: Tensor, step: int, HW: int, stream_id: int = 0) -> Tensor:
    """Raw Philox4x32-10 words, int32 [ns,HW,4] holding the uint32 bit patterns (include/diffsensei_hip.h)."""
    ns = seeds.shape[0]
    _chk_seeds(seeds, ns)
    out = torch.empty((ns, HW, 4), dtype=torch.int32, device=seeds.device)
    check(_lib.load().ds_philox_u32(_p(seeds), int(step), int(stream_id), _p(out), ns, HW, _stream()), "ds_philox_u32")
    return out


def philox_normal(seeds: Tensor, step: int, HW: int, stream_id: int = 0) -> Tensor:
    """The sampler's noise on its own: fp32 [ns,4,HW] standard normals for (seeds[n], pixel, step, stream_id)."""
    ns = seeds.shape[0]
    _chk_seeds(seeds, ns)
    out = torch.empty((ns, 4, HW), dtype=torch.float32, device=seeds.device)
    check(_lib.load().ds_philox_normal_f32(_p(seeds), int(step), int(stream_id), _p(out), ns, HW, _stream()),
          "ds_philox_normal_f32")
    return out


def prepare_model_input(latents: Tensor, model_in: Tensor, table: Tensor, do_cfg: bool = True,
                        ctr: Optional[Tensor] = None) -> None:
    _chk(latents, model_in)
    ns = latents.shape[0]
    HW = latents.shape[2] * latents.shape[3]
    check(_lib.load().ds_prepare_model_input_f16(_p(latents), _p(model_in), _p(table), _p(ctr), ns, HW, int(do_cfg),
                                                 _stream()), "ds_prepare_model_input_f16")


def nhwc_to_nchw(x: Tensor) -> Tensor:
    """[B,HW,C] -> [B,C,HW]"""
    _chk(x)
    B, HW, Cc = x.shape
    y = torch.empty((B, Cc, HW), dtype=torch.float16, device=x.device)
    check(_lib.load().ds_nhwc_to_nchw_f16(_p(x), _p(y), B, HW, Cc, _stream()), "ds_nhwc_to_nchw_f16")
    return y


def nchw_to_nhwc(x: Tensor) -> Tensor:
    """[B,C,HW] -> [B,HW,C]"""
    _chk(x)
    B, Cc, HW = x.shape
    y = torch.empty((B, HW, Cc), dtype=torch.float16, device=x.device)
    check(_lib.load().ds_nchw_to_nhwc_f16(_p(x), _p(y), B, HW, Cc, _stream()), "ds_nchw_to_nhwc_f16")
    return y


def pad_rows(x: Tensor, row_off: int, rows_in: int, rows_out: int) -> Tensor:
    """x: [B,total_rows,C] -> [B,rows_out,C] = x[:, row_off:row_off+rows_in] zero-padded."""
    _chk(x)
    B, T, Cc = x.shape
    y = torch.empty((B, rows_out, Cc), dtype=torch.float16, device=x.device)
    check(_lib.load().ds_pad_rows_f16(_p(x), _p(y), B, rows_in, rows_out, row_off, T, Cc, _stream()), "ds_pad_rows_f16")
    return y


# ------------------------------------------------------------------------------------------------ bf16 (VAE decoder)
_BF = torch.bfloat16


def conv3x3_bf16(x: Tensor, w: Tensor, bias: Tensor, upsample: bool = False, residual: Optional[Tensor] = None) -> Tensor:
    """x: [B,H,W,Cin] bf16 NHWC, w: [Cout,3,3,Cin] -> [B,Ho,Wo,Cout] (stride 1; upsample = nearest x2 in front)."""
    _chk(x, w, bias, residual, dtype=_BF)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    y = torch.empty((B, Ho, Wo, Cout), dtype=_BF, device=x.device)
    check(_lib.load().ds_conv3x3_bf16(_p(x), _p(w), _p(bias), _p(residual), _p(y), B, H, W, Cin, Cout, int(upsample),
                                      _stream()), "ds_conv3x3_bf16")
    return y


def gemm_bf16(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None) -> Tensor:
    """y = x @ w.T + bias (+ residual), all bf16; M, N multiples of 16, K of 128."""
    _chk(x, w, bias, residual, dtype=_BF)
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=_BF, device=x.device)
    check(_lib.load().ds_gemm_bf16(_p(x), K, _p(w), K, _p(bias), _p(residual), N, _p(y), N, M, N, K, _stream()),
          "ds_gemm_bf16")
    return y


def gemm_batched_nt_bf16(a: Tensor, b: Tensor) -> Tensor:
    """out[z] = a @ b[z].T ; a: [M,K] shared, b: [Z,N,K] -> [Z,M,N] (V^T[z] = Wv @ X_z^T)."""
    _chk(a, b, dtype=_BF)
    Z, N, K = b.shape
    M = a.shape[0]
    out = torch.empty((Z, M, N), dtype=_BF, device=b.device)
    check(_lib.load().ds_gemm_bf16_batched(_p(a), K, 0, _p(b), K, N * K, _p(out), N, M * N, M, N, K, Z, _stream()),
          "ds_gemm_bf16_batched")
    return out


def groupnorm_bf16(x: Tensor, gamma: Tensor, beta: Tensor, groups: int, eps: float, silu: bool) -> Tensor:
    """x: [B,HW,C] bf16 -> GroupNorm (+SiLU)."""
    _chk(x, gamma, beta, dtype=_BF)
    B, HW, C = x.shape
    L = _lib.load()
    ws = torch.empty(L.ds_groupnorm_workspace_bytes(B, C), dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    check(L.ds_groupnorm_bf16(_p(x), _p(y), _p(gamma), _p(beta), _p(ws), B, HW, C, groups, eps, int(silu), _stream()),
          "ds_groupnorm_bf16")
    return y


def wide_attention_bf16(q: Tensor, k: Tensor, vt: Tensor, scale: float, n_valid: int = 0) -> Tensor:
    """Single head of dim 512: q, k [B,N,512], vt [B,512,N] -> [B,N,512]; keys >= n_valid (0 = all) are padding."""
    _chk(q, k, vt, dtype=_BF)
    B, N, D = q.shape
    assert D == 512 and vt.shape == (B, 512, N)
    o = torch.empty_like(q)
    check(_lib.load().ds_wide_attn_bf16(_p(q), _p(k), _p(vt), _p(o), B, N, int(n_valid), scale, _stream()),
          "ds_wide_attn_bf16")
    return o


def vae_conv_in(latents: Tensor, pq_w: Tensor, pq_b: Tensor, w: Tensor, bias: Tensor, scaling_factor: float) -> Tensor:
    """latents fp32 NCHW [B,4,H,W]; pq_w [4,4], pq_b [4] fp32; w [C,3,3,4], bias [C] bf16 -> [B,H,W,C] bf16."""
    _chk(latents, pq_w, pq_b, dtype=torch.float32)
    _chk(w, bias, dtype=w.dtype)
    B, _, H, W = latents.shape
    C = w.shape[0]
    y = torch.empty((B, H, W, C), dtype=w.dtype, device=latents.device)
    L = _lib.load()
    fn, name = (L.ds_vae_conv_in_bf16, "ds_vae_conv_in_bf16") if w.dtype == _BF else (L.ds_vae_conv_in_f16, "ds_vae_conv_in_f16")
    check(fn(_p(latents), _p(pq_w), _p(pq_b), _p(w), _p(bias), _p(y), B, H, W, C, scaling_factor, _stream()), name)
    return y


def vae_conv_out(x: Tensor, w: Tensor, bias: Tensor, denormalize: bool = False) -> Tensor:
    """x [B,H,W,C] bf16 (or f16), w [3,3,3,C], bias [3] same dtype -> image fp32 NCHW [B,3,H,W] (denormalize: (y/2+0.5).clamp(0,1))."""
    _chk(x, w, bias, dtype=x.dtype)
    B, H, W, C = x.shape
    img = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
    L = _lib.load()
    fn, name = (L.ds_vae_conv_out_bf16, "ds_vae_conv_out_bf16") if x.dtype == _BF else (L.ds_vae_conv_out_f16, "ds_vae_conv_out_f16")
    check(fn(_p(x), _p(w), _p(bias), _p(img), B, H, W, C, int(denormalize), _stream()), name)
    return img


# ---- VAE encoder (vae.py VaeEncoderEngine): the four ops the decoder has no counterpart of
def conv3x3_down(x: Tensor, w: Tensor, bias: Tensor) -> Tensor:
    """diffusers' Downsample2D(padding=0): F.pad(x, (0,1,0,1)) + 3x3 conv, stride 2.  x [B,H,W,Cin] NHWC f16 or bf16,
    w [Cout,3,3,Cin] -> [B,H//2,W//2,Cout]."""
    _chk(x, w, bias, dtype=x.dtype)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    if H < 2 or W < 2 or tuple(w.shape[1:]) != (3, 3, Cin):
        raise ValueError(f"conv3x3_down: x {tuple(x.shape)}, w {tuple(w.shape)}")
    y = torch.empty((B, H // 2, W // 2, Cout), dtype=x.dtype, device=x.device)
    L = _lib.load()
    fn, name = (L.ds_conv3x3_down_bf16, "ds_conv3x3_down_bf16") if x.dtype == _BF else (L.ds_conv3x3_down_f16, "ds_conv3x3_down_f16")
    check(fn(_p(x), _p(w), _p(bias), _p(y), B, H, W, Cin, Cout, _stream()), name)
    return y


def vae_enc_conv_in(image: Tensor, w: Tensor, bias: Tensor) -> Tensor:
    """image: uint8 NHWC [B,H,W,3] (normalised to 2 u / 255 - 1 in the kernel) or fp32 NCHW [B,3,H,W] in [-1, 1];
    w [C,3,3,3], bias [C] f16 or bf16 -> [B,H,W,C] in that type."""
    _chk(w, bias, dtype=w.dtype)
    if image.dtype == torch.uint8:
        _chk(image, dtype=torch.uint8)
        if image.dim() != 4 or image.shape[3] != 3:
            raise ValueError(f"vae_enc_conv_in: uint8 image [B,H,W,3] expected, got {tuple(image.shape)}")
        B, H, W, _ = image.shape
    else:
        _chk(image, dtype=torch.float32)
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError(f"vae_enc_conv_in: fp32 image [B,3,H,W] expected, got {tuple(image.shape)}")
        B, _, H, W = image.shape
    C = w.shape[0]
    if tuple(w.shape[1:]) != (3, 3, 3):
        raise ValueError(f"vae_enc_conv_in: w [C,3,3,3] expected, got {tuple(w.shape)}")
    y = torch.empty((B, H, W, C), dtype=w.dtype, device=image.device)
    L = _lib.load()
    fn, name = (L.ds_vae_enc_conv_in_bf16, "ds_vae_enc_conv_in_bf16") if w.dtype == _BF else (L.ds_vae_enc_conv_in_f16, "ds_vae_enc_conv_in_f16")
    check(fn(_p(image), int(image.dtype == torch.uint8), _p(w), _p(bias), _p(y), B, H, W, C, _stream()), name)
    return y


def vae_enc_conv_out(x: Tensor, w: Tensor, bias: Tensor) -> Tensor:
    """x [B,H,W,C] f16 or bf16, w [8,3,3,C] same type (quant_conv folded in: vae.fold_quant_conv), bias fp32 [8] ->
    posterior moments fp32 NCHW [B,8,H,W]: 4 x mean, 4 x logvar clamped to [-30, 20]."""
    _chk(x, w, dtype=x.dtype)
    _chk(bias, dtype=torch.float32)
    B, H, W, C = x.shape
    if tuple(w.shape) != (8, 3, 3, C) or bias.numel() != 8:
        raise ValueError(f"vae_enc_conv_out: w [8,3,3,{C}] and bias [8] expected, got {tuple(w.shape)}, {tuple(bias.shape)}")
    mom = torch.empty((B, 8, H, W), dtype=torch.float32, device=x.device)
    L = _lib.load()
    fn, name = (L.ds_vae_enc_conv_out_bf16, "ds_vae_enc_conv_out_bf16") if x.dtype == _BF else (L.ds_vae_enc_conv_out_f16, "ds_vae_enc_conv_out_f16")
    check(fn(_p(x), _p(w), _p(bias), _p(mom), B, H, W, C, _stream()), name)
    return mom


def vae_latents(moments: Tensor, scale: Sequence[float], shift: Optional[Sequence[float]] = None,
                seeds: Optional[Tensor] = None) -> Tensor:
    """moments fp32 [B,8,h,w] -> fp16 latents [B,4,h,w] = fp16((z - shift[c]) * scale[c]); z = mean, or with `seeds` (device
    int64 [B]) mean + exp(0.5 logvar) * Philox normal (seeds[b], pixel, step 0, stream_id 1).  scale / shift: 4 host floats."""
    import ctypes
    _chk(moments, dtype=torch.float32)
    if moments.dim() != 4 or moments.shape[1] != 8:
        raise ValueError(f"vae_latents: moments [B,8,h,w] expected, got {tuple(moments.shape)}")
    B, _, h, w = moments.shape
    if seeds is not None:
        _chk_seeds(seeds, B)
    if len(scale) != 4 or (shift is not None and len(shift) != 4):
        raise ValueError("vae_latents: scale and shift hold one value per latent channel (4)")
    sc = (ctypes.c_float * 4)(*[float(v) for v in scale])
    sh = (ctypes.c_float * 4)(*[float(v) for v in shift]) if shift is not None else None
    out = torch.empty((B, 4, h, w), dtype=torch.float16, device=moments.device)
    check(_lib.load().ds_vae_latents_f16(_p(moments), _p(seeds), sh, sc, _p(out), B, h * w, _stream()), "ds_vae_latents_f16")
    return out


# ---- f16 twins used by the decoder's scaled-fp16 mode (vae.py)
def groupnorm_scaled(x: Tensor, gamma: Tensor, beta: Tensor, groups: int, eps: float, silu: bool, out_scale: float) -> Tensor:
    """x: [B,HW,C] f16 -> act(GroupNorm(x)) * out_scale."""
    _chk(x, gamma, beta)
    B, HW, C = x.shape
    L = _lib.load()
    ws = torch.empty(L.ds_groupnorm_workspace_bytes(B, C), dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    check(L.ds_groupnorm_scaled_f16(_p(x), _p(y), _p(gamma), _p(beta), _p(ws), B, HW, C, groups, eps, int(silu),
                                    float(out_scale), _stream()), "ds_groupnorm_scaled_f16")
    return y


def wide_attention_f16(q: Tensor, k: Tensor, vt: Tensor, scale: float, n_valid: int = 0) -> Tensor:
    """`wide_attention_bf16` on f16 tensors."""
    _chk(q, k, vt)
    B, N, D = q.shape
    assert D == 512 and vt.shape == (B, 512, N)
    o = torch.empty_like(q)
    check(_lib.load().ds_wide_attn_f16(_p(q), _p(k), _p(vt), _p(o), B, N, int(n_valid), scale, _stream()), "ds_wide_attn_f16")
    return o


# ---- MLLM pre-pass: LLaMA greedy decoding (csrc/llm.hip) ----------------------------------------------------
def llm_gemv(x: Tensor, w: Tensor, out: Optional[Tensor] = None, residual: Optional[Tensor] = None, rms: bool = False,
             swiglu: bool = False, eps: float = 1e-6, gain: Optional[Tensor] = None) -> Tensor:
    """x: [M<=any, K] rows; w: [N,K] (swiglu: [2N,K] gate rows then up rows).  `rms`: a LlamaRMSNorm in front - with
    `gain` [K] the reference's roundings (f16(gain * f16(x / rms))), without it only the 1/rms scale (gain folded into w by
    the caller).  `residual` may be `out` itself (in-place h += ...)."""
    _chk(x, w, residual, gain)
    assert w.shape[1] == x.shape[1]
    return _llm_proj("ds_llm_gemv_f16", False, x, w, (), out, residual, rms, swiglu, eps, gain)


def _llm_proj(entry: str, strided: bool, x: Tensor, w: Tensor, extra: tuple, out: Optional[Tensor], residual: Optional[Tensor],
              rms: bool, swiglu: bool, eps: float, gain: Optional[Tensor], M: Optional[int] = None,
              N: Optional[int] = None) -> Tensor:
    """The body of the six projection wrappers, which check their operands' types first.  `entry`: the library's entry
    point; `extra`: the weight format's operands behind eps (w_scale, w_exp).  The gemv family (`strided` false) takes whole
    contiguous tensors and passes K / N as leading dimensions; the gemm16 family takes the `M` / `N` restrictions and passes
    row strides."""
    K = x.shape[1]
    rows = w.shape[0] // (2 if swiglu else 1)
    M = x.shape[0] if M is None else int(M)
    N = rows if N is None else int(N)
    if strided:
        assert 0 < M <= x.shape[0] and 0 < N <= rows and (not swiglu or N == rows)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=x.device)
    _chk(out)
    ldx, ldy, ldr = K, N, N
    if strided:
        assert out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= M and out.shape[1] >= N
        ldx, ldy, ldr = x.stride(0), out.stride(0), 0
        if residual is not None:
            assert residual.dim() == 2 and residual.stride(1) == 1 and residual.shape[0] >= M and residual.shape[1] >= N
            ldr = residual.stride(0)
    check(getattr(_lib.load(), entry)(_p(x), ldx, _p(w), _p(out), ldy, _p(residual), ldr, M, N, K, int(rms), _p(gain),
                                      int(swiglu), eps, *(_p(t) for t in extra), _stream()), entry)
    return out


def llm_attention(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, rope_cos: Tensor, rope_sin: Tensor, state: Tensor,
                  heads: int, kv_heads: int, scale: float, out: Optional[Tensor] = None) -> Tensor:
    """qkv: [M,(heads+2*kv_heads)*D] un-rotated; caches [T_max, kv_heads*D]; appends the M rows at state[0].."""
    return _llm_attn(False, qkv, k_cache, v_cache, None, rope_cos, rope_sin, state, heads, kv_heads, scale, out)


def _llm_attn(slots: bool, qkv: Tensor, k_cache: Tensor, v_cache: Tensor, exps: Optional[tuple], rope_cos: Tensor,
              rope_sin: Tensor, state: Tensor, heads: int, kv_heads: int, scale: float, out: Optional[Tensor]) -> Tensor:
    """The body of llm_attention, llm_attention_slots and their fp8-cache forms (`exps`: (k_exp, v_exp), or None for fp16
    caches).  `slots`: one cache [T_max, ...] per row of qkv behind a leading slot dimension, and state int32 [S, 8]."""
    _chk(qkv)
    _chk(rope_cos, rope_sin, dtype=torch.float32)
    _chk(state, dtype=torch.int32)
    M = qkv.shape[0]
    D = qkv.shape[1] // (heads + 2 * kv_heads)
    T_max = k_cache.shape[-2]
    lead = (M, T_max) if slots else (T_max,)
    if exps is not None:
        _chk_kv8(k_cache, v_cache, *exps, lead, kv_heads, D)
    else:
        _chk(k_cache, v_cache)
        assert k_cache.shape == v_cache.shape == lead + (kv_heads * D,)
    assert rope_cos.shape == (T_max, D // 2) and (not slots or state.shape == (M, 8))
    if out is None:
        out = torch.empty((M, heads * D), dtype=torch.float16, device=qkv.device)
    entry = "ds_llm_attn" + ("_slots" if slots else "") + ("_f16" if exps is None else "_kv8")
    cache = (_p(k_cache), _p(v_cache), k_cache.shape[-1]) + ((k_cache.stride(0),) if slots else ())
    if exps is not None:   # the exponent planes: rows of kv_heads bytes, per slot behind the caches' slot stride
        cache += (_p(exps[0]), _p(exps[1]), kv_heads) + ((exps[0].stride(0),) if slots else ())
    check(getattr(_lib.load(), entry)(_p(qkv), qkv.shape[1], *cache, _p(rope_cos), _p(rope_sin), _p(out), heads * D, _p(state),
                                      M, heads, kv_heads, D, T_max, scale, _stream()), entry)
    return out


def llm_rmsnorm(x: Tensor, gamma: Tensor, eps: float, out: Optional[Tensor] = None, feat: Optional[Tensor] = None,
                state: Optional[Tensor] = None) -> Tensor:
    _chk(x, gamma, feat)
    M, H = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(_lib.load().ds_llm_rmsnorm_f16(_p(x), H, _p(gamma), _p(out), H, _p(feat), _p(state), M, H,
                                         0 if feat is None else feat.shape[0], eps, _stream()), "ds_llm_rmsnorm_f16")
    return out


def llm_embed(table: Tensor, state: Tensor, out: Tensor) -> Tensor:
    _chk(table, out)
    _chk(state, dtype=torch.int32)
    check(_lib.load().ds_llm_embed_f16(_p(table), _p(state), _p(out), table.shape[1], table.shape[0], _stream()),
          "ds_llm_embed_f16")
    return out


def llm_select(logits: Tensor, chain: Optional[Tensor], adv: int, state: Tensor, out_ids: Tensor) -> None:
    """Greedy pick + image-token logits processor + bookkeeping in the device state block (see the header)."""
    _chk(logits)
    _chk(chain, state, out_ids, dtype=torch.int32)
    check(_lib.load().ds_llm_select_f16(_p(logits), logits.numel(), _p(chain), 0 if chain is None else chain.numel(),
                                        out_ids.numel(), adv, _p(state), _p(out_ids), _stream()), "ds_llm_select_f16")


def llm_advance(state: Tensor, rows: int) -> None:
    _chk(state, dtype=torch.int32)
    check(_lib.load().ds_llm_advance(_p(state), rows, _stream()), "ds_llm_advance")


def blend(a: Tensor, b: Tensor, scale: float) -> Tensor:
    """a*scale + b*(1-scale) (fp16, same shape, numel % 8 == 0)."""
    _chk(a, b)
    assert a.shape == b.shape
    out = torch.empty_like(a)
    check(_lib.load().ds_blend_f16(_p(a), _p(b), _p(out), a.numel(), scale, _stream()), "ds_blend_f16")
    return out


def llm_swiglu(gate_up: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """[M, 2I] (gate | up) -> silu(gate) * up  [M, I]."""
    _chk(gate_up, out)
    M, I2 = gate_up.shape
    if out is None:
        out = torch.empty((M, I2 // 2), dtype=torch.float16, device=gate_up.device)
    check(_lib.load().ds_llm_swiglu_f16(_p(gate_up), _p(out), M, I2 // 2, _stream()), "ds_llm_swiglu_f16")
    return out


# ---- batched decode: up to 16 sequences per weight pass (csrc/llm.hip) ----------------------------------------
def llm_gemm16(x: Tensor, w: Tensor, out: Optional[Tensor] = None, residual: Optional[Tensor] = None, rms: bool = False,
               swiglu: bool = False, eps: float = 1e-6, gain: Optional[Tensor] = None, M: Optional[int] = None,
               N: Optional[int] = None) -> Tensor:
    """`llm_gemv` for M <= 16 rows on the matrix pipe: the weights are streamed once for all rows.  `out` / `residual`
    may be larger than [M, N] (their row stride is used; rows past M and columns past N stay untouched); `M` / `N`
    restrict the call to the first rows of `x` / weight rows of `w` (swiglu: `w` must then hold exactly 2N rows)."""
    _chk(x, w, residual, gain)
    assert w.shape[1] == x.shape[1]
    return _llm_proj("ds_llm_gemm16", True, x, w, (), out, residual, rms, swiglu, eps, gain, M, N)


# ---- int8 weight-only decoding (W8A16): the twins of llm_gemv / llm_gemm16 with int8 weights + fp32 row scales -----------
def _chk_w8(x: Tensor, w: Tensor, w_scale: Tensor, swiglu: bool) -> None:
    _chk(w, dtype=torch.int8)
    _chk(w_scale, dtype=torch.float32)
    if w.dim() != 2 or w.shape[1] != x.shape[1] or w.shape[1] % 16:
        raise ValueError(f"int8 weights must be [N, K] with K = {x.shape[1]} a multiple of 16, got {tuple(w.shape)}")
    if swiglu and w.shape[0] % 2:
        raise ValueError("SwiGLU weights hold gate rows then up rows: an even number of rows")
    if w_scale.dim() != 1 or w_scale.shape[0] != w.shape[0]:
        raise ValueError(f"w_scale must be fp32 [{w.shape[0]}] (one scale per weight row), got {tuple(w_scale.shape)}")


def llm_gemv_w8(x: Tensor, w: Tensor, w_scale: Tensor, out: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                rms: bool = False, swiglu: bool = False, eps: float = 1e-6, gain: Optional[Tensor] = None) -> Tensor:
    """`llm_gemv` with int8 weights: w int8 [N,K] (swiglu: [2N,K]), w_scale fp32 [N] ([2N]); y = (x' . q[n]) * w_scale[n]."""
    _chk(x, residual, gain)
    _chk_w8(x, w, w_scale, swiglu)
    return _llm_proj("ds_llm_gemv_w8", False, x, w, (w_scale,), out, residual, rms, swiglu, eps, gain)


def llm_gemm16_w8(x: Tensor, w: Tensor, w_scale: Tensor, out: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                  rms: bool = False, swiglu: bool = False, eps: float = 1e-6, gain: Optional[Tensor] = None,
                  M: Optional[int] = None, N: Optional[int] = None) -> Tensor:
    """`llm_gemm16` with int8 weights and fp32 row scales (`N` restricts the call to the first N rows of w / w_scale)."""
    _chk(x, residual, gain)
    _chk_w8(x, w, w_scale, swiglu)
    return _llm_proj("ds_llm_gemm16_w8", True, x, w, (w_scale,), out, residual, rms, swiglu, eps, gain, M, N)


def llm_dequant_w8(w: Tensor, w_scale: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """f16(f32(w) * w_scale[:, None]) for int8 w [N,K] (K % 16 == 0); `out`: fp16, at least N*K elements, contiguous."""
    _chk(w, dtype=torch.int8)
    _chk(w_scale, dtype=torch.float32)
    N, K = w.shape
    if K % 16 or w_scale.shape != (N,):
        raise ValueError(f"int8 weights [N, K % 16 == 0] with fp32 scales [N] are needed, got {tuple(w.shape)} / {tuple(w_scale.shape)}")
    if out is None:
        out = torch.empty((N, K), dtype=torch.float16, device=w.device)
    _chk(out)
    assert out.numel() >= N * K
    check(_lib.load().ds_llm_dequant_w8(_p(w), _p(w_scale), _p(out), N, K, _stream()), "ds_llm_dequant_w8")
    return out.view(-1)[:N * K].view(N, K)


# ---- MXFP4 weight-only decoding (W4A16): packed e2m1 weights + E8M0 block exponents + fp32 row scales ----------------------
def _chk_fp4(x: Tensor, w: Tensor, w_exp: Tensor, w_scale: Tensor, swiglu: bool) -> None:
    _chk(w, w_exp, dtype=torch.uint8)
    _chk(w_scale, dtype=torch.float32)
    K = x.shape[1]
    if w.dim() != 2 or K % 32 or w.shape[1] * 2 != K:
        raise ValueError(f"MXFP4 weights must be uint8 [N, K/2] with K = {K} a multiple of 32, got {tuple(w.shape)}")
    if swiglu and w.shape[0] % 2:
        raise ValueError("SwiGLU weights hold gate rows then up rows: an even number of rows")
    if w_exp.dim() != 2 or tuple(w_exp.shape) != (w.shape[0], K // 32):
        raise ValueError(f"w_exp must be uint8 [{w.shape[0]}, {K // 32}] (one exponent per 32-element block), got {tuple(w_exp.shape)}")
    if w_scale.dim() != 1 or w_scale.shape[0] != w.shape[0]:
        raise ValueError(f"w_scale must be fp32 [{w.shape[0]}] (one scale per weight row), got {tuple(w_scale.shape)}")


def llm_gemv_fp4(x: Tensor, w: Tensor, w_exp: Tensor, w_scale: Tensor, out: Optional[Tensor] = None,
                 residual: Optional[Tensor] = None, rms: bool = False, swiglu: bool = False, eps: float = 1e-6,
                 gain: Optional[Tensor] = None) -> Tensor:
    """`llm_gemv` with MXFP4 weights (`mllm.quantize_rows_mxfp4`): w uint8 [N,K/2] (swiglu: [2N,K/2]), w_exp uint8 [N,K/32],
    w_scale fp32 [N]; y = (x' . (e2m1 * 2^(w_exp-127))[n]) * w_scale[n]."""
    _chk(x, residual, gain)
    _chk_fp4(x, w, w_exp, w_scale, swiglu)
    return _llm_proj("ds_llm_gemv_fp4", False, x, w, (w_scale, w_exp), out, residual, rms, swiglu, eps, gain)


def llm_gemm16_fp4(x: Tensor, w: Tensor, w_exp: Tensor, w_scale: Tensor, out: Optional[Tensor] = None,
                   residual: Optional[Tensor] = None, rms: bool = False, swiglu: bool = False, eps: float = 1e-6,
                   gain: Optional[Tensor] = None, M: Optional[int] = None, N: Optional[int] = None) -> Tensor:
    """`llm_gemm16` with MXFP4 weights (`N` restricts the call to the first N rows of w / w_exp / w_scale)."""
    _chk(x, residual, gain)
    _chk_fp4(x, w, w_exp, w_scale, swiglu)
    return _llm_proj("ds_llm_gemm16_fp4", True, x, w, (w_scale, w_exp), out, residual, rms, swiglu, eps, gain, M, N)


def llm_dequant_fp4(w: Tensor, w_exp: Tensor, w_scale: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """f16(f32(e2m1 * 2^(w_exp-127)) * w_scale[:, None]) for MXFP4 w [N,K/2] (K % 32 == 0); `out`: fp16, at least N*K
    elements, contiguous."""
    _chk(w, w_exp, dtype=torch.uint8)
    _chk(w_scale, dtype=torch.float32)
    N, K = w.shape[0], 2 * w.shape[1]
    if w.dim() != 2 or K % 32 or tuple(w_exp.shape) != (N, K // 32) or tuple(w_scale.shape) != (N,):
        raise ValueError(f"MXFP4 weights [N, K/2] (K % 32 == 0) with exponents [N, K/32] and fp32 scales [N] are needed, got "
                         f"{tuple(w.shape)} / {tuple(w_exp.shape)} / {tuple(w_scale.shape)}")
    if out is None:
        out = torch.empty((N, K), dtype=torch.float16, device=w.device)
    _chk(out)
    assert out.numel() >= N * K
    check(_lib.load().ds_llm_dequant_fp4(_p(w), _p(w_scale), _p(out), N, K, _p(w_exp), _stream()), "ds_llm_dequant_fp4")
    return out.view(-1)[:N * K].view(N, K)


def llm_attention_slots(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, rope_cos: Tensor, rope_sin: Tensor, state: Tensor,
                        heads: int, kv_heads: int, scale: float, out: Optional[Tensor] = None) -> Tensor:
    """One new row per slot: qkv [S,(heads+2*kv_heads)*D]; caches [S, T_max, kv_heads*D]; state int32 [S, 8].  Slot s
    appends at state[s][0] in its own cache; a slot with state[s][2] set is left alone."""
    return _llm_attn(True, qkv, k_cache, v_cache, None, rope_cos, rope_sin, state, heads, kv_heads, scale, out)


def _chk_kv8(k_cache: Tensor, v_cache: Tensor, k_exp: Tensor, v_exp: Tensor, lead: tuple, kv_heads: int, D: int) -> None:
    _chk(k_cache, v_cache, k_exp, v_exp, dtype=torch.uint8)
    if tuple(k_cache.shape) != lead + (kv_heads * D,) or v_cache.shape != k_cache.shape:
        raise ValueError(f"fp8 caches must be uint8 {lead + (kv_heads * D,)}, got {tuple(k_cache.shape)} / {tuple(v_cache.shape)}")
    if tuple(k_exp.shape) != lead + (kv_heads,) or v_exp.shape != k_exp.shape:
        raise ValueError(f"cache exponents must be uint8 {lead + (kv_heads,)} (one per row and kv head), got "
                         f"{tuple(k_exp.shape)} / {tuple(v_exp.shape)}")


def llm_attention_kv8(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, k_exp: Tensor, v_exp: Tensor, rope_cos: Tensor,
                      rope_sin: Tensor, state: Tensor, heads: int, kv_heads: int, scale: float,
                      out: Optional[Tensor] = None) -> Tensor:
    """`llm_attention` on the fp8 KV cache (mllm.quantize_kv_fp8): caches uint8 [T_max, kv_heads*D] of e4m3 codes, exponents
    uint8 [T_max, kv_heads]; appends the codes and exponent bytes of the M rows at state[0].. and attends over the dequantised
    cache, the rows of this launch included."""
    return _llm_attn(False, qkv, k_cache, v_cache, (k_exp, v_exp), rope_cos, rope_sin, state, heads, kv_heads, scale, out)


def llm_attention_slots_kv8(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, k_exp: Tensor, v_exp: Tensor, rope_cos: Tensor,
                            rope_sin: Tensor, state: Tensor, heads: int, kv_heads: int, scale: float,
                            out: Optional[Tensor] = None) -> Tensor:
    """`llm_attention_slots` on the fp8 KV cache: caches uint8 [S, T_max, kv_heads*D], exponents uint8 [S, T_max, kv_heads]."""
    return _llm_attn(True, qkv, k_cache, v_cache, (k_exp, v_exp), rope_cos, rope_sin, state, heads, kv_heads, scale, out)


def llm_rmsnorm_slots(x: Tensor, gamma: Tensor, eps: float, out: Optional[Tensor] = None, feat: Optional[Tensor] = None,
                      state: Optional[Tensor] = None) -> Tensor:
    """x [S,H]; feat [S, max_out, H] (optional) receives row s at state[s][1]-1 unless slot s is finished."""
    _chk(x, gamma, feat)
    S, H = x.shape
    if out is None:
        out = torch.empty_like(x)
    if feat is not None:
        _chk(state, dtype=torch.int32)
        assert feat.shape[0] == S and feat.shape[2] == H and state.shape == (S, 8)
    check(_lib.load().ds_llm_rmsnorm_slots_f16(_p(x), H, _p(gamma), _p(out), H, _p(feat), _p(state), S, H,
                                               0 if feat is None else feat.shape[1], eps, _stream()),
          "ds_llm_rmsnorm_slots_f16")
    return out


def llm_embed_slots(table: Tensor, state: Tensor, out: Tensor) -> Tensor:
    _chk(table, out)
    _chk(state, dtype=torch.int32)
    S = state.shape[0]
    assert state.shape == (S, 8) and out.shape == (S, table.shape[1])
    check(_lib.load().ds_llm_embed_slots_f16(_p(table), _p(state), _p(out), out.stride(0), S, table.shape[1],
                                             table.shape[0], _stream()), "ds_llm_embed_slots_f16")
    return out


def llm_select_slots(logits: Tensor, chain: Optional[Tensor], adv: int, state: Tensor, out_ids: Tensor,
                     pause: bool = False) -> None:
    """`llm_select` per slot: logits [S,V], state int32 [S,8] (eos and max_new per slot), out_ids int32 [S,cap].
    pause (chain fast-forward): a slot that did not finish and whose new id lies in chain[:-1] gets state[s][2] = 2; that form
    has no exported entry point and runs as DS_OP_LLM_SELECT_SLOTS with i[5] = 1."""
    _chk(logits)
    _chk(chain, state, out_ids, dtype=torch.int32)
    S, V = logits.shape
    assert state.shape == (S, 8) and out_ids.shape[0] == S
    n_chain = 0 if chain is None else chain.numel()
    if pause:
        import ctypes
        op = _lib.DsOp()
        op.code = _lib.OP["LLM_SELECT_SLOTS"]
        for k, v in enumerate((V, n_chain, out_ids.shape[1], adv, S, 1)):
            op.i[k] = int(v)
        op.l[0] = int(logits.stride(0))
        for k, t in enumerate((logits, chain, state, out_ids)):
            op.p[k] = _p(t)
        check(_lib.load().ds_op_run(ctypes.byref(op), _stream()), "ds_op_run(LLM_SELECT_SLOTS)")
        return
    check(_lib.load().ds_llm_select_slots_f16(_p(logits), logits.stride(0), V, _p(chain), n_chain, out_ids.shape[1], adv,
                                              _p(state), _p(out_ids), S, _stream()), "ds_llm_select_slots_f16")


def llm_attention_rows(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, rope_cos: Tensor, rope_sin: Tensor, state: Tensor,
                       table: Tensor, heads: int, kv_heads: int, scale: float, out: Optional[Tensor] = None,
                       k_exp: Optional[Tensor] = None, v_exp: Optional[Tensor] = None) -> Tensor:
    """Ragged attention over the rows of several slots in one launch (llm_attn_rows_kernel through DS_OP_LLM_ATTN_ROWS[_KV8];
    there is no exported entry point).  qkv [R,(heads+2*kv_heads)*D] un-rotated; caches [S, T_max, kv_heads*D] (fp16, or uint8
    codes with `k_exp` / `v_exp` uint8 [S, T_max, kv_heads]: the fp8 cache); state int32 [S, 8]; table int32 [R, 2] on the
    device, row R = (slot, r): row R of qkv / out is row r of that slot's segment, a run of consecutive rows (any length) that
    starts at cache length state[slot][0].  Row r attends over the slot's cache and the segment's rows 0..r and appends its K
    and V at state[slot][0] + r; state[slot][2] is not looked at and the state is not written.  Per row the bits are those of
    `llm_attention` / `llm_attention_kv8` fed the same segment in chunks with the cursor at the start length."""
    import ctypes
    kv8 = k_exp is not None or v_exp is not None
    _chk(qkv)
    _chk(rope_cos, rope_sin, dtype=torch.float32)
    _chk(state, table, dtype=torch.int32)
    R = qkv.shape[0]
    D = qkv.shape[1] // (heads + 2 * kv_heads)
    S, T_max = k_cache.shape[0], k_cache.shape[1]
    if kv8:
        _chk_kv8(k_cache, v_cache, k_exp, v_exp, (S, T_max), kv_heads, D)
    else:
        _chk(k_cache, v_cache)
        assert k_cache.shape == v_cache.shape == (S, T_max, kv_heads * D)
    assert state.shape == (S, 8) and rope_cos.shape == (T_max, D // 2)
    if tuple(table.shape) != (R, 2) or not table.is_contiguous():
        raise ValueError(f"llm_attention_rows: the row table must be a contiguous int32 [{R}, 2], got {tuple(table.shape)}")
    if out is None:
        out = torch.empty((R, heads * D), dtype=torch.float16, device=qkv.device)
    assert out.shape == (R, heads * D) and out.is_contiguous() and qkv.is_contiguous()
    op = _lib.DsOp()
    op.code = _lib.OP["LLM_ATTN_ROWS_KV8" if kv8 else "LLM_ATTN_ROWS"]
    for k, v in enumerate((R, heads, kv_heads, D, T_max, S)):
        op.i[k] = int(v)
    op.f[0] = float(scale)
    for k, v in enumerate((qkv.shape[1], k_cache.shape[2], heads * D, k_cache.stride(0))
                          + ((kv_heads, k_exp.stride(0)) if kv8 else ())):
        op.l[k] = int(v)
    for k, t in enumerate((qkv, k_cache, v_cache, rope_cos, rope_sin, out, state, k_exp, v_exp, table)):
        op.p[k] = _p(t)
    check(_lib.load().ds_op_run(ctypes.byref(op), _stream()), "ds_op_run(LLM_ATTN_ROWS)")
    return out


def image_to_u8(image: Tensor) -> Tensor:
    """[B,3,H,W] fp32 in [0,1] -> [B,H,W,3] uint8 = (x*255).round() (half to even), the PIL tail of `postprocess`."""
    _chk(image, dtype=torch.float32)
    B, Cc, H, W = image.shape
    if Cc != 3:
        raise _lib.DiffSenseiHipError("image_to_u8: 3 channels expected")
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=image.device)
    check(_lib.load().ds_image_f32_to_u8_nhwc(_p(image), _p(out), B, H, W, _stream()), "ds_image_f32_to_u8_nhwc")
    return out


# ------------------------------------------------------------------------------------------------ LoRA merge
def _chk_rows(t: Optional[Tensor], what: str) -> None:
    """An f16 matrix whose rows are contiguous (a row or column slice of a larger buffer is fine: the row stride travels
    as the leading dimension)."""
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.DiffSenseiHipError("diffsensei_amd ops need CUDA(HIP) tensors — there is no CPU path")
    bind_device(t.device)
    if t.dtype != torch.float16 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise _lib.DiffSenseiHipError(f"lora_merge: {what} must be an fp16 matrix with contiguous rows")


def lora_merge_op(W: Tensor, out: Tensor, A: Optional[Tensor] = None, B: Optional[Tensor] = None,
                  seg: Optional[Tensor] = None, s: Optional[Tensor] = None, map: Optional[Tensor] = None,
                  colscale: Optional[Tensor] = None, out2: Optional[Tensor] = None, nseg: Optional[int] = None,
                  conv_cin: int = 0) -> _lib.DsOp:
    """The DS_OP_LORA_MERGE plan op of `lora_merge` (same operands; `seg` / `s` / `map` are device tensors here)."""
    if W.dim() == 4:
        if conv_cin != W.shape[1] or tuple(W.shape[2:]) != (3, 3) or not W.is_contiguous():
            raise ValueError("lora_merge: a 4-D base is a contiguous [Cout, Cin, 3, 3] weight merged with conv_cin = Cin")
        W = W.reshape(W.shape[0], -1)
    _chk_rows(W, "W"), _chk_rows(out, "out"), _chk_rows(A, "A"), _chk_rows(B, "B"), _chk_rows(out2, "out2")
    _chk(seg, map, dtype=torch.int32)
    _chk(s, dtype=torch.float32)
    _chk(colscale)
    N, K = W.shape
    n = 0 if seg is None else (seg.numel() - 1 if nseg is None else int(nseg))
    R = 0 if A is None else A.shape[0]
    if tuple(out.shape) != (N, K) or (out2 is not None and tuple(out2.shape) != (N, K)):
        raise ValueError(f"lora_merge: out / out2 must be [{N}, {K}] like W")
    if n > 0:
        if A is None or B is None or s is None or A.shape[1] != K or tuple(B.shape) != (N, R):
            raise ValueError(f"lora_merge: A must be [R, {K}] and B [{N}, R] with seg [n + 1] and s [n]")
        if seg.numel() < n + 1 or s.numel() < n:
            raise ValueError(f"lora_merge: {n} adapters need seg [{n + 1}] and s [{n}]")
    if map is not None and map.numel() != N:
        raise ValueError(f"lora_merge: map must be int32 [{N}]")
    if (colscale is None) != (out2 is None) or (colscale is not None and colscale.numel() != K):
        raise ValueError(f"lora_merge: out2 comes with colscale fp16 [{K}]")
    if conv_cin and (conv_cin <= 0 or K != 9 * conv_cin or W.stride(0) != K):
        raise ValueError(f"lora_merge: convolution mode reads a contiguous [N, Cin, 3, 3] base as [N, 9 * Cin]; got K {K}, Cin {conv_cin}")
    op = _lib.DsOp()
    op.code = _lib.OP["LORA_MERGE"]
    for k, v in enumerate((N, K, R, n, conv_cin)):
        op.i[k] = int(v)
    ld = lambda t: 0 if t is None else int(t.stride(0))
    for k, v in enumerate((ld(W), ld(out), ld(A), ld(B), ld(out2))):
        op.l[k] = v
    for k, t in enumerate((W, out, A if n else None, B if n else None, seg if n else None, s if n else None, map, colscale, out2)):
        op.p[k] = _p(t)
    return op


def lora_merge(W: Tensor, A: Optional[Tensor] = None, B: Optional[Tensor] = None, seg=None, s=None,
               out: Optional[Tensor] = None, map: Optional[Tensor] = None, colscale: Optional[Tensor] = None,
               out2: Optional[Tensor] = None, conv_cin: int = 0) -> Tensor:
    """out[n] = f16(f32(W[map[n]]) + sum_i s[i] * B[map[n], seg[i]:seg[i+1]] @ A[seg[i]:seg[i+1]]) (lora_merge_kernel through
    DS_OP_LORA_MERGE; there is no exported entry point).  W [N,K] is the base weight and is never written: `out` must be
    another buffer.  conv_cin = Cin > 0 is the convolution mode: W is a 3x3 weight in checkpoint order ([N, Cin, 3, 3], or its
    [N, 9 * Cin] view), A [R, 9 * Cin] and `out` are in the packed tap-major order k = (ky * 3 + kx) * Cin + ci
    (`engine.pack_conv3x3`), so no adapter gives `out` the bits of pack_conv3x3(W).  A [R,K] / B [N,R]: up to 8 adapters concatenated along the rank; `seg` (n + 1 offsets) and `s` (n
    strengths) may be sequences or device tensors; none: `out` gets the bits of W.  `out` / `out2` may be row or column slices of
    larger buffers.  out2 = f16(f32(out) * f32(colscale)), the fused-LayerNorm copy (`engine.pack_ln_fused`'s gw)."""
    if W.dim() == 4 and W.is_contiguous():
        W = W.reshape(W.shape[0], -1)
    _chk_rows(W, "W")
    dev = W.device
    if seg is not None and not torch.is_tensor(seg):
        seg = torch.tensor([int(v) for v in seg], dtype=torch.int32).to(dev)
    if s is not None and not torch.is_tensor(s):
        s = torch.tensor([float(v) for v in s], dtype=torch.float32).to(dev)
    if seg is not None and seg.numel() < 2:
        seg = s = None
    if out is None:
        out = torch.empty((W.shape[0], W.shape[1]), dtype=torch.float16, device=dev)
    op = lora_merge_op(W, out, A, B, seg, s, map, colscale, out2, conv_cin=conv_cin)
    import ctypes
    check(_lib.load().ds_op_run(ctypes.byref(op), _stream()), "ds_op_run(LORA_MERGE)")
    return out
