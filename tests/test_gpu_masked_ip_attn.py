"""GPU: `ip_attn_kernel` (csrc/attention.hip) - softmax(q kt^T s) vt + ip_scale * softmax(q ki^T s + M(bbox)) vi with the region
mask built in registers - against a plain fp64 reference of the same operation on the CPU, across the kernel's data-dependent paths.

Inputs are seeded fp16 tensors handed to the kernel as they are (no GEMM in front), so the reference sees exactly the kernel's
operands.  The reference: fp64 softmax over the text keys < Lt; fp64 softmax over the IP keys < Li with the additive 0 / -10000 mask
of `oracle.attention_ref.ip_region_mask` (pinned to the reference's own prepare_attention_mask_ip at these layouts by
tests/test_oracle_ip_layouts.py); t + ip_scale * i.  Closeness: the `_close` rule of tests/test_gpu_ops.py at tol = 4e-3
(err <= tol * (max|ref| + 1e-3)), the tolerance this kernel has there - same arithmetic; every measured error goes through
tests/_gates.gate.  Boxes: oracle/ip_box_cases.py, a different set in every batch item.

Which case enters which path of the kernel:
  per-key masking with a mask present   test_token_layouts [d4_t1_k4] [d8_t8_k4] [d16_t8_k8] [d16_t20_k4] [d16_t16_k1] [d0_t16_k4]
                                        (grouped form: [d16_t16_k4] [d16_t16_k5] [d32_t32_k2])
  set_range across 32-bit words         test_token_layouts [d16_t20_k4]: character ranges 16..35, 36..55, 56..75, 76..95
  box lanes 4..7                        test_token_layouts [d16_t8_k8], [d16_t16_k5]; test_region_flags_vs_oracle [8]
  Li = 96 (no padding key)              test_token_layouts [d16_t16_k5] [d32_t32_k2] [d16_t20_k4]
  Lt in {64, 65, 80, 81} (T16 limits)   test_text_lengths [64] [65] [80] [81] (and 1, 33, 96); T16 vs the full kernel bit for bit
                                        wherever both counts lie in (64, 80]
  qt in {2, 4, 8}, ragged tail, partial last tile on the register-staged kernel      test_tile_walk (N = 960, 680, 234)
  wave-dependent block skipping         every case with B = 3 or the 16 x 16 grid: the "wave1" box (only the second wavefront of
                                        a block has that character's keys open)
  strided key / value panels            test_stacked_panels_and_column_slices, test_plan_path
  q / o column slices, guard rows       test_stacked_panels_and_column_slices
  ip_scale_dev                          test_scale_source, test_plan_path
  padding content                       test_padding_content
  per-key masking through the launch plan (Li = 24)     test_unet_forward_two_characters_eight_tokens
"""
import ctypes as C
import functools

import pytest
import torch

from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
LP = 96
TOL = 4e-3

# (B, heads, (mask_h, mask_w)): 63 tokens = less than one tile, wavefronts 2-3 idle, odd width | 234 = one tile + a partial one |
# one whole tile pair | 7.5 tiles | mask_h = 1 (linspace of one step is 0)
SHAPES = [(3, 1, (7, 9)), (3, 3, (18, 13)), (1, 3, (16, 16)), (3, 1, (24, 40)), (1, 1, (1, 40))]
# (n_dummy, tok_per_ip, max_ips); Li = n_dummy + max_ips * tok_per_ip
LAYOUTS = [(16, 16, 4), (4, 1, 4), (8, 8, 4), (16, 8, 8), (16, 16, 5), (32, 32, 2), (16, 16, 1), (16, 20, 4), (0, 16, 4)]


def _lid(v):
    return f"d{v[0]}_t{v[1]}_k{v[2]}"


def _sid(v):
    return f"B{v[0]}h{v[1]}_{v[2][0]}x{v[2][1]}"


def _r(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).half()


@functools.lru_cache(maxsize=None)
def _data(B, heads, hw, Lt, Li, seed=0, qscale=1.0):
    """Seeded operands with zero padding (CPU, fp16).  Cached: the tests share them and never write to them."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * heads + hw[0] * 100 + hw[1] + Lt * 3 + Li)
    N, Cc = hw[0] * hw[1], heads * 64
    q = _r((B, N, Cc), g, qscale)
    kt, ki, vtt, vti = _r((B, LP, Cc), g), _r((B, LP, Cc), g), _r((B, Cc, LP), g), _r((B, Cc, LP), g)
    kt[:, Lt:], ki[:, Li:], vtt[:, :, Lt:], vti[:, :, Li:] = 0, 0, 0, 0
    return q, kt, vtt, ki, vti


def _boxes(hw, max_ips, B):
    from oracle.ip_box_cases import box_cases
    return box_cases(hw[0], hw[1], max_ips, B)


def _ref_parts(q, kt, vtt, ki, vti, bbox, heads, hw, Lt, Li, n_dummy, tok_per_ip, dtype=torch.float64):
    """(text part, IP part) [B,N,C] in `dtype` on the CPU: softmax(q k^T / 8 + mask) v per head, keys < Lt / < Li only."""
    from oracle.attention_ref import ip_region_mask, mask_grid_size
    B, N, Cc = q.shape
    assert mask_grid_size(N, hw[0] / hw[1]) == tuple(hw)   # the grid the reference infers is the one the kernel is told
    mask = ip_region_mask(bbox, N, 1, hw[0] / hw[1], bbox.shape[1] * tok_per_ip, n_dummy)   # [B,1,N,Li] 0 / -10000
    qh = q.to(dtype).view(B, N, heads, 64).transpose(1, 2)

    def part(k, vt, L, m):
        kh = k[:, :L].to(dtype).view(B, L, heads, 64).transpose(1, 2)
        vh = vt[:, :, :L].to(dtype).view(B, heads, 64, L).transpose(-1, -2)
        s = torch.matmul(qh, kh.transpose(-1, -2)) * 0.125
        if m is not None:
            s = s + m.to(dtype)
        return torch.matmul(torch.softmax(s, dim=-1), vh).transpose(1, 2).reshape(B, N, Cc)

    return part(kt, vtt, Lt, None), part(ki, vti, Li, mask)


@functools.lru_cache(maxsize=None)
def _case(B, heads, hw, Lt, layout, seed=0, qscale=1.0):
    """operands, boxes and the fp64 reference parts of one configuration (computed once, shared, never written to)"""
    nd, tpi, K = layout
    Li = nd + K * tpi
    ops_ = _data(B, heads, hw, Lt, Li, seed, qscale)
    bbox = _boxes(hw, K, B)
    t, i = _ref_parts(*ops_, bbox, heads, hw, Lt, Li, nd, tpi)
    return ops_, bbox, t, i


def _err(got, ref):
    """the `_close` rule of tests/test_gpu_ops.py as one number: err <= tol * max(max|ref|, 1e-3) + 1e-3 * tol"""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return (got - ref).abs().max().item() / (max(ref.abs().max().item(), 1e-3) + 1e-3)


def _run(ops, operands, bbox, heads, hw, Lt, layout, ip_scale=0.6, **kw):
    nd, tpi, K = layout
    dev = [t.to(DEV) if t.device.type == "cpu" else t for t in operands]
    return ops.masked_ip_attention(*dev, bbox.to(DEV), heads, hw, ip_scale, Lt=Lt, Li=nd + K * tpi, n_dummy=nd,
                                   tok_per_ip=tpi, **kw)


def _check_layout(hip_lib, ops, B, heads, hw, Lt, layout):
    nd, tpi, K = layout
    Li = nd + K * tpi
    operands, bbox, t, i = _case(B, heads, hw, Lt, layout)
    y = _run(ops, operands, bbox, heads, hw, Lt, layout)
    tol = TOL
    if nd == 0:
        # No dummy keys: a token outside every box has -10000 on EVERY key, and fp32 fma(raw, scale, -10000) keeps the logit only
        # to ulp(1e4)/2 = 4.9e-4.  The floor is the deviation of the fp32 oracle (`sdpa` with the mask) from the fp64 reference on
        # these very inputs, measured here on the CPU: 1.1e-4 - 1.6e-4 over the five shapes, so 3x it stays below 4e-3 and the
        # gate is 4e-3 like everywhere else.
        from oracle.attention_ref import ip_region_mask, sdpa
        q, kt, vtt, ki, vti = (x.float() for x in operands)
        m = ip_region_mask(bbox, q.shape[1], 1, hw[0] / hw[1], K * tpi, nd)
        hd = lambda x, L: x[:, :L].reshape(B, L, heads, 64).transpose(1, 2)
        qh = q.view(B, -1, heads, 64).transpose(1, 2)
        i32 = sdpa(qh, hd(ki, Li), vti[:, :, :Li].reshape(B, heads, 64, Li).transpose(-1, -2), m)
        i32 = i32.transpose(1, 2).reshape(q.shape)
        floor = gate(f"ip attn {_lid(layout)} {_sid((B, heads, hw))}: fp32 oracle vs fp64 reference (CPU floor)",
                     _err(t + 0.6 * i32.double(), t + 0.6 * i), TOL)
        tol = max(TOL, 3 * floor)
    gate(f"ip attn {_lid(layout)} Lt={Lt} {_sid((B, heads, hw))} vs fp64 reference", _err(y, t + 0.6 * i), tol)
    if 64 < Lt <= 80 and 64 < Li <= 80:   # the T16 instantiation ran: the same kernel over all 96 key slots gives the same bits
        try:
            hip_lib.ds_set_option(b"ip_attn_variant", 3)
            y3 = _run(ops, operands, bbox, heads, hw, Lt, layout)
        finally:
            hip_lib.ds_set_option(b"ip_attn_variant", 0)
        assert torch.equal(y3, y), "T16 (padding keys 80..95 not issued) differs from the full kernel"


# ------------------------------------------------------------------------------------------------ a. token layouts
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
def test_token_layouts(hip_lib, layout, shape):
    from diffsensei_amd import ops
    _check_layout(hip_lib, ops, *shape, 77, layout)


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("Lt", [1, 33, 64, 65, 80, 81, 96])
def test_text_lengths(hip_lib, Lt, shape):
    from diffsensei_amd import ops
    _check_layout(hip_lib, ops, *shape, Lt, (16, 16, 4))


# ------------------------------------------------------------------------------------------------ b. box geometry
@pytest.mark.parametrize("max_ips", [1, 4, 8])
def test_region_flags_vs_oracle(hip_lib, max_ips):
    """`ops.ip_region_flags` (the kernel's own inside test) against `ip_region_mask`, bit for bit, on every grid and box set."""
    from diffsensei_amd import ops
    from oracle.attention_ref import ip_region_mask
    for _, _, hw in SHAPES + [(3, 1, (20, 34))]:
        N = hw[0] * hw[1]
        bbox = _boxes(hw, max_ips, 3)
        m = ip_region_mask(bbox, N, 1, hw[0] / hw[1], max_ips, 1)[:, 0]                     # [3,N,1+K]
        flags = ops.ip_region_flags(bbox.to(DEV), N, hw).cpu()
        inside = torch.stack([(flags >> k) & 1 for k in range(max_ips)], -1).bool()
        assert torch.equal(inside, m[:, :, 1:] == 0), (hw, max_ips)
        assert torch.equal(m[:, :, 0] == 0, ~inside.any(-1)), (hw, max_ips)
        assert max_ips == 8 or (flags >> max_ips).eq(0).all()


# ------------------------------------------------------------------------------------------------ c. tile walk
def _qt(N, bh, min_blocks):
    """the launcher's rule (ds_launch_ip_attn): double the tiles per block while the grid keeps `min_blocks` blocks"""
    tiles, qt = (N + 127) // 128, 1
    while qt < 8 and (tiles + 2 * qt - 1) // (2 * qt) * bh >= min_blocks:
        qt *= 2
    return qt


@pytest.mark.parametrize("layout", [(16, 16, 4), (16, 20, 4)], ids=_lid)
@pytest.mark.parametrize("hw,blocks", [((24, 40), (1, 5, 10)), ((20, 34), (1, 5, 8)), ((18, 13), (1, 3))],
                         ids=["N960", "N680", "N234"])
def test_tile_walk(hip_lib, hw, blocks, layout):
    """The register-staged kernel (variant 1) walking 8, 4, 2 query tiles per block gives the bits of one tile per block, which
    is close to the reference.  B * heads = 3.  N = 960: 7.5 tiles (partial last tile); N = 680: 5.3 tiles, so with qt = 4 the
    last block has two of its four tiles and the last of them 40 rows; N = 234: two tiles in a block of eight."""
    from diffsensei_amd import ops
    N = hw[0] * hw[1]
    operands, bbox, t, i = _case(3, 1, hw, 77, layout)
    want = {(24, 40): [8, 4, 2], (20, 34): [8, 4, 2], (18, 13): [8, 8]}[hw]
    assert [_qt(N, 3, mb) for mb in blocks] == want and _qt(N, 3, 1 << 20) == 1
    dev = [x.to(DEV) for x in operands]
    try:
        hip_lib.ds_set_option(b"ip_attn_variant", 1)
        hip_lib.ds_set_option(b"ip_attn_min_blocks", 1 << 20)
        y1 = _run(ops, dev, bbox, 1, hw, 77, layout).clone()
        for mb in blocks:
            hip_lib.ds_set_option(b"ip_attn_min_blocks", mb)
            y = _run(ops, dev, bbox, 1, hw, 77, layout)
            assert torch.equal(y, y1), f"qt = {_qt(N, 3, mb)} (min_blocks {mb}) differs from one tile per block"
    finally:
        hip_lib.ds_set_option(b"ip_attn_variant", 0)
        hip_lib.ds_set_option(b"ip_attn_min_blocks", 1024)
    gate(f"ip attn tile walk {_lid(layout)} N={N} qt=1 vs fp64 reference", _err(y1, t + 0.6 * i), TOL)


# ------------------------------------------------------------------------------------------------ d. strides, scale, padding
BASES = [((18, 13), (16, 16, 4)), ((24, 40), (16, 20, 4)), ((7, 9), (8, 8, 4))]
_bid = lambda v: f"{v[0][0]}x{v[0][1]}_{_lid(v[1])}"


def _dense(ops, hw, layout, heads=3, **kw):
    operands, bbox, t, i = _case(3, heads, hw, 77, layout)
    return operands, bbox, _run(ops, operands, bbox, heads, hw, 77, layout, **kw), t, i


@pytest.mark.parametrize("base", BASES, ids=_bid)
def test_stacked_panels_and_column_slices(hip_lib, base):
    """The layout engine.py builds for IP_ATTN - key panels as column slices of a stacked [B,96,W] buffer (ldk = W, sk = 96 W),
    value panels as row slices of a stacked [B,W,96] buffer (sv = 96 W, pointer offset off * 96) - plus q read from and o written
    into column slices of wider buffers: the bits of the dense call, and not one element written outside o's [B,N,C]."""
    from diffsensei_amd import ops
    hw, layout = base
    heads, B, N, Cc = 3, 3, hw[0] * hw[1], 192
    operands, bbox, y0, _, _ = _dense(ops, hw, layout)
    q, kt, vtt, ki, vti = operands
    g = torch.Generator().manual_seed(5)
    W, off = Cc + 128, 64
    stk = lambda: _r((B, LP, W), g).to(DEV)
    stv = lambda: _r((B, W, LP), g).to(DEV)
    Kt, Ki, Vt, Vi = stk(), stk(), stv(), stv()
    Kt[:, :, off:off + Cc], Ki[:, :, off:off + Cc] = kt.to(DEV), ki.to(DEV)
    Vt[:, off:off + Cc], Vi[:, off:off + Cc] = vtt.to(DEV), vti.to(DEV)
    ktv, kiv, vtv, viv = Kt[:, :, off:off + Cc], Ki[:, :, off:off + Cc], Vt[:, off:off + Cc], Vi[:, off:off + Cc]
    assert ktv.stride() == (LP * W, W, 1) and vtv.stride() == (W * LP, LP, 1) and vtv.data_ptr() == Vt.data_ptr() + 2 * off * LP
    y = _run(ops, (q, ktv, vtv, kiv, viv), bbox, heads, hw, 77, layout)
    assert torch.equal(y, y0), "stacked key / value panels"
    y = _run(ops, (q, Kt[:, :, off:], Vt[:, off:], Ki[:, :, off:], Vi[:, off:]), bbox, heads, hw, 77, layout,
             ldk=W, sk=LP * W, sv=W * LP)
    assert torch.equal(y, y0), "stacked key / value panels, explicit ldk / sk / sv"
    # q a column slice (ldq = C + 64), o a column slice (ldo = C + 24) of a flat [B*N + 64 guard rows, ldo] canary buffer
    ldq, ldo, qo, oo, guard, canary = Cc + 64, Cc + 24, 32, 8, 64, -777.0
    Q = _r((B, N, ldq), g).to(DEV)
    Q[:, :, qo:qo + Cc] = q.to(DEV)
    O = torch.full((B * N + guard, ldo), canary, dtype=torch.float16, device=DEV)
    ov = O[:B * N].view(B, N, ldo)[:, :, oo:oo + Cc]
    r = _run(ops, (Q[:, :, qo:qo + Cc], ktv, vtv, kiv, viv), bbox, heads, hw, 77, layout, out=ov)
    assert r.data_ptr() == ov.data_ptr()
    assert torch.equal(ov, y0), "q / o column slices"
    O[:B * N, oo:oo + Cc] = canary
    assert (O == canary).all(), "the kernel wrote outside o's [B,N,C] (neighbouring columns or the guard rows past N)"


@pytest.mark.parametrize("base", BASES[:2], ids=_bid)
def test_scale_source(hip_lib, base):
    from diffsensei_amd import ops
    hw, layout = base
    operands, bbox, y0, t, i = _dense(ops, hw, layout)
    sd = torch.tensor([0.6], dtype=torch.float32, device=DEV)
    y = _run(ops, operands, bbox, 3, hw, 77, layout, ip_scale=123.0, ip_scale_dev=sd)
    assert torch.equal(y, y0), "ip_scale_dev = 0.6 must override the scalar"
    y = _run(ops, operands, bbox, 3, hw, 77, layout, ip_scale=0.0)
    gate(f"ip attn {_bid(base)} ip_scale=0 vs fp64 text part", _err(y, t), TOL)
    y = _run(ops, operands, bbox, 3, hw, 77, layout, ip_scale=-0.35)
    gate(f"ip attn {_bid(base)} ip_scale=-0.35 vs fp64 reference", _err(y, t - 0.35 * i), TOL)
    sd.fill_(-0.35)
    assert torch.equal(_run(ops, operands, bbox, 3, hw, 77, layout, ip_scale=0.6, ip_scale_dev=sd), y)


@pytest.mark.parametrize("layout", [(16, 16, 4), (8, 8, 4), (16, 8, 8), (32, 32, 2)], ids=_lid)
def test_padding_content(hip_lib, layout):
    """Key rows >= Lt / Li and the matching value columns hold large finite garbage (+-6e4): the same bits as with zeros.
    Grouped and per-key masking, T16 and the full kernel, Li <= 64 (whole key blocks of padding) and Li = 96 (text padding only)."""
    from diffsensei_amd import ops
    hw = (18, 13)
    nd, tpi, K = layout
    Li = nd + K * tpi
    operands, bbox, y0, _, _ = _dense(ops, hw, layout)
    q, kt, vtt, ki, vti = (x.clone() for x in operands)
    g = torch.Generator().manual_seed(11)
    junk = lambda shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1).half() * 6e4
    kt[:, 77:], vtt[:, :, 77:] = junk(kt[:, 77:].shape), junk(vtt[:, :, 77:].shape)
    if Li < LP:
        ki[:, Li:], vti[:, :, Li:] = junk(ki[:, Li:].shape), junk(vti[:, :, Li:].shape)
    assert torch.equal(_run(ops, (q, kt, vtt, ki, vti), bbox, 3, hw, 77, layout), y0)


@pytest.mark.parametrize("base", BASES[:2], ids=_bid)
def test_batch_independence(hip_lib, base):
    from diffsensei_amd import ops
    hw, layout = base
    operands, bbox, y0, _, _ = _dense(ops, hw, layout)
    perm = [2, 0, 1]
    y = _run(ops, [x[perm].contiguous() for x in operands], bbox[perm].contiguous(), 3, hw, 77, layout)
    for j, src in enumerate(perm):
        assert torch.equal(y[j], y0[src]), f"item {src} changed when moved to batch position {j}"


@pytest.mark.parametrize("base", BASES[:2], ids=_bid)
def test_plan_path(hip_lib, base):
    """The same call as a DS_OP_IP_ATTN op through ds_op_run (the launch plan's form), stacked panels and ip_scale_dev included."""
    from diffsensei_amd import ops
    from diffsensei_amd.engine import make_op
    hw, layout = base
    nd, tpi, K = layout
    heads, B, N, Cc = 3, 3, hw[0] * hw[1], 192
    operands, bbox, y0, _, _ = _dense(ops, hw, layout)
    q, kt, vtt, ki, vti = (x.to(DEV) for x in operands)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bd, o = bbox.to(DEV), torch.zeros((B, N, Cc), dtype=torch.float16, device=DEV)
    ints = (B, heads, N, 77, nd + K * tpi, nd, tpi, K, hw[0], hw[1])
    op = make_op("IP_ATTN", i=ints, f=(0.125, 0.6), l=(Cc, Cc, Cc, LP * Cc, Cc * LP), p=(q, kt, vtt, ki, vti, bd, o, None))
    assert hip_lib.ds_op_run(C.byref(op), stream) == 0, hip_lib.ds_last_error().decode()
    assert torch.equal(o, y0), "dense op"
    W, off = Cc + 64, 64
    g = torch.Generator().manual_seed(6)
    Kt, Ki, Vt, Vi = _r((B, LP, W), g).to(DEV), _r((B, LP, W), g).to(DEV), _r((B, W, LP), g).to(DEV), _r((B, W, LP), g).to(DEV)
    Kt[:, :, off:], Ki[:, :, off:], Vt[:, off:], Vi[:, off:] = kt, ki, vtt, vti
    sd = torch.tensor([0.6], dtype=torch.float32, device=DEV)
    o.zero_()
    op = make_op("IP_ATTN", i=ints, f=(0.125, 123.0), l=(Cc, Cc, W, LP * W, W * LP),
                 p=(q, Kt.data_ptr() + 2 * off, Vt.data_ptr() + 2 * off * LP, Ki.data_ptr() + 2 * off,
                    Vi.data_ptr() + 2 * off * LP, bd, o, sd))
    assert hip_lib.ds_op_run(C.byref(op), stream) == 0, hip_lib.ds_last_error().decode()
    assert torch.equal(o, y0), "stacked panels + ip_scale_dev through the op"


# ------------------------------------------------------------------------------------------------ e. sharp logits
@pytest.mark.parametrize("layout", [(16, 16, 4), (16, 8, 8)], ids=_lid)
def test_sharp_logits(hip_lib, layout):
    """Scores of about +-40 (near one-hot rows), and one IP key - the first key of character 1 - whose scaled score is +50 for
    EVERY query row, the largest by far: the rows inside box 1 put all their weight on it, for all other rows it is masked and
    must get none.  q = 9 * (noise orthogonal to u) + 20 u per head, that key = 20 u (|u| = 1): raw 400, scaled 50."""
    from diffsensei_amd import ops
    from oracle.attention_ref import ip_region_mask
    nd, tpi, K = layout
    B, heads, hw, Lt, Li = 3, 3, (18, 13), 77, nd + K * tpi
    N = hw[0] * hw[1]
    g = torch.Generator().manual_seed(21)
    u = torch.randn(heads, 64, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    r = torch.randn(B, N, heads, 64, generator=g)
    q = (9 * (r - (r * u).sum(-1, keepdim=True) * u) + 20 * u).reshape(B, N, heads * 64).half()
    _, kt, vtt, ki, vti = (x.clone() for x in _data(B, heads, hw, Lt, Li))
    hot = nd + tpi                                                   # first key of character 1
    ki[:, hot] = (20 * u).reshape(-1).half()
    bbox = _boxes(hw, K, B)
    m = ip_region_mask(bbox, N, 1, hw[0] / hw[1], K * tpi, nd)[:, 0, :, hot]
    assert (m == 0).any() and (m != 0).any()                        # open for some rows, masked for others
    s = (q.double().view(B, N, heads, 64).transpose(1, 2) @ ki.double().view(B, LP, heads, 64).transpose(1, 2).transpose(-1, -2))[..., :Li] / 8
    assert (s[..., hot] > 45).all() and (s.argmax(-1) == hot).float().mean() > 0.99 and 30 < s[..., :hot].abs().max() < 60
    t, i = _ref_parts(q, kt, vtt, ki, vti, bbox, heads, hw, Lt, Li, nd, tpi)
    y = _run(ops, (q, kt, vtt, ki, vti), bbox, heads, hw, Lt, layout)
    gate(f"ip attn sharp logits {_lid(layout)} vs fp64 reference", _err(y, t + 0.6 * i), TOL)


# ------------------------------------------------------------------------------------------------ f. refusals
def test_refusals(hip_lib):
    from diffsensei_amd import ops
    from diffsensei_amd._lib import DiffSenseiHipError
    hw, heads, B = (7, 9), 1, 1
    operands = [x.to(DEV) for x in _data(B, heads, hw, 77, 80)]
    call = lambda K=4, **kw: ops.masked_ip_attention(*operands, torch.zeros(B, K, 4, device=DEV), heads, kw.pop("hw", hw), 0.6,
                                                     **kw)
    call()                                                              # the well-formed call goes through
    with pytest.raises(DiffSenseiHipError, match="n_dummy"):
        call(Li=80, n_dummy=16, tok_per_ip=8)                           # 16 + 4 * 8 != 80
    with pytest.raises(DiffSenseiHipError, match="layout"):
        call(K=9, Li=88, n_dummy=16, tok_per_ip=8)                      # max_ips = 9
    with pytest.raises(DiffSenseiHipError, match="exceed"):
        call(K=3, Li=97, n_dummy=16, tok_per_ip=27)                     # Li = 97 > 96
    with pytest.raises(DiffSenseiHipError, match="grid"):
        call(hw=(7, 8))                                                 # mask_h * mask_w != N
    with pytest.raises(DiffSenseiHipError, match="multiples of 8"):
        call(ldk=68)                                                    # ldk % 8 != 0


# ------------------------------------------------------------------------------------------------ model level
def test_unet_forward_two_characters_eight_tokens(hip_lib):
    """A tiny-config UNet with max_num_ips = 2, num_vision_tokens = 8 (Li = 24: per-key masking, reached through the launch plan
    with the engine's stacked panels) against oracle/unet_ref, two distinct boxes per item; the gates of
    tests/test_gpu_unet.py::test_unet_forward_vs_oracle for the tiny config."""
    import dataclasses

    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    from oracle.unet_ref import UNetOracle
    cfg = dataclasses.replace(tiny_config(), max_num_ips=2, num_vision_tokens=8)
    assert cfg.num_ip_tokens == 24
    sd = {k: v.half() for k, v in random_state_dict(cfg, 0).items()}
    model = UNetMangaModel(cfg, device=DEV)
    model.load_state_dict(sd)
    model._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    B, H, W = 2, 32, 24
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 4, H, W, generator=g).half()
    enc = torch.randn(B, cfg.num_text_tokens + cfg.num_ip_tokens, cfg.cross_attention_dim, generator=g).half()
    te = torch.randn(B, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g).half()
    tid = torch.tensor([[H * 8, W * 8, 0, 0, H * 8, W * 8]] * B, dtype=torch.float16)
    bbox = torch.tensor([[[0.05, 0.10, 0.50, 0.95], [0.40, 0.30, 0.95, 0.80]], [[0.0, 0.0, 0.30, 0.40], [0.60, 0.50, 1.0, 1.0]]])
    db = torch.zeros(B, 8, 4, dtype=torch.float16)
    db[1, 0] = torch.tensor([0.05, 0.02, 0.30, 0.15], dtype=torch.float16)
    out = model(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": H / W},
                added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    rel = lambda a, b: ((a.float().cpu() - b.float()).norm() / b.float().norm()).item()
    assert out.shape == x.shape and torch.isfinite(out).all()
    for name, q, tol in (("fp16-storage oracle", lambda t: t.half().float(), 5e-3), ("fp32 oracle", lambda t: t, 6e-3)):
        o = UNetOracle(cfg, sd, q=q)
        o.ip_scale = 0.6
        with torch.no_grad():
            r = o.forward(x, 801.0, enc, te, tid, bbox, H / W, db)
        gate(f"tiny UNet 2 x 8 IP tokens {H}x{W} vs {name}", rel(out, r), tol)
    # the boxes reach the output through the per-key mask
    out2 = model(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox.flip(1), "aspect_ratio": H / W},
                 added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    assert rel(out2, out.cpu()) > 1e-4
