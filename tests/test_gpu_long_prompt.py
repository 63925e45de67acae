"""GPU: prompts longer than 77 tokens - the long-prompt form of the fused cross-attention (ip_attn_long_kernel: 1..384 text keys
in up to four 96-key panels, online softmax across them), the engine sized by `text_tokens`, and chunked prompt encoding in the
pipeline and the serving layer.

Kernel gates: 4e-3 of max|ref| against the fp32 oracle, the bound of tests/test_gpu_ops.py::test_masked_ip_attention_core, through
tests/_gates.gate.  Engine gates: those of tests/test_gpu_unet.py::test_unet_forward_vs_oracle for the tiny config (5e-3 against
the fp16-storage oracle, 6e-3 against the fp32 one).  The poisoned-memory cases join the case list of
tests/test_gpu_poisoned_memory.py (its completeness test asks every entry of `_lib.SIGNATURES` for one) and run here.
"""
import ctypes as C
import functools
import math
import types

import pytest
import torch

from tests._gates import gate

try:
    import test_gpu_poisoned_memory as P          # the module object pytest itself collects (tests/ is on sys.path)
except ImportError:                               # collected under another import mode
    from tests import test_gpu_poisoned_memory as P

DEV = "cuda"
LP = 96
TOL = 4e-3
NS = types.SimpleNamespace
hq = lambda t: t.half().float()


def _r(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).half()


def _panels(Lt):
    return (Lt + LP - 1) // LP


def _three_boxes(B):
    bbox = torch.zeros(B, 4, 4)
    bbox[-1, 0] = torch.tensor([0.05, 0.10, 0.50, 0.95])
    bbox[-1, 1] = torch.tensor([0.50, 0.10, 0.95, 0.95])
    bbox[-1, 2] = torch.tensor([0.30, 0.30, 0.70, 0.60])
    return bbox


def _err(got, ref):
    """max|got - ref| / max(max|ref|, 1e-3): the `_close` rule of tests/test_gpu_ops.py as one number"""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)


# ------------------------------------------------------------------------------------------------ kernel vs the fp32 oracle
SCALES = (0.6, -0.35)
KERNEL_CASES = [(2, 2, (16, 16), Lt) for Lt in (97, 154, 192, 231, 308, 384)] + [(1, 4, (24, 40), 231), (1, 20, (32, 32), 154)]


@functools.lru_cache(maxsize=None)
def _projected_case(B, heads, hw, Lt):
    """q, enc = [text (Lt) | 16 dummy + 4 x 16 image tokens], the four projections and the oracle's two parts (fp32, like
    `_ip_attn_ref` of tests/test_gpu_ops.py but split at Lt).  Computed once per case, shared, never written to."""
    from oracle.attention_ref import _heads, ip_region_mask, sdpa
    g = torch.Generator().manual_seed(B + heads + hw[0] + 31 * Lt)
    N, Cc, X = hw[0] * hw[1], heads * 64, 128
    q, enc = _r((B, N, Cc), g), _r((B, Lt + 80, X), g)
    wk, wv, wki, wvi = (_r((Cc, X), g, 1 / math.sqrt(X)) for _ in range(4))
    bbox = _three_boxes(B)
    txt, ip = enc[:, :Lt], enc[:, Lt:]
    qh = _heads(q.float(), heads)
    h_ = lambda t: _heads(t.half().float(), heads)
    t_out = sdpa(qh, h_(txt.float() @ wk.float().t()), h_(txt.float() @ wv.float().t()))
    m = ip_region_mask(bbox, N, heads, hw[0] / hw[1], 64, 16)
    i_out = sdpa(qh, h_(ip.float() @ wki.float().t()), h_(ip.float() @ wvi.float().t()), m)
    back = lambda o: o.transpose(1, 2).reshape(B, N, Cc)
    return NS(q=q, enc=enc, wk=wk, wv=wv, wki=wki, wvi=wvi, bbox=bbox, t=back(t_out), i=back(i_out))


def _rows_entry_b1(q, kt, vtt, ki, vti, bbox, heads, hw, Lt, scale_dev):
    """B = 1: `ops.masked_ip_attention` takes a one-element scale vector for the one-scale form, so the per-row entry point is
    called as the C ABI states it."""
    from diffsensei_amd import _lib
    lib = _lib.load()
    B, N, Cc = q.shape
    out = torch.empty_like(q)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.ds_masked_ip_attn_long_rows_f16(p(q), Cc, p(kt), p(vtt), p(ki), p(vti), p(bbox), p(out), Cc, B, heads, N, Lt, kt.shape[1] // LP,
                                             80, 16, 16, 4, hw[0], hw[1], 0.125, p(scale_dev), kt.stride(1), kt.stride(0), vtt.stride(0),
                                             ki.stride(1), ki.stride(0), vti.stride(0), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ds_last_error().decode()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [False, True], ids=["one-scale", "per-row"])
@pytest.mark.parametrize("B,heads,hw,Lt", KERNEL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_long_prompt_attention_vs_oracle(hip_lib, B, heads, hw, Lt, rows):
    from diffsensei_amd import ops
    h = _projected_case(B, heads, hw, Lt)
    X, Cc, T = 128, heads * 64, _panels(Lt)
    encd = h.enc.to(DEV)
    txt, ip = ops.pad_rows(encd, 0, Lt, LP * T), ops.pad_rows(encd, Lt, 80, LP)
    kt = ops.gemm(txt.view(-1, X), h.wk.to(DEV)).view(B, LP * T, Cc)
    ki = ops.gemm(ip.view(-1, X), h.wki.to(DEV)).view(B, LP, Cc)
    vtt, vti = ops.gemm_batched_nt(h.wv.to(DEV), txt), ops.gemm_batched_nt(h.wvi.to(DEV), ip)
    assert vtt.shape == (B, Cc, LP * T)
    q, bbox = h.q.to(DEV), h.bbox.to(DEV)
    if not rows:
        y = ops.masked_ip_attention(q, kt, vtt, ki, vti, bbox, heads, hw, SCALES[0], Lt=Lt)
        ref = h.t + SCALES[0] * h.i
    else:
        s = torch.tensor(SCALES[:B], dtype=torch.float32)
        sd = s.to(DEV)
        y = (ops.masked_ip_attention(q, kt, vtt, ki, vti, bbox, heads, hw, 0.0, Lt=Lt, ip_scale_dev=sd) if B > 1
             else _rows_entry_b1(q, kt, vtt, ki, vti, bbox, heads, hw, Lt, sd))
        ref = h.t + s.view(B, 1, 1) * h.i
    gate(f"long-prompt attention B{B} heads{heads} {hw[0]}x{hw[1]} Lt{Lt} {'per-row' if rows else 'one'} scale vs fp32 oracle",
         _err(y, ref), TOL)


# ------------------------------------------------------------------------------------------------ direct panels
@functools.lru_cache(maxsize=None)
def _direct_case(B, heads, hw, Lt, seed=0):
    """Zero-padded fp16 panels given directly (no projection) and the fp64 parts of tests/test_gpu_masked_ip_attn.py::_ref_parts."""
    g = torch.Generator().manual_seed(977 * seed + 7 * B + 13 * heads + hw[0] * 100 + hw[1] + Lt * 3)
    N, Cc, T = hw[0] * hw[1], heads * 64, _panels(Lt)
    q = _r((B, N, Cc), g)
    kt, ki, vtt, vti = _r((B, LP * T, Cc), g), _r((B, LP, Cc), g), _r((B, Cc, LP * T), g), _r((B, Cc, LP), g)
    kt[:, Lt:], ki[:, 80:], vtt[:, :, Lt:], vti[:, :, 80:] = 0, 0, 0, 0
    return NS(q=q, kt=kt, vtt=vtt, ki=ki, vti=vti, bbox=_three_boxes(B), heads=heads, hw=hw, Lt=Lt)


def _direct_ref(h):
    from tests.test_gpu_masked_ip_attn import _ref_parts
    return _ref_parts(h.q, h.kt, h.vtt, h.ki, h.vti, h.bbox, h.heads, h.hw, h.Lt, 80, 16, 16)


@pytest.mark.gpu
def test_maximum_moves_between_panels(hip_lib):
    """Lt = 231: key rows 5 (first panel) and 200 (third panel) are multiplied by 8; one half of the query rows points along key
    5, the other along key 200, per head.  For the second half the running maximum rises two panels in: what an online-softmax
    rescale that forgets O or the row sum gets wrong.  Asserted on the CPU reference: both halves exist and the winner holds
    more than half of the probability in each."""
    from diffsensei_amd import ops
    B, heads, hw, Lt = 2, 2, (16, 16), 231
    base = _direct_case(B, heads, hw, Lt, seed=1)
    N = hw[0] * hw[1]
    kt = base.kt.clone()
    kt[:, 5] *= 8
    kt[:, 200] *= 8
    first = torch.arange(N) % 2 == 0                      # query rows whose largest score is key 5; the others: key 200
    unit = lambda k: (k.float().view(B, 1, heads, 64) / k.float().view(B, 1, heads, 64).norm(dim=-1, keepdim=True))
    q = (0.15 * base.q.float().view(B, N, heads, 64)
         + 1.5 * torch.where(first.view(1, N, 1, 1), unit(kt[:, 5]), unit(kt[:, 200]))).reshape(B, N, heads * 64).half()
    h = NS(**{**vars(base), "q": q, "kt": kt})
    s = (q.double().view(B, N, heads, 64).transpose(1, 2) @ kt[:, :Lt].double().view(B, Lt, heads, 64).permute(0, 2, 3, 1)) / 8
    pr = torch.softmax(s, -1)                             # [B, heads, N, Lt]
    win = pr.argmax(-1)
    assert first.any() and (~first).any()
    assert (win[:, :, first] == 5).all() and (win[:, :, ~first] == 200).all()
    assert pr[:, :, first, 5].min() > 0.5 and pr[:, :, ~first, 200].min() > 0.5
    t, i = _direct_ref(h)
    y = ops.masked_ip_attention(q.to(DEV), kt.to(DEV), h.vtt.to(DEV), h.ki.to(DEV), h.vti.to(DEV), h.bbox.to(DEV), heads, hw, 0.6, Lt=Lt)
    gate("long-prompt attention, maximum in panel 0 / panel 2 (Lt 231) vs fp64 reference", _err(y, t + 0.6 * i), TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("Lt", [154, 231])
def test_padding_keys_are_inert(hip_lib, Lt):
    """Rows >= Lt of the text K panel and columns >= Lt of the V^T panel filled with 1e4: the same bits as with zeros there."""
    from diffsensei_amd import ops
    h = _direct_case(2, 2, (16, 16), Lt, seed=2)
    kt, vtt = h.kt.clone(), h.vtt.clone()
    kt[:, Lt:], vtt[:, :, Lt:] = 1e4, 1e4
    run = lambda k, v: ops.masked_ip_attention(h.q.to(DEV), k.to(DEV), v.to(DEV), h.ki.to(DEV), h.vti.to(DEV), h.bbox.to(DEV), h.heads,
                                               h.hw, 0.6, Lt=Lt)
    y0, y1 = run(h.kt, h.vtt), run(kt, vtt)
    assert torch.isfinite(y1).all() and torch.equal(y0, y1)


@pytest.mark.gpu
def test_limits_are_refused_before_any_launch(hip_lib):
    from diffsensei_amd import ops
    from diffsensei_amd._lib import DiffSenseiHipError
    B, heads, hw = 1, 1, (8, 8)
    g = torch.Generator().manual_seed(5)
    q, ki, vti = _r((B, 64, 64), g).to(DEV), _r((B, LP, 64), g).to(DEV), _r((B, 64, LP), g).to(DEV)
    bbox = torch.zeros(B, 4, 4, device=DEV)
    call = lambda rows, Lt, **kw: ops.masked_ip_attention(q, _r((B, rows, 64), g).to(DEV), _r((B, 64, rows), g).to(DEV), ki, vti, bbox,
                                                          heads, hw, 0.6, Lt=Lt, **kw)
    assert torch.isfinite(call(4 * LP, 384)).all()                     # the cap itself goes through
    with pytest.raises(DiffSenseiHipError, match="384"):
        call(5 * LP, 385)
    with pytest.raises(DiffSenseiHipError, match="384"):
        call(4 * LP, 385)
    with pytest.raises(DiffSenseiHipError, match="Lt=0"):
        call(2 * LP, 0)
    with pytest.raises(DiffSenseiHipError, match="panels"):
        call(3 * LP, 150)                                              # 150 keys need two panels, not three
    kwide = torch.zeros(B, 2 * LP, 68, dtype=torch.float16, device=DEV)[:, :, :64]      # row stride 68: no multiple of 8
    with pytest.raises(DiffSenseiHipError, match="multiples of 8"):
        ops.masked_ip_attention(q, kwide, _r((B, 64, 2 * LP), g).to(DEV), ki, vti, bbox, heads, hw, 0.6, Lt=154)


# ------------------------------------------------------------------------------------------------ inside poisoned memory
POISON_LT = 231
POISON_SCALES = (0.6, -0.35, 0.9)


@functools.lru_cache(maxsize=None)
def _poison_data(B, heads, hw):
    h = _direct_case(B, heads, hw, POISON_LT, seed=3)
    kt, vtt, ki, vti = h.kt.clone(), h.vtt.clone(), h.ki.clone(), h.vti.clone()
    kt[:, POISON_LT:], vtt[:, :, POISON_LT:], ki[:, 80:], vti[:, :, 80:] = P.LOUD, P.LOUD, P.LOUD, P.LOUD   # the caller's padding: anything finite
    t, i = _direct_ref(h)
    scales = torch.tensor(POISON_SCALES[:B], dtype=torch.float32)
    return NS(q=h.q, kt=kt, vtt=vtt, ki=ki, vti=vti, bbox=h.bbox, heads=heads, hw=hw, scales=scales, ref=t + 0.6 * i,
              ref_rows=t + scales.double().view(B, 1, 1) * i)


def _poison_run(rows):
    def run(m, h):
        bbox = m.place(h.bbox)
        sd = m.place(h.scales) if rows else None
        if m.plain:
            return (m.ops.masked_ip_attention(m.place(h.q), m.place(h.kt), m.place(h.vtt), m.place(h.ki), m.place(h.vti), bbox, h.heads,
                                              h.hw, 0.6, Lt=POISON_LT, ip_scale_dev=sd),)
        B, N, Cc = h.q.shape
        LT = h.kt.shape[1]
        Wd, off, Wi, offi, ldq, qo, ldo = Cc + 128, 64, Cc + 72, 8, Cc + 64, 32, Cc + 24

        def stacked(shape, sl, t):                  # the operand inside a wider buffer whose other columns / rows are poison
            host = m.poison(shape, torch.float16)
            host[sl] = t
            return m.place(host)[sl]
        col = lambda o: (slice(None), slice(None), slice(o, o + Cc))
        row = lambda o: (slice(None), slice(o, o + Cc))
        kt, ki = stacked((B, LT, Wd), col(off), h.kt), stacked((B, LP, Wi), col(offi), h.ki)       # text and IP strides differ
        vtt, vti = stacked((B, Wd, LT), row(off), h.vtt), stacked((B, Wi, LP), row(offi), h.vti)
        q = stacked((B, N, ldq), col(qo), h.q)
        o = m.out((B * N, Cc), ld=ldo).unflatten(0, (B, N))
        return (m.ops.masked_ip_attention(q, kt, vtt, ki, vti, bbox, h.heads, h.hw, 0.6, out=o, Lt=POISON_LT, ip_scale_dev=sd),)
    return run


def _poison_check(rows):
    def check(o, h):
        e = _err(o[0], h.ref_rows if rows else h.ref)
        assert e <= TOL, f"long-prompt attention vs fp64 reference: {e:.3g} > {TOL}"
    return check


LONG_CASES = [P.Case(f"ip-attn-long-B3-18x13-Lt{POISON_LT}", ["ds_masked_ip_attn_long_f16"], functools.partial(_poison_data, 3, 3, (18, 13)),
                     _poison_run(False), _poison_check(False)),
              P.Case(f"ip-attn-long-rows-B3-18x13-Lt{POISON_LT}", ["ds_masked_ip_attn_long_rows_f16"],
                     functools.partial(_poison_data, 3, 3, (18, 13)), _poison_run(True), _poison_check(True))]
P.CASES.extend(LONG_CASES)     # on import, which pytest does for every test module before it runs a test


def test_the_long_prompt_entry_points_have_their_cases():
    """Host only: what tests/test_gpu_poisoned_memory.py::test_every_entry_point_has_a_case needs from this file."""
    from diffsensei_amd._lib import SIGNATURES
    ours = {e for c in LONG_CASES for e in c.entry}
    assert ours == {"ds_masked_ip_attn_long_f16", "ds_masked_ip_attn_long_rows_f16"} and ours <= set(SIGNATURES)
    assert all(any(c is k for k in P.CASES) for c in LONG_CASES) and len({c.id for c in P.CASES}) == len(P.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: c.id)
def test_long_prompt_result_depends_on_nothing_but_the_operands(hip_lib, case):
    P.test_result_depends_on_nothing_but_the_operands(hip_lib, case)


# ------------------------------------------------------------------------------------------------ engine
def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


def _long_inputs(cfg, n_txt, B, H, W, seed):
    from tests.test_gpu_unet import _inputs
    x, _, te, tid, bbox, db = _inputs(cfg, B, H, W, seed)
    g = torch.Generator().manual_seed(seed + 1000 * n_txt)
    enc = torch.randn(B, n_txt + cfg.num_ip_tokens, cfg.cross_attention_dim, generator=g).half()
    return x, enc, te, tid, bbox, db


@pytest.fixture(scope="module")
def tiny(hip_lib):
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    from oracle.unet_ref import UNetOracle
    cfg = tiny_config()
    sd = {k: v.half() for k, v in random_state_dict(cfg, 0).items()}
    model = UNetMangaModel(cfg, device=DEV)
    model.load_state_dict(sd)
    model._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    o16, o32 = UNetOracle(cfg, sd, q=hq), UNetOracle(cfg, sd)
    o16.ip_scale = o32.ip_scale = 0.6
    return cfg, sd, model, o16, o32


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(16, 16), (8, 32)])
@pytest.mark.parametrize("n_txt", [154, 231])
def test_unet_forward_long_prompt_vs_oracle(tiny, n_txt, H, W):
    cfg, sd, model, o16, o32 = tiny
    x, enc, te, tid, bbox, db = _long_inputs(cfg, n_txt, 2, H, W, seed=n_txt + H)
    out = model(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": H / W},
                added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    eng = model.engine(2, H, W, H / W, text_tokens=n_txt)
    assert eng.text_tokens == n_txt and eng.text_panels == _panels(n_txt) and eng.enc.shape[1] == n_txt + cfg.num_ip_tokens
    assert eng is not model.engine(2, H, W, H / W)                      # the 77-token engine is another cache entry
    with torch.no_grad():
        r16 = o16.forward(x, 801.0, enc, te, tid, bbox, H / W, db)
        r32 = o32.forward(x, 801.0, enc, te, tid, bbox, H / W, db)
    assert out.shape == x.shape and torch.isfinite(out).all()
    gate(f"tiny UNet {H}x{W}, {n_txt} text tokens vs fp16-storage oracle", _rel(out, r16), 5e-3)
    gate(f"tiny UNet {H}x{W}, {n_txt} text tokens vs fp32 oracle", _rel(out, r32), 6e-3)
    # the tail of the text reaches the output: change the last text token only
    enc2 = enc.clone()
    enc2[:, n_txt - 1] += 1.0
    out2 = model(x.to(DEV), 801.0, enc2.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": H / W},
                 added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    assert not torch.equal(out2, out)
    with pytest.raises(ValueError, match="text tokens"):                # a tensor of another length is refused, not reshaped
        eng.set_request(enc[:, 1:], te, tid, bbox, None, 0.6)


@pytest.mark.gpu
def test_two_sampler_steps_eager_and_graph_long_prompt(tiny):
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    from diffsensei_amd.unet import dialog_pixel_boxes
    cfg, sd, model, o16, o32 = tiny
    ns, H, W, steps, n_txt = 1, 16, 16, 2, 154
    x, enc, te, tid, bbox, db = _long_inputs(cfg, n_txt, 2 * ns, H, W, seed=3)
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(steps)
    lat0 = (x[:ns].float() * sch.init_noise_sigma).half()
    eng = model.engine(2 * ns, H, W, H / W, text_tokens=n_txt)
    eng.build_sampler(ns, sch.kind, True)
    results = []
    for mode in ("eager", "graph"):
        eng.set_request(enc, te, tid, bbox, dialog_pixel_boxes(db, H, W), 0.6)
        eng.load_schedule(torch.from_numpy(sch.coef_table(7.5)))
        eng.latents.copy_(lat0)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            eng.prep_plan.run(st.cuda_stream)
            if mode == "graph" and not eng.step_plan.captured:
                eng.step_plan.capture(st.cuda_stream)
            for _ in range(steps):
                (eng.step_plan.replay if mode == "graph" else eng.step_plan.run)(st.cuda_stream)
        st.synchronize()
        assert int(eng.ctr.item()) == steps
        results.append(eng.latents.clone())
    assert torch.isfinite(results[0]).all() and not torch.equal(results[0].cpu(), lat0)
    assert torch.equal(results[0], results[1]), "hipGraph replay differs from eager launches"


def _describe(lib, ops_):
    out = []
    for op in ops_:
        name = C.create_string_buffer(96)
        fl, by = C.c_double(), C.c_double()
        assert lib.ds_op_describe(C.byref(op), name, 96, C.byref(fl), C.byref(by)) == 0
        out.append((op.code, tuple(op.i), tuple(op.f), tuple(op.l), name.value.decode(), fl.value, by.value))
    return out


@pytest.mark.gpu
def test_default_text_length_keeps_the_plan(tiny, hip_lib):
    """text_tokens None and 77 describe the plan of an engine built without the argument, op for op: codes, every integer, float
    and stride slot, the kernel ds_op_describe names and its figures.  No IP_ATTN op uses the long form's slots."""
    from diffsensei_amd._lib import OP
    from diffsensei_amd.engine import UNetEngine
    cfg, sd, model, o16, o32 = tiny
    pk = model.packed()
    plans = [_describe(hip_lib, UNetEngine(pk, 2, 16, 16, 1.0, **kw).forward_ops) for kw in ({}, {"text_tokens": None}, {"text_tokens": 77})]
    assert plans[0] == plans[1] == plans[2] and len(plans[0]) > 50
    ip = [d for d in plans[0] if d[0] == OP["IP_ATTN"]]
    assert ip and all(d[1][3] == 77 and d[1][11] == 0 and d[3][5:8] == (0, 0, 0) and d[4] == "ip_attn_kernel" for d in ip)
    assert model.engine(2, 16, 16, 1.0) is model.engine(2, 16, 16, 1.0, text_tokens=None) is model.engine(2, 16, 16, 1.0, text_tokens=77)
    long = [d for d in _describe(hip_lib, UNetEngine(pk, 2, 16, 16, 1.0, text_tokens=154).forward_ops) if d[0] == OP["IP_ATTN"]]
    assert len(long) == len(ip) and all(d[1][3] == 154 and d[1][11] == 2 and d[4] == "ip_attn_long_kernel" for d in long)
    with pytest.raises(ValueError, match="384"):
        UNetEngine(pk, 2, 16, 16, 1.0, text_tokens=385)


# ------------------------------------------------------------------------------------------------ pipeline: chunked encoding
from tests._sampler_common import DIALOG, IP_BBOX, SDXL, parts  # noqa: E402,F401  (`parts`: the tiny pipeline's modules, a fixture)


@pytest.fixture(scope="module")
def text_pipe(parts):
    """tests/_sampler_common.py's tiny pipeline with two stand-in CLIP text encoders (widths 96 + 160 = the tiny UNet's
    cross_attention_dim 256, projection 128 = its pooled width) and the stand-in tokenizers of tests/_long_prompt_common.py."""
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    from diffsensei_amd.unet import UNetMangaModel
    from tests._long_prompt_common import tokenizers
    torch.manual_seed(1)
    c1 = CLIPTextConfig(vocab_size=1000, hidden_size=96, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2,
                        max_position_embeddings=77, hidden_act="quick_gelu", eos_token_id=999, bos_token_id=998, pad_token_id=0)
    c2 = CLIPTextConfig(vocab_size=1000, hidden_size=160, intermediate_size=320, num_hidden_layers=3, num_attention_heads=2,
                        max_position_embeddings=77, hidden_act="gelu", projection_dim=128, eos_token_id=999, bos_token_id=998,
                        pad_token_id=0)
    te1, te2 = CLIPTextModel(c1).eval(), CLIPTextModelWithProjection(c2).eval()
    t1, t2 = tokenizers()
    unet = UNetMangaModel(parts["cfg"], device=DEV)
    unet.load_state_dict(parts["sd"])
    pipe = DiffSenseiPipeline(None, te1, te2, t1, t2, EulerDiscreteScheduler(**SDXL), unet, parts["clip"])
    pipe.register_manga_modules(magi_image_encoder=parts["mae"], image_proj_model=parts["rs"])
    common = dict(height=128, width=128, num_inference_steps=2, guidance_scale=7.5, num_samples=2, ip_images=parts["imgs"],
                  ip_bbox=IP_BBOX, dialog_bbox=DIALOG, ip_scale=0.6)
    return pipe, common, parts["lat0"]


def _call(pipe, common, lat0, **kw):
    out = pipe(latents=lat0.clone(), output_type="latent", **{**common, **kw}).images
    return out.clone(), dict(pipe.last_run_info)


@pytest.mark.gpu
def test_short_prompt_is_unchanged_by_max_prompt_chunks(text_pipe):
    """(a) at most 75 ids: max_prompt_chunks = 3 gives the bits of the default, in one chunk."""
    from tests._long_prompt_common import prompt
    pipe, common, lat0 = text_pipe
    text = prompt(60)
    y1, i1 = _call(pipe, common, lat0, prompt=text)
    y3, i3 = _call(pipe, common, lat0, prompt=text, max_prompt_chunks=3)
    assert torch.isfinite(y1).all() and torch.equal(y1, y3)
    assert i1["prompt_chunks"] == i3["prompt_chunks"] == 1 and i1["prompt_tokens_dropped"] == i3["prompt_tokens_dropped"] == 0


@pytest.mark.gpu
def test_long_prompt_equals_hand_concatenated_chunks(text_pipe):
    """(b) 180 ids under max_prompt_chunks = 3: the latents of a call with `prompt_embeds` concatenated by hand from three
    separate `encode` calls per encoder, pooled from the first chunk of encoder 2.  (c) max_prompt_chunks = 2 reports the
    30 ids it drops - per text: both tokenizers see the prompt, and the empty negative is forced to zeros - and differs."""
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from tests._long_prompt_common import prompt
    pipe, common, lat0 = text_pipe
    text = prompt(180)
    y3, i3 = _call(pipe, common, lat0, prompt=text, max_prompt_chunks=3)
    assert i3["prompt_chunks"] == 3 and i3["prompt_tokens_dropped"] == 0 and torch.isfinite(y3).all()
    hidden, pooled = [], None
    for tok, te in ((pipe.tokenizer, pipe.text_encoder), (pipe.tokenizer_2, pipe.text_encoder_2)):
        raw = DiffSenseiPipeline._raw_ids(tok, text)
        assert len(raw) == 180
        parts_, first = [], None
        for c in range(3):
            ids = torch.tensor([[tok.bos_token_id] + raw[75 * c:75 * (c + 1)] + [tok.eos_token_id]])
            ids = torch.cat([ids, torch.full((1, 77 - ids.shape[1]), tok.pad_token_id)], dim=1)
            h, p = te.encode(ids)
            parts_.append(h)
            first = p if first is None else first
        hidden.append(torch.cat(parts_, dim=1))
        pooled = first
    pe = torch.cat(hidden, dim=-1)
    assert pe.shape == (1, 231, 256) and pooled.shape == (1, 128)
    yh, ih = _call(pipe, common, lat0, prompt="", prompt_embeds=pe, pooled_prompt_embeds=pooled)
    assert ih["prompt_chunks"] == 3 and torch.equal(y3, yh)
    y2, i2 = _call(pipe, common, lat0, prompt=text, max_prompt_chunks=2)
    assert i2["prompt_chunks"] == 2 and i2["prompt_tokens_dropped"] == 2 * 30 and not torch.equal(y2, y3)
    y1, i1 = _call(pipe, common, lat0, prompt=text)
    assert i1["prompt_chunks"] == 1 and i1["prompt_tokens_dropped"] == 2 * 105 and not torch.equal(y1, y2)


@pytest.mark.gpu
def test_batcher_keeps_chunk_counts_apart(text_pipe):
    """(d) one 1-chunk and one 3-chunk request through the batcher: two UNet batches, each the bits of its single call."""
    from diffsensei_amd.serving import BucketBatcher
    from tests._long_prompt_common import prompt
    pipe, common, lat0 = text_pipe
    reqs = [dict(common, prompt=prompt(50, seed=1), max_prompt_chunks=3, latents=lat0.clone()),
            dict(common, prompt=prompt(180, seed=2), max_prompt_chunks=3, latents=lat0.clone())]
    single = [_call(pipe, {k: v for k, v in r.items() if k != "latents"}, lat0) for r in reqs]
    assert [i["prompt_chunks"] for _, i in single] == [1, 3]
    b = BucketBatcher(pipe, mix_scales=True)
    for r in reqs:
        b.submit(**r)
    outs = b.run(output_type="latent")
    assert sorted(b.last_plan) == [[0], [1]]
    for (want, _), got in zip(single, outs):
        assert torch.equal(want, got)
    with pytest.raises(ValueError, match="prompt chunks"):
        pipe.generate_batch(reqs, output_type="latent")


# ------------------------------------------------------------------------------------------------ stand-alone processor
@pytest.mark.gpu
def test_standalone_processor_takes_a_long_text(hip_lib):
    """`MaskedIPAttnProcessor2_0.__call__` with 231 text tokens in front of the 80 image tokens pads the text to three panels and
    calls the long-prompt op: against oracle.attention_ref.masked_ip_cross_attention with fp16 storage, the kernel's 4e-3 of
    max|ref| (the projections around the core are the oracle's own fp16 points)."""
    from diffsensei_amd.attention_processor import AttentionWeights, MaskedIPAttnProcessor2_0
    from oracle.attention_ref import masked_ip_cross_attention
    g = torch.Generator().manual_seed(41)
    B, heads, hw, Lt, X = 2, 2, (16, 16), 231, 64
    N, Cc = hw[0] * hw[1], heads * 64
    x, enc = _r((B, N, Cc), g), _r((B, Lt + 80, X), g)
    wq, wo, bo = _r((Cc, Cc), g, 1 / math.sqrt(Cc)), _r((Cc, Cc), g, 1 / math.sqrt(Cc)), _r((Cc,), g, 0.1)
    wk, wv, wki, wvi = (_r((Cc, X), g, 1 / math.sqrt(X)) for _ in range(4))
    bbox = _three_boxes(B)
    attn = AttentionWeights(Cc, X, heads, DEV)
    attn.to_q.weight, attn.to_k.weight, attn.to_v.weight = wq.to(DEV), wk.to(DEV), wv.to(DEV)
    attn.to_out[0].weight, attn.to_out[0].bias = wo.to(DEV), bo.to(DEV)
    proc = MaskedIPAttnProcessor2_0(Cc, X, scale=0.6, num_ip_tokens=64, num_dummy_tokens=16, device=DEV)
    proc.to_k_ip.weight, proc.to_v_ip.weight = wki.to(DEV), wvi.to(DEV)
    y = proc(attn, x.to(DEV), encoder_hidden_states=enc.to(DEV), bbox=bbox.to(DEV), aspect_ratio=hw[0] / hw[1])
    f = lambda t: t.float()
    ref = masked_ip_cross_attention(f(x), f(enc), bbox, hw[0] / hw[1], f(wq), f(wk), f(wv), f(wki), f(wvi), f(wo), f(bo), heads, 0.6,
                                    64, 16, q=hq)
    gate("MaskedIPAttnProcessor2_0 with 231 text tokens vs fp16-storage oracle", _err(y, ref), TOL)
