"""GPU: guidance scale and IP scale per panel - `sampler_step_kernel` with a `guidance[ns]` vector, `ip_attn_kernel` with an
`ip_scale[B]` vector, and the pipeline / engine layers that carry both from the requests to the kernels.

Almost every comparison is `torch.equal`, and that is derived, not tuned: per panel the arithmetic is the instruction
sequence of the one-scalar path (gd = half(g_n * float(half(ec - eu))), w = (part ? s_b : 1) / psum), and every kernel on
the path treats batch rows independently (tests/test_gpu_pipeline_variants.py::test_generate_batch_equals_separate_calls
explains the one exception, the GEMM tiling chosen by M - which is why the pipeline comparisons here keep the batch
shape, and with it the plan, the same on both sides).  The two closeness checks use tolerances that exist already: 4e-3 of
tests/test_gpu_masked_ip_attn.py for the attention kernel against the oracle, the fused-sampler gate of 1.2e-2 of
tests/test_gpu_pipeline_variants.py for the whole loop.
"""
import numpy as np
import pytest
import torch

from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
LP = 96
hq = lambda t: t.half().float()
SDXL = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, timestep_spacing="leading")


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


# ------------------------------------------------------------------------------------------------ 1. step kernel
NS, SH, SW, GUIDANCE = 3, 10, 10, (1.5, 5.0, 7.5)      # 300 threads: panel boundaries inside a block, ragged second block


def _scheduler(kind):
    from diffsensei_amd import schedulers as S
    sch = [S.EulerDiscreteScheduler(), S.DDIMScheduler(), S.DPMSolverMultistepScheduler(**SDXL),
           S.EulerAncestralDiscreteScheduler(**SDXL)][kind]
    sch.set_timesteps(5)
    assert sch.kind == kind
    return sch


def _steps(kind, do_cfg, table, guidance, inputs):
    """Three consecutive steps (device counter 0, 1, 2) from the same start; returns (latents, model_in, prev_x0)."""
    from diffsensei_amd import ops
    lat0, eps, seeds, solver = inputs
    lat = lat0.to(DEV)
    rows = 2 * NS if do_cfg else NS
    xin = torch.zeros(rows, SH * SW, 4, dtype=torch.float16, device=DEV)
    prev = torch.zeros_like(lat)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for i in range(3):
        ctr.fill_(i)
        e = eps[i][:rows].to(DEV).contiguous()
        if kind == 2:
            ops.cfg_dpm_step(e, lat, xin, table, solver, prev, do_cfg, ctr, guidance=guidance)
        elif kind == 3:
            ops.cfg_sampler_step_noise(e, lat, xin, table, seeds, 3, do_cfg, ctr, guidance=guidance)
        else:
            ops.cfg_sampler_step(e, lat, xin, table, kind, do_cfg, ctr, guidance=guidance)
    torch.cuda.synchronize()
    return lat, xin, prev


def _step_inputs(kind, sch):
    g = torch.Generator().manual_seed(40 + kind)
    lat0 = (torch.randn(NS, 4, SH, SW, generator=g) * sch.init_noise_sigma).half()
    eps = [(torch.randn(2 * NS, SH * SW, 4, generator=g) * 0.5).half() for _ in range(3)]
    seeds = torch.tensor([11, 2 ** 40 + 5, 977], dtype=torch.int64, device=DEV) if kind == 3 else None
    solver = torch.from_numpy(sch.solver_table()).to(DEV) if kind == 2 else None
    return lat0, eps, seeds, solver


@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["euler", "ddim", "dpm", "euler_ancestral"])
def test_step_kernel_guidance_per_panel(hip_lib, kind):
    """Panel n of the launch with guidance = [1.5, 5.0, 7.5] is, bit for bit, panel n of the existing scalar entry point run
    on the whole batch with g_n in column 7: latents, both CFG halves of model_in, prev_x0 (DPM).  Column 7 of the
    per-panel launch's table holds a value no panel uses, so a kernel that still read it would be caught."""
    sch = _scheduler(kind)
    inputs = _step_inputs(kind, sch)
    gvec = torch.tensor(GUIDANCE, dtype=torch.float32, device=DEV)
    lat, xin, prev = _steps(kind, True, torch.from_numpy(sch.coef_table(99.0)).to(DEV), gvec, inputs)
    assert torch.isfinite(lat).all()
    seen = []
    for n, gn in enumerate(GUIDANCE):
        lat_s, xin_s, prev_s = _steps(kind, True, torch.from_numpy(sch.coef_table(gn)).to(DEV), None, inputs)
        assert torch.equal(lat[n], lat_s[n]), f"latents of panel {n} (guidance {gn})"
        assert torch.equal(xin[n], xin_s[n]) and torch.equal(xin[NS + n], xin_s[NS + n]), f"model_in of panel {n}"
        assert torch.equal(prev[n], prev_s[n]), f"prev_x0 of panel {n}"
        seen.append(lat_s)
    # the comparison has teeth: the other panels' guidance gives panel 0 other latents
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[1][0], seen[2][0])


@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["euler", "ddim", "dpm", "euler_ancestral"])
def test_step_kernel_guidance_is_not_read_without_cfg(hip_lib, kind):
    sch = _scheduler(kind)
    inputs = _step_inputs(kind, sch)
    table = torch.from_numpy(sch.coef_table(1.0)).to(DEV)
    a = _steps(kind, False, table, None, inputs)
    b = _steps(kind, False, table, torch.tensor([3.0, -8.0, 1e4], dtype=torch.float32, device=DEV), inputs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_step_and_attention_refuse_bad_vectors(hip_lib):
    from diffsensei_amd import _lib, ops
    sch = _scheduler(0)
    lat0, eps, _, _ = _step_inputs(0, sch)
    lat, xin = lat0.to(DEV), torch.zeros(2 * NS, SH * SW, 4, dtype=torch.float16, device=DEV)
    table = torch.from_numpy(sch.coef_table(5.0)).to(DEV)
    for bad in (torch.ones(NS + 1, device=DEV), torch.ones(NS, device=DEV).half(), torch.ones(NS)):
        with pytest.raises(_lib.DiffSenseiHipError):
            ops.cfg_sampler_step(eps[0].to(DEV), lat, xin, table, 0, True, guidance=bad)
    q, kt, vtt, ki, vti, bbox = _attn_case((16, 16))
    for bad in (torch.ones(3, device=DEV), torch.ones(2, device=DEV).half(), torch.ones(2)):
        with pytest.raises(_lib.DiffSenseiHipError):
            ops.masked_ip_attention(q[:2], kt[:2], vtt[:2], ki[:2], vti[:2], bbox[:2], 2, (16, 16), 1.0, ip_scale_dev=bad)


# ------------------------------------------------------------------------------------------------ 2. IP attention
AB, AHEADS, LT, LI, SCALES = 4, 2, 77, 80, (0.0, 0.35, 1.0, 1.7)
_attn_cache = {}


def _attn_case(hw):
    """Seeded operands on the device and the boxes of oracle/ip_box_cases.py (a different set per batch item), the way
    tests/test_gpu_masked_ip_attn.py builds them; made once per grid and never written to."""
    if hw not in _attn_cache:
        from oracle.ip_box_cases import box_cases
        g = torch.Generator().manual_seed(100 * hw[0] + hw[1])
        N, Cc = hw[0] * hw[1], AHEADS * 64
        r = lambda *s: torch.randn(s, generator=g).half()
        q, kt, ki, vtt, vti = r(AB, N, Cc), r(AB, LP, Cc), r(AB, LP, Cc), r(AB, Cc, LP), r(AB, Cc, LP)
        kt[:, LT:], ki[:, LI:], vtt[:, :, LT:], vti[:, :, LI:] = 0, 0, 0, 0
        _attn_cache[hw] = tuple(t.to(DEV) for t in (q, kt, vtt, ki, vti, box_cases(hw[0], hw[1], 4, AB).float()))
    return _attn_cache[hw]


def _attn_oracle(operands, hw, b, scale):
    """Row b through oracle/attention_ref (fp32 `sdpa` + `ip_region_mask`) with that row's scale."""
    from oracle.attention_ref import ip_region_mask, mask_grid_size, sdpa
    q, kt, vtt, ki, vti, bbox = (t[b:b + 1].float().cpu() for t in operands)
    N = q.shape[1]
    assert mask_grid_size(N, hw[0] / hw[1]) == tuple(hw)
    heads = lambda x, L: x[:, :L].reshape(1, L, AHEADS, 64).transpose(1, 2)
    vals = lambda vt, L: vt[:, :, :L].reshape(1, AHEADS, 64, L).transpose(-1, -2)
    qh = q.view(1, N, AHEADS, 64).transpose(1, 2)
    mask = ip_region_mask(bbox, N, 1, hw[0] / hw[1], LI - 16, 16)
    t = sdpa(qh, heads(kt, LT), vals(vtt, LT))
    i = sdpa(qh, heads(ki, LI), vals(vti, LI), mask)
    return (t + scale * i).transpose(1, 2).reshape(N, AHEADS * 64)


@pytest.mark.parametrize("variant", [0, 1, 2, 3], ids=["auto", "four_wave", "ring", "no_t16"])
@pytest.mark.parametrize("hw", [(16, 16), (12, 20)], ids=["N256", "N240_ragged"])
def test_ip_attention_scale_per_row(hip_lib, hw, variant):
    """Row b of the launch with ip_scale_dev = [0, 0.35, 1, 1.7] is, bit for bit, row b of the one-scalar launch on the same
    batch with s_b - for every ip_attn_variant the library offers (2, the LDS-DMA ring, runs where N % 256 == 0 and is the
    four-wave kernel elsewhere) - and close to the oracle called with that row's scale.  N = 240 leaves the 128-row query
    tile ragged."""
    from diffsensei_amd import ops
    operands = _attn_case(hw)
    q, kt, vtt, ki, vti, bbox = operands
    run = lambda **kw: ops.masked_ip_attention(q, kt, vtt, ki, vti, bbox, AHEADS, hw, kw.pop("ip_scale", 123.0), Lt=LT, Li=LI, **kw)
    try:
        assert hip_lib.ds_set_option(b"ip_attn_variant", variant) == 0
        y = run(ip_scale_dev=torch.tensor(SCALES, dtype=torch.float32, device=DEV))
        for b, s in enumerate(SCALES):
            assert torch.equal(y[b], run(ip_scale=s)[b]), f"row {b}: vector element vs host scalar {s}"
            assert torch.equal(y[b], run(ip_scale_dev=torch.tensor([s], dtype=torch.float32, device=DEV))[b]), \
                f"row {b}: vector element vs device scalar {s}"
    finally:
        hip_lib.ds_set_option(b"ip_attn_variant", 0)
    assert not torch.equal(y[1], run(ip_scale=SCALES[2])[1])          # the scale matters
    for b, s in enumerate(SCALES):
        ref = _attn_oracle(operands, hw, b, s).double()
        err = (y[b].double().cpu() - ref).abs().max().item() / (max(ref.abs().max().item(), 1e-3) + 1e-3)
        gate(f"per-row ip attn {hw[0]}x{hw[1]} variant {variant} row {b} scale {s} vs oracle", err, 4e-3)


def test_ip_attention_scale_per_row_through_the_plan_op(hip_lib):
    """DS_OP_IP_ATTN with i[10] = 1 (the launch plan's form) gives the bits of `ops.masked_ip_attention` with the vector."""
    import ctypes as C
    from diffsensei_amd import ops
    from diffsensei_amd.engine import make_op
    hw = (12, 20)
    q, kt, vtt, ki, vti, bbox = _attn_case(hw)
    N, Cc = hw[0] * hw[1], AHEADS * 64
    sv = torch.tensor(SCALES, dtype=torch.float32, device=DEV)
    want = ops.masked_ip_attention(q, kt, vtt, ki, vti, bbox, AHEADS, hw, 1.0, Lt=LT, Li=LI, ip_scale_dev=sv)
    o = torch.zeros_like(want)
    op = make_op("IP_ATTN", i=(AB, AHEADS, N, LT, LI, 16, 16, 4, hw[0], hw[1], 1), f=(0.125, 123.0),
                 l=(Cc, Cc, Cc, LP * Cc, Cc * LP), p=(q, kt, vtt, ki, vti, bbox, o, sv))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip_lib.ds_op_run(C.byref(op), stream) == 0, hip_lib.ds_last_error().decode()
    assert torch.equal(o, want)


# ------------------------------------------------------------------------------------------------ 3. pipeline
@pytest.fixture(scope="module")
def pipe(hip_lib):
    """The tiny pipeline of tests/test_gpu_pipeline_variants.py (128 x 128, 3 steps, latents given), restated."""
    from transformers import CLIPVisionConfig, CLIPVisionModel, ViTMAEConfig, ViTMAEModel
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.resampler import Resampler
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    torch.manual_seed(0)
    clip = CLIPVisionModel(CLIPVisionConfig(hidden_size=160, intermediate_size=320, num_hidden_layers=3,
                                            num_attention_heads=2, image_size=224, patch_size=14, hidden_act="quick_gelu")).eval()
    mae = ViTMAEModel(ViTMAEConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                                   image_size=224, patch_size=16, mask_ratio=0.0)).eval()
    cfg = tiny_config()
    sd = {k: v.half() for k, v in random_state_dict(cfg, 4).items()}
    unet = UNetMangaModel(cfg, device=DEV)
    unet.load_state_dict(sd)
    unet.set_manga_modules()
    sd = {k: v.float().cpu() for k, v in unet.state_dict().items()}
    rs = Resampler(dim=128, depth=2, dim_head=64, heads=2, num_queries=16, num_dummy_tokens=16, embedding_dim=160,
                   magi_embedding_dim=128, output_dim=cfg.cross_attention_dim, ff_mult=4, device=DEV).init_random(5)
    p = DiffSenseiPipeline(None, None, None, None, None, EulerDiscreteScheduler(), unet, clip)
    p.register_manga_modules(magi_image_encoder=mae, image_proj_model=rs)
    from PIL import Image
    rng = np.random.RandomState(3)
    img = lambda: Image.fromarray(rng.randint(0, 256, (224, 224, 3), dtype=np.uint8))
    g = torch.Generator().manual_seed(9)
    pe = lambda: torch.randn(1, 77, cfg.cross_attention_dim, generator=g).half()
    pool = lambda: torch.randn(1, 128, generator=g).half()
    base = dict(prompt="a manga panel", height=128, width=128, num_inference_steps=3)
    A = dict(base, prompt_embeds=pe(), pooled_prompt_embeds=pool(), latents=torch.randn(1, 4, 16, 16, generator=g).half(),
             ip_images=[img()], ip_bbox=[[0.1, 0.1, 0.6, 0.9]], dialog_bbox=[[0.0, 0.0, 0.3, 0.2]],
             guidance_scale=3.0, ip_scale=0.4)
    B = dict(base, prompt_embeds=pe(), pooled_prompt_embeds=pool(), latents=torch.randn(1, 4, 16, 16, generator=g).half(),
             ip_images=[img(), img()], ip_bbox=[[0.0, 0.0, 0.5, 1.0], [0.5, 0.0, 1.0, 1.0]], dialog_bbox=[],
             guidance_scale=7.5, ip_scale=1.0)
    return p, cfg, sd, rs, clip, mae, A, B


def _clone(r, **over):
    c = {k: (v.clone() if torch.is_tensor(v) else (list(v) if isinstance(v, list) else v)) for k, v in r.items()}
    c.update(over)
    return c


def _scales(r):
    return dict(guidance_scale=r["guidance_scale"], ip_scale=r["ip_scale"])


def _mixed_and_uniform(p, A, B, **extra):
    """generate_batch on [A, B] with their own sliders, and the two uniform runs of the same batch shape."""
    run = lambda ra, rb: p.generate_batch([dict(ra, **extra), dict(rb, **extra)], output_type="latent")
    mixed = run(_clone(A), _clone(B))
    info = dict(p.last_run_info)
    at_a = run(_clone(A), _clone(B, **_scales(A)))
    at_b = run(_clone(A, **_scales(B)), _clone(B))
    return mixed, at_a, at_b, info


def test_mixed_generate_batch_equals_uniform_batches(pipe):
    """Requests A (g = 3.0, s = 0.4) and B (g = 7.5, s = 1.0) in ONE UNet batch - refused before guidance and IP scale
    were per panel: row A is row A of the same batch run at A's values, row B row B of the batch at B's values."""
    p, cfg, sd, rs, clip, mae, A, B = pipe
    mixed, at_a, at_b, info = _mixed_and_uniform(p, A, B)
    assert info["batch"] == 4 and info["guidance_scales"] == [3.0, 7.5] and info["ip_scales"] == [0.4, 1.0]
    assert torch.equal(mixed[0], at_a[0]), "request A inside the mixed batch"
    assert torch.equal(mixed[1], at_b[1]), "request B inside the mixed batch"
    assert not torch.equal(mixed[0], at_b[0]) and not torch.equal(mixed[1], at_a[1])      # the sliders matter
    assert p.unet.ip_scale() == 1.0                  # the processors hold the last request's value, as after any batch


def test_sweep_in_one_call_equals_uniform_calls(pipe):
    """`num_samples=2` with two guidance and two IP scales: panel n is panel n of the uniform call at its values."""
    p, cfg, sd, rs, clip, mae, A, B = pipe
    lat = torch.cat([A["latents"], B["latents"]])
    kw = lambda **over: dict(_clone(A, latents=lat.clone(), num_samples=2, output_type="latent"), **over)
    sweep = p(**kw(guidance_scale=[3.0, 7.5], ip_scale=[0.4, 1.0])).images
    assert p.last_run_info["guidance_scales"] == [3.0, 7.5] and p.last_run_info["ip_scales"] == [0.4, 1.0]
    lo = p(**kw(guidance_scale=3.0, ip_scale=0.4)).images
    hi = p(**kw(guidance_scale=7.5, ip_scale=1.0)).images
    assert torch.equal(sweep[0], lo[0]) and torch.equal(sweep[1], hi[1])
    assert not torch.equal(sweep[0], hi[0]) and not torch.equal(sweep[1], lo[1])
    assert torch.equal(p(**kw(guidance_scale=np.float32(3.0), ip_scale=torch.tensor(0.4))).images, lo)   # any real number
    only_g = p(**kw(guidance_scale=(3.0, 7.5), ip_scale=0.4)).images          # one slider a sequence, the other a number
    assert torch.equal(only_g[0], lo[0]) and not torch.equal(only_g[1], hi[1])


def test_captured_graph_reads_the_new_vectors(pipe):
    """The vectors are static buffers: a second call on the same shape with the two vectors swapped replays the graph
    captured by the first and equals the eager run of that call."""
    p, cfg, sd, rs, clip, mae, A, B = pipe
    lat = torch.cat([A["latents"], B["latents"]])
    kw = lambda g, s: dict(_clone(B, latents=lat.clone(), num_samples=2, output_type="latent"), guidance_scale=g, ip_scale=s)
    old = p.use_graph
    try:
        p.use_graph = True
        first = p(**kw([3.0, 7.5], [0.4, 1.0])).images
        eng = p.unet.engine(4, 16, 16, 1.0)
        assert p.last_run_info["graph"] and eng.per_panel and eng.step_plan.captured
        plan = eng.step_plan
        swapped = p(**kw([7.5, 3.0], [1.0, 0.4])).images
        assert p.last_run_info["graph"] and eng.step_plan is plan, "the second call must replay the first call's graph"
        p.use_graph = False
        eager = p(**kw([7.5, 3.0], [1.0, 0.4])).images
        assert not p.last_run_info["graph"]
    finally:
        p.use_graph = old
    assert torch.equal(swapped, eager)
    assert not torch.equal(swapped, first)


@pytest.mark.parametrize("name", ["EulerDiscreteScheduler", "DDIMScheduler", "DPMSolverMultistepScheduler",
                                  "EulerAncestralDiscreteScheduler"])
def test_mixed_generate_batch_under_each_scheduler(pipe, name):
    from diffsensei_amd import schedulers as S
    p, cfg, sd, rs, clip, mae, A, B = pipe
    old = p.scheduler
    try:
        p.scheduler = getattr(S, name)() if name in ("EulerDiscreteScheduler", "DDIMScheduler") else getattr(S, name)(**SDXL)
        extra = dict(noise_seeds=[5]) if p.scheduler.stochastic else {}
        mixed, at_a, at_b, _ = _mixed_and_uniform(p, A, B, **extra)
    finally:
        p.scheduler = old
    assert torch.isfinite(mixed[0]).all() and torch.isfinite(mixed[1]).all()
    assert torch.equal(mixed[0], at_a[0]) and torch.equal(mixed[1], at_b[1])
    assert not torch.equal(mixed[1], at_a[1])


def _oracle(cfg, sd, rs, clip, mae, req, guidance, ip_scale):
    """The oracle sampling loop of tests/test_gpu_pipeline_variants.py::_oracle for ONE request (one sample) with its own
    guidance and IP scale."""
    from PIL import Image
    from transformers import CLIPImageProcessor, ViTImageProcessor
    from oracle.pipeline_ref import sample_loop
    from oracle.resampler_ref import resampler_forward
    from oracle.scheduler_ref import EulerDiscreteOracle
    from oracle.unet_ref import UNetOracle
    imgs = req["ip_images"]
    n_real = len(imgs)
    padded = list(imgs) + [Image.new("RGB", (224, 224))] * (4 - n_real)
    with torch.no_grad():
        ce = clip(CLIPImageProcessor()(images=padded, return_tensors="pt").pixel_values,
                  output_hidden_states=True).hidden_states[-2].unsqueeze(0)
        me = mae(ViTImageProcessor()(images=padded, return_tensors="pt").pixel_values).last_hidden_state[:, 0].unsqueeze(0)
        ce[0, n_real:], me[0, n_real:] = 0, 0
        rsd = {k: v.float().cpu() for k, v in rs.state_dict().items()}
        img = hq(resampler_forward(rsd, ce, me, 2, 64))
        neg = hq(resampler_forward(rsd, torch.zeros_like(ce), torch.zeros_like(me), 2, 64))
        pe, pooled = req["prompt_embeds"].float(), req["pooled_prompt_embeds"].float()
        enc = torch.cat([torch.cat([torch.zeros_like(pe), pe]), torch.cat([neg, img])], dim=1)
        te = torch.cat([torch.zeros(1, pooled.shape[1]), pooled])
        tid = torch.tensor([[128, 128, 0, 0, 128, 128]] * 2, dtype=torch.float32)
        bbox = torch.zeros(2, 4, 4)
        for j, bx in enumerate(req["ip_bbox"]):
            bbox[1:, j] = torch.tensor(bx)
        db = torch.zeros(2, 8, 4, dtype=torch.float16)
        for j, bx in enumerate(req["dialog_bbox"]):
            db[1:, j] = torch.tensor(bx).half()
        sch = EulerDiscreteOracle().set_timesteps(3)
        return sample_loop(UNetOracle(cfg, sd, q=hq), EulerDiscreteOracle(), hq(req["latents"].float() * sch.init_noise_sigma),
                           hq(enc), hq(te), tid, bbox, db, guidance, 3, ip_scale, q=hq)


def test_mixed_pair_against_the_oracle(pipe):
    """Each request of the mixed batch against the oracle loop run for that request alone with ITS guidance and IP scale,
    at the fused-sampler gate (1.2e-2) of tests/test_gpu_pipeline_variants.py."""
    p, cfg, sd, rs, clip, mae, A, B = pipe
    out = p.generate_batch([_clone(A), _clone(B)], output_type="latent")
    for name, r, o in (("A", A, out[0]), ("B", B, out[1])):
        ref = _oracle(cfg, sd, rs, clip, mae, r, r["guidance_scale"], r["ip_scale"])
        gate(f"test_gpu_per_panel_scales: mixed batch, request {name} vs its own oracle loop", _rel(o, ref), 1.2e-2)


def test_refusals(pipe):
    p, cfg, sd, rs, clip, mae, A, B = pipe
    lat = torch.cat([A["latents"], B["latents"]])
    kw = lambda **over: dict(_clone(A, latents=lat.clone(), num_samples=2, output_type="latent"), **over)
    with pytest.raises(ValueError):
        p(**kw(guidance_scale=[0.5, 5.0]))                               # CFG off and on in one batch
    with pytest.raises(ValueError):
        p(**kw(guidance_scale=[3.0, 5.0, 7.5]))                          # three values for two samples
    with pytest.raises(ValueError):
        p(**kw(ip_scale=[0.4]))
    with pytest.raises(ValueError):
        p.generate_batch([_clone(A, guidance_scale=1.0), _clone(B)], output_type="latent")
    with pytest.raises(ValueError):
        p.generate_batch([_clone(A), _clone(B, height=256, width=256)], output_type="latent")
    # both requests without CFG share a batch like any other pair
    out = p.generate_batch([_clone(A, guidance_scale=1.0), _clone(B, guidance_scale=0.5)], output_type="latent")
    assert p.last_run_info["batch"] == 2 and torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()
