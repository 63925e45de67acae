"""GPU: `UNetMangaModel.forward` and the fused sampling loop (launch plan over the HIP kernels, through the C ABI)
against the CPU oracle on identical seeded weights and inputs.

Tolerances: the HIP path stores activations in fp16 like the reference's fp16 inference; it is compared with the
oracle run in fp16-storage emulation (`q = half-roundtrip`) at relative L2 error <= 5e-3 on a full UNet forward (measured
1.3-1.6e-3 at every size from the tiny config to 2048 x 2048; the gate was 2e-2 until round 5) and with the pure-fp32
oracle at <= 6e-3.  Every model-level gate goes through tests/_gates.gate, which logs the measured value beside its tolerance.
The 50-step loops (all four samplers) are held to twice the distance between those two oracles' own loops, computed in the test.
"""
import pytest
import torch

from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
hq = lambda t: t.half().float()


def _inputs(cfg, B=2, H=16, W=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g).half()
    enc = torch.randn(B, cfg.num_text_tokens + cfg.num_ip_tokens, cfg.cross_attention_dim, generator=g).half()
    pooled = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
    te = torch.randn(B, pooled, generator=g).half()
    tid = torch.tensor([[H * 8, W * 8, 0, 0, H * 8, W * 8]] * B, dtype=torch.float16)
    bbox = torch.zeros(B, 4, 4)
    bbox[B // 2:, 0] = torch.tensor([0.05, 0.10, 0.50, 0.95])
    bbox[B // 2:, 1] = torch.tensor([0.50, 0.10, 0.95, 0.95])
    db = torch.zeros(B, 8, 4, dtype=torch.float16)
    db[B // 2:, 0] = torch.tensor([0.05, 0.02, 0.30, 0.15], dtype=torch.float16)
    db[B // 2:, 1] = torch.tensor([0.65, 0.02, 0.95, 0.15], dtype=torch.float16)
    return x, enc, te, tid, bbox, db


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


@pytest.fixture(scope="module")
def tiny(hip_lib):
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    from oracle.unet_ref import UNetOracle
    cfg = tiny_config()
    sd = {k: v.half() for k, v in random_state_dict(cfg, 0).items()}
    model = UNetMangaModel(cfg, device=DEV)
    model.load_state_dict(sd)
    model._attn_processors = {}
    oracle16 = UNetOracle(cfg, sd, q=hq)
    oracle32 = UNetOracle(cfg, sd)
    return cfg, sd, model, oracle16, oracle32


@pytest.mark.parametrize("H,W", [(16, 16), (8, 32)])
def test_unet_forward_vs_oracle(tiny, H, W):
    cfg, sd, model, o16, o32 = tiny
    x, enc, te, tid, bbox, db = _inputs(cfg, 2, H, W)
    model._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    o16.ip_scale = o32.ip_scale = 0.6
    out = model(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": H / W},
                added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    with torch.no_grad():
        r16 = o16.forward(x, 801.0, enc, te, tid, bbox, H / W, db)
        r32 = o32.forward(x, 801.0, enc, te, tid, bbox, H / W, db)
    assert out.shape == x.shape and torch.isfinite(out).all()
    gate(f"tiny UNet {H}x{W} vs fp16-storage oracle", _rel(out, r16), 5e-3)
    gate(f"tiny UNet {H}x{W} vs fp32 oracle", _rel(out, r32), 6e-3)
    # conditioning reaches the output through the HIP path too
    out2 = model(x.to(DEV), 401.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": H / W},
                 added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    assert _rel(out2, out) > 1e-3
    out3 = model(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": torch.zeros_like(bbox), "aspect_ratio": H / W},
                 added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=None).sample
    assert _rel(out3[1], out[1]) > 1e-4
    # determinism
    out4 = model(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": H / W},
                 added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    assert torch.equal(out, out4)


@pytest.mark.parametrize("H,W", [(18, 13), (7, 9), (33, 20), (17, 17)])
def test_unet_forward_any_latent_size(tiny, H, W):
    """The reference takes every image side that is a multiple of 8 (demo sliders step 8): latent sides need not be
    multiples of 4.  Downsample2D gives ceil(h/2); the up path resizes to the skip's size (diffusers
    `forward_upsample_size`), token counts need not be multiples of 8.  HIP plan vs the oracle, same tolerances."""
    cfg, sd, model, o16, o32 = tiny
    x, enc, te, tid, bbox, db = _inputs(cfg, 2, H, W, seed=H * 100 + W)
    model._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    o16.ip_scale = 0.6
    out = model(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": H / W},
                added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    with torch.no_grad():
        r16 = o16.forward(x, 801.0, enc, te, tid, bbox, H / W, db)
    assert out.shape == x.shape and torch.isfinite(out).all()
    gate(f"tiny UNet {H}x{W} (any latent size) vs fp16-storage oracle", _rel(out, r16), 5e-3)


@pytest.mark.parametrize("kind", ["euler", "ddim"])
def test_sampling_loop_vs_oracle(tiny, kind):
    """4 fused steps (UNet + CFG + scheduler) on the GPU vs oracle/pipeline_ref.sample_loop, eager and hipGraph."""
    from diffsensei_amd.schedulers import DDIMScheduler, EulerDiscreteScheduler
    from diffsensei_amd.unet import dialog_pixel_boxes
    from oracle.pipeline_ref import sample_loop
    from oracle.scheduler_ref import DDIMOracle, EulerDiscreteOracle
    cfg, sd, model, o16, o32 = tiny
    ns, H, W, steps = 1, 16, 16, 4
    x, enc, te, tid, bbox, db = _inputs(cfg, 2 * ns, H, W, seed=3)
    sch = EulerDiscreteScheduler() if kind == "euler" else DDIMScheduler()
    sch.set_timesteps(steps)
    lat0 = (x[:ns].float() * sch.init_noise_sigma).half()
    with torch.no_grad():
        ref = sample_loop(o16, EulerDiscreteOracle() if kind == "euler" else DDIMOracle(), lat0.float(), enc.float(),
                          te.float(), tid.float(), bbox, db, 7.5, steps, 0.6, q=hq)
    eng = model.engine(2 * ns, H, W, H / W)
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
    assert torch.equal(results[0], results[1]), "hipGraph replay differs from eager launches"
    gate(f"4 fused {kind} steps (CFG 7.5) vs oracle sample_loop", _rel(results[0], ref), 1.2e-2)


# ---- the model in the loop for the benchmarked 50 steps, all four samplers
LOOP_STEPS, LOOP_SNAPS, LOOP_SEEDS = 50, (5, 10, 25, 50), [20260101]
_LOOP_KINDS = {"euler": 0, "ddim": 1, "dpm": 2, "euler_a": 3}
_loop_oracles = {}          # kind -> (snapshots of the fp16-storage oracle loop, of the fp32 one): one CPU pass each per module


def _loop_scheduler(kind):
    from diffsensei_amd import schedulers as S
    from tests._sampler_common import SDXL
    cls = [S.EulerDiscreteScheduler, S.DDIMScheduler, S.DPMSolverMultistepScheduler, S.EulerAncestralDiscreteScheduler]
    sch = cls[_LOOP_KINDS[kind]](**SDXL)
    sch.set_timesteps(LOOP_STEPS)
    return sch


def _loop_oracle_scheduler(kind, exact):
    """The scheduler restatement; exact: without fp16 points of its own (the fp32 loop)."""
    from oracle.scheduler_ref import DDIMOracle, EulerDiscreteOracle
    from tests._dpm_ref import DPMSolverOracle
    from tests._euler_a_ref import EulerAncestralOracle
    if kind == "euler":
        return EulerDiscreteOracle()
    if kind == "ddim":
        return DDIMOracle()
    if kind == "dpm":
        return DPMSolverOracle(q=(lambda t: t)) if exact else DPMSolverOracle()
    return EulerAncestralOracle(seeds=LOOP_SEEDS, exact=exact)


def _loop_oracle_curves(tiny, kind, lat0, inputs):
    from oracle.pipeline_ref import sample_loop
    if kind not in _loop_oracles:
        cfg, sd, model, o16, o32 = tiny
        x, enc, te, tid, bbox, db = inputs
        args = (enc.float(), te.float(), tid.float(), bbox, db, 7.5, LOOP_STEPS, 0.6)
        with torch.no_grad():
            r16 = sample_loop(o16, _loop_oracle_scheduler(kind, False), lat0.float(), *args, q=hq, record=LOOP_SNAPS)[1]
            r32 = sample_loop(o32, _loop_oracle_scheduler(kind, True), lat0.float(), *args, record=LOOP_SNAPS)[1]
        _loop_oracles[kind] = (r16, r32)
    return _loop_oracles[kind]


@pytest.mark.parametrize("kind", list(_LOOP_KINDS))
def test_sampling_loop_50_steps_vs_oracle(tiny, kind):
    """50 fused steps (UNet + CFG 7.5 + scheduler, ns 1, 16 x 16 latents) on the GPU, eager and 50 replays of the captured step
    plan, against oracle/pipeline_ref.sample_loop with the fp16-storage UNet oracle and with the fp32 one.  The yardstick is
    the references' own distance D16_32(k) = rel-L2(oracle16, oracle32) after k steps: the device differs from oracle16 by
    summation order and fused rounding points only - a perturbation of the same kind and at most the same size - so at
    k = 5, 10, 25, 50 it has to stay within 2 * D16_32(k) of both.  Condition on the references alone: D16_32(50) <= 1e-2
    (the loop through this random-weight UNet is not chaotic)."""
    from diffsensei_amd.unet import dialog_pixel_boxes
    cfg, sd, model, o16, o32 = tiny
    ns, H, W = 1, 16, 16
    inputs = _inputs(cfg, 2 * ns, H, W, seed=3)
    x, enc, te, tid, bbox, db = inputs
    sch = _loop_scheduler(kind)
    lat0 = (x[:ns].float() * sch.init_noise_sigma).half()
    eng = model.engine(2 * ns, H, W, H / W)
    eng.build_sampler(ns, sch.kind, True)
    table = torch.from_numpy(sch.coef_table(7.5))
    assert table.shape == (LOOP_STEPS, 8)
    results = []
    for mode in ("eager", "graph"):
        eng.set_request(enc, te, tid, bbox, dialog_pixel_boxes(db, H, W), 0.6)
        eng.load_schedule(table, solver_rows=torch.from_numpy(sch.solver_table()) if kind == "dpm" else None,
                          noise_seeds=LOOP_SEEDS if kind == "euler_a" else None)
        eng.latents.copy_(lat0)
        snaps = {}
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            eng.prep_plan.run(st.cuda_stream)
            if mode == "graph" and not eng.step_plan.captured:
                eng.step_plan.capture(st.cuda_stream)
            for k in range(1, LOOP_STEPS + 1):
                (eng.step_plan.replay if mode == "graph" else eng.step_plan.run)(st.cuda_stream)
                if k in LOOP_SNAPS:
                    snaps[k] = eng.latents.clone()
        st.synchronize()
        assert int(eng.ctr.item()) == LOOP_STEPS
        results.append(snaps)
    for k in LOOP_SNAPS:
        assert torch.equal(results[0][k], results[1][k]), f"hipGraph replay differs from eager launches after {k} steps"
    r16, r32 = _loop_oracle_curves(tiny, kind, lat0, inputs)
    d16_32 = {k: _rel(r16[k], r32[k]) for k in LOOP_SNAPS}
    d32 = {k: _rel(results[0][k], r32[k]) for k in LOOP_SNAPS}
    d16 = {k: _rel(results[0][k], r16[k]) for k in LOOP_SNAPS}
    for k in LOOP_SNAPS:                            # every figure first, then the assertions
        assert torch.isfinite(results[0][k]).all()
        print(f"{kind} after {k} steps: D16_32 {d16_32[k]:.3e}, device vs fp32 loop {d32[k]:.3e}, vs fp16-storage loop {d16[k]:.3e}")
    gate(f"50-step {kind} loop: D16_32(50), the references alone", d16_32[LOOP_STEPS], 1e-2)
    for k in LOOP_SNAPS:
        gate(f"{k} of 50 fused {kind} steps (CFG 7.5) vs the fp32 oracle loop (2 x D16_32)", d32[k], 2 * d16_32[k])
        gate(f"{k} of 50 fused {kind} steps (CFG 7.5) vs the fp16-storage oracle loop (2 x D16_32)", d16[k], 2 * d16_32[k])


def test_unet_model_api_surface(hip_lib):
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import tiny_config
    m = UNetMangaModel.from_config(tiny_config(), device=DEV).init_random(0)
    m.set_manga_modules(max_num_ips=4, num_vision_tokens=16, max_num_dialogs=8)
    assert m.config.max_num_ips == 4 and m.config["cross_attention_dim"] == 256
    procs = m.attn_processors
    assert sum(hasattr(p, "scale") for p in procs.values()) == sum(n.endswith("attn2.processor") for n in procs)
    sd = m.state_dict()
    k = next(n for n in sd if n.endswith("attn2.processor.to_k_ip.weight"))
    assert torch.equal(sd[k], sd[k.replace("processor.to_k_ip", "to_k")])   # IP K initialised from text K
    with pytest.raises(RuntimeError):
        m.load_state_dict({"nope": torch.zeros(1)})
    with pytest.raises(ValueError):
        m(torch.zeros(2, 4, 16, 16), 1.0, torch.zeros(2, 157, 256))


@pytest.fixture(scope="module")
def sdxl_model(hip_lib):
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import sdxl_config
    cfg = sdxl_config()
    return cfg, UNetMangaModel(cfg, device=DEV).init_random(0)


def test_unet_sdxl_shapes_one_forward(sdxl_model):
    """Full SDXL-size weights, 512x512 latent (64x64), CFG batch 2: finite, deterministic, batch items independent."""
    cfg, m = sdxl_model
    x, enc, te, tid, bbox, db = _inputs(cfg, 2, 64, 64, seed=7)
    kw = dict(cross_attention_kwargs={"bbox": bbox, "aspect_ratio": 1.0},
              added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db)
    y = m(x.to(DEV), 981.0, enc.to(DEV), **kw).sample
    assert y.shape == (2, 4, 64, 64) and torch.isfinite(y).all() and y.float().std() > 1e-3
    assert torch.equal(y, m(x.to(DEV), 981.0, enc.to(DEV), **kw).sample)
    xs = torch.cat([x[1:], x[:1]])
    sw = lambda t: torch.cat([t[1:], t[:1]])
    y2 = m(xs.to(DEV), 981.0, sw(enc).to(DEV), cross_attention_kwargs={"bbox": sw(bbox), "aspect_ratio": 1.0},
           added_cond_kwargs={"text_embeds": sw(te), "time_ids": sw(tid)}, dialog_bbox=sw(db)).sample
    assert _rel(y2[0], y[1]) < 2e-3 and _rel(y2[1], y[0]) < 2e-3


def test_unet_sdxl_forward_vs_oracle(sdxl_model):
    """PARITY AT A BASELINE SHAPE: the full SDXL-size UNet (2.9 B parameters incl. the IP projections) at 512x512
    (64x64 latents, BASELINE.json configs[0]'s resolution), CFG batch 2 with character boxes and a dialog box: the HIP launch
    plan vs the CPU oracle on identical weights and inputs.  Tolerance: relative L2 <= 5e-3 against the oracle with fp16
    storage emulation (what the reference's fp16 inference does between ops; measured 1.5e-3), <= 6e-3 against pure fp32."""
    from oracle.unet_ref import UNetOracle
    cfg, m = sdxl_model
    x, enc, te, tid, bbox, db = _inputs(cfg, 2, 64, 64, seed=11)
    m._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    y = m(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": 1.0},
          added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        o16 = UNetOracle(cfg, sd, q=hq)
        o16.ip_scale = 0.6
        r16 = o16.forward(x, 801.0, enc, te, tid, bbox, 1.0, db)
        o32 = UNetOracle(cfg, sd)
        o32.ip_scale = 0.6
        r32 = o32.forward(x, 801.0, enc, te, tid, bbox, 1.0, db)
    assert y.shape == r16.shape and torch.isfinite(y).all()
    e16, e32 = _rel(y, r16), _rel(y, r32)
    print(f"SDXL 512x512 forward: rel-L2 vs fp16-storage oracle {e16:.3e}, vs fp32 oracle {e32:.3e}")
    gate("SDXL UNet 512x512 vs fp16-storage oracle", e16, 5e-3)
    gate("SDXL UNet 512x512 vs fp32 oracle", e32, 6e-3)
    # the conditional row must differ from the unconditional one (boxes / dialog reach the output at this size too)
    assert _rel(y[1], y[0]) > 1e-3


@pytest.fixture(scope="module")
def oracle_1024(sdxl_model):
    """The seed-13 CFG pair at 1024 x 1024 (two character boxes, two dialog boxes) and its fp16-storage oracle forward - one CPU
    forward (~1 min on the GPU box's host cores) shared by every test below that ties a 1024 x 1024 plan to the oracle."""
    from oracle.unet_ref import UNetOracle
    cfg, m = sdxl_model
    inputs = _inputs(cfg, 2, 128, 128, seed=13)
    x, enc, te, tid, bbox, db = inputs
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        o16 = UNetOracle(cfg, sd, q=hq)
        o16.ip_scale = 0.6
        r16 = o16.forward(x, 801.0, enc, te, tid, bbox, 1.0, db)
    del o16, sd
    return inputs, r16


def test_unet_sdxl_forward_vs_oracle_1024(sdxl_model, oracle_1024):
    """PARITY AT THE METRIC'S SHAPE (BASELINE.json metric / configs[1], [2]): full SDXL-size weights, 1024x1024
    (128x128 latents), CFG batch 2, 2 character boxes + 2 dialog boxes - the HIP launch plan vs the CPU oracle with
    fp16-storage emulation, relative L2 <= 5e-3 (measured 1.52e-3; reference path: src/pipelines/pipeline_diffsensei.py:322-329 ->
    src/models/unet.py:116-347).  Then the SAME two rows inside UNet batches of 32 and of 64 - 64 is the batch `python bench.py`
    runs (num_samples 32; rows 0..31 = the unconditional row, 32..63 = the conditional row): those launch plans dispatch to
    the large-problem kernels (gemm_pp at M = 65536 / 262144 with the V^T projections folded into the persistent walk at
    nbatch 64, conv_halo256, self_attn_sp_kernel, the N = 4096 masked-IP grid; single activation tensors reach 1.3 GB), and
    their rows must reproduce the oracle-checked B = 2 result (<= 2e-3 relative L2; bit-equality is reported) and each other
    bit for bit inside a batch, tying the BENCHED dispatch to the oracle-checked one."""
    cfg, m = sdxl_model
    (x, enc, te, tid, bbox, db), r16 = oracle_1024
    m._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    kw = lambda bb, t_e, t_i, d: dict(cross_attention_kwargs={"bbox": bb, "aspect_ratio": 1.0},
                                      added_cond_kwargs={"text_embeds": t_e, "time_ids": t_i}, dialog_bbox=d)
    y = m(x.to(DEV), 801.0, enc.to(DEV), **kw(bbox, te, tid, db)).sample
    assert y.shape == (2, 4, 128, 128) and torch.isfinite(y).all()
    # ---- batch 32: rows replicated 16x per CFG half
    rep = lambda t: torch.cat([t[:1].repeat(16, *([1] * (t.dim() - 1))), t[1:].repeat(16, *([1] * (t.dim() - 1)))])
    y32 = m(rep(x).to(DEV), 801.0, rep(enc).to(DEV), **kw(rep(bbox), rep(te), rep(tid), rep(db))).sample
    assert y32.shape == (32, 4, 128, 128) and torch.isfinite(y32).all()
    for r in range(32):
        assert torch.equal(y32[r], y32[0 if r < 16 else 16]), f"row {r} of the batch-32 forward differs from its replica"
    d0, d1 = _rel(y32[0], y[0]), _rel(y32[16], y[1])
    print(f"SDXL 1024x1024: batch-32 rows vs batch-2 rows rel-L2 {d0:.3e} / {d1:.3e}, bit-equal: "
          f"{torch.equal(y32[0], y[0]) and torch.equal(y32[16], y[1])}")
    # (<= 4e-3: since round 4 the large batches run the LayerNorms of the 1280-channel blocks fused into the GEMMs around
    # them - 1.3e-3 apart from the LayerNorm-kernel plan of the batch-2 forward, both equally far from the oracle below)
    assert d0 <= 4e-3 and d1 <= 4e-3, (d0, d1)
    # ---- batch 64 = the benchmark's own UNet batch (bench.py: num_samples 32, CFG): rows replicated 32x per CFG half
    rep64 = lambda t: torch.cat([t[:1].repeat(32, *([1] * (t.dim() - 1))), t[1:].repeat(32, *([1] * (t.dim() - 1)))])
    y64 = m(rep64(x).to(DEV), 801.0, rep64(enc).to(DEV), **kw(rep64(bbox), rep64(te), rep64(tid), rep64(db))).sample
    assert y64.shape == (64, 4, 128, 128) and torch.isfinite(y64).all()
    for r in range(64):
        assert torch.equal(y64[r], y64[0 if r < 32 else 32]), f"row {r} of the batch-64 forward differs from its replica"
    e0, e1 = _rel(y64[0], y[0]), _rel(y64[32], y[1])
    print(f"SDXL 1024x1024: batch-64 rows vs batch-2 rows rel-L2 {e0:.3e} / {e1:.3e}, bit-equal to the batch-32 rows: "
          f"{torch.equal(y64[0], y32[0]) and torch.equal(y64[32], y32[16])}")
    assert e0 <= 4e-3 and e1 <= 4e-3, (e0, e1)
    eng64 = m._engines[next(k for k in m._engines if k[0] == 64)]
    print(f"batch-64 plan: {len(eng64.forward_ops)} launches, {getattr(eng64, 'ln_fused_blocks', 0)} transformer blocks with fused LayerNorms")
    y64 = torch.stack([y64[0], y64[32]]).clone()
    torch.cuda.empty_cache()
    # ---- oracle (the module fixture's one forward)
    e2, e32, e64 = _rel(y, r16), _rel(torch.stack([y32[0], y32[16]]), r16), _rel(y64, r16)
    print(f"SDXL 1024x1024 forward: rel-L2 vs fp16-storage oracle: batch 2 {e2:.3e}, rows of batch 32 {e32:.3e}, "
          f"rows of batch 64 (the benched batch) {e64:.3e}")
    gate("SDXL UNet 1024x1024 batch 2 vs fp16-storage oracle", e2, 5e-3)
    gate("SDXL UNet 1024x1024 rows of batch 32 vs fp16-storage oracle", e32, 5e-3)
    gate("SDXL UNet 1024x1024 rows of batch 64 (the benched batch) vs fp16-storage oracle", e64, 5e-3)
    assert _rel(y[1], y[0]) > 1e-3


def test_unet_sdxl_partial_layernorm_fusion_768(sdxl_model, monkeypatch):
    """The launch-plan builder fuses per norm and per kernel family: at 768 x 768 (96 x 96 latents, 576 tokens at the
    1280-channel level) and UNet batch 16 the out-projections, q|k and the GEGLU projections of the 1280-channel level reach
    gemm_pp_kernel's branch-free epilogues (M = 9216 = 36 row tiles), the transposed to_v (576 columns per image: no whole
    256-column tile) and the out-projections of the 640-channel level run the 128-wide kernels' fused epilogue - every norm is
    fused, through a mix of the two families.  Rows of that forward vs the batch-2 forward of the same inputs built with
    DIFFSENSEI_LN_FUSION=0 (every LayerNorm a launch of its own): <= 4e-3, bit-equal inside the batch - whatever tile, wave and
    lane a row lands in (images start at offsets 576 r mod 256 inside the row tiles); the plan must really be the mixed one."""
    cfg, m = sdxl_model
    x, enc, te, tid, bbox, db = _inputs(cfg, 2, 96, 96, seed=17)
    m._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    kw = lambda bb, t_e, t_i, d: dict(cross_attention_kwargs={"bbox": bb, "aspect_ratio": 1.0},
                                      added_cond_kwargs={"text_embeds": t_e, "time_ids": t_i}, dialog_bbox=d)
    with monkeypatch.context() as mp:
        mp.setenv("DIFFSENSEI_LN_FUSION", "0")
        y = m(x.to(DEV), 801.0, enc.to(DEV), **kw(bbox, te, tid, db)).sample
        assert getattr(m._engines[next(k for k in m._engines if k[0] == 2 and k[1] == 96)], "ln_fused_launches", 0) == 0
    rep = lambda t: torch.cat([t[:1].repeat(8, *([1] * (t.dim() - 1))), t[1:].repeat(8, *([1] * (t.dim() - 1)))])
    y16 = m(rep(x).to(DEV), 801.0, rep(enc).to(DEV), **kw(rep(bbox), rep(te), rep(tid), rep(db))).sample
    eng = m._engines[next(k for k in m._engines if k[0] == 16)]
    fused = getattr(eng, "ln_fused_launches", 0)
    print(f"768x768 batch 16: {getattr(eng, 'ln_fused_blocks', 0)} blocks with fused LayerNorms, {fused} LayerNorm launches replaced")
    assert getattr(eng, "ln_fused_blocks", 0) == 70 and fused == 210, "expected every LayerNorm of every transformer block fused"
    assert 0 < eng.ln_finalize_launches < 210, "expected a mix of gemm_pp_kernel consumers (finalize launch) and 128-wide ones (none)"
    for r in range(16):
        assert torch.equal(y16[r], y16[0 if r < 8 else 8])
    d0, d1 = _rel(y16[0], y[0]), _rel(y16[8], y[1])
    print(f"768x768: batch-16 rows (partial LayerNorm fusion) vs batch-2 rows rel-L2 {d0:.3e} / {d1:.3e}")
    assert d0 <= 4e-3 and d1 <= 4e-3, (d0, d1)


def test_unet_sdxl_small_batch_rows_are_position_independent(sdxl_model):
    """72 x 72 latents (324 / 1296 tokens per image at the two attention levels: images start at every offset inside the 64- and
    128-row tiles of the small-batch GEMMs), three copies each of two inputs = UNet batch 6: every LayerNorm of the plan is folded
    into the 128-wide kernels' epilogues (row form, operand-swapped form, statistics producers), and the copies must come out
    bit-identical - the check that caught a slot-dependent f16 rounding in round 4 (profiles/r04_determinism_bisect.txt)."""
    cfg, m = sdxl_model
    x, enc, te, tid, bbox, db = _inputs(cfg, 2, 72, 72, seed=23)
    m._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    rep = lambda t: torch.cat([t[:1].repeat(3, *([1] * (t.dim() - 1))), t[1:].repeat(3, *([1] * (t.dim() - 1)))])
    y = m(rep(x).to(DEV), 801.0, rep(enc).to(DEV), cross_attention_kwargs={"bbox": rep(bbox), "aspect_ratio": 1.0},
          added_cond_kwargs={"text_embeds": rep(te), "time_ids": rep(tid)}, dialog_bbox=rep(db)).sample
    eng = m._engines[next(k for k in m._engines if k[0] == 6 and k[1] == 72)]
    assert eng.ln_fused_launches >= 140, eng.ln_fused_launches
    for r in range(6):
        assert torch.equal(y[r], y[0 if r < 3 else 3]), r
    assert _rel(y[3], y[0]) > 1e-3
    # with norm1 fused, the transposed to_v GEMM reads the RAW residual stream `t_hidden` at ceil8(N) rows per image -
    # up to 7 rows behind the last image when N % 8 != 0 (324 tokens here).  The stream therefore carries 8 rows of slack that no
    # producer may write and that must read as zero (they become the V^T pad columns: 0 x NaN would poison the P V MFMA).
    checked = 0
    for (role, level), t in eng.scratch.items():
        if role != "t_hidden":
            continue
        H, W = eng.hw[level]
        N, Cc = H * W, cfg.block_out_channels[level]
        M = 6 * N
        assert t.numel() >= (M + 8) * Cc, (level, t.numel(), (M + 8) * Cc)
        slack = t[M * Cc:(M + 8) * Cc]
        assert torch.count_nonzero(slack).item() == 0, f"level {level}: a producer wrote into the slack behind the hidden stream"
        checked += N % 8 != 0
    assert checked >= 1, "expected a level whose token count is not a multiple of 8"


# ---- the 1024 x 1024 UNet batches of BASELINE configs[2] (num_samples 4 -> batch 8; 2048 x 2048 at batch 2 has the same GEMM and
# convolution plan but for the V^T projections: tests/test_gpu_unet_plans.py) and of num_samples 2 (batch 4): their plans send the
# projections to kernels no batch-2 or batch-64 plan runs (gemm_g320_kernel's plain form, the 128-row tiles of gemm_t160_kernel).
# Rows are DISTINCT (uncond, cond) pairs - replicas would hide a batch-index fault; pair 0 is the oracle-checked seed-13 pair.

def _pairs_1024(cfg, oracle_1024, n):
    from tests.test_gpu_large_shapes import _item
    inputs, _ = oracle_1024
    pairs = [(tuple(t[:1] for t in inputs), tuple(t[1:] for t in inputs))]
    return pairs + [(_item(cfg, 128, 128, 3000 + s, False), _item(cfg, 128, 128, 4000 + s, True)) for s in range(1, n)]


@pytest.fixture(scope="module")
def batch2_pairs_1024(sdxl_model, oracle_1024):
    """Four pairs and the batch-2 forward of each (the plan test_unet_sdxl_forward_vs_oracle_1024 ties to the oracle)."""
    from tests.test_gpu_large_shapes import _forward
    cfg, m = sdxl_model
    m._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    pairs = _pairs_1024(cfg, oracle_1024, 4)
    return pairs, [_forward(m, list(p)).float().cpu() for p in pairs]


def _kernel_inventory(eng):
    import ctypes as C
    from collections import Counter
    from diffsensei_amd import _lib
    lib = _lib.load()
    name, fl, by, names = C.create_string_buffer(96), C.c_double(), C.c_double(), Counter()
    for op in eng.forward_ops:
        assert lib.ds_op_describe(C.byref(op), name, 96, C.byref(fl), C.byref(by)) == 0
        names[name.value.decode()] += 1
    return names


def _distinct_pairs_case(sdxl_model, oracle_1024, batch2_pairs_1024, n, tol_rows, tol_oracle):
    """UNet batch 2 n: rows 0..n-1 the unconditional items of pairs 0..n-1, rows n..2n-1 their conditional items.  Every row vs the
    batch-2 forward of its own pair; the negative control (row i vs pair j != i) must be > 10x that gate; pair 0 vs the oracle."""
    from tests.test_gpu_large_shapes import _forward
    cfg, m = sdxl_model
    m._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    pairs, y2 = batch2_pairs_1024
    pairs, y2 = pairs[:n], y2[:n]
    y = _forward(m, [p[0] for p in pairs] + [p[1] for p in pairs]).float().cpu()
    assert y.shape == (2 * n, 4, 128, 128) and torch.isfinite(y).all()
    own = max(max(_rel(y[j], y2[j][0]), _rel(y[n + j], y2[j][1])) for j in range(n))
    other = min(min(_rel(y[i], y2[j][0]), _rel(y[n + i], y2[j][1])) for i in range(n) for j in range(n) if i != j)
    print(f"SDXL 1024x1024 UNet batch {2 * n} of {n} distinct pairs: worst row vs its own batch-2 forward {own:.3e}, "
          f"closest row vs another pair's {other:.3e}")
    gate(f"SDXL UNet 1024x1024 batch {2 * n} of distinct pairs vs their batch-2 forwards, worst row", own, tol_rows)
    gate(f"SDXL UNet 1024x1024 batch {2 * n}: row vs another pair's batch-2 forward (negative control)", other, 10 * tol_rows, lower=True)
    _, r16 = oracle_1024
    gate(f"SDXL UNet 1024x1024 rows of batch {2 * n} (pair 0) vs fp16-storage oracle", _rel(torch.stack([y[0], y[n]]), r16), tol_oracle)
    eng = m._engines[next(k for k in m._engines if k[0] == 2 * n and k[1] == 128)]
    names = _kernel_inventory(eng)
    print(f"batch-{2 * n} plan, {len(eng.forward_ops)} launches: {dict(sorted(names.items()))}")
    return names


def test_unet_sdxl_batch8_of_distinct_pairs_1024(sdxl_model, oracle_1024, batch2_pairs_1024):
    """BASELINE configs[2]'s UNet batch (num_samples 4, CFG): the q|k projections of the 1280-channel level (M = 8192, N = 2560,
    K = 1280) and the 640-channel level's attn2.to_q / conv_shortcut (M = 32768, N = 640) run gemm_g320_kernel's plain form."""
    # measured on MI355X: worst row 1.47e-3, pair 0 vs the oracle 1.51e-3, closest row vs another pair 1.33
    names = _distinct_pairs_case(sdxl_model, oracle_1024, batch2_pairs_1024, 4, 4e-3, 4.5e-3)
    assert names["gemm_g320_kernel<plain>"] == 71 and names["gemm_g320_kernel"] == 0, names
    assert not any(k.startswith("gemm_t160") for k in names), names


def test_unet_sdxl_batch4_of_distinct_pairs_1024(sdxl_model, oracle_1024, batch2_pairs_1024):
    """num_samples 2 (UNet batch 4): every N = 1280 projection of the 1280-channel level (M = 4096) runs the 128 x 160 tiles of
    gemm_t160_kernel - as LayerNorm-statistics producer (160-column format), consumer and plain - and the 640-channel level's q|k
    (M = 16384, N = 1280, K = 640) gemm_g320_kernel's plain form."""
    # measured on MI355X: worst row 1.39e-3, pair 0 vs the oracle 1.52e-3, closest row vs another pair 1.33
    names = _distinct_pairs_case(sdxl_model, oracle_1024, batch2_pairs_1024, 2, 4e-3, 4.5e-3)
    assert names["gemm_t160_kernel<128 rows>"] == 253 and names["gemm_t160_kernel"] == 0, names
    assert names["gemm_g320_kernel<plain>"] == 10, names


def test_unet_sdxl_forward_vs_oracle_768(sdxl_model):
    """768 x 768 (96 x 96 latents) at UNet batch 2 vs the fp16-storage oracle - the inputs of
    test_unet_sdxl_partial_layernorm_fusion_768, whose batch-16 rows are compared with a batch-2 forward of this size."""
    from oracle.unet_ref import UNetOracle
    cfg, m = sdxl_model
    x, enc, te, tid, bbox, db = _inputs(cfg, 2, 96, 96, seed=17)
    m._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    y = m(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": 1.0},
          added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample.float().cpu()
    assert y.shape == (2, 4, 96, 96) and torch.isfinite(y).all()
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        o16 = UNetOracle(cfg, sd, q=hq)
        o16.ip_scale = 0.6
        r16 = o16.forward(x, 801.0, enc, te, tid, bbox, 1.0, db)
    gate("SDXL UNet 768x768 batch 2 vs fp16-storage oracle", _rel(y, r16), 4.5e-3)   # measured 1.52e-3
    assert _rel(y[1], y[0]) > 1e-3
