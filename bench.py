#!/usr/bin/env python
"""Headline benchmark: manga panels/sec at 50 denoise steps, 1024x1024, 2 character refs (BASELINE.json `metric`).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is ONE `DiffSenseiPipeline.__call__` over a batch of `--num-samples` panels: character encoders
(CLIP-H + Magi ViT-MAE + Resampler) -> 50 x (UNet forward on the CFG batch + CFG + scheduler step) on the HIP launch
plan.  Inputs are synthetic and already resident in HBM where tensors are involved (prompt embeddings, character
images are 224x224 uint8 that go through the reference's CPU image processors).  Weights: seeded random at the true
SDXL / CLIP-H / ViT-MAE / Resampler shapes (no checkpoint is reachable offline; throughput is value independent).
The timed region also runs both SDXL text encoders (CLIP-L + OpenCLIP bigG shapes, HIP engine) on the prompt and the
negative prompt (token ids from a synthetic tokenizer: no vocabulary files offline) and ends, like the reference's
`__call__` (pipeline_diffsensei.py:339-367), with the SDXL VAE decode + denormalisation on the scaled-fp16 HIP decoder (config.vae_precision) and the
conversion to PIL images on the host (uint8 conversion on the device, 3 bytes per pixel over PCIe); `--output pt` stops
at [0,1] fp32 images on the device (round-1 region), `--no-vae` at the latents.

N > 1: one process per GPU, weights broadcast from rank 0 over RCCL once (time reported, outside the timed region),
each rank serves its own requests with no data-path collective -> "scaling": "weak".  Timing: barrier +
synchronize on both sides, MAX over ranks; value = N * K * num_samples / t.

A plain run sets up, warms up, times the K steps and prints the line; `roofline`, `cpu_baseline` and `parity` are null there.
`--full` adds them after the timed steps (the `--no-*` options below drop single ones again):
`roofline` (dominant kernel of the UNet forward, algorithmic flops / HIP-event time
vs the 2.5 PFLOP/s dense fp16 MFMA peak), `cpu_baseline` (the whole `__call__` of BASELINE.json configs[0] on the fp32 CPU
oracle, the Euler loop interrupted after 2 of 20 steps and only the loop extrapolated; rank 0 at N=1 only) and `parity`
(`path: "__call__"`: the SAME call - prompt, negative prompt, noise, weights, interrupt point - through `pipe(...)` on the
GPU: relative L2 of the latents, and the uint8 image bytes compared.  The bench FAILS when the latents differ by more than
6e-3 (bounded 2-step sample; measured 1.7e-3) / 1.2e-2 (`--cpu-full`, all 20 steps: fp16 storage vs fp32 compounds through
CFG 7.5; measured 2.1e-3) or the image by more than 8e-3 (measured 1.9e-3); until round 5 these gates were 3e-2 / 6e-2 / 5e-2).

`--dump-outputs DIR` writes what the last timed step returned (rank 0) as float32 / float64 `.npy` files, see dump_outputs().
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

T_START = time.perf_counter()
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MFMA_PEAK_TFLOPS = 2500.0      # dense fp16/bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def log_phase(what):
    log(f"bench.py: {what} at {time.perf_counter() - T_START:.1f} s")


def build_pipeline(device, num_gpus, rank, seed=0, with_vae=True, agent=None, keep_oracle=False):
    """Reference construction recipe (scripts/demo/gradio_wo_mllm.py:161-200) with synthetic weights."""
    from transformers import CLIPVisionConfig, CLIPVisionModel, ViTMAEConfig, ViTMAEModel
    from diffsensei_amd.distributed import broadcast_pipeline
    from diffsensei_amd.encoders import ClipVisionEngine, ViTMAEEngine
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.resampler import Resampler
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import sdxl_config

    t0 = time.perf_counter()
    cfg = sdxl_config()
    unet = UNetMangaModel(cfg, device=device).init_random(seed if rank == 0 else 1000 + rank)
    torch.manual_seed(seed)
    clip_cfg = CLIPVisionConfig(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16,
                                image_size=224, patch_size=14, hidden_act="gelu", projection_dim=1024)   # ViT-H/14
    mae_cfg = ViTMAEConfig(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                           image_size=224, patch_size=16, mask_ratio=0.0)                                  # Magi crop encoder
    keep = {}                    # fp32 CPU modules holding exactly the engines' fp16 weights: the oracle chain of `parity`

    def cpu_module(name, m):
        m = m.eval()
        with torch.no_grad():
            for prm in m.parameters():
                prm.copy_(prm.half().float())
        if keep_oracle:
            keep[name] = m
        return m

    with torch.device("cpu"):
        clip = ClipVisionEngine.from_transformers(cpu_module("image_encoder", CLIPVisionModel(clip_cfg)), device)
        magi = ViTMAEEngine.from_transformers(cpu_module("magi", ViTMAEModel(mae_cfg)), device)
    resampler = Resampler(dim=1280, depth=4, dim_head=64, heads=20, num_queries=16, num_dummy_tokens=16,
                          embedding_dim=1280, magi_embedding_dim=768, output_dim=cfg.cross_attention_dim, ff_mult=4,
                          device=device).init_random(seed + 1)
    # SDXL prompt encoders (CLIP ViT-L/14 text, OpenCLIP bigG/14 text) at their true shapes, random init
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    from diffsensei_amd.encoders import ClipTextEngine
    t1 = CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                        num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu")
    t2 = CLIPTextConfig(vocab_size=49408, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32,
                        num_attention_heads=20, max_position_embeddings=77, hidden_act="gelu", projection_dim=1280)
    with torch.device("cpu"):
        te1 = ClipTextEngine.from_transformers(cpu_module("text_encoder", CLIPTextModel(t1)), device)
        te2 = ClipTextEngine.from_transformers(cpu_module("text_encoder_2", CLIPTextModelWithProjection(t2)), device)
    # SDXL VAE decoder (49.5 M parameters) at its true shapes, random init (scaled-fp16 HIP engine unless DIFFSENSEI_VAE_PRECISION says bf16)
    # The seeded state dict is rounded ONCE to the engine's storage type and that very dict feeds both the engine and (kept
    # below) the oracle of `parity`, so the two sides hold the same weights bit for bit (the oracle used a bf16
    # rounding of its own while the scaled-fp16 engine held fp16 roundings).
    from diffsensei_amd.vae import VaeConfig, VaeDecoderEngine, random_state_dict as vae_random_sd
    vae = vae_sd = None
    if with_vae:
        vprec = os.environ.get("DIFFSENSEI_VAE_PRECISION", "fp16-scaled")
        vdt = torch.bfloat16 if vprec == "bf16" else torch.float16
        vae_sd = {k: v.to(vdt).float() for k, v in vae_random_sd(VaeConfig(), seed + 2).items()}
        vae = VaeDecoderEngine.from_state_dict(vae_sd, VaeConfig(), device, precision=vprec)
    t_init = time.perf_counter() - t0
    tok = SyntheticTokenizer()
    pipe = DiffSenseiPipeline(vae=vae, text_encoder=te1, text_encoder_2=te2, tokenizer=tok, tokenizer_2=tok,
                              scheduler=EulerDiscreteScheduler(), unet=unet, image_encoder=clip)
    pipe.register_manga_modules(magi_image_encoder=magi, image_proj_model=resampler)
    if keep_oracle:
        keep.update(tokenizer=tok, tokenizer_2=tok, resampler_heads=20, resampler_dim_head=64, vae_sd=vae_sd)
        pipe._oracle_modules = keep
    # N > 1: every engine's frozen weights (pipe.tensors() [+ the MLLM agent]) are re-homed into one flat arena per dtype and
    # the arena goes out from rank 0 in asynchronous 512 MiB slices (no staging copies), then an all-reduced checksum proves
    # the replicas are bit-identical (ranks != 0 were seeded differently on purpose)
    bstats = {"bytes": 0, "seconds": 0.0, "buckets": 0, "verify_ms": 0.0, "tensors": 0, "consolidate_s": 0.0}
    if num_gpus > 1:
        dist.barrier()
        bstats = broadcast_pipeline(pipe, extra=[agent] if agent is not None else [])
    return pipe, {"init_s": round(t_init, 2), "broadcast_bytes": bstats["bytes"],
                  "broadcast_ms": round(bstats["seconds"] * 1e3, 2), "broadcast_buckets": bstats["buckets"],
                  "broadcast_rehome_ms": round(bstats.get("consolidate_s", 0.0) * 1e3, 2),
                  "broadcast_verify_ms": round(bstats["verify_ms"], 2), "broadcast_tensors": bstats["tensors"]}


class SyntheticTokenizer:
    """CLIP tokenizer stand-in (no vocabulary files offline): hashes words to ids, BOS 49406 / EOS+pad 49407, 77 slots."""
    model_max_length = 77

    def __call__(self, text, padding=None, max_length=77, truncation=True, return_tensors="pt"):
        words = [1 + (sum(ord(c) * (i + 1) for i, c in enumerate(w)) % 49000) for w in text.split()]
        ids = [49406] + words[: max_length - 2] + [49407]
        ids += [49407] * (max_length - len(ids))
        return type("Enc", (), {"input_ids": torch.tensor([ids])})()


def synthetic_request(device, size, seed, output_type="pt", refs=2):
    import numpy as np
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    rng = np.random.RandomState(seed)
    imgs = [Image.fromarray(rng.randint(0, 256, (224, 224, 3), dtype=np.uint8)) for _ in range(refs)]
    boxes = [[0.05, 0.10, 0.50, 0.95], [0.50, 0.10, 0.95, 0.95]] if refs <= 2 else \
        [[0.03, 0.05, 0.48, 0.50], [0.52, 0.05, 0.97, 0.50], [0.03, 0.52, 0.48, 0.97], [0.52, 0.52, 0.97, 0.97]]
    return dict(
        prompt="A young man with a surprised expression holding a baby on his back", height=size, width=size,
        num_inference_steps=50, guidance_scale=7.5, ip_images=imgs,
        ip_bbox=boxes[:refs], ip_scale=0.6,
        dialog_bbox=[[0.05, 0.02, 0.30, 0.15], [0.65, 0.02, 0.95, 0.15]],
        negative_prompt="think lines, pure black background, colored, lowres, bad anatomy, worst quality, low quality",
        generator=torch.Generator().manual_seed(seed), output_type=output_type)


def mllm_synthetic_inputs(seed=7):
    """Synthetic tokenised instruction of scripts/demo/gradio.py:36-60 (no tokenizer files offline):
    [bos, 40 text ids, <img>, 64 placeholders, </img>, 3 text ids, <img>] - the trailing <img> starts the forced 64-token
    image block (random weights never emit it on their own), 66 new tokens in total.  Pure host code (CPU-tested)."""
    boi = 32100
    chain = [boi] + [boi + 1 + i for i in range(64)] + [boi + 65]
    g = torch.Generator().manual_seed(seed)
    text = lambda n: torch.randint(3, 32000, (n,), generator=g).tolist()
    ids = [1] + text(40) + chain + text(3) + [boi]
    mask = torch.zeros(len(ids), dtype=torch.bool)
    mask[42:42 + 64] = True
    return {"input_ids": torch.tensor(ids), "ids_cmp_mask": mask, "chain": chain, "max_new": 66}


def build_mllm_agent(device, seed=7):
    """The agent of scripts/demo/gradio.py:255-270 at LLaMA-2-13B dimensions with seeded random weights."""
    from diffsensei_amd.mllm import (ContinuousLVLM, LlamaConfig, LlamaDecodeEngine, QwenResampler,
                                     random_llama_state_dict, random_qwen_resampler_state_dict)
    cfg = LlamaConfig()
    llm = LlamaDecodeEngine(cfg, random_llama_state_dict(cfg, device, seed), device, max_positions=256, max_new_tokens=128)
    res_in = QwenResampler(random_qwen_resampler_state_dict(8, cfg.hidden_size, 2048, device, seed + 1), 32, device)
    res_out = QwenResampler(random_qwen_resampler_state_dict(8, 2048, cfg.hidden_size, device, seed + 2), 32, device)
    return ContinuousLVLM(llm, res_in, res_out), mllm_synthetic_inputs(seed)


def cpu_call_and_gpu_parity(pipe, req, cpu_full=False, parity=True, budget_steps=2):
    """BASELINE configs[0] - 512x512, 20-step Euler, text-only (`ip_images=[]`), batch 1 - as ONE whole call of the
    reference function (pipeline_diffsensei.py:180-372) on both sides:

    * `cpu_baseline`: `oracle.pipeline_ref.call_oracle` on the host cores in fp32 - tokenise, both SDXL text encoders,
      prepare_ip_image_embeds (4 black references through the HF processors, CLIP-H, ViT-MAE, zeroed, Resampler), the Euler
      loop, the fp32 VAE decode, postprocess to uint8.  Bounded sample: the loop is interrupted after `budget_steps` of the 20
      steps (the reference's own `interrupt` flag: the remaining iterations `continue`) and ONLY the loop time is
      extrapolated to 20 steps; encoders, VAE decode and postprocess are measured whole.  `--cpu-full`: all 20 steps.
    * `parity` (`path: "__call__"`): the SAME call - same prompt, negative prompt, initial noise, weights (the oracle's
      modules hold the engines' fp16-rounded weights), same interrupt point - through `pipe(...)` on the GPU, compared on
      the latents (relative L2, tolerance 6e-3 for <= 4 steps / 1.2e-2 for the 20-step run: fp16 storage vs pure fp32
      compounding through CFG 7.5) and on the uint8 image bytes the call returns (`image_rel_l2` on pixels / 255, the
      fraction of bytes that differ at all and by more than 1 LSB, the largest difference)."""
    import numpy as np
    from diffsensei_amd.unet_config import sdxl_config
    from diffsensei_amd.vae import VaeConfig
    from oracle.pipeline_ref import call_oracle
    from oracle.unet_ref import UNetOracle
    mods = dict(pipe._oracle_modules)
    vcfg = VaeConfig()
    assert mods.get("vae_sd") is not None, "parity needs the VAE (the engine and the oracle share ONE rounded state dict)"
    mods["vae_cfg"] = {"layers_per_block": vcfg.layers_per_block, "norm_num_groups": vcfg.norm_num_groups, "eps": vcfg.eps,
                       "scaling_factor": vcfg.scaling_factor}
    mods["resampler_sd"] = {k: v.float().cpu() for k, v in pipe.image_proj_model.state_dict().items()}
    unet_o = UNetOracle(sdxl_config(), {k: v.float().cpu() for k, v in pipe.unet._sd.items()})
    size, steps, gs, ip_scale = 512, 20, 7.5, 0.6
    lat0 = torch.randn(1, 4, size // 8, size // 8, generator=torch.Generator().manual_seed(0))
    n_run = steps if cpu_full else budget_steps
    tm = {}
    t0 = time.perf_counter()
    ref = call_oracle(mods, unet_o, req["prompt"], req["negative_prompt"], size, size, steps, gs, lat0, ip_images=[],
                      ip_bbox=[], ip_scale=ip_scale, dialog_bbox=[], num_samples=1, max_steps=n_run, timings=tm)
    wall = time.perf_counter() - t0
    fixed = tm["text_encoders_s"] + tm["character_encoders_s"] + tm["vae_postprocess_s"]
    panel_s = fixed + tm["denoise_s"] * steps / n_run
    cpu = {"value": round(1.0 / panel_s, 6), "unit": "panels/s", "cores": torch.get_num_threads(), "kind": "port",
           "s_per_panel": round(panel_s, 1),
           "sample": (f"the whole __call__ of BASELINE configs[0] (512x512, 20-step Euler, text-only, batch 1) on the fp32 torch "
                      f"oracle, {wall:.1f} s measured: text encoders {tm['text_encoders_s']:.1f} s + character encoders / "
                      f"Resampler {tm['character_encoders_s']:.1f} s + {n_run} of {steps} Euler steps (CFG batch 2) "
                      f"{tm['denoise_s']:.1f} s + fp32 VAE decode / uint8 {tm['vae_postprocess_s']:.1f} s; " +
                      ("nothing extrapolated" if n_run == steps else f"only the loop is extrapolated to {steps} steps")),
           "spread_note": "box-to-box spread of this figure is up to 2x (host cores shared; BASELINE.md section 5)"}
    del unet_o
    if not parity:
        return cpu, None

    def stop(p, i, t, kw):
        if i + 1 >= n_run:
            p._interrupt = True
        return kw

    kw = dict(prompt=req["prompt"], negative_prompt=req["negative_prompt"], height=size, width=size, num_inference_steps=steps,
              guidance_scale=gs, num_samples=1, ip_images=[], ip_bbox=[], ip_scale=ip_scale, dialog_bbox=[],
              callback_on_step_end=stop)
    got_lat = pipe(latents=lat0.clone(), output_type="latent", **kw).images.float().cpu()
    pil = pipe(latents=lat0.clone(), output_type="pil", **kw).images
    got_u8 = np.asarray(pil[0])
    assert torch.isfinite(got_lat).all() and got_u8.shape == ref["u8"][0].shape == (size, size, 3)
    rl = ref["latents"].float()
    d = got_u8.astype(np.int16) - ref["u8"][0].astype(np.int16)
    a, b = got_u8.astype(np.float64) / 255.0, ref["u8"][0].astype(np.float64) / 255.0
    par = {"path": "__call__",
           "config": "C1: 512x512, 20-step Euler, text-only, batch 1 (BASELINE.json configs[0]), prompt + negative prompt -> PIL",
           "steps": n_run, "interrupted_after": None if n_run == steps else n_run,
           "rel_l2": round(((got_lat - rl).norm() / rl.norm()).item(), 6),
           "max_abs": round((got_lat - rl).abs().max().item(), 5),
           "tolerance": 6e-3 if n_run <= 4 else 1.2e-2,
           "image_rel_l2": round(float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12)), 6), "image_tolerance": 8e-3,
           "u8_frac_differ": round(float((d != 0).mean()), 6), "u8_frac_gt_1lsb": round(float((np.abs(d) > 1).mean()), 6),
           "u8_max_diff": int(np.abs(d).max()), "u8_std_ref": round(float(ref["u8"][0].std()), 2),
           "vs": "oracle/pipeline_ref.call_oracle (fp32 torch + transformers modules, CPU) on the same weights / prompt / noise"}
    return cpu, par


def vae_precision_note(pipe, ns, size, call_s, world):
    """What the VAE leg of the timed region computes in, beside what the reference does there (fp32: it upcasts the VAE,
    pipeline_diffsensei.py:339-344), and a LOWER bound of the headline if a true-fp32 decode were required: fp32 MFMA runs at
    1/16 of the fp16 rate (157 TFLOP/s, MI355X_MICROARCH.md), so 10.5 TFLOP per 1024^2 image cost >= 67 ms instead of the
    ~14 ms measured for the scaled-fp16 decoder (tools/vae_bench.py, profiles/r03_vae_conv_out_8lane.txt)."""
    fp32_ms = 10.5e12 * (size / 1024.0) ** 2 / 157e12 * 1e3
    ours_ms = 14.3 * (size / 1024.0) ** 2
    extra_s = ns * max(fp32_ms - ours_ms, 0.0) * 1e-3
    return {"engine": pipe.vae.precision,
            "arithmetic": ("fp16 operands with every stored tensor scaled by 2^-6, fp32 accumulation / statistics / softmax"
                           if pipe.vae.precision == "fp16-scaled" else "bf16 storage, fp32 accumulation / statistics / softmax"),
            "reference": "fp32 (vae upcast, pipeline_diffsensei.py:339-344)",
            "parity_evidence": "tests/test_gpu_vae.py::test_vae_decode_1024_vs_oracle (1024x1024, chunked batch 8, uint8 within "
                               "1 LSB of the fp32 oracle on >= 99.9 % of the bytes), ::test_decoder_uint8_parity_where_fp16_would_overflow",
            "fp32_decode_exposure": {"per_image_ms_at_fp32_mfma_peak": round(fp32_ms, 1), "per_image_ms_this_engine": round(ours_ms, 1),
                                     "value_lower_bound_if_fp32_decode": round(world * ns / (call_s + extra_s), 4)}}


DUMP_WHOLE_BYTES = 48 << 20     # outputs up to this size (as float32) are written whole, and no dump is larger
DUMP_SAMPLE = 1 << 22           # else: this many elements drawn with numpy's default_rng(0), + the first panel + per-panel means


def dump_outputs(images, out_type, ddir):
    """`--dump-outputs DIR`: what the last timed step handed its caller, for an output-by-output comparison of two builds.
    pil: the uint8 RGB images as one (n, H, W, 3) array; pt: the (n, 3, H, W) [0,1] images; latent: the (n, 4, h, w) latents.
    Written as float32 `<name>.npy` when it fits DUMP_WHOLE_BYTES; otherwise `<name>_sample.npy` (DUMP_SAMPLE elements of the
    flattened array at indices drawn by numpy.random.default_rng(0), so they depend only on the output's size),
    `<name>_first.npy` (panel 0 whole, when it fits the rest of DUMP_WHOLE_BYTES: up to 1024^2 at the default --size) and
    `<name>_mean.npy` (float64 mean of every panel)."""
    import numpy as np
    if out_type == "pil":
        name, arr = "images", np.stack([np.asarray(im) for im in images])
    else:
        name, arr = ("latents" if out_type == "latent" else "images"), images.float().cpu().numpy()
    os.makedirs(ddir, exist_ok=True)
    files = {}
    if arr.size * 4 <= DUMP_WHOLE_BYTES:
        files[name] = arr.astype(np.float32)
    else:
        idx = np.random.default_rng(0).integers(0, arr.size, DUMP_SAMPLE)
        files[name + "_sample"] = arr.reshape(-1)[idx].astype(np.float32)
        if (arr[0].size + DUMP_SAMPLE) * 4 + arr.shape[0] * 8 <= DUMP_WHOLE_BYTES:
            files[name + "_first"] = arr[0].astype(np.float32)
        files[name + "_mean"] = arr.reshape(arr.shape[0], -1).mean(axis=1, dtype=np.float64)
    for k, v in files.items():
        np.save(os.path.join(ddir, k + ".npy"), v)
    log("bench.py: outputs written to", ddir, {k: list(v.shape) for k, v in files.items()})


def profile_forward_ops(pipe, reps=3):
    """HIP-event time of every op of the UNet forward plan, on the stream the kernels are launched on; grouped by
    the gfx950 kernel they dispatch to.  Returns (per-kernel table, forward_ms)."""
    from diffsensei_amd import _lib
    lib = _lib.load()
    eng = next(iter(pipe.unet._engines.values()))
    ops = eng.forward_ops
    st = torch.cuda.Stream()
    n = len(ops)
    acc = [0.0] * n
    with torch.cuda.stream(st):
        for rep in range(reps + 1):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            evs[0].record(st)
            for k, op in enumerate(ops):
                rc = lib.ds_op_run(C.byref(op), st.cuda_stream)
                assert rc == 0, lib.ds_last_error()
                evs[k + 1].record(st)
            st.synchronize()
            if rep:  # first pass warms caches
                for k in range(n):
                    acc[k] += evs[k].elapsed_time(evs[k + 1])
    table = {}
    name = C.create_string_buffer(96)
    fl, by = C.c_double(), C.c_double()
    for k, op in enumerate(ops):
        lib.ds_op_describe(C.byref(op), name, 96, C.byref(fl), C.byref(by))
        d = table.setdefault(name.value.decode(), {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
        d["launches"] += 1
        d["ms"] += acc[k] / reps
        d["flops"] += fl.value
        d["bytes"] += by.value
    return table, sum(acc) / reps


def spawn_ranks(n: int) -> int:
    """Re-run this command line as `python -m torch.distributed.run --nnodes=1 --nproc-per-node n ... bench.py <same flags>`
    on a free local port (rendezvous on 127.0.0.1: the container hostname may not resolve) and return its exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    log("bench.py: no torchrun environment, starting", n, "ranks:", " ".join(cmd[1:8]), "...")
    return subprocess.call(cmd, env=env)


def dry_run(args, rank: int, world: int) -> None:
    """The launcher / process-group / timing skeleton of main() with a sleep for a step (no GPU, no kernels)."""
    for _ in range(args.warmup):
        time.sleep(0.01)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.01)
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt])
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if rank == 0:
        print(json.dumps({"metric": "dry run (no kernels)", "value": None, "unit": "panels/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 2),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dry_run": True}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--num-samples", type=int, default=int(os.environ.get("DS_BENCH_NUM_SAMPLES", "32")),
                    help="panels per call (UNet batch = 2 x this).  The metric fixes resolution, steps and references, not the "
                         "batch: 32 makes every projection of the level-2 transformers a whole number of 256-tile rounds "
                         "(round 3: 1.34 panels/s vs 1.29 at 16, profiles/r03_bench_ns32_*.json); DS_BENCH_NUM_SAMPLES overrides")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure `roofline` (per-kernel HIP-event times of the UNet forward), "
                         "`cpu_baseline` and `parity` (BASELINE configs[0] on the fp32 CPU oracle and through pipe(...)); "
                         "a plain run leaves them null")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0) to DIR/*.npy, float32 / float64 (dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no cpu_baseline / parity")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: no roofline")
    ap.add_argument("--no-vae", action="store_true", help="stop at the latents (the first timed region of round 1)")
    ap.add_argument("--output", choices=("pil", "pt"), default="pil",
                    help="pil: PIL images on the host like the reference's __call__ (default, the metric's region); "
                         "pt: [0,1] fp32 images left on the device (the round-1 region)")
    ap.add_argument("--refs", type=int, default=2, choices=(0, 1, 2, 3, 4),
                    help="character references in the request (BASELINE config 2: 1, config 5: 4)")
    ap.add_argument("--no-dialog", action="store_true", help="no dialog boxes (BASELINE config 2)")
    ap.add_argument("--no-parity", action="store_true",
                    help="with --full: skip the GPU-vs-oracle parity run on BASELINE configs[0]")
    ap.add_argument("--cpu-full", action="store_true",
                    help="implies --full: cpu_baseline runs ALL 20 Euler steps of BASELINE configs[0] plus the fp32 VAE "
                         "decode on the host cores (~6 min on the GPU box) instead of the bounded 2-step sample, and `parity` "
                         "compares the 20-step latents and the decoded image (SURVEY 8d: the whole call, not an extrapolation)")
    ap.add_argument("--mllm", action="store_true",
                    help="BASELINE config 3: run the MLLM pre-pass (LLaMA-2-13B dims, 66 new tokens) inside the timed "
                         "region and feed its ip_image_embeds to the sampler (scripts/demo/gradio.py:85-129); "
                         "not part of the default metric line (round 1: every stage GPU-tested and the pre-pass "
                         "measured on its own by tools/mllm_bench.py; the combined full-size run is still to be taken)")
    ap.add_argument("--dry-run", action="store_true",
                    help="control flow only (launcher, process group, barriers, max-over-ranks timing, the JSON line): the "
                         "step is a 10 ms sleep, no kernels, runs without a GPU - tests/test_distributed_gloo.py uses it")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    args.full = args.full or args.cpu_full

    # `python bench.py --gpus N` without a torchrun environment: start the N ranks ourselves (the plain form
    # used to die on the WORLD_SIZE assert).  Under torchrun (RANK / WORLD_SIZE exported) this is skipped.
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    from diffsensei_amd.distributed import init_from_env
    rank, world, local = init_from_env(("nccl" if torch.cuda.is_available() else "gloo") if args.gpus > 1 else None)
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher exported WORLD_SIZE={world}")
    if args.dry_run:
        return dry_run(args, rank, world)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    from diffsensei_amd import build as _build
    if rank == 0:
        _build.build(verbose=False)
    if world > 1:
        dist.barrier()
    log_phase("library ready")

    do_roofline = args.full and not args.no_roofline
    do_cpu_baseline = args.full and not args.no_cpu_baseline and rank == 0 and world == 1
    agent = mllm_in = None
    if args.mllm:
        agent, mllm_in = build_mllm_agent(device, seed=7 if rank == 0 else 70 + rank)
    pipe, setup = build_pipeline(device, world, rank, with_vae=not args.no_vae, agent=agent, keep_oracle=do_cpu_baseline)
    log_phase("weights ready")
    ns = args.num_samples
    out_type = "latent" if args.no_vae else args.output
    req = synthetic_request(device, args.size, seed=1234 + rank, output_type=out_type, refs=args.refs)
    if args.no_dialog:
        req["dialog_bbox"] = []

    def one_step():
        r = req
        if agent is not None:                      # gradio.py:85-129: references -> MLLM -> blended character tokens
            from diffsensei_amd.mllm import mllm_prepass
            emb = mllm_prepass(pipe, agent, mllm_in["input_ids"], mllm_in["ids_cmp_mask"], r["ip_images"], 0.4,
                               img_ids_list=mllm_in["chain"], eos_token_id=2, max_new_tokens=mllm_in["max_new"])
            r = dict(r, ip_images=[], ip_image_embeds=emb, ip_bbox=list(r["ip_bbox"]) + [[0.0] * 4] * (4 - len(r["ip_bbox"])))
        out = pipe(num_samples=ns, **r)
        return out.images

    for i in range(args.warmup):
        one_step()
        if i == 0:
            torch.cuda.synchronize()
            log_phase("first warmup step done")
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    log_phase("timed steps start")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        lat = one_step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if out_type == "pil":
        assert len(lat) == ns and all(im.size == (args.size, args.size) and im.mode == "RGB" for im in lat)
        import numpy as np
        px = np.asarray(lat[0])
        assert px.std() > 0, "constant image"
    else:
        assert torch.isfinite(lat.float()).all(), "non-finite output"
        if not args.no_vae:
            assert lat.shape == (ns, 3, args.size, args.size) and float(lat.min()) >= 0.0 and float(lat.max()) <= 1.0
    panels = world * args.steps * ns
    value = panels / dt
    log_phase("timed steps done")
    if rank == 0 and args.dump_outputs:
        dump_outputs(lat, out_type, args.dump_outputs)

    roofline = None
    extra = {}
    if rank == 0 and do_roofline:
        table, fwd_ms = profile_forward_ops(pipe)
        # gemm_pp_kernel has five instantiations since round 4 (template argument FUSE: 0 plain, 1 / 9 / 4 fused-LayerNorm
        # consumers with the plain / GEGLU / operand-swapped epilogue, 2 producer): the same main loop, separate symbols in a
        # rocprofv3 trace.  The roofline object is that of the kernel as a whole, as in rounds 1-3; `instantiations` lists
        # each symbol's own launches / average duration / rate for the comparison with the trace.
        fam = {k: v for k, v in table.items() if k.startswith("gemm_pp_kernel<")}
        if fam:
            table = {k: v for k, v in table.items() if k not in fam}
            table["gemm_pp_kernel"] = {f: sum(v[f] for v in fam.values()) for f in ("launches", "ms", "flops", "bytes")}
        dom = max(table.items(), key=lambda kv: kv[1]["ms"])
        name, d = dom
        ach = d["flops"] / (d["ms"] * 1e-3) / 1e12
        peak = MFMA_PEAK_TFLOPS
        roofline = {"bound": "mfma", "achieved": round(ach, 1), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(ach / peak, 4), "traffic": None, "kernel": name,
                    "launches_per_forward": d["launches"], "avg_launch_us": round(d["ms"] * 1e3 / d["launches"], 2),
                    "algorithmic_tflop_per_forward": round(d["flops"] / 1e12, 3)}
        if name == "gemm_pp_kernel" and fam:
            roofline["instantiations"] = {k: {"launches": v["launches"], "avg_launch_us": round(v["ms"] * 1e3 / v["launches"], 2),
                                              "tflops": round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 1)}
                                          for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])}
        # HBM-side traffic comes from separate rocprofv3 --pmc passes (tools/gpu_pmc_pp.sh), committed under profiles/:
        # it cannot be collected inside this process.  Attached only when it was measured for this very kernel.
        for pmc_name in ("r05_pmc_gemm_pp.json", "r04_pmc_gemm_pp.json", "r03_pmc_gemm_pp.json", "r02_pmc_gemm_pp.json", "r01_pmc_gemm_pp.json"):   # newest committed pass for this kernel
            pmc_path = os.path.join(ROOT, "profiles", pmc_name)
            if not os.path.exists(pmc_path):
                continue
            pmc = json.load(open(pmc_path))
            # ... and for a launch this workload issues: the pass measured the GEGLU projection of the 32x32-token level at one
            # UNet batch (M = batch x 1024 tokens), so other --num-samples / --size settings leave traffic null.
            if pmc.get("kernel", "").startswith(name) and pmc["shape"].get("M") == 2 * ns * (args.size // 32) ** 2:
                roofline["traffic"] = pmc["traffic_bytes_per_launch"]
                roofline["traffic_detail"] = {"unit": "bytes per launch (FETCH_SIZE x2 + WRITE_SIZE, L2 fabric side)",
                                              "launch": pmc["shape"], "algorithmic_bytes": pmc["algorithmic_bytes_per_launch"],
                                              "l2_hit_rate": pmc["l2_hit_rate"], "source": "profiles/" + pmc_name}
                break
        tot_fl = sum(v["flops"] for v in table.values())
        extra = {"unet_forward_ms_event_sum": round(fwd_ms, 3),
                 "unet_forward_algorithmic_tflop": round(tot_fl / 1e12, 2),
                 "unet_forward_tflops": round(tot_fl / (fwd_ms * 1e-3) / 1e12, 1),
                 "per_kernel": {k: {"launches": v["launches"], "ms": round(v["ms"], 3),
                                    "tflops": round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 1),
                                    "gbs": round(v["bytes"] / max(v["ms"], 1e-9) / 1e6, 1)} for k, v in
                                sorted(table.items(), key=lambda kv: -kv[1]["ms"])}}
        log(json.dumps(extra, indent=1))

    cpu_baseline = parity = None
    if do_cpu_baseline:
        cpu_baseline, parity = cpu_call_and_gpu_parity(pipe, req, cpu_full=args.cpu_full,
                                                         parity=not (args.no_parity or args.no_vae))
        if parity is not None:
            log("parity:", json.dumps(parity))
            assert parity["rel_l2"] <= parity["tolerance"], \
                f"GPU latents differ from the CPU oracle on BASELINE configs[0]: {parity}"
            assert parity["image_rel_l2"] <= parity["image_tolerance"], \
                f"GPU image differs from the CPU oracle on BASELINE configs[0]: {parity}"

    if rank == 0:
        line = {
            "metric": "manga panels/sec at 50 denoise steps, 1024x1024, 2 char refs",
            "value": round(value, 4), "unit": "panels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": f"{args.size}x{args.size}, 50-step Euler, CFG 7.5, {args.refs} character refs (padded to 4) + "
                                   f"{0 if args.no_dialog else 2} dialog boxes, num_samples={ns} per call (UNet batch {2 * ns}), "
                                   f"one call per step",
                       "output": out_type, "self_attention": "fp16",
                       "timed_region": "2 SDXL text encoders (prompt + negative prompt), CLIP-H + ViT-MAE + Resampler "
                                       "character encoding, 50 x (UNet + CFG + scheduler step)" +
                                       ("; VAE decode excluded (output: latents)" if args.no_vae else
                                        f", SDXL VAE decode + denormalize ({pipe.vae.precision} HIP engine)" +
                                        ("; uint8 conversion on the device, D2H, PIL images on the host (reference :367)"
                                         if out_type == "pil" else "; output: [0,1] fp32 images on the device")),
                       "mllm_prepass": ("LLaMA-2-13B dims, 111-token prompt + 66 new tokens (64-token image block), both "
                                        "QwenResamplers, blend; timed") if args.mllm else None,
                       "vae_precision": None if args.no_vae else vae_precision_note(pipe, ns, args.size, dt / args.steps, world),
                       "num_samples": ns, "unet_batch": 2 * ns, "hipgraph": pipe.last_run_info.get("graph"),
                       "kernel_launches_per_denoise_step": pipe.last_run_info.get("ops_per_step"),
                       "weights": "seeded random at SDXL UNet / CLIP-L + bigG text / CLIP-H / ViT-MAE / Resampler / VAE decoder shapes", **setup},
            "roofline": roofline, "cpu_baseline": cpu_baseline, "parity": parity,
        }
        if extra:
            line["unet_forward"] = {k: extra[k] for k in ("unet_forward_ms_event_sum", "unet_forward_algorithmic_tflop",
                                                          "unet_forward_tflops")}
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
