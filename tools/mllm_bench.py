#!/usr/bin/env python
"""MLLM pre-pass decode rate at LLaMA-2-13B dimensions (random weights): tokens/s of the captured one-token plan and
the HBM roofline fraction (algorithmic bytes = every layer matrix + lm_head once per token).
    python tools/mllm_bench.py [--layers 40] [--prompt 96] [--new 192] [--sequences S] [--weight-dtype {float16,int8,mxfp4}]
                               [--kv-dtype {float16,fp8}] [--max-positions T]
--sequences S > 1: the batched decode (`generate_batch`, S sequences per weight pass): ms per step, tokens/s over all
sequences, the HBM fraction of a step, and the per-launch time of `llm_gemm16_kernel` at the projection shapes.
--weight-dtype int8: the engine holds int8 projection weights with fp32 row scales (W8A16); the bytes of a step come from
`weight_bytes_per_token()` (1 byte per quantised weight + the scales + the fp16 lm_head), the per-launch shapes run the int8
form of the kernel.
--weight-dtype mxfp4: MXFP4 projection weights (W4A16: 0.5 byte per weight, 1 per 32-element block, 4 per row), priced and
launched the same way on the fp4 forms.
--kv-dtype fp8: the KV cache holds e4m3 codes and one exponent byte per (row, kv head) (`quantize_kv_fp8`); the result carries
`kv_cache_bytes` and `attn_launches`: the per-launch time of the attention op alone, slot form, for 1 and 16 slots at cache
lengths 256 and 1000 (same event-pair method as the projections' table), priced against the K and V bytes the launch reads.
Both modes print the per-launch time of the five projection shapes on the kernel the mode's token step runs (M = 1: the
`llm_gemv` form, M = S: `llm_gemm16`), priced against the bytes of that launch's weights.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffsensei_amd.mllm import LlamaConfig, LlamaDecodeEngine, random_llama_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--prompt", type=int, default=96)
ap.add_argument("--new", type=int, default=192)
ap.add_argument("--graph", choices=["both", "on", "off"], default="both")
ap.add_argument("--gemv-variant", type=int, default=0, help="0 pipelined, 1 one column per wavefront, 2 streaming")
ap.add_argument("--sequences", type=int, default=1, help="sequences per weight pass (1: the one-sequence token loop)")
ap.add_argument("--weight-dtype", choices=["float16", "int8", "mxfp4"], default="float16",
                help="int8 / mxfp4: W8A16 / W4A16 projection weights (lm_head, embedding and norm gains stay fp16)")
ap.add_argument("--kv-dtype", choices=["float16", "fp8"], default="float16", help="fp8: e4m3 KV cache with per-head exponents")
ap.add_argument("--max-positions", type=int, default=0, help="KV cache rows per slot (0: prompt + new + 8)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
from diffsensei_amd import _lib
assert _lib.load().ds_set_option(b"llm_gemv_variant", a.gemv_variant) == 0
cfg = LlamaConfig(num_hidden_layers=a.layers)
t0 = time.perf_counter()
sd = random_llama_state_dict(cfg, dev, 0)
eng = LlamaDecodeEngine(cfg, sd, dev, max_positions=a.max_positions or a.prompt + a.new + 8, max_new_tokens=a.new, poll_every=16,
                        max_sequences=a.sequences, weight_dtype=a.weight_dtype, kv_dtype=a.kv_dtype)
del sd
torch.cuda.synchronize()
init_s = time.perf_counter() - t0
emb = (torch.randn(a.prompt, cfg.hidden_size, device=dev) * 0.5).half()


def launch_times(M):
    """Per-launch times of the five projection shapes at M rows, back to back (event pair around 20 launches after 3 warm-up
    launches), on the kernels of this engine's weight type: llm_gemv at M = 1, llm_gemm16 otherwise."""
    from diffsensei_amd import ops
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    x5, x13 = (torch.randn(M, H, device=dev) * 0.5).half(), (torch.randn(M, I, device=dev) * 0.5).half()
    form = "gemv" if M == 1 else "gemm16"
    suffix = {"float16": "", "int8": "_w8", "mxfp4": "_fp4"}[a.weight_dtype]
    # what comes with the weights of layer 0: nothing (fp16), the row scales (int8), the block exponents and row scales (mxfp4)
    extra = lambda ss, es: () if not ss else ((ss[0],) if not es else (es[0], ss[0]))
    shapes = {"qkv": (x5, eng.wqkv[0], extra(eng.sqkv, eng.eqkv), eng.qkv_dim, dict(rms=True, gain=eng.g_in[0])),
              "o": (x5, eng.wo[0], extra(eng.so, eng.eo), H, {}),
              "gate_up": (x5, eng.wgu[0], extra(eng.sgu, eng.egu), I, dict(rms=True, swiglu=True, gain=eng.g_post[0])),
              "down": (x13, eng.wdown[0], extra(eng.sdown, eng.edown), H, {}), "lm_head": (x5, eng.lm_head, (), V, {})}
    kern = {}
    for name, (x, w, ex, N, kw) in shapes.items():
        fn = getattr(ops, f"llm_{form}{suffix if ex else ''}")
        y = torch.zeros(M, N, dtype=torch.float16, device=dev)
        run = lambda: fn(x, w, *ex, out=y, **kw)
        for _ in range(3):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            run()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 20
        nbytes = sum(float(t.element_size()) * t.numel() for t in (w,) + tuple(ex))
        kern[name] = {"N": N, "K": int(x.shape[1]), "weights": str(w.dtype).replace("torch.", ""), "us": round(us, 2),
                      "GBps": round(nbytes / us / 1e3, 1)}
    return kern


def attn_launch_times():
    """Per-launch time of the attention op alone (slot form, one new row per slot; event pair around 20 launches after 3
    warm-up launches) for 1 and 16 slots at cache lengths 256 and 1000, on caches of this engine's kv dtype.  The cache
    content is random codes / values with mid-range exponents: the time does not depend on it.  GBps prices the K and V rows
    (and exponent bytes) the launch reads, once per kv head."""
    from diffsensei_amd import ops
    D, Hq, Hkv = cfg.head_dim, cfg.num_attention_heads, cfg.kv_heads
    T_max, scale, out = 1024, 1.0 / D ** 0.5, {}
    g = torch.Generator(device=dev).manual_seed(1)
    fr = torch.outer(torch.arange(T_max, dtype=torch.float32), 1.0 / (cfg.rope_theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D)))
    cos, sin = fr.cos().to(dev).contiguous(), fr.sin().to(dev).contiguous()
    for S in (1, 16):
        qkv = (torch.randn(S, (Hq + 2 * Hkv) * D, device=dev, generator=g) * 0.5).half()
        if a.kv_dtype == "fp8":
            kc, vc = (torch.randint(0, 0x78, (S, T_max, Hkv * D), device=dev, generator=g, dtype=torch.uint8) for _ in range(2))
            ke, ve = (torch.full((S, T_max, Hkv), 120, device=dev, dtype=torch.uint8) for _ in range(2))
            run = lambda st: ops.llm_attention_slots_kv8(qkv, kc, vc, ke, ve, cos, sin, st, Hq, Hkv, scale, out=y)
            row_bytes = 2 * Hkv * (D + 1)
        else:
            kc, vc = ((torch.randn(S, T_max, Hkv * D, device=dev, generator=g) * 0.5).half() for _ in range(2))
            run = lambda st: ops.llm_attention_slots(qkv, kc, vc, cos, sin, st, Hq, Hkv, scale, out=y)
            row_bytes = 2 * Hkv * D * 2
        y = torch.zeros(S, Hq * D, dtype=torch.float16, device=dev)
        for n in (256, 1000):
            st = torch.tensor([[n, 1, 0, 0, 9, 2, 0, 0]] * S, dtype=torch.int32, device=dev)      # the launch does not move it
            for _ in range(3):
                run(st)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                run(st)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / 20
            out[f"slots{S}_len{n}"] = {"us": round(us, 2), "GBps": round(S * (n + 1) * row_bytes / us / 1e3, 1)}
    return out


def batched(S):
    embs = [(torch.randn(a.prompt, cfg.hidden_size, device=dev) * 0.5).half() for _ in range(S)]
    rows = []
    for graph in {"both": (True, False), "on": (True,), "off": (False,)}[a.graph]:
        eng.use_graph = graph
        for rep in range(2):                               # rep 0 warms up (and captures)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.generate_batch(embs, [1] * S, -1, a.new)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        assert all(o["ids"].numel() == a.new and torch.isfinite(o["hidden"].float()).all() for o in out)
        rows.append({"graph": graph, "seconds": round(dt, 4), "new_tokens": a.new})
    for rep in range(2):                                   # prompt pass alone (max_new_tokens = 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate_batch(embs, [1] * S, -1, 1)
        torch.cuda.synchronize()
        prompt_ms = round((time.perf_counter() - t0) * 1e3, 2)
    for r in rows:
        r["ms_per_step"] = round((r["seconds"] * 1e3 - prompt_ms) / (a.new - 1), 4)
    best = min(r["ms_per_step"] for r in rows)
    gbs = eng.weight_bytes_per_token() / (best * 1e-3) / 1e9
    kern = launch_times(S)
    print(json.dumps({"workload": f"LLaMA-2-13B dims x {a.layers} layers, {S} sequences greedy, prompt {a.prompt} + {a.new} new tokens",
                      "weight_dtype": a.weight_dtype, "kv_dtype": a.kv_dtype, "kv_cache_bytes": eng.kv_cache_bytes(),
                      "max_positions": eng.T_max, "attn_launches": attn_launch_times(),
                      "init_s": round(init_s, 1), "sequences": S, "runs": rows, "prompt_ms": prompt_ms,
                      "weight_bytes_per_step": eng.weight_bytes_per_token(), "ms_per_step": best,
                      "decode_tokens_per_s": round(S * 1e3 / best, 2),
                      "roofline": {"bound": "hbm", "kernel": "llm_gemm16_kernel", "achieved": round(gbs, 1), "peak": 8000.0,
                                   "unit": "GB/s", "frac": round(gbs / 8000.0, 4),
                                   "note": "whole token step priced against the weight bytes, read once for all sequences"},
                      "ops_per_step": eng.last_run_info["ops_per_token"], f"gemm16_launches_m{S}": kern}))


if a.sequences > 1:
    batched(a.sequences)
    sys.exit(0)
rows = []
for graph in {"both": (True, False), "on": (True,), "off": (False,)}[a.graph]:
    eng.use_graph = graph
    for rep in range(2):                                   # rep 0 warms up (and captures)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.generate(emb, 1, -1, a.new)              # eos -1: never stops early
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    n = int(out["ids"].numel())
    assert n == a.new and torch.isfinite(out["hidden"].float()).all()
    rows.append({"graph": graph, "seconds": round(dt, 4), "new_tokens": n})
prompt_ms = {}
for path in ("mfma", "chunks"):                            # prompt pass alone (max_new_tokens = 1)
    eng.prompt_path = path
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate(emb, 1, -1, 1)
        torch.cuda.synchronize()
        prompt_ms[path] = round((time.perf_counter() - t0) * 1e3, 2)
eng.prompt_path = "mfma"
# token loop alone = whole call - prompt pass; one weight pass per token after the first
for r in rows:
    r["ms_per_token"] = round((r["seconds"] * 1e3 - prompt_ms["mfma"]) / (r["new_tokens"] - 1), 4)
best = min(r["ms_per_token"] for r in rows)
gbs = eng.weight_bytes_per_token() / (best * 1e-3) / 1e9
print(json.dumps({"workload": f"LLaMA-2-13B dims x {a.layers} layers, batch 1 greedy, prompt {a.prompt} + {a.new} new tokens",
                  "weight_dtype": a.weight_dtype, "kv_dtype": a.kv_dtype, "kv_cache_bytes": eng.kv_cache_bytes(),
                  "max_positions": eng.T_max, "attn_launches": attn_launch_times(), "ms_per_token": best,
                  "init_s": round(init_s, 1), "runs": rows, "prompt_ms": prompt_ms,
                  "weight_bytes_per_token": eng.weight_bytes_per_token(), "decode_tokens_per_s": round(1e3 / best, 2),
                  "roofline": {"bound": "hbm", "kernel": "llm_gemv_pipe_kernel", "achieved": round(gbs, 1), "peak": 8000.0,
                               "unit": "GB/s", "frac": round(gbs / 8000.0, 4),
                               "note": "whole token step (204 launches) priced against the weight bytes"},
                  "ops_per_token": eng.last_run_info["ops_per_token"], "gemv_variant": a.gemv_variant,
                  "gemv_launches_m1": launch_times(1)}))
