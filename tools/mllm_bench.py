#!/usr/bin/env python
"""MLLM pre-pass decode rate at LLaMA-2-13B dimensions (random weights): tokens/s of the captured one-token plan and
the HBM roofline fraction (algorithmic bytes = every layer matrix + lm_head once per token).
    python tools/mllm_bench.py [--layers 40] [--prompt 96] [--new 192] [--sequences S] [--weight-dtype {float16,int8}]
--sequences S > 1: the batched decode (`generate_batch`, S sequences per weight pass): ms per step, tokens/s over all
sequences, the HBM fraction of a step, and the per-launch time of `llm_gemm16_kernel` at the projection shapes.
--weight-dtype int8: the engine holds int8 projection weights with fp32 row scales (W8A16); the bytes of a step come from
`weight_bytes_per_token()` (1 byte per quantised weight + the scales + the fp16 lm_head), the per-launch shapes run the int8
form of the kernel.
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
ap.add_argument("--weight-dtype", choices=["float16", "int8"], default="float16",
                help="int8: W8A16 projection weights (lm_head, embedding and norm gains stay fp16)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
from diffsensei_amd import _lib
assert _lib.load().ds_set_option(b"llm_gemv_variant", a.gemv_variant) == 0
cfg = LlamaConfig(num_hidden_layers=a.layers)
t0 = time.perf_counter()
sd = random_llama_state_dict(cfg, dev, 0)
eng = LlamaDecodeEngine(cfg, sd, dev, max_positions=a.prompt + a.new + 8, max_new_tokens=a.new, poll_every=16,
                        max_sequences=a.sequences, weight_dtype=a.weight_dtype)
del sd
torch.cuda.synchronize()
init_s = time.perf_counter() - t0
emb = (torch.randn(a.prompt, cfg.hidden_size, device=dev) * 0.5).half()


def batched(S):
    from diffsensei_amd import ops
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
    # per-launch times of the new kernel, M = 16, back to back (event pair around 20 launches after 3 warm-up launches)
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    x5, x13 = (torch.randn(16, H, device=dev) * 0.5).half(), (torch.randn(16, I, device=dev) * 0.5).half()
    y = torch.zeros(16, max(eng.qkv_dim, I, V), dtype=torch.float16, device=dev)
    w8 = a.weight_dtype == "int8"
    sc = lambda ss: ss[0] if w8 else None                  # row scales of layer 0 (int8), None: the fp16 kernel
    shapes = {"qkv": (x5, eng.wqkv[0], sc(eng.sqkv), eng.qkv_dim, dict(rms=True, gain=eng.g_in[0])),
              "o": (x5, eng.wo[0], sc(eng.so), H, {}),
              "gate_up": (x5, eng.wgu[0], sc(eng.sgu), I, dict(rms=True, swiglu=True, gain=eng.g_post[0])),
              "down": (x13, eng.wdown[0], sc(eng.sdown), H, {}), "lm_head": (x5, eng.lm_head, None, V, {})}
    kern = {}
    for name, (x, w, s, N, kw) in shapes.items():
        run = (lambda: ops.llm_gemm16(x, w, out=y, N=N, **kw)) if s is None else \
              (lambda: ops.llm_gemm16_w8(x, w, s, out=y, N=N, **kw))
        for _ in range(3):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            run()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 20
        kern[name] = {"N": N, "K": int(x.shape[1]), "weights": str(w.dtype).replace("torch.", ""), "us": round(us, 2),
                      "GBps": round(float(w.element_size()) * w.numel() / us / 1e3, 1)}
    print(json.dumps({"workload": f"LLaMA-2-13B dims x {a.layers} layers, {S} sequences greedy, prompt {a.prompt} + {a.new} new tokens",
                      "weight_dtype": a.weight_dtype,
                      "init_s": round(init_s, 1), "sequences": S, "runs": rows, "prompt_ms": prompt_ms,
                      "weight_bytes_per_step": eng.weight_bytes_per_token(), "ms_per_step": best,
                      "decode_tokens_per_s": round(S * 1e3 / best, 2),
                      "roofline": {"bound": "hbm", "kernel": "llm_gemm16_kernel", "achieved": round(gbs, 1), "peak": 8000.0,
                                   "unit": "GB/s", "frac": round(gbs / 8000.0, 4),
                                   "note": "whole token step priced against the weight bytes, read once for all sequences"},
                      "ops_per_step": eng.last_run_info["ops_per_token"], "gemm16_launches_m16": kern}))


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
                  "weight_dtype": a.weight_dtype, "ms_per_token": best,
                  "init_s": round(init_s, 1), "runs": rows, "prompt_ms": prompt_ms,
                  "weight_bytes_per_token": eng.weight_bytes_per_token(), "decode_tokens_per_s": round(1e3 / best, 2),
                  "roofline": {"bound": "hbm", "kernel": "llm_gemv_pipe_kernel", "achieved": round(gbs, 1), "peak": 8000.0,
                               "unit": "GB/s", "frac": round(gbs / 8000.0, 4),
                               "note": "whole token step (204 launches) priced against the weight bytes"},
                  "ops_per_token": eng.last_run_info["ops_per_token"], "gemv_variant": a.gemv_variant}))
