#!/usr/bin/env python
"""Chain fast-forward of the MLLM pre-pass at LLaMA-2-13B dimensions (random weights, 64 image tokens): the whole decode and
the whole pre-pass with the mode off and on, interleaved in one process, `--rounds` rounds.
    python tools/mllm_chain_ff_bench.py [--sequences S] [--weight-dtype {float16,mxfp4}] [--kv-dtype {float16,fp8}] [--rounds 2]
                                        [--layers 40] [--new 120]
Every sequence is a prompt of 96 rows ending in <img> ([bos, 25 text, <img>, 64 placeholders, </img>, 3 text, <img>]), so the
prompt's pick makes <img_00000> and 64 forced ids follow; max_new 120, no eos.  One engine: the mode is its
`chain_fast_forward` attribute (the plan cache is keyed by it), flipped between runs.  Per run: ms of the decode
(`generate` / `generate_batch` on prepared embeddings) and of the pre-pass (`ContinuousLVLM.generate[_batch]`: input resampler,
decode, output resampler); with the mode on also the fast-forward pass (event pair around it), the attention launches inside
it (event pairs around `ops.llm_attention_rows`), the token steps launched and how many of them no sequence needed.
Prints one JSON line per run and a summary line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffsensei_amd import ops
from diffsensei_amd.mllm import (ContinuousLVLM, LlamaConfig, LlamaDecodeEngine, QwenResampler, random_llama_state_dict,
                                 random_qwen_resampler_state_dict)

ap = argparse.ArgumentParser()
ap.add_argument("--sequences", type=int, default=1)
ap.add_argument("--weight-dtype", choices=["float16", "int8", "mxfp4"], default="float16")
ap.add_argument("--kv-dtype", choices=["float16", "fp8"], default="float16")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--new", type=int, default=120)
a = ap.parse_args()
dev = torch.device("cuda", 0)
S, N_IMG, BOI = a.sequences, 64, 32100
chain = [BOI] + [BOI + 1 + i for i in range(N_IMG)] + [BOI + 1 + N_IMG]
cfg = LlamaConfig(num_hidden_layers=a.layers)
llm = LlamaDecodeEngine(cfg, random_llama_state_dict(cfg, dev, 7), dev, max_positions=256, max_new_tokens=128,
                        max_sequences=S, weight_dtype=a.weight_dtype, kv_dtype=a.kv_dtype, chain_fast_forward=True)
agent = ContinuousLVLM(llm, QwenResampler(random_qwen_resampler_state_dict(8, cfg.hidden_size, 2048, dev, 8), 32, dev),
                       QwenResampler(random_qwen_resampler_state_dict(8, 2048, cfg.hidden_size, dev, 9), 32, dev))
llm.set_image_token_chain(chain)


def request(seed):
    g = torch.Generator().manual_seed(seed)
    text = lambda n: torch.randint(3, 32000, (n,), generator=g).tolist()
    ids = [1] + text(25) + chain + text(3) + [BOI]
    mask = torch.zeros(len(ids), dtype=torch.bool)
    mask[27:27 + N_IMG] = True
    assert len(ids) == 96
    return dict(input_ids=torch.tensor(ids)[None], ids_cmp_mask=mask[None], num_img_gen_tokens=N_IMG, max_new_tokens=a.new,
                image_embeds=torch.randn(1, N_IMG, 2048, generator=g).half().to(dev), img_ids_list=chain, eos_token_id=-1)


reqs = [request(100 + s) for s in range(S)]
embs = []
for r in reqs:
    e = llm.embed_tokens(r["input_ids"].view(-1))
    e[r["ids_cmp_mask"].view(-1).to(dev)] = agent.input_resampler(r["image_embeds"]).reshape(-1, e.shape[-1])
    embs.append(e)

# event pairs around the pass and around the attention launches inside it
marks = {"pass": [], "attn": []}


def timed(kind, fn):
    def wrapped(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*args, **kw)
        e1.record()
        marks[kind].append((e0, e1))
        return out
    return wrapped


llm._fast_forward = timed("pass", llm._fast_forward)
ops.llm_attention_rows = timed("attn", ops.llm_attention_rows)


def run(mode, what):
    llm.chain_fast_forward = mode
    for k in marks:
        marks[k].clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if what == "decode":
        if S == 1:
            out = [llm.generate(embs[0], BOI, -1, a.new)]
        else:
            out = llm.generate_batch(embs, [BOI] * S, -1, a.new)
        n_ids = [len(o["ids"]) for o in out]
    else:
        out = agent.generate(**reqs[0]) if S == 1 else agent.generate_batch(reqs)
        n_ids = [len(o["output_ids"]) for o in ([out] if S == 1 else out)]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    info = llm.last_run_info
    rows = info["fast_forward_rows"]
    rows = [rows] if S == 1 else rows
    # with a pass a sequence needs new - 1 - rows token steps; whatever was launched beyond the largest need fed no sequence
    wasted = info["token_steps_launched"] - max(n - 1 - r for n, r in zip(n_ids, rows))
    rec = {"sequences": S, "weight_dtype": a.weight_dtype, "kv_dtype": a.kv_dtype, "mode": "on" if mode else "off", "what": what,
           "ms": round(ms, 2), "new_tokens": n_ids[0], "token_steps_launched": info["token_steps_launched"], "wasted_steps": wasted,
           "fast_forward_rows": rows[0], "fast_forward_passes": info["fast_forward_passes"]}
    if mode:
        el = lambda k: sum(e0.elapsed_time(e1) for e0, e1 in marks[k])
        # the pass's event pair ends behind its last launch; its host work (the state and id copies) is inside it
        rec.update(pass_ms=round(el("pass"), 2), pass_attention_ms=round(el("attn"), 2),
                   pass_gemm_and_rest_ms=round(el("pass") - el("attn"), 2), attention_launches=len(marks["attn"]))
    print(json.dumps(rec), flush=True)
    return rec


for mode in (False, True):                                   # warm-up: plans, graph capture, the dequantised scratch
    run(mode, "decode")
recs = [run(mode, what) for _ in range(a.rounds) for what in ("decode", "prepass") for mode in (False, True)]
summary = {"sequences": S, "weight_dtype": a.weight_dtype, "kv_dtype": a.kv_dtype}
for what in ("decode", "prepass"):
    off = [r["ms"] for r in recs if r["what"] == what and r["mode"] == "off"]
    on = [r["ms"] for r in recs if r["what"] == what and r["mode"] == "on"]
    spread = max(max(off) - min(off), max(on) - min(on))
    summary[what] = {"off_ms": off, "on_ms": on, "gain_ms": round(min(off) - max(on), 2), "larger_spread_ms": round(spread, 2),
                     "shorter_by_more_than_3_spreads": bool(min(off) - max(on) > 3 * spread)}
steps_off = [r for r in recs if r["what"] == "decode" and r["mode"] == "off"]
summary["default_ms_per_token_step_incl_prompt"] = [round(r["ms"] / r["token_steps_launched"], 3) for r in steps_off]
print(json.dumps({"summary": summary}), flush=True)
