"""What a longer text context costs at SDXL dimensions (random weights): the attn2 op, the whole UNet forward and the prepare plan
for 77 text tokens (ip_attn_kernel) against 154 / 231 / 308 (ip_attn_long_kernel: 2 / 3 / 4 panels of 96 keys).

    python tools/long_prompt_bench.py [--out profiles/long_prompt.txt] [--rounds 5] [--reps 20]

1. The op alone at (B 64, heads 10, N 4096) and (B 64, heads 20, N 1024), the two cross-attention shapes of a 1024 x 1024 UNet
   batch of 64: `reps` launches between two device events, `rounds` rounds with the four text lengths interleaved, median per
   launch (min .. max over the rounds).  Boxes as under classifier-free guidance: the first half of the batch has none (those
   rows attend the dummy keys only), the second half three.  Beside each long time stands the yardstick: the 77-token time of
   the same run times (T + 1) / 2 - the text side's work scaled by its panels, the image side fixed.  No threshold is set on it.
2. The engine's forward plan (eager, between device events, median of `rounds`) at 128 x 128 latents for UNet batch 2 and 64 with
   1, 2 and 3 chunks of 77 tokens, and its prepare plan (pad, K / V^T projections of every layer, added-condition MLP).
One process; every configuration is warmed up before it is timed.  Nothing is profiled here: times are launch-to-completion."""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the flagship workload's pipeline, synthetic weights)
from diffsensei_amd import ops  # noqa: E402

LP = 96


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def op_case(B, heads, hw, Lt, dev, g):
    N, Cc, T = hw[0] * hw[1], heads * 64, (Lt + LP - 1) // LP
    r = lambda *s: torch.randn(*s, generator=g, device=dev).half()
    q, kt, vtt, ki, vti = r(B, N, Cc), r(B, LP * T, Cc), r(B, Cc, LP * T), r(B, LP, Cc), r(B, Cc, LP)
    kt[:, Lt:], vtt[:, :, Lt:], ki[:, 80:], vti[:, :, 80:] = 0, 0, 0, 0
    bbox = torch.zeros(B, 4, 4, device=dev)
    bbox[B // 2:, 0] = torch.tensor([0.05, 0.10, 0.50, 0.95], device=dev)
    bbox[B // 2:, 1] = torch.tensor([0.50, 0.10, 0.95, 0.95], device=dev)
    bbox[B // 2:, 2] = torch.tensor([0.30, 0.30, 0.70, 0.60], device=dev)
    out = torch.empty_like(q)
    return lambda: ops.masked_ip_attention(q, kt, vtt, ki, vti, bbox, heads, hw, 0.6, Lt=Lt, out=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="2,64")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=dev).manual_seed(0)
    lengths = (77, 154, 231, 308)
    say(f"# attn2 op alone, us per launch: median (min .. max) of {a.rounds} rounds of {a.reps} launches, text lengths interleaved")
    for B, heads, hw in ((64, 10, (64, 64)), (64, 20, (32, 32))):
        fns = {Lt: op_case(B, heads, hw, Lt, dev, g) for Lt in lengths}
        for fn in fns.values():
            events_ms(fn, 3)
        times = {Lt: [] for Lt in lengths}
        for _ in range(a.rounds):
            for Lt in lengths:
                times[Lt].append(events_ms(fns[Lt], a.reps) * 1e3)
        base = med(times[77])[0]
        for Lt in lengths:
            m, lo, hi = med(times[Lt])
            T = (Lt + LP - 1) // LP
            tail = "ip_attn_kernel" if Lt == 77 else (f"ip_attn_long_kernel, T = {T}; yardstick 77-token time x (T + 1) / 2 = "
                                                      f"{base * (T + 1) / 2:8.1f} us, measured / yardstick = {m / (base * (T + 1) / 2):.2f}")
            say(f"B {B} heads {heads:2d} N {hw[0] * hw[1]:4d} Lt {Lt:3d}: {m:8.1f} us ({lo:.1f} .. {hi:.1f})   {tail}")
        del fns
        torch.cuda.empty_cache()

    pipe, _ = bench.build_pipeline(dev, 1, 0)
    cfg = pipe.unet.config
    H = W = 128
    say(f"# UNet forward plan and prepare plan at {H} x {W} latents (1024 x 1024), eager, ms: median (min .. max) of {a.rounds}")
    for B in (int(v) for v in a.batches.split(",")):
        for chunks in (1, 2, 3):
            n_txt = 77 * chunks
            eng = pipe.unet.engine(B, H, W, 1.0, text_tokens=n_txt)
            r = lambda *s: torch.randn(*s, generator=g, device=dev).half()
            bbox = torch.zeros(B, cfg.max_num_ips, 4, device=dev)
            bbox[B // 2:, 0] = torch.tensor([0.05, 0.10, 0.50, 0.95], device=dev)
            bbox[B // 2:, 1] = torch.tensor([0.50, 0.10, 0.95, 0.95], device=dev)
            tid = torch.tensor([[1024, 1024, 0, 0, 1024, 1024]] * B, dtype=torch.float16, device=dev)
            eng.set_request(r(B, n_txt + cfg.num_ip_tokens, cfg.cross_attention_dim), r(*eng.text_embeds.shape), tid, bbox, None, 0.6)
            eng.x_in.copy_(r(*eng.x_in.shape))
            for _ in range(2):
                eng.forward_plan.run()
            torch.cuda.synchronize()
            assert torch.isfinite(eng.eps).all()
            fwd = med([events_ms(eng.forward_plan.run, 1) for _ in range(a.rounds)])
            prep = med([events_ms(eng.prepare_plan.run, 1) for _ in range(a.rounds)])
            kv = 2 * eng.k_txt.numel() * 2 / 2 ** 20
            say(f"UNet batch {B:2d}, {chunks} chunk(s) = {n_txt:3d} text tokens: forward {fwd[0]:8.2f} ms ({fwd[1]:.2f} .. {fwd[2]:.2f})   "
                f"prepare {prep[0]:7.3f} ms ({prep[1]:.3f} .. {prep[2]:.3f})   text K + V^T panels {kv:7.1f} MiB")
            del eng
            pipe.unet._engines.clear()
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
