"""What few-step sampling buys at SDXL dimensions: one batch-1 1024 x 1024 call at 50 Euler steps (guidance 5) against the same
call with `LCMScheduler` at 4 and 8 steps (guidance 1, a rank-64 adapter merged on every target), and the UNet-forward time
per step with and without the adapter merged.

    python tools/few_step_bench.py [--out profiles/lcm_few_step.txt] [--size 1024] [--rank 64] [--calls 3]

Random weights and a random adapter (no distilled adapter exists for this UNet): the TIMES are those
of a trained adapter, the pictures are not - what a 4-step picture of a trained distillation looks like is not measured here.
One process; every configuration is warmed up once (engine build, graph capture, merge plan) and then timed `calls` times with
a host clock around a call that ends in a device synchronise; the figure is the median.  A call is the whole
`pipe(...)`: prompt and image encoders, sampling loop, VAE decode.  The forward time is the engine's forward plan alone
(eager, synchronised, median of 10): a merged adapter changes weight values, not the plan, so it must not change.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the flagship workload's pipeline and request, synthetic weights)
from diffsensei_amd.lora import all_target_modules  # noqa: E402
from diffsensei_amd.schedulers import EulerDiscreteScheduler, LCMScheduler  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    pipe, _ = bench.build_pipeline(dev, 1, 0)
    cfg = pipe.unet.config
    req = bench.synthetic_request(dev, a.size, 0, output_type="pt")
    req["num_samples"] = 1
    g = torch.Generator(device=dev).manual_seed(1)
    lora = {}
    for m, shp in all_target_modules(cfg).items():
        lora[m + ".lora_A.weight"] = (torch.randn(a.rank, *shp[1:], generator=g, device=dev) * 0.01).half()
        lora[m + ".lora_B.weight"] = (torch.randn(shp[0], a.rank, generator=g, device=dev) * 0.01).half()

    def call(steps, guidance):
        r = dict(req, num_inference_steps=steps, guidance_scale=guidance, generator=torch.Generator().manual_seed(0))
        out = pipe(**r).images
        assert torch.isfinite(out).all()
        return out

    def timed(steps, guidance):
        call(steps, guidance)                                         # warm-up of this configuration
        ts = sorted(wall(lambda: call(steps, guidance))[0] for _ in range(a.calls))
        return ts[len(ts) // 2], ts[0], ts[-1]

    def forward_ms(batch):
        H = a.size // 8
        eng = pipe.unet.engine(batch, H, H, 1.0)
        ts = sorted(wall(lambda: eng.forward_plan.run())[0] * 1e3 for _ in range(10))
        return ts[5]

    say(f"# Few-step sampling at SDXL dimensions, random weights: one panel at {a.size} x {a.size}, whole pipe(...) call, "
        f"median (min .. max) of {a.calls} after one warm-up call")
    e = timed(50, 5.0)
    say(f"EulerDiscreteScheduler, 50 steps, guidance 5 (UNet batch 2):            {e[0]:7.3f} s ({e[1]:.3f} .. {e[2]:.3f})")
    fwd2_base, fwd1_base = forward_ms(2), None
    pipe.scheduler = LCMScheduler.from_config(pipe.scheduler.config)
    pipe.load_lora_weights(lora, adapter_name="distill")
    t_first, _ = wall(lambda: pipe.set_adapters(["distill"], [1.0]))
    rows = {}
    for steps in (4, 8):
        rows[steps] = timed(steps, 1.0)
        say(f"LCMScheduler, {steps} steps, guidance 1 (UNet batch 1), rank-{a.rank} adapter merged:  {rows[steps][0]:7.3f} s "
            f"({rows[steps][1]:.3f} .. {rows[steps][2]:.3f}) = {e[0] / rows[steps][0]:.1f} x fewer seconds than 50 Euler steps")
    fwd1_on = forward_ms(1)
    pipe.scheduler = EulerDiscreteScheduler.from_config(pipe.scheduler.config)
    call(2, 5.0)                      # the batch-2 engine was dropped when the adapter was loaded: a real request sets it up again
    fwd2_on = forward_ms(2)
    t_off, _ = wall(lambda: pipe.set_adapters([]))
    fwd1_base, fwd2_off = forward_ms(1), forward_ms(2)
    say(f"UNet forward per step, eager plan, median of 10: batch 1 adapter merged {fwd1_on:.2f} ms / none {fwd1_base:.2f} ms; "
        f"batch 2 adapter merged {fwd2_on:.2f} ms / none {fwd2_off:.2f} ms (before the adapter was loaded: {fwd2_base:.2f} ms)")
    say(f"set_adapters: first time (builds and captures the merge plan) {t_first * 1e3:.1f} ms, back to none {t_off * 1e3:.1f} ms")
    fixed = rows[4][0] - 4 * fwd1_on / 1e3
    say(f"of the 4-step call, {4 * fwd1_on / 1e3:.3f} s are UNet forwards and {fixed:.3f} s everything else (encoders, VAE decode, host)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
