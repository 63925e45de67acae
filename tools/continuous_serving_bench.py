#!/usr/bin/env python3
"""Bucketed vs continuous batching on a mixed-step queue (profiles/continuous_serving.txt).

    python tools/continuous_serving_bench.py [--requests 48] [--max-panels 16] [--size 1024] [--steps 20,30,50]

SDXL-size seeded weights and 1024 x 1024 panels, as bench.py builds them.  The queue holds `--requests` single-panel
requests whose step counts cycle through `--steps`.  Case (a) is `BucketBatcher(max_panels=N)` as it is: one static UNet
batch per step count.  Case (b) is the same queue with `continuous=True`: N panel slots, each with its own schedule,
refilled as panels finish.  Both cases are run once to warm up (launch plans, hipGraph capture) and once timed; the
forward counts and idle slot steps are derived on the host (`serving.plan_continuous`).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=48)
    ap.add_argument("--max-panels", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", default="20,30,50")
    ap.add_argument("--output", choices=("pil", "latent"), default="pil")
    args = ap.parse_args()
    import bench
    from diffsensei_amd.serving import BucketBatcher, plan_batches, plan_continuous
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    pipe, _ = bench.build_pipeline(dev, 1, 0)
    cycle = [int(s) for s in args.steps.split(",")]
    steps = [cycle[i % len(cycle)] for i in range(args.requests)]

    def queue():
        reqs = []
        for i, n in enumerate(steps):
            r = bench.synthetic_request(dev, args.size, 100 + i)
            r.pop("output_type")
            r["num_inference_steps"] = n
            reqs.append(r)
        return reqs

    def run(continuous):
        b = BucketBatcher(pipe, max_panels=args.max_panels, continuous=continuous)
        for r in queue():
            b.submit(**r)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = b.run(output_type=args.output)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(out) == args.requests and all(o is not None for o in out)
        return dt, b

    result = {"requests": args.requests, "steps": cycle, "max_panels": args.max_panels, "size": args.size, "output": args.output}
    for name, continuous in (("bucketed", False), ("continuous", True)):
        run(continuous)                                            # warm-up: plans, graph capture, allocator
        dt, b = run(continuous)
        if continuous:
            plan = plan_continuous(steps, [1] * args.requests, b.last_slots[0])
            counts = {"forwards": plan["forwards"], "unet_batch": 2 * b.last_slots[0], "idle_slot_steps": plan["idle_slot_steps"],
                      "runs": len(b.last_plan)}
        else:
            batches = plan_batches(queue(), args.max_panels, b.max_pixels)
            fw = sum(steps[bt[0]] for bt in batches)
            counts = {"forwards": fw, "unet_batch": [2 * len(bt) for bt in batches],
                      "idle_slot_steps": sum(steps[bt[0]] * (args.max_panels - len(bt)) for bt in batches), "runs": len(batches)}
        result[name] = dict(wall_s=round(dt, 3), panels_per_s=round(args.requests / dt, 4), **counts)
        print(f"{name}: {result[name]}", file=sys.stderr, flush=True)
    result["speedup"] = round(result["bucketed"]["wall_s"] / result["continuous"]["wall_s"], 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
