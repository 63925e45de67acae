#!/usr/bin/env python
"""One pipeline call of a few steps under Euler or Euler Ancestral at the benchmark shape, for a kernel trace of
`sampler_step_kernel` kind 0 against kind 3 (the Philox + Box-Muller draw) on the same box:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o euler   -- python tools/euler_a_vs_euler.py --sampler euler
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o euler_a -- python tools/euler_a_vs_euler.py --sampler euler_a
Eager launches (no hipGraph), latents out (no VAE), synthetic weights.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampler", choices=("euler", "euler_a"), required=True)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--num-samples", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    import bench
    from diffsensei_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    dev = torch.device("cuda", 0)
    pipe, _ = bench.build_pipeline(dev, 1, 0, with_vae=False)
    pipe.use_graph = False
    if args.sampler == "euler_a":
        pipe.scheduler = EulerAncestralDiscreteScheduler.from_config(EulerDiscreteScheduler().config)
    else:
        pipe.scheduler = EulerDiscreteScheduler()
    req = bench.synthetic_request(dev, args.size, seed=1234, output_type="latent", refs=2)
    req["num_inference_steps"] = args.steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pipe(num_samples=args.num_samples, **req).images
    torch.cuda.synchronize()
    print(json.dumps({"sampler": args.sampler, "kind": pipe.scheduler.kind, "steps": args.steps,
                      "num_samples": args.num_samples, "size": args.size, "wall_s": round(time.perf_counter() - t0, 3),
                      "finite": bool(torch.isfinite(out).all()), "noise_seeds": pipe.last_run_info["noise_seeds"]}),
          flush=True)


if __name__ == "__main__":
    main()
