#!/usr/bin/env python
"""Same-box A/B of the two samplers on one pipeline, alternating Euler (50 and 25 steps) and DPM-Solver++ 2M Karras
(25 steps):
  * ms_per_step: device time between the step-1 and the last step's end (CUDA events recorded from
    `callback_on_step_end`, so the plan rebuild, graph capture and eager first step of a swap are excluded); compare
    dpm25 with euler25, calls of the same length;
  * wall: one whole `__call__` (the second of two back-to-back calls with the same scheduler, so no rebuild is timed).
    python tools/dpm_vs_euler.py --num-samples 1 --refs 1 --output-type pil      # BASELINE configs[1] shape
    python tools/dpm_vs_euler.py --num-samples 32 --output-type latent          # UNet batch 64 at 1024^2
    python tools/dpm_vs_euler.py --kernel-only {euler,dpm}                       # sampler_step_kernel alone (rocprofv3)
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def kernel_only(which: str, reps: int) -> dict:
    """`reps` launches of sampler_step_kernel at the UNet batch-64 latent shape (ns 32, 128 x 128, CFG), kind 0 or 2."""
    from diffsensei_amd import ops
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    dev = torch.device("cuda", 0)
    ns, H, W = 32, 128, 128
    eps = (torch.randn(2 * ns, H * W, 4, device=dev) * 0.5).half()
    lat = torch.randn(ns, 4, H, W, device=dev).half()
    xin = torch.empty_like(eps)
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    if which == "dpm":
        sch = DPMSolverMultistepScheduler.from_config(EulerDiscreteScheduler().config, use_karras_sigmas=True)
        sch.set_timesteps(25)
        table = torch.from_numpy(sch.coef_table(7.5)).to(dev)
        solver = torch.from_numpy(sch.solver_table()).to(dev)
        prev = torch.zeros_like(lat)
        ctr.fill_(10)                                      # a second-order row
        step = lambda: ops.cfg_dpm_step(eps, lat, xin, table, solver, prev, True, ctr)
    else:
        sch = EulerDiscreteScheduler()
        sch.set_timesteps(50)
        table = torch.from_numpy(sch.coef_table(7.5)).to(dev)
        ctr.fill_(10)
        step = lambda: ops.cfg_sampler_step(eps, lat, xin, table, sch.kind, True, ctr)
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    return {"kernel": which, "launches": reps, "host_us_per_launch": round((time.perf_counter() - t0) / reps * 1e6, 2),
            "bytes_per_launch": (2 * ns * H * W * 4 + ns * 4 * H * W * 2 + 2 * ns * H * W * 4
                                 + (ns * 4 * H * W * 2 if which == "dpm" else 0)) * 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-samples", type=int, default=1)
    ap.add_argument("--refs", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--output-type", default="pil")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-only", choices=("euler", "dpm"))
    args = ap.parse_args()
    if args.kernel_only:
        print(json.dumps(kernel_only(args.kernel_only, 200)), flush=True)
        return
    import bench
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    dev = torch.device("cuda", 0)
    pipe, _ = bench.build_pipeline(dev, 1, 0, with_vae=args.output_type != "latent")
    euler = EulerDiscreteScheduler()
    dpm = DPMSolverMultistepScheduler.from_config(euler.config, use_karras_sigmas=True)
    arms = {"euler50": (euler, 50), "dpm25": (dpm, 25), "euler25": (euler, 25)}

    def call(name):
        sch, steps = arms[name]
        pipe.scheduler = sch
        req = bench.synthetic_request(dev, args.size, seed=1234, output_type=args.output_type, refs=args.refs)
        req["num_inference_steps"] = steps
        evs = []

        def cb(p, i, t, kw):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            evs.append(ev)
            return kw

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(num_samples=args.num_samples, callback_on_step_end=cb, **req)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return wall, evs[1].elapsed_time(evs[-1]) / (len(evs) - 2)

    res = {k: {"ms_per_step": [], "wall_s": []} for k in arms}
    for name in arms:                                    # warm-up: plans, graph capture, lazy kernel state
        call(name)
    for r in range(args.reps):
        order = list(arms) if r % 2 == 0 else list(arms)[::-1]
        for name in order:
            _, ms1 = call(name)                          # first call after the swap: rebuild + capture not in ms_per_step
            wall, ms2 = call(name)
            res[name]["ms_per_step"] += [round(ms1, 3), round(ms2, 3)]
            res[name]["wall_s"].append(round(wall, 4))
    out = {"num_samples": args.num_samples, "unet_batch": 2 * args.num_samples, "size": args.size, "refs": args.refs,
           "output_type": args.output_type, "arms": res}
    for k, v in res.items():
        ms = v["ms_per_step"]
        v["ms_per_step_median"] = sorted(ms)[len(ms) // 2]
        v["ms_per_step_spread"] = round(max(ms) - min(ms), 3)
        v["wall_s_median"] = sorted(v["wall_s"])[len(v["wall_s"]) // 2]
    out["dpm25_over_euler50_wall"] = round(res["dpm25"]["wall_s_median"] / res["euler50"]["wall_s_median"], 4)
    out["ms_per_step_diff_dpm25_minus_euler25"] = round(res["dpm25"]["ms_per_step_median"]
                                                        - res["euler25"]["ms_per_step_median"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
