#!/usr/bin/env python3
"""Everything the device ever sees from `LCMScheduler`, CPU only: timesteps, coef_table, solver_table and renoise_table at
a fixed list of step counts, for the default config and for one with other distillation keys.

    python tools/dump_lcm_tables.py [-o tests/golden/lcm_tables.npz]

tests/test_lcm_scheduler.py regenerates the arrays from the working tree and wants every one equal bit for bit, so a
change of schedulers.py that moves one bit of an LCM table fails there.  Regenerate the file only for a change that is
meant to move a table.  The matrix of the other four samplers (tools/dump_scheduler_tables.py) is not touched.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

STEPS = (1, 2, 3, 4, 8, 50)
CONFIGS = {"default": {}, "orig100_scale5": dict(original_inference_steps=100, timestep_scaling=5.0)}
GUIDANCE = 1.5


def dump() -> dict:
    from diffsensei_amd.schedulers import LCMScheduler
    out = {}
    for name, kw in CONFIGS.items():
        for n in STEPS:
            s = LCMScheduler(**kw)
            s.set_timesteps(n)
            key = f"{name}/n{n}/"
            out[key + "timesteps"] = np.asarray(s.timesteps_np)
            out[key + "coef"] = s.coef_table(GUIDANCE)
            out[key + "solver"] = s.solver_table()
            out[key + "renoise"] = s.renoise_table()
    return out


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(root, "tests", "golden", "lcm_tables.npz"))
    args = ap.parse_args()
    arrays = dump()
    np.savez_compressed(args.out, **arrays)
    print(f"{len(arrays)} arrays -> {args.out} ({os.path.getsize(args.out)} bytes)")
