#!/usr/bin/env python3
"""Characterisation of diffsensei_amd/schedulers.py, CPU only: for a fixed matrix of configs, everything the device ever
sees from a scheduler (timesteps, sigmas, init_noise_sigma, coef_table, solver_table, step_orders) and what every
refused / swapped construction does (ok + the resulting `.config`, or the exception's name).

    python tools/dump_scheduler_tables.py [--root CHECKOUT] [-o tests/golden/scheduler_tables.npz]

`--root` is the checkout whose `diffsensei_amd` is dumped (default: this one).  tests/golden/scheduler_tables.npz is the
dump of the commit BEFORE the schedulers were put on one base class; tests/test_scheduler_tables_golden.py regenerates
the matrix from the working tree and wants every array and every outcome equal, so a change of schedulers.py that moves
one bit of a table fails there.  Regenerate the file only for a change that is meant to move a table.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys

import numpy as np

STEPS = (1, 2, 3, 14, 15, 50)
SPACINGS = ("leading", "linspace", "trailing")
SDXL = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
            timestep_spacing="leading")
CLASSES = ("EulerDiscreteScheduler", "DDIMScheduler", "DPMSolverMultistepScheduler", "EulerAncestralDiscreteScheduler")

# the REFUSED lists of tests/test_dpm_scheduler.py and tests/test_euler_ancestral_scheduler.py (the golden test checks
# that they still are) and the loop of test_capi_and_host.py::test_scheduler_config_keys_that_change_the_schedule_are_refused
DPM_REFUSED = [("algorithm_type", "dpmsolver"), ("algorithm_type", "sde-dpmsolver++"), ("algorithm_type", "sde-dpmsolver"),
               ("solver_order", 3), ("thresholding", True), ("use_lu_lambdas", True), ("use_exponential_sigmas", True),
               ("use_beta_sigmas", True), ("use_flow_sigmas", True), ("variance_type", "learned_range"),
               ("lambda_min_clipped", -5.1), ("rescale_betas_zero_snr", True), ("trained_betas", [0.1, 0.2]),
               ("prediction_type", "v_prediction"), ("prediction_type", "sample"), ("beta_schedule", "linear"),
               ("solver_type", "bh2"), ("final_sigmas_type", "denoise_to_zero"), ("timestep_spacing", "karras")]
EULER_A_REFUSED = [("trained_betas", [0.1, 0.2]), ("prediction_type", "v_prediction"), ("prediction_type", "sample"),
                   ("rescale_betas_zero_snr", True), ("beta_schedule", "linear"), ("beta_schedule", "squaredcos_cap_v2"),
                   ("timestep_spacing", "karras")]
EULER_DDIM_OK = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                     steps_offset=1, timestep_spacing="leading", prediction_type="epsilon", interpolation_type="linear",
                     use_karras_sigmas=False, trained_betas=None, clip_sample=False, set_alpha_to_one=False,
                     skip_prk_steps=True, sample_max_value=1.0, rescale_betas_zero_snr=False, final_sigmas_type="zero",
                     timestep_type="discrete")
EULER_DDIM_REFUSED = [("use_karras_sigmas", True), ("rescale_betas_zero_snr", True), ("trained_betas", [0.1, 0.2]),
                      ("interpolation_type", "log_linear"), ("final_sigmas_type", "sigma_min"), ("clip_sample", True),
                      ("set_alpha_to_one", True), ("timestep_type", "continuous"), ("use_exponential_sigmas", True),
                      ("thresholding", True)]


def table_matrix():
    """[(entry name, class name, constructor kwargs)], one per config; every entry is dumped at every n of STEPS."""
    out = [("euler", "EulerDiscreteScheduler", {}), ("ddim", "DDIMScheduler", {})]
    # the keys that leave the sigmas alone vary fastest, so neighbouring solver tables compress against each other
    for spacing, karras, final, solver_type, order, lof in itertools.product(
            SPACINGS, (False, True), ("zero", "sigma_min"), ("midpoint", "heun"), (1, 2), (True, False)):
        kw = dict(SDXL, timestep_spacing=spacing, use_karras_sigmas=karras, final_sigmas_type=final,
                  solver_type=solver_type, solver_order=order, lower_order_final=lof)
        out.append((f"dpm/{spacing}/karras{int(karras)}/{final}/{solver_type}/order{order}/lof{int(lof)}",
                    "DPMSolverMultistepScheduler", kw))
    out.append(("dpm/euler_at_final", "DPMSolverMultistepScheduler",
                dict(SDXL, final_sigmas_type="sigma_min", lower_order_final=False, euler_at_final=True)))
    for spacing in SPACINGS:
        out.append((f"euler_a/{spacing}", "EulerAncestralDiscreteScheduler", dict(SDXL, timestep_spacing=spacing)))
    return out


def collect_tables(schedulers) -> dict:
    """{"<entry>/n<steps>/<field>": array}."""
    arrays = {}
    for name, cls, kw in table_matrix():
        for n in STEPS:
            sch = getattr(schedulers, cls)(**kw)
            sch.set_timesteps(n)
            got = {"timesteps": sch.timesteps.numpy(), "init_noise_sigma": np.float64(sch.init_noise_sigma),
                   "coef_table": sch.coef_table(7.5)}
            sigmas = getattr(sch, "sigmas", None)
            if sigmas is not None:
                got["sigmas"] = sigmas if isinstance(sigmas, np.ndarray) else sigmas.numpy()
            if sch.solver_table() is not None:
                got["solver_table"] = sch.solver_table()
            if hasattr(sch, "step_orders"):
                got["step_orders"] = sch.step_orders()
            for field, a in got.items():
                arrays[f"{name}/n{n}/{field}"] = np.array(a)
    return arrays


def _outcome(make) -> dict:
    try:
        return {"ok": dict(make().config)}
    except Exception as e:   # the refusals are NotImplementedError; anything else is recorded as what it is
        return {"raises": type(e).__name__}


def collect_outcomes(schedulers) -> dict:
    """{"<class> <route> <key>=<value>": {"ok": config} | {"raises": name}} for every refusal the tests list, through
    the constructor and through `from_config`, and for the cross-class `from_config` swaps."""
    cls = {name: getattr(schedulers, name) for name in CLASSES}
    euler, ddim, dpm, euler_a = (cls[name] for name in CLASSES)
    out = {}
    for c, base, refused in ((dpm, SDXL, DPM_REFUSED), (euler_a, SDXL, EULER_A_REFUSED),
                             (euler, EULER_DDIM_OK, EULER_DDIM_REFUSED), (ddim, EULER_DDIM_OK, EULER_DDIM_REFUSED)):
        for key, bad in refused:
            out[f"{c.__name__} constructor {key}={bad!r}"] = _outcome(lambda: c(**dict(base, **{key: bad})))
            out[f"{c.__name__} from_config {key}={bad!r}"] = _outcome(
                lambda: c.from_config(c(**base).config, **{key: bad}))
    sources = {"EulerDiscreteScheduler": euler, "DDIMScheduler": ddim, "DPMSolverMultistepScheduler": lambda: dpm(**SDXL),
               "DPMSolverMultistepScheduler(karras)": lambda: dpm(**dict(SDXL, use_karras_sigmas=True)),
               "EulerAncestralDiscreteScheduler": lambda: euler_a(**SDXL)}
    for (src, make), target in itertools.product(sources.items(), CLASSES):
        out[f"{target} from_config of {src}"] = _outcome(lambda: cls[target].from_config(make().config))
    return out


def pack(arrays: dict, outcomes: dict) -> dict:
    """One flat array per dtype plus a JSON index {key: [dtype, offset, shape]}: ~3000 npz members of a few hundred
    bytes each would be mostly zip headers."""
    blobs, index = {}, {}
    for key, a in arrays.items():
        dt = a.dtype.name
        parts = blobs.setdefault(dt, [])
        index[key] = [dt, sum(p.size for p in parts), list(a.shape)]
        parts.append(a.ravel())
    packed = {f"blob_{dt}": np.concatenate(parts) for dt, parts in blobs.items()}
    packed["index"] = np.array(json.dumps(index))
    packed["outcomes"] = np.array(json.dumps(outcomes))
    return packed


def unpack(npz) -> tuple:
    """(arrays, outcomes) of a file written from `pack`."""
    arrays = {}
    for key, (dt, offset, shape) in json.loads(str(npz["index"])).items():
        arrays[key] = npz[f"blob_{dt}"][offset:offset + int(np.prod(shape, dtype=np.int64))].reshape(shape)
    return arrays, json.loads(str(npz["outcomes"]))


def collect(root: str = None) -> tuple:
    """(arrays, outcomes) of the `diffsensei_amd.schedulers` importable from `root` (default: already on sys.path)."""
    if root is not None:
        sys.path.insert(0, os.path.abspath(root))
    from diffsensei_amd import schedulers
    # outcomes go through JSON like the stored ones (-inf stays -inf; a config holds no tuples)
    return collect_tables(schedulers), json.loads(json.dumps(collect_outcomes(schedulers)))


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=here, help="checkout whose diffsensei_amd.schedulers is dumped")
    ap.add_argument("-o", "--out", default=os.path.join(here, "tests", "golden", "scheduler_tables.npz"))
    args = ap.parse_args()
    arrays, outcomes = collect(args.root)
    np.savez_compressed(args.out, **pack(arrays, outcomes))
    refused = sum("raises" in o for o in outcomes.values())
    print(f"{args.out}: {len(arrays)} arrays of {len(table_matrix()) * len(STEPS)} entries, {len(outcomes)} outcomes "
          f"({refused} refused), {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
