"""What a LoRA switch costs at SDXL dimensions: `set_adapters` in place against the route that existed before it -
`load_state_dict(merged)` + re-pack + engine build + graph capture up to the first forward.

    python tools/lora_switch_bench.py [--out profiles/lora_switch.txt] [--rank 128] [--size 1024] [--batch 2]

Random weights, one rank-`rank` adapter on the reference's four targets (to_q / to_k / to_v / to_out.0 of attn1 and attn2),
UNet batch `batch` at size x size.  One process, this order: base forward (packs, builds the engine), in-place switches,
forward timings with and without the adapter, then the rebuild route.  Wall times, synchronised.  Both routes are timed to
the same end point: everything is ready for the next forward, which is not part of either figure.  The merged weights of
the rebuild route already lie in device memory (the case most favourable to it).  Exit status 1 if the in-place switch is
not at least `--min-ratio` (5) times faster.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diffsensei_amd import _lib, ops  # noqa: E402
from diffsensei_amd.lora import target_modules  # noqa: E402
from diffsensei_amd.unet import UNetMangaModel  # noqa: E402
from diffsensei_amd.unet_config import sdxl_config  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes / s


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rank", type=int, default=128)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--forwards", type=int, default=10)
    ap.add_argument("--min-ratio", type=float, default=5.0)
    a = ap.parse_args()
    dev = torch.device("cuda")
    lib = _lib.load()
    cfg = sdxl_config()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    model = UNetMangaModel(cfg, device=dev).init_random(0)
    g = torch.Generator(device=dev).manual_seed(1)
    lora = {}
    for m, (N, K) in target_modules(cfg).items():
        if m.endswith(("to_q", "to_k", "to_v", "to_out.0")):
            lora[m + ".lora_A.weight"] = (torch.randn(a.rank, K, generator=g, device=dev) * 0.02).half()
            lora[m + ".lora_B.weight"] = (torch.randn(N, a.rank, generator=g, device=dev) * 0.02).half()
    model.load_lora_adapter(lora, "style")
    B, H = a.batch, a.size // 8
    x = torch.randn(B, 4, H, H, generator=g, device=dev).half()
    enc = torch.randn(B, cfg.num_text_tokens + cfg.num_ip_tokens, cfg.cross_attention_dim, generator=g, device=dev).half()
    te = torch.randn(B, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g, device=dev).half()
    tid = torch.tensor([[a.size, a.size, 0, 0, a.size, a.size]] * B, dtype=torch.float16)
    bbox = torch.zeros(B, cfg.max_num_ips, 4)

    def forward():
        return model(x, 801.0, enc, cross_attention_kwargs={"bbox": bbox, "aspect_ratio": 1.0},
                     added_cond_kwargs={"text_embeds": te, "time_ids": tid}).sample

    def graph_forward():
        eng = model.engine(B, H, H, 1.0)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            if not eng.forward_plan.captured:
                eng.forward_plan.capture(st.cuda_stream)
            eng.forward_plan.replay(st.cuda_stream)
        st.synchronize()

    def capture_only():
        eng = model.engine(B, H, H, 1.0)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            if not eng.forward_plan.captured:
                eng.forward_plan.capture(st.cuda_stream)
        st.synchronize()

    def forward_ms(n):
        eng = model.engine(B, H, H, 1.0)
        ts = []
        for _ in range(n):
            ts.append(wall(lambda: eng.forward_plan.run())[0] * 1e3)
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    say(f"# LoRA switch at SDXL dimensions: rank {a.rank} on to_q/to_k/to_v/to_out.0, UNet batch {B} at {a.size} x {a.size}")
    t_first, base_out = wall(lambda: (forward(), graph_forward())[0])
    say(f"first base forward (pack + engine build + capture + two forwards, for scale): {t_first:.2f} s")
    eng = model.engine(B, H, H, 1.0)

    # ---- in place
    t_build, _ = wall(lambda: model.set_adapters(["style"], 1.0))
    say(f"set_adapters, first time (builds the merge plan):          {t_build * 1e3:9.1f} ms")
    times = []
    for k in range(3):
        t_off, _ = wall(lambda: model.set_adapters([]))
        t_on, _ = wall(lambda: model.set_adapters(["style"], 1.0))
        times.append((t_off, t_on))
        say(f"switch {k}: set_adapters([]) {t_off * 1e3:8.1f} ms   set_adapters(['style']) {t_on * 1e3:8.1f} ms")
    t_inplace = sorted(t for _, t in times)[1]
    mp = model._lora.last_plan
    pk = model.packed()
    t_plan = sorted(wall(lambda: mp.plan.replay())[0] for _ in range(5))[2]
    t_eager = sorted(wall(lambda: mp.plan.run())[0] for _ in range(5))[2]
    t_ref = sorted(wall(lambda: pk.refresh_derived(mp.blocks))[0] for _ in range(3))[1]
    tot_b = tot_f = 0.0
    for op in mp.ops:
        fl, by = C.c_double(), C.c_double()
        lib.ds_op_describe(C.byref(op), None, 0, C.byref(fl), C.byref(by))
        tot_b, tot_f = tot_b + by.value, tot_f + fl.value
    launches = -(-len(mp.ops) // 24)       # the plan executor groups up to 24 consecutive merges into one launch
    say(f"split: merge plan as one hipGraph replay {t_plan * 1e3:.2f} ms ({len(mp.ops)} matrices in {launches} launches, "
        f"{tot_b / 1e9:.2f} GB, {tot_f / 1e12:.3f} TFLOP: {tot_b / t_plan / 1e12:.2f} TB/s = "
        f"{100 * tot_b / t_plan / HBM_ACHIEVABLE:.0f} % of the 6.3 TB/s achievable; the same plan as eager launches "
        f"{t_eager * 1e3:.2f} ms), derived refresh {t_ref * 1e3:.2f} ms")
    assert model.engine(B, H, H, 1.0) is eng
    merged_out = forward().clone()

    # ---- forward time: same plan, other weight values
    on = forward_ms(a.forwards)
    model.set_adapters([])
    off1 = forward_ms(a.forwards)
    off2 = forward_ms(a.forwards)
    say(f"forward, eager plan, median (min .. max) of {a.forwards}: adapter active {on[0]:.2f} ({on[1]:.2f} .. {on[2]:.2f}) ms, "
        f"none {off1[0]:.2f} ({off1[1]:.2f} .. {off1[2]:.2f}) ms, none again (A/A) {off2[0]:.2f} ({off2[1]:.2f} .. {off2[2]:.2f}) ms")

    # ---- the route without in-place merging: merged weights through load_state_dict
    merged = dict(model.state_dict())
    for m in target_modules(cfg):
        if m + ".lora_A.weight" in lora:
            A_, B_ = lora[m + ".lora_A.weight"], lora[m + ".lora_B.weight"]
            merged[m + ".weight"] = ops.lora_merge(merged[m + ".weight"], A_, B_, [0, a.rank], [1.0])
    model.delete_adapters("style")         # the rebuild route carries no adapter machinery at all
    torch.cuda.synchronize()

    def rebuild():
        model.load_state_dict(merged)
        model.packed()
        capture_only()                     # engine build + capture of the forward plan; no forward
    t_rebuild, _ = wall(rebuild)
    out2 = forward().clone()
    say(f"rebuild route (load_state_dict(merged, on the device) + pack + engine build + capture, no forward): {t_rebuild * 1e3:.1f} ms")
    say(f"same output bits on both routes: {bool(torch.equal(out2, merged_out))}")
    ratio = t_rebuild / t_inplace
    ok = ratio >= a.min_ratio
    say(f"in place {t_inplace * 1e3:.1f} ms vs rebuild {t_rebuild * 1e3:.1f} ms, both up to (not including) the next forward: "
        f"{ratio:.1f} x ({'meets' if ok else 'MISSES'} the {a.min_ratio:g} x required)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
