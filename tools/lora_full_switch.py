"""What switching an adapter on EVERY target costs at SDXL dimensions - the transformer-block linears plus conv1 / conv2 /
conv_shortcut / time_emb_proj of every resnet and the four sampler convolutions - against rebuilding `PackedUNet`.

    python tools/lora_full_switch.py [--out profiles/lora_full_switch.txt] [--rank 64] [--size 1024] [--batch 2]

Random weights, one rank-`rank` adapter on every module of `lora.all_target_modules`, UNet batch `batch` at size x size.  One
process, this order: base forward (packs, builds the engine, folds the upsamplers), the first `set_adapters` (builds and
captures the merge plan), three off / on switches, the split of a switch (merge plan replay, derived refresh), then
`PackedUNet(cfg, state_dict, device)` built three times in the same run - the re-pack alone, without the engine build and the
graph capture that a real rebuild also pays.  Wall times, synchronised.  The figure of the linear-only plan
(profiles/lora_switch.txt, rank 128 on to_q / to_k / to_v / to_out.0) is quoted beside them when that file is there.  Exit
status 1 if the in-place switch is not faster than the rebuild.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffsensei_amd import _lib  # noqa: E402
from diffsensei_amd.engine import PackedUNet  # noqa: E402
from diffsensei_amd.lora import all_target_modules, target_modules  # noqa: E402
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
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=2)
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
    targets = all_target_modules(cfg)
    lora = {}
    for m, shp in targets.items():
        lora[m + ".lora_A.weight"] = (torch.randn(a.rank, *shp[1:], generator=g, device=dev) * 0.02).half()
        lora[m + ".lora_B.weight"] = (torch.randn(shp[0], a.rank, generator=g, device=dev) * 0.02).half()
    B, H = a.batch, a.size // 8
    x = torch.randn(B, 4, H, H, generator=g, device=dev).half()
    enc = torch.randn(B, cfg.num_text_tokens + cfg.num_ip_tokens, cfg.cross_attention_dim, generator=g, device=dev).half()
    te = torch.randn(B, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g, device=dev).half()
    tid = torch.tensor([[a.size, a.size, 0, 0, a.size, a.size]] * B, dtype=torch.float16)
    bbox = torch.zeros(B, cfg.max_num_ips, 4)

    def forward():
        return model(x, 801.0, enc, cross_attention_kwargs={"bbox": bbox, "aspect_ratio": 1.0},
                     added_cond_kwargs={"text_embeds": te, "time_ids": tid}).sample

    n_lin = len(target_modules(cfg))
    say(f"# LoRA switch on every target at SDXL dimensions: rank {a.rank} on {len(targets)} modules ({n_lin} linears, "
        f"{len(targets) - n_lin} convolutions and time_emb_proj), UNet batch {B} at {a.size} x {a.size}")
    t_first, base_out = wall(lambda: forward().clone())
    say(f"first base forward (pack + engine build + forward, for scale): {t_first:.2f} s")
    model.load_lora_adapter(lora, "full")
    forward()                                     # loading may move buffers once (dealias): the engine is built again here
    eng = model.engine(B, H, H, 1.0)
    pk = model.packed()
    folds = [k for k in pk.w if k.endswith(".up2fold")]
    t_build, _ = wall(lambda: model.set_adapters(["full"], 1.0))
    say(f"set_adapters, first time (builds and captures the merge plan): {t_build * 1e3:9.1f} ms")
    times = []
    for k in range(3):
        t_off, _ = wall(lambda: model.set_adapters([]))
        t_on, _ = wall(lambda: model.set_adapters(["full"], 1.0))
        times.append((t_off, t_on))
        say(f"switch {k}: set_adapters([]) {t_off * 1e3:8.1f} ms   set_adapters(['full']) {t_on * 1e3:8.1f} ms")
    t_on = sorted(t for _, t in times)[1]
    t_off = sorted(t for t, _ in times)[1]
    mp = model._lora.last_plan
    t_plan = sorted(wall(lambda: mp.plan.replay())[0] for _ in range(5))[2]
    t_ref = sorted(wall(lambda: pk.refresh_derived(mp.blocks, mp.folds))[0] for _ in range(3))[1]
    tot_b = tot_f = 0.0
    for op in mp.ops:
        fl, by = C.c_double(), C.c_double()
        lib.ds_op_describe(C.byref(op), None, 0, C.byref(fl), C.byref(by))
        tot_b, tot_f = tot_b + by.value, tot_f + fl.value
    launches = -(-len(mp.ops) // 24)
    say(f"split: merge plan as one hipGraph replay {t_plan * 1e3:.2f} ms ({len(mp.ops)} matrices in {launches} launches, "
        f"{tot_b / 1e9:.2f} GB, {tot_f / 1e12:.3f} TFLOP: {tot_b / t_plan / 1e12:.2f} TB/s = "
        f"{100 * tot_b / t_plan / HBM_ACHIEVABLE:.0f} % of the 6.3 TB/s achievable), derived refresh {t_ref * 1e3:.2f} ms "
        f"({len(mp.folds)} upsampler folds recomputed, {len(folds)} exist)")
    assert model.engine(B, H, H, 1.0) is eng and model.packed() is pk, "a switch must not rebuild anything"
    merged_out = forward().clone()
    say(f"forward output moved by the adapter: {bool(not torch.equal(merged_out, base_out))}")
    model.set_adapters([])
    say(f"forward output back to the base bits after set_adapters([]): {bool(torch.equal(forward(), base_out))}")

    sd = model._sd
    t_pack = sorted(wall(lambda: PackedUNet(cfg, sd, dev))[0] for _ in range(3))
    say(f"PackedUNet(cfg, state_dict, device), the re-pack alone (no engine build, no capture), 3 runs: "
        f"{' / '.join(f'{t * 1e3:.1f}' for t in t_pack)} ms")
    ref = os.path.join(ROOT, "profiles", "lora_switch.txt")
    if os.path.exists(ref):
        last = [ln.strip() for ln in open(ref) if ln.startswith("in place")]
        say(f"linear-only plan, for comparison (profiles/lora_switch.txt; rank 128 on to_q/to_k/to_v/to_out.0): {last[-1] if last else 'n/a'}")
    ok = max(t_on, t_off) < t_pack[1]
    say(f"full-target switch: on {t_on * 1e3:.1f} ms, off {t_off * 1e3:.1f} ms (medians of 3) vs PackedUNet rebuild {t_pack[1] * 1e3:.1f} ms "
        f"(median of 3): {t_pack[1] / max(t_on, t_off):.1f} x ({'faster' if ok else 'NOT faster'} than the rebuild)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
