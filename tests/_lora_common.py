"""Shared by the LoRA GPU tests: seeded adapters for the tiny UNet, the merged weights in fp32 (what the oracle runs on)
and the "fresh" route - a state dict in which every target matrix is `ops.lora_merge`'s plain output.

Magnitude: A and B are normal with std 0.08, so B A has entries of about 0.08^2 sqrt(r) = 0.02 beside base weights of
1 / sqrt(K) = 0.06 - 0.09: the merged UNet's output is tens of percent away from the base's (the tests gate that on the
oracles themselves), so a merge that does nothing cannot pass.
"""
import torch

from diffsensei_amd.lora import parse_lora_state_dict, target_modules

STD = 0.08
REFERENCE_LEAVES = ("to_q", "to_k", "to_v", "to_out.0")          # the reference's LoraConfig target_modules


def make_adapter(cfg, rank, seed, keep=lambda m: True, fmt="peft", prefix=""):
    """A LoRA state dict (fp32 tensors with f16 values) on every target module `keep` accepts."""
    g = torch.Generator().manual_seed(seed)
    down, up = {"peft": ("lora_A.weight", "lora_B.weight"), "peft_named": ("lora_A.default.weight", "lora_B.default.weight"),
                "diffusers": ("lora.down.weight", "lora.up.weight")}[fmt]
    sd = {}
    for m, (N, K) in target_modules(cfg).items():
        if keep(m):
            sd[f"{prefix}{m}.{down}"] = (torch.randn(rank, K, generator=g) * STD).half().float()
            sd[f"{prefix}{m}.{up}"] = (torch.randn(N, rank, generator=g) * STD).half().float()
    return sd


def merged_fp32(cfg, sd, adapters):
    """sd with W + sum weight * alpha / r * B A on every target, in fp32.  adapters: [(lora state dict, weight), ...]."""
    out = {k: v.float().cpu() for k, v in sd.items()}
    for lora_sd, weight in adapters:
        for m, (A, B, alpha) in parse_lora_state_dict(lora_sd, cfg=cfg).items():
            out[m + ".weight"] = out[m + ".weight"] + weight * alpha / A.shape[0] * (B.float() @ A.float())
    return out


def fresh_route(cfg, sd, adapters, device):
    """sd (f16) with every target matrix replaced by the plain output of `ops.lora_merge` for these adapters and weights:
    what a model must be loaded with to compute, without any adapter machinery, what `set_adapters` gives in place."""
    from diffsensei_amd import ops
    parsed = [(parse_lora_state_dict(lora_sd, cfg=cfg), float(w)) for lora_sd, w in adapters]
    out = dict(sd)
    for m in target_modules(cfg):
        hits = [(p[m], w) for p, w in parsed if m in p]
        if not hits:
            continue
        A = torch.cat([h[0] for h, _ in hits], 0).to(device)
        B = torch.cat([h[1] for h, _ in hits], 1).contiguous().to(device)
        seg = [0]
        for h, _ in hits:
            seg.append(seg[-1] + h[0].shape[0])
        # the strength as the merge plan forms it: fp32(alpha / r) * fp32(weight), rounded to fp32
        s = torch.tensor([h[2] / h[0].shape[0] for h, _ in hits], dtype=torch.float32) * torch.tensor([w for _, w in hits], dtype=torch.float32)
        out[m + ".weight"] = ops.lora_merge(sd[m + ".weight"].to(device).half().contiguous(), A, B, seg, s.to(device)).cpu()
    return out
