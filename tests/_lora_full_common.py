"""tests/_lora_common.py extended to every target of `lora.all_target_modules`: seeded adapters with convolution and
time_emb_proj matrices in any of the three key forms, the merged weights in fp32 (what the oracle runs on) and the "fresh"
route - a state dict, in checkpoint layout, in which every target weight is `ops.lora_merge`'s plain output.

Magnitude: as in tests/_lora_common.py, A and B are normal with std 0.08 on the linears; on the convolutions, whose base
weights are 1 / sqrt(9 Cin) = 0.015 - 0.04, std 0.05 gives B A entries of about 0.05^2 sqrt(r) = 0.007.  With every layer
of the UNet moved the output is tens of percent away from the base's, which the tests gate on the oracles themselves.
"""
import torch

from diffsensei_amd.lora import all_target_modules, parse_lora_state_dict

STD_LINEAR, STD_CONV = 0.08, 0.05
NAMES = {"peft": lambda m: (f"{m}.lora_A.weight", f"{m}.lora_B.weight"),
         "diffusers": lambda m: (f"unet.{m}.lora.down.weight", f"unet.{m}.lora.up.weight"),
         "underscore": lambda m: (f"lora_unet_{m.replace('.', '_')}.lora_down.weight", f"lora_unet_{m.replace('.', '_')}.lora_up.weight")}


def make_full_adapter(cfg, rank, seed, keep=lambda m: True, fmt="peft"):
    """A LoRA state dict (fp32 tensors with f16 values) on every target `keep` accepts, convolutions with a 4-D down matrix
    of the layer's own kernel size and (underscore form) a [Cout, r, 1, 1] up matrix."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for m, shp in all_target_modules(cfg).items():
        if not keep(m):
            continue
        std = STD_CONV if len(shp) == 4 else STD_LINEAR
        down, up = NAMES[fmt](m)
        sd[down] = (torch.randn(rank, *shp[1:], generator=g) * std).half().float()
        B = (torch.randn(shp[0], rank, generator=g) * std).half().float()
        sd[up] = B[:, :, None, None] if len(shp) == 4 and fmt == "underscore" else B
    return sd


def _delta(A, B):
    return B.float() @ A.float() if A.dim() == 2 else torch.einsum("or,rikl->oikl", B.float(), A.float())


def merged_fp32_full(cfg, sd, adapters):
    """sd with W + sum weight * alpha / r * B A on every target, in fp32 and checkpoint layout."""
    out = {k: v.float().cpu() for k, v in sd.items()}
    for lora_sd, weight in adapters:
        for m, (A, B, alpha) in parse_lora_state_dict(lora_sd, cfg=cfg).items():
            out[m + ".weight"] = out[m + ".weight"] + weight * alpha / A.shape[0] * _delta(A, B)
    return out


def fresh_route_full(cfg, sd, adapters, device):
    """sd (f16) with every target weight replaced by the plain output of `ops.lora_merge` for these adapters and weights,
    brought back to the checkpoint layout (a packed 3x3 output is un-permuted; packing it again gives the same bits)."""
    from diffsensei_amd import ops
    from diffsensei_amd.lora import pack_conv_down
    parsed = [(parse_lora_state_dict(lora_sd, cfg=cfg), float(w)) for lora_sd, w in adapters]
    out = dict(sd)
    for m, shp in all_target_modules(cfg).items():
        hits = [(p[m], w) for p, w in parsed if m in p]
        if not hits:
            continue
        A = torch.cat([pack_conv_down(h[0]) for h, _ in hits], 0).contiguous().to(device)
        B = torch.cat([h[1] for h, _ in hits], 1).contiguous().to(device)
        seg = [0]
        for h, _ in hits:
            seg.append(seg[-1] + h[0].shape[0])
        # the strength as the merge plan forms it: fp32(alpha / r) * fp32(weight), rounded to fp32
        s = torch.tensor([h[2] / h[0].shape[0] for h, _ in hits], dtype=torch.float32) * torch.tensor([w for _, w in hits], dtype=torch.float32)
        W = sd[m + ".weight"].to(device).half().contiguous()
        if len(shp) == 4 and shp[2] == 3:
            got = ops.lora_merge(W, A, B, seg, s.to(device), conv_cin=shp[1])
            got = got.reshape(shp[0], 3, 3, shp[1]).permute(0, 3, 1, 2).contiguous()
        else:
            got = ops.lora_merge(W.reshape(shp[0], -1), A, B, seg, s.to(device)).reshape(shp)
        out[m + ".weight"] = got.cpu()
    return out
