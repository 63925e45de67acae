"""TEST INFRASTRUCTURE ONLY: fp32 torch restatement of `AutoencoderKL.encode` (diffusers [3P]) with diffusers key names.

    AutoencoderKL.encode(x)   = quant_conv(Encoder(x)) -> moments: latent_channels x mean, latent_channels x logvar
    Encoder                   = conv_in(3 -> C0) -> n x DownEncoderBlock2D -> UNetMidBlock2D -> GroupNorm(32, eps 1e-6)
                                -> SiLU -> conv_out(C3 -> 2 lc)          block_out_channels (C0..C3) = (128,256,512,512)
    DownEncoderBlock2D i      = layers_per_block x ResnetBlock2D [+ Downsample2D(padding=0): F.pad(x, (0,1,0,1)),
                                Conv2d 3x3 stride 2 without padding]; no downsample in the last block
    DiagonalGaussianDistribution: logvar clamped to [-30, 20]

PARITY UNPINNED, like the decoder's oracle (oracle/vae_ref.py, whose `_resnet` / `_attention` this file imports):
diffusers is not importable here, so no golden vector of the real module exists; the restatement follows the published
module structure and is the fp32 yard-stick of the HIP encoder.  `diffsensei_amd.vae.vae_encoder_param_shapes` lists the keys.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle.vae_ref import _attention, _resnet

Tensor = torch.Tensor


def downsample(x: Tensor, w: Tensor, b: Optional[Tensor]) -> Tensor:
    """Downsample2D(padding=0): pad right and bottom by one, then 3x3, stride 2, no padding."""
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)


def vae_encode(sd: Dict[str, Tensor], x: Tensor, layers_per_block: int = 2, groups: int = 32, eps: float = 1e-6,
               n_down: int = 4, taps: Optional[dict] = None) -> Tensor:
    """x [B,3,H,W] in [-1, 1] -> moments [B,2*lc,H/8,W/8] fp32 (logvar clamped).  `taps`: max |residual stream| per block."""
    sd = {k: v.float() for k, v in sd.items()}
    tap = (lambda name, t: taps.__setitem__(name, float(t.abs().max()))) if taps is not None else (lambda name, t: None)
    h = F.conv2d(x.float(), sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"], padding=1)
    tap("conv_in", h)
    for i in range(n_down):
        for j in range(layers_per_block):
            h = _resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}", h, groups, eps)
        d = f"encoder.down_blocks.{i}.downsamplers.0.conv"
        if f"{d}.weight" in sd:
            h = downsample(h, sd[f"{d}.weight"], sd[f"{d}.bias"])
        tap(f"down_blocks.{i}", h)
    h = _resnet(sd, "encoder.mid_block.resnets.0", h, groups, eps)
    h = _attention(sd, "encoder.mid_block.attentions.0", h, groups, eps)
    h = _resnet(sd, "encoder.mid_block.resnets.1", h, groups, eps)
    tap("mid_block", h)
    h = F.silu(F.group_norm(h, groups, sd["encoder.conv_norm_out.weight"], sd["encoder.conv_norm_out.bias"], eps))
    h = F.conv2d(h, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"], padding=1)
    m = F.conv2d(h, sd["quant_conv.weight"], sd["quant_conv.bias"])
    lc = m.shape[1] // 2
    return torch.cat([m[:, :lc], m[:, lc:].clamp(-30.0, 20.0)], dim=1)
