#!/usr/bin/env python
"""GPU timing of the VAE encoder at 1024 x 1024 beside the decode of the same batch (HIP events, warm, median), and the
encoder's own ops one by one at the shapes they have there: the three downsample launches and the three encoder-only
kernels.  Writes what profiles/vae_encode.txt holds."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffsensei_amd import ops
from diffsensei_amd.vae import VaeConfig, VaeDecoderEngine, random_encoder_state_dict, random_state_dict

REPS = 7


def timed(fn, reps=REPS):
    fn()
    fn()                                    # warm: code objects, allocator
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    cfg = VaeConfig()
    precision = sys.argv[1] if len(sys.argv) > 1 else "fp16-scaled"
    eng = VaeDecoderEngine.from_state_dict({**random_state_dict(cfg, 0), **random_encoder_state_dict(cfg, 0)}, cfg, "cuda",
                                           precision=precision)
    enc = eng.encoder
    H = W = 1024
    efl, dfl = enc.encode_flops(H, W), eng.decode_flops(H // 8, W // 8)
    print(f"VAE at {H} x {W}, {precision}, median of {REPS} (min .. max), HIP events, warm; {torch.cuda.get_device_name(0)}")
    print(f"algorithmic flops per image: encode {efl / 1e12:.2f} TFLOP, decode {dfl / 1e12:.2f} TFLOP")
    g = torch.Generator().manual_seed(0)
    for B in (1, 8):
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
        lat = (torch.randn(B, 4, H // 8, W // 8, generator=g) * 0.9).cuda()
        ms, lo, hi = timed(lambda: enc.encode_latents(img))
        print(f"encode_latents B={B} (chunks of {enc.encode_chunk(H, W, B)}): {ms:8.2f} ms ({lo:.2f} .. {hi:.2f})  "
              f"{ms / B:7.2f} ms/image  {efl * B / ms / 1e9:6.1f} TFLOP/s algorithmic")
        ms, lo, hi = timed(lambda: eng.decode(lat, return_dict=False, scaling_factor=cfg.scaling_factor, denormalize=True))
        print(f"decode         B={B} (chunks of {eng.decode_chunk(H // 8, W // 8, B)}): {ms:8.2f} ms ({lo:.2f} .. {hi:.2f})  "
              f"{ms / B:7.2f} ms/image  {dfl * B / ms / 1e9:6.1f} TFLOP/s algorithmic")
    # ---- the encoder's own ops at the shapes of one image
    C = cfg.block_out_channels
    dt = enc.dt
    print("per op, one 1024 x 1024 image:")
    total_down, fl_down = 0.0, 0.0
    for i in range(len(C) - 1):
        h, w = H >> i, W >> i
        x = torch.randn(1, h, w, C[i], device="cuda").to(dt)
        name = f"encoder.down_blocks.{i}.downsamplers.0.conv"
        ms, lo, hi = timed(lambda: ops.conv3x3_down(x, enc.w[f"{name}.weight"], enc.w[f"{name}.bias"]))
        fl = 2.0 * (h // 2) * (w // 2) * 9 * C[i] * C[i]
        total_down, fl_down = total_down + ms, fl_down + fl
        print(f"  conv3x3_down [{h},{w},{C[i]}] -> [{h // 2},{w // 2},{C[i]}]: {ms:7.3f} ms ({lo:.3f} .. {hi:.3f})  {fl / ms / 1e9:6.1f} TFLOP/s")
    print(f"  three downsample launches: {total_down:.3f} ms, {100 * fl_down / efl:.1f} % of the encoder's flops")
    img = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    ms, lo, hi = timed(lambda: ops.vae_enc_conv_in(img, enc.w["encoder.conv_in.weight"], enc.w["encoder.conv_in.bias"]))
    print(f"  vae_enc_conv_in_kernel  [{H},{W},3] -> {C[0]}: {ms:7.3f} ms ({lo:.3f} .. {hi:.3f})")
    x = torch.randn(1, H // 8, W // 8, C[-1], device="cuda").to(dt)
    ms, lo, hi = timed(lambda: ops.vae_enc_conv_out(x, enc.w["encoder.conv_out.weight+q"], enc.w["encoder.conv_out.bias+q"]))
    print(f"  vae_enc_conv_out_kernel [{H // 8},{W // 8},{C[-1]}] -> 8: {ms:7.3f} ms ({lo:.3f} .. {hi:.3f})")
    mom = torch.randn(1, 8, H // 8, W // 8, device="cuda")
    seeds = torch.tensor([7], dtype=torch.int64, device="cuda")
    shift, scale = enc.latents_affine()
    ms, lo, hi = timed(lambda: ops.vae_latents(mom, scale, shift))
    ms2, lo2, hi2 = timed(lambda: ops.vae_latents(mom, scale, shift, seeds))
    print(f"  vae_latents_kernel      mode {ms:7.3f} ms ({lo:.3f} .. {hi:.3f}), sample {ms2:7.3f} ms ({lo2:.3f} .. {hi2:.3f})")


if __name__ == "__main__":
    main()
