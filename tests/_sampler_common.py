"""Shared by the sampler tests (tests/test_gpu_dpm.py, tests/test_gpu_euler_ancestral.py and their CPU counterparts): the
SDXL scheduler config, the fp16 rounding and comparison helpers, and the tiny pipeline (`parts` fixture, `_pipe`) the
whole-pipeline tests run.  A plain module, not a conftest: a test file imports what it uses, the `parts` fixture by name."""
import numpy as np
import pytest
import torch

DEV = "cuda"
hq = lambda t: t.half().float()
SDXL = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
            timestep_spacing="leading")


def _close(got, ref, tol=1.5e-3, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    den = max(ref.abs().max().item(), 1e-3)
    assert err <= tol * den + 1e-3 * tol, f"{what}: max err {err:.4g} vs max|ref| {den:.4g}"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).contiguous()


# ---------------------------------------------------------------- the whole pipeline
@pytest.fixture(scope="module")
def parts(hip_lib):
    from PIL import Image
    from transformers import CLIPVisionConfig, CLIPVisionModel, ViTMAEConfig, ViTMAEModel
    from diffsensei_amd.resampler import Resampler
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    torch.manual_seed(0)
    clip = CLIPVisionModel(CLIPVisionConfig(hidden_size=160, intermediate_size=320, num_hidden_layers=4,
                                            num_attention_heads=2, image_size=224, patch_size=14, hidden_act="gelu")).eval()
    mae = ViTMAEModel(ViTMAEConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=256,
                                   image_size=224, patch_size=16, mask_ratio=0.0)).eval()
    cfg = tiny_config()
    sd = {k: v.half() for k, v in random_state_dict(cfg, 2).items()}
    rs = Resampler(dim=128, depth=2, dim_head=64, heads=2, num_queries=16, num_dummy_tokens=16, embedding_dim=160,
                   magi_embedding_dim=128, output_dim=cfg.cross_attention_dim, ff_mult=4, device=DEV).init_random(3)
    rng = np.random.RandomState(0)
    imgs = [Image.fromarray(rng.randint(0, 256, (224, 224, 3), dtype=np.uint8)) for _ in range(2)]
    g = torch.Generator().manual_seed(5)
    pe = torch.randn(1, 77, cfg.cross_attention_dim, generator=g).half()
    pooled = torch.randn(1, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g).half()
    lat0 = torch.randn(2, 4, 16, 16, generator=g).half()
    return dict(clip=clip, mae=mae, cfg=cfg, sd=sd, rs=rs, imgs=imgs, pe=pe, pooled=pooled, lat0=lat0)


IP_BBOX = [[0.05, 0.10, 0.50, 0.95], [0.50, 0.10, 0.95, 0.95]]
DIALOG = [[0.05, 0.02, 0.30, 0.15], [0.65, 0.02, 0.95, 0.15]]


def _pipe(parts, scheduler):
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.unet import UNetMangaModel
    unet = UNetMangaModel(parts["cfg"], device=DEV)
    unet.load_state_dict(parts["sd"])
    pipe = DiffSenseiPipeline(None, None, None, None, None, scheduler, unet, parts["clip"])
    pipe.register_manga_modules(magi_image_encoder=parts["mae"], image_proj_model=parts["rs"])
    return pipe
