"""CPU: the host side of the VAE encoder - the key set, the decoder helpers left where they were, the reference's
downsample against a triple loop, the quant_conv fold, the refusals of `redraw_image` (raised before any encoder runs)
and bucketing."""
import hashlib
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _vae_encode_ref as E


def test_encoder_param_shapes_sdxl():
    from diffsensei_amd.vae import VaeConfig, vae_encoder_param_shapes, vae_param_shapes
    sh = vae_encoder_param_shapes(VaeConfig())
    # conv_in 2; down blocks 18 + 20 + 20 + 16 (two resnets each, a shortcut where the width changes, a downsampler on all but
    # the last); mid block 8 + 10 + 8; conv_norm_out, conv_out, quant_conv 2 each
    assert len(sh) == 108
    assert all(k.startswith(("encoder.", "quant_conv.")) for k in sh)
    assert not set(sh) & set(vae_param_shapes(VaeConfig()))
    want = {
        "encoder.conv_in.weight": (128, 3, 3, 3), "encoder.conv_in.bias": (128,),
        "encoder.down_blocks.0.resnets.0.norm1.weight": (128,),
        "encoder.down_blocks.0.resnets.1.conv2.weight": (128, 128, 3, 3),
        "encoder.down_blocks.0.downsamplers.0.conv.weight": (128, 128, 3, 3),
        "encoder.down_blocks.1.resnets.0.conv1.weight": (256, 128, 3, 3),
        "encoder.down_blocks.1.resnets.0.conv_shortcut.weight": (256, 128, 1, 1),
        "encoder.down_blocks.1.resnets.1.norm1.bias": (256,),
        "encoder.down_blocks.1.downsamplers.0.conv.bias": (256,),
        "encoder.down_blocks.2.resnets.0.conv_shortcut.bias": (512,),
        "encoder.down_blocks.2.downsamplers.0.conv.weight": (512, 512, 3, 3),
        "encoder.down_blocks.3.resnets.1.conv1.weight": (512, 512, 3, 3),
        "encoder.mid_block.resnets.0.conv1.weight": (512, 512, 3, 3),
        "encoder.mid_block.attentions.0.group_norm.weight": (512,),
        "encoder.mid_block.attentions.0.to_q.weight": (512, 512),
        "encoder.mid_block.attentions.0.to_out.0.bias": (512,),
        "encoder.mid_block.resnets.1.norm2.bias": (512,),
        "encoder.conv_norm_out.weight": (512,),
        "encoder.conv_out.weight": (8, 512, 3, 3), "encoder.conv_out.bias": (8,),
        "quant_conv.weight": (8, 8, 1, 1), "quant_conv.bias": (8,),
    }
    for k, v in want.items():
        assert sh[k] == v, k
    for absent in ("encoder.down_blocks.3.downsamplers.0.conv.weight", "encoder.down_blocks.0.resnets.0.conv_shortcut.weight",
                   "encoder.down_blocks.3.resnets.0.conv_shortcut.weight", "encoder.down_blocks.0.resnets.2.norm1.weight"):
        assert absent not in sh
    keys = list(sh)
    assert keys[0] == "encoder.conv_in.weight" and keys[-2:] == ["quant_conv.weight", "quant_conv.bias"]
    assert keys.index("encoder.mid_block.resnets.0.norm1.weight") > keys.index("encoder.down_blocks.3.resnets.1.conv2.bias")


def _sha(t):
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()[:16]


def test_decoder_random_state_dict_unchanged():
    """The first and the last draw of `random_state_dict(cfg, 0)`, hashed on the commit before the encoder existed: one
    extra draw from its generator would move every decoder test's weights."""
    from diffsensei_amd.vae import VaeConfig, random_encoder_state_dict, random_state_dict, vae_param_shapes
    sd = random_state_dict(VaeConfig(), 0)
    assert len(sd) == 140 and list(sd) == list(vae_param_shapes(VaeConfig()))
    assert _sha(sd["post_quant_conv.weight"]) == "8d1d75f4dc7f7df5"
    assert _sha(sd["decoder.conv_out.bias"]) == "0d8d2221a82027cc"
    enc = random_encoder_state_dict(VaeConfig(), 0)
    assert not set(enc) & set(sd)
    assert torch.equal(random_encoder_state_dict(VaeConfig(), 0)["quant_conv.bias"], enc["quant_conv.bias"])
    assert not torch.equal(random_encoder_state_dict(VaeConfig(), 1)["quant_conv.bias"], enc["quant_conv.bias"])


def _down_loops(x, w):
    """Output (Y, X) = sum over ky, kx of w[ky, kx] * x[2Y + ky, 2X + kx]; rows >= H and columns >= W read as zero."""
    H, W = x.shape
    out = torch.zeros(H // 2, W // 2, dtype=torch.float64)
    for Y in range(H // 2):
        for X in range(W // 2):
            for ky in range(3):
                for kx in range(3):
                    iy, ix = 2 * Y + ky, 2 * X + kx
                    if iy < H and ix < W:
                        out[Y, X] += w[ky, kx] * x[iy, ix]
    return out


def test_reference_downsample_is_the_one_sided_pad():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(3, 3, generator=g, dtype=torch.float64)
    for H, W in ((5, 6), (6, 6)):
        x = torch.randn(H, W, generator=g, dtype=torch.float64)
        got = E.downsample(x[None, None], w[None, None], None)[0, 0]
        assert got.shape == (H // 2, W // 2)
        assert torch.allclose(got, _down_loops(x, w), rtol=0, atol=1e-12)
    # 6 x 6: the symmetric-pad stride-2 convolution (the UNet's) is another function of the same input
    x = torch.randn(6, 6, generator=g, dtype=torch.float64)
    sym = F.conv2d(x[None, None], w[None, None], None, stride=2, padding=1)[0, 0]
    one = E.downsample(x[None, None], w[None, None], None)[0, 0]
    assert sym.shape == one.shape == (3, 3) and float((sym - one).abs().max()) > 0.1
    # 5 x 6: the last output row reads rows 2, 3, 4 - the pad row is never read, the pad column (6) is
    x = torch.randn(5, 6, generator=g, dtype=torch.float64)
    nopad_rows = F.conv2d(F.pad(x[None, None], (0, 1, 0, 0)), w[None, None], None, stride=2)[0, 0]
    assert torch.equal(E.downsample(x[None, None], w[None, None], None)[0, 0], nopad_rows)


def test_quant_conv_fold():
    from diffsensei_amd.vae import fold_quant_conv
    g = torch.Generator().manual_seed(5)
    wc, bc = torch.randn(8, 64, 3, 3, generator=g) / 24.0, torch.randn(8, generator=g)
    wq, bq = torch.randn(8, 8, 1, 1, generator=g) * 0.5, torch.randn(8, generator=g)
    x = torch.randn(2, 64, 9, 11, generator=g)
    w2, b2 = fold_quant_conv(wc, bc, wq, bq)
    assert w2.shape == (8, 64, 3, 3) and b2.shape == (8,) and w2.dtype == b2.dtype == torch.float32
    ref = F.conv2d(F.conv2d(x, wc, bc, padding=1), wq, bq)
    got = F.conv2d(x, w2, b2, padding=1)
    assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-6


# ---------------------------------------------------------------- refusals, before any encoder runs
def _pipe(vae):
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    unet = types.SimpleNamespace(config=types.SimpleNamespace(sample_size=16, in_channels=4, max_num_ips=4),
                                 device=torch.device("cpu"), dtype=torch.float16, attn_processors={})
    p = DiffSenseiPipeline(vae, None, None, None, None, EulerDiscreteScheduler(), unet, None)

    def boom(*a, **k):
        raise AssertionError("an encoder ran before the redraw arguments were checked")
    p.encode_prompt = p.prepare_ip_image_embeds = p._denoise = boom
    return p


def _vae_with_encoder():
    def boom(*a, **k):
        raise AssertionError("the VAE encoder ran before the redraw arguments were checked")
    return types.SimpleNamespace(encoder=types.SimpleNamespace(encode_latents=boom), decode=None)


def test_redraw_image_refusals():
    from PIL import Image
    pipe = _pipe(_vae_with_encoder())
    img = Image.fromarray(np.zeros((128, 128, 3), dtype=np.uint8))
    box = [[0.5, 0, 1, 1]]
    call = lambda p=pipe, **kw: p(**dict(dict(prompt="p", height=128, width=128, num_inference_steps=10), **kw))
    cases = [
        dict(redraw_image=img, redraw_latents=torch.zeros(1, 4, 16, 16), redraw_bbox=box),          # both
        dict(redraw_image=Image.fromarray(np.zeros((128, 120, 3), dtype=np.uint8)), redraw_bbox=box),   # wrong size
        dict(redraw_image=Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8)), redraw_bbox=box),
        dict(redraw_image=torch.zeros(1, 3, 128, 64), redraw_bbox=box),
        dict(redraw_image=np.zeros((100, 100, 3), dtype=np.uint8), redraw_bbox=box, height=100, width=100),   # not a multiple of 8
        dict(redraw_image=torch.zeros(3, 128, 128, 3, dtype=torch.uint8), redraw_bbox=box, num_samples=2),   # 3 images, 2 samples
        dict(redraw_image=torch.full((1, 3, 128, 128), 1.5), redraw_bbox=box),                        # float outside [0, 1]
        dict(redraw_image=torch.zeros(128, 128, 3, dtype=torch.int32), redraw_bbox=box),
        dict(redraw_image="page.png", redraw_bbox=box),
        dict(redraw_image=img),                                                                       # no region
        dict(redraw_image=img, redraw_bbox=box, strength=0.05),                                       # no step would run
        dict(redraw_image=img, redraw_bbox=box, strength=1.5),
        dict(redraw_image=img, redraw_mask=torch.full((16, 16), 2.0)),
        dict(redraw_image_seeds=[1]),                                                                 # seeds without a picture
    ]
    for kw in cases:
        with pytest.raises(ValueError):
            call(**kw)
    # a VAE without an encoder (none at all, or one that decodes only)
    for vae in (None, types.SimpleNamespace(encoder=None, decode=None), types.SimpleNamespace(decode=None)):
        with pytest.raises(ValueError, match="encoder"):
            call(_pipe(vae), redraw_image=img, redraw_bbox=box, strength=0.6)
        with pytest.raises(ValueError, match="encoder"):
            _pipe(vae).encode_image(img)
    # every request of a batch is checked before the first picture is encoded
    ok = dict(prompt="p", height=128, width=128, num_inference_steps=10, redraw_image=img, redraw_bbox=box, strength=0.6)
    plain = dict(prompt="p", height=128, width=128, num_inference_steps=10)
    lat = dict(plain, redraw_latents=torch.zeros(1, 4, 16, 16), redraw_bbox=box, strength=0.6)
    for reqs in ([ok, plain], [ok, dict(ok, strength=0.3)], [ok, dict(ok, redraw_latents=torch.zeros(1, 4, 16, 16))],
                 [ok, dict(ok, redraw_image=Image.fromarray(np.zeros((64, 128, 3), dtype=np.uint8)))],
                 [ok, dict(ok, redraw_image_seeds=[3])], [dict(ok, strength=0.05)] * 2, [lat, dict(lat, redraw_image_seeds=[1])]):
        with pytest.raises(ValueError):
            pipe.generate_batch(reqs, output_type="latent")
    # what passes the checks reaches the VAE encoder (the stub) - and nothing else first
    for kw in (dict(redraw_image=img), dict(redraw_image=[img, img], num_samples=2), dict(redraw_image=np.zeros((128, 128, 3), dtype=np.uint8)),
               dict(redraw_image=torch.zeros(1, 128, 128, 3, dtype=torch.uint8)), dict(redraw_image=torch.rand(1, 3, 128, 128)),
               dict(redraw_image=img, redraw_image_seeds=[7])):
        with pytest.raises(AssertionError, match="VAE encoder ran"):
            call(redraw_bbox=box, strength=0.6, **kw)
    with pytest.raises(AssertionError, match="VAE encoder ran"):
        pipe.generate_batch([ok, dict(lat)], output_type="latent")          # a picture and kept latents share a batch


def test_image_tensor_forms():
    from PIL import Image
    from diffsensei_amd.pipeline import DiffSenseiPipeline as P
    rng = np.random.RandomState(0)
    a = rng.randint(0, 256, (16, 24, 3), dtype=np.uint8)
    for form in (Image.fromarray(a), [Image.fromarray(a)], a, a[None], torch.from_numpy(a), torch.from_numpy(a)[None]):
        t = P._image_tensor(form)
        assert t.dtype == torch.uint8 and t.shape == (1, 16, 24, 3) and np.array_equal(t[0].numpy(), a)
    t = P._image_tensor(Image.fromarray(a[..., 0]))                               # greyscale -> RGB
    assert t.shape == (1, 16, 24, 3) and np.array_equal(t[0, ..., 1].numpy(), a[..., 0])
    f = torch.rand(2, 3, 16, 24)
    t = P._image_tensor(f)
    assert t.dtype == torch.float32 and torch.equal(t, f * 2.0 - 1.0)
    t = P._image_tensor(f.half())
    assert t.dtype == torch.float32 and float(t.min()) >= -1 and float(t.max()) <= 1


def test_bucket_key_treats_redraw_image_like_redraw_latents():
    from PIL import Image
    from diffsensei_amd.serving import bucket_key, plan_batches
    img = Image.fromarray(np.zeros((512, 512, 3), dtype=np.uint8))
    plain = {"height": 512, "width": 512}
    assert bucket_key(plain) == (512, 512, 40, 5.0, 1.0)
    assert bucket_key(dict(plain, redraw_image=None)) == (512, 512, 40, 5.0, 1.0)
    rd = lambda s=None: dict(plain, redraw_image=img, redraw_bbox=[[0, 0, 1, 1]], **({} if s is None else {"strength": s}))
    assert bucket_key(rd()) == (512, 512, 40, 5.0, 1.0, ("redraw", 1.0))
    assert bucket_key(rd(0.5), mix_scales=True) == (512, 512, 40, True, ("redraw", 0.5))
    lat = dict(plain, redraw_latents=torch.zeros(1, 4, 64, 64), redraw_bbox=[[0, 0, 1, 1]], strength=0.5)
    assert bucket_key(lat) == bucket_key(rd(0.5))
    batches = plan_batches([plain, rd(0.5), lat, rd(1.0), dict(plain)], max_panels=8)
    assert sorted(sorted(b) for b in batches) == [[0, 4], [1, 2], [3]]
