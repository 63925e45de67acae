"""GPU: LoRA through `DiffSenseiPipeline` and the batching front end (the tiny pipeline of test_gpu_pipeline_variants.py,
3 steps, 128 x 128).

* `load_lora_weights` from a .safetensors file + `set_adapters` gives, bit for bit, the latents of a pipeline whose UNet was
  loaded with the merged weights (`ops.lora_merge`'s plain outputs); `unload_lora_weights` gives back the base latents.
* `BucketBatcher` with requests of two adapter states and some without the field: batches never mix states, each output
  equals its single-request run, and the pipeline's adapter state after `run()` is what it was before - also after an
  exception inside a batch.
"""
import pytest
import torch

from tests._lora_common import REFERENCE_LEAVES, fresh_route, make_adapter

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


def _pipeline(cfg, sd, clip, mae):
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.resampler import Resampler
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    from diffsensei_amd.unet import UNetMangaModel
    unet = UNetMangaModel(cfg, device=DEV)
    unet.load_state_dict(sd)
    rs = Resampler(dim=128, depth=2, dim_head=64, heads=2, num_queries=16, num_dummy_tokens=16, embedding_dim=160,
                   magi_embedding_dim=128, output_dim=cfg.cross_attention_dim, ff_mult=4, device=DEV).init_random(5)
    p = DiffSenseiPipeline(None, None, None, None, None, EulerDiscreteScheduler(), unet, clip)
    p.register_manga_modules(magi_image_encoder=mae, image_proj_model=rs)
    return p


@pytest.fixture(scope="module")
def parts(hip_lib):
    from transformers import CLIPVisionConfig, CLIPVisionModel, ViTMAEConfig, ViTMAEModel
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    torch.manual_seed(0)
    clip = CLIPVisionModel(CLIPVisionConfig(hidden_size=160, intermediate_size=320, num_hidden_layers=3,
                                            num_attention_heads=2, image_size=224, patch_size=14, hidden_act="quick_gelu")).eval()
    mae = ViTMAEModel(ViTMAEConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                                   image_size=224, patch_size=16, mask_ratio=0.0)).eval()
    cfg = tiny_config()
    sd = {k: v.half() for k, v in random_state_dict(cfg, 4).items()}
    a = make_adapter(cfg, 8, 1, fmt="peft_named", prefix="base_model.model.")
    b = make_adapter(cfg, 12, 2, keep=lambda m: m.endswith(REFERENCE_LEAVES), fmt="diffusers", prefix="unet.")
    return cfg, sd, clip, mae, a, b


def _request(cfg, seed, **kw):
    g = torch.Generator().manual_seed(seed)
    r = dict(prompt="a manga panel", height=128, width=128, num_inference_steps=3, guidance_scale=7.5,
             prompt_embeds=torch.randn(1, 77, cfg.cross_attention_dim, generator=g).half(),
             pooled_prompt_embeds=torch.randn(1, 128, generator=g).half(), latents=torch.randn(1, 4, 16, 16, generator=g).half(),
             ip_images=[], ip_bbox=[], dialog_bbox=[[0.0, 0.0, 0.3, 0.2]], ip_scale=0.6)
    r.update(kw)
    return r


_clone = lambda r: {k: (v.clone() if torch.is_tensor(v) else (list(v) if isinstance(v, list) else (dict(v) if isinstance(v, dict) else v)))
                    for k, v in r.items()}


def test_load_lora_weights_file_equals_premerged_unet(parts, tmp_path):
    from safetensors.torch import save_file
    cfg, sd, clip, mae, a, b = parts
    path = str(tmp_path / "style.safetensors")
    te = {"text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight": torch.zeros(4, 8)}
    save_file({k: v.contiguous() for k, v in {**a, **te}.items()}, path)
    p = _pipeline(cfg, sd, clip, mae)
    req = _request(cfg, 3)
    base = p(output_type="latent", **_clone(req)).images.clone()
    base_img = {k: v.clone() for k, v in p.unet.packed().w.items()}
    with pytest.raises(ValueError, match="text_encoder"):
        p.load_lora_weights(path, adapter_name="style")
    assert p.load_lora_weights(path, adapter_name="style", unet_only=True) == 1
    p.load_lora_weights(b, adapter_name="char")
    p.set_adapters(["style", "char"], [0.9, 0.5])
    got = p(output_type="latent", **_clone(req)).images.clone()
    pre = _pipeline(cfg, fresh_route(cfg, sd, [(a, 0.9), (b, 0.5)], DEV), clip, mae)
    want = pre(output_type="latent", **_clone(req)).images
    assert torch.equal(got, want)
    assert _rel(got, base) > 5e-2                                      # and that is not the base model
    p.unload_lora_weights()
    assert p.unet.active_adapters() == [] and p.unet.loaded_adapters() == []
    now = p.unet.packed().w                                            # the byte image of the packed weights is back
    assert set(now) == set(base_img) and all(torch.equal(now[k].view(torch.int16), base_img[k].view(torch.int16)) for k in base_img)
    assert torch.equal(p(output_type="latent", **_clone(req)).images, base)


def test_batcher_keeps_adapter_states_apart_and_restores(parts):
    from diffsensei_amd.serving import BucketBatcher
    cfg, sd, clip, mae, a, b = parts
    p = _pipeline(cfg, sd, clip, mae)
    p.load_lora_weights(a, adapter_name="style")
    p.load_lora_weights(b, adapter_name="char")
    reqs = [_request(cfg, 10, lora={"style": 1.0}), _request(cfg, 11), _request(cfg, 12, lora={"char": 0.5, "style": 0.25}),
            _request(cfg, 13, lora={}), _request(cfg, 14, lora={"style": 1.0}), _request(cfg, 15)]
    p.set_adapters(["char"], [0.75])                                   # what requests without the field run on
    single = []
    for r in reqs:
        r = _clone(r)
        st = r.pop("lora", None)
        if st is not None:
            p.set_adapters(list(st), list(st.values()))
        single.append(p(output_type="latent", **r).images.clone())
        p.set_adapters(["char"], [0.75])
    assert _rel(single[0], single[3]) > 5e-2 and _rel(single[1], single[3]) > 1e-2     # the states differ in the output
    bt = BucketBatcher(p, max_panels=1)                                # every request in a batch of its own: the single-request plan
    for r in reqs:
        bt.submit(**_clone(r))
    outs = bt.run(output_type="latent")
    assert p.unet.adapter_weights() == {"char": 0.75}
    for i, (o, s_) in enumerate(zip(outs, single)):
        assert torch.equal(o, s_), i
    calls = []
    real = p.unet.set_adapters
    p.unet.set_adapters = lambda names, weights=1.0: (calls.append(list(names)), real(names, weights))[1]
    bt = BucketBatcher(p, max_panels=8)                                # requests of one state share a UNet batch
    for r in reqs:
        bt.submit(**_clone(r))
    outs = bt.run(output_type="latent")
    assert sorted(map(sorted, bt.last_plan)) == [[0, 4], [1, 5], [2], [3]]
    p.unet.set_adapters = real
    # three states asked for + one switch for the batch without the field (it runs on the state from before the run);
    # the last of these is the restore: no set-and-restore pair per batch
    assert len(calls) <= 5, calls
    assert p.unet.adapter_weights() == {"char": 0.75}
    for i, (o, s_) in enumerate(zip(outs, single)):
        if i in (2, 3):
            assert torch.equal(o, s_), i
        else:
            # two requests in one UNet batch: another GEMM tiling, the fp16 noise floor of the existing batcher test
            assert _rel(o, s_) <= 2e-3, (i, _rel(o, s_))
    with pytest.raises(ValueError, match="lora"):
        p.generate_batch([_clone(reqs[0]), _clone(reqs[1])], output_type="latent")
    with pytest.raises(ValueError):
        p.generate_batch([dict(_clone(reqs[0]), lora={"nope": 1.0})], output_type="latent")
    with pytest.raises(TypeError):                                     # fails inside the batch, after the adapters were set
        p.generate_batch([dict(_clone(reqs[0]), no_such_field=1)], output_type="latent")
    assert p.unet.adapter_weights() == {"char": 0.75}
