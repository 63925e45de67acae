"""GPU: LoRA adapters on EVERY target of `UNetMangaModel` (tiny config, B = 2, 16 x 16 latents): a rank-8 adapter in the
underscore key form on every linear, conv1 / conv2 / conv_shortcut / time_emb_proj of every resnet and the four sampler
convolutions, and a rank-5 peft-named one on the convolutions alone.

* the merged forward meets the oracle on the fp32-merged weights at the gates of tests/test_gpu_lora_unet.py (5e-3; at
  least 5e-2 away from the oracle on the base weights), and the two fp32 oracles differ by tens of percent: a merge that
  does nothing cannot pass;
* in place == fresh: a second model loaded with `ops.lora_merge`'s own outputs (tests/_lora_full_common.fresh_route_full)
  has bit-identical packed tensors - the folded upsampler weights included - and forward output, eager and as a replay of
  a hipGraph captured BEFORE the switch; no packed pointer moves;
* `.weight.up2fold` after a merge is `ops.fold_upsample2x` of the merged packed weight;
* `set_adapters([])` gives back the byte image of every packed buffer, `.up2fold` included.
"""
import pytest
import torch

from tests._gates import gate
from tests._lora_full_common import fresh_route_full, make_full_adapter, merged_fp32_full
from tests.test_gpu_lora_unet import H, W, _assert_images_equal, _forward, _image, _model
from tests.test_gpu_unet import _inputs, _rel, hq

pytestmark = pytest.mark.gpu
DEV = "cuda"
UPS = ("up_blocks.0.upsamplers.0.conv", "up_blocks.1.upsamplers.0.conv")
WEIGHTS = [1.0, 0.7]


@pytest.fixture(scope="module")
def setup(hip_lib):
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    cfg = tiny_config()
    sd = {k: v.half() for k, v in random_state_dict(cfg, 0).items()}
    a = make_full_adapter(cfg, 8, 1, fmt="underscore")                                     # every target, old and new
    b = make_full_adapter(cfg, 5, 2, keep=lambda m: ".conv" in m or m.endswith(".conv"), fmt="peft")   # the convolutions
    model = _model(cfg, sd)
    inp = _inputs(cfg, 2, H, W)
    base_out = _forward(model, inp, graph=True)           # the forward plan is captured here, before any adapter exists
    assert torch.equal(base_out, _forward(model, inp))
    pk = model.packed()
    assert all(u + ".weight.up2fold" in pk.w for u in UPS), "the 16 x 16 forward runs both upsamplers folded"
    base_img = _image(model)
    model.load_lora_adapter(a, "a")
    model.load_lora_adapter(b, "b")
    # loading may give packed matrices that shared the state dict's storage a buffer of their own, once, and drops the engines
    # that named the old address; the plan every later switch has to survive is captured here, with no adapter active
    assert torch.equal(_forward(model, inp, graph=True), base_out)
    _assert_images_equal(_image(model), base_img, "loading an adapter changes no bit")
    return cfg, sd, a, b, model, inp, base_out, base_img


def test_adapters_cover_every_target(setup):
    from diffsensei_amd.lora import all_target_modules, target_modules
    cfg, sd, a, b, model, *_ = setup
    t = all_target_modules(cfg)
    assert set(model._lora.adapters["a"]) == set(t) and len(t) > len(target_modules(cfg))
    assert set(model._lora.adapters["b"]) == {m for m, s in t.items() if len(s) == 4}


def test_merged_forward_vs_oracle(setup):
    from oracle.unet_ref import UNetOracle
    cfg, sd, a, b, model, inp, base_out, base_img = setup
    x, enc, te, tid, bbox, db = inp
    ads = [(a, WEIGHTS[0]), (b, WEIGHTS[1])]
    merged, base = merged_fp32_full(cfg, sd, ads), merged_fp32_full(cfg, sd, [])
    oracles = [UNetOracle(cfg, merged, q=hq), UNetOracle(cfg, base, q=hq), UNetOracle(cfg, merged), UNetOracle(cfg, base)]
    for o in oracles:
        o.ip_scale = 0.6
    with torch.no_grad():
        r_merged, r_base, r32m, r32b = (o.forward(x, 801.0, enc, te, tid, bbox, H / W, db) for o in oracles)
    print(f"[lora full] fp32 oracle merged vs base: rel-L2 {_rel(r32m, r32b):.4g}")
    gate("LoRA on every layer, tiny UNet: fp32 oracle on merged vs on base weights (tens of percent)", _rel(r32m, r32b), 1e-1,
         lower=True)
    model.set_adapters(["a", "b"], WEIGHTS)
    out = _forward(model, inp)
    assert torch.isfinite(out).all()
    print(f"[lora full] merged in place vs oracle on merged weights: rel-L2 {_rel(out, r_merged):.4g}; vs base oracle {_rel(out, r_base):.4g}")
    gate("LoRA on every layer, tiny UNet 16x16, merged in place, vs fp16-storage oracle on the merged weights", _rel(out, r_merged), 5e-3)
    gate("LoRA on every layer, tiny UNet 16x16, merged in place, vs the oracle on the BASE weights (negative control)",
         _rel(out, r_base), 5e-2, lower=True)
    assert all(torch.equal(model.state_dict()[k].cpu(), sd[k]) for k in sd), "state_dict() must stay the base"


def test_in_place_equals_fresh_and_nothing_moves(setup):
    from diffsensei_amd import ops
    cfg, sd, a, b, model, inp, base_out, base_img = setup
    model.set_adapters([])
    eng, pk = model.engine(2, H, W, H / W), model.packed()
    assert eng.forward_plan.captured
    ptrs = {k: v.data_ptr() for k, v in pk.w.items()}
    model.set_adapters(["a", "b"], WEIGHTS)
    assert model.engine(2, H, W, H / W) is eng and model.packed() is pk and eng.forward_plan.captured
    assert {k: v.data_ptr() for k, v in pk.w.items()} == ptrs, "a packed buffer moved"
    fresh = _model(cfg, fresh_route_full(cfg, sd, [(a, WEIGHTS[0]), (b, WEIGHTS[1])], DEV))
    fresh_out = _forward(fresh, inp)
    got, want = _image(model), _image(fresh)
    assert all(u + ".weight.up2fold" in want for u in UPS)
    _assert_images_equal(got, want, "in place vs fresh pack")
    changed = [k for k in base_img if not torch.equal(got[k], base_img[k])]
    for leaf in ("conv1.weight", "conv2.weight", "conv_shortcut.weight", "downsamplers.0.conv.weight", "upsamplers.0.conv.weight",
                 "upsamplers.0.conv.weight.up2fold", "attn1.qk.weight", "ff.net.2.weight"):
        assert any(k.endswith(leaf) for k in changed), f"no {leaf} was rewritten"
    assert "temb_all.weight" in changed and "conv_in.weight" not in changed and "conv_out.weight" not in changed
    assert not any(k.endswith(".bias") and "_ln" not in k for k in changed)
    for u in UPS:                                             # the fold of the merged packed weight, by the native kernel
        assert torch.equal(pk.w[u + ".weight.up2fold"].view(torch.int16), ops.fold_upsample2x(pk.w[u + ".weight"]).view(torch.int16))
    out = _forward(model, inp)
    assert torch.equal(out, fresh_out) and not torch.equal(out, base_out)
    assert torch.equal(_forward(model, inp, graph=True), fresh_out), "replay of the graph captured before the switch"


def test_none_restores_every_buffer(setup):
    cfg, sd, a, b, model, inp, base_out, base_img = setup
    model.set_adapters(["a", "b"], WEIGHTS)
    assert not torch.equal(_forward(model, inp), base_out)
    model.set_adapters(["a", "b"], [0.0, 0.0])
    _assert_images_equal(_image(model), base_img, "weight 0")
    model.set_adapters(["b"], [1.0])                          # only convolutions: the linears stay the base
    img = _image(model)
    assert torch.equal(img["temb_all.weight"], base_img["temb_all.weight"])
    assert not torch.equal(img[UPS[0] + ".weight.up2fold"], base_img[UPS[0] + ".weight.up2fold"])
    model.set_adapters([])
    _assert_images_equal(_image(model), base_img, "set_adapters([])")
    assert set(_image(model)) == set(base_img)
    assert torch.equal(_forward(model, inp), base_out) and torch.equal(_forward(model, inp, graph=True), base_out)
