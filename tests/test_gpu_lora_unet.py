"""GPU: LoRA adapters on `UNetMangaModel` (tiny config, B = 2, 16 x 16 latents; a rank-8 adapter on every target kind and a
rank-12 one on the reference's four - to_q / to_k / to_v / to_out.0 - in the other key format).

* the merged forward meets the oracle on the merged fp32 weights at the tiny UNet's 5e-3 gate, and is at least 5e-2 away
  from the oracle on the base weights (the two fp32 oracles themselves differ by 0.1 - 0.3: checked first, on the CPU);
* in place == fresh: a second model loaded with `ops.lora_merge`'s plain outputs has bit-identical packed tensors and
  forward output, eager and as a hipGraph replay; engines and every packed pointer survive `set_adapters`;
* weight 0, `delete_adapters` and "no adapters" give back the byte image of the packed weights and the forward bits;
* new weights replay the cached merge plan; `load_state_dict` under an active adapter re-applies it;
* a model loaded from device tensors never writes into them; 320-row GEGLU copies follow a merge.
"""
import pytest
import torch

from tests._gates import gate
from tests._lora_common import REFERENCE_LEAVES, fresh_route, make_adapter, merged_fp32
from tests.test_gpu_unet import _inputs, _rel, hq

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = W = 16


def _model(cfg, sd):
    from diffsensei_amd.unet import UNetMangaModel
    m = UNetMangaModel(cfg, device=DEV)
    m.load_state_dict(sd)
    m._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    return m


def _forward(model, inp, graph=False):
    """One forward at t = 801; graph: the same request replayed from a capture of the engine's forward plan."""
    from diffsensei_amd import ops
    x, enc, te, tid, bbox, db = inp
    out = model(x.to(DEV), 801.0, enc.to(DEV), cross_attention_kwargs={"bbox": bbox, "aspect_ratio": H / W},
                added_cond_kwargs={"text_embeds": te, "time_ids": tid}, dialog_bbox=db).sample
    if not graph:
        return out.clone()
    eng = model.engine(x.shape[0], H, W, H / W)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        if not eng.forward_plan.captured:
            eng.forward_plan.capture(st.cuda_stream)
        eng.eps.zero_()
        eng.ctr.zero_()
        eng.forward_plan.replay(st.cuda_stream)
    st.synchronize()
    return ops.nhwc_to_nchw(eng.eps).reshape(out.shape).clone()


def _image(model):
    return {k: v.clone() for k, v in model.packed().w.items()}


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16) if a.dtype == torch.float16 else a, b.contiguous().view(torch.int16) if b.dtype == torch.float16 else b)


def _assert_images_equal(got, want, what):
    assert set(want) <= set(got), what
    bad = [k for k in want if not _same_bits(got[k], want[k])]
    assert not bad, f"{what}: {len(bad)} packed tensors differ, first {bad[:4]}"


@pytest.fixture(scope="module")
def setup(hip_lib):
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    cfg = tiny_config()
    sd = {k: v.half() for k, v in random_state_dict(cfg, 0).items()}
    a = make_adapter(cfg, 8, 1)                                                              # every target kind, peft names
    b = make_adapter(cfg, 12, 2, keep=lambda m: m.endswith(REFERENCE_LEAVES), fmt="diffusers", prefix="unet.")
    model = _model(cfg, sd)
    inp = _inputs(cfg, 2, H, W)
    base_out = _forward(model, inp)
    base_img = _image(model)
    model.load_lora_adapter(a, "a")
    model.load_lora_adapter(b, "b")
    return cfg, sd, a, b, model, inp, base_out, base_img


def _fresh(cfg, sd, adapters, inp):
    m = _model(cfg, fresh_route(cfg, sd, adapters, DEV))
    return m, _forward(m, inp)


def test_merged_forward_vs_oracle(setup):
    from oracle.unet_ref import UNetOracle
    cfg, sd, a, b, model, inp, base_out, base_img = setup
    x, enc, te, tid, bbox, db = inp
    ads = [(a, 1.0), (b, 0.7)]
    o_merged, o_base32 = UNetOracle(cfg, merged_fp32(cfg, sd, ads), q=hq), UNetOracle(cfg, merged_fp32(cfg, sd, []))
    o_merged32, o_base = UNetOracle(cfg, merged_fp32(cfg, sd, ads)), UNetOracle(cfg, merged_fp32(cfg, sd, []), q=hq)
    for o in (o_merged, o_base32, o_merged32, o_base):
        o.ip_scale = 0.6
    with torch.no_grad():
        r_merged, r_base = (o.forward(x, 801.0, enc, te, tid, bbox, H / W, db) for o in (o_merged, o_base))
        r32m, r32b = (o.forward(x, 801.0, enc, te, tid, bbox, H / W, db) for o in (o_merged32, o_base32))
    gate("LoRA tiny UNet: fp32 oracle on merged vs on base weights (the adapters matter)", _rel(r32m, r32b), 5e-2, lower=True)
    model.set_adapters(["a", "b"], [1.0, 0.7])
    assert model.active_adapters() == ["a", "b"] and model.adapter_weights() == {"a": 1.0, "b": 0.7}
    out = _forward(model, inp)
    assert torch.isfinite(out).all()
    gate("LoRA tiny UNet 16x16, adapters merged in place, vs fp16-storage oracle on the merged weights", _rel(out, r_merged), 5e-3)
    gate("LoRA tiny UNet 16x16, adapters merged in place, vs the oracle on the BASE weights (negative control)",
         _rel(out, r_base), 5e-2, lower=True)
    assert set(model.state_dict()) == set(sd) and all(torch.equal(model.state_dict()[k].cpu(), sd[k]) for k in sd), \
        "state_dict() must stay the base"


def test_in_place_equals_fresh(setup):
    cfg, sd, a, b, model, inp, base_out, base_img = setup
    model.set_adapters([])
    eng = model.engine(2, H, W, H / W)
    ptrs = {k: v.data_ptr() for k, v in model.packed().w.items()}
    pk = model.packed()
    model.set_adapters(["a", "b"], [1.0, 0.7])
    assert model.engine(2, H, W, H / W) is eng and model.packed() is pk
    assert {k: v.data_ptr() for k, v in model.packed().w.items()} == ptrs
    fresh, fresh_out = _fresh(cfg, sd, [(a, 1.0), (b, 0.7)], inp)
    _assert_images_equal(_image(model), _image(fresh), "in place vs fresh pack")
    out = _forward(model, inp)
    assert torch.equal(out, fresh_out)
    assert torch.equal(_forward(model, inp, graph=True), fresh_out), "hipGraph replay after an in-place merge"
    assert not torch.equal(out, base_out)
    # the captured graph survives the next switch as well: same engine, new weights
    model.set_adapters(["b"], [1.0])
    assert model.engine(2, H, W, H / W) is eng and eng.forward_plan.captured
    _, fresh_b = _fresh(cfg, sd, [(b, 1.0)], inp)
    assert torch.equal(_forward(model, inp, graph=True), fresh_b)      # `a`'s matrices went back to the base


def test_zero_weight_delete_and_none_restore_the_base(setup):
    cfg, sd, a, b, model, inp, base_out, base_img = setup
    model.set_adapters(["a", "b"], [1.0, 0.7])
    assert not torch.equal(_forward(model, inp), base_out)
    model.set_adapters(["a", "b"], [0.0, 0.0])
    _assert_images_equal(_image(model), base_img, "weight 0")
    assert torch.equal(_forward(model, inp), base_out)
    model.set_adapters(["a", "b"], [1.0, 0.7])
    model.set_adapters([])
    _assert_images_equal(_image(model), base_img, "set_adapters([])")
    assert torch.equal(_forward(model, inp), base_out)
    model.load_lora_adapter(make_adapter(cfg, 5, 3), "c")
    model.set_adapters(["c", "b"], [1.0, 1.0])
    assert not torch.equal(_forward(model, inp), base_out)
    model.delete_adapters("c")
    assert model.active_adapters() == ["b"] and "c" not in model.loaded_adapters()
    _, fresh_b = _fresh(cfg, sd, [(b, 1.0)], inp)
    assert torch.equal(_forward(model, inp), fresh_b)
    model.delete_adapters(["b"])
    _assert_images_equal(_image(model), base_img, "delete_adapters")
    assert torch.equal(_forward(model, inp), base_out)
    model.load_lora_adapter(b, "b")                                   # the module fixture keeps both loaded


def test_new_weights_replay_the_cached_plan(setup):
    cfg, sd, a, b, model, inp, base_out, base_img = setup
    model.set_adapters(["a", "b"], [1.0, 0.7])
    plan = model._lora.last_plan
    n_plans = len(model._lora.plans)
    model.set_adapters(["a", "b"], [0.4, -0.6])
    assert model._lora.last_plan is plan and len(model._lora.plans) == n_plans, "new weights must not build a new plan"
    fresh, fresh_out = _fresh(cfg, sd, [(a, 0.4), (b, -0.6)], inp)
    _assert_images_equal(_image(model), _image(fresh), "new weights, cached plan")
    assert torch.equal(_forward(model, inp), fresh_out)


def test_load_state_dict_under_an_active_adapter(setup):
    from diffsensei_amd.unet_config import random_state_dict
    cfg, sd, a, b, model, inp, base_out, base_img = setup
    model.set_adapters(["a"], [0.8])
    sd2 = {k: v.half() for k, v in random_state_dict(cfg, 7).items()}
    try:
        model.load_state_dict(sd2)
        assert model.active_adapters() == ["a"]
        out = _forward(model, inp)
        _, fresh_out = _fresh(cfg, sd2, [(a, 0.8)], inp)
        assert torch.equal(out, fresh_out)
        model.set_adapters([])
        assert torch.equal(_forward(model, inp), _forward(_model(cfg, sd2), inp))
    finally:
        model.load_state_dict(sd)
        model.set_adapters([])


def test_callers_tensors_are_never_written(hip_lib):
    """A model loaded from DEVICE tensors packs several target matrices as they lie, sharing the caller's storage.  Neither the
    caller's tensors, nor a `state_dict()` taken before the merge, nor a second model loaded from the same tensors may see
    the merged values."""
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    cfg = tiny_config()
    host = {k: v.half() for k, v in random_state_dict(cfg, 0).items()}
    dev_sd = {k: v.to(DEV) for k, v in host.items()}
    inp = _inputs(cfg, 2, H, W)
    first, second = _model(cfg, dev_sd), _model(cfg, dev_sd)
    base_out = _forward(second, inp)
    _forward(first, inp)                                   # packed and an engine built BEFORE the adapter is loaded
    early = first.state_dict()
    first.load_lora_adapter(make_adapter(cfg, 8, 1), "a")
    eng = first.engine(2, H, W, H / W)
    first.set_adapters("a")
    assert first.engine(2, H, W, H / W) is eng             # loading may move buffers once; set_adapters never does
    out = _forward(first, inp)
    assert not torch.equal(out, base_out)
    for k, v in host.items():
        assert torch.equal(dev_sd[k].cpu(), v), f"the caller's tensor {k} was overwritten"
        assert torch.equal(early[k].cpu(), v) and torch.equal(first.state_dict()[k].cpu(), v), k
    assert torch.equal(_forward(second, inp), base_out), "a second model on the same tensors runs the first one's adapter"
    _, fresh_out = _fresh(cfg, host, [(make_adapter(cfg, 8, 1), 1.0)], inp)
    assert torch.equal(out, fresh_out)


def test_g320_copies_follow_the_merge(hip_lib):
    """The 320-row GEGLU copies exist only where a plan asked for them (batch-1 requests at the 1280-channel level); made by
    hand here on a config whose GEGLU half (4 x 320) takes that packing, they must follow a merge and a reset like a fresh
    re-pack of the merged 128-row packing."""
    from diffsensei_amd.engine import pack_geglu320, unpack_geglu
    from diffsensei_amd.unet_config import UNetMangaConfig, random_state_dict, tiny_config
    t0 = tiny_config()
    cfg = UNetMangaConfig(block_out_channels=(64, 128, 320), transformer_layers_per_block=(1, 1, 1), attention_head_dim=(1, 2, 5),
                          cross_attention_dim=t0.cross_attention_dim, addition_time_embed_dim=t0.addition_time_embed_dim,
                          projection_class_embeddings_input_dim=t0.projection_class_embeddings_input_dim, sample_size=16)
    sd = {k: v.half() for k, v in random_state_dict(cfg, 0).items()}
    model = _model(cfg, sd)
    pk = model.packed()
    t = "mid_block.attentions.0.transformer_blocks.0"
    for ln in (False, True) if f"{t}.ff.net.0.proj.weight_ln" in pk.w else (False,):
        pk.geglu320(t, ln)
    keys = [k for k in pk.w if k.startswith(t) and k.endswith(".g320")]
    assert keys
    before = {k: pk.w[k].clone() for k in keys}
    ptrs = {k: pk.w[k].data_ptr() for k in keys}
    model.load_lora_adapter(make_adapter(cfg, 8, 1, keep=lambda m: m.startswith(t)), "a")
    model.set_adapters("a")
    assert model.packed() is pk and {k: pk.w[k].data_ptr() for k in keys} == ptrs
    for k in keys:
        want = pack_geglu320(unpack_geglu(pk.w[k[:-len(".g320")]]))
        assert torch.equal(pk.w[k], want), k
    assert not torch.equal(pk.w[f"{t}.ff.net.0.proj.weight.g320"], before[f"{t}.ff.net.0.proj.weight.g320"])
    model.set_adapters([])
    for k in keys:
        assert torch.equal(pk.w[k].view(torch.int16), before[k].view(torch.int16)), k
