"""Host side of the LoRA adapters (no GPU): key parsing and refusals of `lora.parse_lora_state_dict`, the split of the
reference's `ckpt.pth["unet_trained"]`, and the serving key - requests without `lora` keep today's bucket keys, literally."""
import pytest
import torch

from diffsensei_amd.lora import (drop_text_encoder_keys, parse_lora_state_dict, split_reference_ckpt, target_modules)
from diffsensei_amd.serving import bucket_key, plan_batches
from diffsensei_amd.unet_config import tiny_config

CFG = tiny_config()
T0 = "down_blocks.1.attentions.0.transformer_blocks.0"
Q, KX, FF, PIN = f"{T0}.attn1.to_q", f"{T0}.attn2.to_k", f"{T0}.ff.net.0.proj", "down_blocks.1.attentions.0.proj_in"


def _ab(module, r, seed=0):
    N, K = target_modules(CFG)[module]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(r, K, generator=g) * 0.02, torch.randn(N, r, generator=g) * 0.02


def test_targets_are_the_transformer_block_linears():
    t = target_modules(CFG)
    assert t[Q] == (128, 128) and t[KX] == (128, 256) and t[FF] == (1024, 128) and t[PIN] == (128, 128)
    assert all(".attentions." in m for m in t)
    per_block = 10
    blocks = sum(1 for m in t if m.endswith("attn1.to_q"))
    assert len(t) == blocks * per_block + 2 * sum(1 for m in t if m.endswith(".proj_in"))


@pytest.mark.parametrize("down,up", [("lora_A.weight", "lora_B.weight"), ("lora_A.default.weight", "lora_B.default.weight"),
                                     ("lora.down.weight", "lora.up.weight")])
@pytest.mark.parametrize("prefix", ["", "unet.", "base_model.model.", "base_model.model.unet."])
def test_key_forms_and_prefixes(down, up, prefix):
    sd = {}
    want = {}
    for i, (m, r) in enumerate([(Q, 4), (KX, 8), (FF, 12), (PIN, 3)]):
        A, B = _ab(m, r, i)
        sd[f"{prefix}{m}.{down}"], sd[f"{prefix}{m}.{up}"] = A, B
        want[m] = (A, B, r)
    got = parse_lora_state_dict(sd, cfg=CFG)
    assert set(got) == set(want)
    for m, (A, B, r) in want.items():
        a, b, alpha = got[m]
        assert a.dtype == b.dtype == torch.float16 and alpha == float(r)      # alpha defaults to the rank
        assert torch.equal(a, A.half()) and torch.equal(b, B.half())


def test_alpha_key_argument_default():
    A, B = _ab(Q, 8)
    sd = {f"{Q}.lora_A.weight": A, f"{Q}.lora_B.weight": B}
    assert parse_lora_state_dict(sd, cfg=CFG)[Q][2] == 8.0
    sd[f"{Q}.alpha"] = torch.tensor(4.0)
    assert parse_lora_state_dict(sd, cfg=CFG)[Q][2] == 4.0
    assert parse_lora_state_dict(sd, alpha=16, cfg=CFG)[Q][2] == 16.0          # the argument wins


OFFENDERS = [
    "down_blocks.1.resnets.0.conv1.lora_A.weight",                             # a convolution
    "time_embedding.linear_1.lora_A.weight",                                   # time embedding
    f"{T0}.attn2.processor.to_k_ip.lora_A.weight",                             # IP projections
    f"{T0}.attn1.processor.to_q_lora.down.weight",                             # processor-era names
    "lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q.lora_down.weight",   # kohya
    "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight",
    f"{Q}.weight",                                                             # not an adapter key at all
]


@pytest.mark.parametrize("key", OFFENDERS)
def test_everything_else_is_refused_by_name(key):
    A, B = _ab(Q, 4)
    sd = {f"{Q}.lora_A.weight": A, f"{Q}.lora_B.weight": B, key: torch.zeros(4, 4)}
    with pytest.raises(ValueError) as e:
        parse_lora_state_dict(sd, cfg=CFG)
    assert key in str(e.value)


def test_text_encoder_keys_are_dropped_only_on_request():
    A, B = _ab(Q, 4)
    sd = {f"unet.{Q}.lora_A.weight": A, f"unet.{Q}.lora_B.weight": B,
          "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight": torch.zeros(4, 8),
          "text_encoder_2.text_model.encoder.layers.0.self_attn.q_proj.lora_B.weight": torch.zeros(8, 4)}
    with pytest.raises(ValueError, match="text_encoder"):
        parse_lora_state_dict(sd, cfg=CFG)
    kept, n = drop_text_encoder_keys(sd)
    assert n == 2 and set(parse_lora_state_dict(kept, cfg=CFG)) == {Q}


def test_wrong_shapes_nonfinite_and_unpaired_are_refused():
    A, B = _ab(Q, 4)
    with pytest.raises(ValueError, match=Q):
        parse_lora_state_dict({f"{Q}.lora_A.weight": A[:, :-8], f"{Q}.lora_B.weight": B}, cfg=CFG)
    with pytest.raises(ValueError, match=Q):
        parse_lora_state_dict({f"{Q}.lora_A.weight": A, f"{Q}.lora_B.weight": B[:, :3]}, cfg=CFG)
    with pytest.raises(ValueError, match=Q):                                   # transposed: B where A belongs
        parse_lora_state_dict({f"{Q}.lora_A.weight": B, f"{Q}.lora_B.weight": A}, cfg=CFG)
    bad = A.clone()
    bad[1, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        parse_lora_state_dict({f"{Q}.lora_A.weight": bad, f"{Q}.lora_B.weight": B}, cfg=CFG)
    big = B.clone()
    big[0, 0] = 1e6                                                            # finite in fp32, inf in the inference dtype
    with pytest.raises(ValueError, match="non-finite"):
        parse_lora_state_dict({f"{Q}.lora_A.weight": A, f"{Q}.lora_B.weight": big}, cfg=CFG)
    with pytest.raises(ValueError, match=Q):
        parse_lora_state_dict({f"{Q}.lora_A.weight": A}, cfg=CFG)
    Ar, Br = torch.zeros(257, 128), torch.zeros(128, 257)
    with pytest.raises(ValueError, match="rank"):
        parse_lora_state_dict({f"{Q}.lora_A.weight": Ar, f"{Q}.lora_B.weight": Br}, cfg=CFG)
    with pytest.raises(ValueError, match="more than one adapter"):
        parse_lora_state_dict({f"{Q}.lora_A.a.weight": A, f"{Q}.lora_B.b.weight": B}, cfg=CFG)
    with pytest.raises(ValueError, match="empty"):
        parse_lora_state_dict({}, cfg=CFG)


def test_split_reference_ckpt():
    """The names `unet.named_parameters()` gives after peft's `add_adapter` on to_k / to_q / to_v / to_out.0, plus the
    trainable IP projections (reference scripts/train/train.py:163-165, 195-214)."""
    trained = {}
    for leaf in ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0"):
        A, B = _ab(f"{T0}.{leaf}", 8)
        trained[f"{T0}.{leaf}.lora_A.default.weight"], trained[f"{T0}.{leaf}.lora_B.default.weight"] = A, B
    trained[f"{T0}.attn2.processor.to_k_ip.weight"] = torch.randn(128, 256)
    trained[f"{T0}.attn2.processor.to_v_ip.weight"] = torch.randn(128, 256)
    plain, lora = split_reference_ckpt(trained)
    assert set(plain) == {f"{T0}.attn2.processor.to_k_ip.weight", f"{T0}.attn2.processor.to_v_ip.weight"}
    assert len(lora) == 16
    parsed = parse_lora_state_dict(lora, cfg=CFG)
    assert len(parsed) == 8 and all(v[2] == 8.0 for v in parsed.values())
    from diffsensei_amd.unet_config import param_shapes
    assert all(k in param_shapes(CFG) for k in plain)                          # goes to load_state_dict(strict=False)


def test_model_bookkeeping_without_a_device():
    from diffsensei_amd.unet import UNetMangaModel
    unet = UNetMangaModel(CFG, device="cpu")
    A, B = _ab(Q, 4)
    unet.load_lora_adapter({f"{Q}.lora_A.weight": A, f"{Q}.lora_B.weight": B}, "style")
    with pytest.raises(ValueError, match="already loaded"):
        unet.load_lora_adapter({f"{Q}.lora_A.weight": A, f"{Q}.lora_B.weight": B}, "style")
    with pytest.raises(ValueError, match="not loaded"):
        unet.set_adapters(["other"])
    with pytest.raises(ValueError, match="weights"):
        unet.set_adapters(["style"], [1.0, 2.0])
    unet.set_adapters("style", 0.5)
    assert unet.active_adapters() == ["style"] and unet.adapter_weights() == {"style": 0.5}
    unet.delete_adapters("style")
    assert unet.active_adapters() == [] and unet.loaded_adapters() == []


# ---- serving
def test_bucket_key_without_lora_is_what_it_was():
    r = dict(height=1024, width=768, num_inference_steps=30, guidance_scale=7.5, ip_scale=0.6)
    assert bucket_key(r) == (1024, 768, 30, 7.5, 0.6)
    assert bucket_key(r, True) == (1024, 768, 30, True)
    assert bucket_key({}) == (None, None, 40, 5.0, 1.0)
    rd = dict(r, redraw_latents=object(), strength=0.5)
    assert bucket_key(rd) == (1024, 768, 30, 7.5, 0.6, ("redraw", 0.5))
    assert bucket_key(rd, True) == (1024, 768, 30, True, ("redraw", 0.5))


def test_bucket_key_with_lora():
    r = dict(height=512, width=512)
    a = bucket_key(dict(r, lora={"style": 1.0}))
    assert a == (512, 512, 40, 5.0, 1.0, ("lora", (("style", 1.0),)))
    assert bucket_key(dict(r, lora={})) == (512, 512, 40, 5.0, 1.0, ("lora", ()))
    assert bucket_key(dict(r, lora={"b": 0.5, "a": 1})) == bucket_key(dict(r, lora={"a": 1.0, "b": 0.5}))   # order-free
    keys = {bucket_key(x) for x in (r, dict(r, lora={}), dict(r, lora={"style": 1.0}), dict(r, lora={"style": 0.5}),
                                    dict(r, lora={"other": 1.0}), dict(r, lora={"style": 1.0, "other": 1.0}))}
    assert len(keys) == 6
    rd = dict(r, redraw_latents=object(), strength=0.5, lora={"style": 1.0})
    assert bucket_key(rd, True) == (512, 512, 40, True, ("redraw", 0.5), ("lora", (("style", 1.0),)))


def test_plan_batches_never_mixes_adapter_states():
    states = [None, {"a": 1.0}, {}, {"a": 1.0}, None, {"a": 0.5}, {"b": 1.0}, {"a": 1.0}, {}]
    reqs = [dict(height=512, width=512) if s is None else dict(height=512, width=512, lora=s) for s in states]
    for mix in (False, True):
        batches = plan_batches(reqs, max_panels=32, mix_scales=mix)
        assert sorted(i for b in batches for i in b) == list(range(len(reqs)))
        for b in batches:
            assert len({repr(states[i]) for i in b}) == 1
        assert len(batches) == 5
