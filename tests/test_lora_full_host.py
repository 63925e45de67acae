"""Host side of LoRA on every UNet layer (no GPU): the full target list of `lora.all_target_modules`, the three key forms
(peft, diffusers, underscore `lora_unet_...`), the underscore table, and every refusal by key."""
import pytest
import torch

from diffsensei_amd.lora import (all_target_modules, pack_conv_down, parse_lora_state_dict, target_modules, underscore_table)
from diffsensei_amd.unet_config import build_topology, param_shapes, sdxl_config, tiny_config

CONFIGS = {"tiny": tiny_config(), "sdxl": sdxl_config()}
CFG = CONFIGS["tiny"]
R0 = "down_blocks.1.resnets.0"                       # 64 -> 128: has a shortcut
CONV1, CONV2, SHORT, TEMB = f"{R0}.conv1", f"{R0}.conv2", f"{R0}.conv_shortcut", f"{R0}.time_emb_proj"
DOWN, UP = "down_blocks.0.downsamplers.0.conv", "up_blocks.0.upsamplers.0.conv"
Q = "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"
NEW = [CONV1, CONV2, SHORT, TEMB, DOWN, UP]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_new_target_appears_with_its_shape(name):
    cfg = CONFIGS[name]
    t, shapes, topo = all_target_modules(cfg), param_shapes(cfg), build_topology(cfg)
    old = target_modules(cfg)
    assert list(t)[:len(old)] == list(old) and all(t[m] == old[m] for m in old)       # the linears first, as they were
    new = {m: s for m, s in t.items() if m not in old}
    resnets = [r for blk in list(topo.down) + [topo.mid] + list(topo.up) for r in blk["resnets"]]
    want = {}
    for r in resnets:
        want[f"{r.prefix}.conv1"] = (r.cout, r.cin, 3, 3)
        want[f"{r.prefix}.conv2"] = (r.cout, r.cout, 3, 3)
        want[f"{r.prefix}.time_emb_proj"] = (r.cout, cfg.time_embed_dim)
        if r.has_shortcut:
            want[f"{r.prefix}.conv_shortcut"] = (r.cout, r.cin, 1, 1)
    for blk in topo.down:
        if blk["downsample"]:
            c = blk["resnets"][-1].cout
            want[blk["downsample"]] = (c, c, 3, 3)
    for blk in topo.up:
        if blk["upsample"]:
            c = blk["resnets"][-1].cout
            want[blk["upsample"]] = (c, c, 3, 3)
    assert new == want
    assert all(tuple(shapes[m + ".weight"]) == s for m, s in t.items())
    assert sum(1 for m in new if m.endswith(("downsamplers.0.conv", "upsamplers.0.conv"))) == 4
    # what the kernel's convolution mode needs, at every target of both configs
    assert all(s[0] % 8 == 0 and s[1] % 8 == 0 for s in t.values())
    if name == "tiny":
        assert t[CONV1] == (128, 64, 3, 3) and t[CONV2] == (128, 128, 3, 3) and t[SHORT] == (128, 64, 1, 1)
        assert t[TEMB] == (128, cfg.time_embed_dim) and t[DOWN] == (64, 64, 3, 3) and t[UP] == (256, 256, 3, 3)
        assert t["up_blocks.0.resnets.0.conv1"] == (256, 512, 3, 3)                    # concatenated input
    for m in ("conv_in", "conv_out", "time_embedding.linear_1", "time_embedding.linear_2", "add_embedding.linear_1",
              "add_embedding.linear_2", "conv_norm_out", f"{R0}.norm1", f"{R0}.norm2"):
        assert m not in t
    assert not any("to_k_ip" in m or "to_v_ip" in m or "dialog" in m or ".norm" in m for m in t)


def test_target_modules_is_unchanged():
    t = target_modules(CFG)
    assert all(".attentions." in m and len(s) == 2 for m, s in t.items())
    assert t[Q] == (128, 128) and CONV1 not in t and TEMB not in t
    blocks = sum(1 for m in t if m.endswith("attn1.to_q"))
    assert len(t) == blocks * 10 + 2 * sum(1 for m in t if m.endswith(".proj_in"))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_underscore_table_is_collision_free(name):
    cfg = CONFIGS[name]
    t = all_target_modules(cfg)
    table = underscore_table(cfg)
    assert len(table) == len(t) and set(table.values()) == set(t)
    assert all(u == m.replace(".", "_") and "." not in u for u, m in table.items())
    assert table["down_blocks_1_resnets_0_conv_shortcut"] == SHORT
    assert table["down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_out_0"].endswith("attn1.to_out.0")


def _ab(module, r, seed=0, b4=False):
    shp = all_target_modules(CFG)[module]
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(r, *shp[1:], generator=g) * 0.02
    B = torch.randn(shp[0], r, generator=g) * 0.02
    return A, (B[:, :, None, None] if b4 and len(shp) == 4 else B)


FORMS = {"peft": lambda m: (f"{m}.lora_A.weight", f"{m}.lora_B.weight", f"{m}.alpha"),
         "peft_named": lambda m: (f"base_model.model.{m}.lora_A.default.weight", f"base_model.model.{m}.lora_B.default.weight",
                                  f"base_model.model.{m}.alpha"),
         "diffusers": lambda m: (f"unet.{m}.lora.down.weight", f"unet.{m}.lora.up.weight", f"unet.{m}.alpha"),
         "underscore": lambda m: tuple(f"lora_unet_{m.replace('.', '_')}.{s}" for s in ("lora_down.weight", "lora_up.weight", "alpha"))}


def test_the_three_name_forms_parse_to_the_same_adapter():
    mods = [(Q, 4), (CONV1, 8), (CONV2, 3), (SHORT, 5), (TEMB, 6), (DOWN, 2), (UP, 7)]
    parsed = {}
    for form, names in FORMS.items():
        sd = {}
        for i, (m, r) in enumerate(mods):
            A, B = _ab(m, r, i, b4=form in ("diffusers", "underscore"))          # [Cout, r, 1, 1] and [Cout, r] are both accepted
            down, up, alpha = names(m)
            sd[down], sd[up], sd[alpha] = A, B, torch.tensor(r / 2)
        parsed[form] = parse_lora_state_dict(sd, cfg=CFG)
    first = parsed["peft"]
    assert set(first) == {m for m, _ in mods}
    for i, (m, r) in enumerate(mods):
        A, B = _ab(m, r, i)
        a, b, alpha = first[m]
        assert a.dtype == b.dtype == torch.float16 and alpha == r / 2
        assert torch.equal(a, A.half()) and torch.equal(b, B.half()) and b.dim() == 2
        assert a.dim() == (4 if m in (CONV1, CONV2, SHORT, DOWN, UP) else 2)
    for form, got in parsed.items():
        assert set(got) == set(first), form
        for m in first:
            assert torch.equal(got[m][0], first[m][0]) and torch.equal(got[m][1], first[m][1]) and got[m][2] == first[m][2], (form, m)
    # the down matrix in the packed order: k = (ky * 3 + kx) * Cin + ci, and the product is the checkpoint-order delta, packed
    from diffsensei_amd.engine import pack_conv3x3
    A, B, _ = first[CONV1]
    Ap = pack_conv_down(A)
    assert Ap.shape == (8, 9 * 64) and Ap[3, (1 * 3 + 2) * 64 + 5] == A[3, 5, 1, 2]
    delta = torch.einsum("or,rikl->oikl", B.double(), A.double())
    assert torch.equal(pack_conv3x3(delta), B.double() @ Ap.double())
    assert pack_conv_down(first[SHORT][0]).shape == (5, 64) and pack_conv_down(first[Q][0]) is first[Q][0]


def _pair(m=CONV1, r=4):
    A, B = _ab(m, r)
    return {f"{m}.lora_A.weight": A, f"{m}.lora_B.weight": B}


REFUSED_KEYS = [
    "conv_in.lora_A.weight", "conv_out.lora_B.weight", "time_embedding.linear_1.lora_A.weight",
    "add_embedding.linear_2.lora_A.weight", f"{R0}.norm1.lora_A.weight", "conv_norm_out.lora_A.weight",
    "down_blocks.1.attentions.0.transformer_blocks.0.attn2.processor.to_k_ip.lora_A.weight",
    "dialog_bbox_embedding.lora_A.weight", "lora_unet_conv_in.lora_down.weight",
    "lora_unet_down_blocks_1_resnets_0_norm1.lora_down.weight", "lora_unet_down_blocks_9_resnets_0_conv1.lora_down.weight",
    "lora_unet_down_blocks_1_resnets_0_conv1.weight",
    # other adapter families, on a layer that IS a target
    "lora_unet_down_blocks_1_resnets_0_conv1.lora_mid.weight", "lora_unet_down_blocks_1_resnets_0_conv1.hada_w1_a",
    "lora_unet_down_blocks_1_resnets_0_conv1.hada_w2_b", "lora_unet_down_blocks_1_resnets_0_conv1.lokr_w1",
    "lora_unet_down_blocks_1_resnets_0_conv1.dora_scale", f"{CONV2}.lora_magnitude_vector.weight",
    # the SGM block naming
    "lora_unet_input_blocks_4_0_in_layers_2.lora_down.weight", "lora_unet_middle_block_0_out_layers_3.lora_up.weight",
    "lora_unet_output_blocks_2_0_skip_connection.alpha",
]


@pytest.mark.parametrize("key", REFUSED_KEYS)
def test_refusals_name_the_key(key):
    sd = dict(_pair(), **{key: torch.zeros(4, 4)})
    with pytest.raises(ValueError) as e:
        parse_lora_state_dict(sd, cfg=CFG)
    assert key in str(e.value)
    if "input_blocks" in key or "middle_block" in key or "output_blocks" in key:
        assert "SGM" in str(e.value)


def test_unpaired_halves_and_misfitting_shapes_name_their_keys():
    A, B = _ab(CONV1, 4)
    for lone in (f"{CONV1}.lora_A.weight", f"lora_unet_{CONV1.replace('.', '_')}.lora_up.weight", f"{TEMB}.alpha"):
        with pytest.raises(ValueError) as e:
            parse_lora_state_dict(dict(_pair(Q), **{lone: A}) if "alpha" not in lone else dict(_pair(Q), **{lone: torch.tensor(1.0)}), cfg=CFG)
        assert lone in str(e.value)
    dk, uk = f"{CONV1}.lora_A.weight", f"{CONV1}.lora_B.weight"
    bad = [
        (A[:, :, :1, :1].contiguous(), B),                # a 1x1 down matrix on a 3x3 layer
        (A.reshape(4, -1), B),                            # flattened
        (A[:, :-8], B),                                   # wrong Cin
        (A, B[:-8]),                                      # wrong Cout
        (A, B[:, :3]),                                    # ranks differ
        (A, B[:, :, None, None].expand(-1, -1, 3, 3)),    # the up matrix must be 1x1
        (B, A),                                           # swapped
    ]
    for a, b in bad:
        with pytest.raises(ValueError) as e:
            parse_lora_state_dict({dk: a, uk: b}, cfg=CFG)
        assert CONV1 in str(e.value) and dk in str(e.value)
    As, Bs = _ab(SHORT, 4)
    with pytest.raises(ValueError, match=SHORT):          # a 3x3 down matrix on the 1x1 shortcut
        parse_lora_state_dict({f"{SHORT}.lora_A.weight": As.expand(-1, -1, 3, 3), f"{SHORT}.lora_B.weight": Bs}, cfg=CFG)
    parse_lora_state_dict({f"{SHORT}.lora_A.weight": As, f"{SHORT}.lora_B.weight": Bs}, cfg=CFG)
    with pytest.raises(ValueError, match="more than one adapter"):
        parse_lora_state_dict(dict(_pair(), **{f"lora_unet_{CONV1.replace('.', '_')}.lora_down.weight": A}), cfg=CFG)


def test_text_encoder_keys_still_go_through_the_drop():
    from diffsensei_amd.lora import drop_text_encoder_keys
    sd = dict(_pair(), **{"lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": torch.zeros(4, 8),
                          "lora_te2_text_model_encoder_layers_0_mlp_fc1.lora_up.weight": torch.zeros(8, 4)})
    with pytest.raises(ValueError, match="lora_te1"):
        parse_lora_state_dict(sd, cfg=CFG)
    kept, n = drop_text_encoder_keys(sd)
    assert n == 2 and set(parse_lora_state_dict(kept, cfg=CFG)) == {CONV1}


def test_model_holds_convolution_adapters_kernel_ready():
    from diffsensei_amd.unet import UNetMangaModel
    unet = UNetMangaModel(CFG, device="cpu")
    unet.load_lora_adapter(dict(_pair(CONV1, 4), **_pair(TEMB, 2)), "style")
    ad = unet._lora.adapters["style"]
    assert ad[CONV1][0].shape == (4, 9 * 64) and ad[CONV1][1].shape == (128, 4) and ad[TEMB][0].shape == (2, CFG.time_embed_dim)
    assert list(unet._lora.order) == list(all_target_modules(CFG))
