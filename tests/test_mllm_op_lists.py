"""CPU: the launch lists of `LlamaDecodeEngine` against a recording made before the one-sequence and the batched decode
paths were merged (tests/golden/mllm_op_lists.json, recorded at commit 6c8fd86 with `describe` below on `_ops(M, kind)`
of a `max_sequences=1` engine and `_ops_batch()` of a `max_sequences=4` engine).  Every op is stored as its `i`, `f` and `l`
slots plus, for every non-null `p` slot, the NAME of the engine tensor it points into and the byte offset - no addresses.

What may differ is spelled out here and nowhere else:
  * buffer names: the recording's `*_b` buffers are today's per-slot buffers, and the one-sequence buffers are their slot 0
    (`RENAMED`; the byte offsets stay, slot 0 is at offset 0);
  * in the width-1 token list the embed, attention, final-norm and pick entries carry the slot-form op codes with their
    extra slots (slots = 1, slot_stride, ldo, ldl): `SLOT_FORM` maps every slot of the recorded one-sequence op to the slot
    of the slot-form op that must hold the same value, and fixes the extra ones.
The width-S list must equal the recorded `_ops_batch()` exactly, and so must the prompt chunk lists."""
import json
import os

import pytest
import torch

from diffsensei_amd import _lib
from diffsensei_amd import mllm as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mllm_op_lists.json")
CFG = dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1)   # test_mllm_w8_host.py
T_MAX, CAP = 32, 8
CHAIN = [60, 10, 11, 12, 61]
OP_NAME = {v: k for k, v in _lib.OP.items()}

# recorded buffer name -> today's name (same byte offset)
RENAMED = {"state_b": "state", "out_ids_b": "out_ids", "feat": "feats", "feat_b": "feats", "hn_b": "hn", "logits_b": "logits"}


def _sd(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(s, generator=g) * 0.05 for k, s in M.llama_param_shapes(cfg).items()}


def _engine(weight_dtype: str, chain: bool, max_sequences: int):
    cfg = M.LlamaConfig(**CFG)
    eng = M.LlamaDecodeEngine(cfg, _sd(cfg), "cpu", max_positions=T_MAX, max_new_tokens=CAP, max_sequences=max_sequences,
                              weight_dtype=weight_dtype)
    if chain:
        eng.set_image_token_chain(CHAIN)
    return eng


def describe(eng, ops_) -> list:
    """[{op, i, f, l, p}] with p = {slot: [tensor name, byte offset]}: the engine tensor (attribute, or element of a list
    attribute) a pointer lies in.  Views are not named: `kc` / `vc` (of `kcs` / `vcs`, where an engine has them) and `feat`
    where the engine also has `feats`."""
    spans = []
    for name, v in sorted(vars(eng).items()):
        if name in ("kc", "vc") or (name == "feat" and hasattr(eng, "feats")):
            continue
        if isinstance(v, torch.Tensor):
            spans.append((name, v))
        elif isinstance(v, list) and v and all(isinstance(t, torch.Tensor) for t in v):
            spans += [(f"{name}[{k}]", t) for k, t in enumerate(v)]
    spans = [(n, t.data_ptr(), t.numel() * t.element_size()) for n, t in spans]

    def where(q: int):
        hits = [(n, q - a) for n, a, size in spans if a <= q < a + size]
        assert len(hits) == 1, f"pointer in {len(hits)} engine tensors: {hits}"
        return list(hits[0])

    return [{"op": OP_NAME[int(o.code)], "i": list(o.i), "f": list(o.f), "l": list(o.l),
             "p": {str(k): where(q) for k, q in enumerate(o.p) if q}} for o in ops_]


def _renamed(rec: list) -> list:
    out = []
    for o in rec:
        p = {}
        for k, (name, off) in o["p"].items():
            p[k] = [RENAMED.get(name, name), off]
        out.append(dict(o, p=p))
    return out


# one-sequence op -> (slot-form op, {field: {recorded slot: slot of the slot form}}, {field: {extra slot: value}})
# (include/diffsensei_hip.h, DS_OP_LLM_*: the slot forms take `slots` in front of or behind the one-sequence i[] and a stride more)
H_, V_ = CFG["hidden_size"], CFG["vocab_size"]
KV_ = H_                                                    # kv_heads * head_dim of CFG
SLOT_FORM = {
    "LLM_EMBED": ("LLM_EMBED_SLOTS", {"i": {0: 1, 1: 2}}, {"i": {0: 1}, "l": {0: H_}}),                   # slots, ldo
    "LLM_ATTN": ("LLM_ATTN_SLOTS", {"i": {k: k for k in range(5)}, "l": {0: 0, 1: 1, 2: 2}}, {"l": {3: T_MAX * KV_}}),
    "LLM_RMSNORM": ("LLM_RMSNORM_SLOTS", {"i": {0: 0, 1: 1, 2: 2}, "l": {0: 0, 1: 1}}, {}),
    "LLM_SELECT": ("LLM_SELECT_SLOTS", {"i": {0: 0, 1: 1, 2: 2, 3: 3}}, {"i": {4: 1}, "l": {0: V_}}),      # slots, ldl
}


def _as_slot_form(o: dict) -> dict:
    """The recorded one-sequence op `o` rewritten as the slot-form op of one slot that the width-1 token list holds now."""
    if o["op"] not in SLOT_FORM:
        return o
    name, shared, extra = SLOT_FORM[o["op"]]
    new = {"op": name, "i": [0] * 16, "f": list(o["f"]), "l": [0] * 12, "p": o["p"]}
    for fld in ("i", "l"):
        moved = shared.get(fld, {})
        assert all(v == 0 for k, v in enumerate(o[fld]) if k not in moved), "a recorded slot would be dropped"
        for src, dst in moved.items():
            new[fld][dst] = o[fld][src]
        for dst, v in extra.get(fld, {}).items():
            assert dst not in moved.values()
            new[fld][dst] = v
    if o["op"] == "LLM_ATTN":
        assert o["i"][0] == 1                               # rows of the one-sequence op = slots of the slot form
    return new


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


CASES = [(w, c) for w in ("float16", "int8") for c in (False, True)]


@pytest.mark.parametrize("weight_dtype,chain", CASES)
def test_prompt_chunk_lists_did_not_move(golden, weight_dtype, chain):
    eng = _engine(weight_dtype, chain, 1)
    for rows, kind in ((5, "chunk"), (16, "last")):
        rec = _renamed(golden[f"{weight_dtype}/chain={int(chain)}/S=1/{kind}{rows}"])
        assert describe(eng, eng._chunk_ops(rows, kind)) == rec


@pytest.mark.parametrize("weight_dtype,chain", CASES)
def test_width_1_token_list_is_the_recorded_one_in_slot_form(golden, weight_dtype, chain):
    rec = _renamed(golden[f"{weight_dtype}/chain={int(chain)}/S=1/token1"])
    want = [_as_slot_form(o) for o in rec]
    assert sum(o["op"] != r["op"] for o, r in zip(want, rec)) == CFG["num_hidden_layers"] + 3
    for S in (1, 4):                                        # `generate` launches the same list whatever the engine was built for
        eng = _engine(weight_dtype, chain, S)
        got = describe(eng, eng._token_ops(1))
        if S == 4:                                          # ... up to the distance between two cache slots, which one slot never uses
            for o in got:
                if o["op"] == "LLM_ATTN_SLOTS":
                    assert o["l"][3] == T_MAX * KV_
        assert got == want


@pytest.mark.parametrize("weight_dtype,chain", CASES)
def test_width_s_token_list_did_not_move(golden, weight_dtype, chain):
    eng = _engine(weight_dtype, chain, 4)
    assert describe(eng, eng._token_ops(4)) == _renamed(golden[f"{weight_dtype}/chain={int(chain)}/S=4/batch"])
