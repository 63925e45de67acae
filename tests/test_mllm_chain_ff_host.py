"""CPU: the host side of the chain fast-forward (`LlamaDecodeEngine(chain_fast_forward=True)`, diffsensei_amd/mllm.py).

`forced_run` against the fp32 oracle (oracle/llama_ref.py: `greedy_generate` with the reference's logits processor): from the
state after the oracle's pick i, it must return the oracle's next ids exactly as long as the oracle keeps being forced - also
when the eos is an image id (the run ends inside the block) and when max_new cuts the block.  A chain with a repeated id is
refused only with the mode on, and the mode changes the launch lists in the pick's pause flag and in nothing else."""
import pytest
import torch

from diffsensei_amd import _lib
from diffsensei_amd import mllm as M
from tests import _chain_ff_cases as C
from tests.test_mllm_op_lists import CAP, CFG, CHAIN, T_MAX, _sd, describe


def _expected_run(ref, i):
    """the oracle's ids after index i up to the first one that was a choice"""
    j = i + 1
    while j < len(ref["ids"]) and j in ref["forced"]:
        j += 1
    return ref["ids"][i + 1:j]


RUNS = [(name, C.EOS, C.MAX_NEW) for name in C.CASES] + [
    ("mid_burst", 605, C.MAX_NEW),          # the eos is an image id: the oracle stops inside the block
    ("from_prompt", 601, C.MAX_NEW),        # ... the very first forced id: nothing is left to fast-forward
    ("from_prompt", 617, C.MAX_NEW),        # ... </img> itself
    ("mid_burst", C.EOS, 12),               # max_new cuts the block
    ("mid_burst", C.EOS, 5),                # ... after its first id
    ("mid_burst", C.EOS, 4),                # ... before it: 209 is the last id out
    ("from_prompt", C.EOS, 1),
]


@pytest.mark.parametrize("name,eos,max_new", RUNS)
def test_forced_run_is_the_oracles_forced_stretch(name, eos, max_new):
    ref, chain = C.oracle(name, eos=eos, max_new=max_new), C.chain_of(name)
    ids = ref["ids"]
    assert len(ids) <= max_new and (len(ids) == max_new or ids[-1] == eos)
    for i, cur in enumerate(ids):
        if cur == eos:                      # the sequence finished with this id: the kernel never pauses it, no state to run from
            assert i == len(ids) - 1
            continue
        want = _expected_run(ref, i)
        got = M.forced_run(chain, cur, i + 1, max_new, eos)
        assert got == want, (name, i, got, want)
        assert bool(got) == (i + 1 < max_new and cur in chain[:-1])   # exactly the slots the pick kernel pauses
    # from the last prompt id with nothing out: the whole first stretch (what folding it into the prompt pass would use)
    assert M.forced_run(chain, int(C.make_prompt(name)[0][-1]), 0, max_new, eos) == (ids[:1] + _expected_run(ref, 0) if 0 in ref["forced"] else [])


def test_the_cases_are_the_ones_the_gpu_test_quotes():
    for name, (head, _, _, ranges, margin) in C.CASES.items():
        ref = C.oracle(name)
        assert len(ref["ids"]) == C.MAX_NEW
        assert ref["forced"] == [i for a, b in ranges for i in range(a, b + 1)], name
        for a, _ in ranges:
            if a > 0:
                assert ref["ids"][a - 1] == head                      # the chain's first id was a free pick
        if margin is not None:
            free = [float(m) for i, m in enumerate(ref["margins"]) if i not in ref["forced"]]
            assert abs(min(free) - margin) < 2e-3 and min(free) >= 5e-2, (name, min(free))


def _engine(ff, chain=CHAIN, **kw):
    cfg = M.LlamaConfig(**CFG)
    args = dict(chain_fast_forward=True) if ff else {}
    eng = M.LlamaDecodeEngine(cfg, _sd(cfg), "cpu", max_positions=T_MAX, max_new_tokens=CAP, **args, **kw)
    eng.set_image_token_chain(chain)
    return eng


def test_a_repeated_chain_id_is_refused_only_with_the_mode_on():
    rep = [60, 10, 11, 10, 61]
    with pytest.raises(ValueError):
        _engine(True, rep)
    eng = _engine(False, rep)
    assert eng.n_chain == 5 and not eng.chain_fast_forward
    eng = _engine(True)
    with pytest.raises(ValueError):
        eng.set_image_token_chain(rep)
    assert eng._chain_ids == CHAIN, "a refused chain leaves the engine's chain as it was"
    eng.set_image_token_chain(None)
    assert eng.n_chain == 0


@pytest.mark.parametrize("weight_dtype,kv_dtype", [("float16", "float16"), ("int8", "float16"), ("mxfp4", "fp8")])
def test_the_mode_changes_the_pause_flag_of_the_pick_and_nothing_else(weight_dtype, kv_dtype):
    off = _engine(False, max_sequences=4, weight_dtype=weight_dtype, kv_dtype=kv_dtype)
    on = _engine(True, max_sequences=4, weight_dtype=weight_dtype, kv_dtype=kv_dtype)
    lists = (("_token_ops", (1,), "LLM_SELECT_SLOTS", 5), ("_token_ops", (4,), "LLM_SELECT_SLOTS", 5),
             ("_chunk_ops", (16, "last"), "LLM_SELECT", 4), ("_chunk_ops", (5, "chunk"), None, None))
    for fn, args, pick, slot in lists:
        a, b = describe(off, getattr(off, fn)(*args)), describe(on, getattr(on, fn)(*args))
        assert len(a) == len(b)
        differ = [(x, y) for x, y in zip(a, b) if x != y]
        if pick is None:
            assert not differ
            continue
        assert len(differ) == 1 and a[-1]["op"] == pick
        x, y = differ[0]
        assert x is a[-1] and x["i"][slot] == 0 and y["i"][slot] == 1
        y["i"][slot] = 0
        assert x == y, "the pick differs in more than its pause flag"
    assert off._plan(1, "token") is off._plan(1, "token")
    assert (_lib.OP["LLM_ATTN_ROWS"], _lib.OP["LLM_ATTN_ROWS_KV8"]) == (42, 43)


def test_the_plan_cache_key_holds_the_mode():
    eng = _engine(False)
    keys = set(eng._plans)
    eng._plan(1, "token")
    (key,) = set(eng._plans) - keys
    assert key[-1] is False
    eng.chain_fast_forward = True
    assert eng._plan(1, "token") is not eng._plans[key] and key[:-1] + (True,) in eng._plans
