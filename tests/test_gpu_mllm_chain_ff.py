"""GPU: the chain fast-forward (`LlamaDecodeEngine(chain_fast_forward=True)`) on the tiny model of oracle/make_golden_mllm.py,
against the fp32 CPU oracle.  Engines as in test_gpu_mllm_batch.py: max_positions 96, max_new_tokens 40, poll_every 4, EOS 2;
36 new tokens.

The cases (tests/_chain_ff_cases.py; tests/test_mllm_chain_ff_host.py asserts their figures on the CPU):
  mid_burst    chain [209] + IMG_IDS, text-ending prompt (31, 6, 7), 32 tokens: the oracle picks 209 at index 3, is forced at
               4..21 and free after; smallest free margin 0.144 - all 36 ids must match
  from_prompt  the same chain, prompt (22, 17, 3) ending in <img>: forced at 0..16; smallest free margin 0.065 - all 36
  two_blocks   chain [26] + IMG_IDS, text-ending (50, 6, 7): 26 picked at 6 and 26, forced 7..24 and 27..35 (cut by max_new);
               smallest free margin 0.162 - all 36
  neighbour    (50, 6, 7) under chain [209] + IMG_IDS never enters the chain; margins below 5e-2 may flip (test_gpu_mllm.py's
               rule), compared up to the flip
A launch plan holds one chain, so the four make two batches: [mid_burst, from_prompt, neighbour] under 209 and [two_blocks,
from_prompt] under 26 (from_prompt's oracle is the same under both: it never picks 26 or 209).

fp8 cache: the oracle seen through quantize_kv_fp8 (tests/_kv8_ref.py) gives the same ids for the three quoted cases, smallest
free margins 0.087 / 0.054 / 0.165, so all 36 must match there too.  mxfp4 weights: on the dequantised weights the oracle never
picks 209 or 26 for the text-ending prompts (its margins there are 1e-3 .. 1e-2), so under mxfp4 only from_prompt has a forced
block (0..16; smallest free margin 8e-3 / 1.1e-2 with the fp8 cache): every case still runs, by the flip rule against that
oracle, and the block of from_prompt must be reproduced.

What a pass decodes: the forced ids but the one the prompt pass's own pick makes - index 0 of from_prompt - so
`fast_forward_rows` is 18 / 16 / 18 + 9; in every run it equals the number of forced indices >= 1 of the ids returned.

Hidden states and img_gen_feat: gate() at min(ceiling, 3 x the value measured on MI355X), ceiling 3e-2 (1e-2 against the fp8
oracle with fp16 weights), the gates of test_gpu_mllm_batch.py / test_gpu_mllm_kv8.py; MEASURED holds the largest value per
gate family (log: profiles/mllm_chain_ff_measured_gates.jsonl)."""
import pytest
import torch

from tests import _chain_ff_cases as C
from tests._gates import gate
from tests.test_gpu_mllm_batch import _check_ids, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = {"mid_burst": 18, "from_prompt": 16, "two_blocks": 27, "neighbour": 0}
BATCHES = {209: ["mid_burst", "from_prompt", "neighbour"], 26: ["two_blocks", "from_prompt"]}
CONFIGS = [(w, kv) for w in ("float16", "mxfp4") for kv in ("float16", "fp8")]

# measured on MI355X (gfx950): the largest max|err| / max|ref| of each gate family over its cases, rounded up to 2 digits
MEASURED = {
    "hidden/float16/float16": 0.0018, "img_gen_feat/float16/float16": 0.0017,
    "hidden/float16/fp8": 0.0078, "img_gen_feat/float16/fp8": 0.0082,
    "hidden/mxfp4/float16": 0.014, "img_gen_feat/mxfp4/float16": 0.0037,
    "hidden/mxfp4/fp8": 0.011, "img_gen_feat/mxfp4/fp8": 0.0094,
}


def _ceiling(w, kv):
    return 1e-2 if (kv == "fp8" and w == "float16") else 3e-2


def _g(family, what, value, w, kv):
    top = _ceiling(w, kv)
    # two runs of the engine against each other ("across compositions": measured 0, bit-identical) get the gate of the
    # hidden states against the oracle: nothing promises equal bits there, and 3 x 0 would
    key = f"{'hidden' if family.startswith('hidden') else family}/{w}/{kv}"
    return gate(f"chain ff {family}, {w}/{kv}, {what}", value, min(top, 3 * MEASURED[key]) if key in MEASURED else top)


@pytest.fixture(scope="module")
def env(hip_lib):
    from oracle import make_golden_mllm as G
    from diffsensei_amd.mllm import ContinuousLVLM, LlamaConfig, LlamaDecodeEngine, QwenResampler
    cfg = LlamaConfig(vocab_size=G.TINY["vocab_size"], hidden_size=G.TINY["hidden_size"],
                      intermediate_size=G.TINY["intermediate_size"], num_hidden_layers=G.TINY["num_hidden_layers"],
                      num_attention_heads=G.TINY["num_attention_heads"], rms_norm_eps=G.TINY["rms_norm_eps"])
    sd, sd_in, sd_out = C.weights()
    res_in, res_out = QwenResampler(sd_in, G.RES_IN["num_heads"], DEV), QwenResampler(sd_out, G.RES_OUT["num_heads"], DEV)
    engines, runs = {}, {}

    def agent(S=4, w="float16", kv="float16", graph=True, ff=True):
        """one engine per configuration, shared by the tests below (ff None: built without the argument)"""
        key = (S, w, kv, graph, ff)
        if key not in engines:
            kw = {} if ff is None else {"chain_fast_forward": ff}
            engines[key] = ContinuousLVLM(LlamaDecodeEngine(cfg, sd, DEV, max_positions=96, max_new_tokens=40, use_graph=graph,
                                                            poll_every=4, max_sequences=S, weight_dtype=w, kv_dtype=kv, **kw),
                                          res_in, res_out)
        return engines[key]

    def request(name, head, eos=C.EOS):
        ids, mask, img = C.make_prompt(name)
        return dict(input_ids=ids[None], image_embeds=img.to(DEV), ids_cmp_mask=mask[None], num_img_gen_tokens=G.N_IMG,
                    max_new_tokens=C.MAX_NEW, img_ids_list=[head] + list(G.IMG_IDS), eos_token_id=eos)

    def embs(a, names):
        out = []
        for n in names:
            ids, mask, img = C.make_prompt(n)
            e = a.llm.embed_tokens(ids)
            e[mask.to(DEV)] = a.input_resampler(img.to(DEV)).reshape(-1, e.shape[-1])
            out.append(e)
        return out

    def one(a, name, head):
        """`generate` of one case -> (agent output, hidden rows, run info)"""
        out = a.generate(**request(name, head))
        n = len(out["output_ids"])
        return out, a.llm.feat[:n - 1].clone(), dict(a.llm.last_run_info)

    def batch(a, names, head, eos=None):
        outs = a.generate_batch([request(n, head, (eos or {}).get(n, C.EOS)) for n in names])
        hid = [a.llm.feats[s, :len(o["output_ids"]) - 1].clone() for s, o in enumerate(outs)]
        return outs, hid, dict(a.llm.last_run_info)

    def cached(kind, w, kv, graph, *key):
        """the runs several tests look at: ("one", name) / ("batch", head), once per configuration"""
        k = (kind, w, kv, graph) + key
        if k not in runs:
            a = agent(4, w, kv, graph)
            runs[k] = one(a, key[0], C.CASES[key[0]][0]) if kind == "one" else batch(a, BATCHES[key[0]], key[0])
        return runs[k]

    return {"G": G, "agent": agent, "request": request, "embs": embs, "one": one, "batch": batch, "cached": cached}


def _forced_after_first(ids, chain):
    return sum(1 for i in range(1, len(ids)) if ids[i - 1] in chain[:-1])


def _check(env, name, head, out, hidden, rows, w, kv, what):
    """assertions 1 - 3 for one sequence: ids by the case's rule, hidden states and img_gen_feat through the gates, the rows
    the passes decoded.  Returns the number of ids in common with the oracle."""
    G = env["G"]
    chain = [head] + list(G.IMG_IDS)
    ref = C.oracle(name, chain_head=head, kv8=kv == "fp8", mxfp4=w == "mxfp4")
    got = out["output_ids"].tolist()
    quoted = w == "float16" and C.CASES[name][4] is not None and (head == C.CASES[name][0] or name == "from_prompt")
    if quoted:
        free = [float(m) for i, m in enumerate(ref["margins"]) if i not in ref["forced"]]
        assert min(free) >= 5e-2, (name, kv, min(free))
        assert got == ref["ids"], f"{what}: all {C.MAX_NEW} ids must match"
        assert rows == ROWS[name], f"{what}: {rows} rows went through the passes"
        n_same = len(got)
    else:
        n_same = _check_ids(got, ref["ids"], ref["margins"].tolist(), what)
        if name == "from_prompt":
            assert n_same > G.N_IMG + 1 and rows >= ROWS[name], "the forced block must be reproduced, in one pass"
    assert rows == _forced_after_first(got, chain), f"{what}: every forced id after the first pick comes from a pass"
    assert hidden.shape[0] == len(got) - 1
    if n_same > 1:
        _g("hidden", what, _rel(hidden[:n_same - 1], ref["hidden"][:n_same - 1]), w, kv)
    blocks = [e for e, t in enumerate(got) if t == G.EOI and e >= G.N_IMG]
    if blocks and blocks[0] < n_same and ref["img_gen_feat"] is not None:
        _g("img_gen_feat", what, _rel(out["img_gen_feat"][0], ref["img_gen_feat"][0]), w, kv)
    return n_same


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("w,kv", CONFIGS)
def test_generate_matches_the_oracle(env, w, kv, graph):
    for name, (head, _, _, _, _) in C.CASES.items():
        out, hidden, info = env["cached"]("one", w, kv, graph, name)
        what = f"generate {name} graph={graph}"
        _check(env, name, head, out, hidden, info["fast_forward_rows"], w, kv, what)
        n = len(out["output_ids"])
        assert info["new_tokens"] == n and (graph or not info["graph"])
        assert info["token_steps_launched"] <= (n - 1) - info["fast_forward_rows"] + 3 * info["fast_forward_passes"], what
        if name == "from_prompt" and n == C.MAX_NEW and info["fast_forward_rows"] == 16:
            # the prompt's pick pauses the slot: the pass runs before any token step, so no step is wasted
            assert info["fast_forward_passes"] == 1 and info["token_steps_launched"] == (C.MAX_NEW - 1) - 16, what
        if w == "float16":
            assert info["fast_forward_passes"] == {"mid_burst": 1, "from_prompt": 1, "two_blocks": 2, "neighbour": 0}[name]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("w,kv", CONFIGS)
def test_batches_match_the_oracle(env, w, kv, graph):
    for head, names in BATCHES.items():
        outs, hid, info = env["cached"]("batch", w, kv, graph, head)
        assert info["sequences"] == len(names)
        for k, name in enumerate(names):
            _check(env, name, head, outs[k], hid[k], info["fast_forward_rows"][k], w, kv, f"batch {head}/{name} graph={graph}")


@pytest.mark.parametrize("w,kv", CONFIGS)
def test_graph_and_eager_are_bit_identical(env, w, kv):
    for key in [("one", n) for n in C.CASES] + [("batch", h) for h in BATCHES]:
        a, b = env["cached"](key[0], w, kv, True, key[1]), env["cached"](key[0], w, kv, False, key[1])
        if key[0] == "one":
            a, b = ([a[0]], [a[1]], a[2]), ([b[0]], [b[1]], b[2])
        for x, y, hx, hy in zip(a[0], b[0], a[1], b[1]):
            assert torch.equal(x["output_ids"], y["output_ids"]) and torch.equal(hx, hy), key
        assert a[2]["fast_forward_rows"] == b[2]["fast_forward_rows"]


@pytest.mark.parametrize("w,kv", [("float16", "float16"), ("float16", "fp8")])
def test_a_sequence_does_not_depend_on_its_slot_or_on_what_ran_before(env, w, kv):
    """alone in slot 0, alone in slot 3, and again after other sequences have used the engine: the same bits.  Across batch
    compositions the GEMM row count of a pass changes and nothing promises equal bits: equal ids, gated hidden states (whether
    they came out bit-identical is printed, and recorded in DESIGN.md 9.14)."""
    a = env["agent"](4, w, kv, True)
    llm = a.llm
    for name in ("mid_burst", "from_prompt"):
        head = C.CASES[name][0]
        llm.set_image_token_chain([head] + list(env["G"].IMG_IDS))
        e = env["embs"](a, [name])
        last = [int(C.make_prompt(name)[0][-1])]
        got = []
        for slots in ([0], [3]):
            got.append(llm.generate_batch(e, last, C.EOS, C.MAX_NEW, slots=slots)[0])
            assert llm.last_run_info["fast_forward_rows"] == [_forced_after_first(got[-1]["ids"].tolist(), llm._chain_ids)]
        env["batch"](a, BATCHES[209], 209)                  # other sequences in every slot, other passes
        got.append(llm.generate_batch(e, last, C.EOS, C.MAX_NEW, slots=[0])[0])
        for other in got[1:]:
            assert torch.equal(other["ids"], got[0]["ids"]) and torch.equal(other["hidden"], got[0]["hidden"]), name
        outs, hid, _ = env["cached"]("batch", w, kv, True, 209)
        k = BATCHES[209].index(name)
        assert outs[k]["output_ids"].tolist() == got[0]["ids"].tolist(), "another batch composition, other ids"
        same = torch.equal(hid[k], got[0]["hidden"])
        print(f"[chain ff] {name} {w}/{kv}: alone vs batch of three hidden states bit-identical: {same}")
        _g("hidden across compositions", name, _rel(hid[k], got[0]["hidden"]), w, kv)
    # two slots paused by the prompt's pick share one pass of 2 x 16 rows (and mid_burst gets its own later): other GEMM shapes
    outs, hid, info = env["batch"](a, ["from_prompt", "mid_burst", "from_prompt"], 209)
    assert info["fast_forward_rows"] == [16, 18, 16] and info["fast_forward_passes"] == 2
    for k in (0, 2):
        assert outs[k]["output_ids"].tolist() == got[0]["ids"].tolist()
        print(f"[chain ff] from_prompt {w}/{kv}: alone vs two in one pass, slot {k}, bit-identical: {torch.equal(hid[k], got[0]['hidden'])}")
        _g("hidden across compositions", f"two in one pass, slot {k}", _rel(hid[k], got[0]["hidden"]), w, kv)


def test_mode_off_is_the_engine_without_the_argument(env):
    off, plain = env["agent"](4, "float16", "float16", True, ff=False), env["agent"](4, "float16", "float16", True, ff=None)
    assert off.llm.chain_fast_forward is False and plain.llm.chain_fast_forward is False
    for name in ("mid_burst", "from_prompt"):
        head = C.CASES[name][0]
        x, hx, ix = env["one"](off, name, head)
        y, hy, iy = env["one"](plain, name, head)
        assert torch.equal(x["output_ids"], y["output_ids"]) and torch.equal(hx, hy)
        assert ix["token_steps_launched"] == iy["token_steps_launched"] == C.MAX_NEW - 1
        assert ix["fast_forward_rows"] == 0 and ix["fast_forward_passes"] == 0
        assert x["output_ids"].tolist() == C.oracle(name)["ids"]
    bx, by = env["batch"](off, BATCHES[209], 209), env["batch"](plain, BATCHES[209], 209)
    for k in range(3):
        assert torch.equal(bx[0][k]["output_ids"], by[0][k]["output_ids"]) and torch.equal(bx[1][k], by[1][k])
    assert bx[2]["token_steps_launched"] == C.MAX_NEW - 1 and bx[2]["fast_forward_rows"] == [0, 0, 0]


@pytest.mark.parametrize("w,kv", [("float16", "float16"), ("float16", "fp8")])
def test_a_slot_that_finishes_inside_the_pass(env, w, kv):
    """eos = an image id: the run ends inside the block.  The slot returns ids[:stop] and stop - 1 hidden rows; its
    neighbours (their passes and token steps are their own) keep the bits of the run without the early stop."""
    a = env["agent"](4, w, kv, True)
    want = C.oracle("mid_burst", kv8=kv == "fp8")["ids"]
    eos0 = 605
    stop = want.index(eos0) + 1
    assert 4 < stop < 22
    outs, hid, info = env["batch"](a, BATCHES[209], 209, eos={"mid_burst": eos0})
    assert outs[0]["output_ids"].tolist() == want[:stop] and hid[0].shape[0] == stop - 1
    assert info["new_tokens"][0] == stop and info["fast_forward_rows"][0] == stop - 4
    ref_outs, ref_hid, _ = env["cached"]("batch", w, kv, True, 209)
    # the shorter pass is another GEMM shape: its rows are gated against the full run's, not compared bit for bit
    _g("hidden across compositions", "slot finished inside the pass", _rel(hid[0], ref_hid[0][:stop - 1]), w, kv)
    for k in (1, 2):
        assert torch.equal(outs[k]["output_ids"], ref_outs[k]["output_ids"]) and torch.equal(hid[k], ref_hid[k]), k
    alone = env["one"](a, "mid_burst", 209)                 # the engine goes on as if nothing had happened
    assert torch.equal(alone[0]["output_ids"], env["cached"]("one", w, kv, True, "mid_burst")[0]["output_ids"])
    assert torch.equal(alone[1], env["cached"]("one", w, kv, True, "mid_burst")[1])


def test_the_chunked_prompt_path_pauses_too(env):
    """prompt_path="chunks" ends in the one-sequence pick (DS_OP_LLM_SELECT, pause flag in i[4]): the same ids, the pass
    before any token step"""
    from diffsensei_amd.mllm import ContinuousLVLM, LlamaDecodeEngine
    base = env["agent"](4, "float16", "float16", True)
    llm = LlamaDecodeEngine(base.llm.cfg, C.weights()[0], DEV, max_positions=96, max_new_tokens=40, poll_every=4,
                            prompt_path="chunks", chain_fast_forward=True)
    out, hidden, info = env["one"](ContinuousLVLM(llm, base.input_resampler, base.output_resampler), "from_prompt", 209)
    _check(env, "from_prompt", 209, out, hidden, info["fast_forward_rows"], "float16", "float16", "chunked prompt path")
    assert info["fast_forward_passes"] == 1 and info["token_steps_launched"] == (C.MAX_NEW - 1) - 16


def test_a_repeated_chain_id_is_refused(env):
    a = env["agent"](4, "float16", "float16", True)
    with pytest.raises(ValueError):
        a.llm.set_image_token_chain([600, 601, 601, 617])
