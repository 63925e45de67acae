"""GPU: batched MLLM decode (LlamaDecodeEngine.generate_batch, ContinuousLVLM.generate_batch, mllm_prepass_batch) on the
tiny configuration of oracle/make_golden_mllm.py, against the fp32 CPU oracle (oracle/llama_ref.py).

Four prompts of different lengths share one decode loop on an engine with four slots.  For the three new prompts every
free-choice top-2 margin of the oracle is >= 5e-2 (minima 0.188, 0.107, 0.057 - asserted below), above the fp16 logit
noise, so all 28 ids must equal the oracle's; the golden prompt keeps the flip rule of test_gpu_mllm.py.  Hidden states
and image features agree with the oracle to 3e-2 (the existing gates).  Batch independence is bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "mllm_tiny.npz")
PROMPTS = [(22, 17, 3), (24, 30, 2), (27, 6, 6), (7, 9, 5)]          # (seed, n1, n2); the last one is the golden prompt
EOS = 2


def make_prompt(G, seed, n1, n2):
    """`G.tiny_prompt` with text lengths (n1, n2): [bos, n1 text, <img>, 16 placeholders, </img>, n2 text, <img>]."""
    g = torch.Generator().manual_seed(seed)
    t = lambda n: torch.randint(3, 590, (n,), generator=g).tolist()
    ids = [1] + t(n1) + [G.BOI] + G.IMG_IDS[1:-1] + [G.EOI] + t(n2) + [G.BOI]
    mask = [False] * len(ids)
    for i in range(n1 + 2, n1 + 2 + G.N_IMG):
        mask[i] = True
    image_embeds = torch.randn(1, G.N_IMG, G.RES_IN["kv_dim"], generator=g)
    return torch.tensor(ids), torch.tensor(mask), image_embeds


def _rel(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), (got.shape, ref.shape)
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)


def _check_ids(got, want, margins, what):
    """test_gpu_mllm.py's rule: identical, except that a choice whose fp32 top-2 margin is inside the fp16 logit noise may
    flip (everything after such a flip is a different continuation)."""
    got, want = list(got), list(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            assert margins[i] < 5e-2, f"{what}: id {i} is {a}, oracle {b} (margin {margins[i]:.3g})"
            return i
    assert len(got) == len(want), f"{what}: {len(got)} ids vs {len(want)}"
    return len(want)


@pytest.fixture(scope="module")
def env(hip_lib):
    from oracle import llama_ref as R
    from oracle import make_golden_mllm as G
    from diffsensei_amd.mllm import ContinuousLVLM, LlamaConfig, LlamaDecodeEngine, QwenResampler
    cfg = LlamaConfig(vocab_size=G.TINY["vocab_size"], hidden_size=G.TINY["hidden_size"],
                      intermediate_size=G.TINY["intermediate_size"], num_hidden_layers=G.TINY["num_hidden_layers"],
                      num_attention_heads=G.TINY["num_attention_heads"], rms_norm_eps=G.TINY["rms_norm_eps"])
    sd, sd_in, sd_out = G.tiny_weights(), G.tiny_resampler(G.RES_IN, 11), G.tiny_resampler(G.RES_OUT, 12)
    res_in, res_out = QwenResampler(sd_in, G.RES_IN["num_heads"], DEV), QwenResampler(sd_out, G.RES_OUT["num_heads"], DEV)
    mk = lambda graph: ContinuousLVLM(LlamaDecodeEngine(cfg, sd, DEV, max_positions=96, max_new_tokens=40, use_graph=graph,
                                                        poll_every=4, max_sequences=4), res_in, res_out)
    prompts = [make_prompt(G, *p) for p in PROMPTS]
    assert [len(p[0]) for p in prompts] == [40, 52, 32, 34]
    assert all(torch.equal(a, b) for a, b in zip(prompts[3], G.tiny_prompt()))
    refs = [R.lvlm_generate(sd, R.LlamaRefConfig(**G.TINY), sd_in, sd_out, (G.RES_IN["num_heads"], G.RES_OUT["num_heads"]),
                            ids, img, mask, G.IMG_IDS, EOS, G.MAX_NEW, G.N_IMG) for ids, mask, img in prompts]
    agent = mk(True)
    agent.llm.set_image_token_chain(G.IMG_IDS)

    def embs(which):
        out = []
        for k in which:
            ids, mask, img = prompts[k]
            e = agent.llm.embed_tokens(ids)
            e[mask.to(DEV)] = agent.input_resampler(img.to(DEV)).reshape(-1, e.shape[-1])
            out.append(e)
        return out

    def decode(eng, which, eos=EOS, slots=None):
        eng.set_image_token_chain(G.IMG_IDS)
        return eng.generate_batch(embs(which), [int(prompts[k][0][-1]) for k in which], eos, G.MAX_NEW, slots=slots)

    first = decode(agent.llm, [0, 1, 2, 3])                 # the shared reference run: all four, graph engine, slots 0..3
    info = dict(agent.llm.last_run_info)
    engines = {}

    def engine(S, weights="float16", graph=True):
        """one engine per (slots, weight type, graph), shared by the tests below"""
        key = (S, weights, graph)
        if key not in engines:
            engines[key] = LlamaDecodeEngine(cfg, sd, DEV, max_positions=96, max_new_tokens=40, use_graph=graph, poll_every=4,
                                             max_sequences=S, weight_dtype=weights)
            engines[key].set_image_token_chain(G.IMG_IDS)
        return engines[key]

    return {"G": G, "mk": mk, "agent": agent, "prompts": prompts, "refs": refs, "decode": decode, "first": first,
            "info": info, "gold": dict(np.load(GOLD)), "embs": embs, "engine": engine}


def test_batch_of_four_matches_the_oracle(env):
    G, refs, first = env["G"], env["refs"], env["first"]
    for k, (want_min, ref) in enumerate(zip((0.188, 0.107, 0.057), refs[:3])):
        free = ref["margins"][G.N_IMG + 1:]                 # the forced chain and </img> are not choices
        assert float(free.min()) >= 5e-2 and abs(float(free.min()) - want_min) < 2e-3, (k, float(free.min()))
        assert first[k]["ids"].tolist() == ref["output_ids"].tolist(), f"prompt {k}: all {G.MAX_NEW} ids must match"
        gate(f"hidden states, prompt {k}", _rel(first[k]["hidden"], ref["hidden"]), 3e-2)
    ref, gold = refs[3], env["gold"]
    assert ref["output_ids"].tolist() == gold["a_ids"].tolist()
    n_same = _check_ids(first[3]["ids"].tolist(), gold["a_ids"].tolist(), ref["margins"].tolist(), "golden prompt")
    assert n_same > G.N_IMG, "the forced image chain and </img> must always match"
    gate("hidden states, golden prompt", _rel(first[3]["hidden"][:n_same - 1],
                                              torch.from_numpy(gold["a_hidden"][:n_same - 1])), 3e-2)
    info = env["info"]
    assert info["sequences"] == 4 and info["prompt_tokens"] == [40, 52, 32, 34] and info["graph"]
    assert info["new_tokens"] == [len(o["ids"]) for o in first] and info["new_tokens"][:3] == [G.MAX_NEW] * 3
    assert info["token_steps_launched"] == G.MAX_NEW - 1


def test_agent_generate_batch_matches_the_oracle(env):
    G, agent, refs = env["G"], env["agent"], env["refs"]
    reqs = [dict(input_ids=ids[None], image_embeds=img.to(DEV), ids_cmp_mask=mask[None], num_img_gen_tokens=G.N_IMG,
                 max_new_tokens=G.MAX_NEW, img_ids_list=G.IMG_IDS, eos_token_id=EOS) for ids, mask, img in env["prompts"]]
    outs = agent.generate_batch(reqs)
    assert agent.llm.last_run_info["graph"], "the second call replays the captured token step"
    for k, (out, ref) in enumerate(zip(outs, refs)):
        assert out["output_ids"].tolist() == env["first"][k]["ids"].tolist(), "same ids as the engine-level run"
        assert out["num_gen_imgs"] == ref["num_gen_imgs"] == 1 and bool(out["ids_gen_mask"][:G.N_IMG].all())
        assert out["img_gen_feat"].shape == (1, G.N_IMG, G.RES_OUT["embed_dim"])
        gate(f"img_gen_feat, prompt {k}", _rel(out["img_gen_feat"], ref["img_gen_feat"]), 3e-2)
    with pytest.raises(ValueError):
        agent.generate_batch([reqs[0], dict(reqs[1], img_ids_list=[599] + list(G.IMG_IDS))])


def test_early_stop_of_one_sequence_leaves_the_others_alone(env):
    G, first = env["G"], env["first"]
    want = env["refs"][0]["output_ids"].tolist()
    eos0 = want[G.N_IMG + 4]
    stop = want.index(eos0) + 1                             # the id is appended, then the slot is finished
    assert G.N_IMG < stop <= G.N_IMG + 5
    out = env["decode"](env["agent"].llm, [0, 1, 2, 3], eos=[eos0, EOS, EOS, EOS])
    assert out[0]["ids"].tolist() == want[:stop] and out[0]["hidden"].shape[0] == stop - 1
    assert torch.equal(out[0]["hidden"], first[0]["hidden"][:stop - 1])
    for k in (1, 2, 3):
        assert torch.equal(out[k]["ids"], first[k]["ids"]) and torch.equal(out[k]["hidden"], first[k]["hidden"])
    info = env["agent"].llm.last_run_info
    assert info["new_tokens"][0] == stop and info["new_tokens"][1:] == [len(o["ids"]) for o in first[1:]]


def test_a_sequence_does_not_depend_on_its_slot_or_its_neighbours(env):
    eng, first = env["agent"].llm, env["first"]
    alone0 = env["decode"](eng, [0])[0]
    assert eng.last_run_info["sequences"] == 1
    alone3 = env["decode"](eng, [0], slots=[3])[0]
    order = [2, 0, 3, 1]
    mixed = env["decode"](eng, order)
    for what, got in (("alone in slot 0", alone0), ("alone in slot 3", alone3), ("batch of four, permuted", mixed[1])):
        assert torch.equal(got["ids"], first[0]["ids"]), what
        assert torch.equal(got["hidden"], first[0]["hidden"]), what
    for pos, k in enumerate(order):
        assert torch.equal(mixed[pos]["ids"], first[k]["ids"]) and torch.equal(mixed[pos]["hidden"], first[k]["hidden"])


def test_eager_and_graph_are_bit_identical(env):
    eager = env["mk"](False).llm
    out = env["decode"](eager, [0, 1, 2, 3])
    assert not eager.last_run_info["graph"]
    for a, b in zip(out, env["first"]):
        assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["hidden"], b["hidden"])
    eng = env["agent"].llm
    plans = len(eng._plans)
    again = env["decode"](eng, [0, 1, 2, 3])                # the captured graph is reused, every step is a replay
    assert eng.last_run_info["graph"] and len(eng._plans) == plans
    for a, b in zip(again, env["first"]):
        assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["hidden"], b["hidden"])
    eng.weights_changed()
    assert not eng._plans, "weights_changed() drops the batched token plan too"


def test_generate_batch_argument_checks(env):
    eng = env["agent"].llm
    H = eng.cfg.hidden_size
    emb = torch.zeros(10, H, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError):
        eng.generate_batch([emb] * 5, [1] * 5, 2, 4)                               # 5 sequences, 4 slots
    with pytest.raises(ValueError):
        eng.generate_batch([emb, torch.zeros(90, H, dtype=torch.float16, device=DEV)], [1, 1], 2, 20)   # cache too small
    with pytest.raises(ValueError):
        eng.generate_batch([emb], [1], 2, 41)                                      # above the engine's capacity
    with pytest.raises(ValueError):
        eng.generate_batch([emb.float()], [1], 2, 4)
    with pytest.raises(ValueError):
        eng.generate_batch([emb.cpu()], [1], 2, 4)
    with pytest.raises(ValueError):
        eng.generate_batch([emb, emb], [1, 1], 2, 4, slots=[1, 1])
    with pytest.raises(ValueError):
        type(eng)(eng.cfg, env["G"].tiny_weights(), DEV, max_positions=32, max_new_tokens=8, max_sequences=17)


def test_mllm_prepass_batch_matches_per_request_prepass(env):
    """One decode loop for four requests against four `mllm_prepass` calls on the same agent.  The two differ in the
    decode kernels only (MFMA vs fdot2 accumulation order), so where the ids agree the image-block rows come from hidden
    states that differ by fp16 rounding: measured 4.7e-4 .. 6.9e-4 of max|ref| on MI355X (all ids equal); gate 3e-2 as for the oracle."""
    from diffsensei_amd.mllm import mllm_prepass, mllm_prepass_batch
    G, agent = env["G"], env["agent"]

    class Cfg:
        num_vision_tokens, max_num_ips = G.N_IMG, 1

    class Pipe:
        class unet:
            config = Cfg

        @staticmethod
        def encode_ip_tokens(ip_images):                    # [1, dummy + max_num_ips * num_vision_tokens, dim]
            return torch.cat([torch.zeros_like(ip_images[0]), ip_images[0]], 1)

    reqs = [dict(input_ids=ids, ids_cmp_mask=mask, ip_images=[img.half().to(DEV)], mllm_scale=0.2 + 0.2 * k)
            for k, (ids, mask, img) in enumerate(env["prompts"])]
    kw = dict(img_ids_list=G.IMG_IDS, eos_token_id=EOS, max_new_tokens=G.MAX_NEW)
    got = mllm_prepass_batch(Pipe, agent, reqs, **kw)
    assert len(got) == 4
    for k, r in enumerate(reqs):
        ref = mllm_prepass(Pipe, agent, r["input_ids"], r["ids_cmp_mask"], r["ip_images"], r["mllm_scale"], **kw)
        assert got[k].shape == ref.shape == (1, G.N_IMG, G.RES_IN["kv_dim"])
        gate(f"blended ip_image_embeds, request {k}", _rel(got[k], ref), 3e-2)


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("weights", ["float16", "int8"])
@pytest.mark.parametrize("T0", [5, 16, 17, 40])            # chunk lists (16: a full chunk) | MFMA pass, 1 row and chunks past it
def test_generate_does_not_depend_on_max_sequences(env, T0, weights, graph):
    """`generate` is slot 0 at width 1 whatever the engine was built for: the same weights and prompt on an engine with one
    slot and on one with four give the same ids and hidden states, bit for bit."""
    G = env["G"]
    ids = env["prompts"][1][0]
    emb = env["embs"]([1])[0][:T0].contiguous()
    outs = []
    for S in (1, 4):
        eng = env["engine"](S, weights, graph)
        outs.append(eng.generate(emb, int(ids[T0 - 1]), EOS, G.MAX_NEW))
        info = eng.last_run_info
        assert info["prompt_tokens"] == T0 and info["new_tokens"] == len(outs[-1]["ids"]) > 1
        assert info["ops_per_token"] == 5 * eng.cfg.num_hidden_layers + 4
    assert torch.equal(outs[0]["ids"], outs[1]["ids"]), "the ids depend on max_sequences"
    assert outs[0]["hidden"].shape[0] == len(outs[0]["ids"]) - 1 and torch.equal(outs[0]["hidden"], outs[1]["hidden"])


def test_generate_and_generate_batch_share_an_engine(env):
    """The two forms share every buffer.  `generate` after `generate_batch` (slots 1..3 hold finished sequences, the tap
    rows those of another prompt) and `generate_batch` after `generate` give the bits of a fresh engine: all ids and all
    hidden rows, for a prompt on the MFMA pass and one on the chunk lists."""
    G, used, first = env["G"], env["agent"].llm, env["first"]
    ids = env["prompts"][1][0]
    emb = env["embs"]([1])[0]
    fresh = type(used)(used.cfg, G.tiny_weights(), DEV, max_positions=96, max_new_tokens=40, use_graph=True, poll_every=4,
                       max_sequences=4)
    fresh.set_image_token_chain(G.IMG_IDS)
    for T0 in (len(ids), 16):
        e = emb[:T0].contiguous()
        want = fresh.generate(e, int(ids[T0 - 1]), EOS, G.MAX_NEW)
        assert "sequences" not in fresh.last_run_info and fresh.last_run_info["new_tokens"] == len(want["ids"]) > 1
        env["decode"](used, [0, 1, 2, 3])
        got = used.generate(e, int(ids[T0 - 1]), EOS, G.MAX_NEW)
        assert torch.equal(got["ids"], want["ids"]) and torch.equal(got["hidden"], want["hidden"]), f"generate after a batch, T0={T0}"
        again = env["decode"](fresh, [0, 1, 2, 3])          # ... and the reverse, on the engine that has only run `generate`
        for k, (a, b) in enumerate(zip(again, first)):
            assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["hidden"], b["hidden"]), f"batch after generate, T0={T0}, {k}"
