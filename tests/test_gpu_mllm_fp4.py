"""GPU: the MLLM pre-pass with MXFP4 weight-only decoding (`LlamaDecodeEngine(weight_dtype="mxfp4")`) on the tiny
configuration of oracle/make_golden_mllm.py.

Oracle: the fp32 CPU oracle (oracle/llama_ref.lvlm_generate) on the state dict whose 14 projection matrices are replaced
by `dequantize_rows_mxfp4(*quantize_rows_mxfp4(w))` - the weights the MXFP4 kernels compute with.  Unlike int8, 4-bit
weights change the tiny model's picks (the first id that differs from tests/golden/mllm_tiny.npz is id 19), so the expected
ids are the oracle's on the dequantised weights, not the golden file's.  Precondition, asserted first and on the CPU: on both
golden prompts that oracle runs all MAX_NEW = 28 ids with every fp32 top-2 margin >= 5e-2 (measured: minimum 0.089), so
under the rule of test_gpu_mllm._check_ids (identical except where the oracle's margin is below 5e-2) all 28 ids must
match.  Fed-back hidden states and `img_gen_feat` agree with the oracle to 3e-2, the gates of the fp16 and int8 engine
tests.  Nothing here says anything about a trained 13B checkpoint."""
import os

import numpy as np
import pytest
import torch

from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "mllm_tiny.npz")
# (seed, n1, n2): 40, 52 and 32 prompt tokens.  On the dequantised weights the oracle's margins stay >= 5e-2 up to id 24 / for
# all 28 ids / up to id 24 (minimum over the first N_IMG + 6 ids: 0.67 / 0.16 / 0.23); test_gpu_mllm_w8.py's (24, 30, 2) drops
# to 1.5e-3 at id 17 with these weights.
BATCH_PROMPTS = [(22, 17, 3), (33, 30, 2), (27, 6, 6)]
PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
        "mlp.down_proj")


def _rel(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), (got.shape, ref.shape)
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)


def _check_ids(got, want, margins, what):
    """test_gpu_mllm.py's rule: identical, except that a choice whose fp32 top-2 margin is inside the fp16 logit noise may
    legitimately flip (everything after such a flip is a different continuation)."""
    got, want = list(got), list(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            assert margins[i] < 5e-2, f"{what}: id {i} is {a}, oracle {b} (margin {margins[i]:.3g})"
            return i
    assert len(got) == len(want), f"{what}: {len(got)} ids vs {len(want)}"
    return len(want)


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


@pytest.fixture(scope="module")
def tiny(hip_lib):
    from oracle import llama_ref as R
    from oracle import make_golden_mllm as G
    from diffsensei_amd.mllm import (ContinuousLVLM, LlamaConfig, LlamaDecodeEngine, QwenResampler, dequantize_rows_mxfp4,
                                     quantize_rows_mxfp4)
    cfg = LlamaConfig(vocab_size=G.TINY["vocab_size"], hidden_size=G.TINY["hidden_size"],
                      intermediate_size=G.TINY["intermediate_size"], num_hidden_layers=G.TINY["num_hidden_layers"],
                      num_attention_heads=G.TINY["num_attention_heads"], rms_norm_eps=G.TINY["rms_norm_eps"])
    sd = G.tiny_weights()
    sd_in, sd_out = G.tiny_resampler(G.RES_IN, 11), G.tiny_resampler(G.RES_OUT, 12)
    sd_q = dict(sd)
    names = [f"model.layers.{i}.{n}.weight" for i in range(cfg.num_hidden_layers) for n in PROJ]
    assert len(names) == 14
    for k in names:
        sd_q[k] = dequantize_rows_mxfp4(*quantize_rows_mxfp4(sd[k]))
    gold = dict(np.load(GOLD))
    heads = (G.RES_IN["num_heads"], G.RES_OUT["num_heads"])

    def oracle(prompt, eos):
        ids, mask, img = prompt
        return R.lvlm_generate(sd_q, R.LlamaRefConfig(**G.TINY), sd_in, sd_out, heads, ids, img, mask, G.IMG_IDS, eos,
                               G.MAX_NEW, G.N_IMG)

    refs = {tag: oracle(G.tiny_prompt(), int(gold[f"{tag}_eos"])) for tag in "ab"}
    mk = lambda graph=True, path="mfma", S=1: LlamaDecodeEngine(cfg, sd, DEV, max_positions=96, max_new_tokens=40,
                                                                 use_graph=graph, poll_every=4, prompt_path=path,
                                                                 max_sequences=S, weight_dtype="mxfp4")
    res_in, res_out = QwenResampler(sd_in, G.RES_IN["num_heads"], DEV), QwenResampler(sd_out, G.RES_OUT["num_heads"], DEV)
    return {"G": G, "mk": mk, "res_in": res_in, "res_out": res_out, "LVLM": ContinuousLVLM, "gold": gold, "refs": refs,
            "oracle": oracle}


def _precondition(tiny):
    """On both golden prompts the dequantised-weight oracle emits all MAX_NEW ids and every one of its picks has a margin of
    at least 5e-2: the id rule then allows no flip at all."""
    G = tiny["G"]
    assert G.MAX_NEW == 28
    for tag in "ab":
        ref = tiny["refs"][tag]
        assert len(ref["output_ids"]) == G.MAX_NEW and len(ref["margins"]) == G.MAX_NEW, tag
        assert float(min(ref["margins"].tolist())) >= 5e-2, (tag, ref["margins"].tolist())


@pytest.mark.parametrize("path", ["mfma", "chunks"])      # prompt pass: dequantise + GEMM projections / 16-row fp4 passes
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_mxfp4_generate_matches_the_oracle_on_dequantised_weights(tiny, graph, tag, path):
    _precondition(tiny)
    G, gold, ref = tiny["G"], tiny["gold"], tiny["refs"][tag]
    input_ids, mask, image_embeds = G.tiny_prompt()
    eos = int(gold[f"{tag}_eos"])
    agent = tiny["LVLM"](tiny["mk"](graph, path), tiny["res_in"], tiny["res_out"])
    assert agent.llm.weight_dtype == "mxfp4" and agent.llm.wqkv[0].dtype == torch.uint8 and agent.llm.eqkv[0].dtype == torch.uint8
    for rep in range(2):                                                                  # 2nd call reuses the plan/graph
        out = agent.generate(input_ids=input_ids[None], image_embeds=image_embeds.to(DEV), ids_cmp_mask=mask[None],
                             num_img_gen_tokens=G.N_IMG, max_new_tokens=G.MAX_NEW, img_ids_list=G.IMG_IDS,
                             eos_token_id=eos)
        what = f"{tag}/graph={graph}/{path}/rep={rep}"
        # the image block's ids come back rewritten to the <img_xxxxx> ids, in the oracle's output as in ours
        n_same = _check_ids(out["output_ids"].tolist(), ref["output_ids"].tolist(), ref["margins"].tolist(), what)
        assert n_same == G.MAX_NEW, "every margin is >= 5e-2 (precondition): all ids must match"
        info = agent.llm.last_run_info
        assert info["prompt_tokens"] == len(input_ids) > 16, "the prompt must be long enough for the MFMA prompt pass"
        assert info["graph"] == (graph and (rep > 0 or info["new_tokens"] > 2))
        if path == "mfma":                                 # the dequant scratch really ran: one buffer of the largest group
            assert agent.llm._w16 is not None and agent.llm._w16.numel() == 2 * agent.llm.wgu[0].numel()
        gate(f"mxfp4 fed-back hidden states, {what}", _rel(agent.llm.feat[:n_same - 1], ref["hidden"][:n_same - 1]), 3e-2)
        assert out["num_gen_imgs"] == 1 and bool(out["ids_gen_mask"][:G.N_IMG].all())
        gate(f"mxfp4 img_gen_feat, {what}", _rel(out["img_gen_feat"][0], ref["img_gen_feat"][0]), 3e-2)


def test_mxfp4_generate_batch_matches_each_prompts_oracle(tiny):
    """max_sequences = 4, three prompts of different lengths in one decode loop (MXFP4 llm_gemm16_kernel, the batched prompt
    pass through the dequant scratch), each against its own oracle run on the dequantised weights."""
    _precondition(tiny)
    G = tiny["G"]
    prompts = [make_prompt(G, *p) for p in BATCH_PROMPTS]
    assert [len(p[0]) for p in prompts] == [40, 52, 32]
    refs = [tiny["oracle"](p, 2) for p in prompts]
    for p, ref in zip(BATCH_PROMPTS, refs):               # on the CPU, before any GPU time is spent
        assert float(min(ref["margins"].tolist()[:G.N_IMG + 6])) >= 5e-2, (p, ref["margins"].tolist())
    agent = tiny["LVLM"](tiny["mk"](True, "mfma", 4), tiny["res_in"], tiny["res_out"])
    reqs = [dict(input_ids=ids[None], image_embeds=img.to(DEV), ids_cmp_mask=mask[None], num_img_gen_tokens=G.N_IMG,
                 max_new_tokens=G.MAX_NEW, img_ids_list=G.IMG_IDS, eos_token_id=2) for ids, mask, img in prompts]
    for rep in range(2):                                                                  # 2nd call replays the graph
        outs = agent.generate_batch(reqs)
        info = agent.llm.last_run_info
        assert info["sequences"] == 3 and info["prompt_tokens"] == [40, 52, 32]
        for k, (out, ref) in enumerate(zip(outs, refs)):
            what = f"batch prompt {k}/rep={rep}"
            n_same = _check_ids(out["output_ids"].tolist(), ref["output_ids"].tolist(), ref["margins"].tolist(), what)
            assert n_same >= G.N_IMG + 6, "the first N_IMG + 6 margins are >= 5e-2: those ids must match"
            gate(f"mxfp4 hidden states, {what}", _rel(agent.llm.feats[k, :n_same - 1], ref["hidden"][:n_same - 1]), 3e-2)
            assert out["num_gen_imgs"] >= 1 and bool(out["ids_gen_mask"][:G.N_IMG].all())
            gate(f"mxfp4 img_gen_feat, {what}", _rel(out["img_gen_feat"][0], ref["img_gen_feat"][0]), 3e-2)
    assert agent.llm.last_run_info["graph"]
