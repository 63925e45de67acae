"""The cases of the chain fast-forward tests (test_mllm_chain_ff_host.py, test_gpu_mllm_chain_ff.py) on the tiny model of
oracle/make_golden_mllm.py, and their fp32 CPU oracle (oracle/llama_ref.py), computed once per process.

Prompts are `test_gpu_mllm_batch.make_prompt`'s, except that a text-ending prompt drops the final <img>: the model then picks
the chain's first id by itself, somewhere inside a burst of token steps.  The chain's first id is an ordinary text id here
(209 or 26: ids the tiny model picks freely for these prompts), followed by the tiny model's image-token list."""
import functools

import torch

EOS, MAX_NEW = 2, 36
# name: (first chain id, (seed, n1, n2), text-ending, forced index ranges of the oracle, smallest free-choice margin)
CASES = {
    "mid_burst": (209, (31, 6, 7), True, [(4, 21)], 0.144),          # 209 picked at index 3
    "from_prompt": (209, (22, 17, 3), False, [(0, 16)], 0.065),      # the prompt ends in <img>: forced from index 0
    "two_blocks": (26, (50, 6, 7), True, [(7, 24), (27, 35)], 0.162),  # 26 picked at 6 and 26; the second block cut by max_new
    "neighbour": (209, (50, 6, 7), True, [], None),                  # never enters the chain; flip rule of test_gpu_mllm.py
}


def chain_of(name):
    from oracle import make_golden_mllm as G
    return [CASES[name][0]] + list(G.IMG_IDS)


def make_prompt(name):
    """[bos, n1 text, <img>, 16 placeholders, </img>, n2 text (, <img>)] -> ids, mask, image_embeds"""
    from oracle import make_golden_mllm as G
    _, (seed, n1, n2), text_ending, _, _ = CASES[name]
    g = torch.Generator().manual_seed(seed)
    t = lambda n: torch.randint(3, 590, (n,), generator=g).tolist()
    ids = [1] + t(n1) + [G.BOI] + G.IMG_IDS[1:-1] + [G.EOI] + t(n2) + ([] if text_ending else [G.BOI])
    mask = [False] * len(ids)
    for i in range(n1 + 2, n1 + 2 + G.N_IMG):
        mask[i] = True
    image_embeds = torch.randn(1, G.N_IMG, G.RES_IN["kv_dim"], generator=g)
    return torch.tensor(ids), torch.tensor(mask), image_embeds


@functools.lru_cache(maxsize=None)
def weights():
    from oracle import make_golden_mllm as G
    return G.tiny_weights(), G.tiny_resampler(G.RES_IN, 11), G.tiny_resampler(G.RES_OUT, 12)


@functools.lru_cache(maxsize=None)
def weights_mxfp4():
    """the tiny weights with the decoder's projection matrices seen through MXFP4 (what the mxfp4 engine computes with)"""
    from oracle import make_golden_mllm as G
    from diffsensei_amd.mllm import dequantize_rows_mxfp4, quantize_rows_mxfp4
    sd = dict(weights()[0])
    for i in range(G.TINY["num_hidden_layers"]):
        for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                  "mlp.down_proj"):
            k = f"model.layers.{i}.{n}.weight"
            sd[k] = dequantize_rows_mxfp4(*quantize_rows_mxfp4(sd[k]))
    return sd


@functools.lru_cache(maxsize=None)
def oracle(name, eos=EOS, max_new=MAX_NEW, chain_head=None, kv8=False, mxfp4=False):
    """`greedy_generate` of the case (chain_head: another first chain id; kv8: the fp8-cache forward of tests/_kv8_ref.py;
    mxfp4: on the dequantised MXFP4 weights) -> {"ids" (list), "hidden", "margins", "forced" (the indices that were no
    choice: the id before them - the last prompt id for index 0 - lies in chain[:-1]), "img_gen_feat" (the output resampler
    over the 16 hidden rows in front of every </img> that has them, or None)}"""
    import contextlib

    from oracle import llama_ref as R
    from oracle import make_golden_mllm as G
    from tests import _kv8_ref as K8
    sd, sd_in, sd_out = weights()
    ids, mask, img = make_prompt(name)
    chain = chain_of(name) if chain_head is None else [chain_head] + list(G.IMG_IDS)
    emb = sd["model.embed_tokens.weight"].float()[ids].clone()
    emb[mask] = R.qwen_resampler(sd_in, img.float(), G.RES_IN["num_heads"]).reshape(-1, emb.shape[-1])
    with (K8.kv8_oracle() if kv8 else contextlib.nullcontext()):
        g = R.greedy_generate(weights_mxfp4() if mxfp4 else sd, R.LlamaRefConfig(**G.TINY), emb, int(ids[-1]), chain, eos, max_new)
    out = g["ids"].tolist()
    prev = [int(ids[-1])] + out[:-1]
    blocks = [g["hidden"][e - G.N_IMG:e] for e, t in enumerate(out) if t == G.EOI and e >= G.N_IMG]
    feat = R.qwen_resampler(sd_out, torch.stack(blocks), G.RES_OUT["num_heads"]) if blocks else None
    return {"ids": out, "hidden": g["hidden"], "margins": g["margins"], "img_gen_feat": feat,
            "forced": [i for i, p in enumerate(prev) if p in chain[:-1]]}
