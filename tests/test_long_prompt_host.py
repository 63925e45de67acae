"""Host: chunked prompt encoding - the chunker, the `max_prompt_chunks` argument checks, and the chunk count in the serving
keys and in the up-front checks of a batch / a continuous run.  Nothing here needs a GPU: no encoder runs before these checks."""
import pytest
import torch

from tests._long_prompt_common import prompt, tokenizers

BOS, EOS = 998, 999


@pytest.mark.parametrize("pad", [EOS, 0])
@pytest.mark.parametrize("n", [0, 1, 75, 76, 150, 151, 400])
def test_chunk_token_ids(n, pad):
    from diffsensei_amd.pipeline import chunk_count, chunk_token_ids
    ids = list(range(1, n + 1))
    for max_chunks in (1, 2, 3, 4):
        k_all = max(1, -(-n // 75))
        k, dropped = chunk_count(n, max_chunks)
        assert k == min(k_all, max_chunks) and dropped == max(0, n - 75 * k)
        out = chunk_token_ids(ids, BOS, EOS, pad, max_chunks)
        assert out.dtype == torch.int64 and out.shape == (k, 77)
        for c in range(k):
            part = ids[75 * c:75 * (c + 1)]
            row = out[c].tolist()
            assert row[0] == BOS and row[1:1 + len(part)] == part and row[1 + len(part)] == EOS
            assert row[2 + len(part):] == [pad] * (75 - len(part))
        kept = [v for c in range(k) for v in out[c, 1:76].tolist()][:min(n, 75 * k)]
        assert kept == ids[:75 * k]                                   # the tail is what is dropped, nothing else
    assert chunk_count(n, 4) == ({0: 1, 1: 1, 75: 1, 76: 2, 150: 2, 151: 3, 400: 4}[n], 100 if n == 400 else 0)


@pytest.mark.parametrize("n", [0, 1, 40, 75])
def test_one_chunk_is_the_padded_ids_of_today(n):
    """Up to 75 ids the one chunk equals `tok(text, padding="max_length", max_length=77, truncation=True)`, for the tokenizer
    that pads with its EOS and for the one that pads with 0."""
    from diffsensei_amd.pipeline import DiffSenseiPipeline, chunk_token_ids
    text = prompt(n)
    for tok in tokenizers():
        today = tok(text, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
        raw = DiffSenseiPipeline._raw_ids(tok, text)
        assert len(raw) == n
        for max_chunks in (1, 3):
            assert torch.equal(chunk_token_ids(raw, tok.bos_token_id, tok.eos_token_id, tok.pad_token_id, max_chunks), today)


def _host_pipe():
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import tiny_config
    t1, t2 = tokenizers()
    return DiffSenseiPipeline(None, None, None, t1, t2, EulerDiscreteScheduler(), UNetMangaModel(tiny_config(), device="cpu"), None)


@pytest.fixture(scope="module")
def pipe():
    return _host_pipe()


@pytest.mark.parametrize("bad", [0, 5, -1, 2.0, "2", None, True])
def test_max_prompt_chunks_argument_errors(pipe, bad):
    """Anything but an integer in 1..4 is a ValueError before any encoder runs - this pipeline has none to run."""
    with pytest.raises(ValueError, match="max_prompt_chunks"):
        pipe("a panel", height=128, width=128, max_prompt_chunks=bad)
    with pytest.raises(ValueError, match="max_prompt_chunks"):
        pipe.generate_batch([dict(prompt="a panel", height=128, width=128), dict(prompt="b", height=128, width=128, max_prompt_chunks=bad)])
    with pytest.raises(ValueError, match="max_prompt_chunks"):
        pipe.generate_continuous([dict(prompt="b", height=128, width=128, max_prompt_chunks=bad)], slots=2)


def test_prompt_embeds_lengths(pipe):
    cfg = pipe.unet.config
    pooled = torch.zeros(1, 128)
    for n, neg, msg in ((0, None, "1..384"), (385, None, "1..384"), (154, 77, "same length")):
        with pytest.raises(ValueError, match=msg):
            pipe(None, height=128, width=128, prompt_embeds=torch.zeros(1, n, cfg.cross_attention_dim), pooled_prompt_embeds=pooled,
                 negative_prompt_embeds=None if neg is None else torch.zeros(1, neg, cfg.cross_attention_dim))


def test_prompt_chunk_count(pipe):
    long, short = prompt(180), prompt(40)
    assert pipe.prompt_chunk_count(dict(prompt=short)) == 1
    assert pipe.prompt_chunk_count(dict(prompt=long)) == 1                                   # the default truncates, as before
    assert [pipe.prompt_chunk_count(dict(prompt=long, max_prompt_chunks=m)) for m in (1, 2, 3, 4)] == [1, 2, 3, 3]
    assert pipe.prompt_chunk_count(dict(prompt=short, max_prompt_chunks=4)) == 1
    assert pipe.prompt_chunk_count(dict(prompt=short, prompt_2=long, max_prompt_chunks=4)) == 3   # the maximum over the tokenizers
    assert pipe.prompt_chunk_count(dict(prompt=short, negative_prompt=long, max_prompt_chunks=2)) == 2   # and, under CFG, the negatives
    assert pipe.prompt_chunk_count(dict(prompt=short, negative_prompt=long, max_prompt_chunks=2, guidance_scale=1.0)) == 2
    assert pipe.prompt_chunk_count(dict(prompt_embeds=torch.zeros(1, 231, 8))) == 3


def test_serving_keys_separate_chunk_counts(pipe):
    from diffsensei_amd.serving import BucketBatcher, bucket_key, continuous_key, plan_batches
    base = dict(height=128, width=128, num_inference_steps=4)
    plain, one = dict(base, prompt=prompt(40)), dict(base, prompt=prompt(40), max_prompt_chunks=3)
    three, two = dict(base, prompt=prompt(180), max_prompt_chunks=3), dict(base, prompt=prompt(180), max_prompt_chunks=2)
    chunks = pipe.prompt_chunk_count
    for key in (lambda r: bucket_key(r, False, chunks), lambda r: bucket_key(r, True, chunks), lambda r: continuous_key(r, chunks)):
        ks = [key(r) for r in (one, two, three)]
        assert len(set(ks)) == 3 and [k[-1] for k in ks] == [("chunks", 1), ("chunks", 2), ("chunks", 3)]
        assert key(dict(three, prompt=prompt(160, seed=1))) == key(three)                   # another prompt of the same count shares
    # a request without the field keeps the key it had
    assert bucket_key(plain) == (128, 128, 4, 5.0, 1.0) and bucket_key(plain, True) == (128, 128, 4, True)
    assert continuous_key(plain) == (128, 128, True, None)
    # direct embeddings: 77 tokens is the key of today, another length its own bucket
    pe = lambda n: dict(base, prompt_embeds=torch.zeros(1, n, 8))
    assert bucket_key(pe(77)) == bucket_key(plain) and bucket_key(pe(154))[-1] == ("chunks", 2) == continuous_key(pe(154))[-1]
    with pytest.raises(ValueError, match="tokenizers"):
        bucket_key(three)                                                                    # the count of a text prompt needs them
    with pytest.raises(ValueError, match="max_prompt_chunks"):
        bucket_key(dict(base, prompt="x", max_prompt_chunks=7), False, chunks)
    assert plan_batches([one, three, dict(one), two, dict(three)], 8, None, True, chunks) == [[0, 2], [1, 4], [3]]
    b = BucketBatcher(pipe, mix_scales=True)
    assert [b.submit(**r) for r in (one, three)] == [0, 1]


def test_mixed_chunk_counts_are_refused_up_front(pipe):
    base = dict(height=128, width=128, num_inference_steps=4)
    reqs = [dict(base, prompt=prompt(40), max_prompt_chunks=3), dict(base, prompt=prompt(180), max_prompt_chunks=3)]
    with pytest.raises(ValueError, match=r"request 1 has 3 prompt chunks \(231 text tokens\), request 0 has 1 \(77\)"):
        pipe._check_continuous(reqs, 4)
    with pytest.raises(ValueError, match=r"request 1 has 3 prompt chunks .* request 0 has 1"):
        pipe.generate_continuous(reqs, slots=4)
    with pytest.raises(ValueError, match=r"request 1 has 3 prompt chunks .* request 0 has 1"):
        pipe.generate_batch(reqs)
