"""Shared by tests/test_long_prompt_host.py and tests/test_gpu_long_prompt.py: the stand-in CLIP tokenizers of the chunked-prompt
tests.  `ChunkTokenizer` is tests/test_gpu_pipeline.py's `_FakeTokenizer` (words hashed to ids, BOS / EOS like CLIP) with what
chunking needs of a real CLIPTokenizer: `add_special_tokens=False`, the three special ids as attributes, and padding with its
OWN pad id - tokenizer 1 pads with its EOS like CLIP-L, tokenizer 2 with id 0 like OpenCLIP-bigG."""
import torch

from tests.test_gpu_pipeline import _FakeTokenizer


class ChunkTokenizer(_FakeTokenizer):
    def __init__(self, pad=None, **kw):
        super().__init__(**kw)
        self.bos_token_id, self.eos_token_id = self.bos, self.eos
        self.pad_token_id = self.eos if pad is None else pad

    def words(self, text):
        n = len(text.split())
        return super().__call__(text, max_length=n + 2).input_ids[0, 1:n + 1].tolist()      # the parent's hashing, nothing cut

    def __call__(self, text, padding=None, max_length=77, truncation=True, return_tensors="pt", add_special_tokens=True):
        words = self.words(text)
        if not add_special_tokens:
            return type("Enc", (), {"input_ids": words if truncation is False else words[:max_length]})()
        ids = [self.bos] + words[: max_length - 2] + [self.eos]
        ids += [self.pad_token_id] * (max_length - len(ids))
        return type("Enc", (), {"input_ids": torch.tensor([ids])})()


def tokenizers():
    return ChunkTokenizer(), ChunkTokenizer(pad=0)


def prompt(n_words, seed=0):
    """A prompt of exactly n_words words (one id each), different for different seeds."""
    return " ".join(f"w{seed}x{(i * 7 + seed) % 977}" for i in range(n_words))
