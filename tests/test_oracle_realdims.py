"""CPU: the oracle pinned to the reference's own modules at the model's REAL widths (tests/golden/realdim_<case>.npz).

The fixtures hold outputs only (oracle/make_golden.py realdims ran reference src/models/attention_processor.py and
src/models/resampler.py unmodified); inputs and weights are regenerated from oracle/realdim_cases.py, and a SHA-256 of what was
regenerated must equal the one stored beside the outputs.  Tolerances are test_oracle_golden.py's; the fp16-rounded oracle's
distance from the fixture is the yardstick tests/test_gpu_realdims.py quotes for the HIP product.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import realdim_cases as RC
from oracle.attention_ref import masked_ip_cross_attention, self_attention
from oracle.resampler_ref import resampler_forward

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROC = list(RC.PROCESSOR_CASES)
_half = lambda t: t.half().float()


@functools.lru_cache(maxsize=None)
def _case(name):
    return RC.resampler_case() if name == RC.RESAMPLER_CASE else RC.processor_case(name)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    g = np.load(os.path.join(GOLDEN, f"realdim_{name}.npz"))
    return {k: g[k] for k in g.files}


def _masked(c, rows, q=lambda t: t):
    w = c["cross"]
    return masked_ip_cross_attention(c["x"], c["enc"], c["bbox"], c["aspect_ratio"], w["wq"], w["wk"], w["wv"], w["wk_ip"],
                                     w["wv_ip"], w["wo"], w["bo"], c["heads"], c["scale"], c["num_ip_tokens"],
                                     c["num_dummy_tokens"], q=q, rows=rows)


def _self(c, rows, q=lambda t: t):
    w = c["self"]
    return self_attention(c["x"], w["wq"], w["wk"], w["wv"], w["wo"], w["bo"], c["heads"], q=q, rows=rows)


def _rel_max(y, ref):
    return ((y - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("name", PROC + [RC.RESAMPLER_CASE])
def test_regenerated_inputs_have_the_stored_digest(name):
    g = _fixture(name)
    assert str(g["case"]) == name and int(g["seed"]) == _case(name)["seed"]
    assert _case(name)["digest"] == str(g["digest"]), \
        f"{name}: oracle/realdim_cases.py no longer generates the inputs that tests/golden/realdim_{name}.npz was computed from"


@pytest.mark.parametrize("name", PROC)
def test_fixture_rows_are_the_generator_s(name):
    g, c = _fixture(name), _case(name)
    rows = g["rows"].tolist()
    H, W = c["hw"]
    assert rows == RC.fixture_rows(name) and len(rows) >= 24
    assert {0, 1, 127, 128, W - 1, W, c["N"] - W, c["N"] - 2, c["N"] - 1} <= set(rows)
    assert g["y_masked_ip"].shape == g["y_self"].shape == (RC.BATCH, len(rows), c["C"])
    # item 0: a stored row inside each box and one outside all of them; item 1 (all-zero boxes): only token (0, 0) is inside
    ins = torch.stack([RC._inside(H, W, b) for b in RC.BOXES[0]])[:, rows]
    assert bool(ins.any(1).all()) and bool((~ins.any(0)).any())
    assert [int(RC._inside(H, W, b).sum()) for b in RC.BOXES[1]] == [1] * 4


# c1280_32x32_sharp: logits of std ~ 16 make the fp32 softmax itself ill-conditioned (a logit error of 1e-6 relative moves a
# near-one-hot probability by 1e-5), so the oracle-vs-reference difference is larger there: measured 1.03e-5 (masked IP) and
# 9.7e-6 (self) max abs on max|y| 4.5 / 4.0, i.e. 2.4e-6 relative - the tolerance is that measurement x 3
_ATOL = {"c1280_32x32_sharp": 3.1e-5}


@pytest.mark.parametrize("name", PROC)
def test_masked_ip_oracle_matches_reference_rows(name):
    g, c = _fixture(name), _case(name)
    y = _masked(c, torch.tensor(g["rows"]).long())
    ref = torch.tensor(g["y_masked_ip"])
    print(f"{name}: masked-IP oracle vs reference max abs {(y - ref).abs().max():.3g}, max|y| {ref.abs().max():.3g}")
    assert torch.allclose(y, ref, atol=_ATOL.get(name, 2e-6), rtol=1e-5)


@pytest.mark.parametrize("name", PROC)
def test_self_attn_oracle_matches_reference_rows(name):
    g, c = _fixture(name), _case(name)
    y = _self(c, torch.tensor(g["rows"]).long())
    ref = torch.tensor(g["y_self"])
    print(f"{name}: self-attention oracle vs reference max abs {(y - ref).abs().max():.3g}, max|y| {ref.abs().max():.3g}")
    assert torch.allclose(y, ref, atol=_ATOL.get(name, 2e-6), rtol=1e-5)


def test_row_subset_is_the_full_oracle_s_rows():
    """`rows=` of the oracle is a restriction of its full output (the grid and mask are still those of all N tokens)."""
    name = "c1280_25x37"
    g, c = _fixture(name), _case(name)
    rows = torch.tensor(g["rows"]).long()
    assert torch.allclose(_masked(c, None)[:, rows], _masked(c, rows), atol=2e-6, rtol=1e-5)
    assert torch.allclose(_self(c, None)[:, rows], _self(c, rows), atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize("name", PROC)
def test_fp16_rounded_oracle_is_the_yardstick(name):
    """A condition on the CASES, not on the product: with fp16 rounding between ops the oracle stays below 2e-3 of max|y| from
    the reference.  Measured (max|err| / max|y|, rel-L2), masked IP then self-attention:
        c640_64x64         4.9e-4, 5.0e-4    3.8e-4, 2.6e-4
        c1280_32x32        6.2e-4, 5.0e-4    3.8e-4, 2.9e-4
        c1280_24x40        6.3e-4, 5.0e-4    4.3e-4, 2.9e-4
        c1280_25x37        5.5e-4, 5.0e-4    3.9e-4, 3.0e-4
        c1280_32x32_sharp  1.89e-3, 1.22e-3  1.78e-3, 1.36e-3   (near-one-hot softmax: a rounded logit moves whole rows)"""
    g, c = _fixture(name), _case(name)
    rows = torch.tensor(g["rows"]).long()
    for what, y, ref in (("masked IP", _masked(c, rows, _half), torch.tensor(g["y_masked_ip"])),
                         ("self", _self(c, rows, _half), torch.tensor(g["y_self"]))):
        e, l2 = _rel_max(y, ref), ((y - ref).norm() / ref.norm()).item()
        print(f"{name}: fp16-rounded {what} oracle vs reference: {e:.3g} of max|y|, rel-L2 {l2:.3g}")
        assert e < 2e-3, (name, what, e)


def test_resampler_oracle_matches_reference_at_the_model_dims():
    g, c = _fixture(RC.RESAMPLER_CASE), _case(RC.RESAMPLER_CASE)
    cfg = c["config"]
    nd, nq = cfg["num_dummy_tokens"], cfg["num_queries"]
    y = resampler_forward(c["sd"], c["x"], c["magi"], cfg["heads"], cfg["dim_head"])
    ref = torch.tensor(g["out"])
    assert y.shape == ref.shape == (1, nd + RC.RESAMPLER_CHARS * nq, cfg["output_dim"])
    print(f"Resampler oracle vs reference max abs {(y - ref).abs().max():.3g}, max|y| {ref.abs().max():.3g}")
    assert torch.allclose(y, ref, atol=1e-5, rtol=1e-5)
    assert torch.equal(ref[0, :nd], c["sd"]["dummy_tokens"])
    # absent characters (zeroed CLIP and Magi inputs): the stored rows are one such character's; the others repeat `out`
    ya = resampler_forward(c["sd"], c["x_absent"], c["magi_absent"], cfg["heads"], cfg["dim_head"])
    a0 = int(g["absent_character"])
    assert a0 in RC.RESAMPLER_ABSENT
    sl = lambda ch: slice(nd + ch * nq, nd + (ch + 1) * nq)
    for ch in range(RC.RESAMPLER_CHARS):
        want = torch.tensor(g["out_absent_rows"]) if ch in RC.RESAMPLER_ABSENT else ref[0, sl(ch)]
        assert torch.allclose(ya[0, sl(ch)], want, atol=1e-5, rtol=1e-5), ch
    # the yardstick for the HIP Resampler: measured 1.0e-3 of max|y|, rel-L2 9.7e-4 (absent rows 8.8e-4, 7.8e-4)
    yh = resampler_forward(c["sd"], c["x"], c["magi"], cfg["heads"], cfg["dim_head"], q=_half)
    e, l2 = _rel_max(yh, ref), ((yh - ref).norm() / ref.norm()).item()
    print(f"fp16-rounded Resampler oracle vs reference: {e:.3g} of max|y|, rel-L2 {l2:.3g}")
    assert e < 2e-3, e
