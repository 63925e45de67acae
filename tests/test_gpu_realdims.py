"""GPU: the drop-in attention processors and the image-projection Resampler at the model's REAL widths, against outputs of the
reference's own modules (tests/golden/realdim_<case>.npz) and against the fp32 oracle on every row.

Inputs and weights are regenerated from oracle/realdim_cases.py (fp16-exact values, so the fp32 reference and the fp16 product read
the same numbers); the fixtures hold only reference outputs.  Every comparison is max|err| / max|ref| and relative L2, both through
tests/_gates.gate.  Each tolerance below is 3 x the value measured on MI355X against the reference fixture (never above the 1e-2
bar the toy-width fixture tests used to have); the measured figure stands beside it, and beside that the YARDSTICK: the distance of
the fp16-rounded oracle from the same fixture (tests/test_oracle_realdims.py), i.e. what fp16 storage between ops costs by itself.
Log of the run that set them: profiles/realdims_measured_gates.jsonl.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import realdim_cases as RC
from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROC = list(RC.PROCESSOR_CASES)

# (max|err| / max|ref|, rel-L2) gates per case = 3 x measured vs the reference fixture rows (largest over the kernel variants run);
# the same pair gates the all-rows comparison with the oracle (measured there: within 1.2 x the row figures, sharp self 1.7 x).
#                                    gate                 measured              yardstick (fp16-rounded oracle)
MASKED_IP_TOL = {
    "c640_64x64":        (1.5e-3, 1.4e-3),    # 5.00e-4, 4.80e-4      4.9e-4, 5.0e-4
    "c1280_32x32":       (1.6e-3, 1.4e-3),    # 5.28e-4, 4.69e-4      6.2e-4, 5.0e-4
    "c1280_24x40":       (1.5e-3, 1.4e-3),    # 5.08e-4, 4.71e-4      6.3e-4, 5.0e-4
    "c1280_25x37":       (1.5e-3, 1.4e-3),    # 4.95e-4, 4.71e-4      5.5e-4, 5.0e-4
    "c1280_32x32_sharp": (6.0e-3, 3.6e-3),    # 2.00e-3, 1.22e-3      1.89e-3, 1.22e-3
}
# measured: self_attn_sp_kernel (attn_variant 0 / 3), which is the larger of the two everywhere; the flash kernels (1 / 2) measure
# 3.8e-4 .. 4.1e-4, 2.6e-4 .. 3.1e-4 on the plain cases and 1.73e-3, 1.36e-3 on sharp.  Sharp on self_attn_sp_kernel is 1.2 x its
# yardstick on the fixture rows and 2.0 x (3.6e-3) over all rows: that kernel rounds Q, pre-multiplied by scale * log2(e), to f16
# once, so its logit error grows with |logit| (std 16 here) - the behaviour test_self_attention_sp_deferred_rescale["hot"] allows for.
SELF_TOL = {
    "c640_64x64":        (1.2e-3, 8.2e-4),    # 3.96e-4, 2.74e-4      3.8e-4, 2.6e-4
    "c1280_32x32":       (1.2e-3, 9.6e-4),    # 4.13e-4, 3.21e-4      3.8e-4, 2.9e-4
    "c1280_24x40":       (1.4e-3, 9.8e-4),    # 4.72e-4, 3.27e-4      4.3e-4, 2.9e-4
    "c1280_25x37":       (1.2e-3, 9.9e-4),    # 4.00e-4, 3.29e-4      3.9e-4, 3.0e-4
    "c1280_32x32_sharp": (6.4e-3, 4.8e-3),    # 2.15e-3, 1.60e-3      1.78e-3, 1.36e-3
}
RESAMPLER_TOL = (3.3e-3, 3.0e-3)              # 1.105e-3, 9.89e-4     1.0e-3, 9.7e-4
RESAMPLER_ABSENT_TOL = (2.9e-3, 2.4e-3)       # 9.74e-4, 7.94e-4      8.8e-4, 7.8e-4
RESAMPLER_BATCH2_TOL = (3.2e-3, 3.0e-3)       # 1.075e-3, 9.97e-4 (vs the fp32 oracle: this input has no fixture)


@functools.lru_cache(maxsize=None)
def _case(name):
    return RC.resampler_case() if name == RC.RESAMPLER_CASE else RC.processor_case(name)


def _fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"realdim_{name}.npz"))
    c = _case(name)
    assert str(g["digest"]) == c["digest"], f"{name}: regenerated inputs are not the ones the fixture was computed from"
    return g


@functools.lru_cache(maxsize=None)
def _oracle_full(name, kind):
    """fp32 oracle on ALL rows (CPU, once per case), in chunks of query rows so that no N x N score matrix is held."""
    from oracle.attention_ref import masked_ip_cross_attention, self_attention
    c = _case(name)
    out = []
    for r0 in range(0, c["N"], 512):
        rows = torch.arange(r0, min(r0 + 512, c["N"]))
        if kind == "masked_ip":
            w = c["cross"]
            out.append(masked_ip_cross_attention(c["x"], c["enc"], c["bbox"], c["aspect_ratio"], w["wq"], w["wk"], w["wv"],
                                                 w["wk_ip"], w["wv_ip"], w["wo"], w["bo"], c["heads"], c["scale"],
                                                 c["num_ip_tokens"], c["num_dummy_tokens"], rows=rows))
        else:
            w = c["self"]
            out.append(self_attention(c["x"], w["wq"], w["wk"], w["wv"], w["wo"], w["bo"], c["heads"], rows=rows))
    return torch.cat(out, dim=1)


def _figures(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max()).item(), ((got - ref).norm() / ref.norm()).item()


def _gate_pair(what, got, ref, tol):
    e, l2 = _figures(got, ref)
    gate(f"{what}: max|err|/max|ref|", e, tol[0])
    gate(f"{what}: rel-L2", l2, tol[1])


_h = lambda t: t.half().to(DEV)


def _attention_weights(c, kind):
    from diffsensei_amd.attention_processor import AttentionWeights
    w = c["cross" if kind == "masked_ip" else "self"]
    attn = AttentionWeights(c["C"], c["cross_dim"] if kind == "masked_ip" else None, c["heads"], DEV)
    attn.to_q.weight, attn.to_k.weight, attn.to_v.weight = _h(w["wq"]), _h(w["wk"]), _h(w["wv"])
    attn.to_out[0].weight, attn.to_out[0].bias = _h(w["wo"]), _h(w["bo"])
    return attn


@pytest.mark.parametrize("name", PROC)
def test_masked_ip_processor_at_real_dims(hip_lib, golden_dir, name):
    """MaskedIPAttnProcessor2_0 with the reference's call protocol: C 640 / 1280, cross dim 2048, 77 + 16 + 4 x 16 context tokens,
    overlapping / nested / corner boxes and a no-character batch item.  ip_attn_variant 0 (what a user gets), 3 (all 96 key slots)
    and - where N % 256 == 0 - 2 (the LDS-DMA ring kernel) must give the same bits."""
    from diffsensei_amd import _lib
    from diffsensei_amd.attention_processor import MaskedIPAttnProcessor2_0, mask_grid_size
    lib = _lib.load()
    c, g = _case(name), _fixture(golden_dir, name)
    assert mask_grid_size(c["N"], c["aspect_ratio"]) == c["hw"]         # the grid is inferred from N and H / W alone
    attn = _attention_weights(c, "masked_ip")
    proc = MaskedIPAttnProcessor2_0(c["C"], c["cross_dim"], scale=c["scale"], num_ip_tokens=c["num_ip_tokens"],
                                    num_dummy_tokens=c["num_dummy_tokens"], device=DEV)
    proc.to_k_ip.weight, proc.to_v_ip.weight = _h(c["cross"]["wk_ip"]), _h(c["cross"]["wv_ip"])
    x, enc, bbox = _h(c["x"]), _h(c["enc"]), c["bbox"].to(DEV)
    out = {}
    try:
        for v in (0, 3) + ((2,) if c["N"] % 256 == 0 else ()):
            assert lib.ds_set_option(b"ip_attn_variant", v) == 0
            out[v] = proc(attn, x, encoder_hidden_states=enc, bbox=bbox, aspect_ratio=c["aspect_ratio"]).clone()
    finally:
        lib.ds_set_option(b"ip_attn_variant", 0)
    for v, y in out.items():
        assert torch.equal(y, out[0]), f"{name}: ip_attn_variant {v} differs from the default kernel"
    y = out[0].float().cpu()
    rows = torch.tensor(g["rows"]).long()
    _gate_pair(f"masked-IP processor {name} vs reference rows", y[:, rows], torch.tensor(g["y_masked_ip"]), MASKED_IP_TOL[name])
    _gate_pair(f"masked-IP processor {name} vs oracle, all rows", y, _oracle_full(name, "masked_ip"), MASKED_IP_TOL[name])


@pytest.mark.parametrize("name", PROC)
def test_self_attn_processor_at_real_dims(hip_lib, golden_dir, name):
    """AttnProcessor2_0 on the same hidden states with its own weights, attn_variant 0-3.  Variant 0 is the dispatch's own choice:
    ((N + 255) // 256) * B * heads >= 128 -> self_attn_sp_kernel (= variant 3).  At batch 2 that is 320 blocks for c640_64x64
    and 160 for every C = 1280 case (N = 925 .. 1024: 4 x 2 x 20), so all five cases resolve to self_attn_sp_kernel; variants 1 / 2
    are the 32- / 64-row flash kernels, bit-identical to each other."""
    from diffsensei_amd import _lib
    from diffsensei_amd.attention_processor import AttnProcessor2_0
    lib = _lib.load()
    c, g = _case(name), _fixture(golden_dir, name)
    assert ((c["N"] + 255) // 256) * RC.BATCH * c["heads"] >= 128
    attn = _attention_weights(c, "self")
    x = _h(c["x"])
    out = {}
    try:
        for v in (0, 1, 2, 3):
            assert lib.ds_set_option(b"attn_variant", v) == 0
            out[v] = AttnProcessor2_0()(attn, x).clone()
    finally:
        lib.ds_set_option(b"attn_variant", 0)
    assert torch.equal(out[1], out[2]), f"{name}: 32-row and 64-row flash kernels differ"
    assert torch.equal(out[0], out[3]), f"{name}: the dispatch did not choose self_attn_sp_kernel"
    rows = torch.tensor(g["rows"]).long()
    for v in (0, 1, 2, 3):
        y = out[v].float().cpu()
        _gate_pair(f"self processor {name} attn_variant {v} vs reference rows", y[:, rows], torch.tensor(g["y_self"]),
                   SELF_TOL[name])
        _gate_pair(f"self processor {name} attn_variant {v} vs oracle, all rows", y, _oracle_full(name, "self"), SELF_TOL[name])


# ------------------------------------------------------------------------------------------------ Resampler
@functools.lru_cache(maxsize=None)
def _resampler(depth=None):
    """The HIP Resampler at the model's dims with the case's weights; `depth` < 4 keeps the first layers only."""
    from diffsensei_amd.resampler import Resampler
    cfg = dict(_case(RC.RESAMPLER_CASE)["config"])
    if depth is None:
        return Resampler(**cfg, device=DEV).load_state_dict(_case(RC.RESAMPLER_CASE)["sd"])
    cfg["depth"] = depth
    return Resampler(**cfg, device=DEV).load_state_dict(_resampler().state_dict())


def test_resampler_at_the_model_dims(hip_lib, golden_dir):
    """dim 1280, depth 4, 20 heads of 64, 16 queries, 257 CLIP + 1 Magi token per character, output 2048: M = 64 GEMMs against
    K = 1280 / 5120 with GELU and residual, M = 4 x 274 into N = 2560, small_attn_kernel with 20 heads and 274 keys, LayerNorm at
    1280 / 2048 over four fp16 residual layers."""
    c, g = _case(RC.RESAMPLER_CASE), _fixture(golden_dir, RC.RESAMPLER_CASE)
    cfg = c["config"]
    nd, nq = cfg["num_dummy_tokens"], cfg["num_queries"]
    rs = _resampler()
    y = rs(c["x"], c["magi"])
    assert y.shape == (1, nd + RC.RESAMPLER_CHARS * nq, cfg["output_dim"]) and y.dtype == torch.float16
    assert torch.equal(y[0, :nd].cpu(), c["sd"]["dummy_tokens"].half()), "dummy rows are not fp16(dummy_tokens)"
    _gate_pair("Resampler (model dims) vs reference, all 80 rows", y, torch.tensor(g["out"]), RESAMPLER_TOL)
    # absent characters: zeroed CLIP and Magi inputs; every such character gives the stored rows, the others repeat `out`
    ya = rs(c["x_absent"], c["magi_absent"])
    a0 = int(g["absent_character"])
    sl = lambda ch: slice(nd + ch * nq, nd + (ch + 1) * nq)
    for ch in range(RC.RESAMPLER_CHARS):
        if ch in RC.RESAMPLER_ABSENT:
            assert torch.equal(ya[0, sl(ch)], ya[0, sl(a0)]), ch
        else:
            assert torch.equal(ya[0, sl(ch)], y[0, sl(ch)]), f"character {ch} changed when others were zeroed"
    _gate_pair("Resampler (model dims), absent character vs reference", ya[0, sl(a0)], torch.tensor(g["out_absent_rows"]),
               RESAMPLER_ABSENT_TOL)


def test_resampler_at_the_model_dims_two_panels_and_depth_drift(hip_lib):
    """bsz = 2 (8 characters: M = 128 latent rows, 2192 key / value rows) against the fp32 oracle, and - printed, not gated - how
    the error grows with the number of layers (same weights, first 1 .. 4 layers)."""
    from oracle.resampler_ref import resampler_forward
    c = _case(RC.RESAMPLER_CASE)
    cfg = c["config"]
    x2, m2 = RC.resampler_batch_input(2, RC.RESAMPLER_SEED + 1)
    ref = resampler_forward(c["sd"], x2, m2, cfg["heads"], cfg["dim_head"])
    y = _resampler()(x2, m2)
    assert y.shape == ref.shape == (2, 80, cfg["output_dim"])
    _gate_pair("Resampler (model dims) bsz 2 vs oracle", y, ref, RESAMPLER_BATCH2_TOL)
    drift = []
    for depth in (1, 2, 3, 4):
        sd = {k: v for k, v in c["sd"].items() if not k.startswith("layers.") or int(k.split(".")[1]) < depth}
        ref_d = resampler_forward(sd, c["x"], c["magi"], cfg["heads"], cfg["dim_head"])
        e, l2 = _figures(_resampler(depth)(c["x"], c["magi"]), ref_d)
        drift.append(f"{depth}: {e:.2e} / {l2:.2e}")
    print("Resampler drift by depth (max|err|/max|ref| / rel-L2 vs fp32 oracle): " + ", ".join(drift))
