"""Oracle (test infrastructure only): character-box sets that probe the region mask of MaskedIPAttnProcessor2_0.

`box_cases(h, w, max_ips, batch)` returns [batch, max_ips, 4] fp32 boxes (x1, y1, x2, y2) for an h x w token grid, a different
set in every batch item.  oracle/make_golden.py feeds them to the reference's own `prepare_attention_mask_ip`
(tests/golden/ip_region_masks_layouts.npz) and tests/test_gpu_masked_ip_attn.py feeds the same sets to the HIP kernel.

Kinds (a batch item takes the first `max_ips` entries of its row of `_ORDER`):
  wave1    the tokens of query rows 32..63 of the first 128-row tile and no others: whole grid rows where some lie inside that
           range (16 x 16: exactly rows 32..63), else the piece of one grid row.  Edges halfway between grid coordinates, -1 / 2
           where there is no neighbour - so only the second wavefront of a block has this character's keys open
  ov_a/b   two boxes that overlap: a token open to two characters
  one      exactly one token, x1 = x2 and y1 = y2 on its fp32 grid coordinate
  empty    x1 > x2: no token
  outside  reaches outside [0, 1] on three sides
  zeros    (0, 0, 0, 0): the reference's "no character" padding - token (0, 0) IS inside (inclusive edges)
  edge     all four edges equal to fp32 grid coordinates `torch.linspace` produces, x1 / y1 from the first half of its formula
           (start + i * step, i < n/2), x2 / y2 from the second (end - (n-1-i) * step): inclusive comparisons decide by one ulp
  full     (0, 0, 1, 1): every token inside, the dummy keys closed everywhere
"""
from __future__ import annotations

import torch

_ORDER = (
    ("wave1", "ov_a", "ov_b", "one", "empty", "outside", "zeros", "edge"),
    ("edge", "full", "zeros", "empty", "ov_a", "wave1", "one", "outside"),
    ("outside", "ov_b", "zeros", "zeros", "wave1", "ov_a", "edge", "one"),
)


def _mid(c: torch.Tensor, i: int, below: bool) -> float:
    """halfway between grid coordinate i and its lower (upper) neighbour; -1 (2) where there is none"""
    j = i - 1 if below else i + 1
    if j < 0:
        return -1.0
    if j >= c.numel():
        return 2.0
    return 0.5 * (float(c[i]) + float(c[j]))


def box_cases(h: int, w: int, max_ips: int, batch: int, first: int = 0) -> torch.Tensor:
    assert 1 <= max_ips <= 8
    xs, ys = torch.linspace(0, 1, steps=w), torch.linspace(0, 1, steps=h)   # fp32, as the reference builds them
    r0, r1 = (32 + w - 1) // w, min(64, h * w) // w - 1                      # whole grid rows inside tokens [32, 64)
    if r1 >= r0:
        wave1 = [-1.0, _mid(ys, r0, True), 2.0, _mid(ys, r1, False)]
    else:
        r = 32 // w
        c0, c1 = 32 - r * w, min(w - 1, 63 - r * w)
        wave1 = [_mid(xs, c0, True), _mid(ys, r, True), _mid(xs, c1, False), _mid(ys, r, False)]
    tr, tc = h // 3, (2 * w) // 3
    xh = (w + 1) // 2                                                        # first index of linspace's second half
    kinds = {
        "wave1": wave1,
        "ov_a": [0.10, 0.15, 0.60, 0.70],
        "ov_b": [0.40, 0.45, 0.90, 0.95],
        "one": [float(xs[tc]), float(ys[tr]), float(xs[tc]), float(ys[tr])],
        "empty": [0.80, 0.10, 0.20, 0.90],
        "outside": [-0.50, -0.25, 0.35, 1.50],
        "zeros": [0.0, 0.0, 0.0, 0.0],
        "edge": [float(xs[max(w // 2 - 1, 0) // 2]), float(ys[max(h // 2 - 1, 0)]),
                 float(xs[min(xh + (w - 1 - xh) // 2, w - 1)]), float(ys[min((h + 1) // 2, h - 1)])],
        "full": [0.0, 0.0, 1.0, 1.0],
    }
    out = torch.empty(batch, max_ips, 4, dtype=torch.float32)
    for b in range(batch):
        for k in range(max_ips):
            out[b, k] = torch.tensor(kinds[_ORDER[(first + b) % len(_ORDER)][k]], dtype=torch.float32)
    return out
