"""CPU: `oracle.attention_ref.ip_region_mask` at token layouts other than the model's 16 + 4 x 16 is pinned to outputs of the
reference's own `prepare_attention_mask_ip` (tests/golden/ip_region_masks_layouts.npz, written by
`python -m oracle.make_golden layouts` from the unmodified reference module), and the box sets of oracle/ip_box_cases.py do
what their names say on every grid tests/test_gpu_masked_ip_attn.py uses them on."""
import os

import numpy as np
import pytest
import torch

from oracle.attention_ref import ip_region_mask, mask_grid_size
from oracle.ip_box_cases import _ORDER, box_cases

GRIDS = [(7, 9), (18, 13), (16, 16), (24, 40), (1, 40), (20, 34)]


def test_layout_masks_bit_exact(golden_dir):
    g = np.load(os.path.join(golden_dir, "ip_region_masks_layouts.npz"))
    names = sorted({k[: -len("_bbox")] for k in g.files if k.endswith("_bbox")})
    assert len(names) == 8
    seen = set()
    for n in names:
        nd, tpi, k, h, w = (int(v) for v in g[n + "_layout"])
        seen.add((nd, tpi, k))
        bbox = torch.tensor(g[n + "_bbox"])
        assert torch.equal(bbox, box_cases(h, w, k, 3)), n             # the GPU test runs the kernel on these very boxes
        assert mask_grid_size(h * w, h / w) == (h, w)
        m = ip_region_mask(bbox, h * w, 1, h / w, k * tpi, nd)
        masked = (m[:, 0] < -1).numpy().astype(np.int8)
        assert masked.shape == g[n + "_masked"].shape == (3, h * w, nd + k * tpi)
        assert (masked == g[n + "_masked"]).all(), n
    assert seen == {(4, 1, 4), (8, 8, 4), (16, 8, 8), (16, 20, 4)}


def _inside(bbox, h, w):
    """[B, N, K] bool from the oracle's mask with one key per character and one dummy key"""
    k = bbox.shape[1]
    m = ip_region_mask(bbox, h * w, 1, h / w, k, 1)[:, 0]
    return m[:, :, 1:] == 0, m[:, :, 0] == 0


@pytest.mark.parametrize("h,w", GRIDS)
def test_box_cases_do_what_they_say(h, w):
    assert mask_grid_size(h * w, h / w) == (h, w)
    n = h * w
    bbox = box_cases(h, w, 8, 3)
    inside, dummy_open = _inside(bbox, h, w)
    assert torch.equal(dummy_open, ~inside.any(-1))
    xs, ys = torch.linspace(0, 1, steps=w), torch.linspace(0, 1, steps=h)
    for b in range(3):
        for k, kind in enumerate(_ORDER[b]):
            idx = inside[b, :, k].nonzero().flatten().tolist()
            if kind == "wave1":
                assert idx and all(32 <= i < 64 for i in idx), (kind, idx)
                if (h, w) == (16, 16):
                    assert idx == list(range(32, 64))
            elif kind == "one":
                assert idx == [(h // 3) * w + (2 * w) // 3]
            elif kind == "empty":
                assert idx == []
            elif kind == "zeros":
                assert idx == [0]
            elif kind == "outside":
                assert idx and all(i % w <= 0.35 * (w - 1) + 1e-6 for i in idx) and len(idx) % h == 0
            elif kind == "edge":
                x1, y1, x2, y2 = bbox[b, k].tolist()
                cols = [j for j in range(w) if x1 <= float(xs[j]) <= x2]
                rows = [i for i in range(h) if y1 <= float(ys[i]) <= y2]
                # the edges are grid coordinates: the edge tokens themselves are inside
                assert float(xs[cols[0]]) == x1 and float(xs[cols[-1]]) == x2 and float(ys[rows[0]]) == y1 and float(ys[rows[-1]]) == y2
                assert cols[0] < w / 2 <= cols[-1] and (h == 1 or rows[0] < h / 2 <= rows[-1])
                assert idx == [i * w + j for i in rows for j in cols]
    # item 0 holds the overlapping pair: some token is open to both characters (grids with more than one row)
    if h > 1:
        assert (inside[0, :, 1] & inside[0, :, 2]).any()
    # the full-image box of item 1 closes the dummy keys everywhere; items 0 and 2 keep tokens that lie in no box
    assert not dummy_open[1].any() and dummy_open[0].any() and dummy_open[2].any()
    assert n == inside.shape[1]
