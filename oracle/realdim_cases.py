"""Frozen inputs and weights for the attention processors and the image-projection Resampler at the model's real widths.

One processor case at C = 1280 has ~13 M weights and the Resampler 84 M, so nothing here can be committed as data: every tensor is
regenerated from a seed on both sides - by oracle/make_golden.py (which feeds them to the reference's own modules and stores only
the outputs, tests/golden/realdim_<case>.npz) and by the tests (which feed them to the oracle and to the HIP product).

Numbers come from `numpy.random.RandomState(seed).standard_normal`: the legacy MT19937 stream, which NumPy keeps frozen.  Each
tensor is scaled by its fan-in (matrices K**-0.5, biases 0.05-0.1, norm gains 1 + 0.1 n, latents dim**-0.5, dummy tokens 1), rounded
to fp16 and handed out as fp32, so that an fp32 reference and an fp16 engine read identical values.  Every case carries a SHA-256
over the little-endian fp16 bytes of all it generated, in generation order: the fixture stores it, and a test that regenerates
something else fails by name instead of comparing against outputs of other inputs.

This module is the project's own code: it imports nothing from the reference and is read by CPU and GPU tests alike.
"""
from __future__ import annotations

import hashlib
from typing import Dict, List, Tuple

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------- processors
CROSS_DIM = 2048
NUM_TEXT, NUM_DUMMY, NUM_IP, MAX_IPS = 77, 16, 64, 4     # 77 text + 16 dummy + 4 x 16 character tokens
IP_SCALE = 0.6
BATCH = 2
FIXTURE_ROWS = 24                                         # rows of each batch item kept in the fixture

# item 0: two overlapping boxes, one nested inside their overlap, one tiny box in the bottom-right corner;
# item 1: four all-zero boxes - the reference's no-character row, where only token (0, 0) is "inside"
BOXES = [[[0.05, 0.10, 0.60, 0.90], [0.40, 0.20, 0.95, 0.95], [0.45, 0.30, 0.55, 0.60], [0.97, 0.97, 1.00, 1.00]],
         [[0.0, 0.0, 0.0, 0.0]] * 4]

# name -> (C, heads, grid H, grid W, gain on to_q / to_k / to_k_ip, seed)
PROCESSOR_CASES: Dict[str, Tuple[int, int, int, int, float, int]] = {
    "c640_64x64": (640, 10, 64, 64, 1.0, 6401),           # the 1024^2 level that dominates the forward
    "c1280_32x32": (1280, 20, 32, 32, 1.0, 12801),
    "c1280_24x40": (1280, 20, 24, 40, 1.0, 12802),        # non-square aspect ratio; last 128-row query tile half full
    "c1280_25x37": (1280, 20, 25, 37, 1.0, 12803),        # 925 tokens: no multiple of 8, grid inferred from N and H / W
    "c1280_32x32_sharp": (1280, 20, 32, 32, 4.0, 12801),  # c1280_32x32 with q / k weights x 4: logit std ~ 16, near one-hot softmax
}

# ---------------------------------------------------------------------------------------------- Resampler
RESAMPLER_CASE = "resampler_model"
RESAMPLER_SEED = 20481
RESAMPLER_CONFIG = dict(dim=1280, depth=4, dim_head=64, heads=20, num_queries=16, num_dummy_tokens=16, embedding_dim=1280,
                        magi_embedding_dim=768, output_dim=2048, ff_mult=4)
RESAMPLER_CHARS, RESAMPLER_SEQ = 4, 257                   # characters per panel, CLIP tokens per character (+ 1 Magi token)
RESAMPLER_ABSENT = (2, 3)                                 # characters zeroed in the second input


class _Stream:
    """Seeded normal numbers, rounded through fp16, with a running digest of everything handed out."""

    def __init__(self, seed: int):
        self.rs = np.random.RandomState(seed)
        self.sha = hashlib.sha256()

    def normal(self, shape, scale: float = 1.0, shift: float = 0.0, gain: float = 1.0) -> torch.Tensor:
        a = (shift + scale * self.rs.standard_normal(shape)).astype("<f2")
        if gain != 1.0:
            a = (a.astype(np.float32) * gain).astype("<f2")
        self.sha.update(np.ascontiguousarray(a).tobytes())
        return torch.from_numpy(a.astype(np.float32))

    def digest(self) -> str:
        return self.sha.hexdigest()


def processor_case(name: str) -> dict:
    """Inputs and weights of one processor case (fp32 tensors holding fp16-exact values).

    `cross`: wq, wk, wv, wk_ip, wv_ip, wo, bo of MaskedIPAttnProcessor2_0 (nn.Linear layout [out, in]);
    `self`: wq, wk, wv, wo, bo of AttnProcessor2_0, drawn from the same stream after them."""
    C, heads, H, W, gain, seed = PROCESSOR_CASES[name]
    s = _Stream(seed)
    N = H * W
    x = s.normal((BATCH, N, C))
    enc = s.normal((BATCH, NUM_TEXT + NUM_DUMMY + NUM_IP, CROSS_DIM))
    cross = {"wq": s.normal((C, C), C ** -0.5, gain=gain), "wk": s.normal((C, CROSS_DIM), CROSS_DIM ** -0.5, gain=gain),
             "wv": s.normal((C, CROSS_DIM), CROSS_DIM ** -0.5),
             "wk_ip": s.normal((C, CROSS_DIM), CROSS_DIM ** -0.5, gain=gain),
             "wv_ip": s.normal((C, CROSS_DIM), CROSS_DIM ** -0.5), "wo": s.normal((C, C), C ** -0.5),
             "bo": s.normal((C,), 0.1)}
    self_w = {"wq": s.normal((C, C), C ** -0.5, gain=gain), "wk": s.normal((C, C), C ** -0.5, gain=gain),
              "wv": s.normal((C, C), C ** -0.5), "wo": s.normal((C, C), C ** -0.5), "bo": s.normal((C,), 0.1)}
    return {"name": name, "seed": seed, "C": C, "heads": heads, "hw": (H, W), "N": N, "aspect_ratio": H / W,
            "scale": IP_SCALE, "num_ip_tokens": NUM_IP, "num_dummy_tokens": NUM_DUMMY, "cross_dim": CROSS_DIM,
            "x": x, "enc": enc, "bbox": torch.tensor(BOXES, dtype=torch.float32), "cross": cross, "self": self_w,
            "digest": s.digest()}


def _inside(H: int, W: int, box) -> torch.Tensor:
    """[N] bool: token (i, j) at (x, y) = (linspace(0, 1, W)[j], linspace(0, 1, H)[i]) lies in `box`, both ends inclusive."""
    xs = torch.linspace(0, 1, steps=W).repeat(H)
    ys = torch.linspace(0, 1, steps=H).repeat_interleave(W)
    x1, y1, x2, y2 = (torch.tensor(v, dtype=torch.float32) for v in box)
    return (xs >= x1) & (xs <= x2) & (ys >= y1) & (ys <= y2)


def _nearest(H: int, W: int, allowed: torch.Tensor, cx: float, cy: float) -> int:
    xs = torch.linspace(0, 1, steps=W).repeat(H)
    ys = torch.linspace(0, 1, steps=H).repeat_interleave(W)
    d = (xs - cx) ** 2 + (ys - cy) ** 2
    d = torch.where(allowed, d, torch.full_like(d, float("inf")))
    return int(torch.argmin(d))


def fixture_rows(name: str) -> List[int]:
    """The query rows whose reference outputs the fixture keeps (the same set for both batch items), sorted: the corners of the
    first two 128-row tiles, of the first and last grid line and of the sequence; for each box of item 0 the token nearest its
    centre among those inside it; the token nearest the grid's centre among those outside every box; a seeded choice for the rest."""
    _, _, H, W, _, seed = PROCESSOR_CASES[name]
    N = H * W
    rows = [0, 1, 127, 128, W - 1, W, N - W, N - 2, N - 1]
    ins = [_inside(H, W, b) for b in BOXES[0]]
    for b, m in zip(BOXES[0], ins):
        assert bool(m.any()), (name, b)
        rows.append(_nearest(H, W, m, (b[0] + b[2]) / 2, (b[1] + b[3]) / 2))
    outside = ~torch.stack(ins).any(0)
    rows.append(_nearest(H, W, outside, 0.5, 0.5))
    chosen = sorted(set(rows))
    for r in np.random.RandomState(seed + 1).permutation(N):
        if len(chosen) >= FIXTURE_ROWS:
            break
        if int(r) not in chosen:
            chosen.append(int(r))
    return sorted(chosen)


def resampler_state_names() -> List[str]:
    """State-dict keys of the perceiver Resampler at RESAMPLER_CONFIG, in generation order."""
    names = ["latents", "proj_in.weight", "proj_in.bias", "proj_in_magi.weight", "proj_in_magi.bias"]
    for i in range(RESAMPLER_CONFIG["depth"]):
        a, f = f"layers.{i}.0.", f"layers.{i}.1."
        names += [a + "norm1.weight", a + "norm1.bias", a + "norm2.weight", a + "norm2.bias", a + "to_q.weight",
                  a + "to_kv.weight", a + "to_out.weight", f + "0.weight", f + "0.bias", f + "1.weight", f + "3.weight"]
    return names + ["proj_out.weight", "proj_out.bias", "norm_out.weight", "norm_out.bias", "dummy_tokens"]


def _resampler_shape(k: str) -> tuple:
    c = RESAMPLER_CONFIG
    d, inner, ffi, out = c["dim"], c["dim_head"] * c["heads"], int(c["dim"] * c["ff_mult"]), c["output_dim"]
    fixed = {"latents": (1, c["num_queries"], d), "proj_in.weight": (d, c["embedding_dim"]), "proj_in.bias": (d,),
             "proj_in_magi.weight": (d, c["magi_embedding_dim"]), "proj_in_magi.bias": (d,), "proj_out.weight": (out, d),
             "proj_out.bias": (out,), "norm_out.weight": (out,), "norm_out.bias": (out,),
             "dummy_tokens": (c["num_dummy_tokens"], out)}
    if k in fixed:
        return fixed[k]
    leaf = k.split(".", 2)[2]
    return {"0.norm1.weight": (d,), "0.norm1.bias": (d,), "0.norm2.weight": (d,), "0.norm2.bias": (d,),
            "0.to_q.weight": (inner, d), "0.to_kv.weight": (2 * inner, d), "0.to_out.weight": (d, inner),
            "1.0.weight": (d,), "1.0.bias": (d,), "1.1.weight": (ffi, d), "1.3.weight": (d, ffi)}[leaf]


def resampler_case() -> dict:
    """State dict (reference key names), the full input `x [1, 4, 257, 1280]`, `magi [1, 4, 768]`, and the same two with the
    characters RESAMPLER_ABSENT zeroed (`x_absent`, `magi_absent`)."""
    c = RESAMPLER_CONFIG
    s = _Stream(RESAMPLER_SEED)
    sd = {}
    for k in resampler_state_names():
        shp = _resampler_shape(k)
        if len(shp) == 1 and k.endswith(".weight"):
            sd[k] = s.normal(shp, 0.1, shift=1.0)             # norm gains
        elif k.endswith(".bias"):
            sd[k] = s.normal(shp, 0.05)
        elif k == "latents":
            sd[k] = s.normal(shp, c["dim"] ** -0.5)
        elif k == "dummy_tokens":
            sd[k] = s.normal(shp)
        else:
            sd[k] = s.normal(shp, shp[1] ** -0.5)
    x = s.normal((1, RESAMPLER_CHARS, RESAMPLER_SEQ, c["embedding_dim"]))
    magi = s.normal((1, RESAMPLER_CHARS, c["magi_embedding_dim"]))
    xa, ma = x.clone(), magi.clone()
    for ch in RESAMPLER_ABSENT:
        xa[:, ch] = 0
        ma[:, ch] = 0
    return {"name": RESAMPLER_CASE, "seed": RESAMPLER_SEED, "config": dict(c), "sd": sd, "x": x, "magi": magi,
            "x_absent": xa, "magi_absent": ma, "digest": s.digest()}


def resampler_batch_input(bsz: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """A further seeded input of `bsz` panels (not part of the fixture; compared with the oracle at test time)."""
    c = RESAMPLER_CONFIG
    s = _Stream(seed)
    return (s.normal((bsz, RESAMPLER_CHARS, RESAMPLER_SEQ, c["embedding_dim"])),
            s.normal((bsz, RESAMPLER_CHARS, c["magi_embedding_dim"])))
