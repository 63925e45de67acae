"""Generate tests/golden/*.npz by EXECUTING the reference's importable modules (CPU, fp32).

Run in the build container only (needs /root/reference, which does not exist on the GPU box):

    python -m oracle.make_golden            # every fixture
    python -m oracle.make_golden layouts    # only ip_region_masks_layouts.npz
    python -m oracle.make_golden realdims   # only realdim_<case>.npz (real-width processors and Resampler)

Imports reference src/models/attention_processor.py and src/models/resampler.py unmodified (they depend
only on torch), drives them with seeded inputs through a duck-typed `attn` stub that has exactly the
attributes the processors touch (to_q/to_k/to_v/to_out/heads/spatial_norm/group_norm/norm_cross/
residual_connection/rescale_output_factor), and stores inputs, weights and outputs.  The oracle
(oracle/attention_ref.py, oracle/resampler_ref.py) and the HIP path are both tested against these files.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("DIFFSENSEI_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


class _AttnStub(nn.Module):
    """Stand-in for diffusers.models.attention_processor.Attention (only what the processors read)."""

    def __init__(self, dim, cross_dim, heads):
        super().__init__()
        self.to_q = nn.Linear(dim, dim, bias=False)
        self.to_k = nn.Linear(cross_dim, dim, bias=False)
        self.to_v = nn.Linear(cross_dim, dim, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(dim, dim, bias=True), nn.Dropout(0.0)])
        self.heads = heads
        self.spatial_norm = None
        self.group_norm = None
        self.norm_cross = False
        self.residual_connection = False
        self.rescale_output_factor = 1.0


MASK_CASES = [
    # name, H, W, bboxes [B,4,4]
    ("square32", 32, 32, [[[0.05, 0.10, 0.50, 0.95], [0.50, 0.10, 0.95, 0.95], [0, 0, 0, 0], [0, 0, 0, 0]],
                          [[0, 0, 0, 0]] * 4]),
    ("odd33_exact_half", 33, 33, [[[0.0, 0.0, 0.5, 0.5], [0.5, 0.5, 1.0, 1.0], [0.25, 0.25, 0.75, 0.75],
                                   [0.03125, 0.0625, 0.96875, 0.9375]]]),
    ("wide24x40", 24, 40, [[[0.1, 0.2, 0.4, 0.9], [0.35, 0.0, 0.8, 0.55], [0.9, 0.9, 1.0, 1.0], [0, 0, 0, 0]]]),
    ("tall48x32", 48, 32, [[[0.0, 0.0, 1.0, 1.0], [0.2, 0.3, 0.21, 0.31], [0.6, 0.1, 0.3, 0.9], [0.5, 0.5, 0.5, 0.5]]]),
    ("lvl16", 16, 16, [[[0.05, 0.10, 0.50, 0.95], [0.50, 0.10, 0.95, 0.95], [0, 0, 0, 0], [0, 0, 0, 0]]]),
    ("tiny8x12", 8, 12, [[[0.0, 0.0, 0.45, 1.0], [0.46, 0.0, 1.0, 1.0], [0.2, 0.2, 0.8, 0.8], [0.0, 0.5, 1.0, 0.5]]]),
]

# token layouts other than the model's 16 + 4 x 16: (num_dummy_tokens, tokens per character, max_num_ips); the first is the
# reference's constructor default (num_ip_tokens = 4, num_dummy_tokens = 4)
LAYOUT_CASES = [(4, 1, 4), (8, 8, 4), (16, 8, 8), (16, 20, 4)]
LAYOUT_GRIDS = [(7, 9), (18, 13)]


def write_layout_masks(processor_cls):
    """tests/golden/ip_region_masks_layouts.npz: the reference's prepare_attention_mask_ip at LAYOUT_CASES x LAYOUT_GRIDS on the
    box sets of oracle/ip_box_cases.py (three batch items, one head), int8 "masked" flags [3, N, num_dummy + num_ip]."""
    from oracle.ip_box_cases import box_cases
    out = {}
    for nd, tpi, k in LAYOUT_CASES:
        proc = processor_cls(hidden_size=64, cross_attention_dim=32, num_ip_tokens=k * tpi, num_dummy_tokens=nd)
        for h, w in LAYOUT_GRIDS:
            bbox = box_cases(h, w, k, 3)
            m = proc.prepare_attention_mask_ip(bbox, torch.zeros(3, h * w, 64), 1, h / w)
            name = f"d{nd}_t{tpi}_k{k}_{h}x{w}"
            out[name + "_bbox"] = bbox.numpy()
            out[name + "_layout"] = np.array([nd, tpi, k, h, w], dtype=np.int32)
            out[name + "_masked"] = (m[:, 0] < -1.0).numpy().astype(np.int8)
    np.savez_compressed(os.path.join(OUT, "ip_region_masks_layouts.npz"), **out)


def _save_npz(path, arrays):
    """np.savez_compressed with a fixed member date, so that two runs write the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as fh:
                np.lib.format.write_array(fh, np.asanyarray(v), allow_pickle=False)


def write_realdims(masked_cls, self_cls, resampler_cls):
    """tests/golden/realdim_<case>.npz: the reference's processors and Resampler at the model's real widths, on the inputs and
    weights of oracle/realdim_cases.py.  Stored: case name, seed, digest of the inputs, reference outputs in fp32 - for the
    processors the rows `fixture_rows(case)` of each batch item, all columns - and nothing else (the inputs are regenerated)."""
    from oracle import realdim_cases as RC
    total = 0
    for name in RC.PROCESSOR_CASES:
        c = RC.processor_case(name)
        rows = RC.fixture_rows(name)
        H, W = c["hw"]
        need = {0, 1, 127, 128, W - 1, W, c["N"] - W, c["N"] - 2, c["N"] - 1}
        assert need <= set(rows) and len(rows) >= 24 and len(set(rows)) == len(rows), name
        attn = _AttnStub(c["C"], c["cross_dim"], c["heads"])
        proc = masked_cls(hidden_size=c["C"], cross_attention_dim=c["cross_dim"], scale=c["scale"],
                          num_ip_tokens=c["num_ip_tokens"], num_dummy_tokens=c["num_dummy_tokens"])
        w = c["cross"]
        with torch.no_grad():
            attn.to_q.weight.copy_(w["wq"]); attn.to_k.weight.copy_(w["wk"]); attn.to_v.weight.copy_(w["wv"])
            attn.to_out[0].weight.copy_(w["wo"]); attn.to_out[0].bias.copy_(w["bo"])
            proc.to_k_ip.weight.copy_(w["wk_ip"]); proc.to_v_ip.weight.copy_(w["wv_ip"])
            y = proc(attn, c["x"], encoder_hidden_states=c["enc"], bbox=c["bbox"], aspect_ratio=c["aspect_ratio"])
            attn1 = _AttnStub(c["C"], c["C"], c["heads"])
            w = c["self"]
            attn1.to_q.weight.copy_(w["wq"]); attn1.to_k.weight.copy_(w["wk"]); attn1.to_v.weight.copy_(w["wv"])
            attn1.to_out[0].weight.copy_(w["wo"]); attn1.to_out[0].bias.copy_(w["bo"])
            y1 = self_cls()(attn1, c["x"])
        assert y.shape == y1.shape == c["x"].shape and y.dtype == y1.dtype == torch.float32
        path = os.path.join(OUT, f"realdim_{name}.npz")
        _save_npz(path, {"case": np.array(name), "seed": np.int64(c["seed"]), "digest": np.array(c["digest"]),
                         "rows": np.array(rows, dtype=np.int32), "y_masked_ip": y[:, rows].numpy(),
                         "y_self": y1[:, rows].numpy()})
        total += os.path.getsize(path)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))

    c = RC.resampler_case()
    cfg = c["config"]
    rs = resampler_cls(**cfg).eval()
    rs.load_state_dict(c["sd"], strict=True)
    with torch.no_grad():
        out = rs(c["x"], c["magi"])
        out_absent = rs(c["x_absent"], c["magi_absent"])
    nd, nq = cfg["num_dummy_tokens"], cfg["num_queries"]
    assert out.shape == (1, nd + RC.RESAMPLER_CHARS * nq, cfg["output_dim"])
    # characters are processed independently: zeroing some leaves the others' rows (and the dummy rows) as they were, and
    # every zeroed character gives the same 16 rows - one of them is all the second input adds
    sl = lambda ch: slice(nd + ch * nq, nd + (ch + 1) * nq)
    present = [ch for ch in range(RC.RESAMPLER_CHARS) if ch not in RC.RESAMPLER_ABSENT]
    assert torch.equal(out_absent[:, :nd], out[:, :nd])
    for ch in present:
        assert torch.allclose(out_absent[:, sl(ch)], out[:, sl(ch)], atol=1e-6, rtol=0), ch
    a0 = RC.RESAMPLER_ABSENT[0]
    for ch in RC.RESAMPLER_ABSENT[1:]:
        assert torch.allclose(out_absent[:, sl(ch)], out_absent[:, sl(a0)], atol=1e-6, rtol=0), ch
    path = os.path.join(OUT, f"realdim_{RC.RESAMPLER_CASE}.npz")
    _save_npz(path, {"case": np.array(RC.RESAMPLER_CASE), "seed": np.int64(c["seed"]), "digest": np.array(c["digest"]),
                     "out": out.numpy(), "absent_character": np.int32(a0), "out_absent_rows": out_absent[0, sl(a0)].numpy()})
    total += os.path.getsize(path)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    assert total < 3 * (1 << 20), total
    print(f"wrote realdim_*.npz: {total} bytes together")


def main():
    sys.path.insert(0, REF)
    from src.models.attention_processor import AttnProcessor2_0, MaskedIPAttnProcessor2_0
    from src.models.resampler import Resampler
    os.makedirs(OUT, exist_ok=True)
    if sys.argv[1:] == ["layouts"]:   # only the layout masks (no random numbers involved; the other fixtures stay as they are)
        write_layout_masks(MaskedIPAttnProcessor2_0)
        return
    if sys.argv[1:] == ["realdims"]:  # only tests/golden/realdim_*.npz (seeded by oracle/realdim_cases.py, not by torch)
        write_realdims(MaskedIPAttnProcessor2_0, AttnProcessor2_0, Resampler)
        return
    torch.manual_seed(0)

    # ---- 1. region masks (reference prepare_attention_mask_ip), stored as uint8 "masked" flags
    proc = MaskedIPAttnProcessor2_0(hidden_size=64, cross_attention_dim=32, num_ip_tokens=64, num_dummy_tokens=16)
    out = {}
    for name, h, w, boxes in MASK_CASES:
        bbox = torch.tensor(boxes, dtype=torch.float32)
        hs = torch.zeros(bbox.shape[0], h * w, 64)
        m = proc.prepare_attention_mask_ip(bbox, hs, 1, h / w)      # [B,1,N,80]
        out[name + "_bbox"] = bbox.numpy()
        out[name + "_hw"] = np.array([h, w], dtype=np.int32)
        out[name + "_masked"] = (m[:, 0] < -1.0).numpy().astype(np.uint8)
    np.savez_compressed(os.path.join(OUT, "ip_region_masks.npz"), **out)

    # ---- 2. masked IP cross-attention processor end to end (small dims, SDXL token counts 77 + 80)
    dim, xdim, heads, hh, ww, b = 128, 64, 2, 16, 16, 2
    attn = _AttnStub(dim, xdim, heads)
    proc = MaskedIPAttnProcessor2_0(hidden_size=dim, cross_attention_dim=xdim, scale=0.6, num_ip_tokens=64,
                                    num_dummy_tokens=16)
    x = torch.randn(b, hh * ww, dim)
    enc = torch.randn(b, 77 + 80, xdim)
    bbox = torch.tensor([[[0.05, 0.10, 0.50, 0.95], [0.50, 0.10, 0.95, 0.95], [0, 0, 0, 0], [0, 0, 0, 0]],
                         [[0, 0, 0, 0]] * 4], dtype=torch.float32)
    with torch.no_grad():
        y = proc(attn, x, encoder_hidden_states=enc, bbox=bbox, aspect_ratio=hh / ww)
    np.savez_compressed(
        os.path.join(OUT, "masked_ip_attn.npz"),
        x=x.numpy(), enc=enc.numpy(), bbox=bbox.numpy(), hw=np.array([hh, ww], np.int32), heads=np.int32(heads),
        scale=np.float32(0.6), wq=attn.to_q.weight.detach().numpy(), wk=attn.to_k.weight.detach().numpy(),
        wv=attn.to_v.weight.detach().numpy(), wk_ip=proc.to_k_ip.weight.detach().numpy(),
        wv_ip=proc.to_v_ip.weight.detach().numpy(), wo=attn.to_out[0].weight.detach().numpy(),
        bo=attn.to_out[0].bias.detach().numpy(), y=y.numpy())

    # ---- 3. self-attention processor
    attn1 = _AttnStub(dim, dim, heads)
    sp = AttnProcessor2_0()
    with torch.no_grad():
        y1 = sp(attn1, x)
    np.savez_compressed(
        os.path.join(OUT, "self_attn.npz"), x=x.numpy(), heads=np.int32(heads),
        wq=attn1.to_q.weight.detach().numpy(), wk=attn1.to_k.weight.detach().numpy(),
        wv=attn1.to_v.weight.detach().numpy(), wo=attn1.to_out[0].weight.detach().numpy(),
        bo=attn1.to_out[0].bias.detach().numpy(), y=y1.numpy())

    # ---- 4. Resampler (small dims; structure identical to configs/model/diffsensei.yaml)
    rs = Resampler(dim=128, depth=2, dim_head=64, heads=2, num_queries=16, num_dummy_tokens=16, embedding_dim=96,
                   magi_embedding_dim=64, output_dim=256, ff_mult=4).eval()
    xi = torch.randn(1, 4, 17, 96)
    mg = torch.randn(1, 4, 64)
    with torch.no_grad():
        yo = rs(xi, mg)
        yz = rs(torch.zeros_like(xi), torch.zeros_like(mg))
    d = {"in_x": xi.numpy(), "in_magi": mg.numpy(), "out": yo.numpy(), "out_zero": yz.numpy()}
    for k, v in rs.state_dict().items():
        d["sd." + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "resampler.npz"), **d)

    # ---- 5. region masks at other token layouts
    write_layout_masks(MaskedIPAttnProcessor2_0)

    # ---- 6. processors and Resampler at the model's real widths (last: building the modules draws from torch's generator)
    write_realdims(MaskedIPAttnProcessor2_0, AttnProcessor2_0, Resampler)
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
