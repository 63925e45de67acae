"""The cases of test_gpu_attention_bits.py: every instantiation of the flash / fused cross-attention kernels of csrc/attention.hip
and csrc/attention_sp.hip (`self_attn_kernel<1>`, `<2>`, `self_attn_sp_kernel`, `ip_attn_kernel` four-wave with and without T16
and the eight-wave ring, `ip_attn_long_kernel`, `ip_region_flags_kernel`) at the smallest shapes that cross every seam of their
softmax paths, staging and stores, and the sha256 of every output as the kernels gave it BEFORE their row store, IP-side region
logic, Q load, panel staging and softmax passes were moved into shared device functions (tests/golden/attention_bits.json).
The family's other tests compare the variants with one another or with fp64 references at measured tolerances, which a reordered
add inside a shared piece passes; this one does not.

No random generator: every operand is an integer formula, k / 64 with a per-channel power-of-two scale, exact in f16.

    python -m tests._attention_bits_cases [path]     # writes the fixture: run on the build whose bits are to be the record

Seams.  ip_attn_kernel: token layouts (n_dummy, tok_per_ip, max_ips) (16, 16, 4) = 80 IP keys (grouped biases; with 77 text keys
the T16 instantiation under ip_attn_variant 1, the plain one under 3), (16, 20, 4) = 96 (per-key biases), (8, 8, 4) = 40 (two key
blocks), (16, 16, 2) = 48 (the later characters' keys never open); text keys 77 / 96 / 40; grids 18 x 13 (N 234: partial last tile
and wave), 9 x 7 (N 63: one partly filled wave; W - 1 = 6 is the width whose reciprocal rounds off), 16 x 16 and 32 x 32 (N % 256
== 0: the ring); one and eight query tiles per block, and on 32 x 32 with B * heads = 2 the ip_attn_min_blocks at which the
launcher's rule gives FOUR (the ring's three slots all cycle); a host scalar, a device scalar and per-row IP scales (distinct, one
negative); q / out / key panels as column slices of wider buffers.  Boxes per batch row: overlapping boxes + a box with x1 == x2
exactly on a grid coordinate + an empty one; all boxes empty (dummies only: whole key blocks are skipped); one small box.
ip_attn_long_kernel: 97 / 154 / 192 / 231 / 308 / 384 text keys (2, 3, 4 panels; a last panel of 1 key, full last panels, half
blocks wholly past Lt), N 234 and 512, one and eight tiles per block, both scale sources, text panels with strides of their own,
text keys of the last panel scaled by 4 (the row maximum moves there: alpha != 1), and one text panel through the C entry point.
Self-attention: Nq = Nk 64 / 200 / 320 and Nq 200 with Nk 77 under attn_variant 1 / 2 / 3 / 4, once with a wide output stride."""
import collections
import functools
import hashlib
import json
import os
import sys

import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_bits.json")
LAYOUT = {"L80": (16, 16, 4), "L96": (16, 20, 4), "L40": (8, 8, 4), "L48": (16, 16, 2)}   # (n_dummy, tok_per_ip, max_ips)
ONE, EIGHT = 1 << 20, 1                                  # ip_attn_min_blocks: one query tile per block / as many as eight
# ip_attn_variant 0..3 / "long"; grid (mask_h, mask_w); mb: ip_attn_min_blocks, or "four" (found from the launcher's rule);
# scale: host | dev (device scalar) | rows; wide: operands are column slices of wider buffers; boost: last text panel x 4;
# capi: through ds_masked_ip_attn_long_f16 itself (one text panel)
IP = collections.namedtuple("IP", "variant layout Lt grid B heads mb scale wide boost capi", defaults=(False, False, False))
SELF = collections.namedtuple("SELF", "variant Nq Nk wide")
FLAGS = collections.namedtuple("FLAGS", "grid B max_ips")


def _ip_short(v):
    c = [IP(v, lay, Lt, (18, 13), 3, 2, ONE, "rows" if Lt == 96 else "host") for lay in LAYOUT for Lt in (77, 96, 40)]
    c += [IP(v, "L80", 77, (18, 13), 3, 2, EIGHT, "dev"), IP(v, "L80", 77, (9, 7), 3, 2, EIGHT, "rows"),
          IP(v, "L96", 96, (9, 7), 3, 1, ONE, "host"), IP(v, "L80", 77, (16, 16), 3, 2, EIGHT, "rows"),
          IP(v, "L80", 77, (32, 32), 2, 1, "four", "rows"), IP(v, "L80", 77, (18, 13), 3, 2, ONE, "rows", True),
          IP(v, "L96", 40, (18, 13), 3, 2, EIGHT, "host", True)]
    return c


def _groups():
    g = {"ip-v1": _ip_short(1), "ip-v3": _ip_short(3)}
    g["ip-v2"] = ([IP(2, lay, Lt, (16, 16), 3, 2, ONE, sc) for lay, Lt, sc in (("L80", 77, "host"), ("L96", 96, "rows"), ("L40", 40, "dev"))] +
                  [IP(2, lay, Lt, (32, 32), 2, 1, "four", sc) for lay, Lt, sc in (("L80", 77, "rows"), ("L96", 40, "host"), ("L48", 96, "rows"))] +
                  [IP(2, "L80", 77, (32, 32), 2, 1, ONE, "host"), IP(2, "L40", 77, (32, 32), 2, 1, EIGHT, "rows"),
                   IP(2, "L80", 77, (16, 16), 3, 2, ONE, "rows", True)])
    lts = (97, 154, 192, 231, 308, 384)
    g["ip-long"] = ([IP("long", "L80", Lt, (18, 13), 3, 2, ONE, "rows" if k % 2 else "host") for k, Lt in enumerate(lts)] +
                    [IP("long", "L80", Lt, (16, 32), 2, 2, EIGHT, "host" if k % 2 else "rows") for k, Lt in enumerate(lts)] +
                    [IP("long", lay, 154, (18, 13), 3, 2, EIGHT, "dev") for lay in ("L96", "L40", "L48")] +
                    [IP("long", "L80", 231, (18, 13), 3, 2, ONE, "rows", True), IP("long", "L96", 97, (9, 7), 3, 1, EIGHT, "host", True),
                     IP("long", "L80", 154, (18, 13), 3, 2, ONE, "host", False, True),
                     IP("long", "L80", 308, (16, 32), 2, 2, EIGHT, "rows", False, True),
                     IP("long", "L80", 77, (18, 13), 3, 2, ONE, "host", False, False, True),
                     IP("long", "L96", 96, (16, 32), 2, 2, EIGHT, "dev", False, False, True)])
    for v in (1, 2, 3, 4):
        g[f"self-v{v}"] = [SELF(v, 64, 64, False), SELF(v, 200, 200, False), SELF(v, 320, 320, False), SELF(v, 200, 77, False),
                           SELF(v, 200, 200, True)]
    g["flags"] = [FLAGS((9, 7), 3, 4), FLAGS((18, 13), 3, 2)]
    return g


GROUPS = _groups()


def case_name(group, case):
    f = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("T" if v is True else "F" if v is False else str(v))
    return group + ":" + "-".join(f(v) for v in case)


def tiles_per_block(tiles, bh, min_blocks, cap_by_tiles):
    """the launcher's rule: double the query tiles per block while the grid keeps min_blocks blocks"""
    qt = 1
    while qt < 8 and (not cap_by_tiles or qt * 2 <= tiles) and -(-tiles // (2 * qt)) * bh >= min_blocks:
        qt *= 2
    return qt


def min_blocks_for(case):
    if case.mb != "four":
        return case.mb
    rows = 256 if case.variant in (2, "long") else 128
    tiles, bh = -(-case.grid[0] * case.grid[1] // rows), case.B * case.heads
    mb = [m for m in range(1, 65) if tiles_per_block(tiles, bh, m, case.variant == 2) == 4]
    assert mb, case
    return mb[0]


def _formula(shape, mults, seed):
    """k / 64 * 2^-(last index % 3), k = (sum idx_i * mult_i + seed) % 251 - 125: exact in f16, |value| < 2"""
    acc = torch.full(shape, seed, dtype=torch.int64)
    for d, (n, m) in enumerate(zip(shape, mults)):
        view = [1] * len(shape)
        view[d] = n
        acc = acc + (torch.arange(n, dtype=torch.int64) * m).view(view)
    last = torch.arange(shape[-1], dtype=torch.int64).view([1] * (len(shape) - 1) + [shape[-1]])
    v = (acc % 251 - 125).float() / 64 * torch.pow(2.0, -(last % 3).float())
    assert torch.equal(v.half().float(), v)
    return v.half()


def boxes(grid, B, max_ips):
    """[B, max_ips, 4] fp32 (x1, y1, x2, y2).  Row 0: two overlapping boxes, a box with x1 == x2 exactly on a grid coordinate, an
    empty box; row 1: every box empty; row 2: one small box, the others empty.  (max_ips 2: the first two of each.)"""
    xs = torch.linspace(0, 1, grid[1])
    edge = float(xs[grid[1] // 3])
    empty = [0.6, 0.6, 0.4, 0.4]
    rows = [[[0.05, 0.10, 0.60, 0.95], [0.40, 0.30, 0.95, 0.80], [edge, 0.20, edge, 0.90], empty],
            [empty, empty, empty, empty],
            [empty, [0.70, 0.05, 0.98, 0.45], empty, empty]]
    if max_ips == 2:
        rows[0] = [rows[0][0], rows[0][2]]
    return torch.tensor([r[:max_ips] for r in rows[:B]], dtype=torch.float32)


def _slice_of_wide(t, pad):
    """the same values as a column slice (dim 2) of a buffer `pad` columns wider on both sides"""
    wide = torch.zeros((t.shape[0], t.shape[1], t.shape[2] + 2 * pad), dtype=t.dtype, device=t.device)
    wide[:, :, pad:pad + t.shape[2]] = t
    return wide[:, :, pad:pad + t.shape[2]]


@functools.lru_cache(maxsize=None)
def ip_operands(N, B, heads, Ltp, boost):
    """host operands: q [B,N,C], text keys [B,Ltp,C] / values [B,C,Ltp], IP keys [B,96,C] / values [B,C,96]"""
    C = heads * 64
    kt = _formula((B, Ltp, C), (389, 113, 43), 3)
    if boost:
        kt[:, Ltp - 96:, :] *= 4          # exact: |k| < 8
    return {"q": _formula((B, N, C), (977, 131, 29), 7), "kt": kt, "vtt": _formula((B, C, Ltp), (211, 89, 53), 1),
            "ki": _formula((B, 96, C), (337, 61, 17), 5), "vti": _formula((B, C, 96), (151, 73, 37), 9)}


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        assert torch.isfinite(t.float()).all()
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_ip(case):
    from diffsensei_amd import _lib, ops
    L = _lib.load()
    n_dummy, tpi, max_ips = LAYOUT[case.layout]
    Li, N, C = n_dummy + tpi * max_ips, case.grid[0] * case.grid[1], case.heads * 64
    long = case.variant == "long"
    Ltp = 96 * (-(-case.Lt // 96)) if long else 96
    o = {k: v.cuda() for k, v in ip_operands(N, case.B, case.heads, Ltp, case.boost).items()}
    bbox = boxes(case.grid, case.B, max_ips).cuda()
    out = torch.zeros((case.B, N, C), dtype=torch.float16, device="cuda")
    if case.wide:
        o["q"], out = _slice_of_wide(o["q"], 64), _slice_of_wide(out, 32)
        if long:                                       # the text panels alone: strides of their own
            o["kt"] = _slice_of_wide(o["kt"], 8)
        else:                                          # text and IP panels share their strides: one stacked buffer each
            k2 = torch.cat([o["kt"], o["ki"]], dim=2).contiguous()
            v2 = torch.cat([o["vtt"], o["vti"]], dim=1).contiguous()
            o["kt"], o["ki"], o["vtt"], o["vti"] = k2[:, :, :C], k2[:, :, C:], v2[:, :C], v2[:, C:]
    scales = torch.tensor([0.75, -0.5, 1.25][:case.B], dtype=torch.float32, device="cuda")
    dev = {"host": None, "dev": scales[:1].contiguous(), "rows": scales}[case.scale]
    assert L.ds_set_option(b"ip_attn_variant", 0 if long else case.variant) == 0
    assert L.ds_set_option(b"ip_attn_min_blocks", min_blocks_for(case)) == 0
    try:
        if case.capi:
            assert Ltp == 96 and case.scale != "rows"
            rc = L.ds_masked_ip_attn_long_f16(o["q"].data_ptr(), C, o["kt"].data_ptr(), o["vtt"].data_ptr(), o["ki"].data_ptr(),
                                              o["vti"].data_ptr(), bbox.data_ptr(), out.data_ptr(), C, case.B, case.heads, N, case.Lt, 1,
                                              Li, n_dummy, tpi, max_ips, case.grid[0], case.grid[1], 0.125, 0.6,
                                              None if dev is None else dev.data_ptr(), 0, 0, 0, 0, 0, 0,
                                              torch.cuda.current_stream().cuda_stream)
            assert rc == 0, L.ds_last_error().decode()
        else:
            ops.masked_ip_attention(o["q"], o["kt"], o["vtt"], o["ki"], o["vti"], bbox, case.heads, case.grid, 0.6, Lt=case.Lt, Li=Li,
                                    n_dummy=n_dummy, tok_per_ip=tpi, out=out, ip_scale_dev=dev)
    finally:
        assert L.ds_set_option(b"ip_attn_variant", 0) == 0
        assert L.ds_set_option(b"ip_attn_min_blocks", 1024) == 0
    return _digest(out)


@functools.lru_cache(maxsize=None)
def self_operands(Nq, Nk):
    B, heads = 2, 2
    return {"q": _formula((B, Nq, heads * 64), (977, 131, 29), 7), "k": _formula((B, Nk, heads * 64), (389, 113, 43), 3),
            "vt": _formula((B, heads, 64, (Nk + 7) // 8 * 8), (211, 97, 89, 53), 1)}


def run_self(case):
    from diffsensei_amd import _lib
    L = _lib.load()
    B, heads, C = 2, 2, 128
    o = {k: v.cuda() for k, v in self_operands(case.Nq, case.Nk).items()}
    out = torch.zeros((B, case.Nq, C), dtype=torch.float16, device="cuda")
    if case.wide:
        out = _slice_of_wide(out, 32)
    ldo = out.stride(1)
    assert L.ds_set_option(b"attn_variant", case.variant) == 0
    try:
        rc = L.ds_self_attn_f16(o["q"].data_ptr(), C, case.Nq * C, o["k"].data_ptr(), C, case.Nk * C, o["vt"].data_ptr(),
                                o["vt"].shape[-1], out.data_ptr(), ldo, case.Nq * ldo, B, heads, case.Nq, case.Nk, 0.125,
                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.ds_last_error().decode()
    finally:
        assert L.ds_set_option(b"attn_variant", 0) == 0
    return _digest(out)


def run_flags(case):
    from diffsensei_amd import ops
    return _digest(ops.ip_region_flags(boxes(case.grid, case.B, case.max_ips).cuda(), case.grid[0] * case.grid[1], case.grid))


def run_group(group):
    """{case name: sha256} of one group"""
    run = {IP: run_ip, SELF: run_self, FLAGS: run_flags}
    return {case_name(group, case): run[type(case)](case) for case in GROUPS[group]}


def main():
    digests = {}
    for group in GROUPS:
        digests.update(run_group(group))
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as fh:
        json.dump(digests, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(digests)} cases -> {path}")


if __name__ == "__main__":
    main()
