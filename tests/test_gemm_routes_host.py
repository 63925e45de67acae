"""CPU: the kernel every GEMM / 3x3 convolution op is routed to (csrc/gemm.hip `route()`), against a table recorded from the
commit BEFORE the dispatch was put behind that one function (tests/golden/gemm_routes.npz).

The library loads without a GPU and `ds_op_describe`, `ds_gemm_ln_fusable`, `ds_gemm_t160_fits`, `ds_gemm_g320_fits` and
`ds_conv3x3_gn_chunks` are host logic, so the whole table is walked here: shapes x roles x A/B knobs.

  (a) the four planner queries answer exactly as recorded, everywhere;
  (b) `ds_op_describe` names the recorded kernel, except where the recorded name was not the kernel the launch of that commit
      ran.  Those rows fall in four classes, and the test states the name it expects for each of them by rule - a Python
      transcription of what ds_launch_gemm did AFTER its `choose()` for the fused-LayerNorm roles:
        1 consumer of partial sums whose automatic choice is not one of the 128-wide kinds: gemm_glds_kernel<BM,false,1>,
          BM = 64 when ceil(M/128) ceil(N/128) < 384, else 128;
        2 producer whose automatic choice cannot emit the statistics: gemm_pp_kernel<0,2> where the ping-pong kernel's
          fused epilogue takes the shape, else gemm_glds_kernel<BM,false,1> as in 1;
        3 consumer of finalised statistics, or producer, that no kernel serves: "refused";
        4 producer asked for the 160-column statistics format off gemm_t160_kernel: "refused".
      A differing row outside the classes fails; so does a class without rows (the grid lost the case).

Re-record (only from a tree whose dispatch is the reference for the change under test):  python tests/test_gemm_routes_host.py --record
"""
import ctypes as C
import itertools
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_routes.npz")

M_AXIS = (1, 32, 64, 100, 256, 272, 1000, 1024, 2048, 4096, 8192, 10240, 10368, 13100, 16384, 32768, 65536, 262144)
N_AXIS = (8, 64, 128, 136, 320, 640, 1280, 2560, 5120, 10240)
K_AXIS = (8, 64, 128, 192, 320, 640, 1280, 1288, 2560, 5120)
BATCHES = (1, 2, 8)
# the non-default knobs walk thinned shape axes (every role still); the default dispatch walks the full product
M_THIN = (64, 272, 2048, 8192, 10240, 10368, 65536)
N_THIN = (64, 136, 320, 640, 1280, 2560, 5120)
K_THIN = (64, 192, 640, 1280, 1288, 5120)
ROLES = ("plain", "residual", "split_a", "geglu", "geglu320", "producer0", "producer64", "producer160", "consumer",
         "consumer_partial", "consumer_swapped", "consumer_swapped_partial")
GEMM_KNOBS = ([()] + [(("gemm_variant", v),) for v in (1, 2, 3, 7, 8, 9, 10, 11)] + [(("gemm_t160", v),) for v in (1, 2, 3)] +
              [(("gemm_g320", 1),), (("gemm_ring", 1),), (("gemm_pp_narrow", 1),), (("gemm_variant", 11), ("gemm_t160", 3))])

CONV_B = (1, 2, 4, 8, 64)
CONV_HW = (8, 16, 32, 33, 64, 128)
CONV_C = ((64, 128), (320, 320), (640, 640), (1280, 1280), (1920, 640))
CONV_FORMS = ("stride1", "stride2", "up", "up_odd", "up_fold")
CONV_KNOBS = ([()] + [(("conv_halo_variant", v),) for v in (1, 2, 3, 4)] + [(("conv_deep_blocks", v),) for v in (0, 2)] +
              [(("gemm_variant", v),) for v in (1, 8, 10)])
PTR = 0x1000   # dummy non-null pointer: host queries dereference nothing


def _lib():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from diffsensei_amd import _lib
    return _lib.load(), _lib.DsOp


class _Knobs:
    """Sets the options of one grid entry on this thread; every key it touched is back at 0 on exit (default of the two knobs
    that are not switches: conv_deep_blocks 1)."""
    DEFAULT = {"conv_deep_blocks": 1}

    def __init__(self, lib, knobs):
        self.lib, self.knobs = lib, knobs

    def __enter__(self):
        for k, v in self.knobs:
            assert self.lib.ds_set_option(k.encode(), v) == 0
        return self

    def __exit__(self, *exc):
        for k, _ in self.knobs:
            self.lib.ds_set_option(k.encode(), self.DEFAULT.get(k, 0))


def gemm_shapes(knobs):
    ms, ns, ks = (M_AXIS, N_AXIS, K_AXIS) if not knobs else (M_THIN, N_THIN, K_THIN)
    return itertools.product(ms, ns, ks, BATCHES)


def fill_gemm(op, role, M, N, K, batch):
    """One DS_OP_GEMM the way engine.py builds it: ldx = ldw = K, ldy = N; dummy pointers."""
    C.memset(C.byref(op), 0, C.sizeof(op))
    op.code = 1
    n = 2 * N if role == "geglu" else N
    n_out = n // 2 if role in ("geglu", "geglu320") else n
    op.i[0], op.i[1], op.i[2], op.i[3], op.i[5], op.i[7] = M, n, K, K, batch, 1
    op.l[0], op.l[2], op.l[3], op.l[4] = K, K, n_out, n_out
    op.p[0], op.p[2], op.p[3] = PTR, PTR, PTR
    if role == "residual":
        op.p[6] = PTR
    elif role == "split_a":
        op.p[1], op.i[3], op.l[0], op.l[1] = PTR, K // 2, K // 2, K - K // 2
    elif role == "geglu":
        op.i[4] = 1
    elif role == "geglu320":
        op.i[4] = 4
    elif role.startswith("producer"):     # out-projection + residual that leaves the row statistics (i[11]: their format)
        op.p[4], op.p[6], op.p[9], op.i[11] = PTR, PTR, PTR, int(role[len("producer"):])
    elif role in ("consumer", "consumer_partial"):
        op.p[4], op.p[7], op.p[8], op.i[9] = PTR, PTR, PTR, int(role.endswith("partial"))
    elif role.startswith("consumer_swapped"):   # V^T: b' rides in ln_c, rows of the normalised matrix in l[10], l[11]
        op.p[7], op.p[8], op.i[8], op.i[9] = PTR, PTR, 1, int(role.endswith("partial"))
        op.l[10], op.l[11] = N, N * batch


def gemm_rows(knobs):
    for M, N, K, batch in gemm_shapes(knobs):
        for role in ROLES:
            if role == "geglu320" and N % 320:
                continue
            yield role, M, N, K, batch


def conv_rows():
    for B, hw, (cin, cout), form, gn in itertools.product(CONV_B, CONV_HW, CONV_C, CONV_FORMS, (0, 1)):
        yield B, hw, cin, cout, form, gn


def fill_conv(op, B, hw, cin, cout, form, gn):
    C.memset(C.byref(op), 0, C.sizeof(op))
    op.code = 2
    op.i[0], op.i[1], op.i[2], op.i[3], op.i[4] = B, hw, hw, cin, cout
    op.i[5] = 2 if form == "stride2" else 1
    op.i[6] = {"up": 1, "up_odd": 1, "up_fold": 2}.get(form, 0)
    if form == "up_odd":
        op.i[8] = op.i[9] = 2 * hw - 1
    op.p[0], op.p[1], op.p[2], op.p[3] = PTR, PTR, PTR, PTR
    if gn:
        op.p[6] = PTR


def walk(lib, DsOp):
    """Everything the table holds, in grid order: kernel names of the GEMM and conv rows, and the planner queries."""
    op, buf = DsOp(), C.create_string_buffer(96)

    def describe():
        assert lib.ds_op_describe(C.byref(op), buf, 96, None, None) == 0
        return buf.value.decode()

    gemm, conv, q_ln, q_t160, q_g320, q_gn = [], [], [], [], [], []
    for knobs in GEMM_KNOBS:
        with _Knobs(lib, knobs):
            for role, M, N, K, batch in gemm_rows(knobs):
                fill_gemm(op, role, M, N, K, batch)
                gemm.append(describe())
            for M, N, K, batch in gemm_shapes(knobs):
                q_ln += [lib.ds_gemm_ln_fusable(M, N, K, 0, batch), lib.ds_gemm_ln_fusable(M, 2 * N, K, 1, batch),
                         lib.ds_gemm_ln_fusable(M, N, K, 4, batch)]
                q_t160.append(lib.ds_gemm_t160_fits(M, N, K, batch))
                q_g320.append(lib.ds_gemm_g320_fits(M, N, K, batch))
    for knobs in CONV_KNOBS:
        with _Knobs(lib, knobs):
            for row in conv_rows():
                fill_conv(op, *row)
                conv.append(describe())
            for B, hw, (cin, cout) in itertools.product(CONV_B, CONV_HW, CONV_C):
                q_gn.append(lib.ds_conv3x3_gn_chunks(B, hw, hw, cin, cout))
    return gemm, conv, q_ln, q_t160, q_g320, q_gn


def record():
    lib, DsOp = _lib()
    gemm, conv, q_ln, q_t160, q_g320, q_gn = walk(lib, DsOp)
    names = sorted(set(gemm) | set(conv))
    assert len(names) < 256
    idx = {n: k for k, n in enumerate(names)}
    np.savez_compressed(GOLDEN, names=np.array(names), gemm=np.array([idx[n] for n in gemm], np.uint8),
                        conv=np.array([idx[n] for n in conv], np.uint8), ln_fusable=np.array(q_ln, np.int8),
                        t160_fits=np.array(q_t160, np.int8), g320_fits=np.array(q_g320, np.int8),
                        gn_chunks=np.array(q_gn, np.int16), version=np.array(lib.ds_version()))
    size = os.path.getsize(GOLDEN)
    assert size <= 256 * 1024, size
    print(f"{GOLDEN}: {len(gemm)} GEMM rows, {len(conv)} conv rows, {len(names)} kernel names, {size} bytes")


# ---- what ds_launch_gemm did with a fused-LayerNorm role after its automatic choice (the rule of classes 1-4)
def _wide(name):
    return name.startswith(("gemm_glds_kernel", "gemm_t160_kernel")) or name == "gemm_g320_kernel<plain>"


def _forced_wide(M, N):
    return f"gemm_glds_kernel<{64 if -(-M // 128) * -(-N // 128) < 384 else 128},false,1>"


def _pp_fused(M, N, K, swapped):
    """gemm_pp_kernel takes the shape (M, N % 16, K % 128) AND its fused epilogues do: whole 256-row tiles (operand-swapped:
    32-row pieces), whole 256-column tiles or - not swapped - whole 64-column strips."""
    return (M % 16 == 0 and N % 16 == 0 and K % 128 == 0 and (M % 32 == 0 if swapped else M % 256 == 0) and
            (N % 256 == 0 or (N % 64 == 0 and not swapped)))


def expected_name(role, M, N, K, batch, recorded):
    """-> (name, class or None)."""
    if role in ("consumer_partial", "consumer_swapped_partial"):
        return (recorded, None) if _wide(recorded) else (_forced_wide(M, N), 1)
    if role in ("consumer", "consumer_swapped"):
        return (recorded, None) if _pp_fused(M, N, K, role == "consumer_swapped") else ("refused", 3)
    if not role.startswith("producer"):
        return recorded, None
    strip = int(role[len("producer"):])
    on_pp = recorded in ("gemm_pp_kernel<0,2>", "gemm_pp_kernel<0,0>")     # the automatic choice for this problem
    pp_ok = _pp_fused(M, N, K, False)
    wide_ok = batch == 1 and N % 128 == 0 and K % 64 == 0
    name, cls = recorded, None
    if (not pp_ok) if on_pp else not (_wide(recorded) and wide_ok):
        if not (pp_ok or wide_ok):
            return "refused", 3
        name = "gemm_pp_kernel<0,2>" if pp_ok else recorded if _wide(recorded) else _forced_wide(M, N)
    elif on_pp:
        name = "gemm_pp_kernel<0,2>"
    if strip == 160 and not name.startswith("gemm_t160_kernel"):
        return "refused", 4
    return name, (2 if name != recorded else None)


# the five divergent launches the change was filed with: (knobs, role, M, N, K, batch) -> name
EXAMPLES = {
    ((), "producer0", 10368, 2560, 1280, 1): "gemm_glds_kernel<128,false,1>",
    ((), "consumer_partial", 10240, 2560, 1280, 1): "gemm_glds_kernel<128,false,1>",
    ((("gemm_variant", 1),), "consumer_partial", 2048, 1280, 1280, 1): "gemm_glds_kernel<64,false,1>",
    ((), "producer0", 2048, 1280, 1288, 1): "refused",
    ((), "consumer", 10368, 2560, 1280, 1): "refused",
}


def test_routes_match_the_recorded_table(hip_lib):
    lib, DsOp = _lib()
    with np.load(GOLDEN) as f:
        rec = {key: f[key] for key in f.files}
    names = [str(n) for n in rec["names"]]
    gemm, conv, q_ln, q_t160, q_g320, q_gn = walk(lib, DsOp)
    # (a) planner queries
    for key, got in (("ln_fusable", q_ln), ("t160_fits", q_t160), ("g320_fits", q_g320), ("gn_chunks", q_gn)):
        want = rec[key]
        assert len(got) == len(want), f"{key}: the grid changed ({len(got)} rows, {len(want)} recorded)"
        bad = np.flatnonzero(np.array(got, np.int64) != want.astype(np.int64))
        assert bad.size == 0, f"{key}: {bad.size} answers differ from the recording, first at row {bad[0]}"
    # (b) kernel names
    assert len(gemm) == len(rec["gemm"]) and len(conv) == len(rec["conv"])
    classes, moved, seen, wrong = Counter(), Counter(), {}, []
    rows = ((knobs, row) for knobs in GEMM_KNOBS for row in gemm_rows(knobs))
    for k, (knobs, (role, M, N, K, batch)) in enumerate(rows):
        recorded = names[rec["gemm"][k]]
        want, cls = expected_name(role, M, N, K, batch, recorded)
        if cls is not None and want != recorded:
            classes[cls] += 1
            moved[(cls, recorded, want)] += 1
        if gemm[k] != want:
            wrong.append((knobs, role, M, N, K, batch, recorded, want, gemm[k]))
        if (knobs, role, M, N, K, batch) in EXAMPLES:
            seen[(knobs, role, M, N, K, batch)] = (recorded, gemm[k])
    for k, row in enumerate((knobs, row) for knobs in CONV_KNOBS for row in conv_rows()):
        if conv[k] != names[rec["conv"][k]]:
            wrong.append(row + (names[rec["conv"][k]], names[rec["conv"][k]], conv[k]))
    print(f"{len(gemm)} GEMM rows, {len(conv)} conv rows; rows whose recorded name was not the launched kernel, per class: "
          f"{dict(sorted(classes.items()))}")
    for (cls, a, b), n in sorted(moved.items()):
        print(f"  class {cls}: {n:6d} x {a} -> {b}")
    assert not wrong, f"{len(wrong)} rows differ from the expected name, e.g. {wrong[:5]}"
    assert all(classes[c] > 0 for c in (1, 2, 3, 4)), f"a class has no rows: {dict(classes)}"
    for key, name in EXAMPLES.items():
        assert key in seen, f"the grid lost {key}"
        assert seen[key][1] == name and seen[key][0] != name, (key, seen[key])


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
    else:
        sys.exit("usage: python tests/test_gemm_routes_host.py --record")
