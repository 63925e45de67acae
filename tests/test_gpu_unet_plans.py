"""GPU: the launch plans of the benchmarked UNet batches (SDXL-size weights) - which kernels they send where, and that a plan and
its launch cannot disagree silently.

  * every GEMM the plans of 1024 x 1024 at UNet batch 2, 4, 8, 64 and of 2048 x 2048 at batch 2 send to the one-block-per-CU
    kernels (gemm_t160_kernel, gemm_g320_kernel) has its (kernel, M, N, K) in the per-op lists of tests/test_gpu_gemm_t160.py /
    tests/test_gpu_gemm_g320.py, which test each entry against fp64 and the kernel it replaces;
  * the 2048 x 2048 batch-2 plan runs the GEMMs and 3x3 convolutions of the 1024 x 1024 batch-8 plan (whose whole forward
    tests/test_gpu_unet.py checks by default) except for the V^T projections, whose per-image token count differs;
  * a LayerNorm-statistics producer planned for gemm_t160_kernel's 160-column format, or a convolution planned to leave N
    GroupNorm chunks per image, either runs as planned or fails - it never writes another format when an A/B knob on the
    launching thread moves it to another kernel.

The plans are built one at a time and freed; no forward runs here.
"""
import ctypes as C
import gc
from collections import Counter

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def sdxl_packed(hip_lib):
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import sdxl_config
    m = UNetMangaModel(sdxl_config(), device=DEV).init_random(0)
    return m.packed()


def _engine(pk, B, H):
    from diffsensei_amd.engine import UNetEngine
    return UNetEngine(pk, B, H, H, 1.0)


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _describe(lib, op):
    name, fl, by = C.create_string_buffer(96), C.c_double(), C.c_double()
    assert lib.ds_op_describe(C.byref(op), name, 96, C.byref(fl), C.byref(by)) == 0
    return name.value.decode()


def _gemm_conv_seq(lib, eng):
    """(kernel, M, N, K, batch) of every GEMM and CONV3X3 op, in plan order."""
    seq = []
    for op in eng.forward_ops:
        if op.code == 1:
            seq.append((_describe(lib, op), op.i[0], op.i[1], op.i[2], max(op.i[5], 1)))
        elif op.code == 2:
            Ho = op.i[8] or 2 * op.i[1] if op.i[6] else (op.i[1] + 1) // 2 if op.i[5] == 2 else op.i[1]
            Wo = op.i[9] or 2 * op.i[2] if op.i[6] else (op.i[2] + 1) // 2 if op.i[5] == 2 else op.i[2]
            seq.append((_describe(lib, op), op.i[0] * Ho * Wo, op.i[4], 9 * op.i[3], 1))
    return seq


def test_plans_send_the_one_block_per_cu_kernels_only_tested_shapes(sdxl_packed):
    from diffsensei_amd import _lib
    from tests.test_gpu_gemm_g320 import PLAN_SHAPES as G320
    from tests.test_gpu_gemm_t160 import PLAN_SHAPES as T160
    lib = _lib.load()
    tested = {s[:4] for s in T160 + G320}
    seen = set()
    for B, H in [(2, 128), (4, 128), (8, 128), (64, 128), (2, 256)]:
        eng = _engine(sdxl_packed, B, H)
        for op in eng.forward_ops:
            if op.code != 1:
                continue
            nm = _describe(lib, op)
            if nm.startswith(("gemm_t160", "gemm_g320")):
                key = (nm, op.i[0], op.i[1], op.i[2])
                assert key in tested, f"{H * 8} x {H * 8}, UNet batch {B}: {key} has no per-op test"
                seen.add(key)
        del eng
        _free()
    # and the lists hold no stale entry (the ragged-M g320 shape is the one that is no plan's)
    assert tested - seen == {("gemm_g320_kernel<plain>", 13100, 1280, 640)}, tested - seen


def test_2048_batch2_plan_is_the_1024_batch8_plan_but_for_the_vt_projections(sdxl_packed):
    """Why the 2048 x 2048 whole-forward oracle test can stay opt-in: at UNet batch 2 it has the M = B H W of 1024 x 1024 at batch
    8, so every GEMM and convolution of its plan has the shape and the kernel of the batch-8 plan - except the transposed to_v
    projections (one GEMM per image, [C, tokens] = Wv LN(x)^T): 4 096 | 16 384 tokens x 2 images at 2048 x 2048 against
    1 024 | 4 096 x 8 images.  At 2048 x 2048 they run gemm_pp_kernel's operand-swapped consumer (<0,4>, 1280 channels) and the
    128-wide kernels' (640 channels), tested at exactly these shapes in tests/test_gpu_ln_fusion.py
    (test_consumer_swapped_vs_layernorm_linear, test_wide_consumer_swapped_vs_layernorm_linear); the attention ops of 2048 x 2048
    in tests/test_gpu_large_shapes.py."""
    from diffsensei_amd import _lib
    lib = _lib.load()
    eng = _engine(sdxl_packed, 8, 128)
    a = _gemm_conv_seq(lib, eng)
    del eng
    _free()
    eng = _engine(sdxl_packed, 2, 256)
    b = _gemm_conv_seq(lib, eng)
    del eng
    _free()
    assert len(a) == len(b)
    diff = [(k, x, y) for k, (x, y) in enumerate(zip(a, b)) if x[:4] != y[:4]]
    kinds = Counter((x, y) for _, x, y in diff)
    for (x, y), n in sorted(kinds.items()):
        print(f"{n:3d} x  1024^2 batch 8 {x}  |  2048^2 batch 2 {y}")
    assert kinds == {
        (("gemm_glds_kernel<128,false,1>", 1280, 1024, 1280, 8), ("gemm_pp_kernel<0,4>", 1280, 4096, 1280, 2)): 60,
        (("gemm_glds_kernel<128,false,1>", 640, 4096, 640, 8), ("gemm_glds_kernel<128,false,1>", 640, 16384, 640, 2)): 10,
    }, kinds


def _plan_b2_1024(sdxl_packed):
    eng = _engine(sdxl_packed, 2, 128)
    by_ptr = {t.data_ptr(): t for t in eng.keep if isinstance(t, torch.Tensor)}
    return eng, by_ptr


def test_t160_statistics_format_is_never_written_by_another_kernel(sdxl_packed):
    """proj_in of a 1280-channel transformer at UNet batch 2 is planned as a gemm_t160_kernel producer of the 160-column statistics
    format (i[11] = 160: 24 entries per row, its consumers add 24).  Launched with gemm_variant 3 (ping-pong kernel) or gemm_t160 1
    (ring kernel) on the same thread, the op must either fail with a statistics-format message or leave the very same partials -
    a 64-column producer would write 20 entries per row that the consumers then mis-add."""
    from diffsensei_amd import _lib
    lib = _lib.load()
    eng, by_ptr = _plan_b2_1024(sdxl_packed)
    op = next(o for o in eng.forward_ops if o.code == 1 and o.p[9] and not o.p[6] and o.i[11] == 160
              and _describe(lib, o) == "gemm_t160_kernel")
    M, N, K = op.i[0], op.i[1], op.i[2]
    assert (M, N, K) == (2048, 1280, 1280)
    x, y, part = by_ptr[op.p[0]], by_ptr[op.p[3]], by_ptr[op.p[9]]
    nent = 3 * N // 160
    x[:M * K].copy_((torch.randn(M * K, generator=torch.Generator().manual_seed(5)) * 2 + 0.3).half())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    part.zero_()
    assert lib.ds_op_run(C.byref(op), stream) == 0, lib.ds_last_error().decode()
    torch.cuda.synchronize()
    want_y, want_p = y[:M * N].clone(), part[:nent * M * 2].clone()
    assert torch.isfinite(want_p).all() and bool((want_p[-M * 2:] != 0).any())
    outcomes = {}
    for key, val in ((b"gemm_variant", 3), (b"gemm_t160", 1)):
        part.zero_()
        assert lib.ds_set_option(key, val) == 0
        try:
            rc = lib.ds_op_run(C.byref(op), stream)
            torch.cuda.synchronize()
            err = lib.ds_last_error().decode() if rc else ""
        finally:
            lib.ds_set_option(key, 0)
        if rc:
            assert "statistics format" in err, err
            outcomes[key.decode()] = "refused"
        else:
            assert torch.equal(part[:nent * M * 2], want_p), f"{key.decode()} {val}: the planned statistics format was not written"
            assert torch.equal(y[:M * N], want_y)
            outcomes[key.decode()] = "same partials"
    print(f"statistics producer {M}x{N}x{K} under A/B knobs: {outcomes}")
    del eng, by_ptr
    _free()


def test_conv_groupnorm_chunk_count_is_checked_at_launch(sdxl_packed):
    """A conv1 of the batch-2 plan leaves norm2's GroupNorm partials (CONV3X3 i[10] = the chunk count the GROUPNORM op adds up).
    conv_halo_variant 2 (16 x 16-pixel tiles) on the launching thread would write half as many chunks per image: the launch must
    refuse; with the knob back at 0 it runs."""
    from diffsensei_amd import _lib
    lib = _lib.load()
    eng, _ = _plan_b2_1024(sdxl_packed)
    ops = eng.forward_ops
    k = next(j for j, o in enumerate(ops) if o.code == 2 and o.p[6] and o.i[1] == 32 and o.i[3] == 1280)
    op = ops[k]
    gn = next(o for o in ops[k + 1:] if o.code == 3)
    assert op.i[10] == gn.i[6] == int(lib.ds_conv3x3_gn_chunks(op.i[0], op.i[1], op.i[2], op.i[3], op.i[4])) == 8
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ds_set_option(b"conv_halo_variant", 2) == 0
    try:
        rc = lib.ds_op_run(C.byref(op), stream)
        torch.cuda.synchronize()
        err = lib.ds_last_error().decode() if rc else ""
        name2 = _describe(lib, op)
    finally:
        lib.ds_set_option(b"conv_halo_variant", 0)
    assert rc != 0, "a convolution planned for 8 GroupNorm chunks per image ran a kernel that writes 4"
    assert "GroupNorm" in err, err
    assert (_describe(lib, op), name2) == ("conv_halo_deep_kernel", "conv_halo256_kernel")
    assert lib.ds_op_run(C.byref(op), stream) == 0, lib.ds_last_error().decode()
    torch.cuda.synchronize()
    del eng
    _free()
