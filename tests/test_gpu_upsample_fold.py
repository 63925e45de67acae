"""GPU: Upsample2D at exactly x2 (nearest x2 + conv3x3; diffusers Upsample2D reached from reference src/models/unet.py:304-332)
as four 2x2 phase convolutions of the input - csrc/conv_halo.hip "Phase mode": the native weight fold, the phase mode of the
three halo-patch kernels against fp32 and against the nine-tap gather form, and the whole SDXL forward with the plan switch
on and off."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests._gates import gate
from tests.test_gpu_ops import _close, _conv_case, _r

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("Cout,Cin", [(64, 64), (200, 128), (640, 640), (1280, 1280)])
def test_native_fold_equals_torch_fold(hip_lib, Cout, Cin):
    """ds_fold_upsample2x_f16 == engine.fold_upsample2x_reference (fp32 sum in (ky, kx) order, one rounding to f16), bit for bit."""
    from diffsensei_amd import ops
    from diffsensei_amd.engine import fold_upsample2x_reference
    g = torch.Generator().manual_seed(Cout + Cin)
    # mixed magnitudes: sums whose fp32 value depends on the order of the additions are in the data
    # (clamped: the inputs and the sums of four stay finite in f16)
    w = (torch.randn((Cout, 3, 3, Cin), generator=g) * torch.exp(3 * torch.randn((Cout, 3, 3, Cin), generator=g))).clamp(-1e3, 1e3).half().to(DEV)
    got = ops.fold_upsample2x(w)
    want = fold_upsample2x_reference(w.reshape(Cout, 9 * Cin))
    assert got.shape == want.shape == (4, Cout, 4 * Cin) and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
    assert torch.equal(got.cpu(), fold_upsample2x_reference(w.reshape(Cout, 9 * Cin).cpu()))


# ragged tiles (H, W not multiples of 8 / 16), 1 .. 20 channel slices, Cout not a multiple of 128 (64: the 64-column tail path
# of conv_halo256_kernel; 192, 320: a ragged last channel tile), and the two upsamplers of the benchmark at batch 2
PHASE_CASES = [(2, 9, 13, 64, 64), (1, 24, 40, 1280, 640), (2, 8, 12, 128, 192), (1, 17, 16, 640, 320), (3, 5, 33, 192, 128),
               (2, 32, 32, 1280, 1280), (2, 64, 64, 640, 640)]


@pytest.mark.parametrize("B,H,W,Cin,Cout", PHASE_CASES)
def test_phase_mode_of_the_three_halo_kernels(hip_lib, B, H, W, Cin, Cout):
    """ds_conv3x3_up2fold_f16 on natively folded weights, each halo kernel forced (conv_halo_variant 1 = 8x16 pixels, 2 = 16x16,
    3 = ring-buffered 8x16) and the automatic dispatch: vs F.conv2d(F.interpolate(x, 2, "nearest")) in fp32 at the project's op
    tolerance (2e-3 of max |ref|), vs the nine-tap kernel on the same input at the same tolerance (each is within ~4e-4 of the
    fp32 result), with per-image bias + residual, and bit-identical between the three kernels as the nine-tap mode is.
    Relative L2 vs fp32: CPU model of the f16-rounded fold 2.5e-4 (nine-tap form 2.1e-4); measured on MI355X 2.49e-4 .. 2.54e-4
    over these cases (nine-tap form: 2.06e-4 .. 2.08e-4) -> gate at 3x the largest, 7.6e-4."""
    from diffsensei_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(B * H + Cin + Cout + 1)
    x, w, b, ref = _conv_case(g, B, H, W, Cin, Cout, True)
    rb = _r((B, Cout), g)
    res = _r(tuple(ref.shape), g)
    ref2 = (ref + rb.float()[:, :, None, None]).half().float() + res.float()
    res_d = res.permute(0, 2, 3, 1).contiguous().to(DEV)
    wf = ops.fold_upsample2x(w)
    nine = ops.conv3x3(x, w, b, upsample=True)
    out = {}
    try:
        for v in (1, 2, 3, 0):
            assert lib.ds_set_option(b"conv_halo_variant", v) == 0
            out[v] = (ops.conv3x3_up2fold(x, wf, b), ops.conv3x3_up2fold(x, wf, b, rowbias=rb.to(DEV), residual=res_d))
    finally:
        lib.ds_set_option(b"conv_halo_variant", 0)
    assert out[1][0].shape == nine.shape == (B, 2 * H, 2 * W, Cout)
    for v, what in ((1, "halo 8x16"), (2, "halo 16x16"), (3, "halo ring-buffered")):
        _close(out[v][0].permute(0, 3, 1, 2), ref, what=f"phase mode, {what}")
        _close(out[v][1].permute(0, 3, 1, 2), ref2, what=f"phase mode, {what} + rowbias + residual")
        _close(out[v][0], nine, what=f"phase mode, {what} vs the nine-tap kernel")
    assert torch.equal(out[1][0], out[2][0]) and torch.equal(out[1][1], out[2][1]), "16x16 and 8x16 halo kernels differ in phase mode"
    assert torch.equal(out[1][0], out[3][0]) and torch.equal(out[1][1], out[3][1]), "ring-buffered and single-buffer 8x16 kernels differ in phase mode"
    assert torch.equal(out[1][0], out[0][0]) and torch.equal(out[1][1], out[0][1]), "automatic dispatch differs in phase mode"
    r_fold, r_nine = _rel(out[0][0].permute(0, 3, 1, 2), ref), _rel(nine.permute(0, 3, 1, 2), ref)
    print(f"{B}x{H}x{W} {Cin}->{Cout}: rel-L2 vs fp32: phase mode {r_fold:.3e}, nine-tap {r_nine:.3e}; "
          f"phase vs nine-tap {_rel(out[0][0], nine):.3e}")
    gate(f"upsample conv {B}x{H}x{W} {Cin}->{Cout}, phase mode vs fp32 conv2d", r_fold, 7.6e-4)


def test_phase_mode_refuses_what_it_does_not_implement(hip_lib):
    """Folded weights serve the exact x2 case of the halo kernels: Cin % 64 != 0 is an error, not another kernel."""
    from diffsensei_amd import _lib, ops
    x = torch.zeros(1, 8, 8, 32, dtype=torch.float16, device=DEV)
    wf = torch.zeros(4, 64, 4 * 32, dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.DiffSenseiHipError):
        ops.conv3x3_up2fold(x, wf, None)


@pytest.fixture(scope="module")
def sdxl_model(hip_lib):
    from diffsensei_amd.unet import UNetMangaModel
    from diffsensei_amd.unet_config import sdxl_config
    cfg = sdxl_config()
    return cfg, UNetMangaModel(cfg, device=DEV).init_random(0)


def test_sdxl_forward_1024_fold_on_vs_off_and_vs_oracle(sdxl_model, monkeypatch):
    """Whole SDXL-size forward at 1024 x 1024, CFG batch 2, plan switch DIFFSENSEI_UPSAMPLE_FOLD on (default) vs off: the two
    plans differ in their two upsampler launches only (i[6] 2 vs 1).  Relative L2 between the outputs: measured 9.93e-4 on MI355X
    (9.92e-4 for the same pair of plans at batch 64, tools/forward_plan_ab.py; either is 1.53e-3 from the fp16-storage oracle)
    -> gate at 3x, 3.0e-3; the default plan vs
    UNetOracle(q = fp16 storage) at the existing 5e-3 (measured 1.53e-3)."""
    from oracle.unet_ref import UNetOracle
    from tests.test_gpu_unet import _inputs, hq
    cfg, m = sdxl_model
    x, enc, te, tid, bbox, db = _inputs(cfg, 2, 128, 128, seed=13)
    m._attn_processors = {"x": type("P", (), {"scale": 0.6})()}
    kw = dict(cross_attention_kwargs={"bbox": bbox, "aspect_ratio": 1.0}, added_cond_kwargs={"text_embeds": te, "time_ids": tid},
              dialog_bbox=db)
    ys, flags = {}, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DIFFSENSEI_UPSAMPLE_FOLD", mode)
        m._engines.clear()
        ys[mode] = m(x.to(DEV), 801.0, enc.to(DEV), **kw).sample.clone()
        eng = next(iter(m._engines.values()))
        flags[mode] = [op.i[6] for op in eng.forward_ops if op.code == 2 and op.i[6]]
    monkeypatch.delenv("DIFFSENSEI_UPSAMPLE_FOLD")
    m._engines.clear()
    assert flags == {"1": [2, 2], "0": [1, 1]}
    assert torch.isfinite(ys["1"]).all() and ys["1"].shape == (2, 4, 128, 128)
    gate("SDXL UNet 1024x1024 batch 2, upsample fold on vs off", _rel(ys["1"], ys["0"]), 3.0e-3)
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        o16 = UNetOracle(cfg, sd, q=hq)
        o16.ip_scale = 0.6
        r16 = o16.forward(x, 801.0, enc, te, tid, bbox, 1.0, db)
    print(f"SDXL 1024x1024 batch 2 vs fp16-storage oracle: fold on {_rel(ys['1'], r16):.3e}, off {_rel(ys['0'], r16):.3e}")
    gate("SDXL UNet 1024x1024 batch 2 (folded upsamplers) vs fp16-storage oracle", _rel(ys["1"], r16), 5e-3)
