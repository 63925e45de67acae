"""CPU: nearest x2 + conv3x3 (diffusers Upsample2D, reached from reference src/models/unet.py:304-332) as four 2x2 phase
convolutions - the algebra of the weight fold (`engine.fold_upsample2x_reference`, the torch model of ds_fold_upsample2x_f16) and
the plan-time choice between the folded form (CONV3X3 i[6] == 2) and the nine-tap gather form (i[6] == 1)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F


def phase_conv_model(x, w, fold_dtype=torch.float32):
    """x [B,Cin,H,W], w [Cout,Cin,3,3] -> [B,Cout,2H,2W] through the folded weights: phase (py, px) is a 2x2 convolution of x
    padded by one row / column on the side the phase looks at."""
    from diffsensei_amd.engine import fold_upsample2x_reference
    Cout, Cin = w.shape[:2]
    wp = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()
    wf = fold_upsample2x_reference(wp, fold_dtype).float().reshape(4, Cout, 2, 2, Cin)
    B, _, H, W = x.shape
    out = torch.empty(B, Cout, 2 * H, 2 * W)
    for py in range(2):
        for px in range(2):
            xp = F.pad(x, (1 - px, px, 1 - py, py))      # taps (a, b) read input (Y + py + a - 1, X + px + b - 1)
            out[:, :, py::2, px::2] = F.conv2d(xp, wf[py * 2 + px].permute(0, 3, 1, 2))
    return out


@pytest.mark.parametrize("B,H,W", [(1, 9, 13), (2, 8, 12), (1, 1, 1)])
def test_folded_phases_are_the_upsampled_convolution(B, H, W):
    """fp32 folded weights: the four phase convolutions ARE F.conv2d(F.interpolate(x, 2, "nearest"), w, padding=1), borders and
    odd sizes included - relative L2 <= 1e-6 (fp32 summation order is all that differs)."""
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W)
    x, w = torch.randn(B, 8, H, W, generator=g), torch.randn(6, 8, 3, 3, generator=g)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, padding=1)
    got = phase_conv_model(x, w)
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"{B}x{H}x{W}: folded vs upsample + conv3x3 rel-L2 {rel:.3e}")
    assert rel <= 1e-6, rel


def test_fold_layout_and_single_rounding():
    """[Cout, 9 Cin] -> [4][Cout, 4 Cin], k = (a*2+b) Cin + ci; each entry the fp32 sum of 1, 2 or 4 taps rounded to f16 once."""
    from diffsensei_amd.engine import fold_upsample2x_reference
    g = torch.Generator().manual_seed(3)
    Cout, Cin = 5, 7
    w = torch.randn(Cout, 3, 3, Cin, generator=g).half()
    wf = fold_upsample2x_reference(w.reshape(Cout, 9 * Cin))
    assert wf.shape == (4, Cout, 4 * Cin) and wf.dtype == torch.float16
    wf = wf.reshape(2, 2, Cout, 2, 2, Cin)
    f = w.float()
    assert torch.equal(wf[0, 0, :, 0, 0], w[:, 0, 0])                                                  # one tap: unchanged
    assert torch.equal(wf[1, 1, :, 1, 1], w[:, 2, 2])
    assert torch.equal(wf[0, 1, :, 0, 0], (f[:, 0, 0] + f[:, 0, 1]).half())                            # two taps of one row
    assert torch.equal(wf[0, 0, :, 1, 1], (((f[:, 1, 1] + f[:, 1, 2]) + f[:, 2, 1]) + f[:, 2, 2]).half())  # four, (ky, kx) order
    assert torch.equal(wf[1, 0, :, 0, 1], (f[:, 0, 1] + f[:, 0, 2] + f[:, 1, 1] + f[:, 1, 2]).half())


def _describe(lib, op):
    name, fl, by = C.create_string_buffer(96), C.c_double(), C.c_double()
    assert lib.ds_op_describe(C.byref(op), name, 96, C.byref(fl), C.byref(by)) == 0
    return name.value.decode(), fl.value


def test_plan_folds_exact_x2_upsamplers_only(hip_lib, monkeypatch):
    """An even latent size: both upsamplers of the tiny config are exactly x2 -> CONV3X3 i[6] == 2 on the folded weight, at
    every batch alike; DIFFSENSEI_UPSAMPLE_FOLD=0 brings i[6] == 1 and the 3x3 weight back; an odd size keeps the gather form.
    ds_op_describe counts the algorithmic work of the operation (2 M N 9 Cin) in both forms, under a halo kernel's name."""
    from diffsensei_amd.engine import PackedUNet, UNetEngine
    from diffsensei_amd.unet_config import random_state_dict, tiny_config
    cfg = tiny_config()
    pk = PackedUNet(cfg, random_state_dict(cfg, 0), torch.device("cpu"))
    ups = lambda eng: [op for op in eng.forward_ops if op.code == 2 and op.i[6]]
    on = UNetEngine(pk, 2, 16, 16)
    assert [(op.i[1], op.i[2], op.i[6], op.i[8], op.i[9]) for op in ups(on)] == [(4, 4, 2, 8, 8), (8, 8, 2, 16, 16)]
    names = [n for n in pk.w if n.endswith(".up2fold")]
    assert len(names) == 2
    for op, n in zip(ups(on), sorted(names)):
        wf = pk.w[n]
        assert op.p[1] == wf.data_ptr() and wf.shape == (4, op.i[4], 4 * op.i[3])
    assert [op.i[6] for op in ups(UNetEngine(pk, 8, 16, 16))] == [2, 2]            # not a function of the batch
    with monkeypatch.context() as mp:
        mp.setenv("DIFFSENSEI_UPSAMPLE_FOLD", "0")
        off = UNetEngine(pk, 2, 16, 16)
    assert [op.i[6] for op in ups(off)] == [1, 1]
    assert all(op.p[1] == pk.w[n[:-len(".up2fold")]].data_ptr() for op, n in zip(ups(off), sorted(names)))
    assert len(on.forward_ops) == len(off.forward_ops)
    d_on, d_off = [_describe(hip_lib, op) for op in on.forward_ops], [_describe(hip_lib, op) for op in off.forward_ops]
    assert sum(f for _, f in d_on) == sum(f for _, f in d_off) > 0
    for a, b, op in zip(d_on, d_off, on.forward_ops):
        assert a[1] == b[1]
        if op.code == 2 and op.i[6]:
            assert a[0].startswith("conv_halo") and a[1] == 2.0 * op.i[0] * op.i[8] * op.i[9] * op.i[4] * 9 * op.i[3]
    odd = UNetEngine(pk, 2, 18, 13)            # (18, 13) <- (9, 7) <- (5, 4): 9 x 7 is not 2 x (5 x 4)
    assert [(op.i[1], op.i[2], op.i[6]) for op in ups(odd)] == [(5, 4, 1), (9, 7, 1)]
    mixed = UNetEngine(pk, 2, 18, 16)          # (18, 16) <- (9, 8) <- (5, 4): only the last upsampler is exactly x2
    assert [(op.i[1], op.i[2], op.i[6]) for op in ups(mixed)] == [(5, 4, 1), (9, 8, 2)]


def test_phase_mode_patch_reads_are_conflict_free():
    """Tap (a, b) of phase (py, px) reads the patch at shift (py + a) * 18 + (px + b) with the swizzle rebuilt from px + b: one of
    the nine shifts of the 3x3 form.  The bank model (tools/lds_bank_model.py) for the four reads of every phase, both wave rows,
    every fragment and k-step of the 8x16 and 16x16 kernels: the conflict-free 4 LDS cycles."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "lds_bank_model", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "lds_bank_model.py"))
    bank = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bank)
    col = bank.SWIZZLES["patch column (qx>>1)&7"]
    for rows_per_wave_row, n_mi in ((4, 2), (8, 4)):
        for py in range(2):
            for px in range(2):
                for a in range(2):
                    for b in range(2):
                        tap9 = (py + a) * 3 + (px + b)
                        for wm in range(2):
                            for mi in range(n_mi):
                                for kk in range(4):
                                    assert bank.read_cycles(bank.halo_fragment(rows_per_wave_row, wm, mi, tap9, kk, col)) == 4
