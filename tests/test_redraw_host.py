"""CPU: the host side of region redraw - the mask rule, the strength arithmetic, the renoise tables against the numpy
restatement of tests/_redraw_ref.py, DPM-Solver++ tables that start mid-schedule, bucketing, and every refusal of the
pipeline (raised before any encoder runs)."""
import types

import numpy as np
import pytest
import torch

from tests import _redraw_ref as R

SDXL = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, timestep_spacing="leading")


# ---------------------------------------------------------------- the mask rule
def test_mask_from_boxes_hand_computed():
    from diffsensei_amd.pipeline import redraw_mask_from_boxes as f
    # right half of a 4 x 4 grid: centres 0.125 0.375 | 0.625 0.875
    assert f([[0.5, 0, 1, 1]], 4, 4).tolist() == [[0, 0, 1, 1]] * 4
    # edges exactly on pixel centres (8 columns: centres k/8 + 1/16, all exact in binary): x1 = 0.4375 is the centre of
    # column 3 and is IN (x1 <= c), x2 = 0.6875 is the centre of column 5 and is OUT (c < x2)
    assert f([[0.4375, 0, 0.6875, 1]], 2, 8).tolist() == [[0, 0, 0, 1, 1, 0, 0, 0]] * 2
    # the same for rows: y1 = 0.25 is the centre of row 0 of 2 (in), y2 = 0.75 the centre of row 1 (out)
    assert f([[0, 0.25, 1, 0.75]], 2, 2).tolist() == [[1, 1], [0, 0]]
    # non-square 8 x 12 (h x w): x in [0.25, 0.5) -> columns 3, 4, 5 (centres 3.5/12 .. 5.5/12); y in [0.5, 1] -> rows 4..7
    want = torch.zeros(8, 12)
    want[4:8, 3:6] = 1
    assert torch.equal(f([[0.25, 0.5, 0.5, 1.0]], 8, 12), want)
    # union of two boxes, and the empty box
    assert torch.equal(f([[0, 0, 0.5, 0.5], [0.5, 0.5, 1, 1]], 4, 4),
                       torch.tensor([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]], dtype=torch.float32))
    assert f([[0.3, 0.3, 0.3, 0.9]], 8, 12).sum() == 0
    for boxes, h, w in (([[0.1, 0.2, 0.77, 0.9]], 8, 12), ([[0.0, 0.0, 1.0, 1.0]], 3, 5), ([[0.5, 0, 1, 1]], 16, 16)):
        assert torch.equal(f(boxes, h, w), R.mask_from_boxes(boxes, h, w))
    with pytest.raises(ValueError):
        f([[0, 0, 1]], 4, 4)


# ---------------------------------------------------------------- strength
def _schedulers(n=10):
    from diffsensei_amd import schedulers as S
    e = S.EulerDiscreteScheduler()
    out = {"euler": e, "ddim": S.DDIMScheduler(), "dpm": S.DPMSolverMultistepScheduler.from_config(e.config),
           "dpm_karras_min": S.DPMSolverMultistepScheduler.from_config(e.config, use_karras_sigmas=True,
                                                                       final_sigmas_type="sigma_min"),
           "euler_a": S.EulerAncestralDiscreteScheduler.from_config(e.config)}
    for s in out.values():
        s.set_timesteps(n)
    return out


def test_start_index_literals():
    for name, s in _schedulers(10).items():
        assert s.start_index(0.6) == 4, name
        assert s.start_index(1.0) == 0, name
        assert s.start_index(0.1) == 9, name
        for bad in (0.05, 0.0, -0.1, 1.01, float("nan"), "0.5", None, True):
            with pytest.raises(ValueError):
                s.start_index(bad)
    s = _schedulers(40)["euler"]
    assert [s.start_index(v) for v in (0.3, 0.5, 0.999, 0.025)] == [28, 20, 1, 39]
    assert all(s.start_index(v) == R.start_index(40, v) for v in np.linspace(0.03, 1.0, 41))
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    with pytest.raises(RuntimeError):
        EulerDiscreteScheduler().start_index(0.5)


def test_renoise_tables_vs_numpy_restatement():
    """fp32 tables against float64 numpy: a handful of fp32 roundings (sigma interpolation, a square root, a product), so
    4 ulp of fp32 = 2.4e-7 relative is the bound."""
    n = 10
    sch = _schedulers(n)
    kinds = {"euler": "sigma", "euler_a": "sigma", "ddim": "ddim", "dpm": "dpm", "dpm_karras_min": "dpm"}
    for name, s in sch.items():
        got = s.renoise_table()
        assert got.dtype == np.float32 and got.shape == (n + 1, 2), name
        assert got[n].tolist() == [1.0, 0.0], name                       # also with final_sigmas_type="sigma_min"
        sig = None if name == "ddim" else np.asarray(s.sigmas, dtype=np.float64)
        if name in ("euler", "euler_a"):                                 # the sigmas themselves, restated
            ac = R.alphas_cumprod()
            train = np.sqrt((1 - ac) / ac)
            ts = (np.arange(0, n) * (1000 // n)).round()[::-1] + 1
            np.testing.assert_allclose(sig[:n], np.interp(ts, np.arange(1000), train), rtol=2.4e-7)
        ref = R.renoise_rows(kinds[name], s.timesteps_np, sig)
        np.testing.assert_allclose(got, ref, rtol=2.4e-7, atol=0, err_msg=name)
    # the kernel's own step coefficients agree: the state a step reads is the state the table describes
    assert np.array_equal(sch["ddim"].renoise_table()[:n], sch["ddim"].coef_table(1.0)[:, 2:4])
    assert np.array_equal(sch["euler"].renoise_table()[:n, 1], sch["euler"].coef_table(1.0)[:, 2])
    assert np.array_equal(sch["dpm"].renoise_table()[:n, ::-1], sch["dpm"].solver_table()[:, 1:3])


@pytest.mark.parametrize("extra", [{}, {"use_karras_sigmas": True}, {"solver_type": "heun"}, {"solver_order": 1}])
def test_dpm_solver_table_mid_schedule(extra):
    from diffsensei_amd.schedulers import DPMSolverMultistepScheduler
    for n in (10, 20):
        s = DPMSolverMultistepScheduler(**dict(SDXL, **extra))
        s.set_timesteps(n)
        full = s.solver_table()
        assert np.array_equal(s.solver_table(start=0), full) and np.array_equal(s.solver_table(0), full)
        for k in (1, 4, n - 2, n - 1):
            part = s.solver_table(start=k)
            assert part.shape == (n - k, 8)
            assert part[0, 0] == 1.0 and part[0, 5] == 0.0 and part[0, 6] == 0.0           # first order: no prev_x0 yet
            assert np.array_equal(part[0, 1:5], full[k, 1:5])                              # the same step otherwise
            assert np.array_equal(part[1:], full[k + 1:])
        for bad in (-1, n):
            with pytest.raises(ValueError):
                s.solver_table(start=bad)


# ---------------------------------------------------------------- serving
def test_bucket_key_plain_requests_unchanged_and_redraw_separate():
    from diffsensei_amd.serving import bucket_key, plan_batches
    assert bucket_key({"height": 1024, "width": 768}) == (1024, 768, 40, 5.0, 1.0)
    assert bucket_key({"height": 512, "width": 512, "num_inference_steps": 25, "guidance_scale": 7.5, "ip_scale": 0.6,
                       "strength": 1.0}) == (512, 512, 25, 7.5, 0.6)
    assert bucket_key({"height": 512, "width": 512, "guidance_scale": [5.0, 6.0], "num_samples": 2}) == \
        (512, 512, 40, (5.0, 6.0), 1.0)
    assert bucket_key({"height": 512, "width": 512, "guidance_scale": 0.5}, mix_scales=True) == (512, 512, 40, False)
    assert bucket_key({}, mix_scales=True) == (None, None, 40, True)
    x0 = torch.zeros(1, 4, 64, 64)
    rd = lambda s=None: dict({"height": 512, "width": 512, "redraw_latents": x0, "redraw_bbox": [[0, 0, 1, 1]]},
                             **({} if s is None else {"strength": s}))
    assert bucket_key(rd()) == (512, 512, 40, 5.0, 1.0, ("redraw", 1.0))
    assert bucket_key(rd(0.5), mix_scales=True) == (512, 512, 40, True, ("redraw", 0.5))
    plain = {"height": 512, "width": 512}
    reqs = [plain, rd(0.5), dict(plain), rd(1.0), rd(0.5), rd(), dict(plain, redraw_latents=None)]
    for mix in (False, True):
        batches = plan_batches(reqs, max_panels=8, mix_scales=mix)
        assert sorted(sorted(b) for b in batches) == [[0, 2, 6], [1, 4], [3, 5]], (mix, batches)


# ---------------------------------------------------------------- refusals, before any encoder runs
@pytest.fixture()
def pipe():
    from diffsensei_amd.pipeline import DiffSenseiPipeline
    from diffsensei_amd.schedulers import EulerDiscreteScheduler
    unet = types.SimpleNamespace(config=types.SimpleNamespace(sample_size=16, in_channels=4, max_num_ips=4),
                                 device=torch.device("cpu"), dtype=torch.float16, attn_processors={})
    p = DiffSenseiPipeline(None, None, None, None, None, EulerDiscreteScheduler(), unet, None)

    def boom(*a, **k):
        raise AssertionError("an encoder ran before the redraw arguments were checked")
    p.encode_prompt = p.prepare_ip_image_embeds = p._denoise = boom
    return p


def test_pipeline_refusals(pipe):
    x0 = torch.zeros(1, 4, 16, 16)
    box = [[0.5, 0, 1, 1]]
    call = lambda **kw: pipe(**dict(dict(prompt="p", height=128, width=128, num_inference_steps=10), **kw))
    cases = [
        dict(redraw_bbox=box),                                                     # region without latents
        dict(redraw_mask=torch.ones(16, 16)),
        dict(redraw_latents=x0),                                                   # latents without a region
        dict(redraw_latents=x0, redraw_bbox=[]),
        dict(strength=0.5),                                                        # strength without a redraw
        dict(redraw_latents=torch.zeros(1, 4, 16, 8), redraw_bbox=box),            # wrong shapes
        dict(redraw_latents=torch.zeros(4, 16, 16), redraw_bbox=box),
        dict(redraw_latents=torch.zeros(3, 4, 16, 16), redraw_bbox=box, num_samples=2),
        dict(redraw_latents=torch.zeros(1, 3, 16, 16), redraw_bbox=box),
        dict(redraw_latents=x0, redraw_mask=torch.ones(12, 16)),
        dict(redraw_latents=x0, redraw_mask=torch.ones(1, 2, 16, 16)),
        dict(redraw_latents=x0, redraw_mask=torch.ones(3, 16, 16), num_samples=2),
        dict(redraw_latents=x0, redraw_mask=torch.ones(16)),
        dict(redraw_latents=x0, redraw_mask=[[1.0] * 16] * 16),
        dict(redraw_latents=x0, redraw_bbox=[[0, 0, 1]]),
        dict(redraw_latents=x0, redraw_mask=torch.full((16, 16), 1.5)),            # mask outside [0, 1]
        dict(redraw_latents=x0, redraw_mask=torch.full((16, 16), -0.1)),
        dict(redraw_latents=x0, redraw_mask=torch.full((16, 16), float("nan"))),
        dict(redraw_latents=x0, redraw_bbox=box, strength=0.0),                    # strength out of range
        dict(redraw_latents=x0, redraw_bbox=box, strength=1.5),
        dict(redraw_latents=x0, redraw_bbox=box, strength=-0.5),
        dict(redraw_latents=x0, redraw_bbox=box, strength="0.5"),
        dict(redraw_latents=x0, redraw_bbox=box, strength=0.05),                   # no step would run (10 steps)
        dict(strength=2.0),
    ]
    for kw in cases:
        with pytest.raises(ValueError):
            call(**kw)
    # the same fields are checked for every request of a batch before the first one is encoded, and a batch is one thing
    ok = dict(prompt="p", height=128, width=128, num_inference_steps=10, redraw_latents=x0, redraw_bbox=box, strength=0.6)
    plain = dict(prompt="p", height=128, width=128, num_inference_steps=10)
    for reqs in ([ok, plain], [plain, ok], [ok, dict(ok, strength=0.3)], [ok, dict(ok, redraw_mask=torch.full((16, 16), 2.0))],
                 [ok, dict(ok, redraw_latents=torch.zeros(1, 4, 8, 8))], [plain, dict(plain, strength=0.5)]):
        with pytest.raises(ValueError):
            pipe.generate_batch(reqs, output_type="latent")
    # what passes the checks reaches the encoders (the stub), also in the mask forms the API lists
    for kw in (dict(redraw_bbox=box), dict(redraw_mask=torch.rand(16, 16)), dict(redraw_mask=torch.rand(2, 16, 16), num_samples=2),
               dict(redraw_mask=torch.rand(2, 1, 128, 128), num_samples=2), dict(redraw_bbox=box, redraw_mask=torch.zeros(128, 128))):
        with pytest.raises(AssertionError, match="encoder ran"):
            call(redraw_latents=x0, strength=0.6, **kw)


def test_redraw_inputs_masks(pipe):
    x0 = torch.randn(1, 4, 16, 16)
    r = pipe._redraw_inputs(x0, [[0.5, 0, 1, 1]], None, 1.0, 3, 128, 128)
    assert r["x0"].shape == (3, 4, 16, 16) and r["x0"].dtype == torch.float16 and torch.equal(r["x0"][2], x0[0].half())
    assert r["mask"].shape == (3, 16, 16) and torch.equal(r["mask"][1], R.mask_from_boxes([[0.5, 0, 1, 1]], 16, 16))
    # pixel resolution: nearest, like torch.nn.functional.interpolate's default; boxes and a mask combine by maximum
    pm = torch.rand(2, 1, 128, 128)
    r = pipe._redraw_inputs(x0, [[0, 0, 0.25, 1]], pm, 0.5, 2, 128, 128)
    want = torch.maximum(pm[:, 0, ::8, ::8], R.mask_from_boxes([[0, 0, 0.25, 1]], 16, 16)[None])
    assert torch.equal(r["mask"], want) and r["strength"] == 0.5
    soft = torch.linspace(0, 1, 256).reshape(16, 16)
    assert torch.equal(pipe._redraw_inputs(x0, None, soft, 1.0, 2, 128, 128)["mask"], soft[None].expand(2, 16, 16))
    assert pipe._redraw_inputs(None, None, None, 1.0, 1, 128, 128) is None
    assert pipe._redraw_inputs(None, [], None, 1.0, 1, 128, 128) is None


def test_redraw_buffer_layout(hip_lib):
    """Offsets follow from ns and HW alone; the fp32 part starts on a 16-byte boundary."""
    from diffsensei_amd import ops
    for ns, H, W in ((3, 8, 12), (1, 1, 1), (2, 3, 5)):
        HW = H * W
        f = (18 * ns * HW + 15) // 16 * 16
        assert hip_lib.ds_redraw_buffer_bytes(ns, HW) == f + 16 + 8 * ops.REDRAW_MAX_ROWS
        buf = torch.zeros(hip_lib.ds_redraw_buffer_bytes(ns, HW), dtype=torch.uint8)
        x0, nz, m, hdr, rows = ops.redraw_views(buf, ns, H, W)
        base = buf.data_ptr()
        assert [t.data_ptr() - base for t in (x0, nz, m, hdr, rows)] == [0, 8 * ns * HW, 16 * ns * HW, f, f + 16]
        assert x0.shape == nz.shape == (ns, 4, H, W) and m.shape == (ns, H, W) and rows.shape == (ops.REDRAW_MAX_ROWS, 2)
        with pytest.raises(Exception):
            ops.redraw_views(buf[:-1], ns, H, W)
