"""GPU: the slot form of the per-row decode kernels of the MLLM pre-pass (csrc/llm.hip: llm_attn_kernel, llm_select_kernel,
llm_rmsnorm_kernel, llm_embed_kernel with state_stride = 8, through the `ops.llm_*_slots` functions) - one row, one KV cache,
one state row, one feature buffer and one id list per sequence slot; a finished slot is left alone.  The comparisons with
the one-sequence `ops.llm_*` functions test the stride handling of one kernel: both forms launch the same `__global__`."""
import math

import pytest
import torch

from tests._gates import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _h(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).half()


def _ref_attention_row(q, k, v, theta=10000.0):
    """fp32: the last of T rows attends to rows 0..T-1 (rotate_half rotary); q [heads,D], k/v [T,heads,D]."""
    from tests._llm_attn_ref import causal_attention_ref
    out, kr = causal_attention_ref(q[None], k, v, k.shape[0] - 1, theta=theta)
    return out[0], kr


@pytest.mark.parametrize("D,heads,kv_heads", [(128, 3, 3), (64, 4, 2)])
def test_attention_slots(hip_lib, D, heads, kv_heads):
    """Three slots at cache lengths 0, 7, 23; the slot at length 7 is finished."""
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(D + heads)
    S, T_max, lens, fin = 3, 40, [0, 7, 23], [0, 1, 0]
    rep, W = heads // kv_heads, (heads + 2 * kv_heads) * D
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(T_max).float(), inv)
    cos, sin = fr.cos().to(DEV).contiguous(), fr.sin().to(DEV).contiguous()
    kc = torch.zeros(S, T_max, kv_heads * D, dtype=torch.float16, device=DEV)
    vc = torch.zeros_like(kc)
    hist = [_h((lens[s] + 1, W), g) for s in range(S)]                         # each slot's own rows, the last one is new
    one = torch.zeros(1, 8, dtype=torch.int32, device=DEV)
    for s in range(S):                                                         # fill the caches through the one-slot kernel
        if lens[s]:
            one.zero_()
            for r0 in range(0, lens[s], 16):
                m = min(16, lens[s] - r0)
                ops.llm_attention(hist[s][r0:r0 + m].to(DEV), kc[s], vc[s], cos, sin, one[0], heads, kv_heads,
                                  1.0 / math.sqrt(D))
                ops.llm_advance(one[0], m)
    kc0, vc0 = kc.clone(), vc.clone()
    state = torch.tensor([[lens[s], 1, fin[s], 0, 9, 2, 0, 0] for s in range(S)], dtype=torch.int32, device=DEV)
    state0 = state.clone()
    qkv = torch.stack([hist[s][-1] for s in range(S)]).to(DEV)
    out = torch.full((S, heads * D), 7.0, dtype=torch.float16, device=DEV)
    ops.llm_attention_slots(qkv, kc, vc, cos, sin, state, heads, kv_heads, 1.0 / math.sqrt(D), out=out)
    assert torch.equal(state, state0), "attention must not move the counters"
    for s in range(S):
        T = lens[s] + 1
        if fin[s]:
            assert torch.equal(kc[s], kc0[s]) and torch.equal(vc[s], vc0[s]), "a finished slot's cache was written"
            assert bool((out[s] == 7.0).all()), "a finished slot's output row was written"
            continue
        h = hist[s]
        q = h[-1, :heads * D].view(heads, D)
        k = h[:, heads * D:(heads + kv_heads) * D].view(T, kv_heads, D).repeat_interleave(rep, 1)
        v = h[:, (heads + kv_heads) * D:].view(T, kv_heads, D).repeat_interleave(rep, 1)
        ref, kr = _ref_attention_row(q, k, v)
        err = (out[s].float().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)
        gate(f"attention slot {s} (length {lens[s]})", err, 4e-3)
        kerr = (kc[s, :T].view(T, kv_heads, D).float().cpu() - kr[:, ::rep]).abs().max().item() / kr.abs().max().item()
        gate(f"rotated key cache slot {s}", kerr, 2e-3)
        assert torch.equal(vc[s, :T].cpu(), h[:, (heads + kv_heads) * D:]), "value cache must be a bit copy"
        assert torch.equal(kc[s, :T - 1], kc0[s, :T - 1]), "rows before the new one were rewritten"
        assert not kc[s, T:].any() and not vc[s, T:].any(), "rows past the slot's length were written"


@pytest.mark.parametrize("D,heads,kv_heads", [(128, 3, 3), (64, 4, 2)])
def test_one_sequence_rows_match_one_row_slot_launches(hip_lib, D, heads, kv_heads):
    """One launch of the one-sequence form with rows = 3 at pos0 = 7 (row m at position pos0 + m, the keys of the same
    launch read un-rotated from qkv) against three one-row launches of the slot form on one slot whose cache length is
    advanced by hand in between (every key read from the cache): outputs and cache rows are bit-equal."""
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(7 * D + heads)
    T_max, pos0, rows = 40, 7, 3
    W, scale = (heads + 2 * kv_heads) * D, 1.0 / math.sqrt(D)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(T_max).float(), inv)
    cos, sin = fr.cos().to(DEV).contiguous(), fr.sin().to(DEV).contiguous()
    hist = _h((pos0 + rows, W), g).to(DEV)
    kc = torch.zeros(1, T_max, kv_heads * D, dtype=torch.float16, device=DEV)
    vc = torch.zeros_like(kc)
    one = torch.zeros(8, dtype=torch.int32, device=DEV)
    ops.llm_attention(hist[:pos0], kc[0], vc[0], cos, sin, one, heads, kv_heads, scale)        # the 7 rows in front
    ops.llm_advance(one, pos0)
    kc_seq, vc_seq, kc_slot, vc_slot = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    out_seq = ops.llm_attention(hist[pos0:], kc_seq[0], vc_seq[0], cos, sin, one, heads, kv_heads, scale)
    assert int(one[0]) == pos0, "attention must not move the counters"
    state = torch.tensor([[pos0, 1, 0, 0, 9, 2, 0, 0]], dtype=torch.int32, device=DEV)
    out_slot = torch.zeros_like(out_seq)
    for m in range(rows):
        ops.llm_attention_slots(hist[pos0 + m:pos0 + m + 1], kc_slot, vc_slot, cos, sin, state, heads, kv_heads, scale,
                                out=out_slot[m:m + 1])
        state[0, 0] += 1
    assert torch.equal(out_seq, out_slot), "row m of one launch differs from the same position decoded alone"
    assert torch.equal(kc_seq, kc_slot) and torch.equal(vc_seq, vc_slot), "the appended cache rows differ"
    assert kc_seq[0, pos0:pos0 + rows].any() and not kc_seq[0, pos0 + rows:].any() and torch.equal(kc_seq[0, :pos0], kc[0, :pos0])


def test_select_slots_match_the_one_slot_kernel(hip_lib):
    """The scenarios of test_llm_select_processor_semantics, three at a time in three slots with different prev, eos and
    max_new: every slot's state row and id list equal what the one-slot kernel leaves."""
    from diffsensei_amd import ops
    V, cap = 3000, 8
    chain = torch.tensor([2900, 2901, 2902, 2903], dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(0)
    base = -torch.rand(V, generator=g) - 0.5
    tie = base.clone(); tie[1234] = 0.0; tie[77] = 0.0
    lg = base.clone(); lg[2000] = 4.0; lg[2902] = 9.0
    # (logits, prev, n_out, max_new, eos, finished)
    cases = [(base, 5, 0, 8, 2, 0), (tie, 5, 0, 8, 2, 0), (lg, 5, 0, 8, 2, 0),
             (lg, 2900, 1, 8, 2, 0), (lg, 2901, 2, 8, 2, 0), (lg, 2902, 3, 8, 2, 0),
             (lg, 2903, 4, 8, 2, 0), (lg, 5, 3, 8, 2000, 0), (lg, 5, 7, 8, 2, 0),
             (lg, 5, 6, 8, 2, 0), (lg, 5, 4, 8, 2, 1), (base, 2900, 2, 3, 2901, 0)]
    for use_chain in (True, False):
        ch = chain if use_chain else None
        for c0 in range(0, len(cases), 3):
            trio = cases[c0:c0 + 3]
            logits = torch.stack([c[0] for c in trio]).half().to(DEV)
            rows = [[10 + s, c[2], c[5], c[1], c[3], c[4], 0, 0] for s, c in enumerate(trio)]
            state = torch.tensor(rows, dtype=torch.int32, device=DEV)
            out_ids = torch.full((3, cap), -1, dtype=torch.int32, device=DEV)
            want_state, want_ids = [], []
            for s in range(3):
                st = torch.tensor(rows[s], dtype=torch.int32, device=DEV)
                ids = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
                ops.llm_select(logits[s].contiguous(), ch, 1, st, ids)
                want_state.append(st)
                want_ids.append(ids)
            ops.llm_select_slots(logits, ch, 1, state, out_ids)
            assert torch.equal(state, torch.stack(want_state)), (use_chain, c0, state.tolist())
            assert torch.equal(out_ids, torch.stack(want_ids)), (use_chain, c0, out_ids.tolist())
    # the semantics themselves, on one trio: image ids zeroed -> lowest wins; ties -> lowest id; finished -> no-op
    logits = torch.stack([base, tie, lg]).half().to(DEV)
    state = torch.tensor([[10, 0, 0, 5, 8, 2, 0, 0], [11, 0, 0, 5, 8, 2, 0, 0], [12, 4, 1, 5, 8, 2, 0, 0]],
                         dtype=torch.int32, device=DEV)
    out_ids = torch.full((3, cap), -1, dtype=torch.int32, device=DEV)
    ops.llm_select_slots(logits, chain, 1, state, out_ids)
    assert state.tolist() == [[11, 1, 0, 2901, 8, 2, 0, 0], [12, 1, 0, 77, 8, 2, 0, 0], [12, 4, 1, 5, 8, 2, 0, 0]]
    assert out_ids[0, 0] == 2901 and out_ids[1, 0] == 77 and bool((out_ids[2] == -1).all())


def test_rmsnorm_slots_feature_tap_and_embed(hip_lib):
    from diffsensei_amd import ops
    g = torch.Generator().manual_seed(3)
    S, H, cap = 3, 512, 4
    x, gam = _h((S, H), g, 3.0), (1 + 0.1 * torch.randn(H, generator=g)).half()
    ref = gam.float() * (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)).half().float()
    feat = torch.zeros(S, cap, H, dtype=torch.float16, device=DEV)
    state = torch.tensor([[0, 3, 0, 4, 9, 2, 0, 0], [5, 1, 0, 17, 9, 2, 0, 0], [2, 2, 1, 600, 9, 2, 0, 0]],
                         dtype=torch.int32, device=DEV)
    y = ops.llm_rmsnorm_slots(x.to(DEV), gam.to(DEV), 1e-6, feat=feat, state=state)
    err = (y.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    gate("rmsnorm slots", err, 2e-3)
    assert torch.equal(y, ops.llm_rmsnorm(x.to(DEV), gam.to(DEV), 1e-6)), "same rows as the one-sequence kernel"
    assert torch.equal(feat[0, 2], y[0]) and not feat[0, [0, 1, 3]].any(), "slot 0: 3 ids out -> feature row 2"
    assert torch.equal(feat[1, 0], y[1]) and not feat[1, 1:].any(), "slot 1: 1 id out -> feature row 0"
    assert not feat[2].any(), "a finished slot writes no feature row"
    assert not ops.llm_rmsnorm_slots(x.to(DEV), gam.to(DEV), 1e-6).isnan().any()       # no tap
    table = _h((640, H), g).to(DEV)
    h = torch.zeros(S, H, dtype=torch.float16, device=DEV)
    ops.llm_embed_slots(table, state, h)
    assert torch.equal(h, table[[4, 17, 600]]), "row s is embed[state[s][3]]"
