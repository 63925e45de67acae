#!/usr/bin/env python
"""A/B of the attention kernels between two builds of the kernel library (DIFFSENSEI_LIB selects the build of a process).

    AB_TAG=base DIFFSENSEI_LIB=.../libdiffsensei_hip_base.so python tools/attention_kernels_ab.py measure ROUND >> ab.jsonl
    AB_TAG=new                                               python tools/attention_kernels_ab.py measure ROUND >> ab.jsonl
    python tools/attention_kernels_ab.py compare ab.jsonl

measure: one JSON line per kernel and shape, the time of one launch in us as a HIP-event interval over REPS launches (after 3
warm-up launches), plus the SHA-1 of a long-prompt UNet forward (batch 2, 154 text keys).  Shapes: the cross-attention of a
1024 x 1024 UNet batch of 64 (B 64, heads 10 / 20, N 4096 / 1024: tools/one_ipattn.py's and tools/long_prompt_bench.py's) under
ip_attn_variant 0 (T16), 3 (without), 2 (ring) and at 154 / 308 text keys (ip_attn_long_kernel); self-attention at tools/
attn_bench.py's batch-8 and batch-2 shapes under attn_variant 1 / 2 / 3.
compare: per kernel and shape the base build's min .. max over its rounds, the margin (that range widened by its width on
both sides: the project's usual one) and whether every round of the new build lies inside it; forward records written by
tools/forward_lib_ab.py may be given as further files (their tag, batch, forward_ms and sha1 are used)."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(paths):
    rows = []
    for p in paths:
        with open(p) as fh:
            for line in fh:
                if line.strip():
                    rows.append(json.loads(line))
    keys, tags = [], sorted({r["tag"] for r in rows}, key=lambda t: t != "base")
    for r in rows:
        r["key"] = r.get("key") or f"forward batch {r['batch']}"
        r["us"] = r.get("us", r.get("forward_ms", 0.0) * 1e3)
        if r["key"] not in keys:
            keys.append(r["key"])
    ok = True
    for k in keys:
        t = {tag: [r["us"] for r in rows if r["key"] == k and r["tag"] == tag] for tag in tags}
        sha = {tag: sorted({r["sha1"][:12] for r in rows if r["key"] == k and r["tag"] == tag and r.get("sha1")}) for tag in tags}
        base = t[tags[0]]
        lo, hi = min(base), max(base)
        lo, hi = lo - (hi - lo), hi + (hi - lo)
        line = f"{k:58s} " + "  ".join(f"{tag} {min(v):9.1f} .. {max(v):9.1f}" for tag, v in t.items() if v)
        if len(tags) == 2 and t[tags[1]] and any(u for u in base):
            inside = max(t[tags[1]]) <= hi
            ok &= inside
            line += f"  margin <= {hi:9.1f}: {'inside' if inside else 'OUTSIDE'}"
        if any(sha.values()):
            same = len({tuple(v) for v in sha.values() if v}) == 1
            ok &= same
            line += f"  sha1 {'equal' if same else 'DIFFER'} {sha[tags[0]]}"
        print(line)
    print("every kernel inside the base build's margin, every digest equal" if ok else "NOT all inside / equal")
    return 0 if ok else 1


def measure(rnd):
    import torch  # noqa: E402
    from diffsensei_amd import _lib, ops  # noqa: E402

    tag = os.environ.get("AB_TAG", "base" if os.environ.get("DIFFSENSEI_LIB") else "new")
    REPS = int(os.environ.get("REPS", "20"))
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g, device=dev).half()


    def timed(fn):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / REPS * 1e3


    def say(key, us=0.0, **kw):
        print(json.dumps(dict(tag=tag, round=rnd, key=key, us=round(us, 2), **kw)), flush=True)


    for B, heads, hw in ((64, 10, (64, 64)), (64, 20, (32, 32))):
        N, Cc = hw[0] * hw[1], heads * 64
        bbox = torch.zeros(B, 4, 4, device=dev)
        bbox[B // 2:, 0] = torch.tensor([0.05, 0.10, 0.50, 0.95], device=dev)
        bbox[B // 2:, 1] = torch.tensor([0.50, 0.10, 0.95, 0.95], device=dev)
        bbox[B // 2:, 2] = torch.tensor([0.30, 0.30, 0.70, 0.60], device=dev)
        q, ki, vti, out = R(B, N, Cc), R(B, 96, Cc), R(B, Cc, 96), torch.empty(B, N, Cc, dtype=torch.float16, device=dev)
        for Lt in (77, 154, 308):
            T = (Lt + 95) // 96
            kt, vtt = R(B, 96 * T, Cc), R(B, Cc, 96 * T)
            fn = lambda: ops.masked_ip_attention(q, kt, vtt, ki, vti, bbox, heads, hw, 0.6, Lt=Lt, out=out)
            for var, name in ((0, "ip_attn_kernel<4,false,true>"), (3, "ip_attn_kernel<4,false,false>"), (2, "ip_attn_kernel<8,true,false>")) if T == 1 \
                    else ((0, "ip_attn_long_kernel<8>"),):
                lib.ds_set_option(b"ip_attn_variant", var)
                say(f"{name} B {B} heads {heads} N {N} Lt {Lt}", timed(fn))
            lib.ds_set_option(b"ip_attn_variant", 0)
    for B, heads, N in ((8, 20, 1024), (8, 10, 4096), (2, 10, 4096)):
        q, k, vt = R(B, N, heads * 64), R(B, N, heads * 64), R(B, heads, 64, N)
        for var, name in ((1, "self_attn_kernel<1>"), (2, "self_attn_kernel<2>"), (3, "self_attn_sp_kernel")):
            lib.ds_set_option(b"attn_variant", var)
            say(f"{name} B {B} heads {heads} N {N}", timed(lambda: ops.self_attention(q, k, vt, heads)))
        lib.ds_set_option(b"attn_variant", 0)

    # one long-prompt UNet forward (batch 2, two chunks = 154 text keys): the digest of its output
    import bench  # noqa: E402
    pipe, _ = bench.build_pipeline(dev, 1, 0)
    cfg = pipe.unet.config
    B, H, W = 2, 128, 128
    eng = pipe.unet.engine(B, H, W, 1.0, text_tokens=154)
    gc = torch.Generator().manual_seed(1)
    rc = lambda *s: torch.randn(*s, generator=gc).half().to(dev)
    bbox = torch.zeros(B, cfg.max_num_ips, 4, device=dev)
    bbox[B // 2:, 0] = torch.tensor([0.05, 0.10, 0.50, 0.95], device=dev)
    bbox[B // 2:, 1] = torch.tensor([0.50, 0.10, 0.95, 0.95], device=dev)
    tid = torch.tensor([[1024, 1024, 0, 0, 1024, 1024]] * B, dtype=torch.float16, device=dev)
    eng.set_request(rc(B, 154 + cfg.num_ip_tokens, cfg.cross_attention_dim), rc(*eng.text_embeds.shape), tid, bbox, None, 0.6)
    eng.x_in.copy_(rc(*eng.x_in.shape))
    eng.forward_plan.run()
    torch.cuda.synchronize()
    assert torch.isfinite(eng.eps).all()
    sha = hashlib.sha1(eng.eps.cpu().numpy().tobytes()).hexdigest()
    say("UNet forward batch 2, 154 text keys", timed(eng.forward_plan.run), sha1=sha)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2:]))
    if len(sys.argv) >= 2 and sys.argv[1] == "measure":
        sys.exit(measure(int(sys.argv[2]) if len(sys.argv) > 2 else 0))
    sys.exit(__doc__)
