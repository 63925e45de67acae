"""UNet LoRA adapters, merged into the packed weight buffers in place.

The reference trains its UNet this way (scripts/train/train.py:162-174: `unet.add_adapter(LoraConfig(r=lora_rank,
lora_alpha=lora_rank, target_modules=["to_k", "to_q", "to_v", "to_out.0"]))`, rank 128 in configs/train/diffsensei/*.yaml)
and saves the adapter matrices inside `ckpt.pth["unet_trained"]`, next to the full `to_k_ip` / `to_v_ip` tensors.

Host side only - nothing here computes on the data path:

* `parse_lora_state_dict` turns a peft- or diffusers-format dict into `{module: (A, B, alpha)}` and refuses everything it
  does not merge, naming the keys;
* `LoraState` (one per `UNetMangaModel`) holds the loaded adapters on the device in f16 and, for `set_adapters`, builds or
  reuses a launch plan of `DS_OP_LORA_MERGE` ops (csrc/lora.hip) that rewrites the packed buffers FROM THE BASE WEIGHTS of
  the state dict: W' = W + sum_i weight_i * alpha_i / r_i * B_i A_i.  The buffers keep their addresses, so the UNet launch
  plans, the captured hipGraphs and the activation buffers survive a switch; what packing derives from a merged weight (the
  c / b' vectors of the fused LayerNorms, the 320-row GEGLU copies) is re-derived into its existing storage by the packing
  functions themselves (`PackedUNet.refresh_derived`).

Targets (`all_target_modules`) are the transformer-block linears (`target_modules`, what the reference trains) and, for the
distillation and style adapters that reach further, conv1 / conv2 / conv_shortcut / time_emb_proj of every resnet and the
down / upsampler convolutions.  A 3x3 weight lives in the packed tap-major order while its base and the adapter come in
checkpoint order: the kernel's convolution mode reads the base as it lies and the adapter's down matrix is permuted once
at load time (`pack_conv_down`), so the state dict's tensor stays the only base.  conv_shortcut is a plain matrix,
time_emb_proj a row range of `temb_all.weight`, and an upsampler's folded phase weights are recomputed in place.

The peft key names (`<module>.lora_A[.<adapter>].weight` / `.lora_B...`) are restated from peft's saved format; peft itself
is not a dependency.  The underscore names (`lora_unet_<module with '.' written '_'>.lora_down.weight`) are resolved through
a table built from this UNet's own targets (`underscore_table`).
"""
from __future__ import annotations

import os
import re
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from .unet_config import UNetMangaConfig, build_topology, param_shapes, sdxl_config

Tensor = torch.Tensor
MAX_ACTIVE = 8      # adapters merged at once (one segment each; DS_LORA_MAX_SEGMENTS of csrc/ds_kernels.h is 16)
MAX_RANK = 256

BLOCK_LEAVES = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v",
                "attn2.to_out.0", "ff.net.0.proj", "ff.net.2")
_PREFIXES = ("unet.", "base_model.model.")
_KEY = re.compile(r"^(?P<m>.+?)\.(?:(?P<peft>lora_[AB])(?:\.(?P<ad>[^.]+))?\.weight|lora\.(?P<dif>down|up)\.weight"
                  r"|lora_(?P<und>down|up)\.weight|(?P<alpha>alpha))$")
UNDERSCORE_PREFIX = "lora_unet_"
_SGM = ("input_blocks_", "middle_block_", "output_blocks_", "time_embed_", "label_emb_", "out_")
# adapter families that are not a plain B A product: refused by key, never half-merged
_OTHER_FAMILIES = (("lora_mid", "a Tucker-decomposed convolution adapter (LoCon lora_mid)"), ("hada_", "a LoHa (Hadamard) adapter"),
                   ("lokr_", "a LoKr (Kronecker) adapter"), ("dora_scale", "a DoRA magnitude"),
                   ("lora_magnitude_vector", "a DoRA magnitude"))


def target_modules(cfg: UNetMangaConfig) -> "OrderedDict[str, Tuple[int, int]]":
    """module path -> (N, K) of every nn.Linear inside the transformer blocks: the matrices an adapter may target."""
    shapes = param_shapes(cfg)
    topo = build_topology(cfg)
    out: "OrderedDict[str, Tuple[int, int]]" = OrderedDict()
    attns = [a for blk in topo.down for a in blk["attns"]] + list(topo.mid["attns"]) + [a for blk in topo.up for a in blk["attns"]]
    for a in attns:
        mods = [f"{a.prefix}.proj_in"]
        for k in range(a.depth):
            mods += [f"{a.prefix}.transformer_blocks.{k}.{leaf}" for leaf in BLOCK_LEAVES]
        mods.append(f"{a.prefix}.proj_out")
        for m in mods:
            shp = tuple(shapes[m + ".weight"])
            if len(shp) == 2:
                out[m] = shp
    return out


def all_target_modules(cfg: UNetMangaConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """module path -> shape of the base weight of everything an adapter may target: the transformer-block linears of
    `target_modules` as (N, K), then per resnet conv1 / conv2 (Cout, Cin, 3, 3), conv_shortcut (Cout, Cin, 1, 1) and
    time_emb_proj (Cout, time_embed_dim), and the down / upsampler convolutions (C, C, 3, 3).  conv_in, conv_out, the time and
    add embeddings, every norm, to_k_ip / to_v_ip and the dialog embedding are not targets."""
    shapes = param_shapes(cfg)
    topo = build_topology(cfg)
    out: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict(target_modules(cfg))
    for blk in list(topo.down) + [topo.mid] + list(topo.up):
        for r in blk["resnets"]:
            for leaf in ("conv1", "conv2", "conv_shortcut", "time_emb_proj"):
                if f"{r.prefix}.{leaf}.weight" in shapes:
                    out[f"{r.prefix}.{leaf}"] = tuple(shapes[f"{r.prefix}.{leaf}.weight"])
        for smp in (blk.get("downsample"), blk.get("upsample")):
            if smp:
                out[smp] = tuple(shapes[smp + ".weight"])
    return out


def underscore_table(cfg: UNetMangaConfig) -> Dict[str, str]:
    """{module path with '.' replaced by '_': module path} over `all_target_modules(cfg)`: how a `lora_unet_<name>` key finds
    its module ('_' also occurs inside names - to_q, proj_in - so the name is looked up, never split).  The underscore form
    must be unique."""
    table: Dict[str, str] = {}
    for m in all_target_modules(cfg):
        u = m.replace(".", "_")
        assert u not in table, f"underscore names collide: {table[u]} and {m} both give {u}"
        table[u] = m
    return table


def _strip(key: str) -> str:
    again = True
    while again:
        again = False
        for p in _PREFIXES:
            if key.startswith(p):
                key, again = key[len(p):], True
    return key


def _first(keys: Sequence[str]) -> str:
    keys = list(keys)
    return f"{keys[:3]}" + (f" (+{len(keys) - 3})" if len(keys) > 3 else "")


def drop_text_encoder_keys(sd: Dict[str, Tensor]) -> Tuple[Dict[str, Tensor], int]:
    """(the dict without its `text_encoder*` adapters, how many keys were dropped) - `load_lora_weights(unet_only=True)`."""
    keep = {k: v for k, v in sd.items() if not k.startswith(("text_encoder", "lora_te"))}
    return keep, len(sd) - len(keep)


def parse_lora_state_dict(sd: Dict[str, Tensor], alpha: Optional[float] = None, cfg: Optional[UNetMangaConfig] = None,
                          device=None) -> Dict[str, Tuple[Tensor, Tensor, float]]:
    """{module: (A, B [N,r], alpha)} in f16 (on `device` if given) from

        peft        <module>.lora_A.weight / .lora_B.weight, also with an adapter name (<module>.lora_A.default.weight)
        diffusers   <module>.lora.down.weight / .lora.up.weight
        both        optional prefixes `unet.` / `base_model.model.`, optional scalar <module>.alpha
        underscore  lora_unet_<module with '.' written '_'>.lora_down.weight / .lora_up.weight / .alpha

    `module` is a diffusers UNet path (down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q).  The merged factor is
    alpha / r: the `alpha` argument, else the dict's `<module>.alpha`, else r (the reference's lora_alpha = lora_rank).
    Every module of `all_target_modules(cfg)` (default: SDXL) is a target.  For a linear A is [r, K]; for a convolution A is
    [r, Cin, kh, kw] with the layer's own kernel size and B is [Cout, r, 1, 1] or [Cout, r] (returned 2-D):
    dW[o,i,ky,kx] = sum_r B[o,r] A[r,i,ky,kx].  Any other key is a ValueError that names it - conv_in / conv_out, the time and
    add embeddings, norms, to_k_ip / to_v_ip, processor-era `to_q_lora` names, SGM block names (`lora_unet_input_blocks_...`),
    Tucker / LoHa / LoKr / DoRA tensors and `text_encoder*` adapters included: nothing is ignored silently."""
    cfg = cfg or sdxl_config()
    targets = all_target_modules(cfg)
    under = underscore_table(cfg)
    if not sd:
        raise ValueError("LoRA state dict is empty")
    down: Dict[str, Tensor] = {}
    up: Dict[str, Tensor] = {}
    alphas: Dict[str, float] = {}
    names: Dict[str, str] = {}
    keys: Dict[str, List[str]] = {}
    bad: List[str] = []
    for key, v in sd.items():
        for mark, what in _OTHER_FAMILIES:
            if mark in key:
                raise ValueError(f"LoRA key {key} belongs to {what}; only plain down / up (B A) adapters are merged")
        k = _strip(key)
        if k.startswith(UNDERSCORE_PREFIX):
            rest = k[len(UNDERSCORE_PREFIX):]
            if rest.startswith(_SGM):
                raise ValueError(f"LoRA key {key} uses the SGM (original Stable Diffusion) block naming - input_blocks / "
                                 f"middle_block / output_blocks; convert the adapter to diffusers module names first")
            u, dot, tail = rest.partition(".")
            k = f"{under[u]}.{tail}" if dot and u in under else None
        mt = _KEY.match(k) if k is not None else None
        if mt is None or mt.group("m") not in targets:
            bad.append(key)
            continue
        m = mt.group("m")
        keys.setdefault(m, []).append(key)
        if mt.group("alpha"):
            alphas[m] = float(v)
            continue
        is_down = mt.group("peft") == "lora_A" or "down" in (mt.group("dif"), mt.group("und"))
        slot = down if is_down else up
        ad = mt.group("ad") or ""
        if m in slot or names.setdefault(m, ad) != ad:
            raise ValueError(f"LoRA state dict holds more than one adapter for {m} (key {key}): load them one at a time")
        slot[m] = v
    if bad:
        raise ValueError(f"LoRA keys that are not adapters of a target of this UNet (the transformer-block linears, proj_in, "
                         f"proj_out, and per resnet conv1, conv2, conv_shortcut, time_emb_proj, the down / upsampler "
                         f"convolutions) and are not merged: {_first(bad)}")
    lone = sorted(set(down) ^ set(up)) + sorted(m for m in alphas if m not in down)
    if lone:
        raise ValueError(f"LoRA modules without both a down (lora_A) and an up (lora_B) matrix: {_first(lone)} "
                         f"(keys {_first([k for m in lone for k in keys[m]])})")
    out: Dict[str, Tuple[Tensor, Tensor, float]] = {}
    for m in down:
        A, B = down[m], up[m]
        shp = targets[m]
        N, K = shp[0], shp[1]
        if len(shp) == 4:
            kh, kw = shp[2], shp[3]
            if B.dim() == 4 and tuple(B.shape[2:]) == (1, 1):
                B = B.reshape(B.shape[0], B.shape[1])
            fits = A.dim() == 4 and B.dim() == 2 and tuple(A.shape[1:]) == (K, kh, kw) and B.shape[0] == N and A.shape[0] == B.shape[1]
            want = f"A is [r, {K}, {kh}, {kw}] with the layer's own kernel size, B is [{N}, r, 1, 1] or [{N}, r]"
        else:
            fits = A.dim() == 2 and B.dim() == 2 and A.shape[1] == K and B.shape[0] == N and A.shape[0] == B.shape[1]
            want = f"A is [r, {K}], B is [{N}, r]"
        if not fits:
            raise ValueError(f"LoRA {m}: A {tuple(A.shape)} / B {tuple(up[m].shape)} do not fit the {list(shp)} weight "
                             f"({want}; keys {_first(keys[m])})")
        r = A.shape[0]
        if not 1 <= r <= MAX_RANK:
            raise ValueError(f"LoRA {m}: rank {r} is outside 1..{MAX_RANK}")
        A16, B16 = A.detach().to(torch.float16), B.detach().to(torch.float16)
        if not (bool(torch.isfinite(A16).all()) and bool(torch.isfinite(B16).all())):
            raise ValueError(f"LoRA {m}: non-finite values (in fp16, the inference dtype)")
        a = float(alpha) if alpha is not None else alphas.get(m, float(r))
        if a != a or a in (float("inf"), float("-inf")):
            raise ValueError(f"LoRA {m}: alpha {a} is not finite")
        if device is not None:
            A16, B16 = A16.to(device), B16.to(device)
        out[m] = (A16.contiguous(), B16.contiguous(), a)
    return out


def pack_conv_down(A: Tensor) -> Tensor:
    """A convolution adapter's down matrix [r, Cin, kh, kw] in the packed weights' tap-major order [r, kh*kw*Cin]
    (k = (ky*kw+kx)*Cin + ci, `engine.pack_conv3x3`); a linear's [r, K] as it is."""
    return A if A.dim() == 2 else A.permute(0, 2, 3, 1).reshape(A.shape[0], -1).contiguous()


def split_reference_ckpt(unet_trained: Dict[str, Tensor]) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
    """`ckpt.pth["unet_trained"]` of the reference's LoRA training mode (scripts/train/train.py:163-165, 195-214: every
    parameter with requires_grad, i.e. the adapter matrices AND the full to_k_ip / to_v_ip tensors) -> (plain tensors for
    `load_state_dict(strict=False)`, adapter dict for `load_lora_adapter`).  peft's `base_layer.` infix of a wrapped linear
    is removed from the plain names."""
    plain: Dict[str, Tensor] = {}
    lora: Dict[str, Tensor] = {}
    for k, v in unet_trained.items():
        if ".lora_A." in k or ".lora_B." in k or ".lora." in k:
            lora[k] = v
        else:
            plain[_strip(k).replace(".base_layer.", ".")] = v
    return plain, lora


def read_lora_file(path: Union[str, os.PathLike]) -> Dict[str, Tensor]:
    """`.safetensors`, or a `.bin` / `.pth` / `.pt` pickle read with weights_only=True (as loading.load_weights)."""
    path = os.fspath(path)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    if path.endswith((".bin", ".pth", ".pt")):
        return torch.load(path, map_location="cpu", weights_only=True)
    raise ValueError(f"{path}: a LoRA file is .safetensors, .bin, .pth or .pt")


def _names(names) -> List[str]:
    if names is None:
        return []
    return [names] if isinstance(names, str) else list(names)


class _MergePlan:
    """One launch plan of LORA_MERGE ops for an ordered adapter set, with its device tables."""

    def __init__(self, plan, modules, seg, table, scale, blocks, ops, folds=()):
        self.plan, self.modules, self.seg, self.table = plan, modules, seg, table
        self.folds = list(folds)    # upsamplers whose packed 3x3 weight the plan rewrites (PackedUNet.refresh_derived)
        self.ops = ops              # the DsOp list (roofline accounting: ds_op_describe)
        self.scale = scale          # host fp32 [modules, adapters]: alpha / r where the adapter targets the module, else 0
        self.blocks = blocks        # {transformer block: parts of PackedUNet.ln_fused to re-derive}


class LoraState:
    """The adapters of one `UNetMangaModel`: loaded (`adapters`), active with their weights (`active`), and which modules of
    the packed buffers currently differ from the base (`applied`)."""

    def __init__(self, cfg: UNetMangaConfig):
        self.cfg = cfg
        self.adapters: "OrderedDict[str, Dict[str, Tuple[Tensor, Tensor, float]]]" = OrderedDict()
        self.active: List[Tuple[str, float]] = []
        self.applied: set = set()
        self.plans: Dict[Tuple, _MergePlan] = {}
        self._perm: Dict[int, Tensor] = {}
        self.last_plan: Optional[_MergePlan] = None
        self.targets = all_target_modules(cfg)
        self.order: List[str] = list(self.targets)
        self._stream = None          # side stream the merge plans are captured and replayed on

    # ---- bookkeeping
    def load(self, sd_or_path, name: str, alpha: Optional[float], device) -> None:
        if name in self.adapters:
            raise ValueError(f"adapter {name!r} is already loaded; delete_adapters it first")
        sd = sd_or_path if isinstance(sd_or_path, dict) else read_lora_file(sd_or_path)
        # held kernel-ready: a convolution's down matrix is permuted to the packed order once, here
        self.adapters[name] = {m: (pack_conv_down(A), B, a) for m, (A, B, a) in parse_lora_state_dict(sd, alpha, self.cfg, device).items()}

    def invalidate(self) -> None:
        """The packed buffers (or the base tensors the plans read) are gone: the next `packed()` re-applies `active`."""
        self.plans.clear()
        self.applied = set()
        self._perm = {}
        self.last_plan = None

    def resolve(self, names, weights) -> List[Tuple[str, float]]:
        names = _names(names)
        ws = [float(weights)] * len(names) if not isinstance(weights, (list, tuple)) else [float(w) for w in weights]
        if len(ws) != len(names):
            raise ValueError(f"set_adapters: {len(names)} adapters, {len(ws)} weights")
        if len(set(names)) != len(names):
            raise ValueError(f"set_adapters: an adapter is named twice in {names}")
        unknown = [n for n in names if n not in self.adapters]
        if unknown:
            raise ValueError(f"set_adapters: {unknown} not loaded (loaded: {list(self.adapters)})")
        if len(names) > MAX_ACTIVE:
            raise ValueError(f"set_adapters: at most {MAX_ACTIVE} adapters are merged at once, got {len(names)}")
        if any(w != w or abs(w) == float("inf") for w in ws):
            raise ValueError("set_adapters: weights must be finite")
        return list(zip(names, ws))

    def to(self, device) -> None:
        for ad in self.adapters.values():
            for m, (A, B, a) in list(ad.items()):
                ad[m] = (A.to(device), B.to(device), a)
        self.invalidate()

    # ---- where a module's weight lives in the packed buffers
    def _geglu_map(self, pk, N: int) -> Tensor:
        if N not in self._perm:
            from .engine import pack_geglu
            idx = torch.arange(N, dtype=torch.int32)
            self._perm[N] = pack_geglu(idx[:, None], idx)[1].to(pk.device)
        return self._perm[N]

    def _dest(self, pk, m: str) -> dict:
        """out (a view of the packed buffer the module's rows live in), and where there is one the fused-LayerNorm copy out2
        with its gamma, the GEGLU row map, and (block, part) of what `refresh_derived` re-derives."""
        w = pk.w
        shp = self.targets[m]
        if len(shp) == 4 and shp[2] == 3:           # packed tap-major; an upsampler also has its folded phase weights
            d = dict(out=w[m + ".weight"], conv_cin=shp[1])
            if ".upsamplers." in m:
                d["fold"] = m
            return d
        if m.endswith(".time_emb_proj"):
            off = pk.temb_off[m[:-len(".time_emb_proj")]]
            return dict(out=w["temb_all.weight"][off:off + shp[0]])
        leaf = next((lf for lf in BLOCK_LEAVES if m.endswith("." + lf)), None)
        if leaf is None:                            # proj_in / proj_out, conv_shortcut (packed as a plain [Cout, Cin] matrix)
            return dict(out=w[m + ".weight"])
        t = m[:-len(leaf) - 1]
        has_ln = f"{t}.attn1.qk.weight_ln" in w
        ln = lambda name, norm, part: dict(out2=w[name], colscale=w[f"{t}.{norm}.weight"], block=t, part=part) if has_ln else {}
        if leaf in ("attn1.to_q", "attn1.to_k"):
            C = w[f"{t}.attn1.qk.weight"].shape[0] // 2
            rows = slice(0, C) if leaf == "attn1.to_q" else slice(C, 2 * C)
            d = dict(out=w[f"{t}.attn1.qk.weight"][rows], **ln(f"{t}.attn1.qk.weight_ln", "norm1", "qk"))
            if has_ln:
                d["out2"] = d["out2"][rows]
            return d
        if leaf == "attn1.to_v":
            return dict(out=w[m + ".weight"], **ln(m + ".weight_ln", "norm1", "v"))
        if leaf == "attn2.to_q":
            return dict(out=w[m + ".weight"], **ln(m + ".weight_ln", "norm2", "q2"))
        if leaf in ("attn2.to_k", "attn2.to_v"):
            C = w[f"{t}.attn2.to_q.weight"].shape[0]
            off = pk.kv_off[t]
            return dict(out=w["xattn.k_text" if leaf == "attn2.to_k" else "xattn.v_text"][off:off + C])
        if leaf == "ff.net.0.proj":
            d = dict(out=w[m + ".weight"], map=self._geglu_map(pk, w[m + ".weight"].shape[0]), block=t, part="ff")
            d.update(ln(m + ".weight_ln", "norm3", "ff"))
            return d
        return dict(out=w[m + ".weight"])

    # ---- the merge
    def _build(self, pk, sd: Dict[str, Tensor], names: Tuple[str, ...], modules: Tuple[str, ...]) -> _MergePlan:
        from . import ops
        from .engine import Plan
        n = len(names)
        dev = pk.device
        seg_host = torch.zeros(len(modules), n + 1, dtype=torch.int32)
        scale = torch.zeros(len(modules), max(n, 1), dtype=torch.float32)
        seg = torch.zeros(len(modules), n + 1, dtype=torch.int32, device=dev)
        table = torch.zeros(len(modules), max(n, 1), dtype=torch.float32, device=dev)
        keep: list = [seg, table]
        op_list, blocks, folds = [], {}, []
        for j, m in enumerate(modules):
            As, Bs, off = [], [], 0
            for i, name in enumerate(names):
                hit = self.adapters[name].get(m)
                if hit is not None:
                    As.append(hit[0]), Bs.append(hit[1])
                    off += hit[0].shape[0]
                    scale[j, i] = hit[2] / hit[0].shape[0]
                seg_host[j, i + 1] = off
            d = self._dest(pk, m)
            base = sd[m + ".weight"]
            if base.dim() == 4:                     # checkpoint order; the kernel's convolution mode reads it as it lies
                base = base.reshape(base.shape[0], -1)
            A = B = None
            if As:
                A = As[0] if len(As) == 1 else torch.cat(As, 0).contiguous()
                B = Bs[0] if len(Bs) == 1 else torch.cat(Bs, 1).contiguous()
            op_list.append(ops.lora_merge_op(base, d["out"], A, B, seg[j] if As else None, table[j] if As else None,
                                             d.get("map"), d.get("colscale"), d.get("out2"), nseg=n if As else 0,
                                             conv_cin=d.get("conv_cin", 0)))
            keep += [base, A, B, d["out"], d.get("out2"), d.get("colscale"), d.get("map")]
            if "block" in d:
                blocks.setdefault(d["block"], set()).add(d["part"])
            if "fold" in d:
                folds.append(d["fold"])
        seg.copy_(seg_host)
        return _MergePlan(Plan(op_list, [k for k in keep if k is not None]), modules, seg, table, scale, blocks, op_list, folds)

    def touched(self, names: Sequence[str]) -> set:
        return {m for n in names for m in self.adapters[n]}

    MAX_PLANS = 8       # cached merge plans (each multi-adapter plan owns concatenated A / B copies): least recently used goes

    def dealias(self, pk, sd: Dict[str, Tensor], modules) -> bool:
        """A matrix that is packed as it lies (to_v, to_out.0, ff.net.2, ...) shares its storage with the state dict - and with
        whatever tensor the caller loaded it from.  Before such a matrix can be a merge target the PACKED side gets storage
        of its own, so that a merge never writes into a tensor somebody else holds.  Returns whether any buffer moved (the
        caller then drops the launch plans that name the old address)."""
        moved = False
        for m in modules:
            key = m + ".weight"
            if key in pk.w and key in sd and pk.w[key].untyped_storage().data_ptr() == sd[key].untyped_storage().data_ptr():
                pk.w[key] = pk.w[key].clone()
                moved = True
        return moved

    def apply(self, pk, sd: Dict[str, Tensor], active: List[Tuple[str, float]]) -> None:
        """Rewrite, from the base weights in `sd`, every packed matrix that the adapters merged so far or the new ones touch:
        a matrix that loses its last adapter gets a copy op and returns to the base bits.  `active` is recorded once the
        buffers hold it."""
        names = tuple(n for n, _ in active)
        want = self.touched(names) | self.applied
        modules = tuple(m for m in self.order if m in want)
        if not modules:
            self.active = list(active)
            return
        key = (names, modules)
        mp = self.plans.pop(key, None)
        if mp is None:
            mp = self._build(pk, sd, names, modules)
        self.plans[key] = mp                              # dict order = recency
        while len(self.plans) > self.MAX_PLANS:
            self.plans.pop(next(iter(self.plans)))
        if names:
            mp.table.copy_(mp.scale * torch.tensor([w for _, w in active], dtype=torch.float32)[None, :])
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=pk.device)
        cur = torch.cuda.current_stream(pk.device)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):             # one hipGraph launch instead of one launch per matrix
            if not mp.plan.captured:
                mp.plan.capture(self._stream.cuda_stream)
            mp.plan.replay(self._stream.cuda_stream)
        cur.wait_stream(self._stream)
        pk.refresh_derived(mp.blocks, mp.folds)
        self.applied = self.touched(names)
        self.active = list(active)
        self.last_plan = mp
