"""Host mirror of reference src/pipelines/pipeline_diffsensei.py `DiffSenseiPipeline`.

Same constructor, `register_manga_modules`, `check_inputs`, `prepare_ip_image_embeds`, `prepare_dialog_bbox`,
`set_ip_scale` and `__call__` signature (reference :43-57, :73-79, :81-102, :104-154, :156-170, :172-178, :181-203;
extra TRAILING keyword arguments only).  Returns an object with `.images`.

What runs where
  * denoising loop (UNet + CFG + scheduler step): C++ launch plan over the HIP kernels, one `step_plan` run (or
    hipGraph replay) per step, zero host arithmetic and zero host<->device syncs inside the loop;
  * character encoders (CLIP-H, Magi ViT-MAE) + Resampler: HIP engines (`encoders.py`, `resampler.py`);
  * the two SDXL CLIP text encoders (`encode_prompt`): HIP engine (`encoders.ClipTextEngine`),
    transformers models passed to the constructor are re-laid-out for it; tokenisation stays on the host;
  * the VAE decode + denormalisation (reference :339-367): HIP engine `vae.VaeDecoderEngine`
    (bf16 storage / fp32 math where the reference upcasts the VAE to fp32); a diffusers `AutoencoderKL` passed to the
    constructor is re-laid-out for it, any other object with the `decode` protocol is used as is;
    `output_type` in {"pil", "np", "pt", "latent"}.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple, Union

import torch

from .engine import _is_number
from .encoders import ClipTextEngine, ClipVisionEngine, ViTMAEEngine
from .schedulers import draw_noise_seeds
from .unet import UNetMangaModel, dialog_pixel_boxes
from .vae import VaeDecoderEngine

Tensor = torch.Tensor


@dataclass
class StableDiffusionXLPipelineOutput:
    images: Any


CHUNK_IDS = 75            # prompt ids per chunk: a CLIP window of 77 less BOS and EOS
MAX_PROMPT_CHUNKS = 4     # 4 x 77 = 308 text keys, inside the 384 of the long-prompt cross-attention kernel
MAX_TEXT_TOKENS = 384


def chunk_count(n_ids: int, max_chunks: int) -> Tuple[int, int]:
    """(chunks, dropped ids) of a prompt of `n_ids` ids (without special tokens): k = max(1, ceil(n / 75)) clipped to
    `max_chunks`; what does not fit into the kept chunks is dropped from the tail."""
    k = min(max(1, -(-int(n_ids) // CHUNK_IDS)), int(max_chunks))
    return k, max(0, int(n_ids) - CHUNK_IDS * k)


def chunk_token_ids(ids, bos: int, eos: int, pad: int, max_chunks: int) -> Tensor:
    """Prompt ids WITHOUT special tokens -> int64 [k, 77]: every chunk is [bos] + up to 75 ids + [eos], then `pad` up to 77
    (the tokenizer's own pad id: CLIP-L pads with its EOS, OpenCLIP-bigG with id 0).  k and the dropped tail: `chunk_count`.
    For at most 75 ids the one chunk is what `tok(text, padding="max_length", max_length=77, truncation=True)` gives."""
    ids = [int(v) for v in (ids.reshape(-1).tolist() if torch.is_tensor(ids) else ids)]
    k, _ = chunk_count(len(ids), max_chunks)
    rows = []
    for c in range(k):
        part = ids[c * CHUNK_IDS:(c + 1) * CHUNK_IDS]
        row = [int(bos)] + part + [int(eos)]
        rows.append(row + [int(pad)] * (CHUNK_IDS + 2 - len(row)))
    return torch.tensor(rows, dtype=torch.int64)


def check_max_prompt_chunks(value) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= MAX_PROMPT_CHUNKS:
        raise ValueError(f"`max_prompt_chunks` must be an integer in 1..{MAX_PROMPT_CHUNKS}, got {value!r}")
    return value


def _black_image():
    from PIL import Image
    return Image.new("RGB", (224, 224), (0, 0, 0))


def redraw_mask_from_boxes(boxes, h: int, w: int) -> Tensor:
    """fp32 [h, w], 1 inside the union of the normalised boxes [x1, y1, x2, y2] and 0 outside: latent pixel (y, x) is
    repainted iff x1 <= (x + 0.5) / w < x2 and y1 <= (y + 0.5) / h < y2 - its centre lies in the half-open box (float64)."""
    cx = (torch.arange(w, dtype=torch.float64) + 0.5) / w
    cy = (torch.arange(h, dtype=torch.float64) + 0.5) / h
    m = torch.zeros(h, w, dtype=torch.bool)
    for b in boxes:
        if len(b) != 4:
            raise ValueError(f"`redraw_bbox`: boxes are [x1, y1, x2, y2], got {list(b)}")
        x1, y1, x2, y2 = (float(v) for v in b)
        m |= ((cy >= y1) & (cy < y2))[:, None] & ((cx >= x1) & (cx < x2))[None, :]
    return m.to(torch.float32)


class DiffSenseiPipeline:
    def __init__(self, vae, text_encoder, text_encoder_2, tokenizer, tokenizer_2, scheduler, unet: UNetMangaModel,
                 image_encoder, feature_extractor=None, force_zeros_for_empty_prompt: bool = True):
        self.scheduler, self.unet = scheduler, unet          # first: the engine conversions below read unet.device
        self.vae = self._as_vae_engine(vae)
        self.tokenizer, self.tokenizer_2 = tokenizer, tokenizer_2
        self.text_encoder = self._as_text_engine(text_encoder)
        self.text_encoder_2 = self._as_text_engine(text_encoder_2)
        self.image_encoder = self._as_clip_engine(image_encoder)
        self.feature_extractor = feature_extractor
        self.force_zeros_for_empty_prompt = force_zeros_for_empty_prompt
        self.vae_scale_factor = 8
        self.default_sample_size = unet.config.sample_size
        self.progress_bar_config = {"disable": True}
        self.magi_image_encoder = None
        self.image_proj_model = None
        self._clip_proc = None
        # character references are resized / cropped / normalised by csrc/preprocess.hip (bytes identical to Pillow; e2e
        # character tokens vs the host processors rel-L2 6.9e-4, profiles/r02_device_preprocess_e2e.log).  False, or a
        # reference that is not a PIL image, goes through the transformers processors on the host like the reference.
        # DIFFSENSEI_DEVICE_PREPROCESS=0 restores the reference's host path process-wide.
        self.device_preprocess = os.environ.get("DIFFSENSEI_DEVICE_PREPROCESS", "1") != "0"
        self._device_pre = None
        self._magi_proc = None
        self._guidance_scale = 1.0
        self._interrupt = False
        self._stream = None
        self.use_graph = os.environ.get("DIFFSENSEI_GRAPH", "1") != "0"
        self.last_run_info = {}
        self.last_prompt_info = {}
        self._keep_adapters_until = None     # set inside `hold_adapters()`: the adapter state to restore at its end

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, unet: Optional[UNetMangaModel] = None, image_encoder=None,
                        torch_dtype: Optional[torch.dtype] = torch.float16, device: Optional[Union[str, torch.device]] = None,
                        **components) -> "DiffSenseiPipeline":
        """The reference's construction call (scripts/demo/gradio_wo_mllm.py:189-194, gradio.py:232-237; inherited there
        from diffusers' DiffusionPipeline [3P]): read a diffusers-layout directory - `model_index.json`,
        `scheduler/scheduler_config.json`, `vae/`, `text_encoder/`, `text_encoder_2/`, `tokenizer/`, `tokenizer_2/`
        (safetensors or .bin) - without diffusers, and build the HIP engines.  Components passed as keyword arguments
        (`unet=`, `image_encoder=`, also `vae=`, `scheduler=`, ...) are used as given, exactly like the reference does for
        its UNetMangaModel and CLIP image encoder; a missing `unet=` is loaded from `unet/`."""
        if torch_dtype not in (None, torch.float16):
            raise ValueError("the MI355X engines compute in fp16 (the reference's inference dtype): torch_dtype=torch.float16")
        if not os.path.isdir(os.fspath(pretrained_model_name_or_path)):
            raise FileNotFoundError(f"{pretrained_model_name_or_path}: a local checkpoint directory is required "
                                    f"(there is no hub download in this framework)")
        from .loading import load_pipeline_components
        dev = torch.device(device) if device is not None else (unet.device if unet is not None else torch.device("cuda"))
        names = ("vae", "text_encoder", "text_encoder_2", "tokenizer", "tokenizer_2", "scheduler", "feature_extractor")
        unknown = set(components) - set(names) - {"force_zeros_for_empty_prompt"}
        if unknown:
            raise TypeError(f"from_pretrained: unexpected components {sorted(unknown)}")
        have = {n: components.get(n) for n in names}
        have.update(unet=unet, image_encoder=image_encoder)
        if "force_zeros_for_empty_prompt" in components:
            have["force_zeros_for_empty_prompt"] = components["force_zeros_for_empty_prompt"]
        c = load_pipeline_components(pretrained_model_name_or_path, dev, have)
        return cls(vae=c["vae"], text_encoder=c["text_encoder"], text_encoder_2=c["text_encoder_2"], tokenizer=c["tokenizer"],
                   tokenizer_2=c["tokenizer_2"], scheduler=c["scheduler"], unet=c["unet"], image_encoder=c["image_encoder"],
                   feature_extractor=c.get("feature_extractor"),
                   force_zeros_for_empty_prompt=c["force_zeros_for_empty_prompt"])

    # ---- plumbing
    @property
    def _execution_device(self):
        return self.unet.device

    @property
    def device(self):
        return self.unet.device

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def interrupt(self):
        return self._interrupt

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1

    def to(self, device=None, dtype=None, **kw):
        self.unet.to(device=device, dtype=dtype)
        if self.image_proj_model is not None:
            self.image_proj_model.to(device=device, dtype=dtype)
        return self

    def _as_clip_engine(self, m):
        if m is None or isinstance(m, ClipVisionEngine):
            return m
        return ClipVisionEngine.from_transformers(m, self.unet.device)

    def _as_vae_engine(self, m):
        """A diffusers AutoencoderKL is re-laid-out for the HIP decoder; anything else with `.decode` is used as is."""
        if m is None or isinstance(m, VaeDecoderEngine):
            return m
        if hasattr(m, "state_dict") and hasattr(getattr(m, "config", None), "block_out_channels"):
            return VaeDecoderEngine.from_diffusers(m, self.unet.device)
        return m

    def _as_text_engine(self, m):
        if m is None or isinstance(m, ClipTextEngine):
            return m
        return ClipTextEngine.from_transformers(m, self.unet.device)

    def _as_magi_engine(self, m):
        if m is None or isinstance(m, ViTMAEEngine):
            return m
        return ViTMAEEngine.from_transformers(m, self.unet.device)

    def tensors(self) -> List[Tensor]:
        """Every frozen weight tensor of the pipeline's engines (UNet state dict, text encoders, CLIP-H, Magi, Resampler,
        VAE decoder): the list `distributed.broadcast_pipeline` sends from rank 0 over RCCL.  Components that are not HIP
        engines (a user-supplied VAE object with its own `.decode`) are skipped."""
        out: List[Tensor] = []
        for m in (self.unet, self.text_encoder, self.text_encoder_2, self.image_encoder, self.magi_image_encoder,
                  self.image_proj_model, self.vae):
            if m is not None and hasattr(m, "tensors"):
                out += list(m.tensors())
        return out

    def register_manga_modules(self, magi_image_encoder, image_proj_model):
        """reference :73-79"""
        self.magi_image_encoder = self._as_magi_engine(magi_image_encoder)
        self.image_proj_model = image_proj_model

    # ---- reference :81-102 (same checks, same messages)
    def check_inputs(self, prompt, prompt_2, ip_images, ip_image_embeds, ip_bbox):
        if prompt is None:
            raise ValueError(f"`prompt` has to be of type `str` but is {type(prompt)}")
        elif prompt is not None and not isinstance(prompt, str):
            raise ValueError(f"`prompt` has to be of type `str` but is {type(prompt)}")
        elif prompt_2 is not None and not isinstance(prompt_2, str):
            raise ValueError(f"`prompt_2` has to be of type `str` but is {type(prompt_2)}")
        if len(ip_images) > 0 and ip_image_embeds is not None:
            raise ValueError(f"`ip_images` and `ip_image_embeds` can not be input together!")
        num_ips = len(ip_image_embeds) if ip_image_embeds is not None else len(ip_images)
        if num_ips != len(ip_bbox):
            raise ValueError(f"`ip_images` must have the same length as `ip_bbox`. But they are in length {num_ips} "
                             f"and {len(ip_bbox)}!")

    def _processors(self):
        if self._clip_proc is None:
            from transformers import CLIPImageProcessor, ViTImageProcessor
            self._clip_proc, self._magi_proc = CLIPImageProcessor(), ViTImageProcessor()
        return self._clip_proc, self._magi_proc

    def _encode_refs(self, ip_images, zero_padded: bool):
        """CLIP penultimate states [1,4,257,1280] and Magi CLS embeddings [1,4,768] of the (black-padded) references."""
        max_num_ips = self.unet.config.max_num_ips
        ip_images = list(ip_images)[:max_num_ips]
        num_ips = len(ip_images)
        while len(ip_images) < max_num_ips:
            ip_images.append(_black_image())
        if self.device_preprocess and all(hasattr(im, "convert") and hasattr(im, "size") for im in ip_images):
            # Pillow's resize + crop + normalise on the device (preprocess.py): only the RGB bytes go up
            if self._device_pre is None:
                from .preprocess import DevicePreprocessor
                self._device_pre = DevicePreprocessor(self._execution_device)
            clip_px, magi_px = self._device_pre.clip(ip_images), self._device_pre.vit(ip_images)
        else:
            clip_proc, magi_proc = self._processors()
            clip_px = clip_proc(images=ip_images, return_tensors="pt").pixel_values
            magi_px = magi_proc(images=ip_images, return_tensors="pt").pixel_values
        clip_embeds = self.image_encoder.penultimate_hidden(clip_px).unsqueeze(0)
        magi_embeds = self.magi_image_encoder.cls_embedding(magi_px).unsqueeze(0)
        if zero_padded:
            clip_embeds[0, num_ips:] = 0
            magi_embeds[0, num_ips:] = 0
        return clip_embeds, magi_embeds

    def encode_ip_tokens(self, ip_images) -> Tensor:
        """Resampler tokens [1, num_dummy + max_num_ips*num_vision_tokens, dim] of the references exactly as the MLLM
        pre-pass computes them (reference scripts/demo/gradio.py:85-98: black padding, padded slots NOT zeroed)."""
        clip_embeds, magi_embeds = self._encode_refs(ip_images, zero_padded=False)
        x = self.image_proj_model(clip_embeds, magi_embeds)
        return x.view(1, -1, x.shape[-1])

    # ---- reference :104-154
    def prepare_ip_image_embeds(self, ip_images, ip_image_embeds, ip_bbox, num_samples):
        cfg = self.unet.config
        dev = self._execution_device
        max_num_ips = cfg.max_num_ips
        if ip_image_embeds is not None:
            ip_image_embeds = ip_image_embeds[:max_num_ips]
        ip_bbox = [list(b) for b in ip_bbox][:max_num_ips]
        while len(ip_bbox) < max_num_ips:
            ip_bbox.append([0.0, 0.0, 0.0, 0.0])
        clip_embeds, magi_embeds = self._encode_refs(ip_images, zero_padded=True)   # [1,4,257,1280], [1,4,768]
        image_embeds = self.image_proj_model(clip_embeds, magi_embeds)
        negative_image_embeds = self.image_proj_model(torch.zeros_like(clip_embeds), torch.zeros_like(magi_embeds))
        bbox = torch.tensor(ip_bbox, dtype=torch.float32).unsqueeze(0).to(dev)
        negative_bbox = torch.zeros_like(bbox)
        nv = cfg.num_vision_tokens
        image_embeds = image_embeds.view(1, nv + max_num_ips * nv, image_embeds.shape[-1])
        if ip_image_embeds is not None:
            n_e, _, dim = ip_image_embeds.shape
            image_embeds[0, nv:(1 + n_e) * nv, :] = ip_image_embeds.to(image_embeds).view(1, -1, dim)
        negative_image_embeds = negative_image_embeds.view(1, nv + max_num_ips * nv, image_embeds.shape[-1])
        image_embeds = image_embeds.repeat(num_samples, 1, 1).to(torch.float16)
        negative_image_embeds = negative_image_embeds.repeat(num_samples, 1, 1).to(torch.float16)
        return (negative_image_embeds, image_embeds, negative_bbox.repeat(num_samples, 1, 1),
                bbox.repeat(num_samples, 1, 1))

    # ---- reference :156-170
    def prepare_dialog_bbox(self, dialog_bbox, num_samples):
        max_num_dialogs = self.unet.config.max_num_dialogs
        dialog_bbox = [list(b) for b in dialog_bbox][:max_num_dialogs]
        while len(dialog_bbox) < max_num_dialogs:
            dialog_bbox.append([0.0, 0.0, 0.0, 0.0])
        db = torch.tensor(dialog_bbox, dtype=torch.float32).unsqueeze(0).to(dtype=self.unet.dtype)
        db = db.repeat(num_samples, 1, 1)
        return torch.zeros_like(db), db

    # ---- reference :172-178
    def set_ip_scale(self, scale):
        for attn_processor in self.unet.attn_processors.values():
            if hasattr(attn_processor, "scale"):
                attn_processor.scale = scale

    # ---- text encoding (transformers modules, not on this path; diffusers SDXL `encode_prompt` semantics [3P])
    @staticmethod
    def _raw_ids(tok, text) -> List[int]:
        """The ids of `text` without special tokens and without truncation (host only)."""
        ids = tok(text, add_special_tokens=False, truncation=False).input_ids
        ids = ids.reshape(-1).tolist() if torch.is_tensor(ids) else ids
        if ids and isinstance(ids[0], (list, tuple)):
            ids = ids[0]
        return [int(v) for v in ids]

    def _prompt_texts(self, prompt, prompt_2, do_cfg, negative_prompt, negative_prompt_2):
        """[(tokenizer, text), ...] of everything `encode_prompt` encodes: both prompts and, under CFG unless the empty
        negative is forced to zeros, both negative prompts."""
        toks = [self.tokenizer, self.tokenizer_2]
        texts = list(zip(toks, [prompt, prompt_2 or prompt]))
        if not (do_cfg and negative_prompt is None and self.force_zeros_for_empty_prompt):
            texts += list(zip(toks, [negative_prompt or "", negative_prompt_2 or negative_prompt or ""]))
        return texts

    def prompt_chunk_count(self, request: dict) -> int:
        """How many 77-token chunks the text context of this request (the keyword arguments of `__call__`) will have: from
        the length of `prompt_embeds` if given, else from tokenizing its prompts under `max_prompt_chunks` (host only, no
        encoder runs).  `serving.bucket_key` keys on it: one engine, and one UNet batch, has one text length."""
        pe = request.get("prompt_embeds")
        if pe is not None:
            return -(-int(pe.shape[-2]) // 77)
        mc = check_max_prompt_chunks(request.get("max_prompt_chunks", 1))
        if mc == 1 or self.tokenizer is None:
            return 1
        g = request.get("guidance_scale", 5.0)
        g = g if _is_number(g) else (g.reshape(-1).tolist() if torch.is_tensor(g) else list(g))[0]
        texts = self._prompt_texts(request.get("prompt"), request.get("prompt_2"), float(g) > 1,
                                   request.get("negative_prompt"), request.get("negative_prompt_2"))
        return max(chunk_count(len(self._raw_ids(tok, text)), mc)[0] for tok, text in texts)

    def encode_prompt(self, prompt, prompt_2, device, num_images_per_prompt, do_cfg, negative_prompt, negative_prompt_2,
                      max_prompt_chunks: int = 1):
        """max_prompt_chunks = 1: the reference's path - one 77-token window per encoder, the tail of a longer prompt
        truncated.  2..4: chunked encoding.  The ids of every text (both prompts and, under CFG, both negatives) are cut
        into chunks of 75 (`chunk_token_ids`); k is the largest chunk count among them, shorter ones are padded with empty
        chunks; each encoder encodes its [k, 77] ids in one call; the penultimate hidden states are concatenated on the
        token axis to [1, 77 k, 2048].  The pooled embedding is that of the FIRST chunk of `text_encoder_2`: this project's
        rule (diffusers was not at hand to compare with).  A prompt of at most 75 ids gives the tensors of the one-window
        path.  `self.last_prompt_info` = {"prompt_chunks": k, "prompt_tokens_dropped": n} (n: ids cut from the tails, summed
        over the texts; None when max_prompt_chunks = 1 and the tokenizer cannot tokenize without special tokens)."""
        if self.text_encoder is None or self.tokenizer is None:
            raise ValueError("no text encoders registered: pass prompt_embeds / negative_prompt_embeds / "
                             "pooled_prompt_embeds / negative_pooled_prompt_embeds")
        max_prompt_chunks = check_max_prompt_chunks(max_prompt_chunks)
        if max_prompt_chunks > 1:
            return self._encode_prompt_chunked(prompt, prompt_2, device, num_images_per_prompt, do_cfg, negative_prompt,
                                               negative_prompt_2, max_prompt_chunks)
        try:
            dropped = sum(chunk_count(len(self._raw_ids(tok, text)), 1)[1]
                          for tok, text in self._prompt_texts(prompt, prompt_2, do_cfg, negative_prompt, negative_prompt_2))
        except TypeError:         # a tokenizer without `add_special_tokens`: the count is unknown, the encoding is unaffected
            dropped = None
        self.last_prompt_info = {"prompt_chunks": 1, "prompt_tokens_dropped": dropped}
        prompts = [prompt, prompt_2 or prompt]
        negs = [negative_prompt or "", negative_prompt_2 or negative_prompt or ""]
        toks, encs = [self.tokenizer, self.tokenizer_2], [self.text_encoder, self.text_encoder_2]

        def enc(texts):
            embs, pooled = [], None
            for text, tok, te in zip(texts, toks, encs):
                ids = tok(text, padding="max_length", max_length=tok.model_max_length, truncation=True,
                          return_tensors="pt").input_ids
                hidden, pooled = te.encode(ids)     # HIP text-encoder engine: (hidden_states[-2], out[0])
                embs.append(hidden)
            return torch.cat(embs, dim=-1), pooled

        with torch.no_grad():
            pe, pp = enc(prompts)
            if do_cfg and negative_prompt is None and self.force_zeros_for_empty_prompt:
                ne, npool = torch.zeros_like(pe), torch.zeros_like(pp)
            else:
                ne, npool = enc(negs)
        rep = lambda t: t.repeat_interleave(num_images_per_prompt, dim=0).to(device, torch.float16)
        return rep(pe), rep(ne), rep(pp), rep(npool)

    def _encode_prompt_chunked(self, prompt, prompt_2, device, num_images_per_prompt, do_cfg, negative_prompt,
                               negative_prompt_2, max_chunks):
        texts = self._prompt_texts(prompt, prompt_2, do_cfg, negative_prompt, negative_prompt_2)
        raw = [self._raw_ids(tok, text) for tok, text in texts]
        counts = [chunk_count(len(ids), max_chunks) for ids in raw]
        k = max(c for c, _ in counts)
        self.last_prompt_info = {"prompt_chunks": k, "prompt_tokens_dropped": sum(d for _, d in counts)}
        encs = [self.text_encoder, self.text_encoder_2]

        def enc(pair):            # pair: the entries of `texts` / `raw` of one side, tokenizer 1 then tokenizer 2
            embs, pooled = [], None
            for j, te in zip(pair, encs):
                tok = texts[j][0]
                special = (tok.bos_token_id, tok.eos_token_id, tok.pad_token_id)
                ids = chunk_token_ids(raw[j], *special, max_chunks)
                if ids.shape[0] < k:                      # a shorter text: empty chunks behind it
                    ids = torch.cat([ids, chunk_token_ids([], *special, 1).repeat(k - ids.shape[0], 1)], dim=0)
                hidden, pooled = te.encode(ids)           # [k, 77, D], [k, P]: one call per encoder
                embs.append(hidden.reshape(1, k * hidden.shape[1], hidden.shape[2]))
                pooled = pooled[:1]                       # the first chunk's (the last encoder's is the one returned)
            return torch.cat(embs, dim=-1), pooled

        with torch.no_grad():
            pe, pp = enc((0, 1))
            if len(texts) == 2:                           # CFG with the empty negative forced to zeros
                ne, npool = torch.zeros_like(pe), torch.zeros_like(pp)
            else:
                ne, npool = enc((2, 3))
        rep = lambda t: t.repeat_interleave(num_images_per_prompt, dim=0).to(device, torch.float16)
        return rep(pe), rep(ne), rep(pp), rep(npool)

    def prepare_latents(self, batch_size, num_channels, height, width, dtype, device, generator, latents=None):
        return self._draw_noise(batch_size, num_channels, height, width, dtype, device, generator, latents) \
            * self.scheduler.init_noise_sigma

    def _draw_noise(self, batch_size, num_channels, height, width, dtype, device, generator, latents=None):
        """The unit-variance draw of `prepare_latents` (or the `latents` given in its place), before the scaling."""
        shape = (batch_size, num_channels, int(height) // self.vae_scale_factor, int(width) // self.vae_scale_factor)
        if latents is None:
            gdev = generator.device if generator is not None and not isinstance(generator, list) else torch.device(device)
            latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
        else:
            latents = latents.to(device=device, dtype=dtype)
        return latents

    # ---- region redraw: the request's kept latents and mask, checked on the host before anything runs
    def _redraw_inputs(self, redraw_latents, redraw_bbox, redraw_mask, strength, num_samples, height, width):
        """None for a plain request, else {"x0": fp16 [ns,4,h,w], "mask": fp32 [ns,h,w] (1 = repaint), "strength"}.
        ValueError for a mask or boxes without `redraw_latents` or the reverse, wrong shapes, mask values outside
        [0, 1] and `strength` outside (0, 1]."""
        import numbers
        if isinstance(strength, bool) or not isinstance(strength, numbers.Real) or not 0.0 < float(strength) <= 1.0:
            raise ValueError(f"`strength` has to be in (0, 1], got {strength!r}")
        has_region = redraw_mask is not None or (redraw_bbox is not None and len(redraw_bbox) > 0)
        if redraw_latents is None:
            if has_region:
                raise ValueError("`redraw_bbox` / `redraw_mask` say where to repaint; `redraw_latents` (the latents to keep) is missing")
            if float(strength) != 1.0:
                raise ValueError("`strength` shortens a redraw; without `redraw_latents` the whole schedule runs")
            return None
        if not has_region:
            raise ValueError("`redraw_latents` given without `redraw_bbox` or `redraw_mask`: nothing says where to repaint")
        h, w = int(height) // self.vae_scale_factor, int(width) // self.vae_scale_factor
        x0 = redraw_latents
        if not torch.is_tensor(x0) or x0.dim() != 4 or tuple(x0.shape[1:]) != (4, h, w) or x0.shape[0] not in (1, num_samples):
            raise ValueError(f"`redraw_latents`: [1 or {num_samples}, 4, {h}, {w}] is needed, got "
                             f"{tuple(x0.shape) if torch.is_tensor(x0) else type(x0)}")
        x0 = x0.detach().to("cpu", torch.float16)
        if not torch.isfinite(x0).all():
            raise ValueError("`redraw_latents` holds non-finite values")
        if x0.shape[0] == 1 and num_samples > 1:
            x0 = x0.repeat(num_samples, 1, 1, 1)
        mask = torch.zeros(num_samples, h, w, dtype=torch.float32)
        if redraw_bbox is not None and len(redraw_bbox) > 0:
            mask = torch.maximum(mask, redraw_mask_from_boxes(redraw_bbox, h, w)[None])
        if redraw_mask is not None:
            m = redraw_mask
            if not torch.is_tensor(m) or m.dim() not in (2, 3, 4) or (m.dim() == 4 and m.shape[1] != 1):
                raise ValueError("`redraw_mask`: a tensor [h,w], [ns,h,w] or [ns,1,h,w] is needed")
            m = m.detach().to("cpu", torch.float32)
            m = m.reshape((1, 1) + tuple(m.shape)) if m.dim() == 2 else (m[:, None] if m.dim() == 3 else m)
            if m.shape[0] not in (1, num_samples):
                raise ValueError(f"`redraw_mask`: {m.shape[0]} masks for {num_samples} samples")
            if tuple(m.shape[2:]) == (int(height), int(width)) and (h, w) != (int(height), int(width)):
                m = torch.nn.functional.interpolate(m, size=(h, w))          # nearest, like diffusers' prepare_mask_latents [3P]
            elif tuple(m.shape[2:]) != (h, w):
                raise ValueError(f"`redraw_mask`: {tuple(m.shape[2:])} is neither the latent size {(h, w)} nor the "
                                 f"image size {(int(height), int(width))}")
            if not bool(((m >= 0) & (m <= 1)).all()):
                raise ValueError("`redraw_mask` values have to lie in [0, 1]")
            mask = torch.maximum(mask, m[:, 0].expand(num_samples, h, w))
        return {"x0": x0, "mask": mask.contiguous(), "strength": float(strength)}

    # ---- region redraw from a picture: the VAE encoder in front of the `redraw_latents` path
    @staticmethod
    def _image_tensor(image) -> Tensor:
        """A PIL image or a list of them (converted to RGB), a uint8 array / tensor [H,W,3] or [B,H,W,3], or a float tensor
        [B,3,H,W] in [0, 1] -> what `VaeEncoderEngine.encode` takes, on the host: uint8 [B,H,W,3] or fp32 [B,3,H,W] in
        [-1, 1].  No resize: a side that is not a multiple of 8 is a ValueError."""
        import numpy as np
        if hasattr(image, "convert"):                               # one PIL image
            image = [image]
        if isinstance(image, (list, tuple)):
            if not image or not all(hasattr(im, "convert") for im in image):
                raise ValueError("`redraw_image`: a list holds PIL images")
            arrs = [np.asarray(im.convert("RGB")) for im in image]
            if any(a.shape != arrs[0].shape for a in arrs):
                raise ValueError(f"`redraw_image`: the images differ in size: {[a.shape[:2] for a in arrs]}")
            image = np.stack(arrs)
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image))
        if not torch.is_tensor(image):
            raise ValueError(f"`redraw_image`: a PIL image, a uint8 array or a tensor is needed, got {type(image)}")
        x = image.detach()
        if x.dtype == torch.uint8:
            x = x[None] if x.dim() == 3 else x
            if x.dim() != 4 or x.shape[3] != 3:
                raise ValueError(f"`redraw_image`: uint8 pixels are [H,W,3] or [B,H,W,3], got {tuple(image.shape)}")
            H, W = int(x.shape[1]), int(x.shape[2])
        elif x.is_floating_point():
            if x.dim() != 4 or x.shape[1] != 3:
                raise ValueError(f"`redraw_image`: a float tensor is [B,3,H,W] in [0, 1], got {tuple(image.shape)}")
            x = x.to("cpu", torch.float32)
            if not bool(((x >= 0) & (x <= 1)).all()):
                raise ValueError("`redraw_image`: float pixels have to lie in [0, 1]")
            x = x * 2.0 - 1.0
            H, W = int(x.shape[2]), int(x.shape[3])
        else:
            raise ValueError(f"`redraw_image`: uint8 or float pixels are needed, got {x.dtype}")
        if x.shape[0] == 0 or H == 0 or W == 0 or H % 8 or W % 8:
            raise ValueError(f"`redraw_image`: sides must be multiples of 8 (there is no resize), got {H} x {W}")
        return x.to("cpu").contiguous()

    def _vae_encoder(self):
        enc = getattr(self.vae, "encoder", None)
        if enc is None:
            raise ValueError("`redraw_image` / `encode_image` need a VAE with encoder weights (`encoder.*` and `quant_conv.*` in "
                             "its state dict); this one decodes only - pass `redraw_latents` instead")
        return enc

    def _redraw_image_input(self, redraw_image, redraw_latents, num_samples, height, width) -> Optional[Tensor]:
        """None without `redraw_image`, else the host tensor `_image_tensor` makes of it.  ValueError - before any encoder
        runs - when `redraw_latents` is given too, the VAE has no encoder, or the size is not `height` x `width`."""
        if redraw_image is None:
            return None
        if redraw_latents is not None:
            raise ValueError("`redraw_image` and `redraw_latents` both say what to keep: give one of them")
        self._vae_encoder()
        x = self._image_tensor(redraw_image)
        H, W = (x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[2], x.shape[3])
        if (H, W) != (int(height), int(width)):
            raise ValueError(f"`redraw_image` is {H} x {W} (height x width), the call is {int(height)} x {int(width)}: there is no resize")
        if x.shape[0] not in (1, num_samples):
            raise ValueError(f"`redraw_image`: 1 or {num_samples} images are needed, got {x.shape[0]}")
        return x

    @torch.no_grad()
    def encode_image(self, image, seeds: Optional[Sequence[int]] = None) -> Tensor:
        """Picture -> the fp16 latents [B,4,H/8,W/8] that `redraw_latents` takes (and `output_type="latent"` returns): the
        mode of the VAE posterior, scaled like the pipeline's latents, or with `seeds` (one int64 per image) a sample.
        `image`: see `_image_tensor`."""
        enc = self._vae_encoder()
        return enc.encode_latents(self._image_tensor(image), seeds)

    def decode_latents(self, latents: Tensor, output_type: str = "pil"):
        """Latents (a call with `output_type="latent"`, which are also what `redraw_latents` takes) -> images, exactly
        as `__call__` post-processes its own."""
        return self._postprocess(latents, output_type)

    # ---- reference :180-372
    @torch.no_grad()
    def __call__(self, prompt: str, prompt_2: str = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 40, guidance_scale: float = 5.0,
                 negative_prompt: Optional[Union[str, List[str]]] = None,
                 negative_prompt_2: Optional[Union[str, List[str]]] = None, num_samples: Optional[int] = 1,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                 original_size: Optional[Tuple[int, int]] = None, crops_coords_top_left: Tuple[int, int] = (0, 0),
                 target_size: Optional[Tuple[int, int]] = None, min_size_step: Optional[int] = 8,
                 ip_images=[], ip_image_embeds: Optional[Tensor] = None, ip_bbox: Optional[List[List[float]]] = [],
                 ip_scale: Optional[int] = 1.0, dialog_bbox: Optional[List[List[float]]] = [],
                 # ---- trailing extensions (not in the reference signature)
                 latents: Optional[Tensor] = None, prompt_embeds: Optional[Tensor] = None,
                 negative_prompt_embeds: Optional[Tensor] = None, pooled_prompt_embeds: Optional[Tensor] = None,
                 negative_pooled_prompt_embeds: Optional[Tensor] = None, output_type: str = "pil",
                 callback_on_step_end=None, callback_on_step_end_tensor_inputs: Sequence[str] = ("latents",),
                 noise_seeds: Optional[Sequence[int]] = None, redraw_latents: Optional[Tensor] = None,
                 redraw_bbox: Optional[List[List[float]]] = None, redraw_mask: Optional[Tensor] = None,
                 strength: float = 1.0, redraw_image=None, redraw_image_seeds: Optional[Sequence[int]] = None,
                 max_prompt_chunks: int = 1):
        """`callback_on_step_end(pipe, step_index, timestep, {"latents": device tensor}) -> dict | None` is diffusers'
        SDXL-pipeline hook [3P]; together with `pipe._interrupt = True` it is the reference's early exit: the loop
        `continue`s over the remaining steps (reference :314-315) and the call still decodes and post-processes.  Latents
        may be edited in place or returned (`{"latents": new}`), as in diffusers; `latents` is the only tensor the launch
        plan can hand out per step, so other `callback_on_step_end_tensor_inputs` are refused like diffusers refuses unknown
        names.

        `noise_seeds` (stochastic samplers only: `EulerAncestralDiscreteScheduler`, `LCMScheduler`): `num_samples` non-negative
        int64 seeds, one per panel, that the step kernel draws its noise from; by default they are drawn from `generator`
        after the initial latents (`schedulers.draw_noise_seeds`).  The seeds used are in `last_run_info["noise_seeds"]`.

        `guidance_scale` and `ip_scale` are a number, as in the reference, or a sequence of `num_samples` numbers, one per
        sample (a slider sweep in one pass: the kernels take both per panel).  Classifier-free guidance is on or off
        for the whole batch, so a sequence is all > 1 or all <= 1.  `last_run_info["guidance_scales"]` /
        `["ip_scales"]` list what every panel used.

        Region redraw: `redraw_latents` [1 or num_samples, 4, H/8, W/8] - the latents of an earlier
        call with `output_type="latent"`; one row gives `num_samples` variants - are kept outside the region and
        repainted inside it.  The region is the union of the normalised `redraw_bbox` boxes (a latent pixel is in when
        its centre is) and / or `redraw_mask` ([h,w], [ns,h,w] or [ns,1,h,w] in [0, 1], latent or image resolution, soft
        values allowed), combined by maximum.  `strength` in (0, 1] runs the last int(steps * strength) steps from the
        kept latents noised to that level; 1.0 starts from pure noise.  The noise is the draw of a plain call (or
        `latents=`); the callback gets the run-relative step index and the true timestep;
        `last_run_info["redraw"]` = {"t_start", "steps_run", "repaint_fraction"}.  `redraw_image` (a PIL image or a list, a
        uint8 array / tensor [H,W,3] or [B,H,W,3], a float tensor [B,3,H,W] in [0, 1]; exactly `height` x `width`, no resize)
        takes the place of `redraw_latents`: it goes through the VAE encoder (`encode_image`: the posterior's mode, or a
        sample when `redraw_image_seeds` gives one int64 per image) and then follows the same path.

        Long prompts: `max_prompt_chunks` (1..4; anything else is a ValueError before any encoder runs).  1, the default, is
        the reference's behaviour: the prompt is truncated to one 77-token CLIP window.  With 2..4 a prompt of more than 75
        ids is encoded in chunks of 75 (`encode_prompt`) and the UNet attends all 77 k text tokens
        (`last_run_info["prompt_chunks"]` = k, `["prompt_tokens_dropped"]` = ids cut behind the last chunk, 0 if none).
        `prompt_embeds` / `negative_prompt_embeds` may have any equal length in 1..384; a shorter negative is an error."""
        check_max_prompt_chunks(max_prompt_chunks)
        bad = [k for k in callback_on_step_end_tensor_inputs if k != "latents"]
        if bad:
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in ['latents'], but found {bad}")
        self._interrupt = False                                   # reference :226
        cond = self._conditioning(prompt, prompt_2, height, width, num_inference_steps, guidance_scale, negative_prompt,
                                  negative_prompt_2, num_samples, generator, original_size, crops_coords_top_left,
                                  target_size, ip_images, ip_image_embeds, ip_bbox, ip_scale, dialog_bbox, latents,
                                  prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds,
                                  negative_pooled_prompt_embeds, noise_seeds, redraw_latents, redraw_bbox, redraw_mask,
                                  strength, redraw_image, redraw_image_seeds, max_prompt_chunks)
        out_latents = self._denoise([cond], num_inference_steps, callback_on_step_end)
        return StableDiffusionXLPipelineOutput(images=self._postprocess(out_latents, output_type))

    # ---- one request's conditioning tensors (reference :205-309), `num_samples` rows each, conditional and negative
    def _conditioning(self, prompt, prompt_2, height, width, num_inference_steps, guidance_scale, negative_prompt,
                      negative_prompt_2, num_samples, generator, original_size, crops_coords_top_left, target_size,
                      ip_images, ip_image_embeds, ip_bbox, ip_scale, dialog_bbox, latents, prompt_embeds,
                      negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, noise_seeds=None,
                      redraw_latents=None, redraw_bbox=None, redraw_mask=None, strength=1.0, redraw_image=None,
                      redraw_image_seeds=None, max_prompt_chunks=1):
        check_max_prompt_chunks(max_prompt_chunks)
        self._check_prompt_embeds(prompt_embeds, negative_prompt_embeds)
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        original_size = original_size or (height, width)
        target_size = target_size or (height, width)
        self.check_inputs(prompt, prompt_2, ip_images, ip_image_embeds, ip_bbox)
        if height % self.vae_scale_factor or width % self.vae_scale_factor:
            raise ValueError(f"`height` and `width` have to be divisible by {self.vae_scale_factor} but are {height} and {width}.")
        num_samples = 1 if num_samples is None else num_samples
        # a picture to keep: its own checks first, then every other redraw field against latents of the right shape - all
        # before any encoder runs, the VAE's included
        image = self._redraw_image_input(redraw_image, redraw_latents, num_samples, height, width)
        if image is not None:
            redraw_latents = torch.zeros(1, 4, height // self.vae_scale_factor, width // self.vae_scale_factor)
        elif redraw_image_seeds is not None:
            raise ValueError("`redraw_image_seeds` seed the encoding of `redraw_image`, which is missing")
        redraw = self._redraw_inputs(redraw_latents, redraw_bbox, redraw_mask, strength, num_samples, height, width)
        if redraw is not None:                                   # "no step would run" is a ValueError before any encoder too
            self.scheduler.set_timesteps(num_inference_steps, device=self._execution_device)
            self.scheduler.start_index(redraw["strength"])
        if image is not None:                                    # from here on it is the `redraw_latents` path, unchanged
            redraw = self._redraw_inputs(self._vae_encoder().encode_latents(image, redraw_image_seeds), redraw_bbox,
                                         redraw_mask, strength, num_samples, height, width)
        guidance = self._panel_values(guidance_scale, num_samples, "guidance_scale")
        ip_scales = self._panel_values(ip_scale, num_samples, "ip_scale")
        self._cfg_side(guidance)
        self._guidance_scale = guidance_scale if _is_number(guidance_scale) else guidance[0]
        device = self._execution_device
        self.set_ip_scale(ip_scale if _is_number(ip_scale) else ip_scales[-1])
        do_cfg = self.do_classifier_free_guidance

        if prompt_embeds is None:
            prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds = \
                self.encode_prompt(prompt, prompt_2, device, num_samples, do_cfg, negative_prompt, negative_prompt_2,
                                   max_prompt_chunks)
            prompt_info = dict(self.last_prompt_info)
        else:
            prompt_info = {"prompt_chunks": -(-int(prompt_embeds.shape[-2]) // 77), "prompt_tokens_dropped": 0}
            f = lambda t: None if t is None else t.to(device, torch.float16)
            prompt_embeds, pooled_prompt_embeds = f(prompt_embeds), f(pooled_prompt_embeds)
            negative_prompt_embeds = f(negative_prompt_embeds) if negative_prompt_embeds is not None \
                else torch.zeros_like(prompt_embeds)
            negative_pooled_prompt_embeds = f(negative_pooled_prompt_embeds) if negative_pooled_prompt_embeds is not None \
                else torch.zeros_like(pooled_prompt_embeds)
            if prompt_embeds.shape[0] == 1 and num_samples > 1:
                prompt_embeds = prompt_embeds.repeat(num_samples, 1, 1)
                negative_prompt_embeds = negative_prompt_embeds.repeat(num_samples, 1, 1)
                pooled_prompt_embeds = pooled_prompt_embeds.repeat(num_samples, 1)
                negative_pooled_prompt_embeds = negative_pooled_prompt_embeds.repeat(num_samples, 1)

        self.scheduler.set_timesteps(num_inference_steps, device=device)
        # a redraw keeps the draw unscaled: the start kernel makes the start state from it (the same fp16 product at strength 1)
        lat = (self.prepare_latents if redraw is None else self._draw_noise)(
            num_samples, self.unet.config.in_channels, height, width, torch.float16, device, generator, latents)
        # a stochastic sampler's per-panel Philox seeds, drawn AFTER the initial latents: a deterministic scheduler
        # consumes the generator exactly as before, and a given generator starts Euler Ancestral from Euler's latents
        seeds = None
        if self.scheduler.stochastic:
            seeds = [int(v) for v in noise_seeds] if noise_seeds is not None else draw_noise_seeds(num_samples, generator)
            if len(seeds) != num_samples or any(v < 0 or v >= 2 ** 63 for v in seeds):
                raise ValueError(f"`noise_seeds`: {num_samples} integers in [0, 2**63) are needed, got {seeds}")
        elif noise_seeds is not None:
            raise ValueError(f"`noise_seeds` given, but {type(self.scheduler).__name__} draws no noise")
        neg_img, img, neg_bbox, bbox = self.prepare_ip_image_embeds(ip_images, ip_image_embeds, list(ip_bbox), num_samples)
        add_time_ids = torch.tensor([list(original_size) + list(crops_coords_top_left) + list(target_size)],
                                    dtype=torch.float16, device=device).repeat(num_samples, 1)
        neg_dialog, dialog = self.prepare_dialog_bbox(list(dialog_bbox), num_samples)
        to = lambda t: t.to(device)
        return {"n": num_samples, "lat": lat, "time_ids": add_time_ids, "noise_seeds": seeds,
                "guidance": guidance, "ip_scales": ip_scales, "redraw": redraw, "prompt_info": prompt_info,
                "pos": (to(prompt_embeds), to(pooled_prompt_embeds), to(img), to(bbox), to(dialog)),
                "neg": (to(negative_prompt_embeds), to(negative_pooled_prompt_embeds), to(neg_img), to(neg_bbox),
                        to(neg_dialog))}

    @staticmethod
    def _check_prompt_embeds(prompt_embeds, negative_prompt_embeds, what: str = "") -> None:
        """Direct embeddings: [*, L, D] with 1 <= L <= 384, the negative ones of the same length (never padded)."""
        if prompt_embeds is None:
            return
        n = int(prompt_embeds.shape[-2]) if torch.is_tensor(prompt_embeds) and prompt_embeds.dim() >= 2 else 0
        if not 1 <= n <= MAX_TEXT_TOKENS:
            raise ValueError(f"{what}`prompt_embeds` must hold 1..{MAX_TEXT_TOKENS} text tokens, got {n}")
        if negative_prompt_embeds is not None and int(negative_prompt_embeds.shape[-2]) != n:
            raise ValueError(f"{what}`negative_prompt_embeds` has {int(negative_prompt_embeds.shape[-2])} text tokens, "
                             f"`prompt_embeds` {n}: both must have the same length (pad the shorter text yourself)")

    # ---- the denoising loop over one UNet batch assembled from >= 1 requests of the same shape (reference :310-337)
    @staticmethod
    def _panel_values(value, num_samples: int, name: str) -> List[float]:
        """`guidance_scale` / `ip_scale` as one float per sample: a number for all of them, or `num_samples` numbers."""
        if _is_number(value):
            return [float(value)] * num_samples
        vals = [float(v) for v in (value.reshape(-1).tolist() if torch.is_tensor(value) else value)]
        if len(vals) != num_samples:
            raise ValueError(f"`{name}`: a number or {num_samples} numbers (num_samples) are needed, got {len(vals)}")
        return vals

    @staticmethod
    def _cfg_side(guidance: List[float]) -> bool:
        """Classifier-free guidance changes the batch layout, so it is on (every value > 1) or off for a whole batch."""
        on = [g > 1 for g in guidance]
        if any(on) != all(on):
            raise ValueError(f"guidance scales {guidance} mix classifier-free guidance on (> 1) and off (<= 1) in one "
                             f"UNet batch; run them in separate calls (serving: separate buckets)")
        return all(on)

    @staticmethod
    def _prompt_run_info(infos) -> dict:
        """`last_run_info` entries of a UNet batch: its chunk count and the prompt ids dropped, summed over its requests."""
        infos = [i for i in infos if i]
        dropped = [i["prompt_tokens_dropped"] for i in infos]
        return {"prompt_chunks": max([i["prompt_chunks"] for i in infos], default=1),
                "prompt_tokens_dropped": None if any(d is None for d in dropped) else sum(dropped)}

    def _denoise(self, conds, num_inference_steps, callback_on_step_end=None) -> Tensor:
        device = self._execution_device
        guidance = [g for c in conds for g in c["guidance"]]          # per panel, in batch order
        ip_scales = [s for c in conds for s in c["ip_scales"]]
        self._cfg_side(guidance)
        self._guidance_scale = guidance[-1]
        do_cfg = self.do_classifier_free_guidance
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        lat = torch.cat([c["lat"] for c in conds], dim=0)
        num_samples = lat.shape[0]
        H, W = lat.shape[-2], lat.shape[-1]
        aspect_ratio = H / W
        lengths = sorted({int(c[side][0].shape[1]) for c in conds for side in ("pos", "neg")})
        if len(lengths) > 1:              # one engine, and one UNet batch, has one text length
            raise ValueError(f"the requests of one UNet batch have text contexts of {lengths[0]} and {lengths[-1]} tokens "
                             f"({-(-lengths[0] // 77)} and {-(-lengths[-1] // 77)} prompt chunks): run them in separate "
                             f"batches (serving: `bucket_key` keeps them apart)")
        cat = lambda side, i: torch.cat([c[side][i] for c in conds], dim=0)
        prompt_embeds, add_text_embeds, img, bbox, dialog = (cat("pos", i) for i in range(5))
        add_time_ids = torch.cat([c["time_ids"] for c in conds], dim=0)
        if do_cfg:  # CFG batch layout: all negative rows, then all conditional rows (reference :300-309)
            prompt_embeds = torch.cat([cat("neg", 0), prompt_embeds], dim=0)
            add_text_embeds = torch.cat([cat("neg", 1), add_text_embeds], dim=0)
            add_time_ids = torch.cat([add_time_ids, add_time_ids], dim=0)
            img = torch.cat([cat("neg", 2), img], dim=0)
            bbox = torch.cat([cat("neg", 3), bbox], dim=0)
            dialog = torch.cat([cat("neg", 4), dialog], dim=0)
        else:
            # Without CFG the reference still passes bbox = cat([negative_ip_bbox, ip_bbox]) (reference :270-273) while the
            # UNet batch is only the `num_samples` conditional rows, so its mask builder indexes the FIRST num_samples rows:
            # the all-zero negative boxes (attention_processor.py:141-163 loops `for i in range(batch)`).  Mirrored here so
            # guidance_scale <= 1 gives the reference's images; `dialog_bbox` is not concatenated there and stays positive.
            bbox = cat("neg", 3)
        enc = torch.cat([prompt_embeds, img], dim=1)

        # one plan replay per step
        B = enc.shape[0]
        eng = self.unet.engine(B, H, W, aspect_ratio, text_tokens=prompt_embeds.shape[1])
        redraw = [c.get("redraw") for c in conds]
        if any(r is None for r in redraw) and any(r is not None for r in redraw):
            raise ValueError("a UNet batch is all region redraw or all plain sampling, not a mix")
        redraw = None if redraw[0] is None else redraw
        t_start = 0
        if redraw is not None:
            if len({r["strength"] for r in redraw}) != 1:
                raise ValueError("the redraw requests of one UNet batch must share `strength` (one schedule per batch)")
            t_start = self.scheduler.start_index(redraw[0]["strength"])
        steps_run = num_inference_steps - t_start
        eng.build_sampler(num_samples, self.scheduler.kind, do_cfg, redraw=redraw is not None)
        # rows n and ns + n of a CFG batch are panel n: both carry its IP scale
        eng.set_request(enc, add_text_embeds, add_time_ids, bbox, dialog_pixel_boxes(dialog, H, W),
                        ip_scales + ip_scales if do_cfg else ip_scales)
        # DPM-Solver++ rows; None for Euler / DDIM.  A redraw that starts mid-schedule runs its first row first order
        solver = self.scheduler.solver_table() if not t_start else self.scheduler.solver_table(start=t_start)
        # the panels' own seeds, in batch order: a panel's noise does not depend on the requests batched beside it
        seeds = [v for c in conds for v in c["noise_seeds"]] if self.scheduler.stochastic else None
        # a redraw loads the rows [t_start:] of every table; the device counter still starts at 0, so Euler Ancestral's
        # Philox step index is the run-relative step
        eng.load_schedule(torch.from_numpy(self.scheduler.coef_table(guidance[0])[t_start:]),
                          None if solver is None else torch.from_numpy(solver), seeds, guidance=guidance)
        if redraw is None:
            eng.latents.copy_(lat)
        else:                                              # the prep plan writes the start state out of this buffer
            mask = torch.cat([r["mask"] for r in redraw], dim=0)
            eng.load_redraw(torch.cat([r["x0"] for r in redraw], dim=0), lat, mask,
                            torch.from_numpy(self.scheduler.renoise_table()[t_start:]),
                            full_strength=redraw[0]["strength"] == 1.0,
                            init_noise_sigma=self.scheduler.init_noise_sigma)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=device)
        st = self._stream
        st.wait_stream(torch.cuda.current_stream(device))
        graph = False
        with torch.cuda.stream(st):
            eng.prep_plan.run(st.cuda_stream)
            n0 = 0
            if self.use_graph:
                if not eng.step_plan.captured:
                    eng.step_plan.run(st.cuda_stream)          # first step eager (also warms lazy kernel state)
                    n0 = 1
                    eng.step_plan.capture(st.cuda_stream)
                graph = True
            timesteps = self.scheduler.timesteps[t_start:]     # a callback gets the run-relative index and the true timestep

            def hook(i):
                # diffusers' contract [3P]: `latents = callback_outputs.pop("latents", latents)` - a callback may return a
                # dict with replaced latents instead of editing `eng.latents` in place; both forms are honoured
                ret = callback_on_step_end(self, i, timesteps[i], {"latents": eng.latents})
                if isinstance(ret, dict):
                    new = ret.get("latents")
                    if isinstance(new, Tensor) and new.data_ptr() != eng.latents.data_ptr():
                        eng.latents.copy_(new.to(eng.latents.device, eng.latents.dtype).reshape(eng.latents.shape))

            if n0 and callback_on_step_end is not None:
                hook(0)
            for i in range(n0, steps_run):
                if self._interrupt:                               # reference :314-315 `if self.interrupt: continue`
                    continue
                if graph:
                    eng.step_plan.replay(st.cuda_stream)
                else:
                    eng.step_plan.run(st.cuda_stream)
                if callback_on_step_end is not None:              # launched, not synchronised: the hook sees device tensors
                    hook(i)
        torch.cuda.current_stream(device).wait_stream(st)
        self.last_run_info = {"graph": graph, "ops_per_step": eng.step_plan.n, "batch": B, "latent_hw": (H, W),
                              "noise_seeds": seeds, "guidance_scales": guidance, "ip_scales": ip_scales}
        self.last_run_info.update(self._prompt_run_info([c.get("prompt_info") for c in conds]))
        if redraw is not None:
            self.last_run_info["redraw"] = {"t_start": t_start, "steps_run": steps_run,
                                            "repaint_fraction": float(mask.mean())}
        return eng.latents.clone()

    # ---- reference :339-367: VAE decode + image_processor.postprocess
    def _postprocess(self, out_latents: Tensor, output_type: str):
        if output_type == "latent" or self.vae is None:
            if output_type != "latent" and self.vae is None:
                raise ValueError("no VAE registered: call with output_type='latent'")
            return out_latents
        scaling = getattr(getattr(self.vae, "config", None), "scaling_factor", 0.13025)
        if output_type == "pil" and isinstance(self.vae, VaeDecoderEngine) and out_latents.is_cuda \
                and (out_latents.shape[2] * out_latents.shape[3] * 64) % 4 == 0 and out_latents.shape[0] > 1:
            return self._decode_to_pil_pipelined(out_latents, scaling)
        if isinstance(self.vae, VaeDecoderEngine):  # incl. postprocess' denormalize, all on the HIP kernels
            image = self.vae.decode(out_latents, return_dict=False, scaling_factor=scaling, denormalize=True,
                                    latents_affine=True)[0]      # latents_mean / latents_std (:348-357) folded at load time
        else:
            vc = getattr(self.vae, "config", None)
            lm, ls = getattr(vc, "latents_mean", None), getattr(vc, "latents_std", None)
            z = out_latents.float()
            if lm is not None and ls is not None:                # reference :348-357, a user-supplied decoder object
                view = lambda v: torch.tensor(list(v), dtype=z.dtype, device=z.device).view(1, -1, 1, 1)
                z = z * view(ls) / scaling + view(lm)
            else:
                z = z / scaling
            image = self.vae.decode(z, return_dict=False)[0]
            image = (image / 2 + 0.5).clamp(0, 1)
        if output_type == "pt":
            return image
        from PIL import Image
        if output_type == "pil" and image.is_cuda and image.dtype == torch.float32 and image.shape[1] == 3 \
                and (image.shape[2] * image.shape[3]) % 4 == 0:
            # (x*255).round() -> uint8 NHWC on the device: 3 B/pixel cross PCIe instead of 12, no host arithmetic
            from . import ops
            u8 = ops.image_to_u8(image.contiguous())
            host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(u8, non_blocking=True)
            torch.cuda.current_stream(image.device).synchronize()
            return [Image.fromarray(im) for im in host.numpy()]
        image = image.permute(0, 2, 3, 1).float().cpu().numpy()
        if output_type == "np":
            return image
        return [Image.fromarray((im * 255).round().astype("uint8")) for im in image]

    def _decode_to_pil_pipelined(self, out_latents: Tensor, scaling: float):
        """`vae.decode` + `image_processor.postprocess(output_type="pil")` (reference :359-367) for several images, the same
        kernels and bytes as the one-shot path above, but chunk by chunk: while the decoder works on chunk i + 1 the host wraps the
        uint8 pixels of chunk i (already copied to pinned memory) into PIL images - the ~1.5 ms per 1024 x 1024 image that
        `Image.fromarray` costs no longer sits behind the whole decode with the GPU idle."""
        from PIL import Image
        from . import ops
        B, _, h, w = out_latents.shape
        chunk = self.vae.decode_chunk(h, w, B)
        stream = torch.cuda.current_stream(out_latents.device)
        pending, images = [], []

        def drain(n_keep):
            while len(pending) > n_keep:
                ev, host = pending.pop(0)
                ev.synchronize()
                images.extend(Image.fromarray(im) for im in host.numpy())

        for i in range(0, B, chunk):
            img = self.vae.decode(out_latents[i:i + chunk], return_dict=False, scaling_factor=scaling, denormalize=True,
                                  latents_affine=True)[0]
            u8 = ops.image_to_u8(img.contiguous())
            host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(u8, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            pending.append((ev, host))
            drain(1)          # wrap the PREVIOUS chunk while this one is still on the GPU
        drain(0)
        return images

    def _encode_request_images(self, requests: List[dict], images: List[Optional[Tensor]]) -> List[dict]:
        """The `redraw_image` requests of a batch with `redraw_latents` in the picture's place: all pictures go through the
        VAE encoder in ONE `encode_latents` call (they share height and width).  Seeds: all picture requests or none."""
        idx = [i for i, im in enumerate(images) if im is not None]
        clean = [{k: v for k, v in r.items() if k not in ("redraw_image", "redraw_image_seeds")} for r in requests]
        if not idx:
            return clean
        if len({images[i].dtype for i in idx}) != 1:
            raise ValueError("generate_batch: the `redraw_image`s of one batch are all uint8 or all float")
        seeded = [requests[i].get("redraw_image_seeds") is not None for i in idx]
        if any(seeded) != all(seeded):
            raise ValueError("generate_batch: `redraw_image_seeds` for every `redraw_image` of the batch, or for none")
        seeds = None
        if all(seeded):
            seeds = []
            for i in idx:
                s = [int(v) for v in requests[i]["redraw_image_seeds"]]
                if len(s) != images[i].shape[0]:
                    raise ValueError(f"generate_batch: {images[i].shape[0]} `redraw_image_seeds` are needed, got {len(s)}")
                seeds += s
        lat = self._vae_encoder().encode_latents(torch.cat([images[i] for i in idx]), seeds)
        off = 0
        for i in idx:
            n = images[i].shape[0]
            clean[i]["redraw_latents"] = lat[off:off + n]
            off += n
        return clean

    # ---- LoRA adapters of the UNet (diffusers protocol names; lora.py)
    def load_lora_weights(self, path_or_dict, adapter_name: str = "default", alpha: Optional[float] = None,
                          unet_only: bool = False) -> int:
        """Load a UNet LoRA (`.safetensors`, `.bin` / `.pth` read with weights_only=True, or a state dict; peft or diffusers key
        names) under `adapter_name`; `set_adapters` activates it.  Adapters of the text encoders are not merged: their keys are
        refused like every other unknown key unless `unet_only=True`, which drops them.  Returns how many keys were dropped."""
        from .lora import drop_text_encoder_keys, read_lora_file
        sd = path_or_dict if isinstance(path_or_dict, dict) else read_lora_file(path_or_dict)
        dropped = 0
        if unet_only:
            sd, dropped = drop_text_encoder_keys(sd)
        self.unet.load_lora_adapter(sd, adapter_name, alpha)
        self.last_lora_dropped_keys = dropped
        return dropped

    def set_adapters(self, adapter_names, adapter_weights=1.0):
        self.unet.set_adapters(adapter_names, adapter_weights)

    def delete_adapters(self, adapter_names):
        self.unet.delete_adapters(adapter_names)

    def unload_lora_weights(self):
        """Back to the base weights; every loaded adapter is dropped."""
        self.unet.set_adapters([])
        self.unet.delete_adapters(self.unet.loaded_adapters())

    # ---- several requests of one shape in ONE UNet batch (serving front-end)
    def generate_batch(self, requests: List[dict], output_type: str = "pil") -> List[Any]:
        """`_generate_batch` under the adapter state the requests ask for.  A request may carry `lora={name: weight, ...}`
        ({} = no adapter; names as loaded with `load_lora_weights`); without the field it runs on whatever is set.  The merged
        weights are a property of the whole UNet batch, so a batch that mixes states is refused (`serving.bucket_key` keeps
        them apart); the state is set for the batch and the previous one restored afterwards, also on an exception."""
        absent = object()
        states = [r.get("lora", absent) for r in requests]
        norm = lambda st: st if st is absent else tuple(sorted((str(k), float(v)) for k, v in dict(st or {}).items()))
        if len({norm(st) for st in states}) > 1:
            raise ValueError("generate_batch: requests of one batch must share their `lora` adapters and weights")
        held = self._keep_adapters_until                  # inside `hold_adapters()`: the state from before the run
        if not requests or (states[0] is absent and held is None):
            return self._generate_batch(requests, output_type)
        # adapters are merged in sorted-name order for a request (its dict has no order to rely on); a batch without the
        # field inside a held run goes back to the state from before the run, in that state's own order
        want = list(held.items()) if states[0] is absent else list(norm(states[0]))
        before = self.unet.adapter_weights()
        requests = [{k: v for k, v in r.items() if k != "lora"} for r in requests]
        if want == list(before.items()):                  # already the state asked for: no switch, nothing to restore
            return self._generate_batch(requests, output_type)
        self.unet.set_adapters([k for k, _ in want], [v for _, v in want])
        try:
            return self._generate_batch(requests, output_type)
        finally:
            if held is None:
                self.unet.set_adapters(list(before), list(before.values()))

    def hold_adapters(self):
        """Context manager for a run of `generate_batch` calls (`BucketBatcher.run`): inside it a batch leaves its adapter
        state set - the next batch switches only if it wants another one - and the state from before is restored once, at
        the end, also on an exception."""
        import contextlib

        @contextlib.contextmanager
        def hold():
            if self._keep_adapters_until is not None:      # nested: the outer one restores
                yield
                return
            self._keep_adapters_until = before = self.unet.adapter_weights()
            try:
                yield
            finally:
                self._keep_adapters_until = None
                if list(self.unet.adapter_weights().items()) != list(before.items()):
                    self.unet.set_adapters(list(before), list(before.values()))
        return hold()

    # a request of `generate_batch` / `generate_continuous`: the keyword arguments of `__call__` (without `output_type`)
    _REQUEST_FIELDS = ("prompt", "prompt_2", "height", "width", "num_inference_steps", "guidance_scale", "negative_prompt",
                       "negative_prompt_2", "num_samples", "generator", "original_size", "crops_coords_top_left", "target_size",
                       "ip_images", "ip_image_embeds", "ip_bbox", "ip_scale", "dialog_bbox", "latents", "prompt_embeds",
                       "negative_prompt_embeds", "pooled_prompt_embeds", "negative_pooled_prompt_embeds", "noise_seeds",
                       "redraw_latents", "redraw_bbox", "redraw_mask", "strength")
    _REQUEST_KEYWORDS = ("max_prompt_chunks",)     # request fields `_conditioning` takes by keyword (behind `redraw_image`)
    _REQUEST_DEFAULTS = dict(prompt_2=None, height=None, width=None, num_inference_steps=40, guidance_scale=5.0,
                             negative_prompt=None, negative_prompt_2=None, num_samples=1, generator=None, original_size=None,
                             crops_coords_top_left=(0, 0), target_size=None, ip_images=[], ip_image_embeds=None, ip_bbox=[],
                             ip_scale=1.0, dialog_bbox=[], latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                             pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, noise_seeds=None,
                             redraw_latents=None, redraw_bbox=None, redraw_mask=None, strength=1.0, max_prompt_chunks=1)

    @torch.no_grad()
    def _generate_batch(self, requests: List[dict], output_type: str = "pil") -> List[Any]:
        """Each request: the keyword arguments of `__call__` (without `output_type`).  All must share height, width and
        num_inference_steps (`serving.bucket_key`), and their guidance scales lie on one side of 1 (classifier-free
        guidance is on or off for the whole UNet batch); prompts, character references, boxes, seeds, `num_samples`,
        `guidance_scale` and `ip_scale` are per request.  A batch is all region redraw (`redraw_latents` or `redraw_image`, each
        request with its own kept latents / picture and mask, one shared `strength`) or all plain; the pictures of a batch are
        encoded in one pass.  Returns one `.images`-like object per request,
        in order."""
        if not requests:
            return []
        self._interrupt = False          # like `__call__` (reference :226): an earlier interrupted call must not leak into this one
        key = lambda r: (r.get("height"), r.get("width"), r.get("num_inference_steps", 40))
        if any(key(r) != key(requests[0]) for r in requests):
            raise ValueError("generate_batch: requests must share height/width/steps")
        sides = [self._cfg_side(self._panel_values(r.get("guidance_scale", 5.0), r.get("num_samples", 1) or 1, "guidance_scale"))
                 for r in requests]                 # before any encoder runs
        if any(s != sides[0] for s in sides):
            raise ValueError("generate_batch: requests mix classifier-free guidance on (guidance_scale > 1) and off (<= 1)")
        rd = [r.get("redraw_latents") is not None or r.get("redraw_image") is not None for r in requests]
        if any(rd) != all(rd):
            raise ValueError("generate_batch: a batch is all region redraw (`redraw_latents` / `redraw_image`) or all plain, not a mix")
        images = []
        self._check_prompt_chunks(requests, "generate_batch")
        for r in requests:                          # every request's redraw fields, before any encoder runs
            h = r.get("height") or self.default_sample_size * self.vae_scale_factor
            w = r.get("width") or self.default_sample_size * self.vae_scale_factor
            ns = r.get("num_samples", 1) or 1
            img = self._redraw_image_input(r.get("redraw_image"), r.get("redraw_latents"), ns, h, w)
            if img is None and r.get("redraw_image_seeds") is not None:
                raise ValueError("generate_batch: `redraw_image_seeds` without `redraw_image`")
            images.append(img)
            x0 = r.get("redraw_latents") if img is None else torch.zeros(1, 4, h // self.vae_scale_factor, w // self.vae_scale_factor)
            self._redraw_inputs(x0, r.get("redraw_bbox"), r.get("redraw_mask"), r.get("strength", 1.0), ns, h, w)
        if all(rd) and len({float(r.get("strength", 1.0)) for r in requests}) != 1:
            raise ValueError("generate_batch: the redraw requests of one batch must share `strength`")
        if any(im is not None for im in images):    # "no step would run" is a ValueError before the VAE encoder too
            self.scheduler.set_timesteps(requests[0].get("num_inference_steps", 40), device=self._execution_device)
            self.scheduler.start_index(float(requests[0].get("strength", 1.0)))
        requests = self._encode_request_images(requests, images)
        names, defaults = self._REQUEST_FIELDS, self._REQUEST_DEFAULTS
        conds = []
        for r in requests:
            unknown = set(r) - set(names) - set(self._REQUEST_KEYWORDS)
            if unknown:
                raise TypeError(f"generate_batch: unknown request fields {sorted(unknown)}")
            conds.append(self._conditioning(*[r[n] if n in r else defaults[n] for n in names],
                                            **{n: r[n] for n in self._REQUEST_KEYWORDS if n in r}))
        out = self._denoise(conds, requests[0].get("num_inference_steps", 40))
        images = self._postprocess(out, output_type)
        res, off = [], 0
        for c in conds:
            res.append(images[off:off + c["n"]])
            off += c["n"]
        return res

    # ---- continuous batching: per-panel schedules, slots refilled in flight (serving front-end)
    def generate_continuous(self, requests: List[dict], slots: int, output_type: str = "pil") -> List[Any]:
        """Run `requests` (the dicts `generate_batch` takes) through ONE UNet batch of `slots` panel slots in which every
        slot carries its own schedule: when a panel finishes, its slot goes to the next request while the others keep
        going.  All requests share height, width, the side of 1 their guidance is on and `lora` (one adapter state for the
        run, handled like `generate_batch` handles it); everything else is per request - `num_inference_steps`,
        `strength`, plain or region redraw, prompts, references, boxes, seeds, both sliders.  Requests are admitted
        strictly in order, the head of the queue at the first step boundary at which `num_samples` slots are free
        (`serving.plan_continuous`, which this method executes); a waiting request's conditioning runs at its admission.
        If any request is a redraw the sampler is the redraw sampler and plain panels carry mask 1.  Finished latents are
        cloned out of their slots at the boundary at which they finish and decoded after the run; results come back in
        request order.  `num_samples > slots` is a ValueError before anything runs, as is every other input check of every
        request (`_check_continuous`: sizes, guidance sides, redraw fields, step counts, prompts and references, slider and
        seed lists, given latents - `latents` is [num_samples, 4, H/8, W/8] here).  `last_run_info["continuous"]` is the executed plan.  There is no `callback_on_step_end` here."""
        absent = object()
        states = [r.get("lora", absent) for r in requests]
        norm = lambda st: st if st is absent else tuple(sorted((str(k), float(v)) for k, v in dict(st or {}).items()))
        if len({norm(st) for st in states}) > 1:
            raise ValueError("generate_continuous: the requests of one run must share their `lora` adapters and weights")
        held = self._keep_adapters_until
        if not requests or (states[0] is absent and held is None):
            return self._generate_continuous(requests, slots, output_type)
        want = list(held.items()) if states[0] is absent else list(norm(states[0]))
        before = self.unet.adapter_weights()
        requests = [{k: v for k, v in r.items() if k != "lora"} for r in requests]
        if want == list(before.items()):
            return self._generate_continuous(requests, slots, output_type)
        checked = self._check_continuous(requests, slots)    # every refusal before the weights are touched
        self.unet.set_adapters([k for k, _ in want], [v for _, v in want])
        try:
            return self._generate_continuous(requests, slots, output_type, checked)
        finally:
            if held is None:
                self.unet.set_adapters(list(before), list(before.values()))

    def _check_continuous(self, requests: List[dict], slots: int):
        """Every input check of every request of a continuous run, before any encoder: returns (plan, schedules, images,
        do_cfg) - `serving.plan_continuous` over the steps each request runs, each request's `panel_schedule`, and its
        `redraw_image` as a host tensor (or None)."""
        from . import ops
        from .serving import plan_continuous
        slots = int(slots)
        if slots < 1:
            raise ValueError("generate_continuous: slots must be >= 1")
        names = self._REQUEST_FIELDS
        for i, r in enumerate(requests):
            unknown = set(r) - set(names) - {"redraw_image", "redraw_image_seeds"} - set(self._REQUEST_KEYWORDS)
            if unknown:
                raise TypeError(f"generate_continuous: unknown request fields {sorted(unknown)}")
            if int(r.get("num_samples", 1) or 1) > slots:
                raise ValueError(f"generate_continuous: request {i} has num_samples {r.get('num_samples')} > slots {slots}")
        size = lambda r: (r.get("height") or self.default_sample_size * self.vae_scale_factor,
                          r.get("width") or self.default_sample_size * self.vae_scale_factor)
        if any(size(r) != size(requests[0]) for r in requests):
            raise ValueError("generate_continuous: requests must share height and width")
        sides = [self._cfg_side(self._panel_values(r.get("guidance_scale", 5.0), r.get("num_samples", 1) or 1, "guidance_scale"))
                 for r in requests]
        if any(s != sides[0] for s in sides):
            raise ValueError("generate_continuous: requests mix classifier-free guidance on (guidance_scale > 1) and off (<= 1)")
        self._check_prompt_chunks(requests, "generate_continuous")
        schedules, images = [], []
        for i, r in enumerate(requests):
            h, w = size(r)
            ns = r.get("num_samples", 1) or 1
            img = self._redraw_image_input(r.get("redraw_image"), r.get("redraw_latents"), ns, h, w)
            if img is None and r.get("redraw_image_seeds") is not None:
                raise ValueError("generate_continuous: `redraw_image_seeds` without `redraw_image`")
            images.append(img)
            x0 = r.get("redraw_latents") if img is None else torch.zeros(1, 4, h // self.vae_scale_factor, w // self.vae_scale_factor)
            rd = self._redraw_inputs(x0, r.get("redraw_bbox"), r.get("redraw_mask"), r.get("strength", 1.0), ns, h, w)
            self._check_request_fields(i, r, img, ns, h, w)
            steps = r.get("num_inference_steps", 40)
            if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
                raise ValueError(f"generate_continuous: request {i}: num_inference_steps {steps!r} is not a positive integer")
            sch = self.scheduler.panel_schedule(steps, 1.0 if rd is None else rd["strength"])   # "no step would run" raises here
            if sch["steps"] > ops.PANEL_MAX_ROWS:
                raise ValueError(f"generate_continuous: request {i} runs {sch['steps']} steps, a slot holds {ops.PANEL_MAX_ROWS}")
            schedules.append(sch)
        plan = plan_continuous([s["steps"] for s in schedules], [int(r.get("num_samples", 1) or 1) for r in requests], slots)
        return plan, schedules, images, sides[0]

    def _text_tokens(self, request: dict) -> int:
        """The text length of a request's context: that of its `prompt_embeds`, else 77 per prompt chunk."""
        pe = request.get("prompt_embeds")
        return int(pe.shape[-2]) if pe is not None else 77 * self.prompt_chunk_count(request)

    def _check_prompt_chunks(self, requests: List[dict], who: str) -> None:
        """Before any encoder runs: every request's `max_prompt_chunks` and direct embeddings, and that all requests of
        the UNet batch have one text length (the engine is sized by it)."""
        lengths = []
        for i, r in enumerate(requests):
            what = f"{who}: request {i}: "
            try:
                check_max_prompt_chunks(r.get("max_prompt_chunks", 1))
            except ValueError as e:
                raise ValueError(what + str(e)) from None
            self._check_prompt_embeds(r.get("prompt_embeds"), r.get("negative_prompt_embeds"), what)
            lengths.append(self._text_tokens(r))
        for i, n in enumerate(lengths):
            if n != lengths[0]:
                raise ValueError(f"{who}: request {i} has {-(-n // 77)} prompt chunks ({n} text tokens), request 0 has "
                                 f"{-(-lengths[0] // 77)} ({lengths[0]}): requests with different chunk counts never share a "
                                 f"UNet batch (`serving.bucket_key` / `continuous_key` keep them apart)")

    def _check_request_fields(self, i: int, r: dict, image: Optional[Tensor], ns: int, h: int, w: int) -> None:
        """The checks `_conditioning` and `_encode_request_images` would make of request i at its admission - by then other
        requests' steps have run -, made up front instead: prompts and references, the size, the slider and seed lists,
        given latents, the picture's seeds, and a prompt without text encoders."""
        what = f"generate_continuous: request {i}: "
        get = lambda k: r[k] if k in r else self._REQUEST_DEFAULTS.get(k)
        self.check_inputs(get("prompt"), get("prompt_2"), get("ip_images"), get("ip_image_embeds"), list(get("ip_bbox")))
        if h % self.vae_scale_factor or w % self.vae_scale_factor:
            raise ValueError(f"{what}`height` and `width` have to be divisible by {self.vae_scale_factor} but are {h} and {w}.")
        self._panel_values(get("ip_scale"), ns, "ip_scale")
        seeds = get("noise_seeds")
        if seeds is not None:
            if not self.scheduler.stochastic:
                raise ValueError(f"{what}`noise_seeds` given, but {type(self.scheduler).__name__} draws no noise")
            seeds = [int(v) for v in seeds]
            if len(seeds) != ns or any(v < 0 or v >= 2 ** 63 for v in seeds):
                raise ValueError(f"{what}`noise_seeds`: {ns} integers in [0, 2**63) are needed, got {seeds}")
        gen = get("generator")
        if isinstance(gen, (list, tuple)) and len(gen) != ns:
            raise ValueError(f"{what}{len(gen)} generators for {ns} samples")
        lat = get("latents")
        shape = (ns, self.unet.config.in_channels, h // self.vae_scale_factor, w // self.vae_scale_factor)
        if lat is not None and (not torch.is_tensor(lat) or tuple(lat.shape) != shape):
            raise ValueError(f"{what}`latents` {tuple(lat.shape) if torch.is_tensor(lat) else type(lat)}, {shape} is needed")
        rs = get("redraw_image_seeds") if "redraw_image_seeds" in r else None
        if image is not None and rs is not None and len([int(v) for v in rs]) != image.shape[0]:
            raise ValueError(f"{what}{image.shape[0]} `redraw_image_seeds` are needed, got {len(rs)}")
        if get("prompt_embeds") is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError(f"{what}no text encoders registered: pass prompt_embeds / negative_prompt_embeds / "
                                 "pooled_prompt_embeds / negative_pooled_prompt_embeds")
        elif get("pooled_prompt_embeds") is None:
            raise ValueError(f"{what}`prompt_embeds` needs `pooled_prompt_embeds`")

    @torch.no_grad()
    def _generate_continuous(self, requests: List[dict], slots: int, output_type: str = "pil", checked=None) -> List[Any]:
        if not requests:
            return []
        self._interrupt = False
        slots = int(slots)
        plan, schedules, images, do_cfg = checked if checked is not None else self._check_continuous(requests, slots)
        device = self._execution_device
        names, defaults = self._REQUEST_FIELDS, self._REQUEST_DEFAULTS
        any_redraw = any(r.get("redraw_latents") is not None or r.get("redraw_image") is not None for r in requests)
        r0 = requests[0]
        H = (r0.get("height") or self.default_sample_size * self.vae_scale_factor) // self.vae_scale_factor
        W = (r0.get("width") or self.default_sample_size * self.vae_scale_factor) // self.vae_scale_factor
        B = 2 * slots if do_cfg else slots
        eng = self.unet.engine(B, H, W, H / W, text_tokens=self._text_tokens(requests[0]))
        eng.build_sampler(slots, self.scheduler.kind, do_cfg, redraw=any_redraw, panel_schedules=True)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=device)
        st = self._stream
        st.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(st):
            eng.reset_slots()
        admit, finish, where = {}, {}, {}
        for s, r, sl in plan["admissions"]:
            admit.setdefault(s, []).append((r, sl))
            finish.setdefault(plan["finish"][r], []).append(r)
            where[r] = sl
        out: List[Optional[Tensor]] = [None] * len(requests)
        graph = False
        # The conditioning of a request is made on the caller's stream and read on the sampling stream, which runs far behind
        # the host.  Every such tensor is told so (`record_stream`) and kept referenced until the caller's stream has waited
        # for the sampling stream at the end of the run: its memory cannot go to a later request's conditioning before the
        # copies that read it have executed.
        alive: list = []

        def hand_over(*tensors):
            for t in tensors:
                if torch.is_tensor(t):
                    if t.is_cuda:
                        t.record_stream(st)
                    alive.append(t)

        def admit_request(r, sl, s):
            req = self._encode_request_images([requests[r]], [images[r]])[0]
            cond = self._conditioning(*[req[n] if n in req else defaults[n] for n in names],
                                      **{n: req[n] for n in self._REQUEST_KEYWORDS if n in req})
            if cond["pos"][0].shape[1] + cond["pos"][2].shape[1] != eng.enc.shape[1]:
                raise ValueError(f"generate_continuous: request {r} has a text context of {cond['pos'][0].shape[1]} tokens, "
                                 f"the run's engine {eng.text_tokens}")
            sch = schedules[r]
            pos, neg = cond["pos"], cond["neg"]
            if do_cfg:     # a slot's rows in batch order: the negative ones, then the conditional ones (`_denoise`)
                enc = torch.cat([torch.cat([neg[0], neg[2]], dim=1), torch.cat([pos[0], pos[2]], dim=1)], dim=0)
                text, tids = torch.cat([neg[1], pos[1]], dim=0), torch.cat([cond["time_ids"]] * 2, dim=0)
                bbox, dialog = torch.cat([neg[3], pos[3]], dim=0), torch.cat([neg[4], pos[4]], dim=0)
            else:          # without CFG the rows carry the all-zero negative boxes, like `_denoise`
                enc, text, tids = torch.cat([pos[0], pos[2]], dim=1), pos[1], cond["time_ids"]
                bbox, dialog = neg[3], pos[4]
            rd = cond["redraw"]
            boxes = dialog_pixel_boxes(dialog, H, W)
            hand_over(enc, text, tids, bbox, dialog, boxes, cond["lat"], cond["time_ids"], *pos, *neg,
                      *((rd["x0"], rd["mask"]) if rd is not None else ()))
            st.wait_stream(torch.cuda.current_stream(device))      # the conditioning ran on the caller's stream
            with torch.cuda.stream(st):
                eng.set_slot_request(sl, enc, text, tids, bbox, boxes, cond["ip_scales"])
                eng.load_slots(sl, torch.from_numpy(sch["rows"]),
                               None if sch["solver_rows"] is None else torch.from_numpy(sch["solver_rows"]),
                               torch.from_numpy(sch["renoise_rows"]) if rd is not None else None,
                               cond["noise_seeds"], cond["guidance"], start=s,
                               latents=cond["lat"] if rd is None else None,
                               redraw=None if rd is None else {"x0": rd["x0"], "noise": cond["lat"], "mask": rd["mask"],
                                                                "full_strength": rd["strength"] == 1.0},
                               init_noise_sigma=sch["init_noise_sigma"])
                eng.start_slots(sl)
            return cond

        conds = {}
        for s in range(plan["forwards"] + 1):
            if s in finish:                                        # this boundary: harvest, then hand the slots on
                with torch.cuda.stream(st):
                    for r in finish[s]:
                        idx = torch.tensor(where[r], dtype=torch.int64).pin_memory().to(device, non_blocking=True)
                        out[r] = eng.latents.index_select(0, idx)
            for r, sl in admit.get(s, []):
                conds[r] = admit_request(r, sl, s)
            if s == plan["forwards"]:
                break
            with torch.cuda.stream(st):
                if self.use_graph and not eng.step_plan.captured:
                    eng.step_plan.run(st.cuda_stream)              # first step eager (also warms lazy kernel state)
                    eng.step_plan.capture(st.cuda_stream)
                elif self.use_graph:
                    eng.step_plan.replay(st.cuda_stream)
                    graph = True
                else:
                    eng.step_plan.run(st.cuda_stream)
        torch.cuda.current_stream(device).wait_stream(st)
        for t in out:                                              # allocated on the sampling stream, read on the caller's
            t.record_stream(torch.cuda.current_stream(device))
        alive.clear()                                              # the caller's stream is behind every copy that read them
        self.last_run_info = {"graph": graph, "ops_per_step": eng.step_plan.n, "batch": B, "latent_hw": (H, W),
                              "noise_seeds": [conds[r]["noise_seeds"] for r in range(len(requests))],
                              "guidance_scales": [conds[r]["guidance"] for r in range(len(requests))],
                              "ip_scales": [conds[r]["ip_scales"] for r in range(len(requests))],
                              "continuous": dict(plan),
                              **self._prompt_run_info([conds[r].get("prompt_info") for r in range(len(requests))])}
        images_out = self._postprocess(torch.cat(out, dim=0), output_type)
        res, off = [], 0
        for r in range(len(requests)):
            n = out[r].shape[0]
            res.append(images_out[off:off + n])
            off += n
        return res
