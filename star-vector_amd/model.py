"""Host-side mirror of the reference's operator interface for the im2svg hot path.

Same names, argument meaning and error behaviour as the reference classes, so a caller of
``StarVectorForCausalLM.generate_im2svg`` / ``model.model.image_encoder`` / ``image_projection`` /
``svg_transformer.transformer.generate`` can switch without edits.  Every forward goes through the
C-ABI HIP engine (``engine.HipEngine``); there is no PyTorch compute path here.

Reference lines mirrored:
  StarVectorConfig / StarVectorForCausalLM   starvector/model/starvector_arch.py:96-193
  StarVectorBase orchestration               starvector/model/models/starvector_base.py:203-295
  StarVectorStarCoder (v1)                   starvector/model/models/starvector_v1.py:6-22
  ImageEncoder (clip branch)                 starvector/model/image_encoder/image_encoder.py:9-119
  Adapter                                    starvector/model/adapters/adapter.py:12-39
  StarCoderModel                             starvector/model/llm/starcoder.py:9-53
  ImageTrainProcessor                        starvector/data/util.py:40-68
"""
from __future__ import annotations

import json
import os
import sys
import contextlib
import dataclasses
import functools
import numbers
import threading
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from .engine import EngineConfig, HipEngine, prefill_chunk_rows as resolve_prefill_chunk_rows, resolve_kv_dtype, resolve_weight_dtype

# Set while the calling thread runs an exclusive job of a ContinuousBatcher (beam search, multi-row batches): inside it the
# mirror talks to the engine directly; every OTHER thread keeps going through the batcher's queue.
_EXCLUSIVE = threading.local()


def _in_exclusive_job() -> bool:
    return bool(getattr(_EXCLUSIVE, "active", False))


def _exclusive(batcher, fn):
    """`fn()` as an exclusive job of `batcher`: requests share the engine, the job runs with the engine to itself, in turn (FIFO with
    the generation requests).  The flag is thread-local: only the scheduler thread running the job sees it."""
    def job():
        _EXCLUSIVE.active = True
        try:
            return fn()
        finally:
            _EXCLUSIVE.active = False
    return batcher.run_exclusive(job)


def _call_lock(engine):
    """The lock one engine call (or one cb_reset .. cb_reset sequence) holds; engines without one take none."""
    return getattr(engine, "call_lock", None) or contextlib.nullcontext()


def _is_padded(mask) -> bool:
    """Whether an attention mask marks any padding.  Reading it is a device round trip when the mask lives on the GPU: ask once per call."""
    return mask is not None and not bool((mask == 1).all())


class _GenerateOutput(dict):
    """Stand-in for transformers' Generate*DecoderOnlyOutput when transformers is not importable: the same field names, read as
    attributes or as keys."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


_DECODER_ONLY_FIELDS = ("sequences", "scores", "logits", "attentions", "hidden_states", "past_key_values")
_BEAM_FIELDS = ("sequences", "sequences_scores", "scores", "logits", "beam_indices", "attentions", "hidden_states", "past_key_values")


def generate_output(beam: bool, **fields):
    """HF's GenerateDecoderOnlyOutput / GenerateBeamDecoderOnlyOutput (generation/utils.py) with `fields`, the rest None."""
    try:
        from transformers.generation.utils import GenerateBeamDecoderOnlyOutput, GenerateDecoderOnlyOutput
        return (GenerateBeamDecoderOnlyOutput if beam else GenerateDecoderOnlyOutput)(**fields)
    except ImportError:
        return _GenerateOutput({k: fields.get(k) for k in (_BEAM_FIELDS if beam else _DECODER_ONLY_FIELDS)})


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)   # data/util.py:33-38
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


class StarVectorConfig:
    """starvector_arch.py:96-131 (fields the hot path reads) + the engine sizing knobs."""
    model_type = "starvector"

    def __init__(self, starcoder_model_name: str = "bigcode/starcoderbase-1b", image_encoder_type: str = "clip",
                 adapter_norm: str = "layer_norm", image_size: int = 224, max_length: int = 8192,
                 max_length_train: int = 8192, use_flash_attn: bool = True, use_cache: bool = True,
                 num_attention_heads: int = 16, num_hidden_layers: int = 24, vocab_size: int = 49152,
                 hidden_size: int = 2048, num_kv_heads: int = 4, torch_dtype: str = "bfloat16",
                 # engine-only (not in the reference config): shapes that the reference takes from the HF
                 # sub-model configs, and the batch/sequence capacity the KV pool is sized for
                 n_inner: Optional[int] = None, n_positions: Optional[int] = None, added_tokens: Optional[int] = None,
                 vit_width: int = 1024, vit_layers: int = 23, vit_heads: int = 16, patch_size: int = 14,
                 max_batch: int = 32, exclusive_device: Optional[bool] = None, weight_dtype: Optional[str] = None,
                 kv_cache_dtype: Optional[str] = None, prefill_chunk_rows: Optional[int] = None, **kwargs):
        self.starcoder_model_name = starcoder_model_name
        self.image_encoder_type = image_encoder_type
        self.adapter_norm = adapter_norm
        self.image_size = image_size
        self.max_length = max_length
        self.max_length_train = max_length_train
        self.use_flash_attn = use_flash_attn
        self.use_cache = use_cache
        self.num_attention_heads = num_attention_heads
        self.num_hidden_layers = num_hidden_layers
        self.vocab_size = vocab_size
        self.hidden_size = hidden_size
        self.num_kv_heads = num_kv_heads
        self.torch_dtype = torch_dtype
        self.n_inner = n_inner if n_inner is not None else 4 * hidden_size
        v2 = "starcoder2" in starcoder_model_name
        # bigcode/starcoderbase-1b: 8192 learned positions; bigcode/starcoder2-7b: max_position_embeddings 16384
        self.n_positions = n_positions if n_positions is not None else (16384 if v2 else 8192)
        # [PAD] + <svg-start>,<image-start>,<caption-start> (llm/starcoder.py:40-53); v2 adds <svg-end> (llm/starcoder2.py:47)
        self.added_tokens = added_tokens if added_tokens is not None else (5 if v2 else 4)
        self.vit_width, self.vit_layers, self.vit_heads, self.patch_size = vit_width, vit_layers, vit_heads, patch_size
        self.max_batch = max_batch
        # one process per GPU and nothing else decoding on it (the deployment the engine is built for): allows the launches whose blocks
        # wait for each other (INTEGRATION.md "Deployment knob").  None = the environment decides (SV_EXCLUSIVE_DEVICE=1), default off
        # None: SV_EXCLUSIVE_DEVICE (0 / 1 / auto), default "auto" = the fused decode launches on until one of them finds the GPU shared, then off for good
        # with the failed call re-run (include/starvector_hip.h, sv_config.exclusive_device = 2): same tokens either way
        env = os.environ.get("SV_EXCLUSIVE_DEVICE", "auto")
        self.exclusive_device = ({"0": False, "1": True}.get(env, "auto")) if exclusive_device is None else exclusive_device
        # decoder weight format: "bf16" (the reference's precision), "fp8_e4m3" / "fp8", "mxfp4" (EngineConfig.weight_dtype).  None = the
        # environment's SV_WEIGHT_DTYPE, else "bf16"
        self.weight_dtype = resolve_weight_dtype(weight_dtype)
        # KV-cache format: "bf16" / "auto" (the reference's precision) or "fp8_e4m3" / "fp8" (EngineConfig.kv_dtype).  None = the environment's
        # SV_KV_DTYPE, else "bf16"
        self.kv_cache_dtype = resolve_kv_dtype(kv_cache_dtype)
        # row budget of the prompt passes (EngineConfig.prefill_chunk_rows; 0 = off).  None = the environment's SV_PREFILL_CHUNK_ROWS, else 0
        self.prefill_chunk_rows = resolve_prefill_chunk_rows(prefill_chunk_rows)
        for k, v in kwargs.items():
            setattr(self, k, v)

    @staticmethod
    def _visible_keys(window: int, semantics: str) -> int:
        if semantics not in ("flash_attention_2", "sdpa", "eager"):
            raise ValueError(f"window_semantics={semantics!r}: 'flash_attention_2' (W + 1 keys, transformers 4.49's FA2 call, "
                             "what the reference loads) or 'sdpa' / 'eager' (W keys)")
        window = int(window or 0)
        return window + 1 if (window > 0 and semantics == "flash_attention_2") else window

    @property
    def is_v2(self) -> bool:                      # starvector_arch.py:139-144 picks the class the same way
        return "starcoder2" in self.starcoder_model_name

    def engine_config(self) -> EngineConfig:
        dt = str(self.torch_dtype).replace("torch.", "")
        if dt in ("float16", "half", "float32", "float"):
            # the reference's 1B validation config is fp16 (configs/generation/hf/starvector-1b/im2svg.yaml:16) and
            # scripts/quickstart.py:16 casts the image to fp16: such callers keep working -- weights and inputs are converted at
            # the boundary, the engine computes in bfloat16 (same exponent range as fp32; token streams may differ from an fp16
            # run at near-ties, which is what any dtype change does)
            import warnings
            warnings.warn(f"torch_dtype={self.torch_dtype}: the HIP engine computes in bfloat16; weights and inputs are "
                          "converted at the boundary", stacklevel=2)
        elif dt not in ("bfloat16", "auto"):
            raise ValueError(f"unsupported torch_dtype={self.torch_dtype} (bfloat16, or float16 / float32 converted to it)")
        if self.is_v2:
            # StarVector-8B: siglip_384 tower + StarCoder2 decoder (configs/models/starvector-8b/im2svg-stack.yaml)
            if self.image_encoder_type != "siglip_384":
                raise NotImplementedError(f"image_encoder_type={self.image_encoder_type!r}: v2 is built for siglip_384")
            g = lambda k, d: getattr(self, k, d)
            return EngineConfig(image_size=g("siglip_image_size", 384), patch_size=g("siglip_patch_size", 16),
                                vit_width=self.vit_width, vit_layers=g("siglip_layers", 24), vit_heads=self.vit_heads,
                                adapter_norm=self.adapter_norm, hidden=self.hidden_size, n_layer=self.num_hidden_layers,
                                n_head=self.num_attention_heads, n_inner=self.n_inner,
                                vocab=self.vocab_size + self.added_tokens, n_positions=self.n_positions,
                                max_batch=self.max_batch, max_seq_len=min(self.max_length, self.n_positions), arch="v2",
                                n_kv_head=self.num_kv_heads, rope_theta=g("rope_theta", 1e6),
                                vit_mlp=g("siglip_mlp", 4096), vit_eps=1e-6,
                                # bigcode/starcoder2-7b config.json: sliding_window 4096.  The reference loads the decoder with
                                # attn_implementation="flash_attention_2" (llm/starcoder2.py:21-26); transformers 4.49 hands FA2
                                # window_size=(W, W), i.e. the query sees W + 1 keys, while its eager/sdpa mask (and later releases
                                # everywhere) show W.  `window_semantics` picks which one the engine's window (= number of visible
                                # keys) mirrors: "flash_attention_2" (default: what the reference runs) or "sdpa".
                                sliding_window=self._visible_keys(g("sliding_window", 4096), g("window_semantics", "flash_attention_2")),
                                exclusive_device=self.exclusive_device, weight_dtype=resolve_weight_dtype(self.weight_dtype),
                                kv_dtype=resolve_kv_dtype(getattr(self, "kv_cache_dtype", None)),
                                prefill_chunk_rows=resolve_prefill_chunk_rows(getattr(self, "prefill_chunk_rows", None)))
        if self.image_encoder_type != "clip":
            raise NotImplementedError(f"image_encoder_type={self.image_encoder_type!r}: v1 is built for the clip branch")
        return EngineConfig(image_size=self.image_size, patch_size=self.patch_size, vit_width=self.vit_width,
                            vit_layers=self.vit_layers, vit_heads=self.vit_heads, adapter_norm=self.adapter_norm,
                            hidden=self.hidden_size, n_layer=self.num_hidden_layers, n_head=self.num_attention_heads,
                            n_inner=self.n_inner, vocab=self.vocab_size + self.added_tokens,
                            n_positions=self.n_positions, max_batch=self.max_batch,
                            max_seq_len=min(self.max_length, self.n_positions), exclusive_device=self.exclusive_device,
                            weight_dtype=resolve_weight_dtype(self.weight_dtype),
                                kv_dtype=resolve_kv_dtype(getattr(self, "kv_cache_dtype", None)),
                                prefill_chunk_rows=resolve_prefill_chunk_rows(getattr(self, "prefill_chunk_rows", None)))


def config_from_checkpoint(cfg_json: Dict, shapes: Dict[str, tuple]) -> StarVectorConfig:
    """`config.json` of a reference checkpoint + the shapes of its tensors -> StarVectorConfig.  The reference takes the
    decoder's vocabulary (after `resize_token_embeddings`), position count and MLP width from the HF sub-model it
    instantiates (llm/starcoder.py:33-53, llm/starcoder2.py:22-53); offline they are read off the saved tensors, which
    is what those numbers ended up as.  Explicit entries of `cfg_json` win."""
    cfg = StarVectorConfig(**{**cfg_json, "torch_dtype": "bfloat16"})
    dec = "model.svg_transformer.transformer." + ("model." if cfg.is_v2 else "transformer.")
    emb = shapes.get(dec + ("embed_tokens.weight" if cfg.is_v2 else "wte.weight"))
    if emb is not None:
        if "hidden_size" not in cfg_json:
            cfg.hidden_size = int(emb[1])
        if "added_tokens" not in cfg_json:
            cfg.added_tokens = int(emb[0]) - int(cfg.vocab_size)
            if cfg.added_tokens < 0:
                raise ValueError(f"checkpoint embeds {emb[0]} tokens, fewer than vocab_size {cfg.vocab_size}")
    wpe = shapes.get(dec + "wpe.weight")
    if wpe is not None and "n_positions" not in cfg_json:
        cfg.n_positions = int(wpe[0])
    fc = shapes.get(dec + ("layers.0." if cfg.is_v2 else "h.0.") + "mlp.c_fc.weight")
    if fc is not None and "n_inner" not in cfg_json:
        cfg.n_inner = int(fc[0])
    elif "n_inner" not in cfg_json:
        cfg.n_inner = 4 * cfg.hidden_size
    return cfg


# --------------------------------------------------------------------------------------------------
# tokenizer used when the gated StarCoder tokenizer is not on disk
# --------------------------------------------------------------------------------------------------
class _Encoding(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def to(self, device):
        return _Encoding({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in self.items()})


class ByteTokenizer:
    """Deterministic byte-level stand-in with the tokenizer surface the path uses
    (llm/starcoder.py:40-53): eos id 0, ``[PAD]`` = vocab_size, then the three added tokens."""

    def __init__(self, vocab_size: int = 49152, v2: bool = False):
        self.vocab_size = vocab_size
        self.eos_token, self.eos_token_id = "<|endoftext|>", 0
        self.bos_token_id = 0
        self.pad_token, self.pad_token_id = "[PAD]", vocab_size
        self.added = {"<svg-start>": vocab_size + 1, "<image-start>": vocab_size + 2, "<caption-start>": vocab_size + 3}
        if v2:                                    # llm/starcoder2.py:47 adds <svg-end> too, pads on the left (:53)
            self.added["<svg-end>"] = vocab_size + 4
        self.padding_side = "left" if v2 else "right"

    def __len__(self):
        return self.vocab_size + 1 + len(self.added)

    def encode(self, text: str, add_special_tokens: bool = False) -> List[int]:
        if text in self.added:
            return [self.added[text]]
        return [1 + b for b in text.encode("utf-8")]

    def __call__(self, text, add_special_tokens: bool = False, return_tensors: Optional[str] = None, **kw):
        single = isinstance(text, str)
        rows = [self.encode(t) for t in ([text] if single else text)]
        if return_tensors is None:
            return _Encoding(input_ids=rows[0] if single else rows)
        n = max(len(r) for r in rows)
        ids = torch.full((len(rows), n), self.pad_token_id, dtype=torch.long)
        mask = torch.zeros((len(rows), n), dtype=torch.long)
        for i, r in enumerate(rows):
            if getattr(self, "padding_side", "right") == "left":      # llm/starcoder2.py:53
                ids[i, n - len(r):] = torch.tensor(r, dtype=torch.long)
                mask[i, n - len(r):] = 1
            else:
                ids[i, : len(r)] = torch.tensor(r, dtype=torch.long)
                mask[i, : len(r)] = 1
        return _Encoding(input_ids=ids, attention_mask=mask)

    def decode(self, ids, skip_special_tokens: bool = True) -> str:
        out = bytearray()
        for t in (ids.tolist() if torch.is_tensor(ids) else ids):
            if 1 <= t <= 256:
                out.append(t - 1)
            elif not skip_special_tokens:
                out.extend(f"<{t}>".encode())
        return out.decode("utf-8", "replace")

    def batch_decode(self, ids, skip_special_tokens: bool = True) -> List[str]:
        return [self.decode(r, skip_special_tokens) for r in ids]


# --------------------------------------------------------------------------------------------------
# image pre-processing (host side, PIL): data/util.py:40-68
# --------------------------------------------------------------------------------------------------
class ImageTrainProcessor:
    """starvector/data/util.py:40-68.  ``device=None`` (default): the reference's own host recipe with Pillow.
    ``device="cuda"``: the same arithmetic on the GPU (``sv_preprocess_image``: composite, pad, Pillow-exact bicubic
    resize, /255, normalise) -- the float32 tensor is bit-identical, it just never leaves the device."""

    def __init__(self, mean=None, std=None, size: int = 224, device=None, **kwargs):
        self._mean, self._std = tuple(mean or CLIP_MEAN), tuple(std or CLIP_STD)
        self.mean = torch.tensor(self._mean).view(3, 1, 1)
        self.std = torch.tensor(self._std).view(3, 1, 1)
        self.size = size
        self.device = device

    def _pixels(self, img):
        import numpy as np
        # engine-side processor: always the device kernels (palette / grey / CMYK images are only re-encoded as RGB(A)
        # first -- the reference itself cannot normalise a non-RGB image with its 3-channel mean)
        if img.mode not in ("RGB", "RGBA"):
            img = img.convert("RGBA" if "transparency" in img.info or img.mode in ("LA", "PA") else "RGB")
        return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).to(self.device, non_blocking=True)

    def batch(self, images) -> torch.Tensor:
        """A list of PIL images -> float32 [n, 3, size, size] in ONE device call (`sv_preprocess_images`): the serving path
        pre-processes a whole request batch with three launches instead of one synchronised round trip per image."""
        if self.device is None:
            return torch.stack([self(img) for img in images], 0)
        from .engine import op_preprocess_images
        return op_preprocess_images([self._pixels(img) for img in images], self.size, self._mean, self._std)

    def __call__(self, img):
        from PIL import Image
        import numpy as np
        if self.device is not None:
            from .engine import op_preprocess_image
            return op_preprocess_image(self._pixels(img), self.size, self._mean, self._std)
        if img.mode == "RGBA":                               # _rgba_to_rgb_white (data/util.py:64-67)
            bg = Image.new("RGB", img.size, (255, 255, 255))
            bg.paste(img, mask=img.split()[3])
            img = bg
        w, h = img.size                                      # _pad_to_square, white (data/util.py:56-62)
        m = max(w, h)
        if (w, h) != (m, m):
            canvas = Image.new(img.mode, (m, m), 255 if img.mode in ("L", "1") else (255,) * len(img.getbands()))
            canvas.paste(img, ((m - w) // 2, (m - h) // 2))
            img = canvas
        if img.size != (self.size, self.size):               # transforms.Resize(size, BICUBIC) on a PIL image
            img = img.resize((self.size, self.size), Image.BICUBIC)
        if img.mode != "RGB":
            img = img.convert("RGB")
        x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.0   # ToTensor
        x = (x - self.mean) / self.std
        return x if self.device is None else x.to(self.device)


class SimpleStarVectorProcessor:
    """starvector_arch.py:17-90: the HF-style processor a v1 checkpoint's `AutoProcessor` resolves to, reached as
    `starvector.model.processor` (starvector_v1.py:10; scripts/quickstart-hf.py and the validation dataset call it as
    `processor(image, return_tensors="pt")["pixel_values"]`).  Same pixels as ImageTrainProcessor except for RGBA input:
    here the alpha band is DROPPED (`img.convert("RGB")`, :41), not composited on white.  One image -> [3, S, S], a list ->
    [B, 3, S, S]; `text` goes through the tokenizer with the reference's arguments (:76-83).
    With `device` set the resize / normalise run on that GPU (`sv_preprocess_image`), bit-identical to the host recipe."""

    def __init__(self, tokenizer=None, size: int = 224, mean=None, std=None, device=None, **kwargs):
        self.tokenizer = tokenizer
        self.mean, self.std, self.size = tuple(mean or CLIP_MEAN), tuple(std or CLIP_STD), size
        self._pixels = ImageTrainProcessor(mean=self.mean, std=self.std, size=size, device=device)

    def _one(self, img):
        if img.mode == "RGBA":
            img = img.convert("RGB")
        return self._pixels(img)

    def __call__(self, images=None, text=None, max_length=None, **kwargs):
        if images is None and text is None:
            raise ValueError("You have to specify at least one of `images` or `text`.")
        data = {}
        if text is not None:
            data.update(self.tokenizer(text, truncation=True, add_special_tokens=True, padding="longest",
                                       max_length=max_length, return_tensors="pt"))
        if images is not None:
            data["pixel_values"] = (torch.stack([self._one(i) for i in images]) if isinstance(images, (list, tuple))
                                    else self._one(images))
        try:
            from transformers import BatchFeature
            return BatchFeature(data=data)
        except Exception:                                   # transformers not importable: same mapping + attribute access
            return _Encoding(**data)


# --------------------------------------------------------------------------------------------------
# modules
# --------------------------------------------------------------------------------------------------
class _EngineModule(nn.Module):
    """nn.Module shell so .eval()/.cuda()/.to() calls of existing callers keep working; holds no
    parameters (weights live repacked inside the engine)."""

    def __init__(self, engine: HipEngine):
        super().__init__()
        object.__setattr__(self, "_engine", engine)


class SiglipProcessor:
    """What `AutoProcessor.from_pretrained("google/siglip-large-patch16-384")` does to images (image_encoder.py:45-48):
    HF SiglipImageProcessor -- convert to RGB (alpha dropped), stretch to size x size with Pillow's BICUBIC resampler,
    rescale by 1/255, normalise with mean = std = 0.5.  Runs on the engine's GPU (`sv_preprocess_image`, recipe 1; bit
    identical to the HF PIL processor); call signature and return shape follow the HF processor."""

    class _Out:
        def __init__(self, pixel_values):
            self.pixel_values = pixel_values

        def __getitem__(self, k):
            return getattr(self, k)

    def __init__(self, size: int = 384, device=None, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        self.size, self.device, self.mean, self.std = size, device, tuple(mean), tuple(std)

    def __call__(self, images=None, return_tensors="pt", **kw):
        import numpy as np
        from .engine import op_preprocess_images
        if images is None:
            raise ValueError("images is required")
        imgs = images if isinstance(images, (list, tuple)) else [images]
        px = []
        for img in imgs:
            if img.mode not in ("RGB", "RGBA"):
                img = img.convert("RGB")
            px.append(torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).to(self.device, non_blocking=True))
        return SiglipProcessor._Out(op_preprocess_images(px, self.size, self.mean, self.std, recipe="siglip"))   # one call


class ImageEncoder(_EngineModule):
    """image_encoder.py:91-94 (clip branch): ln_vision(VisionTransformer(image)) -> [B,257,1024]; siglip branch
    (:108-109): the HF vision tower's last_hidden_state -> [B,576,1024]."""

    def __init__(self, engine: HipEngine, image_size: int = 224, image_encoder_type: str = "clip"):
        super().__init__(engine)
        self.image_encoder_type = image_encoder_type
        # the engine lives on a GPU, so the images are pre-processed there as well (bit-identical to the Pillow recipe)
        dev = torch.device("cuda", engine.device) if engine is not None and hasattr(engine, "device") else None
        if "siglip" in image_encoder_type:
            self.processor = SiglipProcessor(size=image_size, device=dev)
        else:
            self.processor = ImageTrainProcessor(size=image_size, device=dev)

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        return self._engine.encode_image(image)

    def process_images(self, images):                      # image_encoder.py:112-117
        if self.image_encoder_type == "clip":
            if hasattr(self.processor, "batch") and len(images) > 1:        # same list of [1, 3, S, S] tensors, one device call
                return list(self.processor.batch(list(images)).unsqueeze(1).unbind(0))
            return [self.processor(image).unsqueeze(0) for image in images]
        return self.processor(images=images, return_tensors="pt").pixel_values.unsqueeze(0)     # sic: [1, B, 3, S, S]


class Adapter(_EngineModule):
    """adapter.py:33-39: Linear -> Swish -> Linear -> LayerNorm([Q,D]) | BatchNorm1d(Q)."""

    def __init__(self, engine: HipEngine, query_length: int, adapter_norm: str):
        super().__init__(engine)
        self.query_length = query_length
        self.adapter_norm = adapter_norm

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        return self._engine.adapter(hidden_states)


class _TokenEmbedding(_EngineModule):
    def forward(self, input_ids: torch.Tensor) -> torch.Tensor:
        return self._engine.embed_tokens(input_ids)


class _Backbone(_EngineModule):
    """stand-in for GPTBigCodeModel / Starcoder2Model: exposes ``wte`` (starvector_v1.py:16-18) and
    ``embed_tokens`` (starvector_v2.py:45-47)."""

    def __init__(self, engine: HipEngine):
        super().__init__(engine)
        self.wte = _TokenEmbedding(engine)
        self.embed_tokens = self.wte


@dataclasses.dataclass(frozen=True)
class _GenRequest:
    """One `HipCausalLM.generate` call after its defaults are resolved and its refusals have passed: what the routes read instead of loose
    arguments.  A length group of a padded batch runs on a copy (`dataclasses.replace`) with its own lengths and stop."""
    # the sampling parameters, as the engine takes them
    do_sample: bool
    temperature: float
    top_p: float
    top_k: int
    repetition_penalty: float
    length_penalty: float
    num_beams: int
    early_stopping: object             # False | True | "never", handed on as given
    eos: int
    pad: int
    stopping_criteria: object          # resolved by `stop`, where the route first needs it: an unsupported criterion raises there, as before
    seed: int                          # at most one draw per public call: sub-calls and the exclusive job reuse it
    max_length: int
    min_length: int
    padded: bool                       # the mask has pads (read once)
    G: int                             # samples per prompt of the shared form (1: inputs_embeds holds one row per returned row)
    n_return: int                      # num_return_sequences as asked (repeated into the rows where the shared form is not taken)
    # what the call asked for
    return_dict: bool
    output_scores: bool
    output_logits: bool
    stats: object                      # False, True or the tuple of statistics names (output_token_logprobs, with return_dict)
    topk: Optional[dict]               # dict(k=, source=) of output_top_logprobs
    proc: dict                         # the keywords of HipEngine.generate_processed, {} when no processor is set
    lookup: Optional[tuple]            # (prompt_lookup_num_tokens, max_matching_ngram_size, prompt_lookup_sampling)
    streamer: object

    @property
    def want(self) -> bool:            # the [steps, rows, vocab] slabs (without return_dict HF ignores both arguments)
        return self.return_dict and bool(self.output_scores or self.output_logits)

    @functools.cached_property
    def stop(self) -> Optional[List[int]]:
        return HipCausalLM._stop_ids(self.stopping_criteria)

    def min_new(self, prompt_len: int) -> int:
        # HF (_prepare_generated_length): with inputs_embeds min_length is reduced by the prompt length -- 0 on the im2svg path
        # (SURVEY.md 8a-a11), positive only for a text2svg caption shorter than min_length; MinLengthLogitsProcessor then
        # keeps EOS at -inf for that many new tokens (in beam search HF applies it to the log-probabilities: so does the scorer).
        return max(self.min_length - prompt_len, 0)

    def engine_kw(self, min_new: int, on_tokens=None, sync_every: Optional[int] = None) -> dict:
        """The keywords of the engine's `generate` family.  `sync_every` (and with it `on_tokens`) goes down on the routes that stream;
        `min_new_tokens` only when non-zero."""
        kw = dict(do_sample=self.do_sample, temperature=self.temperature, top_p=self.top_p, eos_token_id=self.eos, pad_token_id=self.pad,
                  stop_ids=self.stop, seed=self.seed, repetition_penalty=self.repetition_penalty, num_beams=self.num_beams,
                  length_penalty=self.length_penalty, early_stopping=self.early_stopping, top_k=self.top_k)
        if sync_every is not None:
            kw.update(on_tokens=on_tokens, sync_every=sync_every)
        if min_new:
            kw["min_new_tokens"] = min_new
        return kw

    def cb_request(self, budget: int, min_new: int, row: int = 0) -> dict:
        """The request dict of `HipEngine.cb_admit` / `ContinuousBatcher.generate` for row `row` of the call: its own seed (the golden-ratio
        stride, the seeds of the length-group route: same tokens), and the stop sequence on row 0 alone (the reference's stop looks at row 0)."""
        return dict(max_new_tokens=budget, do_sample=self.do_sample, eos_token_id=self.eos, pad_token_id=self.pad, temperature=self.temperature,
                    top_p=self.top_p, top_k=self.top_k, repetition_penalty=self.repetition_penalty, min_new_tokens=min_new,
                    seed=(self.seed + 0x9E3779B97F4A7C15 * row) & (2 ** 63 - 1), stop_ids=self.stop if row == 0 else None)


# What is not built, per thing asked for: (asked, the condition it meets, exception, message), walked in this order by `_refuse`.
_NOT_BUILT = (
    ("attentions", "always", NotImplementedError, "output_attentions / output_hidden_states are not built: the decode step keeps neither"),
    ("slabs", "padded", NotImplementedError, "output_scores / output_logits with a padded attention_mask are not built: padded rows "
                                             "are generated group by group, without HF's common step axis"),
    ("stats", "beams", NotImplementedError, "output_token_logprobs with num_beams > 1 is not built: beam search reports sequences_scores, and "
                                            "beam rows reorder"),
    ("stats", "padded", NotImplementedError, "output_token_logprobs with a padded attention_mask is not built: padded rows run as "
                                             "continuous-batching slots, which keep no per-token statistics"),
    ("stats", "batcher", NotImplementedError, "output_token_logprobs with a batcher attached is not built: its requests run as "
                                              "continuous-batching slots, which keep no per-token statistics"),
    ("topk", "no_dict", ValueError, "output_top_logprobs needs return_dict_in_generate=True: the lists travel on the returned object"),
    ("topk", "beams", NotImplementedError, "output_top_logprobs with num_beams > 1 is not built: beam search reports sequences_scores, and "
                                           "beam rows reorder"),
    ("topk", "padded", NotImplementedError, "output_top_logprobs with a padded attention_mask is not built: padded rows run as "
                                            "continuous-batching slots, which keep no per-token lists"),
    ("topk", "batcher", NotImplementedError, "output_top_logprobs with a batcher attached is not built: its requests run as "
                                             "continuous-batching slots, which keep no per-token lists"),
    ("proc", "beams", NotImplementedError, "no_repeat_ngram_size / bad_words_ids / min_p with num_beams > 1 are not built: beam rows reorder "
                                           "their histories"),
    ("proc", "padded", NotImplementedError, "no_repeat_ngram_size / bad_words_ids / min_p with a padded attention_mask are not built: padded "
                                            "rows run as continuous-batching slots, whose requests carry no such processors"),
)


def _refuse(asked: str, cond: dict) -> None:
    for what, when, exc, message in _NOT_BUILT:
        if what == asked and cond[when]:
            raise exc(message)


class HipCausalLM(_EngineModule):
    """The object the reference reaches as ``svg_transformer.transformer``: ``.generate(**kwargs)`` with
    the keyword set built at starvector_base.py:228-241 (+ :289-295), ``.transformer.wte``."""

    def __init__(self, engine: HipEngine, eos_token_id: int, pad_token_id: int):
        super().__init__(engine)
        self.transformer = _Backbone(engine)          # GPTBigCodeForCausalLM.transformer
        self.model = self.transformer                 # Starcoder2ForCausalLM.model
        self.eos_token_id = eos_token_id
        self.pad_token_id = pad_token_id
        self.seed = None          # None: every sampling call draws its seed from torch's generator; an int pins it
        self.batcher = None       # a batching.ContinuousBatcher: concurrent single-sequence calls share one decode loop

    @staticmethod
    def _stop_ids(stopping_criteria) -> Optional[List[int]]:
        if not stopping_criteria:
            return None
        stops: List[List[int]] = []
        for crit in stopping_criteria:
            s = getattr(crit, "stops", None)
            if s is None:
                raise NotImplementedError(f"unsupported stopping criterion {type(crit).__name__}: the engine evaluates "
                                          "the reference's StoppingCriteriaSub (token-sequence stop) on device")
            stops.extend([list(map(int, x)) for x in s])
        if len(stops) > 1:
            raise NotImplementedError("one stop sequence is supported (the reference passes exactly one: '</svg>')")
        return stops[0] if stops else None

    def _shared_batcher(self):
        """The batcher this thread's engine work has to queue behind: None without one, and inside an exclusive job of it (the job has the
        engine to itself and talks to it directly)."""
        return None if _in_exclusive_job() else getattr(self, "batcher", None)

    @torch.no_grad()
    def generate(self, inputs_embeds: torch.Tensor = None, attention_mask: Optional[torch.Tensor] = None,
                 do_sample: bool = False, top_p: Optional[float] = 1.0, temperature: Optional[float] = 1.0,
                 num_beams: int = 1, max_length: int = 30, min_length: int = 0, repetition_penalty: float = 1.0,
                 length_penalty: float = 1.0, use_cache: bool = True, stopping_criteria=None,
                 early_stopping: bool = False, pad_token_id: Optional[int] = None, eos_token_id: Optional[int] = None,
                 num_return_sequences: int = 1, top_k: Optional[int] = 50, streamer=None, seed: Optional[int] = None,
                 return_dict_in_generate: bool = False, output_scores: bool = False, output_logits: bool = False,
                 share_prompt: bool = True, no_repeat_ngram_size: int = 0, bad_words_ids=None, min_p: Optional[float] = None,
                 output_token_logprobs: bool = False, output_top_logprobs: Optional[int] = None, top_logprobs_source: str = "raw",
                 prompt_lookup_num_tokens: Optional[int] = None, max_matching_ngram_size: Optional[int] = None,
                 prompt_lookup_sampling: bool = False, **unused):
        # Resolve the call into one `_GenRequest`, refuse what is not built (`_NOT_BUILT`), hand it to its route (`_route_*`).
        # use_cache is accepted and ignored: the engine always uses its paged KV cache, the results are identical.
        # top_k: the reference never passes it; its pinned transformers==4.49.0 (pyproject.toml:18) defaults
        # GenerationConfig.top_k to 50, so every do_sample call there is top-k 50 followed by top-p.  Same default here.
        if inputs_embeds is None:
            raise ValueError("inputs_embeds is required (the reference always generates from embeddings)")
        # prompt_lookup_sampling=True (an extension, opt-in): prompt_lookup_num_tokens may come with do_sample and / or a repetition penalty
        # (sv_generate_lookup_sampled: the tokens of the same call without drafts, per seed).  Alone it asks for nothing that could be done.
        if prompt_lookup_sampling and not prompt_lookup_num_tokens:
            raise ValueError("`prompt_lookup_sampling` needs `prompt_lookup_num_tokens`: it selects how drafted tokens are verified, and "
                             "without drafts there is nothing to verify")
        batcher = getattr(self, "batcher", None)
        padded = _is_padded(attention_mask)
        cond = dict(always=True, padded=padded, beams=int(num_beams) > 1, batcher=batcher is not None, no_dict=not return_dict_in_generate)
        # HF structured outputs (return_dict_in_generate): without it output_scores / output_logits are ignored, as HF ignores them
        if return_dict_in_generate and (unused.get("output_attentions") or unused.get("output_hidden_states")):
            _refuse("attentions", cond)
        if return_dict_in_generate and (output_scores or output_logits):
            _refuse("slabs", cond)
        # output_token_logprobs (an extension, not an HF argument; read with return_dict_in_generate like output_scores): the returned object
        # also carries token_logprobs, token_logprobs_processed and token_entropies [rows, n_new], computed inside the decode loop
        # (sv_generate_stats) -- no [steps, rows, vocab] slab.  Where that route is not built the call raises, it never drops the argument.
        # True: all three; a tuple of the field names: those alone (generate_im2svg_grpo leaves the processed log-prob out).
        stats = output_token_logprobs if return_dict_in_generate and output_token_logprobs else False
        if stats:
            _refuse("stats", cond)
        # output_top_logprobs = k (an extension, sv_generate_topk): the returned object also carries top_token_ids / top_logprobs [rows, n_new, k]
        # -- the k most likely ids of every step and their log-probs, best first -- and token_ranks [rows, n_new], under the distribution
        # top_logprobs_source names ("raw": that of token_logprobs, "processed": that of token_logprobs_processed).  It raises wherever
        # output_token_logprobs raises, and without return_dict_in_generate (there is no object to carry the fields): never dropped.
        topk = None
        if output_top_logprobs is not None and output_top_logprobs is not False:
            from .engine import token_topk_request
            token_topk_request(dict(k=output_top_logprobs, source=top_logprobs_source))      # ValueError: k outside 1..32, an unknown source
            _refuse("topk", cond)
            topk = dict(k=int(output_top_logprobs), source=top_logprobs_source)
        # HF's token-changing processors, on device (sv_generate_processed): NoRepeatNGram, NoBadWords, MinP.  Set = the call goes through
        # HipEngine.generate_processed; where that route is not built the call raises, it never drops the argument.
        proc = self._processor_args(no_repeat_ngram_size, bad_words_ids, min_p, do_sample, eos_token_id)
        if proc:
            _refuse("proc", cond)
        # Random stream: HF draws from torch's global generator, so repeated calls differ and torch.manual_seed controls them.
        # The device sampler is a pure function of (seed, step, row): the per-call seed is therefore DRAWN from torch's
        # generator (same reproducibility contract), unless the caller pins it with `seed=` (tests, data-parallel ranks).
        # The draw stands behind the refusals above (a call refused there leaves the generator alone) and in front of the range checks below.
        if seed is None:
            seed = self.seed
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, ()).item()) if do_sample else 0
        num_beams = int(num_beams)
        if num_beams < 1:
            raise ValueError("`num_beams` has to be an integer strictly greater than 0")     # HF's own check
        if num_beams > 8:
            raise NotImplementedError("num_beams > 8 is not built")
        num_return_sequences = int(num_return_sequences or 1)
        if num_return_sequences < 1:
            raise ValueError("`num_return_sequences` has to be at least 1")
        if num_return_sequences > 1 and num_beams > 1:
            # HF expands the inputs (repeat_interleave) and samples every copy independently; the reference forces
            # num_beams = 1 whenever it asks for several sequences (starvector_base.py:273-276)
            raise NotImplementedError("num_return_sequences > 1 with beam search is not built "
                                      "(the reference sets num_beams=1 on this path)")
        # Several samples of one prompt: where the engine offers the shared call, the un-repeated prompts go down and the engine runs ONE
        # prompt pass per prompt (sv_generate_shared; a padded batch: sv_cb_admit_shared) -- rows, tokens and random draws are those of the
        # repeated route, which stays for engines without it and for share_prompt=False (A/B, the equality tests).
        G = 1
        if num_return_sequences > 1:
            eng = self._engine
            if padded:
                can = (hasattr(eng, "cb_admit_shared") and inputs_embeds.shape[0] * num_return_sequences <= eng.cfg.max_batch
                       and self._shared_batcher() is None)
            else:
                can = hasattr(eng, "generate_shared")
            if share_prompt and can:
                G = num_return_sequences
            else:
                inputs_embeds = inputs_embeds.repeat_interleave(num_return_sequences, dim=0)
                attention_mask = None if attention_mask is None else attention_mask.repeat_interleave(num_return_sequences, dim=0)
        if repetition_penalty is not None and not repetition_penalty > 0:
            raise ValueError("`repetition_penalty` has to be a strictly positive float")   # HF's own check
        one = lambda v: float(v if v is not None else 1.0)                 # None is HF's "off" for these four
        request = _GenRequest(
            do_sample=bool(do_sample), temperature=one(temperature), top_p=one(top_p), top_k=int(top_k or 0),
            repetition_penalty=one(repetition_penalty), length_penalty=one(length_penalty), num_beams=num_beams, early_stopping=early_stopping,
            eos=int(self.eos_token_id if eos_token_id is None else eos_token_id),
            pad=int(self.pad_token_id if pad_token_id is None else pad_token_id), stopping_criteria=stopping_criteria,
            seed=int(seed) & (2 ** 63 - 1), max_length=int(max_length), min_length=int(min_length or 0), padded=padded, G=G,
            n_return=num_return_sequences, return_dict=bool(return_dict_in_generate), output_scores=output_scores, output_logits=output_logits,
            stats=stats, topk=topk, proc=proc, streamer=streamer,
            lookup=(prompt_lookup_num_tokens, max_matching_ngram_size, bool(prompt_lookup_sampling)) if prompt_lookup_num_tokens else None)
        if request.lookup is not None:
            return self._route_lookup(request, inputs_embeds)
        if padded:
            seqs = self._route_padded(request, inputs_embeds, attention_mask)
            return generate_output(num_beams > 1, sequences=seqs) if return_dict_in_generate else seqs
        return self._route_unpadded(request, inputs_embeds)

    # ---- the routes: each takes the request and the embeddings ---------------------------------------------------------------------------------
    @staticmethod
    def _streaming(streamer, rows):
        # HF streamer protocol (generation/streamers.py): put(prompt ids) once -- none with inputs_embeds --, put(next_tokens [rows]) per
        # step, end().  Returns the engine callback; tokens arrive in bursts of `sync_every` steps: the decode loop does not return to the
        # host every token.
        streamer.put(torch.empty(rows, 0, dtype=torch.long))

        def on_tokens(tokens, first_col):
            for c in range(tokens.shape[1]):
                streamer.put(tokens[:, c])
        return on_tokens

    def _route_unpadded(self, r: _GenRequest, inputs_embeds):
        """An all-real prompt batch: the classic engine call, or -- while a batcher shares the engine with other requests -- a request of
        its decode loop (one row, nothing beyond tokens asked) or an exclusive job around the classic call (everything else)."""
        rows, on_tokens = inputs_embeds.shape[0] * r.G, None
        if r.streamer is not None:
            if r.num_beams > 1:
                raise ValueError("`streamer` cannot be used with beam search")          # HF's own check
            on_tokens = self._streaming(r.streamer, rows)
        batcher = self._shared_batcher()
        if batcher is None:
            out = self._route_classic(r, inputs_embeds, on_tokens)
        elif r.want or r.proc or r.num_beams > 1 or rows > 1:
            # beam search / a multi-row HF batch while requests share the engine: run it with the engine to itself, in turn
            out = _exclusive(batcher, lambda: self._route_classic(r, inputs_embeds, on_tokens))
        else:
            out = self._route_batcher_single(r, inputs_embeds, on_tokens)
        if r.streamer is not None:
            r.streamer.end()
        return out

    def _route_batcher_single(self, r: _GenRequest, inputs_embeds, on_tokens):
        # serving: one request per call (serve/model_worker.py:120-181), many calls in flight -> they share the engine's decode loop
        # instead of taking turns; the tokens are those of the solo call
        S0 = inputs_embeds.shape[1]
        on_chunk = None if on_tokens is None else (lambda toks, first: on_tokens(toks.view(1, -1), first))
        out = self.batcher.generate(inputs_embeds.to(torch.bfloat16), r.cb_request(r.max_length - S0, r.min_new(S0)), on_chunk)
        out = out.to(inputs_embeds.device)
        return generate_output(False, sequences=out) if r.return_dict else out

    def _route_classic(self, r: _GenRequest, inputs_embeds, on_tokens):
        """HipEngine.generate, generate_shared (G samples per prompt from one prompt pass) or generate_processed (no_repeat_ngram_size /
        bad_words_ids / min_p; rectangular and shared prompts alike), and HF's output object around what it returns."""
        eng, beams = self._engine, r.num_beams > 1
        extra, slabs = {}, {}
        if r.return_dict and (r.want or beams or r.stats or r.topk):
            extra, slabs = self._output_slabs(r, inputs_embeds)
            if r.stats:     # (these keywords go down only when asked for: an engine without them is never handed them)
                extra["token_stats"] = True if r.stats is True else tuple(r.stats)
            if r.topk:
                extra["token_topk"] = r.topk
        with _call_lock(eng):          # the same lock the slot path holds: a classic generate never lands between its cb_reset / cb_admit
            call = eng.generate if r.G == 1 else functools.partial(eng.generate_shared, n_samples=r.G)
            if r.proc:
                call = functools.partial(eng.generate_processed, n_samples=r.G, **r.proc)
            kw = r.engine_kw(r.min_new(inputs_embeds.shape[1]), on_tokens, sync_every=8 if r.streamer is not None else 32)
            out = call(inputs_embeds.to(torch.bfloat16), max_length=r.max_length, **kw, **extra)
        if not r.return_dict:
            return out
        if not extra:
            return generate_output(False, sequences=out)
        L = int(out["n_generated"])
        fields = dict(sequences=out["sequences"],
                      scores=tuple(slabs["scores_out"][t] for t in range(L)) if "scores_out" in slabs else None,
                      logits=tuple(slabs["logits_out"][t] for t in range(L)) if "logits_out" in slabs else None)
        if beams:
            dev = out["sequences"].device
            fields["beam_indices"] = out["beam_indices"].to(dev)
            fields["sequences_scores"] = out["sequences_scores"].to(dev) if r.output_scores else None
        if not r.stats and not r.topk:
            return generate_output(beams, **fields)
        # the extension's three fields beside HF's: HF's output dataclass has no place for them, so the object is the stand-in with the same
        # field names, read as attributes or as keys
        res = _GenerateOutput({k: fields.get(k) for k in _DECODER_ONLY_FIELDS})
        if r.stats:
            res.update({k: out.get(k) for k in ("token_logprobs", "token_logprobs_processed", "token_entropies")})
        if r.topk:
            res.update({k: out.get(k) for k in ("top_token_ids", "top_logprobs", "token_ranks")})
        return res

    def _route_lookup(self, r: _GenRequest, inputs_embeds):
        # HF's prompt lookup decoding (prompt_lookup_num_tokens = K, max_matching_ngram_size): greedy generate that verifies K drafted tokens
        # per step (sv_generate_lookup) -- the tokens are those of the call without it.  With prompt_lookup_sampling the call's own selection
        # verifies the drafts (sv_generate_lookup_sampled: sampling, a repetition penalty).  What the engine does not build raises, naming it.
        num_tokens, ngram, sampled = r.lookup
        K = int(num_tokens)
        if K < 1:
            raise ValueError(f"`prompt_lookup_num_tokens` has to be a positive integer, but is {num_tokens}")
        refused = [name for name, on in (
            ("do_sample", not sampled and r.do_sample), ("num_beams > 1", r.num_beams > 1),
            ("repetition_penalty != 1", not sampled and r.repetition_penalty != 1.0),
            ("no_repeat_ngram_size / bad_words_ids / min_p", bool(r.proc)), ("output_scores / output_logits", r.want),
            ("output_token_logprobs", bool(r.stats)), ("output_top_logprobs", bool(r.topk)),
            ("num_return_sequences > 1", r.n_return > 1), ("a padded attention_mask", r.padded),
            ("a batcher (continuous batching does not draft)", self._shared_batcher() is not None),
            ("a streamer with more than one row", r.streamer is not None and inputs_embeds.shape[0] > 1)) if on]
        if refused and sampled:
            raise NotImplementedError("prompt_lookup_num_tokens with " + ", ".join(refused) + " is not built: verification of drafted tokens "
                                      "(sv_generate_lookup_sampled) takes one sample per prompt, without beams, processors or per-step outputs")
        if refused:
            raise NotImplementedError("prompt_lookup_num_tokens with " + ", ".join(refused) + " is not built: greedy verification of drafted "
                                      "tokens (sv_generate_lookup) takes greedy calls without per-step outputs")
        eng, name = self._engine, "generate_lookup_sampled" if sampled else "generate_lookup"
        if not hasattr(eng, name):
            raise NotImplementedError("prompt_lookup_num_tokens: this engine has no " + name)
        on_tokens = self._streaming(r.streamer, inputs_embeds.shape[0]) if r.streamer is not None else None
        # greedy verification takes the ids, the stop and the hold; the sampled one also the selection of the plain call: the tokens must be that call's
        names = ("eos_token_id", "pad_token_id", "stop_ids", "min_new_tokens")
        if sampled:
            names += ("do_sample", "temperature", "top_p", "top_k", "seed", "repetition_penalty")
        with _call_lock(eng):
            kw = r.engine_kw(r.min_new(inputs_embeds.shape[1]))
            out = getattr(eng, name)(inputs_embeds.to(torch.bfloat16), max_length=r.max_length, num_draft_tokens=K, max_ngram=int(ngram or 0),
                                     on_tokens=on_tokens, **{k: v for k, v in kw.items() if k in names})
        if r.streamer is not None:
            r.streamer.end()
        return generate_output(False, sequences=out) if r.return_dict else out

    def _route_padded(self, r: _GenRequest, inputs_embeds, attention_mask):
        # Padded prompts (text2svg with captions of different lengths; the v2 tokenizer pads on the left, llm/starcoder2.py:53).
        # HF masks the padded keys and numbers positions by cumsum(mask), so a padded row behaves exactly like the same row
        # with its padding removed (checked against HF for left and right padding, GPTBigCode and StarCoder2).  Rows run as slots of one
        # decode loop or as one ragged beam search where the engine offers them; else the engine takes rectangular all-ones prompts, so rows
        # are grouped by their real length and generated group by group.  The streamer is never called here.
        mask = attention_mask.to(torch.bool)
        if r.G > 1:                    # the shared form: inputs_embeds holds the un-repeated prompts, row b samples prompt b // G
            mask = mask.repeat_interleave(r.G, dim=0)
        B, S = mask.shape[0], inputs_embeds.shape[1]
        eng = self._engine
        if not bool(mask[:, -1].all()):
            # right padding: only the ragged route takes it (every row runs with its padding removed, wherever the padding sits); the
            # rectangular length-group route continues from the last position and needs a real token there
            if not hasattr(eng, "prefill_ragged"):
                raise ValueError("the last prompt position of every row must be a real token (generation continues from it)")
            if not bool(mask.any(dim=1).all()):
                raise ValueError("every row needs at least one real prompt position")
        budget = r.max_length - S                                  # HF counts the budget from the PADDED prompt length
        if budget <= 0:
            raise ValueError(f"max_length ({r.max_length}) must exceed the prompt length ({S})")
        lengths = mask.sum(dim=1).tolist()
        r.stop                                                     # (an unsupported criterion raises here, in front of every engine call)
        if r.G > 1 or (r.num_beams == 1 and hasattr(eng, "cb_admit") and B <= eng.cfg.max_batch and self._shared_batcher() is None):
            return self._route_slots(r, inputs_embeds, mask, lengths, budget)
        if r.num_beams > 1 and hasattr(eng, "generate_ragged") and B * r.num_beams <= eng.cfg.max_batch:
            return self._route_beams(r, inputs_embeds, mask, lengths, budget)
        return self._route_groups(r, inputs_embeds, mask, lengths, budget)

    @staticmethod
    def _hf_padded(outs, length, pad, device):
        """HF's padded batch from the rows' own token streams: cut at `length` (the step at which row 0's stop ended every row; None:
        the longest row), finished rows padded."""
        L = length if length is not None else max(t.shape[0] for t in outs)
        res = torch.full((len(outs), L), pad, dtype=torch.long, device=device)
        for b, t in enumerate(outs):
            k = min(L, t.shape[0])
            res[b, :k] = t[:k].to(device)
        return res

    def _route_groups(self, r: _GenRequest, inputs_embeds, mask, lengths, budget):
        """One unpadded call per group of rows of equal real length, routed as a public unpadded call is (a batcher included)."""
        B, S = mask.shape[0], inputs_embeds.shape[1]
        outs, fired_at, stop = [None] * B, None, r.stop
        for n in sorted(set(lengths)):
            rows = [b for b in range(B) if lengths[b] == n]
            emb = torch.stack([inputs_embeds[b][mask[b]] for b in rows], 0)
            # HF subtracts the PADDED prompt length from min_length as well: the same number of EOS-free steps for every row.
            # The reference's stop looks at row 0 of the batch only: the other groups run without it.
            sub = dataclasses.replace(r, max_length=n + budget, min_length=n + r.min_new(S), padded=False, return_dict=False, streamer=None,
                                      stopping_criteria=r.stopping_criteria if rows[0] == 0 else None)
            toks = self._route_unpadded(sub, emb)
            if rows[0] == 0 and stop and toks.shape[1] >= len(stop) and toks[0, -len(stop):].tolist() == list(stop):
                fired_at = toks.shape[1]                           # row 0 ended the whole batch at this step
            for i, b in enumerate(rows):
                outs[b] = toks[i]
        return self._hf_padded(outs, fired_at, r.pad, inputs_embeds.device)

    def _route_beams(self, r: _GenRequest, inputs_embeds, mask, lengths, budget):
        """Beam search / beam-sample over a padded batch as ONE ragged engine call (sv_generate_ragged): one prompt pass over the rows
        with their padding removed and one search for all requests, instead of a complete serial generate call per length group.  The
        engine follows HF's padded-batch semantics itself: the budget counts from the longest prompt (so max_length = longest + the budget
        HF derives from the padded length), the row-0 stop ends every request, finished hypotheses are padded.  No streaming keywords."""
        eng = self._engine
        seqs = [inputs_embeds[b][mask[b]].to(torch.bfloat16).contiguous() for b in range(inputs_embeds.shape[0])]
        kw = dict(r.engine_kw(r.min_new(inputs_embeds.shape[1])), early_stopping=r.early_stopping or False)

        def call():
            with _call_lock(eng):
                return eng.generate_ragged(seqs, max_length=max(lengths) + budget, **kw)
        batcher = self._shared_batcher()       # requests share the engine: the search runs with the engine to itself, in turn
        return (call() if batcher is None else _exclusive(batcher, call)).to(inputs_embeds.device)

    def _route_slots(self, r: _GenRequest, inputs_embeds, mask, lengths, budget):
        """Rows of different real length in ONE decode loop: every row is a slot of the engine's continuous batch (own prompt
        length, positions and KV pages), the prompt pass is ONE ragged pass over all rows where the engine offers it
        (`prefill_ragged`; else prompt passes run per length group: they are rectangular), and all rows then decode
        together -- instead of one full generate call per length group.  HF semantics of the padded batch are restored on
        the host: the reference's row-0 stop ends every row at row 0's step, finished rows are padded."""
        eng = self._engine
        reqs = [r.cb_request(budget, r.min_new(inputs_embeds.shape[1]), row=b) for b in range(mask.shape[0])]
        with _call_lock(eng):  # from the first cb_reset to the last: another thread's generate must not reset or admit in between
            outs, fired_len = self._run_slots(eng, inputs_embeds, mask, lengths, reqs, r.stop, r.G)
        return self._hf_padded(outs, fired_len, r.pad, inputs_embeds.device)

    @staticmethod
    def _run_slots(eng, inputs_embeds, mask, lengths, reqs, stop, G=1):
        B = mask.shape[0]
        row = lambda b: inputs_embeds[b // G][mask[b]].to(torch.bfloat16).contiguous()
        eng.cb_reset()
        try:
            if G > 1:
                # the shared form: one ragged prompt pass over the B / G prompts, row b is a request of prompt b // G with the seed row b
                # has on the repeated route (sv_cb_admit_shared): same tokens
                slot_of = list(eng.cb_admit_shared([row(b) for b in range(0, B, G)], None, [b // G for b in range(B)], reqs))
            elif hasattr(eng, "prefill_ragged"):
                slot_of = list(eng.cb_admit([row(b) for b in range(B)], reqs))      # one ragged prompt pass for all rows
            else:
                slot_of = [None] * B
                for n in sorted(set(lengths)):
                    rows = [b for b in range(B) if lengths[b] == n]
                    emb = torch.stack([inputs_embeds[b][mask[b]] for b in rows], 0).to(torch.bfloat16).contiguous()
                    for b, s_ in zip(rows, eng.cb_admit(emb, [reqs[b] for b in rows])):
                        slot_of[b] = s_
            fired_len = None
            while True:
                live = eng.cb_step(16)
                lv, st = eng.cb_poll()
                if stop and not lv[slot_of[0]]:
                    r0 = eng.cb_read(slot_of[0], 0, st[slot_of[0]]).tolist()
                    if len(r0) >= len(stop) and r0[-len(stop):] == list(stop):
                        fired_len = len(r0)            # row 0 ended the whole batch at this step (starvector_base.py:9-20)
                        break
                if live == 0:
                    break
            lv, st = eng.cb_poll()
            outs = [eng.cb_read(slot_of[b], 0, st[slot_of[b]]) for b in range(B)]
        finally:
            eng.cb_reset()
        return outs, fired_len

    def _processor_args(self, no_repeat_ngram_size, bad_words_ids, min_p, do_sample, eos_token_id):
        """HF's own checks of no_repeat_ngram_size / bad_words_ids / min_p (generation/logits_process.py, transformers 4.49), then the
        engine's limits; returns the keywords of HipEngine.generate_processed, {} when none of the three is set."""
        n = no_repeat_ngram_size
        if n is None:
            n = 0
        if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 0:
            raise ValueError(f"`no_repeat_ngram_size` has to be an integer >= 0, but is {no_repeat_ngram_size}")
        words = None
        if bad_words_ids is not None:
            if not isinstance(bad_words_ids, (list, tuple)) or len(bad_words_ids) == 0:
                raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids}.")
            if any(not isinstance(w, (list, tuple)) or len(w) == 0 for w in bad_words_ids):
                raise ValueError(f"`bad_words_ids` has to be a list of non-empty lists, but is {bad_words_ids}.")
            if any(isinstance(t, bool) or not isinstance(t, numbers.Integral) or t < 0 for w in bad_words_ids for t in w):
                raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad_words_ids}.")
            # HF drops a bad word that is exactly [eos_token_id] (NoBadWordsLogitsProcessor.__init__)
            eos = int(self.eos_token_id if eos_token_id is None else eos_token_id)
            words = [[int(t) for t in w] for w in bad_words_ids if [int(t) for t in w] != [eos]]
        if min_p is not None:
            min_p = float(min_p)
            if not 0.0 <= min_p <= 1.0:
                raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
            if not do_sample:
                min_p = None                    # a warper: HF builds it for sampling calls only
        if n == 0 and words is None and min_p is None:
            return {}
        from .engine import logits_processors
        vocab = getattr(getattr(self._engine, "cfg", None), "vocab", None)
        logits_processors(n, words, min_p or 0.0, vocab=vocab)          # the limits: ValueError here, before any engine call
        return dict(no_repeat_ngram_size=int(n), bad_words_ids=words or None, min_p=float(min_p or 0.0))

    def _output_slabs(self, r: _GenRequest, inputs_embeds):
        """[max_new, rows, V] fp32 slabs for output_scores / output_logits on the engine's device, after checking they fit (the engine
        writes step t of every row into slab[t])."""
        eng = self._engine
        B, S0 = inputs_embeds.shape[0], inputs_embeds.shape[1]
        rows, max_new, V = B * r.num_beams * r.G, r.max_length - S0, int(eng.cfg.vocab)
        names = [n for n, on in (("scores_out", r.output_scores), ("logits_out", r.output_logits)) if on]
        extra = dict(return_outputs=True)
        if not names or max_new <= 0:
            return extra, {}
        need = len(names) * max_new * rows * V * 4
        free_fn = getattr(eng, "mem_free_bytes", None)
        free = free_fn() if free_fn is not None else None
        if free is not None and need > free:
            raise MemoryError(f"output_scores / output_logits need {need / 1e9:.2f} GB ({len(names)} x {max_new} steps x {rows} rows x "
                              f"{V} fp32) on the GPU, {free / 1e9:.2f} GB are free: lower max_length or the batch")
        dev = getattr(eng, "_dev", None) or inputs_embeds.device
        slabs = {n: torch.empty(max_new, rows, V, dtype=torch.float32, device=dev) for n in names}
        extra.update(slabs)
        return extra, slabs

    def compute_transition_scores(self, sequences: torch.Tensor, scores, beam_indices: Optional[torch.Tensor] = None,
                                  normalize_logits: bool = False) -> torch.Tensor:
        """HF GenerationMixin.compute_transition_scores (generation/utils.py) with the engine's vocabulary size: the score of each
        generated token at its step ([batch, steps]; beam search: along the returned hypothesis, 0 after its end)."""
        V = int(self._engine.cfg.vocab)
        if beam_indices is None:
            beam_indices = torch.arange(scores[0].shape[0]).view(-1, 1).to(sequences.device)
            beam_indices = beam_indices.expand(-1, len(scores))
        stacked = torch.stack(scores).reshape(len(scores), -1).transpose(0, 1)
        if normalize_logits:
            stacked = stacked.reshape(-1, V, stacked.shape[-1])
            stacked = torch.nn.functional.log_softmax(stacked, dim=1)
            stacked = stacked.reshape(-1, stacked.shape[-1])
        mask = beam_indices < 0
        max_beam_length = (1 - mask.long()).sum(-1).max()
        beam_indices = beam_indices.clone()[:, :max_beam_length]
        mask = mask[:, :max_beam_length]
        beam_indices[mask] = 0
        cut = sequences.shape[-1] - max_beam_length
        indices = sequences[:, cut:] + beam_indices * V
        out = stacked.gather(0, indices)
        out[mask] = 0
        return out


def completion_mask(new_tokens: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """[rows, n_new] int64: 1 up to and including the token that ended the row -- its first EOS; the last column for a row that ran to the end
    of the call (the budget, or the stop sequence on row 0, which ends every row at that column) -- and 0 on the pads behind an EOS."""
    n = new_tokens.shape[1]
    cols = torch.arange(n, device=new_tokens.device).unsqueeze(0)
    is_eos = new_tokens == int(eos_token_id)
    first = torch.where(is_eos.any(dim=1), is_eos.int().argmax(dim=1), torch.full_like(new_tokens[:, 0], n - 1).to(torch.int64))
    return (cols <= first.unsqueeze(1)).to(torch.int64)


class StoppingCriteriaSub:
    """starvector_base.py:9-20: stop the whole batch when ROW 0 ends with one of ``stops``.
    Carried to the device by HipCausalLM.generate (no per-step host sync)."""

    def __init__(self, stops=()):
        self.stops = [list(s) for s in stops]

    def __call__(self, input_ids, scores=None, **kw):
        return any(input_ids[0][-len(s):].tolist() == s for s in self.stops)


class StarCoderModel(nn.Module):
    """llm/starcoder.py:9-53: tokenizer + causal LM + the '<svg' prompt."""

    def __init__(self, engine: HipEngine, tokenizer, max_length: int, v2: bool = False):
        super().__init__()
        self.tokenizer = tokenizer
        self.max_length = max_length
        # v1 passes pad_token_id=[PAD] explicitly (starvector_base.py:289-295); v2 passes nothing
        # (starvector_v2.py:53-57), so HF falls back to pad_token_id = eos_token_id
        self.transformer = HipCausalLM(engine, tokenizer.eos_token_id,
                                       tokenizer.eos_token_id if v2 else tokenizer.pad_token_id)
        self.prompt = "<svg"
        self.svg_start_token = "<svg-start>"
        self.image_start_token = "<image-start>"
        self.text_start_token = "<caption-start>"
        self.svg_start_token_id = tokenizer.encode(self.svg_start_token)[0]
        if v2:
            self.svg_end_token = "<svg-end>"
            self.svg_end_token_id = tokenizer.encode(self.svg_end_token)[0]


class StarVectorStarCoder(nn.Module):
    """StarVectorBase + v1 binding (starvector_base.py:22-48,203-295; starvector_v1.py)."""

    def __init__(self, config: StarVectorConfig, engine: HipEngine, tokenizer, v2: bool = False):
        super().__init__()
        self.task = "im2svg"
        self.model_precision = torch.bfloat16
        ec = engine.cfg
        self.svg_transformer = StarCoderModel(engine, tokenizer, config.max_length, v2=v2)
        self.image_encoder = ImageEncoder(engine, ec.image_size, config.image_encoder_type)
        self.query_length = ec.query_length                          # starvector_base.py:85-106
        self.image_projection = Adapter(engine, self.query_length, ec.adapter_norm)
        self.max_length = config.max_length_train - self.query_length - 4
        # starvector_v1.py:10 -> AutoProcessor = SimpleStarVectorProcessor (HF-style call); starvector_v2.py:12 -> the tower's
        # image processor.  `image_encoder.processor` stays the plain callable `process_images` uses (image_encoder.py:112-117)
        self.processor = self.image_encoder.processor if v2 else SimpleStarVectorProcessor(
            tokenizer, size=ec.image_size, device=getattr(self.image_encoder.processor, "device", None))

    def use_image_encoder(self):
        return True

    def _get_embeddings(self, input_ids):                             # starvector_v1.py:16-18
        return self.svg_transformer.transformer.transformer.wte(input_ids)

    def _tokenize(self, text, max_length, device, add_special_tokens=True):
        tokens = self.svg_transformer.tokenizer(text, add_special_tokens=add_special_tokens, padding="longest",
                                                return_tensors="pt")
        return tokens.to(device)

    def _prepare_generation_inputs(self, batch, prompt, device):      # starvector_base.py:203-221
        image = batch["image"].to(device).to(self.model_precision)
        if image.dim() == 3:                  # one un-batched image, what `processor(pil)["pixel_values"]` returns for v1
            image = image.unsqueeze(0)
        if prompt is None:
            prompt = self.svg_transformer.prompt
        prompt_tokens = self._tokenize([prompt] * image.size(0), None, device, add_special_tokens=False)
        # image_projection(image_encoder(image)) and _get_embeddings(prompt ids), written straight into ONE inputs_embeds buffer instead of
        # two tensors + torch.cat (same values: tests/test_gpu_e2e.py; the separate module calls stay available and equal)
        enc = self.image_encoder(image)
        ids = prompt_tokens.input_ids.to(device)
        prep = getattr(getattr(self.image_projection, "_engine", None), "prepare_inputs", None)
        if prep is not None and not bool((prompt_tokens.attention_mask == 0).any()):
            inputs_embeds = prep(enc, ids)
        else:
            inputs_embeds = torch.cat([self.image_projection(enc), self._get_embeddings(ids)], dim=1)
        embedded_att = torch.ones(inputs_embeds.shape[0], inputs_embeds.shape[1] - ids.shape[1], dtype=torch.long, device=device)
        attention_mask = torch.cat([embedded_att, prompt_tokens.attention_mask], dim=1)
        return inputs_embeds, attention_mask, prompt_tokens

    def _get_generation_kwargs(self, base_kwargs):                    # starvector_base.py:223-241
        end_sequence = self.svg_transformer.tokenizer("</svg>", add_special_tokens=False)["input_ids"]
        # extension, opt-in (HipCausalLM.generate): prompt_lookup_num_tokens together with sampling / a repetition penalty
        lookup_sampling = {"prompt_lookup_sampling": True} if base_kwargs.get("prompt_lookup_sampling") else {}
        return {
            **lookup_sampling,
            "inputs_embeds": base_kwargs["inputs_embeds"],
            "attention_mask": base_kwargs["attention_mask"],
            "do_sample": base_kwargs.get("use_nucleus_sampling", True),
            "top_p": base_kwargs.get("top_p", 0.9),
            "temperature": base_kwargs.get("temperature", 1),
            "num_beams": base_kwargs.get("num_beams", 2),
            "max_length": base_kwargs.get("max_length", 30),
            "min_length": base_kwargs.get("min_length", 1),
            "repetition_penalty": base_kwargs.get("repetition_penalty", 1.0),
            "length_penalty": base_kwargs.get("length_penalty", 1.0),
            "use_cache": base_kwargs.get("use_cache", True),
            "stopping_criteria": [StoppingCriteriaSub(stops=[end_sequence])],
            # not in the reference's whitelist (so its serve worker's streamer never streams, serve/model_worker.py:129-175);
            # kept here so that the same call does stream
            "streamer": base_kwargs.get("streamer"),
            # extension: pins the device sampler's random stream (default: drawn per call from torch's generator, so that
            # `torch.manual_seed` reproduces a run and repeated calls differ, as with HF's torch.multinomial)
            "seed": base_kwargs.get("seed"),
            # HF's prompt lookup decoding, off unless asked for (HipCausalLM.generate)
            "prompt_lookup_num_tokens": base_kwargs.get("prompt_lookup_num_tokens"),
            "max_matching_ngram_size": base_kwargs.get("max_matching_ngram_size"),
        }

    def _get_im2svg_specific_kwargs(self, kwargs):                    # starvector_base.py:289-295
        return {"early_stopping": True, "pad_token_id": self.svg_transformer.tokenizer.pad_token_id}

    def _get_text2svg_specific_kwargs(self, kwargs):                  # starvector_base.py:332-339
        return {"eos_token_id": self.svg_transformer.tokenizer.eos_token_id, "early_stopping": True,
                "length_penalty": kwargs.get("length_penalty", 1.0)}

    def generate_text2svg(self, batch, **kwargs):
        """starvector_base.py:297-330, restated by intent: embed(caption ids + <svg-start>) -> generate -> new token ids.
        The snapshot's version cannot run (it passes two positional arguments to _get_generation_kwargs, :321-324, and
        subtracts the prompt length from max_length twice); here `max_length` counts the prompt once, as in im2svg.
        Captions of different lengths are padded by the tokenizer; the padded rows run without their pads
        (HipCausalLM._route_padded), which reproduces HF's masked generation exactly."""
        device = batch["image"].device if "image" in batch else torch.device("cuda", self._engine_device())
        prompt_tokens = self._tokenize(list(batch["caption"]), kwargs.get("max_length", 30), device, add_special_tokens=False)
        trigger = self._tokenize([self.svg_transformer.svg_start_token] * len(batch["caption"]), None, device,
                                 add_special_tokens=False)
        input_tokens = torch.cat([prompt_tokens.input_ids, trigger.input_ids], dim=1)
        attention_mask = torch.cat([prompt_tokens.attention_mask, trigger.attention_mask], dim=1)
        inputs_embeds = self._get_embeddings(input_tokens)
        generation_kwargs = self._get_generation_kwargs({**kwargs, "inputs_embeds": inputs_embeds,
                                                         "attention_mask": attention_mask})
        generation_kwargs.update(self._get_text2svg_specific_kwargs(kwargs))
        return self.svg_transformer.transformer.generate(**generation_kwargs)

    def _engine_device(self):
        return self.svg_transformer.transformer._engine.device

    def generate_im2svg(self, batch, **kwargs):                       # starvector_base.py:243-259
        return self.generate_im2svg_grpo(batch, **kwargs)["raw_svg"]

    def generate_im2svg_grpo(self, batch, **kwargs):                  # starvector_base.py:261-286
        device = batch["image"].device
        inputs_embeds, attention_mask, prompt_tokens = self._prepare_generation_inputs(batch, kwargs.get("prompt"), device)
        generation_kwargs = self._get_generation_kwargs({**kwargs, "inputs_embeds": inputs_embeds,
                                                         "attention_mask": attention_mask})
        generation_kwargs.update(self._get_im2svg_specific_kwargs(kwargs))
        num_return_sequences = kwargs.get("num_return_sequences", 1)
        if num_return_sequences > 1:                                   # :273-276
            generation_kwargs["num_return_sequences"] = num_return_sequences
            generation_kwargs["num_beams"] = 1
            if "share_prompt" in kwargs:                               # extension: False = the repeated prompts (A/B)
                generation_kwargs["share_prompt"] = kwargs["share_prompt"]
        top_k = kwargs.get("return_top_logprobs")
        if not kwargs.get("return_logprobs") and not top_k:
            outputs = self.svg_transformer.transformer.generate(**generation_kwargs)
            outputs = torch.cat([prompt_tokens.input_ids.repeat(num_return_sequences, 1), outputs], dim=1)    # :279
            raw_svg = self.svg_transformer.tokenizer.batch_decode(outputs, skip_special_tokens=True)
            return {"raw_svg": raw_svg, "outputs": outputs, "inputs_embeds": inputs_embeds}
        # extension (return_logprobs=True): the roll-out policy's own per-token log-probs and entropies from the decode loop (GRPO's old
        # log-probs: log_softmax(logits / temperature) at every sampled token, what completion_logprobs returns for the same weights), and the
        # mask of the columns that belong to each completion
        # return_top_logprobs=k: the k most likely ids of every step, their log-probs and the sampled token's rank under the same distribution
        # (on-policy distillation targets); alone or beside return_logprobs
        ask = {}
        if kwargs.get("return_logprobs"):
            ask["output_token_logprobs"] = ("token_logprobs", "token_entropies")
        if top_k:
            ask.update(output_top_logprobs=top_k, top_logprobs_source=kwargs.get("top_logprobs_source", "raw"))
        gen = self.svg_transformer.transformer.generate(**generation_kwargs, return_dict_in_generate=True, **ask)
        new = gen["sequences"]
        lm = self.svg_transformer.transformer
        eos = generation_kwargs.get("eos_token_id")
        outputs = torch.cat([prompt_tokens.input_ids.repeat(num_return_sequences, 1), new], dim=1)    # :279
        raw_svg = self.svg_transformer.tokenizer.batch_decode(outputs, skip_special_tokens=True)
        res = {"raw_svg": raw_svg, "outputs": outputs, "inputs_embeds": inputs_embeds}
        if kwargs.get("return_logprobs"):
            res.update(logprobs=gen["token_logprobs"], entropies=gen["token_entropies"])
        res["completion_mask"] = completion_mask(new, int(lm.eos_token_id if eos is None else eos))
        if top_k:
            res.update({k: gen[k] for k in ("top_token_ids", "top_logprobs", "token_ranks")})
        return res


class StarVectorStarCoder2(StarVectorStarCoder):
    """v2 binding (starvector_v2.py:8-63): StarCoder2 decoder, SigLIP tower, `embed_tokens`, no im2svg kwargs."""

    def __init__(self, config: StarVectorConfig, engine: HipEngine, tokenizer):
        super().__init__(config, engine, tokenizer, v2=True)

    def _get_embeddings(self, input_ids):                             # starvector_v2.py:45-47
        return self.svg_transformer.transformer.model.embed_tokens(input_ids)

    def _get_im2svg_specific_kwargs(self, kwargs):                    # starvector_v2.py:53-57
        return {}

    def _get_text2svg_specific_kwargs(self, kwargs):                  # starvector_v2.py:59-63
        return {"eos_token_id": self.svg_transformer.tokenizer.eos_token_id}


class StarVectorForCausalLM(nn.Module):
    """starvector_arch.py:133-193 facade."""
    config_class = StarVectorConfig

    def __init__(self, config: StarVectorConfig, state_dict: Optional[Dict[str, torch.Tensor]] = None, tokenizer=None,
                 device: Optional[int] = None):
        super().__init__()
        self.config = config
        ecfg = config.engine_config()
        self.engine = HipEngine(ecfg, device=device)
        if ecfg.weight_dtype != "bf16":
            print(f"[starvector_amd] decoder weights quantised to {ecfg.weight_dtype} at load: not the reference's precision "
                  "(accuracy on a real checkpoint is unmeasured)", file=sys.stderr)
        if ecfg.kv_dtype != "bf16":
            info = self.engine.kv_info()
            print(f"[starvector_amd] KV cache kept as {ecfg.kv_dtype} ({info['page_bytes']} bytes per page, pool {info['pool_bytes'] / 2**20:.0f} MiB): "
                  "not the reference's precision (accuracy on a real checkpoint is unmeasured)", file=sys.stderr)
        if state_dict is not None:
            self.engine.load_state_dict(state_dict)
        if tokenizer is None:
            tokenizer = ByteTokenizer(config.vocab_size, v2=config.is_v2)
        cls = StarVectorStarCoder2 if config.is_v2 else StarVectorStarCoder       # starvector_arch.py:139-144
        self.model = cls(config, self.engine, tokenizer)

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype="bfloat16", tokenizer=None, **kwargs):
        """Load a LOCAL checkpoint directory in the reference's format (config.json + *.safetensors).
        There is no network here: hub names are rejected with a clear error."""
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path!r} is not a local directory (hub download is unavailable offline)")
        with open(os.path.join(path, "config.json")) as f:
            cfg_json = json.load(f)
        from safetensors.torch import load_file
        sd: Dict[str, torch.Tensor] = {}
        for fn in sorted(os.listdir(path)):
            if fn.endswith(".safetensors"):
                sd.update(load_file(os.path.join(path, fn)))
        cfg = config_from_checkpoint({**cfg_json, **{k: v for k, v in kwargs.items() if k != "byte_tokenizer_fallback"}},
                                     {k: tuple(v.shape) for k, v in sd.items()})
        if tokenizer is None:
            tok_files = ("tokenizer.json", "tokenizer_config.json", "vocab.json", "tokenizer.model", "merges.txt")
            if any(os.path.exists(os.path.join(path, f)) for f in tok_files):
                # a checkpoint that ships a tokenizer must load it: a silent byte-level stand-in would turn '<svg' / '</svg>'
                # into the wrong ids (the stop would never fire, the output would decode to garbage) -- errors propagate
                from transformers import AutoTokenizer
                tokenizer = AutoTokenizer.from_pretrained(path, use_fast=False)
            elif kwargs.get("byte_tokenizer_fallback", False):
                import warnings
                warnings.warn(f"{path!r} has no tokenizer files: using the byte-level stand-in tokenizer (ids are bytes + 1; "
                              "NOT the StarCoder vocabulary -- only meaningful for synthetic weights)", RuntimeWarning)
                tokenizer = None
            else:
                raise FileNotFoundError(
                    f"{path!r} has no tokenizer files (tokenizer.json / vocab.json / ...): pass tokenizer=..., or "
                    "byte_tokenizer_fallback=True to use the byte-level stand-in (synthetic weights only)")
        return cls(cfg, state_dict=sd, tokenizer=tokenizer)

    @staticmethod
    def _scoring_mask_lead(attention_mask, shape):
        """The mask analysis of the scoring passes (`forward`, `completion_logprobs`): None when no row has leading pads, else the
        number of leading pads per row.  Raises for masks that are not left / right padding."""
        if not _is_padded(attention_mask):
            return None
        # Right padding (completions padded after their EOS, what a GRPO trainer passes): under the causal mask a real
        # position never sees a later key and HF's positions (cumsum(mask) - 1) equal the plain index for it, so the
        # logits of every real position are those of the unmasked run.  Rows at padded positions are unspecified (HF's
        # differ there too from any unpadded run; the caller multiplies them away with the same mask).
        # Left padding: the pinned transformers (4.49; gpt_bigcode/modeling_gpt_bigcode.py:980-983) masks the padded keys and
        # numbers positions by cumsum(mask) - 1 inside the model's forward, i.e. a left-padded row IS the same row with its
        # padding removed (pinned against HF: oracle/make_golden.py::run_forward_case, tests/golden/tiny_forward) -> rows are
        # grouped by their number of leading pads, scored without them, and their logits put back at the real positions.
        m = attention_mask.to(torch.bool)
        if m.shape != tuple(shape):
            raise ValueError(f"attention_mask {tuple(m.shape)} does not cover inputs_embeds {tuple(shape)}")
        lead = (m.cumsum(1) == 0).sum(1)                                  # leading pads per row
        if bool((lead >= m.shape[1]).any()):
            empty = (lead >= m.shape[1]).nonzero().flatten().tolist()
            raise ValueError(f"attention_mask rows {empty} are all zeros: a row needs at least one real position to be scored")
        idx = torch.arange(m.shape[1], device=m.device).unsqueeze(0)
        real = idx >= lead.unsqueeze(1)
        if bool((m[:, 1:] & ~m[:, :-1] & real[:, :-1]).any()):            # a 1 after a 0 behind the leading pads
            raise NotImplementedError("attention masks with holes are not built for the scoring forward (left / right padding only)")
        return lead if bool(lead.any()) else None

    def _run_scoring(self, fn):
        """One engine call of a scoring pass: queued as an exclusive job when a ContinuousBatcher shares the engine, else under the
        engine's call lock."""
        lm = getattr(getattr(self.model, "svg_transformer", None), "transformer", None)
        batcher = getattr(lm, "batcher", None)
        if batcher is not None and not _in_exclusive_job():
            # requests share the engine's decode loop: the scoring pass wants the engine to itself (it would fail with SV_ESTATE
            # while slots are live) -> queue it as an exclusive job, FIFO with the generation requests
            return _exclusive(batcher, fn)
        with _call_lock(self.engine):
            return fn()

    @torch.no_grad()
    def forward(self, vision_embeds, input_ids, num_generations, attention_mask, num_logits_to_keep):
        """starvector_arch.py:161-184, inference mode (no autograd graph: the engine holds no torch parameters): logits of
        the completions given the visual prefix, as GRPO's log-prob pass asks for them."""
        completion_embeds = self.model._get_embeddings(input_ids)
        inputs_embeds = torch.cat([vision_embeds.repeat(num_generations, 1, 1).to(completion_embeds.dtype),
                                   completion_embeds], dim=1)
        lead = self._scoring_mask_lead(attention_mask, inputs_embeds.shape[:2])
        emb16, keep = inputs_embeds.to(torch.bfloat16), int(num_logits_to_keep or 0)

        def score(e16):
            return self._run_scoring(lambda: self.engine.forward_logits(e16, keep))

        if lead is None:
            logits = score(emb16)
        else:
            S = emb16.shape[1]
            if keep and int(lead.max()) + keep > S:
                raise ValueError(f"num_logits_to_keep ({keep}) reaches into the left padding of a row ({int(lead.max())} pads of {S})")
            logits = None
            for pads in sorted(set(lead.tolist())):
                rows = (lead == pads).nonzero().flatten()
                lg = score(emb16[rows, pads:].contiguous())                   # [rows, keep or S - pads, V]
                if logits is None:
                    logits = torch.zeros(emb16.shape[0], keep or S, lg.shape[-1], dtype=lg.dtype, device=lg.device)
                logits[rows.to(lg.device), (0 if keep else pads):] = lg
        try:
            from transformers.modeling_outputs import CausalLMOutputWithCrossAttentions
            return CausalLMOutputWithCrossAttentions(loss=None, logits=logits, past_key_values=None, hidden_states=None,
                                                     attentions=None, cross_attentions=None)
        except Exception:                                   # transformers not importable: same field names
            import types
            return types.SimpleNamespace(loss=None, logits=logits, past_key_values=None, hidden_states=None,
                                         attentions=None, cross_attentions=None)

    @torch.no_grad()
    def completion_logprobs(self, vision_embeds, input_ids, num_generations, attention_mask, num_logits_to_keep,
                            temperature: float = 1.0, return_entropy: bool = False, top_logprobs: int = 0, unpadded: bool = False,
                            share_prefix: bool = False):
        """What a GRPO trainer computes from `forward`'s logits, without the logits: float32 [B, n], out[b, j] = the log-probability
        of input_ids[b, -n + j] given everything before it -- selective_log_softmax(forward(...).logits[:, :-1] / temperature, ids)
        with the softmax in fp32 over the bf16 logits (sv_forward_logprobs: device memory does not grow with B * n * vocab).
        n = num_logits_to_keep (0 / None: every completion token that has a position before it).  Padding as in `forward`: an
        entry whose token is right padding is 0; left-padded rows are scored without their pads; masks with holes raise
        NotImplementedError.  return_entropy: also the entropy [B, n] of the distribution each token was drawn from (0 at pads).
        top_logprobs = k in 1..32 (sv_forward_topk; teacher-forced distillation targets): the result is a dict instead -- "logprobs" [B, n],
        "entropies" when asked for, and "top_token_ids" / "top_logprobs" [B, n, k] (the k most likely ids of every position, best first, and
        their log-probs) and "token_ranks" [B, n] (the rank of the token itself, 0 at pads).
        unpadded=True (sv_forward_logprobs_ragged): with a mask that has pads, every row is stripped of its left and right pads and all rows go
        down in ONE ragged pass -- no pad goes through a layer or the lm_head, and there is one prompt pass whatever the pad counts.  The values
        equal scoring each row alone without its pads, bit for bit; they are NOT the bits of the padded call (unpadded=False), where a
        right-padded row takes its GEMM kernels by the padded length S, not by its own.  Entries at pads hold the fill values: 0 for log-prob,
        entropy and rank, id -1 / log-prob 0 in the lists.  A mask without pads takes the rectangular call; an engine without
        `forward_logprobs_ragged` raises NotImplementedError.
        share_prefix=True (sv_forward_logprobs_prefixed): vision_embeds is [P, Sv, hidden] and is NOT repeated -- row r of input_ids belongs to
        image r % P (the reference's `repeat` order) and every image's visual rows go through the decoder ONCE, not num_generations times.  Rows
        are stripped of their right padding as under unpadded=True and go down in one prefixed pass; a mask with left pads (they would lie in
        the shared prefix) raises ValueError, one with holes NotImplementedError.  A row the entry point would refuse (its split-K remainder rows
        would reach into the prefix: `HipEngine.prefix_refused`) is scored through `forward_logprobs_ragged` on its concatenation in the same
        call.  Shapes, fill values and dict keys as above; the values equal each stripped row's solo run bit for bit, hence unpadded=True
        wherever that call takes the ragged pass."""
        k = int(top_logprobs or 0)
        if share_prefix:
            return self._completion_logprobs_shared(vision_embeds, input_ids, num_generations, attention_mask, num_logits_to_keep, temperature,
                                                    return_entropy, k)
        completion_embeds = self.model._get_embeddings(input_ids)
        inputs_embeds = torch.cat([vision_embeds.repeat(num_generations, 1, 1).to(completion_embeds.dtype),
                                   completion_embeds], dim=1)
        B, S = inputs_embeds.shape[:2]
        L = input_ids.shape[1]
        n = int(num_logits_to_keep or 0) or (L if S > L else L - 1)
        if n < 1 or n > L or n + 1 > S:
            raise ValueError(f"num_logits_to_keep ({n}) must be in 1..{min(L, S - 1)}: every scored token needs a position before it")
        if attention_mask is not None and tuple(attention_mask.shape) != (B, S):
            raise ValueError(f"attention_mask {tuple(attention_mask.shape)} does not cover inputs_embeds {(B, S)}")
        lead = self._scoring_mask_lead(attention_mask, (B, S))
        if lead is not None and int(lead.max()) + n + 1 > S:
            raise ValueError(f"num_logits_to_keep ({n}) reaches into the left padding of a row ({int(lead.max())} pads of {S})")
        emb16 = inputs_embeds.to(torch.bfloat16)
        # n + 1 rows are kept: row i predicts the token at position S - n + i; the last row predicts nothing (-100)
        targets = torch.full((B, n + 1), -100, dtype=torch.int32, device=emb16.device)
        targets[:, :n] = input_ids[:, L - n:].to(device=emb16.device, dtype=torch.int32)
        if attention_mask is not None:
            pad = ~attention_mask.to(torch.bool)[:, S - n:].to(emb16.device)       # the token itself is padding
            targets[:, :n] = targets[:, :n].masked_fill(pad, -100)
        if unpadded and _is_padded(attention_mask):
            return self._completion_logprobs_unpadded(emb16, targets, attention_mask, n, temperature, return_entropy, k)

        def score(e16, tg):
            # (top_k goes down only when asked for: an engine without it is never handed it)
            r = self._run_scoring(lambda: self.engine.forward_logprobs(e16, tg, n + 1, temperature, return_entropy, **({"top_k": k} if k else {})))
            return r.logprobs, r.entropy, ((r.top_token_ids, r.top_logprobs, r.token_ranks) if k else None)

        if lead is None:
            lp, ent, top = score(emb16, targets)
        else:
            lp = torch.zeros(B, n + 1, dtype=torch.float32, device=emb16.device)
            ent = torch.zeros_like(lp) if return_entropy else None
            top = None
            if k:
                top = (torch.full((B, n + 1, k), -1, dtype=torch.int32, device=emb16.device),
                       torch.zeros(B, n + 1, k, dtype=torch.float32, device=emb16.device),
                       torch.zeros(B, n + 1, dtype=torch.int32, device=emb16.device))
            for pads in sorted(set(lead.tolist())):
                rows = (lead == pads).nonzero().flatten().to(emb16.device)
                a, h, t3 = score(emb16[rows, pads:].contiguous(), targets[rows].contiguous())
                lp[rows] = a
                if return_entropy:
                    ent[rows] = h
                if k:
                    for dst, src in zip(top, t3):
                        dst[rows] = src
        lp = lp[:, :n].contiguous()
        if return_entropy:
            ent = ent[:, :n]
            if attention_mask is not None:
                ent = ent.masked_fill(pad, 0.0)
            ent = ent.contiguous()
        if k:
            res = {"logprobs": lp, "top_token_ids": top[0][:, :n].contiguous(), "top_logprobs": top[1][:, :n].contiguous(),
                   "token_ranks": top[2][:, :n].contiguous()}
            if return_entropy:
                res["entropies"] = ent
            return res
        if not return_entropy:
            return lp
        return lp, ent

    def _completion_logprobs_unpadded(self, emb16, targets, attention_mask, n, temperature, return_entropy, k):
        """`completion_logprobs(unpadded=True)` behind the mask checks: targets [B, n + 1] holds -100 at pads and in its last column.  Row b's
        real positions are lead .. end - 1 (no holes); its scored tokens sit at S - n .. end - 1 (entries 0 .. c - 1 of the output, c of them,
        none when the row ends before S - n), so its last c + 1 rows are kept: row S - n - 1 + j predicts entry j, the last row nothing."""
        fn = getattr(self.engine, "forward_logprobs_ragged", None)
        if fn is None:
            raise NotImplementedError("completion_logprobs(unpadded=True) needs an engine with forward_logprobs_ragged")
        B, S = emb16.shape[:2]
        m = attention_mask.to(torch.bool).to(emb16.device)
        lens = m.sum(1).tolist()
        lead = (m.cumsum(1) == 0).sum(1).tolist()
        count = [max(0, lead[b] + lens[b] - (S - n)) for b in range(B)]
        keep = [c + 1 for c in count]
        packed_targets = torch.cat([torch.cat([targets[b, :c], targets[b, n:]]) for b, c in enumerate(count)])
        r = self._run_scoring(lambda: fn(emb16[m], packed_targets, keep, lengths=lens, temperature=temperature, entropy=return_entropy,
                                         **({"top_k": k} if k else {})))
        # scatter: entry j < count[b] of row b comes from packed row first[b] + j (the -100 row behind every sequence's entries is dropped)
        first = torch.tensor([sum(keep[:b]) for b in range(B)], device=emb16.device).unsqueeze(1)
        j = torch.arange(n, device=emb16.device).unsqueeze(0)
        scored = j < torch.tensor(count, device=emb16.device).unsqueeze(1)
        src = (first + j)[scored]

        def dense(packed, fill, *tail):
            out = torch.full((B, n, *tail), fill, dtype=packed.dtype, device=packed.device)
            out[scored] = packed[src]
            return out

        lp = dense(r.logprobs, 0.0)
        ent = dense(r.entropy, 0.0) if return_entropy else None
        if k:
            res = {"logprobs": lp, "top_token_ids": dense(r.top_token_ids, -1, k), "top_logprobs": dense(r.top_logprobs, 0.0, k),
                   "token_ranks": dense(r.token_ranks, 0)}
            if return_entropy:
                res["entropies"] = ent
            return res
        return (lp, ent) if return_entropy else lp

    def _completion_logprobs_shared(self, vision_embeds, input_ids, num_generations, attention_mask, num_logits_to_keep, temperature,
                                    return_entropy, k):
        """`completion_logprobs(share_prefix=True)`: the unpadded pass with every image's visual rows as a shared prefix.  Row b = (prefix b % P,
        own rows = its completion embeddings up to its last real position); its scored tokens sit at S - n .. end - 1 as in the unpadded pass,
        so its last c + 1 rows are kept -- c = own length reaches the prefix's last row, which predicts the first completion token."""
        fn = getattr(self.engine, "forward_logprobs_prefixed", None)
        if fn is None or getattr(self.engine, "forward_logprobs_ragged", None) is None:
            raise NotImplementedError("completion_logprobs(share_prefix=True) needs an engine with forward_logprobs_prefixed")
        own = self.model._get_embeddings(input_ids).to(torch.bfloat16)
        dev_ = own.device
        B, L = input_ids.shape
        P, Sv = vision_embeds.shape[:2]
        S = Sv + L
        if B != P * int(num_generations):
            raise ValueError(f"share_prefix: {B} completions are not num_generations ({num_generations}) x {P} images")
        n = int(num_logits_to_keep or 0) or L
        if n < 1 or n > L:
            raise ValueError(f"num_logits_to_keep ({n}) must be in 1..{L}: every scored token needs a position before it")
        if attention_mask is None:
            m = torch.ones(B, S, dtype=torch.bool, device=dev_)
        else:
            if tuple(attention_mask.shape) != (B, S):
                raise ValueError(f"attention_mask {tuple(attention_mask.shape)} does not cover inputs_embeds {(B, S)}")
            if self._scoring_mask_lead(attention_mask, (B, S)) is not None:
                raise ValueError("share_prefix: left padding would lie inside the shared visual prefix (right padding only)")
            m = attention_mask.to(torch.bool).to(dev_)
        ends = m.sum(1).tolist()                                   # real positions 0 .. end - 1 (no lead, no holes)
        lens = [e - Sv for e in ends]
        if min(lens) < 1:
            raise ValueError(f"share_prefix: rows {[b for b, v in enumerate(lens) if v < 1]} end inside the visual prefix: a row needs one completion token")
        targets = torch.full((B, n + 1), -100, dtype=torch.int32, device=dev_)
        targets[:, :n] = input_ids[:, L - n:].to(device=dev_, dtype=torch.int32).masked_fill(~m[:, S - n:], -100)
        count = [max(0, e - (S - n)) for e in ends]
        keep = [c + 1 for c in count]
        row_targets = [torch.cat([targets[b, :c], targets[b, n:]]) for b, c in enumerate(count)]
        prefixes = [vision_embeds[u].to(torch.bfloat16).to(dev_) for u in range(P)]
        seqs = [own[b, :lens[b]] for b in range(B)]
        prefix_of = [b % P for b in range(B)]
        refused = set(self.engine.prefix_refused([Sv] * P, lens, prefix_of))
        take = [b for b in range(B) if b not in refused]
        kw = dict(temperature=temperature, entropy=return_entropy, **({"top_k": k} if k else {}))
        parts = []                                                 # (rows, result) per engine call
        if take:
            used = sorted({prefix_of[b] for b in take})            # (a prefix whose every row is refused stays out of the pass)
            slot = {u: i for i, u in enumerate(used)}
            parts.append((take, self._run_scoring(lambda: fn([prefixes[u] for u in used], [seqs[b] for b in take], [slot[prefix_of[b]] for b in take],
                                                               torch.cat([row_targets[b] for b in take]), [keep[b] for b in take], **kw))))
        if refused:
            rest = sorted(refused)
            cat = [torch.cat([prefixes[prefix_of[b]], seqs[b]]) for b in rest]
            parts.append((rest, self._run_scoring(lambda: self.engine.forward_logprobs_ragged(cat, torch.cat([row_targets[b] for b in rest]),
                                                                                              [keep[b] for b in rest], **kw))))

        def dense(name, fill, *tail):
            out = None
            for rows, r in parts:
                packed, first = getattr(r, name), 0
                if out is None:
                    out = torch.full((B, n, *tail), fill, dtype=packed.dtype, device=packed.device)
                for b in rows:                                     # the -100 row behind every sequence's entries is dropped
                    out[b, :count[b]] = packed[first:first + count[b]]
                    first += keep[b]
            return out

        lp = dense("logprobs", 0.0)
        ent = dense("entropy", 0.0) if return_entropy else None
        if k:
            res = {"logprobs": lp, "top_token_ids": dense("top_token_ids", -1, k), "top_logprobs": dense("top_logprobs", 0.0, k),
                   "token_ranks": dense("token_ranks", 0)}
            if return_entropy:
                res["entropies"] = ent
            return res
        return (lp, ent) if return_entropy else lp

    def generate_im2svg(self, batch, **kwargs):           # starvector_arch.py:186-187
        return self.model.generate_im2svg(batch, **kwargs)

    def generate_im2text(self, batch, **kwargs):          # starvector_arch.py:189-190 forwards to a method the
        raise NotImplementedError("generate_im2text does not exist in the reference either (starvector_arch.py:189)")

    def process_images(self, images):                     # starvector_arch.py:192-193
        return self.model.image_encoder.process_images(images)
