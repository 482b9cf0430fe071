"""Python handle on the C-ABI engine: tensors in, tensors out (PyTorch is only the allocator/stream)."""
from __future__ import annotations

import ctypes as C
import enum
import os
import threading
from dataclasses import dataclass
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import SvConfig, SvSampling, check


class Exp(enum.IntFlag):
    """The A/B switches of an engine (`HipEngine.set_exp`, the SV_EXP environment variable): mirror of `enum sv_exp_bits` in
    include/starvector_hip_debug.h, where each switch is described; tests/test_native_host_logic.py pins it against the library."""
    NO_LN_FOLD = 2
    MLP_FUSED_FORCE = 128
    MLP_FUSED_OFF = 512
    SEPARATE_ARGMAX = 1024
    ROWLN_CATTN_OFF = 8192
    ROWLN_CATTN_FORCE = 16384
    NO_PRUNE_LAST = 32768
    BATCH_REMAINDER = 4194304

    @classmethod
    def known(cls) -> int:
        mask = 0
        for m in cls:
            mask |= int(m)
        return mask

    @classmethod
    def parse(cls, text) -> "Exp":
        """A mask from names and / or numbers joined by '+', '|' or ',' ("MLP_FUSED_FORCE+16384", "SV_EXP_NO_LN_FOLD", "0");
        ValueError for a name or a bit that is no switch."""
        mask = 0
        for part in str(text).replace("|", "+").replace(",", "+").split("+"):
            part = part.strip()
            name = part.upper()[7:] if part.upper().startswith("SV_EXP_") else part.upper()
            if name in cls.__members__:
                mask |= int(cls.__members__[name])
            else:
                try:
                    mask |= int(part, 0)
                except ValueError:
                    raise ValueError(f"unknown switch {part!r}; the switches: {', '.join(cls.__members__)}") from None
        bad = mask & ~cls.known()
        if mask < 0 or bad:
            raise ValueError(f"mask {mask}: bits {[1 << i for i in range(32) if bad >> i & 1]} are no switch of this build "
                             f"(the switches: {', '.join(f'{m.name} = {int(m)}' for m in cls)})")
        return cls(mask)


@dataclass
class EngineConfig:
    """Shapes of the path; defaults = StarVector-1B (StarVectorConfig, starvector_arch.py:96-131)."""
    image_size: int = 224
    patch_size: int = 14
    vit_width: int = 1024
    vit_layers: int = 23
    vit_heads: int = 16
    adapter_norm: str = "layer_norm"
    hidden: int = 2048
    n_layer: int = 24
    n_head: int = 16
    n_inner: int = 8192
    vocab: int = 49156
    n_positions: int = 8192
    max_batch: int = 32
    max_seq_len: int = 2048
    ln_eps: float = 1e-5
    # StarVector-8B: SigLIP tower + StarCoder2 (RoPE, GQA); defaults describe v1
    arch: str = "v1"
    n_kv_head: int = 1
    rope_theta: float = 1e6
    vit_mlp: int = 4096
    vit_eps: float = 1e-6
    sliding_window: int = 0          # v2: keys visible to a query (4096 for bigcode/starcoder2-7b); 0 = all
    weight_dtype: str = "bf16"       # "fp8_e4m3": decoder weights + lm_head quantised at load (per-row scales), BASELINE config 5;
                                     # "mxfp4": the same tensors as OCP MXFP4 (e2m1 codes, one e8m0 scale per 32 k: sv_config.weight_dtype)
    exclusive_device: object = False # False / True / "auto" (2: on until a fused launch gives up, then off for good and the call re-run: sv_config.exclusive_device).
                                     # True: this engine alone launches kernels on its GPU while decoding (one process per GPU): enables the
                                     # all-blocks-resident fused launches (include/starvector_hip.h sv_config.exclusive_device); same tokens
    kv_dtype: str = "bf16"           # the paged KV cache's format: "bf16", or "fp8_e4m3" -- e4m3 codes and one power-of-two scale per key and
                                     # head, half the pool and half the decode attention's stream (sv_create_kv; not a reference numerics mode)
    prefill_chunk_rows: int = 0      # row budget of the prompt passes (HipEngine.set_prefill_chunk, applied after creation; 0 = the environment's
                                     # SV_PREFILL_CHUNK_ROWS, else off): same tokens, prompt-pass workspaces bounded by the budget

    @property
    def query_length(self) -> int:
        return (self.image_size // self.patch_size) ** 2 + (1 if self.arch == "v1" else 0)

    @staticmethod
    def starvector_8b(max_batch: int = 16, max_seq_len: int = 4096) -> "EngineConfig":
        """siglip_384 (google/siglip-large-patch16-384) + bigcode/starcoder2-7b shapes."""
        return EngineConfig(image_size=384, patch_size=16, vit_width=1024, vit_layers=24, vit_heads=16, hidden=4608,
                            n_layer=32, n_head=36, n_inner=18432, vocab=49152 + 5, n_positions=16384,
                            max_batch=max_batch, max_seq_len=max_seq_len, arch="v2", n_kv_head=4, rope_theta=1e6,
                            vit_mlp=4096, vit_eps=1e-6, sliding_window=4096)


class TokenLogprobs(NamedTuple):
    """`HipEngine.forward_logprobs`: [B, n] tensors; `entropy` / `argmax` are None unless asked for."""
    logprobs: torch.Tensor                     # float32: log softmax(logits / temperature) at the target id; 0 where the target is -100
    logsumexp: torch.Tensor                    # float32: logsumexp(logits / temperature)
    entropy: Optional[torch.Tensor] = None     # float32: entropy of softmax(logits / temperature)
    argmax: Optional[torch.Tensor] = None      # int32: the lowest index holding the row's maximum


class TokenTopLogprobs(NamedTuple):
    """`HipEngine.forward_logprobs(..., top_k=k)`: the fields of `TokenLogprobs` and the lists (a type of its own: code that walks the four
    fields of `TokenLogprobs` keeps meeting four)."""
    logprobs: torch.Tensor
    logsumexp: torch.Tensor
    entropy: Optional[torch.Tensor]
    argmax: Optional[torch.Tensor]
    top_token_ids: torch.Tensor                # int32 [B, n, k]: the k most likely ids, best first (-1 where fewer exist)
    top_logprobs: torch.Tensor                 # float32 [B, n, k]: their log-probs (-inf where the id is -1)
    token_ranks: torch.Tensor                  # int32 [B, n]: 1 + the ids with a larger logit than the target; 0 where the target is -100


TOKEN_STATS = ("token_logprobs", "token_logprobs_processed", "token_entropies")      # HipEngine.generate(token_stats=...), sv_token_stats's order
TOPK_MAX = 32                                   # SV_TOPK_MAX
TOPK_SOURCES = ("raw", "processed")             # sv_token_topk.source 0 / 1


def token_topk_request(token_topk):
    """`HipEngine.generate(token_topk=...)`: an int k, or dict(k=, source="raw" | "processed", rank=True) -> (k, source index, rank)."""
    req = {"k": token_topk} if not isinstance(token_topk, dict) else dict(token_topk)
    unknown = set(req) - {"k", "source", "rank"}
    if unknown or "k" not in req:
        raise ValueError(f"token_topk must be an int or dict(k=, source=, rank=), got {token_topk!r}")
    k, source, rank = req["k"], req.get("source", "raw"), req.get("rank", True)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= TOPK_MAX:
        raise ValueError(f"token_topk: k must be an int in 1..{TOPK_MAX}, got {k!r}")
    if source not in TOPK_SOURCES:
        raise ValueError(f"token_topk: source must be one of {TOPK_SOURCES}, got {source!r}")
    return k, TOPK_SOURCES.index(source), bool(rank)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(t: torch.Tensor, dtype, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError(f"{what} must be a CUDA(HIP) tensor; the engine has no CPU path")
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
    return t.contiguous()


WEIGHT_DTYPES = {"bf16": 0, "fp8_e4m3": 1, "mxfp4": 2}          # SV_WEIGHT_*
_WEIGHT_DTYPE_ALIASES = {"fp8": "fp8_e4m3", "bfloat16": "bf16"}


def resolve_weight_dtype(weight_dtype=None) -> str:
    """The canonical name of a decoder weight format: "bf16", "fp8_e4m3" (also "fp8") or "mxfp4".  None = the environment's
    SV_WEIGHT_DTYPE, else "bf16"."""
    if weight_dtype is None:
        weight_dtype = os.environ.get("SV_WEIGHT_DTYPE") or "bf16"
    name = str(weight_dtype).lower()
    name = _WEIGHT_DTYPE_ALIASES.get(name, name)
    if name not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {sorted(WEIGHT_DTYPES)} (or 'fp8'), got {weight_dtype!r}")
    return name


def weight_dtype_code(weight_dtype) -> int:
    return WEIGHT_DTYPES[resolve_weight_dtype(weight_dtype)]


KV_DTYPES = {"bf16": 0, "fp8_e4m3": 1}                           # SV_KV_*
_KV_DTYPE_ALIASES = {"fp8": "fp8_e4m3", "bfloat16": "bf16", "auto": "bf16"}


def resolve_kv_dtype(kv_dtype=None) -> str:
    """The canonical name of a KV-cache format: "bf16" (also "auto") or "fp8_e4m3" (also "fp8").  None = the environment's SV_KV_DTYPE,
    else "bf16"."""
    if kv_dtype is None:
        kv_dtype = os.environ.get("SV_KV_DTYPE") or "bf16"
    name = str(kv_dtype).lower()
    name = _KV_DTYPE_ALIASES.get(name, name)
    if name not in KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {sorted(KV_DTYPES)} (or 'fp8' / 'auto'), got {kv_dtype!r}")
    return name


def kv_dtype_code(kv_dtype) -> int:
    return KV_DTYPES[resolve_kv_dtype(kv_dtype)]


def prefill_chunk_rows(prefill_chunk_rows=None) -> int:
    """The row budget of the prompt passes (sv_set_prefill_chunk): 0 = off, n >= 1 = at most n own rows per pass.  None = the environment's
    SV_PREFILL_CHUNK_ROWS, else 0."""
    v = prefill_chunk_rows
    if v is None:
        v = os.environ.get("SV_PREFILL_CHUNK_ROWS") or 0
    try:
        if isinstance(v, (bool, float)):
            raise ValueError
        n = int(v)
    except (TypeError, ValueError):
        raise ValueError(f"prefill_chunk_rows must be an int >= 0 (0 = off), got {v!r}") from None
    if n < 0:
        raise ValueError(f"prefill_chunk_rows must be an int >= 0 (0 = off), got {v!r}")
    return n


def kv_page_bytes(kv_dtype, head_dim: int) -> int:
    """Bytes of one KV page (64 tokens of one layer and KV head): bf16 K | V, or e4m3 codes + one scale byte per token for K and for V."""
    return 64 * head_dim * 2 + 128 if kv_dtype_code(kv_dtype) else 64 * head_dim * 2 * 2


def kv_pool_bytes(cfg: "EngineConfig") -> int:
    """Bytes of the KV pool an engine of this configuration allocates (what sv_kv_info reports): per layer and KV head, the pages of
    max_batch sequences of max_seq_len tokens and one more (the page free slots of a continuous batch write to)."""
    pages = cfg.max_batch * ((cfg.max_seq_len + 63) // 64) + 1
    n_kv = cfg.n_kv_head if cfg.arch == "v2" else 1
    return cfg.n_layer * n_kv * pages * kv_page_bytes(cfg.kv_dtype, cfg.hidden // cfg.n_head)


def _exclusive_code(v) -> int:
    """sv_config.exclusive_device: 0 (shared GPU), 1 (this engine owns it), 2 ("auto": optimistic, falls back for good at the first give-up)."""
    if isinstance(v, str):
        if v.lower() in ("auto", "optimistic", "2"):
            return 2
        return 1 if v.lower() in ("1", "true", "yes") else 0
    if v is True or v is False or v is None:
        return int(bool(v))
    return 2 if int(v) == 2 else int(bool(v))


class HipEngine:
    """Owns one ``sv_engine`` (weights repacked into library memory, paged KV pool, workspaces)."""

    def __init__(self, cfg: EngineConfig, device: Optional[int] = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.StarVectorHipError("no HIP device visible; the StarVector engine requires a GPU")
        self.cfg = cfg
        self.device = torch.cuda.current_device() if device is None else int(device)
        c = SvConfig(cfg.image_size, cfg.patch_size, cfg.vit_width, cfg.vit_layers, cfg.vit_heads,
                     _lib.SV_NORM_LAYER if cfg.adapter_norm == "layer_norm" else _lib.SV_NORM_BATCH,
                     cfg.hidden, cfg.n_layer, cfg.n_head, cfg.n_inner, cfg.vocab, cfg.n_positions,
                     cfg.max_batch, cfg.max_seq_len, cfg.ln_eps, self.device,
                     _lib.SV_ARCH_V2 if cfg.arch == "v2" else _lib.SV_ARCH_V1, cfg.n_kv_head, cfg.rope_theta,
                     cfg.vit_mlp, cfg.vit_eps if cfg.arch == "v2" else cfg.ln_eps,
                     int(cfg.sliding_window) if cfg.arch == "v2" else 0,
                     weight_dtype_code(cfg.weight_dtype), _exclusive_code(getattr(cfg, "exclusive_device", False)))
        h = C.c_void_p()
        # the default spelling takes sv_create; any other one ("fp8_e4m3", or "auto" / "bfloat16" for the bf16 cache) sv_create_kv with its code
        kv_name = getattr(cfg, "kv_dtype", "bf16")
        if kv_name == "bf16":
            check(self.lib.sv_create(C.byref(c), C.byref(h)), "sv_create")
        else:
            check(self.lib.sv_create_kv(C.byref(c), kv_dtype_code(kv_name), C.byref(h)), "sv_create_kv")
        self._h = h
        self._dev = torch.device("cuda", self.device)
        # One multi-call sequence at a time per engine: a padded batch run as slots (cb_reset ... cb_reset), a classic
        # generate, a scoring forward.  The library serialises single calls with its own mutex; THIS lock keeps two host
        # threads from interleaving their call sequences (thread B's cb_reset would release thread A's slots).
        self.call_lock = threading.RLock()
        self._cb_lp_k = {}                   # slot -> the k its current holder records with (cb_read_logprobs sizes its buffers by it)
        rows = prefill_chunk_rows(getattr(cfg, "prefill_chunk_rows", 0) or None)      # 0 in the config: the environment's default, else off
        if rows:
            self.set_prefill_chunk(rows)

    def kv_info(self) -> dict:
        """The KV cache's format, the bytes of one page (64 tokens of one layer and KV head) and of the whole pool (sv_kv_info)."""
        fmt, page, pool = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        check(self.lib.sv_kv_info(self._h, C.byref(fmt), C.byref(page), C.byref(pool)), "sv_kv_info")
        return {"kv_dtype": {v: k for k, v in KV_DTYPES.items()}[fmt.value], "page_bytes": page.value, "pool_bytes": pool.value}

    def close(self):
        if getattr(self, "_h", None):
            self.lib.sv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights -------------------------------------------------------------------------------
    def load_weight(self, name: str, t: torch.Tensor) -> None:
        if t.dtype == torch.bfloat16:
            dt = _lib.SV_DTYPE_BF16
        elif t.dtype == torch.float32:
            dt = _lib.SV_DTYPE_F32
        else:
            t = t.to(torch.float32)
            dt = _lib.SV_DTYPE_F32
        t = t.to(self._dev).contiguous()
        shape = (C.c_int64 * max(t.dim(), 1))(*(t.shape if t.dim() else (1,)))
        check(self.lib.sv_load_weight(self._h, name.encode(), _ptr(t), dt, max(t.dim(), 1), shape, _stream()),
              f"sv_load_weight({name})")

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> None:
        """Ingest a reference state_dict (keys as saved by the reference, train/util.py:71)."""
        skipped = []
        for k, v in sd.items():
            if k.endswith("num_batches_tracked") or k.endswith(".attn.bias") or k.endswith(".attn.masked_bias") \
                    or ".visual_encoder.head." in k or k.endswith("rotary_emb.inv_freq"):
                continue
            try:
                self.load_weight(k, v)
            except KeyError:
                skipped.append(k)
        if strict and skipped:
            raise KeyError(f"unexpected keys in state_dict: {skipped[:5]}{'...' if len(skipped) > 5 else ''}")
        check(self.lib.sv_weights_complete(self._h), "sv_weights_complete")

    def expected_weights(self) -> List[Tuple[str, int, bool, bool]]:
        """(reference state_dict key, element count, required, loaded) for every tensor this engine expects, sorted by name."""
        n = self.lib.sv_weight_count(self._h)
        if n < 0:
            check(n, "sv_weight_count")
        out = []
        name = C.create_string_buffer(512)
        numel, req, loaded = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        for i in range(n):
            check(self.lib.sv_weight_info(self._h, i, name, 512, C.byref(numel), C.byref(req), C.byref(loaded)), "sv_weight_info")
            out.append((name.value.decode(), int(numel.value), bool(req.value), bool(loaded.value)))
        return out

    def load_random_weights(self, seed: int = 1234, std: float = 0.02) -> None:
        """Random-init weights of this architecture, drawn ON THE GPU one tensor at a time (throughput runs; there is no network for
        checkpoints): Linear / embedding / position tensors and biases N(0, std), LayerNorm / BatchNorm scales (and running_var) 1,
        their biases (and running_mean) 0.  Each tensor has its own generator seeded by (seed, crc32(name)): the values do not depend
        on the enumeration order or on what else is loaded."""
        import zlib
        for name, numel, required, _ in self.expected_weights():
            if not required:
                continue                                   # the tied lm_head: the engine packs wte for it
            norm = ".ln_" in name or "norm" in name        # ln_1 / ln_2 / ln_pre / ln_vision / ln_f, layer_norm*, *layernorm, norm
            if norm and (name.endswith(".weight") or name.endswith("running_var")):
                t = torch.ones(numel, dtype=torch.bfloat16, device=self._dev)
            elif norm and (name.endswith(".bias") or name.endswith("running_mean")):
                t = torch.zeros(numel, dtype=torch.bfloat16, device=self._dev)
            else:
                g = torch.Generator(device=self._dev).manual_seed((int(seed) << 32) ^ zlib.crc32(name.encode()))
                t = torch.empty(numel, dtype=torch.float32, device=self._dev).normal_(0.0, std, generator=g).to(torch.bfloat16)
            self.load_weight(name, t)
        check(self.lib.sv_weights_complete(self._h), "sv_weights_complete")

    # ---- forward entry points -----------------------------------------------------------------
    def encode_image(self, image: torch.Tensor) -> torch.Tensor:
        image = _need(image, torch.bfloat16, "image")
        B = image.shape[0]
        if image.shape[1:] != (3, self.cfg.image_size, self.cfg.image_size):
            raise ValueError(f"image must be [B,3,{self.cfg.image_size},{self.cfg.image_size}], got {tuple(image.shape)}")
        out = torch.empty(B, self.cfg.query_length, self.cfg.vit_width, dtype=torch.bfloat16, device=image.device)
        check(self.lib.sv_encode_image(self._h, _ptr(image), B, _ptr(out), _stream()), "sv_encode_image")
        return out

    def adapter(self, x: torch.Tensor) -> torch.Tensor:
        x = _need(x, torch.bfloat16, "adapter input")
        B = x.shape[0]
        if x.shape[1:] != (self.cfg.query_length, self.cfg.vit_width):
            raise ValueError(f"adapter input must be [B,{self.cfg.query_length},{self.cfg.vit_width}]")
        out = torch.empty(B, self.cfg.query_length, self.cfg.hidden, dtype=torch.bfloat16, device=x.device)
        check(self.lib.sv_adapter(self._h, _ptr(x), B, _ptr(out), _stream()), "sv_adapter")
        return out

    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        ids = _need(ids, torch.int64, "input_ids")
        out = torch.empty(*ids.shape, self.cfg.hidden, dtype=torch.bfloat16, device=ids.device)
        check(self.lib.sv_embed_tokens(self._h, _ptr(ids), ids.numel(), _ptr(out), _stream()), "sv_embed_tokens")
        return out

    def prepare_inputs(self, enc: torch.Tensor, prompt_ids: torch.Tensor) -> torch.Tensor:
        """a1 (starvector_base.py:203-221) without the concatenation: adapter(enc) and the prompt's token embeddings are written straight
        into one [B, T + P, hidden] inputs_embeds buffer (the reference builds it with torch.cat; same values, no ATen kernel)."""
        enc = _need(enc, torch.bfloat16, "adapter input")
        ids = _need(prompt_ids, torch.int64, "input_ids")
        B, T = enc.shape[0], self.cfg.query_length
        if enc.shape[1:] != (T, self.cfg.vit_width) or ids.dim() != 2 or ids.shape[0] != B:
            raise ValueError(f"prepare_inputs: enc [B,{T},{self.cfg.vit_width}] and prompt_ids [B,P] expected")
        P = ids.shape[1]
        out = torch.empty(B, T + P, self.cfg.hidden, dtype=torch.bfloat16, device=enc.device)
        check(self.lib.sv_adapter_into(self._h, _ptr(enc), B, _ptr(out), T + P, _stream()), "sv_adapter_into")
        check(self.lib.sv_embed_tokens_into(self._h, _ptr(ids), B, P, _ptr(out), T + P, T, _stream()), "sv_embed_tokens_into")
        return out

    def prefill(self, inputs_embeds: torch.Tensor) -> torch.Tensor:
        x = _need(inputs_embeds, torch.bfloat16, "inputs_embeds")
        B, S0, D = x.shape
        if D != self.cfg.hidden:
            raise ValueError("inputs_embeds hidden size mismatch")
        logits = torch.empty(B, self.cfg.vocab, dtype=torch.float32, device=x.device)
        check(self.lib.sv_prefill(self._h, _ptr(x), B, S0, _ptr(logits), _stream()), "sv_prefill")
        return logits

    def _packed(self, embeds, lengths=None):
        """A ragged batch as (packed [sum(len), D] bf16, ctypes int32 lengths, list of lengths): from a list of [S_i, D] tensors, or from
        an already packed tensor and its lengths."""
        if lengths is None:
            seqs = [t.reshape(-1, t.shape[-1]) for t in embeds]
            if not seqs:
                raise ValueError("empty ragged batch")
            lens = [int(t.shape[0]) for t in seqs]
            x = torch.cat(seqs, dim=0) if len(seqs) > 1 else seqs[0]
        else:
            lens = [int(v) for v in lengths]
            x = embeds
        x = _need(x, torch.bfloat16, "inputs_embeds")
        if x.dim() != 2 or x.shape[1] != self.cfg.hidden:
            raise ValueError(f"packed inputs_embeds must be [sum(lengths), {self.cfg.hidden}], got {list(x.shape)}")
        if not lens or min(lens) < 1 or sum(lens) != x.shape[0]:
            raise ValueError(f"lengths {lens} do not describe the {x.shape[0]} packed rows (each >= 1)")
        return x, (C.c_int32 * len(lens))(*lens), lens

    def _prompt_form(self, embeds, lengths=None):
        """The prompts of a generate call as (x, ctypes lengths or None, B, S0): a rectangular [B, S0, D] tensor (lengths None), or the ragged
        form -- a packed [sum(lengths), D] tensor with `lengths`, or a list of [S_i, D] tensors -- where S0 is the longest prompt."""
        if lengths is not None or isinstance(embeds, (list, tuple)):
            x, lens_arr, lens = self._packed(embeds, lengths)
            B, S0, D = len(lens), max(lens), x.shape[1]
        else:
            x, lens_arr = _need(embeds, torch.bfloat16, "inputs_embeds"), None
            B, S0, D = x.shape
        if D != self.cfg.hidden:
            raise ValueError("inputs_embeds hidden size mismatch")
        return x, lens_arr, B, S0

    @staticmethod
    def _sampling(max_length, S0, stop_ids, on_tokens, *, do_sample, temperature, top_p, eos_token_id, pad_token_id, seed, sync_every,
                  repetition_penalty, num_beams=1, length_penalty=1.0, early_stopping=False, top_k=0, min_new_tokens=0):
        """The sv_sampling of a generate call after its budget check: (struct, max_new, what its pointers refer to -- the stop-id array and
        the streaming callback: keep it alive for the duration of the call --, the list that receives the callback's exception)."""
        max_new = max_length - S0
        if max_new <= 0:
            raise ValueError(f"max_length ({max_length}) must exceed the prompt length ({S0})")
        stops = list(stop_ids) if stop_ids else []
        arr = (C.c_int32 * max(len(stops), 1))(*stops) if stops else None
        sp = SvSampling(int(bool(do_sample)), float(temperature), float(top_p), int(max_length), int(eos_token_id),
                        int(pad_token_id), len(stops), C.cast(arr, C.POINTER(C.c_int32)) if stops else None,
                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(sync_every), float(repetition_penalty),
                        int(num_beams), float(length_penalty), _early_code(early_stopping), int(top_k or 0), None, None,
                        max(int(min_new_tokens or 0), 0))
        cb, cb_errors = None, []
        if on_tokens is not None:
            cb, cb_errors = token_callback(on_tokens)
            sp.on_tokens = C.cast(cb, C.c_void_p)
        return sp, max_new, (arr, cb), cb_errors

    def prefill_ragged(self, embeds, lengths=None) -> torch.Tensor:
        """One prompt pass over sequences of different lengths (sv_prefill_ragged): `embeds` a list of [S_i, D] tensors, or a packed
        [sum(lengths), D] tensor with `lengths`.  Returns the last-row logits [B, vocab]; every row's logits and KV entries are the bits
        of `prefill` on that sequence alone, and `decode_step` continues every row at its own position."""
        x, arr, lens = self._packed(embeds, lengths)
        logits = torch.empty(len(lens), self.cfg.vocab, dtype=torch.float32, device=x.device)
        check(self.lib.sv_prefill_ragged(self._h, _ptr(x), len(lens), arr, _ptr(logits), _stream()), "sv_prefill_ragged")
        return logits

    def prefill_open(self, total_lens) -> None:
        """Assign pages for sequences of these total lengths; every context becomes 0, nothing is computed (sv_prefill_open)."""
        tl = [int(v) for v in total_lens]
        check(self.lib.sv_prefill_open(self._h, len(tl), (C.c_int32 * max(len(tl), 1))(*tl)), "sv_prefill_open")

    def prefill_extend(self, embeds_packed, lens, total_lens=None) -> torch.Tensor:
        """Append lens[b] >= 0 rows to cached sequence b (sv_prefill_extend): `embeds_packed` the new rows back to back [sum(lens), D] (or a
        list of [n_i, D] tensors, one per sequence with lens[b] > 0).  `total_lens` states the length of the sequence each belongs to (None: the
        free extension, context + lens).  Returns logits [B, vocab]: the rows of the sequences this call brings to their total length hold their
        last-row logits, the other rows are NaN.  `decode_step` and further extensions continue every row at its own position."""
        ln = [int(v) for v in lens]
        if isinstance(embeds_packed, (list, tuple)):
            embeds_packed = torch.cat([t.reshape(-1, t.shape[-1]) for t in embeds_packed], dim=0)
        x = _need(embeds_packed, torch.bfloat16, "embeds_packed")
        if x.dim() != 2 or x.shape[1] != self.cfg.hidden or (ln and min(ln) >= 0 and sum(ln) != x.shape[0]):
            raise ValueError(f"embeds_packed must be [sum(lens) = {sum(ln)}, {self.cfg.hidden}], got {list(x.shape)}")
        tl = None
        if total_lens is not None:
            tl = [int(v) for v in total_lens]
            if len(tl) != len(ln):
                raise ValueError("total_lens: one total length per sequence")
        ints = lambda v: (C.c_int32 * max(len(v), 1))(*v)
        logits = torch.full((len(ln), self.cfg.vocab), float("nan"), dtype=torch.float32, device=x.device)
        check(self.lib.sv_prefill_extend(self._h, _ptr(x), len(ln), ints(ln), ints(tl) if tl is not None else None, _ptr(logits), _stream()),
              "sv_prefill_extend")
        return logits

    def set_prefill_chunk(self, rows: int) -> None:
        """Row budget of every prompt pass with a generate tail (sv_set_prefill_chunk): 0 = off; rows > 0: a pass of more packed rows runs as
        several passes of at most `rows` own rows over the cache, with the same logits, pages and tokens."""
        check(self.lib.sv_set_prefill_chunk(self._h, prefill_chunk_rows(rows)), "sv_set_prefill_chunk")

    def generate_ragged(self, embeds, max_length: int, lengths=None, **kw):
        """`generate` over prompts of different lengths in ONE prompt pass (sv_generate_ragged): HF's padded-batch semantics, `max_length`
        counts from the longest prompt, every row gets max_length - max(lengths) new tokens.  Same keywords and return value as `generate`."""
        return self.generate(embeds if lengths is not None else list(embeds), max_length, lengths=lengths, **kw)

    def generate_shared(self, embeds, max_length: int, n_samples: int, lengths=None, **kw):
        """``n_samples`` continuations of every prompt from ONE prompt pass over the un-repeated prompts (sv_generate_shared): ``embeds`` is
        [B, S0, D], or a list of [S_i, D] prompts / a packed tensor with ``lengths`` (the ragged form, budget from the longest prompt).  Returns
        B * n_samples rows, row b * n_samples + j = sample j of prompt b -- bit for bit what ``generate`` / ``generate_ragged`` return for
        the prompts repeated with ``repeat_interleave(n_samples, dim=0)``; the rows of a prompt share its full KV pages.  Same keywords and
        return value as ``generate``."""
        return self.generate(embeds, max_length, lengths=lengths, n_samples=n_samples, **kw)

    def generate_processed(self, embeds, max_length: int, no_repeat_ngram_size: int = 0, bad_words_ids=None, min_p: float = 0.0,
                           lengths=None, n_samples: int = 1, **kw):
        """``generate`` with HF's token-changing processors on device (sv_generate_processed): ``no_repeat_ngram_size`` (1..8: no n-gram of the
        generated ids repeats), ``bad_words_ids`` (at most 64 id sequences of at most 8 ids: never completed) and ``min_p`` (with do_sample:
        tokens below min_p * p_max are dropped after top-k / top-p).  ``embeds`` as in ``generate`` / ``generate_ragged`` / ``generate_shared``
        (``lengths``, ``n_samples``); same keywords and return value.  All three off: exactly ``generate``'s tokens.  ValueError beyond the
        limits or with num_beams > 1."""
        lp = logits_processors(no_repeat_ngram_size, bad_words_ids, min_p, vocab=self.cfg.vocab)
        return self.generate(embeds, max_length, lengths=lengths, n_samples=n_samples, logits_processors=lp, **kw)

    def generate_lookup(self, embeds, max_length: int, num_draft_tokens: int, max_ngram: int = 0, min_ngram: int = 0, lengths=None,
                        eos_token_id: int = 0, pad_token_id: int = 0, stop_ids: Optional[Sequence[int]] = None, sync_every: int = 0,
                        on_tokens=None, min_new_tokens: int = 0, return_counts: bool = False, **refused):
        """Greedy ``generate`` with prompt-lookup speculative decoding (sv_generate_lookup; HF's ``prompt_lookup_num_tokens``): every step
        verifies ``num_draft_tokens`` (1..15) drafted tokens of each sequence, drafted by an n-gram lookup (``max_ngram`` .. ``min_ngram``,
        0 = 3 and 1) over the ids the sequence has generated, and emits the accepted ones plus one more.  The tokens are those of
        ``generate`` / ``generate_ragged`` bit for bit.  ``embeds`` as there ([B, S0, D], or a list / packed tensor with ``lengths``).
        ``num_draft_tokens=0`` is the plain call.  ``return_counts=True``: (tokens, dict(steps, drafted, accepted)).  Sampling, beam search, a
        repetition penalty, processors, per-step outputs, statistics, top-k lists and n_samples > 1 raise NotImplementedError; so does
        streaming (``on_tokens``) with more than one row."""
        for name, off in (("do_sample", False), ("num_beams", 1), ("repetition_penalty", 1.0), ("logits_processors", None), ("scores_out", None),
                          ("logits_out", None), ("return_outputs", False), ("token_stats", False), ("token_topk", None), ("n_samples", 1)):
            if name in refused:
                v = refused.pop(name)
                if v is not None and v != off:
                    raise NotImplementedError(f"generate_lookup: {name}={v!r} is not built with prompt-lookup decoding (greedy verification, tokens only)")
        if refused:
            raise TypeError(f"generate_lookup: unexpected arguments {sorted(refused)}")
        return self._lookup_call("sv_generate_lookup", embeds, max_length, num_draft_tokens, max_ngram, min_ngram, lengths, eos_token_id,
                                 pad_token_id, stop_ids, sync_every, on_tokens, min_new_tokens, return_counts)

    def generate_lookup_sampled(self, embeds, max_length: int, num_draft_tokens: int, max_ngram: int = 0, min_ngram: int = 0, lengths=None,
                                eos_token_id: int = 0, pad_token_id: int = 0, stop_ids: Optional[Sequence[int]] = None, sync_every: int = 0,
                                on_tokens=None, min_new_tokens: int = 0, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0,
                                top_p: float = 1.0, seed: int = 0, repetition_penalty: float = 1.0, return_counts: bool = False, **refused):
        """``generate_lookup`` with the selection the call asks for (sv_generate_lookup_sampled): ``do_sample`` with ``temperature`` / ``top_k`` /
        ``top_p`` / ``seed``, and any ``repetition_penalty``.  Token-exact per seed: the tokens are those of ``generate`` / ``generate_ragged``
        with the same arguments bit for bit -- a row draws with the (seed, step, row) triple the plain call uses at its column, and a draft is
        accepted when it equals the token drawn in front of it.  Everything else as ``generate_lookup``; beam search, processors, per-step
        outputs, statistics, top-k lists and n_samples > 1 raise NotImplementedError, naming the argument; so does streaming with more than
        one row."""
        for name, off in (("num_beams", 1), ("logits_processors", None), ("scores_out", None), ("logits_out", None), ("return_outputs", False),
                          ("token_stats", False), ("token_topk", None), ("n_samples", 1)):
            if name in refused:
                v = refused.pop(name)
                if v is not None and v != off:
                    raise NotImplementedError(f"generate_lookup_sampled: {name}={v!r} is not built with prompt-lookup decoding (tokens only, one "
                                              "sample per prompt, no beams)")
        if refused:
            raise TypeError(f"generate_lookup_sampled: unexpected arguments {sorted(refused)}")
        if do_sample and not (float(temperature) > 0 and float(top_p) > 0):
            raise ValueError("generate_lookup_sampled: temperature and top_p must be > 0")
        if repetition_penalty is not None and not float(repetition_penalty) > 0:
            raise ValueError("generate_lookup_sampled: repetition_penalty has to be a strictly positive float")
        return self._lookup_call("sv_generate_lookup_sampled", embeds, max_length, num_draft_tokens, max_ngram, min_ngram, lengths, eos_token_id,
                                 pad_token_id, stop_ids, sync_every, on_tokens, min_new_tokens, return_counts, do_sample=bool(do_sample),
                                 temperature=float(temperature), top_k=int(top_k or 0), top_p=float(top_p), seed=int(seed),
                                 repetition_penalty=float(1.0 if repetition_penalty is None else repetition_penalty))

    def _lookup_call(self, entry, embeds, max_length, num_draft_tokens, max_ngram, min_ngram, lengths, eos_token_id, pad_token_id, stop_ids,
                     sync_every, on_tokens, min_new_tokens, return_counts, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                     repetition_penalty=1.0):
        x, lens_arr, B, S0 = self._prompt_form(embeds, lengths)
        sp, max_new, _keep, cb_errors = self._sampling(
            max_length, S0, stop_ids, on_tokens, do_sample=do_sample, temperature=temperature, top_p=top_p, eos_token_id=eos_token_id,
            pad_token_id=pad_token_id, seed=seed, sync_every=sync_every, repetition_penalty=repetition_penalty, top_k=top_k,
            min_new_tokens=min_new_tokens)
        lk = _lib.SvLookup(int(num_draft_tokens), int(max_ngram), int(min_ngram))
        out = torch.empty(B, max_new, dtype=torch.int64, device=x.device)
        n, counts = C.c_int32(0), (C.c_int32 * 3)()
        check(getattr(self.lib, entry)(self._h, _ptr(x), B, lens_arr, S0, C.byref(sp), C.byref(lk), _ptr(out), C.byref(n), counts, _stream()), entry)
        if cb_errors:
            raise cb_errors[0]
        toks = out[:, :n.value]
        if return_counts:
            return toks, dict(steps=counts[0], drafted=counts[1], accepted=counts[2])
        return toks

    def set_lookup_drafts(self, stream) -> None:
        """Test surface (sv_debug_set_lookup_drafts): draft j of sequence b of the generate_lookup / generate_lookup_sampled calls that follow
        is stream[b][n_emit_b + j] instead of the lookup; ``None`` clears it."""
        if stream is None:
            check(self.lib.sv_debug_set_lookup_drafts(self._h, None, 0, 0), "sv_debug_set_lookup_drafts")
            return
        t = torch.as_tensor(stream, dtype=torch.int32).cpu().contiguous()
        if t.dim() == 1:
            t = t.view(1, -1)
        arr = (C.c_int32 * t.numel())(*t.flatten().tolist())
        check(self.lib.sv_debug_set_lookup_drafts(self._h, arr, t.shape[0], t.shape[1]), "sv_debug_set_lookup_drafts")

    def block_table_row(self, row: int) -> List[int]:
        """The block-table row of a decode row / slot as the device holds it (sv_debug_block_table)."""
        buf = (C.c_int32 * 4096)()
        n = self.lib.sv_debug_block_table(self._h, int(row), buf, 4096)
        if n < 0:
            check(n, "sv_debug_block_table")
        return list(buf)[:n]

    def free_pages(self) -> Tuple[int, int]:
        """(free KV pages, pages of the pool) of the host allocator after the last generate call or admit / release (sv_debug_free_pages)."""
        f, t = C.c_int32(0), C.c_int32(0)
        check(self.lib.sv_debug_free_pages(self._h, C.byref(f), C.byref(t)), "sv_debug_free_pages")
        return int(f.value), int(t.value)

    def prompt_passes(self) -> int:
        """Prompt passes (rectangular and ragged, admits included) this engine has run so far (sv_debug_prompt_passes)."""
        n = C.c_int64(0)
        check(self.lib.sv_debug_prompt_passes(self._h, C.byref(n)), "sv_debug_prompt_passes")
        return int(n.value)

    def forward_logits(self, inputs_embeds: torch.Tensor, num_logits_to_keep: int = 0) -> torch.Tensor:
        """Scoring forward: bf16 logits [B, n, vocab] of the last n = num_logits_to_keep positions (0 = all positions)."""
        x = _need(inputs_embeds, torch.bfloat16, "inputs_embeds")
        B, S, D = x.shape
        if D != self.cfg.hidden:
            raise ValueError("inputs_embeds hidden size mismatch")
        n = int(num_logits_to_keep) if num_logits_to_keep and num_logits_to_keep > 0 else S
        out = torch.empty(B, n, self.cfg.vocab, dtype=torch.bfloat16, device=x.device)
        check(self.lib.sv_forward_logits(self._h, _ptr(x), B, S, n, _ptr(out), _stream()), "sv_forward_logits")
        return out

    def forward_logprobs(self, inputs_embeds: torch.Tensor, targets: torch.Tensor, num_logits_to_keep: int = 0,
                         temperature: float = 1.0, entropy: bool = False, argmax: bool = False, top_k: int = 0):
        """Scoring forward without logits: for each of the last n = num_logits_to_keep positions (0 = all) the log-probability of
        targets[b, j] under softmax(logits / temperature), the logits being the bf16 rows `forward_logits` returns, in fp32
        (sv_forward_logprobs).  targets: integer [B, n]; -100 = ignore (log-prob 0).  Device memory does not grow with B * n * vocab.
        ``top_k`` = k in 1..32 (sv_forward_topk) returns a ``TokenTopLogprobs``, which also holds ``top_token_ids`` / ``top_logprobs`` [B, n, k] -- the k most likely ids of every
        position, best first, equal logits by ascending id, and their log-probs; the slot holding the target equals ``logprobs`` bit for bit --
        and ``token_ranks`` [B, n], 1 + the number of ids with a larger logit than the target (0 where the target is -100)."""
        x = _need(inputs_embeds, torch.bfloat16, "inputs_embeds")
        B, S, D = x.shape
        if D != self.cfg.hidden:
            raise ValueError("inputs_embeds hidden size mismatch")
        n = int(num_logits_to_keep) if num_logits_to_keep and num_logits_to_keep > 0 else S
        t, res = self._score_outputs(x, targets, (B, n), "[B, n]", entropy, argmax, top_k)
        if top_k:
            check(self.lib.sv_forward_topk(self._h, _ptr(x), B, S, n, _ptr(t), float(temperature), *map(_ptr, res[:4]), top_k,
                                           *map(_ptr, res[4:]), _stream()), "sv_forward_topk")
        else:
            check(self.lib.sv_forward_logprobs(self._h, _ptr(x), B, S, n, _ptr(t), float(temperature), *map(_ptr, res), _stream()),
                  "sv_forward_logprobs")
        return res

    @staticmethod
    def _score_outputs(x, targets, shape, what, entropy, argmax, top_k):
        """What `forward_logprobs` and `forward_logprobs_ragged` share: the ``top_k`` and ``targets`` checks, the int32 targets and the result
        tuple of empty output tensors of `shape` ([B, n] or [sum(keep)]; the lists one dimension more) -- a ``TokenTopLogprobs`` with ``top_k``."""
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k <= TOPK_MAX:
            raise ValueError(f"top_k must be an int in 0..{TOPK_MAX}, got {top_k!r}")
        if tuple(targets.shape) != tuple(shape):
            raise ValueError(f"targets must be {what} = {list(shape)}, got {tuple(targets.shape)}")
        if targets.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"targets must be int32 or int64, got {targets.dtype}")
        new = lambda dtype, *more: torch.empty(*shape, *more, dtype=dtype, device=x.device)
        res = TokenLogprobs(new(torch.float32), new(torch.float32), new(torch.float32) if entropy else None, new(torch.int32) if argmax else None)
        if top_k:
            res = TokenTopLogprobs(*res, new(torch.int32, top_k), new(torch.float32, top_k), new(torch.int32))
        return _need(targets.to(torch.int32), torch.int32, "targets"), res

    def forward_logprobs_ragged(self, embeds, targets, keep, lengths=None, temperature: float = 1.0, entropy: bool = False,
                                argmax: bool = False, top_k: int = 0):
        """`forward_logprobs` over sequences of different lengths in ONE prompt pass, no padding row computed (sv_forward_logprobs_ragged):
        `embeds` a list of [S_i, D] tensors, or a packed [sum(lengths), D] tensor with `lengths`; keep[b] in 1..S_b = the last rows of sequence b
        that are scored; targets: integer [sum(keep)], each sequence's kept rows back to back in sequence order, -100 = ignore.  Returns
        the result types of `forward_logprobs` with packed tensors ([sum(keep)], lists [sum(keep), k]).  Every sequence's slice holds the
        bits of `forward_logprobs(x_b[None], targets_b[None], keep[b], ...)` on that sequence alone, whatever shares the call with it."""
        x, arr, lens = self._packed(embeds, lengths)
        keep = [int(v) for v in keep]
        if len(keep) != len(lens) or any(not 1 <= k <= n for k, n in zip(keep, lens)):
            raise ValueError(f"keep {keep} must hold one count in 1..length for each of the lengths {lens}")
        t, res = self._score_outputs(x, targets, (sum(keep),), "[sum(keep)]", entropy, argmax, top_k)
        lists = res[4:] if top_k else (None, None, None)
        check(self.lib.sv_forward_logprobs_ragged(self._h, _ptr(x), len(lens), arr, (C.c_int32 * len(keep))(*keep), _ptr(t), float(temperature),
                                                  *map(_ptr, res[:4]), top_k, *map(_ptr, lists), _stream()), "sv_forward_logprobs_ragged")
        return res

    def forward_logprobs_prefixed(self, prefixes, seqs, prefix_of, targets, keep, temperature: float = 1.0, entropy: bool = False,
                                  argmax: bool = False, top_k: int = 0):
        """`forward_logprobs_ragged` over sequences that share prefixes, every prefix through the decoder ONCE (sv_forward_logprobs_prefixed):
        `prefixes` and `seqs` are lists of [n, D] bf16 tensors, sequence b stands for cat(prefixes[prefix_of[b]], seqs[b]); keep[b] in
        1..len_b + 1 = the last rows of that concatenation that are scored (len_b + 1 reaches the prefix's last row, which predicts the first own
        token); targets: integer [sum(keep)] in sequence order, -100 = ignore.  Returns the result types of `forward_logprobs_ragged`.  Every
        sequence's slice holds the bits of `forward_logprobs(cat(prefix, seq)[None], targets_b[None], keep[b], ...)` alone.  A sequence whose
        split-K remainder rows would reach into its prefix is refused (ValueError naming it; `prefix_plan` says so beforehand): score it with
        `forward_logprobs_ragged` on the concatenation.  Every weight format.  No KV page is written: `decode_step` refuses afterwards."""
        px, parr, plens = self._packed(prefixes)
        x, arr, lens = self._packed(seqs)
        prefix_of, keep = [int(v) for v in prefix_of], [int(v) for v in keep]
        if len(prefix_of) != len(lens) or any(not 0 <= u < len(plens) for u in prefix_of):
            raise ValueError(f"prefix_of {prefix_of} must hold one index in 0..{len(plens) - 1} for each of the {len(lens)} sequences")
        if len(keep) != len(lens) or any(not 1 <= k <= n + 1 for k, n in zip(keep, lens)):
            raise ValueError(f"keep {keep} must hold one count in 1..length + 1 for each of the lengths {lens}")
        t, res = self._score_outputs(x, targets, (sum(keep),), "[sum(keep)]", entropy, argmax, top_k)
        lists = res[4:] if top_k else (None, None, None)
        ints = lambda v: (C.c_int32 * len(v))(*v)
        check(self.lib.sv_forward_logprobs_prefixed(self._h, _ptr(px), len(plens), parr, _ptr(x), len(lens), arr, ints(prefix_of), ints(keep), _ptr(t),
                                                    float(temperature), *map(_ptr, res[:4]), top_k, *map(_ptr, lists), _stream()),
              "sv_forward_logprobs_prefixed")
        return res

    def prefix_refused(self, prefix_lengths, lengths, prefix_of) -> List[int]:
        """The sequences `forward_logprobs_prefixed` would refuse on this engine: those whose split-K remainder rows would reach into their
        prefix at one of the decoder's four projections (`prefix_plan`; host arithmetic).  Each one is a property of its own (Pl, len) alone."""
        c = self.cfg
        D, F, dh = c.hidden, c.n_inner, c.hidden // c.n_head
        qkv = c.n_head * dh + 2 * max(int(c.n_kv_head), 1) * dh
        proj = ((qkv, D, "none"), (D, D, "none"), (F, D, "gelu_tanh"), (D, F, "none"))
        seen: Dict[Tuple[int, int], bool] = {}
        out = []
        for b, (n, u) in enumerate(zip(lengths, prefix_of)):
            key = (int(prefix_lengths[int(u)]), int(n))
            if key not in seen:
                seen[key] = any(prefix_plan([key[0]], [key[1]], [0], N, K, act)["refused"] is not None for N, K, act in proj)
            if seen[key]:
                out.append(b)
        return out

    def set_score_chunk_rows(self, rows: int) -> None:
        """Rows per lm_head chunk of `forward_logprobs` (a multiple of 256; 0 = default).  Test surface: the outputs do not depend on it."""
        check(self.lib.sv_debug_set_score_chunk_rows(self._h, int(rows)), "sv_debug_set_score_chunk_rows")

    def decode_step(self, tokens: torch.Tensor) -> torch.Tensor:
        tokens = _need(tokens.to(torch.int32), torch.int32, "tokens")
        B = tokens.numel()
        logits = torch.empty(B, self.cfg.vocab, dtype=torch.float32, device=tokens.device)
        check(self.lib.sv_decode_step(self._h, _ptr(tokens), B, _ptr(logits), _stream()), "sv_decode_step")
        return logits

    def generate(self, inputs_embeds: torch.Tensor, max_length: int, do_sample: bool = False,
                 temperature: float = 1.0, top_p: float = 1.0, eos_token_id: int = 0, pad_token_id: int = 0,
                 stop_ids: Optional[Sequence[int]] = None, seed: int = 0, sync_every: int = 32,
                 repetition_penalty: float = 1.0, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping=False, top_k: int = 0, on_tokens=None, min_new_tokens: int = 0,
                 scores_out: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None,
                 return_outputs: bool = False, lengths: Optional[Sequence[int]] = None, n_samples: int = 1,
                 logits_processors=None, token_stats: bool = False, token_topk=None):
        """HF ``generate`` semantics for inputs_embeds: returns ONLY the new tokens, int64 [B, N].
        ``lengths``: the ragged form -- inputs_embeds is packed [sum(lengths), D], one prompt pass for all of them, ``max_length`` counts from
        the longest prompt (see ``generate_ragged``).
        ``num_beams`` > 1 runs HF's beam search on device (``early_stopping``: False, True or "never"); with
        ``do_sample`` it is HF's beam-sample.  ``top_k`` (0 = off) is HF's TopKLogitsWarper, applied before top-p.
        ``on_tokens(tokens [B, n] int64 cpu, first_col)``: streaming callback, called every ``sync_every`` steps with the
        columns that became final and once more at the end.  ``min_new_tokens``: HF's MinLengthLogitsProcessor after the
        prompt length has been subtracted from ``min_length`` (EOS cannot be chosen before that many new tokens).
        ``n_samples`` > 1: that many continuations of every prompt from ONE prompt pass (sv_generate_shared, see ``generate_shared``); the
        outputs have B * n_samples rows, row b * n_samples + j = sample j of prompt b.
        Per-step outputs (sv_generate_ex): ``scores_out`` / ``logits_out`` are fp32 device tensors [max_new, rows, ld] (rows = B, or
        B * num_beams under beam search; ld >= vocab) that receive HF's processed scores / raw logits of every generated column.
        ``return_outputs=True`` returns a dict {"sequences", "n_generated"} plus, under beam search, "sequences_scores" [B] and
        "beam_indices" [B, n] int64 instead of the bare token tensor.
        ``logits_processors``: what ``logits_processors(...)`` returns; the call then goes through sv_generate_processed (see ``generate_processed``).
        ``token_stats=True`` (sv_generate_stats; greedy and sampling, not beam search): the call returns the ``return_outputs`` dict with three
        more fp32 device tensors [rows, n_generated] -- "token_logprobs" (log_softmax(raw logits / T) at the emitted token, T = temperature when
        do_sample, else 1), "token_logprobs_processed" (log_softmax of the processed scores at it: HF's compute_transition_scores with
        normalize_logits=True) and "token_entropies" (entropy of softmax(raw logits / T)); 0 after a row has finished.  The tokens are those of
        the call without it; one more launch per decode step (two with a token ban or min_new_tokens), no [rows, vocab] output.  A tuple of
        those three names instead of True asks for them alone: without "token_logprobs_processed" the launch skips the warper thresholds and
        the second sweep of the row.
        ``token_topk=k`` or ``dict(k=, source="raw" | "processed", rank=True)`` (sv_generate_topk; k in 1..32, greedy and sampling, alone or with
        ``token_stats``): the dict gains "top_token_ids" int32 and "top_logprobs" fp32 [rows, n_generated, k] -- the k most likely ids of every
        step's distribution, best first, equal values by ascending id, (-1, -inf) where fewer than k exist -- and, with ``rank``,
        "token_ranks" int32 [rows, n_generated] = 1 + the ids more likely than the emitted one.  "raw" is the distribution of "token_logprobs",
        "processed" that of "token_logprobs_processed"; the slot of the emitted id equals that statistic bit for bit.  After a row has
        finished: -1 / 0 / 0.  "raw" with ``rank`` and a processor that rewrites the row (a token ban, min_new_tokens) is a ValueError: the raw
        list is then taken before the token is known -- ask for "processed", or rank=False."""
        tk_req = None
        if token_topk is not None and token_topk is not False:
            tk_req = token_topk_request(token_topk)
            if int(num_beams) > 1:
                raise ValueError("token_topk with num_beams > 1 is not built (beam search reports sequences_scores; beam rows reorder)")
        x, lens_arr, B, S0 = self._prompt_form(inputs_embeds, lengths)
        G = int(n_samples)
        if G < 1:
            raise ValueError(f"n_samples must be >= 1, got {n_samples}")
        lp = None
        if logits_processors is not None:
            lp, _lp_keep = logits_processors              # the struct and the host arrays its pointers refer to
            if int(num_beams) > 1:
                raise ValueError("no_repeat_ngram_size / bad_words_ids / min_p with num_beams > 1 is not built")
        if token_stats and int(num_beams) > 1:
            raise ValueError("token_stats with num_beams > 1 is not built (beam search reports sequences_scores; beam rows reorder)")
        n_prompts = B
        if G > 1 and int(num_beams) > 1:
            raise NotImplementedError("n_samples > 1 under beam search (num_beams > 1) is not built")
        if G > 1:
            n_prompts, B = B, B * G                     # B: the decode rows from here on
        sp, max_new, _keep, cb_errors = self._sampling(
            max_length, S0, stop_ids, on_tokens, do_sample=do_sample, temperature=temperature, top_p=top_p, eos_token_id=eos_token_id,
            pad_token_id=pad_token_id, seed=seed, sync_every=sync_every, repetition_penalty=repetition_penalty, num_beams=num_beams,
            length_penalty=length_penalty, early_stopping=early_stopping, top_k=top_k, min_new_tokens=min_new_tokens)
        out = torch.empty(B, max_new, dtype=torch.int64, device=x.device)
        n = C.c_int32(0)
        # a call that asks for nothing beyond the tokens passes no sv_generate_outputs (and takes no beam-search host buffers)
        need_outs = not (scores_out is None and logits_out is None and not return_outputs and not token_stats and tk_req is None)
        rows = B * int(num_beams) if int(num_beams) > 1 else B
        outs = _lib.SvGenerateOutputs()
        ld = None
        for name, t in (("scores_out", scores_out), ("logits_out", logits_out)):
            if t is None:
                continue
            if t.is_cuda and not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous (the engine writes into it)")
            t = _need(t, torch.float32, name)
            if t.dim() != 3 or t.shape[0] < max_new or t.shape[1] != rows or t.shape[2] < self.cfg.vocab:
                raise ValueError(f"{name} must be [>= {max_new}, {rows}, >= {self.cfg.vocab}] fp32, got {list(t.shape)}")
            if ld is not None and t.shape[2] != ld:
                raise ValueError("scores_out and logits_out must have the same last dimension")
            ld = t.shape[2]
            setattr(outs, "dev_scores" if name == "scores_out" else "dev_logits", _ptr(t))
        outs.ld = int(ld or 0)
        beam = need_outs and int(num_beams) > 1
        seq_scores = (C.c_float * B)() if beam else None
        beam_idx = (C.c_int64 * (B * max_new))() if beam else None
        if beam:
            outs.host_sequences_scores = C.cast(seq_scores, C.POINTER(C.c_float))
            outs.host_beam_indices = C.cast(beam_idx, C.POINTER(C.c_int64))
        stats, ts, topk, tk = None, None, None, None
        if token_stats:
            names = TOKEN_STATS if token_stats is True else tuple(token_stats)
            if not names or any(k not in TOKEN_STATS for k in names):
                raise ValueError(f"token_stats must be True or a non-empty tuple of {TOKEN_STATS}, got {token_stats!r}")
            stats = {k: torch.empty(B, max_new, dtype=torch.float32, device=x.device) for k in TOKEN_STATS if k in names}
            ts = _lib.SvTokenStats(*[_ptr(stats.get(k)) for k in TOKEN_STATS], max_new)
        if tk_req is not None:
            k, source, want_rank = tk_req
            topk = {"top_token_ids": torch.empty(B, max_new, k, dtype=torch.int32, device=x.device),
                    "top_logprobs": torch.empty(B, max_new, k, dtype=torch.float32, device=x.device)}
            if want_rank:
                topk["token_ranks"] = torch.empty(B, max_new, dtype=torch.int32, device=x.device)
            tk = _lib.SvTokenTopk(k, source, _ptr(topk["top_token_ids"]), _ptr(topk["top_logprobs"]), _ptr(topk.get("token_ranks")), max_new)
        # the entry point is the first whose argument the call has: each takes the arguments of the one below it and one more
        ref = lambda s: C.byref(s) if s is not None else None
        outs = outs if need_outs else None
        group = (n_prompts, lens_arr, S0, G, C.byref(sp))
        if tk is not None:
            name, args = "sv_generate_topk", group + (ref(lp), ref(outs), ref(ts), C.byref(tk))
        elif ts is not None:
            name, args = "sv_generate_stats", group + (ref(lp), ref(outs), C.byref(ts))
        elif lp is not None:
            name, args = "sv_generate_processed", group + (C.byref(lp), ref(outs))
        elif G > 1:
            name, args = "sv_generate_shared", group + (ref(outs),)
        elif lens_arr is not None:
            name, args = "sv_generate_ragged", (B, lens_arr, C.byref(sp), ref(outs))
        elif need_outs:
            name, args = "sv_generate_ex", (B, S0, C.byref(sp), ref(outs))
        else:
            name, args = "sv_generate", (B, S0, C.byref(sp))
        check(getattr(self.lib, name)(self._h, _ptr(x), *args, _ptr(out), C.byref(n), _stream()), name)
        if cb_errors:
            raise cb_errors[0]
        L = n.value
        if not return_outputs and stats is None and topk is None:
            return out[:, :L]
        res = {"sequences": out[:, :L], "n_generated": L}
        if stats is not None:
            res.update({k: v[:, :L] for k, v in stats.items()})
        if topk is not None:
            res.update({k: v[:, :L] for k, v in topk.items()})
        if beam:
            res["sequences_scores"] = torch.tensor(list(seq_scores), dtype=torch.float32)
            res["beam_indices"] = torch.tensor(list(beam_idx), dtype=torch.int64).view(B, max_new)[:, :L].contiguous()
        return res

    # ---- continuous batching: one request per row of the engine's batch (include/starvector_hip.h, sv_cb_*) ----------------
    def cb_admit(self, inputs_embeds: torch.Tensor, requests: Sequence[dict], logprobs: Optional[Sequence] = None) -> List[int]:
        """Prompt pass of len(requests) new requests (inputs_embeds [n, S0, D] bf16, equal prompt length) into free slots while
        the live slots keep their KV cache; samples their first token.  Each request: dict(max_new_tokens, do_sample=False,
        temperature=1, top_p=1, top_k=0, seed=0, eos_token_id=0, pad_token_id=0, stop_ids=None, repetition_penalty=1,
        min_new_tokens=0), plus the vLLM-semantics keys (include/starvector_hip.h, ABI 9; they need semantics="vllm"):
        presence_penalty=0, frequency_penalty=0, min_p=0, prompt_ids=None, logit_bias=None ({id: bias}), stop_any_ids=None.
        ``logprobs``: one entry per request, None or dict(k=0..32, source="raw" | "processed") -- the request records, for every token it
        emits, the token's log-prob and rank and the k most likely ids (`cb_read_logprobs`; sv_cb_admit_logprobs).  None, or every entry
        None: the call below, unchanged.
        Returns the slot ids.  Raises StarVectorBusy when slots or KV pages are short."""
        if logprobs is not None and any(l is not None for l in logprobs):
            seqs = list(inputs_embeds) if isinstance(inputs_embeds, (list, tuple)) else list(_need(inputs_embeds, torch.bfloat16, "inputs_embeds"))
            return self.cb_admit_shared(seqs, None, list(range(len(seqs))), requests, logprobs=logprobs)
        if isinstance(inputs_embeds, (list, tuple)):
            # per-request embeddings [S_i, D] of different lengths: ONE ragged prompt pass for all of them (sv_cb_admit_ragged)
            x, lens_arr, lens = self._packed(inputs_embeds)
            n = len(lens)
            if n != len(requests):
                raise ValueError("inputs_embeds / requests mismatch")
            arr, keep = cb_requests(requests)
            slots = (C.c_int32 * n)()
            check(self.lib.sv_cb_admit_ragged(self._h, _ptr(x), n, lens_arr, arr, slots, _stream()), "sv_cb_admit_ragged")
            del keep
            return list(slots)
        x = _need(inputs_embeds, torch.bfloat16, "inputs_embeds")
        n, S0, D = x.shape
        if D != self.cfg.hidden or n != len(requests):
            raise ValueError("inputs_embeds / requests mismatch")
        arr, keep = cb_requests(requests)
        slots = (C.c_int32 * n)()
        check(self.lib.sv_cb_admit(self._h, _ptr(x), n, S0, arr, slots, _stream()), "sv_cb_admit")
        del keep
        return list(slots)

    def cb_admit_shared(self, embeds, lengths, group: Sequence[int], requests: Sequence[dict], logprobs: Optional[Sequence] = None) -> List[int]:
        """Group admit (sv_cb_admit_shared): ``embeds`` a list of [S_u, D] prompts (``lengths`` None) or a packed tensor with ``lengths``;
        request i samples prompt ``group[i]`` with its own parameters (the dicts of ``cb_admit``).  ONE prompt pass over the prompts; the
        requests of a prompt share its full KV pages.  Prompts may come in any order here: they are renumbered in the order their first
        request appears, as the C entry point wants them.  ``logprobs``: as in `cb_admit`, one entry per request (every sample of a prompt may
        ask for its own k).  Returns the slot ids; raises StarVectorBusy when slots or pages are short."""
        group = [int(g) for g in group]
        if len(group) != len(requests) or not group:
            raise ValueError("group / requests mismatch")
        if lengths is None:
            seqs = [t.reshape(-1, t.shape[-1]) for t in embeds]
        else:
            seqs = list(torch.split(embeds, [int(v) for v in lengths], dim=0))
        if min(group) < 0 or max(group) >= len(seqs):
            raise ValueError(f"group entries must lie in [0, {len(seqs)})")
        order = list(dict.fromkeys(group))               # prompts in the order of their first request
        if len(order) != len(seqs):
            raise ValueError("every prompt needs at least one request")
        rank = {u: k for k, u in enumerate(order)}
        x, lens_arr, lens = self._packed([seqs[u] for u in order])
        n = len(group)
        arr, keep = cb_requests(requests)
        slots = (C.c_int32 * n)()
        grp = (C.c_int32 * n)(*[rank[g] for g in group])
        lps = cb_logprobs(requests, logprobs)
        if lps is None:
            check(self.lib.sv_cb_admit_shared(self._h, _ptr(x), len(lens), lens_arr, n, grp, arr, slots, _stream()), "sv_cb_admit_shared")
        else:
            check(self.lib.sv_cb_admit_logprobs(self._h, _ptr(x), len(lens), lens_arr, n, grp, arr, lps, slots, _stream()), "sv_cb_admit_logprobs")
            for s_, l in zip(slots, lps):
                self._cb_lp_k[int(s_)] = int(l.k) if l.enable else None
        del keep
        return list(slots)

    def cb_read_logprobs(self, slot: int, first: int, count: int):
        """Columns [first, first + count) of a recording slot's record (sv_cb_read_logprobs), host tensors: (token log-probs fp32 [count],
        ranks int32 [count], ids int32 [count, k], log-probs fp32 [count, k]) with the slot's own k.  Only columns the slot has emitted
        exist; a slot that records nothing raises ValueError."""
        k = self._cb_lp_k.get(int(slot)) or 0
        n = max(int(count), 1)
        lp, rk = (C.c_float * n)(), (C.c_int32 * n)()
        ids, lps = (C.c_int32 * max(n * k, 1))(), (C.c_float * max(n * k, 1))()
        check(self.lib.sv_cb_read_logprobs(self._h, int(slot), int(first), int(count), lp, rk, ids, lps), "sv_cb_read_logprobs")
        count = int(count)
        return (torch.tensor(list(lp)[:count], dtype=torch.float32), torch.tensor(list(rk)[:count], dtype=torch.int32),
                torch.tensor(list(ids)[:count * k], dtype=torch.int32).view(count, k),
                torch.tensor(list(lps)[:count * k], dtype=torch.float32).view(count, k))

    def cb_step(self, n_steps: int = 8) -> int:
        """n_steps decode steps for every live slot (hipGraph replay); returns how many slots are still generating."""
        live = C.c_int32(0)
        check(self.lib.sv_cb_step(self._h, int(n_steps), C.byref(live), _stream()), "sv_cb_step")
        return live.value

    def cb_poll(self):
        """(live flags, tokens emitted so far) per slot, two lists of max_batch ints."""
        n = self.cfg.max_batch
        lv, st = (C.c_int32 * n)(), (C.c_int32 * n)()
        check(self.lib.sv_cb_poll(self._h, lv, st, n), "sv_cb_poll")
        return list(lv), list(st)

    def cb_read(self, slot: int, first: int, count: int) -> torch.Tensor:
        buf = (C.c_int64 * max(count, 1))()
        check(self.lib.sv_cb_read(self._h, int(slot), int(first), int(count), buf), "sv_cb_read")
        return torch.tensor(list(buf)[:count], dtype=torch.int64)

    def cb_release(self, slot: int) -> None:
        check(self.lib.sv_cb_release(self._h, int(slot)), "sv_cb_release")

    def cb_reset(self) -> None:
        check(self.lib.sv_cb_reset(self._h), "sv_cb_reset")

    def cb_set_lookup(self, num_draft_tokens: int, max_ngram: int = 0, min_ngram: int = 0) -> None:
        """Prompt-lookup drafting for the continuous batch (sv_cb_set_lookup): with num_draft_tokens = K > 0 every slot owns K + 1 decode rows,
        a `cb_step` step verifies up to K drafted tokens per slot and emits 1 .. K + 1, and the batch holds max_batch // (K + 1) slots.  Every
        request's tokens, finish and record are those of a batch with drafting off.  0 = off (the default).  Only while no batch is active:
        before the first admit or after `cb_reset` (RuntimeError otherwise); the setting stays across `cb_reset`."""
        lk = _lib.SvLookup(int(num_draft_tokens), int(max_ngram), int(min_ngram))
        check(self.lib.sv_cb_set_lookup(self._h, C.byref(lk)), "sv_cb_set_lookup")

    def cb_lookup_counts(self, slot: int = -1) -> dict:
        """{steps, drafted, accepted} of a slot since its admit; slot = -1: the batch's totals (steps: one per live slot and step)."""
        c = (C.c_int32 * 3)()
        check(self.lib.sv_cb_lookup_counts(self._h, int(slot), c), "sv_cb_lookup_counts")
        return {"steps": c[0], "drafted": c[1], "accepted": c[2]}

    def cb_set_prefix_cache(self, on: bool) -> None:
        """The continuous batch's prefix cache (sv_cb_set_prefix_cache): with it on, an admit reuses the full 64-row KV pages earlier admits of
        the batch computed for the same leading prompt rows -- found by digests of the embedding rows, kept resident after their requests were
        released while no admit needs the pages -- and computes only the rows behind them.  Every request's tokens, finish and record are
        those of a batch with the cache off.  Off by default.  Only while no batch is active (RuntimeError otherwise); the setting stays
        across `cb_reset`, the cached pages do not.  NotImplementedError on an fp8 KV cache."""
        check(self.lib.sv_cb_set_prefix_cache(self._h, 1 if on else 0), "sv_cb_set_prefix_cache")

    def cb_prefix_cache_info(self) -> dict:
        """{lookups: full prompt pages looked up, reused, resident: pages in the table, unheld: of those without a holder, evictions} since
        the batch began (sv_cb_prefix_cache_info); all zero while the cache is off."""
        c = (C.c_int64 * 5)()
        check(self.lib.sv_cb_prefix_cache_info(self._h, c), "sv_cb_prefix_cache_info")
        return {"lookups": c[0], "reused": c[1], "resident": c[2], "unheld": c[3], "evictions": c[4]}

    def cb_set_lookup_drafts(self, streams) -> None:
        """Test surface (sv_debug_cb_set_lookup_drafts): draft j of slot s < len(streams) of the drafting batch admitted next is
        streams[s][step_s + j] instead of the lookup (rows of equal length; nothing is drafted beyond them).  None clears it."""
        if streams is None:
            check(self.lib.sv_debug_cb_set_lookup_drafts(self._h, None, 0, 0), "sv_debug_cb_set_lookup_drafts")
            return
        t = torch.as_tensor(streams, dtype=torch.int32).contiguous()
        if t.dim() != 2 or t.numel() == 0:
            raise ValueError("streams must be [n, ld] ids")
        arr = (C.c_int32 * t.numel())(*t.flatten().tolist())
        check(self.lib.sv_debug_cb_set_lookup_drafts(self._h, arr, t.shape[0], t.shape[1]), "sv_debug_cb_set_lookup_drafts")

    def beam_history(self):
        """(parent beams, tokens), each int32 [n_steps, batch * num_beams], of the last beam-search ``generate``."""
        n, rows = C.c_int32(0), C.c_int32(0)
        check(self.lib.sv_beam_history(self._h, None, None, 0, C.byref(n), C.byref(rows)), "sv_beam_history")
        par, tok = (C.c_int32 * (n.value * rows.value))(), (C.c_int32 * (n.value * rows.value))()
        check(self.lib.sv_beam_history(self._h, par, tok, n.value, C.byref(n), C.byref(rows)), "sv_beam_history")
        shape = (n.value, rows.value)
        return torch.tensor(list(par), dtype=torch.int32).view(shape), torch.tensor(list(tok), dtype=torch.int32).view(shape)

    def mem_free_bytes(self) -> int:
        """Free memory on the engine's GPU (what a generate call with per-step outputs checks its slabs against)."""
        return int(torch.cuda.mem_get_info(self.device)[0])

    def last_timing(self) -> Dict[str, float]:
        buf = (C.c_double * 4)()
        check(self.lib.sv_last_timing(self._h, buf), "sv_last_timing")
        return {"ttft_ms": buf[0], "decode_ms": buf[1], "decode_steps": buf[2], "graph": bool(buf[3]), "graph_steps": int(buf[3])}

    def step_plan(self) -> Dict[str, int]:
        """What the last generate() call's decode step actually was (sv_debug_step_plan): kernel nodes of its captured graph and which
        of the fused launches ran -- the engine's own decisions, not a re-derivation from the configuration."""
        buf = (C.c_int32 * 4)()
        check(self.lib.sv_debug_step_plan(self._h, buf), "sv_debug_step_plan")
        return {"graph_kernel_nodes": int(buf[0]), "rowln_cattn_fused": bool(buf[1]), "greedy_in_lm_head": bool(buf[2]), "mlp_fused": bool(buf[3])}

    def set_exp(self, mask: int) -> None:
        """A/B switches of the live engine: a mask of `Exp` members, 0 = the product path (in-process A/B runs: tools/ab_exp.py).
        ValueError for a bit that is no switch; the engine keeps its mask then."""
        check(self.lib.sv_debug_set_exp(self._h, int(mask)), "sv_debug_set_exp")

    def debug_attn_trace(self) -> torch.Tensor:
        """[rows * kv heads * splits, 16] int64 wall-clock stamps (100 MHz) of the decode attention of the middle layer of the last
        step (engine created with SV_ATTN_TRACE=1 in the environment; include/starvector_hip.h, sv_debug_attn_trace)."""
        cap = 8192
        buf = (C.c_int64 * (cap * 16))()
        n = self.lib.sv_debug_attn_trace(self._h, buf, cap)
        if n < 0:
            check(n, "sv_debug_attn_trace")
        return torch.tensor(list(buf[: n * 16]), dtype=torch.int64).view(n, 16)

    def debug_occupy_cus(self, blocks: int, lds_bytes: int = 144 * 1024, ms: int = 300):
        """Test tenant (include/starvector_hip_debug.h, sv_debug_occupy_cus): pin `lds_bytes` of LDS on `blocks` CUs for `ms` milliseconds
        from a stream of its own; returns at once."""
        check(self.lib.sv_debug_occupy_cus(self._h, blocks, lds_bytes, ms), "sv_debug_occupy_cus")

    def debug_xcc_map(self, blocks: int, heavy: bool = False):
        """[blocks] list of XCC_IDs: where the blocks of a 1-D launch of 8-wave blocks ran (heavy: with the decode attention's LDS footprint and
        10 us of residence, so that a grid above the CU count runs in rounds; include/starvector_hip.h, sv_debug_xcc_map)."""
        buf = (C.c_int32 * blocks)()
        check(self.lib.sv_debug_xcc_map(self._h, blocks, 1 if heavy else 0, buf), "sv_debug_xcc_map")
        return list(buf)

    def debug_mlp_trace(self) -> torch.Tensor:
        """[blocks, 8] int64 wall-clock stamps (100 MHz) of the last fused MLP launch of the middle layer (engine created with
        SV_MLP_TRACE=1 in the environment; include/starvector_hip.h, sv_debug_mlp_trace)."""
        buf = (C.c_int64 * (1024 * 8))()
        n = self.lib.sv_debug_mlp_trace(self._h, buf, 1024)
        if n < 0:
            check(n, "sv_debug_mlp_trace")
        return torch.tensor(list(buf[: n * 8]), dtype=torch.int64).view(n, 8)

    def debug_kv_load(self, layer: int, kv: torch.Tensor, lens: Optional[torch.Tensor] = None) -> None:
        """Test surface of the decode attention (include/starvector_hip.h, sv_debug_kv_load): kv [B, S, 2 * n_kv_head * head_dim]
        bf16 (k heads | v heads, K as cached) becomes tokens 0..S-1 of `layer`'s paged KV; every row's position is set to S, or to
        lens[b] (int32 [B], <= S) for a ragged batch."""
        kv = _need(kv, torch.bfloat16, "kv")
        B, S, _ = kv.shape
        if lens is not None:
            lens = _need(lens, torch.int32, "lens")
            if lens.numel() != B or int(lens.max()) > S or int(lens.min()) < 0:
                raise ValueError("lens must be int32 [B] with 0 <= lens[b] <= S")
        check(self.lib.sv_debug_kv_load(self._h, int(layer), _ptr(kv) if S > 0 else C.c_void_p(0), B, S, _ptr(lens), _stream()),
              "sv_debug_kv_load")
        torch.cuda.current_stream().synchronize()          # the caller may free `kv` right away

    def debug_kv_read(self, layer: int, row: int, first: int, count: int) -> torch.Tensor:
        """Tokens [first, first + count) of decode row `row` of `layer` as the attention will see them (sv_debug_kv_read): bf16
        [count, 2 * n_kv_head * head_dim] (k heads | v heads), from a pool of either format."""
        width = 2 * (self.cfg.n_kv_head if self.cfg.arch == "v2" else 1) * (self.cfg.hidden // self.cfg.n_head)
        out = torch.empty(int(count), width, dtype=torch.bfloat16, device=self._dev)
        check(self.lib.sv_debug_kv_read(self._h, int(layer), int(row), int(first), int(count), _ptr(out), _stream()), "sv_debug_kv_read")
        return out

    def debug_kv_gather(self, layer: int, row: int, count: int) -> torch.Tensor:
        """Tokens [0, count) of decode row `row` of `layer` through the extension pass's pages -> rows launch (sv_debug_kv_gather): the
        layout and the bits of `debug_kv_read(layer, row, 0, count)`."""
        width = 2 * (self.cfg.n_kv_head if self.cfg.arch == "v2" else 1) * (self.cfg.hidden // self.cfg.n_head)
        out = torch.empty(int(count), width, dtype=torch.bfloat16, device=self._dev)
        check(self.lib.sv_debug_kv_gather(self._h, int(layer), int(row), int(count), _ptr(out), _stream()), "sv_debug_kv_gather")
        return out

    def debug_attn_decode(self, layer: int, qkv: torch.Tensor, advance: bool = True) -> torch.Tensor:
        """One launch of the decode attention of `layer` for the new token whose c_attn output is qkv [B, QKV] float32 (before
        RoPE); returns [B, n_head * head_dim] bf16 and (advance) steps the positions, so repeated calls walk the sequence."""
        qkv = _need(qkv, torch.float32, "qkv")
        B = qkv.shape[0]
        out = torch.empty(B, self.cfg.hidden, dtype=torch.bfloat16, device=qkv.device)     # n_head * head_dim == hidden
        check(self.lib.sv_debug_attn_decode(self._h, int(layer), _ptr(qkv), B, _ptr(out), int(bool(advance)), _stream()),
              "sv_debug_attn_decode")
        return out

    def debug_attn_decode_slabs(self, layer: int, slabs: torch.Tensor, bias: Optional[torch.Tensor] = None,
                                advance: bool = True) -> torch.Tensor:
        """debug_attn_decode fed as a decode step feeds the launch: slabs [splitk, B, QKV] float32 (the split-K slabs of the c_attn
        GEMM, splitk 1, 2, 4 or 8) and bias [QKV] bf16 (None: zero); the kernel sums the slabs in slab order, then adds the bias."""
        slabs = _need(slabs, torch.float32, "slabs")
        splitk, B = slabs.shape[0], slabs.shape[1]
        if bias is not None:
            bias = _need(bias, torch.bfloat16, "bias")
            if bias.numel() != slabs.shape[2]:
                raise ValueError("bias must be bf16 [QKV]")
        out = torch.empty(B, self.cfg.hidden, dtype=torch.bfloat16, device=slabs.device)   # n_head * head_dim == hidden
        check(self.lib.sv_debug_attn_decode_slabs(self._h, int(layer), _ptr(slabs), splitk, _ptr(bias), B, _ptr(out),
                                                  int(bool(advance)), _stream()), "sv_debug_attn_decode_slabs")
        return out

    def debug_attn_decode_draft(self, layer: int, slabs: torch.Tensor, n_seq: int, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """What a verification step of generate_lookup does around one attention launch (sv_debug_attn_decode_draft): slabs
        [splitk, n_seq * K1, QKV] float32, row s * K1 + j = the c_attn output of sequence s's j-th next token.  The rows of a sequence share its
        pages at positions pos_s + j, every row's K / V is pre-written, ONE attention launch runs over all rows; returns
        [n_seq * K1, n_head * head_dim] bf16 and leaves the engine where K1 advancing ``debug_attn_decode_slabs`` calls leave it."""
        slabs = _need(slabs, torch.float32, "slabs")
        splitk, rows = slabs.shape[0], slabs.shape[1]
        if rows % int(n_seq):
            raise ValueError(f"{rows} rows are not n_seq={n_seq} sequences of equally many rows")
        if bias is not None:
            bias = _need(bias, torch.bfloat16, "bias")
            if bias.numel() != slabs.shape[2]:
                raise ValueError("bias must be bf16 [QKV]")
        out = torch.empty(rows, self.cfg.hidden, dtype=torch.bfloat16, device=slabs.device)
        check(self.lib.sv_debug_attn_decode_draft(self._h, int(layer), _ptr(slabs), splitk, _ptr(bias), int(n_seq), rows // int(n_seq),
                                                  _ptr(out), _stream()), "sv_debug_attn_decode_draft")
        return out

    def profile_decode_step(self, B: int, iters: int = 5) -> Dict[str, Dict[str, float]]:
        """HIP-event time per decode step by kernel class (eager launches of the graph's kernels)."""
        buf = (C.c_double * 10)()
        check(self.lib.sv_profile_decode_step(self._h, B, iters, buf, _stream()), "sv_profile_decode_step")
        names = ["skinny_gemm", "attn_decode", "row_update_ln"]
        res = {n: {"ms_per_step": buf[2 * i], "launches_per_step": buf[2 * i + 1]} for i, n in enumerate(names)}
        res["event_pair_overhead_ms"] = buf[6]
        res["skinny_chain_ms_per_step"] = buf[7]
        res["others_chain_ms_per_step"] = buf[8]
        return res

    TTFT_STAGES = ("encoder_gemm", "encoder_attention", "encoder_rows", "adapter_gemm", "adapter_norm_and_token_gather",
                   "prefill_gemm", "gemm_remainder_rows", "prefill_attention", "prefill_rows", "lm_head", "first_token_select")

    def profile_ttft(self, image: Optional[torch.Tensor], prompt_ids: torch.Tensor, iters: int = 3) -> Dict[str, float]:
        """Where the time to first token goes (include/starvector_hip_debug.h, sv_profile_ttft): ms per stage of ONE pass
        image -> encoder -> adapter -> prompt rows -> prompt pass -> lm_head -> first greedy token, HIP events in front of every
        launch group.  image: bf16 [B,3,S,S] or None (text2svg); prompt_ids: int64 [B, P]."""
        ids = _need(prompt_ids, torch.int64, "prompt_ids")
        B, P = ids.shape
        img = _need(image, torch.bfloat16, "image") if image is not None else None
        buf = (C.c_double * 24)()
        check(self.lib.sv_profile_ttft(self._h, _ptr(img), B, _ptr(ids), P, int(iters), buf, _stream()), "sv_profile_ttft")
        res = {n: buf[2 * i] for i, n in enumerate(self.TTFT_STAGES)}
        res["launches"] = {n: int(round(buf[2 * i + 1])) for i, n in enumerate(self.TTFT_STAGES)}
        res["event_pair_overhead_ms"] = buf[22]
        res["first_to_last_event_ms"] = buf[23]
        return res


def logits_processors(no_repeat_ngram_size=0, bad_words_ids=None, min_p=0.0, vocab: Optional[int] = None):
    """The sv_logits_processors struct of HF's no_repeat_ngram_size / bad_words_ids / min_p and the host arrays its pointers refer to (keep the
    pair alive for the duration of the call).  The limits of include/starvector_hip.h are checked here too -- ValueError, nothing is truncated:
    n-grams of at most 8 ids, at most 64 bad-word sequences of 1..8 ids, every id in [0, vocab), min_p in [0, 1]."""
    n = int(no_repeat_ngram_size or 0)
    if n < 0 or n > _lib.LP_MAX_NGRAM:
        raise ValueError(f"no_repeat_ngram_size {n} unsupported (0..{_lib.LP_MAX_NGRAM})")
    words = [[int(t) for t in w] for w in (bad_words_ids or [])]
    if len(words) > _lib.LP_MAX_BAD_WORDS:
        raise ValueError(f"{len(words)} bad-word sequences (at most {_lib.LP_MAX_BAD_WORDS})")
    for i, w in enumerate(words):
        if not 1 <= len(w) <= _lib.LP_MAX_BAD_WORD_LEN:
            raise ValueError(f"bad-word sequence {i} has {len(w)} ids (1..{_lib.LP_MAX_BAD_WORD_LEN})")
        for t in w:
            if t < 0 or (vocab is not None and t >= int(vocab)):
                raise ValueError(f"bad-word sequence {i}: id {t} outside the vocabulary")
    mp = float(min_p or 0.0)
    if not 0.0 <= mp <= 1.0:
        raise ValueError(f"min_p must lie in [0, 1], got {min_p}")
    lens = (C.c_int32 * max(len(words), 1))(*[len(w) for w in words])
    flat = [t for w in words for t in w]
    ids = (C.c_int32 * max(len(flat), 1))(*flat)
    lp = _lib.SvLogitsProcessors(n, len(words), C.cast(lens, C.POINTER(C.c_int32)) if words else None,
                                 C.cast(ids, C.POINTER(C.c_int32)) if words else None, mp)
    return lp, (lens, ids)


def cb_requests(requests: Sequence[dict]):
    """The sv_cb_request array of `HipEngine.cb_admit`'s request dicts, and the host arrays its pointers refer to (keep them alive
    for the duration of the call)."""
    n = len(requests)
    arr = (_lib.SvCbRequest * n)()
    keep = []
    for i, r in enumerate(requests):
        stops = list(r.get("stop_ids") or [])
        if len(stops) > 16:
            raise ValueError("stop sequence longer than 16 ids")
        a = arr[i]
        a.do_sample = int(bool(r.get("do_sample", False))); a.temperature = float(r.get("temperature", 1.0))
        a.top_p = float(r.get("top_p", 1.0)); a.top_k = int(r.get("top_k", 0) or 0)
        a.seed = int(r.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF; a.max_new_tokens = int(r["max_new_tokens"])
        a.eos_token_id = int(r.get("eos_token_id", 0)); a.pad_token_id = int(r.get("pad_token_id", 0))
        a.min_new_tokens = int(r.get("min_new_tokens", 0) or 0); a.repetition_penalty = float(r.get("repetition_penalty", 1.0) or 1.0)
        a.n_stop = len(stops)
        for k, t in enumerate(stops):
            a.stop_ids[k] = int(t)
        sem = r.get("semantics", "hf")
        if sem not in ("hf", "vllm", 0, 1):
            raise ValueError(f"semantics must be 'hf' or 'vllm', not {sem!r}")
        a.semantics = 1 if sem in ("vllm", 1) else 0
        a.presence_penalty = float(r.get("presence_penalty", 0.0) or 0.0)
        a.frequency_penalty = float(r.get("frequency_penalty", 0.0) or 0.0)
        a.min_p = float(r.get("min_p", 0.0) or 0.0)
        prompt = [int(t) for t in (r.get("prompt_ids") or [])]
        if prompt:
            buf = (C.c_int32 * len(prompt))(*prompt)
            keep.append(buf)
            a.n_prompt_ids, a.prompt_ids = len(prompt), C.cast(buf, C.POINTER(C.c_int32))
        bias = dict(r.get("logit_bias") or {})
        if len(bias) > _lib.CB_MAX_LOGIT_BIAS:
            raise ValueError(f"{len(bias)} logit_bias entries (at most {_lib.CB_MAX_LOGIT_BIAS})")
        if bias:
            ids = (C.c_int32 * len(bias))(*[int(k) for k in bias])
            vals = (C.c_float * len(bias))(*[float(v) for v in bias.values()])
            keep += [ids, vals]
            a.n_logit_bias = len(bias)
            a.logit_bias_ids, a.logit_bias_values = C.cast(ids, C.POINTER(C.c_int32)), C.cast(vals, C.POINTER(C.c_float))
        anys = [int(t) for t in (r.get("stop_any_ids") or [])]
        if len(anys) > _lib.CB_MAX_STOP_ANY:
            raise ValueError(f"{len(anys)} stop_any_ids (at most {_lib.CB_MAX_STOP_ANY})")
        a.n_stop_any = len(anys)
        for k, t in enumerate(anys):
            a.stop_any_ids[k] = t
    return arr, keep


def cb_logprobs(requests: Sequence[dict], logprobs: Optional[Sequence]):
    """The sv_cb_logprobs array parallel to `cb_requests(requests)`: entry i from logprobs[i] = None | dict(k=, source=) (source 0 / "raw",
    1 / "processed"; default: processed for a vLLM-semantics request, whose raw row no longer exists, raw otherwise).  None when nobody asks."""
    if logprobs is None or all(l is None for l in logprobs):
        return None
    if len(logprobs) != len(requests):
        raise ValueError("one logprobs entry per request")
    arr = (_lib.SvCbLogprobs * len(requests))()
    for i, (r, l) in enumerate(zip(requests, logprobs)):
        if l is None:
            continue
        vl = r.get("semantics", "hf") in ("vllm", 1)
        src = l.get("source")
        src = ("processed" if vl else "raw") if src is None else src
        if src not in ("raw", "processed", 0, 1):
            raise ValueError(f"logprobs source must be 'raw' or 'processed', not {src!r}")
        arr[i].enable, arr[i].k, arr[i].source = 1, int(l.get("k", 0) or 0), 1 if src in ("processed", 1) else 0
    return arr


def token_callback(on_tokens):
    """Wrap ``on_tokens(tokens [B, n] int64 cpu, first_col)`` as an `sv_token_callback`.  An exception cannot unwind through
    the C frames of `sv_generate` (ctypes would print and drop it): the first one is kept, later bursts are skipped, and
    the caller re-raises it when `sv_generate` has returned.  Returns (C callback, list that receives the exception)."""
    errors = []

    def _cb(_user, ptr, batch, first_col, n_cols):
        if errors:
            return
        try:
            flat = torch.tensor(ptr[: batch * n_cols], dtype=torch.int64).view(batch, n_cols)
            on_tokens(flat, int(first_col))
        except BaseException as ex:                        # noqa: BLE001 -- re-raised by the caller
            errors.append(ex)

    return _lib.TOKEN_CALLBACK(_cb), errors


def _early_code(early_stopping) -> int:
    """HF's early_stopping: False | True | "never"  ->  0 | 1 | 2."""
    if early_stopping is True or early_stopping is False or early_stopping is None:
        return int(bool(early_stopping))
    if early_stopping == "never":
        return 2
    raise ValueError("`early_stopping` must be a boolean or 'never'")   # HF's own check


class HipBeamScorer:
    """The device-side beam-search bookkeeping on its own (what HF's ``_beam_search`` does between two forward passes).
    ``step(logits)`` consumes the [batch * num_beams, vocab] fp32 logits of one step and returns
    (done, parent_rows, tokens, running_scores); ``finalize()`` returns (tokens [batch, L], scores [batch])."""

    def __init__(self, batch: int, num_beams: int, vocab: int, max_new: int, eos_token_id: int, pad_token_id: int,
                 length_penalty: float = 1.0, early_stopping=False, repetition_penalty: float = 1.0,
                 stop_ids: Optional[Sequence[int]] = None, do_sample: bool = False, temperature: float = 1.0,
                 top_p: float = 1.0, top_k: int = 0, seed: int = 0, min_new_tokens: int = 0, capture=None):
        """``capture``: None, or (scores, logits) -- fp32 [max_new, batch * num_beams, ld >= vocab] tensors of one shape (either may be None):
        every step also writes its processed log-probs and raw rows there (sv_debug_beam_set_capture: beam_capture_kernel)."""
        self.lib = _lib.load()
        stops = list(stop_ids) if stop_ids else []
        arr = (C.c_int32 * max(len(stops), 1))(*stops) if stops else None
        cfg = _lib.SvBeamConfig(int(batch), int(num_beams), int(vocab), int(max_new), int(eos_token_id),
                                int(pad_token_id), _early_code(early_stopping), float(length_penalty),
                                float(repetition_penalty), len(stops),
                                C.cast(arr, C.POINTER(C.c_int32)) if stops else None, int(bool(do_sample)),
                                float(temperature), float(top_p), int(top_k or 0), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                max(int(min_new_tokens or 0), 0))
        self._h = C.c_void_p()
        self.rows, self.batch, self.vocab, self.max_new = batch * num_beams, batch, vocab, max_new
        check(self.lib.sv_beam_create(C.byref(cfg), C.byref(self._h)), "sv_beam_create")
        self._capture = None
        if capture is not None:
            self.set_capture(*capture)

    def set_capture(self, scores=None, logits=None):
        """The steps that follow write slab t of ``scores`` / ``logits`` (see ``capture`` above); both None: cleared."""
        outs = [o for o in (scores, logits) if o is not None]
        for o in outs:
            if not o.is_cuda or o.dtype != torch.float32 or o.dim() != 3 or not o.is_contiguous() or o.shape != outs[0].shape or \
                    o.shape[1] != self.rows:
                raise ValueError("capture slabs must be contiguous fp32 CUDA tensors [max_new, batch * num_beams, ld] of one shape")
        ld, steps = (outs[0].shape[2], outs[0].shape[0]) if outs else (0, 0)
        check(self.lib.sv_debug_beam_set_capture(self._h, _ptr(scores), _ptr(logits), ld, steps), "sv_debug_beam_set_capture")
        self._capture = (scores, logits)                 # the slabs outlive the steps

    def step(self, logits: torch.Tensor):
        x = _need(logits, torch.float32, "logits")
        if x.shape != (self.rows, self.vocab):
            raise ValueError(f"logits must be [{self.rows}, {self.vocab}]")
        done = C.c_int32(0)
        par, tok, sc = (C.c_int32 * self.rows)(), (C.c_int32 * self.rows)(), (C.c_float * self.rows)()
        check(self.lib.sv_beam_step(self._h, _ptr(x), x.stride(0), C.byref(done), par, tok, sc, _stream()), "sv_beam_step")
        return bool(done.value), torch.tensor(list(par)), torch.tensor(list(tok)), torch.tensor(list(sc))

    def finalize(self):
        toks = (C.c_int64 * (self.batch * self.max_new))()
        sc = (C.c_float * self.batch)()
        n = C.c_int32(0)
        check(self.lib.sv_beam_finalize(self._h, toks, C.byref(n), sc, _stream()), "sv_beam_finalize")
        t = torch.tensor(list(toks), dtype=torch.int64).view(self.batch, self.max_new)[:, : n.value].contiguous()
        return t, torch.tensor(list(sc))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.sv_beam_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bench_linear(M: int, N: int, K: int, act: str = "none", residual: bool = False, iters: int = 10) -> float:
    """Average microseconds of one big-M MFMA GEMM launch on pseudo-random operands (HIP events)."""
    lib = _lib.load()
    us = C.c_double(0.0)
    check(lib.sv_bench_linear(M, N, K, _lib.ACT[act], int(residual), iters, C.byref(us), _stream()), "sv_bench_linear")
    return us.value


# ---- single operators (used by the parity tests; one per SURVEY.md section 8a row) ----------------
def op_layernorm(x, gamma, beta, eps=1e-5):
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); M, D = x.shape
    y = torch.empty_like(x)
    check(lib.sv_op_layernorm(_ptr(x), _ptr(_need(gamma, torch.bfloat16, "gamma")),
                              _ptr(_need(beta, torch.bfloat16, "beta")), _ptr(y), M, D, eps, _stream()))
    return y


def op_linear(x, W, bias=None, residual=None, act="none", out_f32=False):
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); W = _need(W, torch.bfloat16, "W")
    M, K = x.shape; N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    b = _need(bias, torch.bfloat16, "bias") if bias is not None else None
    r = _need(residual, torch.bfloat16, "residual") if residual is not None else None
    check(lib.sv_op_linear(_ptr(x), _ptr(W), _ptr(b), _ptr(r), _ptr(y), M, N, K, _lib.ACT[act], int(out_f32), _stream()))
    return y


def set_gemm_form(form: int) -> None:
    """-1: the tuned choice (default); 0 / 1: every big-M GEMM launch of the process takes 128^2 tiles / 256^2 tiles, rows not peeled;
    2: 256^2 tiles + the row remainder through the tail kernel; 3: every row through the one-wave-per-tile kernel (with a sequence
    structure: the rows a sequence leaves over its tiles through the split-K remainder kernel as in every form)
    (sv_debug_set_gemm_form).  Same bits every way; test and A/B surface."""
    check(_lib.load().sv_debug_set_gemm_form(int(form)))


def set_linear_seq_rows(seq_rows: int) -> None:
    """Sequence structure `linear` / `bench_linear` hand to the big-M dispatch (sv_debug_set_linear_seq_rows): S > 0 = the rows are
    sequences of S rows (where the per-sequence form holds for the projection, the rows a sequence leaves over its 256-row tiles take
    the split-K remainder kernel), S < 0 = the rows are the last rows of sequences of |S| rows, 0 = none (default)."""
    check(_lib.load().sv_debug_set_linear_seq_rows(int(seq_rows)))


def gemm_seq_form(S: int, N: int, K: int, act: str = "none") -> bool:
    """Does the projection (N, K, act) take the per-sequence remainder form for sequences of S rows (sv_debug_gemm_seq_form; host arithmetic)?"""
    rc = _lib.load().sv_debug_gemm_seq_form(int(S), int(N), int(K), _lib.ACT[act])
    if rc < 0:
        check(rc, "sv_debug_gemm_seq_form")
    return rc == 1


def ragged_plan(lengths: Sequence[int], N: int, K: int, act: str = "none", q_tile: int = 32) -> Dict[str, object]:
    """What the ragged prompt pass decides for sequences of these lengths at the projection (N, K, act) (sv_debug_ragged_plan; host
    arithmetic): the packed rows that take the split-K remainder kernel, the sequences whose last row is one of them, and the sizes of
    the attention / KV-write block lists."""
    lens = [int(v) for v in lengths]
    B = len(lens)
    cap = max(3 * B, 1)
    rows, last, out = (C.c_int32 * cap)(), (C.c_int32 * cap)(), (C.c_int32 * 4)()
    check(_lib.load().sv_debug_ragged_plan((C.c_int32 * max(B, 1))(*lens), B, int(N), int(K), _lib.ACT[act], int(q_tile), rows, last, cap, out),
          "sv_debug_ragged_plan")
    return {"rows": list(rows)[: out[0]], "last": list(last)[: out[1]], "attn_blocks": out[2], "kv_blocks": out[3]}


def extend_plan(contexts: Sequence[int], lengths: Sequence[int], totals: Optional[Sequence[int]], N: int, K: int, act: str = "none",
                q_tile: int = 32, budget: int = 0) -> List[Dict[str, object]]:
    """What an extension call decides at the projection (N, K, act) under a row budget (sv_debug_extend_plan; host arithmetic, no GPU): one
    dict per pass -- "seqs" [(b, context before the pass, rows, first packed row)], "rows" the packed rows that take the split-K remainder
    kernel, "tiles" [(b, query tile)] of the attention, "groups" [(b, 32-token group)] the page writer touches, "fin" the sequences that reach
    their total length."""
    cx, ln = [int(v) for v in contexts], [int(v) for v in lengths]
    tl = None if totals is None else [int(v) for v in totals]
    if len(cx) != len(ln) or (tl is not None and len(tl) != len(ln)):
        raise ValueError("one context, length and total per sequence")
    ints = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    n = C.c_int32(0)
    args = (ints(cx), ints(ln), ints(tl) if tl is not None else None, len(ln), int(budget), int(N), int(K), _lib.ACT[act], int(q_tile))
    lib = _lib.load()
    rc = lib.sv_debug_extend_plan(*args, (C.c_int32 * 1)(), 0, C.byref(n))
    if rc != 0 and n.value == 0:
        check(rc, "sv_debug_extend_plan")
    out = (C.c_int32 * n.value)()
    check(lib.sv_debug_extend_plan(*args, out, n.value, C.byref(n)), "sv_debug_extend_plan")
    o, i, passes = list(out), 1, []

    def take(width):
        nonlocal i
        cnt = o[i]
        vals = o[i + 1: i + 1 + cnt * width]
        i += 1 + cnt * width
        return vals if width == 1 else [tuple(vals[j: j + width]) for j in range(0, len(vals), width)]
    for _ in range(o[0]):
        passes.append({"seqs": take(4), "rows": take(1), "tiles": take(2), "groups": take(2), "fin": take(1)})
    return passes


def prefix_plan(prefix_lengths: Sequence[int], lengths: Sequence[int], prefix_of: Sequence[int], N: int, K: int, act: str = "none",
                q_tile: int = 32) -> Dict[str, object]:
    """What the shared-prefix scoring pass decides at the projection (N, K, act) (sv_debug_prefix_plan; host arithmetic, no GPU), rows packed
    prefixes first: "row_pos" the solo index of every packed row, "rows" the packed (own) rows that take the split-K remainder kernel,
    "blocks" the (sequence, query tile) pairs of the prefixed attention launch, "refused" the first sequence whose remainder rows would reach
    into its prefix (None: the call is taken)."""
    pl, ln, po = [int(v) for v in prefix_lengths], [int(v) for v in lengths], [int(v) for v in prefix_of]
    if len(po) != len(ln):
        raise ValueError("one prefix index per sequence")
    P, B = len(pl), len(ln)
    total = sum(max(v, 0) for v in pl + ln)
    cap = max(total, 3 * B, 2 * sum(max(n, 0) // max(int(q_tile), 1) + 2 for n in ln), 1)      # (a sequence lists at most len / q_tile + 2 tiles)
    ints = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    pos, rows, blocks, out = (C.c_int32 * cap)(), (C.c_int32 * cap)(), (C.c_int32 * cap)(), (C.c_int32 * 4)()
    check(_lib.load().sv_debug_prefix_plan(ints(pl), P, ints(ln), ints(po), B, int(N), int(K), _lib.ACT[act], int(q_tile), pos, rows, blocks, cap, out),
          "sv_debug_prefix_plan")
    b = list(blocks)[: 2 * out[1]]
    return {"row_pos": list(pos)[: out[3]], "rows": list(rows)[: out[0]], "blocks": list(zip(b[0::2], b[1::2])),
            "refused": None if out[2] < 0 else int(out[2])}


def shared_plan(lengths: Sequence[int], group: Sequence[int], budgets: Sequence[int]) -> Dict[str, object]:
    """The page plan of a shared prompt pass (sv_debug_shared_plan; host arithmetic, no GPU): per request the shared and the private
    block-table entries, and the pages the admit takes in all."""
    U, n = len(lengths), len(group)
    sh, pv, tot = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))(), C.c_int64(0)
    check(_lib.load().sv_debug_shared_plan((C.c_int32 * max(U, 1))(*[int(v) for v in lengths]), U, (C.c_int32 * max(n, 1))(*[int(v) for v in group]),
                                           (C.c_int32 * max(n, 1))(*[int(v) for v in budgets]), n, sh, pv, C.byref(tot)), "sv_debug_shared_plan")
    return {"shared": list(sh)[:n], "private": list(pv)[:n], "total": int(tot.value)}


def set_skinny_form(form: int) -> None:
    """Kernel of the 33..64-row decode GEMMs (sv_debug_set_skinny_form): 0 registers only, 1 LDS ring (default), 2 / 3 its fixed depths."""
    check(_lib.load().sv_debug_set_skinny_form(int(form)))


def skinny_form() -> int:
    """The form `set_skinny_form` left in force, process-wide (creating an engine does not touch it)."""
    return int(_lib.load().sv_debug_skinny_form())


def set_op_col_tiles(col_tiles: int) -> None:
    """Column tiles per block (1..3, 0 = default) of the op-level decode GEMMs at 33..64 rows (sv_debug_set_col_tiles)."""
    check(_lib.load().sv_debug_set_col_tiles(int(col_tiles)))


def tailsplit_launches() -> int:
    """Process-wide count of tail-split launches (StarVector-8B's c_fc at <= 32 rows; sv_debug_tailsplit_launches)."""
    n = C.c_int64(0)
    check(_lib.load().sv_debug_tailsplit_launches(C.byref(n)), "sv_debug_tailsplit_launches")
    return n.value


def cols_rowhalf_launches() -> tuple[int, int]:
    """Process-wide (launches, row halves) of the decode output projection's row-half form (sv_debug_cols_rowhalf_launches)."""
    n, h = C.c_int64(0), C.c_int64(0)
    check(_lib.load().sv_debug_cols_rowhalf_launches(C.byref(n), C.byref(h)), "sv_debug_cols_rowhalf_launches")
    return n.value, h.value


def op_linear_skinny(x, W, bias=None, splitk=1):
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); W = _need(W, torch.bfloat16, "W")
    M, K = x.shape; N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    b = _need(bias, torch.bfloat16, "bias") if bias is not None else None
    check(lib.sv_op_linear_skinny(_ptr(x), _ptr(W), _ptr(b), _ptr(y), M, N, K, splitk, _stream()))
    return y


def op_linear_skinny_fp8(x, W, bias=None, splitk=1):
    """Returns (y fp32 [M, N], row scales fp32 [N]) of the fp8-weight decode GEMM (weights quantised on device)."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); W = _need(W, torch.bfloat16, "W")
    M, K = x.shape; N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    sc = torch.empty(N, dtype=torch.float32, device=x.device)
    b = _need(bias, torch.bfloat16, "bias") if bias is not None else None
    check(lib.sv_op_linear_skinny_fp8(_ptr(x), _ptr(W), _ptr(b), _ptr(y), _ptr(sc), M, N, K, splitk, _stream()))
    return y, sc


def op_linear_skinny_epi(x, W, bias=None, act="none", out_f32=False):
    """The decode GEMM's fused epilogues (split-K 1): act(bf16(x W^T + bias)) as bf16 rows (the c_fc form), or with out_f32
    the lm_head form: float32 rows of x W^T holding bf16-rounded values (no bias)."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); W = _need(W, torch.bfloat16, "W")
    M, K = x.shape; N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    b = _need(bias, torch.bfloat16, "bias") if bias is not None else None
    check(lib.sv_op_linear_skinny_epi(_ptr(x), _ptr(W), _ptr(b), _ptr(y), M, N, K, _lib.ACT[act], int(out_f32), _stream()),
          "sv_op_linear_skinny_epi")
    return y


def op_linear_skinny_epi_fp8(x, W, bias=None, act="none", out_f32=False):
    """`op_linear_skinny_epi` with the weight quantised to fp8 e4m3 on device (an fp8 engine's c_fc / lm_head launch): returns
    (y, row scales fp32 [N])."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); W = _need(W, torch.bfloat16, "W")
    M, K = x.shape; N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    sc = torch.empty(N, dtype=torch.float32, device=x.device)
    b = _need(bias, torch.bfloat16, "bias") if bias is not None else None
    check(lib.sv_op_linear_skinny_epi_fp8(_ptr(x), _ptr(W), _ptr(b), _ptr(y), _ptr(sc), M, N, K, _lib.ACT[act], int(out_f32), _stream()),
          "sv_op_linear_skinny_epi_fp8")
    return y, sc


def op_linear_fp8(x, W, bias=None, residual=None, act="none", out_f32=False):
    """`op_linear` with the weight quantised to fp8 e4m3 on device: the big-M kernels on the bf16 image of the quantised values, the row
    scales applied to the accumulator (an fp8 engine's prompt pass).  Returns (y, row scales fp32 [N])."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); W = _need(W, torch.bfloat16, "W")
    M, K = x.shape; N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    sc = torch.empty(N, dtype=torch.float32, device=x.device)
    b = _need(bias, torch.bfloat16, "bias") if bias is not None else None
    r = _need(residual, torch.bfloat16, "residual") if residual is not None else None
    check(lib.sv_op_linear_fp8(_ptr(x), _ptr(W), _ptr(b), _ptr(r), _ptr(y), _ptr(sc), M, N, K, _lib.ACT[act], int(out_f32), _stream()),
          "sv_op_linear_fp8")
    return y, sc


def op_pack_weight_fp8(W):
    """The fp8 quantiser as sv_load_weight runs it, W [N, K] bf16 or float32: returns the raw images (scales fp32 [Npad], the decode image
    uint8 [Npad * K], the bf16 image [Npad * K]); their layouts are stated in starvector_hip_debug.h."""
    lib = _lib.load()
    if W.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("W must be bfloat16 or float32")
    W = _need(W, W.dtype, "W")
    N, K = W.shape
    Npad = (N + 31) // 32 * 32
    sc = torch.empty(Npad, dtype=torch.float32, device=W.device)
    wq = torch.empty(Npad * K, dtype=torch.uint8, device=W.device)
    wp = torch.empty(Npad * K, dtype=torch.bfloat16, device=W.device)
    check(lib.sv_op_pack_weight_fp8(_ptr(W), int(W.dtype == torch.float32), N, K, _ptr(sc), _ptr(wq), _ptr(wp), _stream()),
          "sv_op_pack_weight_fp8")
    return sc, wq, wp


def op_pack_weight_mxfp4(W):
    """The MXFP4 quantiser as sv_load_weight runs it, W [N, K] bf16 or float32: returns the raw images (scale bytes uint8 [Npad, K / 32], the
    decode image uint8 [Npad / 32 * K / 64 * 1088], the bf16 image [Npad * K]); their layouts are stated in starvector_hip_debug.h."""
    lib = _lib.load()
    if W.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("W must be bfloat16 or float32")
    W = _need(W, W.dtype, "W")
    N, K = W.shape
    Npad = (N + 31) // 32 * 32
    sc = torch.empty(Npad, max(K // 32, 1), dtype=torch.uint8, device=W.device)
    w4 = torch.empty(Npad // 32 * max(K // 64, 1) * 1088, dtype=torch.uint8, device=W.device)
    wp = torch.empty(Npad * K, dtype=torch.bfloat16, device=W.device)
    check(lib.sv_op_pack_weight_mxfp4(_ptr(W), int(W.dtype == torch.float32), N, K, _ptr(sc), _ptr(w4), _ptr(wp), _stream()),
          "sv_op_pack_weight_mxfp4")
    return sc, w4, wp


def op_linear_skinny_mxfp4(x, W, bias=None, splitk=1, col_tiles=0):
    """Returns (y fp32 [M, N], scale bytes uint8 [N, K / 32]) of the MXFP4-weight decode GEMM (weights quantised on device); col_tiles =
    column tiles per block (1, 2, 4: identical bits; 0 = the launcher's default).  M may exceed 32."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); W = _need(W, torch.bfloat16, "W")
    M, K = x.shape; N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    sc = torch.empty(N, max(K // 32, 1), dtype=torch.uint8, device=x.device)
    b = _need(bias, torch.bfloat16, "bias") if bias is not None else None
    check(lib.sv_op_linear_skinny_mxfp4(_ptr(x), _ptr(W), _ptr(b), _ptr(y), _ptr(sc), M, N, K, splitk, int(col_tiles), _stream()),
          "sv_op_linear_skinny_mxfp4")
    return y, sc


def op_linear_skinny_epi_mxfp4(x, W, bias=None, act="none", out_f32=False, col_tiles=0):
    """`op_linear_skinny_epi` with the weight quantised to MXFP4 on device (an mxfp4 engine's c_fc / lm_head launch): returns
    (y, scale bytes uint8 [N, K / 32])."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); W = _need(W, torch.bfloat16, "W")
    M, K = x.shape; N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    sc = torch.empty(N, max(K // 32, 1), dtype=torch.uint8, device=x.device)
    b = _need(bias, torch.bfloat16, "bias") if bias is not None else None
    check(lib.sv_op_linear_skinny_epi_mxfp4(_ptr(x), _ptr(W), _ptr(b), _ptr(y), _ptr(sc), M, N, K, _lib.ACT[act], int(out_f32), int(col_tiles),
                                            _stream()), "sv_op_linear_skinny_epi_mxfp4")
    return y, sc


def op_lm_head_argmax(x, W):
    """The lm_head form of the decode GEMM with the greedy selection folded into its epilogue (what a plain greedy generate
    runs per step): returns (logits float32 [M, N] holding bf16-rounded values, arg-max column per row as an int64 cpu tensor)."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); W = _need(W, torch.bfloat16, "W")
    M, K = x.shape; N = W.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    idx = (C.c_int32 * M)()
    check(lib.sv_op_lm_head_argmax(_ptr(x), _ptr(W), _ptr(y), idx, M, N, K, _stream()), "sv_op_lm_head_argmax")
    return y, torch.tensor(list(idx), dtype=torch.int64)


def op_decode_proj_fold(x, Wp, bp, h, gamma, beta, Wf, bf_, act="gelu_tanh", eps=1e-5):
    """The 6-launch decode layer's two kernels (csrc/decode_cols.hip): returns (h2 bf16 [M, D], y bf16 [M, F])."""
    lib = _lib.load()
    t = lambda v, n: _need(v, torch.bfloat16, n)
    x, Wp, h, gamma, beta, Wf = t(x, "x"), t(Wp, "Wp"), t(h, "h"), t(gamma, "gamma"), t(beta, "beta"), t(Wf, "Wf")
    bp = t(bp, "bp") if bp is not None else None
    bf_ = t(bf_, "bf") if bf_ is not None else None
    M, Kp = x.shape; D = Wp.shape[0]; F = Wf.shape[0]
    h2 = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
    y = torch.empty(M, F, dtype=torch.bfloat16, device=x.device)
    check(lib.sv_op_decode_proj_fold(_ptr(x), _ptr(Wp), _ptr(bp), _ptr(h), _ptr(gamma), _ptr(beta), float(eps), _ptr(Wf), _ptr(bf_),
                                     _ptr(h2), _ptr(y), M, D, Kp, F, _lib.ACT[act], _stream()), "sv_op_decode_proj_fold")
    return h2, y


def bench_decode_linear(M: int, N: int, K: int, splitk: int = 1, mode: int = 0, iters: int = 100) -> float:
    """Average microseconds per launch of one decode GEMM (mode 0 fp32 slabs, 1 bias + GELU, 2 fp32 logits)."""
    lib = _lib.load()
    us = C.c_double(0.0)
    check(lib.sv_bench_decode_linear(M, N, K, splitk, mode, iters, C.byref(us), _stream()), "sv_bench_decode_linear")
    return us.value


def op_cvt_bf16_hw(x):
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib.sv_op_cvt_bf16_hw(_ptr(x), _ptr(y), x.numel(), _stream()))
    return y


def op_attention(q, k, v, n_head, n_kv_head, causal, scale=None):
    lib = _lib.load()
    q = _need(q, torch.bfloat16, "q"); k = _need(k, torch.bfloat16, "k"); v = _need(v, torch.bfloat16, "v")
    B, S, HD = q.shape
    hd = HD // n_head
    out = torch.empty_like(q)
    check(lib.sv_op_attention(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, S, n_head, n_kv_head, hd, int(causal),
                              float(scale if scale is not None else hd ** -0.5), _stream()))
    return out


def op_attention_prefill(qkv, q_off, k_off, v_off, n_head, n_kv_head, head_dim, *, B=None, S=None, lens=None, causal=True,
                         window=0, last_rows=0, scale=None, out=None):
    """The prompt-pass attention as the engine launches it: q / k / v are column ranges (element offsets) of the rows of ONE bf16
    buffer `qkv` [rows, row_stride].  Either (B, S) or `lens` (a list of lengths: the ragged form over packed rows).  `out`
    ([rows, n_head * head_dim], bf16, contiguous) may be handed in pre-filled: with last_rows > 0 only the trailing query tiles
    are written.  Returns `out`."""
    lib = _lib.load()
    if not qkv.is_cuda or qkv.dtype != torch.bfloat16 or qkv.dim() != 2 or not qkv.is_contiguous():
        raise ValueError("qkv must be a contiguous 2-D bfloat16 CUDA(HIP) tensor [rows, row_stride]")
    if (lens is None) == (B is None or S is None):
        raise ValueError("give either B and S or lens")
    if lens is not None:
        lens = [int(x) for x in lens]
        B, S = len(lens), 0
        rows = sum(max(x, 0) for x in lens)
        c_lens = (C.c_int32 * max(B, 1))(*lens)
    else:
        B, S = int(B), int(S)
        rows = max(B, 0) * max(S, 0)
        c_lens = None
    stride, width = qkv.shape[1], int(n_head) * int(head_dim)
    # the kernel addresses rows * row_stride elements of qkv and rows * n_head * head_dim of out: both must lie inside the tensors
    if rows > qkv.shape[0]:
        raise ValueError(f"qkv holds {qkv.shape[0]} rows, the call addresses {rows}")
    if out is None:
        out = torch.empty(rows, width, dtype=torch.bfloat16, device=qkv.device)
    elif not out.is_cuda or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.numel() < rows * width:
        raise ValueError(f"out must be a contiguous bfloat16 CUDA(HIP) tensor of at least {rows} x {width} elements")
    check(lib.sv_op_attention_prefill(_ptr(qkv), int(q_off), int(k_off), int(v_off), stride, _ptr(out), B, S, c_lens, int(n_head),
                                      int(n_kv_head), int(head_dim), int(bool(causal)), float(scale if scale is not None else head_dim ** -0.5),
                                      int(window), int(last_rows), _stream()), "sv_op_attention_prefill")
    return out


def op_attn_prefill_prefixed(qkv, q_off, k_off, v_off, n_head, n_kv_head, head_dim, prefix_lens, lens, prefix_of, *, window=0, scale=None,
                             out=None):
    """The prompt-pass attention in its PREFIXED form alone (sv_op_attn_prefill_prefixed): the rows of `qkv` [rows, row_stride] are the prefixes
    back to back, then every sequence's own rows; sequence b attends as cat(prefix[prefix_of[b]], own rows).  Only the own rows of `out`
    ([rows, n_head * head_dim], may be handed in pre-filled) are written.  Returns `out`."""
    lib = _lib.load()
    if not qkv.is_cuda or qkv.dtype != torch.bfloat16 or qkv.dim() != 2 or not qkv.is_contiguous():
        raise ValueError("qkv must be a contiguous 2-D bfloat16 CUDA(HIP) tensor [rows, row_stride]")
    pl, ln, po = [int(v) for v in prefix_lens], [int(v) for v in lens], [int(v) for v in prefix_of]
    if len(po) != len(ln) or not pl or not ln:
        raise ValueError("one prefix index per sequence, at least one prefix and one sequence")
    rows = sum(max(v, 0) for v in pl + ln)
    stride, width = qkv.shape[1], int(n_head) * int(head_dim)
    # the kernel addresses rows * row_stride elements of qkv and rows * n_head * head_dim of out: both must lie inside the tensors
    if rows > qkv.shape[0]:
        raise ValueError(f"qkv holds {qkv.shape[0]} rows, the call addresses {rows}")
    if out is None:
        out = torch.empty(rows, width, dtype=torch.bfloat16, device=qkv.device)
    elif not out.is_cuda or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.numel() < rows * width:
        raise ValueError(f"out must be a contiguous bfloat16 CUDA(HIP) tensor of at least {rows} x {width} elements")
    ints = lambda v: (C.c_int32 * len(v))(*v)
    check(lib.sv_op_attn_prefill_prefixed(_ptr(qkv), int(q_off), int(k_off), int(v_off), stride, _ptr(out), len(pl), ints(pl), len(ln), ints(ln),
                                          ints(po), int(n_head), int(n_kv_head), int(head_dim), float(scale if scale is not None else head_dim ** -0.5),
                                          int(window), _stream()), "sv_op_attn_prefill_prefixed")
    return out


def op_plane_layernorm(x, gamma, beta, eps=1e-5, y_batch_stride=None, out=None):
    """y_batch_stride (elements): plane b goes to out.flatten()[b * y_batch_stride:] -- the form the engine launches; `out` may be handed in pre-filled."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); B = x.shape[0]; QD = x[0].numel()
    g, b = _need(gamma, torch.bfloat16, "gamma"), _need(beta, torch.bfloat16, "beta")
    _op_size(g, QD, "gamma"); _op_size(b, QD, "beta")
    if y_batch_stride is None:
        y = torch.empty_like(x) if out is None else _op_out(out, torch.bfloat16, B * QD)
        check(lib.sv_op_plane_layernorm(_ptr(x), _ptr(g), _ptr(b), _ptr(y), B, QD, eps, _stream()))
        return y
    stride = int(y_batch_stride)
    need = (B - 1) * stride + QD
    y = torch.empty(need, dtype=torch.bfloat16, device=x.device) if out is None else _op_out(out, torch.bfloat16, need)
    check(lib.sv_op_plane_layernorm_strided(_ptr(x), _ptr(g), _ptr(b), _ptr(y), B, QD, eps, stride, _stream()), "sv_op_plane_layernorm_strided")
    return y


# ---- the row kernels of the prompt side and the decode residual stream (sv_op_* of the same names).  The C entry points see pointers
# only, so every wrapper checks here that the tensors hold what the kernel will address; `out` may be handed in pre-filled, so that a
# test can see what a kernel leaves alone.
def _op_out(out, dtype, need: int):
    if not out.is_cuda or out.dtype != dtype or not out.is_contiguous() or out.numel() < need:
        raise ValueError(f"out must be a contiguous {dtype} CUDA(HIP) tensor of at least {need} elements, got {tuple(out.shape)} {out.dtype}")
    return out


def _op_size(t, need: int, what: str):
    if t.numel() < need:
        raise ValueError(f"{what} holds {t.numel()} elements, the call addresses {need}")
    return t


def _op_index(t, dtype, n: int, lo: int, hi: int, what: str):
    """An index tensor of the device: `n` entries of `dtype`, every one in [lo, hi)."""
    t = _need(t, dtype, what)
    if t.numel() != n:
        raise ValueError(f"{what} must hold {n} entries, got {t.numel()}")
    if n and (int(t.min()) < lo or int(t.max()) >= hi):
        raise ValueError(f"{what} has an entry outside [{lo}, {hi})")
    return t


def xp_elems(M: int, K: int) -> int:
    """Elements of a fragment-order ("xp", csrc/common.h) buffer of M rows of K columns: whole tiles of 32 rows."""
    return (int(M) + 31) // 32 * 32 * int(K)


def op_im2col(img, patch: int, Kpad: int, out=None):
    lib = _lib.load()
    img = _need(img, torch.bfloat16, "img")
    B, Cc, S, S2 = img.shape
    if Cc != 3 or S != S2 or S % patch:
        raise ValueError("img must be [B, 3, S, S] with S a multiple of patch")
    rows = B * (S // patch) ** 2
    out = torch.empty(rows, Kpad, dtype=torch.bfloat16, device=img.device) if out is None else _op_out(out, torch.bfloat16, rows * Kpad)
    check(lib.sv_op_im2col(_ptr(img), _ptr(out), B, S, int(patch), int(Kpad), _stream()), "sv_op_im2col")
    return out


def op_vit_embed_lnpre(patch_out, cls, pos, gamma, beta, B: int, NP: int, Dv: int, eps=1e-5, out=None):
    """patch_out: [B * NP, ldp] with ldp >= Dv (the row stride is taken from its shape)."""
    lib = _lib.load()
    t = lambda v, n: _need(v, torch.bfloat16, n)
    patch_out, cls, pos, gamma, beta = t(patch_out, "patch_out"), t(cls, "cls"), t(pos, "pos"), t(gamma, "gamma"), t(beta, "beta")
    if patch_out.dim() != 2 or patch_out.shape[0] < B * NP:
        raise ValueError(f"patch_out must be [>= {B * NP}, ldp]")
    ldp = patch_out.shape[1]
    _op_size(cls, Dv, "cls"); _op_size(pos, (NP + 1) * Dv, "pos"); _op_size(gamma, Dv, "gamma"); _op_size(beta, Dv, "beta")
    need = B * (NP + 1) * Dv
    out = torch.empty(B, NP + 1, Dv, dtype=torch.bfloat16, device=patch_out.device) if out is None else _op_out(out, torch.bfloat16, need)
    check(lib.sv_op_vit_embed_lnpre(_ptr(patch_out), ldp, _ptr(cls), _ptr(pos), _ptr(gamma), _ptr(beta), _ptr(out), B, NP, Dv, float(eps),
                                    _stream()), "sv_op_vit_embed_lnpre")
    return out


def op_dec_embed(emb, table, row_pos=None, out=None):
    """emb [B, S0, D] + table[t]: t = the row's index inside its sequence, or row_pos[row] (int32 [B * S0])."""
    lib = _lib.load()
    emb, table = _need(emb, torch.bfloat16, "emb"), _need(table, torch.bfloat16, "table")
    B, S0, D = emb.shape
    if table.dim() != 2 or table.shape[1] != D:
        raise ValueError("table must be [positions, D]")
    if row_pos is not None:
        row_pos = _op_index(row_pos, torch.int32, B * S0, 0, table.shape[0], "row_pos")
    elif table.shape[0] < S0:
        raise ValueError(f"table holds {table.shape[0]} positions, S0 is {S0}")
    out = torch.empty_like(emb) if out is None else _op_out(out, torch.bfloat16, emb.numel())
    check(lib.sv_op_dec_embed(_ptr(emb), _ptr(table), _ptr(out), B, S0, D, _ptr(row_pos), _stream()), "sv_op_dec_embed")
    return out


def op_gather_rows(table, ids, per_seq: int = 0, seq_stride: int = 0, out=None):
    """out row r = table[ids[r]]; per_seq > 0: row r is written at element (r // per_seq) * seq_stride + (r % per_seq) * D of `out`."""
    lib = _lib.load()
    table = _need(table, torch.bfloat16, "table")
    V, D = table.shape
    n = ids.numel()
    ids = _op_index(ids, torch.int64, n, 0, V, "ids")
    if per_seq:
        if per_seq < 0 or n % per_seq or seq_stride < per_seq * D:
            raise ValueError("n must be a multiple of per_seq and seq_stride >= per_seq * D")
        need = (n // per_seq - 1) * int(seq_stride) + per_seq * D
    else:
        need = n * D
    out = torch.empty(need, dtype=torch.bfloat16, device=table.device) if out is None else _op_out(out, torch.bfloat16, need)
    check(lib.sv_op_gather_rows(_ptr(table), _ptr(ids), _ptr(out), n, D, int(per_seq), int(seq_stride), _stream()), "sv_op_gather_rows")
    return out


def _rag_seq(lens, device):
    """Descriptors {first packed row, length} of sequences packed back to back."""
    lens = [int(x) for x in lens]
    if not lens or min(lens) < 1:
        raise ValueError("lens must be a non-empty list of lengths >= 1")
    first, desc = 0, []
    for n in lens:
        desc += [first, n]
        first += n
    return torch.tensor(desc, dtype=torch.int32, device=device), first


def op_gather_last_rows(h, B: Optional[int] = None, S0: Optional[int] = None, lens=None, out=None):
    """h [rows, D]: the last row of each of B sequences of S0 rows, or (lens) of each sequence of the packed ragged form."""
    lib = _lib.load()
    h = _need(h, torch.bfloat16, "h")
    rows, D = h.shape
    if lens is not None:
        desc, total = _rag_seq(lens, h.device)
        B, S0 = len(lens), 0
    else:
        desc, total = None, int(B) * int(S0)
    if total > rows:
        raise ValueError(f"h holds {rows} rows, the call addresses {total}")
    out = torch.empty(B, D, dtype=torch.bfloat16, device=h.device) if out is None else _op_out(out, torch.bfloat16, B * D)
    check(lib.sv_op_gather_last_rows(_ptr(h), _ptr(out), int(B), int(S0), D, _ptr(desc), _stream()), "sv_op_gather_last_rows")
    torch.cuda.current_stream().synchronize()                  # `desc` is a temporary
    return out


def op_gather_tail_rows(h, n_keep: int, out=None):
    lib = _lib.load()
    h = _need(h, torch.bfloat16, "h")
    B, S0, D = h.shape
    if not 1 <= n_keep <= S0:
        raise ValueError("1 <= n_keep <= S0")
    out = torch.empty(B * n_keep, D, dtype=torch.bfloat16, device=h.device) if out is None else _op_out(out, torch.bfloat16, B * n_keep * D)
    check(lib.sv_op_gather_tail_rows(_ptr(h), _ptr(out), B, S0, int(n_keep), D, _stream()), "sv_op_gather_tail_rows")
    return out


def op_gather_tail_rows_ragged(h, lens, keep, out=None):
    """h [rows, D], sequences of `lens` rows packed back to back: the last keep[b] rows of every sequence, packed [sum(keep), D]."""
    lib = _lib.load()
    h = _need(h, torch.bfloat16, "h")
    rows, D = h.shape
    lens, keep = [int(x) for x in lens], [int(x) for x in keep]
    if not lens or len(keep) != len(lens) or any(not 1 <= k <= n for k, n in zip(keep, lens)):
        raise ValueError("lens and keep must be non-empty lists of equal size with 1 <= keep[b] <= lens[b]")
    if sum(lens) > rows:
        raise ValueError(f"h holds {rows} rows, the call addresses {sum(lens)}")
    first, total, desc = 0, 0, []
    for n, k in zip(lens, keep):
        desc += [first, n, k, total]
        first += n
        total += k
    desc = torch.tensor(desc, dtype=torch.int32, device=h.device)
    out = torch.empty(total, D, dtype=torch.bfloat16, device=h.device) if out is None else _op_out(out, torch.bfloat16, total * D)
    check(lib.sv_op_gather_tail_rows_ragged(_ptr(h), _ptr(out), len(lens), D, _ptr(desc), total, _stream()), "sv_op_gather_tail_rows_ragged")
    torch.cuda.current_stream().synchronize()                  # `desc` is a temporary
    return out


def op_gather_listed_rows(x, rows, D: int, out=None):
    """x [R, ldx] (ldx >= D): out[i] = x[rows[i], :D]."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x")
    R, ldx = x.shape
    if D > ldx:
        raise ValueError("D > ldx")
    n = rows.numel()
    rows = _op_index(rows, torch.int32, n, 0, R, "rows")
    out = torch.empty(n, D, dtype=torch.bfloat16, device=x.device) if out is None else _op_out(out, torch.bfloat16, n * D)
    check(lib.sv_op_gather_listed_rows(_ptr(x), ldx, _ptr(rows), n, _ptr(out), int(D), _stream()), "sv_op_gather_listed_rows")
    return out


def op_ragged_row_pos(lens, out):
    """out (int32, at least sum(lens) entries, handed in by the caller): out[first_b + j] = j."""
    lib = _lib.load()
    desc, total = _rag_seq(lens, out.device)
    _op_out(out, torch.int32, total)
    check(lib.sv_op_ragged_row_pos(_ptr(desc), len(lens), _ptr(out), _stream()), "sv_op_ragged_row_pos")
    torch.cuda.current_stream().synchronize()
    return out


def op_ragged_positions(lens, rep: int, delta: int, out):
    """out (int32, at least len(lens) * rep entries): out[i] = lens[i // rep] + delta."""
    lib = _lib.load()
    desc, _ = _rag_seq(lens, out.device)
    if rep < 1:
        raise ValueError("rep >= 1")
    _op_out(out, torch.int32, len(lens) * int(rep))
    check(lib.sv_op_ragged_positions(_ptr(out), _ptr(desc), len(lens), int(rep), int(delta), _stream()), "sv_op_ragged_positions")
    torch.cuda.current_stream().synchronize()
    return out


def op_token_batchnorm(x, w, b, running_mean, running_var, eps=1e-5, y_batch_stride=None, out=None):
    lib = _lib.load()
    t = lambda v, n: _need(v, torch.bfloat16, n)
    x, w, b, rm, rv = t(x, "x"), t(w, "w"), t(b, "b"), t(running_mean, "running_mean"), t(running_var, "running_var")
    B, Q, D = x.shape
    for v, n in ((w, "w"), (b, "b"), (rm, "running_mean"), (rv, "running_var")):
        _op_size(v, Q, n)
    stride = Q * D if y_batch_stride is None else int(y_batch_stride)
    need = (B - 1) * stride + Q * D
    out = torch.empty(need, dtype=torch.bfloat16, device=x.device) if out is None else _op_out(out, torch.bfloat16, need)
    check(lib.sv_op_token_batchnorm(_ptr(x), _ptr(w), _ptr(b), _ptr(rm), _ptr(rv), _ptr(out), B, Q, D, float(eps), stride, _stream()),
          "sv_op_token_batchnorm")
    return out


def op_layernorm_packed(x, gamma, beta, eps=1e-5, out=None):
    """LayerNorm of x [M, D] written in fragment order: a flat buffer of xp_elems(M, D) elements (rows >= M are not written)."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); M, D = x.shape
    g, b = _need(gamma, torch.bfloat16, "gamma"), _need(beta, torch.bfloat16, "beta")
    _op_size(g, D, "gamma"); _op_size(b, D, "beta")
    need = xp_elems(M, D)
    out = torch.empty(need, dtype=torch.bfloat16, device=x.device) if out is None else _op_out(out, torch.bfloat16, need)
    check(lib.sv_op_layernorm_packed(_ptr(x), _ptr(g), _ptr(b), _ptr(out), M, D, float(eps), _stream()), "sv_op_layernorm_packed")
    return out


def op_pack_rows(x, out=None):
    """x [M, K] row-major -> fragment order (flat, xp_elems(M, K) elements)."""
    lib = _lib.load()
    x = _need(x, torch.bfloat16, "x"); M, K = x.shape
    need = xp_elems(M, K)
    out = torch.empty(need, dtype=torch.bfloat16, device=x.device) if out is None else _op_out(out, torch.bfloat16, need)
    check(lib.sv_op_pack_rows(_ptr(x), K, _ptr(out), M, K, _stream()), "sv_op_pack_rows")
    return out


def op_unpack_rows(xp, M: int, K: int, out=None):
    lib = _lib.load()
    xp = _need(xp, torch.bfloat16, "xp")
    _op_size(xp, xp_elems(M, K), "xp")
    out = torch.empty(M, K, dtype=torch.bfloat16, device=xp.device) if out is None else _op_out(out, torch.bfloat16, M * K)
    check(lib.sv_op_unpack_rows(_ptr(xp), _ptr(out), K, int(M), int(K), _stream()), "sv_op_unpack_rows")
    return out


def op_row_update_ln(h, gamma, beta, xp_out, M: int, D: int, eps=1e-5, *, ws=None, bias=None, ldh: int = 0,
                     wte=None, wpe=None, tokens=None, positions=None):
    """The decode row update on its own (csrc/kernels.h RowUpdateArgs).  `h` (in / out) is row-major with row stride ldh, or, ldh == 0,
    fragment order; `xp_out` receives LayerNorm(h) in fragment order; both are the caller's buffers.  Residual mode: ws fp32
    [splitk, rows_ws, ldws] and bias [D].  Embedding mode (ws None): wte [V, D], optional wpe [P, D], tokens / positions int32 [M]."""
    lib = _lib.load()
    t = lambda v, n: _need(v, torch.bfloat16, n)
    h, gamma, beta, xp_out = t(h, "h"), t(gamma, "gamma"), t(beta, "beta"), t(xp_out, "xp_out")
    M, D, ldh = int(M), int(D), int(ldh)
    _op_size(gamma, D, "gamma"); _op_size(beta, D, "beta"); _op_size(xp_out, xp_elems(M, D), "xp_out")
    _op_size(h, (M - 1) * ldh + D if ldh else xp_elems(M, D), "h")
    if ws is not None:
        ws = _need(ws, torch.float32, "ws")
        if ws.dim() != 3 or ws.shape[1] < M or ws.shape[2] < D or bias is None:
            raise ValueError("residual mode: ws must be [splitk, rows_ws >= M, ldws >= D] and bias given")
        splitk, rows_ws, ldws_ = ws.shape
        bias = _op_size(t(bias, "bias"), D, "bias")
        check(lib.sv_op_row_update_ln(_ptr(ws), splitk, ldws_, rows_ws, _ptr(bias), _ptr(h), ldh, None, None, None, None, _ptr(gamma), _ptr(beta),
                                      float(eps), _ptr(xp_out), M, D, _stream()), "sv_op_row_update_ln")
        return h, xp_out
    wte = t(wte, "wte")
    if wte.dim() != 2 or wte.shape[1] != D:
        raise ValueError("wte must be [V, D]")
    tokens = _op_index(tokens, torch.int32, M, 0, wte.shape[0], "tokens")
    if wpe is not None:
        wpe = t(wpe, "wpe")
        if wpe.dim() != 2 or wpe.shape[1] != D:
            raise ValueError("wpe must be [P, D]")
    positions = _op_index(positions, torch.int32, M, 0, wpe.shape[0] if wpe is not None else 1 << 30, "positions")
    check(lib.sv_op_row_update_ln(None, 0, 0, 0, None, _ptr(h), ldh, _ptr(wte), _ptr(wpe), _ptr(tokens), _ptr(positions), _ptr(gamma), _ptr(beta),
                                  float(eps), _ptr(xp_out), M, D, _stream()), "sv_op_row_update_ln")
    return h, xp_out


def op_argmax(logits):
    lib = _lib.load()
    logits = _need(logits, torch.float32, "logits"); B, V = logits.shape
    if V % 4:
        raise ValueError("V must be a multiple of 4")
    out = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(lib.sv_op_argmax(_ptr(logits), B, V, V, _ptr(out), _stream()))
    return out


def op_logprob_rows(logits, targets, temperature: float = 1.0, valid: Optional[int] = None):
    """logprob_rows_kernel on caller-given bf16 rows [R, ld] (ld a multiple of 8), `valid` = V columns count (default ld); targets
    int32 [R].  Returns (logprob, logsumexp, entropy, argmax, (flag, first flagged row))."""
    lib = _lib.load()
    logits = _need(logits, torch.bfloat16, "logits")
    R, ld = logits.shape
    V = ld if valid is None else int(valid)
    targets = _need(targets.to(torch.int32), torch.int32, "targets")
    if targets.numel() != R:
        raise ValueError("one target per row")
    dev = logits.device
    lp, lse, ent = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(3))
    am = torch.empty(R, dtype=torch.int32, device=dev)
    flag = (C.c_int32 * 2)()
    check(lib.sv_op_logprob_rows(_ptr(logits), R, V, ld, _ptr(targets), float(temperature), _ptr(lp), _ptr(lse), _ptr(ent), _ptr(am),
                                 flag, _stream()), "sv_op_logprob_rows")
    return lp, lse, ent, am, (int(flag[0]), int(flag[1]))


def op_topk_rows_bf16(logits, targets, logsumexp, k: int, temperature: float = 1.0, valid: Optional[int] = None):
    """topk_rows_bf16_kernel (sv_forward_topk's kernel) on the rows of `op_logprob_rows` and the logsumexp it returned for them.  Returns
    (ids int32 [R, k], logprobs fp32 [R, k], ranks int32 [R])."""
    lib = _lib.load()
    logits = _need(logits, torch.bfloat16, "logits")
    R, ld = logits.shape
    V = ld if valid is None else int(valid)
    targets = _need(targets.to(torch.int32), torch.int32, "targets")
    lse = _need(logsumexp, torch.float32, "logsumexp")
    if targets.numel() != R or lse.numel() != R:
        raise ValueError("one target and one logsumexp per row")
    ids = torch.empty(R, max(int(k), 1), dtype=torch.int32, device=logits.device)
    lps = torch.empty(R, max(int(k), 1), dtype=torch.float32, device=logits.device)
    rank = torch.empty(R, dtype=torch.int32, device=logits.device)
    check(lib.sv_op_topk_rows_bf16(_ptr(logits), R, V, ld, _ptr(targets), float(temperature), _ptr(lse), int(k), _ptr(ids), _ptr(lps), _ptr(rank),
                                   _stream()), "sv_op_topk_rows_bf16")
    return ids, lps, rank


def op_token_topk(logits, tokens, k: int, temperature: float = 1.0, valid: Optional[int] = None):
    """sv_generate_topk's raw-source row function on caller-given fp32 rows [B, ld], `valid` = V columns (default ld); tokens int32 [B] or None
    (no rank).  Returns (ids int32 [B, k], logprobs fp32 [B, k], ranks int32 [B])."""
    lib = _lib.load()
    logits = _need(logits, torch.float32, "logits")
    B, ld = logits.shape
    V = ld if valid is None else int(valid)
    if tokens is not None:
        tokens = _need(tokens.to(torch.int32), torch.int32, "tokens")
        if tokens.numel() != B:
            raise ValueError("one token per row")
    ids = torch.empty(B, max(int(k), 1), dtype=torch.int32, device=logits.device)
    lps = torch.empty(B, max(int(k), 1), dtype=torch.float32, device=logits.device)
    rank = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(lib.sv_op_token_topk(_ptr(logits), B, V, ld, float(temperature), _ptr(tokens), int(k), _ptr(ids), _ptr(lps), _ptr(rank), _stream()),
          "sv_op_token_topk")
    return ids, lps, rank


def op_cb_select(logits, requests: Sequence[dict], history=None):
    """The continuous-batching selection (cb_step_kernel) on caller-given fp32 rows [B, V]: row b is request requests[b] (the
    `cb_admit` dict) after the output ids history[b] (a list; its length is the step).  Returns int32 [B] on the host."""
    lib = _lib.load()
    logits = _need(logits, torch.float32, "logits")
    B, V = logits.shape
    ld = (V + 3) // 4 * 4
    if ld != V:
        pad = torch.full((B, ld), -float("inf"), dtype=torch.float32, device=logits.device)
        pad[:, :V] = logits
        logits = pad
    history = [list(map(int, h)) for h in (history or [[]] * B)]
    if len(history) != B or len(requests) != B:
        raise ValueError("one request and one history per row")
    ld_hist = max(1, max(len(h) for h in history))
    hist = (C.c_int32 * (B * ld_hist))()
    for b, h in enumerate(history):
        for t, x in enumerate(h):
            hist[b * ld_hist + t] = x
    lens = (C.c_int32 * B)(*[len(h) for h in history])
    arr, keep = cb_requests(requests)
    out = (C.c_int32 * B)()
    check(lib.sv_op_cb_select(_ptr(logits), B, V, ld, arr, hist, ld_hist, lens, out, _stream()), "sv_op_cb_select")
    del keep
    return torch.tensor(list(out), dtype=torch.int32)


def op_cb_logprobs(logits, requests: Sequence[dict], logprobs: Sequence, history=None):
    """`op_cb_select` plus one logprobs entry per row (None | dict(k=, source=), as `HipEngine.cb_admit` takes them): the recording form of
    cb_step_kernel on caller-given rows.  Returns host tensors (tokens int32 [B], token log-probs fp32 [B], ranks int32 [B], ids int32 [B, K],
    log-probs fp32 [B, K]) with K = the largest k asked (at least 1); a row's entries past its own k read (-1, -inf), a row that records nothing
    reads (NaN, 0) and an empty list."""
    lib = _lib.load()
    logits = _need(logits, torch.float32, "logits")
    B, V = logits.shape
    ld = (V + 3) // 4 * 4
    if ld != V:
        pad = torch.full((B, ld), -float("inf"), dtype=torch.float32, device=logits.device)
        pad[:, :V] = logits
        logits = pad
    history = [list(map(int, h)) for h in (history or [[]] * B)]
    if len(history) != B or len(requests) != B or len(logprobs) != B:
        raise ValueError("one request, one logprobs entry and one history per row")
    ld_hist = max(1, max(len(h) for h in history))
    hist = (C.c_int32 * (B * ld_hist))()
    for b, h in enumerate(history):
        for t, x in enumerate(h):
            hist[b * ld_hist + t] = x
    lens = (C.c_int32 * B)(*[len(h) for h in history])
    arr, keep = cb_requests(requests)
    lps = cb_logprobs(requests, logprobs)
    if lps is None:
        lps = (_lib.SvCbLogprobs * B)()
    K = max([1] + [int(l.k) for l in lps if l.enable])
    out, lp, rk = (C.c_int32 * B)(), (C.c_float * B)(), (C.c_int32 * B)()
    ids, vals = (C.c_int32 * (B * K))(), (C.c_float * (B * K))()
    check(lib.sv_op_cb_logprobs(_ptr(logits), B, V, ld, arr, lps, hist, ld_hist, lens, out, lp, rk, ids, vals, K, _stream()), "sv_op_cb_logprobs")
    del keep
    return (torch.tensor(list(out), dtype=torch.int32), torch.tensor(list(lp), dtype=torch.float32), torch.tensor(list(rk), dtype=torch.int32),
            torch.tensor(list(ids), dtype=torch.int32).view(B, K), torch.tensor(list(vals), dtype=torch.float32).view(B, K))


def op_cb_lookup_step(logits, K: int, requests: Sequence[dict], base, live, history, rows, positions, n_draft, max_ngram: int = 0,
                      min_ngram: int = 0, forced=None, logprobs: Optional[Sequence] = None):
    """ONE launch of the drafting batch's selection (cb_lookup_step_kernel; sv_op_cb_lookup_step) on caller-given state: n = len(requests)
    slots of K + 1 rows, logits fp32 [n * (K + 1), V] (row s * (K + 1) + j = slot s's row j).  Slot s: request requests[s] (the `cb_admit`
    dict), prompt length base[s], live[s], the ids it has emitted history[s] (a list), and the step in flight rows[s] / positions[s] (K + 1
    each) with n_draft[s] live drafts.  forced: None or a list of equal-length id lists (slot s < len(forced) drafts forced[s][step + j]).
    Returns a dict of host lists: live, history, rows, positions, n_draft (the state after the launch), counts [n][3] = {steps, drafted,
    accepted} of this launch, finished, bad -- and, with `logprobs` (one entry per slot, as `cb_admit` takes them), logprob / rank [n][K + 1]:
    the record of the columns each slot emitted (NaN / 0 behind them)."""
    lib = _lib.load()
    logits = _need(logits, torch.float32, "logits")
    n, K1 = len(requests), int(K) + 1
    R, V = logits.shape
    if R != n * K1:
        raise ValueError(f"logits must have n * (K + 1) = {n * K1} rows, got {R}")
    ld = (V + 3) // 4 * 4
    if ld != V:
        pad = torch.full((R, ld), -float("inf"), dtype=torch.float32, device=logits.device)
        pad[:, :V] = logits
        logits = pad
    history = [list(map(int, h)) for h in history]
    if not (len(history) == len(base) == len(live) == len(rows) == len(positions) == len(n_draft) == n):
        raise ValueError("one entry per slot in base / live / history / rows / positions / n_draft")
    if any(len(r) != K1 for r in rows) or any(len(r) != K1 for r in positions):
        raise ValueError("rows / positions hold K + 1 entries per slot")
    ld_hist = max(len(h) for h in history) + K1
    hist = (C.c_int32 * (n * ld_hist))()
    for s, h in enumerate(history):
        hist[s * ld_hist: s * ld_hist + len(h)] = h
    lens = (C.c_int32 * n)(*[len(h) for h in history])
    c_base = (C.c_int32 * n)(*[int(v) for v in base])
    c_live = (C.c_int32 * n)(*[int(bool(v)) for v in live])
    c_rows = (C.c_int32 * (n * K1))(*[int(v) for r in rows for v in r])
    c_pos = (C.c_int32 * (n * K1))(*[int(v) for r in positions for v in r])
    c_nd = (C.c_int32 * n)(*[int(v) for v in n_draft])
    c_forced, fn, fld = None, 0, 0
    if forced is not None:
        fn, fld = len(forced), len(forced[0])
        if any(len(f) != fld for f in forced):
            raise ValueError("forced rows must have equal length")
        c_forced = (C.c_int32 * (fn * fld))(*[int(v) for f in forced for v in f])
    arr, keep = cb_requests(requests)
    lps = cb_logprobs(requests, logprobs) if logprobs is not None else None
    counts, flags = (C.c_int32 * (3 * n))(), (C.c_int32 * 3)()
    lp, rk = (C.c_float * (n * K1))(), (C.c_int32 * (n * K1))()
    check(lib.sv_op_cb_lookup_step(_ptr(logits), n, int(K), V, ld, arr, lps, c_base, c_live, hist, ld_hist, lens, c_rows, c_pos, c_nd, int(max_ngram),
                                   int(min_ngram), c_forced, fn, fld, counts, flags, lp if lps is not None else None,
                                   rk if lps is not None else None, _stream()), "sv_op_cb_lookup_step")
    del keep
    out = {"live": [int(v) for v in c_live], "history": [list(hist[s * ld_hist: s * ld_hist + lens[s]]) for s in range(n)],
           "rows": [list(c_rows[s * K1:(s + 1) * K1]) for s in range(n)], "positions": [list(c_pos[s * K1:(s + 1) * K1]) for s in range(n)],
           "n_draft": list(c_nd), "counts": [list(counts[3 * s:3 * s + 3]) for s in range(n)], "finished": flags[0], "bad": flags[2]}
    if lps is not None:
        out["logprob"] = [list(lp[s * K1:(s + 1) * K1]) for s in range(n)]
        out["rank"] = [list(rk[s * K1:(s + 1) * K1]) for s in range(n)]
    return out


def op_ban_tokens(logits, history, no_repeat_ngram_size=0, bad_words_ids=None):
    """The token-ban kernel of `generate_processed` (ban_tokens_kernel) on caller-given fp32 rows [B, V]: row b has generated the ids
    history[b] (a list) so far.  The kernel works in place on a copy whose row stride is V rounded up to 4 (padding columns zero).  Returns
    (rows [B, V], padding columns [B, ld - V]): the rows with the ids NoRepeatNGram(no_repeat_ngram_size) and NoBadWords(bad_words_ids) ban at
    that point set to -inf and every other value untouched, and the padding as the kernel left it."""
    lib = _lib.load()
    logits = _need(logits, torch.float32, "logits")
    B, V = logits.shape
    ld = (V + 3) // 4 * 4
    buf = torch.zeros(B, ld, dtype=torch.float32, device=logits.device)
    buf[:, :V] = logits
    history = [list(map(int, h)) for h in history]
    if len(history) != B:
        raise ValueError("one history per row")
    ld_hist = max(1, max(len(h) for h in history))
    hist = (C.c_int32 * (B * ld_hist))()
    for b, h in enumerate(history):
        hist[b * ld_hist: b * ld_hist + len(h)] = h
    lens = (C.c_int32 * B)(*[len(h) for h in history])
    lp, keep = logits_processors(no_repeat_ngram_size, bad_words_ids, 0.0, vocab=V)
    check(lib.sv_op_ban_tokens(_ptr(buf), B, V, ld, hist, ld_hist, lens, C.byref(lp), _stream()), "sv_op_ban_tokens")
    del keep
    return buf[:, :V].clone(), buf[:, V:].clone()


def op_preprocess_image(pixels: torch.Tensor, size: int, mean, std, recipe: str = "starvector") -> torch.Tensor:
    """uint8 [H, W, 3|4] on the GPU -> float32 [3, size, size].  recipe "starvector": composite on white, pad to square,
    Pillow-exact bicubic resize, ToTensor, Normalize (starvector/data/util.py:40-68); "siglip": HF SiglipImageProcessor
    (alpha dropped, stretch-resize, rescale 1/255, normalise) as the v2 tower uses it (image_encoder.py:45-48)."""
    lib = _lib.load()
    px = _need(pixels, torch.uint8, "pixels")
    if px.dim() != 3 or px.shape[2] not in (3, 4):
        raise ValueError("pixels must be uint8 [H, W, 3] (RGB) or [H, W, 4] (RGBA)")
    out = torch.empty(3, size, size, dtype=torch.float32, device=px.device)
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    check(lib.sv_preprocess_image(_ptr(px), px.shape[1], px.shape[0], px.shape[2], int(size),
                                  {"starvector": 0, "siglip": 1}[recipe], m3, s3, _ptr(out), _stream()), "sv_preprocess_image")
    return out


def op_preprocess_images(pixels, size: int, mean, std, recipe: str = "starvector") -> torch.Tensor:
    """A batch of uint8 [H, W, 3|4] GPU tensors (any sizes) -> float32 [n, 3, size, size], one call (`sv_preprocess_images`):
    three launches per 32 images, no host copy, no synchronisation, workspace from torch's caching allocator."""
    lib = _lib.load()
    if len(pixels) == 0:
        raise ValueError("empty batch")
    px = [_need(t, torch.uint8, "pixels") for t in pixels]
    for t in px:
        if t.dim() != 3 or t.shape[2] not in (3, 4):
            raise ValueError("pixels must be uint8 [H, W, 3] (RGB) or [H, W, 4] (RGBA)")
    n = len(px)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in px])
    ws_ = (C.c_int32 * n)(*[t.shape[1] for t in px])
    hs_ = (C.c_int32 * n)(*[t.shape[0] for t in px])
    cs_ = (C.c_int32 * n)(*[t.shape[2] for t in px])
    rc = {"starvector": 0, "siglip": 1}[recipe]
    need = lib.sv_preprocess_workspace_bytes(ws_, hs_, n, int(size), rc)
    if need < 0:
        check(int(need), "sv_preprocess_workspace_bytes")
    work = torch.empty(int(need), dtype=torch.uint8, device=px[0].device)
    out = torch.empty(n, 3, size, size, dtype=torch.float32, device=px[0].device)
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    check(lib.sv_preprocess_images(ptrs, ws_, hs_, cs_, n, int(size), rc, m3, s3, _ptr(out), _ptr(work), int(need), _stream()),
          "sv_preprocess_images")
    return out


def op_sample_top_p(logits, temperature, top_p, seed, step, top_k=0):
    lib = _lib.load()
    logits = _need(logits, torch.float32, "logits"); B, V = logits.shape
    out = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(lib.sv_op_sample(_ptr(logits), B, V, V, float(temperature), int(top_k), float(top_p), int(seed), int(step),
                           _ptr(out), _stream()))
    return out


def op_capture_rows(rows, valid: Optional[int] = None, do_sample: bool = True, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                    min_p: float = 0.0, seen=None, penalty: float = 1.0, eos_token_id: int = -1, hold_eos: bool = False,
                    scores_out=None, logits_out=None):
    """The per-step output launch of generate(output_scores / output_logits) on caller-given fp32 rows [B, ld] (sv_op_capture_rows:
    capture_warp_kernel + capture_write_kernel), `valid` = V columns (default ld).  ``seen``: per-row sets of ids for the repetition
    ``penalty``.  scores_out / logits_out: fp32 [>= B, >= V] tensors of one row stride that receive the processed and the raw rows in place
    (default: fresh [B, V] tensors); columns >= V and rows >= B of them are left as they were.  Returns (scores, logits)."""
    lib = _lib.load()
    x = _need(rows, torch.float32, "rows")
    B, ld = x.shape
    V = ld if valid is None else int(valid)
    if scores_out is None and logits_out is None:
        scores_out = torch.empty(B, V, dtype=torch.float32, device=x.device)
        logits_out = torch.empty(B, V, dtype=torch.float32, device=x.device)
    outs = [o for o in (scores_out, logits_out) if o is not None]
    for o in outs:
        if o.dtype != torch.float32 or o.dim() != 2 or o.shape[0] < B or o.shape[1] < V or o.stride(1) != 1 or o.stride(0) != outs[0].stride(0):
            raise ValueError("outputs must be fp32 [>= B, >= V] with unit column stride and one row stride")
    bits, words = None, 0
    if seen is not None:
        words = (V + 31) // 32
        host = torch.zeros(B, words, dtype=torch.int64)
        for r, ids in enumerate(seen):
            for i in ids:
                host[r, int(i) >> 5] |= 1 << (int(i) & 31)
        bits = (host - ((host >> 31) << 32)).to(torch.int32).to(x.device)          # the uint32 words, bit for bit
    check(lib.sv_op_capture_rows(_ptr(x), B, V, x.stride(0), _ptr(bits), words, float(penalty), int(eos_token_id), int(bool(hold_eos)),
                                 int(bool(do_sample)), float(temperature), int(top_k or 0), float(top_p), float(min_p), _ptr(scores_out),
                                 _ptr(logits_out), outs[0].stride(0), _stream()), "sv_op_capture_rows")
    return scores_out, logits_out


def op_lookup_draft(hist: Sequence[int], K: int, max_ngram: int = 3, min_ngram: int = 1, max_new: Optional[int] = None) -> List[int]:
    """The n-gram lookup of generate_lookup on one history (sv_op_lookup_draft; lookup.draft is its restatement)."""
    lib = _lib.load()
    L = len(hist)
    max_new = int(max_new if max_new is not None else L + K + 1)
    h = (C.c_int32 * max(L, 1))(*[int(t) for t in hist])
    out, n = (C.c_int32 * 16)(), C.c_int32(0)
    check(lib.sv_op_lookup_draft(h, L, int(K), int(max_ngram), int(min_ngram), max_new, out, C.byref(n), _stream()), "sv_op_lookup_draft")
    return [out[j] for j in range(n.value)]


def op_lookup_accept(state, winners) -> None:
    """One lookup_step_kernel launch (sv_op_lookup_accept) on a lookup.LookupState, updated in place as LookupState.step(winners) updates it."""
    lib = _lib.load()
    n_seq, K1, ld = state.n_seq, state.K + 1, state.max_new
    flat = lambda rows: (C.c_int32 * (n_seq * K1))(*[int(t) for r in rows for t in r])
    hist = (C.c_int32 * (n_seq * ld))(*[int(t) for h in state.hist for t in h])
    st = (C.c_int32 * (4 * n_seq))(*[int(v) for s in range(n_seq)
                                     for v in (state.n_emit[s], state.finished[s], state.base[s], state.n_draft[s])])
    call = (C.c_int32 * 8)(state.limit, int(state.done), state.n_emitted, state.bad, state.steps, state.drafted, state.accepted, 0)
    stop = (C.c_int32 * max(len(state.stop), 1))(*[int(t) for t in state.stop])
    nrows, npos = (C.c_int32 * (n_seq * K1))(), flat(state.positions)
    check(lib.sv_op_lookup_accept(flat(winners), flat(state.rows), n_seq, state.K, state.max_ngram, state.min_ngram, hist, ld, st, call,
                                  stop if state.stop else None, len(state.stop), int(state.eos), int(state.pad), state.max_new, int(state.vocab),
                                  nrows, npos, _stream()), "sv_op_lookup_accept")
    for s in range(n_seq):
        state.hist[s] = [hist[s * ld + c] for c in range(ld)]
        state.n_emit[s], state.finished[s], state.base[s], state.n_draft[s] = st[4 * s], bool(st[4 * s + 1]), st[4 * s + 2], st[4 * s + 3]
        state.rows[s] = [nrows[s * K1 + j] for j in range(K1)]
        state.positions[s] = [npos[s * K1 + j] for j in range(K1)]
    state.limit, state.done, state.n_emitted, state.bad, state.steps, state.drafted, state.accepted = \
        call[0], bool(call[1]), call[2], call[3], call[4], call[5], call[6]


def op_lookup_hold(logits: torch.Tensor, K1: int, eos: int, min_new: int, n_emit: Sequence[int]) -> torch.Tensor:
    """The min-length hold of a verification step on caller-given rows (sv_op_lookup_hold): a copy of logits [rows, ld] fp32 with
    [r, eos] = -inf wherever n_emit[r // K1] + r % K1 < min_new."""
    lib = _lib.load()
    x = _need(logits, torch.float32, "logits").clone()
    rows, ld = x.shape
    arr = (C.c_int32 * len(n_emit))(*[int(v) for v in n_emit])
    check(lib.sv_op_lookup_hold(_ptr(x), ld, rows, int(K1), int(eos), int(min_new), arr, _stream()), "sv_op_lookup_hold")
    return x


def op_lookup_sample(logits: torch.Tensor, K1: int, n_emit: Sequence[int], temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                     seen=None, penalty: float = 1.0, return_slices: bool = False):
    """The draw of generate_lookup_sampled on caller-given rows (sv_op_lookup_sample): logits [rows, ld] fp32, row s * K1 + j draws with
    (seed, n_emit[s] + j, s).  ``seen``: per-row sets of ids (one iterable per row) for the repetition ``penalty``.  Returns the id of every
    row as lookup_step_kernel reads it (0x7fffffff: no finite score); ``return_slices``: also the [rows, 8] values and ids of the hand-over."""
    lib = _lib.load()
    x = _need(logits, torch.float32, "logits")
    rows, ld = x.shape
    arr = (C.c_int32 * len(n_emit))(*[int(v) for v in n_emit])
    words, bits = 0, None
    if seen is not None:
        words = (ld + 31) // 32
        bits = (C.c_uint32 * (rows * words))()
        for r, ids in enumerate(seen):
            for i in ids:
                bits[r * words + (int(i) >> 5)] |= 1 << (int(i) & 31)
    out, pv, pi = (C.c_int32 * rows)(), (C.c_float * (rows * 8))(), (C.c_int32 * (rows * 8))()
    check(lib.sv_op_lookup_sample(_ptr(x), rows, ld, ld, int(K1), arr, float(temperature), int(top_k), float(top_p), int(seed) & (2 ** 64 - 1), bits, words,
                                  float(penalty), out, pv, pi, _stream()), "sv_op_lookup_sample")
    if return_slices:
        return list(out), [list(pv[r * 8:r * 8 + 8]) for r in range(rows)], [list(pi[r * 8:r * 8 + 8]) for r in range(rows)]
    return list(out)


def op_lookup_seen(hist, L_before: Sequence[int], L_after: Sequence[int], n_draft: Sequence[int], rows, vocab: int, seq_seen=None):
    """One lookup_seen_kernel launch (sv_op_lookup_seen): hist [n_seq][ld] generated ids, seq_seen the sequences' id sets over columns
    [0, L_before) (default: empty), rows [n_seq][K1] the next step's ids with n_draft live drafts.  Returns (sequence sets, row sets) as
    Python sets of ids -- every set bit of the bitmaps, whatever its position."""
    lib = _lib.load()
    n_seq, ld, K1 = len(hist), len(hist[0]), len(rows[0])
    words = (int(vocab) + 31) // 32
    ia = lambda v: (C.c_int32 * len(v))(*[int(t) for t in v])
    seq = (C.c_uint32 * (n_seq * words))()
    for s, ids in enumerate(seq_seen or []):
        for i in ids:
            seq[s * words + (int(i) >> 5)] |= 1 << (int(i) & 31)
    row = (C.c_uint32 * (n_seq * K1 * words))()
    check(lib.sv_op_lookup_seen(ia([t for h in hist for t in h]), ld, n_seq, K1, words, ia(L_before), ia(L_after), ia(n_draft),
                                ia([t for r in rows for t in r]), seq, row, _stream()), "sv_op_lookup_seen")
    unpack = lambda buf, k: {w * 32 + b for w in range(words) for b in range(32) if (buf[k * words + w] >> b) & 1}
    return [unpack(seq, s) for s in range(n_seq)], [unpack(row, r) for r in range(n_seq * K1)]
