"""vLLM's offline API (`LLM`, `SamplingParams`) over the HIP engine: the reference's recommended backend (`generation_engine: vllm`)
runs here with one changed import line,

    from starvector_amd.vllm import LLM, SamplingParams          # instead of: from vllm import LLM, SamplingParams

The sampler semantics are vLLM 0.5.5's (the version the reference's generation configs link), per request and step: logit_bias
(the OpenAI server's logits processor, clamped to [-100, 100]) -> min_tokens hold of EOS and the stop ids -> repetition penalty
over prompt ids + output ids -> frequency and presence penalties over the output counts -> greedy argmax when temperature < 1e-5,
else temperature -> top-k -> top-p -> min_p -> one draw.  All of it runs on device in the continuous-batching step
(sampling.hip, cb_step_kernel); this module maps the parameters, queues the requests on a `ContinuousBatcher` and builds the
outputs.  Deviations from the StarVector vLLM fork: the prompt ids are the token ids of the request's TEXT prompt (image
positions carry no id here and count as none), and draws are distributional (vLLM's exponential-race RNG is not reproduced).
The n samples of an input (`SamplingParams.n`, the validator's `num_generations`) go in as ONE group: the image encoder and adapter
run once per input, and the samples admitted together share one prompt pass and the prompt's full KV pages (`sv_cb_admit_shared`;
`generate(..., share_prompt=False)` queues every sample on its own, the same tokens).
Log-probs come through a keyword of `LLM.generate`: `generate(..., logprobs=k)` fills, for every request of the call,
`CompletionOutput.logprobs` (one {token id: Logprob} dict per token: the k most likely ids with ranks 1..k plus the sampled token with its own
rank) and `cumulative_logprob`, from the record the continuous batch keeps on device (`sv_cb_admit_logprobs`, source "processed": the
distribution vLLM's Sampler reports).  `SamplingParams(logprobs=...)` itself still raises, as do the fields below.
Not built: prompt_logprobs (image positions carry no token id), best_of > n, stop strings, beam search.
"""
from __future__ import annotations

import itertools
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Union

import torch

_SAMPLING_EPS = 1e-5            # vLLM: temperature below this is greedy
_BIAS_CLAMP = 100.0             # the OpenAI server clamps every logit_bias value to [-100, 100]
_MAX_STOP_IDS = 8
_MAX_BIAS = 128


class SamplingParams:
    """vLLM 0.5.5's `SamplingParams`: same field names, defaults and range checks (`_verify_args`).  `logit_bias` ({token id:
    bias}) is the OpenAI server's argument, applied first like its logits processor.  Fields that are not built raise
    NotImplementedError when set: best_of > n, logprobs, prompt_logprobs, stop strings, use_beam_search."""

    def __init__(self, n: int = 1, best_of: Optional[int] = None, presence_penalty: float = 0.0,
                 frequency_penalty: float = 0.0, repetition_penalty: float = 1.0, temperature: float = 1.0,
                 top_p: float = 1.0, top_k: int = -1, min_p: float = 0.0, seed: Optional[int] = None,
                 use_beam_search: bool = False, stop: Optional[Union[str, List[str]]] = None,
                 stop_token_ids: Optional[List[int]] = None, ignore_eos: bool = False, max_tokens: Optional[int] = 16,
                 min_tokens: int = 0, logprobs: Optional[int] = None, prompt_logprobs: Optional[int] = None,
                 skip_special_tokens: bool = True, logit_bias: Optional[Dict[int, float]] = None):
        self.n = n
        self.best_of = n if best_of is None else best_of
        self.presence_penalty = float(presence_penalty)
        self.frequency_penalty = float(frequency_penalty)
        self.repetition_penalty = float(repetition_penalty)
        self.temperature = float(temperature)
        self.top_p = float(top_p)
        self.top_k = int(top_k)
        self.min_p = float(min_p)
        self.seed = seed
        self.use_beam_search = use_beam_search
        self.stop = [stop] if isinstance(stop, str) else list(stop or [])
        self.stop_token_ids = [int(t) for t in (stop_token_ids or [])]
        self.ignore_eos = bool(ignore_eos)
        self.max_tokens = max_tokens
        self.min_tokens = int(min_tokens)
        self.logprobs = logprobs
        self.prompt_logprobs = prompt_logprobs
        self.skip_special_tokens = bool(skip_special_tokens)
        self.logit_bias = {int(k): float(v) for k, v in (logit_bias or {}).items()}
        self._verify_args()
        if self.temperature < _SAMPLING_EPS:           # vLLM: greedy ignores top-p, top-k and min-p
            self.top_p, self.top_k, self.min_p = 1.0, -1, 0.0
            if self.best_of > 1:
                raise ValueError(f"best_of must be 1 when using greedy sampling. Got {self.best_of}.")

    def _verify_args(self) -> None:
        if self.n < 1:
            raise ValueError(f"n must be at least 1, got {self.n}.")
        if self.best_of < self.n:
            raise ValueError(f"best_of must be greater than or equal to n, got n={self.n} and best_of={self.best_of}.")
        if not -2.0 <= self.presence_penalty <= 2.0:
            raise ValueError(f"presence_penalty must be in [-2, 2], got {self.presence_penalty}.")
        if not -2.0 <= self.frequency_penalty <= 2.0:
            raise ValueError(f"frequency_penalty must be in [-2, 2], got {self.frequency_penalty}.")
        if not self.repetition_penalty > 0.0:
            raise ValueError(f"repetition_penalty must be greater than zero, got {self.repetition_penalty}.")
        if self.temperature < 0.0:
            raise ValueError(f"temperature must be non-negative, got {self.temperature}.")
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p}.")
        if self.top_k < -1 or self.top_k == 0:
            raise ValueError(f"top_k must be -1 (disable), or at least 1, got {self.top_k}.")
        if not 0.0 <= self.min_p <= 1.0:
            raise ValueError(f"min_p must be in [0, 1], got {self.min_p}.")
        if self.max_tokens is not None and self.max_tokens < 1:
            raise ValueError(f"max_tokens must be at least 1, got {self.max_tokens}.")
        if self.min_tokens < 0:
            raise ValueError(f"min_tokens must be greater than or equal to 0, got {self.min_tokens}.")
        if self.max_tokens is not None and self.min_tokens > self.max_tokens:
            raise ValueError(f"min_tokens must be less than or equal to max_tokens={self.max_tokens}, got {self.min_tokens}.")
        if len(self.stop_token_ids) > _MAX_STOP_IDS:
            raise ValueError(f"at most {_MAX_STOP_IDS} stop_token_ids are supported, got {len(self.stop_token_ids)}.")
        if len(self.logit_bias) > _MAX_BIAS:
            raise ValueError(f"at most {_MAX_BIAS} logit_bias entries are supported, got {len(self.logit_bias)}.")
        if self.best_of > self.n:
            raise NotImplementedError("best_of > n is not built: every sample is returned (set best_of = n)")
        if self.use_beam_search:
            raise NotImplementedError("vLLM beam search is not built (the engine's HF beam search is HipCausalLM.generate)")
        if self.logprobs is not None or self.prompt_logprobs is not None:
            raise NotImplementedError("logprobs / prompt_logprobs are not built")
        if self.stop:
            raise NotImplementedError("stop strings are not built: use stop_token_ids")

    @property
    def greedy(self) -> bool:
        return self.temperature < _SAMPLING_EPS

    def __repr__(self) -> str:
        keys = ("n", "presence_penalty", "frequency_penalty", "repetition_penalty", "temperature", "top_p", "top_k", "min_p",
                "seed", "stop_token_ids", "ignore_eos", "max_tokens", "min_tokens", "skip_special_tokens", "logit_bias")
        return "SamplingParams(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in keys) + ")"


@dataclass
class Logprob:
    """vLLM's `Logprob`: one entry of a position's {token id: Logprob} dict."""
    logprob: float
    rank: Optional[int] = None
    decoded_token: Optional[str] = None


@dataclass
class CompletionOutput:
    index: int
    text: str
    token_ids: List[int]
    cumulative_logprob: Optional[float] = None
    logprobs: Optional[list] = None
    finish_reason: Optional[str] = None
    stop_reason: Optional[int] = None


@dataclass
class RequestOutput:
    request_id: str
    prompt: Optional[str]
    prompt_token_ids: List[int]
    outputs: List[CompletionOutput] = field(default_factory=list)
    finished: bool = True


def sample_seeds(sp: SamplingParams) -> List[int]:
    """One seed per sample of a request: derived from `sp.seed` (reproducible, distinct across the n samples), else drawn
    from torch's generator, the contract of HipCausalLM.generate (torch.manual_seed reproduces a run)."""
    if sp.seed is not None:
        return [(int(sp.seed) + 0x9E3779B97F4A7C15 * (j + 1)) & (2 ** 63 - 1) for j in range(sp.n)]
    return [int(torch.randint(0, 2 ** 62, ()).item()) for _ in range(sp.n)]


def request_params(sp: SamplingParams, seed: int, max_new_tokens: int, prompt_ids: Sequence[int], eos_token_id: int,
                   pad_token_id: int, vocab: int) -> dict:
    """One sample of a request as the continuous batch's request dict (`HipEngine.cb_admit`, semantics 'vllm')."""
    for t in list(sp.logit_bias) + sp.stop_token_ids:
        if not 0 <= t < vocab:
            raise ValueError(f"token id {t} is outside the vocabulary (0..{vocab - 1})")
    greedy = sp.greedy
    return dict(
        semantics="vllm", max_new_tokens=int(max_new_tokens), do_sample=not greedy,
        temperature=1.0 if greedy else sp.temperature,
        top_p=1.0 if greedy else sp.top_p,
        top_k=0 if (greedy or sp.top_k == -1) else sp.top_k,
        min_p=0.0 if greedy else sp.min_p,
        presence_penalty=sp.presence_penalty, frequency_penalty=sp.frequency_penalty,
        repetition_penalty=sp.repetition_penalty, seed=int(seed),
        eos_token_id=-1 if sp.ignore_eos else int(eos_token_id), pad_token_id=int(pad_token_id),
        min_new_tokens=sp.min_tokens, prompt_ids=[int(t) for t in prompt_ids],
        logit_bias={t: max(-_BIAS_CLAMP, min(_BIAS_CLAMP, b)) for t, b in sp.logit_bias.items()},
        stop_any_ids=list(sp.stop_token_ids))


def parse_inputs(inputs, sampling_params) -> List[tuple]:
    """[(prompt text, image or None, SamplingParams)] in input order.  inputs: a string, a {"prompt", "multi_modal_data":
    {"image"}} dict, or a list of those; sampling_params: one SamplingParams (or None: the defaults) or one per input."""
    if isinstance(inputs, (str, dict)):
        inputs = [inputs]
    inputs = list(inputs)
    if sampling_params is None:
        sampling_params = SamplingParams()
    if isinstance(sampling_params, SamplingParams):
        params = [sampling_params] * len(inputs)
    else:
        params = list(sampling_params)
        if len(params) != len(inputs):
            raise ValueError(f"{len(params)} SamplingParams for {len(inputs)} inputs (give one, or one per input)")
    out = []
    for x, sp in zip(inputs, params):
        if not isinstance(sp, SamplingParams):
            raise TypeError(f"expected SamplingParams, got {type(sp).__name__}")
        if isinstance(x, str):
            out.append((x, None, sp))
        elif isinstance(x, dict):
            if "prompt" not in x:
                raise ValueError("an input dict needs a 'prompt' (prompt_token_ids inputs are not built)")
            mm = x.get("multi_modal_data") or {}
            extra = set(mm) - {"image"}
            if extra:
                raise NotImplementedError(f"multi_modal_data keys {sorted(extra)} are not built (image only)")
            out.append((str(x["prompt"]), mm.get("image"), sp))
        else:
            raise TypeError(f"an input is a string or a dict, got {type(x).__name__}")
    return out


def finish_of(token_ids: List[int], sp: SamplingParams, eos_token_id: int):
    """(finish_reason, stop_reason, number of ids the text decodes): vLLM's stop checker -- EOS (unless ignore_eos) first, then
    a stop id (stop_reason = the id), else the length limit; the EOS / stop id stays in token_ids but not in the text."""
    last = token_ids[-1] if token_ids else None
    if last is not None and not sp.ignore_eos and last == eos_token_id:
        return "stop", None, len(token_ids) - 1
    if last is not None and last in sp.stop_token_ids:
        return "stop", last, len(token_ids) - 1
    return "length", None, len(token_ids)


def completion_logprobs(token_ids: Sequence[int], token_logprobs, ranks, top_ids, top_logprobs, decode=None):
    """vLLM's per-token dicts from a request's record (`batching.TokenLogprobs`; tensors or nested lists): position t maps the listed ids
    (ids of -1 dropped) to Logprob(log-prob, rank = list position + 1) and holds the sampled token with its own log-prob and rank when the list
    does not -- vLLM's own order: the sampled entry first, the list on top of it.  Returns (dicts, cumulative_logprob = the sum of the sampled
    tokens' log-probs).  decode(id) -> the entry's decoded_token (None: left unset)."""
    as_list = lambda x: x.tolist() if hasattr(x, "tolist") else list(x)
    token_logprobs, ranks, top_ids, top_logprobs = map(as_list, (token_logprobs, ranks, top_ids, top_logprobs))
    if not (len(token_ids) == len(token_logprobs) == len(ranks) == len(top_ids) == len(top_logprobs)):
        raise ValueError("one record column per token")
    text = (lambda t: None) if decode is None else decode
    out, total = [], 0.0
    for t, tok in enumerate(token_ids):
        d = {int(tok): Logprob(float(token_logprobs[t]), int(ranks[t]), text(int(tok)))}
        for j, (i, lp) in enumerate(zip(top_ids[t], top_logprobs[t])):
            if int(i) >= 0:
                d[int(i)] = Logprob(float(lp), j + 1, text(int(i)))
        out.append(d)
        total += float(token_logprobs[t])
    return out, total


class LLM:
    """vLLM's offline `LLM` over the HIP engine.  `model` is a LOCAL checkpoint directory in the reference's format, loaded by
    `StarVectorForCausalLM.from_pretrained` (hub names fail there: no download).  `max_num_seqs` = the engine's batch rows (the
    continuous batch queues anything beyond it), `max_model_len` = its sequence capacity.  `dtype` float16 / float32 run in
    bfloat16 (with a warning).  `trust_remote_code` is accepted for compatibility (the model code is this package).

    Speculative decoding, vLLM 0.5.5's own arguments: ``speculative_model="[ngram]", num_speculative_tokens=K`` (1..15),
    ``ngram_prompt_lookup_max=n`` (0 / None = 3), ``ngram_prompt_lookup_min=m`` (0 / None = 1) switch on prompt-lookup drafting in the
    continuous batch (`HipEngine.cb_set_lookup`): every decode step verifies up to K drafted tokens per request, and the engine then
    runs max_num_seqs // (K + 1) requests at a time.  Any other `speculative_model` raises NotImplementedError (there is no draft model).
    The draft searches the request's OUTPUT ids only -- the prompt here is `inputs_embeds` (image features and text embeddings), not ids,
    where vLLM's n-gram worker searches prompt and output.  That changes the acceptance rate, never the tokens: every request returns
    what it returns without these arguments.

    ``quantization="fp8"`` / ``"mxfp4"`` quantise the decoder weights at load (`EngineConfig.weight_dtype`); None = the environment's
    SV_WEIGHT_DTYPE, else bf16.  Any other string raises ValueError.  Neither is the reference's precision.

    ``kv_cache_dtype="fp8"`` / ``"fp8_e4m3"`` keeps the paged KV cache as e4m3 codes with one power-of-two scale per key and head
    (`EngineConfig.kv_dtype`): half the pool and half the decode attention's stream; ``"auto"`` = bf16 (or the environment's SV_KV_DTYPE).
    Any other string raises ValueError.  Prompt-lookup drafting is not built for it.  Not the reference's precision.

    ``enable_prefix_caching=True`` (vLLM's keyword) switches on the continuous batch's prefix cache (`HipEngine.cb_set_prefix_cache`): within a
    `generate` call a prompt whose leading rows an earlier request brought -- the same image again, the part of a group of n samples that did
    not fit at once -- reuses that request's full KV pages.  The keys are digests of the prompt's embedding rows, not token ids; the tokens are
    those without the argument.  NotImplementedError together with an fp8 ``kv_cache_dtype``."""

    def __init__(self, model: str, tokenizer=None, dtype: str = "auto", max_model_len: Optional[int] = None,
                 max_num_seqs: Optional[int] = None, trust_remote_code: bool = False, speculative_model: Optional[str] = None,
                 num_speculative_tokens: Optional[int] = None, ngram_prompt_lookup_max: Optional[int] = None,
                 ngram_prompt_lookup_min: Optional[int] = None, quantization: Optional[str] = None, kv_cache_dtype: str = "auto",
                 enable_prefix_caching: bool = False, **kwargs):
        from .model import StarVectorForCausalLM
        if kv_cache_dtype not in ("auto", "fp8", "fp8_e4m3"):
            raise ValueError(f"kv_cache_dtype must be \"auto\", \"fp8\" or \"fp8_e4m3\", got {kv_cache_dtype!r}")
        if kv_cache_dtype != "auto" and speculative_model is not None:
            raise NotImplementedError("speculative_model=\"[ngram]\" with an fp8 KV cache is not built (the drafts' K / V pre-write is bf16)")
        if enable_prefix_caching and kv_cache_dtype != "auto":
            raise NotImplementedError("enable_prefix_caching with an fp8 KV cache is not built (a prompt pass behind cached pages sees the dequantised "
                                      "cache: the tokens would not be those without the cache)")
        self._prefix_cache = bool(enable_prefix_caching)
        if quantization is not None and quantization not in ("fp8", "mxfp4"):
            raise ValueError(f"quantization must be \"fp8\", \"mxfp4\" or None, got {quantization!r}")
        self._lookup = {}
        if speculative_model is not None:
            if speculative_model != "[ngram]":
                raise NotImplementedError(f"speculative_model={speculative_model!r} is not built: there is no draft model, only \"[ngram]\" "
                                          "(prompt-lookup drafting)")
            if num_speculative_tokens is None or not 1 <= int(num_speculative_tokens) <= 15:
                raise ValueError(f"num_speculative_tokens must lie in 1..15 with speculative_model=\"[ngram]\", got {num_speculative_tokens}")
            self._lookup = dict(prompt_lookup_num_tokens=int(num_speculative_tokens), max_matching_ngram_size=int(ngram_prompt_lookup_max or 0),
                                min_matching_ngram_size=int(ngram_prompt_lookup_min or 0))
        elif num_speculative_tokens or ngram_prompt_lookup_max or ngram_prompt_lookup_min:
            raise ValueError("num_speculative_tokens / ngram_prompt_lookup_max / ngram_prompt_lookup_min need speculative_model=\"[ngram]\"")
        dt = str(dtype).replace("torch.", "")
        if dt in ("float16", "half", "float32", "float"):
            warnings.warn(f"dtype={dtype}: the HIP engine computes in bfloat16; weights and inputs are converted", UserWarning)
        elif dt not in ("auto", "bfloat16"):
            raise ValueError(f"unsupported dtype={dtype} (bfloat16 / auto, or float16 / float32 converted to bfloat16)")
        load_kw = {}
        if quantization is not None:
            load_kw["weight_dtype"] = {"fp8": "fp8_e4m3", "mxfp4": "mxfp4"}[quantization]
        if kv_cache_dtype != "auto":
            load_kw["kv_cache_dtype"] = "fp8_e4m3"
        if max_num_seqs is not None:
            load_kw["max_batch"] = int(max_num_seqs)
        if max_model_len is not None:
            load_kw["max_length"] = int(max_model_len)
        if "byte_tokenizer_fallback" in kwargs:
            load_kw["byte_tokenizer_fallback"] = bool(kwargs.pop("byte_tokenizer_fallback"))
        ignored = {"gpu_memory_utilization", "enforce_eager", "tensor_parallel_size", "seed", "swap_space"}
        unknown = sorted(set(kwargs) - ignored)
        if unknown:
            raise TypeError(f"LLM: unsupported arguments {unknown}")
        if int(kwargs.get("tensor_parallel_size", 1) or 1) != 1:
            raise NotImplementedError("tensor_parallel_size > 1 is not built (data parallel: starvector_amd.parallel)")
        if tokenizer is not None and isinstance(tokenizer, str):
            from transformers import AutoTokenizer
            tokenizer = AutoTokenizer.from_pretrained(tokenizer, use_fast=False)
        self.model = StarVectorForCausalLM.from_pretrained(model, tokenizer=tokenizer, **load_kw)
        self.engine = self.model.engine
        self._sv = self.model.model
        self.tokenizer = self._sv.svg_transformer.tokenizer
        self.max_model_len = int(self.engine.cfg.max_seq_len)
        self._ids = itertools.count()

    def get_tokenizer(self):
        return self.tokenizer

    # ---- inputs -> (prompt ids, inputs_embeds [1, S0, D]) -----------------------------------------------------------------
    def _pixels(self, image):
        if torch.is_tensor(image):
            return image if image.dim() == 4 else image.unsqueeze(0)
        out = self._sv.processor(images=image, return_tensors="pt")
        pv = getattr(out, "pixel_values", None)
        pv = out["pixel_values"] if pv is None else pv
        return pv if pv.dim() == 4 else pv.unsqueeze(0)

    def _embed(self, prompt: str, image):
        device = torch.device("cuda", self.engine.device)
        if image is not None:
            emb, _, prompt_tokens = self._sv._prepare_generation_inputs({"image": self._pixels(image)}, prompt, device)
            ids = prompt_tokens.input_ids[0]
        else:
            ids = self._sv._tokenize([prompt], None, device, add_special_tokens=False).input_ids
            if ids.shape[1] == 0:
                raise ValueError("an empty text prompt has nothing to continue from")
            emb = self._sv._get_embeddings(ids)
            ids = ids[0]
        return [int(t) for t in ids.tolist()], emb.to(torch.bfloat16).contiguous()

    def prepare(self, inputs, sampling_params=None) -> List[dict]:
        """The requests `generate` submits, in input order then sample order: dicts with input, index, prompt, prompt_ids, emb
        ([1, S0, D] bf16) and params (the `HipEngine.cb_admit` request dict)."""
        tok = self.tokenizer
        eos = int(tok.eos_token_id)
        pad = tok.pad_token_id
        pad = eos if pad is None else int(pad)
        vocab = int(self.engine.cfg.vocab)
        jobs = []
        for i, (prompt, image, sp) in enumerate(parse_inputs(inputs, sampling_params)):
            ids, emb = self._embed(prompt, image)
            room = self.max_model_len - emb.shape[1]
            if room < 1:
                raise ValueError(f"input {i}: the prompt ({emb.shape[1]} positions) leaves no room below max_model_len {self.max_model_len}")
            max_new = room if sp.max_tokens is None else min(int(sp.max_tokens), room)
            for j, seed in enumerate(sample_seeds(sp)):
                jobs.append(dict(input=i, index=j, prompt=prompt, prompt_ids=ids, emb=emb, sp=sp,
                                 params=request_params(sp, seed, max_new, ids, eos, pad, vocab)))
        return jobs

    def generate(self, inputs, sampling_params=None, use_tqdm: bool = True, share_prompt: bool = True, logprobs: Optional[int] = None,
                 **kwargs) -> List[RequestOutput]:
        """One RequestOutput per input, in input order, each with its n CompletionOutputs.  Every (input, sample) pair is one
        request of the engine's continuous batch; more of them than `max_num_seqs` wait in its queue.  The samples of an input are
        submitted as one group (one prompt pass for those admitted together); share_prompt=False submits each on its own.
        logprobs = k (0..32), for every request of the call: `CompletionOutput.logprobs` (per token {id: Logprob} over the k most likely ids
        and the sampled one) and `cumulative_logprob`, as vLLM's `SamplingParams.logprobs` would; None: neither, and the requests run as before."""
        if kwargs.get("lora_request") is not None or kwargs.get("prompt_adapter_request") is not None:
            raise NotImplementedError("LoRA / prompt adapters are not built")
        if logprobs is not None and not 0 <= int(logprobs) <= 32:
            raise ValueError(f"logprobs must lie in 0..32, got {logprobs}.")
        from .batching import ContinuousBatcher
        jobs = self.prepare(inputs, sampling_params)
        if logprobs is not None:
            for j in jobs:
                j["params"] = dict(j["params"], logprobs=int(logprobs), logprob_source="processed")
        batcher = ContinuousBatcher(self.engine, **getattr(self, "_lookup", {}), **(dict(prefix_cache=True) if getattr(self, "_prefix_cache", False) else {}))
        try:
            handles = []
            for _, grp in itertools.groupby(jobs, key=lambda j: j["input"]):
                grp = list(grp)
                if share_prompt and len(grp) > 1:
                    handles += batcher.submit_group(grp[0]["emb"], [j["params"] for j in grp])
                else:
                    handles += [batcher.submit(j["emb"], j["params"]) for j in grp]
            toks = [h.result().view(-1).tolist() for h in handles]
            recs = [h.logprobs for h in handles]
        finally:
            batcher.close()
        eos = int(self.tokenizer.eos_token_id)
        outs: Dict[int, RequestOutput] = {}
        for j, t, rec in zip(jobs, toks, recs):
            ro = outs.get(j["input"])
            if ro is None:
                ro = outs[j["input"]] = RequestOutput(str(next(self._ids)), j["prompt"], list(j["prompt_ids"]))
            reason, stop_reason, n_text = finish_of(t, j["sp"], eos)
            text = self.tokenizer.decode(t[:n_text], skip_special_tokens=j["sp"].skip_special_tokens)
            comp = CompletionOutput(j["index"], text, t, finish_reason=reason, stop_reason=stop_reason)
            if rec is not None:
                comp.logprobs, comp.cumulative_logprob = completion_logprobs(t, *rec, decode=lambda i: self.tokenizer.decode([i]))
            ro.outputs.append(comp)
        return [outs[i] for i in sorted(outs)]

    def close(self) -> None:
        self.engine.close()
