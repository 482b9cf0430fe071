"""CPU: what `HipCausalLM.generate` and the `HipEngine.generate` family do with their arguments, pinned to a recording.

Part A drives `HipCausalLM.generate` over recording stand-in engines of three capability sets (every method; `generate` plus the
continuous-batching calls without `prefill_ragged`; `generate` alone), with and without a recording batcher.  A case is one keyword set;
tests/golden/generate_routes.json holds, per case, either the exception (type name, exact message) or the ordered list of engine and
batcher calls (method, keyword names, every scalar with its type, every tensor as shape / dtype / sum, the request dicts of the admits
with their seeds, the call lock's enter / exit), the returned value, the streamer's events and whether torch's generator moved.  The
table reaches every route, every refusal of the method and its helpers, one case per adjacent pair of checks that violates both, None for
every defaulted parameter, the three mask forms, shared prompts both ways, the size limits and the length budget.

Part B drives `HipEngine.generate`, its ragged / shared / processed wrappers and both lookup calls over a recording library (an engine
built with `__new__`, CPU tensors): per case the entry point, its integer arguments and lengths, every field of the sv_sampling it was
handed, which of the other structs were non-NULL with their scalar fields -- or the exception.

``python -m tests.test_generate_routes_host --record`` rewrites the fixture from the tree."""
import ctypes as C
import json
import os
import sys
import types

import pytest
import torch

from starvector_amd import engine as E, model as M
from starvector_amd.model import HipCausalLM, StoppingCriteriaSub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "generate_routes.json")
EXTENSION_FIELDS = ("token_logprobs", "token_logprobs_processed", "token_entropies", "top_token_ids", "top_logprobs", "token_ranks")


def _summ(v, total=True):
    """A string that pins `v`: tensors by dtype, shape and exact sum (the values are small integers), scalars by their repr (1, 1.0 and True differ)"""
    if isinstance(v, torch.Tensor):
        return f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}" + (f"={float(v.double().sum())!r}" if total else "")
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(_summ(x, total) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}={_summ(x, total)}" for k, x in sorted(v.items())) + "}"
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    return "<callable>" if callable(v) else f"<{type(v).__name__}>"


# ---- part A: the stand-in engines ------------------------------------------------------------------------------------------------------------
class _Lock:
    def __init__(self, log):
        self.log = log

    def __enter__(self):
        self.log.append("call_lock.enter")

    def __exit__(self, *exc):
        self.log.append("call_lock.exit")


class _EngGenerate:
    """`generate` alone.  The 'model' emits, for every row, tokens derived from the row's real prompt only (the sum of its embedding entries)."""
    device = 0

    def __init__(self, log, max_batch=8, free=1 << 30):
        self.log, self.free = log, free
        self.cfg = types.SimpleNamespace(vocab=7, max_batch=max_batch)
        self.call_lock = _Lock(log)
        self.slots = {}

    def _note(self, method, args, kw):
        # one line per call: method(positional arguments; keywords by name)  (the slabs arrive uninitialised: their shape alone)
        self.log.append(f"{method}({_summ(args)[1:-1]}; " + ", ".join(f"{k}={_summ(kw[k], k not in ('scores_out', 'logits_out'))}" for k in sorted(kw)) + ")")

    @staticmethod
    def _stream(row, budget):
        base = int(row.float().sum().round())
        return [(base + 3 * t) % 97 + 1 for t in range(budget)]

    def _model(self, rows, budget, kw):
        if budget <= 0:
            raise ValueError("the stand-in engine: no budget")
        B = len(rows)
        toks = torch.tensor([self._stream(r, budget) for r in rows], dtype=torch.long)
        n, stop = budget, kw.get("stop_ids")
        if stop:                                                                           # row-0 stop, like the engine
            r0 = toks[0].tolist()
            for t in range(len(stop) - 1, budget):
                if r0[t + 1 - len(stop):t + 1] == list(stop):
                    n = t + 1
                    break
        toks = toks[:, :n]
        if kw.get("on_tokens") is not None:
            kw["on_tokens"](toks, 0)
        if not (kw.get("return_outputs") or kw.get("token_stats") or kw.get("token_topk")):
            return toks
        res = {"sequences": toks, "n_generated": n}
        for name, fill in (("scores_out", 1.0), ("logits_out", 2.0)):
            if kw.get(name) is not None:
                kw[name].fill_(fill)
        if int(kw.get("num_beams", 1)) > 1:
            res["sequences_scores"] = torch.arange(B, dtype=torch.float32)
            res["beam_indices"] = torch.ones(B, n, dtype=torch.int64)
        if kw.get("token_stats"):
            names = E.TOKEN_STATS if kw["token_stats"] is True else tuple(kw["token_stats"])
            res.update({k: torch.full((B, n), float(3 + E.TOKEN_STATS.index(k))) for k in names})
        if kw.get("token_topk"):
            k = int(kw["token_topk"]["k"])
            res.update(top_token_ids=torch.ones(B, n, k, dtype=torch.int32), top_logprobs=torch.full((B, n, k), 2.0),
                       token_ranks=torch.ones(B, n, dtype=torch.int32))
        return res

    def generate(self, inputs_embeds, max_length, **kw):
        self._note("generate", [inputs_embeds, max_length], kw)
        return self._model(list(inputs_embeds), max_length - inputs_embeds.shape[1], kw)


class _EngSlots(_EngGenerate):
    """`generate` plus the continuous-batching calls, scripted as tests/test_host_logic.py's _FakeSlotEngine does; no `prefill_ragged`."""

    def cb_reset(self):
        self.log.append("cb_reset()")
        self.slots = {}

    def _admit(self, rows, reqs):
        out = []
        for row, r in zip(rows, reqs):
            s = min(set(range(self.cfg.max_batch)) - set(self.slots))
            self.slots[s] = dict(stream=self._stream(row, r["max_new_tokens"]), n=1, live=True, stop=r.get("stop_ids"), eos=r.get("eos_token_id", -1))
            self._finish(s)
            out.append(s)
        return out

    def cb_admit(self, emb, reqs):
        self._note("cb_admit", [emb], {"requests": reqs})
        return self._admit(list(emb), reqs)

    def _finish(self, s):
        sl = self.slots[s]
        got = sl["stream"][:sl["n"]]
        if sl["n"] >= len(sl["stream"]) or got[-1] == sl["eos"] or (sl["stop"] and got[-len(sl["stop"]):] == list(sl["stop"])):
            sl["live"] = False

    def cb_step(self, n):
        for _ in range(n):
            for s, sl in self.slots.items():
                if sl["live"]:
                    sl["n"] += 1
                    self._finish(s)
        live = sum(1 for sl in self.slots.values() if sl["live"])
        self.log.append(f"cb_step({n}) -> {live}")
        return live

    def cb_poll(self):
        lv = [int(self.slots[s]["live"]) if s in self.slots else 0 for s in range(self.cfg.max_batch)]
        st = [self.slots[s]["n"] if s in self.slots else 0 for s in range(self.cfg.max_batch)]
        return lv, st

    def cb_read(self, s, start, n):
        self.log.append(f"cb_read({s}, {start}, {n})")
        return torch.tensor(self.slots[s]["stream"][start:start + n], dtype=torch.long)


class _EngAll(_EngSlots):
    """Every method the mirror probes for."""

    def prefill_ragged(self, embeds, lengths=None):
        raise AssertionError("the mirror never needs the bare prompt pass")

    def mem_free_bytes(self):
        return self.free

    def cb_admit_shared(self, embs, lengths, group, reqs):
        self._note("cb_admit_shared", [embs, lengths, group], {"requests": reqs})
        return self._admit([embs[g] for g in group], reqs)

    def generate_shared(self, inputs_embeds, max_length, **kw):
        self._note("generate_shared", [inputs_embeds, max_length], kw)
        return self._model(list(inputs_embeds.repeat_interleave(kw["n_samples"], dim=0)), max_length - inputs_embeds.shape[1], kw)

    def generate_processed(self, inputs_embeds, max_length, **kw):
        self._note("generate_processed", [inputs_embeds, max_length], kw)
        return self._model(list(inputs_embeds.repeat_interleave(kw.get("n_samples", 1), dim=0)), max_length - inputs_embeds.shape[1], kw)

    def generate_ragged(self, embeds, max_length, **kw):
        self._note("generate_ragged", [embeds, max_length], kw)
        return self._model(list(embeds), max_length - max(int(t.shape[0]) for t in embeds), kw)

    def generate_lookup(self, inputs_embeds, max_length, **kw):
        self._note("generate_lookup", [inputs_embeds, max_length], kw)
        return self._model(list(inputs_embeds), max_length - inputs_embeds.shape[1], kw)

    def generate_lookup_sampled(self, inputs_embeds, max_length, **kw):
        self._note("generate_lookup_sampled", [inputs_embeds, max_length], kw)
        return self._model(list(inputs_embeds), max_length - inputs_embeds.shape[1], kw)


ENGINES = {"all": _EngAll, "slots": _EngSlots, "generate": _EngGenerate}


class _Batcher:
    def __init__(self, log, eng):
        self.log, self.eng = log, eng

    def generate(self, inputs_embeds, params, on_tokens=None):
        self.log.append(f"batcher.generate({_summ(inputs_embeds)}; params={_summ(params)}, on_tokens={_summ(on_tokens)})")
        toks = self.eng._model(list(inputs_embeds), params["max_new_tokens"], {"stop_ids": params.get("stop_ids")})[0]
        if on_tokens is not None:
            on_tokens(toks, 0)
        return toks.view(1, -1)

    def run_exclusive(self, fn):
        self.log.append("batcher.run_exclusive(")
        try:
            return fn()
        finally:
            self.log.append(f") left in the job: {M._in_exclusive_job()}")


class _Streamer:
    def __init__(self):
        self.events = []

    def put(self, t):
        self.events.append(["put", list(t.shape), t.flatten().tolist()])

    def end(self):
        self.events.append(["end"])


class _NoStops:
    pass


def _emb(B, S, D=3):
    return ((torch.arange(B * S * D).view(B, S, D) * 7 + 3) % 5).float()


def _mask(form, B, S):
    if not isinstance(form, str):
        return torch.tensor(form)
    m = torch.ones(B, S, dtype=torch.long)
    for b in range(B):
        pads = (2, 0, 1)[b % 3] if form != "ones" else 0
        if pads and form == "left":
            m[b, :pads] = 0
        elif pads:
            m[b, S - pads:] = 0
    return m


def _result(out):
    if isinstance(out, torch.Tensor):
        return {"type": "Tensor", "tokens": out.tolist()}
    keys = [k for k in out.keys() if out[k] is not None]
    kind = "extension" if any(k in keys for k in EXTENSION_FIELDS) else ("beam" if "beam_indices" in out.keys() or "Beam" in type(out).__name__ else "plain")
    return {"type": kind, "fields": _summ({k: out[k] for k in keys}), "tokens": out["sequences"].tolist()}


def _run_a(case):
    """kw: generate's keywords, plus emb=(B, S), mask="ones" | "left" | "right" | rows, stop=True (the pair row 0 emits at steps 2-3),
    streamer=True; opt: engine=dict(max_batch=, free=), self_seed=, inside_job=True"""
    _, caps, with_batcher, kw, opt = case
    log, kw = [], dict(kw)
    eng = ENGINES[caps](log, **opt.get("engine", {}))
    lm = HipCausalLM.__new__(HipCausalLM)
    torch.nn.Module.__init__(lm)
    object.__setattr__(lm, "_engine", eng)
    lm.eos_token_id, lm.pad_token_id, lm.seed = 0, 99, opt.get("self_seed")
    if with_batcher:
        lm.batcher = _Batcher(log, eng)
    shape = kw.pop("emb", (2, 6))
    if shape is not None:
        kw["inputs_embeds"] = _emb(*shape)
    form = kw.pop("mask", None)
    if form is not None:
        kw["attention_mask"] = _mask(form, *shape)
    if kw.pop("stop", False):
        row0 = kw["inputs_embeds"][0] if form is None else kw["inputs_embeds"][0][kw["attention_mask"][0].bool()]
        kw["stopping_criteria"] = [StoppingCriteriaSub(stops=[_EngGenerate._stream(row0, 4)[2:4]])]
    streamer = _Streamer() if kw.pop("streamer", False) else None
    if streamer is not None:
        kw["streamer"] = streamer
    torch.manual_seed(1234)
    before = torch.get_rng_state()
    M._EXCLUSIVE.active = bool(opt.get("inside_job"))
    try:
        rec = {"result": _result(lm.generate(**kw))}
    except Exception as e:                                  # noqa: BLE001 -- the exception is what the case records
        rec = {"raises": [type(e).__name__, str(e)]}
    finally:
        M._EXCLUSIVE.active = False
    rec["calls"] = log
    if streamer is not None:
        rec["streamer"] = streamer.events
    rec["rng_changed"] = not torch.equal(before, torch.get_rng_state())
    return rec


RD = dict(return_dict_in_generate=True)
SAMPLE = dict(do_sample=True, seed=11, temperature=0.7, top_p=0.9, top_k=5, repetition_penalty=1.2)
ONE = dict(emb=(1, 6))
BIG = dict(emb=(4, 6))
SMALL = dict(engine=dict(max_batch=3))
JOB = dict(inside_job=True)
RIGHT_EMPTY = [[1, 1, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0]]

A_CASES = [
    # ---- the classic route: generate / generate_shared / generate_processed
    ("classic/greedy defaults", "all", False, dict(max_length=11), {}),
    ("classic/greedy on an engine with generate alone", "generate", False, dict(max_length=11), {}),
    ("classic/sampling, pinned seed", "all", False, dict(max_length=11, **SAMPLE), {}),
    ("classic/sampling, the seed of the object", "all", False, dict(max_length=11, do_sample=True), dict(self_seed=5)),
    ("classic/sampling, a pinned seed wins over the object's", "all", False, dict(max_length=11, do_sample=True, seed=2 ** 63 + 9), dict(self_seed=5)),
    ("classic/sampling, drawn seed", "all", False, dict(max_length=11, do_sample=True), {}),
    ("classic/temperature None", "all", False, dict(max_length=11, temperature=None, do_sample=True, seed=1), {}),
    ("classic/top_p None", "all", False, dict(max_length=11, top_p=None, do_sample=True, seed=1), {}),
    ("classic/top_k None", "all", False, dict(max_length=11, top_k=None, do_sample=True, seed=1), {}),
    ("classic/repetition_penalty None", "all", False, dict(max_length=11, repetition_penalty=None), {}),
    ("classic/length_penalty None", "all", False, dict(max_length=11, length_penalty=None, num_beams=2), {}),
    ("classic/pad_token_id None, eos_token_id given", "all", False, dict(max_length=11, pad_token_id=None, eos_token_id=4), {}),
    ("classic/eos_token_id None, pad_token_id given", "all", False, dict(max_length=11, eos_token_id=None, pad_token_id=5), {}),
    ("classic/min_p None", "all", False, dict(max_length=11, min_p=None, do_sample=True, seed=1), {}),
    ("classic/every default None", "all", False, dict(max_length=11, temperature=None, top_p=None, top_k=None, repetition_penalty=None,
                                                    length_penalty=None, pad_token_id=None, eos_token_id=None, min_p=None), {}),
    ("classic/stop sequence", "all", False, dict(max_length=14, stop=True), {}),
    ("classic/empty stopping criteria", "all", False, dict(max_length=11, stopping_criteria=[]), {}),
    ("classic/min_length above the prompt length", "all", False, dict(max_length=14, min_length=9), {}),
    ("classic/min_length below the prompt length", "all", False, dict(max_length=14, min_length=3), {}),
    ("classic/the engine refuses an exhausted budget", "all", False, dict(max_length=6), {}),
    ("classic/all-ones mask", "all", False, dict(max_length=11, mask="ones"), {}),
    ("classic/use_cache False and unknown keywords", "all", False, dict(max_length=11, use_cache=False, output_attentions=True, foo=1), {}),
    ("classic/beams", "all", False, dict(max_length=11, num_beams=2, length_penalty=0.5, early_stopping=True), {}),
    ("classic/beams never, beam-sample", "all", False, dict(max_length=11, num_beams=8, early_stopping="never", do_sample=True, seed=3, min_length=8), {}),
    ("classic/beams, return_dict", "all", False, dict(max_length=9, num_beams=2, **RD), {}),
    ("classic/beams, return_dict, scores", "all", False, dict(max_length=9, num_beams=2, output_scores=True, **RD), {}),
    ("classic/return_dict alone", "all", False, dict(max_length=9, **RD), {}),
    ("classic/return_dict, scores and logits", "all", False, dict(max_length=9, output_scores=True, output_logits=True, **RD), {}),
    ("classic/return_dict, logits: the engine refuses an exhausted budget", "all", False, dict(max_length=6, output_logits=True, **RD), {}),
    ("classic/output_scores without return_dict is ignored", "all", False, dict(max_length=9, output_scores=True, output_token_logprobs=True), {}),
    ("classic/token statistics", "all", False, dict(max_length=9, output_token_logprobs=True, **RD), {}),
    ("classic/token statistics, two names", "all", False, dict(max_length=9, output_token_logprobs=("token_logprobs", "token_entropies"), **RD), {}),
    ("classic/top-k lists", "all", False, dict(max_length=9, output_top_logprobs=3, **RD), {}),
    ("classic/top-k lists, processed, with statistics and scores", "all", False,
     dict(max_length=9, output_top_logprobs=2, top_logprobs_source="processed", output_token_logprobs=True, output_scores=True, **RD), {}),
    ("classic/output_top_logprobs False is not asked", "all", False, dict(max_length=9, output_top_logprobs=False), {}),
    ("classic/streamer", "all", False, dict(max_length=9, streamer=True), {}),
    ("classic/streamer, return_dict", "all", False, dict(max_length=9, streamer=True, **RD), {}),
    ("shared/three samples", "all", False, dict(max_length=9, num_return_sequences=3, do_sample=True, seed=11), {}),
    ("shared/three samples, streamer", "all", False, dict(max_length=9, num_return_sequences=3, streamer=True), {}),
    ("shared/share_prompt False repeats", "all", False, dict(max_length=9, num_return_sequences=3, do_sample=True, seed=11, share_prompt=False), {}),
    ("shared/an engine without the shared call repeats", "generate", False, dict(max_length=9, num_return_sequences=2, do_sample=True, seed=11), {}),
    ("shared/num_return_sequences None", "all", False, dict(max_length=9, num_return_sequences=None), {}),
    ("shared/scores", "all", False, dict(max_length=9, num_return_sequences=2, output_scores=True, **RD), {}),
    ("processed/no_repeat_ngram_size", "all", False, dict(max_length=9, no_repeat_ngram_size=2), {}),
    ("processed/bad words, the eos word dropped", "all", False, dict(max_length=9, bad_words_ids=[[3, 4], (5,), [0]]), {}),
    ("processed/bad words, eos given", "all", False, dict(max_length=9, bad_words_ids=[[3, 4], [5]], eos_token_id=5), {}),
    ("processed/min_p sampling, two samples", "all", False, dict(max_length=9, min_p=0.25, do_sample=True, seed=3, num_return_sequences=2), {}),
    ("processed/min_p greedy builds no warper", "all", False, dict(max_length=9, min_p=0.25), {}),
    ("processed/no_repeat_ngram_size None", "all", False, dict(max_length=9, no_repeat_ngram_size=None), {}),
    ("processed/with statistics and a streamer", "all", False, dict(max_length=9, no_repeat_ngram_size=3, output_token_logprobs=True, streamer=True, **RD), {}),
    # ---- the lookup route
    ("lookup/greedy", "all", False, dict(max_length=9, prompt_lookup_num_tokens=3), {}),
    ("lookup/ngram size, min_length, stop, explicit ids", "all", False,
     dict(max_length=14, prompt_lookup_num_tokens=2, max_matching_ngram_size=2, min_length=8, stop=True, eos_token_id=4, pad_token_id=5), {}),
    ("lookup/repetition_penalty 1.0 and None pass", "all", False, dict(max_length=9, prompt_lookup_num_tokens=3, repetition_penalty=None), {}),
    ("lookup/return_dict", "all", False, dict(max_length=9, prompt_lookup_num_tokens=3, **RD), {}),
    ("lookup/streamer", "all", False, dict(max_length=9, prompt_lookup_num_tokens=3, streamer=True, **ONE), {}),
    ("lookup/sampled", "all", False, dict(max_length=9, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, **SAMPLE), {}),
    ("lookup/sampled, drawn seed", "all", False, dict(max_length=9, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, do_sample=True), {}),
    ("lookup/sampled, greedy with None warpers", "all", False,
     dict(max_length=9, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, temperature=None, top_p=None, top_k=None, repetition_penalty=None), {}),
    ("lookup/sampled, streamer", "all", False, dict(max_length=9, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, streamer=True, **ONE), {}),
    ("lookup/inside an exclusive job the batcher does not refuse", "all", True, dict(max_length=9, prompt_lookup_num_tokens=3), JOB),
    ("lookup/all-ones mask", "all", False, dict(max_length=9, prompt_lookup_num_tokens=3, mask="ones"), {}),
    # ---- padded prompts: slots
    ("slots/left padding", "all", False, dict(max_length=10, mask="left", **BIG), {}),
    ("slots/right padding", "all", False, dict(max_length=10, mask="right", **BIG), {}),
    ("slots/left padding, stop", "all", False, dict(max_length=14, mask="left", stop=True, **BIG), {}),
    ("slots/left padding, eos ends a row", "all", False, dict(max_length=12, mask="left", eos_token_id=_EngGenerate._stream(_emb(2, 6)[1], 3)[2]), {}),
    ("slots/sampling, min_length, None defaults", "all", False,
     dict(max_length=10, mask="left", do_sample=True, seed=7, min_length=8, temperature=None, top_p=None, top_k=None, repetition_penalty=None,
          pad_token_id=None, eos_token_id=None), {}),
    ("slots/sampling, explicit values, drawn seed", "all", False,
     dict(max_length=10, mask="right", do_sample=True, temperature=0.7, top_p=0.9, top_k=5, repetition_penalty=1.2, pad_token_id=5, eos_token_id=4), {}),
    ("slots/return_dict", "all", False, dict(max_length=10, mask="left", **RD), {}),
    ("slots/the streamer is never called", "all", False, dict(max_length=10, mask="left", streamer=True), {}),
    ("slots/per length group without prefill_ragged", "slots", False, dict(max_length=10, mask="left", stop=True, **BIG), {}),
    ("slots/shared samples", "all", False, dict(max_length=10, mask="left", num_return_sequences=2, do_sample=True, seed=5), {}),
    ("slots/shared samples, share_prompt False", "all", False, dict(max_length=10, mask="left", num_return_sequences=2, do_sample=True, seed=5, share_prompt=False), {}),
    ("slots/samples repeat without the group admit", "slots", False, dict(max_length=10, mask="left", num_return_sequences=2, do_sample=True, seed=5), {}),
    ("slots/shared samples beyond max_batch repeat and run by length", "all", False,
     dict(max_length=10, mask="left", num_return_sequences=2, do_sample=True, seed=5), SMALL),
    ("slots/inside an exclusive job", "all", True, dict(max_length=10, mask="left"), JOB),
    ("slots/shared samples inside an exclusive job", "all", True, dict(max_length=10, mask="left", num_return_sequences=2), JOB),
    # ---- padded prompts: beams
    ("padded beams/left padding", "all", False, dict(max_length=10, mask="left", num_beams=2, **BIG), {}),
    ("padded beams/right padding, stop, values", "all", False,
     dict(max_length=14, mask="right", num_beams=3, stop=True, length_penalty=0.5, early_stopping=True, min_length=8, do_sample=True, seed=4,
          temperature=0.7, top_p=0.9, top_k=5, repetition_penalty=1.2, eos_token_id=4, pad_token_id=5), {}),
    ("padded beams/None defaults, return_dict", "all", False,
     dict(max_length=10, mask="left", num_beams=2, temperature=None, top_p=None, top_k=None, length_penalty=None, early_stopping=None, **RD), {}),
    ("padded beams/a batcher queues the search", "all", True, dict(max_length=10, mask="left", num_beams=2), {}),
    ("padded beams/inside an exclusive job", "all", True, dict(max_length=10, mask="left", num_beams=2), JOB),
    # ---- padded prompts: length groups
    ("groups/generate alone, left padding", "generate", False, dict(max_length=10, mask="left", **BIG), {}),
    ("groups/generate alone, stop, min_length, sampling", "generate", False,
     dict(max_length=14, mask="left", stop=True, min_length=8, do_sample=True, seed=6, **BIG), {}),
    ("groups/generate alone, beams", "generate", False, dict(max_length=10, mask="left", num_beams=2, **BIG), {}),
    ("groups/generate alone, drawn seed is drawn once", "generate", False, dict(max_length=10, mask="left", do_sample=True, **BIG), {}),
    ("groups/generate alone, the streamer is never called", "generate", False, dict(max_length=10, mask="left", streamer=True), {}),
    ("groups/B above max_batch", "all", False, dict(max_length=10, mask="left", **BIG), SMALL),
    ("groups/B * num_beams above max_batch", "all", False, dict(max_length=10, mask="left", num_beams=2, **BIG), SMALL),
    ("groups/a batcher: single rows join it, the others run exclusive", "slots", True, dict(max_length=10, mask="left", stop=True, **BIG), {}),
    ("groups/a batcher, generate alone", "generate", True, dict(max_length=10, mask="left", **BIG), {}),
    # ---- a batcher, unpadded
    ("batcher single/greedy", "all", True, dict(max_length=10, **ONE), {}),
    ("batcher single/sampling values, stop, min_length", "all", True, dict(max_length=14, stop=True, min_length=8, eos_token_id=4, pad_token_id=5, **SAMPLE, **ONE), {}),
    ("batcher single/None defaults, drawn seed", "all", True,
     dict(max_length=10, do_sample=True, temperature=None, top_p=None, top_k=None, repetition_penalty=None, **ONE), {}),
    ("batcher single/streamer", "all", True, dict(max_length=10, streamer=True, **ONE), {}),
    ("batcher single/return_dict", "all", True, dict(max_length=10, **RD, **ONE), {}),
    ("exclusive/two rows", "all", True, dict(max_length=10, **SAMPLE), {}),
    ("exclusive/two rows, drawn seed, stop, min_length", "all", True, dict(max_length=14, do_sample=True, stop=True, min_length=8), {}),
    ("exclusive/beams", "all", True, dict(max_length=10, num_beams=2, length_penalty=0.5, early_stopping=True, **ONE), {}),
    ("exclusive/processors", "all", True, dict(max_length=10, no_repeat_ngram_size=3, bad_words_ids=[[4, 5]], **ONE), {}),
    ("exclusive/scores", "all", True, dict(max_length=9, output_scores=True, **RD, **ONE), {}),
    ("exclusive/return_dict, beams", "all", True, dict(max_length=9, num_beams=2, **RD, **ONE), {}),
    ("exclusive/shared samples", "all", True, dict(max_length=10, num_return_sequences=2, do_sample=True, seed=5, **ONE), {}),
    ("exclusive/samples, share_prompt False", "all", True, dict(max_length=10, num_return_sequences=2, do_sample=True, seed=5, share_prompt=False, **ONE), {}),
    ("exclusive/generate alone", "generate", True, dict(max_length=10), {}),
    ("exclusive/streamer", "all", True, dict(max_length=10, streamer=True), {}),
    ("exclusive/streamer, shared samples", "all", True, dict(max_length=10, streamer=True, num_return_sequences=2, **ONE), {}),
    ("exclusive/inside a job the call runs directly", "all", True, dict(max_length=10), JOB),
    ("exclusive/inside a job a single row runs directly", "all", True, dict(max_length=10, streamer=True, **ONE), JOB),
    # ---- the refusals, in the order the method meets them; "pair": both checks violated
    ("raise/inputs_embeds missing", "all", False, dict(emb=None, max_length=10), {}),
    ("raise/pair inputs_embeds + lookup sampling alone", "all", False, dict(emb=None, prompt_lookup_sampling=True), {}),
    ("raise/lookup sampling alone", "all", False, dict(max_length=10, prompt_lookup_sampling=True), {}),
    ("raise/pair lookup sampling alone + output_attentions", "all", False, dict(max_length=10, prompt_lookup_sampling=True, output_attentions=True, **RD), {}),
    ("raise/output_attentions", "all", False, dict(max_length=10, output_attentions=True, **RD), {}),
    ("raise/output_hidden_states", "all", False, dict(max_length=10, output_hidden_states=True, **RD), {}),
    ("raise/pair output_attentions + scores padded", "all", False, dict(max_length=10, output_attentions=True, output_scores=True, mask="left", **RD), {}),
    ("raise/scores padded", "all", False, dict(max_length=10, output_scores=True, mask="left", **RD), {}),
    ("raise/logits padded right", "all", False, dict(max_length=10, output_logits=True, mask="right", **RD), {}),
    ("raise/pair scores padded + statistics beams", "all", False, dict(max_length=10, output_scores=True, mask="left", output_token_logprobs=True, num_beams=2, **RD), {}),
    ("raise/statistics beams", "all", False, dict(max_length=10, output_token_logprobs=True, num_beams=2, **RD), {}),
    ("raise/pair statistics beams + padded", "all", False, dict(max_length=10, output_token_logprobs=True, num_beams=2, mask="left", **RD), {}),
    ("raise/statistics padded", "all", False, dict(max_length=10, output_token_logprobs=True, mask="left", **RD), {}),
    ("raise/pair statistics padded + batcher", "all", True, dict(max_length=10, output_token_logprobs=True, mask="left", **RD), {}),
    ("raise/statistics batcher", "all", True, dict(max_length=10, output_token_logprobs=True, **RD), {}),
    ("raise/statistics batcher, inside a job too", "all", True, dict(max_length=10, output_token_logprobs=True, **RD), JOB),
    ("raise/pair statistics batcher + top-k k", "all", True, dict(max_length=10, output_token_logprobs=True, output_top_logprobs=33, **RD), {}),
    ("raise/top-k k 33", "all", False, dict(max_length=10, output_top_logprobs=33, **RD), {}),
    ("raise/top-k k True", "all", False, dict(max_length=10, output_top_logprobs=True, **RD), {}),
    ("raise/top-k source", "all", False, dict(max_length=10, output_top_logprobs=3, top_logprobs_source="warped", **RD), {}),
    ("raise/pair top-k k + no return_dict", "all", False, dict(max_length=10, output_top_logprobs=0), {}),
    ("raise/top-k without return_dict", "all", False, dict(max_length=10, output_top_logprobs=3), {}),
    ("raise/pair top-k without return_dict + beams", "all", False, dict(max_length=10, output_top_logprobs=3, num_beams=2), {}),
    ("raise/top-k beams", "all", False, dict(max_length=10, output_top_logprobs=3, num_beams=2, **RD), {}),
    ("raise/pair top-k beams + padded", "all", False, dict(max_length=10, output_top_logprobs=3, num_beams=2, mask="right", **RD), {}),
    ("raise/top-k padded", "all", False, dict(max_length=10, output_top_logprobs=3, mask="right", **RD), {}),
    ("raise/pair top-k padded + batcher", "all", True, dict(max_length=10, output_top_logprobs=3, mask="right", **RD), {}),
    ("raise/top-k batcher", "all", True, dict(max_length=10, output_top_logprobs=3, **RD), {}),
    ("raise/pair top-k batcher + no_repeat_ngram_size", "all", True, dict(max_length=10, output_top_logprobs=3, no_repeat_ngram_size=-1, **RD), {}),
    ("raise/no_repeat_ngram_size -1", "all", False, dict(max_length=10, no_repeat_ngram_size=-1), {}),
    ("raise/no_repeat_ngram_size 1.5", "all", False, dict(max_length=10, no_repeat_ngram_size=1.5), {}),
    ("raise/no_repeat_ngram_size True", "all", False, dict(max_length=10, no_repeat_ngram_size=True), {}),
    ("raise/pair no_repeat_ngram_size + bad_words_ids", "all", False, dict(max_length=10, no_repeat_ngram_size=-1, bad_words_ids=[]), {}),
    ("raise/bad_words_ids empty", "all", False, dict(max_length=10, bad_words_ids=[]), {}),
    ("raise/bad_words_ids no list", "all", False, dict(max_length=10, bad_words_ids=3), {}),
    ("raise/bad_words_ids empty word", "all", False, dict(max_length=10, bad_words_ids=[[1], []]), {}),
    ("raise/pair bad_words_ids empty word + negative id", "all", False, dict(max_length=10, bad_words_ids=[[-1], []]), {}),
    ("raise/bad_words_ids negative id", "all", False, dict(max_length=10, bad_words_ids=[[1, -2]]), {}),
    ("raise/pair bad_words_ids negative id + min_p", "all", False, dict(max_length=10, bad_words_ids=[[1, -2]], min_p=2.0), {}),
    ("raise/min_p 2", "all", False, dict(max_length=10, min_p=2.0), {}),
    ("raise/pair min_p + limits", "all", False, dict(max_length=10, min_p=-0.5, no_repeat_ngram_size=9), {}),
    ("raise/limits no_repeat_ngram_size 9", "all", False, dict(max_length=10, no_repeat_ngram_size=9), {}),
    ("raise/limits bad word outside the vocabulary", "all", False, dict(max_length=10, bad_words_ids=[[1, 7]]), {}),
    ("raise/pair limits + processors beams", "all", False, dict(max_length=10, no_repeat_ngram_size=9, num_beams=2), {}),
    ("raise/processors beams", "all", False, dict(max_length=10, no_repeat_ngram_size=2, num_beams=2), {}),
    ("raise/pair processors beams + padded", "all", False, dict(max_length=10, bad_words_ids=[[1, 2]], num_beams=2, mask="left"), {}),
    ("raise/processors padded", "all", False, dict(max_length=10, min_p=0.2, do_sample=True, mask="left"), {}),
    ("raise/processors padded leave the generator alone", "all", False, dict(max_length=10, no_repeat_ngram_size=2, do_sample=True, mask="left"), {}),
    ("raise/pair processors padded + num_beams 0, before the draw", "all", False, dict(max_length=10, no_repeat_ngram_size=2, mask="left", num_beams=0, do_sample=True), {}),
    ("raise/num_beams 0", "all", False, dict(max_length=10, num_beams=0), {}),
    ("raise/num_beams 9 after the draw", "all", False, dict(max_length=10, num_beams=9, do_sample=True), {}),
    ("raise/num_beams 2 with a processor before the draw", "all", False, dict(max_length=10, num_beams=2, no_repeat_ngram_size=2, do_sample=True), {}),
    ("raise/pair num_beams 0 + num_return_sequences", "all", False, dict(max_length=10, num_beams=0, num_return_sequences=-1), {}),
    ("raise/pair num_beams 9 + num_return_sequences", "all", False, dict(max_length=10, num_beams=9, num_return_sequences=-1), {}),
    ("raise/num_return_sequences -1", "all", False, dict(max_length=10, num_return_sequences=-1), {}),
    ("raise/several sequences under beam search", "all", False, dict(max_length=10, num_return_sequences=2, num_beams=2), {}),
    ("raise/pair several sequences under beam search + repetition_penalty", "all", False, dict(max_length=10, num_return_sequences=2, num_beams=2, repetition_penalty=0), {}),
    ("raise/repetition_penalty 0", "all", False, dict(max_length=10, repetition_penalty=0.0), {}),
    ("raise/pair repetition_penalty + lookup K", "all", False, dict(max_length=10, repetition_penalty=-1.0, prompt_lookup_num_tokens=-2), {}),
    ("raise/lookup K -2", "all", False, dict(max_length=10, prompt_lookup_num_tokens=-2), {}),
    ("raise/pair lookup K + refused", "all", False, dict(max_length=10, prompt_lookup_num_tokens=-2, do_sample=True, seed=1), {}),
    ("raise/lookup do_sample", "all", False, dict(max_length=10, prompt_lookup_num_tokens=3, do_sample=True, seed=1), {}),
    ("raise/lookup repetition_penalty", "all", False, dict(max_length=10, prompt_lookup_num_tokens=3, repetition_penalty=1.2), {}),
    ("raise/lookup beams, samples, padded mask, streamer rows", "all", False,
     dict(max_length=10, prompt_lookup_num_tokens=3, num_beams=2, mask="left", streamer=True), {}),
    ("raise/lookup samples", "all", False, dict(max_length=10, prompt_lookup_num_tokens=3, num_return_sequences=2), {}),
    ("raise/lookup processors, scores, statistics, lists", "all", False,
     dict(max_length=10, prompt_lookup_num_tokens=3, no_repeat_ngram_size=2, output_scores=True, output_token_logprobs=True, output_top_logprobs=2, **RD), {}),
    ("raise/lookup batcher", "all", True, dict(max_length=10, prompt_lookup_num_tokens=3), {}),
    ("raise/lookup sampled: beams, samples", "all", False,
     dict(max_length=10, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, do_sample=True, seed=1, repetition_penalty=1.3, num_beams=2), {}),
    ("raise/lookup sampled: padded, batcher, streamer rows", "all", True,
     dict(max_length=10, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, mask="right", streamer=True), {}),
    ("raise/pair lookup refused + no such engine call", "generate", False, dict(max_length=10, prompt_lookup_num_tokens=3, do_sample=True, seed=1), {}),
    ("raise/lookup on an engine without it", "generate", False, dict(max_length=10, prompt_lookup_num_tokens=3), {}),
    ("raise/lookup sampled on an engine without it", "slots", False, dict(max_length=10, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True), {}),
    ("raise/lookup unsupported stopping criterion", "all", False, dict(max_length=10, prompt_lookup_num_tokens=3, stopping_criteria=[_NoStops()]), {}),
    ("raise/padded right without prefill_ragged", "slots", False, dict(max_length=10, mask="right"), {}),
    ("raise/padded right without prefill_ragged, generate alone", "generate", False, dict(max_length=10, mask="right"), {}),
    ("raise/padded row without a real position", "all", False, dict(max_length=10, mask=RIGHT_EMPTY), {}),
    ("raise/pair padded row without a real position + budget", "all", False, dict(max_length=6, mask=RIGHT_EMPTY), {}),
    ("raise/padded budget", "all", False, dict(max_length=6, mask="left"), {}),
    ("raise/pair padded budget + stopping criterion", "all", False, dict(max_length=6, mask="left", stopping_criteria=[_NoStops()]), {}),
    ("raise/padded unsupported stopping criterion", "all", False, dict(max_length=10, mask="left", stopping_criteria=[_NoStops()]), {}),
    ("raise/unsupported stopping criterion", "all", False, dict(max_length=10, stopping_criteria=[_NoStops()]), {}),
    ("raise/pair unsupported stopping criterion + two stop sequences", "all", False,
     dict(max_length=10, stopping_criteria=[StoppingCriteriaSub(stops=[[1], [2]]), _NoStops()]), {}),
    ("raise/two stop sequences", "all", False, dict(max_length=10, stopping_criteria=[StoppingCriteriaSub(stops=[[1], [2]])]), {}),
    ("raise/two stop sequences, batcher single", "all", True, dict(max_length=10, stopping_criteria=[StoppingCriteriaSub(stops=[[1]]), StoppingCriteriaSub(stops=[[2]])], **ONE), {}),
    ("raise/streamer beams", "all", False, dict(max_length=10, streamer=True, num_beams=2), {}),
    ("raise/streamer beams, batcher", "all", True, dict(max_length=10, streamer=True, num_beams=2), {}),
    ("raise/pair streamer beams + slabs do not fit", "all", False, dict(max_length=10, streamer=True, num_beams=2, output_scores=True, **RD), dict(engine=dict(free=100))),
    ("raise/slabs do not fit", "all", False, dict(max_length=10, output_scores=True, output_logits=True, **RD), dict(engine=dict(free=100))),
    ("raise/slabs do not fit, exclusive", "all", True, dict(max_length=10, output_scores=True, **RD), dict(engine=dict(free=100))),
]


# ---- part B: HipEngine.generate and its family over a recording library ------------------------------------------------------------------------
def _field(struct, name, ctype):
    v = getattr(struct, name)
    if ctype is C.c_void_p:
        return bool(v)
    if isinstance(ctype, type) and issubclass(ctype, C._Pointer):
        if name == "stop_ids":
            return [v[i] for i in range(struct.n_stop)] if v else None
        if name == "bad_word_lens":
            return [v[i] for i in range(struct.n_bad_words)] if v else None
        if name == "bad_word_ids":
            return [v[i] for i in range(sum(struct.bad_word_lens[j] for j in range(struct.n_bad_words)))] if v else None
        return bool(v)
    return v


def _arg(a):
    if a is None or isinstance(a, (int, float)):
        return a
    if isinstance(a, C.c_void_p):
        return "ptr" if a.value else None
    if isinstance(a, C.Array):
        return list(a)
    obj = getattr(a, "_obj", None)                          # C.byref(...)
    if isinstance(obj, C.Structure):
        return f"{type(obj).__name__}(" + ", ".join(f"{n}={_field(obj, n, t)!r}" for n, t in obj._fields_) + ")"
    if isinstance(obj, C.c_int32):
        return "int32*"
    return f"<{type(a).__name__}>"


class _RecLib:
    """Stands in for the loaded library: every entry point records its arguments, reports one generated column and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            if name.startswith("sv_generate"):                  # (not what the engine object does when it is collected)
                self.calls.append(f"{name}(" + ", ".join(str(_arg(a)) for a in args) + ")")
            for a in args:
                if isinstance(getattr(a, "_obj", None), C.c_int32):
                    a._obj.value = 1
                    break
            return 0
        return entry


def _prompts(form):
    x = ((torch.arange(7 * 4).view(7, 4) * 3 + 1) % 5).to(torch.bfloat16)
    if form == "rect":
        return (x[:6].view(2, 3, 4).contiguous(),), {}
    if form == "packed":
        return (x,), {"lengths": [3, 4]}
    if form == "list":
        return ([x[:3], x[3:]],), {}
    if form == "wide":
        return (torch.zeros(2, 3, 5, dtype=torch.bfloat16),), {}
    if form == "empty list":
        return ([],), {}
    if form == "packed 3d":
        return (x.view(1, 7, 4),), {"lengths": [3, 4]}
    if form == "packed, lengths off":
        return (x,), {"lengths": [3, 5]}
    raise KeyError(form)


def _shape(v):
    if isinstance(v, torch.Tensor):
        return _summ(v, False)
    if isinstance(v, dict):
        return {k: _shape(x) for k, x in sorted(v.items())}
    if isinstance(v, tuple):
        return [_shape(x) for x in v]
    return v


def _run_b(case, monkeypatch):
    """kw: the method's keywords, plus slabs=("scores_out", ...) | "bad shape" | "two widths", on_tokens=True"""
    _, method, form, kw = case
    monkeypatch.setattr(E, "_need", lambda t, dtype, what: t.contiguous())
    monkeypatch.setattr(E, "_stream", lambda: None)
    eng = E.HipEngine.__new__(E.HipEngine)
    eng.lib, eng._h, eng.cfg = _RecLib(), C.c_void_p(1), types.SimpleNamespace(hidden=4, vocab=5)
    args, more = _prompts(form)
    kw = dict(kw, **more)
    slabs = kw.pop("slabs", ())
    if slabs == "bad shape":
        kw["scores_out"] = torch.zeros(7, 3, 5)
    elif slabs == "two widths":
        kw.update(scores_out=torch.zeros(7, 2, 5), logits_out=torch.zeros(7, 2, 6))
    else:
        rows = 2 * int(kw.get("num_beams", 1)) * int(kw.get("n_samples", 1))
        kw.update({n: torch.zeros(7, rows, 5) for n in slabs})
    if kw.pop("on_tokens", False):
        kw["on_tokens"] = lambda toks, first: None
    try:
        rec = {"result": _shape(getattr(eng, method)(*args, **kw))}
    except Exception as e:                                  # noqa: BLE001 -- the exception is what the case records
        rec = {"raises": [type(e).__name__, str(e)]}
    rec["calls"] = eng.lib.calls
    return rec


ML = dict(max_length=10)
LK = dict(max_length=10, num_draft_tokens=3)
VALUES = dict(do_sample=True, temperature=0.75, top_p=0.5, eos_token_id=4, pad_token_id=5, seed=2 ** 64 + 3, sync_every=8, repetition_penalty=1.5,
              length_penalty=0.5, top_k=6, min_new_tokens=2)

B_CASES = [
    ("generate/plain", "generate", "rect", ML),
    ("generate/every value", "generate", "rect", dict(ML, stop_ids=[7, 8], on_tokens=True, **VALUES)),
    ("generate/None and negative scalars", "generate", "rect", dict(ML, top_k=None, min_new_tokens=-3, stop_ids=[], early_stopping=None)),
    ("generate/beams", "generate", "rect", dict(ML, num_beams=3, early_stopping="never")),
    ("generate_ex/return_outputs", "generate", "rect", dict(ML, return_outputs=True)),
    ("generate_ex/beams with return_outputs", "generate", "rect", dict(ML, num_beams=2, early_stopping=True, return_outputs=True)),
    ("generate_ex/slabs", "generate", "rect", dict(ML, slabs=("scores_out", "logits_out"))),
    ("generate_ex/beams, scores", "generate", "rect", dict(ML, num_beams=2, slabs=("scores_out",))),
    ("ragged/lengths", "generate", "packed", ML),
    ("ragged/generate_ragged list", "generate_ragged", "list", dict(ML, stop_ids=[7], min_new_tokens=2)),
    ("ragged/generate_ragged packed, beams, return_outputs", "generate_ragged", "packed", dict(ML, num_beams=2, return_outputs=True)),
    ("shared/n_samples", "generate", "rect", dict(ML, n_samples=3, do_sample=True, seed=5)),
    ("shared/generate_shared rect", "generate_shared", "rect", dict(ML, n_samples=2, on_tokens=True)),
    ("shared/generate_shared list", "generate_shared", "list", dict(ML, n_samples=2)),
    ("shared/generate_shared packed, return_outputs", "generate_shared", "packed", dict(ML, n_samples=2, return_outputs=True)),
    ("shared/generate_shared one sample is generate", "generate_shared", "rect", dict(ML, n_samples=1)),
    ("processed/rect", "generate_processed", "rect", dict(ML, no_repeat_ngram_size=2, bad_words_ids=[[3], [1, 2]], min_p=0.25, do_sample=True)),
    ("processed/list, samples", "generate_processed", "list", dict(ML, no_repeat_ngram_size=3, n_samples=2)),
    ("processed/packed", "generate_processed", "packed", dict(ML, bad_words_ids=[[4]])),
    ("processed/all off", "generate_processed", "rect", ML),
    ("stats/True", "generate", "rect", dict(ML, token_stats=True)),
    ("stats/two names, processors, samples, ragged", "generate_processed", "list",
     dict(ML, no_repeat_ngram_size=2, n_samples=2, token_stats=("token_logprobs", "token_entropies"))),
    ("topk/k", "generate", "rect", dict(ML, token_topk=3)),
    ("topk/dict, statistics, slabs", "generate", "rect",
     dict(ML, token_topk=dict(k=2, source="processed", rank=False), token_stats=True, slabs=("logits_out",))),
    ("topk/False is not asked", "generate", "rect", dict(ML, token_topk=False)),
    ("lookup/rect", "generate_lookup", "rect", LK),
    ("lookup/every value, packed", "generate_lookup", "packed",
     dict(LK, max_ngram=4, min_ngram=2, eos_token_id=4, pad_token_id=5, stop_ids=[7, 8], sync_every=8, min_new_tokens=2, return_counts=True)),
    ("lookup/list, on_tokens, off values pass", "generate_lookup", "list",
     dict(LK, on_tokens=True, do_sample=False, num_beams=1, repetition_penalty=1.0, logits_processors=None, n_samples=1, token_stats=False)),
    ("lookup_sampled/rect", "generate_lookup_sampled", "rect", LK),
    ("lookup_sampled/every value, list", "generate_lookup_sampled", "list",
     dict(LK, max_ngram=4, min_ngram=2, eos_token_id=4, pad_token_id=5, stop_ids=[7], sync_every=8, min_new_tokens=2, do_sample=True, temperature=0.75,
          top_k=6, top_p=0.5, seed=2 ** 64 + 3, repetition_penalty=1.5, return_counts=True, on_tokens=True)),
    ("lookup_sampled/None scalars, packed", "generate_lookup_sampled", "packed", dict(LK, top_k=None, repetition_penalty=None, min_new_tokens=None)),
    # the refusals of generate, in its order
    ("raise/token_topk k", "generate", "rect", dict(ML, token_topk=40)),
    ("raise/token_topk unknown key", "generate", "rect", dict(ML, token_topk=dict(k=2, best=True))),
    ("raise/token_topk beams", "generate", "rect", dict(ML, token_topk=2, num_beams=2)),
    ("raise/pair token_topk beams + hidden size", "generate", "wide", dict(ML, token_topk=2, num_beams=2)),
    ("raise/hidden size", "generate", "wide", ML),
    ("raise/packed: empty list", "generate_ragged", "empty list", ML),
    ("raise/packed: not 2-d", "generate", "packed 3d", ML),
    ("raise/packed: lengths do not add up", "generate", "packed, lengths off", ML),
    ("raise/pair hidden size + n_samples", "generate", "wide", dict(ML, n_samples=0)),
    ("raise/n_samples 0", "generate", "rect", dict(ML, n_samples=0)),
    ("raise/pair n_samples + processors beams", "generate_processed", "rect", dict(ML, n_samples=0, no_repeat_ngram_size=2, num_beams=2)),
    ("raise/processors beams", "generate_processed", "rect", dict(ML, no_repeat_ngram_size=2, num_beams=2)),
    ("raise/processors limits", "generate_processed", "rect", dict(ML, no_repeat_ngram_size=9)),
    ("raise/pair processors beams + statistics beams", "generate_processed", "rect", dict(ML, no_repeat_ngram_size=2, num_beams=2, token_stats=True)),
    ("raise/statistics beams", "generate", "rect", dict(ML, num_beams=2, token_stats=True)),
    ("raise/pair statistics beams + samples beams", "generate", "rect", dict(ML, num_beams=2, token_stats=True, n_samples=2)),
    ("raise/samples beams", "generate", "rect", dict(ML, num_beams=2, n_samples=2)),
    ("raise/pair samples beams + budget", "generate", "rect", dict(max_length=3, num_beams=2, n_samples=2)),
    ("raise/budget", "generate", "rect", dict(max_length=3)),
    ("raise/budget from the longest prompt", "generate_ragged", "list", dict(max_length=4)),
    ("raise/pair budget + early_stopping", "generate", "rect", dict(max_length=3, early_stopping="soon")),
    ("raise/early_stopping", "generate", "rect", dict(ML, early_stopping="soon")),
    ("raise/pair early_stopping + slab shape", "generate", "rect", dict(ML, early_stopping="soon", slabs="bad shape")),
    ("raise/slab shape", "generate", "rect", dict(ML, slabs="bad shape")),
    ("raise/slab widths", "generate", "rect", dict(ML, slabs="two widths")),
    ("raise/pair slab shape + statistics names", "generate", "rect", dict(ML, slabs="bad shape", token_stats=("token_logprob",))),
    ("raise/statistics names", "generate", "rect", dict(ML, token_stats=("token_logprob",))),
    ("raise/statistics empty tuple is not asked", "generate", "rect", dict(ML, token_stats=())),
    # generate_lookup / generate_lookup_sampled
    ("raise/lookup do_sample", "generate_lookup", "rect", dict(LK, do_sample=True)),
    ("raise/lookup num_beams", "generate_lookup", "rect", dict(LK, num_beams=2)),
    ("raise/lookup repetition_penalty", "generate_lookup", "rect", dict(LK, repetition_penalty=1.2)),
    ("raise/lookup logits_processors", "generate_lookup", "rect", dict(LK, logits_processors=(1, 2))),
    ("raise/lookup scores_out", "generate_lookup", "rect", dict(LK, scores_out=3)),
    ("raise/lookup logits_out", "generate_lookup", "rect", dict(LK, logits_out=3)),
    ("raise/lookup return_outputs", "generate_lookup", "rect", dict(LK, return_outputs=True)),
    ("raise/lookup token_stats", "generate_lookup", "rect", dict(LK, token_stats=True)),
    ("raise/lookup token_topk", "generate_lookup", "rect", dict(LK, token_topk=3)),
    ("raise/lookup n_samples", "generate_lookup", "rect", dict(LK, n_samples=2)),
    ("raise/lookup pair do_sample + n_samples", "generate_lookup", "rect", dict(LK, n_samples=2, do_sample=True)),
    ("raise/lookup pair n_samples + unexpected", "generate_lookup", "rect", dict(LK, n_samples=2, foo=1)),
    ("raise/lookup unexpected", "generate_lookup", "rect", dict(LK, foo=1, bar=2, seed=3)),
    ("raise/lookup pair unexpected + hidden size", "generate_lookup", "wide", dict(LK, foo=1)),
    ("raise/lookup hidden size", "generate_lookup", "wide", LK),
    ("raise/lookup pair hidden size + budget", "generate_lookup", "wide", dict(max_length=3, num_draft_tokens=3)),
    ("raise/lookup budget", "generate_lookup", "rect", dict(max_length=3, num_draft_tokens=3)),
    ("raise/lookup budget from the longest prompt", "generate_lookup", "list", dict(max_length=4, num_draft_tokens=3)),
    ("raise/lookup packed: lengths do not add up", "generate_lookup", "packed, lengths off", LK),
    ("raise/lookup_sampled num_beams", "generate_lookup_sampled", "rect", dict(LK, num_beams=2)),
    ("raise/lookup_sampled logits_processors", "generate_lookup_sampled", "rect", dict(LK, logits_processors=(1, 2))),
    ("raise/lookup_sampled return_outputs", "generate_lookup_sampled", "rect", dict(LK, return_outputs=True)),
    ("raise/lookup_sampled token_stats", "generate_lookup_sampled", "rect", dict(LK, token_stats=True)),
    ("raise/lookup_sampled token_topk", "generate_lookup_sampled", "rect", dict(LK, token_topk=3)),
    ("raise/lookup_sampled n_samples", "generate_lookup_sampled", "rect", dict(LK, n_samples=2)),
    ("raise/lookup_sampled scores_out, logits_out", "generate_lookup_sampled", "rect", dict(LK, scores_out=3, logits_out=3)),
    ("raise/lookup_sampled pair n_samples + unexpected", "generate_lookup_sampled", "rect", dict(LK, n_samples=2, foo=1)),
    ("raise/lookup_sampled unexpected", "generate_lookup_sampled", "rect", dict(LK, length_penalty=1.0)),
    ("raise/lookup_sampled pair unexpected + temperature", "generate_lookup_sampled", "rect", dict(LK, foo=1, do_sample=True, temperature=0.0)),
    ("raise/lookup_sampled temperature", "generate_lookup_sampled", "rect", dict(LK, do_sample=True, temperature=0.0)),
    ("raise/lookup_sampled top_p", "generate_lookup_sampled", "rect", dict(LK, do_sample=True, top_p=0.0)),
    ("raise/lookup_sampled temperature 0 is fine without do_sample", "generate_lookup_sampled", "rect", dict(LK, temperature=0.0)),
    ("raise/lookup_sampled pair temperature + repetition_penalty", "generate_lookup_sampled", "rect", dict(LK, do_sample=True, top_p=0.0, repetition_penalty=0.0)),
    ("raise/lookup_sampled repetition_penalty", "generate_lookup_sampled", "rect", dict(LK, repetition_penalty=-1.0)),
    ("raise/lookup_sampled pair repetition_penalty + hidden size", "generate_lookup_sampled", "wide", dict(LK, repetition_penalty=-1.0)),
    ("raise/lookup_sampled hidden size", "generate_lookup_sampled", "wide", LK),
    ("raise/lookup_sampled budget", "generate_lookup_sampled", "rect", dict(max_length=3, num_draft_tokens=3)),
]


def _gold():
    with open(FIXTURE) as f:
        return json.load(f)


def _json(rec):
    return json.loads(json.dumps(rec))


def test_table_and_fixture_hold_the_same_cases():
    ids = ["A/" + c[0] for c in A_CASES] + ["B/" + c[0] for c in B_CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    gold = _gold()
    assert sorted(gold) == sorted(ids), (sorted(set(ids) - set(gold)), sorted(set(gold) - set(ids)))
    # a case under raise/ is refused (a few of them state what is NOT refused, and say so); every other case reaches the engine
    for i in ids:
        if "/raise/" not in i:
            assert ("raises" in gold[i]) == ("refuses" in i), i
    # every engine and batcher method of the route table is reached
    reached = {c.split("(")[0] for i in ids if i.startswith("A/") for c in gold[i]["calls"]}
    assert {"generate", "generate_shared", "generate_processed", "generate_lookup", "generate_lookup_sampled", "cb_admit", "cb_admit_shared",
            "generate_ragged", "batcher.generate", "batcher.run_exclusive"} <= reached
    entries = {c.split("(")[0] for i in ids if i.startswith("B/") for c in gold[i]["calls"]}
    assert entries == {"sv_generate", "sv_generate_ex", "sv_generate_ragged", "sv_generate_shared", "sv_generate_processed", "sv_generate_stats",
                       "sv_generate_topk", "sv_generate_lookup", "sv_generate_lookup_sampled"}


@pytest.mark.parametrize("case", A_CASES, ids=[c[0] for c in A_CASES])
def test_model_generate_is_the_recorded_one(case):
    gold = _gold()
    assert "A/" + case[0] in gold, "not in the fixture: record it from the parent"
    assert _json(_run_a(case)) == gold["A/" + case[0]]


@pytest.mark.parametrize("case", B_CASES, ids=[c[0] for c in B_CASES])
def test_engine_generate_is_the_recorded_one(case, monkeypatch):
    gold = _gold()
    assert "B/" + case[0] in gold, "not in the fixture: record it from the parent"
    assert _json(_run_b(case, monkeypatch)) == gold["B/" + case[0]]


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python -m tests.test_generate_routes_host --record")
    rec = {"A/" + c[0]: _run_a(c) for c in A_CASES}
    with pytest.MonkeyPatch.context() as mp:
        rec.update({"B/" + c[0]: _run_b(c, mp) for c in B_CASES})
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"recorded {len(rec)} cases -> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")
