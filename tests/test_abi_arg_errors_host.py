"""CPU: the argument checks that the generate, scoring and continuous-batch admit entry points of the C ABI run in front of the engine check,
pinned to the letter.  Every case calls the built library with a NULL engine; tests/golden/abi_arg_errors.json maps case id ->
[return code, sv_last_error text].  The table reaches every refusal in front of check_ready, one case per adjacent pair of checks that
violates both (which of the two is reported is part of the contract), and the hand-overs between entry points (topk NULL, stats NULL,
an all-zero sv_logits_processors, k == 0), which decide whose name a message carries.

``python -m tests.test_abi_arg_errors_host --record`` rewrites the fixture from the library in the tree."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_arg_errors.json")
P = C.c_void_p(64)                                                 # never dereferenced: the checks come first
NAN, INF = float("nan"), float("inf")


def _arr(v, ty=C.c_int32):
    return (ty * len(v))(*v) if v is not None else None


def _ref(x):
    return C.byref(x) if x is not None else None


# ---- generate family -------------------------------------------------------------------------------------------------------------------------
def _generate(lib, L, entry, embeds=P, B=2, lens=None, S0=4, G=1, sp={}, lp=None, stats=None, topk=None, outs=None, toks=P, n=True):
    """sp / lp / stats / topk / outs: dict of fields over well-formed defaults, None = a NULL pointer; lp["words"] = the bad-word sequences"""
    if sp is not None:
        sp = L.SvSampling(**dict(dict(max_length=14, num_beams=1, temperature=1.0, top_p=1.0, eos_token_id=-1), **sp))
    keep = []
    if lp is not None:
        lp = dict(lp)
        words = lp.pop("words", None)
        if words is not None:
            keep = [_arr([len(w) for w in words]), _arr([i for w in words for i in w])]
            lp.update(n_bad_words=len(words), bad_word_lens=keep[0], bad_word_ids=keep[1])
        lp = L.SvLogitsProcessors(**lp)
    if stats is not None:
        stats = L.SvTokenStats(**dict(dict(dev_logprob=P, dev_logprob_processed=None, dev_entropy=None, ld=10), **stats))
    if topk is not None:
        topk = L.SvTokenTopk(**dict(dict(k=5, source=0, dev_ids=P, dev_logprobs=P, dev_rank=None, ld=10), **topk))
    if outs is not None:
        outs = L.SvGenerateOutputs(**outs)
    ng = C.byref(C.c_int32(0)) if n else None
    head, tail = (None, embeds, B), (toks, ng, None)
    mid = (_arr(lens), S0, G, _ref(sp))
    args = {"sv_generate": head + (S0, _ref(sp)) + tail,
            "sv_generate_ex": head + (S0, _ref(sp), _ref(outs)) + tail,
            "sv_generate_ragged": head + (_arr(lens), _ref(sp), _ref(outs)) + tail,
            "sv_generate_shared": head + mid + (_ref(outs),) + tail,
            "sv_generate_processed": head + mid + (_ref(lp), _ref(outs)) + tail,
            "sv_generate_stats": head + mid + (_ref(lp), _ref(outs), _ref(stats)) + tail,
            "sv_generate_topk": head + mid + (_ref(lp), _ref(outs), _ref(stats), _ref(topk)) + tail}[entry]
    return getattr(lib, entry)(*args)


NGRAM = dict(no_repeat_ngram_size=2)                               # a well-formed processor request
STATS_NULL = dict(dev_logprob=None)                                # every statistics pointer NULL
BEAMS = dict(num_beams=2)
HOLD = dict(eos_token_id=3, min_new_tokens=2)                      # the min-length hold rewrites the raw row

GENERATE = [
    # sv_generate / sv_generate_ex check nothing in front of the engine
    ("generate/ok", "sv_generate", {}),
    ("generate/everything bad", "sv_generate", dict(embeds=None, B=0, S0=0, sp=None, toks=None, n=False)),
    ("generate_ex/ok", "sv_generate_ex", {}),
    ("generate_ex/everything bad", "sv_generate_ex", dict(embeds=None, B=0, S0=0, sp=None, toks=None, n=False, outs=dict(ld=1))),
    # sv_generate_ragged: null, B, lengths (no n_samples)
    ("ragged/ok", "sv_generate_ragged", dict(lens=(3, 5))),
    ("ragged/embeds NULL", "sv_generate_ragged", dict(lens=(3, 5), embeds=None)),
    ("ragged/lens NULL", "sv_generate_ragged", dict(lens=None)),
    ("ragged/sp NULL", "sv_generate_ragged", dict(lens=(3, 5), sp=None)),
    ("ragged/tokens NULL", "sv_generate_ragged", dict(lens=(3, 5), toks=None)),
    ("ragged/n_generated NULL", "sv_generate_ragged", dict(lens=(3, 5), n=False)),
    ("ragged/B 0", "sv_generate_ragged", dict(lens=(3, 5), B=0)),
    ("ragged/B -1", "sv_generate_ragged", dict(lens=(3, 5), B=-1)),
    ("ragged/length 0", "sv_generate_ragged", dict(lens=(3, 0))),
    ("ragged/length -2 first", "sv_generate_ragged", dict(lens=(-2, 0))),
    ("ragged/pair null + B", "sv_generate_ragged", dict(lens=(3, 5), sp=None, B=0)),
    ("ragged/pair B + length", "sv_generate_ragged", dict(lens=(0, 0), B=0)),
    # sv_generate_shared: null, B, n_samples, lengths / S0
    ("shared/ok", "sv_generate_shared", dict(G=3)),
    ("shared/ok ragged, S0 unused", "sv_generate_shared", dict(lens=(3, 5), S0=0, G=3)),
    ("shared/embeds NULL", "sv_generate_shared", dict(embeds=None)),
    ("shared/sp NULL", "sv_generate_shared", dict(sp=None)),
    ("shared/tokens NULL", "sv_generate_shared", dict(toks=None)),
    ("shared/n_generated NULL", "sv_generate_shared", dict(n=False)),
    ("shared/B 0", "sv_generate_shared", dict(B=0)),
    ("shared/n_samples 0", "sv_generate_shared", dict(G=0)),
    ("shared/length 0", "sv_generate_shared", dict(lens=(3, 0))),
    ("shared/S0 0", "sv_generate_shared", dict(S0=0)),
    ("shared/pair null + B", "sv_generate_shared", dict(toks=None, B=0)),
    ("shared/pair B + n_samples", "sv_generate_shared", dict(B=0, G=0)),
    ("shared/pair n_samples + length", "sv_generate_shared", dict(G=0, lens=(0, 5))),
    ("shared/pair n_samples + S0", "sv_generate_shared", dict(G=0, S0=0)),
    # sv_generate_processed: an all-zero (or NULL) lp is sv_generate_shared; otherwise null, the processors, beams, B, n_samples, lengths / S0
    ("processed/lp NULL is shared", "sv_generate_processed", dict(B=0)),
    ("processed/lp all zero is shared", "sv_generate_processed", dict(lp={}, G=0)),
    ("processed/lp all zero ok", "sv_generate_processed", dict(lp={})),
    ("processed/ok", "sv_generate_processed", dict(lp=NGRAM)),
    ("processed/ok words + min_p", "sv_generate_processed", dict(lp=dict(words=[[7], [1, 2]], min_p=0.5), sp=dict(do_sample=1))),
    ("processed/embeds NULL", "sv_generate_processed", dict(lp=NGRAM, embeds=None)),
    ("processed/sp NULL", "sv_generate_processed", dict(lp=NGRAM, sp=None)),
    ("processed/tokens NULL", "sv_generate_processed", dict(lp=NGRAM, toks=None)),
    ("processed/n_generated NULL", "sv_generate_processed", dict(lp=NGRAM, n=False)),
    ("processed/ngram -1", "sv_generate_processed", dict(lp=dict(no_repeat_ngram_size=-1))),
    ("processed/ngram 9", "sv_generate_processed", dict(lp=dict(no_repeat_ngram_size=9))),
    ("processed/n_bad_words -1", "sv_generate_processed", dict(lp=dict(n_bad_words=-1))),
    ("processed/n_bad_words 65", "sv_generate_processed", dict(lp=dict(n_bad_words=65))),
    ("processed/words NULL", "sv_generate_processed", dict(lp=dict(n_bad_words=1))),
    ("processed/min_p 2", "sv_generate_processed", dict(lp=dict(min_p=2.0))),
    ("processed/min_p nan", "sv_generate_processed", dict(lp=dict(min_p=NAN))),
    ("processed/word of 0 ids", "sv_generate_processed", dict(lp=dict(words=[[7], []]))),
    ("processed/word of 9 ids", "sv_generate_processed", dict(lp=dict(words=[list(range(9))]))),
    ("processed/word id -1", "sv_generate_processed", dict(lp=dict(words=[[7], [1, -1]]))),
    ("processed/beams", "sv_generate_processed", dict(lp=NGRAM, sp=BEAMS)),
    ("processed/B 0", "sv_generate_processed", dict(lp=NGRAM, B=0)),
    ("processed/n_samples 0", "sv_generate_processed", dict(lp=NGRAM, G=0)),
    ("processed/length 0", "sv_generate_processed", dict(lp=NGRAM, lens=(3, 0))),
    ("processed/S0 0", "sv_generate_processed", dict(lp=NGRAM, S0=0)),
    ("processed/pair null + ngram", "sv_generate_processed", dict(lp=dict(no_repeat_ngram_size=9), sp=None)),
    ("processed/pair ngram + n_bad_words", "sv_generate_processed", dict(lp=dict(no_repeat_ngram_size=9, n_bad_words=65))),
    ("processed/pair n_bad_words + words NULL", "sv_generate_processed", dict(lp=dict(n_bad_words=-1, min_p=2.0))),
    ("processed/pair words NULL + min_p", "sv_generate_processed", dict(lp=dict(n_bad_words=1, min_p=2.0))),
    ("processed/pair min_p + word length", "sv_generate_processed", dict(lp=dict(words=[[]], min_p=2.0))),
    ("processed/pair word length + id", "sv_generate_processed", dict(lp=dict(words=[[-1], []]))),
    ("processed/pair processors + beams", "sv_generate_processed", dict(lp=dict(min_p=2.0), sp=BEAMS)),
    ("processed/pair beams + B", "sv_generate_processed", dict(lp=NGRAM, sp=BEAMS, B=0)),
    ("processed/pair B + n_samples", "sv_generate_processed", dict(lp=NGRAM, B=0, G=0)),
    ("processed/pair n_samples + length", "sv_generate_processed", dict(lp=NGRAM, G=0, lens=(3, 0))),
    ("processed/pair n_samples + S0", "sv_generate_processed", dict(lp=NGRAM, G=0, S0=0)),
    # sv_generate_stats: stats NULL is sv_generate_processed; otherwise null, the pointers, beams, B, n_samples, lengths / S0, ld, the processors
    ("stats/NULL is processed", "sv_generate_stats", dict(lp=NGRAM, B=0)),
    ("stats/NULL and lp zero is shared", "sv_generate_stats", dict(lp={}, B=0)),
    ("stats/NULL ok", "sv_generate_stats", {}),
    ("stats/ok", "sv_generate_stats", dict(stats={})),
    ("stats/ok with processors", "sv_generate_stats", dict(stats={}, lp=NGRAM, G=2)),
    ("stats/ok ld unchecked without a budget", "sv_generate_stats", dict(stats=dict(ld=0), sp=dict(max_length=4))),
    ("stats/embeds NULL", "sv_generate_stats", dict(stats={}, embeds=None)),
    ("stats/sp NULL", "sv_generate_stats", dict(stats={}, sp=None)),
    ("stats/tokens NULL", "sv_generate_stats", dict(stats={}, toks=None)),
    ("stats/n_generated NULL", "sv_generate_stats", dict(stats={}, n=False)),
    ("stats/all pointers NULL", "sv_generate_stats", dict(stats=STATS_NULL)),
    ("stats/beams", "sv_generate_stats", dict(stats={}, sp=BEAMS)),
    ("stats/B 0", "sv_generate_stats", dict(stats={}, B=0)),
    ("stats/n_samples 0", "sv_generate_stats", dict(stats={}, G=0)),
    ("stats/length 0", "sv_generate_stats", dict(stats={}, lens=(3, 0))),
    ("stats/S0 0", "sv_generate_stats", dict(stats={}, S0=0)),
    ("stats/ld 9", "sv_generate_stats", dict(stats=dict(ld=9))),
    ("stats/ld against the longest", "sv_generate_stats", dict(stats=dict(ld=8), lens=(3, 5))),
    ("stats/ngram 9", "sv_generate_stats", dict(stats={}, lp=dict(no_repeat_ngram_size=9))),
    ("stats/word id -1", "sv_generate_stats", dict(stats={}, lp=dict(words=[[-1]]))),
    ("stats/pair null + pointers", "sv_generate_stats", dict(stats=STATS_NULL, sp=None)),
    ("stats/pair pointers + beams", "sv_generate_stats", dict(stats=STATS_NULL, sp=BEAMS)),
    ("stats/pair beams + B", "sv_generate_stats", dict(stats={}, sp=BEAMS, B=0)),
    ("stats/pair B + n_samples", "sv_generate_stats", dict(stats={}, B=0, G=0)),
    ("stats/pair n_samples + length", "sv_generate_stats", dict(stats={}, G=0, lens=(0, 5))),
    ("stats/pair n_samples + S0", "sv_generate_stats", dict(stats={}, G=0, S0=0)),
    ("stats/pair length + ld", "sv_generate_stats", dict(stats=dict(ld=1), lens=(3, 0))),
    ("stats/pair S0 + ld", "sv_generate_stats", dict(stats=dict(ld=1), S0=0)),
    ("stats/pair ld + processors", "sv_generate_stats", dict(stats=dict(ld=9), lp=dict(min_p=2.0))),
    # sv_generate_topk: topk NULL is sv_generate_stats; otherwise null, the statistics pointers, B, n_samples, lengths / S0, the list request
    # (k, source, pointers, beams, ld, the raw rank behind a rewrite), the statistics' ld, the processors
    ("topk/NULL is stats", "sv_generate_topk", dict(stats=STATS_NULL)),
    ("topk/NULL and stats NULL is processed", "sv_generate_topk", dict(lp=NGRAM, G=0)),
    ("topk/NULL, stats NULL and lp zero is shared", "sv_generate_topk", dict(G=0)),
    ("topk/NULL ok", "sv_generate_topk", {}),
    ("topk/ok", "sv_generate_topk", dict(topk={})),
    ("topk/ok with statistics, rank and processors", "sv_generate_topk", dict(topk=dict(dev_rank=P, source=1), stats={}, lp=NGRAM, G=2)),
    ("topk/ok ld unchecked without a budget", "sv_generate_topk", dict(topk=dict(ld=0), stats=dict(ld=0), sp=dict(max_length=3))),
    ("topk/embeds NULL", "sv_generate_topk", dict(topk={}, embeds=None)),
    ("topk/sp NULL", "sv_generate_topk", dict(topk={}, sp=None)),
    ("topk/tokens NULL", "sv_generate_topk", dict(topk={}, toks=None)),
    ("topk/n_generated NULL", "sv_generate_topk", dict(topk={}, n=False)),
    ("topk/all statistics pointers NULL", "sv_generate_topk", dict(topk={}, stats=STATS_NULL)),
    ("topk/B 0", "sv_generate_topk", dict(topk={}, B=0)),
    ("topk/n_samples 0", "sv_generate_topk", dict(topk={}, G=0)),
    ("topk/length 0", "sv_generate_topk", dict(topk={}, lens=(3, 0))),
    ("topk/S0 0", "sv_generate_topk", dict(topk={}, S0=0)),
    ("topk/k 0", "sv_generate_topk", dict(topk=dict(k=0))),
    ("topk/k 33", "sv_generate_topk", dict(topk=dict(k=33))),
    ("topk/source 2", "sv_generate_topk", dict(topk=dict(source=2))),
    ("topk/ids NULL", "sv_generate_topk", dict(topk=dict(dev_ids=None))),
    ("topk/logprobs NULL", "sv_generate_topk", dict(topk=dict(dev_logprobs=None))),
    ("topk/beams", "sv_generate_topk", dict(topk={}, sp=BEAMS)),
    ("topk/ld 9", "sv_generate_topk", dict(topk=dict(ld=9))),
    ("topk/raw rank behind an n-gram ban", "sv_generate_topk", dict(topk=dict(dev_rank=P), lp=NGRAM)),
    ("topk/raw rank behind bad words", "sv_generate_topk", dict(topk=dict(dev_rank=P), lp=dict(words=[[7]]))),
    ("topk/raw rank behind the min-length hold", "sv_generate_topk", dict(topk=dict(dev_rank=P), sp=HOLD)),
    ("topk/raw rank behind min_p alone is fine", "sv_generate_topk", dict(topk=dict(dev_rank=P), lp=dict(min_p=0.5))),
    ("topk/statistics ld 9", "sv_generate_topk", dict(topk={}, stats=dict(ld=9))),
    ("topk/min_p 2", "sv_generate_topk", dict(topk={}, lp=dict(min_p=2.0))),
    ("topk/pair null + statistics pointers", "sv_generate_topk", dict(topk={}, stats=STATS_NULL, toks=None)),
    ("topk/pair statistics pointers + B", "sv_generate_topk", dict(topk={}, stats=STATS_NULL, B=0)),
    ("topk/pair B + n_samples", "sv_generate_topk", dict(topk={}, B=0, G=0)),
    ("topk/pair n_samples + length", "sv_generate_topk", dict(topk={}, G=0, lens=(0, 5))),
    ("topk/pair n_samples + S0", "sv_generate_topk", dict(topk={}, G=0, S0=0)),
    ("topk/pair length + k", "sv_generate_topk", dict(topk=dict(k=0), lens=(3, 0))),
    ("topk/pair S0 + k", "sv_generate_topk", dict(topk=dict(k=0), S0=0)),
    ("topk/pair k + source", "sv_generate_topk", dict(topk=dict(k=0, source=2))),
    ("topk/pair source + pointers", "sv_generate_topk", dict(topk=dict(source=2, dev_ids=None))),
    ("topk/pair pointers + beams", "sv_generate_topk", dict(topk=dict(dev_logprobs=None), sp=BEAMS)),
    ("topk/pair beams + ld", "sv_generate_topk", dict(topk=dict(ld=9), sp=BEAMS)),
    ("topk/pair ld + raw rank", "sv_generate_topk", dict(topk=dict(ld=9, dev_rank=P), lp=NGRAM)),
    ("topk/pair raw rank + statistics ld", "sv_generate_topk", dict(topk=dict(dev_rank=P), sp=HOLD, stats=dict(ld=9))),
    ("topk/pair statistics ld + processors", "sv_generate_topk", dict(topk={}, stats=dict(ld=9), lp=dict(min_p=2.0))),
]


# ---- scoring family --------------------------------------------------------------------------------------------------------------------------
def _score(lib, L, entry, embeds=P, B=2, S=8, n_keep=4, lens=(9, 20), keep=(3, 5), targets=P, t=1.0, outs=(P, P, None, None), k=4, ids=P, lps=P,
           rank=P):
    if entry == "sv_forward_logits":
        return lib.sv_forward_logits(None, embeds, B, S, n_keep, outs[0], None)
    if entry == "sv_forward_logprobs":
        return lib.sv_forward_logprobs(None, embeds, B, S, n_keep, targets, t, *outs, None)
    if entry == "sv_forward_topk":
        return lib.sv_forward_topk(None, embeds, B, S, n_keep, targets, t, *outs, k, ids, lps, rank, None)
    return lib.sv_forward_logprobs_ragged(None, embeds, B, _arr(lens), _arr(keep), targets, t, *outs, k, ids, lps, rank, None)


NO_OUT = (None, None, None, None)
LOGPROBS, TOPK, RAGGED = "sv_forward_logprobs", "sv_forward_topk", "sv_forward_logprobs_ragged"

SCORING = [
    ("forward_logits/ok", "sv_forward_logits", {}),
    ("forward_logits/everything bad", "sv_forward_logits", dict(embeds=None, B=0, S=0, n_keep=0, outs=NO_OUT)),
    # sv_forward_logprobs: null, outputs, temperature, n_keep
    ("logprobs/ok", LOGPROBS, {}),
    ("logprobs/ok argmax alone", LOGPROBS, dict(outs=(None, None, None, P))),
    ("logprobs/embeds NULL", LOGPROBS, dict(embeds=None)),
    ("logprobs/targets NULL", LOGPROBS, dict(targets=None)),
    ("logprobs/no output", LOGPROBS, dict(outs=NO_OUT)),
    ("logprobs/temperature 0", LOGPROBS, dict(t=0.0)),
    ("logprobs/temperature nan", LOGPROBS, dict(t=NAN)),
    ("logprobs/temperature inf", LOGPROBS, dict(t=INF)),
    ("logprobs/S 0", LOGPROBS, dict(S=0)),
    ("logprobs/n_keep 0", LOGPROBS, dict(n_keep=0)),
    ("logprobs/n_keep above S", LOGPROBS, dict(n_keep=9)),
    ("logprobs/B 0 is the engine's", LOGPROBS, dict(B=0)),
    ("logprobs/pair null + outputs", LOGPROBS, dict(targets=None, outs=NO_OUT)),
    ("logprobs/pair outputs + temperature", LOGPROBS, dict(outs=NO_OUT, t=0.0)),
    ("logprobs/pair temperature + n_keep", LOGPROBS, dict(t=-1.0, n_keep=0)),
    # sv_forward_topk: k == 0 is sv_forward_logprobs; otherwise k, the list pointers, then sv_forward_logprobs' checks under its own name
    ("forward_topk/k 0 is logprobs", TOPK, dict(k=0, outs=NO_OUT)),
    ("forward_topk/k 0 ignores the list pointers", TOPK, dict(k=0, ids=None, lps=None, rank=None)),
    ("forward_topk/k 0 temperature", TOPK, dict(k=0, t=0.0)),
    ("forward_topk/ok", TOPK, {}),
    ("forward_topk/ok the lists alone", TOPK, dict(outs=NO_OUT, rank=None)),
    ("forward_topk/k -1", TOPK, dict(k=-1)),
    ("forward_topk/k 33", TOPK, dict(k=33)),
    ("forward_topk/ids NULL", TOPK, dict(ids=None)),
    ("forward_topk/list logprobs NULL", TOPK, dict(lps=None)),
    ("forward_topk/embeds NULL", TOPK, dict(embeds=None)),
    ("forward_topk/targets NULL", TOPK, dict(targets=None)),
    ("forward_topk/temperature 0", TOPK, dict(t=0.0)),
    ("forward_topk/n_keep 0", TOPK, dict(n_keep=0)),
    ("forward_topk/n_keep above S", TOPK, dict(n_keep=9)),
    ("forward_topk/pair k + null", TOPK, dict(k=33, embeds=None)),
    ("forward_topk/pair list pointers + null", TOPK, dict(ids=None, targets=None)),
    ("forward_topk/pair null + temperature", TOPK, dict(embeds=None, t=0.0)),
    ("forward_topk/pair temperature + n_keep", TOPK, dict(t=NAN, n_keep=0)),
    # sv_forward_logprobs_ragged: null, B, lengths and keeps, temperature, k, the list pointers, outputs
    ("scoring_ragged/ok", RAGGED, {}),
    ("scoring_ragged/ok k 0 ignores the list pointers", RAGGED, dict(k=0, ids=None, lps=None, rank=None)),
    ("scoring_ragged/ok the lists alone", RAGGED, dict(outs=NO_OUT)),
    ("scoring_ragged/embeds NULL", RAGGED, dict(embeds=None)),
    ("scoring_ragged/lens NULL", RAGGED, dict(lens=None)),
    ("scoring_ragged/keep NULL", RAGGED, dict(keep=None)),
    ("scoring_ragged/targets NULL", RAGGED, dict(targets=None)),
    ("scoring_ragged/B 0", RAGGED, dict(B=0)),
    ("scoring_ragged/length 0", RAGGED, dict(lens=(9, 0))),
    ("scoring_ragged/keep 0", RAGGED, dict(keep=(3, 0))),
    ("scoring_ragged/keep above its length", RAGGED, dict(keep=(10, 5))),
    ("scoring_ragged/temperature 0", RAGGED, dict(t=0.0)),
    ("scoring_ragged/temperature inf", RAGGED, dict(t=INF)),
    ("scoring_ragged/k -1", RAGGED, dict(k=-1)),
    ("scoring_ragged/k 33", RAGGED, dict(k=33)),
    ("scoring_ragged/ids NULL", RAGGED, dict(ids=None)),
    ("scoring_ragged/list logprobs NULL", RAGGED, dict(lps=None)),
    ("scoring_ragged/no output", RAGGED, dict(k=0, outs=NO_OUT)),
    ("scoring_ragged/pair null + B", RAGGED, dict(keep=None, B=0)),
    ("scoring_ragged/pair B + length", RAGGED, dict(B=-1, lens=(0, 0))),
    ("scoring_ragged/pair length + keep of one sequence", RAGGED, dict(lens=(9, 0), keep=(3, 0))),
    ("scoring_ragged/pair keep of sequence 0 + length of sequence 1", RAGGED, dict(lens=(9, 0), keep=(0, 5))),
    ("scoring_ragged/pair keep + temperature", RAGGED, dict(keep=(3, 21), t=0.0)),
    ("scoring_ragged/pair temperature + k", RAGGED, dict(t=0.0, k=33)),
    ("scoring_ragged/pair temperature + outputs", RAGGED, dict(t=0.0, k=0, outs=NO_OUT)),
    ("scoring_ragged/pair k + outputs", RAGGED, dict(k=-1, outs=NO_OUT)),
]


# ---- continuous-batch admit family -----------------------------------------------------------------------------------------------------------
def _admit(lib, L, entry, embeds=P, n=2, S0=4, lens=(5, 7), U=2, group=(0, 1), reqs={}, lps=None, slots=True):
    """reqs: fields of every request over well-formed defaults, None = NULL; lps: one dict per request, None = NULL"""
    if reqs is not None:
        one = dict(dict(temperature=1.0, top_p=1.0, max_new_tokens=4, eos_token_id=-1), **reqs)
        reqs = (L.SvCbRequest * max(n, 1))(*[L.SvCbRequest(**one) for _ in range(max(n, 1))])
    if lps is not None:
        lps = (L.SvCbLogprobs * len(lps))(*[L.SvCbLogprobs(**d) for d in lps])
    out = (C.c_int32 * max(n, 1))() if slots else None
    if entry == "sv_cb_admit":
        return lib.sv_cb_admit(None, embeds, n, S0, reqs, out, None)
    if entry == "sv_cb_admit_ragged":
        return lib.sv_cb_admit_ragged(None, embeds, n, _arr(lens), reqs, out, None)
    if entry == "sv_cb_admit_shared":
        return lib.sv_cb_admit_shared(None, embeds, U, _arr(lens), n, _arr(group), reqs, out, None)
    return lib.sv_cb_admit_logprobs(None, embeds, U, _arr(lens), n, _arr(group), reqs, lps, out, None)


def _group_cases(tag, entry):
    """sv_cb_admit_shared and sv_cb_admit_logprobs: null, then the prompt / group description"""
    return [
        (tag + "/ok", entry, {}),
        (tag + "/ok three requests over two prompts", entry, dict(n=3, group=(0, 0, 1))),
        (tag + "/embeds NULL", entry, dict(embeds=None)),
        (tag + "/lens NULL", entry, dict(lens=None)),
        (tag + "/group NULL", entry, dict(group=None)),
        (tag + "/requests NULL", entry, dict(reqs=None)),
        (tag + "/slots NULL", entry, dict(slots=False)),
        (tag + "/n_prompts 0", entry, dict(U=0)),
        (tag + "/n 0", entry, dict(n=0)),
        (tag + "/more prompts than requests", entry, dict(U=3, lens=(5, 7, 9))),
        (tag + "/prompt length 0", entry, dict(lens=(5, 0))),
        (tag + "/group entry negative", entry, dict(group=(0, -1))),
        (tag + "/group entry above n_prompts", entry, dict(group=(0, 2))),
        (tag + "/group out of order", entry, dict(group=(1, 0))),
        (tag + "/prompt without a request", entry, dict(group=(0, 0))),
        (tag + "/pair null + n_prompts", entry, dict(reqs=None, U=0)),
        (tag + "/pair n_prompts + prompt length", entry, dict(U=3, lens=(0, 7, 9))),
        (tag + "/pair prompt length + group entry", entry, dict(lens=(5, 0), group=(0, 2))),
        (tag + "/pair group entry + order", entry, dict(n=3, U=3, lens=(5, 7, 9), group=(0, 3, 2))),
        (tag + "/pair order + prompt without a request", entry, dict(n=3, U=3, lens=(5, 7, 9), group=(0, 2, 0))),
    ]


REC = dict(enable=1, k=4, source=1)
ADMIT = [
    # sv_cb_admit looks at the engine first
    ("admit/ok", "sv_cb_admit", {}),
    ("admit/everything bad", "sv_cb_admit", dict(embeds=None, n=0, S0=0, reqs=None, slots=False)),
    # sv_cb_admit_ragged: null or empty, prompt lengths
    ("admit_ragged/ok", "sv_cb_admit_ragged", {}),
    ("admit_ragged/embeds NULL", "sv_cb_admit_ragged", dict(embeds=None)),
    ("admit_ragged/lens NULL", "sv_cb_admit_ragged", dict(lens=None)),
    ("admit_ragged/requests NULL", "sv_cb_admit_ragged", dict(reqs=None)),
    ("admit_ragged/slots NULL", "sv_cb_admit_ragged", dict(slots=False)),
    ("admit_ragged/n 0", "sv_cb_admit_ragged", dict(n=0)),
    ("admit_ragged/prompt length 0", "sv_cb_admit_ragged", dict(lens=(5, 0))),
    ("admit_ragged/bad requests are the engine's", "sv_cb_admit_ragged", dict(reqs=dict(max_new_tokens=0, semantics=3))),
    ("admit_ragged/pair null + prompt length", "sv_cb_admit_ragged", dict(slots=False, lens=(0, 7))),
] + _group_cases("admit_shared", "sv_cb_admit_shared") + _group_cases("admit_logprobs", "sv_cb_admit_logprobs") + [
    # sv_cb_admit_logprobs: what each request records, behind the group description
    ("admit_logprobs/ok records", "sv_cb_admit_logprobs", dict(lps=[REC, dict(enable=1, k=0, source=0)])),
    ("admit_logprobs/ok a request that does not record is not looked at", "sv_cb_admit_logprobs", dict(lps=[REC, dict(enable=0, k=99, source=7)])),
    ("admit_logprobs/k -1", "sv_cb_admit_logprobs", dict(lps=[REC, dict(REC, k=-1)])),
    ("admit_logprobs/k 33", "sv_cb_admit_logprobs", dict(lps=[dict(REC, k=33), REC])),
    ("admit_logprobs/source 2", "sv_cb_admit_logprobs", dict(lps=[REC, dict(REC, source=2)])),
    ("admit_logprobs/raw source on a vLLM request", "sv_cb_admit_logprobs", dict(reqs=dict(semantics=1), lps=[REC, dict(REC, source=0)])),
    ("admit_logprobs/pair group + records", "sv_cb_admit_logprobs", dict(group=(0, 0), lps=[dict(REC, k=33), REC])),
    ("admit_logprobs/pair k + source", "sv_cb_admit_logprobs", dict(lps=[dict(REC, k=33, source=2), REC])),
    ("admit_logprobs/pair source + raw source on a vLLM request", "sv_cb_admit_logprobs", dict(reqs=dict(semantics=1), lps=[dict(REC, source=-1), REC])),
    ("admit_logprobs/pair request 0 + request 1", "sv_cb_admit_logprobs", dict(lps=[dict(REC, source=2), dict(REC, k=33)])),
]

CASES = [(cid, _generate, entry, kw) for cid, entry, kw in GENERATE] + [(cid, _score, entry, kw) for cid, entry, kw in SCORING] + \
        [(cid, _admit, entry, kw) for cid, entry, kw in ADMIT]


def _load():
    import __graft_entry__ as ge
    ge.build()
    from starvector_amd import _lib
    return _lib.load(), _lib


def _run(lib, L, case):
    _, call, entry, kw = case
    rc = call(lib, L, entry, **kw)
    return [rc, lib.sv_last_error().decode()]


@pytest.fixture(scope="module")
def lib():
    return _load()


def test_table_and_fixture_hold_the_same_cases():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    gold = json.load(open(FIXTURE))
    assert sorted(gold) == sorted(ids), (sorted(set(ids) - set(gold)), sorted(set(gold) - set(ids)))
    # nothing reaches an engine: every case is refused, the well-formed ones at the engine check
    assert all(rc == -22 for rc, _ in gold.values())
    assert all(gold[i][1] == "null engine" for i in ids if "/ok" in i or "is the engine's" in i or i.endswith("everything bad"))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_code_and_message_are_the_recorded_ones(lib, case):
    gold = json.load(open(FIXTURE))
    assert case[0] in gold, "not in the fixture: record it from the parent's build"
    assert _run(*lib, case) == gold[case[0]]


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python -m tests.test_abi_arg_errors_host --record")
    handle, L = _load()
    with open(FIXTURE, "w") as f:
        json.dump({c[0]: _run(handle, L, c) for c in CASES}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} cases -> {FIXTURE}")
