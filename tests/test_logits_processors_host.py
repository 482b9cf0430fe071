"""CPU: HF's no_repeat_ngram_size / bad_words_ids / min_p on the host side -- the torch restatement of the two ban processors against
transformers' own classes, the new C ABI (sv_logits_processors, sv_generate_processed, sv_op_ban_tokens) and its argument checks, and
HipCausalLM.generate's routing over a stand-in engine.

The restatement follows transformers (the reference's pin is 4.49; the classes have not changed since): NoBadWords skips a sequence that
is "longer than the context" (`len(sequence_ids) > input_ids.shape[1]`), so a sequence of L > 1 ids bans its last id from t >= L on --
with exactly L - 1 ids generated nothing is banned yet, even when they are the sequence's prefix."""
import ctypes as C
import os
import re

import pytest
import torch

from starvector_amd import _lib, engine as E
from tests.test_host_logic import _fake_lm
from tests.test_shared_prompt_host import _FakeSharedEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -float("inf")


# ---- the restatement (also carried by tests/test_gpu_logits_processors.py) ------------------------------------------------------------
def ngram_bans(g, n):
    """NoRepeatNGram(n) after the ids g[0 .. t-1]: { g[j+n-1] : 0 <= j <= t-n, g[j .. j+n-2] == g[t-n+1 .. t-1] }."""
    t = len(g)
    if n < 1 or t < n - 1:
        return set()
    suffix = g[t - n + 1:]                     # n - 1 ids (none for n = 1)
    return {g[j + n - 1] for j in range(0, t - n + 1) if g[j:j + n - 1] == suffix}


def bad_word_bans(g, words):
    """NoBadWords after g: a single id always; the last id of a longer sequence when t >= L and the last L - 1 ids are its prefix."""
    t, out = len(g), set()
    for w in words:
        L = len(w)
        if L == 1 or (t >= L and g[t - L + 1:] == list(w[:-1])):
            out.add(w[-1])
    return out


def restate(scores, hists, n=0, words=()):
    """scores [B, V] fp32, hists: one id list per row -> the processed rows (banned ids at -inf, everything else untouched)."""
    out = scores.clone()
    for b, g in enumerate(hists):
        ids = sorted(ngram_bans(list(g), n) | bad_word_bans(list(g), [list(w) for w in words]))
        if ids:
            out[b, torch.tensor(ids, dtype=torch.long)] = NEG
    return out


# ---- against transformers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_ngram_restatement_is_transformers(n):
    lp = pytest.importorskip("transformers").generation.logits_process
    gen = torch.Generator().manual_seed(100 + n)
    V, B, banned = 23, 6, 0
    for t in (0, max(n - 2, 0), n - 1, n, n + 1, 17, 130):
        ids = torch.randint(0, 5, (B, t), generator=gen)           # a 5-id alphabet: suffixes recur
        for b in range(B // 2):                                    # and periodic rows (periods 3, 4, 5): long n-grams recur too, from j = 0 on
            ids[b] = torch.randint(0, 5, (3 + b,), generator=gen).repeat(t // (3 + b) + 1)[:t]
        sc = torch.randn(B, V, generator=gen)
        want = lp.NoRepeatNGramLogitsProcessor(n)(ids, sc.clone())
        got = restate(sc, ids.tolist(), n=n)
        assert torch.equal(got, want), (n, t)
        banned += int(torch.isinf(got).sum())
    assert banned > 0                                              # the alphabet is small enough for the ban to bite


def test_bad_words_restatement_is_transformers():
    lp = pytest.importorskip("transformers").generation.logits_process
    gen = torch.Generator().manual_seed(7)
    V, B = 23, 8
    words = [[9], [1, 2], [3, 3, 4], [0, 1, 2, 3, 4, 0, 1, 22], [2, 2], [4, 0, 11]]
    hit = 0
    for t in (0, 1, 2, 3, 7, 8, 40):
        for _ in range(6):
            ids = torch.randint(0, 5, (B, t), generator=gen)
            if t >= 7:
                ids[0, -7:] = torch.tensor(words[3][:-1])            # the 8-id sequence's prefix, at t = 7 (not yet) and beyond (banned)
            sc = torch.randn(B, V, generator=gen)
            want = lp.NoBadWordsLogitsProcessor(words, eos_token_id=None)(ids, sc.clone())
            got = restate(sc, ids.tolist(), words=words)
            assert torch.equal(got, want), t
            hit += int(torch.isinf(got[:, [2, 4, 11, 22]]).sum())
            assert bool(torch.isinf(got[:, 9]).all())
    assert hit > 20
    # t = L - 1 with the whole history equal to the prefix: transformers does not ban yet (sequence longer than the context)
    sc = torch.zeros(1, V)
    assert not torch.isinf(lp.NoBadWordsLogitsProcessor([[1, 2]], eos_token_id=None)(torch.tensor([[1]]), sc.clone())).any()
    assert not torch.isinf(restate(sc, [[1]], words=[[1, 2]])).any()
    assert torch.isinf(restate(sc, [[0, 1]], words=[[1, 2]]))[0, 2]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_struct_symbols_and_abi_version(lib):
    prod, dbg = _header("starvector_hip.h"), _header("starvector_hip_debug.h")
    body = re.search(r"typedef struct sv_logits_processors \{(.*?)\} sv_logits_processors;", prod, flags=re.S).group(1)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", d)[-1] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.SvLogitsProcessors._fields_]
    assert fields == ["no_repeat_ngram_size", "n_bad_words", "bad_word_lens", "bad_word_ids", "min_p"]
    assert _lib.SvLogitsProcessors.bad_word_lens.offset == 8 and _lib.SvLogitsProcessors.min_p.offset == 24
    assert re.search(r"\bsv_generate_processed\s*\(", prod) and not re.search(r"\bsv_op_ban_tokens\s*\(", prod)
    assert re.search(r"\bsv_op_ban_tokens\s*\(", dbg)
    assert len(_lib.PRODUCT_PROTOTYPES["sv_generate_processed"][1]) == len(_lib.PRODUCT_PROTOTYPES["sv_generate_shared"][1]) + 1
    assert len(_lib.DEBUG_PROTOTYPES["sv_op_ban_tokens"][1]) == 9
    assert hasattr(lib, "sv_generate_processed") and hasattr(lib, "sv_op_ban_tokens")
    assert lib.sv_abi_version() == 9 and _lib.ABI_VERSION == 9 and "#define SV_ABI_VERSION 9" in prod
    # sv_sampling and sv_cb_request are what they were
    assert [f[0] for f in _lib.SvSampling._fields_][-1] == "min_new_tokens" and [f[0] for f in _lib.SvCbRequest._fields_][-1] == "stop_any_ids"


def _lp(n=0, words=(), min_p=0.0):
    lens = (C.c_int32 * max(len(words), 1))(*[len(w) for w in words])
    flat = [t for w in words for t in w]
    ids = (C.c_int32 * max(len(flat), 1))(*flat)
    s = _lib.SvLogitsProcessors(n, len(words), C.cast(lens, C.POINTER(C.c_int32)), C.cast(ids, C.POINTER(C.c_int32)), min_p)
    s._keep = (lens, ids)
    return s


def test_c_argument_checks_need_no_device(lib):
    def err():
        return lib.sv_last_error().decode()
    p, n = C.c_void_p(16), C.c_int32(0)                            # never dereferenced: the checks come first
    sp = _lib.SvSampling(max_length=32)
    gp = lib.sv_generate_processed

    def call(lp, sampling=sp, eng=None):
        return gp(eng, p, 2, None, 4, 1, C.byref(sampling), C.byref(lp) if lp is not None else None, None, p, C.byref(n), None)
    assert call(_lp(n=9)) == -22 and "no_repeat_ngram_size 9" in err()
    assert call(_lp(n=-1)) == -22
    assert call(_lp(words=[[1]] * 65)) == -22 and "65 bad-word sequences" in err()
    assert call(_lp(words=[[1], list(range(9))])) == -22 and "sequence 1 has 9 ids" in err()
    assert call(_lp(words=[[1], []])) == -22 and "sequence 1 has 0 ids" in err()
    assert call(_lp(words=[[1, -3]])) == -22 and "outside the vocabulary" in err()
    assert call(_lp(min_p=1.5)) == -22 and "min_p" in err()
    bad = _lib.SvLogitsProcessors(0, 2, None, None, 0.0)
    assert call(bad) == -22 and "null" in err()
    beams = _lib.SvSampling(max_length=32, num_beams=2)
    assert call(_lp(n=2), beams) == -22 and "num_beams 2" in err()
    assert call(_lp(words=[[5]]), beams) == -22 and "num_beams 2" in err()
    # the limits themselves pass and reach the engine check; NULL and all-zero are sv_generate_shared
    assert call(_lp(n=8, words=[[1] * 8] * 64, min_p=1.0)) == -22 and "null engine" in err()
    assert call(None) == -22 and "null engine" in err()
    assert call(_lp()) == -22 and "null engine" in err()
    assert gp(None, p, 2, None, 4, 0, C.byref(sp), C.byref(_lp()), None, p, C.byref(n), None) == -22 and "sv_generate_shared: bad n_samples=0" in err()
    # the operator checks the ids against ITS vocabulary before any device work
    op = lib.sv_op_ban_tokens
    hist, lens = (C.c_int32 * 4)(1, 2, 3, 4), (C.c_int32 * 2)(2, 1)
    assert op(p, 2, 100, 100, hist, 2, lens, C.byref(_lp(words=[[5, 100]])), None) == -22 and "id 100 outside the vocabulary" in err()
    assert op(p, 2, 100, 100, hist, 2, lens, C.byref(_lp(n=9)), None) == -22
    assert op(p, 2, 100, 100, hist, 2, (C.c_int32 * 2)(3, 1), C.byref(_lp(n=2)), None) == -22 and "history length 3" in err()
    assert op(p, 2, 3, 4, hist, 2, lens, C.byref(_lp(n=2)), None) == -22 and "history id outside" in err()
    assert op(None, 2, 100, 100, hist, 2, lens, C.byref(_lp(n=2)), None) == -22 and op(p, 2, 100, 99, hist, 2, lens, C.byref(_lp(n=2)), None) == -22


def test_python_argument_checks():
    for kw, msg in ((dict(no_repeat_ngram_size=9), "no_repeat_ngram_size 9"), (dict(bad_words_ids=[[1]] * 65), "65 bad-word"),
                    (dict(bad_words_ids=[list(range(9))]), "has 9 ids"), (dict(bad_words_ids=[[3, 516]], vocab=516), "id 516 outside"),
                    (dict(min_p=1.2), "min_p")):
        with pytest.raises(ValueError, match=msg):
            E.logits_processors(**kw)
    lp, keep = E.logits_processors(3, [[7], [1, 2, 3]], 0.25, vocab=516)
    assert (lp.no_repeat_ngram_size, lp.n_bad_words, lp.min_p) == (3, 2, 0.25)
    assert list(lp.bad_word_lens[:2]) == [1, 3] and list(lp.bad_word_ids[:4]) == [7, 1, 2, 3]
    lp, keep = E.logits_processors()
    assert (lp.no_repeat_ngram_size, lp.n_bad_words, lp.min_p) == (0, 0, 0.0) and not lp.bad_word_lens


# ---- HipCausalLM.generate over a stand-in engine ---------------------------------------------------------------------------------------
class _FakeProcessedEngine(_FakeSharedEngine):
    """The stand-in engine with the shared call, which also offers the processed call: records what it was asked and answers with
    `generate`'s tokens for the prompts repeated."""

    def __init__(self, vocab=None):
        super().__init__()
        self.processed = []
        if vocab is not None:
            self.cfg = type("Cfg", (), {"vocab": vocab, "max_batch": 8})()

    def generate_processed(self, embeds, max_length, no_repeat_ngram_size=0, bad_words_ids=None, min_p=0.0, n_samples=1, **kw):
        self.processed.append(dict(rows=int(embeds.shape[0]), no_repeat_ngram_size=no_repeat_ngram_size, bad_words_ids=bad_words_ids,
                                   min_p=min_p, n_samples=n_samples))
        out = self.generate(embeds.repeat_interleave(n_samples, dim=0), max_length, **kw)
        self.calls.pop()
        return out


def _lm(vocab=None):
    lm = _fake_lm()
    object.__setattr__(lm, "_engine", _FakeProcessedEngine(vocab))
    return lm


PARENT_KW = {"do_sample", "temperature", "top_p", "seed", "repetition_penalty", "num_beams", "length_penalty", "early_stopping", "top_k",
             "sync_every"}


def test_generate_routes_the_three_arguments_to_the_processed_call():
    torch.manual_seed(0)
    emb = torch.randint(0, 5, (2, 6, 3)).float()
    lm = _lm()
    out = lm.generate(inputs_embeds=emb, max_length=6 + 5, no_repeat_ngram_size=2)        # (dropped silently before this feature)
    assert lm._engine.processed == [dict(rows=2, no_repeat_ngram_size=2, bad_words_ids=None, min_p=0.0, n_samples=1)]
    assert lm._engine.calls == [] and out.shape == (2, 5)
    lm = _lm()
    lm.generate(inputs_embeds=emb, max_length=6 + 5, bad_words_ids=[[3, 4], (7,), [0]], eos_token_id=0)
    assert lm._engine.processed[0]["bad_words_ids"] == [[3, 4], [7]]                     # HF drops a bad word that is exactly [eos]
    lm = _lm()
    lm.generate(inputs_embeds=emb, max_length=6 + 5, min_p=0.1, do_sample=True, seed=3, num_return_sequences=2)
    assert lm._engine.processed == [dict(rows=2, no_repeat_ngram_size=0, bad_words_ids=None, min_p=0.1, n_samples=2)]
    lm = _lm()
    lm.generate(inputs_embeds=emb, max_length=6 + 5, min_p=0.1)                          # greedy: HF builds no warper
    assert lm._engine.processed == [] and len(lm._engine.calls) == 1
    # without the three arguments: the engine calls of the code before the feature
    lm, old = _lm(), _fake_lm()
    a = lm.generate(inputs_embeds=emb, max_length=6 + 5, do_sample=True, seed=11, repetition_penalty=1.2)
    b = old.generate(inputs_embeds=emb, max_length=6 + 5, do_sample=True, seed=11, repetition_penalty=1.2)
    assert lm._engine.processed == [] and lm._engine.calls == old._engine.calls == [(2, 6, 5, None)]
    assert lm._engine.last_kw == old._engine.last_kw and set(lm._engine.last_kw) == PARENT_KW and torch.equal(a, b)


def test_generate_raises_where_the_processed_route_is_not_built():
    emb = torch.ones(2, 6, 3)
    mask = torch.tensor([[0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
    for kw in (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[1, 2]]), dict(min_p=0.2, do_sample=True)):
        lm = _lm()
        with pytest.raises(NotImplementedError, match="num_beams"):
            lm.generate(inputs_embeds=emb, max_length=6 + 5, num_beams=2, **kw)
        with pytest.raises(NotImplementedError, match="padded"):
            lm.generate(inputs_embeds=emb, max_length=6 + 5, attention_mask=mask, **kw)
        assert lm._engine.processed == [] and lm._engine.calls == []
        lm.generate(inputs_embeds=emb, max_length=6 + 5, attention_mask=torch.ones(2, 6, dtype=torch.long), **kw)      # an all-ones mask is no padding
        assert len(lm._engine.processed) == 1


def test_generate_applies_hf_range_checks_and_the_limits():
    emb = torch.ones(1, 6, 3)
    lm = _lm(vocab=516)
    for kw in (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(bad_words_ids=[]), dict(bad_words_ids=[[]]),
               dict(bad_words_ids=[[1, -2]]), dict(bad_words_ids=[3]), dict(min_p=-0.1), dict(min_p=1.01, do_sample=True),
               dict(no_repeat_ngram_size=9), dict(bad_words_ids=[[1]] * 65), dict(bad_words_ids=[list(range(9))]),
               dict(bad_words_ids=[[1, 516]])):
        with pytest.raises(ValueError):
            lm.generate(inputs_embeds=emb, max_length=6 + 5, **kw)
    assert lm._engine.processed == [] and lm._engine.calls == []
    lm.generate(inputs_embeds=emb, max_length=6 + 5, bad_words_ids=[[1, 515]], no_repeat_ngram_size=8)
    assert len(lm._engine.processed) == 1


def test_under_a_batcher_the_processed_call_takes_the_exclusive_route():
    class _Batcher:
        jobs = 0

        def run_exclusive(self, call):
            self.jobs += 1
            return call()

        def generate(self, *a, **k):
            raise AssertionError("a call with processors must not join the shared decode loop: its request struct carries none")
    emb = torch.ones(1, 6, 3)
    lm = _lm()
    lm.batcher = _Batcher()
    out = lm.generate(inputs_embeds=emb, max_length=6 + 5, no_repeat_ngram_size=3, bad_words_ids=[[4, 5]])
    assert lm.batcher.jobs == 1 and out.shape == (1, 5)
    assert lm._engine.processed == [dict(rows=1, no_repeat_ngram_size=3, bad_words_ids=[[4, 5]], min_p=0.0, n_samples=1)]
