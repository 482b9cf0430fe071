"""CPU: prompt-lookup speculative decoding without a GPU -- the invariant of the Python restatement (starvector_amd/lookup.py: whatever
the drafts are, the emitted stream is the plain greedy stream), the argument checks sv_generate_lookup runs in front of the engine, and
HipCausalLM.generate's two HF keywords over a fake engine."""
import ctypes as C
import random
import types

import pytest
import torch

from starvector_amd import _lib
from starvector_amd import lookup as LK
from starvector_amd.model import HipCausalLM

V = 7


def _model(seed):
    """a deterministic toy model with a small vocabulary (so that n-grams repeat): the next id from the last three ids and the sequence"""
    def model(s, prefix, eos_barred):
        t = random.Random(hash((seed, s, tuple(prefix[-3:]), len(prefix) // 5))).randrange(V)
        return (t + 1) % V if eos_barred and t == 1 else t
    return model


@pytest.mark.parametrize("seed", range(200))
def test_any_draft_source_emits_the_plain_greedy_stream(seed):
    r = random.Random(seed)
    n_seq, K = r.choice([1, 1, 2, 3]), r.choice([1, 3, 7, 15])
    max_new = r.choice([1, 2, K + 1, K + 2, 20, 40])
    eos, stop, min_new = r.choice([-1, 1]), r.choice([(), (2,), (3, 4), (0, 0)]), r.choice([0, 0, 5])      # (0, 0): the stop completed by pads
    forced = [[r.randrange(V) for _ in range(max_new)] for _ in range(n_seq)] if r.random() < 0.5 else None
    model = _model(seed)
    plain = LK.plain_greedy(model, n_seq, max_new, eos, 0, stop, min_new)
    toks, st = LK.lookup_greedy(model, n_seq, K, max_new, eos, 0, stop, min_new, max_ngram=r.choice([1, 3, 8]), forced=forced)
    assert toks == plain, (n_seq, K, max_new, eos, stop, min_new, forced is not None)
    assert 0 <= st.accepted <= st.drafted and st.steps <= max(max_new - 1, 0)


def test_the_oracle_drafts_are_all_accepted_and_wrong_ones_cost_nothing_but_steps():
    model = _model(3)
    n = 41
    stream = LK.plain_greedy(model, 1, n)[0]
    for K in (1, 3, 7, 15):
        toks, st = LK.lookup_greedy(model, 1, K, n, forced=[stream])
        assert toks[0] == stream and st.steps == -(-(n - 1) // (K + 1)) and st.accepted == st.drafted == n - 1 - st.steps
        toks, st = LK.lookup_greedy(model, 1, K, n, forced=[[(t + 1) % V for t in stream]])
        assert toks[0] == stream and st.steps == n - 1 and st.accepted == 0


def test_draft_picks_the_latest_match_and_backs_off():
    assert LK.draft([1, 2, 3, 9, 1, 2, 3, 8, 1, 2, 3], 2) == [8, 1]                      # several matches: the latest wins
    assert LK.draft([1, 2, 3, 4, 1, 2, 3], 8) == [4, 1, 2, 3]                            # the continuation is cut at the end of the history
    assert LK.draft([1, 2, 3, 4, 5], 4) == []                                            # no match at all
    assert LK.draft([5, 6, 7, 9, 9, 7], 3, max_ngram=3) == [9, 9, 7]                     # back-off from 3 to 1
    assert LK.draft([4, 4], 3, max_ngram=3) == [4]                                       # L < n for n = 3 and 2; n = 1 matches position 0
    assert LK.draft([4], 3) == []
    assert LK.draft([1, 2, 1, 2, 1], 4, max_new=7) == [2]                                # the budget leaves room for one draft


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _sp(**kw):
    sp = _lib.SvSampling(0, 1.0, 1.0, 16, -1, 0, 0, None, 0, 0, 1.0, 1, 1.0, 0, 0, None, None, 0)
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def test_argument_checks_run_in_front_of_the_engine(lib):
    p, n = C.c_void_p(16), C.c_int32(0)                  # never dereferenced: the checks come first

    def call(sp, lk, embeds=p, B=1, lens=None, S0=4, out=p, ngen=None):
        rc = lib.sv_generate_lookup(None, embeds, B, lens, S0, C.byref(sp) if sp is not None else None, C.byref(lk) if lk is not None else None,
                                    out, C.byref(n) if ngen is None else ngen, None, None)
        return rc, lib.sv_last_error().decode()

    L = _lib.SvLookup
    assert call(_sp(), L(16, 0, 0)) == (-22, "sv_generate_lookup: num_draft_tokens 16 unsupported (0..15)")
    assert call(_sp(), L(-1, 0, 0)) == (-22, "sv_generate_lookup: num_draft_tokens -1 unsupported (0..15)")
    assert call(_sp(), L(3, 9, 0)) == (-22, "sv_generate_lookup: max_ngram 9 unsupported (1..8, 0 = 3)")
    assert call(_sp(), L(3, 2, 3)) == (-22, "sv_generate_lookup: min_ngram 3 must lie in 1..max_ngram 2 (0 = 1)")
    assert call(_sp(), L(3, 0, 4)) == (-22, "sv_generate_lookup: min_ngram 4 must lie in 1..max_ngram 3 (0 = 1)")
    assert call(_sp(), L(3, 0, 0), embeds=None) == (-22, "sv_generate_lookup: null argument")
    assert call(None, L(3, 0, 0)) == (-22, "sv_generate_lookup: null argument")
    assert call(_sp(), L(3, 0, 0), out=None) == (-22, "sv_generate_lookup: null argument")
    assert call(_sp(), L(3, 0, 0), B=0) == (-22, "sv_generate_lookup: bad B=0")
    assert call(_sp(), L(3, 0, 0), S0=0) == (-22, "sv_generate_lookup: bad S0=0")
    lens = (C.c_int32 * 2)(3, 0)
    assert call(_sp(), L(3, 0, 0), B=2, lens=lens) == (-22, "sv_generate_lookup: length 0 of sequence 1 (must be >= 1)")
    rc, msg = call(_sp(do_sample=1), L(3, 0, 0))
    assert rc == -95 and msg.startswith("sv_generate_lookup: do_sample is not built")
    rc, msg = call(_sp(num_beams=2), L(3, 0, 0))
    assert rc == -95 and msg.startswith("sv_generate_lookup: num_beams 2 is not built")
    rc, msg = call(_sp(repetition_penalty=1.5), L(3, 0, 0))
    assert rc == -95 and msg.startswith("sv_generate_lookup: repetition_penalty 1.5 is not built")
    cb = _lib.TOKEN_CALLBACK(lambda *a: None)
    rc, msg = call(_sp(on_tokens=C.cast(cb, C.c_void_p)), L(3, 0, 0), B=2)
    assert rc == -95 and msg.startswith("sv_generate_lookup: streaming (on_tokens) with B 2 > 1 is not built")
    # everything in order: the engine check is what is left; without lookup the call IS sv_generate / sv_generate_ragged
    assert call(_sp(), L(3, 0, 0)) == (-22, "null engine")
    assert call(_sp(), None) == (-22, "null engine") and call(_sp(), L(0, 0, 0)) == (-22, "null engine")
    assert call(_sp(), None, B=2, lens=lens) == (-22, "sv_generate_ragged: length 0 of sequence 1 (must be >= 1)")
    assert C.sizeof(_lib.SvLookup) == 12 and [f[0] for f in _lib.SvLookup._fields_] == ["num_draft_tokens", "max_ngram", "min_ngram"]


class _Eng:
    def __init__(self):
        self.cfg = types.SimpleNamespace(vocab=11, max_batch=32)
        self.calls = []

    def generate(self, inputs_embeds, max_length, **kw):
        self.calls.append(("generate", kw))
        return torch.zeros(inputs_embeds.shape[0], max_length - inputs_embeds.shape[1], dtype=torch.long)

    def generate_lookup(self, embeds, max_length, **kw):
        self.calls.append(("generate_lookup", dict(kw, max_length=max_length)))
        n = max_length - embeds.shape[1]
        if kw.get("on_tokens"):
            kw["on_tokens"](torch.ones(embeds.shape[0], n, dtype=torch.long), 0)
        return torch.ones(embeds.shape[0], n, dtype=torch.long)


def _lm():
    lm = HipCausalLM.__new__(HipCausalLM)
    torch.nn.Module.__init__(lm)
    object.__setattr__(lm, "_engine", _Eng())
    lm.eos_token_id, lm.pad_token_id, lm.seed = 0, 1, 0
    lm.batcher = None
    return lm


def test_the_hf_keywords_reach_generate_lookup():
    lm, emb = _lm(), torch.zeros(2, 3, 4)
    out = lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=5, max_matching_ngram_size=2, min_length=6, eos_token_id=4)
    name, kw = lm._engine.calls[-1]
    assert name == "generate_lookup" and out.shape == (2, 6) and bool((out == 1).all())
    assert kw["num_draft_tokens"] == 5 and kw["max_ngram"] == 2 and kw["max_length"] == 9 and kw["eos_token_id"] == 4 and kw["pad_token_id"] == 1
    assert kw["min_new_tokens"] == 3 and kw["stop_ids"] is None and kw["on_tokens"] is None
    res = lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=5, return_dict_in_generate=True)
    assert torch.equal(res.sequences, out)
    # default off: no existing call changes
    lm.generate(inputs_embeds=emb, max_length=9)
    lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=None, max_matching_ngram_size=3)
    lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=0)
    assert [c[0] for c in lm._engine.calls[-3:]] == ["generate"] * 3
    assert all("num_draft_tokens" not in c[1] and "prompt_lookup_num_tokens" not in c[1] for c in lm._engine.calls[-3:])

    class Streamer:
        def __init__(self):
            self.got, self.ended = [], False

        def put(self, t):
            self.got.append(t)

        def end(self):
            self.ended = True
    s = Streamer()
    lm.generate(inputs_embeds=emb[:1], max_length=9, prompt_lookup_num_tokens=2, streamer=s)
    assert s.ended and len(s.got) == 1 + 6 and s.got[0].shape == (1, 0)


@pytest.mark.parametrize("extra,name", [
    (dict(do_sample=True), "do_sample"), (dict(num_beams=2), "num_beams > 1"), (dict(repetition_penalty=1.3), "repetition_penalty"),
    (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(bad_words_ids=[[3]]), "bad_words_ids"),
    (dict(return_dict_in_generate=True, output_scores=True), "output_scores"), (dict(return_dict_in_generate=True, output_token_logprobs=True), "output_token_logprobs"),
    (dict(return_dict_in_generate=True, output_top_logprobs=4), "output_top_logprobs"), (dict(num_return_sequences=2), "num_return_sequences"),
    (dict(attention_mask=torch.tensor([[0, 1, 1], [1, 1, 1]])), "attention_mask"), (dict(streamer=object()), "streamer")])
def test_refused_combinations_raise_and_never_drop_the_argument(extra, name):
    lm, emb = _lm(), torch.zeros(2, 3, 4)
    with pytest.raises(NotImplementedError, match=name):
        lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=3, **extra)
    assert not lm._engine.calls
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=-2)


def test_generate_im2svg_kwargs_pass_through():
    from starvector_amd.model import StarVectorStarCoder
    base = types.SimpleNamespace(svg_transformer=types.SimpleNamespace(tokenizer=lambda text, add_special_tokens=False: {"input_ids": [5, 6]}))
    kw = StarVectorStarCoder._get_generation_kwargs(base, dict(inputs_embeds=1, attention_mask=2, prompt_lookup_num_tokens=7, max_matching_ngram_size=4))
    assert kw["prompt_lookup_num_tokens"] == 7 and kw["max_matching_ngram_size"] == 4
    kw = StarVectorStarCoder._get_generation_kwargs(base, dict(inputs_embeds=1, attention_mask=2))
    assert kw["prompt_lookup_num_tokens"] is None and kw["max_matching_ngram_size"] is None
