"""CPU: prompt-lookup decoding with the call's own selection (sv_generate_lookup_sampled) without a GPU.
  * the two exactness arguments on the Python restatement (starvector_amd/lookup.py): for ANY deterministic chooser keyed by (sequence, column,
    prefix) -- the sampler with its seed fixed is one -- the lookup stream is the plain stream, with and without the seen-set model of the
    repetition penalty, and the step / drafted / accepted counts are the greedy restatement's for that stream;
  * the checks sv_generate_lookup_sampled runs in front of the engine;
  * the refusals of HipEngine.generate_lookup_sampled and of HipCausalLM.generate's opt-in keyword over a fake engine."""
import ctypes as C
import random
import types

import pytest
import torch

from starvector_amd import _lib
from starvector_amd import lookup as LK
from starvector_amd.engine import HipEngine
from starvector_amd.model import HipCausalLM

V = 7


def _chooser(seed, penalised):
    """A deterministic toy sampler over a small vocabulary (so that n-grams repeat): the id is a function of the sequence, the COLUMN (the
    sampler's step counter), the last ids of the prefix and -- under the penalty model -- the whole seen set, which it avoids when it can."""
    def choose(s, col, prefix, seen, eos_barred):
        assert (seen is not None) == penalised
        r = random.Random(hash((seed, s, col // 3, tuple(prefix[-2:]))))
        t = r.randrange(V)
        if seen is not None and t in seen and r.random() < 0.6:      # a penalised id loses to its neighbour more often than not
            t = (t + 1 + len(seen)) % V
        return (t + 1) % V if eos_barred and t == 1 else t
    return choose


@pytest.mark.parametrize("penalty", [False, True])
@pytest.mark.parametrize("K", [1, 3, 7, 15])
@pytest.mark.parametrize("seed", range(25))
def test_any_chooser_keyed_by_sequence_column_and_prefix_gives_the_plain_stream(seed, K, penalty):
    r = random.Random(1000 * seed + K)
    n_seq = r.choice([1, 1, 2, 3])
    max_new = r.choice([1, 2, K + 1, K + 2, 20, 40])
    eos, stop, min_new = r.choice([-1, 1]), r.choice([(), (2,), (3, 4), (0, 0)]), r.choice([0, 0, 5])
    forced = [[r.randrange(V) for _ in range(max_new)] for _ in range(n_seq)] if r.random() < 0.5 else None
    choose = _chooser(seed, penalty)
    plain = LK.plain_chosen(choose, n_seq, max_new, eos, 0, stop, min_new, penalty=penalty)
    toks, st = LK.lookup_chosen(choose, n_seq, K, max_new, eos, 0, stop, min_new, max_ngram=r.choice([1, 3, 8]), forced=forced, penalty=penalty)
    assert toks == plain, (n_seq, K, max_new, eos, stop, min_new, forced is not None, penalty)
    assert 0 <= st.accepted <= st.drafted and st.steps <= max(max_new - 1, 0)


@pytest.mark.parametrize("penalty", [False, True])
def test_counts_are_the_greedy_restatements_for_the_same_stream(penalty):
    """The drafts (natural or forced) and the accept rule see only the stream: a greedy model that replays the chooser's stream takes the same
    steps, drafts and accepted drafts."""
    n = 41
    for seed in range(6):
        choose = _chooser(seed, penalty)
        stream = LK.plain_chosen(choose, 1, n, penalty=penalty)[0]
        replay = lambda s, prefix, barred: stream[len(prefix)] if len(prefix) < n else 0
        for K in (1, 3, 7, 15):
            for forced in (None, [stream], [[(t + 1) % V if i % 3 == 0 else t for i, t in enumerate(stream)]], [[(t + 1) % V for t in stream]]):
                toks, st = LK.lookup_chosen(choose, 1, K, n, forced=forced, penalty=penalty)
                ref_toks, ref = LK.lookup_greedy(replay, 1, K, n, forced=forced)
                assert toks[0] == stream == ref_toks[0]
                assert (st.steps, st.drafted, st.accepted) == (ref.steps, ref.drafted, ref.accepted), (seed, K)
            toks, st = LK.lookup_chosen(choose, 1, K, n, forced=[stream], penalty=penalty)
            assert st.steps == -(-(n - 1) // (K + 1)) and st.accepted == st.drafted == n - 1 - st.steps
            toks, st = LK.lookup_chosen(choose, 1, K, n, forced=[[(t + 1) % V for t in stream]], penalty=penalty)
            assert st.steps == n - 1 and st.accepted == 0


def test_a_rows_seen_set_is_the_plain_calls_set_at_its_column():
    """SeenSets against the definition: row j of a sequence holds the ids of the sequence plus its first j drafts -- with every draft in
    front of the row accepted that is set(stream[:column]); a dead row holds row 0's set."""
    stream = [3, 4, 3, 5, 6, 3, 4, 3, 5, 6, 2, 2, 3, 4]
    st = LK.LookupState(n_seq=1, K=3, max_new=len(stream), forced=[stream])
    st.begin(stream[:1], [0])
    sets = LK.SeenSets(1, 3)
    sets.begin([stream[:1]], st)
    while not st.done:
        L, nd = st.n_emit[0], st.n_draft[0]
        for j in range(4):
            assert sets.rows[0][j] == set(stream[:L + (j if j <= nd else 0)]), (L, j)
        st.step([[stream[L + j] if L + j < len(stream) else 0 for j in range(4)]])
        sets.step(st)
        assert sets.seq[0] == set(stream[:st.n_emit[0]]) and sets.cols[0] == st.n_emit[0]


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
    who = "sv_generate_lookup_sampled"

    def call(sp, lk, embeds=p, B=1, lens=None, S0=4, out=p, entry=who):
        rc = getattr(lib, entry)(None, embeds, B, lens, S0, C.byref(sp) if sp is not None else None, C.byref(lk) if lk is not None else None,
                                 out, C.byref(n), None, None)
        return rc, lib.sv_last_error().decode()

    L = _lib.SvLookup
    assert call(_sp(), L(16, 0, 0)) == (-22, who + ": num_draft_tokens 16 unsupported (0..15)")
    assert call(_sp(), L(3, 9, 0)) == (-22, who + ": max_ngram 9 unsupported (1..8, 0 = 3)")
    assert call(_sp(), L(3, 2, 3)) == (-22, who + ": min_ngram 3 must lie in 1..max_ngram 2 (0 = 1)")
    assert call(_sp(), L(3, 0, 0), embeds=None) == (-22, who + ": null argument")
    assert call(None, L(3, 0, 0)) == (-22, who + ": null argument")
    assert call(_sp(), L(3, 0, 0), B=0) == (-22, who + ": bad B=0")
    lens = (C.c_int32 * 2)(3, 0)
    assert call(_sp(), L(3, 0, 0), B=2, lens=lens) == (-22, who + ": length 0 of sequence 1 (must be >= 1)")
    # still refused, by name
    rc, msg = call(_sp(num_beams=2), L(3, 0, 0))
    assert rc == -95 and msg.startswith(who + ": num_beams 2 is not built")
    cb = _lib.TOKEN_CALLBACK(lambda *a: None)
    rc, msg = call(_sp(on_tokens=C.cast(cb, C.c_void_p)), L(3, 0, 0), B=2)
    assert rc == -95 and msg.startswith(who + ": streaming (on_tokens) with B 2 > 1 is not built")
    # taken: sampling and the penalty pass every check that needs no engine
    for sp in (_sp(do_sample=1, top_k=50, top_p=0.9, seed=7), _sp(repetition_penalty=1.3), _sp(do_sample=1, repetition_penalty=1.3)):
        assert call(sp, L(3, 0, 0)) == (-22, "null engine")
    assert call(_sp(do_sample=1), None) == (-22, "null engine") and call(_sp(do_sample=1), L(0, 0, 0)) == (-22, "null engine")
    assert call(_sp(), None, B=2, lens=lens) == (-22, "sv_generate_ragged: length 0 of sequence 1 (must be >= 1)")
    # the greedy entry point refuses both as before, in its own words
    rc, msg = call(_sp(do_sample=1), L(3, 0, 0), entry="sv_generate_lookup")
    assert rc == -95 and msg.startswith("sv_generate_lookup: do_sample is not built (verification is greedy")
    rc, msg = call(_sp(repetition_penalty=1.5), L(3, 0, 0), entry="sv_generate_lookup")
    assert rc == -95 and msg.startswith("sv_generate_lookup: repetition_penalty 1.5 is not built")
    assert _lib.PRODUCT_PROTOTYPES[who] == _lib.PRODUCT_PROTOTYPES["sv_generate_lookup"]


@pytest.mark.parametrize("extra,name", [
    (dict(num_beams=2), "num_beams"), (dict(n_samples=2), "n_samples"), (dict(token_stats=True), "token_stats"), (dict(token_topk=4), "token_topk"),
    (dict(return_outputs=True), "return_outputs"), (dict(logits_processors=object()), "logits_processors"), (dict(scores_out=object()), "scores_out"),
    (dict(logits_out=object()), "logits_out")])
def test_the_engine_method_names_what_it_refuses_before_it_touches_the_engine(extra, name):
    fake = types.SimpleNamespace()                       # no library, no handle: any engine call would raise AttributeError
    with pytest.raises(NotImplementedError, match=name):
        HipEngine.generate_lookup_sampled(fake, torch.zeros(1, 3, 4), 9, 3, do_sample=True, **extra)
    with pytest.raises(TypeError, match="no_such_argument"):
        HipEngine.generate_lookup_sampled(fake, torch.zeros(1, 3, 4), 9, 3, no_such_argument=1)
    with pytest.raises(ValueError, match="temperature"):
        HipEngine.generate_lookup_sampled(fake, torch.zeros(1, 3, 4), 9, 3, do_sample=True, temperature=0.0)
    with pytest.raises(ValueError, match="repetition_penalty"):
        HipEngine.generate_lookup_sampled(fake, torch.zeros(1, 3, 4), 9, 3, repetition_penalty=0.0)


class _Eng:
    def __init__(self):
        self.cfg = types.SimpleNamespace(vocab=11, max_batch=32)
        self.calls = []

    def generate(self, inputs_embeds, max_length, **kw):
        self.calls.append(("generate", kw))
        return torch.zeros(inputs_embeds.shape[0], max_length - inputs_embeds.shape[1], dtype=torch.long)

    def generate_lookup(self, embeds, max_length, **kw):
        self.calls.append(("generate_lookup", dict(kw, max_length=max_length)))
        return torch.ones(embeds.shape[0], max_length - embeds.shape[1], dtype=torch.long)

    def generate_lookup_sampled(self, embeds, max_length, **kw):
        self.calls.append(("generate_lookup_sampled", dict(kw, max_length=max_length)))
        n = max_length - embeds.shape[1]
        if kw.get("on_tokens"):
            kw["on_tokens"](torch.full((embeds.shape[0], n), 2, dtype=torch.long), 0)
        return torch.full((embeds.shape[0], n), 2, dtype=torch.long)


def _lm():
    lm = HipCausalLM.__new__(HipCausalLM)
    torch.nn.Module.__init__(lm)
    object.__setattr__(lm, "_engine", _Eng())
    lm.eos_token_id, lm.pad_token_id, lm.seed = 0, 1, 0
    lm.batcher = None
    return lm


def test_the_keyword_routes_sampled_and_penalised_calls_to_the_new_method():
    lm, emb = _lm(), torch.zeros(2, 3, 4)
    out = lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=5, max_matching_ngram_size=2, prompt_lookup_sampling=True,
                      do_sample=True, top_p=0.9, temperature=0.7, seed=11, repetition_penalty=1.2, min_length=6, eos_token_id=4)
    name, kw = lm._engine.calls[-1]
    assert name == "generate_lookup_sampled" and out.shape == (2, 6) and bool((out == 2).all())
    assert kw["num_draft_tokens"] == 5 and kw["max_ngram"] == 2 and kw["max_length"] == 9 and kw["eos_token_id"] == 4 and kw["pad_token_id"] == 1
    assert kw["do_sample"] is True and kw["top_k"] == 50 and kw["top_p"] == 0.9 and kw["temperature"] == 0.7 and kw["seed"] == 11
    assert kw["repetition_penalty"] == 1.2 and kw["min_new_tokens"] == 3
    # greedy with a penalty, and plain greedy, through the same opt-in route
    lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, repetition_penalty=1.3)
    name, kw = lm._engine.calls[-1]
    assert name == "generate_lookup_sampled" and kw["do_sample"] is False and kw["repetition_penalty"] == 1.3
    res = lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, do_sample=True, seed=1,
                      return_dict_in_generate=True)
    assert torch.equal(res.sequences, out)

    class Streamer:
        def __init__(self):
            self.got, self.ended = [], False

        def put(self, t):
            self.got.append(t)

        def end(self):
            self.ended = True
    s = Streamer()
    lm.generate(inputs_embeds=emb[:1], max_length=9, prompt_lookup_num_tokens=2, prompt_lookup_sampling=True, do_sample=True, seed=1, streamer=s)
    assert s.ended and len(s.got) == 1 + 6 and s.got[0].shape == (1, 0)


def test_without_the_keyword_every_call_and_refusal_is_what_it_was():
    lm, emb = _lm(), torch.zeros(2, 3, 4)
    for extra, name in ((dict(do_sample=True), "do_sample"), (dict(repetition_penalty=1.3), "repetition_penalty")):
        with pytest.raises(NotImplementedError, match=name + ".*greedy verification"):
            lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=3, **extra)
        with pytest.raises(NotImplementedError, match=name):
            lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=3, prompt_lookup_sampling=False, **extra)
    assert not lm._engine.calls
    lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=3)
    assert lm._engine.calls[-1][0] == "generate_lookup" and "do_sample" not in lm._engine.calls[-1][1]
    lm.generate(inputs_embeds=emb, max_length=9, do_sample=True, seed=3)
    assert lm._engine.calls[-1][0] == "generate" and "prompt_lookup_sampling" not in lm._engine.calls[-1][1]


def test_the_keyword_alone_is_a_value_error():
    lm, emb = _lm(), torch.zeros(2, 3, 4)
    for kw in (dict(), dict(prompt_lookup_num_tokens=None), dict(prompt_lookup_num_tokens=0), dict(do_sample=True)):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_sampling=True, **kw)
    assert not lm._engine.calls


@pytest.mark.parametrize("extra,name", [
    (dict(num_beams=2), "num_beams > 1"), (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(bad_words_ids=[[3]]), "bad_words_ids"),
    (dict(do_sample=True, min_p=0.1), "min_p"), (dict(return_dict_in_generate=True, output_scores=True), "output_scores"),
    (dict(return_dict_in_generate=True, output_token_logprobs=True), "output_token_logprobs"),
    (dict(return_dict_in_generate=True, output_top_logprobs=4), "output_top_logprobs"), (dict(num_return_sequences=2), "num_return_sequences"),
    (dict(attention_mask=torch.tensor([[0, 1, 1], [1, 1, 1]])), "attention_mask"), (dict(streamer=object()), "streamer")])
def test_with_the_keyword_the_rest_is_still_refused_by_name(extra, name):
    lm, emb = _lm(), torch.zeros(2, 3, 4)
    with pytest.raises(NotImplementedError, match=name):
        lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, **{"do_sample": True, "seed": 1, **extra})
    assert not lm._engine.calls


def test_an_engine_without_the_method_is_named():
    lm, emb = _lm(), torch.zeros(1, 3, 4)
    object.__setattr__(lm, "_engine", types.SimpleNamespace(cfg=types.SimpleNamespace(vocab=11, max_batch=32)))
    with pytest.raises(NotImplementedError, match="generate_lookup_sampled"):
        lm.generate(inputs_embeds=emb, max_length=9, prompt_lookup_num_tokens=3, prompt_lookup_sampling=True, do_sample=True, seed=1)


def test_generate_im2svg_kwargs_pass_through():
    from starvector_amd.model import StarVectorStarCoder
    base = types.SimpleNamespace(svg_transformer=types.SimpleNamespace(tokenizer=lambda text, add_special_tokens=False: {"input_ids": [5, 6]}))
    kw = StarVectorStarCoder._get_generation_kwargs(base, dict(inputs_embeds=1, attention_mask=2, prompt_lookup_num_tokens=7, prompt_lookup_sampling=True))
    assert kw["prompt_lookup_num_tokens"] == 7 and kw["prompt_lookup_sampling"] is True
    kw = StarVectorStarCoder._get_generation_kwargs(base, dict(inputs_embeds=1, attention_mask=2, prompt_lookup_num_tokens=7))
    assert "prompt_lookup_sampling" not in kw          # off: the keywords of every existing call are what they were
