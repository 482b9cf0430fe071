"""CPU: prompt-lookup drafting in the continuous batch (sv_cb_set_lookup) without a GPU.
  * the exactness argument on the Python restatement (starvector_amd/lookup.py, CbLookupState): whatever the drafts are -- the natural
    lookup, forced right, every m-th wrong, all wrong -- every slot's emitted stream, finish column and live flag are those of the
    one-token-per-step batch, with budget, EOS, stop-sequence and stop_any finishes; the counters are the greedy restatement's for the stream;
  * the row layout and the capacity arithmetic;
  * the checks sv_cb_set_lookup and the other new entry points run in front of the engine."""
import ctypes as C
import random

import pytest

from starvector_amd import _lib
from starvector_amd import lookup as LK
from tests.test_gpu_lookup import _restated_counts

V = 7


def _chooser(seed):
    """A deterministic toy selection over a small vocabulary (so that n-grams repeat), keyed by (slot, column, the last ids of the prefix)."""
    def choose(s, col, prefix, hold):
        r = random.Random(hash((seed, s, col // 3, tuple(prefix[-2:]))))
        t = r.randrange(V)
        return (t + 1) % V if hold and t == 1 else t
    return choose


def _run(st, reqs, choose, max_steps=10_000):
    slots = [st.admit(q, choose) for q in reqs]
    steps = 0
    while st.n_live:
        st.step(choose)
        steps += 1
        assert steps < max_steps
    return slots


@pytest.mark.parametrize("K", [1, 3, 7, 15])
@pytest.mark.parametrize("seed", range(30))
def test_every_slot_emits_the_one_token_per_step_stream(seed, K):
    r = random.Random(1000 * seed + K)
    choose = _chooser(seed)
    n = r.randrange(1, 64 // (K + 1) + 1)
    reqs = [LK.CbRequest(budget=r.choice([1, 2, K + 1, K + 2, 20, 40]), eos=r.choice([-1, 1]), stop=r.choice([(), (2,), (3, 4), (0, 0)]),
                         stop_any=r.choice([(), (5,), (5, 6)]), min_new=r.choice([0, 0, 5]), base=r.randrange(1, 70)) for _ in range(n)]
    plain = [LK.cb_plain_stream(s, q, choose) for s, q in enumerate(reqs)]
    for kind in ("natural", "right", "random", "m2", "m3", "m5", "wrong"):
        forced = None
        if kind == "right":
            forced = [list(p[0]) + [0] * 64 for p in plain]
        elif kind == "random":
            forced = [[r.randrange(V) for _ in range(64)] for _ in plain]
        elif kind == "wrong":
            forced = [[(t + 1) % V for t in p[0]] + [0] * 64 for p in plain]
        elif kind[0] == "m":
            m = int(kind[1:])
            forced = [[(t + 1) % V if i % m == 0 else t for i, t in enumerate(p[0])] + [0] * 64 for p in plain]
        st = LK.CbLookupState(64, K, max_ngram=r.choice([1, 3, 8]), forced=forced)
        slots = _run(st, reqs, choose)
        assert slots == list(range(n))
        for s, q in zip(slots, reqs):
            ref, ref_live = plain[s]
            assert st.hist[s] == ref and st.live[s] == ref_live, (kind, seed, K, s, q)
            c = st.counts[s]
            assert 0 <= c[2] <= c[1] and c[0] + c[2] == len(ref) - 1, (kind, c)          # every step emits its accepted drafts and one token more
        assert st.totals == [sum(c[k] for c in st.counts[:n]) for k in range(3)]
        assert st.n_live == 0 and st.events == n


def _finishes(req, choose, K):
    """the finish column of a request under every kind of draft: the plain batch's"""
    ref, _ = LK.cb_plain_stream(0, req, choose)
    for forced in (None, [list(ref) + [0] * 40], [[(t + 1) % V for t in ref] + [0] * 40]):
        st = LK.CbLookupState(16, K, forced=forced)
        _run(st, [req], choose)
        assert st.hist[0] == ref and not st.live[0]
    return ref


@pytest.mark.parametrize("K", [1, 3, 7, 15])
def test_each_kind_of_finish_inside_an_accepted_run(K):
    stream = [3, 4, 3, 5, 6, 3, 4, 3, 5, 6, 2, 2, 3, 4, 1, 6, 6, 5, 0, 3] * 2
    choose = lambda s, col, prefix, hold: 6 if hold and stream[col] == 1 else stream[col]
    for budget in (1, 2, K + 1, K + 2):
        assert _finishes(LK.CbRequest(budget=budget), choose, K) == stream[:budget]
    assert _finishes(LK.CbRequest(budget=40, eos=1), choose, K) == stream[:15]                      # EOS at column 14
    assert _finishes(LK.CbRequest(budget=40, eos=1, min_new=16), choose, K)[14] == 6               # held: the stream goes on past it
    assert _finishes(LK.CbRequest(budget=40, stop=(5, 6)), choose, K) == stream[:5]                 # a 2-id stop completed at column 4
    assert _finishes(LK.CbRequest(budget=40, stop_any=(2, 0)), choose, K) == stream[:11]


@pytest.mark.parametrize("K", [1, 3, 7, 15])
def test_counters_are_the_greedy_restatements_for_the_same_stream(K):
    n = 45
    for seed in range(4):
        choose = _chooser(seed)
        stream, _ = LK.cb_plain_stream(0, LK.CbRequest(budget=n), choose)
        for forced in (None, stream, [(t + 1) % V if i % 3 == 0 else t for i, t in enumerate(stream)], [(t + 1) % V for t in stream]):
            st = LK.CbLookupState(16, K, forced=None if forced is None else [forced])
            _run(st, [LK.CbRequest(budget=n, base=9)], choose)
            assert st.hist[0] == stream
            if forced is not None:
                assert tuple(st.counts[0]) == _restated_counts(stream, K, forced), (seed, K)
            else:
                toks, ref = LK.lookup_greedy(lambda s, prefix, ban: stream[len(prefix)] if len(prefix) < n else 0, 1, K, n)
                assert toks[0] == stream and tuple(st.counts[0]) == (ref.steps, ref.drafted, ref.accepted)
        st = LK.CbLookupState(16, K, forced=[stream])
        _run(st, [LK.CbRequest(budget=n)], choose)
        assert st.counts[0][0] == -(-(n - 1) // (K + 1)) and st.counts[0][1] == st.counts[0][2] == n - 1 - st.counts[0][0]


def test_row_layout_and_release():
    K, stream = 3, [3, 4, 3, 5, 6, 3, 4, 3, 5, 6, 2, 2]
    choose = lambda s, col, prefix, hold: stream[col] + s
    st = LK.CbLookupState(16, K, forced=[stream, [t + 1 for t in stream]])
    a = st.admit(LK.CbRequest(budget=12, base=10), choose)
    b = st.admit(LK.CbRequest(budget=3, base=70), choose)
    assert (a, b) == (0, 1)
    # row 0 = the last emitted id at its position, rows 1 .. nd the drafts behind it, the rest exact copies of row 0
    assert st.rows_of(0) == [3, 4, 3, 5] and st.positions_of(0) == [10, 11, 12, 13] and st.n_draft[0] == 3
    assert st.rows_of(1) == [4, 5, 4, 4] and st.positions_of(1) == [70, 71, 70, 70] and st.n_draft[1] == 1          # min(K, budget - step - 1)
    assert st.cur_tok[8:] == [0] * 8 and st.counts[0] == [0, 0, 0]
    st.step(choose)
    assert st.hist[0] == stream[:5] and st.rows_of(0) == [6, 3, 4, 3] and st.positions_of(0) == [14, 15, 16, 17]
    assert st.hist[1] == [4, 5, 4] and not st.live[1] and st.rows_of(1) == [4] * 4 and st.positions_of(1) == [72] * 4
    assert st.counts == [[1, 3, 3], [1, 1, 1], [0, 0, 0], [0, 0, 0]] and st.totals == [2, 4, 4] and st.n_live == 1
    before = (list(st.hist[1]), st.rows_of(1))
    st.step(choose)                                      # a dead slot is left untouched
    assert (st.hist[1], st.rows_of(1)) == before and st.counts[1] == [1, 1, 1]
    st.release(1)
    assert st.rows_of(1) == [0] * 4 and st.positions_of(1) == [0] * 4 and st.req[1] is None
    c = st.admit(LK.CbRequest(budget=5, base=4), choose)          # the slot is reused: counters from zero, nothing of the predecessor's history
    assert c == 1 and st.counts[1] == [0, 0, 0] and st.hist[1] == [4]


def test_capacity_and_bucket_arithmetic():
    choose = lambda s, col, prefix, hold: 1
    for mb, K in ((64, 7), (64, 3), (32, 15), (16, 1), (16, 15), (48, 4)):
        st = LK.CbLookupState(mb, K)
        assert st.capacity == mb // (K + 1)
        slots = [st.admit(LK.CbRequest(budget=50), choose) for _ in range(st.capacity + 1)]
        assert slots == list(range(st.capacity)) + [-1] and st.n_live == st.capacity              # the last is SV_EBUSY: nothing is admitted
        assert st.bucket() == min(mb, max(8, 1 << (st.capacity * (K + 1) - 1).bit_length()))
        for s in range(1, st.capacity):
            st.release(s)
        assert st.bucket() == max(8, 1 << K.bit_length())                                          # rows: (highest used slot + 1) * K1, one slot left
    with pytest.raises(ValueError):
        LK.CbLookupState(8, 15)
    st = LK.CbLookupState(64, 7)
    st.admit(LK.CbRequest(budget=50), choose)
    assert st.bucket() == 8
    st.admit(LK.CbRequest(budget=50), choose)
    assert st.bucket() == 16
    for _ in range(3):
        st.admit(LK.CbRequest(budget=50), choose)
    assert st.bucket() == 64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_argument_checks_run_in_front_of_the_engine(lib):
    L = _lib.SvLookup
    who = "sv_cb_set_lookup"

    def call(lk, e=None):
        rc = lib.sv_cb_set_lookup(e, C.byref(lk) if lk is not None else None)
        return rc, lib.sv_last_error().decode()

    assert call(L(16, 0, 0)) == (-22, who + ": num_draft_tokens 16 unsupported (0..15)")
    assert call(L(-1, 0, 0)) == (-22, who + ": num_draft_tokens -1 unsupported (0..15)")
    assert call(L(3, 9, 0)) == (-22, who + ": max_ngram 9 unsupported (1..8, 0 = 3)")
    assert call(L(3, -1, 0)) == (-22, who + ": max_ngram -1 unsupported (1..8, 0 = 3)")
    assert call(L(3, 2, 3)) == (-22, who + ": min_ngram 3 must lie in 1..max_ngram 2 (0 = 1)")
    assert call(L(3, 0, 4)) == (-22, who + ": min_ngram 4 must lie in 1..max_ngram 3 (0 = 1)")
    assert call(L(3, 0, -1)) == (-22, who + ": min_ngram -1 must lie in 1..max_ngram 3 (0 = 1)")
    # in range (and off): the next thing looked at is the handle
    for lk in (L(3, 0, 0), L(15, 8, 8), L(0, 0, 0), None):
        assert call(lk) == (-22, "null engine")
    c3 = (C.c_int32 * 3)()
    assert lib.sv_cb_lookup_counts(None, -1, c3) == -22 and lib.sv_last_error().decode() == "sv_cb_lookup_counts: null argument"
    assert lib.sv_cb_lookup_counts(C.c_void_p(16), 0, None) == -22 and lib.sv_last_error().decode() == "sv_cb_lookup_counts: null argument"
    ids = (C.c_int32 * 4)(1, 2, 3, 4)
    assert lib.sv_debug_cb_set_lookup_drafts(None, ids, 1, 4) == -22 and lib.sv_last_error().decode() == "null engine"


def test_the_operator_checks_its_arguments_before_the_device(lib):
    who = "sv_op_cb_lookup_step"
    n, K = 1, 3
    req = (_lib.SvCbRequest * 1)()
    req[0].max_new_tokens, req[0].eos_token_id, req[0].temperature, req[0].top_p = 8, -1, 1.0, 1.0
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    good = dict(logits=C.c_void_p(16), n=n, K=K, V=100, ld=100, reqs=req, lps=None, base=i32(5), live=i32(1), hist=i32(*[0] * 8), ld_hist=8,
                hist_len=i32(1), rows=i32(0, 0, 0, 0), pos=i32(5, 5, 5, 5), nd=i32(0), mx=0, mn=0, forced=None, fn=0, fld=0, counts=i32(0, 0, 0),
                flags=i32(0, 0, 0), lp=None, rk=None)

    def call(**kw):
        a = {**good, **kw}
        rc = lib.sv_op_cb_lookup_step(a["logits"], a["n"], a["K"], a["V"], a["ld"], a["reqs"], a["lps"], a["base"], a["live"], a["hist"], a["ld_hist"],
                                      a["hist_len"], a["rows"], a["pos"], a["nd"], a["mx"], a["mn"], a["forced"], a["fn"], a["fld"], a["counts"],
                                      a["flags"], a["lp"], a["rk"], None)
        return rc, lib.sv_last_error().decode()

    for name in ("logits", "reqs", "base", "live", "hist", "hist_len", "rows", "pos", "nd", "counts", "flags"):
        assert call(**{name: None}) == (-22, who + ": null argument"), name
    assert call(ld=102) == (-22, who + ": bad argument") and call(n=0) == (-22, who + ": bad argument")
    assert call(K=16) == (-22, who + ": num_draft_tokens 16 unsupported (0..15)")
    assert call(K=0) == (-22, who + ": num_draft_tokens 0 (1..15)")
    assert call(mx=9) == (-22, who + ": max_ngram 9 unsupported (1..8, 0 = 3)")
    assert call(hist_len=i32(5)) == (-22, who + ": slot 0: history length 5 + 4 rows exceed ld_hist 8")
    assert call(nd=i32(4)) == (-22, who + ": slot 0: n_draft 4 outside 0..3")
    assert call(rows=i32(0, 100, 0, 0)) == (-22, who + ": slot 0: row id outside the vocabulary")
    assert call(forced=i32(1, 2), fn=1, fld=0)[1] == who + ": bad forced_n 1 / forced_ld 0"
    lps = (_lib.SvCbLogprobs * 1)()
    lps[0].enable = 1
    assert call(lps=lps) == (-22, who + ": lps without host_logprob / host_rank")


# ---- the Python layers over a scripted engine -----------------------------------------------------------------------------------------------
def test_the_batcher_sets_the_mode_first_and_queues_beyond_its_slots():
    import threading
    from starvector_amd.batching import ContinuousBatcher
    from tests.test_batching_host import _CbEngine, _emb

    class Eng(_CbEngine):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.calls = []

        def cb_set_lookup(self, K, max_ngram=0, min_ngram=0):
            assert not self.slots
            self.calls.append(("set", K, max_ngram, min_ngram))

        def cb_lookup_counts(self, slot=-1):
            return {"steps": 7, "drafted": 5, "accepted": 3}

        def cb_admit(self, emb, reqs):
            assert self.calls and len(self.slots) + len(reqs) <= self.cfg.max_batch // 4, "more requests than slots of 4 rows"
            self.calls.append(("admit", len(reqs)))
            return super().cb_admit(emb, reqs)

    eng = Eng(max_batch=8, delay=0.005)                  # K = 3: two slots of four rows
    b = ContinuousBatcher(eng, steps_per_poll=1, prompt_lookup_num_tokens=3, max_matching_ngram_size=2)
    assert b.slots == 2 and eng.calls == [("set", 3, 2, 0)]
    got = {}
    th = [threading.Thread(target=lambda i=i: got.__setitem__(i, b.generate(_emb(10 * i), dict(max_new_tokens=6)))) for i in range(5)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=30)
    assert all(got[i][0].tolist() == [10 * i + k for k in range(6)] for i in range(5)) and b.max_concurrent <= 2
    assert b.lookup_counts() == {"steps": 7, "drafted": 5, "accepted": 3}
    b.close()
    plain = ContinuousBatcher(_CbEngine(max_batch=8), steps_per_poll=1)       # off: the engine is never asked, every row is a slot
    assert plain.slots == 8 and plain.lookup_counts() == {"steps": 0, "drafted": 0, "accepted": 0}
    plain.close()
    with pytest.raises(NotImplementedError, match="exceed max_batch"):
        ContinuousBatcher(Eng(max_batch=8), prompt_lookup_num_tokens=15)
    with pytest.raises(ValueError):
        ContinuousBatcher(Eng(max_batch=8), prompt_lookup_num_tokens=-1)


def test_the_llm_takes_vllms_ngram_arguments_and_refuses_a_draft_model():
    from starvector_amd import vllm as VL
    with pytest.raises(NotImplementedError, match="draft model"):
        VL.LLM("no-such-dir", speculative_model="facebook/opt-125m", num_speculative_tokens=3)
    for n in (None, 0, 16):
        with pytest.raises(ValueError, match="num_speculative_tokens"):
            VL.LLM("no-such-dir", speculative_model="[ngram]", num_speculative_tokens=n)
    with pytest.raises(ValueError, match="need speculative_model"):
        VL.LLM("no-such-dir", num_speculative_tokens=3)
    assert "OUTPUT ids only" in VL.LLM.__doc__


def test_the_worker_passes_its_flags_to_the_batcher(monkeypatch):
    import types
    from starvector_amd import batching, serve
    seen = {}

    class B:
        def __init__(self, eng, **kw):
            seen.update(kw)
    monkeypatch.setattr(batching, "ContinuousBatcher", B)
    eng = types.SimpleNamespace(cb_admit=None)
    lm = types.SimpleNamespace(_engine=eng, batcher=None)
    model = types.SimpleNamespace(model=types.SimpleNamespace(svg_transformer=types.SimpleNamespace(transformer=lm)), config=None)
    serve.ModelWorker("c", "w", "id", True, "starvector-x", model=model, prompt_lookup_num_tokens=7, max_matching_ngram_size=4)
    assert seen == dict(prompt_lookup_num_tokens=7, max_matching_ngram_size=4)
    seen.clear()
    serve.ModelWorker("c", "w", "id", True, "starvector-x", model=model)
    assert seen == {}                                    # off: the batcher is built exactly as before
