"""GPU: the prefix cache of the continuous batch (sv_cb_set_prefix_cache) at engine level, on the tiny v1 and v2 configurations.  Every test
drives TWO engines with the same weights through the same calls -- one with the cache on, its twin with the cache off -- and the contract is
exactness: every token, every finish, every log-prob record and the K / V bytes of a request's own pages are the twin's, bit for bit, whatever
was cached before and whatever is evicted meanwhile; the counters of sv_cb_prefix_cache_info say what was reused."""
import dataclasses

import pytest
import torch

import starvector_amd as sva
from oracle import starvector_oracle as O
from starvector_amd._lib import StarVectorBusy
from tests.gpu_util import build_engine, dev

pytestmark = pytest.mark.gpu

PAGE = 64
SAMPLED = dict(do_sample=True, temperature=0.9, top_p=0.95, top_k=40, repetition_penalty=1.2)
ZERO = {"lookups": 0, "reused": 0, "resident": 0, "unheld": 0, "evictions": 0}


def _rows(n, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, hidden, generator=g).to(torch.bfloat16).to(dev())


def _req(n_new, seed=None, **kw):
    r = dict(max_new_tokens=n_new, eos_token_id=-1)
    if seed is not None:
        r.update(SAMPLED, seed=seed)
    r.update(kw)
    return r


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


class Pair:
    """the engine with the cache and its twin without: every call goes to both, everything read is compared"""

    def __init__(self, arch, max_batch, max_seq_len):
        base = O.OracleConfig.tiny() if arch == "v1" else O.OracleConfig.tiny_v2()
        self.cfg = dataclasses.replace(base, n_positions=max(base.n_positions, max_seq_len), eos_token_id=-1)
        w = O.make_weights(self.cfg, seed=77)
        self.on = build_engine(self.cfg, w, max_batch=max_batch, max_seq_len=max_seq_len)
        self.off = build_engine(self.cfg, w, max_batch=max_batch, max_seq_len=max_seq_len)
        self.on.cb_set_prefix_cache(True)
        self.both = (self.on, self.off)
        self.hidden = self.cfg.hidden

    def reset(self):
        for e in self.both:
            e.cb_reset()

    def admit(self, embs, reqs, **kw):
        a, b = [e.cb_admit(list(embs), reqs, **kw) for e in self.both]
        assert a == b
        return a

    def admit_rect(self, x, reqs):
        a, b = [e.cb_admit(x, reqs) for e in self.both]
        assert a == b
        return a

    def admit_shared(self, embs, group, reqs, **kw):
        a, b = [e.cb_admit_shared(list(embs), None, group, reqs, **kw) for e in self.both]
        assert a == b
        return a

    def step(self, n=4):
        a, b = [e.cb_step(n) for e in self.both]
        assert a == b
        return a

    def run(self):
        calls = 0
        while self.step() > 0:
            calls += 1
            assert calls < 512

    def tokens(self, slots, tag=""):
        """the emitted tokens and live flags of `slots`: equal on both engines"""
        out = []
        (la, sa), (lb, sb) = [e.cb_poll() for e in self.both]
        for s in slots:
            assert (la[s], sa[s]) == (lb[s], sb[s]), (tag, s)
            ta, tb = self.on.cb_read(s, 0, sa[s]).tolist(), self.off.cb_read(s, 0, sb[s]).tolist()
            assert ta == tb, (tag, s, ta, tb)
            out.append(ta)
        return out

    def release(self, slots):
        for s in slots:
            for e in self.both:
                e.cb_release(s)

    def info(self):
        assert self.off.cb_prefix_cache_info() == ZERO
        return self.on.cb_prefix_cache_info()

    def kv(self, eng, row, first, count):
        return torch.stack([eng.debug_kv_read(i, row, first, count) for i in range(self.cfg.n_layer)]).cpu().view(torch.int16)

    def close(self):
        for e in self.both:
            e.close()


@pytest.fixture(scope="module", params=["v1", "v2"])
def pair(request):
    p = Pair(request.param, max_batch=8, max_seq_len=384)
    yield p
    p.close()


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


# ---- 1. the same prompt again: while the first request is live, and after it was released ------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_repeat_of_a_live_and_of_a_released_request(pair, mode):
    pair.reset()
    for L in (64, 65, 130, 200, 259):
        x = _rows(L, pair.hidden, 10 + L)
        seed = (lambda k: 100 * L + k) if mode == "sampled" else (lambda k: None)
        want = (L - 1) // PAGE
        i0 = pair.info()
        a = pair.admit([x], [_req(6, seed(0))])
        i1 = pair.info()
        assert _delta(i1, i0)["lookups"] == L // PAGE and _delta(i1, i0)["reused"] == 0, (L, i0, i1)
        b = pair.admit([x], [_req(6, seed(1))])                  # while the first one is live
        i2 = pair.info()
        assert _delta(i2, i1)["lookups"] == L // PAGE and _delta(i2, i1)["reused"] == want, (L, i1, i2)
        assert i2["unheld"] == i1["unheld"]
        pair.run()
        ta, tb = pair.tokens(a + b, f"{mode} L={L} live")
        assert len(ta) == len(tb) == 6 and (ta == tb) == (mode == "greedy")
        pair.release(a + b)
        i3 = pair.info()
        assert i3["resident"] == i2["resident"] and i3["unheld"] == i2["unheld"] + L // PAGE      # its full pages wait in the LRU list
        c = pair.admit([x], [_req(6, seed(0))])                  # after both were released
        i4 = pair.info()
        assert _delta(i4, i3)["reused"] == want and i4["unheld"] == i3["unheld"] - want, (L, i3, i4)
        pair.run()
        assert pair.tokens(c, f"{mode} L={L} released") == [ta]
        pair.release(c)
    assert pair.info()["evictions"] == 0


# ---- 2. a shared prefix, and a prompt that differs in row 0 ----------------------------------------------------------------------------------------
def test_shared_prefix_reuses_exactly_the_common_full_pages(pair):
    pair.reset()
    H = pair.hidden
    A = _rows(259, H, 1)                                         # the donor: its split-K remainder rows (259 % 256 = 3) lie in its tail page
    B = torch.cat([A[:128], _rows(62, H, 2)])                    # shares two pages, differs afterwards
    C = A[:200].clone()
    C[0, 0] = -C[0, 0] if float(C[0, 0]) != 0 else 1.0          # differs in row 0: nothing is reused
    D = A[:130].clone()                                          # a shorter total over the same rows
    E = torch.cat([A[:256], _rows(47, H, 3)])                    # 303 rows: own remainder rows, four pages from the donor
    a = pair.admit([A], [_req(5)])
    i0 = pair.info()
    assert i0["reused"] == 0 and i0["resident"] == 4
    got = pair.admit([B, C, D, E], [_req(5, 11), _req(5), _req(5, 12), _req(5)])      # hits and a miss in ONE admit
    i1 = pair.info()
    assert _delta(i1, i0)["reused"] == 2 + 0 + 2 + 4 and _delta(i1, i0)["lookups"] == 2 + 3 + 2 + 4
    assert i1["resident"] == 4 + 0 + 3 + 0 + 0                   # C's three pages are new keys; B's, D's and E's full pages are the donor's
    pair.run()
    pair.tokens(a + got, "shared prefix")
    pair.release(a + got)


# ---- 3. the sharer outlives the donor ----------------------------------------------------------------------------------------------------------------
def test_sharer_outlives_the_donor_and_decodes_across_a_page_boundary(pair):
    pair.reset()
    H = pair.hidden
    donor = _rows(120, H, 21)
    sharer = torch.cat([donor[:64], _rows(56, H, 22)])
    d = pair.admit([donor], [_req(40, 5)])
    s = pair.admit([sharer], [_req(30, 6)])                      # 120 + 30: decodes from page 1 into page 2
    assert pair.info()["reused"] == 1
    pair.step(2)
    pair.release(d)                                              # while it is still generating
    i = pair.info()
    assert i["resident"] == 1 and i["unheld"] == 0               # the sharer holds the page
    pair.run()
    assert len(pair.tokens(s, "sharer")[0]) == 30
    pair.release(s)
    assert pair.info()["unheld"] == 1


# ---- 4. cached pages are read, never written ---------------------------------------------------------------------------------------------------------
def test_reused_pages_keep_their_bytes_and_own_pages_are_the_twins(pair):
    pair.reset()
    H = pair.hidden
    A = _rows(130, H, 31)
    B = torch.cat([A[:128], _rows(22, H, 32)])
    a = pair.admit([A], [_req(8)])
    before = pair.kv(pair.on, a[0], 0, 128)
    assert torch.equal(before, pair.kv(pair.off, a[0], 0, 128))
    b = pair.admit([B], [_req(8, 3)])
    assert pair.info()["reused"] == 2 and a != b
    assert torch.equal(pair.kv(pair.on, a[0], 0, 128), before)              # the donor's pages after the hit's pass
    assert torch.equal(pair.kv(pair.on, b[0], 0, 128), before)              # ... are the sharer's first two
    assert torch.equal(pair.kv(pair.on, b[0], 0, 150), pair.kv(pair.off, b[0], 0, 150))      # cached and own rows: what the twin computed in one shot
    pair.run()
    pair.tokens(a + b, "untouched pages")
    assert torch.equal(pair.kv(pair.on, a[0], 0, 128), before) and torch.equal(pair.kv(pair.on, b[0], 0, 128), before)
    assert torch.equal(pair.kv(pair.on, b[0], 0, 157), pair.kv(pair.off, b[0], 0, 157))      # ... and the decode steps' rows
    assert torch.equal(pair.kv(pair.on, a[0], 0, 137), pair.kv(pair.off, a[0], 0, 137))
    pair.release(a + b)


# ---- 5. eviction ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_eviction_makes_room_and_busy_stays_busy(arch):
    p = Pair(arch, max_batch=2, max_seq_len=256)                 # 8 pages
    H = p.hidden
    P1, P2 = _rows(130, H, 41), _rows(130, H, 42)
    first = {}
    for name, x in (("P1", P1), ("P2", P2)):
        s = p.admit([x], [_req(4)])
        p.run()
        first[name] = p.tokens(s, name)
        p.release(s)
    i = p.info()
    assert (i["resident"], i["unheld"], i["evictions"]) == (4, 4, 0)
    big = p.admit([_rows(200, H, 43), _rows(200, H, 44)], [_req(56), _req(56, 9)])       # 4 + 4 pages: every page of the pool
    i = p.info()
    assert i["evictions"] == 4 and i["unheld"] == 0 and i["resident"] == 6
    p.run()
    p.tokens(big, "after eviction")
    p.release(big)
    i0 = p.info()
    s = p.admit([P1], [_req(4)])                                  # the evicted prompt misses ...
    assert _delta(p.info(), i0)["reused"] == 0
    p.run()
    assert p.tokens(s, "evicted prompt") == first["P1"]           # ... and its tokens are what they were
    p.release(s)
    # an admit the twin refuses is refused here too, and nothing moves (a pool of max_batch x pages_per_seq pages never runs short of pages
    # before it runs short of slots: the cached pages must not change that)
    x = p.admit([_rows(200, H, 45)], [_req(56)])                  # 4 pages and one of the two slots, live
    i1 = p.info()
    for e in p.both:
        with pytest.raises(StarVectorBusy):
            e.cb_admit([_rows(130, H, 46), _rows(130, H, 47)], [_req(60), _req(60)])      # 3 + 3 pages, 4 pages and one slot are left
    assert p.info() == i1
    y = p.admit([_rows(130, H, 48)], [_req(60, 4)])
    p.run()
    p.tokens(x + y, "after a refused admit")
    p.release(x + y)
    s = p.admit([P1], [_req(4)])
    p.run()
    assert p.tokens(s, "P1 at the end") == first["P1"]
    p.close()


# ---- 6. the other admit forms on a hit -----------------------------------------------------------------------------------------------------------------
def test_group_admit_rectangular_admit_and_logprob_records_on_a_hit(pair):
    pair.reset()
    H = pair.hidden
    A, B = _rows(130, H, 51), _rows(200, H, 52)
    s = pair.admit([A, B], [_req(3), _req(3)])
    pair.run()
    pair.release(s)
    i0 = pair.info()
    g = pair.admit_shared([A, torch.cat([B[:64], _rows(30, H, 53)])], [0, 0, 1, 0], [_req(7, 1), _req(7, 2), _req(7, 3), _req(7)])
    i1 = pair.info()
    assert _delta(i1, i0)["reused"] == 2 + 1
    pair.run()
    toks = pair.tokens(g, "group admit")
    assert toks[0] != toks[1]
    pair.release(g)
    # the rectangular form: two prompts of one length, one a hit
    r = pair.admit_rect(torch.stack([A, _rows(130, H, 54)]).contiguous(), [_req(5, 8), _req(5)])
    assert _delta(pair.info(), i1)["reused"] == 2
    pair.run()
    pair.tokens(r, "rectangular admit")
    pair.release(r)
    # records
    lps = [dict(k=3, source="raw"), dict(k=0, source="processed"), None]
    i2 = pair.info()
    slots = pair.admit([B, A, A], [_req(6, 5), _req(6), _req(6)], logprobs=lps)
    assert _delta(pair.info(), i2)["reused"] == 3 + 2 + 2
    pair.run()
    pair.tokens(slots, "log-prob records")
    for s_, l in zip(slots, lps):
        if l is None:
            continue
        ra, rb = [e.cb_read_logprobs(s_, 0, 6) for e in pair.both]
        for x, y in zip(ra, rb):
            assert torch.equal(_bits(x), _bits(y)), s_
    pair.release(slots)


# ---- 7. drafting and a chunk budget on a hit -----------------------------------------------------------------------------------------------------------
def test_drafting_and_chunked_prefill_on_a_hit(pair):
    pair.reset()
    H = pair.hidden
    A = _rows(200, H, 61)
    B = torch.cat([A[:128], _rows(131, H, 62)])                  # 259 rows, 131 own rows: three chunks of at most 64
    plain = pair.admit([A, B], [_req(12), _req(12, 7)])
    pair.run()
    ref = pair.tokens(plain, "reference")
    pair.reset()
    try:
        for e in pair.both:
            e.cb_set_lookup(3)                                   # two slots of four rows
            e.set_prefill_chunk(64)
        a = pair.admit([A], [_req(12)])
        b = pair.admit([B], [_req(12, 7)])
        assert pair.info()["reused"] == 2
        pair.run()
        assert pair.tokens(a + b, "drafting + chunks") == ref
        pair.release(a + b)
        c = pair.admit([B, A], [_req(12, 7), _req(12)])          # both hit: four and three pages
        assert pair.info()["reused"] == 2 + 4 + 3
        pair.run()
        assert pair.tokens(c, "drafting + chunks, all hit") == ref[::-1]
    finally:
        pair.reset()
        for e in pair.both:
            e.cb_set_lookup(0)
            e.set_prefill_chunk(0)


# ---- 8. reset and refusals -------------------------------------------------------------------------------------------------------------------------------
def test_reset_empties_the_table_and_the_setter_refuses(pair):
    pair.reset()
    A = _rows(130, pair.hidden, 71)
    s = pair.admit([A], [_req(3)])
    pair.run()
    ref = pair.tokens(s)
    with pytest.raises(sva.StarVectorHipError, match="active"):
        pair.on.cb_set_prefix_cache(True)
    with pytest.raises(sva.StarVectorHipError, match="active"):
        pair.on.cb_set_prefix_cache(False)
    pair.release(s)
    assert pair.info()["unheld"] == 2
    pair.reset()
    assert pair.info() == ZERO
    s = pair.admit([A], [_req(3)])
    i = pair.info()
    assert i["lookups"] == 2 and i["reused"] == 0 and i["resident"] == 2      # the setting stayed, the pages did not
    pair.run()
    assert pair.tokens(s) == ref
    pair.reset()


def test_the_setter_refuses_an_e4m3_cache():
    from tests.test_gpu_kv_fp8 import _tiny
    cfg, w, eng = _tiny("v1", max_batch=2, max_seq_len=128)
    with pytest.raises(NotImplementedError, match="fp8_e4m3"):
        eng.cb_set_prefix_cache(True)
    eng.cb_set_prefix_cache(False)
    assert eng.cb_prefix_cache_info() == ZERO
    eng.close()


# ---- 9. off is off ---------------------------------------------------------------------------------------------------------------------------------------
def test_switched_off_nothing_is_cached(pair):
    pair.reset()
    pair.on.cb_set_prefix_cache(False)
    try:
        A = _rows(200, pair.hidden, 81)
        for k in range(2):
            s = pair.admit([A], [_req(5, 3)])
            assert pair.on.cb_prefix_cache_info() == ZERO
            pair.run()
            pair.tokens(s, "off")
            pair.release(s)
            fa, fb = [(C.value, T.value) for C, T in [_free(e) for e in pair.both]]
            assert fa == fb and fa[0] == fa[1]                    # every page is back in the free list
    finally:
        pair.reset()
        pair.on.cb_set_prefix_cache(True)


def _free(eng):
    import ctypes
    f, t = ctypes.c_int32(0), ctypes.c_int32(0)
    assert eng.lib.sv_debug_free_pages(eng._h, ctypes.byref(f), ctypes.byref(t)) == 0
    return f, t


# ---- 10. through the batcher -----------------------------------------------------------------------------------------------------------------------------
def test_the_batcher_reuses_pages_across_submits_and_across_the_parts_of_a_group(pair):
    from starvector_amd.batching import ContinuousBatcher
    pair.reset()
    H = pair.hidden
    A, G = _rows(200, H, 91)[None], _rows(130, H, 92)[None]
    params = [dict(_req(6, 40 + k)) for k in range(12)]          # 12 samples of one prompt on 8 rows: admitted in parts
    res, info = {}, {}
    for name, eng, kw in (("on", pair.on, dict(prefix_cache=True)), ("off", pair.off, {})):
        b = ContinuousBatcher(eng, steps_per_poll=2, **kw)
        try:
            one = b.submit(A, _req(6, 1)).result(60)[0].tolist()
            mid = b.prefix_cache_info()
            two = b.submit(A, _req(6, 2)).result(60)[0].tolist()
            after = b.prefix_cache_info()
            grp = [h.result(60)[0].tolist() for h in b.submit_group(G, params)]
            res[name], info[name] = (one, two, grp), (mid, after, b.prefix_cache_info())
        finally:
            b.close()
    assert res["on"] == res["off"]
    assert res["on"][0] != res["on"][1] and len({tuple(t) for t in res["on"][2]}) > 1
    mid, after, end = info["on"]
    assert mid["reused"] == 0 and after["reused"] == 3            # the second submit of the 200-row prompt
    assert end["reused"] - after["reused"] >= 2                   # a later part of the group found the first part's two pages
    assert info["off"] == (ZERO, ZERO, ZERO)
    pair.on.cb_set_prefix_cache(True)                             # (the batcher left the engine reset, the setting on)
