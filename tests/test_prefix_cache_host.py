"""CPU: the prefix cache of the continuous batch (sv_cb_set_prefix_cache) without a GPU.
  * the chaining and hit-length function of the library (sv_debug_prefix_hit) against the restatement in tests/prefix_key_ref.py;
  * the checks the new entry points run in front of the engine;
  * the Python layers: ContinuousBatcher(prefix_cache=), LLM(enable_prefix_caching=), serve --enable-prefix-caching."""
import ctypes as C
import random

import numpy as np
import pytest

from starvector_amd import _lib
from tests import prefix_key_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _u64(pairs):
    flat = [v for p in pairs for v in p]
    return (C.c_uint64 * max(len(flat), 1))(*flat)


def _hit(lib, digests, L, table):
    n = len(digests)
    keys = (C.c_uint64 * max(2 * n, 1))()
    h = C.c_int32(-1)
    rc = lib.sv_debug_prefix_hit(_u64(digests), n, L, _u64(table), len(table), keys, C.byref(h))
    assert rc == 0, lib.sv_last_error().decode()
    return h.value, [(keys[2 * k], keys[2 * k + 1]) for k in range(n)]


def _digests(r, n):
    return [(r.getrandbits(64), r.getrandbits(64)) for _ in range(n)]


def test_the_binding_exposes_the_entry_points(lib):
    for name in ("sv_cb_set_prefix_cache", "sv_cb_prefix_cache_info"):
        assert name in _lib.PRODUCT_PROTOTYPES and hasattr(lib, name)
    for name in ("sv_debug_page_digests", "sv_debug_prefix_hit"):
        assert name in _lib.DEBUG_PROTOTYPES and hasattr(lib, name)


@pytest.mark.parametrize("L", [63, 64, 65, 128, 129, 259])
def test_chain_and_hit_length_against_the_restatement(lib, L):
    r = random.Random(L)
    d = _digests(r, L // 64)
    ref_keys = R.keys_of(d)
    # an empty table, the whole chain in the table (a match longer than (L - 1) / 64 when L is a multiple of 64), every prefix of it
    for n_in in range(len(d) + 1):
        table = ref_keys[:n_in]
        h, keys = _hit(lib, d, L, table)
        assert keys == ref_keys
        assert h == R.hit_pages(d, L, set(table)) == min(n_in, (L - 1) // 64), (L, n_in)
    # keys of other prompts in the table change nothing; the order of the table does not matter
    noise = R.keys_of(_digests(r, 3))
    table = noise + ref_keys[::-1]
    assert _hit(lib, d, L, table)[0] == (L - 1) // 64


def test_full_match_is_capped_so_that_one_own_row_is_computed(lib):
    r = random.Random(5)
    for L, want in ((64, 0), (128, 1), (256, 3), (65, 1), (129, 2)):
        d = _digests(r, L // 64)
        assert len(d) > want or L % 64                             # the match is longer than the cap exactly when L is a multiple of 64
        assert _hit(lib, d, L, R.keys_of(d))[0] == want


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_mismatch_cuts_the_chain_where_it_occurs(lib, where):
    r = random.Random(11)
    L = 259 + 64                                                    # 5 full pages, all reusable
    donor = _digests(r, 5)
    table = R.keys_of(donor)
    k = {"first": 0, "middle": 2, "last": 4}[where]
    d = list(donor)
    d[k] = (d[k][0] ^ 1, d[k][1])                                   # one bit of one lane of one page's digest
    h, keys = _hit(lib, d, L, table)
    assert h == k == R.hit_pages(d, L, set(table))
    assert keys[:k] == table[:k] and all(a != b for a, b in zip(keys[k:], table[k:]))      # every later key differs: position and prefix are in the key
    # the same page content at another depth is another key: a table of the donor's keys shifted by one page matches nothing
    assert _hit(lib, donor[1:], L - 64, table)[0] == 0
    # the lanes are chained separately from one another's digests but not independently: flipping lane b alone also cuts
    d = list(donor)
    d[k] = (d[k][0], d[k][1] ^ (1 << 63))
    assert _hit(lib, d, L, table)[0] == k


def test_the_numpy_digest_sees_every_bit_and_every_position():
    rng = np.random.default_rng(3)
    page = rng.integers(0, 1 << 16, size=(64, 32), dtype=np.uint16)
    base = R.page_digest(page)
    flip = page.copy(); flip[63, 31] ^= 1
    swap_rows = page.copy(); swap_rows[[0, 1]] = swap_rows[[1, 0]]
    swap_el = page.copy(); swap_el[5, [2, 3]] = swap_el[5, [3, 2]]
    for other in (flip, swap_rows, swap_el):
        d = R.page_digest(other)
        assert d[0] != base[0] and d[1] != base[1]
    # the reduction is commutative: any split of the words gives the same pair (here: python ints, word by word)
    w = page.reshape(-1).view("<u8")
    a = sum(R.mix64((int(x) + (i + 1) * R.C1) & R.M64) for i, x in enumerate(w)) & R.M64
    b = 0
    for i, x in enumerate(w):
        b ^= R.mix64(((int(x) ^ R.C3) + (i + 1) * R.C2) & R.M64)
    assert (a, b) == base


def test_argument_checks_run_in_front_of_the_engine(lib):
    err = lambda: lib.sv_last_error().decode()
    assert lib.sv_cb_set_prefix_cache(None, 1) == -22 and err() == "null engine"
    assert lib.sv_cb_set_prefix_cache(None, 0) == -22
    out5 = (C.c_int64 * 5)()
    assert lib.sv_cb_prefix_cache_info(None, out5) == -22 and err() == "sv_cb_prefix_cache_info: null argument"
    assert lib.sv_cb_prefix_cache_info(C.c_void_p(16), None) == -22
    h = C.c_int32(0)
    d = _u64([(1, 2)])
    who = "sv_debug_prefix_hit"
    assert lib.sv_debug_prefix_hit(d, 1, 64, None, 0, None, None) == -22 and err() == who + ": null argument"
    assert lib.sv_debug_prefix_hit(None, 1, 64, None, 0, None, C.byref(h)) == -22
    assert lib.sv_debug_prefix_hit(d, 1, 64, None, 1, None, C.byref(h)) == -22
    assert lib.sv_debug_prefix_hit(d, 1, 128, None, 0, None, C.byref(h)) == -22 and "2 full pages" in err()
    assert lib.sv_debug_prefix_hit(d, 1, 0, None, 0, None, C.byref(h)) == -22
    assert lib.sv_debug_prefix_hit(None, 0, 63, None, 0, None, C.byref(h)) == 0 and h.value == 0
    p, out = C.c_void_p(16), (C.c_uint64 * 64)()
    who = "sv_debug_page_digests"
    lens = (C.c_int32 * 2)(64, 130)
    assert lib.sv_debug_page_digests(None, 2, lens, 0, 64, 4, out, None) == -22 and err() == who + ": null argument"
    assert lib.sv_debug_page_digests(p, 2, lens, 0, 64, 4, None, None) == -22
    assert lib.sv_debug_page_digests(p, 0, lens, 0, 64, 4, out, None) == -22 and "bad argument" in err()
    assert lib.sv_debug_page_digests(p, 2, lens, 0, 60, 4, out, None) == -22 and "multiple of 8" in err()
    assert lib.sv_debug_page_digests(C.c_void_p(24), 2, lens, 0, 64, 4, out, None) == -22 and "16-byte aligned" in err()
    assert lib.sv_debug_page_digests(p, 2, None, 0, 64, 4, out, None) == -22 and "bad prompt length 0" in err()
    assert lib.sv_debug_page_digests(p, 2, (C.c_int32 * 2)(64, 0), 0, 64, 4, out, None) == -22 and "prompt 1" in err()
    assert lib.sv_debug_page_digests(p, 2, lens, 0, 64, 1, out, None) == -22 and "exceed max_pages" in err()


# ---- the Python layers over a scripted engine -----------------------------------------------------------------------------------------------
def test_the_batcher_sets_the_cache_before_the_first_admit():
    from starvector_amd.batching import ContinuousBatcher
    from tests.test_batching_host import _CbEngine, _emb

    class Eng(_CbEngine):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.calls = []

        def cb_reset(self):
            self.calls.append("reset")
            super().cb_reset()

        def cb_set_prefix_cache(self, on):
            assert not self.slots
            self.calls.append(("set", on))

        def cb_prefix_cache_info(self):
            return {"lookups": 4, "reused": 3, "resident": 2, "unheld": 1, "evictions": 0}

        def cb_admit(self, emb, reqs):
            self.calls.append(("admit", len(reqs)))
            return super().cb_admit(emb, reqs)

    eng = Eng(max_batch=4)
    b = ContinuousBatcher(eng, steps_per_poll=1, prefix_cache=True)
    assert eng.calls == ["reset", ("set", True)] and b.prefix_cache
    assert b.generate(_emb(10), dict(max_new_tokens=4))[0].tolist() == [10, 11, 12, 13]
    assert eng.calls[2] == ("admit", 1)
    assert b.prefix_cache_info() == {"lookups": 4, "reused": 3, "resident": 2, "unheld": 1, "evictions": 0}
    b.close()
    plain_eng = _CbEngine(max_batch=4)                  # off: the engine is never asked (it has no such method)
    plain = ContinuousBatcher(plain_eng, steps_per_poll=1)
    assert not plain.prefix_cache and plain.prefix_cache_info() == {"lookups": 0, "reused": 0, "resident": 0, "unheld": 0, "evictions": 0}
    assert plain.generate(_emb(3), dict(max_new_tokens=2))[0].tolist() == [3, 4]
    plain.close()


def test_the_llm_takes_vllms_keyword_and_refuses_it_with_an_fp8_cache(monkeypatch):
    from starvector_amd import batching
    from starvector_amd import vllm as VL
    for kv in ("fp8", "fp8_e4m3"):
        with pytest.raises(NotImplementedError, match="enable_prefix_caching"):
            VL.LLM("no-such-dir", enable_prefix_caching=True, kv_cache_dtype=kv)
    with pytest.raises(Exception) as ei:                # accepted: what fails is the checkpoint directory, not the keyword
        VL.LLM("no-such-dir", enable_prefix_caching=True)
    assert not isinstance(ei.value, (TypeError, NotImplementedError)), ei.value
    assert "enable_prefix_caching" in VL.LLM.__doc__
    # generate hands the flag to its batcher, and only when it is set
    seen = []

    class B:
        def __init__(self, eng, **kw):
            seen.append(kw)
            raise KeyboardInterrupt                     # the test ends here: nothing of generate runs

    monkeypatch.setattr(batching, "ContinuousBatcher", B)
    for flag, want in ((True, dict(prefix_cache=True)), (False, {})):
        llm = VL.LLM.__new__(VL.LLM)
        llm._lookup, llm._prefix_cache, llm.engine = {}, flag, None
        llm.prepare = lambda inputs, sp: []
        with pytest.raises(KeyboardInterrupt):
            llm.generate([], None)
        assert seen.pop() == want


def test_the_worker_and_the_command_line_pass_the_flag(monkeypatch):
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
    serve.ModelWorker("c", "w", "id", True, "starvector-x", model=model, enable_prefix_caching=True)
    assert seen == dict(prefix_cache=True)
    seen.clear()
    serve.ModelWorker("c", "w", "id", True, "starvector-x", model=model, enable_prefix_caching=True, prompt_lookup_num_tokens=3)
    assert seen == dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=0, prefix_cache=True)
    seen.clear()
    serve.ModelWorker("c", "w", "id", True, "starvector-x", model=model)
    assert seen == {}                                    # off: the batcher is built exactly as before
    # the command line: the flag reaches the worker; it is refused without continuous batching and with an fp8 KV cache
    got = {}
    monkeypatch.setattr(serve, "ModelWorker", lambda *a, **kw: got.update(kw) or (_ for _ in ()).throw(SystemExit(0)))
    with pytest.raises(SystemExit):
        serve.main(["--model-path", "x", "--no-register", "--enable-prefix-caching"])
    assert got["enable_prefix_caching"] is True
    got.clear()
    with pytest.raises(SystemExit):
        serve.main(["--model-path", "x", "--no-register"])
    assert got["enable_prefix_caching"] is False
    for extra in (["--no-continuous-batching"], ["--kv-cache-dtype", "fp8"]):
        got.clear()
        with pytest.raises(SystemExit) as ei:
            serve.main(["--model-path", "x", "--no-register", "--enable-prefix-caching"] + extra)
        assert ei.value.code == 2 and not got
