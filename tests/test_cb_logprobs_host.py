"""CPU: per-request log-probs on the continuous batch (sv_cb_admit_logprobs, sv_cb_read_logprobs, sv_op_cb_logprobs) -- the C ABI surface and
its argument checks through the built library, which come before any device work; the batcher's plumbing over a fake engine; the formatting of
`LLM.generate(..., logprobs=k)` from hand-made arrays; `SamplingParams(logprobs=...)` still raising."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from starvector_amd import _lib
from starvector_amd import vllm as VL
from starvector_amd.batching import ContinuousBatcher, TokenLogprobs
from starvector_amd.engine import cb_logprobs, cb_requests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")


def _header(name="starvector_hip.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _err(lib):
    return lib.sv_last_error().decode()


# ---- 1-3. the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols(lib):
    for name in ("sv_cb_admit_logprobs", "sv_cb_read_logprobs"):
        assert hasattr(lib, name) and name in _lib.PRODUCT_PROTOTYPES and name in _header()
    assert hasattr(lib, "sv_op_cb_logprobs") and "sv_op_cb_logprobs" in _lib.DEBUG_PROTOTYPES
    assert "sv_op_cb_logprobs" in _header("starvector_hip_debug.h")


def test_binding_struct_matches_the_header_field_for_field():
    body = re.search(r"typedef struct sv_cb_logprobs \{(.*?)\} sv_cb_logprobs;", _header(), flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert all(d.startswith("int32_t ") for d in decls)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", d)[-1] for d in decls]
    assert fields == [f[0] for f in _lib.SvCbLogprobs._fields_] == ["enable", "k", "source"]
    assert all(f[1] is C.c_int32 for f in _lib.SvCbLogprobs._fields_) and C.sizeof(_lib.SvCbLogprobs) == 12
    admit = _lib.PRODUCT_PROTOTYPES["sv_cb_admit_logprobs"][1]
    shared = _lib.PRODUCT_PROTOTYPES["sv_cb_admit_shared"][1]
    assert len(admit) == len(shared) + 1 and admit[7]._type_ is _lib.SvCbLogprobs and admit[:7] == shared[:7] and admit[8:] == shared[7:]


def test_abi_version_stays_9_and_sv_cb_request_is_unchanged(lib):
    assert lib.sv_abi_version() == 9 == _lib.ABI_VERSION and "#define SV_ABI_VERSION 9" in _header()
    assert [f[0] for f in _lib.SvCbRequest._fields_][-2:] == ["n_stop_any", "stop_any_ids"] and len(_lib.SvCbRequest._fields_) == 23


P = C.c_void_p(64)                                                 # never dereferenced: the checks come first


def _admit(lib, reqs, lps):
    n = len(reqs)
    arr, keep = cb_requests(reqs)
    slots = (C.c_int32 * n)()
    lens, group = (C.c_int32 * n)(*[4] * n), (C.c_int32 * n)(*range(n))
    return lib.sv_cb_admit_logprobs(None, P, n, lens, n, group, arr, lps, slots, None)


@pytest.mark.parametrize("case, entry, words", [
    ("k = -1", dict(k=-1, source=0), ["k=-1", "0..32"]),
    ("k = 33", dict(k=33, source=1), ["k=33", "0..32"]),
    ("source 2", dict(k=3, source=2), ["source=2"]),
    ("source -1", dict(k=3, source=-1), ["source=-1"]),
])
def test_admit_refusals_come_before_any_device_work(lib, case, entry, words):
    reqs = [dict(max_new_tokens=4), dict(max_new_tokens=4)]
    lps = (_lib.SvCbLogprobs * 2)()
    lps[1].enable, lps[1].k, lps[1].source = 1, entry["k"], entry["source"]
    assert _admit(lib, reqs, lps) == -22, case
    for w in words + ["request 1"]:
        assert w in _err(lib), (case, _err(lib))


def test_admit_refuses_the_raw_source_on_a_vllm_slot(lib):
    reqs = [dict(max_new_tokens=4, semantics="vllm"), dict(max_new_tokens=4)]
    lps = (_lib.SvCbLogprobs * 2)()
    lps[0].enable, lps[0].k, lps[0].source = 1, 3, 0
    lps[1].enable, lps[1].k, lps[1].source = 1, 3, 0
    assert _admit(lib, reqs, lps) == -22 and "request 0" in _err(lib) and "source 0" in _err(lib) and "vLLM" in _err(lib)
    # a well-formed request passes every check that needs no engine and stops at the engine itself
    lps[0].source = 1
    assert _admit(lib, reqs, lps) == -22 and "null engine" in _err(lib)
    assert _admit(lib, reqs, None) == -22 and "null engine" in _err(lib)
    # an entry that is not enabled is not read
    lps[0].enable, lps[0].k, lps[0].source = 0, 99, 7
    assert _admit(lib, reqs, lps) == -22 and "null engine" in _err(lib)
    assert lib.sv_cb_read_logprobs(None, 0, 0, 1, None, None, None, None) == -22 and "null engine" in _err(lib)


def test_operator_refusals_come_before_any_device_work(lib):
    arr, keep = cb_requests([dict(max_new_tokens=4, semantics="vllm")])
    lens = (C.c_int32 * 1)(0)
    out, lp, rk, ids, vals = (C.c_int32 * 1)(), (C.c_float * 1)(), (C.c_int32 * 1)(), (C.c_int32 * 4)(), (C.c_float * 4)()

    def call(entry, ld_k=4):
        lps = (_lib.SvCbLogprobs * 1)()
        lps[0].enable, lps[0].k, lps[0].source = 1, entry[0], entry[1]
        return lib.sv_op_cb_logprobs(P, 1, 8, 8, arr, lps, None, 0, lens, out, lp, rk, ids, vals, ld_k, None)

    assert call((33, 1)) == -22 and "k=33" in _err(lib)
    assert call((2, 3)) == -22 and "source=3" in _err(lib)
    assert call((2, 0)) == -22 and "source 0" in _err(lib)
    assert call((5, 1)) == -22 and "ld_k=4" in _err(lib)
    assert lib.sv_op_cb_logprobs(P, 1, 8, 8, arr, None, None, 0, lens, out, lp, rk, ids, vals, 4, None) == -22


def test_python_logprobs_entries():
    reqs = [dict(max_new_tokens=4), dict(max_new_tokens=4, semantics="vllm"), dict(max_new_tokens=4)]
    assert cb_logprobs(reqs, None) is None and cb_logprobs(reqs, [None] * 3) is None
    arr = cb_logprobs(reqs, [dict(k=5), dict(k=0), None])
    assert [(a.enable, a.k, a.source) for a in arr] == [(1, 5, 0), (1, 0, 1), (0, 0, 0)]      # default source: raw under HF, processed under vLLM
    arr = cb_logprobs(reqs, [dict(k=2, source="processed"), dict(k=1, source="raw"), dict(k=3, source=1)])
    assert [(a.enable, a.k, a.source) for a in arr] == [(1, 2, 1), (1, 1, 0), (1, 3, 1)]
    with pytest.raises(ValueError, match="source"):
        cb_logprobs(reqs, [dict(k=2, source="cooked"), None, None])
    with pytest.raises(ValueError, match="one logprobs entry per request"):
        cb_logprobs(reqs, [dict(k=2)])


# ---- the batcher over a fake engine --------------------------------------------------------------------------------------------------------
class _FakeEngine:
    """Slots emit the tokens 10 * slot + step; a recording slot's log-prob of step t is -(slot + t / 10)."""

    class cfg:
        max_batch = 4

    def __init__(self):
        self.used, self.steps, self.budget, self.lp = {}, {}, {}, {}
        self.admit_kwargs = []

    def cb_admit(self, embeds, requests, **kw):
        self.admit_kwargs.append(kw)
        lps = kw.get("logprobs") or [None] * len(requests)
        slots = []
        for r, l in zip(requests, lps):
            s = min(set(range(4)) - set(self.used))
            self.used[s], self.steps[s], self.budget[s], self.lp[s] = True, 1, int(r["max_new_tokens"]), l
            slots.append(s)
        return slots

    def cb_step(self, n):
        for s in self.used:
            self.steps[s] = min(self.budget[s], self.steps[s] + n)
        return sum(self.steps[s] < self.budget[s] for s in self.used)

    def cb_poll(self):
        return ([int(s in self.used and self.steps[s] < self.budget[s]) for s in range(4)], [self.steps.get(s, 0) for s in range(4)])

    def cb_read(self, s, first, count):
        return torch.tensor([10 * s + t for t in range(first, first + count)], dtype=torch.int64)

    def cb_read_logprobs(self, s, first, count):
        if self.lp[s] is None:
            raise ValueError("slot records no log-probs")
        k = self.lp[s]["k"]
        cols = range(first, first + count)
        return (torch.tensor([-(s + t / 10) for t in cols]), torch.tensor([1 + t for t in cols], dtype=torch.int32),
                torch.tensor([[100 * t + j for j in range(k)] for t in cols], dtype=torch.int32).view(count, k),
                torch.tensor([[-float(j) for j in range(k)] for t in cols]).view(count, k))

    def cb_release(self, s):
        del self.used[s]

    def cb_reset(self):
        self.used.clear()


def test_batcher_delivers_the_record_alongside_the_tokens():
    eng = _FakeEngine()
    b = ContinuousBatcher(eng, steps_per_poll=3)
    emb = torch.zeros(1, 2, 8)
    seen = []
    try:
        plain = b.submit(emb, dict(max_new_tokens=5))
        plain.result(10)
        assert eng.admit_kwargs == [{}] and plain.logprobs is None           # a request without the key is admitted as before
        h = b.submit(emb, dict(max_new_tokens=7, logprobs=2, logprob_source="processed"),
                     on_tokens=lambda toks, first: seen.append((first, len(toks), len(h.lp_chunks))))
        toks = h.result(10)
    finally:
        b.close()
    assert eng.admit_kwargs[1] == dict(logprobs=[dict(k=2, source="processed")])
    rec = h.logprobs
    assert isinstance(rec, TokenLogprobs) and toks.shape == (1, 7)
    s = int(toks[0, 0]) // 10
    assert torch.allclose(rec.logprobs, torch.tensor([-(s + t / 10) for t in range(7)])) and rec.ranks.tolist() == list(range(1, 8))
    assert rec.top_ids.shape == rec.top_logprobs.shape == (7, 2) and rec.top_ids[:, 1].tolist() == [100 * t + 1 for t in range(7)]
    assert seen and all(chunks >= 1 for _, _, chunks in seen) and sum(n for _, n, _ in seen) == 7      # the record is there when the tokens arrive


# ---- 4-5. the vLLM layer -------------------------------------------------------------------------------------------------------------------
def test_generate_formatting_from_hand_made_arrays():
    toks = [5, 9, 2]
    token_lp = [-0.5, -3.0, -0.25]
    ranks = [1, 4, 2]
    ids = [[5, 7, 8], [1, 6, -1], [3, 2, -1]]
    lps = [[-0.5, -1.5, -2.5], [-0.1, -2.0, NEG], [-0.125, -0.25, NEG]]
    dicts, total = VL.completion_logprobs(toks, torch.tensor(token_lp), torch.tensor(ranks, dtype=torch.int32),
                                          torch.tensor(ids, dtype=torch.int32), torch.tensor(lps), decode=lambda i: f"<{i}>")
    assert total == sum(token_lp) == -3.75
    assert [sorted(d) for d in dicts] == [[5, 7, 8], [1, 6, 9], [2, 3]]                     # -1 ids dropped; the sampled id added when outside
    assert dicts[0][5] == VL.Logprob(-0.5, 1, "<5>") and dicts[0][7] == VL.Logprob(-1.5, 2, "<7>") and dicts[0][8].rank == 3
    assert dicts[1][9] == VL.Logprob(-3.0, 4, "<9>") and dicts[1][1].rank == 1 and dicts[1][6] == VL.Logprob(-2.0, 2, "<6>")
    assert dicts[2][2] == VL.Logprob(-0.25, 2, "<2>") and dicts[2][3] == VL.Logprob(-0.125, 1, "<3>")
    assert all(not math.isinf(v.logprob) for d in dicts for v in d.values())
    # k = 0: the sampled token alone, with its own rank
    d0, t0 = VL.completion_logprobs([4], [-1.0], [3], [[]], [[]])
    assert d0 == [{4: VL.Logprob(-1.0, 3, None)}] and t0 == -1.0
    with pytest.raises(ValueError, match="one record column per token"):
        VL.completion_logprobs([4, 5], [-1.0], [3], [[]], [[]])
    out = VL.CompletionOutput(0, "", toks, cumulative_logprob=total, logprobs=dicts)
    assert out.cumulative_logprob == -3.75 and len(out.logprobs) == len(out.token_ids)


def test_sampling_params_logprobs_still_raises():
    with pytest.raises(NotImplementedError):
        VL.SamplingParams(logprobs=1)
    with pytest.raises(NotImplementedError):
        VL.SamplingParams(prompt_logprobs=1)
    assert "prompt_logprobs" in VL.__doc__ and "generate(..., logprobs=k)" in VL.__doc__
