"""CPU: the shared prompt pass's host side -- the new C ABI symbols (sv_generate_shared, sv_cb_admit_shared) and their argument checks,
the page plan as sv_debug_shared_plan states it against its closed form, and the routes above the engine: HipCausalLM.generate
(num_return_sequences), the ContinuousBatcher's group submit and vllm.LLM.generate(n) over stand-in engines."""
import ctypes as C
import os
import re

import pytest
import torch

from starvector_amd import _lib, engine as E, vllm as V
from starvector_amd.batching import ContinuousBatcher
from tests.test_host_logic import _FakeEngine, _fake_lm
from tests.test_ragged_host import _FakeRaggedEngine, _ragged_lm
from tests.test_vllm_api_host import _ScriptedEngine, _scripted_llm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE = 64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(sv_[a-z0-9_]+)\s*\(", text))


def test_shared_symbols_are_declared_bound_and_exported(lib):
    prod, dbg = _declared("starvector_hip.h"), _declared("starvector_hip_debug.h")
    for name, n_args in (("sv_generate_shared", 11), ("sv_cb_admit_shared", 9)):
        assert name in prod and name in _lib.PRODUCT_PROTOTYPES and hasattr(lib, name), name
        assert len(_lib.PRODUCT_PROTOTYPES[name][1]) == n_args, name
    for name, n_args in (("sv_debug_shared_plan", 8), ("sv_debug_block_table", 4), ("sv_debug_free_pages", 3)):
        assert name in dbg and name not in prod and name in _lib.DEBUG_PROTOTYPES and hasattr(lib, name), name
        assert len(_lib.DEBUG_PROTOTYPES[name][1]) == n_args, name
    assert lib.sv_abi_version() == 9 and _lib.ABI_VERSION == 9            # entry points only: an old binding keeps working
    assert not [n for n in prod if n.startswith("sv_debug_")]


def _closed_form(lens, group, budgets):
    shared = [lens[g] // PAGE for g in group]
    private = [-(-(lens[g] + b) // PAGE) - lens[g] // PAGE for g, b in zip(group, budgets)]
    return dict(shared=shared, private=private, total=sum(n // PAGE for n in lens) + sum(private))


@pytest.mark.parametrize("lens,group,budgets", [
    ([128], [0, 0, 0, 0], [40] * 4),                       # len % 64 == 0: no tail page to copy, two shared pages
    ([37], [0, 0, 0], [10] * 3),                           # len < 64: nothing shared
    ([259], [0] * 8, [64] * 8),                            # the im2svg prompt: 4 shared pages, the tail page private
    ([5, 64, 259, 130], [0, 0, 1, 1, 1, 2, 3, 3], [20] * 8),
    ([259, 70], [0, 0, 0, 1, 1], [1, 64, 500, 59, 7]),     # different budgets inside a group
])
def test_shared_plan_is_the_closed_form(lens, group, budgets):
    plan = E.shared_plan(lens, group, budgets)
    assert plan == _closed_form(lens, group, budgets)
    # what sharing saves: the repeated route holds ceil((len + budget) / 64) pages per request
    repeated = sum(-(-(lens[g] + b) // PAGE) for g, b in zip(group, budgets))
    per_prompt = {u: group.count(u) for u in set(group)}
    assert repeated - plan["total"] == sum((per_prompt[u] - 1) * (lens[u] // PAGE) for u in per_prompt)


def test_shared_plan_with_one_sample_per_prompt_is_todays_count():
    lens, budgets = [5, 64, 259, 130, 700], [3, 64, 100, 1, 324]
    plan = E.shared_plan(lens, list(range(5)), budgets)
    assert plan["total"] == sum(-(-(n + b) // PAGE) for n, b in zip(lens, budgets))         # sv_cb_admit_ragged's need_pages
    assert [s + p for s, p in zip(plan["shared"], plan["private"])] == [-(-(n + b) // PAGE) for n, b in zip(lens, budgets)]


def test_shared_plan_rejects_what_the_admit_rejects():
    with pytest.raises(ValueError, match="referenced by no request"):
        E.shared_plan([10, 20, 30], [0, 0, 1], [4, 4, 4])                   # prompt 2 has no request
    with pytest.raises(ValueError, match=r"group\[1\] = 3 outside"):
        E.shared_plan([10, 20], [0, 3], [4, 4])
    with pytest.raises(ValueError, match="order their first request appears"):
        E.shared_plan([10, 20], [1, 0], [4, 4])
    with pytest.raises(ValueError, match="prompt 1: bad prompt length 0"):
        E.shared_plan([10, 0], [0, 1], [4, 4])
    with pytest.raises(ValueError, match=r"budgets\[1\] = 0"):
        E.shared_plan([10], [0, 0], [4, 0])
    with pytest.raises(ValueError, match="n_prompts"):
        E.shared_plan([10, 20, 30], [0, 1], [4, 4])                         # more prompts than requests


def test_argument_checks_need_no_engine(lib):
    from starvector_amd._lib import SvCbRequest, SvSampling

    def err():
        return lib.sv_last_error().decode()
    p, n = C.c_void_p(16), C.c_int32(0)                                     # never dereferenced: the checks come first
    good, bad = (C.c_int32 * 2)(5, 9), (C.c_int32 * 2)(5, 0)
    sp = SvSampling(max_length=32)
    gs = lib.sv_generate_shared
    assert gs(None, None, 2, None, 4, 3, C.byref(sp), None, p, C.byref(n), None) == -22 and "null" in err()
    assert gs(None, p, 2, None, 4, 3, None, None, p, C.byref(n), None) == -22 and "null" in err()
    assert gs(None, p, 0, None, 4, 3, C.byref(sp), None, p, C.byref(n), None) == -22 and "B=0" in err()
    assert gs(None, p, 2, None, 4, 0, C.byref(sp), None, p, C.byref(n), None) == -22 and "n_samples=0" in err()
    assert gs(None, p, 2, None, 0, 3, C.byref(sp), None, p, C.byref(n), None) == -22 and "S0=0" in err()
    assert gs(None, p, 2, bad, 0, 3, C.byref(sp), None, p, C.byref(n), None) == -22 and "length 0 of sequence 1" in err()
    assert gs(None, p, 2, good, 0, 3, C.byref(sp), None, p, C.byref(n), None) == -22 and "null engine" in err()
    assert gs(None, p, 2, None, 4, 3, C.byref(sp), None, p, C.byref(n), None) == -22 and "null engine" in err()
    rq, slots = (SvCbRequest * 3)(), (C.c_int32 * 3)()
    grp = (C.c_int32 * 3)(0, 0, 1)
    ad = lib.sv_cb_admit_shared
    assert ad(None, p, 2, None, 3, grp, rq, slots, None) == -22 and "null" in err()
    assert ad(None, p, 2, good, 3, None, rq, slots, None) == -22 and "null" in err()
    assert ad(None, p, 2, good, 0, grp, rq, slots, None) == -22 and "n=0" in err()
    assert ad(None, p, 2, bad, 3, grp, rq, slots, None) == -22 and "prompt 1: bad prompt length 0" in err()
    assert ad(None, p, 2, good, 3, (C.c_int32 * 3)(0, 2, 1), rq, slots, None) == -22 and "group[1] = 2 outside" in err()
    assert ad(None, p, 2, good, 3, (C.c_int32 * 3)(1, 0, 0), rq, slots, None) == -22 and "group[0] = 1" in err()
    assert ad(None, p, 2, good, 3, (C.c_int32 * 3)(0, 0, 0), rq, slots, None) == -22 and "prompt 1 is referenced by no request" in err()
    assert ad(None, p, 2, good, 3, grp, rq, slots, None) == -22 and "null engine" in err()
    out = (C.c_int32 * 4)()
    assert lib.sv_debug_block_table(None, 0, out, 4) == -22 and lib.sv_debug_free_pages(None, out, out) == -22
    assert lib.sv_debug_shared_plan(good, 2, grp, None, 3, out, out, None) == -22 and "null" in err()


# ---- HipCausalLM.generate(num_return_sequences) -------------------------------------------------------------------------------
class _FakeSharedEngine(_FakeEngine):
    """_FakeEngine that also offers the shared call: it records the prompts it was handed and returns what `generate` returns for
    them repeated (the contract of sv_generate_shared)."""

    def __init__(self):
        super().__init__()
        self.shared_calls = []

    def generate_shared(self, inputs_embeds, max_length, n_samples, **kw):
        self.shared_calls.append((tuple(inputs_embeds.shape[:2]), n_samples))
        out = self.generate(inputs_embeds.repeat_interleave(n_samples, dim=0), max_length, **kw)
        self.calls.pop()
        return out


def _shared_lm():
    lm = _fake_lm()
    object.__setattr__(lm, "_engine", _FakeSharedEngine())
    return lm


def test_num_return_sequences_hands_the_engine_the_unrepeated_prompts():
    torch.manual_seed(0)
    emb = torch.randint(0, 5, (2, 6, 3)).float()
    lm, old = _shared_lm(), _fake_lm()
    out = lm.generate(inputs_embeds=emb, max_length=6 + 5, num_return_sequences=3, do_sample=True, seed=11)
    assert lm._engine.shared_calls == [((2, 6), 3)] and lm._engine.calls == []               # B prompts, not 3 B
    ref = old.generate(inputs_embeds=emb, max_length=6 + 5, num_return_sequences=3, do_sample=True, seed=11)
    assert old._engine.calls == [(6, 6, 5, None)]                                            # without the attribute: repeated, as before
    assert out.shape == (6, 5) and torch.equal(out, ref)
    assert torch.equal(out[0], out[1]) and torch.equal(out[3], out[5]) and not torch.equal(out[0], out[3])      # HF's row order: b * G + j
    # the switch: the old route on an engine that offers the shared call
    lm = _shared_lm()
    off = lm.generate(inputs_embeds=emb, max_length=6 + 5, num_return_sequences=3, do_sample=True, seed=11, share_prompt=False)
    assert lm._engine.shared_calls == [] and lm._engine.calls == [(6, 6, 5, None)] and torch.equal(off, ref)
    # one sample per prompt takes exactly the code it takes now
    lm = _shared_lm()
    lm.generate(inputs_embeds=emb, max_length=6 + 5)
    assert lm._engine.shared_calls == [] and lm._engine.calls == [(2, 6, 5, None)]
    # streaming sees B * G rows; beams with several sequences stay not built
    lm = _shared_lm()

    class _S:
        rows = []

        def put(self, t):
            self.rows.append(int(t.shape[0]))

        def end(self):
            pass
    lm.generate(inputs_embeds=emb, max_length=6 + 5, num_return_sequences=3, streamer=_S())
    assert set(_S.rows) == {6}
    with pytest.raises(NotImplementedError):
        lm.generate(inputs_embeds=emb, max_length=6 + 5, num_return_sequences=3, num_beams=2)


class _FakeGroupEngine(_FakeRaggedEngine):
    """_FakeRaggedEngine with the group admit: records (prompt lengths, group) and admits request i with prompt group[i]."""

    def __init__(self, max_batch=8):
        super().__init__(max_batch)
        self.group_admits = []

    def cb_admit_shared(self, embs, lengths, group, reqs):
        assert lengths is None
        self.group_admits.append((tuple(int(t.shape[0]) for t in embs), tuple(group), tuple(r["seed"] for r in reqs)))
        before = len(self.admits)
        out = self.cb_admit([embs[g] for g in group], reqs)
        del self.admits[before:]
        return out


def test_padded_prompts_with_several_samples_share_one_group_admit():
    torch.manual_seed(0)
    emb = torch.randint(0, 5, (3, 6, 3)).float()
    mask = torch.tensor([[0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1]])
    lm = _ragged_lm()
    object.__setattr__(lm, "_engine", _FakeGroupEngine())
    out = lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 4, num_return_sequences=2, do_sample=True, seed=5)
    (lens, group, seeds), = lm._engine.group_admits
    assert lens == (4, 6, 5) and group == (0, 0, 1, 1, 2, 2) and len(set(seeds)) == 6 and lm._engine.admits == []
    ref_lm = _ragged_lm()                                   # no group admit on this engine: the repeated rows, one ragged admit
    ref = ref_lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 4, num_return_sequences=2, do_sample=True, seed=5)
    assert ref_lm._engine.admits == [(4, 4, 6, 6, 5, 5)] and out.shape == (6, 4) and torch.equal(out, ref)
    off = _ragged_lm()
    object.__setattr__(off, "_engine", _FakeGroupEngine())
    out2 = off.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 4, num_return_sequences=2, do_sample=True, seed=5,
                        share_prompt=False)
    assert off._engine.group_admits == [] and torch.equal(out2, ref)


# ---- the batcher's group submit and vllm.LLM.generate(n) ----------------------------------------------------------------------
class _ScriptedGroupEngine(_ScriptedEngine):
    def __init__(self, max_batch=2):
        super().__init__(max_batch)
        self.groups = []

    def prefill_ragged(self, *a, **k):
        raise AssertionError("never needed")

    def cb_admit(self, emb, reqs):
        if isinstance(emb, (list, tuple)):
            emb = torch.stack(list(emb), 0)
        return super().cb_admit(emb, reqs)

    def cb_admit_shared(self, embs, lengths, group, reqs):
        out = self.cb_admit([embs[g] for g in group], reqs)
        self.groups.append((len(embs), tuple(group), tuple(r["seed"] for r in reqs)))
        return out


def test_vllm_n_samples_are_one_group_with_distinct_seeds():
    llm = _scripted_llm(max_batch=4)
    llm.engine = _ScriptedGroupEngine(4)
    sp = V.SamplingParams(n=4, seed=9, max_tokens=3, temperature=0.7)
    outs = llm.generate(["50"], sp)
    (n_prompts, group, seeds), = llm.engine.groups
    assert n_prompts == 1 and group == (0, 0, 0, 0) and list(seeds) == V.sample_seeds(sp) and len(set(seeds)) == 4
    assert [c.index for c in outs[0].outputs] == [0, 1, 2, 3] and all(c.token_ids == [50, 51, 52] for c in outs[0].outputs)
    # the switch and an engine without the group admit: every sample on its own, the same outputs
    llm2 = _scripted_llm(max_batch=4)
    llm2.engine = _ScriptedGroupEngine(4)
    ref = llm2.generate(["50"], sp, share_prompt=False)
    assert llm2.engine.groups == [] and [c.token_ids for c in ref[0].outputs] == [c.token_ids for c in outs[0].outputs]
    llm3 = _scripted_llm(max_batch=4)
    old = llm3.generate(["50"], sp)
    assert [c.token_ids for c in old[0].outputs] == [c.token_ids for c in outs[0].outputs] and len(llm3.engine.seen) == 4


def test_a_group_larger_than_the_engine_is_admitted_in_parts():
    eng = _ScriptedGroupEngine(max_batch=2)
    bt = ContinuousBatcher(eng, steps_per_poll=2)
    try:
        emb = torch.full((1, 2, 8), 20.0)
        hs = bt.submit_group(emb, [dict(max_new_tokens=3 + j, eos_token_id=-1, stop_any_ids=[], seed=j) for j in range(5)])
        toks = [h.result(20).view(-1).tolist() for h in hs]
        assert toks == [list(range(20, 23 + j)) for j in range(5)]          # G = 5 > max_batch = 2: never waits for five slots
        assert all(n == 1 and len(g) == 2 for n, g, _ in eng.groups)        # the parts of two share among themselves
        assert sorted(r["seed"] for r in eng.seen) == [0, 1, 2, 3, 4]
        with pytest.raises(ValueError):
            bt.submit_group(emb, [])
    finally:
        bt.close()
