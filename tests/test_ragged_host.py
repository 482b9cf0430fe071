"""CPU: the ragged prompt pass's host side -- the new C ABI symbols and their argument checks, the dispatch rule as
sv_debug_ragged_plan states it, and the mirror's route (one ragged call for a padded batch where the engine offers it, the
length-group route where it does not)."""
import ctypes as C

import pytest
import torch

from starvector_amd import _lib, engine as E
from starvector_amd.model import HipCausalLM, StoppingCriteriaSub
from tests.test_host_logic import _FakeSlotEngine, _fake_lm, _slot_lm

LENS = [5, 31, 255, 256, 257, 259, 260, 515, 700]
SHAPES_1B = {"c_attn": (2048 + 2 * 128, 2048, "none"), "c_proj": (2048, 2048, "none"), "c_fc": (8192, 2048, "gelu_tanh"),
             "down": (2048, 8192, "none")}
SHAPES_8B = {"c_attn": (4608 + 2 * 4 * 128, 4608, "none"), "c_proj": (4608, 4608, "none"), "c_fc": (18432, 4608, "gelu_tanh"),
             "down": (4608, 18432, "none")}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_ragged_symbols_are_exported_bound_and_validate_before_any_device_work(lib):
    from starvector_amd._lib import SvCbRequest, SvSampling
    for name, n_args in (("sv_prefill_ragged", 6), ("sv_generate_ragged", 9), ("sv_cb_admit_ragged", 7), ("sv_debug_ragged_plan", 10),
                         ("sv_debug_prompt_passes", 2)):
        assert hasattr(lib, name) and len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert lib.sv_abi_version() == 9                                # append-only additions: an old binding keeps working

    def err():
        return lib.sv_last_error().decode()
    p = C.c_void_p(16)                                              # never dereferenced: the checks come first
    n = C.c_int32(0)
    good, bad = (C.c_int32 * 3)(5, 9, 2), (C.c_int32 * 3)(5, 0, 2)
    sp, rq, slots = SvSampling(max_length=32), (SvCbRequest * 3)(), (C.c_int32 * 3)()
    # null pointers
    assert lib.sv_prefill_ragged(None, None, 3, good, p, None) == -22 and "null" in err()
    assert lib.sv_prefill_ragged(None, p, 3, None, p, None) == -22 and "null" in err()
    assert lib.sv_generate_ragged(None, p, 3, good, None, None, p, C.byref(n), None) == -22 and "null" in err()
    assert lib.sv_cb_admit_ragged(None, p, 3, None, rq, slots, None) == -22 and "null" in err()
    # B out of range, a length < 1
    assert lib.sv_prefill_ragged(None, p, 0, good, p, None) == -22 and "B=0" in err()
    assert lib.sv_prefill_ragged(None, p, 3, bad, p, None) == -22 and "length 0 of sequence 1" in err()
    assert lib.sv_generate_ragged(None, p, 0, good, C.byref(sp), None, p, C.byref(n), None) == -22 and "B=0" in err()
    assert lib.sv_generate_ragged(None, p, 3, bad, C.byref(sp), None, p, C.byref(n), None) == -22 and "length 0 of sequence 1" in err()
    assert lib.sv_cb_admit_ragged(None, p, 0, good, rq, slots, None) == -22
    assert lib.sv_cb_admit_ragged(None, p, 3, bad, rq, slots, None) == -22 and "request 1" in err()
    # well-formed arguments without an engine: still an error, never a device touch
    assert lib.sv_prefill_ragged(None, p, 3, good, p, None) == -22 and "null engine" in err()
    assert lib.sv_generate_ragged(None, p, 3, good, C.byref(sp), None, p, C.byref(n), None) == -22 and "null engine" in err()
    assert lib.sv_cb_admit_ragged(None, p, 3, good, rq, slots, None) == -22 and "null engine" in err()
    out4, buf = (C.c_int32 * 4)(), (C.c_int32 * 9)()
    assert lib.sv_debug_ragged_plan(good, 3, 2048, 2048, 0, 64, buf, buf, 9, out4) == -22 and "q_tile" in err()
    assert lib.sv_debug_ragged_plan(good, 3, 2048, 2048, 0, 32, buf, buf, 8, out4) == -22 and "capacity" in err()
    assert lib.sv_debug_ragged_plan(bad, 3, 2048, 2048, 0, 32, buf, buf, 9, out4) == -22
    assert lib.sv_debug_prompt_passes(None, None) == -22


@pytest.mark.parametrize("shapes,q_tile", [(SHAPES_1B, 32), (SHAPES_8B, 128)])
def test_ragged_plan_lists_exactly_the_rows_the_solo_runs_send_to_the_split_k_remainder_kernel(shapes, q_tile):
    """The rule, restated: row j of a sequence of S rows takes the split-K remainder kernel exactly when
    sv_debug_gemm_seq_form(S, N, K, act) holds and j >= S - S % 256 (S > 256, S % 256 in 1..3)."""
    for order in (LENS, LENS[::-1], LENS[3:] + LENS[:3]):
        for name, (N, K, act) in shapes.items():
            want_rows, want_last, r0 = [], [], 0
            for b, S in enumerate(order):
                r = S % 256
                if S > 256 and 1 <= r <= 3 and E.gemm_seq_form(S, N, K, act):
                    want_rows += list(range(r0 + S - r, r0 + S))
                    want_last.append(b)
                r0 += S
            plan = E.ragged_plan(order, N, K, act, q_tile)
            assert plan["rows"] == want_rows and plan["last"] == want_last, (name, order, plan)
            assert plan["attn_blocks"] == sum((S + q_tile - 1) // q_tile for S in order)       # no B x max_tiles grid: only real tiles
            assert plan["kv_blocks"] == sum((S + 31) // 32 for S in order)
    # the lengths reach both answers at the 1B shapes (a rule that never fires would pass the comparison above trivially)
    if shapes is SHAPES_1B:
        assert E.ragged_plan(LENS, *SHAPES_1B["down"])["rows"] and not E.ragged_plan(LENS, *SHAPES_1B["c_attn"])["rows"]
        assert E.ragged_plan([5, 31, 255, 256, 260, 700], *SHAPES_1B["down"])["rows"] == []


class _FakeRaggedEngine(_FakeSlotEngine):
    """_FakeSlotEngine that also offers the ragged entry points: cb_admit takes a list of per-request embeddings, generate_ragged a
    list of prompts; the per-row 'model' is the same (tokens from the row's real prompt only)."""

    def __init__(self, max_batch=8):
        super().__init__(max_batch)
        self.ragged_calls = []

    def prefill_ragged(self, embeds, lengths=None):
        raise AssertionError("the mirror never needs the bare prompt pass")

    def cb_admit(self, emb, reqs):
        if not isinstance(emb, (list, tuple)):
            return super().cb_admit(emb, reqs)
        self.admits.append(tuple(int(t.shape[0]) for t in emb))
        out = []
        for t, r in zip(emb, reqs):
            before = len(self.admits)
            out += super().cb_admit(t[None], [r])
            del self.admits[before:]
        return out

    def cb_release(self, s):
        self.slots.pop(s, None)

    def generate_ragged(self, embeds, max_length, lengths=None, stop_ids=None, pad_token_id=0, **kw):
        lens = [int(t.shape[0]) for t in embeds]
        budget = max_length - max(lens)
        self.ragged_calls.append((tuple(lens), budget, kw.get("num_beams")))
        rows = [_FakeSlotEngine.generate(self, t[None], t.shape[0] + budget)[0] for t in embeds]
        self.calls.clear()
        toks = torch.stack(rows, 0)
        if stop_ids:
            r0 = toks[0].tolist()
            for t in range(len(stop_ids) - 1, budget):
                if r0[t + 1 - len(stop_ids):t + 1] == list(stop_ids):
                    return toks[:, :t + 1]
        return toks


def _ragged_lm():
    lm = HipCausalLM.__new__(HipCausalLM)
    torch.nn.Module.__init__(lm)
    object.__setattr__(lm, "_engine", _FakeRaggedEngine())
    lm.eos_token_id, lm.pad_token_id, lm.seed = 0, 99, 0
    return lm


def test_padded_batch_is_one_ragged_call_where_the_engine_offers_it():
    torch.manual_seed(0)
    emb = torch.randint(0, 5, (4, 6, 3)).float()
    masks = {"left": torch.tensor([[0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1]]),
             "right": torch.tensor([[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 0]])}
    mask = masks["left"]
    lm = _ragged_lm()
    out = lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 7)
    assert out.shape == (4, 7) and lm._engine.calls == [] and lm._engine.ragged_calls == []
    assert lm._engine.admits == [(4, 6, 4, 5)]                          # ONE prompt pass, every row with its real length, in row order
    for b in range(4):                                                  # the budget counts from the padded length: 7 new tokens per row
        solo = _fake_lm().generate(inputs_embeds=emb[b:b + 1, mask[b].bool()], max_length=int(mask[b].sum()) + 7)
        assert torch.equal(solo[0], out[b])
    assert lm._engine.slots == {}
    stop = out[0, 2:4].tolist()
    cut = lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 7, stopping_criteria=[StoppingCriteriaSub(stops=[stop])])
    assert cut.shape == (4, 4) and torch.equal(cut, out[:, :4])         # row 0's stop cuts every row
    # beam search: one ragged generate call, budget from the padded length, row-0 stop handed to the engine
    lm = _ragged_lm()
    beams = lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 7, num_beams=2)
    assert lm._engine.ragged_calls == [((4, 6, 4, 5), 7, 2)] and lm._engine.admits == [] and beams.shape == (4, 7)
    assert torch.equal(beams, out)                                      # (the fake 'model' ignores the beams: the rows are the greedy rows)
    cut = lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 7, num_beams=2, stopping_criteria=[StoppingCriteriaSub(stops=[stop])])
    assert torch.equal(cut, out[:, :4])
    # eos ends a row early: the output is padded like HF's
    lm = _ragged_lm()
    eos = int(out[1, 2])
    padded = lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 7, eos_token_id=eos)
    assert padded[1, :3].tolist() == out[1, :3].tolist() and padded[1, 3:].tolist() == [99] * (padded.shape[1] - 3)
    # with a padded mask the per-step outputs keep raising
    with pytest.raises(NotImplementedError):
        lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=13, return_dict_in_generate=True, output_scores=True)
    # an engine without the ragged entry points keeps the length-group route
    old = _slot_lm()
    ref = old.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 7)
    assert sorted(old._engine.admits) == [(1, 5), (1, 6), (2, 4)] and torch.equal(ref, out)
    old = _fake_lm()
    ref = old.generate(inputs_embeds=emb, attention_mask=mask, max_length=6 + 7, num_beams=2)
    assert sorted(c[:2] for c in old._engine.calls) == [(1, 5), (1, 6), (2, 4)] and torch.equal(ref, out)
    # right padding: the same rows
    lm = _ragged_lm()
    emb_r = torch.zeros_like(emb)
    for b in range(4):
        n = int(mask[b].sum())
        emb_r[b, :n] = emb[b, mask[b].bool()]
    assert torch.equal(lm.generate(inputs_embeds=emb_r, attention_mask=masks["right"], max_length=6 + 7), out)
    assert lm._engine.admits == [(4, 6, 4, 5)]


def test_batcher_admits_waiting_requests_of_different_lengths_in_one_pass():
    from starvector_amd.batching import ContinuousBatcher
    eng = _FakeRaggedEngine()
    bt = ContinuousBatcher(eng, steps_per_poll=4)
    try:
        import threading
        embs = [torch.full((1, n, 3), float(n)) for n in (3, 5, 4)]
        params = dict(max_new_tokens=6, eos_token_id=-1)
        gate = threading.Event()
        orig = eng.cb_step

        def held(n):                                                     # the first request decodes until the other two are queued
            gate.wait(5)
            return orig(n)
        eng.cb_step = held
        res = [None] * 3

        def run(i):
            res[i] = bt.generate(embs[i], dict(params))
        ts = [threading.Thread(target=run, args=(i,)) for i in range(3)]
        ts[0].start()
        while not eng.admits:
            pass
        ts[1].start(); ts[2].start()
        import time
        for _ in range(500):
            with bt._lock:
                if len(bt._pending) == 2:
                    break
            time.sleep(0.01)
        gate.set()
        for t in ts:
            t.join(20)
        assert eng.admits[0] == (3,) and sorted(eng.admits[1]) == [4, 5] and len(eng.admits) == 2      # the two waiting requests: ONE admit
        for i, e in enumerate(embs):
            solo = _fake_lm().generate(inputs_embeds=e, max_length=e.shape[1] + 6, eos_token_id=-1)
            assert torch.equal(res[i].view(-1), solo[0])
    finally:
        bt.close()
