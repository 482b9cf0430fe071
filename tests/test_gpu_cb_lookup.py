"""GPU: prompt-lookup drafting in the continuous batch (sv_cb_set_lookup) at engine level.  The contract everywhere: a request's tokens, its
finish and, where asked, its log-prob record are BIT-IDENTICAL to the same request in a continuous batch of the same engine with drafting
off -- whatever the drafts are (the natural lookup, forced right, partly wrong, all wrong), whoever else is in the batch, however the slot
was admitted.  The forced-right runs are the ones that fail when a row does not see the K / V of its siblings."""
import math

import pytest
import torch

from tests.test_gpu_lookup import _case, _restated_counts, _tiny_random
from tests.test_gpu_vllm_sampling import _tiny

pytestmark = pytest.mark.gpu

S1 = dict(do_sample=True, top_k=50, top_p=0.9, temperature=1.0)
S2 = dict(do_sample=True, top_k=0, top_p=0.95, temperature=0.7)
PEN = dict(repetition_penalty=1.3)
MODES = {"greedy": {}, "topk50": S1, "scan": S2, "greedy_pen": PEN, "topk50_pen": {**S1, **PEN}, "scan_pen": {**S2, **PEN}}


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _set(eng, K, forced=None):
    """the drafting setting and the forced drafts of the batch admitted next (no batch is active)"""
    eng.cb_reset()
    if forced is not None or getattr(eng, "_test_forced", False):
        eng.cb_set_lookup_drafts(forced)
        eng._test_forced = forced is not None
    eng.cb_set_lookup(K)


def _read(eng, slots, lps=None):
    """[(tokens, live, counts, record or None)] per slot"""
    live, steps = eng.cb_poll()
    out = []
    for i, s in enumerate(slots):
        rec = eng.cb_read_logprobs(s, 0, steps[s]) if lps and lps[i] is not None else None
        out.append((eng.cb_read(s, 0, steps[s]).tolist(), live[s], eng.cb_lookup_counts(s), rec))
    return out


def _run(eng, embs, reqs, K=0, forced=None, lps=None, step=8, shared=None):
    _set(eng, K, forced)
    if shared is not None:
        slots = eng.cb_admit_shared(embs, None, shared, reqs, logprobs=lps)
    else:
        slots = eng.cb_admit(embs, reqs, logprobs=lps)
    n_calls = 0
    while eng.cb_step(step) > 0:
        n_calls += 1
        assert n_calls < 4096
    out = _read(eng, slots, lps)
    totals = eng.cb_lookup_counts(-1)
    assert [totals[k] for k in ("steps", "drafted", "accepted")] == [sum(o[2][k] for o in out) for k in ("steps", "drafted", "accepted")]
    eng.cb_reset()
    return out


def _same(got, ref, tag):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0] and g[1] == r[1], (tag, i, g[0], r[0])
        c = g[2]
        assert 0 <= c["accepted"] <= c["drafted"] and c["steps"] + c["accepted"] == len(g[0]) - 1, (tag, i, c)
        if r[3] is not None:
            for a, b in zip(g[3], r[3]):
                assert torch.equal(_bits(a), _bits(b)), (tag, i)


# ---- natural drafts on the goldens ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_b3", "tiny_stop", "tiny_minlen", "tiny_v2_b2", "tiny_v2_window"])
def test_natural_drafts_equal_the_plain_batch_on_the_goldens(name):
    """EOS, each request's stop sequence, the min-length hold, a page crossing with RoPE, the window edge"""
    eng, emb, kw, _hf = _case(name)                      # max_batch 32: 4 slots at K = 7
    n_new = kw["max_length"] - emb.shape[1]
    base = dict(max_new_tokens=n_new, eos_token_id=kw["eos_token_id"], pad_token_id=kw["pad_token_id"], stop_ids=kw.get("stop_ids"),
                min_new_tokens=kw.get("min_new_tokens", 0))
    embs = [emb[i] for i in range(emb.shape[0])]
    for mode, sel in MODES.items():
        reqs = [dict(base, seed=1234 + i, **sel) for i in range(len(embs))]
        plain = _run(eng, embs, reqs)
        for K in (1, 3, 7):
            got = _run(eng, embs, reqs, K=K)
            print(f"[{name}/{mode}] K={K}: {[g[2] for g in got]} for {[len(g[0]) for g in got]} columns")
            _same(got, plain, f"{name} {mode} K={K}")
    eng.close()


# ---- forced drafts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 7])
def test_forced_drafts_right_partly_wrong_and_all_wrong(K):
    eng, emb, cfg = _tiny_random(16, 128, 1)
    n = 45
    for mode in ("greedy", "topk50_pen"):
        req = dict(max_new_tokens=n, eos_token_id=-1, seed=77, **MODES[mode])
        plain = _run(eng, [emb[0]], [req])
        stream = plain[0][0]
        assert len(stream) == n and len(set(stream)) > 4
        got = _run(eng, [emb[0]], [req], K=K, forced=[stream])
        _same(got, plain, f"{mode} all right: a row did not see its siblings' K / V")
        c = got[0][2]
        assert c["steps"] == math.ceil((n - 1) / (K + 1)) and c["accepted"] == c["drafted"] == n - 1 - c["steps"], c
        for m in (2, 3, 5):
            bad = [(t + 1) % cfg.vocab if i % m == 0 else t for i, t in enumerate(stream)]
            got = _run(eng, [emb[0]], [req], K=K, forced=[bad])
            _same(got, plain, f"{mode} every {m}-th draft wrong")
            c = got[0][2]
            assert (c["steps"], c["drafted"], c["accepted"]) == _restated_counts(stream, K, bad), (mode, m, c)
        got = _run(eng, [emb[0]], [req], K=K, forced=[[(t + 1) % cfg.vocab for t in stream]])
        _same(got, plain, f"{mode} all wrong")
        assert got[0][2]["steps"] == n - 1 and got[0][2]["accepted"] == 0
        _same(_run(eng, [emb[0]], [req], K=K), plain, f"{mode} natural after forced")
    eng.close()


# ---- a full batch across the row-tile boundary ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_dtype", ["bf16", "fp8_e4m3"])
def test_full_batch_of_32_and_64_rows(weight_dtype):
    eng, emb, cfg = _tiny_random(64, 256, 8, weight_dtype=weight_dtype)
    n = 70                                               # across a KV page
    for mode in ("greedy", "topk50", "scan_pen"):
        for B in (4, 8):                                 # K = 7: 32 rows, one row tile; 64 rows, two
            embs = [emb[i] for i in range(B)]
            reqs = [dict(max_new_tokens=n, eos_token_id=-1, seed=900 + i, **MODES[mode]) for i in range(B)]
            plain = _run(eng, embs, reqs)
            got = _run(eng, embs, reqs, K=7)
            _same(got, plain, f"{weight_dtype} {mode} B={B} natural")
            got = _run(eng, embs, reqs, K=7, forced=[p[0] for p in plain])      # each slot's own stream: the accepted rows of both tiles feed the cache
            _same(got, plain, f"{weight_dtype} {mode} B={B} forced")
            assert all(g[2]["steps"] == math.ceil((n - 1) / 8) for g in got), [g[2] for g in got]
    eng.close()


@pytest.fixture(scope="module")
def tiny32():
    cfg, w, eng, emb, prompt = _tiny(max_batch=32, max_seq_len=128)
    yield cfg, eng, emb, prompt
    eng.close()


# ---- join and leave -------------------------------------------------------------------------------------------------------------------------
def _staggered(eng, emb, reqs, K, forced=None):
    """three requests admitted at different steps while the others are mid-run; the second one released and its slot reused by a fourth"""
    _set(eng, K, forced)
    a = eng.cb_admit([emb[0]], reqs[:1])[0]
    eng.cb_step(2)
    b = eng.cb_admit([emb[1]], reqs[1:2])[0]
    eng.cb_step(1)
    c = eng.cb_admit([emb[2][:-1], emb[3]], reqs[2:4])               # a ragged admit: prompts of two lengths
    while eng.cb_poll()[0][b]:
        eng.cb_step(3)
    first = _read(eng, [b])[0]
    eng.cb_release(b)
    d = eng.cb_admit([emb[3]], reqs[4:5])[0]
    assert d == b and eng.cb_lookup_counts(d) == dict(steps=0, drafted=0, accepted=0)
    while eng.cb_step(8) > 0:
        pass
    out = _read(eng, [a] + c + [d])
    eng.cb_reset()
    return out[:1] + [first] + out[1:]


@pytest.mark.parametrize("K", [3, 7])
def test_requests_join_and_leave_mid_run(tiny32, K):
    cfg, eng, emb, prompt = tiny32
    reqs = [dict(max_new_tokens=40, eos_token_id=-1), dict(max_new_tokens=9, eos_token_id=-1, seed=3, **S1),
            dict(max_new_tokens=30, eos_token_id=-1, seed=4, **S2, **PEN), dict(max_new_tokens=25, eos_token_id=-1, **PEN),
            dict(max_new_tokens=33, eos_token_id=-1, seed=5, **S1)]
    plain = _staggered(eng, emb, reqs, 0)
    assert [len(p[0]) for p in plain] == [40, 9, 30, 25, 33]
    _same(_staggered(eng, emb, reqs, K), plain, f"K={K} natural")
    # forced by SLOT: slot 1 is held by request 1 and then by request 4 -- right for the first, wrong for the second (none of its tokens may come
    # from the predecessor's stream)
    forced = [(plain[i][0] + [0] * 40)[:40] for i in (0, 1, 2, 3)]
    _same(_staggered(eng, emb, reqs, K, forced), plain, f"K={K} forced")


def test_group_admit_forks_the_tail_page_into_every_slots_rows(tiny32):
    cfg, eng, emb, prompt = tiny32
    assert emb.shape[1] % 64 != 0                        # the prompt's tail page is partly filled: the fork copies it by block-table ROW
    reqs = [dict(max_new_tokens=70, eos_token_id=-1, seed=50 + j, **S1) for j in range(3)] + [dict(max_new_tokens=20, eos_token_id=-1)]
    embs, group = [emb[1], emb[2]], [0, 0, 0, 1]
    plain = _run(eng, embs, reqs, shared=group)
    assert len({tuple(p[0]) for p in plain[:3]}) == 3
    for K in (3, 7):
        _same(_run(eng, embs, reqs, K=K, shared=group), plain, f"K={K} natural")
        _same(_run(eng, embs, reqs, K=K, shared=group, forced=[(p[0] + [0] * 70)[:70] for p in plain]), plain, f"K={K} forced")


def test_one_request_too_many_is_busy_and_nothing_is_admitted(tiny32):
    from starvector_amd._lib import StarVectorBusy
    cfg, eng, emb, prompt = tiny32
    K = 7
    _set(eng, K)
    cap = 32 // (K + 1)
    req = dict(max_new_tokens=6, eos_token_id=-1)
    slots = [eng.cb_admit([emb[i % 4]], [req])[0] for i in range(cap)]
    assert slots == list(range(cap))
    before = eng.cb_poll()
    with pytest.raises(StarVectorBusy):
        eng.cb_admit([emb[0]], [req])
    assert eng.cb_poll() == before
    eng.cb_reset()
    with pytest.raises(StarVectorBusy):                  # in one call as well
        eng.cb_admit([emb[i % 4] for i in range(cap + 1)], [req] * (cap + 1))
    assert eng.cb_poll() == ([0] * 32, [0] * 32)
    eng.cb_reset()


# ---- ends inside an accepted run ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 7])
def test_ends_inside_an_accepted_run(tiny32, K):
    cfg, eng, emb, prompt = tiny32
    free = _run(eng, [emb[0]], [dict(max_new_tokens=30, eos_token_id=-1)])[0][0]
    col = next(c for c in range(2, 30) if c % (K + 1) not in (0, 1) and free[c] not in free[:c] and free[c - 1] not in free[:c - 1])
    cases = [dict(max_new_tokens=b, eos_token_id=-1) for b in (1, 2, K + 1, K + 2)]
    unused = next(v for v in range(cfg.vocab) if v not in free)
    cases += [dict(max_new_tokens=30, eos_token_id=free[col]),                                  # EOS at a drafted column
              dict(max_new_tokens=30, eos_token_id=free[col], min_new_tokens=col + 2),          # held past it
              dict(max_new_tokens=30, eos_token_id=-1, stop_ids=[free[col - 1], free[col]]),     # a 2-id stop completed by a draft row
              dict(max_new_tokens=30, eos_token_id=-1, semantics="vllm", stop_any_ids=[unused, free[col]])]
    lengths = []
    for i, req in enumerate(cases):
        plain = _run(eng, [emb[0]], [req])
        n = len(plain[0][0])
        lengths.append(n)
        got = _run(eng, [emb[0]], [req], K=K, forced=[(plain[0][0] + free)[:30]])
        _same(got, plain, f"K={K} case {i}")
        assert got[0][2]["steps"] == math.ceil((n - 1) / (K + 1)), (i, got[0][2])             # every draft right: full runs, the end inside the last
    assert lengths[:4] == [1, 2, K + 1, K + 2] and lengths[4] == lengths[6] == lengths[7] == col + 1 and lengths[5] > col + 1


# ---- vLLM semantics -------------------------------------------------------------------------------------------------------------------------
def test_vllm_semantics(tiny32):
    cfg, eng, emb, prompt = tiny32
    reqs = [dict(semantics="vllm", max_new_tokens=40, eos_token_id=-1, prompt_ids=prompt, repetition_penalty=1.3, frequency_penalty=0.6,
                 presence_penalty=0.4, logit_bias={300: 0.05, 5: 0.5}),
            dict(semantics="vllm", max_new_tokens=36, eos_token_id=-1, do_sample=True, temperature=0.9, top_k=8, top_p=0.8, min_p=0.02, seed=77,
                 prompt_ids=prompt, repetition_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.1),
            dict(semantics="vllm", max_new_tokens=30, eos_token_id=0, stop_any_ids=[3], min_new_tokens=12, do_sample=True, temperature=1.2, seed=1077),
            dict(max_new_tokens=28, eos_token_id=-1, **PEN)]                                    # an HF slot beside them
    embs = [emb[i] for i in range(4)]
    plain = _run(eng, embs, reqs)
    for K in (3, 7):
        _same(_run(eng, embs, reqs, K=K), plain, f"K={K} natural")
        _same(_run(eng, embs, reqs, K=K, forced=[(p[0] + [0] * 40)[:40] for p in plain]), plain, f"K={K} forced")


# ---- records --------------------------------------------------------------------------------------------------------------------------------
def test_logprob_records_are_the_plain_batchs_bit_for_bit(tiny32):
    cfg, eng, emb, prompt = tiny32
    reqs = [dict(max_new_tokens=24, eos_token_id=-1, repetition_penalty=1.3),
            dict(max_new_tokens=24, eos_token_id=-1, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.2, seed=5),
            dict(semantics="vllm", max_new_tokens=20, eos_token_id=-1, prompt_ids=prompt, repetition_penalty=1.3, frequency_penalty=0.6, logit_bias={5: 0.5}),
            dict(semantics="vllm", max_new_tokens=18, eos_token_id=-1, do_sample=True, temperature=0.9, top_k=8, top_p=0.8, min_p=0.02, seed=9)]
    embs = [emb[i] for i in range(4)]
    for lps in ([dict(k=0, source="raw"), dict(k=5, source="processed"), dict(k=5), dict(k=0)],
                [dict(k=5, source="raw"), dict(k=0, source="processed"), None, dict(k=5)]):
        plain = _run(eng, embs, reqs, lps=lps)
        assert [t for t, *_ in plain] == [t for t, *_ in _run(eng, embs, reqs)]
        for K in (3, 7):
            _same(_run(eng, embs, reqs, K=K, lps=lps), plain, f"K={K} natural")
            _same(_run(eng, embs, reqs, K=K, lps=lps, forced=[(p[0] + [0] * 24)[:24] for p in plain]), plain, f"K={K} forced")


# ---- mode and graphs ------------------------------------------------------------------------------------------------------------------------
def test_mode_switches_and_graphs(tiny32, monkeypatch):
    cfg, eng, emb, prompt = tiny32
    reqs = [dict(max_new_tokens=40, eos_token_id=-1), dict(max_new_tokens=37, eos_token_id=-1, seed=3, **S1, **PEN)]
    embs = [emb[0], emb[1]]
    plain = _run(eng, embs, reqs)
    solo = eng.generate(emb[0:1].contiguous(), max_length=emb.shape[1] + 40, eos_token_id=-1)[0].tolist()
    assert plain[0][0] == solo
    for K in (3, 7, 0, 3):                               # switching between batches is right each time
        if K:
            _same(_run(eng, embs, reqs, K=K), plain, f"K={K}")
            continue
        got = _run(eng, embs, reqs)                      # off again: today's tokens, no counters, and sv_generate works
        assert [g[0] for g in got] == [p[0] for p in plain] and all(g[2] == dict(steps=0, drafted=0, accepted=0) for g in got)
        assert eng.generate(emb[0:1].contiguous(), max_length=emb.shape[1] + 40, eos_token_id=-1)[0].tolist() == solo
    _same(_run(eng, embs, reqs, K=3, step=1), plain, "one step per call")
    monkeypatch.setenv("SV_NO_GRAPH", "1")
    _same(_run(eng, embs, reqs, K=3), plain, "plain launches")
    _same(_run(eng, embs, reqs, K=3, step=1), plain, "plain launches, one step per call")
    monkeypatch.delenv("SV_NO_GRAPH")
    # the setting changes only while no batch is active, and sv_generate stays refused while slots are live
    _set(eng, 3)
    eng.cb_admit([emb[0]], reqs[:1])
    with pytest.raises(RuntimeError, match="a continuous batch is active"):
        eng.cb_set_lookup(7)
    with pytest.raises(RuntimeError, match="a continuous batch is active"):
        eng.cb_set_lookup_drafts([[1, 2, 3]])
    with pytest.raises(RuntimeError, match="continuous batch"):
        eng.generate(emb[0:1].contiguous(), max_length=emb.shape[1] + 4, eos_token_id=-1)
    eng.cb_reset()
    small = _tiny(max_batch=8)[2]
    try:
        with pytest.raises(NotImplementedError, match="exceed engine max_batch"):
            small.cb_set_lookup(15)                      # 8 / 16 < 1 slot
        small.cb_set_lookup(7)                           # one slot of 8 rows
    finally:
        small.close()
    eng.cb_set_lookup(0)


# ---- the Python layers ----------------------------------------------------------------------------------------------------------------------
def test_the_batcher_returns_the_same_tokens_and_streams_every_column_once(tiny32):
    from starvector_amd.batching import ContinuousBatcher
    cfg, eng, emb, prompt = tiny32
    params = [dict(max_new_tokens=40, eos_token_id=-1), dict(max_new_tokens=33, eos_token_id=-1, seed=3, **S1, **PEN),
              dict(max_new_tokens=21, eos_token_id=-1, seed=4, **S2), dict(max_new_tokens=1, eos_token_id=-1)]
    outs = {}
    for K in (0, 3):
        eng.cb_reset()
        eng.cb_set_lookup(0)
        b = ContinuousBatcher(eng, steps_per_poll=2, **(dict(prompt_lookup_num_tokens=K) if K else {}))
        assert b.slots == 32 // (K + 1)
        seen = [[] for _ in params]
        hs = [b.submit(emb[i:i + 1].contiguous(), p, lambda t, first, i=i: seen[i].append((first, t.tolist()))) for i, p in enumerate(params)]
        outs[K] = [h.result(timeout=60)[0].tolist() for h in hs]
        for i, chunks in enumerate(seen):                # every column exactly once, in order
            flat = [x for _, c in chunks for x in c]
            assert flat == outs[K][i] and [f for f, _ in chunks] == [sum(len(c) for _, c in chunks[:j]) for j in range(len(chunks))], (K, i)
        c = b.lookup_counts()
        assert (c["steps"] > 0 and 0 <= c["accepted"] <= c["drafted"]) if K else c == dict(steps=0, drafted=0, accepted=0)
        b.close()
    assert outs[3] == outs[0] and [len(t) for t in outs[0]] == [40, 33, 21, 1]
    eng.cb_reset()
    eng.cb_set_lookup(0)


def test_llm_with_vllms_ngram_arguments_returns_what_it_returns_without(tmp_path):
    import numpy as np
    from PIL import Image
    from oracle import starvector_oracle as O
    from starvector_amd import vllm as VL
    from tests.ckpt_util import write_reference_checkpoint
    cfg = O.OracleConfig.tiny()
    path = str(tmp_path / "ckpt")
    write_reference_checkpoint(path, cfg, O.make_weights(cfg, seed=21))
    rng = np.random.default_rng(3)
    images = [Image.fromarray(rng.integers(0, 255, (40 + 7 * i, 48, 3), dtype=np.uint8)) for i in range(3)]
    inputs = [{"prompt": "<image-start>", "multi_modal_data": {"image": im}} for im in images]
    sps = [VL.SamplingParams(n=2, temperature=0.8, top_p=0.95, min_p=0.05, seed=11, max_tokens=30),
           VL.SamplingParams(n=1, temperature=0.0, max_tokens=40, repetition_penalty=1.3),
           VL.SamplingParams(n=2, temperature=1.0, top_k=40, frequency_penalty=0.5, presence_penalty=0.2, seed=12, max_tokens=25)]
    got = {}
    for name, kw in (("plain", {}), ("ngram", dict(speculative_model="[ngram]", num_speculative_tokens=3, ngram_prompt_lookup_max=4))):
        llm = VL.LLM(model=path, max_num_seqs=16, max_model_len=min(96, cfg.n_positions), trust_remote_code=True, byte_tokenizer_fallback=True, **kw)
        try:
            outs = llm.generate(inputs, sps, use_tqdm=False, logprobs=2 if name == "ngram" else None)
            got[name] = [(c.token_ids, c.finish_reason) for ro in outs for c in ro.outputs]
            if name == "ngram":
                assert all(len(c.logprobs) == len(c.token_ids) for ro in outs for c in ro.outputs)
        finally:
            llm.engine.cb_reset()
            llm.close()
    assert got["ngram"] == got["plain"] and len(got["plain"]) == 5
