"""-m gpu: per-request log-probs, top-k lists and token rank on the continuous batch (sv_cb_admit_logprobs / sv_cb_read_logprobs; sampling.hip
cb_step_kernel<true>, cb_record).  The reference is the float64 restatement of tests/test_gpu_token_topk.py over the row each slot's selection saw:
the raw row for source 0, the processed row -- HF's processors (below) or vLLM's (`_processed`), and for a sampling slot the kept set (`_kept`) --
for source 1.  Ids and ranks are exact; log-probs lie within `_tol`, 4 x torch fp32's own deviation from float64 on the same rows.  An HF slot's
record equals its solo sv_generate_topk output bit for bit."""
import numpy as np
import pytest
import torch

import starvector_amd.engine as E
from oracle import starvector_oracle as O
from starvector_amd import vllm as VL
from tests.gpu_util import dev
from tests.test_gpu_token_topk import _assert_distinct_head, _check_lists, _ref_lists, _ref_rank, _tol
from tests.test_gpu_vllm_sampling import _kept, _processed, _tiny

pytestmark = pytest.mark.gpu
NEG = float("-inf")
SLACK = 1e-4


class _Margin(AssertionError):
    """A reference row that does not decide its own answer with room to spare (a tie, a token on a threshold): pick another seed."""


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _hf_processed(l, r, hist):
    """fp32 logits row after the HF processors of a slot: RepetitionPenaltyLogitsProcessor over the generated ids, MinLength's hold of EOS."""
    l = l.clone().float()
    pen = float(r.get("repetition_penalty", 1.0) or 1.0)
    if hist and pen != 1.0:
        seen = torch.zeros(l.numel(), dtype=torch.bool)
        seen[torch.tensor(list(hist))] = True
        l = torch.where(seen, torch.where(l < 0, l * pen, l / pen), l)
    eos = r.get("eos_token_id", 0)
    if len(hist) < r.get("min_new_tokens", 0) and eos >= 0:
        l[eos] = NEG
    return l


def _reference(raw, req, lp, hist):
    """(keys, x32) of one slot at one step: what the list is ordered by and what is normalised, both fp32 [V], removed ids at -inf."""
    raw = raw.float().cpu()
    vl = req.get("semantics") == "vllm"
    sample = bool(req.get("do_sample"))
    T = float(req.get("temperature", 1.0)) if sample else 1.0
    source = lp.get("source") or ("processed" if vl else "raw")
    if source == "raw":
        return raw, raw / torch.full_like(raw, T)                                   # fp32 division, like the kernel's
    proc = _processed(raw, req, hist) if vl else _hf_processed(raw, req, hist)
    if not sample:
        return proc, proc
    args = (proc, T, int(req.get("top_k", 0) or 0), float(req.get("top_p", 1.0)), float(req.get("min_p", 0.0) or 0.0))
    keep = _kept(*args)
    # the kept set is decided with room on both sides of every threshold: otherwise pick another seed
    if not (torch.equal(keep, _kept(*args, slack=SLACK)) and torch.equal(keep, _kept(*args, slack=-SLACK))):
        raise _Margin("a token sits on a threshold: pick another seed")
    # every filter is a threshold on the value, so the kept ids are the best ones: a removed id as good as a kept one is a tie across the
    # boundary, which `_kept` (a sort) and the kernel (a threshold: equal values stay together) are both free to split their own way
    gone = ~keep & torch.isfinite(proc)
    if bool(gone.any()) and not float(proc[gone].max()) < float(proc[keep].min()):
        raise _Margin("equal values on both sides of the kept set's boundary: pick another seed")
    ninf = torch.full_like(proc, NEG)
    return torch.where(keep, proc, ninf), torch.where(keep, proc / torch.full_like(proc, T), ninf)


def _assert_head_decided(raw, keys, untouched, k):
    """The engine's rows hold bf16 values (the lm_head's output), so equal logits among the best few of 516 are the rule, not a seed to avoid.
    The margin of `_assert_distinct_head` -- the first k + 1 values differ, so values alone decide the order -- is asked of every adjacent pair
    except two ids whose RAW logits are equal and that no processor touches (no bias, not held, never seen, count 0): their processed values
    are the raw ones on any arithmetic, the tie is exact on the device as well, and ascending id decides it on both sides."""
    order = torch.sort(keys, descending=True, stable=True).indices[: k + 1].tolist()
    for a, b in zip(order, order[1:]):
        if not (float(keys[a]) > float(keys[b]) or (float(raw[a]) == float(raw[b]) and untouched[a] and untouched[b])):
            raise _Margin(f"ids {a} / {b}: a tie that a processor touched among the first k + 1 values: pick another seed")


def _compare(name, items):
    """items: dicts with keys / x32 (the reference row), k, tok and the record's column (lp, rank, ids [k], lps [k]).  One tolerance for the call."""
    refs, r64, t32s = [], [], []
    for it in items:
        keys, x32 = it["keys"][None], it["x32"][None]
        ref_ids, ref_lps, n, ref64, t32 = _ref_lists(keys, x32, max(it["k"], 1))
        head = max(0, min(it["k"], int(n[0]) - 1))                                  # over the values that enter: the removed ids are all -inf
        if "raw" in it:
            _assert_head_decided(it["raw"], it["keys"], it["untouched"], head)
        else:
            _assert_distinct_head(keys, head)
        refs.append((ref_ids, ref_lps, ref64))
        r64.append(ref64)
        t32s.append(t32)
    tol = _tol(torch.cat(r64), torch.cat(t32s))
    for i, (it, (ref_ids, ref_lps, ref64)) in enumerate(zip(items, refs)):
        k, tok, tag = it["k"], int(it["tok"]), f"{name}[{i}]"
        ids, lps = it["ids"].cpu()[:k], it["lps"].cpu()[:k]
        if k > 0:
            _check_lists(tag, ids[None], lps[None], ref_ids, ref_lps, tol)
        want_rank = int(_ref_rank(it["keys"][None], torch.tensor([tok]))[0])
        assert int(it["rank"]) == want_rank, (tag, int(it["rank"]), want_rank)
        err = abs(float(it["lp"]) - float(ref64[0, tok]))
        print(f"[{tag}] token log-prob |kernel - f64| {err:.3e} (allowed {tol:.3e})")
        assert err <= tol, tag
        hit = (ids.long() == tok).nonzero().flatten()
        assert hit.numel() == (1 if k > 0 and tok in ref_ids[0].tolist() else 0), tag
        if hit.numel():                                                             # the slot of the emitted id: the token's log-prob, bit for bit
            assert torch.equal(_bits(lps[hit]), _bits(torch.tensor([float(it["lp"])], dtype=torch.float32))), tag


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------------
def _op_case(V):
    g = torch.Generator().manual_seed(4100 + V)
    lg = 2.0 * torch.randn(8, V, generator=g)
    lg[6] = float("nan")
    top = lg.topk(5, -1).indices.tolist()
    other = [int(x) for x in torch.randint(0, V, (8,), generator=g)]
    tk = 4 if V == 7 else 20
    base = dict(max_new_tokens=8, eos_token_id=-1)
    reqs = [
        dict(base),
        dict(base, do_sample=True, temperature=0.8, top_k=tk, top_p=0.9, repetition_penalty=1.3, seed=11),
        dict(base, semantics="vllm", prompt_ids=[top[2][2]], logit_bias={top[2][3]: 1.5, top[2][0]: -0.7}, repetition_penalty=1.2,
             frequency_penalty=0.4, presence_penalty=0.3),
        dict(base, semantics="vllm", do_sample=True, temperature=0.9, top_k=tk + 1, top_p=0.9, min_p=0.05, seed=12),
        dict(semantics="vllm", max_new_tokens=8, eos_token_id=top[4][0], stop_any_ids=[top[4][1]], min_new_tokens=3),
        dict(base),
        dict(base),
        dict(base, do_sample=True, temperature=0.7, top_k=0, top_p=1.0, seed=13),
    ]
    hists = [[], [top[1][0], top[1][1], other[1]], [top[2][0], top[2][0], top[2][1]], [], [top[4][2]], [], [], [other[7]]]
    lps = [dict(k=5, source="raw"), dict(k=8, source="processed"), dict(k=5), dict(k=6), dict(k=4), None, dict(k=3, source="raw"),
           dict(k=0, source="raw")]
    return lg, reqs, hists, lps


@pytest.mark.parametrize("V", [7, 1025, 49157])
def test_operator_mixed_rows(V):
    lg, reqs, hists, lps = _op_case(V)
    tok, lp, rank, ids, vals = E.op_cb_logprobs(lg.to(dev()), reqs, lps, hists)
    assert torch.equal(tok, E.op_cb_select(lg.to(dev()), reqs, hists))              # the record changes no token
    items = []
    for b in (0, 1, 2, 3, 4, 7):
        keys, x32 = _reference(lg[b], reqs[b], lps[b], hists[b])
        items.append(dict(keys=keys, x32=x32, k=lps[b]["k"], tok=tok[b], lp=lp[b], rank=rank[b], ids=ids[b], lps=vals[b]))
    _compare(f"operator V={V}", items)
    assert int(rank[0]) == 1 and int(ids[0, 0]) == int(tok[0])                      # greedy, raw: slot 0 is the emitted token
    held = {reqs[4]["eos_token_id"], reqs[4]["stop_any_ids"][0]}
    assert not held & set(ids[4, :4].tolist()) and int(tok[4]) not in held          # the min_tokens hold: neither id is listed
    if V == 7:                                                                      # k = 8 over at most 4 kept ids: the tail is (-1, -inf)
        assert bool((ids[1, 4:8] == -1).all()) and bool((vals[1, 4:8] == NEG).all())
    # a row that records nothing, the all-NaN row, the row with k = 0
    assert np.isnan(float(lp[5])) and int(rank[5]) == 0 and bool((ids[5] == -1).all())
    assert ids[6, :3].tolist() == [-1] * 3 and int(rank[6]) == 0 and bool(torch.isnan(vals[6, :3]).all()) and np.isnan(float(lp[6]))
    assert int(tok[6]) == 0
    assert bool((ids[7] == -1).all()) and int(rank[7]) >= 1 and np.isfinite(float(lp[7]))
    # a row's record depends on that row alone: the same bits when it is the only row, and when nobody else records
    for b in (1, 3):
        solo = E.op_cb_logprobs(lg[b:b + 1].to(dev()), [reqs[b]], [lps[b]], [hists[b]])
        only = E.op_cb_logprobs(lg.to(dev()), reqs, [lps[i] if i == b else None for i in range(8)], hists)
        k = lps[b]["k"]
        for a, s, o in zip((tok, lp, rank, ids[:, :k], vals[:, :k]), solo, only):
            assert torch.equal(_bits(a[b]), _bits(s[0][..., :k] if s.dim() == 2 else s[0])), b
            assert torch.equal(_bits(a[b]), _bits(o[b][..., :k] if o.dim() == 2 else o[b])), b


# ---- the engine --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny8():
    cfg, w, eng, emb, prompt = _tiny()
    yield cfg, eng, emb, prompt
    eng.close()


def _cb_run(eng, embs, reqs, lps, step=8, shared=None):
    """Admit, run to the end, read every slot: [(tokens list, record or None)] per request."""
    eng.cb_reset()
    if shared is not None:
        slots = eng.cb_admit_shared(embs, None, shared, reqs, logprobs=lps)
    else:
        slots = eng.cb_admit(embs, reqs, logprobs=lps)
    while eng.cb_step(step) > 0:
        pass
    steps = eng.cb_poll()[1]
    out = []
    for s, l in zip(slots, lps or [None] * len(reqs)):
        out.append((eng.cb_read(s, 0, steps[s]).tolist(), eng.cb_read_logprobs(s, 0, steps[s]) if l is not None else None))
    eng.cb_reset()
    return out


def _solo(eng, emb_row, req, lp):
    """The request alone through sv_generate_topk: (tokens, token log-probs of the record's source, ranks, ids, log-probs)."""
    eng.cb_reset()
    S0 = emb_row.shape[0]
    out = eng.generate(emb_row.unsqueeze(0).contiguous(), max_length=S0 + req["max_new_tokens"], do_sample=bool(req.get("do_sample")),
                       temperature=req.get("temperature", 1.0), top_p=req.get("top_p", 1.0), top_k=req.get("top_k", 0), seed=req.get("seed", 0),
                       eos_token_id=req.get("eos_token_id", 0), repetition_penalty=req.get("repetition_penalty", 1.0),
                       min_new_tokens=req.get("min_new_tokens", 0), token_stats=True, token_topk=dict(k=lp["k"], source=lp["source"]))
    name = "token_logprobs" if lp["source"] == "raw" else "token_logprobs_processed"
    return (out["sequences"][0].tolist(), out[name][0].cpu(), out["token_ranks"][0].cpu(), out["top_token_ids"][0].cpu(),
            out["top_logprobs"][0].cpu())


def _hf_requests(eng, emb):
    free = eng.generate(emb[3:4].contiguous(), max_length=emb.shape[1] + 6, eos_token_id=-1)[0].tolist()
    reqs = [
        dict(max_new_tokens=20, eos_token_id=-1, repetition_penalty=1.3),
        dict(max_new_tokens=24, eos_token_id=-1, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.2, seed=5),
        dict(max_new_tokens=17, eos_token_id=-1, do_sample=True, temperature=1.1, top_k=0, top_p=0.95, seed=6),
        dict(max_new_tokens=12, eos_token_id=free[1], min_new_tokens=4),               # without the hold it would stop at column 1
    ]
    lps = [dict(k=5, source="raw"), dict(k=8, source="processed"), dict(k=3, source="raw"), dict(k=32, source="processed")]
    return reqs, lps


def test_engine_hf_slots_equal_their_solo_generate_bit_for_bit(tiny8):
    cfg, eng, emb, prompt = tiny8
    reqs, lps = _hf_requests(eng, emb)
    embs = [emb[i] for i in range(4)]
    got = _cb_run(eng, embs, reqs, lps)
    plain = _cb_run(eng, embs, reqs, None)
    for i, ((toks, rec), (ptoks, _)) in enumerate(zip(got, plain)):
        assert toks == ptoks, i                                                     # the tokens of the same requests without log-probs
        s_toks, s_lp, s_rank, s_ids, s_lps = _solo(eng, embs[i], reqs[i], lps[i])
        n = len(toks)
        assert toks == s_toks[:n] and n >= 5, i
        lp, rank, ids, vals = rec
        assert lp.shape == (n,) and ids.shape == vals.shape == (n, lps[i]["k"])
        assert torch.equal(_bits(lp), _bits(s_lp[:n])), i                           # column 0 (selected inside the admit) included
        assert torch.equal(rank, s_rank[:n].int()) and torch.equal(ids, s_ids[:n].int()) and torch.equal(_bits(vals), _bits(s_lps[:n])), i
    assert got[3][0][-1] == reqs[3]["eos_token_id"] or len(got[3][0]) == 12
    assert reqs[3]["eos_token_id"] not in got[3][1][2][:4].flatten().tolist()       # held at -inf for the first four columns: never listed


def _vllm_items(cfg, eng, embs, reqs, lps):
    """One run of the requests, the emitted tokens teacher-forced through sv_prefill / sv_decode_step for the raw fp32 logits of every step, and
    the restatement of every step.  Raises _Margin when a step's reference row does not decide its own answer (nothing of the record is read
    before that is known)."""
    got = _cb_run(eng, embs, reqs, lps)
    items = []
    for i, (toks, (lp, rank, ids, vals)) in enumerate(got):
        rows = [eng.prefill(embs[i].unsqueeze(0).contiguous())[0].cpu()]
        for t in toks[:-1]:
            rows.append(eng.decode_step(torch.tensor([t], device=dev()))[0].cpu())
        r, k = reqs[i], lps[i]["k"]
        for t, raw in enumerate(rows):
            keys, x32 = _reference(raw, r, lps[i], toks[:t])
            untouched = torch.ones(cfg.vocab, dtype=torch.bool)
            held = ([r["eos_token_id"]] + list(r.get("stop_any_ids") or [])) if t < r.get("min_new_tokens", 0) else []
            for j in list(r.get("prompt_ids") or []) + toks[:t] + list(r.get("logit_bias") or {}) + [h for h in held if h >= 0]:
                untouched[j] = False
            _assert_head_decided(raw, keys, untouched, max(0, min(k, int((keys > NEG).sum()) - 1)))
            items.append(dict(raw=raw, untouched=untouched, keys=keys, x32=x32, k=k, tok=toks[t], lp=lp[t], rank=rank[t],
                              ids=ids[t] if k else torch.empty(0, dtype=torch.int32), lps=vals[t] if k else torch.empty(0)))
    return got, items


def test_engine_vllm_slots_match_the_restatement(tiny8):
    """The engine's logits are bf16 values over 516 ids: two equal ones next to the top-p boundary are common, and there `_kept` and the kernel may
    each split the tie their own way.  So the sampling requests' seeds are chosen at run time, by the REFERENCE alone: the first pair of seeds
    whose every step passes the margin checks of `_reference` and `_assert_head_decided` (the engine is deterministic: always the same pair)."""
    cfg, eng, emb, prompt = tiny8
    lps = [dict(k=5), dict(k=8), dict(k=0)]
    embs = [emb[i] for i in range(3)]
    why = None
    for seed in range(77, 77 + 32):
        reqs = [
            dict(semantics="vllm", max_new_tokens=12, eos_token_id=-1, prompt_ids=prompt, repetition_penalty=1.3, frequency_penalty=0.6,
                 presence_penalty=0.4, logit_bias={300: 0.05}),
            dict(semantics="vllm", max_new_tokens=6, eos_token_id=-1, do_sample=True, temperature=0.9, top_k=8, top_p=0.8, min_p=0.02, seed=seed,
                 prompt_ids=prompt, repetition_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.1, logit_bias={5: 0.5}),
            dict(semantics="vllm", max_new_tokens=6, eos_token_id=0, stop_any_ids=[3], min_new_tokens=4, do_sample=True, temperature=1.2,
                 seed=seed + 1000),
        ]
        try:
            got, items = _vllm_items(cfg, eng, embs, reqs, lps)
            break
        except _Margin as e:
            why = e
    else:
        raise AssertionError(f"no seed in 77..108 gives reference rows with a margin at every step (last: {why})")
    print(f"[engine vLLM] seed {seed}")
    assert [t for t, _ in got] == [t for t, _ in _cb_run(eng, embs, reqs, None)]
    _compare("engine vLLM", items)
    assert bool((got[0][1][1] == 1).all())                                          # greedy: the emitted token is the best of its processed row
    print("[engine vLLM] kept ids per step of the top-k / top-p / min_p slot:", [int((it["keys"] > NEG).sum()) for it in items[12:18]])


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------
def test_record_depends_on_its_slot_alone():
    cfg, w, eng, emb, prompt = _tiny(max_batch=16)
    try:
        target = dict(max_new_tokens=20, eos_token_id=-1, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.2, seed=5)
        lp = dict(k=6, source="processed")
        others = [dict(max_new_tokens=9, eos_token_id=-1), dict(max_new_tokens=22, eos_token_id=-1, do_sample=True, temperature=1.1, seed=3),
                  dict(semantics="vllm", max_new_tokens=15, eos_token_id=-1, frequency_penalty=1.0, prompt_ids=[9])]
        alone = _cb_run(eng, [emb[1]], [target], [lp])[0]
        alone1 = _cb_run(eng, [emb[1]], [target], [lp], step=1)[0]                   # one step per call against eight
        # beside three non-recording slots (bucket 8), then as the tenth of ten (slot 9: bucket 16)
        small = _cb_run(eng, [emb[0], emb[2], emb[1], emb[3]], [others[0], others[1], target, others[2]], [None, None, lp, None])[2]
        fill = [others[j % 3] for j in range(9)]
        big = _cb_run(eng, [emb[j % 4] for j in range(9)] + [emb[1]], fill + [target], [None] * 9 + [lp])[9]
        both = _cb_run(eng, [emb[0], emb[1]], [others[1], target], [dict(k=2, source="raw"), lp])[1]      # a neighbour that records as well
        for name, run in (("step 1", alone1), ("bucket 8", small), ("bucket 16", big), ("neighbour records", both)):
            assert run[0] == alone[0], name
            for a, b in zip(alone[1], run[1]):
                assert torch.equal(_bits(a), _bits(b)), name
        # three samples of one prompt, each with its own k: every one equals its solo run, column 0 included
        reqs = [dict(target, seed=100 + j, max_new_tokens=8) for j in range(3)]
        lps = [dict(k=2, source="processed"), dict(k=5, source="raw"), dict(k=0, source="processed")]
        group = _cb_run(eng, [emb[2]], reqs, lps, shared=[0, 0, 0])
        for j, (toks, rec) in enumerate(group):
            solo = _cb_run(eng, [emb[2]], [reqs[j]], [lps[j]])[0]
            assert toks == solo[0] and rec[2].shape == (8, lps[j]["k"]), j
            for a, b in zip(rec, solo[1]):
                assert torch.equal(_bits(a), _bits(b)), j
            if lps[j]["k"]:
                s_toks, s_lp, s_rank, s_ids, s_lps = _solo(eng, emb[2], reqs[j], lps[j])
                assert torch.equal(_bits(rec[0][:1]), _bits(s_lp[:1])) and torch.equal(rec[2][0], s_ids[0].int()), j
    finally:
        eng.close()


# ---- 5. lifecycle ------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals(tiny8):
    cfg, eng, emb, prompt = tiny8
    eng.cb_reset()
    free = eng.generate(emb[0:1].contiguous(), max_length=emb.shape[1] + 6, eos_token_id=-1)[0].tolist()
    eos = free[2]
    n_eos = free.index(eos) + 1                                                     # the slot ends with its first EOS: at most three columns
    reqs = [dict(max_new_tokens=20, eos_token_id=eos), dict(max_new_tokens=5, eos_token_id=-1), dict(max_new_tokens=30, eos_token_id=-1)]
    s0, s1, s2 = eng.cb_admit([emb[0], emb[1], emb[2]], reqs, logprobs=[dict(k=4, source="raw"), dict(k=2, source="processed"), None])
    with pytest.raises(ValueError, match="emitted 1"):
        eng.cb_read_logprobs(s0, 0, 2)                                              # only the admit's column exists so far
    assert eng.cb_read_logprobs(s0, 0, 1)[2].shape == (1, 4)
    eng.cb_step(8)
    live, steps = eng.cb_poll()
    assert (live[s0], steps[s0]) == (0, n_eos) and (live[s1], steps[s1]) == (0, 5) and live[s2] == 1
    for s, n in ((s0, n_eos), (s1, 5)):                                             # finished mid-call: exactly `steps` columns, the last one included
        lp, rank, ids, vals = eng.cb_read_logprobs(s, 0, n)
        assert bool(torch.isfinite(lp).all()) and bool((rank >= 1).all()) and bool((ids[:, 0] >= 0).all())
        with pytest.raises(ValueError, match=f"emitted {n}"):
            eng.cb_read_logprobs(s, n, 1)
        with pytest.raises(ValueError):
            eng.cb_read_logprobs(s, 0, n + 1)
    assert int(eng.cb_read_logprobs(s0, n_eos - 1, 1)[2][0, 0]) == eos              # greedy, raw: the EOS column lists EOS first
    with pytest.raises(ValueError, match="records no log-probs"):
        eng.cb_read_logprobs(s2, 0, 1)
    first = eng.cb_read_logprobs(s1, 0, 5)
    # a reused slot: the new holder's columns alone, in the new holder's layout
    eng.cb_release(s1)
    with pytest.raises(ValueError, match="not in use"):
        eng.cb_read_logprobs(s1, 0, 1)
    s1b = eng.cb_admit([emb[3]], [dict(max_new_tokens=9, eos_token_id=-1)], logprobs=[dict(k=7, source="raw")])[0]
    assert s1b == s1
    lp, rank, ids, vals = eng.cb_read_logprobs(s1b, 0, 1)
    assert ids.shape == (1, 7)
    with pytest.raises(ValueError, match="emitted 1"):
        eng.cb_read_logprobs(s1b, 1, 1)                                             # the predecessor's columns 1..4 are out of reach
    eng.cb_step(8)
    again = eng.cb_read_logprobs(s1b, 0, 9)
    assert not torch.equal(_bits(again[0][:5]), _bits(first[0])) and int(again[1][0]) == 1
    eng.cb_release(s1b)
    s1c = eng.cb_admit([emb[3]], [dict(max_new_tokens=9, eos_token_id=-1)])[0]     # a holder that does not ask: nothing to read
    assert s1c == s1
    with pytest.raises(ValueError, match="records no log-probs"):
        eng.cb_read_logprobs(s1c, 0, 1)
    eng.cb_reset()
    # every refusal of the admit comes before device work: nothing is admitted, the engine runs on
    for req, lp in ((dict(max_new_tokens=4), dict(k=33, source="raw")), (dict(max_new_tokens=4), dict(k=-1, source="raw")),
                    (dict(max_new_tokens=4, semantics="vllm"), dict(k=3, source="raw"))):
        with pytest.raises(ValueError):
            eng.cb_admit([emb[0]], [req], logprobs=[lp])
        assert eng.cb_poll() == ([0] * 8, [0] * 8)
    arr = E.cb_logprobs([dict(max_new_tokens=4)], [dict(k=3)])
    arr[0].source = 2
    keep = E.cb_requests([dict(max_new_tokens=4)])
    import ctypes as C
    x = emb[0].contiguous()
    rc = eng.lib.sv_cb_admit_logprobs(eng._h, C.c_void_p(x.data_ptr()), 1, (C.c_int32 * 1)(x.shape[0]), 1, (C.c_int32 * 1)(0), keep[0], arr,
                                      (C.c_int32 * 1)(), None)
    assert rc == -22 and "source=2" in eng.lib.sv_last_error().decode()
    assert _cb_run(eng, [emb[0]], [dict(max_new_tokens=4, eos_token_id=-1)], [dict(k=1, source="raw")])[0][1][2].shape == (4, 1)


# ---- 6. the facade -----------------------------------------------------------------------------------------------------------------------
def test_llm_generate_with_logprobs(tmp_path):
    from PIL import Image
    from tests.ckpt_util import write_reference_checkpoint
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=21)
    path = str(tmp_path / "ckpt")
    write_reference_checkpoint(path, cfg, w)
    llm = VL.LLM(model=path, max_num_seqs=4, max_model_len=min(96, cfg.n_positions), trust_remote_code=True, byte_tokenizer_fallback=True)
    try:
        rng = np.random.default_rng(3)
        images = [Image.fromarray(rng.integers(0, 255, (40 + 7 * i, 48, 3), dtype=np.uint8)) for i in range(3)]
        inputs = [{"prompt": "<image-start>", "multi_modal_data": {"image": im}} for im in images]
        sps = [VL.SamplingParams(n=2, temperature=0.8, top_p=0.95, min_p=0.05, seed=11, max_tokens=10),
               VL.SamplingParams(n=1, temperature=0.0, max_tokens=9, repetition_penalty=1.3),
               VL.SamplingParams(n=2, temperature=1.0, top_k=40, frequency_penalty=0.5, seed=12, max_tokens=8)]
        plain = llm.generate(inputs, sps, use_tqdm=False)
        outs = llm.generate(inputs, sps, use_tqdm=False, logprobs=3)
        for ro, po in zip(outs, plain):
            for comp, pc in zip(ro.outputs, po.outputs):
                assert comp.token_ids == pc.token_ids and pc.logprobs is None and pc.cumulative_logprob is None
                assert len(comp.logprobs) == len(comp.token_ids) >= 1
                total = 0.0
                for tok, d in zip(comp.token_ids, comp.logprobs):
                    assert tok in d and 1 <= len(d) <= 4 and all(isinstance(v, VL.Logprob) for v in d.values())
                    n_list = len(d) - (len(d) == 4)                                  # four entries: the sampled id stands outside the list
                    assert sorted(v.rank for v in d.values())[:n_list] == list(range(1, n_list + 1))
                    assert d[tok].rank >= 1 and np.isfinite(d[tok].logprob) and d[tok].logprob <= 0.0
                    assert isinstance(d[tok].decoded_token, str)
                    total += d[tok].logprob
                assert abs(comp.cumulative_logprob - total) <= 1e-9 * max(1.0, abs(total))
        greedy = outs[1].outputs[0]
        assert all(d[t].rank == 1 for t, d in zip(greedy.token_ids, greedy.logprobs))
        zero = llm.generate(inputs[:1], sps[1], use_tqdm=False, logprobs=0)[0].outputs[0]
        assert all(list(d) == [t] for t, d in zip(zero.token_ids, zero.logprobs))
        with pytest.raises(ValueError, match="0..32"):
            llm.generate(inputs[:1], sps[1], use_tqdm=False, logprobs=33)
    finally:
        llm.engine.cb_reset()
        llm.close()
