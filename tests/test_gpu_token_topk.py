"""-m gpu: the k most likely ids of every step, their log-probs and the rank of the emitted / target token (sv_generate_topk, sv_forward_topk;
csrc/topk.h row_topk under sampling.hip token_topk_kernel and score.hip topk_rows_bf16_kernel).  The reference is torch in float64 on the very
rows the kernel read: the caller's rows for the operators, the logits_out / scores_out slabs of the same call for the engine.  Ids and ranks are
exact; log-probs lie within 4 x the largest deviation of torch's own fp32 log_softmax from that float64 reference on the same rows."""
import dataclasses

import pytest
import torch

import starvector_amd.engine as E
from oracle import starvector_oracle as O
from tests.gpu_util import build_engine, dev

pytestmark = pytest.mark.gpu
S0 = 4
NEG = float("-inf")


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def _ref_lists(keys, x32, k):
    """keys [R, V] fp32: what the list is ordered by; x32 [R, V] fp32: what is normalised (removed ids at -inf).  Returns ids [R, k] (descending
    by key, equal keys by ascending id -- a stable sort --, -1 past the ids that enter), float64 log-probs [R, k] (-inf there), the number of ids
    that enter per row, and the float64 / fp32 log_softmax of x32."""
    keys, x32 = keys.cpu(), x32.cpu()
    R, V = keys.shape
    enters = ~torch.isnan(keys) & (keys > NEG)
    kk = torch.where(enters, keys, torch.full_like(keys, NEG))
    order = torch.sort(kk, dim=-1, descending=True, stable=True).indices
    n = enters.sum(-1)
    ref64 = torch.log_softmax(x32.double(), -1)
    ids = torch.full((R, k), -1, dtype=torch.int64)
    lps = torch.full((R, k), NEG, dtype=torch.float64)
    m = min(k, V)
    slot = torch.arange(m).unsqueeze(0) < n.unsqueeze(1)
    ids[:, :m] = torch.where(slot, order[:, :m], torch.full_like(order[:, :m], -1))
    lps[:, :m] = torch.where(slot, ref64.gather(-1, order[:, :m]), torch.full((R, m), NEG, dtype=torch.float64))
    return ids, lps, n, ref64, torch.log_softmax(x32, -1)


def _tol(ref64, t32):
    fin = torch.isfinite(ref64)
    tol = 4.0 * float((t32.double()[fin] - ref64[fin]).abs().max())
    assert tol > 0
    return tol


def _ref_rank(keys, tok):
    keys = keys.cpu()
    xt = keys.gather(-1, tok.cpu().long().clamp(min=0).unsqueeze(-1))
    return 1 + (keys > xt).sum(-1)


def _assert_distinct_head(keys, k):
    """the first k + 1 values of every row are pairwise distinct: the order compared below is decided by values alone"""
    top = torch.sort(keys.cpu().float(), dim=-1, descending=True).values[:, : min(k + 1, keys.shape[1])]
    assert bool((top[:, 1:] < top[:, :-1]).all()), "tie among the first k + 1 values: pick another seed"


def _check_lists(name, got_ids, got_lps, ref_ids, ref_lps, tol):
    assert torch.equal(got_ids.cpu().long(), ref_ids), name
    g = got_lps.cpu().double()
    none = ref_ids < 0
    assert bool((g[none] == NEG).all()), f"{name}: a slot without an id must hold -inf"
    err = float((g[~none] - ref_lps[~none]).abs().max()) if bool((~none).any()) else 0.0
    print(f"[{name}] |kernel - f64| {err:.3e} (allowed {tol:.3e} = 4 x torch fp32's own deviation)")
    assert err <= tol, name


# ---- 1. operator, fp32 random rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [7, 516, 1023, 1024, 1025, 49156, 49157])
def test_operator_fp32_random_rows(V):
    B = 3
    ld = V + 3                                                                      # the row stride is no multiple of anything
    buf = torch.full((B, ld), 1e30)                                                 # columns >= V are never read: they would win every list
    buf[:, :V] = torch.randn(B, V, generator=torch.Generator().manual_seed(1000 + V)) * 3.0
    rows = buf[:, :V]
    _assert_distinct_head(rows, 32)
    tok = torch.randint(0, V, (B,), generator=torch.Generator().manual_seed(V)).to(torch.int32)
    ref_rank = _ref_rank(rows, tok)
    for T in (1.0, 0.7):
        x32 = rows / torch.full_like(rows, T)                                       # fp32 division, like the kernel's
        for k in (1, 5, 32):
            ids, lps, rank = E.op_token_topk(buf.to(dev()), tok.to(dev()), k, T, valid=V)
            ref_ids, ref_lps, n, ref64, t32 = _ref_lists(rows, x32, k)
            _check_lists(f"fp32 V={V} k={k} T={T}", ids, lps, ref_ids, ref_lps, _tol(ref64, t32))
            assert torch.equal(rank.cpu().long(), ref_rank)
            if k > V:
                assert bool((ids[:, V:] == -1).all()) and bool((lps[:, V:] == NEG).all())


# ---- 2. operator, designed rows ------------------------------------------------------------------------------------------------------
def _designed(V):
    g = torch.Generator().manual_seed(7)
    return torch.randn(V, generator=g).clamp(max=2.0)


@pytest.mark.parametrize("V", [1025, 49157])
def test_operator_designed_rows(V):
    k = 5
    scattered = sorted(int(i) for i in torch.randperm(V, generator=torch.Generator().manual_seed(3))[:10])
    assert not set(scattered) & {4, 5, 7, 11, 500, 700, 900, 1024}
    rows, toks, names = [], [], []
    a = _designed(V); a[scattered] = 9.0                                            # ten equal maxima: the five lowest ids, rank 1
    rows.append(a); toks.append(scattered[7]); names.append("plateau")
    b = _designed(V); b[[11, 500, 900]] = torch.tensor([12.0, 11.0, 10.0]); b[scattered] = 9.0      # the plateau straddles slot k
    rows.append(b); toks.append(scattered[9]); names.append("straddle")
    c = _designed(V); c[::3] = NEG; c[5] = 8.0                                      # -inf entries
    rows.append(c); toks.append(5); names.append("neg_inf")
    d = _designed(V); d[::2] = float("nan"); d[7] = 8.0                             # NaN entries: never listed, never counted
    rows.append(d); toks.append(7); names.append("nan")
    e = torch.full((V,), NEG); e[[4, 700, 1024]] = torch.tensor([1.0, 3.0, 2.0])    # exactly k - 2 finite entries
    rows.append(e); toks.append(1024); names.append("k_minus_2")
    f = torch.full((V,), NEG); f[1::2] = float("nan")                               # no comparable value
    rows.append(f); toks.append(0); names.append("nothing")
    h = torch.zeros(V)                                                              # one value everywhere: the plateau is wider than any cap
    rows.append(h); toks.append(V - 1); names.append("flat")
    buf = torch.stack(rows)
    tok = torch.tensor(toks, dtype=torch.int32)
    ids, lps, rank = E.op_token_topk(buf.to(dev()), tok.to(dev()), k, 1.0)
    ids, lps, rank = ids.cpu().long(), lps.cpu(), rank.cpu().long()
    ref_ids, ref_lps, n, ref64, t32 = _ref_lists(buf, buf, k)
    assert torch.equal(ids, ref_ids), (ids, ref_ids)
    assert ids[0].tolist() == scattered[:5] and int(rank[0]) == 1
    assert ids[1].tolist() == [11, 500, 900] + scattered[:2] and int(rank[1]) == 4
    assert int(ids[2, 0]) == 5 and int(rank[2]) == 1 and not any(int(i) % 3 == 0 for i in ids[2])
    assert int(ids[3, 0]) == 7 and int(rank[3]) == 1 and not any(int(i) % 2 == 0 for i in ids[3])
    assert ids[4].tolist() == [700, 1024, 4, -1, -1] and int(rank[4]) == 2
    assert bool((lps[4, 3:] == NEG).all()) and bool(torch.isfinite(lps[4, :3]).all())
    assert ids[5].tolist() == [-1] * 5 and int(rank[5]) == 0 and bool(torch.isnan(lps[5]).all())      # no comparable value: NaN, as dev_logprob
    assert bool(torch.isnan(lps[3]).all())                                          # a NaN in the row: every log-prob is NaN, in torch as here
    assert ids[6].tolist() == [0, 1, 2, 3, 4] and int(rank[6]) == 1
    # the tolerance is taken over the rows of the call, as everywhere in this file -- not row by row: torch's fp32 log_softmax of the flat row
    # happens to land within 2e-8 of float64, a quarter of an ulp of the value it returns (log 1025 = 6.93, ulp 4.8e-7), and no fp32 result
    # can promise that.  (The rows with a NaN are left out: it makes every log-prob NaN, in torch as here.)
    fin = [0, 1, 2, 4, 6]
    tol = _tol(ref64[fin], t32[fin])
    for r in fin:
        _check_lists(names[r], ids[r:r + 1], lps[r:r + 1], ref_ids[r:r + 1], ref_lps[r:r + 1], tol)
    # k = 32 over the flat row and the ten-wide plateau: the k-round path and the selection path give the rule's list
    ids32, _, _ = E.op_token_topk(buf[[0, 6]].to(dev()), None, 32, 1.0)
    ref32 = _ref_lists(buf[[0, 6]], buf[[0, 6]], 32)[0]
    assert torch.equal(ids32.cpu().long(), ref32)


# ---- 3. operator, row independence ---------------------------------------------------------------------------------------------------
def test_operator_row_independence():
    V, k = 49157, 32
    rows = torch.randn(64, V, generator=torch.Generator().manual_seed(5)) * 2.0
    rows[9] = rows[40]                                                              # the same row twice in one launch
    tok = torch.randint(0, V, (64,), generator=torch.Generator().manual_seed(6)).to(torch.int32)
    tok[9] = tok[40]
    all_ = E.op_token_topk(rows.to(dev()), tok.to(dev()), k, 0.7)
    for r in (0, 40, 63):
        solo = E.op_token_topk(rows[r:r + 1].to(dev()), tok[r:r + 1].to(dev()), k, 0.7)
        for a, s in zip(all_, solo):
            assert torch.equal(a[r].view(torch.int32), s[0].view(torch.int32)), r
    for a in all_:
        assert torch.equal(a[9].view(torch.int32), a[40].view(torch.int32))


# ---- 4. operator, bf16 scoring kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [516, 49157])
def test_operator_bf16_rows(V):
    B = 3
    ld = (V + 7) // 8 * 8 + 8
    g = torch.Generator().manual_seed(2000 + V)
    rows = torch.randn(B, V, generator=g).clamp(max=2.5)
    for r in range(B):                                                              # 40 distinct bf16 values above the bulk, at random ids
        pos = torch.randperm(V, generator=g)[:40]
        rows[r, pos] = 3.0 + 0.03125 * torch.arange(40, dtype=torch.float32)[torch.randperm(40, generator=g)]
    buf = torch.full((B, ld), 100.0)
    buf[:, :V] = rows
    buf = buf.to(torch.bfloat16)
    rows = buf[:, :V].float()
    _assert_distinct_head(rows, 32)
    tg = torch.randint(0, V, (B,), generator=g).to(torch.int32)
    tg[1] = -100
    ref_rank = torch.where(tg == -100, torch.zeros(B, dtype=torch.long), _ref_rank(rows, tg))
    for T in (1.0, 0.7):
        lp, lse, ent, am, flag = E.op_logprob_rows(buf.to(dev()), tg.to(dev()), T, valid=V)
        x32 = rows * (torch.ones(()) / torch.full((), T))                           # inv_t = 1.0f / T in fp32, like the kernel's
        for k in (1, 5, 32):
            ids, lps, rank = E.op_topk_rows_bf16(buf.to(dev()), tg.to(dev()), lse, k, T, valid=V)
            ref_ids, ref_lps, n, ref64, t32 = _ref_lists(rows, x32, k)
            _check_lists(f"bf16 V={V} k={k} T={T}", ids, lps, ref_ids, ref_lps, _tol(ref64, t32))
            assert torch.equal(rank.cpu().long(), ref_rank)
            assert torch.equal(ids[:, 0], am)                                       # slot 0 is the arg-max
            if k == 32:
                for r in (0, 2):                                                    # the target's slot: the log-prob of sv_op_logprob_rows, bit for bit
                    hit = (ids[r] == int(tg[r])).nonzero().flatten()
                    want = int(ref_rank[r]) <= 32
                    assert (hit.numel() == 1) == want
                    if want:
                        assert torch.equal(lps[r, hit].view(torch.int32), lp[r:r + 1].view(torch.int32))
    # a planted target inside the list, whatever the seed gave above
    tg2 = torch.tensor([int(_ref_lists(rows, rows, 5)[0][r, 3]) for r in range(B)], dtype=torch.int32)
    lp, lse, ent, am, flag = E.op_logprob_rows(buf.to(dev()), tg2.to(dev()), 0.7, valid=V)
    ids, lps, rank = E.op_topk_rows_bf16(buf.to(dev()), tg2.to(dev()), lse, 5, 0.7, valid=V)
    assert rank.tolist() == [4] * B and torch.equal(lps[:, 3].view(torch.int32), lp.view(torch.int32))


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    cfg = dataclasses.replace(O.OracleConfig.tiny(), n_positions=256)
    w = O.make_weights(cfg, seed=31)
    eng = build_engine(cfg, w, max_batch=40, max_seq_len=160)
    yield cfg, w, eng
    eng.close()


def _emb(eng, B, seed, V, S=S0):
    ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(seed))
    return eng.embed_tokens(ids.to(dev()))


def _slabs(cfg, rows, max_new, names=("logits_out",)):
    return {n: torch.full((max_new, rows, cfg.vocab), float("nan"), dtype=torch.float32, device=dev()) for n in names}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("B", [3, 33])
def test_engine_greedy_raw(tiny, B):
    """5. greedy, raw source, k = 5: tokens of the plain call; slot 0 is the emitted token with rank 1 and token_logprobs' bits; the lists match
    float64 over logits_out; a row ended by EOS reads -1 / 0 / 0 afterwards."""
    cfg, w, eng = tiny
    emb = _emb(eng, B, 61, cfg.vocab)
    n_new, k = 12, 5
    free = eng.generate(emb, max_length=S0 + n_new, eos_token_id=-1)
    eos = int(free[1, 3])                                                           # row 1 ends at column 3 at the latest
    kw = dict(max_length=S0 + n_new, eos_token_id=eos, pad_token_id=cfg.pad_token_id)
    plain = eng.generate(emb, **kw)
    sl = _slabs(cfg, B, n_new)
    out = eng.generate(emb, token_stats=True, token_topk=k, **sl, **kw)
    seq, L = out["sequences"], out["n_generated"]
    assert torch.equal(seq, plain)
    ids, lps, rank = out["top_token_ids"], out["top_logprobs"], out["token_ranks"]
    assert ids.shape == lps.shape == (B, L, k) and rank.shape == (B, L) and ids.dtype == torch.int32 and lps.dtype == torch.float32
    is_eos = seq == eos
    lens = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, torch.full((B,), L, device=seq.device))
    live = torch.arange(L, device=seq.device).unsqueeze(0) < lens.unsqueeze(1)
    assert int(lens[1]) <= 4 and not bool(live.all())
    assert bool((ids[~live] == -1).all()) and bool((lps[~live] == 0).all()) and bool((rank[~live] == 0).all())
    assert torch.equal(ids[..., 0][live].long(), seq[live]) and bool((rank[live] == 1).all())
    assert torch.equal(_bits(lps[..., 0].contiguous()), _bits(out["token_logprobs"].contiguous()))
    raw = sl["logits_out"][:L].transpose(0, 1)[live]                                # [n_live, V], the rows the kernel read
    ref_ids, ref_lps, n, ref64, t32 = _ref_lists(raw, raw, k)
    _check_lists(f"engine greedy B={B}", ids[live], lps[live], ref_ids, ref_lps, _tol(ref64, t32))
    alone = eng.generate(emb, token_topk=dict(k=k, rank=False), **kw)               # without statistics and rank: the same lists
    assert "token_ranks" not in alone and torch.equal(alone["top_token_ids"], ids) and torch.equal(_bits(alone["top_logprobs"]), _bits(lps))


def test_engine_sampling_processed(tiny):
    """6. sampling (top_k 5, top_p 0.9), processed source, k = 8: the emitted id is listed with token_logprobs_processed' bits, the finite slots
    are the kept set (at most 5 of them; HF's TopK keeps every id equal to the 5th value, so a row whose 5th and 6th raw logits are equal --
    seen on the reference's rows, not on the lists -- may keep more), the rest (-1, -inf), exp sums to 1, rank <= the kept set's size."""
    cfg, w, eng = tiny
    B, n_new, k = 4, 12, 8
    emb = _emb(eng, B, 62, cfg.vocab)
    kw = dict(max_length=S0 + n_new, eos_token_id=-1, do_sample=True, temperature=0.7, top_k=5, top_p=0.9, seed=17)
    plain = eng.generate(emb, **kw)
    sl = _slabs(cfg, B, n_new, ("scores_out", "logits_out"))
    out = eng.generate(emb, token_stats=True, token_topk=dict(k=k, source="processed"), **sl, **kw)
    seq = out["sequences"]
    assert torch.equal(seq, plain)
    ids, lps, rank = out["top_token_ids"].long(), out["top_logprobs"], out["token_ranks"]
    scores = sl["scores_out"].transpose(0, 1)                                       # [B, L, V]: kept ids s / T, the rest -inf
    kept = (scores > NEG).sum(-1)
    raw_sorted = sl["logits_out"].transpose(0, 1).sort(-1, descending=True).values
    # every row: at most 5 ids, plus the further ids whose raw logit EQUALS the 5th largest (HF's TopK removes `scores < kth`, so they stay)
    extra = (raw_sorted[..., 5:] == raw_sorted[..., 4:5]).sum(-1)
    assert bool((extra == 0).any()) and bool((kept <= 5 + extra).all()) and int(kept.min()) >= 1
    n_listed = (ids >= 0).sum(-1)
    assert torch.equal(n_listed, kept)                                              # the kept set, whole: at most 5 finite slots ...
    none = ids < 0
    assert bool((lps[none] == NEG).all()) and bool(torch.isfinite(lps[~none]).all())      # ... the rest (-1, -inf)
    hit = ids == seq.unsqueeze(-1)
    assert bool((hit.sum(-1) == 1).all())                                           # the emitted id is listed ...
    assert torch.equal(_bits(lps[hit]), _bits(out["token_logprobs_processed"].reshape(-1)))      # ... with the statistic's bits
    assert bool((rank >= 1).all()) and bool((rank.long() <= kept).all())
    flat = scores.reshape(-1, cfg.vocab)
    assert torch.equal(rank.reshape(-1).cpu().long(), _ref_rank(flat, seq.reshape(-1)))
    ref_ids, ref_lps, n, ref64, t32 = _ref_lists(flat, flat, k)
    tol = _tol(ref64, t32)
    _check_lists("engine sampling processed", ids.reshape(-1, k), lps.reshape(-1, k), ref_ids, ref_lps, tol)
    # every slot is within tol of its float64 log-prob, so each exp is off by at most tol relative to itself and the sum, whose exact terms
    # add up to 1, by at most tol (exp and the sum in float64: they add nothing of their own)
    mass = torch.where(none, torch.zeros_like(lps), lps).double().exp().masked_fill(none, 0.0).sum(-1)
    assert float((mass - 1).abs().max()) <= tol


def test_engine_no_repeat_ngram(tiny):
    """7. no_repeat_ngram_size = 2: the raw lists are those of the raw rows (captured before the ban), the processed lists hold no banned id,
    the raw source with a rank is refused."""
    cfg, w, eng = tiny
    B, n_new, k = 3, 14, 5
    emb = _emb(eng, B, 63, cfg.vocab)
    kw = dict(max_length=S0 + n_new, eos_token_id=-1, no_repeat_ngram_size=2)
    plain = eng.generate_processed(emb, **kw)
    sl = _slabs(cfg, B, n_new, ("logits_out", "scores_out"))
    raw = eng.generate_processed(emb, token_topk=dict(k=k, source="raw", rank=False), **sl, **kw)
    assert torch.equal(raw["sequences"], plain) and "token_ranks" not in raw
    rows = sl["logits_out"].transpose(0, 1).reshape(-1, cfg.vocab)
    ref_ids, ref_lps, n, ref64, t32 = _ref_lists(rows, rows, k)
    _check_lists("ngram raw", raw["top_token_ids"].reshape(-1, k), raw["top_logprobs"].reshape(-1, k), ref_ids, ref_lps, _tol(ref64, t32))
    banned = (sl["scores_out"] == NEG) & (sl["logits_out"] > NEG)
    assert bool(banned.any())                                                       # the ban did remove something
    pro = eng.generate_processed(emb, token_stats=True, token_topk=dict(k=k, source="processed"), **kw)
    assert torch.equal(pro["sequences"], plain)
    sc = sl["scores_out"].transpose(0, 1)                                           # [B, L, V]
    listed = sc.gather(-1, pro["top_token_ids"].long())
    assert bool((listed > NEG).all())                                               # no banned id is listed
    flat = sc.reshape(-1, cfg.vocab)
    ref_ids, ref_lps, n, ref64, t32 = _ref_lists(flat, flat, k)
    _check_lists("ngram processed", pro["top_token_ids"].reshape(-1, k), pro["top_logprobs"].reshape(-1, k), ref_ids, ref_lps, _tol(ref64, t32))
    assert torch.equal(pro["top_token_ids"][..., 0].long(), plain) and bool((pro["token_ranks"] == 1).all())
    assert torch.equal(_bits(pro["top_logprobs"][..., 0].contiguous()), _bits(pro["token_logprobs_processed"].contiguous()))
    with pytest.raises(ValueError, match="source 1"):
        eng.generate_processed(emb, token_topk=dict(k=k, source="raw", rank=True), **kw)
    assert torch.equal(eng.generate_processed(emb, **kw), plain)                    # the refusal left the engine as it was


def test_engine_ragged_and_n_samples(tiny):
    """8. ragged prompts and n_samples = 3: the lists of a row are those of the same row run solo."""
    cfg, w, eng = tiny
    n_new, k = 8, 5
    lens = [3, 6, 4]
    embs = [_emb(eng, 1, 70 + i, cfg.vocab, S=n)[0] for i, n in enumerate(lens)]
    rag = eng.generate_ragged(embs, max_length=max(lens) + n_new, eos_token_id=-1, token_topk=k)
    for i, e in enumerate(embs):
        solo = eng.generate(e.unsqueeze(0).contiguous(), max_length=lens[i] + n_new, eos_token_id=-1, token_topk=k)
        for name in ("sequences", "top_token_ids", "top_logprobs", "token_ranks"):
            assert torch.equal(_bits(rag[name][i:i + 1].contiguous()), _bits(solo[name].contiguous())), (i, name)
    emb = _emb(eng, 2, 75, cfg.vocab)
    kw = dict(max_length=S0 + n_new, eos_token_id=-1, do_sample=True, temperature=0.9, top_k=20, top_p=0.9, seed=9,
              token_topk=dict(k=k, source="processed"))
    shared = eng.generate_shared(emb, n_samples=3, **kw)
    rep = eng.generate(emb.repeat_interleave(3, dim=0).contiguous(), **kw)
    for name in ("sequences", "top_token_ids", "top_logprobs", "token_ranks"):
        assert torch.equal(_bits(shared[name].contiguous()), _bits(rep[name].contiguous())), name
    assert shared["top_token_ids"].shape == (6, n_new, k)


def test_graph_reuse_on_one_engine(tiny):
    """9. k = 5, plain, statistics only, k = 3 with other buffers, on one engine: each call equals a fresh engine's, the plain and the statistics
    call keep their step (the launch count of a fresh engine's) and their bits."""
    cfg, w, eng = tiny
    B, n_new = 4, 40                                                                # several replays of the kept graph per call
    emb_ids = torch.randint(0, cfg.vocab, (B, S0), generator=torch.Generator().manual_seed(64))
    kw = dict(max_length=S0 + n_new, eos_token_id=-1)
    calls = [dict(token_stats=True, token_topk=5), dict(), dict(token_stats=True), dict(token_topk=dict(k=3, source="processed"))]

    def run(e, extra):
        out = e.generate(e.embed_tokens(emb_ids.to(dev())), **extra, **kw)
        out = out if isinstance(out, dict) else {"sequences": out}
        return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}, e.step_plan()["graph_kernel_nodes"]

    got = [run(eng, c) for c in calls]
    for c, (res, nodes) in zip(calls, got):
        fresh = build_engine(cfg, w, max_batch=40, max_seq_len=160)
        try:
            want, want_nodes = run(fresh, c)
        finally:
            fresh.close()
        assert set(res) == set(want), c
        for name in want:
            assert torch.equal(_bits(res[name].contiguous()), _bits(want[name].contiguous())), (c, name)
        assert nodes == want_nodes, c
    assert got[0][1] == got[2][1] + 1                                               # the list is one launch beside the statistics launch
    assert torch.equal(got[0][0]["sequences"], got[1][0]["sequences"])
    for name in ("token_logprobs", "token_logprobs_processed", "token_entropies"):
        assert torch.equal(_bits(got[0][0][name].contiguous()), _bits(got[2][0][name].contiguous())), name


def test_scoring_forward_topk(tiny):
    """10. forward_logprobs(top_k=4) against float64 over sv_forward_logits' bf16 rows; chunked = unchunked, bit for bit."""
    cfg, w, eng = tiny
    B, S, n, k, T = 4, 100, 100, 4, 0.7                                             # 400 kept rows: two chunks of 256
    emb = _emb(eng, B, 65, cfg.vocab, S=S)
    targets = torch.randint(0, cfg.vocab, (B, n), generator=torch.Generator().manual_seed(66)).to(torch.int32)
    targets[0, :5] = -100
    rows = eng.forward_logits(emb, n).float().reshape(B * n, cfg.vocab)             # bf16 values
    outs = []
    try:
        for chunk in (0, 256):
            eng.set_score_chunk_rows(chunk)
            outs.append(eng.forward_logprobs(emb, targets.to(dev()), n, T, top_k=k))
    finally:
        eng.set_score_chunk_rows(0)
    a, b = outs
    plain = eng.forward_logprobs(emb, targets.to(dev()), n, T)
    for name in ("logprobs", "logsumexp", "top_token_ids", "top_logprobs", "token_ranks"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert torch.equal(_bits(a.logprobs), _bits(plain.logprobs)) and len(plain) == 4 and not hasattr(plain, "top_token_ids")
    assert a.top_token_ids.shape == a.top_logprobs.shape == (B, n, k) and a.token_ranks.shape == (B, n)
    x32 = rows * (torch.ones(()) / torch.full((), T))                               # inv_t = 1.0f / T in fp32, like the kernel's
    ref_ids, ref_lps, cnt, ref64, t32 = _ref_lists(rows, x32, k)
    _check_lists("scoring forward", a.top_token_ids.reshape(-1, k), a.top_logprobs.reshape(-1, k), ref_ids, ref_lps, _tol(ref64, t32))
    tg = targets.reshape(-1)
    ref_rank = torch.where(tg == -100, torch.zeros_like(tg, dtype=torch.long), _ref_rank(rows, tg))
    assert torch.equal(a.token_ranks.reshape(-1).cpu().long(), ref_rank)
    hit = (a.top_token_ids.reshape(-1, k).cpu().long() == tg.long().unsqueeze(-1))
    assert bool(hit.any())
    assert torch.equal(_bits(a.top_logprobs.reshape(-1, k).cpu()[hit]), _bits(a.logprobs.reshape(-1).cpu()[hit.any(-1)]))
