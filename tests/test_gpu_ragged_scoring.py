"""-m gpu: the ragged scoring pass -- sequences of different lengths, packed back to back, each with its own number of kept rows, scored in
ONE prompt pass (sv_forward_logprobs_ragged; HipEngine.forward_logprobs_ragged; completion_logprobs(..., unpadded=True)).

Contract: for every sequence of a ragged call every output of its kept rows -- log-prob, logsumexp, entropy, arg-max, the top-k ids and
log-probs, the rank -- is BIT-IDENTICAL to sv_forward_topk on that sequence alone (B = 1, S = its length, n_keep = its keep), whatever the
other sequences, their order and the lm_head chunk size.  No tolerance anywhere: every comparison is torch.equal on the int32 view.  The
reference of every check is the engine's own solo run, which the rest of the suite ties to the oracle, float64 and HF."""
import types

import pytest
import torch

from starvector_amd import engine as E
from starvector_amd.model import StarVectorForCausalLM
from tests.gpu_util import bf, dev
from tests.test_gpu_ragged_prefill import LENS, _embeds, _fullsize_engine, _seq_of, _shuffled, _tiny_engine

pytestmark = pytest.mark.gpu

FIELDS = ("logprobs", "logsumexp", "entropy", "argmax", "top_token_ids", "top_logprobs", "token_ranks")
# kept rows per length: 1, 2 and all rows; 200 of 257 / 130 of 260 / 400 of 515 lie across the sequence's 256-row tile boundaries (the first
# with the peel row, the last across two); 1253 kept rows in all = five chunks of 256 with sequences straddling the chunk edges
KEEP_OF = {5: 5, 31: 1, 255: 2, 256: 256, 257: 200, 259: 259, 260: 130, 515: 400}
TOP_K = 5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _targets(keep, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in keep:
        t = torch.randint(0, vocab, (n,), generator=g, dtype=torch.int32)
        t[torch.rand(n, generator=g) < 0.15] = -100
        out.append(t.to(dev()))
    return out


def _solo(eng, seqs, targets, keep, temperature):
    return [eng.forward_logprobs(x[None].contiguous(), t[None].contiguous(), n, temperature, entropy=True, argmax=True, top_k=TOP_K)
            for x, t, n in zip(seqs, targets, keep)]


def _check_ragged(eng, seqs, targets, keep, solo, temperature, tag):
    got = eng.forward_logprobs_ragged(seqs, torch.cat(targets), keep, temperature=temperature, entropy=True, argmax=True, top_k=TOP_K)
    assert isinstance(got, E.TokenTopLogprobs) and got.logprobs.shape == (sum(keep),) and got.top_token_ids.shape == (sum(keep), TOP_K)
    r0 = 0
    for b, n in enumerate(keep):
        for f in FIELDS:
            assert torch.equal(_bits(getattr(got, f)[r0:r0 + n]), _bits(getattr(solo[b], f)[0])), \
                f"[{tag}, T={temperature}] {f} of sequence {b} (length {seqs[b].shape[0]}, keep {n}) differs from its solo run"
        ign = targets[b] == -100
        assert bool((got.logprobs[r0:r0 + n][ign] == 0).all()) and bool((got.token_ranks[r0:r0 + n][ign] == 0).all())
        r0 += n


def _check_contract(eng, hidden, vocab, lens, keep, seed, tag, scale=1.0):
    """chunks of 256 rows, the default chunk, and the sequences in another order, at two temperatures, against ONE set of solo runs"""
    seqs = _embeds(lens, hidden, seed, scale=scale)
    targets = _targets(keep, vocab, seed + 1)
    order = list(reversed(range(len(lens))))
    order[0], order[2] = order[2], order[0]
    pick = lambda v: [v[i] for i in order]
    for temperature in (1.0, 0.7):
        solo = _solo(eng, seqs, targets, keep, temperature)
        eng.set_score_chunk_rows(256)
        _check_ragged(eng, seqs, targets, keep, solo, temperature, f"{tag}, chunk 256")
        _check_ragged(eng, pick(seqs), pick(targets), pick(keep), pick(solo), temperature, f"{tag}, chunk 256, other order")
        eng.set_score_chunk_rows(0)
        _check_ragged(eng, seqs, targets, keep, solo, temperature, f"{tag}, default chunk")
    # k = 0 is the call without lists: the TokenLogprobs type, the same bits
    plain = eng.forward_logprobs_ragged(seqs, torch.cat(targets), keep, temperature=0.7)
    assert isinstance(plain, E.TokenLogprobs) and plain.entropy is None and plain.argmax is None
    assert torch.equal(_bits(plain.logprobs), _bits(torch.cat([s.logprobs[0] for s in solo])))


# ---- the operator ------------------------------------------------------------------------------------------------------------------------
def test_gather_tail_rows_ragged_operator():
    lens, keep, D = [1, 4, 9, 2], [1, 4, 3, 1], 64
    h = bf(torch.randn(sum(lens), D, generator=torch.Generator().manual_seed(5)))
    out = torch.full((sum(keep) + 1, D), 7.0, dtype=torch.bfloat16, device=dev())
    E.op_gather_tail_rows_ragged(h, lens, keep, out=out)
    rows, first = [], 0
    for n, k in zip(lens, keep):
        rows += list(range(first + n - k, first + n))
        first += n
    assert torch.equal(out[:-1].view(torch.int16), h[torch.tensor(rows, device=dev())].view(torch.int16))
    assert bool((out[-1] == 7.0).all()), "the row behind the output was written"
    for bad in ([1, 4, 0, 1], [1, 5, 3, 1], [1, 4, 3]):
        with pytest.raises(ValueError):
            E.op_gather_tail_rows_ragged(h, lens, bad)


# ---- the bitwise contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_forward_logprobs_ragged_tiny_models_bitwise(arch):
    cfg, eng = _tiny_engine(arch, max_batch=32, max_seq_len=640)
    lens = _shuffled(LENS, 3)
    _check_contract(eng, cfg.hidden, cfg.vocab, lens, [KEEP_OF[n] for n in lens], 71, f"tiny {arch}")
    eng.close()


def test_forward_logprobs_ragged_starvector_1b_dimensions():
    ec, eng = _fullsize_engine(max_batch=32, max_seq_len=640)
    lens = _shuffled(LENS, 4)
    # the length list reaches a peel row and whole tiles at these shapes -- asserted, not assumed (as tests/test_gpu_ragged_prefill.py does)
    D, F, QKV = ec.hidden, ec.n_inner, ec.hidden + 2 * (ec.hidden // ec.n_head)
    plans = {name: E.ragged_plan(lens, N, K, act) for name, (N, K, act) in
             {"c_attn": (QKV, D, "none"), "c_proj": (D, D, "none"), "c_fc": (F, D, "gelu_tanh"), "down": (D, F, "none")}.items()}
    peel = {n: sorted(len([r for r in p["rows"] if _seq_of(lens, r) == b]) for b in p["last"]) for n, p in plans.items()}
    assert any(1 in v for v in peel.values()) and any(3 in v for v in peel.values()), peel
    assert plans["c_proj"]["rows"] and all(len(p["last"]) < len(lens) for p in plans.values()), plans
    assert {5, 256, 260} <= set(lens)
    _check_contract(eng, ec.hidden, ec.vocab, lens, [KEEP_OF[n] for n in lens], 81, "1B dims", scale=0.5)
    eng.close()


def test_forward_logprobs_ragged_sliding_window():
    cfg, eng = _tiny_engine("v2", max_batch=8, max_seq_len=256, window=24)
    lens = [7, 100, 24, 25, 3, 70]
    _check_contract(eng, cfg.hidden, cfg.vocab, lens, [7, 60, 1, 25, 2, 30], 91, "tiny v2 window 24")
    eng.close()


# ---- the mirror --------------------------------------------------------------------------------------------------------------------------
def _mirror(eng):
    m = StarVectorForCausalLM.__new__(StarVectorForCausalLM)
    torch.nn.Module.__init__(m)
    object.__setattr__(m, "engine", eng)
    object.__setattr__(m, "model", types.SimpleNamespace(_get_embeddings=eng.embed_tokens))
    return m


@pytest.mark.parametrize("side", ["left", "right"])
def test_completion_logprobs_unpadded_is_one_prompt_pass_and_equals_the_solo_runs(side):
    cfg, eng = _tiny_engine("v1", max_batch=8, max_seq_len=200)
    m = _mirror(eng)
    lens = [70, 9, 64, 33, 65]
    B, T, S, K = len(lens), 3, max(lens), 4
    L = S - T
    n = 8 if side == "left" else 40          # left: the shortest row holds n + 1 rows; right: rows end before, inside and behind the window
    g = torch.Generator().manual_seed(101)
    vis = bf(torch.randn(1, T, cfg.hidden, generator=g))
    ids = torch.randint(0, cfg.vocab, (B, L), generator=g).to(dev())
    mask = torch.zeros(B, S, dtype=torch.long, device=dev())
    for b, n_b in enumerate(lens):
        mask[b, (slice(S - n_b, S) if side == "left" else slice(0, n_b))] = 1
    emb = torch.cat([vis.repeat(B, 1, 1), eng.embed_tokens(ids)], 1)
    kw = dict(temperature=0.8, return_entropy=True, top_logprobs=K)

    before = eng.prompt_passes()
    out = m.completion_logprobs(vis, ids, B, mask, n, unpadded=True, **kw)
    assert eng.prompt_passes() - before == 1                   # one prompt pass for five rows of five lengths
    assert sorted(out) == ["entropies", "logprobs", "token_ranks", "top_logprobs", "top_token_ids"]
    assert out["logprobs"].shape == out["entropies"].shape == out["token_ranks"].shape == (B, n) and out["top_token_ids"].shape == (B, n, K)
    names = {"logprobs": "logprobs", "entropies": "entropy", "top_token_ids": "top_token_ids", "top_logprobs": "top_logprobs",
             "token_ranks": "token_ranks"}
    fill = {"logprobs": 0, "entropies": 0, "top_token_ids": -1, "top_logprobs": 0, "token_ranks": 0}
    for b, n_b in enumerate(lens):
        lead = S - n_b if side == "left" else 0
        c = max(0, lead + n_b - (S - n))                       # scored tokens of the row: entries 0 .. c - 1
        x = emb[b, lead:lead + n_b]
        tg = torch.cat([ids[b, L - n:L - n + c].to(torch.int32), torch.full((1,), -100, dtype=torch.int32, device=dev())])
        solo = eng.forward_logprobs(x[None].contiguous(), tg[None], c + 1, 0.8, entropy=True, top_k=K)
        for key, f in names.items():
            assert torch.equal(_bits(out[key][b, :c]), _bits(getattr(solo, f)[0, :c])), (side, b, key)
            assert bool((out[key][b, c:] == fill[key]).all()), (side, b, key, "pads do not hold the fill value")
        assert c == 0 or float(out["logprobs"][b, :c].abs().min()) > 0.0

    # the default: the code of before, one prompt pass per pad group
    before = eng.prompt_passes()
    old = m.completion_logprobs(vis, ids, B, mask, n, **kw)
    assert eng.prompt_passes() - before == (len(set(lens)) if side == "left" else 1)
    if side == "left":                                         # every group is one row without its pads: the solo runs again
        for key in names:
            assert torch.equal(_bits(old[key]), _bits(out[key])), key
    else:                                                      # the rectangular call over the padded rows, pads multiplied away
        tg = torch.full((B, n + 1), -100, dtype=torch.int32, device=dev())
        tg[:, :n] = ids[:, L - n:].to(torch.int32).masked_fill(mask[:, S - n:] == 0, -100)
        r = eng.forward_logprobs(emb, tg, n + 1, 0.8, entropy=True, top_k=K)
        assert torch.equal(_bits(old["logprobs"]), _bits(r.logprobs[:, :n]))
        assert torch.equal(_bits(old["entropies"]), _bits(r.entropy[:, :n].masked_fill(mask[:, S - n:] == 0, 0.0)))
        assert torch.equal(old["top_token_ids"], r.top_token_ids[:, :n]) and torch.equal(old["token_ranks"], r.token_ranks[:, :n])
    # no pads: the rectangular call whatever the keyword
    ones = torch.ones_like(mask)
    before = eng.prompt_passes()
    a = m.completion_logprobs(vis, ids, B, ones, n, unpadded=True, **kw)
    b_ = m.completion_logprobs(vis, ids, B, ones, n, **kw)
    assert eng.prompt_passes() - before == 2 and all(torch.equal(_bits(a[key]), _bits(b_[key])) for key in names)
    eng.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_forward_logprobs_ragged_refusals():
    cfg, eng = _tiny_engine("v1", max_batch=4, max_seq_len=64)
    lens, keep = [9, 20, 12], [3, 5, 12]
    seqs = _embeds(lens, cfg.hidden, 111)
    tg = torch.randint(0, cfg.vocab, (sum(keep),), generator=torch.Generator().manual_seed(112), dtype=torch.int32).to(dev())
    ok = eng.forward_logprobs_ragged(seqs, tg, keep)
    with pytest.raises(ValueError, match="keep"):
        eng.forward_logprobs_ragged(seqs, tg[:-5], [3, 0, 12])
    with pytest.raises(ValueError, match="keep"):
        eng.forward_logprobs_ragged(seqs, torch.cat([tg, tg[:1]]), [3, 5, 13])
    with pytest.raises(ValueError, match="targets"):
        eng.forward_logprobs_ragged(seqs, tg[:-1], keep)
    long = _embeds([9, 65], cfg.hidden, 113)
    with pytest.raises(ValueError, match=r"length 65 of sequence 1 out of range \(1\.\.max_seq_len 64\)"):
        eng.forward_logprobs_ragged(long, tg[:2], [1, 1])
    with pytest.raises(ValueError, match="max_batch 4"):
        eng.forward_logprobs_ragged(_embeds([3] * 5, cfg.hidden, 114), tg[:5], [1] * 5)
    bad = tg.clone()
    bad[3 + 5 + 7] = cfg.vocab                                 # sequence 2, kept position 7: packed row 15
    bad[3 + 5 + 9] = -5
    with pytest.raises(ValueError, match=r"target id outside \[0, %d\).*row 15 \(sequence 2, kept position 7\)" % cfg.vocab):
        eng.forward_logprobs_ragged(seqs, bad, keep)
    again = eng.forward_logprobs_ragged(seqs, tg, keep)           # a refused call leaves nothing behind
    assert torch.equal(_bits(again.logprobs), _bits(ok.logprobs))
    eng.close()
