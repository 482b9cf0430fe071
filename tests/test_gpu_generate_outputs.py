"""-m gpu: HF structured generate outputs (return_dict_in_generate with output_scores / output_logits) written from inside the
captured decode step (sv_generate_ex): raw logits against HF's own forward, processed scores against torch restatements of HF's
processors and warpers, beam_indices / sequences_scores against HF's compute_transition_scores invariant and the standalone scorer."""
import dataclasses
import os

import pytest
import torch

from oracle import starvector_oracle as O
from starvector_amd.engine import HipBeamScorer
from starvector_amd.model import HipCausalLM, StoppingCriteriaSub
from tests.gpu_util import build_engine, dev, hf_decoder_bf16, hf_teacher_forced_logits

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1.8e-2          # tests/test_gpu_e2e.py
S0 = 4


@pytest.fixture(scope="module")
def tiny():
    cfg = dataclasses.replace(O.OracleConfig.tiny(), n_positions=256)      # room for > 4 polling chunks of 32 steps
    w = O.make_weights(cfg, seed=31)
    eng = build_engine(cfg, w, max_batch=40, max_seq_len=160)
    yield cfg, w, eng, hf_decoder_bf16(cfg, w)
    eng.close()


def _emb(eng, B, seed, V):
    ids = torch.randint(0, V, (B, S0), generator=torch.Generator().manual_seed(seed))
    return eng.embed_tokens(ids.to(dev()))


def _lm(eng, cfg):
    return HipCausalLM(eng, cfg.eos_token_id, cfg.pad_token_id)


def _restate(lg, prefix_ids, penalty, hold_eos):
    """RepetitionPenaltyLogitsProcessor then the MinLength hold on one fp32 row (HF's own expressions)."""
    s = lg.clone()
    if penalty != 1.0 and len(prefix_ids):
        idx = torch.tensor(sorted(set(prefix_ids)), dtype=torch.long)
        sc = s[idx]
        s[idx] = torch.where(sc < 0, sc * penalty, sc / penalty)
    if hold_eos is not None:
        s[hold_eos] = -float("inf")
    return s


def _check_greedy(cfg, eng, hf, emb, out, plain, penalty=1.0, min_new=0, eos=None):
    seq = out.sequences.cpu()
    assert torch.equal(seq, plain.cpu())
    L = seq.shape[1]
    assert len(out.scores) == len(out.logits) == L
    ref = hf_teacher_forced_logits(hf, emb, eng.embed_tokens, seq.to(dev()))
    scale = float(ref.abs().max())
    for t in range(L):
        lg, sc = out.logits[t].cpu(), out.scores[t].cpu()
        assert lg.shape == (seq.shape[0], cfg.vocab) and sc.dtype == torch.float32
        assert float((lg - ref[:, t]).abs().max()) <= LOGIT_TOL * scale, f"step {t}: raw logits off HF's forward"
        for b in range(seq.shape[0]):
            want = _restate(lg[b], seq[b, :t].tolist(), penalty, eos if t < min_new else None)
            assert torch.equal(sc[b], want), f"step {t} row {b}: processed scores differ from RepetitionPenalty -> MinLength"
            if eos is None or eos not in seq[b, :t].tolist():              # unfinished row: the selection took the argmax
                assert int(torch.argmax(sc[b])) == int(seq[b, t])


def test_greedy_penalty_min_length_eos_and_stop(tiny):
    cfg, w, eng, hf = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, 3, 41, cfg.vocab)
    kw = dict(max_length=S0 + 24, repetition_penalty=1.3, min_length=S0 + 3, eos_token_id=cfg.eos_token_id)
    first = lm.generate(inputs_embeds=emb, **kw).cpu()
    stop = [int(first[0, 12])]                                          # row 0's stop fires at or before column 12
    kw["stopping_criteria"] = [StoppingCriteriaSub([stop])]
    plain = lm.generate(inputs_embeds=emb, **kw)
    out = lm.generate(inputs_embeds=emb, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
    assert plain.shape[1] <= 13
    _check_greedy(cfg, eng, hf, emb, out, plain, penalty=1.3, min_new=3, eos=cfg.eos_token_id)
    # the C ABI at a slab stride that is not a multiple of 4 floats (every row unaligned in turn): same values
    n = plain.shape[1]
    ld = cfg.vocab + 3
    sl = torch.full((24, 3, ld), 7.0, device=dev())
    ll = torch.full((24, 3, ld), 7.0, device=dev())
    r = eng.generate(emb, max_length=S0 + 24, repetition_penalty=1.3, min_new_tokens=3, eos_token_id=cfg.eos_token_id,
                     pad_token_id=cfg.pad_token_id, stop_ids=stop, scores_out=sl, logits_out=ll, return_outputs=True)
    assert torch.equal(r["sequences"].cpu(), plain.cpu()) and r["n_generated"] == n
    for t in range(n):
        assert torch.equal(sl[t, :, :cfg.vocab], out.scores[t]) and torch.equal(ll[t, :, :cfg.vocab], out.logits[t])
    assert bool((sl[:, :, cfg.vocab:] == 7.0).all()) and bool((sl[n:] == 7.0).all())        # nothing outside the rows / steps


@pytest.mark.parametrize("B", [32, 33])
def test_plain_greedy_folded_and_two_row_tiles(tiny, B):
    cfg, w, eng, hf = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, B, 50 + B, cfg.vocab)
    kw = dict(max_length=S0 + 10, eos_token_id=-1)
    plain = lm.generate(inputs_embeds=emb, **kw)
    out = lm.generate(inputs_embeds=emb, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
    _check_greedy(cfg, eng, hf, emb, out, plain)
    assert all(torch.equal(a, b) for a, b in zip(out.scores, out.logits))
    assert torch.equal(lm.generate(inputs_embeds=emb, **kw), plain)        # a plain call after a capturing one: same tokens


def _hf_warp(s, top_k, top_p, min_keep):
    from transformers.generation.logits_process import TopKLogitsWarper, TopPLogitsWarper
    x = s.view(1, -1).clone()
    x = TopKLogitsWarper(top_k, min_tokens_to_keep=min_keep)(None, x)
    x = TopPLogitsWarper(top_p, min_tokens_to_keep=min_keep)(None, x)
    return x.view(-1)


def test_sampling_topk_topp_graph_and_eager(tiny):
    cfg, w, eng, hf = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, 4, 61, cfg.vocab)
    T, k, p, pen = 0.7, 50, 0.95, 1.2
    kw = dict(max_length=S0 + 140, do_sample=True, temperature=T, top_k=k, top_p=p, repetition_penalty=pen, eos_token_id=-1, seed=1234)
    outs = []
    for no_graph in (False, True):
        if no_graph:
            os.environ["SV_NO_GRAPH"] = "1"
        try:
            plain = lm.generate(inputs_embeds=emb, **kw)
            if not no_graph:
                assert eng.last_timing()["graph_steps"] == 32          # the multi-step graph replays
            out = lm.generate(inputs_embeds=emb, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
        finally:
            os.environ.pop("SV_NO_GRAPH", None)
        seq = out.sequences.cpu()
        assert torch.equal(seq, plain.cpu())
        assert len(out.scores) == len(out.logits) == seq.shape[1] == 140
        outs.append(out)
        for t in range(0, 140, 7):
            lg, sc = out.logits[t].cpu(), out.scores[t].cpu()
            for b in range(seq.shape[0]):
                pr = _restate(lg[b], seq[b, :t].tolist(), pen, None)
                fin = torch.isfinite(sc[b])
                assert bool(fin[seq[b, t]]), f"step {t} row {b}: the drawn token has no finite score"
                want = pr[fin] / T
                assert bool(((sc[b][fin] - want).abs() <= want.abs() * 2.4e-7).all()), "kept scores != penalised logits / T"
                ref = _hf_warp(pr / T, k, p, 1)
                diff = (fin != torch.isfinite(ref)).nonzero().flatten()
                if diff.numel():                                      # only at the top-p boundary (warp.h's relative slack)
                    probs = torch.softmax(torch.where(torch.isfinite(ref) | fin, pr / T, torch.full_like(pr, -float("inf"))), -1)
                    edge = float(probs[torch.isfinite(ref)].min())
                    assert diff.numel() <= 2 and all(abs(float(probs[i]) - edge) <= 1e-3 * edge for i in diff.tolist()), \
                        f"step {t} row {b}: kept set differs from HF TopK -> TopP beyond the boundary slack"
    for a, b in zip(outs[0].scores, outs[1].scores):
        assert torch.equal(a, b)                                        # graph replay == eager launches


def _beam_prefix(par, tok, t, r, nb):
    """ids generated by running beam row r before step t (search history of the engine)."""
    ids, x, b = [], r, r // nb
    for s in range(t - 1, -1, -1):
        ids.append(int(tok[s, x]))
        x = b * nb + int(par[s, x])
    return ids


@pytest.mark.parametrize("nb,lp,early,sample", [(2, 1.0, False, False), (3, 0.7, True, False), (3, 1.0, False, False),
                                                (2, 0.7, True, False), (2, 1.0, False, True)])
def test_beam_search_outputs(tiny, nb, lp, early, sample):
    cfg, w, eng, hf = tiny
    lm = _lm(eng, cfg)
    B, n_new, pen, min_new = 2, 20, 1.2, 2
    emb = _emb(eng, B, 70 + nb, cfg.vocab)
    kw = dict(max_length=S0 + n_new, num_beams=nb, length_penalty=lp, early_stopping=early, repetition_penalty=pen,
              min_length=S0 + min_new, eos_token_id=cfg.eos_token_id)
    if sample:
        kw.update(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=77)
    plain = lm.generate(inputs_embeds=emb, **kw)
    out = lm.generate(inputs_embeds=emb, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
    seq = out.sequences.cpu()
    assert torch.equal(seq, plain.cpu())
    L, R = seq.shape[1], B * nb
    assert len(out.scores) == len(out.logits) == L
    par, tok = eng.beam_history()
    for t in range(L):
        lg, sc = out.logits[t].cpu(), out.scores[t].cpu()
        assert lg.shape == (R, cfg.vocab)
        for r in range(R):
            s = _restate(torch.log_softmax(lg[r], -1), _beam_prefix(par, tok, t, r, nb), pen,
                         cfg.eos_token_id if t < min_new else None)
            if sample:
                s = _hf_warp(s / 0.8, 20, 0.9, 2)
            fin = torch.isfinite(sc[r])
            ref_fin = torch.isfinite(s)
            both = fin & ref_fin
            assert float((sc[r][both] - s[both]).abs().max()) <= 2e-6, f"step {t} row {r}: processed log-probs off"
            diff = int((fin != ref_fin).sum())
            assert diff == 0 or (sample and diff <= 2), f"step {t} row {r}: -inf pattern differs in {diff} tokens"
    bi = out.beam_indices.cpu()
    assert bi.shape == (B, L) and bi.dtype == torch.int64
    lengths = (bi >= 0).sum(1)
    for b in range(B):
        n = int(lengths[b])
        assert bool((bi[b, :n] >= b * nb).all()) and bool((bi[b, :n] < (b + 1) * nb).all()) and bool((bi[b, n:] == -1).all())
    ts = lm.compute_transition_scores(out.sequences, out.scores, out.beam_indices)
    rec = ts.sum(1).cpu() / lengths.float() ** lp
    assert torch.allclose(rec, out.sequences_scores.cpu(), rtol=1e-4, atol=0), (rec, out.sequences_scores)
    if not sample:
        # the standalone scorer fed the captured raw logits finishes with the same scores
        slab = out.logits[0]._base
        sc_ = HipBeamScorer(B, nb, cfg.vocab, n_new, cfg.eos_token_id, cfg.pad_token_id, length_penalty=lp, early_stopping=early,
                            repetition_penalty=pen, min_new_tokens=min_new)
        try:
            for t in range(n_new):
                if sc_.step(slab[t].contiguous())[0]:
                    break
            toks, scores = sc_.finalize()
        finally:
            sc_.close()
        assert torch.equal(toks, seq) and torch.equal(scores, out.sequences_scores.cpu())


def test_kept_graph_reads_each_calls_slabs(tiny):
    cfg, w, eng, hf = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, 3, 90, cfg.vocab)
    kw = dict(max_length=S0 + 150, repetition_penalty=1.3, eos_token_id=-1)
    plain = lm.generate(inputs_embeds=emb, **kw)
    a = lm.generate(inputs_embeds=emb, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
    a_copy = [x.clone() for x in a.scores]
    b = lm.generate(inputs_embeds=emb, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
    assert a.scores[0].data_ptr() != b.scores[0].data_ptr()
    assert all(torch.equal(x, y) for x, y in zip(a_copy, a.scores))       # the second call did not write into the first call's slab
    assert all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
    assert all(torch.equal(x, y) for x, y in zip(a.logits, b.logits))
    assert torch.equal(a.sequences, plain) and torch.equal(b.sequences, plain)
    assert torch.equal(lm.generate(inputs_embeds=emb, **kw), plain)


def test_starvector_1b_dims_real_vocab():
    cfg = dataclasses.replace(O.OracleConfig(), n_layer=2, vit_layers=1)
    w = O.make_weights(cfg, seed=95)
    eng = build_engine(cfg, w, max_batch=4, max_seq_len=64)
    try:
        hf = hf_decoder_bf16(cfg, w)
        lm = _lm(eng, cfg)
        emb = _emb(eng, 2, 96, 4000)
        kw = dict(max_length=S0 + 8, repetition_penalty=1.3, min_length=S0 + 2, eos_token_id=cfg.eos_token_id)
        plain = lm.generate(inputs_embeds=emb, **kw)
        out = lm.generate(inputs_embeds=emb, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
        assert out.scores[0].shape == (2, 49156)
        _check_greedy(cfg, eng, hf, emb, out, plain, penalty=1.3, min_new=2, eos=cfg.eos_token_id)
    finally:
        eng.close()
