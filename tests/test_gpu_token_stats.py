"""-m gpu: per-token log-prob, processed log-prob and entropy from the decode loop (sv_generate_stats, sampling.hip token_stats_kernel).
The tokens are those of the call without statistics; the three values are checked against the engine's existing capture path
(output_scores / output_logits) plus torch in float64, and against the scoring forward (sv_forward_logprobs)."""
import dataclasses
import os

import pytest
import torch

from oracle import starvector_oracle as O
from starvector_amd.model import HipCausalLM, StoppingCriteriaSub
from tests.gpu_util import bf, build_engine, dev
from tests.test_gpu_e2e import LOGIT_TOL

pytestmark = pytest.mark.gpu
S0 = 4
KEYS = ("token_logprobs", "token_logprobs_processed", "token_entropies")


@pytest.fixture(scope="module")
def tiny():
    cfg = dataclasses.replace(O.OracleConfig.tiny(), n_positions=256)      # room for > 64 steps
    w = O.make_weights(cfg, seed=31)
    eng = build_engine(cfg, w, max_batch=40, max_seq_len=160)
    yield cfg, w, eng
    eng.close()


def _emb(eng, B, seed, V):
    ids = torch.randint(0, V, (B, S0), generator=torch.Generator().manual_seed(seed))
    return eng.embed_tokens(ids.to(dev()))


def _lm(eng, cfg):
    return HipCausalLM(eng, cfg.eos_token_id, cfg.pad_token_id)


def _stats(lm, emb, **kw):
    return lm.generate(inputs_embeds=emb, return_dict_in_generate=True, output_token_logprobs=True, **kw)


def _lengths(seq, eos):
    """columns of each row up to and including the token that ended it (its first EOS; the call's last column otherwise)"""
    n = seq.shape[1]
    is_eos = seq == eos
    return torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, torch.full((seq.shape[0],), n, device=seq.device))


def _entropy(logp):
    p = logp.exp()
    return -torch.where(p > 0, p * logp, torch.zeros_like(p)).sum(-1)


def _dev_err(a, ref):
    fin = torch.isfinite(ref)
    assert torch.equal(a.double()[~fin], ref[~fin]), "non-finite entries differ"
    return float((a.double()[fin] - ref[fin]).abs().max())


def _check_against_capture(name, out, eos, T):
    """logprob_processed against float64 log_softmax(out.scores) at the emitted token, logprob and entropy against float64
    log_softmax(out.logits / T); tolerance = 4 x the deviation of torch's own float32 log_softmax (entropy) from float64 on the same rows.
    Returns the tolerance of the log-probs."""
    seq = out.sequences
    R, L = seq.shape
    lens = _lengths(seq, eos)
    live = torch.arange(L, device=seq.device).unsqueeze(0) < lens.unsqueeze(1)                      # [R, L]
    lp, lpp, ent = out["token_logprobs"], out["token_logprobs_processed"], out["token_entropies"]
    assert lp.shape == lpp.shape == ent.shape == (R, L) and lp.dtype == torch.float32 and lp.is_cuda
    for v in (lp, lpp, ent):
        assert bool(torch.isfinite(v).all())
        assert bool((v[~live] == 0).all()), "a finished row must read exactly 0"
    assert bool((lp <= 0).all()) and bool((lpp <= 0).all()) and bool((ent >= 0).all())
    scores = torch.stack(out.scores).transpose(0, 1)                                                # [R, L, V] fp32, removed ids at -inf
    x32 = torch.stack(out.logits).transpose(0, 1) / T                                               # fp32 division, like the kernel's
    pick = seq.unsqueeze(-1)
    res = {}
    for what, rows, got in (("processed", scores, lpp), ("raw", x32, lp)):
        ref64 = torch.log_softmax(rows.double(), -1)
        t32 = torch.log_softmax(rows, -1)
        tol = 4.0 * _dev_err(t32[live], ref64[live])
        err = float((got.double() - ref64.gather(-1, pick).squeeze(-1))[live].abs().max())
        print(f"[{name}] logprob ({what}): |kernel - f64| {err:.3e} (allowed {tol:.3e} = 4 x torch fp32's own deviation)")
        res[what] = (err, tol, ref64, t32)
    e64, e32 = _entropy(res["raw"][2]), _entropy(res["raw"][3])
    tol_ent = 4.0 * float((e32.double() - e64)[live].abs().max())
    err_ent = float((ent.double() - e64)[live].abs().max())
    print(f"[{name}] entropy: |kernel - f64| {err_ent:.3e} (allowed {tol_ent:.3e})")
    assert res["processed"][1] > 0 and res["raw"][1] > 0 and tol_ent > 0
    assert res["processed"][0] <= res["processed"][1], name
    assert res["raw"][0] <= res["raw"][1], name
    assert err_ent <= tol_ent, name
    return max(res["raw"][1], res["processed"][1]), live


MODES = {
    "greedy": dict(max_length=S0 + 20, eos_token_id=-1),
    "greedy_penalty_minlen_eos_stop": dict(max_length=S0 + 24, repetition_penalty=1.3, min_length=S0 + 3),
    "sample_topk5_topp08": dict(max_length=S0 + 20, do_sample=True, temperature=0.7, top_k=5, top_p=0.8, seed=61),
    "sample_topk5_topp08_eager": dict(max_length=S0 + 20, do_sample=True, temperature=0.7, top_k=5, top_p=0.8, seed=61),
    "sample_open": dict(max_length=S0 + 20, do_sample=True, temperature=0.7, top_k=0, top_p=1.0, seed=7),
    "min_p": dict(max_length=S0 + 20, do_sample=True, temperature=0.5, top_k=0, top_p=1.0, min_p=0.6, seed=8),
    "no_repeat_ngram": dict(max_length=S0 + 20, no_repeat_ngram_size=2, eos_token_id=-1),
    "bad_words": dict(max_length=S0 + 20, eos_token_id=-1),
    "num_return_sequences": dict(max_length=S0 + 20, do_sample=True, temperature=0.9, top_k=20, top_p=0.9, seed=9, num_return_sequences=3),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_tokens_unaffected_and_values_match_the_capture(tiny, mode):
    """1. tokens and n_generated with statistics on = those of the plain call, and a plain call afterwards still equals the first one;
    2. + 3. the three values against the capture path (the same call with output_scores / output_logits) in float64."""
    cfg, w, eng = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, 4 if mode != "num_return_sequences" else 2, 61, cfg.vocab)
    kw = dict(MODES[mode])
    eos = kw.get("eos_token_id", cfg.eos_token_id)
    if mode == "greedy_penalty_minlen_eos_stop":
        first = lm.generate(inputs_embeds=emb, **kw).cpu()
        kw["stopping_criteria"] = [StoppingCriteriaSub([[int(first[0, 12])]])]      # row 0's stop fires at or before column 12: not a chunk boundary
    if mode == "bad_words":
        first = lm.generate(inputs_embeds=emb, **kw).cpu()
        kw["bad_words_ids"] = [[int(first[0, 1])], [int(first[1, 2]), int(first[1, 3])]]
    if mode.endswith("_eager"):
        os.environ["SV_NO_GRAPH"] = "1"
    try:
        plain = lm.generate(inputs_embeds=emb, **kw)
        st = _stats(lm, emb, **kw)
        both = _stats(lm, emb, output_scores=True, output_logits=True, **kw)
        again = lm.generate(inputs_embeds=emb, **kw)
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    assert torch.equal(st.sequences, plain) and torch.equal(both.sequences, plain) and torch.equal(again, plain)
    if mode == "greedy_penalty_minlen_eos_stop":
        assert plain.shape[1] <= 13                                               # ended on *done inside the first polling chunk
    if mode == "bad_words":
        assert not torch.equal(plain.cpu(), first)
    for k in KEYS:                                                                # with or without the slabs: the same bits
        assert torch.equal(st[k], both[k]), k
    T = kw.get("temperature", 1.0) if kw.get("do_sample") else 1.0
    tol, live = _check_against_capture(mode, both, eos, T)
    lp, lpp = both["token_logprobs"], both["token_logprobs_processed"]
    if mode in ("greedy", "sample_open"):
        assert float((lp - lpp).abs().max()) <= tol                               # nothing is removed or rewritten: the two agree
    if mode.startswith("sample_topk5"):
        # the seed is chosen on the CPU oracle: the first-token distribution of row 0 puts < 10 % of its mass on its five best ids, so
        # the kept set's renormalisation lifts the processed log-prob by > log(10) there
        ids = torch.randint(0, cfg.vocab, (4, S0), generator=torch.Generator().manual_seed(61))
        lg0, _ = O.decoder_prefill(w, cfg, w[O.embed_key(cfg)].float()[ids], mode="bf16")
        assert float(torch.softmax(lg0[0].float() / T, -1).topk(5).values.sum()) < 0.1
        assert float(lp[0, 0]) < float(lpp[0, 0]) - 1.0 and bool((lp[live] <= lpp[live] + tol).all())


def test_agrees_with_the_scoring_forward(tiny):
    """4. sv_forward_logprobs over prompt + the generated tokens with the same T gives `logprob` within 2 x LOGIT_TOL x max|logit| (two bf16
    passes over the same weights: the decode loop and the prompt pass)."""
    cfg, w, eng = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, 3, 71, cfg.vocab)
    for kw, T in ((dict(eos_token_id=-1), 1.0), (dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, seed=5), 0.7)):
        out = _stats(lm, emb, max_length=S0 + 24, output_logits=True, **kw)
        seq = out.sequences
        L = seq.shape[1]
        live = torch.arange(L, device=seq.device).unsqueeze(0) < _lengths(seq, kw.get("eos_token_id", cfg.eos_token_id)).unsqueeze(1)
        full = torch.cat([emb, eng.embed_tokens(seq[:, :-1])], 1)                                   # row S0 - 1 + j predicts seq[:, j]
        sc = eng.forward_logprobs(full, seq.to(torch.int32), num_logits_to_keep=L, temperature=T, entropy=True)
        tol = 2 * LOGIT_TOL * float(torch.stack(out.logits).abs().max())
        err = float((sc.logprobs - out["token_logprobs"])[live].abs().max())
        err_e = float((sc.entropy - out["token_entropies"])[live].abs().max())
        print(f"[scoring forward T={T}] |logprob diff| {err:.3e}, |entropy diff| {err_e:.3e} (allowed {tol:.3e})")
        assert tol > 0 and err <= tol and err_e <= tol          # the entropy is score.hip's definition on the same two passes


def test_a_row_that_finished_reads_zero_from_the_next_column_on(tiny):
    """2. the EOS id is a token that row 1 alone emits in the open-ended call, early: row 1 ends there while the other rows go on, and
    every column behind it is exactly 0 in all three outputs (asserted in _check_against_capture; here: that such columns exist)"""
    cfg, w, eng = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, 4, 61, cfg.vocab)
    for kw in (dict(), dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.8, seed=61)):
        first = lm.generate(inputs_embeds=emb, max_length=S0 + 20, eos_token_id=-1, **kw).cpu()
        others = set(first[[0, 2, 3]].flatten().tolist())
        eos = next(int(t) for t in first[1, :12].tolist() if int(t) not in others)
        kw.update(max_length=S0 + 20, eos_token_id=eos)
        plain = lm.generate(inputs_embeds=emb, **kw)
        out = _stats(lm, emb, output_scores=True, output_logits=True, **kw)
        assert torch.equal(out.sequences, plain)
        lens = _lengths(plain, eos)
        assert int(lens[1]) <= 12 and plain.shape[1] == 20                              # the call went on after row 1 had ended
        _, live = _check_against_capture("row 1 ends early", out, eos, kw.get("temperature", 1.0))
        assert bool((~live).any()) and bool(live[1, :int(lens[1])].all()) and not bool(live[1, int(lens[1]):].any())
        assert bool((out["token_logprobs"][1, :int(lens[1])] < 0).all()) and bool((out["token_entropies"][1, int(lens[1]):] == 0).all())


@pytest.mark.parametrize("B", [1, 33, 40])
def test_row_counts(tiny, B):
    """5. one row, two row tiles, the engine's whole batch"""
    cfg, w, eng = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, B, 50 + B, cfg.vocab)
    for kw in (dict(eos_token_id=-1), dict(do_sample=True, temperature=0.8, top_k=5, top_p=0.9, seed=3)):
        kw["max_length"] = S0 + 8
        plain = lm.generate(inputs_embeds=emb, **kw)
        out = _stats(lm, emb, output_scores=True, output_logits=True, **kw)
        assert torch.equal(out.sequences, plain)
        _check_against_capture(f"B={B} {'sample' if kw.get('do_sample') else 'greedy'}", out, kw.get("eos_token_id", cfg.eos_token_id),
                               kw.get("temperature", 1.0))


def test_vocab_not_a_multiple_of_four():
    """5. OracleConfig.tiny_v2(): vocab 517, the tail lanes of the row sweeps"""
    cfg = O.OracleConfig.tiny_v2()
    assert cfg.vocab % 4 != 0
    eng = build_engine(cfg, O.make_weights(cfg, seed=33), max_batch=4, max_seq_len=64)
    try:
        lm = _lm(eng, cfg)
        emb = _emb(eng, 3, 34, cfg.vocab)
        for kw in (dict(repetition_penalty=1.2), dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.8, seed=2)):
            kw.update(max_length=S0 + 12, eos_token_id=-1)
            plain = lm.generate(inputs_embeds=emb, **kw)
            out = _stats(lm, emb, output_scores=True, output_logits=True, **kw)
            assert torch.equal(out.sequences, plain)
            _check_against_capture("vocab 517", out, -1, kw.get("temperature", 1.0) if kw.get("do_sample") else 1.0)
    finally:
        eng.close()


def test_starvector_1b_dims_real_vocab():
    """5. StarVector-1B dims, vocab 49156: 48 scores per thread plus a remainder"""
    cfg = dataclasses.replace(O.OracleConfig(), n_layer=2, vit_layers=1)
    eng = build_engine(cfg, O.make_weights(cfg, seed=95), max_batch=4, max_seq_len=64)
    try:
        lm = _lm(eng, cfg)
        emb = _emb(eng, 2, 96, 4000)
        for kw in (dict(repetition_penalty=1.3, min_length=S0 + 2), dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, seed=4)):
            kw.update(max_length=S0 + 8, eos_token_id=cfg.eos_token_id)
            plain = lm.generate(inputs_embeds=emb, **kw)
            out = _stats(lm, emb, output_scores=True, output_logits=True, **kw)
            assert torch.equal(out.sequences, plain) and out.scores[0].shape == (2, 49156)
            _check_against_capture("1B dims", out, cfg.eos_token_id, kw.get("temperature", 1.0) if kw.get("do_sample") else 1.0)
    finally:
        eng.close()


def test_more_than_64_steps_cross_the_multi_step_graph_and_the_polling_chunks(tiny):
    """5. 140 steps: the 32-step graph replays and the host polls between chunks (an EOS id inside the vocabulary)"""
    cfg, w, eng = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, 4, 81, cfg.vocab)
    kw = dict(max_length=S0 + 140, do_sample=True, temperature=0.7, top_k=50, top_p=0.95, repetition_penalty=1.2, seed=1234)
    plain = lm.generate(inputs_embeds=emb, **kw)
    assert eng.last_timing()["graph_steps"] == 32
    out = _stats(lm, emb, output_scores=True, output_logits=True, **kw)
    assert eng.last_timing()["graph_steps"] == 32
    assert torch.equal(out.sequences, plain) and plain.shape[1] > 64
    _check_against_capture("140 steps", out, cfg.eos_token_id, 0.7)


def test_kept_graph_writes_each_calls_tensors(tiny):
    """6. the captured statistics step reaches the buffers through the device descriptor: a second call (the kept graph) and a call with
    another seed each fill their own tensors"""
    cfg, w, eng = tiny
    lm = _lm(eng, cfg)
    emb = _emb(eng, 3, 90, cfg.vocab)
    kw = dict(max_length=S0 + 70, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, eos_token_id=-1)
    plain = lm.generate(inputs_embeds=emb, seed=11, **kw)
    a = _stats(lm, emb, seed=11, **kw)
    a_copy = {k: a[k].clone() for k in KEYS}
    b = _stats(lm, emb, seed=11, **kw)                                              # same key: the kept graph
    c = _stats(lm, emb, seed=12, **kw)                                              # another seed: another random stream
    c_copy = {k: c[k].clone() for k in KEYS}
    a2 = _stats(lm, emb, seed=11, **kw)
    assert torch.equal(a.sequences, plain) and torch.equal(b.sequences, plain) and not torch.equal(c.sequences, plain)
    for k in KEYS:
        assert len({a[k].data_ptr(), b[k].data_ptr(), c[k].data_ptr()}) == 3
        assert torch.equal(a[k], a_copy[k]) and torch.equal(c[k], c_copy[k])        # later calls did not write into earlier calls' tensors
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], a2[k]) and not torch.equal(a[k], c[k])
    assert torch.equal(lm.generate(inputs_embeds=emb, seed=11, **kw), plain)        # and the plain step is the plain step again
    assert torch.equal(lm.generate(inputs_embeds=emb, seed=12, **kw), c.sequences)


def test_error_paths_name_the_cause(tiny):
    """7. ld < max_new, all three pointers NULL, num_beams = 2"""
    import ctypes as C

    from starvector_amd import _lib
    cfg, w, eng = tiny
    emb = _emb(eng, 2, 5, cfg.vocab)
    n = C.c_int32(0)
    out = torch.zeros(2, 10, dtype=torch.int64, device=dev())
    buf = torch.full((2, 10), 7.0, device=dev())
    sp = _lib.SvSampling(max_length=S0 + 10, num_beams=1, temperature=1.0, top_p=1.0, eos_token_id=-1)
    ptr = C.c_void_p(buf.data_ptr())

    def call(ts, sp=sp):
        rc = eng.lib.sv_generate_stats(eng._h, C.c_void_p(emb.data_ptr()), 2, None, S0, 1, C.byref(sp), None, None, C.byref(ts),
                                       C.c_void_p(out.data_ptr()), C.byref(n), None)
        return rc, eng.lib.sv_last_error().decode()

    rc, msg = call(_lib.SvTokenStats(ptr, ptr, ptr, 9))
    assert rc == -22 and "ld 9" in msg and "max_new 10" in msg
    rc, msg = call(_lib.SvTokenStats(None, None, None, 10))
    assert rc == -22 and "all NULL" in msg
    rc, msg = call(_lib.SvTokenStats(ptr, ptr, ptr, 10), _lib.SvSampling(max_length=S0 + 10, num_beams=2, temperature=1.0, top_p=1.0))
    assert rc == -22 and "num_beams 2" in msg
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())                                                 # nothing was written
    with pytest.raises(ValueError, match="num_beams > 1"):
        eng.generate(emb, max_length=S0 + 10, num_beams=2, token_stats=True)
    with pytest.raises(NotImplementedError, match="output_token_logprobs with num_beams > 1"):
        _stats(_lm(eng, cfg), emb, max_length=S0 + 10, num_beams=2)
    # one pointer alone, at a stride wider than max_new: only its [rows][:n] cells change
    rc, msg = call(_lib.SvTokenStats(None, None, ptr, 10))
    torch.cuda.synchronize()
    assert rc == 0 and n.value == 10 and bool((buf > 0).all()) and bool((buf < 7.0).all()), msg


def test_ragged_and_shared_forms(tiny):
    """8. (engine level) ragged prompts, 3 samples each, from one prompt pass: the rows of the prompts repeated, bit for bit"""
    cfg, w, eng = tiny
    ids = torch.randint(0, cfg.vocab, (2, 9), generator=torch.Generator().manual_seed(17)).to(dev())
    prompts = [eng.embed_tokens(ids[:1, :9])[0], eng.embed_tokens(ids[1:, :5])[0]]
    kw = dict(max_length=9 + 16, do_sample=True, temperature=0.9, top_k=20, top_p=0.9, seed=21, eos_token_id=cfg.eos_token_id,
              pad_token_id=cfg.pad_token_id, token_stats=True)
    shared = eng.generate_shared(prompts, n_samples=3, **kw)
    repeated = eng.generate_ragged([p for p in prompts for _ in range(3)], **kw)
    assert shared["sequences"].shape[0] == 6 and torch.equal(shared["sequences"], repeated["sequences"])
    for k in KEYS:
        assert torch.equal(shared[k], repeated[k]), k
    assert bool((shared["token_logprobs"][:, 0] < 0).all())


def test_grpo_rollout_returns_logprobs_entropies_and_mask():
    """8. generate_im2svg_grpo(..., num_return_sequences=4, return_logprobs=True) on the tiny model"""
    import starvector_amd as sva
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=41)
    scfg = sva.StarVectorConfig(image_size=cfg.image_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.n_layer,
                                num_attention_heads=cfg.n_head, vocab_size=cfg.vocab - 4, n_inner=cfg.n_inner,
                                n_positions=cfg.n_positions, max_length=cfg.n_positions, vit_width=cfg.vit_width,
                                vit_layers=cfg.vit_layers, vit_heads=cfg.vit_heads, max_batch=8)
    model = sva.StarVectorForCausalLM(scfg, state_dict={k: v.to(torch.bfloat16) for k, v in w.items()})
    model.eval()
    try:
        batch = {"image": bf(O.synthetic_images(2, cfg.image_size, seed=5))}
        S = model.model.query_length + 4
        kw = dict(max_length=S + 40, num_return_sequences=4, temperature=0.9, top_p=0.9, seed=77)
        ref = model.model.generate_im2svg_grpo(batch, **kw)
        assert list(ref) == ["raw_svg", "outputs", "inputs_embeds"]
        r1 = model.model.generate_im2svg_grpo(batch, return_logprobs=True, **kw)
        r2 = model.model.generate_im2svg_grpo(batch, return_logprobs=True, share_prompt=False, **kw)
        assert list(r1) == ["raw_svg", "outputs", "inputs_embeds", "logprobs", "entropies", "completion_mask"]
        assert torch.equal(r1["outputs"], ref["outputs"]) and torch.equal(r2["outputs"], ref["outputs"]) and r1["raw_svg"] == ref["raw_svg"]
        new = r1["outputs"][:, 4:]
        assert r1["logprobs"].shape == r1["entropies"].shape == r1["completion_mask"].shape == new.shape and new.shape[0] == 8
        for k in ("logprobs", "entropies", "completion_mask"):
            assert torch.equal(r1[k], r2[k]), k                                     # the prompts repeated 4 times: bit for bit
        lens = _lengths(new, model.model.svg_transformer.transformer.eos_token_id)
        assert torch.equal(r1["completion_mask"].sum(1), lens)
        m = r1["completion_mask"].bool()
        assert bool(m[:, 0].all())
        assert bool((r1["logprobs"][m] < 0).all()) and bool((r1["logprobs"][~m] == 0).all()) and bool((r1["entropies"][~m] == 0).all())
    finally:
        model.engine.close()
