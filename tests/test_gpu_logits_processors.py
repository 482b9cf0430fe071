"""-m gpu: HF's no_repeat_ngram_size / bad_words_ids / min_p on device (sv_generate_processed, processors.hip).

The ban kernel on its own against a torch restatement of the two processors (tests/test_logits_processors_host.py puts the same restatement
next to transformers' classes), then end to end: every token of a banned greedy call is the lowest-index argmax of that step's own raw
logits with the restatement's bans applied -- an exact check, independent of bf16 near-ties -- no n-gram repeats, the sampler never redraws a
banned id, min_p = 1 is greedy, and an all-zero processor set is sv_generate_shared bit for bit with the same captured step.

NoBadWords follows transformers: a sequence of L > 1 ids bans its last id from t >= L on (a sequence "longer than the context" is skipped)."""
import dataclasses
import os

import pytest
import torch
from safetensors.torch import load_file

from oracle import starvector_oracle as O
from starvector_amd import engine as E
from starvector_amd.model import HipCausalLM
from tests.gpu_util import bf, build_engine, dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -float("inf")
S0 = 4


# ---- the restatement, from the formulas (the copy of tests/test_logits_processors_host.py) ---------------------------------------------
def ngram_bans(g, n):
    """NoRepeatNGram(n) after the ids g[0 .. t-1]: { g[j+n-1] : 0 <= j <= t-n, g[j .. j+n-2] == g[t-n+1 .. t-1] }."""
    t = len(g)
    if n < 1 or t < n - 1:
        return set()
    suffix = g[t - n + 1:]                     # n - 1 ids (none for n = 1)
    return {g[j + n - 1] for j in range(0, t - n + 1) if g[j:j + n - 1] == suffix}


def bad_word_bans(g, words):
    """NoBadWords after g: a single id always; the last id of a longer sequence when t >= L and the last L - 1 ids are its prefix."""
    t, out = len(g), set()
    for w in words:
        L = len(w)
        if L == 1 or (t >= L and g[t - L + 1:] == list(w[:-1])):
            out.add(w[-1])
    return out


def restate(scores, hists, n=0, words=()):
    """scores [B, V] fp32, hists: one id list per row -> the processed rows (banned ids at -inf, everything else untouched)."""
    out = scores.clone()
    for b, g in enumerate(hists):
        ids = sorted(ngram_bans(list(g), n) | bad_word_bans(list(g), [list(w) for w in words]))
        if ids:
            out[b, torch.tensor(ids, dtype=torch.long)] = NEG
    return out


# ---- the operator ----------------------------------------------------------------------------------------------------------------------
V_OP = 49157                                  # odd tail; the operator's row stride is V rounded up to 4
ALPHABET = [0, 3, 4097, 49155, V_OP - 1]      # 5 ids: suffixes recur; the first and the last column of the row are among them
C_ID, D_ID = ALPHABET[2], ALPHABET[4]


def _history(t, n, gen):
    """t ids over the 5-id alphabet.  Short rows are constant C (at t = n the one window is both j = 0 and the last legal j).  Long rows are
    random, begin with C^(n-1) D -- the suffix matches at j = 0 and bans D -- and end with C^max(n, 8): the suffix C^(n-1) matches at the
    last legal j = t - n too (banning C), and the bad words' prefixes of up to 7 C's match."""
    if t < 40:
        return [C_ID] * t
    g = [ALPHABET[i] for i in torch.randint(0, 5, (t,), generator=gen).tolist()]
    g[:n] = [C_ID] * (n - 1) + [D_ID]
    run = max(n, 8)
    g[t - run:] = [C_ID] * run
    return g


BAD_WORDS = [[11],                                        # one id: always
             [C_ID, 20000],                               # prefix C matches every row that ends in C (t >= 2)
             [C_ID, C_ID, C_ID, 30001],                   # matches from t >= 4
             [D_ID, C_ID, C_ID, 30000],                   # fails in its FIRST id only: 30000 is never banned
             [C_ID] * 7 + [40000],                        # 8 ids: the long rows; longer than the history of every short row
             [C_ID, 3, 12345]]                            # prefix (C, 3): never the tail of these histories


@pytest.fixture(scope="module")
def op_logits():
    return torch.randn(4, V_OP, generator=torch.Generator().manual_seed(5)).to(dev())       # computed once, never modified


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_ban_kernel_is_the_restatement(op_logits, n):
    gen = torch.Generator().manual_seed(40 + n)
    lens = [0, max(n - 2, 0), n - 1, n, 130, 8191]
    hists = [_history(t, n, gen) for t in lens]
    cpu = op_logits.cpu()
    for rows in ([0, 1, 2, 3], [2, 3, 4, 5]):                 # B = 4 per launch
        hs = [hists[r] for r in rows]
        for words in ((), BAD_WORDS):
            got, pad = E.op_ban_tokens(op_logits, hs, no_repeat_ngram_size=n, bad_words_ids=list(words) or None)
            want = restate(cpu, hs, n=n, words=words)
            got = got.cpu()
            assert torch.equal(torch.isinf(got), torch.isinf(want)), f"n={n} rows {rows}: the banned set differs from the restatement's"
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"n={n} rows {rows}: a logit outside the banned set changed"
            assert bool((pad == 0).all())                  # nothing behind column V - 1
            for r, g in zip(range(4), hs):
                t = len(g)
                if t >= 40:                                # the designed matches: j = 0 bans D (n >= 2), the last legal j bans C
                    assert got[r, C_ID] == NEG and (n == 1 or got[r, D_ID] == NEG)
                    if words:
                        assert got[r, 20000] == NEG and got[r, 30001] == NEG and got[r, 40000] == NEG
                if words:
                    assert got[r, 11] == NEG and got[r, 30000] != NEG and got[r, 12345] != NEG
                    assert (got[r, 40000] == NEG) == (t >= 8) and (got[r, 20000] == NEG) == (t >= 2)
                if t < n or (n == 1 and t == 0):
                    assert int(torch.isinf(got[r]).sum()) == len(bad_word_bans(g, [list(w) for w in words]))      # no n-gram ban yet
    assert torch.equal(op_logits.cpu(), cpu)                   # the operator works on its own copy


def test_ban_kernel_without_any_processor_changes_nothing(op_logits):
    got, pad = E.op_ban_tokens(op_logits, [[C_ID] * 9] * 4)
    assert torch.equal(got.view(torch.int32), op_logits.view(torch.int32))


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """The random-init tiny decoder of tests/test_gpu_generate_outputs.py: such a model loops (on the CPU the oracle's greedy_generate over
    these prompts repeats 6-9 bigrams per row within 48 tokens, '372 372 372 372' from column 3 on)."""
    cfg = dataclasses.replace(O.OracleConfig.tiny(), n_positions=256)
    w = O.make_weights(cfg, seed=31)
    eng = build_engine(cfg, w, max_batch=8, max_seq_len=160)
    ids = torch.randint(0, cfg.vocab, (3, S0), generator=torch.Generator().manual_seed(41))
    yield cfg, eng, eng.embed_tokens(ids.to(dev()))
    eng.close()


def _ngrams(row, n):
    return [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]


def test_greedy_tokens_are_the_argmax_of_the_banned_raw_logits(tiny):
    cfg, eng, emb = tiny
    lm = HipCausalLM(eng, cfg.eos_token_id, cfg.pad_token_id)
    kw = dict(max_length=S0 + 48, eos_token_id=-1)
    base = lm.generate(inputs_embeds=emb, **kw).cpu()
    for b in range(3):                                              # precondition: without the argument every row repeats a bigram
        bi = _ngrams(base[b].tolist(), 2)
        assert len(set(bi)) < len(bi), f"row {b} does not loop: the test would show nothing"
    # row 0's bigram at columns 1-2: nothing else is banned before it, so the bad word bites at t = 2 (at t = 1 a 2-id sequence is still
    # "longer than the context"); and one id of row 2 that row 0 does not start with
    bad = [int(base[0, 1]), int(base[0, 2])]
    single = next(x for x in base[2].tolist() if x not in base[0, :3].tolist())
    args = dict(no_repeat_ngram_size=2, bad_words_ids=[bad, [single]])
    out = lm.generate(inputs_embeds=emb, return_dict_in_generate=True, output_logits=True, output_scores=True, **args, **kw)
    seq = out.sequences.cpu()
    assert seq.shape == (3, 48) and len(out.logits) == len(out.scores) == 48
    for t in range(48):
        raw, sc = out.logits[t].cpu(), out.scores[t].cpu()
        want = restate(raw, seq[:, :t].tolist(), n=2, words=args["bad_words_ids"])
        assert not bool(torch.isinf(raw).any()), f"step {t}: output_logits must stay raw"
        assert torch.equal(sc.view(torch.int32), want.view(torch.int32)), f"step {t}: output_scores are not the raw row with the bans at -inf"
        assert torch.equal(torch.argmax(want, dim=-1), seq[:, t]), f"step {t}: a token is not the lowest-index argmax of the banned row"
    for b in range(3):
        row = seq[b].tolist()
        assert len(set(_ngrams(row, 2))) == 47, f"row {b} repeats a bigram"
        assert tuple(bad) not in _ngrams(row, 2)[1:] and single not in row      # (columns 0-1 are out of a 2-id bad word's reach, as in HF)
    assert torch.equal(seq[0, :2], base[0, :2]) and seq[0, 2] != base[0, 2] and not torch.equal(seq[2], base[2])      # both bad words changed a token
    # the call without per-step outputs (its own captured step) and the C entry point through HipEngine: the same tokens
    assert torch.equal(lm.generate(inputs_embeds=emb, **args, **kw).cpu(), seq)
    assert torch.equal(eng.generate_processed(emb, S0 + 48, eos_token_id=-1, pad_token_id=cfg.pad_token_id, **args).cpu(), seq)
    assert not eng.step_plan()["greedy_in_lm_head"]               # a ban takes the separate selection launch


def test_bans_inside_the_multi_step_graph_ragged_and_shared(tiny):
    """140 new tokens: the step (with its ban launch) is captured 32 times into one graph; plain launches give the same tokens; the ragged
    and the shared-prompt forms carry the bans too."""
    cfg, eng, emb = tiny
    kw = dict(eos_token_id=-1, pad_token_id=cfg.pad_token_id, no_repeat_ngram_size=3)
    got = eng.generate_processed(emb, S0 + 140, **kw).cpu()
    assert eng.last_timing()["graph_steps"] == 32
    for b in range(3):
        assert len(set(_ngrams(got[b].tolist(), 3))) == 138, f"row {b} repeats a trigram"
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        eager = eng.generate_processed(emb, S0 + 140, **kw).cpu()
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    assert torch.equal(eager, got)
    assert not torch.equal(eng.generate(emb, S0 + 140, eos_token_id=-1, pad_token_id=cfg.pad_token_id).cpu(), got)
    seqs = [emb[0, :3].contiguous(), emb[1].contiguous(), emb[2, :2].contiguous()]
    rag = eng.generate_processed(seqs, S0 + 40, **kw).cpu()
    shared = eng.generate_processed(seqs, S0 + 40, n_samples=2, **kw).cpu()
    assert rag.shape == (3, 40) and shared.shape == (6, 40)
    for b in range(3):
        assert len(set(_ngrams(rag[b].tolist(), 3))) == 38
        assert torch.equal(shared[2 * b], rag[b]) and torch.equal(shared[2 * b + 1], rag[b])
    assert torch.equal(rag[1], got[1, :40])                        # the full-length row is its rectangular self
    with pytest.raises(ValueError, match="num_beams"):
        eng.generate_processed(emb, S0 + 8, num_beams=2, **kw)


def test_sampling_never_redraws_a_banned_id(tiny):
    cfg, eng, emb = tiny
    lm = HipCausalLM(eng, cfg.eos_token_id, cfg.pad_token_id)
    kw = dict(max_length=S0 + 32, eos_token_id=-1, do_sample=True, top_k=4, seed=77)
    plain = lm.generate(inputs_embeds=emb, **kw).cpu()
    assert any(len(set(plain[b].tolist())) < 32 for b in range(3))           # precondition: the unbanned sampler does redraw ids
    out = lm.generate(inputs_embeds=emb, no_repeat_ngram_size=1, return_dict_in_generate=True, output_scores=True, **kw)
    seq = out.sequences.cpu()
    for b in range(3):
        assert len(set(seq[b].tolist())) == 32, f"row {b} drew an id twice"
    for t in (1, 9, 31):                                                     # output_scores: every earlier id at -inf, the drawn one finite
        sc = out.scores[t].cpu()
        for b in range(3):
            assert bool(torch.isinf(sc[b, seq[b, :t]]).all()) and bool(torch.isfinite(sc[b, seq[b, t]]))
    assert torch.equal(lm.generate(inputs_embeds=emb, no_repeat_ngram_size=1, **kw).cpu(), seq)


def test_min_p_one_is_greedy():
    """tests/golden/tiny_b3: a fitted embedding table whose greedy stream has a top-1 / top-2 margin of a quarter of the logit scale -- no
    tie at the top, so min_p = 1 (only p >= p_max survives) leaves the sampler exactly one token per step."""
    g = load_file(os.path.join(ROOT, "tests", "golden", "tiny_b3.safetensors"))
    seed, B, n_new = [int(x) for x in g["meta"]]
    cfg = O.OracleConfig.tiny()
    w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)
    eng = build_engine(cfg, w, max_batch=B, max_seq_len=64)
    lm = HipCausalLM(eng, cfg.eos_token_id, cfg.pad_token_id)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    kw = dict(inputs_embeds=emb, max_length=emb.shape[1] + n_new)
    greedy = lm.generate(**kw).cpu()
    assert torch.equal(greedy, g["tokens"][:, :greedy.shape[1]])                # precondition: the designed stream
    samp = dict(do_sample=True, temperature=5.0, top_k=50, top_p=0.95, seed=5)
    assert not torch.equal(lm.generate(**kw, **samp).cpu(), greedy)             # precondition: the sampler alone leaves it
    assert torch.equal(lm.generate(**kw, min_p=1.0, **samp).cpu(), greedy)
    out = lm.generate(**kw, min_p=1.0, return_dict_in_generate=True, output_scores=True, **samp)
    assert torch.equal(out.sequences.cpu(), greedy)
    for t, s in enumerate(out.scores):                                          # output_scores: min_p's removals at -inf, as in HF
        for b in range(B):
            if cfg.eos_token_id not in greedy[b, :t].tolist():
                assert int(torch.isfinite(s[b]).sum()) == 1
    assert torch.equal(lm.generate(**kw, min_p=0.0, **samp).cpu(), lm.generate(**kw, **samp).cpu())
    eng.close()


# ---- neutrality --------------------------------------------------------------------------------------------------------------------------
def test_all_zero_processors_are_generate_shared_bit_for_bit(tiny):
    cfg, eng, emb = tiny
    sampling = dict(do_sample=True, temperature=0.9, top_p=0.95, top_k=40, repetition_penalty=1.2, seed=1234)
    for kw in (dict(), sampling):
        kw = dict(kw, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
        want = eng.generate_shared(emb, S0 + 140, n_samples=2, **kw).cpu()
        t_want, p_want = eng.last_timing(), eng.step_plan()
        got = eng.generate_processed(emb, S0 + 140, n_samples=2, **kw).cpu()
        t_got, p_got = eng.last_timing(), eng.step_plan()
        assert torch.equal(got, want)
        assert t_got["graph_steps"] == t_want["graph_steps"] == 32 and t_got["decode_steps"] == t_want["decode_steps"]
        assert p_got == p_want                                    # the captured step is the plain call's: no node added, the same fused launches
    assert p_want["graph_kernel_nodes"] > 0
    seqs = [emb[0, :3].contiguous(), emb[1].contiguous()]
    assert torch.equal(eng.generate_processed(seqs, S0 + 20, **kw).cpu(), eng.generate_ragged(seqs, S0 + 20, **kw).cpu())
    assert torch.equal(eng.generate_processed(emb, S0 + 20, **kw).cpu(), eng.generate(emb, S0 + 20, **kw).cpu())
    # a greedy call ignores min_p, a ban after it adds exactly one kernel node to the separate-selection step
    eng.generate(emb, S0 + 20, repetition_penalty=1.1, eos_token_id=-1)
    nodes = eng.step_plan()["graph_kernel_nodes"]
    eng.generate_processed(emb, S0 + 20, no_repeat_ngram_size=2, repetition_penalty=1.1, eos_token_id=-1)
    assert eng.step_plan()["graph_kernel_nodes"] == nodes + 1
