"""GPU: prompt-lookup decoding with the call's own selection (sv_generate_lookup_sampled) at engine level.  The contract is equality, token
for token and per seed, with the plain call on the same engine -- `generate` / `generate_ragged` with the same do_sample / temperature /
top_k / top_p / seed / repetition_penalty -- whatever the drafts are.  Forced all-right drafts are what catch a row that draws with another
(seed, step, row) triple than the plain call's, or whose seen set misses the drafts in front of it: every emitted token but one per step
then comes from a draft row."""
import math
import os

import pytest
import torch

from tests.test_gpu_lookup import _case, _restated_counts, _tiny_random

pytestmark = pytest.mark.gpu

S1 = dict(do_sample=True, top_k=50, top_p=0.9, temperature=1.0, seed=1234)
S2 = dict(do_sample=True, top_k=0, top_p=0.95, temperature=0.7, seed=1234)
PEN = dict(repetition_penalty=1.3)
# the issue's matrix: both sampler settings, then the same with the penalty for do_sample 0 and 1
MODES = {"topk50": S1, "scan": S2, "greedy_pen": PEN, "topk50_pen": {**S1, **PEN}, "scan_pen": {**S2, **PEN}}


@pytest.mark.parametrize("name", ["tiny_b3", "tiny_stop", "tiny_minlen", "tiny_v2_b2", "tiny_v2_window"])
def test_natural_lookup_equals_the_plain_call_on_the_goldens(name):
    """EOS, the row-0 stop, the min-length hold, a page crossing with RoPE, the window edge"""
    eng, emb, kw, _hf = _case(name)
    for mode, sel in MODES.items():
        plain = eng.generate(emb, **sel, **kw).cpu()
        for K in (1, 3, 7):
            got, counts = eng.generate_lookup_sampled(emb, num_draft_tokens=K, return_counts=True, **sel, **kw)
            print(f"[{name}/{mode}] K={K}: {counts} for {plain.shape[1]} columns")
            assert got.shape == plain.shape and torch.equal(got.cpu(), plain), f"{name} {mode} K={K}"
            assert 0 <= counts["accepted"] <= counts["drafted"] and counts["steps"] <= plain.shape[1] - 1
    eng.close()


@pytest.mark.parametrize("K", [1, 3, 7])
def test_forced_drafts_right_partly_wrong_and_all_wrong(K):
    eng, emb, cfg = _tiny_random(16, 128, 1)
    n = 45
    kw = dict(max_length=emb.shape[1] + n, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    greedy = eng.generate(emb, **kw).cpu()
    for mode, sel in MODES.items():
        plain = eng.generate(emb, **sel, **kw).cpu()
        stream = plain[0].tolist()
        assert len(set(stream)) > 4 and (not sel.get("do_sample") or not torch.equal(plain, greedy)), mode
        # the plain call's own stream: every draft is accepted, K + 1 tokens per step -- all but one of them chosen by a draft row
        eng.set_lookup_drafts([stream])
        got, c = eng.generate_lookup_sampled(emb, num_draft_tokens=K, return_counts=True, **sel, **kw)
        assert torch.equal(got.cpu(), plain), f"{mode}: all drafts right"
        assert c["steps"] == math.ceil((n - 1) / (K + 1)) and c["accepted"] == c["drafted"] == n - 1 - c["steps"], (mode, c)
        for m in (2, 3, 5):                              # every m-th draft corrupted: the counts are the restatement's
            bad = [(t + 1) % cfg.vocab if i % m == 0 else t for i, t in enumerate(stream)]
            eng.set_lookup_drafts([bad])
            got, c = eng.generate_lookup_sampled(emb, num_draft_tokens=K, return_counts=True, **sel, **kw)
            assert torch.equal(got.cpu(), plain), f"{mode}: every {m}-th draft wrong"
            assert (c["steps"], c["drafted"], c["accepted"]) == _restated_counts(stream, K, bad), (mode, m, c)
        eng.set_lookup_drafts([[(t + 1) % cfg.vocab for t in stream]])
        got, c = eng.generate_lookup_sampled(emb, num_draft_tokens=K, return_counts=True, **sel, **kw)
        assert torch.equal(got.cpu(), plain) and c["steps"] == n - 1 and c["accepted"] == 0, (mode, c)
        eng.set_lookup_drafts(None)
        assert torch.equal(eng.generate_lookup_sampled(emb, num_draft_tokens=K, **sel, **kw).cpu(), plain)
    eng.close()


@pytest.mark.parametrize("weight_dtype", ["bf16", "fp8_e4m3"])
def test_row_tile_boundary_32_and_64_rows_ragged_and_two_seeds(weight_dtype):
    eng, emb, cfg = _tiny_random(64, 256, 8, weight_dtype=weight_dtype)
    n = 70                                               # across a KV page
    kw = dict(max_length=emb.shape[1] + n, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    for mode, sel in MODES.items():
        for B in (4, 8):                                 # 32 rows: one row tile; 64 rows: two
            x = emb[:B].contiguous()
            plain = eng.generate(x, **sel, **kw).cpu()
            got, c = eng.generate_lookup_sampled(x, num_draft_tokens=7, return_counts=True, **sel, **kw)
            assert torch.equal(got.cpu(), plain), f"{weight_dtype} {mode} B={B}"
            eng.set_lookup_drafts(plain.tolist())        # each row's own stream: the accepted rows of both row tiles feed the cache
            got, c = eng.generate_lookup_sampled(x, num_draft_tokens=7, return_counts=True, **sel, **kw)
            eng.set_lookup_drafts(None)
            assert torch.equal(got.cpu(), plain) and c["steps"] == math.ceil((n - 1) / 8), (weight_dtype, mode, B, c)
        # ragged prompts, 4 sequences x 8 rows
        S0 = emb.shape[1]
        seqs = [emb[0].contiguous(), emb[1, 5:].contiguous(), emb[2, 10:].contiguous(), emb[3, 3:].contiguous()]
        rkw = dict(kw, max_length=S0 + 40)
        plain = eng.generate_ragged(seqs, **sel, **rkw).cpu()
        assert torch.equal(eng.generate_lookup_sampled(seqs, num_draft_tokens=7, **sel, **rkw).cpu(), plain), f"{weight_dtype} {mode} ragged"
        eng.set_lookup_drafts(plain.tolist())
        got, c = eng.generate_lookup_sampled(seqs, num_draft_tokens=7, return_counts=True, **sel, **rkw)
        eng.set_lookup_drafts(None)
        assert torch.equal(got.cpu(), plain) and c["steps"] == math.ceil(39 / 8), (weight_dtype, mode, c)
        # another seed is another stream, and equal again
        if sel.get("do_sample"):
            other = dict(sel, seed=4321)
            x = emb[:4].contiguous()
            a, b = eng.generate(x, **sel, **kw).cpu(), eng.generate(x, **other, **kw).cpu()
            assert not torch.equal(a, b)
            assert torch.equal(eng.generate_lookup_sampled(x, num_draft_tokens=7, **other, **kw).cpu(), b)
            assert torch.equal(eng.generate_lookup_sampled(x, num_draft_tokens=7, **sel, **kw).cpu(), a)
    eng.close()


def test_budgets_eos_stop_and_min_length_inside_an_accepted_run():
    eng, emb, cfg = _tiny_random(32, 128, 3)
    S0, K = emb.shape[1], 3
    for mode in ("topk50", "scan_pen"):
        sel = MODES[mode]
        base = eng.generate(emb, max_length=S0 + 30, eos_token_id=-1, pad_token_id=cfg.pad_token_id, **sel).cpu()
        for max_new in (1, 2, K + 1, K + 2):
            kw = dict(max_length=S0 + max_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
            plain = eng.generate(emb, **sel, **kw).cpu()
            for forced in (None, base.tolist()):
                eng.set_lookup_drafts(forced)
                got = eng.generate_lookup_sampled(emb, num_draft_tokens=K, **sel, **kw)
                assert got.shape == (3, max_new) and torch.equal(got.cpu(), plain), (mode, max_new, forced is not None)
        eng.set_lookup_drafts(base.tolist())
        for kw in (dict(eos_token_id=int(base[1, 6])), dict(eos_token_id=int(base[0, 9]), min_new_tokens=12),
                   dict(eos_token_id=int(base[2, 4]), stop_ids=[int(base[0, 13]), int(base[0, 14])]),
                   dict(eos_token_id=-1, stop_ids=[int(base[0, 5])])):
            kw.update(max_length=S0 + 30, pad_token_id=cfg.pad_token_id)
            plain = eng.generate(emb, **sel, **kw).cpu()
            got = eng.generate_lookup_sampled(emb, num_draft_tokens=K, **sel, **kw).cpu()
            assert got.shape == plain.shape and torch.equal(got, plain), (mode, kw)
        eng.set_lookup_drafts(None)
    eng.close()


def test_top_k_1_sampling_is_the_greedy_lookup():
    eng, emb, cfg = _tiny_random(16, 128, 1)
    kw = dict(max_length=emb.shape[1] + 45, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    greedy = eng.generate_lookup(emb, num_draft_tokens=3, **kw).cpu()
    # no tie on this stream: top-k 1 keeps every id AT the maximum, and a tie would be drawn from
    logits = eng.prefill(emb)[0].float()
    top2 = torch.topk(logits, 2).values
    assert float(top2[0] - top2[1]) > 0
    got = eng.generate_lookup_sampled(emb, num_draft_tokens=3, do_sample=True, top_k=1, seed=77, **kw).cpu()
    plain = eng.generate(emb, do_sample=True, top_k=1, seed=77, **kw).cpu()
    assert torch.equal(got, plain) and torch.equal(got, greedy)
    # and without sampling or a penalty the new entry point IS the greedy lookup
    a, ca = eng.generate_lookup_sampled(emb, num_draft_tokens=3, return_counts=True, **kw)
    b, cb = eng.generate_lookup(emb, num_draft_tokens=3, return_counts=True, **kw)
    assert torch.equal(a.cpu(), greedy) and ca == cb
    eng.close()


def test_isolation_graph_and_eager_streaming_and_refusals():
    eng, emb, cfg = _tiny_random(32, 128, 3)
    kw = dict(max_length=emb.shape[1] + 40, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    sel = MODES["topk50_pen"]
    os.environ.pop("SV_NO_GRAPH", None)
    greedy = eng.generate(emb, **kw).cpu()
    nodes = eng.step_plan()["graph_kernel_nodes"]
    sampled = eng.generate(emb, **sel, **kw).cpu()
    look = eng.generate_lookup(emb, num_draft_tokens=7, **kw).cpu()
    a = eng.generate_lookup_sampled(emb, num_draft_tokens=7, **sel, **kw).cpu()
    assert eng.last_timing()["graph"], "the verification step did not run as a hipGraph replay"
    b = eng.generate_lookup_sampled(emb, num_draft_tokens=7, **sel, **kw).cpu()              # the kept graph
    c = eng.generate_lookup_sampled(emb, num_draft_tokens=7, **dict(sel, seed=99), **kw).cpu()      # another key: the seed travels by value
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        d = eng.generate_lookup_sampled(emb, num_draft_tokens=7, **sel, **kw).cpu()
        assert not eng.last_timing()["graph"]
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    assert torch.equal(a, sampled) and torch.equal(a, b) and torch.equal(a, d)
    assert torch.equal(c, eng.generate(emb, **dict(sel, seed=99), **kw).cpu()) and not torch.equal(c, a)
    assert torch.equal(eng.generate_lookup_sampled(emb, num_draft_tokens=7, sync_every=1, **sel, **kw).cpu(), a)
    # isolation: the calls that were there are the calls they were
    assert torch.equal(eng.generate(emb, **kw).cpu(), greedy) and eng.step_plan()["graph_kernel_nodes"] == nodes
    assert torch.equal(eng.generate(emb, **sel, **kw).cpu(), sampled)
    assert torch.equal(eng.generate_lookup(emb, num_draft_tokens=7, **kw).cpu(), look) and torch.equal(look, greedy)
    assert torch.equal(eng.generate_lookup_sampled(emb, num_draft_tokens=0, **sel, **kw).cpu(), sampled)      # K = 0 IS the plain call
    # streaming with one row: every column once, in order
    one = emb[1:2].contiguous()
    ref = eng.generate(one, **sel, **kw).cpu()
    chunks = []
    got = eng.generate_lookup_sampled(one, num_draft_tokens=3, sync_every=2, on_tokens=lambda t, first: chunks.append((first, t.clone())), **sel, **kw).cpu()
    assert torch.equal(got, ref) and len(chunks) > 1
    assert [f for f, _ in chunks] == [sum(t.shape[1] for _, t in chunks[:i]) for i in range(len(chunks))]
    assert torch.equal(torch.cat([t for _, t in chunks], 1).cpu(), got)
    # refusals that need the engine
    with pytest.raises(NotImplementedError, match="on_tokens"):
        eng.generate_lookup_sampled(emb[:2].contiguous(), num_draft_tokens=3, on_tokens=lambda t, f: None, **sel, **kw)
    with pytest.raises(NotImplementedError, match="max_batch"):
        eng.generate_lookup_sampled(emb, num_draft_tokens=15, **sel, **kw)                   # 3 x 16 rows > 32
    with pytest.raises(NotImplementedError, match="do_sample"):
        eng.generate_lookup(emb, num_draft_tokens=3, do_sample=True, **kw)                   # the greedy method refuses as before
    assert torch.equal(eng.generate_lookup_sampled(emb, num_draft_tokens=7, **sel, **kw).cpu(), a)
    eng.close()
