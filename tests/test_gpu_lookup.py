"""GPU: prompt-lookup speculative decoding (sv_generate_lookup) at engine level.  The contract is token-for-token equality with the plain
greedy call -- `generate` / `generate_ragged` on the same engine, and HF's golden stream where a designed one exists -- whatever the drafts
are: the natural n-gram lookup, forced drafts that are all right, partly wrong, all wrong.  The forced-draft tests are the ones that fail
when a row does not see the K / V of its siblings: an accepted draft's successor was then computed over a hole in the cache."""
import dataclasses
import math
import os

import pytest
import torch
from safetensors.torch import load_file

import starvector_amd as sva
from oracle import starvector_oracle as O
from starvector_amd import lookup as LK
from tests.gpu_util import build_engine, dev, bf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(name):
    return load_file(os.path.join(ROOT, "tests", "golden", name + ".safetensors"))


def _case(name):
    """(engine, embeddings, plain keywords, HF's golden tokens or None) of one golden configuration, on an engine with room for B x 8 rows"""
    g = _golden(name)
    meta = [int(x) for x in g["meta"]]
    kw, hf = {}, None
    if name == "tiny_b3":
        cfg = O.OracleConfig.tiny()
        w = O.apply_fixture_weights(O.make_weights(cfg, seed=meta[0]), cfg, g)
        n_new, hf = meta[2], g["tokens"]
        kw = dict(eos_token_id=cfg.eos_token_id)
    elif name == "tiny_stop":
        cfg = dataclasses.replace(O.OracleConfig.tiny(), eos_token_id=meta[3])
        w = O.apply_fixture_weights(O.make_weights(cfg, seed=meta[0]), cfg, g)
        n_new, hf = meta[2], g["tokens"]
        kw = dict(eos_token_id=meta[3], stop_ids=g["stop_ids"].tolist())
    elif name == "tiny_minlen":
        cfg = dataclasses.replace(O.OracleConfig.tiny(), eos_token_id=meta[3])
        w = O.make_weights(cfg, seed=meta[0])
        n_new = meta[2]
        kw = dict(eos_token_id=meta[3], min_new_tokens=6)
    elif name == "tiny_v2_b2":
        cfg = O.OracleConfig.tiny_v2()
        w = O.make_weights(cfg, seed=meta[0])
        n_new = 70                                       # across a KV page with RoPE positions
        kw = dict(eos_token_id=-1)
    else:
        cfg = dataclasses.replace(O.OracleConfig.tiny_v2(), sliding_window=meta[3], eos_token_id=-1)
        w = O.make_weights(cfg, seed=meta[0])
        n_new = 80                                       # the window start moves through key groups and across a page
        kw = dict(eos_token_id=-1)
    eng = build_engine(cfg, w, max_batch=32, max_seq_len=128)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    kw.update(max_length=emb.shape[1] + n_new, pad_token_id=cfg.pad_token_id)
    return eng, emb, kw, hf


@pytest.mark.parametrize("name", ["tiny_b3", "tiny_stop", "tiny_minlen", "tiny_v2_b2", "tiny_v2_window"])
def test_natural_lookup_equals_the_plain_call_on_the_goldens(name):
    eng, emb, kw, hf = _case(name)
    plain = eng.generate(emb, **kw).cpu()
    if hf is not None:
        assert torch.equal(plain, hf)                    # the designed streams (margins >= 0.25 x the logit scale): HF generate's tokens
    for K in (1, 3, 7):
        got, counts = eng.generate_lookup(emb, num_draft_tokens=K, return_counts=True, **kw)
        print(f"[{name}] K={K}: {counts} for {plain.shape[1]} columns")
        assert got.shape == plain.shape and torch.equal(got.cpu(), plain), f"{name} K={K}"
        assert 0 <= counts["accepted"] <= counts["drafted"] and counts["steps"] <= plain.shape[1] - 1
        if hf is not None:
            assert torch.equal(got.cpu(), hf)
    eng.close()


def _tiny_random(max_batch, max_seq_len, B, weight_dtype="bf16", seed=21):
    cfg = dataclasses.replace(O.OracleConfig.tiny(), n_positions=max(max_seq_len, 128))
    w = O.make_weights(cfg, seed=seed)
    eng = build_engine(cfg, w, max_batch, max_seq_len, weight_dtype=weight_dtype)
    img = bf(O.synthetic_images(B, cfg.image_size, seed=22))
    prompt = torch.tensor([[7, 11]] * B, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    return eng, emb, cfg


def _restated_counts(stream, K, forced):
    """steps / drafted / accepted of the restatement for a model that continues `stream` whatever it is shown"""
    n = len(stream)
    model = lambda s, prefix, ban: stream[len(prefix)] if len(prefix) < n else 0
    toks, st = LK.lookup_greedy(model, 1, K, n, forced=[forced])
    assert toks[0] == list(stream)
    return st.steps, st.drafted, st.accepted


@pytest.mark.parametrize("K", [1, 3, 7])
def test_forced_drafts_right_partly_wrong_and_all_wrong(K):
    eng, emb, cfg = _tiny_random(16, 128, 1)
    n = 45
    kw = dict(max_length=emb.shape[1] + n, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    plain = eng.generate(emb, **kw).cpu()
    stream = plain[0].tolist()
    assert len(set(stream)) > 4
    # the plain call's own continuation: every draft is accepted, K + 1 tokens per step
    eng.set_lookup_drafts([stream])
    got, c = eng.generate_lookup(emb, num_draft_tokens=K, return_counts=True, **kw)
    assert torch.equal(got.cpu(), plain), "all drafts right: a row did not see its siblings' K / V"
    assert c["steps"] == math.ceil((n - 1) / (K + 1)) and c["accepted"] == c["drafted"] == n - 1 - c["steps"], c
    # every m-th draft token corrupted: the step and accept counts are the restatement's
    for m in (2, 3, 5):
        bad = [(t + 1) % cfg.vocab if i % m == 0 else t for i, t in enumerate(stream)]
        eng.set_lookup_drafts([bad])
        got, c = eng.generate_lookup(emb, num_draft_tokens=K, return_counts=True, **kw)
        assert torch.equal(got.cpu(), plain), f"every {m}-th draft wrong"
        assert (c["steps"], c["drafted"], c["accepted"]) == _restated_counts(stream, K, bad), (m, c)
    # all drafts wrong: one token per step
    wrong = [(t + 1) % cfg.vocab for t in stream]
    eng.set_lookup_drafts([wrong])
    got, c = eng.generate_lookup(emb, num_draft_tokens=K, return_counts=True, **kw)
    assert torch.equal(got.cpu(), plain) and c["steps"] == n - 1 and c["accepted"] == 0, c
    eng.set_lookup_drafts(None)
    assert torch.equal(eng.generate_lookup(emb, num_draft_tokens=K, **kw).cpu(), plain)
    eng.close()


@pytest.mark.parametrize("weight_dtype", ["bf16", "fp8_e4m3"])
def test_row_tile_boundary_32_and_64_rows(weight_dtype):
    eng, emb, cfg = _tiny_random(64, 256, 8, weight_dtype=weight_dtype)
    kw = dict(max_length=emb.shape[1] + 200, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    for B in (4, 8):                                     # 32 rows: one row tile; 64 rows: two
        x = emb[:B].contiguous()
        plain = eng.generate(x, **kw).cpu()
        got, c = eng.generate_lookup(x, num_draft_tokens=7, return_counts=True, **kw)
        print(f"[{weight_dtype}] B={B} K=7: {c}")
        assert torch.equal(got.cpu(), plain), f"{weight_dtype} B={B}"
        # forced: each row's own continuation (all accepted), so the accepted rows of both row tiles feed the cache
        eng.set_lookup_drafts(plain.tolist())
        got, c = eng.generate_lookup(x, num_draft_tokens=7, return_counts=True, **kw)
        eng.set_lookup_drafts(None)
        assert torch.equal(got.cpu(), plain) and c["steps"] == math.ceil(199 / 8), (weight_dtype, B, c)
    eng.close()


def test_ragged_prompts():
    eng, emb, cfg = _tiny_random(32, 128, 3)
    seqs = [emb[0, :19].contiguous(), emb[1, 5:19].contiguous(), emb[2, 10:19].contiguous()]
    kw = dict(max_length=19 + 40, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    plain = eng.generate_ragged(seqs, **kw).cpu()
    for K in (3, 7):
        assert torch.equal(eng.generate_lookup(seqs, num_draft_tokens=K, **kw).cpu(), plain)
    eng.set_lookup_drafts(plain.tolist())
    got, c = eng.generate_lookup(seqs, num_draft_tokens=7, return_counts=True, **kw)
    eng.set_lookup_drafts(None)
    assert torch.equal(got.cpu(), plain) and c["steps"] == math.ceil(39 / 8), c
    eng.close()


def test_budgets_eos_and_stop_inside_an_accepted_run():
    eng, emb, cfg = _tiny_random(32, 128, 3)
    S0, K = emb.shape[1], 3
    base = eng.generate(emb, max_length=S0 + 30, eos_token_id=-1, pad_token_id=cfg.pad_token_id).cpu()
    for max_new in (1, 2, K + 1, K + 2):
        kw = dict(max_length=S0 + max_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
        plain = eng.generate(emb, **kw).cpu()
        for forced in (None, base.tolist()):
            eng.set_lookup_drafts(forced)
            got = eng.generate_lookup(emb, num_draft_tokens=K, **kw)
            assert got.shape == (3, max_new) and torch.equal(got.cpu(), plain), (max_new, forced is not None)
    # an EOS and a row-0 stop sequence in the middle of runs of accepted drafts; rows end at different columns
    eng.set_lookup_drafts(base.tolist())
    for kw in (dict(eos_token_id=int(base[1, 6])), dict(eos_token_id=int(base[0, 9]), min_new_tokens=12),
               dict(eos_token_id=int(base[2, 4]), stop_ids=[int(base[0, 13]), int(base[0, 14])]),
               dict(eos_token_id=-1, stop_ids=[int(base[0, 5])])):
        kw.update(max_length=S0 + 30, pad_token_id=cfg.pad_token_id)
        plain = eng.generate(emb, **kw).cpu()
        got = eng.generate_lookup(emb, num_draft_tokens=K, **kw).cpu()
        assert got.shape == plain.shape and torch.equal(got, plain), kw
    eng.set_lookup_drafts(None)
    eng.close()


def test_graph_equals_eager_repeats_streams_and_leaves_the_plain_call_alone():
    eng, emb, cfg = _tiny_random(32, 128, 3)
    kw = dict(max_length=emb.shape[1] + 40, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    os.environ.pop("SV_NO_GRAPH", None)
    before = eng.generate(emb, **kw).cpu()
    nodes = eng.step_plan()["graph_kernel_nodes"]
    a = eng.generate_lookup(emb, num_draft_tokens=7, **kw).cpu()
    assert eng.last_timing()["graph"], "the verification step did not run as a hipGraph replay"
    b = eng.generate_lookup(emb, num_draft_tokens=7, **kw).cpu()
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        c = eng.generate_lookup(emb, num_draft_tokens=7, **kw).cpu()
        assert not eng.last_timing()["graph"]
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    assert torch.equal(a, before) and torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(eng.generate_lookup(emb, num_draft_tokens=7, sync_every=1, **kw).cpu(), a)
    # isolation: the plain call afterwards is the call it was -- same tokens, same captured step
    assert torch.equal(eng.generate(emb, **kw).cpu(), before) and eng.step_plan()["graph_kernel_nodes"] == nodes
    assert torch.equal(eng.generate(emb, do_sample=True, top_p=0.9, seed=3, **kw).cpu(),
                       eng.generate(emb, do_sample=True, top_p=0.9, seed=3, **kw).cpu())
    # num_draft_tokens = 0 IS the plain call
    assert torch.equal(eng.generate_lookup(emb, num_draft_tokens=0, **kw).cpu(), before)
    # streaming with one row: the columns, concatenated, are the returned tokens
    one = emb[1:2].contiguous()
    chunks = []
    got = eng.generate_lookup(one, num_draft_tokens=3, sync_every=2, on_tokens=lambda t, first: chunks.append((first, t.clone())), **kw).cpu()
    assert torch.equal(got, before[1:2]) and len(chunks) > 1
    assert [f for f, _ in chunks] == [sum(t.shape[1] for _, t in chunks[:i]) for i in range(len(chunks))]
    assert torch.equal(torch.cat([t for _, t in chunks], 1).cpu(), got)
    eng.close()


@pytest.mark.parametrize("exclusive", [False, True])
def test_starvector_1b_dimensions(exclusive):
    """StarVector-1B widths, two layers, random weights: with exclusive_device the fused row-update + c_attn and fused MLP launches carry
    the draft rows too."""
    eng = sva.HipEngine(sva.EngineConfig(vit_layers=1, n_layer=2, max_batch=8, max_seq_len=128, exclusive_device=exclusive))
    eng.load_random_weights(seed=13)
    gen = torch.Generator().manual_seed(9)
    emb = (torch.randn(1, 24, eng.cfg.hidden, generator=gen) * 0.5).to(torch.bfloat16).to(dev())
    kw = dict(max_length=24 + 40, eos_token_id=-1, pad_token_id=49152)
    plain = eng.generate(emb, **kw).cpu()
    plan = eng.step_plan()
    if exclusive:
        assert plan["mlp_fused"], plan
    assert torch.equal(eng.generate_lookup(emb, num_draft_tokens=7, **kw).cpu(), plain)
    for forced in (plain.tolist(), [[(t + 1) % 49152 if i % 3 == 0 else t for i, t in enumerate(plain[0].tolist())]]):
        eng.set_lookup_drafts(forced)
        got, c = eng.generate_lookup(emb, num_draft_tokens=7, return_counts=True, **kw)
        assert torch.equal(got.cpu(), plain), (exclusive, c)
    assert torch.equal(eng.generate(emb, **kw).cpu(), plain)
    eng.close()


def test_refusals_name_their_argument():
    eng, emb, cfg = _tiny_random(8, 64, 3)
    kw = dict(max_length=emb.shape[1] + 8, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    for extra, name in ((dict(do_sample=True), "do_sample"), (dict(num_beams=2), "num_beams"), (dict(repetition_penalty=1.2), "repetition_penalty"),
                        (dict(n_samples=2), "n_samples"), (dict(token_stats=True), "token_stats"), (dict(token_topk=4), "token_topk"),
                        (dict(return_outputs=True), "return_outputs"), (dict(logits_processors=object()), "logits_processors")):
        with pytest.raises(NotImplementedError, match=name):
            eng.generate_lookup(emb, num_draft_tokens=3, **extra, **kw)
    with pytest.raises(NotImplementedError, match="max_batch"):
        eng.generate_lookup(emb, num_draft_tokens=3, **kw)                   # 3 x 4 rows > 8
    with pytest.raises(NotImplementedError, match="on_tokens"):
        eng.generate_lookup(emb[:2].contiguous(), num_draft_tokens=3, on_tokens=lambda t, f: None, **kw)
    with pytest.raises(ValueError, match="num_draft_tokens"):
        eng.generate_lookup(emb[:1].contiguous(), num_draft_tokens=16, **kw)
    with pytest.raises(ValueError, match="max_ngram"):
        eng.generate_lookup(emb[:1].contiguous(), num_draft_tokens=3, max_ngram=9, **kw)
    # the C ABI's own refusals (the wrapper above never builds such a sampling block)
    import ctypes as C
    from starvector_amd import _lib
    lib = _lib.load()
    x = emb[:1].contiguous()
    out, n = torch.empty(1, 8, dtype=torch.int64, device=dev()), C.c_int32(0)
    lk = _lib.SvLookup(3, 0, 0)
    for field, val, name in (("do_sample", 1, "do_sample"), ("num_beams", 2, "num_beams"), ("repetition_penalty", 1.3, "repetition_penalty")):
        sp = _lib.SvSampling(0, 1.0, 1.0, x.shape[1] + 8, -1, 0, 0, None, 0, 0, 1.0, 1, 1.0, 0, 0, None, None, 0)
        setattr(sp, field, val)
        rc = lib.sv_generate_lookup(eng._h, C.c_void_p(x.data_ptr()), 1, None, x.shape[1], C.byref(sp), C.byref(lk), C.c_void_p(out.data_ptr()),
                                    C.byref(n), None, None)
        assert rc == -95 and name in lib.sv_last_error().decode(), (field, rc, lib.sv_last_error())
    # the engine still works
    assert eng.generate_lookup(x, num_draft_tokens=3, **kw).shape == (1, 8)
    eng.close()
