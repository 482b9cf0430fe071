"""-m gpu: one prompt pass for the n samples of a prompt (sv_generate_shared, sv_cb_admit_shared).

Contract: the copies of a prompt on the repeated route are bit-identical, so computing one and sharing its KV pages must not change a
single token.  Every comparison is torch.equal / exact integer equality against the repeated-prompt route (`generate` /
`generate_ragged` on the repeat_interleave'd prompts, a request's solo `cb_admit` run), which the rest of the suite ties to HF and
the oracle.  Both decoder families: GPTBigCode (MQA, learned positions) and StarCoder2 (GQA + RoPE, once with a sliding window shorter
than the prompt)."""
import dataclasses
import os

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from starvector_amd import engine as E
from starvector_amd._lib import StarVectorBusy
from oracle import starvector_oracle as O
from tests.gpu_util import bf, build_engine, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE = 64
SAMPLING = dict(do_sample=True, temperature=0.9, top_p=0.95, top_k=40, repetition_penalty=1.2, seed=1234, eos_token_id=-1)


def _tiny_engine(arch, max_batch, max_seq_len, window=0, weight_dtype="bf16"):
    base = O.OracleConfig.tiny() if arch == "v1" else O.OracleConfig.tiny_v2()
    cfg = dataclasses.replace(base, n_positions=max(base.n_positions, max_seq_len), eos_token_id=-1, sliding_window=window)
    w = O.make_weights(cfg, seed=77)
    return cfg, build_engine(cfg, w, max_batch=max_batch, max_seq_len=max_seq_len, weight_dtype=weight_dtype)


def _embeds(lens, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, hidden, generator=g).to(torch.bfloat16).to(dev()) for n in lens]


def _rect(seqs):
    return torch.stack(seqs).contiguous()


def _shared_equals_repeated(eng, hidden, B, G, S0_list, n_new, tag):
    for S0 in S0_list:
        x = _rect(_embeds([S0] * B, hidden, 100 + S0))
        want = eng.generate(x.repeat_interleave(G, dim=0), max_length=S0 + n_new, **SAMPLING).cpu()
        passes = eng.prompt_passes()
        got = eng.generate_shared(x, max_length=S0 + n_new, n_samples=G, **SAMPLING).cpu()
        assert eng.prompt_passes() - passes == 1
        assert got.shape == want.shape == (B * G, n_new), (tag, S0, got.shape, want.shape)       # tokens and n_generated
        assert torch.equal(got, want), f"[{tag}] S0={S0}: the shared call's tokens differ from the repeated prompts'"
        rows = got.view(B, G, n_new)
        assert any(not torch.equal(rows[b, 0], rows[b, 1]) for b in range(B)), f"[{tag}] S0={S0}: the samples of a prompt are all equal"


@pytest.mark.parametrize("arch,window", [("v1", 0), ("v2", 0), ("v2", 24)])
def test_sampling_shared_equals_repeated_prompts(arch, window):
    """test 1: B = 3, G = 4; S0 below a page, exactly two pages, and above a page with a partially filled tail page"""
    cfg, eng = _tiny_engine(arch, max_batch=12, max_seq_len=256, window=window)
    _shared_equals_repeated(eng, cfg.hidden, 3, 4, [40, 128, 150], 36, f"{arch} window {window}")
    eng.close()


def test_sampling_shared_equals_repeated_prompts_fp8_weights():
    """test 8: the same on an engine with fp8 decoder weights"""
    cfg, eng = _tiny_engine("v1", max_batch=12, max_seq_len=256, weight_dtype="fp8_e4m3")
    _shared_equals_repeated(eng, cfg.hidden, 3, 4, [40, 128, 150], 36, "v1 fp8")
    eng.close()


def test_greedy_rows_of_a_request_are_equal_and_are_hfs_tokens():
    """test 2: tests/golden/tiny_b3 (the designed stream: the engine reproduces HF generate token for token)"""
    g = load_file(os.path.join(ROOT, "tests", "golden", "tiny_b3.safetensors"))
    seed, B, n_new = [int(x) for x in g["meta"]]
    cfg = O.OracleConfig.tiny()
    w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)
    G = 4
    eng = build_engine(cfg, w, max_batch=B * G, max_seq_len=64)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    got = eng.generate_shared(emb, max_length=emb.shape[1] + n_new, n_samples=G, eos_token_id=cfg.eos_token_id,
                              pad_token_id=cfg.pad_token_id).cpu()
    assert got.shape == (B * G, n_new)
    for r in range(B * G):
        assert torch.equal(got[r], g["tokens"][r // G]), f"row {r} (sample {r % G} of request {r // G}) is not HF's greedy stream"
    eng.close()


def test_ragged_shared_equals_ragged_repeated_and_solo():
    """test 3: prompts below a page, a multiple of a page, neither; G = 3"""
    cfg, eng = _tiny_engine("v1", max_batch=9, max_seq_len=256)
    lens, G, n_new = [37, 128, 150], 3, 30
    seqs = _embeds(lens, cfg.hidden, 7)
    rep = [s for s in seqs for _ in range(G)]
    want = eng.generate_ragged(rep, max_length=max(lens) + n_new, **SAMPLING).cpu()
    passes = eng.prompt_passes()
    got = eng.generate_shared(seqs, max_length=max(lens) + n_new, n_samples=G, **SAMPLING).cpu()
    assert eng.prompt_passes() - passes == 1
    assert got.shape == want.shape == (9, n_new) and torch.equal(got, want)
    greedy = eng.generate_shared(seqs, max_length=max(lens) + n_new, n_samples=G, eos_token_id=-1).cpu()
    for b, x in enumerate(seqs):
        solo = eng.generate(x[None].contiguous(), max_length=x.shape[0] + n_new, eos_token_id=-1).cpu()[0]
        for j in range(G):
            assert torch.equal(greedy[b * G + j], solo), (b, j)
    # the packed form with lengths, and n_samples = 1 = the ragged call
    packed = torch.cat(seqs, 0)
    assert torch.equal(eng.generate_shared(packed, max_length=max(lens) + n_new, n_samples=G, lengths=lens, **SAMPLING).cpu(), want)
    one = eng.generate_shared(seqs, max_length=max(lens) + n_new, n_samples=1, **SAMPLING).cpu()
    assert torch.equal(one, eng.generate_ragged(seqs, max_length=max(lens) + n_new, **SAMPLING).cpu())
    eng.close()


def test_64_decode_rows_from_a_prompt_pass_of_8():
    """test 4: B = 8, G = 8 on a 64-row engine: the two-row-tile decode kernels, a prompt pass 8 x smaller than the one it is compared with"""
    cfg, eng = _tiny_engine("v2", max_batch=64, max_seq_len=192)
    _shared_equals_repeated(eng, cfg.hidden, 8, 8, [70], 24, "v2 64 rows")
    with pytest.raises(ValueError, match="max_batch"):
        eng.generate_shared(_rect(_embeds([20] * 9, cfg.hidden, 3)), max_length=30, n_samples=8)
    with pytest.raises(NotImplementedError):
        eng.generate_shared(_rect(_embeds([20] * 2, cfg.hidden, 3)), max_length=30, n_samples=2, num_beams=2)
    eng.close()


def test_page_structure_outputs_and_streaming():
    """test 5"""
    cfg, eng = _tiny_engine("v1", max_batch=8, max_seq_len=256)
    lens, G, n_new = [150, 64, 30], 2, 20
    seqs = _embeds(lens, cfg.hidden, 9)
    eng.generate_shared(seqs, max_length=max(lens) + n_new, n_samples=G, eos_token_id=-1)
    rows = [eng.block_table_row(r) for r in range(len(lens) * G)]
    used = set()
    for b, n in enumerate(lens):
        sh, need = n // PAGE, -(-(n + n_new) // PAGE)
        grp = [rows[b * G + j] for j in range(G)]
        for j in range(1, G):
            assert grp[j][:sh] == grp[0][:sh], (b, j)                            # the prompt's full pages: the same entries
        own = [set(r[sh:need]) for r in grp]
        for j in range(G):
            assert len(own[j]) == need - sh
            for k in range(j):
                assert not own[j] & own[k], (b, j, k)                            # pairwise disjoint from the tail page on
            assert not own[j] & set(grp[0][:sh]) and not own[j] & used
        used |= set(grp[0][:sh]).union(*own)
    plan = E.shared_plan(lens, [b for b in range(len(lens)) for _ in range(G)], [n_new] * (len(lens) * G))
    free, total = eng.free_pages()
    assert total - free == plan["total"] == len(used)
    # return_dict_in_generate scores / logits equal the repeated route's (rectangular: the mirror's own route for them)
    from starvector_amd.model import HipCausalLM
    lm = HipCausalLM(eng, eos_token_id=-1, pad_token_id=0)
    x = _rect(_embeds([70] * 3, cfg.hidden, 10))
    kw = dict(inputs_embeds=x, max_length=70 + 12, num_return_sequences=2, do_sample=True, top_p=0.9, temperature=0.8, seed=5,
              return_dict_in_generate=True, output_scores=True, output_logits=True)
    a, b_ = lm.generate(**kw), lm.generate(share_prompt=False, **kw)
    assert a.sequences.shape == (6, 12) and torch.equal(a.sequences, b_.sequences)
    assert len(a.scores) == len(b_.scores) == 12 and a.scores[0].shape[0] == 6
    for t in range(12):
        assert torch.equal(a.scores[t], b_.scores[t]) and torch.equal(a.logits[t], b_.logits[t]), t
    # streaming delivers B * G rows, the columns of the result
    chunks = []
    out = eng.generate_shared(x, max_length=70 + 12, n_samples=2, eos_token_id=-1, sync_every=4,
                              on_tokens=lambda toks, first: chunks.append((first, toks.clone()))).cpu()
    assert all(c.shape[0] == 6 for _, c in chunks) and torch.equal(torch.cat([c for _, c in chunks], 1), out)
    eng.close()


def _solo_cb(eng, x, req):
    s = eng.cb_admit([x], [req])[0]
    while eng.cb_poll()[0][s]:
        eng.cb_step(8)
    toks = eng.cb_read(s, 0, eng.cb_poll()[1][s])
    eng.cb_release(s)
    return toks


def test_group_admit_refcounts_release_and_rollback():
    """test 6"""
    cfg, eng = _tiny_engine("v1", max_batch=8, max_seq_len=256)
    lens = [150, 70]
    seqs = _embeds(lens, cfg.hidden, 21)
    other = _embeds([100], cfg.hidden, 22)[0]
    base = dict(do_sample=True, temperature=0.9, top_p=0.95, top_k=40, eos_token_id=-1)
    reqs = [dict(base, seed=11, max_new_tokens=40), dict(base, seed=12, max_new_tokens=12),
            dict(base, seed=13, max_new_tokens=40, repetition_penalty=1.2),
            dict(base, seed=14, max_new_tokens=40), dict(base, seed=15, max_new_tokens=12),
            dict(semantics="vllm", do_sample=True, temperature=0.8, top_p=0.9, seed=16, max_new_tokens=40, eos_token_id=-1,
                 prompt_ids=[3, 4], presence_penalty=0.3, stop_any_ids=[])]
    group = [0, 0, 0, 1, 1, 1]
    oreq = dict(base, seed=99, max_new_tokens=30)
    eng.cb_reset()
    want = [_solo_cb(eng, seqs[g], r) for g, r in zip(group, reqs)]
    want_other = _solo_cb(eng, other, oreq)
    # a stop id for the vLLM-semantics request taken from its own solo stream: it ends early, on its own
    stop = int(want[5][7])
    reqs[5] = dict(reqs[5], stop_any_ids=[stop])
    want[5] = _solo_cb(eng, seqs[1], reqs[5])
    assert want[5].numel() <= 8
    eng.cb_reset()
    eng.cb_release(eng.cb_admit([other], [dict(oreq, max_new_tokens=1)])[0])      # an active, empty continuous batch: every page is free
    free0, total = eng.free_pages()
    assert free0 == total
    before = eng.prompt_passes()
    slots = eng.cb_admit_shared(seqs, None, group, reqs)
    assert eng.prompt_passes() - before == 1
    plan = E.shared_plan(lens, group, [r["max_new_tokens"] for r in reqs])
    assert free0 - eng.free_pages()[0] == plan["total"]
    for u in (0, 1):
        rows = [eng.block_table_row(slots[i]) for i in range(6) if group[i] == u]
        sh = lens[u] // PAGE
        assert all(r[:sh] == rows[0][:sh] for r in rows) and len({r[sh] for r in rows}) == 3
    # the short-budget samples finish first: release them while their siblings decode on, and hand their pages to a newcomer
    while eng.cb_poll()[0][slots[1]] or eng.cb_poll()[0][slots[4]]:
        eng.cb_step(4)
    for i in (1, 4):
        assert torch.equal(eng.cb_read(slots[i], 0, eng.cb_poll()[1][slots[i]]), want[i]), i
    held = eng.free_pages()[0]
    eng.cb_release(slots[1])
    assert eng.free_pages()[0] - held == plan["private"][1]                       # its own pages at once, no shared page
    eng.cb_release(slots[4])
    s_other = eng.cb_admit([other], [oreq])[0]
    assert s_other in (slots[1], slots[4])
    while eng.cb_step(8) > 0:
        pass
    lv, st = eng.cb_poll()
    for i in (0, 2, 3, 5):
        assert torch.equal(eng.cb_read(slots[i], 0, st[slots[i]]), want[i]), f"request {i} differs from its solo run"
    assert torch.equal(eng.cb_read(s_other, 0, st[s_other]), want_other)
    # a shared page goes back with its last holder
    eng.cb_release(slots[0])
    f1 = eng.free_pages()[0]
    eng.cb_release(slots[2])
    assert eng.free_pages()[0] - f1 == plan["private"][2] + lens[0] // PAGE
    for s in (slots[3], slots[5], s_other):
        eng.cb_release(s)
    assert eng.free_pages()[0] == free0
    # too few slots: refused as a whole, nothing changes; after a release the same admit succeeds
    hold = eng.cb_admit(_embeds([20] * 4, cfg.hidden, 23), [dict(max_new_tokens=8, eos_token_id=-1)] * 4)
    f2 = eng.free_pages()[0]
    with pytest.raises(StarVectorBusy):
        eng.cb_admit_shared(seqs, None, group, reqs)
    assert eng.free_pages()[0] == f2 and sum(eng.cb_poll()[0]) == 4
    eng.cb_release(hold[0])
    eng.cb_release(hold[1])
    slots = eng.cb_admit_shared(seqs, None, group, reqs)
    while eng.cb_step(8) > 0:
        pass
    lv, st = eng.cb_poll()
    for i in range(6):
        assert torch.equal(eng.cb_read(slots[i], 0, st[slots[i]]), want[i]), f"retry: request {i} differs from its solo run"
    eng.cb_reset()
    # prompts given in another order than their first requests: the binding renumbers them
    slots = eng.cb_admit_shared(seqs, None, [1, 0, 1], [reqs[3], reqs[0], reqs[4]])
    while eng.cb_step(8) > 0:
        pass
    lv, st = eng.cb_poll()
    for s, i in zip(slots, (3, 0, 4)):
        assert torch.equal(eng.cb_read(s, 0, st[s]), want[i]), i
    eng.cb_reset()
    eng.close()


def test_vllm_api_and_grpo_rollouts_share_the_prompt(tmp_path):
    """test 7"""
    from PIL import Image
    import starvector_amd as sva
    from starvector_amd import vllm as VL
    from tests.ckpt_util import write_reference_checkpoint
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=21)
    path = str(tmp_path / "ckpt")
    write_reference_checkpoint(path, cfg, w, max_batch=8)
    llm = VL.LLM(model=path, max_num_seqs=8, max_model_len=min(96, cfg.n_positions), trust_remote_code=True, byte_tokenizer_fallback=True)
    rng = np.random.default_rng(3)
    inputs = [{"prompt": "<image-start>", "multi_modal_data": {"image": Image.fromarray(rng.integers(0, 255, (40 + 7 * i, 48, 3), dtype=np.uint8))}}
              for i in range(2)]
    sp = VL.SamplingParams(n=4, temperature=0.8, top_p=0.95, seed=31, max_tokens=14)
    admits, real = [], llm.engine.cb_admit_shared

    def recording(embs, lengths, group, requests):             # what the batcher hands the group admit: (prompts, requests) per call
        admits.append((len(embs), list(group)))
        return real(embs, lengths, group, requests)
    llm.engine.cb_admit_shared = recording
    before = llm.engine.prompt_passes()
    a = llm.generate(inputs, sp, use_tqdm=False)
    # every one of the 2 x 4 samples went in through a group admit, each input's four together (a group is queued atomically and 8 slots
    # are free): one prompt row set per INPUT, never per sample, in one or two prompt passes
    assert sum(len(g) for _, g in admits) == 8 and sum(n for n, _ in admits) == 2, admits
    assert all(g.count(u) == 4 for n, g in admits for u in range(n)), admits
    assert llm.engine.prompt_passes() - before == len(admits) <= 2
    admits.clear()
    b = llm.generate(inputs, sp, use_tqdm=False, share_prompt=False)
    assert admits == []                                        # the switch: every sample on its own
    del llm.engine.cb_admit_shared
    assert [[c.token_ids for c in o.outputs] for o in a] == [[c.token_ids for c in o.outputs] for o in b]
    assert len({tuple(c.token_ids) for c in a[0].outputs}) > 1
    model = llm.model
    batch = {"image": bf(O.synthetic_images(2, cfg.image_size, seed=5))}
    S0 = model.model.query_length + 4
    kw = dict(max_length=S0 + 40, num_return_sequences=4, temperature=0.9, top_p=0.9, seed=77)
    before = llm.engine.prompt_passes()
    r1 = model.model.generate_im2svg_grpo(batch, **kw)
    assert llm.engine.prompt_passes() - before == 1
    r2 = model.model.generate_im2svg_grpo(batch, share_prompt=False, **kw)
    assert r1["outputs"].shape[0] == 8 and torch.equal(r1["outputs"], r2["outputs"]) and r1["raw_svg"] == r2["raw_svg"]
    llm.close()
