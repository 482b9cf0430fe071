"""-m gpu: the ragged prompt pass -- prompts of different lengths, packed back to back, in ONE prefill (sv_prefill_ragged,
sv_generate_ragged, sv_cb_admit_ragged).

Contract: for every sequence of a ragged call the last-row logits, every K / V entry written to its pages and every token generated
afterwards are BIT-IDENTICAL to the same sequence run alone through the rectangular entry point with S0 = its length.  No tolerance
anywhere: every comparison is torch.equal.  The reference of every check is the engine's own solo run, which the rest of the suite ties
to the oracle and to HF."""
import dataclasses
import random

import pytest
import torch

import starvector_amd as sva
from starvector_amd import engine as E
from oracle import starvector_oracle as O
from tests.gpu_util import build_engine, dev

pytestmark = pytest.mark.gpu

LENS = [5, 31, 255, 256, 257, 259, 260, 515]
PAGE = 64                                            # SV_PAGE_TOKENS


def _shuffled(lens, seed):
    out = list(lens)
    random.Random(seed).shuffle(out)
    return out


def _embeds(lens, hidden, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, hidden, generator=g) * scale).to(torch.bfloat16).to(dev()) for n in lens]


def _tiny_engine(arch, max_batch, max_seq_len, window=0):
    base = O.OracleConfig.tiny() if arch == "v1" else O.OracleConfig.tiny_v2()
    cfg = dataclasses.replace(base, n_positions=max(base.n_positions, max_seq_len), eos_token_id=-1, sliding_window=window)
    w = O.make_weights(cfg, seed=77)
    return cfg, build_engine(cfg, w, max_batch=max_batch, max_seq_len=max_seq_len)


def _fullsize_engine(max_batch, max_seq_len, n_layer=2):
    # StarVector-1B decoder dimensions, reduced depth, a small vision tower (the prompt pass never runs it), random weights
    ec = sva.EngineConfig(vit_layers=1, n_layer=n_layer, max_batch=max_batch, max_seq_len=max_seq_len)
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=4321)
    return ec, eng


def _check_prefill_and_steps(eng, seqs, tag, n_steps=3):
    """ragged prefill + n_steps decode steps against the same on each sequence alone; the decode steps read every K / V page and the positions"""
    B = len(seqs)
    solo_logits, solo_steps = [], []
    for b, x in enumerate(seqs):
        lg = eng.prefill(x[None].contiguous())
        cur = [lg.clone()]
        for t in range(n_steps):
            lg = eng.decode_step(cur[-1].argmax(-1))
            cur.append(lg.clone())
        solo_logits.append(cur[0][0])
        solo_steps.append([c[0] for c in cur[1:]])
    lg = eng.prefill_ragged(seqs)
    for b in range(B):
        assert torch.equal(lg[b], solo_logits[b]), f"[{tag}] prefill logits of sequence {b} (length {seqs[b].shape[0]}) differ from its solo run"
    for t in range(n_steps):
        lg = eng.decode_step(lg.argmax(-1))
        for b in range(B):
            assert torch.equal(lg[b], solo_steps[b][t]), f"[{tag}] decode step {t} of sequence {b} (length {seqs[b].shape[0]}) differs from its solo run"


@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_prefill_ragged_tiny_models_bitwise(arch):
    cfg, eng = _tiny_engine(arch, max_batch=32, max_seq_len=640)
    lens = _shuffled(LENS, 3)
    _check_prefill_and_steps(eng, _embeds(lens, cfg.hidden, 11), f"tiny {arch} mixed")
    short = [random.Random(5).randint(8, 96) for _ in range(32)]
    _check_prefill_and_steps(eng, _embeds(short, cfg.hidden, 12), f"tiny {arch} 32 short rows")
    eng.close()


def test_prefill_ragged_sliding_window_prompt_longer_than_window():
    """tiny v2 with the window tests/golden/tiny_v2_window.safetensors was minted for (24): prompts shorter and longer than it in one pass"""
    cfg, eng = _tiny_engine("v2", max_batch=8, max_seq_len=256, window=24)
    lens = [7, 100, 24, 25, 3, 70]
    _check_prefill_and_steps(eng, _embeds(lens, cfg.hidden, 13), "tiny v2 window 24")
    eng.close()


def test_prefill_ragged_starvector_1b_dimensions_every_kernel_class():
    ec, eng = _fullsize_engine(max_batch=32, max_seq_len=640)
    lens = _shuffled(LENS, 4)
    # the length list reaches every kernel class at these shapes -- asserted, not assumed
    D, F, QKV = ec.hidden, ec.n_inner, ec.hidden + 2 * (ec.hidden // ec.n_head)
    plans = {name: E.ragged_plan(lens, N, K, act) for name, (N, K, act) in
             {"c_attn": (QKV, D, "none"), "c_proj": (D, D, "none"), "c_fc": (F, D, "gelu_tanh"), "down": (D, F, "none")}.items()}
    peel = {n: sorted(len([r for r in p["rows"] if _seq_of(lens, r) == b]) for b in p["last"]) for n, p in plans.items()}
    assert any(1 in v for v in peel.values()) and any(3 in v for v in peel.values()), peel          # peel rows of 1 (257) and 3 (259 / 515)
    assert not plans["c_attn"]["rows"] and plans["c_proj"]["rows"], plans              # the rule is per projection
    for p in plans.values():                                                           # the pruned last row: a peel row for some sequences, not for others
        assert len(p["last"]) < len(lens)
        assert all(_seq_of(lens, r) in p["last"] for r in p["rows"])
    assert set(plans["c_fc"]["last"]) < set(plans["down"]["last"]), plans              # ... and for one sequence (259) in one projection but not another
    assert {5, 256, 260} <= set(lens)                                                  # short rows; whole tiles; rows left over without the peel form
    _check_prefill_and_steps(eng, _embeds(lens, ec.hidden, 21, scale=0.5), "1B dims mixed")
    short = [random.Random(6).randint(8, 96) for _ in range(32)]
    _check_prefill_and_steps(eng, _embeds(short, ec.hidden, 22, scale=0.5), "1B dims 32 short rows")
    eng.close()


def _seq_of(lens, row):
    r0 = 0
    for b, n in enumerate(lens):
        if row < r0 + n:
            return b
        r0 += n
    raise AssertionError(row)


def test_generate_ragged_rows_equal_their_solo_runs():
    cfg, eng = _tiny_engine("v1", max_batch=8, max_seq_len=400)
    lens = [70, 5, 259, 64, 33]
    seqs = _embeds(lens, cfg.hidden, 31)
    n_new = 40
    for kw in (dict(eos_token_id=-1), dict(eos_token_id=-1, repetition_penalty=1.3)):
        solo = [eng.generate(x[None].contiguous(), max_length=x.shape[0] + n_new, **kw).cpu()[0] for x in seqs]
        got = eng.generate_ragged(seqs, max_length=max(lens) + n_new, **kw).cpu()
        assert got.shape == (len(lens), n_new)
        for b in range(len(lens)):
            assert torch.equal(got[b], solo[b]), (kw, b)
    # EOS: a token of row 1's own stream ends row 1 (pad afterwards), the others go on
    free = [eng.generate(x[None].contiguous(), max_length=x.shape[0] + n_new, eos_token_id=-1).cpu()[0] for x in seqs]
    eos = int(free[1][6])
    pad = 3
    solo = [eng.generate(x[None].contiguous(), max_length=x.shape[0] + n_new, eos_token_id=eos, pad_token_id=pad).cpu()[0] for x in seqs]
    got = eng.generate_ragged(seqs, max_length=max(lens) + n_new, eos_token_id=eos, pad_token_id=pad).cpu()
    for b in range(len(lens)):
        n = solo[b].numel()
        assert torch.equal(got[b, :min(n, got.shape[1])], solo[b][:got.shape[1]]), b
        assert bool((got[b, n:] == pad).all()), b                           # a finished row is padded while the batch runs on
    # the row-0 stop cuts every row
    stop = [int(free[0][9]), int(free[0][10])]
    got = eng.generate_ragged(seqs, max_length=max(lens) + n_new, eos_token_id=-1, stop_ids=stop).cpu()
    solo0 = eng.generate(seqs[0][None].contiguous(), max_length=lens[0] + n_new, eos_token_id=-1, stop_ids=stop).cpu()[0]
    assert got.shape[1] == solo0.numel() < n_new
    for b in range(len(lens)):
        assert torch.equal(got[b], free[b][:got.shape[1]]), b
    # equal lengths + sampling: exactly the rectangular call with the same seed
    same = _embeds([48] * 4, cfg.hidden, 32)
    kw = dict(do_sample=True, temperature=0.9, top_p=0.95, top_k=40, seed=17, eos_token_id=-1)
    rect = eng.generate(torch.stack(same).contiguous(), max_length=48 + 24, **kw).cpu()
    assert torch.equal(eng.generate_ragged(same, max_length=48 + 24, **kw).cpu(), rect)
    assert torch.equal(eng.prefill_ragged(same), eng.prefill(torch.stack(same).contiguous()))
    eng.close()


@pytest.mark.parametrize("num_beams,length_penalty,early_stopping", [(2, 1.0, False), (3, 0.7, True)])
def test_beam_search_ragged_equals_solo_beam_search(num_beams, length_penalty, early_stopping):
    cfg, eng = _tiny_engine("v1", max_batch=16, max_seq_len=256)
    lens = [PAGE - 1, PAGE, PAGE + 1, 7, 2 * PAGE + 5]            # both sides of a KV page boundary
    seqs = _embeds(lens, cfg.hidden, 41)
    n_new = 20
    kw = dict(num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping, eos_token_id=5, pad_token_id=0,
              return_outputs=True)
    got = eng.generate_ragged(seqs, max_length=max(lens) + n_new, **kw)
    for b, x in enumerate(seqs):
        solo = eng.generate(x[None].contiguous(), max_length=x.shape[0] + n_new, **kw)
        n = solo["sequences"].shape[1]
        g = got["sequences"][b].cpu()
        assert torch.equal(g[:n], solo["sequences"][0].cpu()[:g.numel()]), b
        assert bool((g[n:] == 0).all()), b
        assert torch.equal(got["sequences_scores"][b], solo["sequences_scores"][0]), b
    eng.close()


def test_cb_admit_ragged_mixed_lengths_into_a_live_batch():
    from starvector_amd._lib import StarVectorBusy
    cfg, eng = _tiny_engine("v1", max_batch=8, max_seq_len=200)
    lens = [9, 70, 33, 64, 120]
    seqs = _embeds(lens, cfg.hidden, 51)
    reqs = [dict(max_new_tokens=24, eos_token_id=-1), dict(max_new_tokens=40, eos_token_id=-1, repetition_penalty=1.2),
            dict(max_new_tokens=30, do_sample=True, temperature=0.8, top_p=0.9, top_k=50, seed=11, eos_token_id=-1),
            dict(max_new_tokens=16, eos_token_id=-1), dict(max_new_tokens=50, eos_token_id=-1)]

    def solo(x, r):
        return eng.generate(x[None].contiguous(), max_length=x.shape[0] + r["max_new_tokens"], do_sample=r.get("do_sample", False),
                            temperature=r.get("temperature", 1.0), top_p=r.get("top_p", 1.0), top_k=r.get("top_k", 0), seed=r.get("seed", 0),
                            eos_token_id=-1, repetition_penalty=r.get("repetition_penalty", 1.0)).cpu()[0]
    want = [solo(x, r) for x, r in zip(seqs, reqs)]
    before = eng.prompt_passes()
    slots = eng.cb_admit(seqs[:2], reqs[:2])
    assert eng.cb_step(3) == 2
    slots += eng.cb_admit(seqs[2:], reqs[2:])                  # three prompts of different lengths join the live batch in one pass
    assert eng.prompt_passes() - before == 2
    while eng.cb_step(8) > 0:
        pass
    lv, st = eng.cb_poll()
    for i, s in enumerate(slots):
        assert lv[s] == 0 and st[s] == want[i].numel(), (i, st[s])
        assert torch.equal(eng.cb_read(s, 0, st[s]), want[i]), f"request {i} differs from its solo run"
    eng.cb_reset()
    # resources short: refused as a whole, nothing admitted (two of the eight slots -- and their pages -- are taken, seven more requests cannot fit)
    a = eng.cb_admit(_embeds([100, 90], cfg.hidden, 52), [dict(max_new_tokens=100, eos_token_id=-1)] * 2)
    with pytest.raises(StarVectorBusy):
        eng.cb_admit(_embeds([120, 30, 7, 64, 65, 99, 12], cfg.hidden, 53), [dict(max_new_tokens=70, eos_token_id=-1)] * 7)
    lv, _ = eng.cb_poll()
    assert sum(lv) == 2 and sorted(a) == [0, 1]
    eng.cb_reset()
    eng.close()


@pytest.mark.parametrize("num_beams", [1, 2])
@pytest.mark.parametrize("side", ["left", "right"])
def test_mirror_padded_mask_is_one_ragged_prompt_pass_and_equals_the_unpadded_solo_runs(side, num_beams):
    from starvector_amd.model import HipCausalLM
    cfg, eng = _tiny_engine("v1", max_batch=16, max_seq_len=200)
    lm = HipCausalLM(eng, eos_token_id=-1, pad_token_id=0)
    lens = [70, 9, 64, 33, 65]
    seqs = _embeds(lens, cfg.hidden, 61)
    S, n_new = max(lens), 18
    emb = torch.zeros(len(lens), S, cfg.hidden, dtype=torch.bfloat16, device=dev())
    mask = torch.zeros(len(lens), S, dtype=torch.long, device=dev())
    for b, x in enumerate(seqs):
        sl = slice(S - lens[b], S) if side == "left" else slice(0, lens[b])
        emb[b, sl] = x
        mask[b, sl] = 1
    solo = [lm.generate(inputs_embeds=x[None].contiguous(), max_length=x.shape[0] + n_new, num_beams=num_beams).cpu()[0] for x in seqs]
    before = eng.prompt_passes()
    out = lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=S + n_new, num_beams=num_beams).cpu()
    assert eng.prompt_passes() - before == 1                   # one prompt pass for five prompts of five lengths
    assert out.shape == (len(lens), n_new)
    for b in range(len(lens)):
        assert torch.equal(out[b], solo[b]), (side, num_beams, b)
    eng.close()
