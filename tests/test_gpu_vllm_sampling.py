"""-m gpu: vLLM 0.5.5 sampler semantics in the continuous-batching step (sampling.hip, cb_step_kernel) and the offline
`LLM` / `SamplingParams` API (star-vector_amd/vllm.py).  The contract is restated in torch below (`_processed`, `_kept`):
logit_bias -> min_tokens hold -> repetition over prompt + output ids -> frequency and presence over the output counts ->
greedy argmax, or temperature -> top-k -> top-p -> min_p -> one draw."""
import os

import numpy as np
import pytest
import torch

import starvector_amd.engine as E
from oracle import starvector_oracle as O
from starvector_amd import vllm as VL
from tests.gpu_util import bf, build_engine, dev
from tests.test_gpu_e2e import LOGIT_TOL

pytestmark = pytest.mark.gpu
VOC = 49157                      # StarVector-8B's vocabulary: odd, covers the row tail
ROWS = 64


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _processed(l, r, hist):
    """fp32 logits row after vLLM's processors (steps 1-3 of the contract)."""
    l = l.clone().float()
    V = l.numel()
    for t, b in (r.get("logit_bias") or {}).items():
        l[t] += max(-100.0, min(100.0, float(b)))
    if len(hist) < r.get("min_new_tokens", 0):
        if r.get("eos_token_id", 0) >= 0:
            l[r.get("eos_token_id", 0)] = -float("inf")
        for t in r.get("stop_any_ids") or []:
            l[t] = -float("inf")
    seen = torch.zeros(V, dtype=torch.bool)
    ids = list(r.get("prompt_ids") or []) + list(hist)
    if ids:
        seen[torch.tensor(ids)] = True
    rp = float(r.get("repetition_penalty", 1.0))
    l = torch.where(seen, torch.where(l > 0, l / rp, l * rp), l)
    cnt = torch.bincount(torch.tensor(list(hist), dtype=torch.long), minlength=V).float() if hist else torch.zeros(V)
    l = l - float(r.get("frequency_penalty", 0.0)) * cnt
    l = l - float(r.get("presence_penalty", 0.0)) * (cnt > 0).float()
    return l


def _kept(l, temperature, top_k, top_p, min_p, slack=0.0, minp_first=False):
    """Boolean kept set of the sampling path on processed logits l (steps 5-6); slack > 0 loosens every threshold."""
    s = l.double() / temperature
    keep = torch.isfinite(s)
    if top_k > 0:
        keep &= s >= s.topk(top_k).values[-1]

    def top_p_cut(keep):
        if top_p >= 1.0:
            return keep
        p = torch.where(keep, s, torch.tensor(-float("inf"), dtype=s.dtype)).softmax(-1)
        order = p.argsort()
        cum = p[order].cumsum(0)
        drop = cum <= (1.0 - top_p) - slack
        drop[-1] = False
        k2 = keep.clone()
        k2[order[drop]] = False
        return k2

    def min_p_cut(keep):
        if min_p <= 0.0:
            return keep
        return keep & ((s - s[keep].max()).exp() >= min_p * (1.0 - slack) - 1e-12)

    return top_p_cut(min_p_cut(keep)) if minp_first else min_p_cut(top_p_cut(keep))


def _margin_ok(l, tok, tol):
    """greedy equality where the restated row has a clear winner: a different token is only allowed within tol of the max."""
    return float(l.max() - l[tok]) <= tol


def _rows(seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(ROWS, VOC, generator=g)


def _hist_prompt(lg, b, g):
    """A row's output history and prompt ids built around its own top tokens, so that every processor moves the winner."""
    top = lg[b].topk(6).indices.tolist()
    hist = [top[0], top[0], top[1], int(torch.randint(0, VOC, (1,), generator=g))]
    prompt = [top[2], top[3], int(torch.randint(0, VOC, (1,), generator=g))]
    return hist, prompt


# ---- 1. the operator (sv_op_cb_select: cb_step_kernel itself) ---------------------------------------------------------------
def test_op_greedy_processors_match_the_restatement():
    lg = _rows(1)
    g = torch.Generator().manual_seed(2)
    hp = [_hist_prompt(lg, b, g) for b in range(ROWS)]
    bias_ids = [lg[b].topk(8).indices[5].item() for b in range(ROWS)]
    configs = {
        "bias": lambda b: dict(logit_bias={bias_ids[b]: 1.5, int(lg[b].argmax()): -0.7}),
        "repetition": lambda b: dict(repetition_penalty=1.6),
        "frequency": lambda b: dict(frequency_penalty=0.9),
        "presence": lambda b: dict(presence_penalty=1.3),
        "combined": lambda b: dict(logit_bias={bias_ids[b]: 0.8}, repetition_penalty=1.2, frequency_penalty=0.4,
                                   presence_penalty=-0.3),
    }
    raw = lg.argmax(-1)
    for name, extra in configs.items():
        reqs = [dict(semantics="vllm", max_new_tokens=64, eos_token_id=-1, prompt_ids=hp[b][1], **extra(b)) for b in range(ROWS)]
        got = E.op_cb_select(lg.to(dev()), reqs, [hp[b][0] for b in range(ROWS)]).long()
        moved = 0
        for b in range(ROWS):
            ref = _processed(lg[b], reqs[b], hp[b][0])
            assert _margin_ok(ref, int(got[b]), 1e-4), (name, b, int(got[b]), int(ref.argmax()))
            moved += int(ref.argmax() != raw[b])
        assert moved >= ROWS // 4, (name, moved)              # the rows are designed so that the processor changes the winner


def test_op_bias_forces_and_forbids():
    lg = _rows(3)
    forced = [int(x) for x in torch.randint(0, VOC, (ROWS,), generator=torch.Generator().manual_seed(4))]
    for do_sample in (False, True):
        base = dict(semantics="vllm", max_new_tokens=8, eos_token_id=-1, do_sample=do_sample, temperature=1.0, top_k=50,
                    seed=9)
        got = E.op_cb_select(lg.to(dev()), [dict(base, logit_bias={forced[b]: 100.0}) for b in range(ROWS)]).long()
        assert got.tolist() == forced
        got = E.op_cb_select(lg.to(dev()), [dict(base, logit_bias={forced[b]: 1e6}) for b in range(ROWS)]).long()
        assert got.tolist() == forced                          # clamped to +100, still forced
    top2 = lg.topk(2, -1).indices
    got = E.op_cb_select(lg.to(dev()), [dict(semantics="vllm", max_new_tokens=8, logit_bias={int(top2[b, 0]): -100.0})
                                        for b in range(ROWS)]).long()
    assert got.tolist() == top2[:, 1].tolist()


def test_op_min_tokens_holds_eos_and_stop_ids():
    lg = _rows(5)
    top3 = lg.topk(3, -1).indices
    reqs = [dict(semantics="vllm", max_new_tokens=8, eos_token_id=int(top3[b, 0]), stop_any_ids=[int(top3[b, 1])],
                 min_new_tokens=2) for b in range(ROWS)]
    assert E.op_cb_select(lg.to(dev()), reqs, [[1]] * ROWS).long().tolist() == top3[:, 2].tolist()     # step 1 < 2: held
    assert E.op_cb_select(lg.to(dev()), reqs, [[1, 2]] * ROWS).long().tolist() == top3[:, 0].tolist()  # step 2: released


def test_op_min_p_one_equals_greedy():
    lg = _rows(6)
    greedy = lg.argmax(-1)
    for top_k in (0, 50):
        reqs = [dict(semantics="vllm", max_new_tokens=8, do_sample=True, temperature=0.7, top_p=0.9, top_k=top_k, min_p=1.0,
                     seed=1000 + b) for b in range(ROWS)]
        assert E.op_cb_select(lg.to(dev()), reqs).long().tolist() == greedy.tolist()


def _order_row():
    """Probabilities 0.45 / 0.30 / 0.15 / 0.10 on four ids, the rest negligible: with top_p 0.8 and min_p 0.3, top-p THEN min_p
    keeps {0.45, 0.30, 0.15}; min_p first would renormalise and top-p would then drop 0.15."""
    row = torch.full((VOC,), -40.0)
    ids = [17, 20011, 33333, VOC - 1]
    for i, p in zip(ids, (0.45, 0.30, 0.15, 0.10)):
        row[i] = float(np.log(p))
    return row, ids


def test_op_sampled_tokens_lie_in_the_kept_set():
    lg = _rows(7)
    g = torch.Generator().manual_seed(8)
    hp = [_hist_prompt(lg, b, g) for b in range(ROWS)]
    row, ids = _order_row()
    assert not torch.equal(_kept(row, 1.0, 0, 0.8, 0.3), _kept(row, 1.0, 0, 0.8, 0.3, minp_first=True))
    lg[:8] = row                                                 # the order-sensitive rows
    settings = [dict(temperature=0.8, top_k=50, top_p=0.9, min_p=0.05), dict(temperature=1.0, top_k=0, top_p=0.8, min_p=0.3),
                dict(temperature=1.3, top_k=0, top_p=1.0, min_p=0.1), dict(temperature=0.6, top_k=200, top_p=0.7, min_p=0.0)]
    seen_third = 0
    for si, st in enumerate(settings):
        for call in range(4):
            reqs = [dict(semantics="vllm", max_new_tokens=64, eos_token_id=-1, do_sample=True, seed=97 * call + b,
                         prompt_ids=hp[b][1] if b >= 8 else [], repetition_penalty=1.1 if b >= 8 else 1.0,
                         frequency_penalty=0.2 if b >= 8 else 0.0, **st) for b in range(ROWS)]
            hists = [hp[b][0] + [call] if b >= 8 else [call] * call for b in range(ROWS)]
            got = E.op_cb_select(lg.to(dev()), reqs, hists).long()
            for b in range(ROWS):
                ref = _processed(lg[b], reqs[b], hists[b])
                keep = _kept(ref, st["temperature"], st["top_k"], st["top_p"], st["min_p"], slack=1e-4)
                assert bool(keep[got[b]]), (si, call, b, int(got[b]))
                if b < 8 and si == 1:
                    seen_third += int(got[b] == ids[2])
                    assert int(got[b]) != ids[3]
    assert seen_third > 0                                        # the 0.15 token survives: min_p ran AFTER top-p


def test_op_distribution_matches_the_restatement():
    ids = [100, 5000, 20000, 30000, 40000, 45000, 49000, VOC - 1]
    row = torch.full((VOC,), -30.0)
    for i, v in zip(ids, (2.0, 1.8, 1.5, 1.2, 1.0, 0.5, 0.2, -0.5)):
        row[i] = v
    lg = row.repeat(ROWS, 1)
    hist, prompt = [5000, 5000, 20000], [100]
    st = dict(temperature=0.9, top_k=0, top_p=0.95, min_p=0.05)
    base = dict(semantics="vllm", max_new_tokens=64, eos_token_id=-1, do_sample=True, prompt_ids=prompt, repetition_penalty=1.2,
                frequency_penalty=0.3, presence_penalty=0.2, **st)
    ref = _processed(row, base, hist)
    keep = _kept(ref, st["temperature"], 0, st["top_p"], st["min_p"])
    probs = torch.where(keep, ref.double() / st["temperature"], torch.tensor(-float("inf"), dtype=torch.float64)).softmax(-1)
    draws = []
    for call in range(40):
        reqs = [dict(base, seed=(call * ROWS + b) * 7919 + 1) for b in range(ROWS)]
        draws += E.op_cb_select(lg.to(dev()), reqs, [hist] * ROWS).long().tolist()
    n = len(draws)
    cnt = torch.bincount(torch.tensor(draws), minlength=VOC).double()
    assert float(cnt[~keep].sum()) == 0.0
    sel = keep.nonzero().flatten()
    exp = probs[sel] * n
    chi2 = float(((cnt[sel] - exp) ** 2 / exp).sum())
    assert len(sel) >= 4 and chi2 < 35.0, (chi2, cnt[sel].tolist(), exp.tolist())
    assert float((cnt[sel] / n - probs[sel]).abs().sum()) < 0.06


def test_op_neutral_vllm_is_bit_identical_to_the_hf_paths():
    lg = _rows(9)
    g = torch.Generator().manual_seed(10)
    hists = [[int(x) for x in torch.randint(0, VOC, (3,), generator=g)] for _ in range(ROWS)]
    for top_k in (0, 50):
        base = dict(max_new_tokens=64, eos_token_id=-1, do_sample=True, temperature=0.8, top_p=0.9, top_k=top_k)
        hf = E.op_cb_select(lg.to(dev()), [dict(base, seed=500 + b) for b in range(ROWS)], hists)
        vl = E.op_cb_select(lg.to(dev()), [dict(base, seed=500 + b, semantics="vllm") for b in range(ROWS)], hists)
        assert torch.equal(hf, vl)
        for b in range(ROWS):                                    # the classic sampler: row 0 of a one-row call, same (seed, step)
            one = E.op_sample_top_p(lg[b:b + 1].to(dev()).contiguous(), 0.8, 0.9, seed=500 + b, step=3, top_k=top_k).cpu()
            assert int(one[0]) == int(vl[b]), (top_k, b)
    gr = E.op_cb_select(lg.to(dev()), [dict(max_new_tokens=8, semantics="vllm")] * ROWS).long()
    assert torch.equal(gr, lg.argmax(-1))
    even = lg[:, :VOC - 1].contiguous().to(dev())
    assert torch.equal(E.op_cb_select(even, [dict(max_new_tokens=8, semantics="vllm")] * ROWS).cpu(), E.op_argmax(even).cpu())


# ---- 2. end to end on the tiny oracle model ---------------------------------------------------------------------------------
def _tiny(max_batch=8, max_seq_len=96):
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=21)
    eng = build_engine(cfg, w, max_batch=max_batch, max_seq_len=max_seq_len)
    img = bf(O.synthetic_images(4, cfg.image_size, seed=5))
    prompt = [7, 11]
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(torch.tensor([prompt] * 4, device=dev()))], 1)
    return cfg, w, eng, emb, prompt


def _run(eng, emb_row, req):
    s = eng.cb_admit(emb_row.contiguous(), [req])[0]
    while eng.cb_poll()[0][s]:
        eng.cb_step(8)
    n = eng.cb_poll()[1][s]
    toks = eng.cb_read(s, 0, n).tolist()
    eng.cb_release(s)
    return toks


def test_cb_greedy_with_processors_matches_the_oracle_loop():
    cfg, w, eng, emb, prompt = _tiny()
    n_new = 24
    bias_id = 300
    req = dict(semantics="vllm", max_new_tokens=n_new, eos_token_id=-1, prompt_ids=prompt, repetition_penalty=1.3,
               frequency_penalty=0.6, presence_penalty=0.4, logit_bias={bias_id: 0.05})
    for row in range(2):
        got = _run(eng, emb[row:row + 1], req)
        plain = _run(eng, emb[row:row + 1], dict(max_new_tokens=n_new, eos_token_id=-1))
        assert got != plain                                       # the settings change the stream
        lg, cache = O.decoder_prefill(w, cfg, emb[row:row + 1].float().cpu(), mode="bf16")
        hist = []
        for t in range(n_new):
            ref = _processed(lg[0].float(), req, hist)
            tol = 2 * LOGIT_TOL * float(lg[0].abs().max()) * 1.3
            if got[t] != int(ref.argmax()):
                assert _margin_ok(ref, got[t], tol), (row, t, got[t], int(ref.argmax()))
                break                                              # the streams part at a near-tie: nothing after it compares
            hist.append(got[t])
            lg, cache = O.decoder_decode_step(w, cfg, torch.tensor([got[t]]), cache, mode="bf16")
    eng.close()


def test_vllm_request_beside_others_is_identical_to_alone():
    cfg, w, eng, emb, prompt = _tiny()
    target = dict(semantics="vllm", max_new_tokens=30, eos_token_id=-1, do_sample=True, temperature=0.9, top_p=0.9, top_k=0,
                  min_p=0.05, seed=77, prompt_ids=prompt, repetition_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.1,
                  logit_bias={5: 0.5})
    alone = _run(eng, emb[1:2], target)
    eng.cb_reset()
    others = [dict(max_new_tokens=12, eos_token_id=-1),
              dict(max_new_tokens=40, do_sample=True, temperature=1.1, top_p=0.95, top_k=50, seed=3, eos_token_id=-1,
                   repetition_penalty=1.3),
              dict(semantics="vllm", max_new_tokens=25, eos_token_id=-1, frequency_penalty=1.0, prompt_ids=[9])]
    slots = eng.cb_admit(torch.cat([emb[0:1], emb[1:2], emb[2:3], emb[3:4]], 0).contiguous(),
                         [others[0], target, others[1], others[2]])
    while eng.cb_step(8) > 0:
        pass
    n = eng.cb_poll()[1][slots[1]]
    assert eng.cb_read(slots[1], 0, n).tolist() == alone
    eng.close()


def test_counts_and_seen_rows_do_not_leak_into_a_reused_slot():
    cfg, w, eng, emb, prompt = _tiny()
    r2 = dict(semantics="vllm", max_new_tokens=20, eos_token_id=-1, frequency_penalty=0.5, presence_penalty=0.5,
              repetition_penalty=1.5)
    first = _run(eng, emb[0:1], r2)
    eng.cb_reset()
    r1 = dict(semantics="vllm", max_new_tokens=40, eos_token_id=-1, prompt_ids=first[:8] + prompt, frequency_penalty=-0.5)
    s1 = eng.cb_admit(emb[0:1].contiguous(), [r1])[0]
    while eng.cb_step(8) > 0:
        pass
    eng.cb_release(s1)
    s2 = eng.cb_admit(emb[0:1].contiguous(), [r2])[0]
    assert s2 == s1
    while eng.cb_step(8) > 0:
        pass
    assert eng.cb_read(s2, 0, eng.cb_poll()[1][s2]).tolist() == first
    eng.close()


# ---- 3. the facade on a checkpoint directory ---------------------------------------------------------------------------------
def test_llm_generate_on_a_checkpoint(tmp_path):
    from PIL import Image
    from tests.ckpt_util import write_reference_checkpoint
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=21)
    path = str(tmp_path / "ckpt")
    write_reference_checkpoint(path, cfg, w)
    llm = VL.LLM(model=path, max_num_seqs=4, max_model_len=min(96, cfg.n_positions), trust_remote_code=True,
                 byte_tokenizer_fallback=True)
    assert llm.engine.cfg.max_batch == 4
    rng = np.random.default_rng(3)
    images = [Image.fromarray(rng.integers(0, 255, (40 + 7 * i, 48, 3), dtype=np.uint8)) for i in range(6)]
    inputs = [{"prompt": "<image-start>", "multi_modal_data": {"image": im}} for im in images]
    eos = llm.tokenizer.eos_token_id
    sps = [
        VL.SamplingParams(n=2, temperature=0.8, top_p=0.95, min_p=0.05, seed=11, max_tokens=12),
        VL.SamplingParams(n=2, temperature=1.0, top_k=40, frequency_penalty=0.5, presence_penalty=0.2, seed=12, max_tokens=10),
        VL.SamplingParams(n=1, temperature=0.0, max_tokens=9, logit_bias={eos: 100.0}, min_tokens=3),        # EOS
        VL.SamplingParams(n=1, temperature=0.0, max_tokens=9, logit_bias={66: 100.0}, stop_token_ids=[66], min_tokens=2),
        VL.SamplingParams(n=2, temperature=0.7, repetition_penalty=1.3, seed=14, max_tokens=7, ignore_eos=True),   # length
        VL.SamplingParams(n=2, temperature=0.9, top_p=0.9, seed=15, max_tokens=8, logit_bias={70: 2.0}),
    ]
    outs = llm.generate(inputs, sps, use_tqdm=False)
    assert len(outs) == 6 and [len(o.outputs) for o in outs] == [s.n for s in sps]
    jobs = llm.prepare(inputs, sps)
    assert len(jobs) == 10
    eng = llm.engine
    for job in jobs:
        comp = outs[job["input"]].outputs[job["index"]]
        assert comp.index == job["index"] and outs[job["input"]].prompt_token_ids == job["prompt_ids"]
        eng.cb_reset()
        alone = _run(eng, job["emb"], job["params"])
        assert comp.token_ids == alone, (job["input"], job["index"])
        sp = job["sp"]
        cut = len(comp.token_ids) - (1 if comp.finish_reason == "stop" else 0)
        assert comp.text == llm.tokenizer.decode(comp.token_ids[:cut], skip_special_tokens=sp.skip_special_tokens)
    e, s, l = outs[2].outputs[0], outs[3].outputs[0], outs[4].outputs[0]
    assert (e.finish_reason, e.stop_reason, len(e.token_ids), e.token_ids[-1]) == ("stop", None, 4, eos)
    assert (s.finish_reason, s.stop_reason, len(s.token_ids), s.token_ids[-1]) == ("stop", 66, 3, 66)
    assert (l.finish_reason, l.stop_reason, len(l.token_ids)) == ("length", None, 7)
    assert outs[0].outputs[0].token_ids != outs[0].outputs[1].token_ids         # distinct seeds per sample
    eng.cb_reset()
    llm.close()
