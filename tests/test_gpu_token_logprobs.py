"""GPU: per-token log-probs of the scoring forward (sv_forward_logprobs, csrc/score.hip): the kernel on synthetic rows against
float64, the chunked lm_head bit for bit against sv_forward_logits, the HF golden, the footprint at StarVector-1B size, and
the pass as an exclusive job beside a generation request."""
import dataclasses
import gc
import os
import time

import pytest
import torch

import starvector_amd as sva
from starvector_amd import engine as E
from oracle import starvector_oracle as O
from tests.gpu_util import bf, build_engine, dev
from tests.test_gpu_e2e import LOGIT_TOL

pytestmark = pytest.mark.gpu

EPS32 = float(torch.finfo(torch.float32).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _first_max_index(rows):
    """Lowest index holding each row's maximum (torch.argmax does not promise which of several maxima it returns)."""
    V = rows.shape[-1]
    idx = torch.arange(V, device=rows.device).expand_as(rows)
    return torch.where(rows == rows.max(-1, keepdim=True).values, idx, torch.full_like(idx, V)).min(-1).values


def _f64_reference(rows_bf16, temperature):
    """float64 logsumexp / log_softmax / entropy of softmax(x), x = the bf16 values / temperature; p = 0 terms add 0."""
    x = rows_bf16.double() / temperature
    lse = torch.logsumexp(x, -1)
    logp = x - lse.unsqueeze(-1)
    p = logp.exp()
    ent = -torch.where(p > 0, p * logp, torch.zeros_like(p)).sum(-1)
    return lse, logp, ent


def _f32_torch(rows_bf16, temperature):
    """torch's own float32 arithmetic on the same rows (scaled by the float32 reciprocal like the kernel): the yardstick of what
    float32 can do here -- the kernel differs from it by summation order only."""
    x = rows_bf16.float() * torch.tensor(1.0 / temperature, dtype=torch.float32, device=rows_bf16.device)
    lse = torch.logsumexp(x, -1)
    logp = torch.log_softmax(x, -1)
    p = logp.exp()
    ent = -torch.where(p > 0, p * logp, torch.zeros_like(p)).sum(-1)
    return lse, logp, ent


def _dev_err(a, ref):
    """largest |a - ref| over entries where ref is finite; non-finite entries must agree exactly"""
    fin = torch.isfinite(ref)
    assert torch.equal(a.double()[~fin], ref[~fin]), "non-finite entries differ"
    return float((a.double()[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0


# ---- 1. the operator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [49156, 49157, 516])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_logprob_rows_operator(V, temperature):
    """sv_op_logprob_rows on 64 synthetic bf16 rows against float64.  Tolerance: 4 x the largest deviation of torch's own float32
    log_softmax / logsumexp / entropy of the same rows from float64 (the kernel and torch differ by summation order only)."""
    R, ld = 64, (V + 7) // 8 * 8
    g = torch.Generator(device="cpu").manual_seed(1000 + V)
    rows = torch.randn(R, V, generator=g) * 3.0
    minf = torch.rand(R, V, generator=g) < 0.3
    rows[0:4] = rows[0:4].masked_fill(minf[0:4], float("-inf"))                      # rows with -inf entries
    rows[4:8] = (torch.rand(4, V, generator=g) * 160.0 - 80.0)                       # magnitudes of +-80: no overflow
    rows[4, 0], rows[5, V - 1] = 80.0, -80.0
    tie_expect = {}
    for r, cols in [(8, (5, 300, V - 1)), (9, (V - 2, V - 1)), (10, (0, V - 1)), (11, (17, 18))]:
        rows[r, list(cols)] = 20.0 + r                                              # an exact tie at the maximum: the lowest index wins
        tie_expect[r] = min(cols)
    rows[12] = float("-inf")
    rows[12, 33] = 1.5                                                               # one finite value: lse = x, entropy 0
    rows = rows.to(torch.bfloat16)
    buf = torch.full((R, ld), 1000.0, dtype=torch.bfloat16)                          # the padding columns hold junk above every logit
    buf[:, :V] = rows
    targets = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    targets[0] = int(minf[0].nonzero()[0])                                           # a target whose logit is -inf
    targets[12] = 33
    targets[13] = V - 1
    targets[20], targets[21], targets[22] = -100, V, -5
    good = torch.ones(R, dtype=torch.bool)
    good[20:23] = False
    rows_d, tg = rows.to(dev()), targets.to(dev())
    lp, lse, ent, am, flag = E.op_logprob_rows(buf.to(dev()), tg, temperature, valid=V)
    assert flag == (1, 21), flag                                                     # out-of-range targets: flagged, first at row 21
    assert float(lp[20]) == 0.0 and bool(torch.isnan(lp[21])) and bool(torch.isnan(lp[22]))

    lse64, logp64, ent64 = _f64_reference(rows_d, temperature)
    lse32, logp32, ent32 = _f32_torch(rows_d, temperature)
    gi = good.to(dev()).nonzero().flatten()
    pick = tg[gi].long().unsqueeze(-1)
    want_lp = logp64[gi].gather(-1, pick).squeeze(-1)
    tol_lp = 4.0 * _dev_err(logp32, logp64)
    tol_lse = 4.0 * _dev_err(lse32, lse64)
    tol_ent = 4.0 * _dev_err(ent32, ent64)
    e_lp, e_lse, e_ent = _dev_err(lp[gi], want_lp), _dev_err(lse, lse64), _dev_err(ent, ent64)
    print(f"[logprob_rows V={V} T={temperature}] |kernel - f64|: logprob {e_lp:.3e} (allowed {tol_lp:.3e} = 4 x torch fp32), "
          f"logsumexp {e_lse:.3e} (allowed {tol_lse:.3e}), entropy {e_ent:.3e} (allowed {tol_ent:.3e})")
    assert tol_lp > 0 and tol_lse > 0 and tol_ent > 0
    assert e_lp <= tol_lp and e_lse <= tol_lse and e_ent <= tol_ent
    assert float(lp[0]) == float("-inf")                                             # log-prob of a -inf logit
    assert abs(float(ent[12])) <= tol_ent and abs(float(lse[12]) - 1.5 / temperature) <= 2 * EPS32 * 1.5 / temperature
    # arg-max: exact wherever the maximum is unique or tied by design (every row here: _first_max_index is the rule itself)
    assert torch.equal(am.long(), _first_max_index(rows_d.float()))
    for r, c in tie_expect.items():
        assert int(am[r]) == c, (r, int(am[r]), c)
    # outputs of flagged-target rows other than logprob are still written
    assert _dev_err(lse[20:23], lse64[20:23]) <= tol_lse

    # rows without a finite logit: every output NaN, arg-max -1, flag code 2 with the first such row
    bad = torch.zeros(3, ld, dtype=torch.bfloat16)
    bad[1] = float("-inf")
    bad[2] = float("nan")
    lp, lse, ent, am, flag = E.op_logprob_rows(bad.to(dev()), torch.zeros(3, dtype=torch.int32, device=dev()), temperature, valid=V)
    assert flag == (2, 1), flag
    assert am.tolist()[1:] == [-1, -1] and int(am[0]) == 0
    for t in (lp, lse, ent):
        assert bool(torch.isnan(t[1:]).all()) and bool(torch.isfinite(t[0]))


# ---- 2. exactness underneath ------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_identity(r, logits, targets, temperature):
    """logprob + logsumexp = logit[target] / temperature to one float32 rounding of that sum; arg-max = first maximal index."""
    tg = targets.long()
    real = tg != -100
    x_t = logits.float().gather(-1, tg.clamp(min=0).unsqueeze(-1)).squeeze(-1) / temperature
    s = r.logprobs + r.logsumexp
    bound = 2 * EPS32 * torch.maximum(r.logprobs.abs(), r.logsumexp.abs())
    worst = float(((s - x_t).abs() - bound)[real].max())
    assert worst <= 0.0, f"logprob + logsumexp misses logit[target] / T by {worst:.3e} over the bound"
    if bool((~real).any()):
        assert float(r.logprobs[~real].abs().max()) == 0.0                           # -100: log-prob 0
    flat = logits.float().reshape(-1, logits.shape[-1])
    assert torch.equal(r.argmax.reshape(-1).long(), _first_max_index(flat))


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_chunked_lm_head_is_bit_identical(family):
    """B = 8, S = 110, n_keep = 90 on the tiny model: 720 rows = two full 256-row chunks + a 208-row remainder with the chunk forced
    to 256 rows.  Chunk 256, chunk 512 and the default give bit-identical outputs; they are exactly what the kernel makes of the rows
    sv_forward_logits returns for the same (B, S, n_keep)."""
    cfg = O.OracleConfig.tiny() if family == "v1" else O.OracleConfig.tiny_v2()
    w = O.make_weights(cfg, seed=97)
    eng = build_engine(cfg, w, max_batch=8, max_seq_len=128)
    B, S, n = 8, 110, 90
    g = torch.Generator().manual_seed(5)
    emb = eng.embed_tokens(torch.randint(0, cfg.vocab, (B, S), generator=g).to(dev()))
    targets = torch.randint(0, cfg.vocab, (B, n), generator=g)
    targets[1, 3], targets[7, 89] = -100, -100
    targets = targets.to(dev())
    for temperature in (1.0, 0.5):
        outs = []
        for chunk in (256, 512, 0):
            eng.set_score_chunk_rows(chunk)
            outs.append(eng.forward_logprobs(emb, targets, n, temperature, entropy=True, argmax=True))
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert torch.equal(_bits(a), _bits(b)), "outputs depend on the chunk size"
        logits = eng.forward_logits(emb, n)
        assert logits.shape == (B, n, cfg.vocab)
        _check_identity(outs[0], logits, targets, temperature)
        # the rows underneath are sv_forward_logits' rows bit for bit: the same kernel over them gives the same bits
        ld = (cfg.vocab + 7) // 8 * 8
        rows = torch.zeros(B * n, ld, dtype=torch.bfloat16, device=dev())
        rows[:, :cfg.vocab] = logits.reshape(B * n, cfg.vocab)
        lp, lse, ent, am, flag = E.op_logprob_rows(rows, targets.reshape(-1).to(torch.int32), temperature, valid=cfg.vocab)
        assert flag[0] == 0
        for a, b in zip(outs[0], (lp, lse, ent, am)):
            assert torch.equal(_bits(a).reshape(-1), _bits(b)), "chunked lm_head rows differ from sv_forward_logits' rows"
    # a target outside the vocabulary: ValueError naming the row; the engine stays usable
    bad = targets.clone()
    bad[2, 5] = cfg.vocab
    with pytest.raises(ValueError, match=r"row %d \(sequence 2, kept position 5\)" % (2 * n + 5)):
        eng.forward_logprobs(emb, bad, n)
    again = eng.forward_logprobs(emb, targets, n, 0.5, entropy=True, argmax=True)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, outs[0]))
    eng.close()


# ---- 3. against the reference -----------------------------------------------------------------------------------------------
def test_logprobs_against_hf_golden():
    """tests/golden/tiny_forward holds HF's logits of the pinned forward case.  |engine log-prob - float64 log_softmax(golden)[id]|
    <= 2 x LOGIT_TOL x max|logit|: a log-prob is a difference of two quantities that each move by at most the bf16 band."""
    from safetensors.torch import load_file
    gold = load_file(os.path.join(GOLDEN, "tiny_forward.safetensors"))
    seed, B, n_ids = [int(x) for x in gold["meta"]]
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=seed)
    scfg = sva.StarVectorConfig(image_size=cfg.image_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.n_layer,
                                num_attention_heads=cfg.n_head, vocab_size=cfg.vocab - 4, n_inner=cfg.n_inner,
                                n_positions=cfg.n_positions, max_length=cfg.n_positions, vit_width=cfg.vit_width,
                                vit_layers=cfg.vit_layers, vit_heads=cfg.vit_heads, max_batch=4)
    model = sva.StarVectorForCausalLM(scfg, state_dict={k: v.to(torch.bfloat16) for k, v in w.items()})
    eng = model.engine
    ids = gold["ids"].to(dev())
    vis = eng.adapter(eng.encode_image(bf(gold["image"])))
    emb = torch.cat([vis, eng.embed_tokens(ids)], 1)
    hf = gold["logits_keep5"].double()                                               # [B, 5, V]: the last five positions
    tol = 2 * LOGIT_TOL * float(hf.abs().max())
    # row j of the five predicts ids[:, -4 + j]; the last row has no next id in the case: an arbitrary one
    targets = torch.cat([ids[:, -4:], torch.full((B, 1), 7, device=dev(), dtype=ids.dtype)], 1)
    want = torch.log_softmax(hf, -1).gather(-1, targets.cpu().unsqueeze(-1)).squeeze(-1)
    got = eng.forward_logprobs(emb, targets, 5)
    err = float((got.logprobs.double().cpu() - want).abs().max())
    print(f"[golden] |engine log-prob - HF float64| {err:.3e} (allowed {tol:.3e})")
    assert err <= tol
    # the mirror: the same case through completion_logprobs, one completion per image
    v1 = model.model.image_projection(model.model.image_encoder(bf(gold["image"][:1])))
    S = v1.shape[1] + ids.shape[1]
    out = model.completion_logprobs(v1, ids[:1], 1, torch.ones(1, S, device=dev()), 4)
    assert out.shape == (1, 4) and out.dtype == torch.float32
    assert float((out.double().cpu() - want[:1, :4]).abs().max()) <= tol
    # the left-padded row of the case (mask 0 0 1 ... 1; HF's own logits of the masked batch) beside an unpadded one
    mask = torch.ones(2, S, device=dev())
    mask[0, :2] = 0
    out2, ent2 = model.completion_logprobs(v1, ids[:1].repeat(2, 1), 2, mask, 4, return_entropy=True)
    hf_lp = gold["logits_leftpad2_row0_keep5"].double()                              # [5, V]
    tol_lp = 2 * LOGIT_TOL * float(hf_lp.abs().max())
    logp_lp = torch.log_softmax(hf_lp, -1)
    want_lp = logp_lp[:4].gather(-1, ids[0, -4:].cpu().unsqueeze(-1)).squeeze(-1)
    err = float((out2[0].double().cpu() - want_lp).abs().max())
    print(f"[golden, left-padded row] |engine log-prob - HF float64| {err:.3e} (allowed {tol_lp:.3e})")
    assert err <= tol_lp
    assert torch.equal(_bits(out2[1]), _bits(out[0])), "unpadded row changed by its neighbour's padding"
    assert ent2.shape == (2, 4) and bool((ent2 > 0).all())
    eng.close()


# ---- 4. footprint at real size ----------------------------------------------------------------------------------------------
def test_footprint_and_values_at_starvector_1b_size():
    """StarVector-1B dimensions, seeded random weights, B = 4, S = 2305, n_keep = 2048: 8192 rows.  The logits tensor alone would be
    805 MB and sv_forward_logits' workspace another 811 MB; the first forward_logprobs call may take the documented chunk workspace
    (4096 rows x Vpad 49184 x 2 B = 403 MB) + the two [rows][hidden] buffers (67 MB) + 64 MiB of allocator slack.  (The decoder's own
    prompt-pass workspace and GEMM tuning, common to every entry point, are paid by a prefill of the same shape beforehand.)"""
    cfg = dataclasses.replace(O.OracleConfig(), eos_token_id=-1)
    w = O.make_weights(cfg, seed=1234)
    B, S, n = 4, 2305, 2048
    eng = build_engine(cfg, w, max_batch=B, max_seq_len=S + 7)
    del w
    gc.collect()
    g = torch.Generator().manual_seed(11)
    emb = eng.embed_tokens(torch.randint(0, cfg.vocab, (B, S), generator=g).to(dev()))
    targets = torch.randint(0, cfg.vocab, (B, n), generator=g).to(dev())
    eng.prefill(emb)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    idle0 = torch.cuda.mem_get_info()[0]
    time.sleep(1.0)
    idle1 = torch.cuda.mem_get_info()[0]
    before = torch.cuda.mem_get_info()[0]
    r = eng.forward_logprobs(emb, targets, n, 1.0, entropy=True, argmax=True)
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    vpad = (cfg.vocab + 31) // 32 * 32
    allowed = 4096 * vpad * 2 + 2 * B * n * cfg.hidden * 2 + (64 << 20)
    print(f"[footprint] free memory dropped by {(before - after) / 1e6:.1f} MB over the first forward_logprobs call "
          f"(allowed {allowed / 1e6:.1f} MB; the logits alone would be {B * n * cfg.vocab * 2 / 1e6:.0f} MB)")
    if abs(idle1 - idle0) > (16 << 20):
        print(f"[footprint] assertion skipped: free memory moved by {(idle1 - idle0) / 1e6:.1f} MB while this process was idle "
              "(another tenant is allocating on this GPU)")
    else:
        assert before - after <= allowed, f"{(before - after) / 1e6:.1f} MB > {allowed / 1e6:.1f} MB"
    # values on 512 evenly spaced rows
    logits = eng.forward_logits(emb, n)
    sel = torch.arange(0, B * n, (B * n) // 512, device=dev())[:512]
    rows = logits.reshape(B * n, cfg.vocab)[sel]
    tg = targets.reshape(-1)[sel]
    lse64, logp64, ent64 = _f64_reference(rows, 1.0)
    lse32, logp32, ent32 = _f32_torch(rows, 1.0)
    tol = 4.0 * _dev_err(logp32, logp64)
    want = logp64.gather(-1, tg.unsqueeze(-1)).squeeze(-1)
    err = _dev_err(r.logprobs.reshape(-1)[sel], want)
    print(f"[1B-size values] |logprob - f64| {err:.3e} (allowed {tol:.3e} = 4 x torch fp32's own deviation)")
    assert tol > 0 and err <= tol
    pick = E.TokenLogprobs(r.logprobs.reshape(-1)[sel], r.logsumexp.reshape(-1)[sel], None, r.argmax.reshape(-1)[sel])
    _check_identity(pick, rows, tg, 1.0)
    eng.close()
    del logits, rows, lse64, logp64, ent64, lse32, logp32, ent32
    gc.collect(); torch.cuda.empty_cache()


# ---- 5. beside a generation request -----------------------------------------------------------------------------------------
def test_completion_logprobs_queue_behind_a_generation_request():
    """With a ContinuousBatcher attached and a generation request in flight, completion_logprobs runs as an exclusive job: the
    same numbers as on the idle engine, and the generation's tokens are unchanged."""
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=41)
    scfg = sva.StarVectorConfig(image_size=cfg.image_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.n_layer,
                                num_attention_heads=cfg.n_head, vocab_size=cfg.vocab - 4, n_inner=cfg.n_inner,
                                n_positions=cfg.n_positions, max_length=cfg.n_positions, vit_width=cfg.vit_width,
                                vit_layers=cfg.vit_layers, vit_heads=cfg.vit_heads, max_batch=4)
    model = sva.StarVectorForCausalLM(scfg, state_dict={k: v.to(torch.bfloat16) for k, v in w.items()})
    eng = model.engine
    img = O.synthetic_images(1, cfg.image_size, seed=42)
    vis = eng.adapter(eng.encode_image(bf(img)))
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, cfg.vocab - 4, (2, 12), generator=g).to(dev())
    mask = torch.ones(2, vis.shape[1] + 12, device=dev())
    mask[1, -3:] = 0
    idle, idle_ent = model.completion_logprobs(vis, ids, 2, mask, 10, temperature=0.9, return_entropy=True)
    prompt = torch.cat([vis, eng.embed_tokens(ids[:1, :4])], 1)
    n_new = 100
    alone = eng.generate(prompt, max_length=prompt.shape[1] + n_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id).cpu()
    lm = model.model.svg_transformer.transformer
    lm.batcher = sva.ContinuousBatcher(eng, steps_per_poll=1)
    try:
        req = lm.batcher.submit(prompt, dict(max_new_tokens=n_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id))
        t0 = time.time()
        while lm.batcher.steps_run == 0 and time.time() - t0 < 60:
            time.sleep(0.001)
        in_flight = lm.batcher.steps_run > 0 and not req.done.is_set()
        busy, busy_ent = model.completion_logprobs(vis, ids, 2, mask, 10, temperature=0.9, return_entropy=True)
        toks = req.result(timeout=120).cpu()
    finally:
        lm.batcher.close()
        lm.batcher = None
    assert in_flight, "the generation request was not in flight when the scoring pass was queued"
    assert torch.equal(_bits(busy), _bits(idle)) and torch.equal(_bits(busy_ent), _bits(idle_ent))
    assert torch.equal(toks.reshape(-1), alone.reshape(-1)), "the generation's tokens changed"
    assert float(idle[1, -3:].abs().max()) == 0.0 and float(idle[0].abs().min()) > 0.0
    eng.close()
