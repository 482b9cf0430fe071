"""GPU: the kept SET of Temperature -> TopK -> TopP -> min_p, exactly, in every form the library has of it.

csrc/warp.h and csrc/sample_row.h hold six implementations of one filter -- sample_row_topk (the sampler's fast path), row_warp_stats_regs<16> /
<52> (its fallback), row_warp_stats_select<49> / row_warp_stats_regs<49, ONCE> (the HF output_scores capture and beam-sample) and
row_warp_stats_global (large vocabularies) -- chosen by V, top_k, the candidate count and the calling kernel.  tests/warp_rows.py designs rows
whose kept set is decided by wide margins (tests/test_warper_rows_host.py asserts them on the CPU) and restates HF's warpers in float64
(kept_ref).  Here every caller runs every case and must return that set: no tolerance, no boundary ids.
  capture      sv_op_capture_rows (capture_warp_kernel + capture_write_kernel): isfinite(scores) == kept_ref, kept values = float32 s / T
  beam-sample  one sv_beam_step with sv_debug_beam_set_capture (beam_row_warp_kernel + beam_capture_kernel), min_tokens_to_keep 2, with the
               selection form on and off
  the sampler  1024 draws per case through sample_top_p_kernel, cb_step_kernel (HF and vLLM slots) and lookup_sample_kernel: the SET of drawn
               ids equals kept_ref (every kept id has probability >= 1 / 16: a miss has probability < 1e-27)
Each test prints, with -s, the form every case reached and its kept-set size."""
import os

import pytest
import torch

from starvector_amd import engine as E
from tests import warp_rows as W
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
DRAW_ROWS = 512


def _cases(V, min_keep):
    return [c for c in W.CASES if c.row.numel() == V and c.min_keep == min_keep]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _diff(got, want):
    d = (got ^ want).nonzero().flatten().tolist()
    return f"{len(d)} ids differ, first {d[:8]}: kept on the device {[i for i in d[:8] if got[i]]}"


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------
def _capture(c, ld_in, ld_out, B=3):
    V = c.row.numel()
    src = torch.full((B, ld_in), 100.0)                           # columns >= V of the source would win every maximum if they were read
    src[:, :V] = c.row
    scores = torch.full((B + 1, ld_out), SENTINEL, device=dev())
    logits = torch.full((B + 1, ld_out), SENTINEL, device=dev())
    E.op_capture_rows(src.to(dev()), valid=V, temperature=c.T, top_k=c.top_k, top_p=c.top_p, min_p=c.min_p, scores_out=scores, logits_out=logits)
    return scores.cpu(), logits.cpu()


@pytest.mark.parametrize("V", W.VOCABS)
def test_capture_forms_keep_exactly_the_reference_set(V):
    ld4 = (V + 3) // 4 * 4 + 4
    for c in _cases(V, 1):
        want = W.kept_of(c)
        value = (c.row.double() / W.f32(c.T)).float().masked_fill(~want, W.NEG)        # float32 s / T: the double quotient rounds once
        print(f"capture {c.name}: {W.routes(c)['capture']}, kept {int(want.sum())}")
        for ld_in, ld_out in ((ld4, ld4), (ld4 + 1, ld4 + 3)):                      # 16-byte aligned rows, then neither stride a multiple of 4
            scores, logits = _capture(c, ld_in, ld_out)
            for b in range(3):
                got = torch.isfinite(scores[b, :V])
                assert torch.equal(got, want), (c.name, ld_in, b, _diff(got, want))
                assert torch.equal(_bits(scores[b, :V]), _bits(value)), (c.name, ld_in, b)
                assert torch.equal(_bits(logits[b, :V]), _bits(c.row)), (c.name, ld_in, b)
            for out in (scores, logits):                                               # columns >= V and the row behind the last: untouched
                assert bool((out[:3, V:] == SENTINEL).all()) and bool((out[3] == SENTINEL).all()), (c.name, ld_in)


def test_capture_processors_in_front_of_the_warper():
    """the repetition penalty and the min-length hold change the row the warper sees: a penalised head falls behind its neighbour, the held
    eos leaves the set (kept_ref on the processed row)"""
    c = next(c for c in W.CASES if c.name == "h8-T1.0-k50-cut6-mk1")
    V, heads = c.row.numel(), W.head_cols(c.row.numel())
    seen, eos, pen = [heads[0], 7], heads[1], 2.0                                      # weights 8 and 7: log 8 / 2 lies between log 2 and log 3
    proc = c.row.clone()
    proc[seen] = torch.where(proc[seen] < 0, proc[seen] * pen, proc[seen] / pen)
    proc[eos] = W.NEG
    want = W.kept_ref(proc, c.T, c.top_k, 0.7, 1)                                      # at-or-below masses .04 .13 .25 | .37 ...: cut 0.3
    assert int(want.sum()) == 4 and not bool(want[heads[0]])                           # 6, 5, 4, 3 of the weights 6 5 4 3 2.83 2 1
    src = c.row.to(dev())[None].repeat(2, 1)
    scores, logits = E.op_capture_rows(src, temperature=c.T, top_k=c.top_k, top_p=0.7, seen=[seen, seen], penalty=pen, eos_token_id=eos, hold_eos=True)
    for b in range(2):
        got = torch.isfinite(scores[b].cpu())
        assert torch.equal(got, want), _diff(got, want)
        assert torch.equal(_bits(scores[b].cpu()), _bits(proc.masked_fill(~want, W.NEG)))
        assert torch.equal(_bits(logits[b].cpu()), _bits(c.row))
    greedy, _ = E.op_capture_rows(src, do_sample=False, seen=[seen, seen], penalty=pen, eos_token_id=eos, hold_eos=True)
    assert torch.equal(_bits(greedy[0].cpu()), _bits(proc))                            # no warper: the processed row itself


# ---- beam-sample -------------------------------------------------------------------------------------------------------------------------------
def _beam_step(c, select, ld_out):
    V = c.row.numel()
    old = os.environ.get("SV_BEAM_WARP_SELECT")
    os.environ["SV_BEAM_WARP_SELECT"] = "1" if select else "0"
    try:
        scores = torch.full((2, 4, ld_out), SENTINEL, device=dev())
        logits = torch.full((2, 4, ld_out), SENTINEL, device=dev())
        sc = E.HipBeamScorer(batch=2, num_beams=2, vocab=V, max_new=2, eos_token_id=-1, pad_token_id=0, do_sample=True, temperature=c.T,
                             top_p=c.top_p, top_k=c.top_k, seed=11, capture=(scores, logits))
        try:
            done, parent, tok, _ = sc.step(c.row.to(dev())[None].repeat(4, 1))
        finally:
            sc.close()
    finally:
        if old is None:
            del os.environ["SV_BEAM_WARP_SELECT"]
        else:
            os.environ["SV_BEAM_WARP_SELECT"] = old
    return scores.cpu(), logits.cpu(), tok.tolist()


@pytest.mark.parametrize("V", W.VOCABS)
def test_beam_sample_forms_keep_exactly_the_reference_set(V):
    ld_out = V + 3
    for c in _cases(V, 2):
        want = W.kept_ref(torch.log_softmax(c.row.double(), -1), c.T, c.top_k, c.top_p, 2)
        assert torch.equal(want, W.kept_of(c))
        route = W.routes(c)["beam"]
        print(f"beam-sample {c.name}: {route}, with the selection off {'global' if route == 'global' else 'regs<49,ONCE>'}, kept {int(want.sum())}")
        outs = [_beam_step(c, select, ld_out) for select in (True, False)]
        for scores, logits, tok in outs:
            for r in range(4):
                got = torch.isfinite(scores[0, r, :V])
                assert torch.equal(got, want), (c.name, r, _diff(got, want))
                assert torch.equal(_bits(logits[0, r, :V]), _bits(c.row)), (c.name, r)
            assert bool((scores[0, :, V:] == SENTINEL).all()) and bool((scores[1] == SENTINEL).all()), c.name
            assert bool((logits[0, :, V:] == SENTINEL).all()) and bool((logits[1] == SENTINEL).all()), c.name
            assert all(0 <= t < V and bool(want[t]) for t in tok), (c.name, tok)       # every row has the same logits: the parent does not matter
        assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])), c.name               # selection == bisection, bit for bit
        assert outs[0][2] == outs[1][2], c.name


# ---- the sampler, by draws --------------------------------------------------------------------------------------------------------------------
_ROWS = {}


def _draw_rows(c):
    """DRAW_ROWS copies of the row, built on the device (one buffer per distinct row)"""
    if id(c.row) not in _ROWS:
        _ROWS.clear()                                              # one buffer alive at a time (100 MB at the full vocabulary)
        _ROWS[id(c.row)] = c.row.to(dev())[None].repeat(DRAW_ROWS, 1)
    return _ROWS[id(c.row)]


def _support(tokens, V):
    t = torch.as_tensor(tokens, dtype=torch.int64).flatten().cpu()
    assert bool(((t >= 0) & (t < V)).all()), t[(t < 0) | (t >= V)][:8].tolist()
    return torch.zeros(V, dtype=torch.bool).index_fill_(0, t, True)


def _drawn_by_sampler(c):
    x = _draw_rows(c)
    return _support(torch.cat([E.op_sample_top_p(x, c.T, c.top_p, 2024, step, top_k=c.top_k) for step in (0, 1)]), c.row.numel())


def _drawn_by_cb(c, semantics):
    x, toks = _draw_rows(c), []
    for base in (1000, 5000):                                      # a slot's stream is (its seed, its step, row 0): one seed per row
        reqs = [dict(semantics=semantics, max_new_tokens=4, do_sample=True, temperature=c.T, top_p=c.top_p, top_k=c.top_k, seed=base + b,
                     eos_token_id=-1, **(dict(min_p=c.min_p) if c.min_p else {})) for b in range(DRAW_ROWS)]
        toks.append(E.op_cb_select(x, reqs))
    return _support(torch.cat(toks), c.row.numel())


def _drawn_by_lookup(c):
    x = _draw_rows(c)
    toks = [E.op_lookup_sample(x, 2, [n] * (DRAW_ROWS // 2), temperature=c.T, top_k=c.top_k, top_p=c.top_p, seed=77) for n in (0, 2)]
    return _support(toks[0] + toks[1], c.row.numel())


@pytest.mark.parametrize("V", W.VOCABS)
def test_sampler_forms_draw_exactly_the_reference_set(V):
    cases = [c for c in _cases(V, 1) if W.draw_eligible(c) and not c.min_p]
    assert cases
    for c in cases:
        want = W.kept_of(c)
        print(f"sampler {c.name}: {W.routes(c)['sampler']}, kept {int(want.sum())}")
        got = _drawn_by_sampler(c)
        assert torch.equal(got, want), (c.name, _diff(got, want))


def _one_per_route(cases):
    """per route of sample_row the case with the largest kept set whose top-p is on (its boundary id is what a wrong form drops or adds)"""
    seen, out = set(), []
    for c in sorted(cases, key=lambda c: (c.top_p >= 1.0, -int(W.kept_of(c).sum()))):
        r = W.routes(c)["sampler"]
        if r not in seen:
            seen.add(r)
            out.append(c)
    return out


def test_every_kernel_that_draws_through_sample_row_draws_the_reference_set():
    """cb_step_kernel (an HF slot; a vLLM slot with min_p) and lookup_sample_kernel, one case per route of sample_row"""
    draw = [c for c in W.CASES if W.draw_eligible(c)]
    plain = _one_per_route([c for c in draw if not c.min_p])
    assert {W.routes(c)["sampler"] for c in plain} == {"fast", "fast>TK_PER>regs<52>", "fast>TK_CAP>regs<52>", "regs<16>", "regs<52>", "global"}
    for c in plain:
        want = W.kept_of(c)
        print(f"cb hf slot / lookup {c.name}: {W.routes(c)['sampler']}, kept {int(want.sum())}")
        got = _drawn_by_cb(c, "hf")
        assert torch.equal(got, want), ("cb hf", c.name, _diff(got, want))
        got = _drawn_by_lookup(c)                                  # row s * 2 + j draws with (seed, n_emit + j, s): 1024 distinct triples
        assert torch.equal(got, want), ("lookup", c.name, _diff(got, want))
    minp = [c for c in draw if c.min_p]
    assert {W.routes(c)["sampler"] for c in minp} >= {"fast", "regs<16>", "regs<52>", "global"}
    for c in minp:
        want = W.kept_of(c)
        print(f"cb vllm slot, min_p {c.name}: {W.routes(c)['sampler']}, kept {int(want.sum())}")
        got = _drawn_by_cb(c, "vllm")
        assert torch.equal(got, want), ("cb vllm", c.name, _diff(got, want))


def test_min_p_cases_through_the_capture_equal_the_vllm_slots_draws():
    """min_p has no argument on the plain sampler operator: the capture (row_warp_stats + wp_keep's threshold) and the vLLM slot (sample_row)
    are its two device forms"""
    for c in [c for c in W.CASES if c.min_p and c.row.numel() == 49157 and W.draw_eligible(c)]:
        scores, _ = _capture(c, 49160, 49160, B=1)
        cap = torch.isfinite(scores[0, :49157])
        drawn = _drawn_by_cb(c, "vllm")
        assert torch.equal(cap, W.kept_of(c)) and torch.equal(drawn, cap), (c.name, _diff(drawn, cap))


def test_drawn_support_captured_support_and_reference_are_one_set():
    """the sampler draws through sample_row_topk / row_warp_stats<true, true>, the capture reports through row_warp_stats<false, true>: different
    code.  'The drawn token has a finite captured score' holds because both return kept_ref's set on these rows."""
    names = ("h8-T1.0-k50-cut6-mk1", "h8-T0.7-k50-cut5-mk1", "h8-T1.3-k0-cut5-mk1", "tie-T1.0-k3-p1-mk1", "stride5-T1.0-k50-cut6-mk1",
             "plateau-T1.0-k50-cut6-mk1", "far-T1.0-k2-p0.9-mk1", "v49156-T1.0-k257-cut4-mk1", "v517-T1.0-k50-cut6-mk1", "v53249-T1.0-k0-cut6-mk1")
    for name in names:
        c = next(c for c in W.CASES if c.name == name)
        V = c.row.numel()
        ld = (V + 3) // 4 * 4
        scores, _ = _capture(c, ld, ld, B=1)
        cap, drawn, want = torch.isfinite(scores[0, :V]), _drawn_by_sampler(c), W.kept_of(c)
        r = W.routes(c)
        print(f"cross-form {c.name}: sampler {r['sampler']}, capture {r['capture']}, kept {int(want.sum())}")
        assert torch.equal(cap, want), (name, _diff(cap, want))
        assert torch.equal(drawn, want), (name, _diff(drawn, want))
