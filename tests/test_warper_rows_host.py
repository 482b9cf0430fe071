"""CPU: the designed rows of tests/warp_rows.py are fair.  tests/test_gpu_warper_kept_set.py demands that every device form of the
TopK -> TopP -> min_p warper returns EXACTLY kept_ref's set on them; this file establishes, per case, the conditions on the INPUTS that make
that a fair demand (they are no tolerances):
  1. HF's own code in float32 -- the oracle's warp_scores and, where it imports, transformers' warper classes -- keeps exactly kept_ref's set
  2. no two ids of equal probability straddle the top-p cut (the device keeps a tie group whole, HF cuts inside it)
  3. every id's at-or-below cumulative mass (float64) is at least 1e-4 away from 1 - top_p
  4. every min_p threshold is at least 1e-4 (relative) away from any id's probability ratio
  5. float32 x / T (HF) and x * (1.0f / T) (the device's score functor) rank the row alike, with the same ties
  6. a neighbouring parameter changes the kept set by exactly one id: a form that is off by one id cannot pass
  7. every case the draw tests use keeps ids of renormalised probability >= 1 / 16 only
and that the list reaches every form of every caller."""
import pytest
import torch

from oracle import starvector_oracle as O
from tests import warp_rows as W

try:
    from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
except Exception:                                                  # the pin is optional: the oracle restates these classes
    TopKLogitsWarper = None

MARGIN = 1e-4
IDS = [c.name for c in W.CASES]


def _inputs(c):
    """the float32 rows a caller warps: the row itself; beam-sample (min_tokens_to_keep 2) warps its log_softmax"""
    return [c.row] + ([torch.log_softmax(c.row, -1)] if c.min_keep == 2 else [])


@pytest.mark.parametrize("c", W.CASES, ids=IDS)
def test_hf_in_float32_keeps_the_reference_set(c):
    want = W.kept_of(c)
    for x in _inputs(c):
        assert torch.equal(W.kept_ref(x, c.T, c.top_k, c.top_p, c.min_keep, c.min_p), want)          # float64, shift invariance
        if not c.min_p:
            got = torch.isfinite(O.warp_scores(x[None], c.T, c.top_p, c.top_k, c.min_keep)[0])
            assert torch.equal(got, want), (got ^ want).nonzero().flatten().tolist()
        if TopKLogitsWarper is not None:
            s = TemperatureLogitsWarper(float(c.T))(None, x[None].clone()) if c.T != 1.0 else x[None].clone()
            if c.top_k > 0:
                s = TopKLogitsWarper(top_k=int(c.top_k), min_tokens_to_keep=c.min_keep)(None, s)
            if c.top_p < 1.0:
                s = TopPLogitsWarper(top_p=float(c.top_p), min_tokens_to_keep=c.min_keep)(None, s)
            if c.min_p > 0.0:
                s = MinPLogitsWarper(min_p=float(c.min_p), min_tokens_to_keep=c.min_keep)(None, s)
            got = torch.isfinite(s[0])
            assert torch.equal(got, want), (got ^ want).nonzero().flatten().tolist()


@pytest.mark.parametrize("c", W.CASES, ids=IDS)
def test_top_p_cut_is_wide_and_splits_no_tie_group(c):
    if c.top_p >= 1.0:
        return                                                     # TopP is off (HF builds no warper, the device tests top_p < 1)
    p = torch.sort(W.topk_probs(c.row, c.T, c.top_k, c.min_keep)).values
    cum, cut = p.cumsum(-1), 1.0 - c.top_p
    remove = cum <= cut
    same = p[1:] == p[:-1]
    assert not bool((same & (remove[1:] != remove[:-1])).any()), "a tie group straddles the cut"
    ends = torch.cat([~same, torch.tensor([True])])                # the last id of every tie group: its cum is the group's at-or-below mass
    gap = float((cum[ends] - cut).abs().min())
    assert gap >= MARGIN, gap


@pytest.mark.parametrize("c", [c for c in W.CASES if c.min_p > 0.0], ids=[c.name for c in W.CASES if c.min_p > 0.0])
def test_min_p_threshold_is_wide(c):
    before = W.kept_ref(c.row, c.T, c.top_k, c.top_p, c.min_keep, 0.0)
    s = (c.row.double() / c.T)[before]
    ratio = (s - s.max()).exp()
    assert float(((ratio - c.min_p).abs() / c.min_p).min()) >= MARGIN


@pytest.mark.parametrize("c", W.CASES, ids=IDS)
def test_both_temperature_roundings_rank_alike(c):
    T = torch.tensor(c.T, dtype=torch.float32)
    for x in _inputs(c):
        a = torch.unique(x / T, return_inverse=True)[1]
        b = torch.unique(x * (1.0 / T), return_inverse=True)[1]
        assert torch.equal(a, b) and torch.equal(a, torch.unique(x, return_inverse=True)[1])


@pytest.mark.parametrize("c", W.CASES, ids=IDS)
def test_a_neighbouring_parameter_moves_exactly_one_id(c):
    assert c.control and set(c.control) <= {"top_k", "top_p", "min_p", "min_keep"}
    assert int((W.kept_of(c) ^ W.kept_of(c, **c.control)).sum()) == 1


@pytest.mark.parametrize("c", W.CASES, ids=IDS)
def test_row_is_on_the_grid_and_reaches_the_form_it_names(c):
    fin = c.row[torch.isfinite(c.row)]
    assert c.row.dtype == torch.float32 and c.row.numel() in W.VOCABS
    assert float(fin.abs().max()) <= 64.0 and torch.equal(fin * 64, (fin * 64).round()) and not bool(torch.isnan(c.row).any())
    assert int(W.kept_of(c).sum()) >= c.min_keep
    assert W.routes(c)["sampler" if c.min_keep == 1 else "beam"] == W.ROUTE_OF_FORM.get(c.form, c.form)


def test_draw_cases_keep_only_likely_ids_and_reach_every_sampler_route():
    draw = [c for c in W.CASES if W.draw_eligible(c)]
    for c in draw:
        keep = W.kept_of(c)
        p = (c.row.double() / c.T).masked_fill(~keep, W.NEG).softmax(-1)[keep]
        assert c.min_keep == 1 and float(p.min()) >= 1.0 / 16.0 and (15.0 / 16.0) ** 1024 < 1e-27
    got = {W.routes(c)["sampler"] for c in draw}
    assert got >= {"fast", "fast>TK_PER>regs<52>", "fast>TK_CAP>regs<52>", "regs<16>", "regs<52>", "global"}, got
    assert any(c.top_k == 0 and W.routes(c)["sampler"] == "regs<52>" for c in draw) and any(c.top_k == 257 for c in draw)
    assert any(c.min_p > 0.0 and W.routes(c)["sampler"] == r for c in draw for r in ("fast",)) and any(c.min_p > 0.0 and c.top_k == 0 for c in draw)


def test_the_list_reaches_every_form_of_every_caller_and_every_edge():
    cap = {W.routes(c)["capture"] for c in W.CASES if c.min_keep == 1}
    beam = {W.routes(c)["beam"] for c in W.CASES if c.min_keep == 2}
    every = {"select<49>", "select<49>>WS_CAP>regs<49,ONCE>", "regs<49,ONCE>", "global"}
    assert cap >= every and beam >= every, (cap, beam)
    V = 49157
    assert {c.top_k for c in W.CASES if c.row.numel() == V} >= {1, 2, 50, 256, 257, V - 1, V, V + 1, 0}
    assert {c.T for c in W.CASES} == {1.0, 0.7, 1.3} and {c.min_keep for c in W.CASES} == {1, 2}
    assert {c.row.numel() for c in W.CASES} == set(W.VOCABS)
    heads = W.head_cols(V)
    assert {0, 63, 64, 1023, 1024, V - 1, 48 * 1024} <= set(heads) and any(h + 1 in W.banned_cols(V) or h - 1 in W.banned_cols(V) for h in heads)
    # a cut between every adjacent pair of heads: the kept sizes 1..8 all occur with one row and one top_k
    assert {int(W.kept_of(c).sum()) for c in W.CASES if c.name.startswith("h8-T1.0-k50-cut") and c.min_keep == 1} == set(range(1, 9))
    # more than 90 apart in score / T; a tie group at the k-th value keeps k + 2
    far = [c for c in W.CASES if c.name.startswith("far")]
    assert far and all(float(c.row.max() - c.row[-1]) / c.T > 90.0 for c in far)
    assert all(int(W.kept_of(c).sum()) == c.top_k + 2 for c in W.CASES if c.name.startswith("tie"))


def test_the_operator_entry_points_refuse_bad_arguments_before_any_device_work():
    """sv_op_capture_rows / sv_debug_beam_set_capture: SV_EINVAL with a message, on a machine without a GPU (pointers never dereferenced)"""
    import ctypes as C

    import __graft_entry__ as ge
    ge.build()
    from starvector_amd import _lib
    lib, P = _lib.load(), C.c_void_p(64)

    def cap(rows=P, B=2, V=100, ld=100, seen=None, words=0, pen=1.0, eos=-1, hold=0, do_sample=1, T=1.0, top_k=0, top_p=0.9, min_p=0.0, scores=P,
            logits=P, ld_out=100):
        rc = lib.sv_op_capture_rows(rows, B, V, ld, seen, words, pen, eos, hold, do_sample, T, top_k, top_p, min_p, scores, logits, ld_out, None)
        return rc, lib.sv_last_error().decode()

    for kw, text in ((dict(rows=None), "null dev_rows"), (dict(scores=None, logits=None), "neither output"), (dict(B=0), "bad shape"),
                     (dict(V=0), "bad shape"), (dict(ld=99), "bad shape"), (dict(ld_out=99), "bad shape"), (dict(seen=P, words=3), "seen_words"),
                     (dict(seen=P, words=4, pen=0.0), "penalty"), (dict(hold=1, eos=100), "outside the vocabulary"), (dict(T=0.0), "temperature"),
                     (dict(T=float("nan")), "temperature"), (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(min_p=-0.1), "min_p"),
                     (dict(min_p=float("nan")), "min_p")):
        rc, msg = cap(**kw)
        assert rc == -22 and msg.startswith("sv_op_capture_rows:") and text in msg, (kw, rc, msg)
    assert lib.sv_debug_beam_set_capture(None, P, P, 100, 1) == -22 and "null scorer" in lib.sv_last_error().decode()
