"""Designed rows for the TopK -> TopP -> min_p warper (csrc/warp.h, csrc/sample_row.h) and their float64 reference.  Imports torch only.

A row is a low background with a handful of "head" ids; every score lies on a 1/64 grid with |x| <= 64, so x / T and x * (1 / T) rank alike
and two different scores are at least a factor exp(1 / (64 T)) apart in probability -- far outside the 2^-18 slack of wp_keep.  The kept SET
of such a row is decided by wide margins (tests/test_warper_rows_host.py asserts them per case), so every device form must return it exactly.

  background   -30 - (i % 7) / 64: seven tie groups far below any cut
  ladder       ~300 ids at -14 - j / 64, one per thread of the 1024-thread block: the distinct values a top_k inside the background needs (and
               what lets T0, the k-th largest thread maximum, land above the background: without it ~V / 7 ids tie at T0 and the selections
               fall back -- the `noladder` rows do that on purpose)
  heads        log(w) for weights 8 : 7 : ... : 1 at the columns where the kernels' indexing can go wrong: 0, 63 / 64, 1023 / 1024, V - 1, the
               first column of the row's last partial stride, and next to a banned (-inf) entry
  banned       three -inf entries (columns 1, 2000, V - 2), next to heads
  minimum      one id at -50: the only one top_k = V - 1 drops

CASES is the list the host test qualifies and the GPU tests (tests/test_gpu_warper_kept_set.py) run."""
import math
from collections import namedtuple

import torch

WP_THREADS, WS_CAP, TK_CAP, TK_PER = 1024, 1024, 2048, 4          # csrc/warp.h, csrc/sample_row.h
NEG = float("-inf")
VOCABS = (517, 16384, 49156, 49157, 50177, 53249)

# row: fp32 [V]; control: the parameters of a neighbouring call whose kept set differs by exactly one id; form: the route the case is meant to reach
Case = namedtuple("Case", "name row T top_k top_p min_p min_keep form control")


def f32(x: float) -> float:
    """x as the device receives it (a C float)"""
    return float(torch.tensor(x, dtype=torch.float32))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def kept_ref(row, T, top_k, top_p, min_keep, min_p=0.0):
    """The kept mask (bool [V]) of HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper, restated in
    float64; an id is kept when its final score is finite."""
    s = row.double() / float(T)
    V = s.numel()
    if top_k and top_k > 0:
        k = min(max(int(top_k), min_keep), V)
        kth = torch.topk(s, k).values[-1]
        s = s.masked_fill(s < kth, NEG)
    if top_p < 1.0:
        srt, idx = torch.sort(s, descending=False, stable=True)
        remove = srt.softmax(-1).cumsum(-1) <= (1.0 - top_p)
        remove[-min_keep:] = False
        s = s.masked_fill(torch.zeros(V, dtype=torch.bool).scatter(0, idx, remove), NEG)
    if min_p and min_p > 0.0:
        p = s.softmax(-1)
        remove = p < min_p * p.max()
        idx = torch.argsort(s, descending=True, stable=True)
        rs = remove[idx]
        rs[:min_keep] = False
        s = s.masked_fill(torch.zeros(V, dtype=torch.bool).scatter(0, idx, rs), NEG)
    return torch.isfinite(s)


def kept_of(case, **override):
    """kept_ref of a case (memoised), or of the case with some parameters replaced (the control)"""
    if not override:
        if case.name not in _KEPT:
            _KEPT[case.name] = kept_ref(case.row, case.T, case.top_k, case.top_p, case.min_keep, case.min_p)
        return _KEPT[case.name]
    c = case._replace(**override)
    return kept_ref(c.row, c.T, c.top_k, c.top_p, c.min_keep, c.min_p)


_KEPT = {}


def topk_probs(row, T, top_k, min_keep):
    """float64 probabilities over the top-k survivors (0 elsewhere): what TopP sees"""
    s = row.double() / float(T)
    if top_k and top_k > 0:
        k = min(max(int(top_k), min_keep), s.numel())
        s = s.masked_fill(s < torch.topk(s, k).values[-1], NEG)
    return s.softmax(-1)


def head_cut(row, T, top_k, min_keep, n):
    """the top_p (4 decimals) whose cut 1 - top_p lies midway between the at-or-below masses of the n-th and the (n+1)-th most probable id"""
    cum = torch.sort(topk_probs(row, T, top_k, min_keep)).values.cumsum(-1)
    V = cum.numel()
    return round(1.0 - 0.5 * float(cum[V - n - 1] + cum[V - n]), 4)


# ---- which route a case takes: the dispatch of sample_row / row_warp_stats, restated ------------------------------------------------------------
def _thread_stats(s, k):
    """(ids >= T0, the most of them in one thread's stride), T0 = the k-th largest of the 1024 thread maxima (thread t owns i = t mod 1024)"""
    V = s.numel()
    m = torch.cat([s, torch.full(((-V) % WP_THREADS,), NEG)]).view(-1, WP_THREADS)
    t0 = torch.topk(m.max(0).values, k).values[-1]
    cand = m >= t0
    return int(cand.sum()), int(cand.sum(0).max())


ROUTE_OF_FORM = {"TK_PER": "fast>TK_PER>regs<52>", "TK_CAP": "fast>TK_CAP>regs<52>", "WS_CAP": "select<49>>WS_CAP>regs<49,ONCE>"}


def routes(case):
    """{"sampler": ..., "capture": ..., "beam": ...}: the form each caller's dispatch reaches for this row and these parameters ("beam" with
    SV_BEAM_WARP_SELECT=1; =0 is the same without the selection)"""
    V, top_k = case.row.numel(), case.top_k
    s = (case.row * (1.0 / f32(case.T)))
    general = "regs<16>" if V <= 16 * WP_THREADS else "regs<52>" if V <= 52 * WP_THREADS else "global"
    sampler = general
    if 0 < top_k <= 256 and top_k < V:
        n, per = _thread_stats(s, top_k)
        sampler = f"fast>TK_PER>{general}" if per > TK_PER else f"fast>TK_CAP>{general}" if n > TK_CAP else "fast"

    def nonsampler(min_keep):
        if V > 49 * WP_THREADS:
            return "global"
        k = max(top_k, min_keep)
        if top_k > 0 and k <= 256 and k < V:
            n, _ = _thread_stats(s, k)
            return "select<49>" if n <= WS_CAP else "select<49>>WS_CAP>regs<49,ONCE>"
        return "regs<49,ONCE>"
    return {"sampler": sampler, "capture": nonsampler(1), "beam": nonsampler(2)}


# ---- the rows --------------------------------------------------------------------------------------------------------------------------------
def grid(x: float) -> float:
    return round(x * 64.0) / 64.0


def banned_cols(V):
    return [1, 2000 % V, V - 2]


def head_cols(V):
    cols = []
    for c in (0, 63, 64, 1023, 1024, V - 1, ((V - 1) // WP_THREADS) * WP_THREADS, 2001):
        c %= V
        while c in cols or c in banned_cols(V):
            c = (c + 97) % V
        cols.append(c)
    return cols


def stride_cols(V):
    """five heads in ONE thread's stride (i = 5 mod 1024), three elsewhere"""
    return [5, 5 + 1024, 5 + 2048, 5 + 3072, 5 + 4096, 63, V - 1, 1024]


def make_row(V, weights=(8, 7, 6, 5, 4, 3, 2, 1), cols=None, ladder=True, banned=True, bg=-30.0):
    i = torch.arange(V)
    row = bg - (i % 7).to(torch.float32) / 64.0
    cols = head_cols(V) if cols is None else cols
    taken = set(cols) | (set(banned_cols(V)) if banned else set())
    low = 4242 % V
    while low in taken:
        low += 1
    row[low] = -50.0
    taken.add(low)
    if ladder:
        full = max(V // WP_THREADS, 1)
        for j in range(min(300, V // 2)):
            c = (7 + 163 * j) % min(V, WP_THREADS) + WP_THREADS * (j % full) * (V >= WP_THREADS)
            if c not in taken:
                row[c] = -14.0 - j / 64.0
                taken.add(c)
    for c, w in zip(cols, weights):
        row[c] = grid(math.log(w))
    if banned:
        row[banned_cols(V)] = NEG
    assert float(row[torch.isfinite(row)].abs().max()) <= 64.0 and bool((row[torch.isfinite(row)] * 64 == (row[torch.isfinite(row)] * 64).round()).all())
    return row


def far_row(V, hi, lo):
    """two heads more than 90 apart in score / T: __expf(lo - hi) underflows"""
    row = -60.0 - (torch.arange(V) % 7).to(torch.float32) / 64.0
    row[0], row[V - 1], row[100] = hi, lo, -58.0                 # a third distinct value: what top_k = 3 adds
    return row


def equal_row(V):
    """one value everywhere but the last column: more than WS_CAP / TK_CAP ids tie at every threshold"""
    row = torch.zeros(V)
    row[V - 1] = -1.0 / 64.0
    return row


def _build():
    cases = []

    def add(name, row, T, top_k, top_p, min_p, min_keep, form, control):
        cases.append(Case(name, row, T, top_k, top_p, min_p, min_keep, form, control))

    def cut_cases(tag, row, T, top_k, min_keep, ns, form):
        for n in ns:                                             # n = how many heads the cut leaves
            tp = head_cut(row, T, top_k, min_keep, n)
            other = n + 1 if n < 8 else n - 1
            add(f"{tag}-T{T}-k{top_k}-cut{n}-mk{min_keep}", row, T, top_k, tp, 0.0, min_keep, form, dict(top_p=head_cut(row, T, top_k, min_keep, other)))

    V = 49157
    h8 = make_row(V)
    # top_p between every adjacent pair of heads, then so small that only min_keep ids survive; T in {1, 0.7, 1.3}
    for mk, sel, gen in ((1, "fast", "regs<52>"), (2, "select<49>", "regs<49,ONCE>")):
        cut_cases("h8", h8, 1.0, 50, mk, range(max(mk, 1), 9), sel)
        cut_cases("h8", h8, 1.0, 0, mk, range(max(mk, 1), 9), gen)
        for T in (0.7, 1.3):
            cut_cases("h8", h8, T, 50, mk, (3, 5, 6), sel)
            cut_cases("h8", h8, T, 0, mk, (3, 5, 6), gen)
        for top_k, form in ((50, sel), (0, gen)):
            add(f"h8-T1.0-k{top_k}-p0.01-mk{mk}", h8, 1.0, top_k, 0.01, 0.0, mk, form, dict(top_p=head_cut(h8, 1.0, top_k, mk, mk + 1)))
    # top_k in {1, 2, 50, 256, 257, V - 1, V, V + 1, 0} alone: the k-th value lies among the heads, in the ladder, at the unique minimum
    nob = make_row(V, banned=False)                              # (a banned entry would sit below the minimum: top_k = V - 1 drops nothing then)
    for mk in (1, 2):
        for top_k in (1, 2, 50, 256, 257, V - 1, V, V + 1, 0):
            form = ("fast" if mk == 1 else "select<49>") if 0 < top_k <= 256 else ("regs<52>" if mk == 1 else "regs<49,ONCE>")
            near = top_k + 1 if 0 < top_k < V else V - 1
            if mk == 2 and top_k == 1:
                near = 3                                         # top_k 1 and 2 both keep min_tokens_to_keep = 2 ids
            add(f"nob-T1.0-k{top_k}-p1-mk{mk}", nob, 1.0, top_k, 1.0, 0.0, mk, form, dict(top_k=near))
    add("h8-T0.7-k50-p1-mk1", h8, 0.7, 50, 1.0, 0.0, 1, "fast", dict(top_k=51))
    # a tie group at the k-th value: top_k = 3 keeps k + 2 ids
    tie = make_row(V, weights=(8, 7, 5, 5, 5, 3, 2, 1))
    for mk, form in ((1, "fast"), (2, "select<49>")):
        add(f"tie-T1.0-k3-p1-mk{mk}", tie, 1.0, 3, 1.0, 0.0, mk, form, dict(top_k=6))
        add(f"tie-T1.3-k3-p1-mk{mk}", tie, 1.3, 3, 1.0, 0.0, mk, form, dict(top_k=6))
    # five heads in one thread's stride: the fast path's TK_PER fallback (the block-wide selection takes them)
    st5 = make_row(V, cols=stride_cols(V))
    for mk, form in ((1, "TK_PER"), (2, "select<49>")):
        cut_cases("stride5", st5, 1.0, 50, mk, (4, 6), form)
        add(f"stride5-T1.0-k5-p1-mk{mk}", st5, 1.0, 5, 1.0, 0.0, mk, form, dict(top_k=6))
    # a plateau of 3069 equal ids, three per thread (none in thread 0: it owns three heads), and no ladder: they tie at T0 and at the k-th value -- more than WS_CAP / TK_CAP candidates
    # with at most TK_PER in a thread, so both selections fall back on the candidate count alone; top-p then drops the tie group whole
    plat = make_row(V, ladder=False)
    plat[10 * WP_THREADS + 1:11 * WP_THREADS] = plat[11 * WP_THREADS + 1:12 * WP_THREADS] = plat[12 * WP_THREADS + 1:13 * WP_THREADS] = -20.0
    for mk, form in ((1, "TK_CAP"), (2, "WS_CAP")):
        cut_cases("plateau", plat, 1.0, 50, mk, (4, 6), form)
    # the all-equal row exceeds TK_PER and TK_CAP at once (one test in the kernel); every id but one survives
    for mk, form in ((1, "TK_PER"), (2, "WS_CAP")):
        add(f"equal-T1.0-k50-p1-mk{mk}", equal_row(V), 1.0, 50, 1.0, 0.0, mk, form, dict(top_k=0))
    # head scores more than 90 apart in score / T
    for mk, sel, gen in ((1, "fast", "regs<52>"), (2, "select<49>", "regs<49,ONCE>")):
        add(f"far-T1.0-k2-p1-mk{mk}", far_row(V, 40.0, -55.0), 1.0, 2, 1.0, 0.0, mk, sel, dict(top_k=3))
        add(f"far-T1.0-k2-p0.9-mk{mk}", far_row(V, 40.0, -55.0), 1.0, 2, 0.9, 0.0, mk, sel, dict(min_keep=3 - mk))
        add(f"far-T0.7-k2-p1-mk{mk}", far_row(V, 32.0, -32.0), 0.7, 2, 1.0, 0.0, mk, sel, dict(top_k=3))
        add(f"far-T1.0-k0-p0.9-mk{mk}", far_row(V, 40.0, -55.0), 1.0, 0, 0.9, 0.0, mk, gen, dict(min_keep=3 - mk))
    # min_p cutting between two heads (HF / vLLM order: after top-p); min_tokens_to_keep 1 only (beam-sample has no min_p)
    for T in (1.0, 0.7):
        add(f"h8-T{T}-k50-p1-minp0.3", h8, T, 50, 1.0, 0.3, 1, "fast", dict(min_p=0.2))
        add(f"h8-T{T}-k0-p1-minp0.3", h8, T, 0, 1.0, 0.3, 1, "regs<52>", dict(min_p=0.2))
    add("h8-T1.0-k50-cut7-minp0.3", h8, 1.0, 50, head_cut(h8, 1.0, 50, 1, 7), 0.3, 1, "fast", dict(min_p=0.2))
    add("h8-T1.0-k0-cut5-minp0.1", h8, 1.0, 0, head_cut(h8, 1.0, 0, 1, 5), 0.1, 1, "regs<52>", dict(top_p=head_cut(h8, 1.0, 0, 1, 4)))
    # the other vocabulary sizes: every form of every caller
    for V2, gen_s, gen_c in ((517, "regs<16>", "regs<49,ONCE>"), (16384, "regs<16>", "regs<49,ONCE>"), (49156, "regs<52>", "regs<49,ONCE>"),
                             (50177, "regs<52>", "global"), (53249, "global", "global")):
        r = make_row(V2)
        for mk in (1, 2):
            sel = "fast" if mk == 1 else ("select<49>" if V2 <= 49 * WP_THREADS else "global")
            gen = gen_s if mk == 1 else gen_c
            cut_cases(f"v{V2}", r, 1.0, 50, mk, (4, 6), sel)
            cut_cases(f"v{V2}", r, 1.0, 0, mk, (4, 6), gen)
            cut_cases(f"v{V2}", r, 0.7, 0, mk, (5,), gen)
            add(f"v{V2}-T1.0-k50-p1-mk{mk}", r, 1.0, 50, 1.0, 0.0, mk, sel, dict(top_k=51))
            add(f"v{V2}-T1.0-k257-cut4-mk{mk}", r, 1.0, 257, head_cut(r, 1.0, 257, mk, 4), 0.0, mk, gen, dict(top_p=head_cut(r, 1.0, 257, mk, 3)))
        add(f"v{V2}-T1.0-k0-p1-minp0.3", r, 1.0, 0, 1.0, 0.3, 1, gen_s, dict(min_p=0.2))
    names = [c.name for c in cases]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    return cases


CASES = _build()


def draw_eligible(case):
    """condition 7: every kept id has renormalised probability >= 1 / 16 (1024 draws miss one with probability (15 / 16)^1024 < 1e-28)"""
    if case.min_keep != 1:
        return False
    keep = kept_of(case)
    p = (case.row.double() / float(case.T)).masked_fill(~keep, NEG).softmax(-1)
    return int(keep.sum()) <= 16 and float(p[keep].min()) >= 1.0 / 16.0
