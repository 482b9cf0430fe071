"""Prompt-lookup speculative decoding, restated in plain Python: what csrc/lookup/lookup.hip does on the device per verification step --
draft, accept, emit -- with no engine and no GPU.  The CPU tests hold this restatement to its invariant (whatever the drafts are, the emitted
stream is the plain greedy stream); the GPU tests hold the kernels to this restatement.

The second half restates csrc/lookup_sampled/lookup_sampled.hip (sv_generate_lookup_sampled): a CHOOSER that is a function of (sequence,
column, prefix) stands for the sampler -- its random number is a function of (seed, step = column, row = sequence), its scores a function of
the prefix -- and SeenSets stands for the repetition penalty's bitmaps as lookup_seen_kernel keeps them.

The last part restates csrc/cb_lookup/cb_lookup.hip (sv_cb_set_lookup): CbLookupState is the drafting continuous batch -- slots with their own
budget, EOS, stop sequence and stop_any ids, K + 1 decode rows each, admit / step(chooser) / release -- verified row after row against the
slot's current state.

State of a call over n_seq sequences, as the device keeps it:
    hist[s]      the ids sequence s has generated, at its own column (a list that grows; pads behind an early end)
    n_emit[s]    ids emitted, finished[s], base[s] = prompt length, n_draft[s] = live drafts of the step in flight
    limit        the column count row 0's stop sequence allows (max_new until it fires)
    done, n_emitted, bad, steps, drafted, accepted
A verification step has K + 1 rows per sequence: rows[s][0] = the last emitted id, rows[s][1 .. n_draft] the drafts, the rest copies of row 0.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence


def draft(hist: Sequence[int], K: int, max_ngram: int = 3, min_ngram: int = 1, max_new: Optional[int] = None) -> List[int]:
    """The drafts behind the ids `hist`: for n = max_ngram .. min_ngram the LATEST earlier occurrence of the last n ids that has a
    continuation (largest i with hist[i:i+n] == hist[L-n:L] and i + n < L) gives hist[i+n : i+n+K], cut at L.  At most
    max_new - L - 1 drafts: a step emits its accepted drafts and one id more."""
    L = len(hist)
    if max_new is not None:
        K = min(K, max_new - L - 1)
    if K <= 0:
        return []
    for n in range(max_ngram, min_ngram - 1, -1):
        if L <= n:
            continue
        tail = list(hist[L - n:])
        for i in range(L - n - 1, -1, -1):
            if list(hist[i:i + n]) == tail:
                return list(hist[i + n:min(i + n + K, L)])
    return []


@dataclass
class LookupState:
    n_seq: int
    K: int
    max_new: int
    eos: int = -1
    pad: int = 0
    stop: Sequence[int] = ()
    max_ngram: int = 3
    min_ngram: int = 1
    vocab: int = 1 << 30
    base: List[int] = field(default_factory=list)
    hist: List[List[int]] = field(default_factory=list)
    n_emit: List[int] = field(default_factory=list)
    finished: List[bool] = field(default_factory=list)
    n_draft: List[int] = field(default_factory=list)
    rows: List[List[int]] = field(default_factory=list)
    positions: List[List[int]] = field(default_factory=list)
    limit: int = 0
    done: bool = False
    n_emitted: int = 0
    bad: int = 0
    steps: int = 0
    drafted: int = 0
    accepted: int = 0
    forced: Optional[Sequence[Sequence[int]]] = None        # draft j of sequence s is forced[s][n_emit_s + j] instead of the lookup

    def _stop_at(self, L: int) -> bool:
        n = len(self.stop)
        return n > 0 and L >= n and list(self.hist[0][L - n:L]) == list(self.stop)

    def _draft(self, s: int) -> List[int]:
        L = self.n_emit[s]
        if self.forced is not None:
            K = min(self.K, self.max_new - L - 1)
            return [int(t) for t in self.forced[s][L:L + max(K, 0)]]
        return draft(self.hist[s][:L], self.K, self.max_ngram, self.min_ngram, self.max_new)

    def _finish_pad(self, s: int, stopped: bool) -> None:
        L = self.n_emit[s]
        self.hist[s][L:] = [self.pad] * (self.max_new - L)
        if s == 0 and self.stop and not stopped:
            for c in range(L + 1, self.max_new + 1):
                if self._stop_at(c):
                    self.limit = min(self.limit, c)
                    break

    def _write_rows(self, s: int, drafts: List[int]) -> None:
        L = self.n_emit[s]
        last, pos0 = self.hist[s][L - 1], self.base[s] + L - 1
        nd = len(drafts)
        self.rows[s] = [last] + [drafts[j - 1] if j <= nd else last for j in range(1, self.K + 1)]
        self.positions[s] = [pos0] + [pos0 + j if j <= nd else pos0 for j in range(1, self.K + 1)]
        self.n_draft[s] = nd

    def begin(self, first_tokens: Sequence[int], prompt_lens: Sequence[int], unfinished: Optional[Sequence[bool]] = None) -> None:
        """After the prompt pass and the first token (taken by the plain call's own bookkeeping)."""
        self.base = [int(x) for x in prompt_lens]
        self.hist = [[int(first_tokens[s])] + [0] * (self.max_new - 1) for s in range(self.n_seq)]
        self.n_emit = [1] * self.n_seq
        unf = [True] * self.n_seq if unfinished is None else list(unfinished)
        self.finished = [not unf[s] or self.max_new <= 1 for s in range(self.n_seq)]
        self.n_draft = [0] * self.n_seq
        self.rows = [[] for _ in range(self.n_seq)]
        self.positions = [[] for _ in range(self.n_seq)]
        self.limit, self.steps, self.drafted, self.accepted = self.max_new, 0, 0, 0
        for s in range(self.n_seq):
            if self.finished[s]:
                self._finish_pad(s, False)
            self._write_rows(s, [] if self.finished[s] else self._draft(s))

    def hold_eos(self, s: int, j: int, min_new: int) -> bool:
        """The min-length hold: row j of sequence s chooses column n_emit + j, where EOS is barred while that is below min_new."""
        return self.n_emit[s] + j < min_new

    def step(self, winners: Sequence[Sequence[int]]) -> None:
        """winners[s][j] = the id row j of sequence s chose."""
        if self.done:
            return
        # (row 0 counts as finished once its stop has fired; the others run on until they finish or the call ends, whatever the limit says meanwhile)
        active = [not self.finished[s] for s in range(self.n_seq)]
        for s in range(self.n_seq):
            if not active[s]:
                continue
            t = []
            for j in range(self.K + 1):
                w = int(winners[s][j])
                if not 0 <= w < self.vocab:
                    w, self.bad = 0, self.bad or 1
                t.append(w)
            nd, a = self.n_draft[s], 0
            while a < nd and self.rows[s][a + 1] == t[a]:
                a += 1
            L0 = L = self.n_emit[s]
            f = stopped = False
            for i in range(a + 1):
                self.hist[s][L] = t[i]
                L += 1
                if t[i] == self.eos or L >= self.max_new:
                    f = True
                self.n_emit[s] = L
                if s == 0 and self._stop_at(L):
                    self.limit, stopped, f = min(self.limit, L), True, True
                if f or stopped:
                    break
            self.n_emit[s], self.finished[s] = L, f
            self.drafted += nd
            self.accepted += L - L0 - 1
            if f:
                self._finish_pad(s, stopped)
            self._write_rows(s, [] if f else self._draft(s))
        self.steps += 1
        if all(self.finished[s] or self.n_emit[s] >= self.limit for s in range(self.n_seq)):
            self.n_emitted = min(self.limit, max(self.n_emit))
            self.done = True

    def tokens(self) -> List[List[int]]:
        return [list(self.hist[s][:self.n_emitted]) for s in range(self.n_seq)]


Model = Callable[[int, List[int], bool], int]      # (sequence, ids generated so far, EOS barred) -> the next id


def plain_greedy(model: Model, n_seq: int, max_new: int, eos: int = -1, pad: int = 0, stop: Sequence[int] = (), min_new: int = 0):
    """The plain call's bookkeeping (finish_step): one id per sequence and step, pads behind EOS, row 0's stop ends every row."""
    hist = [[] for _ in range(n_seq)]
    unf = [True] * n_seq
    for t in range(max_new):
        for s in range(n_seq):
            tok = model(s, list(hist[s]), t < min_new) if unf[s] else pad
            hist[s].append(tok)
            unf[s] = unf[s] and tok != eos
        fired = len(stop) > 0 and t + 1 >= len(stop) and hist[0][t + 1 - len(stop):] == list(stop)
        if fired or not any(unf) or t + 1 >= max_new:
            break
    return hist


def lookup_greedy(model: Model, n_seq: int, K: int, max_new: int, eos: int = -1, pad: int = 0, stop: Sequence[int] = (), min_new: int = 0,
                  max_ngram: int = 3, min_ngram: int = 1, forced=None, prompt_lens: Optional[Sequence[int]] = None):
    """The lookup call over the same model: returns (tokens, state).  Row j of a sequence sees the sequence's ids followed by its first j drafts."""
    first = plain_greedy(model, n_seq, 1, eos, pad, stop, min_new)
    st = LookupState(n_seq=n_seq, K=K, max_new=max_new, eos=eos, pad=pad, stop=tuple(stop), max_ngram=max_ngram, min_ngram=min_ngram, forced=forced)
    toks = [h[0] for h in first]
    fired = len(stop) == 1 and toks[0] == stop[0]
    unf = [t != eos for t in toks]
    if fired or not any(unf) or max_new <= 1:
        return [[t] for t in toks], st
    st.begin(toks, prompt_lens or [0] * n_seq, unf)
    while not st.done:
        winners = []
        for s in range(n_seq):
            ctx = st.hist[s][:st.n_emit[s]]
            row = []
            for j in range(K + 1):
                live = j <= st.n_draft[s]
                prefix = ctx + st.rows[s][1:j + 1] if live else ctx
                row.append(model(s, prefix, st.hold_eos(s, j if live else 0, min_new)))
            winners.append(row)
        st.step(winners)
    return st.tokens(), st


# ---- sv_generate_lookup_sampled: the call's own selection verifies the drafts ---------------------------------------------------------------
# (sequence, column, ids in front of the column, seen set or None, EOS barred) -> the id at that column.  Any deterministic function will do:
# the sampler is one (seed fixed), and so is the arg-max under a repetition penalty.
Chooser = Callable[[int, int, List[int], Optional[frozenset], bool], int]


class SeenSets:
    """The repetition penalty's seen sets as the device keeps them in lookup mode (lookup_seen_kernel): one set per SEQUENCE, grown by the ids
    each step emits (columns [cols[s], n_emit[s]) of the history), and from it one set per ROW of the next step: the sequence's set plus the
    drafts in front of the row, rows 1 .. j; a dead row (j > n_draft) gets row 0's set."""

    def __init__(self, n_seq: int, K: int):
        self.n_seq, self.K = n_seq, K
        self.seq = [set() for _ in range(n_seq)]
        self.cols = [0] * n_seq
        self.rows = [[set() for _ in range(K + 1)] for _ in range(n_seq)]

    def begin(self, first_sets: Sequence[Sequence[int]], st: LookupState) -> None:
        """Behind LookupState.begin: first_sets[s] = what the first token's bookkeeping left for sequence s."""
        self.seq = [set(int(t) for t in x) for x in first_sets]
        self.cols = list(st.n_emit)
        self._write_rows(st)

    def step(self, st: LookupState) -> None:
        """Behind LookupState.step."""
        for s in range(self.n_seq):
            for c in range(self.cols[s], st.n_emit[s]):
                self.seq[s].add(st.hist[s][c])
            self.cols[s] = st.n_emit[s]
        self._write_rows(st)

    def _write_rows(self, st: LookupState) -> None:
        for s in range(self.n_seq):
            cur = set(self.seq[s])
            self.rows[s][0] = set(cur)
            for j in range(1, self.K + 1):
                if j <= st.n_draft[s]:
                    cur.add(st.rows[s][j])
                    self.rows[s][j] = set(cur)
                else:
                    self.rows[s][j] = set(self.seq[s])


def plain_chosen(chooser: Chooser, n_seq: int, max_new: int, eos: int = -1, pad: int = 0, stop: Sequence[int] = (), min_new: int = 0,
                 penalty: bool = False):
    """The plain call with a chooser: plain_greedy's bookkeeping; with `penalty` every emitted id (pads included) joins its row's seen set,
    as finish_step does."""
    seen = [set() for _ in range(n_seq)]

    def model(s, prefix, barred):
        return chooser(s, len(prefix), prefix, frozenset(seen[s]) if penalty else None, barred)
    hist = [[] for _ in range(n_seq)]
    unf = [True] * n_seq
    for t in range(max_new):
        for s in range(n_seq):
            tok = model(s, list(hist[s]), t < min_new) if unf[s] else pad
            hist[s].append(tok)
            seen[s].add(tok)
            unf[s] = unf[s] and tok != eos
        fired = len(stop) > 0 and t + 1 >= len(stop) and hist[0][t + 1 - len(stop):] == list(stop)
        if fired or not any(unf) or t + 1 >= max_new:
            break
    return hist


def lookup_chosen(chooser: Chooser, n_seq: int, K: int, max_new: int, eos: int = -1, pad: int = 0, stop: Sequence[int] = (), min_new: int = 0,
                  max_ngram: int = 3, min_ngram: int = 1, forced=None, prompt_lens: Optional[Sequence[int]] = None, penalty: bool = False):
    """The lookup call with a chooser: returns (tokens, state).  Row j of sequence s chooses for column n_emit[s] + j, shown the sequence's ids
    followed by its first j drafts, against the seen set SeenSets keeps for that row.  Both are the plain call's at that column as long as
    the drafts in front of the row are right -- and only then is the row's choice emitted."""
    first = plain_chosen(chooser, n_seq, 1, eos, pad, stop, min_new, penalty)
    st = LookupState(n_seq=n_seq, K=K, max_new=max_new, eos=eos, pad=pad, stop=tuple(stop), max_ngram=max_ngram, min_ngram=min_ngram, forced=forced)
    toks = [h[0] for h in first]
    fired = len(stop) == 1 and toks[0] == stop[0]
    unf = [t != eos for t in toks]
    if fired or not any(unf) or max_new <= 1:
        return [[t] for t in toks], st
    st.begin(toks, prompt_lens or [0] * n_seq, unf)
    sets = SeenSets(n_seq, K)
    sets.begin([[t] for t in toks], st)
    while not st.done:
        winners = []
        for s in range(n_seq):
            ctx = st.hist[s][:st.n_emit[s]]
            row = []
            for j in range(K + 1):
                live = j <= st.n_draft[s]
                prefix = ctx + st.rows[s][1:j + 1] if live else ctx
                jj = j if live else 0
                row.append(chooser(s, st.n_emit[s] + jj, prefix, frozenset(sets.rows[s][j]) if penalty else None, st.hold_eos(s, jj, min_new)))
            winners.append(row)
        st.step(winners)
        sets.step(st)
    return st.tokens(), st


# ---- sv_cb_set_lookup: drafting in the continuous batch ---------------------------------------------------------------------------------------
# csrc/cb_lookup/cb_lookup.hip restated.  A slot of the batch owns K1 = K + 1 decode rows, rows s * K1 .. s * K1 + K of cur_tok / positions;
# its own budget, EOS, stop sequence and stop_any ids; and the three counters {verification steps, drafts verified, drafts accepted}.  One
# block per slot verifies the slot's rows ONE AFTER THE OTHER: row j is selected against the slot's state after rows 0 .. j - 1 have been
# committed, and is looked at only if its draft is the token row j - 1 emitted.
# (slot, column, the ids the row was computed from, hold) -> the id at that column.  `hold` = the column is below the request's min_new (the
# selection bars EOS -- and, under vLLM semantics, the stop_any ids -- while it is set).
CbChooser = Callable[[int, int, List[int], bool], int]


@dataclass
class CbRequest:
    budget: int
    eos: int = -1
    stop: Sequence[int] = ()
    stop_any: Sequence[int] = ()
    min_new: int = 0
    base: int = 0                 # prompt length: column c sits at position base + c


def cb_plain_stream(slot: int, req: CbRequest, chooser: CbChooser):
    """The one-token-per-step batch (cb_step_kernel's bookkeeping) for one request: (the ids it emits, still live -- never, once the budget is spent)."""
    hist: List[int] = []
    while True:
        t = len(hist)
        tok = chooser(slot, t, list(hist), t < req.min_new)
        hist.append(tok)
        fin = tok == req.eos or t + 1 >= req.budget or tok in req.stop_any
        n = len(req.stop)
        if not fin and n > 0 and t + 1 >= n and hist[t + 1 - n:] == list(req.stop):
            fin = True
        if fin:
            return hist, False


class CbLookupState:
    """The drafting batch as the device keeps it.  Per slot: the request, live, hist (step = len(hist)), n_draft, counts [3]; per batch: the
    row arrays cur_tok / positions [max_batch], n_live, events, bad, totals [3] (steps: one per live slot and step)."""

    def __init__(self, max_batch: int, K: int, max_ngram: int = 3, min_ngram: int = 1, vocab: int = 1 << 30, forced=None):
        if K < 1 or max_batch // (K + 1) < 1:
            raise ValueError(f"K {K} + 1 rows per slot do not fit max_batch {max_batch}")
        self.max_batch, self.K, self.K1 = max_batch, K, K + 1
        self.capacity = max_batch // (K + 1)
        self.max_ngram, self.min_ngram, self.vocab, self.forced = max_ngram, min_ngram, vocab, forced
        self.req: List[Optional[CbRequest]] = [None] * self.capacity
        self.live = [False] * self.capacity
        self.hist: List[List[int]] = [[] for _ in range(self.capacity)]
        self.n_draft = [0] * self.capacity
        self.counts = [[0, 0, 0] for _ in range(self.capacity)]
        self.cur_tok = [0] * max_batch
        self.positions = [0] * max_batch
        self.n_live = self.events = self.bad = 0
        self.totals = [0, 0, 0]

    # -- the layout --
    def bucket(self) -> int:
        """rows of the step graph: (highest used slot + 1) * K1, a power of two >= 8, capped at max_batch"""
        hi = max([s + 1 for s in range(self.capacity) if self.req[s] is not None], default=0) * self.K1
        b = 8
        while b < hi:
            b <<= 1
        return min(b, self.max_batch)

    def rows_of(self, s: int) -> List[int]:
        return self.cur_tok[s * self.K1:(s + 1) * self.K1]

    def positions_of(self, s: int) -> List[int]:
        return self.positions[s * self.K1:(s + 1) * self.K1]

    def _draft(self, s: int) -> List[int]:
        L, r = len(self.hist[s]), self.req[s]
        K = min(self.K, r.budget - L - 1)
        if self.forced is not None and s < len(self.forced):
            return [int(t) for t in self.forced[s][L:L + max(K, 0)]]
        return draft(self.hist[s], self.K, self.max_ngram, self.min_ngram, r.budget)

    def _write_rows(self, s: int, drafts: List[int]) -> None:
        L, nd = len(self.hist[s]), len(drafts)
        last, pos0 = self.hist[s][-1], self.req[s].base + L - 1
        for j in range(self.K1):
            live = 1 <= j <= nd
            self.cur_tok[s * self.K1 + j] = drafts[j - 1] if live else last
            self.positions[s * self.K1 + j] = pos0 + (j if live else 0)
        self.n_draft[s] = nd

    def _commit(self, s: int, tok: int) -> bool:
        """the plain step's bookkeeping for one token; returns fin"""
        r = self.req[s]
        if not 0 <= tok < self.vocab:
            tok, self.bad = 0, self.bad or 1
        self.hist[s].append(tok)
        t1 = len(self.hist[s])
        fin = tok == r.eos or t1 >= r.budget or tok in r.stop_any
        n = len(r.stop)
        if not fin and n > 0 and t1 >= n and self.hist[s][t1 - n:] == list(r.stop):
            fin = True
        if fin:
            self.live[s] = False
            self.n_live -= 1
            self.events += 1
        return fin

    # -- the calls --
    def admit(self, req: CbRequest, chooser: CbChooser) -> int:
        """Lowest free slot, or -1 when the batch is full (SV_EBUSY: nothing changes).  The first token comes from the prompt pass's row
        through the `first` form: no drafts to verify, the slot's K1 rows written, its counters from zero."""
        free = [s for s in range(self.capacity) if self.req[s] is None]
        if not free:
            return -1
        s = free[0]
        self.req[s], self.live[s], self.hist[s], self.counts[s] = req, True, [], [0, 0, 0]
        self.n_live += 1
        fin = self._commit(s, chooser(s, 0, [], 0 < req.min_new))
        self._write_rows(s, [] if fin else self._draft(s))
        return s

    def step(self, chooser: CbChooser) -> None:
        """One verification step over every live slot.  Row j of a slot was computed from the slot's ids followed by its first j drafts."""
        for s in range(self.capacity):
            if self.req[s] is None or not self.live[s]:
                continue                              # a dead slot is left untouched
            r, nd, L0 = self.req[s], self.n_draft[s], len(self.hist[s])
            rows = self.rows_of(s)
            j = 0
            while True:
                col = len(self.hist[s])
                tok = chooser(s, col, self.hist[s][:L0] + rows[1:j + 1], col < r.min_new)
                fin = self._commit(s, tok)
                if fin or j >= nd or rows[j + 1] != self.hist[s][-1]:
                    break
                j += 1
            acc = len(self.hist[s]) - L0 - 1
            self._write_rows(s, [] if fin else self._draft(s))
            for c, v in ((self.counts[s], (1, nd, acc)), (self.totals, (1, nd, acc))):
                for k in range(3):
                    c[k] += v[k]

    def release(self, s: int) -> None:
        if self.req[s] is None:
            raise ValueError(f"slot {s} is not in use")
        if self.live[s]:
            self.n_live -= 1
        self.req[s], self.live[s], self.hist[s], self.n_draft[s] = None, False, [], 0
        for j in range(self.K1):
            self.cur_tok[s * self.K1 + j] = self.positions[s * self.K1 + j] = 0
