"""Prompt-lookup speculative decoding, restated in plain Python: what csrc/lookup/lookup.hip does on the device per verification step --
draft, accept, emit -- with no engine and no GPU.  The CPU tests hold this restatement to its invariant (whatever the drafts are, the emitted
stream is the plain greedy stream); the GPU tests hold the kernels to this restatement.

The second half restates csrc/lookup_sampled/lookup_sampled.hip (sv_generate_lookup_sampled): a CHOOSER that is a function of (sequence,
column, prefix) stands for the sampler -- its random number is a function of (seed, step = column, row = sequence), its scores a function of
the prefix -- and SeenSets stands for the repetition penalty's bitmaps as lookup_seen_kernel keeps them.

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
