"""GPU: the two kernels of csrc/lookup_sampled/lookup_sampled.hip on their own.
  * lookup_sample_kernel: row s * K1 + j of a verification step must draw the token sample_top_p_kernel (sv_op_sample) draws for that row
    placed at row index s with step = n_emit[s] + j -- the plain call's (seed, step, row) triple at that column.  Equality, not a histogram.
  * lookup_seen_kernel: the per-sequence and per-row bitmaps against a Python set model (starvector_amd/lookup.py SeenSets)."""
import random

import pytest
import torch

from starvector_amd import engine as E
from starvector_amd import lookup as LK
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu
SENTINEL = 0x7fffffff


def _rows(rows, V, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, V, generator=g) * scale).to(dev())


def _plain_tokens(x, K1, n_emit, **kw):
    """every row's token by the plain sampler: for each distinct step one sv_op_sample launch over [n_seq, V], row s = the row of sequence s
    whose column is that step (row index = sequence index, as in the plain call)"""
    n_seq = len(n_emit)
    out = [None] * (n_seq * K1)
    for step in sorted({n_emit[s] + j for s in range(n_seq) for j in range(K1)}):
        batch = torch.zeros(n_seq, x.shape[1], device=x.device)
        live = [s for s in range(n_seq) if 0 <= step - n_emit[s] < K1]
        for s in live:
            batch[s] = x[s * K1 + step - n_emit[s]]
        got = E.op_sample_top_p(batch, step=step, **kw).cpu().tolist()
        for s in live:
            out[s * K1 + step - n_emit[s]] = got[s]
    return out


@pytest.mark.parametrize("n_seq,K1", [(1, 2), (1, 8), (1, 16), (3, 2), (3, 8), (3, 16)])
def test_every_row_draws_what_the_plain_sampler_draws_at_its_column(n_seq, K1):
    n_emit = [1, 9, 4][:n_seq]                           # mixed: the sequences stand at different columns
    for V in (517, 2053):                                # odd; more than one score per thread of the 1024-thread block
        x = _rows(n_seq * K1, V, 100 * n_seq + K1 + V)
        for top_k in (50, 0):                            # sample_row_topk / the scan fallback
            for top_p in (0.9, 1.0):
                for T in (0.7, 1.0):
                    kw = dict(temperature=T, top_p=top_p, seed=12345, top_k=top_k)
                    got, pval, pidx = E.op_lookup_sample(x, K1, n_emit, return_slices=True, **kw)
                    ref = _plain_tokens(x, K1, n_emit, **kw)
                    assert got == ref, (V, top_k, top_p, T)
                    # the hand-over format: slice 0 = (0, token), the others hold nothing
                    assert all(pval[r] == [0.0] + [float("-inf")] * 7 and pidx[r] == [got[r]] + [SENTINEL] * 7 for r in range(n_seq * K1))
        a = E.op_lookup_sample(x, K1, n_emit, top_k=50, top_p=0.9, seed=12345)
        assert a == E.op_lookup_sample(x, K1, n_emit, top_k=50, top_p=0.9, seed=12345)
        if n_seq * K1 >= 24:                             # the triple matters: over 24+ rows another seed, or other columns, move some draw
            assert a != E.op_lookup_sample(x, K1, n_emit, top_k=50, top_p=0.9, seed=12346)
            assert a != E.op_lookup_sample(x, K1, [n + 1 for n in n_emit], top_k=50, top_p=0.9, seed=12345)


def test_the_penalty_reads_the_bitmap_of_its_own_row():
    """per-row seen sets: the draw over (row, seen set, penalty) equals the draw over the row penalised by hand -- score < 0 ? score * p :
    score / p, one IEEE fp32 operation each, the kernels' own expression -- with no seen set"""
    n_seq, K1, V, pen = 3, 4, 517, 1.3
    n_emit = [2, 5, 3]
    x = _rows(n_seq * K1, V, 77)
    r = random.Random(5)
    seen = [sorted(r.sample(range(V), 40)) + [31, 32, 511, 512, 516] for _ in range(n_seq * K1)]      # word edges, the last id of the last word
    by_hand = x.clone()
    for row, ids in enumerate(seen):
        idx = torch.tensor(sorted(set(ids)), device=x.device)
        v = x[row, idx]
        by_hand[row, idx] = torch.where(v < 0, v * torch.tensor(pen, device=x.device), v / torch.tensor(pen, device=x.device))
    for top_k in (50, 0):
        kw = dict(temperature=0.7, top_p=0.9, seed=99, top_k=top_k)
        got = E.op_lookup_sample(x, K1, n_emit, seen=seen, penalty=pen, **kw)
        assert got == E.op_lookup_sample(by_hand, K1, n_emit, **kw) == _plain_tokens(by_hand, K1, n_emit, **kw)


def test_a_row_without_a_finite_score_hands_over_the_sentinel_and_the_step_raises_bad():
    K1, V = 4, 517
    x = _rows(K1, V, 3)
    x[2] = float("-inf")
    for top_k in (50, 0):
        got, pval, pidx = E.op_lookup_sample(x, K1, [1], top_k=top_k, top_p=0.9, seed=1, return_slices=True)
        assert got[2] == SENTINEL and pval[2] == [float("-inf")] * 8 and pidx[2] == [SENTINEL] * 8
        assert all(0 <= t < V for i, t in enumerate(got) if i != 2)
        # through lookup_step_kernel: three forced drafts, the first two right -- the third row's choice is emitted: id 0, and the flag goes up
        stream = [5, got[0], got[1], 7] + [0] * 8
        st = LK.LookupState(n_seq=1, K=K1 - 1, max_new=12, vocab=V, forced=[stream])
        st.begin(stream[:1], [0])
        assert st.n_emit[0] == 1 and st.n_draft[0] == 3 and st.bad == 0
        E.op_lookup_accept(st, [got])
        assert st.bad == 1 and st.n_emit[0] == 4 and st.hist[0][:4] == [5, got[0], got[1], 0]


def _walk(n_seq, K, max_new, streams, forced, vocab):
    """a forced-draft call over given streams, the set model and the kernel side by side after every step"""
    K1 = K + 1
    st = LK.LookupState(n_seq=n_seq, K=K, max_new=max_new, eos=1, pad=0, forced=forced, vocab=vocab)
    st.begin([row[0] for row in streams], [0] * n_seq)
    sets = LK.SeenSets(n_seq, K)
    sets.begin([[row[0]] for row in streams], st)
    dev_seq = [set(x) for x in sets.seq]
    what = dict(full=False, none=False, dead=False, finished=False)
    while not st.done:
        before = list(st.n_emit)
        st.step([[streams[s][st.n_emit[s] + j] if st.n_emit[s] + j < max_new else 0 for j in range(K1)] for s in range(n_seq)])
        sets.step(st)
        dev_seq, dev_rows = E.op_lookup_seen(st.hist, before, st.n_emit, st.n_draft, st.rows, vocab, seq_seen=dev_seq)
        assert dev_seq == sets.seq, (before, st.n_emit)
        assert dev_rows == [sets.rows[s][j] for s in range(n_seq) for j in range(K1)], (before, st.n_emit, st.n_draft)
        for s in range(n_seq):
            what["full"] |= st.n_emit[s] - before[s] == K1
            what["none"] |= st.n_draft[s] == 0
            what["dead"] |= 0 < st.n_draft[s] < K
            what["finished"] |= st.finished[s] and st.n_emit[s] == before[s]
    return st, what


def test_seen_sets_against_the_set_model():
    V = 517                                              # not a multiple of 32: the last word holds 5 ids
    r = random.Random(3)
    edge = [31, 32, 63, 511, 512, 516]                   # the last bit of a word, the first of the next, the last word, its last id
    streams = [[r.choice(edge + list(range(2, 40))) for _ in range(40)] for _ in range(3)]
    streams[1][9] = 1                                    # an EOS: sequence 1 finishes early and stays frozen
    for row in streams:
        row[3], row[4], row[20] = 516, 31, 512
    seen = dict(full=False, none=False, dead=False, finished=False)
    for K, forced in ((3, streams), (7, streams), (15, streams),
                      (3, [[t if i % 4 else (t + 1) % V for i, t in enumerate(row)] for row in streams]),       # partly wrong: 0 .. 3 accepted
                      (7, [[(t + 1) % V for t in row] for row in streams])):                                     # all wrong
        st, what = _walk(3, K, 38, streams, forced, V)
        assert st.tokens()[0] == streams[0][:38]
        seen = {k: seen[k] or what[k] for k in seen}
    assert all(seen.values()), seen                      # a step that emitted K + 1 ids, n_draft = 0, dead rows, a finished sequence
    # one step on its own: nothing emitted, no draft -- every row is the sequence's set
    seq, rows = E.op_lookup_seen([[516, 5, 0, 0]], [2], [2], [0], [[5, 9, 9, 9]], V, seq_seen=[{516, 5}])
    assert seq == [{516, 5}] and rows == [{516, 5}] * 4
    # K + 1 ids at once with all drafts live: row j adds exactly rows 1 .. j
    seq, rows = E.op_lookup_seen([[3, 31, 32, 511, 516, 0]], [1], [5], [3], [[516, 63, 64, 512]], V, seq_seen=[{3}])
    base = {3, 31, 32, 511, 516}
    assert seq == [base] and rows == [base, base | {63}, base | {63, 64}, base | {63, 64, 512}]
