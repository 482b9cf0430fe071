"""GPU: the kernels of prompt-lookup decoding one by one (csrc/lookup/lookup.hip), each against its reference.

  * lookup_kv_write_kernel: the K / V pre-write restates the arithmetic of attn_decode_kernel's own append.  After sv_debug_kv_load of a
    context, K1 sequential decode-attention launches (each appends its row and advances) must equal ONE launch over n_seq x K1 rows behind
    the pre-write BIT FOR BIT -- and leave the same page bytes, which a further decode step from each state reads back.
  * lookup_step_kernel: the lookup and the accept / emit / stop bookkeeping against the Python restatement (starvector_amd/lookup.py).
  * lookup_hold_eos_kernel: the min-length hold per row."""
import copy
import random

import pytest
import torch

from starvector_amd import engine as E
from starvector_amd import lookup as LK
from tests.gpu_util import dev
from tests.test_gpu_long_context import _attn_engine, _kv_rows, _peaked_case

pytestmark = pytest.mark.gpu

# (query heads, KV heads, head_dim, window): StarVector-1B, head_dim 64 MQA, StarVector-8B (GQA, RoPE, window 4096)
GEOMETRIES = {"1b": (16, 1, 128, 0), "dh64": (16, 1, 64, 0), "8b": (36, 4, 128, 4096)}
_ENGINES = {}


def _engine(geom):
    if geom not in _ENGINES:
        H, nkv, dh, window = GEOMETRIES[geom]
        _ENGINES[geom] = _attn_engine(H, nkv, 24, 4224 if window else 128, window=window, dh=dh)      # 3 sequences x 8 rows
    return _ENGINES[geom]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


CASES = [(g, ctx) for g in GEOMETRIES for ctx in (30, 62)] + [("8b", 4094)]      # a 32-key group, a 64-token page, the window edge


@pytest.mark.parametrize("K1", [2, 4, 8])
@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("geom,ctx", CASES)
def test_prewrite_gives_the_bits_of_sequential_decode(geom, ctx, n_seq, K1):
    H, nkv, dh, window = GEOMETRIES[geom]
    QKV = H * dh + 2 * nkv * dh
    eng = _engine(geom)
    splitk = {2: 1, 4: 4, 8: 8}[K1]
    _, K, V = _peaked_case(n_seq, H, nkv, ctx, 3.0, 700 + ctx + K1, dh=dh)
    kv = _kv_rows(K, V, ctx)
    g = torch.Generator(device=dev()).manual_seed(1000 * K1 + ctx + n_seq)
    rows = n_seq * K1
    # slabs of very different size (the order of the float32 adds matters) and a bias; the q part scaled so that a few keys carry the mass
    slabs = torch.randn(splitk, rows, QKV, generator=g, device=dev()) * torch.logspace(-1, 0.3, splitk, device=dev())[:, None, None]
    slabs[..., :H * dh] *= 2.0
    bias = (torch.randn(QKV, generator=g, device=dev()) * 0.5).to(torch.bfloat16)
    probes = [(torch.randn(1, n_seq, QKV, generator=g, device=dev()) * s).contiguous() for s in (1.0, 3.0)]
    by_seq = slabs.view(splitk, n_seq, K1, QKV)

    eng.debug_kv_load(0, kv)
    seq = [eng.debug_attn_decode_slabs(0, by_seq[:, :, j].contiguous(), bias, advance=True).clone() for j in range(K1)]
    seq_probe = [eng.debug_attn_decode_slabs(0, p, bias, advance=False).clone() for p in probes]
    eng.debug_kv_load(0, kv)
    got = eng.debug_attn_decode_draft(0, slabs.contiguous(), n_seq, bias).view(n_seq, K1, H * dh)
    got_probe = [eng.debug_attn_decode_slabs(0, p, bias, advance=False).clone() for p in probes]

    ref = torch.stack(seq, 1)                                                            # [n_seq, K1, H * dh]
    assert bool(torch.isfinite(ref.float()).all()) and float(ref.float().abs().max()) > 0
    diff = (got.contiguous().view(torch.int16) != ref.contiguous().view(torch.int16)).view(n_seq, K1, -1).sum(-1)
    assert int(diff.sum()) == 0, f"{geom} ctx {ctx} n_seq {n_seq} K1 {K1}: outputs that differ per (sequence, row): {diff.tolist()}"
    # a later row does look at its siblings: row K1 - 1 over a cache without them is another answer
    eng.debug_kv_load(0, kv)
    for _ in range(K1 - 1):
        eng.debug_attn_decode_slabs(0, (by_seq[:, :, 0] * 0.0).contiguous(), None, advance=True)
    alone = eng.debug_attn_decode_slabs(0, by_seq[:, :, K1 - 1].contiguous(), bias, advance=False)
    assert not torch.equal(alone, ref[:, K1 - 1]), "the last row does not depend on the K / V of the rows in front of it"
    # the page bytes both ways leave behind, read back by one more step at position ctx + K1 (two queries)
    for a, b in zip(seq_probe, got_probe):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{geom} ctx {ctx}: the pages differ after the draft launch"


def test_draft_against_the_restatement():
    cases = [([1, 2, 3, 9, 1, 2, 3, 8, 1, 2, 3], 2, 3, 1, None),       # several matches: the latest wins
             ([1, 2, 3, 4, 1, 2, 3], 8, 3, 1, None),                   # the continuation is shorter than K
             ([1, 2, 3, 4, 5], 4, 3, 1, None),                         # no match at all
             ([5, 6, 7, 9, 9, 7], 3, 3, 1, None),                      # back-off from max_ngram to 1
             ([5, 6, 7, 9, 9, 7], 3, 3, 2, None),                      # ... which min_ngram 2 forbids
             ([4, 4], 3, 3, 1, None), ([4], 3, 8, 1, None),            # L < n
             ([1, 2, 1, 2, 1], 4, 3, 1, 7), ([1, 2, 1, 2, 1], 4, 3, 1, 6)]      # the budget clips the drafts
    for hist, K, mx, mn, max_new in cases:
        assert E.op_lookup_draft(hist, K, mx, mn, max_new) == LK.draft(hist, K, mx, mn, max_new), (hist, K, mx, mn, max_new)
    assert E.op_lookup_draft([1, 2, 3, 9, 1, 2, 3, 8, 1, 2, 3], 2) == [8, 1] and E.op_lookup_draft([5, 6, 7, 9, 9, 7], 3) == [9, 9, 7]
    r = random.Random(5)
    for _ in range(60):                                                # long histories over a small alphabet: more than one block stride
        L = r.choice([3, 17, 255, 256, 257, 700])
        hist = [r.randrange(4) for _ in range(L)]
        K, mx = r.choice([1, 5, 15]), r.choice([1, 3, 8])
        mn = r.randrange(1, mx + 1)
        assert E.op_lookup_draft(hist, K, mx, mn, L + 40) == LK.draft(hist, K, mx, mn, L + 40), (hist, K, mx, mn)


def _fields(st):
    return dict(hist=st.hist, n_emit=st.n_emit, finished=[bool(f) for f in st.finished], n_draft=st.n_draft, rows=st.rows, positions=st.positions,
                limit=st.limit, done=bool(st.done), n_emitted=st.n_emitted, bad=st.bad, steps=st.steps, drafted=st.drafted, accepted=st.accepted)


def _walk_both(model, n_seq, K, max_new, eos=-1, pad=0, stop=(), min_new=0, forced=None, lens=None, vocab=1 << 30, spoil=None):
    """a whole call, every step through the restatement AND through the kernel on the same state; returns the final state and what happened"""
    first = [model(s, [], 0 < min_new) for s in range(n_seq)]
    st = LK.LookupState(n_seq=n_seq, K=K, max_new=max_new, eos=eos, pad=pad, stop=tuple(stop), forced=forced, vocab=vocab)
    st.begin(first, lens or [11 + 3 * s for s in range(n_seq)], [t != eos for t in first])
    dv = copy.deepcopy(st)
    dv.forced = None                                     # (the kernel's drafts of the NEXT step are compared through rows / n_draft below)
    seen = dict(accepted=set(), eos_inside=False, clipped=False, frozen=False)
    while not st.done:
        winners = []
        for s in range(n_seq):
            ctx = st.hist[s][:st.n_emit[s]]
            winners.append([model(s, ctx + st.rows[s][1:j + 1] if j <= st.n_draft[s] else ctx, st.hold_eos(s, j, min_new)) for j in range(K + 1)])
        if spoil:
            spoil(st, winners)
        before = copy.deepcopy(st)
        st.step(winners)
        if forced is not None:                           # the kernel drafts by lookup: hand it the state with the forced drafts of this step
            dv.rows, dv.positions, dv.n_draft = copy.deepcopy(before.rows), copy.deepcopy(before.positions), list(before.n_draft)
        E.op_lookup_accept(dv, winners)
        a, b = _fields(st), _fields(dv)
        if forced is not None:                           # ... and compare everything but the next drafts
            for k in ("rows", "positions", "n_draft"):
                a.pop(k), b.pop(k)
        assert a == b, {k: (a[k], b[k]) for k in a if a[k] != b[k]}
        for s in range(n_seq):
            if before.finished[s]:
                seen["frozen"] = seen["frozen"] or before.hist[s] == st.hist[s]
                continue
            got = st.n_emit[s] - before.n_emit[s]
            seen["accepted"].add(min(got - 1, 2) if before.n_draft[s] else -1)
            seen["eos_inside"] |= st.finished[s] and eos in st.hist[s][before.n_emit[s]:st.n_emit[s] - 1 + 1] and got > 1
            seen["clipped"] |= before.n_draft[s] < K and before.n_emit[s] + K + 1 > max_new
    return st, seen


def _stream_model(streams, eos=None):
    def model(s, prefix, barred):
        t = streams[s][len(prefix)] if len(prefix) < len(streams[s]) else 0
        return (t + 1) % 50 if barred and eos is not None and t == eos else t
    return model


def test_accept_against_the_restatement():
    r = random.Random(11)
    streams = [[r.randrange(3, 9) for _ in range(40)] for _ in range(3)]
    partly = [[t if i % 5 else (t + 1) % 50 for i, t in enumerate(row)] for row in streams]      # runs of 0, 1 and 3 accepted drafts
    # accept 0, some, all (forced drafts: wrong, partly wrong, right), three sequences, budget clipping the last runs
    seen = set()
    for forced in ([[(t + 1) % 50 for t in row] for row in streams], partly, streams):
        st, what = _walk_both(_stream_model(streams), 3, 3, 38, forced=forced)
        assert st.tokens() == [row[:38] for row in streams]
        seen |= what["accepted"]
        assert what["clipped"]
    assert {0, 1, 2} <= seen
    # natural lookup over a repetitive stream
    rep = [[(i % 5) + 3 for i in range(40)], [3, 4] * 20]
    st, what = _walk_both(_stream_model(rep), 2, 7, 40)
    assert st.tokens() == rep and st.accepted > 20
    # EOS inside an accepted run; the finished sequence stays frozen while the other runs on
    eos_streams = [list(streams[0]), list(streams[1])]
    eos_streams[0][6] = 2
    st, what = _walk_both(_stream_model(eos_streams), 2, 3, 30, eos=2, pad=1, forced=eos_streams)
    assert what["eos_inside"] and what["frozen"] and st.tokens()[0] == eos_streams[0][:7] + [1] * 23 and st.tokens()[1] == eos_streams[1][:30]
    # a row-0 stop sequence completed inside a run, across two steps, and by the pads behind row 0's EOS
    for K, where in ((7, 10), (3, 9), (1, 5)):           # K = 3: the steps end at columns 4, 8, 12 -- columns 8 and 9 fall into two steps; K = 1: 4 and 5 do
        s0 = list(streams[0])
        s0[where - 1], s0[where] = 20, 21
        st, what = _walk_both(_stream_model([s0, streams[1], streams[2]]), 3, K, 36, stop=(20, 21), forced=[s0, streams[1], streams[2]])
        assert st.n_emitted == where + 1 and st.tokens() == [s0[:where + 1], streams[1][:where + 1], streams[2][:where + 1]]
    s0 = list(streams[0])
    s0[4] = 2
    st, what = _walk_both(_stream_model([s0, streams[1]]), 2, 3, 30, eos=2, pad=1, stop=(1, 1), forced=[s0, streams[1]])
    assert st.n_emitted == 7 and st.tokens()[0] == s0[:5] + [1, 1]
    # the min-length hold moves an early EOS: the drafts (made without it) go wrong there, the stream is the held one
    s0 = list(streams[0])
    s0[3] = 2
    model = _stream_model([s0], eos=2)
    st, what = _walk_both(model, 1, 3, 20, eos=2, pad=1, min_new=8, forced=[s0])
    assert st.tokens() == LK.plain_greedy(model, 1, 20, 2, 1, (), 8) and 2 not in st.tokens()[0][:8]
    # a row without a finite logit: the winner is out of range -> id 0 and the flag

    def spoil(state, winners):
        if state.steps == 2:
            winners[0][0] = 0x7fffffff
    st, what = _walk_both(_stream_model(streams), 1, 3, 20, forced=[streams[0]], vocab=50, spoil=spoil)
    assert st.bad == 1


def test_min_length_hold_per_row():
    g = torch.Generator(device=dev()).manual_seed(3)
    K1, n_emit, min_new, eos = 4, [1, 5, 9], 8, 6
    x = torch.randn(3 * K1, 40, generator=g, device=dev())
    y = E.op_lookup_hold(x, K1, eos, min_new, n_emit)
    st = LK.LookupState(n_seq=3, K=K1 - 1, max_new=32)
    st.n_emit = n_emit
    ref = x.clone()
    for r in range(3 * K1):
        if st.hold_eos(r // K1, r % K1, min_new):
            ref[r, eos] = float("-inf")
    assert torch.equal(y, ref) and int(torch.isinf(y).sum()) == 4 + 3 + 0
    assert torch.equal(E.op_lookup_hold(x, K1, eos, 0, n_emit), x)
