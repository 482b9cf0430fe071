"""-m gpu: the packed prompt passes IN SEQUENCE on one engine -- shared-prefix scoring, ragged generation (which reads the uploaded descriptors
after the pass has returned) and ragged scoring share one plan image that grows on demand.

Contract: what a call returns does not depend on the calls before it.  Every call is repeated after the plan image has grown, and compared with
the same call on a fresh engine with the same weights.  No tolerance anywhere: torch.equal on the tokens and on the int32 view of every
returned tensor."""
import pytest
import torch

from starvector_amd import engine as E
from tests.test_gpu_ragged_scoring import FIELDS, TOP_K, _bits, _embeds, _targets, _tiny_engine

pytestmark = pytest.mark.gpu

PLENS, LENS, PREFIX_OF, KEEP = [33, 33], [5, 31, 32, 40], [0, 1, 0, 1], [6, 1, 3, 40]      # T = 38, 64, 65, 73: around the 32-row tile; keep = len + 1 and 1
GEN_LENS, N_NEW = [5, 37], 8
# 256 + 1 and 256 + 3 rows.  Which of them are remainder rows is the dispatch's rule per projection: at the tiny v2 dimensions the 257-row sequences
# have one at c_fc; at the tiny v1 dimensions no projection takes the per-sequence form at any length (E.gemm_seq_form), so v1 runs without
BIG_LENS, BIG_KEEP = [257, 259] * 8, [3] * 16
MAX_BATCH, MAX_SEQ_LEN = 16, 320


def _tiles(lens, tile):
    return sum((n + tile - 1) // tile for n in lens)


def _projections(cfg):
    D, F, dh = cfg.hidden, cfg.n_inner, cfg.hidden // cfg.n_head
    qkv = cfg.n_head * dh + 2 * max(int(cfg.n_kv_head), 1) * dh
    return ((qkv, D, "none"), (D, D, "none"), (F, D, "gelu_tanh"), (D, F, "none"))


def _assert_the_plan_image_grows(cfg, remainder_rows):
    """int32 entries of the plans, from the host arithmetic alone: the first call's plan at most (32-row query tiles, every list), the big call's at
    least (128-row query tiles, no remainder-row list); the image is allocated for need + need / 2 + 256 entries"""
    P, B = len(PLENS), len(LENS)
    first = 3 * (P + B) + 2 * P + 2 * _tiles(PLENS, 32) + 4 * B + sum(KEEP)
    first += 2 * len(E.prefix_plan(PLENS, LENS, PREFIX_OF, *_projections(cfg)[0], q_tile=32)["blocks"])
    first += sum(len(E.prefix_plan(PLENS, LENS, PREFIX_OF, *p)["rows"]) for p in _projections(cfg))
    big = 2 * len(BIG_LENS) + 2 * _tiles(BIG_LENS, 128) + 2 * _tiles(BIG_LENS, 32) + 4 * len(BIG_LENS)
    assert big > first + first // 2 + 256, (first, big)
    assert any(E.ragged_plan(BIG_LENS, *p)["rows"] for p in _projections(cfg)) == remainder_rows


def _calls(cfg):
    pre, own = _embeds(PLENS, cfg.hidden, 501), _embeds(LENS, cfg.hidden, 502)
    tg = torch.cat(_targets(KEEP, cfg.vocab, 503))
    gen = _embeds(GEN_LENS, cfg.hidden, 504)
    big, big_tg = _embeds(BIG_LENS, cfg.hidden, 505), torch.cat(_targets(BIG_KEEP, cfg.vocab, 506))
    kw = dict(entropy=True, argmax=True, top_k=TOP_K)
    fields = lambda r: [_bits(getattr(r, f)).cpu() for f in FIELDS]
    return [("prefixed scoring", lambda eng: fields(eng.forward_logprobs_prefixed(pre, own, PREFIX_OF, tg, KEEP, **kw))),
            ("ragged generation", lambda eng: [eng.generate_ragged(gen, max_length=max(GEN_LENS) + N_NEW, eos_token_id=-1).cpu()]),
            ("ragged scoring", lambda eng: fields(eng.forward_logprobs_ragged(big, big_tg, BIG_KEEP, **kw)))]


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_packed_passes_in_sequence_across_a_growth_of_the_plan_image(arch):
    cfg, eng = _tiny_engine(arch, max_batch=MAX_BATCH, max_seq_len=MAX_SEQ_LEN)
    assert eng.prefix_refused(PLENS, LENS, PREFIX_OF) == []
    _assert_the_plan_image_grows(cfg, remainder_rows=arch == "v2")
    calls = _calls(cfg)
    first = [run(eng) for _, run in calls]
    assert first[1][0].shape == (len(GEN_LENS), N_NEW)
    for i in (1, 0):                                    # after the growth: the generation again, then the prefixed scoring again
        assert _same(calls[i][1](eng), first[i]), f"[{arch}] {calls[i][0]} differs after the plan image has grown"
    eng.close()
    for (name, run), want in zip(calls, first):
        _, fresh = _tiny_engine(arch, max_batch=MAX_BATCH, max_seq_len=MAX_SEQ_LEN)
        assert _same(run(fresh), want), f"[{arch}] {name} after other passes differs from the same call on a fresh engine"
        fresh.close()
