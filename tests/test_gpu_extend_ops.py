"""-m gpu: prompt rows behind a cached context (sv_prefill_open / sv_prefill_extend) and the two page kernels of csrc/extend/extend.hip.

  * kv_gather_kernel against sv_debug_kv_read, bit for bit: both pool formats, head_dim 128 and 64, MQA and GQA, contexts on both sides of the
    32-token group and the 64-token page;
  * kv_write_extend_kernel through the calls: a cached token keeps what it held, own rows are the one-shot writer's, the tail of the last group
    is zero;
  * contract A (bf16 cache): open + extends with the same total are BIT-IDENTICAL to sv_prefill_ragged over the whole sequence -- logits,
    every K / V entry, the decode steps that follow -- whatever the boundaries and whatever shares the passes;
  * the live remainder form at StarVector-1B dimensions; contract B (e4m3 cache against a bf16 twin, exact); contract C (continuing).
No tolerance anywhere: every comparison is equality of bits."""
import dataclasses

import pytest
import torch

from oracle import starvector_oracle as O
from starvector_amd import engine as E
from tests import kv8_ref as R
from tests.gpu_util import build_engine, dev
from tests.test_gpu_kv_fp8 import _build
from tests.test_gpu_ragged_prefill import _embeds, _fullsize_engine, _tiny_engine

pytestmark = pytest.mark.gpu

CONTEXTS = [1, 31, 32, 33, 63, 64, 65, 130]
LENS = [5, 70, 130, 259, 300]
# every sequence is cut at these solo indices (those below its length): the 32- and 128-row query tiles, the 256-row GEMM tile, the peel rows of 259
CUTS = ([10, 31, 128, 256, 258], [23, 32, 129, 257], [24, 33, 127, 255], [25, 64, 200])


def _pages(eng, n_layer, row, n, first=0):
    return torch.stack([eng.debug_kv_read(i, row, first, n) for i in range(n_layer)]).cpu()


def _deq_quant(rows, head_dim):
    """tests/kv8_ref.py over rows of [.., k heads | v heads]: one scale per token, head and K / V"""
    return R.deq_quant(rows.reshape(*rows.shape[:-1], -1, head_dim)).reshape(rows.shape)


def _cfg(arch, head_dim):
    base = O.OracleConfig.tiny() if arch == "v1" else O.OracleConfig.tiny_v2()
    if head_dim == 64:      # MQA 4 / 1 and GQA 12 / 4 over the same hidden sizes
        base = dataclasses.replace(base, n_head=4) if arch == "v1" else dataclasses.replace(base, n_head=12, n_kv_head=4)
    return dataclasses.replace(base, n_positions=256, eos_token_id=-1)


@pytest.mark.parametrize("kv", ["bf16", "fp8_e4m3"])
@pytest.mark.parametrize("arch,head_dim", [("v1", 128), ("v1", 64), ("v2", 128), ("v2", 64)])
def test_kv_gather_is_kv_read_bit_for_bit(arch, head_dim, kv):
    cfg = _cfg(arch, head_dim)
    eng = _build(cfg, O.make_weights(cfg, seed=77), kv, max_batch=2, max_seq_len=192)
    n_kv = cfg.n_kv_head if arch == "v2" else 1
    g = torch.Generator().manual_seed(5)
    for ctx in CONTEXTS:
        # rows of very different magnitudes: every e4m3 row gets a scale of its own
        rows = (torch.randn(2, ctx, 2 * n_kv * head_dim, generator=g) * torch.exp2(torch.randint(-6, 6, (2, ctx, 1), generator=g).float()))
        layer = ctx % cfg.n_layer
        eng.debug_kv_load(layer, rows.to(torch.bfloat16).to(dev()))
        for row in (0, 1):
            want = eng.debug_kv_read(layer, row, 0, ctx)
            got = eng.debug_kv_gather(layer, row, ctx)
            assert R.same_bits(got, want), f"{arch} head_dim {head_dim} {kv}: context {ctx}, row {row}"
            if kv == "bf16":
                assert torch.equal(got.cpu(), rows[row].to(torch.bfloat16)), f"{arch} head_dim {head_dim}: the stored bits, context {ctx}"
            else:
                assert R.same_bits(got.cpu(), _deq_quant(rows[row].to(torch.bfloat16), head_dim)), f"{arch} head_dim {head_dim}: deq(quant(.)), context {ctx}"
    eng.close()


@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_writer_keeps_cached_tokens_and_writes_own_rows_as_the_one_shot_writer(arch):
    cfg, eng = _tiny_engine(arch, max_batch=2, max_seq_len=256)
    own = 45                                                    # crosses a group boundary from every start, a page boundary from most
    for start in CONTEXTS:
        total = start + own
        x = _embeds([total], cfg.hidden, 100 + start)[0]
        eng.prefill_ragged([x])
        tail = (-total) % 32
        want = _pages(eng, cfg.n_layer, 0, total + tail)
        assert bool((want[:, total:, want.shape[2] // 2:] == 0).all())          # the one-shot writer's zero tail (V)
        eng.prefill_open([total])
        eng.prefill_extend(x[:start], [start], [total])
        cached = _pages(eng, cfg.n_layer, 0, start)
        assert torch.equal(cached, want[:, :start]), f"{arch}: first piece, {start} rows"
        eng.prefill_extend(x[start:], [own], [total])
        got = _pages(eng, cfg.n_layer, 0, total + tail)
        assert torch.equal(got[:, :start], cached), f"{arch}: cached tokens changed by an extension from {start}"
        assert torch.equal(got[:, start:total], want[:, start:total]), f"{arch}: own rows from {start}"
        assert bool((got[:, total:, got.shape[2] // 2:] == 0).all()), f"{arch}: V tail behind {total}"
    eng.close()


def _reference(eng, cfg, seqs, n_steps=2):
    lg = eng.prefill_ragged(seqs)
    pages = [_pages(eng, cfg.n_layer, b, x.shape[0]) for b, x in enumerate(seqs)]
    steps, cur = [], lg
    for _ in range(n_steps):
        cur = eng.decode_step(cur.argmax(-1))
        steps.append(cur.clone())
    return lg.clone(), pages, steps


def _feed(eng, seqs, cuts):
    """open + one extend per cut (and one to the end): every sequence grows to min(its length, cut); -> the last-row logits"""
    lens = [int(x.shape[0]) for x in seqs]
    eng.prefill_open(lens)
    at, logits = [0] * len(seqs), torch.full((len(seqs), eng.cfg.vocab), float("nan"), device=dev())
    for cut in list(cuts) + [max(lens)]:
        take = [max(min(n, cut) - a, 0) for n, a in zip(lens, at)]
        if sum(take) == 0:
            continue
        lg = eng.prefill_extend([x[a:a + t] for x, a, t in zip(seqs, at, take) if t > 0], take, lens)
        for b, (n, a, t) in enumerate(zip(lens, at, take)):
            if t > 0 and a + t == n:
                logits[b] = lg[b]
            else:
                assert bool(torch.isnan(lg[b]).all()), f"logits row {b} written for a sequence that did not finish"
        at = [a + t for a, t in zip(at, take)]
    return logits


@pytest.mark.parametrize("arch,window", [("v1", 0), ("v2", 24)])
def test_contract_a_open_and_extends_equal_the_one_shot_ragged_pass(arch, window):
    cfg, eng = _tiny_engine(arch, max_batch=8, max_seq_len=384, window=window)
    seqs = _embeds(LENS, cfg.hidden, 11)
    ref_lg, ref_pages, ref_steps = _reference(eng, cfg, seqs)
    for cuts in CUTS:
        lg = _feed(eng, seqs, cuts)
        assert torch.equal(lg, ref_lg), f"{arch} cuts {cuts}: last-row logits"
        for b, n in enumerate(LENS):
            assert torch.equal(_pages(eng, cfg.n_layer, b, n), ref_pages[b]), f"{arch} cuts {cuts}: pages of sequence {b} ({n} rows)"
        cur = lg
        for t, want in enumerate(ref_steps):
            cur = eng.decode_step(cur.argmax(-1))
            assert torch.equal(cur, want), f"{arch} cuts {cuts}: decode step {t}"
    # a sequence alone, fed row by row across the first group boundary, equals itself inside the batch
    x = seqs[1]
    eng.prefill_open([x.shape[0]])
    for j in range(34):
        eng.prefill_extend(x[j:j + 1], [1], [x.shape[0]])
    lg = eng.prefill_extend(x[34:], [x.shape[0] - 34], [x.shape[0]])
    assert torch.equal(lg[0], ref_lg[1]) and torch.equal(_pages(eng, cfg.n_layer, 0, x.shape[0]), ref_pages[1])
    eng.close()


def test_live_remainder_form_at_starvector_1b_dimensions():
    ec, eng = _fullsize_engine(max_batch=4, max_seq_len=640)
    D, F = ec.hidden, ec.n_inner
    assert E.gemm_seq_form(259, D, D, "none") and E.gemm_seq_form(515, D, F, "none")          # the remainder kernel is live at these lengths
    lens = [259, 515]
    seqs = _embeds(lens, D, 21, scale=0.5)
    ref_lg, ref_pages, ref_steps = _reference(eng, ec, seqs, n_steps=1)
    for cuts in ([256], [257, 514]):                             # a boundary in front of the three peel rows of 259, and inside them (and of 515)
        plan = E.extend_plan([0, 0], [min(n, cuts[0]) for n in lens], lens, D, D, "none")
        assert [p["rows"] for p in plan] == ([[]] if cuts[0] == 256 else [[256]]), plan
        lg = _feed(eng, seqs, cuts)
        assert torch.equal(lg, ref_lg), f"cuts {cuts}: last-row logits"
        for b, n in enumerate(lens):
            assert torch.equal(_pages(eng, ec.n_layer, b, n), ref_pages[b]), f"cuts {cuts}: pages of sequence {b}"
        assert torch.equal(eng.decode_step(lg.argmax(-1)), ref_steps[0]), f"cuts {cuts}: decode step"
    for budget in (256, 258):                                    # the same through the knob: 258 cuts 259's peel rows after the second
        eng.set_prefill_chunk(budget)
        assert torch.equal(eng.prefill_ragged(seqs), ref_lg), f"budget {budget}"
        for b, n in enumerate(lens):
            assert torch.equal(_pages(eng, ec.n_layer, b, n), ref_pages[b]), f"budget {budget}: pages of sequence {b}"
    eng.close()


@pytest.mark.parametrize("arch", ["v1", "v2"])
@pytest.mark.parametrize("ctx", [33, 64])
def test_contract_b_e4m3_cache_is_exact_against_a_bf16_twin(arch, ctx):
    base = O.OracleConfig.tiny() if arch == "v1" else O.OracleConfig.tiny_v2()
    cfg = dataclasses.replace(base, n_positions=256, eos_token_id=-1)
    w = O.make_weights(cfg, seed=77)
    a = _build(cfg, w, "fp8_e4m3", max_batch=2, max_seq_len=192)
    b = build_engine(cfg, w, max_batch=2, max_seq_len=192)
    own = 40
    x = _embeds([ctx + own], cfg.hidden, 31)[0]
    # 1. the first piece from context 0: both engines see their own rows unquantised
    for e in (a, b):
        e.prefill_open([ctx + own])
    la, lb = a.prefill_extend(x[:ctx], [ctx]), b.prefill_extend(x[:ctx], [ctx])
    assert torch.equal(la, lb)
    cache_a = _pages(a, cfg.n_layer, 0, ctx)
    dh = cfg.hidden // cfg.n_head
    assert R.same_bits(cache_a, _deq_quant(_pages(b, cfg.n_layer, 0, ctx), dh))
    # 2. the twin's cache <- A's dequantised rows, then the same piece on both
    for layer in range(cfg.n_layer):
        b.debug_kv_load(layer, cache_a[layer][None].to(dev()))
    la, lb = a.prefill_extend(x[ctx:], [own]), b.prefill_extend(x[ctx:], [own])
    assert torch.equal(la, lb)
    assert R.same_bits(_pages(a, cfg.n_layer, 0, own, first=ctx), _deq_quant(_pages(b, cfg.n_layer, 0, own, first=ctx), dh))
    assert R.same_bits(_pages(a, cfg.n_layer, 0, ctx), cache_a), "an extension changed the bytes of cached tokens"
    tail = (-(ctx + own)) % 32
    if tail:
        assert bool((_pages(a, cfg.n_layer, 0, tail, first=ctx + own) == 0).all()), "tokens behind the new end: code 0, scale byte 127"
    a.close()
    b.close()


def test_contract_c_decode_continues_an_extended_cache():
    cfg, eng = _tiny_engine("v1", max_batch=2, max_seq_len=128)
    x = _embeds([23], cfg.hidden, 41)[0]
    lg = eng.prefill_ragged([x])
    want = eng.decode_step(lg.argmax(-1)).clone()
    eng.prefill(x[None, :20].contiguous())
    got = eng.prefill_extend(x[20:], [3])
    assert torch.equal(got, lg)
    assert torch.equal(eng.decode_step(got.argmax(-1)), want)
    # ... and an extension continues a decoded cache: the context the host keeps grew with the step
    y = _embeds([4], cfg.hidden, 42)[0]
    eng.prefill_ragged([x])
    eng.decode_step(lg.argmax(-1))
    before = _pages(eng, cfg.n_layer, 0, 24)
    lg2 = eng.prefill_extend(y, [4])                             # rows at positions 24..27
    assert bool(torch.isfinite(lg2).all()) and torch.equal(_pages(eng, cfg.n_layer, 0, 24), before)
    assert float(_pages(eng, cfg.n_layer, 0, 4, first=24).abs().max()) > 0
    assert bool(torch.isfinite(eng.decode_step(lg2.argmax(-1))).all())
    # unknown contexts behind a generate call
    eng.generate(x[None].contiguous(), max_length=30, eos_token_id=-1)
    with pytest.raises(Exception) as ei:
        eng.prefill_extend(y, [4])
    assert "context" in str(ei.value)
    eng.close()


def test_argument_errors_that_read_the_engines_contexts():
    """SV_EINVAL / SV_ESTATE with their messages, the cache untouched: B against the cached sequences, ctx + len > total, a total beyond the
    pages or max_seq_len, unknown contexts, an active continuous batch."""
    from starvector_amd._lib import StarVectorHipError
    cfg, eng = _tiny_engine("v1", max_batch=4, max_seq_len=128)
    x = _embeds([40], cfg.hidden, 51)[0]
    eng.prefill_open([70, 40])
    eng.prefill_extend(x[:30], [30, 0], [70, 40])
    before = _pages(eng, cfg.n_layer, 0, 30)
    for lens, totals, what in (([5], None, "cache holds 2"), ([5, 0, 0], None, "cache holds 2"), ([10, 0], [39, 40], "exceeds its total length"),
                               ([10, 0], [129, 40], "exceeds its pages"), ([0, 10], [70, 65], "exceeds its pages")):
        with pytest.raises(ValueError, match=what):
            eng.prefill_extend(x[:sum(lens)], lens, totals)
    with pytest.raises(ValueError, match="max_seq_len"):
        eng.prefill_open([129])
    assert torch.equal(_pages(eng, cfg.n_layer, 0, 30), before)
    lg = eng.prefill_extend(x[:10], [0, 10], [70, 40])           # the refused calls left the state as it was: row 1 is still at context 0
    assert bool(torch.isnan(lg).all())
    eng.generate(x[None].contiguous(), max_length=50, eos_token_id=-1)
    with pytest.raises(StarVectorHipError, match="context lengths of the cache are unknown") as ei:
        eng.prefill_extend(x[:4], [4])
    assert not isinstance(ei.value, ValueError)                  # SV_ESTATE, not SV_EINVAL
    eng.cb_reset()
    eng.cb_admit([x], [dict(max_new_tokens=4, eos_token_id=-1)])
    with pytest.raises(StarVectorHipError, match="continuous batch") as ei:
        eng.prefill_extend(x[:4], [4])
    assert not isinstance(ei.value, ValueError)
    with pytest.raises(StarVectorHipError, match="continuous batch"):
        eng.prefill_open([20])
    eng.cb_reset()
    eng.close()
