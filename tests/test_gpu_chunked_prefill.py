"""-m gpu: the prompt-pass row budget (sv_set_prefill_chunk).  On a bf16 cache every call returns with a budget exactly what it returns
without one -- logits, greedy / sampled / beam tokens, the shared prompt pass, a continuous batch beside a live slot -- while the prompt
runs as several passes over the cache; an e4m3 cache stays inside LOGIT_TOL of the oracle over its own cache."""
import pytest
import torch

from oracle import starvector_oracle as O
from tests.gpu_util import bf, dev
from tests.test_gpu_e2e import LOGIT_TOL, _golden
from tests.test_gpu_kv_fp8 import _build, _teacher_forced_quantised
from tests.test_gpu_ragged_prefill import _embeds, _tiny_engine
from tests.test_gpu_shared_prompt import SAMPLING

pytestmark = pytest.mark.gpu

LENS = [259, 40, 300, 7]
BUDGETS = [64, 256]


def _each_budget(eng, call, tag, min_passes=2):
    """call() with the budget off, then under every budget: the same result, from more prompt passes"""
    eng.set_prefill_chunk(0)
    before = eng.prompt_passes()
    want = call()
    base = eng.prompt_passes() - before
    for budget in BUDGETS:
        eng.set_prefill_chunk(budget)
        before = eng.prompt_passes()
        got = call()
        assert eng.prompt_passes() - before >= base + min_passes - 1, f"{tag}, budget {budget}: the prompt was not chunked"
        assert torch.equal(got, want), f"{tag}, budget {budget}"
    eng.set_prefill_chunk(0)
    return want


@pytest.mark.parametrize("arch,window", [("v1", 0), ("v2", 24)])
def test_prefill_and_generate_return_the_same_under_a_budget(arch, window):
    cfg, eng = _tiny_engine(arch, max_batch=8, max_seq_len=400, window=window)
    seqs = _embeds(LENS, cfg.hidden, 71)
    rect = torch.stack(_embeds([130] * 3, cfg.hidden, 72)).contiguous()
    n_new = 24
    _each_budget(eng, lambda: eng.prefill_ragged(seqs), f"{arch} sv_prefill_ragged")
    _each_budget(eng, lambda: eng.prefill(rect), f"{arch} sv_prefill")
    for name, kw in (("greedy", dict(eos_token_id=-1)), ("sampling", SAMPLING),
                     ("beams", dict(num_beams=2, eos_token_id=-1, pad_token_id=0))):
        _each_budget(eng, lambda: eng.generate_ragged(seqs, max_length=max(LENS) + n_new, **kw).cpu(), f"{arch} sv_generate_ragged {name}")
        _each_budget(eng, lambda: eng.generate(rect, max_length=130 + n_new, **kw).cpu(), f"{arch} sv_generate {name}")
    eng.close()


def test_generate_shared_returns_the_same_under_a_budget():
    cfg, eng = _tiny_engine("v1", max_batch=8, max_seq_len=400)
    prompts = _embeds([150, 259], cfg.hidden, 73)
    _each_budget(eng, lambda: eng.generate_shared(prompts, max_length=259 + 20, n_samples=3, **SAMPLING).cpu(), "sv_generate_shared")
    eng.close()


def test_continuous_batch_admits_a_long_request_beside_a_live_slot():
    cfg, eng = _tiny_engine("v1", max_batch=4, max_seq_len=400)
    short, long_ = _embeds([50, 300], cfg.hidden, 74)
    reqs = [dict(max_new_tokens=40, eos_token_id=-1), dict(max_new_tokens=30, eos_token_id=-1, repetition_penalty=1.2)]

    def run():
        eng.cb_reset()
        slots = eng.cb_admit([short], reqs[:1])
        assert eng.cb_step(5) == 1
        slots += eng.cb_admit([long_], reqs[1:])                # 300 rows join while slot 0 is live
        while eng.cb_step(8) > 0:
            pass
        _, st = eng.cb_poll()
        out = [eng.cb_read(s, 0, st[s]) for s in slots]
        eng.cb_reset()
        return torch.cat([o.cpu() for o in out])
    want = _each_budget(eng, run, "continuous batch")
    assert want.numel() == 70
    eng.close()


def test_e4m3_cache_chunked_end_to_end_stays_inside_the_logit_tolerance():
    g = _golden("tiny_b3")
    seed, B, n_new = [int(x) for x in g["meta"]]
    cfg = O.OracleConfig.tiny()
    w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)
    eng = _build(cfg, w, max_batch=4, max_seq_len=96)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    eng.set_prefill_chunk(max(emb.shape[1] // 2 + 1, 1))       # every prompt is cut once: its second piece reads the e4m3 pages of its first
    before = eng.prompt_passes()
    worst, scale, checked, near, _, _ = _teacher_forced_quantised(eng, emb, w, cfg, n_new)
    assert eng.prompt_passes() - before >= 2
    print(f"[chunked, e4m3 KV] logits max|err| {worst:.3e} (scale {scale:.3e}, bound {LOGIT_TOL * scale:.3e}); {checked} positions checked exactly")
    assert checked > 0
    eng.close()
