"""GPU: engines with the e4m3 KV cache (sv_create_kv, SV_KV_FP8_E4M3) end to end on the tiny v1 and v2 configurations.

  * teacher-forced logits against the oracle driven step by step: after the prompt pass, and after every step, the oracle cache's new rows
    are replaced by tests/kv8_ref.py's dequantisation -- the prompt pass's own logits come from the unquantised prompt and a step sees its
    own row unquantised, as in the engine.  Bound: LOGIT_TOL through tests/test_gpu_e2e.py `_teacher_forced_check`.
  * exactness on ONE fp8-KV engine: the ragged prompt pass writes the pages the rectangular one writes, sv_generate_shared equals the
    repeated prompts, a continuous-batch request equals its solo sv_generate, beam search across the token-64 page boundary reproduces
    under exclusive_device 0 and 1 (the tail-page copy moves the scale bytes too).
  * the lookup entry points answer SV_ENOTSUP, sv_kv_info reports the format and the halved pool, sv_create and sv_create_kv(.., 0, ..)
    engines produce identical tokens."""
import dataclasses
from unittest import mock

import pytest
import torch

import starvector_amd as sva
from oracle import starvector_oracle as O
from starvector_amd.engine import kv_page_bytes, kv_pool_bytes
from tests import kv8_ref as R
from tests.gpu_util import bf, build_engine, dev
from tests.test_gpu_e2e import LOGIT_TOL, _golden, _teacher_forced_check
from tests.test_gpu_shared_prompt import SAMPLING, _embeds, _rect, _shared_equals_repeated

pytestmark = pytest.mark.gpu


def _build(cfg, w, kv="fp8_e4m3", **kw):
    """tests/gpu_util.py build_engine with the KV format swapped in"""
    ec = sva.EngineConfig
    with mock.patch.object(sva, "EngineConfig", lambda **k: ec(**k, kv_dtype=kv)):
        eng = build_engine(cfg, w, **kw)
    assert eng.kv_info()["kv_dtype"] == sva.engine.resolve_kv_dtype(kv)
    return eng


def _tiny(arch, max_batch, max_seq_len, kv="fp8_e4m3", window=0, **kw):
    base = O.OracleConfig.tiny() if arch == "v1" else O.OracleConfig.tiny_v2()
    cfg = dataclasses.replace(base, n_positions=max(base.n_positions, max_seq_len), eos_token_id=-1, sliding_window=window)
    w = O.make_weights(cfg, seed=77)
    return cfg, w, _build(cfg, w, kv, max_batch=max_batch, max_seq_len=max_seq_len, **kw)


class _QuantisedCacheOracle:
    """The oracle's prompt pass and decode step with the cache rows they ADD replaced by deq(quant(.)) on the way out: the pass that
    computes a row sees it unquantised, every later step reads the quantised row."""

    def __init__(self):
        self.prefill, self.step = O.decoder_prefill, O.decoder_decode_step

    @staticmethod
    def _q(t, first):
        t = t.clone()
        t[..., first:, :] = R.deq_quant(t[..., first:, :]).to(t.dtype)
        return t

    def decoder_prefill(self, w, cfg, emb, mode="fp32"):
        logits, cache = self.prefill(w, cfg, emb, mode)
        return logits, [(self._q(k, 0), self._q(v, 0)) for k, v in cache]

    def decoder_decode_step(self, w, cfg, tokens, cache, mode="fp32"):
        logits, cache = self.step(w, cfg, tokens, cache, mode)
        n = cache[0][0].shape[-2]
        return logits, [(self._q(k, n - 1), self._q(v, n - 1)) for k, v in cache]


def _teacher_forced_quantised(eng, emb, w, cfg, n_new):
    q = _QuantisedCacheOracle()
    with mock.patch.object(O, "decoder_prefill", q.decoder_prefill), mock.patch.object(O, "decoder_decode_step", q.decoder_decode_step):
        return _teacher_forced_check(eng, emb, w, cfg, n_new)


@pytest.mark.parametrize("name", ["tiny_b3", "tiny_v2_b2"])
def test_teacher_forced_logits_against_the_oracle_over_the_quantised_cache(name):
    g = _golden(name)
    seed, B, n_new = [int(x) for x in g["meta"]]
    if name == "tiny_b3":
        cfg = O.OracleConfig.tiny()
        w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)
    else:
        cfg = O.OracleConfig.tiny_v2()
        w = O.make_weights(cfg, seed=seed)
    eng = _build(cfg, w, max_batch=4, max_seq_len=96)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    worst, scale, checked, near, o_toks, margin = _teacher_forced_quantised(eng, emb, w, cfg, n_new)
    print(f"[kv fp8 {name}] logits max|err| {worst:.3e} (scale {scale:.3e}, bound {LOGIT_TOL * scale:.3e}); {checked} token positions checked "
          f"exactly, {near} near-tie flips")
    assert checked > 0
    # the cache the engine holds is the restatement of the oracle's rows to within the logits' own tolerance upstream; the last layer's
    # rows of row 0 are finite and carry a scale
    got = eng.debug_kv_read(cfg.n_layer - 1, 0, 0, emb.shape[1] + n_new - 1).float()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    eng.close()


def _pages(eng, n_layer, row, n):
    return torch.stack([eng.debug_kv_read(i, row, 0, n) for i in range(n_layer)]).cpu()


@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_exactness_on_one_fp8_kv_engine(arch):
    cfg, w, eng = _tiny(arch, max_batch=12, max_seq_len=256)
    # the ragged prompt pass writes the pages the rectangular one writes
    lens = [37, 64, 65, 128, 150]
    seqs = _embeds(lens, cfg.hidden, 7)
    solo = []
    for x in seqs:
        eng.prefill(x[None].contiguous())
        solo.append(_pages(eng, cfg.n_layer, 0, x.shape[0]))
    eng.prefill_ragged(seqs)
    for b, n in enumerate(lens):
        assert R.same_bits(_pages(eng, cfg.n_layer, b, n), solo[b]), f"{arch}: ragged pass, sequence {b} ({n} rows)"
    # one prompt pass for a request's samples
    _shared_equals_repeated(eng, cfg.hidden, 3, 4, [40, 128, 150], 36, f"{arch} fp8 KV")
    # a continuous-batch request equals its solo generate (greedy and sampled), admitted beside others
    emb = _rect(_embeds([70] * 4, cfg.hidden, 9))
    n_new = 40
    alone = [eng.generate(emb[i:i + 1].contiguous(), max_length=70 + n_new, eos_token_id=-1).cpu()[0].tolist() for i in range(4)]
    eng.cb_reset()
    slots = eng.cb_admit(emb.contiguous(), [dict(max_new_tokens=n_new, eos_token_id=-1)] * 4)
    while eng.cb_step(8) > 0:
        pass
    for i, s in enumerate(slots):
        assert eng.cb_read(s, 0, eng.cb_poll()[1][s]).tolist() == alone[i], f"{arch}: continuous-batch request {i}"
    eng.cb_reset()
    eng.close()


@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_beam_search_across_the_page_boundary_under_both_device_modes(arch):
    """num_beams 2 from a 50-row prompt over 40 tokens: the beams' tail page is copied at every reorder in front of token 64, and a copied
    page carries its scale bytes (page_bytes is the format's).  The same tokens with and without the fused launches, twice each."""
    outs = []
    for exclusive in (False, True):
        cfg, w, eng = _tiny(arch, max_batch=8, max_seq_len=128, exclusive_device=exclusive)
        emb = _rect(_embeds([50] * 3, cfg.hidden, 11))
        kw = dict(max_length=50 + 40, num_beams=2, eos_token_id=-1, pad_token_id=0)
        a = eng.generate(emb, **kw).cpu()
        assert torch.equal(a, eng.generate(emb, **kw).cpu())
        outs.append(a)
        eng.close()
    assert outs[0].shape == (3, 40) and torch.equal(outs[0], outs[1])


def test_lookup_entry_points_answer_enotsup():
    cfg, w, eng = _tiny("v1", max_batch=8, max_seq_len=128)
    emb = _rect(_embeds([20] * 2, cfg.hidden, 13))
    with pytest.raises(NotImplementedError, match="KV cache"):
        eng.generate_lookup(emb, max_length=30, num_draft_tokens=3, eos_token_id=-1)
    with pytest.raises(NotImplementedError, match="KV cache"):
        eng.generate_lookup_sampled(emb, max_length=30, num_draft_tokens=3, eos_token_id=-1, do_sample=True, seed=1)
    with pytest.raises(NotImplementedError, match="KV cache"):
        eng.cb_set_lookup(3)
    eng.debug_kv_load(0, torch.zeros(2, 8, 2 * cfg.head_dim, dtype=torch.bfloat16, device=dev()))
    qkv_w = cfg.hidden + 2 * cfg.head_dim
    with pytest.raises(NotImplementedError, match="KV cache"):
        eng.debug_attn_decode_draft(0, torch.zeros(1, 4, qkv_w, device=dev()), 2)
    # the plain calls still run, and a lookup call with no drafts is the plain call
    a = eng.generate(emb, max_length=30, eos_token_id=-1).cpu()
    assert torch.equal(eng.generate_lookup(emb, max_length=30, num_draft_tokens=0, eos_token_id=-1).cpu(), a)
    eng.cb_set_lookup(0)
    eng.close()


@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_kv_info_and_the_default_format(arch):
    cfg, w, f8 = _tiny(arch, max_batch=4, max_seq_len=200)
    info = f8.kv_info()
    assert info == dict(kv_dtype="fp8_e4m3", page_bytes=kv_page_bytes("fp8_e4m3", cfg.head_dim), pool_bytes=kv_pool_bytes(f8.cfg)), info
    emb = _rect(_embeds([30] * 2, cfg.hidden, 17))
    f8.close()
    # bf16: sv_create and sv_create_kv(.., SV_KV_BF16, ..) are one engine
    _, _, plain = _tiny(arch, max_batch=4, max_seq_len=200, kv="bf16")
    assert plain.kv_info() == dict(kv_dtype="bf16", page_bytes=kv_page_bytes("bf16", cfg.head_dim), pool_bytes=kv_pool_bytes(plain.cfg))
    assert info["pool_bytes"] <= 0.51 * plain.kv_info()["pool_bytes"]
    want = plain.generate(emb, max_length=30 + 40, **SAMPLING).cpu()
    greedy = plain.generate(emb, max_length=30 + 40, eos_token_id=-1).cpu()
    plain.close()
    lib = sva._lib.load()
    with mock.patch.object(lib, "sv_create", None):                            # "bfloat16" is created through sv_create_kv(.., 0, ..) alone
        _, _, viakv = _tiny(arch, max_batch=4, max_seq_len=200, kv="bfloat16")
    assert torch.equal(viakv.generate(emb, max_length=30 + 40, **SAMPLING).cpu(), want)
    assert torch.equal(viakv.generate(emb, max_length=30 + 40, eos_token_id=-1).cpu(), greedy)
    viakv.close()
