"""-m gpu: the shared-prefix scoring pass -- G completions per prompt pass of their image's visual rows (sv_forward_logprobs_prefixed;
HipEngine.forward_logprobs_prefixed; completion_logprobs(..., share_prefix=True)) and the prefixed form of the prompt-pass attention on its own
(sv_op_attn_prefill_prefixed).

Contract: every output of a sequence's kept rows is BIT-IDENTICAL to sv_forward_topk on concat(prefix, own rows) alone, whatever the other
sequences, their order, the number of sharers and the lm_head chunk size: every engine comparison is torch.equal on the int32 view against the
engine's own solo run (which the rest of the suite ties to the oracle, float64 and HF).  The attention operator is held to the bits of the
existing ragged operator on the concatenations and to tests/attn_ref.py's float32 reference within the bound of tests/test_gpu_prefill_attention.py."""
import dataclasses
import types

import pytest
import torch

import starvector_amd as sva
from starvector_amd import engine as E
from starvector_amd._lib import StarVectorHipError
from starvector_amd.model import StarVectorForCausalLM
from tests.attn_ref import ref
from oracle import starvector_oracle as O
from tests.gpu_util import bf, build_engine, dev
from tests.test_gpu_prefill_attention import GEOM_IDS, GEOMS, Layout, check_close, fuse, run, same_bits, sentinel_out, untouched
from tests.test_gpu_ragged_prefill import LENS, _shuffled
from tests.test_gpu_ragged_scoring import FIELDS, KEEP_OF, _check_contract as _ragged_contract, _embeds, _targets, _tiny_engine

pytestmark = pytest.mark.gpu
TOP_K = 5


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the attention operator ----------------------------------------------------------------------------------------------------------------
OWN = (1, 3, 31, 40, 200)


def _attention_case(geom, plens, lens, prefix_of, window, seed):
    """packed rows (prefixes, then own rows) and the same rows as concatenations; the prefixed operator against the ragged one and float32"""
    H, Hkv, hd = GEOMS[geom]
    lay = Layout(H, Hkv, hd)
    rows, MP, width = sum(plens) + sum(lens), sum(plens), H * hd
    g = torch.Generator().manual_seed(seed)
    q = (3 * torch.randn(rows, H * hd, generator=g)).bfloat16().float()
    k = torch.randn(rows, Hkv * hd, generator=g).bfloat16().float()
    v = torch.randn(rows, Hkv * hd, generator=g).bfloat16().float()
    p0 = [sum(plens[:u]) for u in range(len(plens))]
    o0 = [MP + sum(lens[:b]) for b in range(len(lens))]
    idx = torch.cat([torch.cat([torch.arange(p0[u], p0[u] + plens[u]), torch.arange(o0[b], o0[b] + lens[b])]) for b, u in enumerate(prefix_of)])
    T = [plens[u] + lens[b] for b, u in enumerate(prefix_of)]
    PAD = 40                                                                   # rows behind the packed ones: never addressed
    out = E.op_attn_prefill_prefixed(fuse(q, k, v, lay, extra_rows=PAD), lay.q_off, lay.k_off, lay.v_off, H, Hkv, hd, plens, lens, prefix_of,
                                     window=window, out=sentinel_out(rows + PAD, width))
    torch.cuda.synchronize()
    tag = f"prefixed {geom} prefixes {plens} own {lens} W={window}"
    assert untouched(out[:MP]), (tag, "a prefix row of the output was written")
    assert untouched(out[rows:]), (tag, "a row behind the last own row was written")
    cat = run(geom, fuse(q[idx], k[idx], v[idx], lay), lay, lens=T, window=window)      # the existing ragged operator on the concatenations
    want = ref(q[idx], k[idx], v[idx], H, Hkv, T, 1, window)
    r0 = 0
    for b, u in enumerate(prefix_of):
        own = slice(r0 + plens[u], r0 + T[b])
        assert same_bits(out[o0[b]:o0[b] + lens[b]], cat[own]), (tag, b, "differs from the ragged operator on the concatenation")
        r0 += T[b]
    own_rows = torch.cat([torch.arange(sum(T[:b]) + plens[u], sum(T[:b + 1])) for b, u in enumerate(prefix_of)])
    check_close(tag, out[MP:rows], want[own_rows], scale=float(want.abs().max()))


@pytest.mark.parametrize("Pl", [5, 32, 64, 70, 127, 128, 257])
@pytest.mark.parametrize("geom", GEOM_IDS)
def test_attention_prefixed_form_is_the_ragged_form_on_the_concatenation(geom, Pl):
    assert {GEOMS[g][2] for g in GEOM_IDS} == {64, 128}
    _attention_case(geom, [Pl], list(OWN), [0] * len(OWN), 0, 1000 + Pl)


@pytest.mark.parametrize("geom", GEOM_IDS)
def test_attention_prefixed_form_shared_prefixes_any_order_and_the_window(geom):
    # three prefixes, one shared by three sequences, one used once; a window inside the prefix, one straddling its end, one wholly in own rows
    _attention_case(geom, [70, 5, 128], [40, 3, 200, 31, 1], [2, 0, 0, 1, 0], 0, 2001)
    _attention_case(geom, [100, 7], [3, 24, 25, 70, 3, 70], [0, 0, 0, 0, 1, 1], 24, 2002)
    _attention_case(geom, [100, 7], [70, 25], [1, 0], 100, 2003)


# ---- the bitwise contract ------------------------------------------------------------------------------------------------------------------
def _cats(prefixes, seqs, prefix_of):
    return [torch.cat([prefixes[u], x]) for u, x in zip(prefix_of, seqs)]


def _solo(eng, cats, targets, keep, temperature):
    return [eng.forward_logprobs(x[None].contiguous(), t[None].contiguous(), n, temperature, entropy=True, argmax=True, top_k=TOP_K)
            for x, t, n in zip(cats, targets, keep)]


def _check_prefixed(eng, prefixes, seqs, prefix_of, targets, keep, solo, temperature, tag):
    got = eng.forward_logprobs_prefixed(prefixes, seqs, prefix_of, torch.cat(targets), keep, temperature=temperature, entropy=True, argmax=True,
                                        top_k=TOP_K)
    assert isinstance(got, E.TokenTopLogprobs) and got.logprobs.shape == (sum(keep),) and got.top_token_ids.shape == (sum(keep), TOP_K)
    r0 = 0
    for b, n in enumerate(keep):
        for f in FIELDS:
            assert torch.equal(_bits(getattr(got, f)[r0:r0 + n]), _bits(getattr(solo[b], f)[0])), \
                f"[{tag}, T={temperature}] {f} of sequence {b} (prefix {prefixes[prefix_of[b]].shape[0]} + own {seqs[b].shape[0]}, keep {n}) differs from its solo run"
        ign = targets[b] == -100
        assert bool((got.logprobs[r0:r0 + n][ign] == 0).all()) and bool((got.token_ranks[r0:r0 + n][ign] == 0).all())
        r0 += n


def _check_contract(eng, hidden, vocab, plens, lens, prefix_of, keep, seed, tag, scale=1.0):
    """chunks of 256 rows, the default chunk, and the sequences (and prefixes) in another order, at two temperatures, against ONE set of solo runs"""
    prefixes, seqs = _embeds(plens, hidden, seed, scale=scale), _embeds(lens, hidden, seed + 1, scale=scale)
    targets = _targets(keep, vocab, seed + 2)
    cats = _cats(prefixes, seqs, prefix_of)
    order = list(reversed(range(len(lens))))
    order[0], order[-1] = order[-1], order[0]
    pick = lambda v: [v[i] for i in order]
    rev = list(reversed(range(len(plens))))                    # the prefixes in reverse order as well
    for temperature in (1.0, 0.7):
        solo = _solo(eng, cats, targets, keep, temperature)
        eng.set_score_chunk_rows(256)
        _check_prefixed(eng, prefixes, seqs, prefix_of, targets, keep, solo, temperature, f"{tag}, chunk 256")
        _check_prefixed(eng, [prefixes[u] for u in rev], pick(seqs), [rev.index(u) for u in pick(prefix_of)], pick(targets), pick(keep), pick(solo),
                        temperature, f"{tag}, chunk 256, other order")
        eng.set_score_chunk_rows(0)
        _check_prefixed(eng, prefixes, seqs, prefix_of, targets, keep, solo, temperature, f"{tag}, default chunk")
    # k = 0 is the call without lists: the TokenLogprobs type, the same bits
    plain = eng.forward_logprobs_prefixed(prefixes, seqs, prefix_of, torch.cat(targets), keep, temperature=0.7)
    assert isinstance(plain, E.TokenLogprobs) and plain.entropy is None and plain.argmax is None
    assert torch.equal(_bits(plain.logprobs), _bits(torch.cat([s.logprobs[0] for s in solo])))


# prefixes of 5, 64 and 257 rows: the first shared by three sequences, the second used once; T = 31, 255, 257 | 256 | 260, 515;
# keep = len + 1 (from the prefix's last row), 1, 2 | all own rows | len + 1, all own rows
TINY = dict(plens=[5, 64, 257], lens=[26, 250, 252, 192, 3, 258], prefix_of=[0, 0, 0, 1, 2, 2], keep=[27, 1, 2, 192, 4, 258])


@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_forward_logprobs_prefixed_tiny_models_bitwise(arch):
    cfg, eng = _tiny_engine(arch, max_batch=32, max_seq_len=640)
    T = [TINY["plens"][u] + n for u, n in zip(TINY["prefix_of"], TINY["lens"])]
    assert T == [31, 255, 257, 256, 260, 515]
    _check_contract(eng, cfg.hidden, cfg.vocab, seed=171, tag=f"tiny {arch}", **TINY)
    eng.close()


# the quantised weight formats: sv_forward_logprobs_ragged holds its own contract on them (the same helper of tests/test_gpu_ragged_scoring.py run
# on such engines), so the prefixed call supports them and is held to the same engine's solo runs
@pytest.mark.parametrize("weight_dtype", ["fp8_e4m3", "mxfp4"])
@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_forward_logprobs_prefixed_quantised_weights_bitwise(arch, weight_dtype):
    base = O.OracleConfig.tiny() if arch == "v1" else O.OracleConfig.tiny_v2()
    cfg = dataclasses.replace(base, n_positions=max(base.n_positions, 640), eos_token_id=-1)
    eng = build_engine(cfg, O.make_weights(cfg, seed=77), max_batch=32, max_seq_len=640, weight_dtype=weight_dtype)
    lens = _shuffled(LENS, 3)                                       # what admits the format: the ragged pass's own contract on this engine
    _ragged_contract(eng, cfg.hidden, cfg.vocab, lens, [KEEP_OF[n] for n in lens], 71, f"ragged, tiny {arch} {weight_dtype}")
    _check_contract(eng, cfg.hidden, cfg.vocab, seed=173, tag=f"tiny {arch} {weight_dtype}", **TINY)
    eng.close()


def _shapes_1b(ec):
    D, F, QKV = ec.hidden, ec.n_inner, ec.hidden + 2 * (ec.hidden // ec.n_head)
    return {"c_attn": (QKV, D, "none"), "c_proj": (D, D, "none"), "c_fc": (F, D, "gelu_tanh"), "down": (D, F, "none")}


@pytest.mark.parametrize("weight_dtype", ["bf16", "fp8_e4m3", "mxfp4"])
def test_forward_logprobs_prefixed_starvector_1b_dimensions(weight_dtype):
    ec = sva.EngineConfig(vit_layers=1, n_layer=2, max_batch=32, max_seq_len=640, weight_dtype=weight_dtype)      # (_fullsize_engine's, in any format)
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=4321)
    plens, lens = [255, 256, 250, 5, 257], [3, 1, 265, 510, 3]
    prefix_of, keep = [0, 1, 2, 3, 4], [4, 2, 265, 2, 1]
    # asserted from the host plan, not assumed: some projection sends 1 and 3 OWN rows of a sequence through the remainder kernel, no prefix row is listed
    plans = {name: E.prefix_plan(plens, lens, prefix_of, N, K, act) for name, (N, K, act) in _shapes_1b(ec).items()}
    MP, first = sum(plens), [sum(plens) + sum(lens[:b]) for b in range(len(lens))]
    per_seq = {n: [len([r for r in p["rows"] if first[b] <= r < first[b] + lens[b]]) for b in range(len(lens))] for n, p in plans.items()}
    assert any(1 in v for v in per_seq.values()) and any(3 in v for v in per_seq.values()), per_seq
    assert all(p["refused"] is None and all(r >= MP for r in p["rows"]) for p in plans.values()), plans
    assert eng.prefix_refused(plens, lens, prefix_of) == []
    _check_contract(eng, ec.hidden, ec.vocab, plens, lens, prefix_of, keep, 181, "1B dims", scale=0.5)
    # (257, 1) and (257, 2): T = 258 / 259 leave two / three remainder rows and own one / two
    for n in (1, 2):
        says = any(E.prefix_plan([257], [n], [0], N, K, act)["refused"] is not None for N, K, act in _shapes_1b(ec).values())
        assert (eng.prefix_refused([257], [n], [0]) == [0]) == says
        pre, seq = _embeds([257], ec.hidden, 191, scale=0.5), _embeds([n], ec.hidden, 192 + n, scale=0.5)
        tg = _targets([n + 1], ec.vocab, 195 + n)
        if says:
            with pytest.raises(ValueError, match=r"sequence 0 \(prefix 257 \+ own %d rows\).*reach into the shared prefix" % n):
                eng.forward_logprobs_prefixed(pre, seq, [0], tg[0], [n + 1])
        else:
            solo = _solo(eng, _cats(pre, seq, [0]), tg, [n + 1], 1.0)
            _check_prefixed(eng, pre, seq, [0], tg, [n + 1], solo, 1.0, f"1B dims (257, {n})")
    eng.close()


def test_forward_logprobs_prefixed_sliding_window():
    # window 24 inside the 100-row prefix (own 3), straddling its end (own 24 / 25: the first own row's window is all prefix), wholly in own rows
    # (own 70); the same own lengths behind a prefix shorter than the window
    cfg, eng = _tiny_engine("v2", max_batch=8, max_seq_len=256, window=24)
    _check_contract(eng, cfg.hidden, cfg.vocab, [100, 7], [3, 24, 25, 70, 3, 24, 25, 70], [0, 0, 0, 0, 1, 1, 1, 1], [4, 24, 1, 30, 2, 25, 25, 71], 191,
                    "tiny v2 window 24")
    eng.close()


# ---- engine state --------------------------------------------------------------------------------------------------------------------------
def test_no_page_is_written_decode_refuses_and_the_next_prompt_pass_is_a_fresh_engines():
    cfg, eng = _tiny_engine("v1", max_batch=8, max_seq_len=200)
    cfg2, fresh = _tiny_engine("v1", max_batch=8, max_seq_len=200)
    prompts = _embeds([70, 9, 64], cfg.hidden, 201)

    def prefill_and_steps(e):
        lg = e.prefill_ragged(prompts)
        out = [lg.clone()]
        for _ in range(3):
            lg = e.decode_step(lg.argmax(-1))
            out.append(lg.clone())
        return out

    prefill_and_steps(eng)                                             # a cache the scoring call must not let anybody continue
    free = eng.free_pages()
    pre, seqs = _embeds([65, 5], cfg.hidden, 202), _embeds([30, 3, 70], cfg.hidden, 203)
    eng.forward_logprobs_prefixed(pre, seqs, [0, 1, 0], torch.cat(_targets([1, 4, 2], cfg.vocab, 204)), [1, 4, 2])
    assert eng.free_pages() == free                                    # no page was assigned
    for B in (3, 2, 1):
        with pytest.raises(StarVectorHipError, match="sv_decode_step"):
            eng.decode_step(torch.zeros(B, dtype=torch.int32, device=dev()))
    for a, b in zip(prefill_and_steps(eng), prefill_and_steps(fresh)):
        assert torch.equal(a, b)
    eng.close()
    fresh.close()


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------------
def _mirror(eng):
    m = StarVectorForCausalLM.__new__(StarVectorForCausalLM)
    torch.nn.Module.__init__(m)
    object.__setattr__(m, "engine", eng)
    object.__setattr__(m, "model", types.SimpleNamespace(_get_embeddings=eng.embed_tokens))
    return m


def test_completion_logprobs_share_prefix_is_one_call_and_equals_the_unpadded_pass():
    cfg, eng = _tiny_engine("v1", max_batch=8, max_seq_len=200)
    m = _mirror(eng)
    P, G, Sv, L, K = 2, 3, 5, 60, 4
    B, S, n = P * G, Sv + L, 40
    ends = [65, 9, 64, 33, 26, 50]                                     # right padding: rows end behind, inside and before the scored window
    g = torch.Generator().manual_seed(211)
    vis = bf(torch.randn(P, Sv, cfg.hidden, generator=g))
    ids = torch.randint(0, cfg.vocab, (B, L), generator=g).to(dev())
    mask = torch.zeros(B, S, dtype=torch.long, device=dev())
    for b, e in enumerate(ends):
        mask[b, :e] = 1
    kw = dict(temperature=0.8, return_entropy=True, top_logprobs=K)
    want = m.completion_logprobs(vis, ids, G, mask, n, unpadded=True, **kw)

    calls = []
    real = eng.forward_logprobs_prefixed

    def spy(prefixes, seqs, *a, **k):
        calls.append(sum(int(x.shape[0]) for x in prefixes) + sum(int(x.shape[0]) for x in seqs))
        return real(prefixes, seqs, *a, **k)

    object.__setattr__(eng, "forward_logprobs_prefixed", spy)
    before = eng.prompt_passes()
    got = m.completion_logprobs(vis, ids, G, mask, n, share_prefix=True, **kw)
    assert eng.prompt_passes() - before == 1 and len(calls) == 1       # one engine call, one prompt pass
    assert calls[0] == P * Sv + sum(e - Sv for e in ends)              # the visual rows once per image + every row's stripped own rows
    assert sorted(got) == sorted(want) == ["entropies", "logprobs", "token_ranks", "top_logprobs", "top_token_ids"]
    for key in want:
        assert got[key].shape == want[key].shape and torch.equal(_bits(got[key]), _bits(want[key])), key
    assert float(got["logprobs"][0].abs().min()) > 0.0 and float(got["logprobs"][1].abs().max()) == 0.0
    eng.close()


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_forward_logprobs_prefixed_refusals():
    cfg, eng = _tiny_engine("v1", max_batch=4, max_seq_len=64)
    pre, seqs = _embeds([5, 7], cfg.hidden, 221), _embeds([9, 20, 12], cfg.hidden, 222)
    po, keep = [0, 1, 1], [3, 5, 13]
    tg = torch.randint(0, cfg.vocab, (sum(keep),), generator=torch.Generator().manual_seed(223), dtype=torch.int32).to(dev())
    ok = eng.forward_logprobs_prefixed(pre, seqs, po, tg, keep)
    call = lambda **kw: eng.forward_logprobs_prefixed(**{**dict(prefixes=pre, seqs=seqs, prefix_of=po, targets=tg, keep=keep), **kw})
    with pytest.raises(ValueError, match="keep"):
        call(keep=[3, 0, 13], targets=tg[:-5])
    with pytest.raises(ValueError, match="keep"):
        call(keep=[3, 5, 14], targets=torch.cat([tg, tg[:1]]))
    with pytest.raises(ValueError, match="targets"):
        call(targets=tg[:-1])
    with pytest.raises(ValueError, match="prefix_of"):
        call(prefix_of=[0, 2, 1])
    with pytest.raises(ValueError, match="prefix 0 is used by no sequence"):
        call(prefix_of=[1, 1, 1])
    with pytest.raises(ValueError, match="bad P=2 / B=1"):
        call(seqs=seqs[:1], prefix_of=[0], keep=[3], targets=tg[:3])
    with pytest.raises(ValueError, match="lengths"):
        call(seqs=[seqs[0], seqs[1][:0], seqs[2]])
    with pytest.raises(ValueError, match=r"length 65 of sequence 1 \(prefix 7 \+ own 58\) out of range \(1\.\.max_seq_len 64\)"):
        call(seqs=_embeds([9, 58, 12], cfg.hidden, 224))
    with pytest.raises(ValueError, match="max_batch 4"):
        call(seqs=_embeds([3] * 5, cfg.hidden, 225), prefix_of=[0, 1, 1, 1, 1], keep=[1] * 5, targets=tg[:5])
    with pytest.raises(ValueError, match="temperature"):
        call(temperature=0.0)
    with pytest.raises(ValueError, match="top_k"):
        call(top_k=33)
    bad = tg.clone()
    bad[3 + 5 + 7] = cfg.vocab                                         # sequence 2, kept position 7: packed row 15
    with pytest.raises(ValueError, match=r"target id outside \[0, %d\).*row 15 \(sequence 2, kept position 7\)" % cfg.vocab):
        call(targets=bad)
    # live continuous-batch slots: SV_ESTATE
    eng.cb_admit(_embeds([6], cfg.hidden, 226)[0][None].contiguous(), [dict(max_new_tokens=4)])
    with pytest.raises(StarVectorHipError, match="sv_forward_logprobs_prefixed: a continuous batch holds the KV cache"):
        call()
    eng.cb_reset()
    again = call()                                                     # a refused call leaves nothing behind
    assert torch.equal(_bits(again.logprobs), _bits(ok.logprobs))
    eng.close()
