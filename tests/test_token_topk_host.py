"""CPU: the top-k lists of the decode loop and the scoring pass (sv_generate_topk, sv_forward_topk) -- the C ABI surface and its argument
checks through the built library, which come before any device work, and the Python plumbing over fake engines: ``output_top_logprobs`` on
HipCausalLM.generate, ``return_top_logprobs`` on generate_im2svg_grpo, ``top_logprobs`` on completion_logprobs, HipEngine's own validation."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from starvector_amd import _lib
from starvector_amd.engine import TOPK_MAX, TokenLogprobs, TokenTopLogprobs, token_topk_request
from starvector_amd.model import HipCausalLM
from tests.test_token_stats_host import _build_model, _images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name="starvector_hip.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _err(lib):
    return lib.sv_last_error().decode()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_structs_and_constants_match_the_header(lib):
    head = _header()
    for name in ("sv_generate_topk", "sv_forward_topk"):
        assert hasattr(lib, name) and name in _lib.PRODUCT_PROTOTYPES
    for name in ("sv_op_token_topk", "sv_op_topk_rows_bf16"):
        assert hasattr(lib, name) and name in _lib.DEBUG_PROTOTYPES and name in _header("starvector_hip_debug.h")
    assert "#define SV_TOPK_MAX 32" in head and _lib.TOPK_MAX == TOPK_MAX == 32
    body = re.search(r"typedef struct sv_token_topk \{(.*?)\} sv_token_topk;", head, flags=re.S).group(1)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", d)[-1] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.SvTokenTopk._fields_] == ["k", "source", "dev_ids", "dev_logprobs", "dev_rank", "ld"]
    assert C.sizeof(_lib.SvTokenTopk) == 40 and _lib.SvTokenTopk.ld.offset == 32
    gen = _lib.PRODUCT_PROTOTYPES["sv_generate_topk"][1]
    assert len(gen) == len(_lib.PRODUCT_PROTOTYPES["sv_generate_stats"][1]) + 1
    assert gen[9]._type_ is _lib.SvTokenStats and gen[10]._type_ is _lib.SvTokenTopk
    assert len(_lib.PRODUCT_PROTOTYPES["sv_forward_topk"][1]) == len(_lib.PRODUCT_PROTOTYPES["sv_forward_logprobs"][1]) + 4
    assert lib.sv_abi_version() == _lib.ABI_VERSION                # entry points only: an old binding keeps working


def _gen(lib, tk, sp=None, lp=None, stats=None, B=2, S0=4):
    n = C.c_int32(0)
    p = C.c_void_p(64)                                             # never dereferenced: the checks come first
    sp = sp or _lib.SvSampling(max_length=S0 + 10, num_beams=1, temperature=1.0, top_p=1.0, eos_token_id=-1)
    return lib.sv_generate_topk(None, p, B, None, S0, 1, C.byref(sp), C.byref(lp) if lp is not None else None, None,
                                C.byref(stats) if stats is not None else None, C.byref(tk) if tk is not None else None, p, C.byref(n), None)


P = C.c_void_p(64)


@pytest.mark.parametrize("case, tk, words", [
    ("k = 0", dict(k=0), ["k=0", "1..32"]),
    ("k = 33", dict(k=33), ["k=33", "1..32"]),
    ("ids NULL", dict(dev_ids=None), ["dev_ids", "NULL"]),
    ("logprobs NULL", dict(dev_logprobs=None), ["dev_logprobs", "NULL"]),
    ("ld < max_new", dict(ld=9), ["ld 9", "max_new 10"]),
    ("source 2", dict(source=2), ["source=2"]),
    ("source -1", dict(source=-1), ["source=-1"]),
])
def test_generate_topk_refusals_come_before_any_device_work(lib, case, tk, words):
    req = dict(k=5, source=0, dev_ids=P, dev_logprobs=P, dev_rank=P, ld=10)
    req.update(tk)
    assert _gen(lib, _lib.SvTokenTopk(**req)) == -22, case
    for w in words:
        assert w in _err(lib), (case, _err(lib))


def test_generate_topk_refuses_beams_and_the_raw_rank_behind_a_rewrite(lib):
    ok = dict(k=5, source=0, dev_ids=P, dev_logprobs=P, dev_rank=P, ld=10)
    beams = _lib.SvSampling(max_length=14, num_beams=2, temperature=1.0, top_p=1.0)
    assert _gen(lib, _lib.SvTokenTopk(**ok), sp=beams) == -22 and "num_beams 2" in _err(lib)
    # the rank of the raw list behind a processor that rewrites the row: the message names the cause and both ways out
    ngram = _lib.SvLogitsProcessors(no_repeat_ngram_size=2)
    hold = _lib.SvSampling(max_length=14, num_beams=1, temperature=1.0, top_p=1.0, eos_token_id=3, min_new_tokens=2)
    words = _lib.SvLogitsProcessors(n_bad_words=1, bad_word_lens=(C.c_int32 * 1)(1), bad_word_ids=(C.c_int32 * 1)(7))
    for kw in (dict(lp=ngram), dict(sp=hold), dict(lp=words)):
        assert _gen(lib, _lib.SvTokenTopk(**ok), **kw) == -22
        msg = _err(lib)
        assert "dev_rank" in msg and "source 0" in msg and "rewrites the raw row" in msg and "source 1" in msg and "no dev_rank" in msg, msg
        # the two ways out pass the checks and reach the engine check (no engine here)
        assert _gen(lib, _lib.SvTokenTopk(**dict(ok, source=1)), **kw) == -22 and "null engine" in _err(lib)
        assert _gen(lib, _lib.SvTokenTopk(**dict(ok, dev_rank=None)), **kw) == -22 and "null engine" in _err(lib)
    # well-formed requests reach the engine check; topk = NULL is sv_generate_stats' path, checks included
    assert _gen(lib, _lib.SvTokenTopk(**ok)) == -22 and "null engine" in _err(lib)
    assert _gen(lib, _lib.SvTokenTopk(**dict(ok, k=32, source=1, dev_rank=None, ld=4096))) == -22 and "null engine" in _err(lib)
    assert _gen(lib, _lib.SvTokenTopk(**ok), stats=_lib.SvTokenStats(P, None, None, 10)) == -22 and "null engine" in _err(lib)
    assert _gen(lib, _lib.SvTokenTopk(**ok), stats=_lib.SvTokenStats(None, None, None, 10)) == -22 and "all NULL" in _err(lib)
    assert _gen(lib, _lib.SvTokenTopk(**ok), stats=_lib.SvTokenStats(P, None, None, 9)) == -22 and "stats ld 9" in _err(lib)
    assert _gen(lib, None, stats=_lib.SvTokenStats(None, None, None, 10)) == -22 and "sv_generate_stats" in _err(lib)
    assert _gen(lib, None) == -22 and "null engine" in _err(lib)


def test_forward_topk_and_the_operators_validate_before_any_device_work(lib):
    def fwd(k, ids=P, lps=P, outs=(P, P, None, None), t=1.0):
        return lib.sv_forward_topk(None, P, 1, 8, 4, P, t, outs[0], outs[1], outs[2], outs[3], k, ids, lps, P, None)

    assert fwd(-1) == -22 and "k=-1" in _err(lib) and "0..32" in _err(lib)
    assert fwd(33) == -22 and "k=33" in _err(lib)
    assert fwd(4, ids=None) == -22 and "dev_topk_ids" in _err(lib)
    assert fwd(4, lps=None) == -22 and "dev_topk_logprobs" in _err(lib)
    assert fwd(4, t=0.0) == -22 and "sv_forward_topk: temperature" in _err(lib)
    assert fwd(4) == -22 and "null engine" in _err(lib)
    assert fwd(4, outs=(None, None, None, None)) == -22 and "null engine" in _err(lib)      # the lists alone are a request
    assert fwd(0, outs=(None, None, None, None)) == -22 and "sv_forward_logprobs: every output pointer is null" in _err(lib)      # k = 0: that call
    assert fwd(0, ids=None, lps=None) == -22 and "null engine" in _err(lib)

    def op32(k=5, V=100, ld=100, ids=P, lps=P, t=1.0):
        return lib.sv_op_token_topk(P, 2, V, ld, t, None, k, ids, lps, None, None)

    assert op32(k=0) == -22 and "k=0" in _err(lib)
    assert op32(k=33) == -22 and "k=33" in _err(lib)
    assert op32(ids=None) == -22 and "dev_ids" in _err(lib)
    assert op32(ld=99) == -22 and "ld >= V" in _err(lib)
    assert op32(t=float("nan")) == -22 and "temperature" in _err(lib)

    def op16(k=5, V=100, ld=104, lse=P, ids=P, base=P):
        return lib.sv_op_topk_rows_bf16(base, 2, V, ld, None, 1.0, lse, k, ids, P, None, None)

    assert op16(k=0) == -22 and "k=0" in _err(lib)
    assert op16(k=40) == -22 and "k=40" in _err(lib)
    assert op16(lse=None) == -22 and "dev_logsumexp" in _err(lib)
    assert op16(ids=None) == -22 and "dev_topk_ids" in _err(lib)
    assert op16(ld=100) == -22 and "multiple of 8" in _err(lib)
    assert op16(base=C.c_void_p(68)) == -22 and "16-byte" in _err(lib)


# ---- HipEngine's own request parsing -------------------------------------------------------------------------------------------------------
def test_token_topk_request_parsing():
    assert token_topk_request(5) == (5, 0, True)
    assert token_topk_request(dict(k=32, source="processed", rank=False)) == (32, 1, False)
    assert token_topk_request(dict(k=1, source="raw")) == (1, 0, True)
    for bad in (0, 33, -1, True, 2.5, "5", dict(source="raw"), dict(k=5, sauce="raw"), dict(k=0), dict(k=5, source="scores"), dict(k=5, source=1)):
        with pytest.raises(ValueError, match="token_topk"):
            token_topk_request(bad)
    assert TokenLogprobs._fields == TokenTopLogprobs._fields[:4] == ("logprobs", "logsumexp", "entropy", "argmax")      # the old type keeps its four
    assert TokenTopLogprobs._fields[4:] == ("top_token_ids", "top_logprobs", "token_ranks")


# ---- HipCausalLM.generate on a fake engine -------------------------------------------------------------------------------------------------
class _Eng:
    """knows token_topk; the fake engines of the earlier host tests do not, and keep passing because the keyword only goes down when set"""

    def __init__(self, vocab):
        self.cfg = types.SimpleNamespace(vocab=vocab, max_batch=64)
        self.calls = []

    def mem_free_bytes(self):
        return 1 << 40

    def generate(self, inputs_embeds, max_length, n_samples=1, **kw):
        B, S, _ = inputs_embeds.shape
        B *= n_samples
        self.calls.append(dict(kw, n_samples=n_samples))
        toks = torch.arange(B * (max_length - S)).view(B, -1) % self.cfg.vocab
        if not (kw.get("return_outputs") or kw.get("token_stats") or kw.get("token_topk")):
            return toks
        res = {"sequences": toks, "n_generated": toks.shape[1]}
        if kw.get("token_stats"):
            for i, k in enumerate(("token_logprobs", "token_logprobs_processed", "token_entropies")):
                res[k] = torch.full(toks.shape, -1.0 - i)
        if kw.get("token_topk"):
            k, source, rank = token_topk_request(kw["token_topk"])
            res["top_token_ids"] = toks.unsqueeze(-1).expand(*toks.shape, k).to(torch.int32)
            res["top_logprobs"] = torch.full((*toks.shape, k), -0.5 - source)
            res["token_ranks"] = torch.ones(toks.shape, dtype=torch.int32)
        return res

    def generate_shared(self, inputs_embeds, max_length, n_samples, **kw):
        return self.generate(inputs_embeds, max_length, n_samples=n_samples, **kw)

    def generate_processed(self, inputs_embeds, max_length, n_samples=1, no_repeat_ngram_size=0, bad_words_ids=None, min_p=0.0, **kw):
        return self.generate(inputs_embeds, max_length, n_samples=n_samples, **kw)


def _lm(vocab=11):
    lm = HipCausalLM.__new__(HipCausalLM)
    torch.nn.Module.__init__(lm)
    object.__setattr__(lm, "_engine", _Eng(vocab))
    lm.eos_token_id, lm.pad_token_id, lm.seed = 0, 1, 0
    lm.batcher = None
    return lm


def test_output_top_logprobs_reaches_the_engine_only_when_set_and_adds_three_fields():
    lm = _lm()
    emb = torch.zeros(2, 3, 4)
    plain = lm.generate(inputs_embeds=emb, max_length=8)
    assert "token_topk" not in lm._engine.calls[-1]
    lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True, output_token_logprobs=True)
    assert "token_topk" not in lm._engine.calls[-1] and lm._engine.calls[-1]["token_stats"] is True
    for kw in (dict(), dict(do_sample=True, top_k=5, top_p=0.8, seed=3), dict(num_return_sequences=3, do_sample=True),
               dict(no_repeat_ngram_size=2), dict(output_scores=True), dict(output_token_logprobs=True)):
        for k, source in ((1, "raw"), (5, "processed"), (32, "raw")):
            out = lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True, output_top_logprobs=k, top_logprobs_source=source, **kw)
            call = lm._engine.calls[-1]
            rows = 2 * kw.get("num_return_sequences", 1)
            assert call["token_topk"] == dict(k=k, source=source) and call["return_outputs"] is True
            assert ("token_stats" in call) == bool(kw.get("output_token_logprobs"))
            assert out.sequences.shape == (rows, 5) and (rows != 2 or torch.equal(out.sequences, plain))
            assert out["top_token_ids"].shape == out["top_logprobs"].shape == (rows, 5, k) and out["token_ranks"].shape == (rows, 5)
            assert out.top_token_ids is out["top_token_ids"] and float(out.top_logprobs[0, 0, 0]) == (-0.5 if source == "raw" else -1.5)
            assert ("token_logprobs" in out.keys()) == bool(kw.get("output_token_logprobs"))
            assert (out.scores is not None) == bool(kw.get("output_scores"))
    without = lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True)
    assert "top_token_ids" not in without.keys() and "token_topk" not in lm._engine.calls[-1]


def test_output_top_logprobs_is_never_dropped():
    lm = _lm()
    emb = torch.zeros(2, 3, 4)
    kw = dict(inputs_embeds=emb, max_length=8, return_dict_in_generate=True, output_top_logprobs=5)
    with pytest.raises(NotImplementedError, match="output_top_logprobs with num_beams > 1"):
        lm.generate(num_beams=2, **kw)
    mask = torch.ones(2, 3, dtype=torch.long)
    mask[1, 0] = 0
    with pytest.raises(NotImplementedError, match="output_top_logprobs with a padded attention_mask"):
        lm.generate(attention_mask=mask, **kw)
    lm.batcher = object()
    with pytest.raises(NotImplementedError, match="output_top_logprobs with a batcher"):
        lm.generate(**kw)
    lm.batcher = None
    with pytest.raises(ValueError, match="return_dict_in_generate"):
        lm.generate(inputs_embeds=emb, max_length=8, output_top_logprobs=5)
    for k in (0, 33, -2, 2.0):
        with pytest.raises(ValueError, match="k must be an int in 1..32"):
            lm.generate(**dict(kw, output_top_logprobs=k))
    with pytest.raises(ValueError, match="source must be one of"):
        lm.generate(top_logprobs_source="logits", **kw)
    assert lm._engine.calls == []                                  # nothing reached the engine
    assert lm.generate(attention_mask=torch.ones(2, 3, dtype=torch.long), **kw)["token_ranks"].shape == (2, 5)


# ---- generate_im2svg_grpo and completion_logprobs ------------------------------------------------------------------------------------------
def test_grpo_return_top_logprobs_passes_through():
    def script(B, n, eos, pad, stop):
        return torch.full((B, n), 65, dtype=torch.long)

    model, eng = _build_model(script)
    real = eng.generate

    def generate(inputs_embeds, max_length, **kw):                # the scripted engine of the statistics tests, taught the new keyword
        tk = kw.pop("token_topk", None)
        res = real(inputs_embeds, max_length, **dict(kw, return_outputs=True))
        eng.calls[-1]["token_topk"] = tk
        k = token_topk_request(tk)[0]
        toks = res["sequences"]
        res.update(top_token_ids=toks.unsqueeze(-1).expand(*toks.shape, k).to(torch.int32), top_logprobs=torch.zeros(*toks.shape, k),
                   token_ranks=torch.ones(toks.shape, dtype=torch.int32))
        return res

    S0 = model.query_length + 4
    model.generate_im2svg_grpo({"image": _images(2)}, max_length=S0 + 6, num_beams=1)
    assert "token_topk" not in eng.calls[-1]                       # not asked for: the keyword does not go down
    eng.generate = generate
    res = model.generate_im2svg_grpo({"image": _images(2)}, max_length=S0 + 6, num_return_sequences=2, return_top_logprobs=4)
    assert list(res) == ["raw_svg", "outputs", "inputs_embeds", "completion_mask", "top_token_ids", "top_logprobs", "token_ranks"]
    assert eng.calls[-1]["token_topk"] == dict(k=4, source="raw") and "token_stats" not in eng.calls[-1]
    assert res["top_token_ids"].shape == res["top_logprobs"].shape == (4, 6, 4) and res["token_ranks"].shape == res["completion_mask"].shape == (4, 6)
    res = model.generate_im2svg_grpo({"image": _images(2)}, max_length=S0 + 6, num_beams=1, return_logprobs=True, return_top_logprobs=2,
                                     top_logprobs_source="processed")
    assert list(res) == ["raw_svg", "outputs", "inputs_embeds", "logprobs", "entropies", "completion_mask", "top_token_ids", "top_logprobs",
                         "token_ranks"]
    assert eng.calls[-1]["token_topk"] == dict(k=2, source="processed") and eng.calls[-1]["token_stats"] == ("token_logprobs", "token_entropies")
    with pytest.raises(NotImplementedError, match="output_top_logprobs with num_beams > 1"):
        model.generate_im2svg_grpo({"image": _images(2)}, max_length=S0 + 6, return_top_logprobs=4)      # the reference's default: 2 beams


class _ScoreEng:
    """forward_logprobs scripted as in the log-prob host tests, plus top_k: ids = target + slot, log-probs = position + slot / 10, rank = slot
    count of the row's position -- placement shows in every field."""

    def __init__(self):
        self.calls = []

    def embed_tokens(self, ids):
        return ids.float().unsqueeze(-1).expand(-1, -1, 4).to(torch.bfloat16)

    def forward_logprobs(self, emb, targets, keep, temperature=1.0, entropy=False, argmax=False, **kw):
        self.calls.append(dict(kw, shape=tuple(emb.shape), keep=keep))
        pos = emb[:, -keep:, 0].float()
        lp = torch.where(targets == -100, torch.zeros_like(pos), 100.0 * pos + targets.float())
        k = kw.get("top_k", 0)
        if not k:
            return TokenLogprobs(lp, torch.zeros_like(lp), pos.clone() if entropy else None, None)
        slot = torch.arange(k)
        ids = (targets.unsqueeze(-1) + slot).to(torch.int32)
        tlp = pos.unsqueeze(-1) + slot.float() / 10
        rank = torch.where(targets == -100, torch.zeros_like(targets), pos.to(torch.int32))
        return TokenTopLogprobs(lp, torch.zeros_like(lp), pos.clone() if entropy else None, None, ids, tlp, rank)


def test_completion_logprobs_top_logprobs_passes_through_and_follows_the_padding():
    from starvector_amd.model import StarVectorForCausalLM
    m = StarVectorForCausalLM.__new__(StarVectorForCausalLM)
    torch.nn.Module.__init__(m)
    eng = _ScoreEng()
    object.__setattr__(m, "engine", eng)
    object.__setattr__(m, "model", types.SimpleNamespace(_get_embeddings=eng.embed_tokens))
    vis = torch.full((1, 3, 4), 9.0, dtype=torch.bfloat16)
    ids = torch.tensor([[5, 6, 7, 8], [1, 2, 3, 4]])
    ref = m.completion_logprobs(vis, ids, 2, None, 3)
    assert isinstance(ref, torch.Tensor) and "top_k" not in eng.calls[-1]                 # not asked for: the keyword does not go down
    out = m.completion_logprobs(vis, ids, 2, None, 3, top_logprobs=2)
    assert eng.calls[-1]["top_k"] == 2 and eng.calls[-1]["keep"] == 4
    assert sorted(out) == ["logprobs", "token_ranks", "top_logprobs", "top_token_ids"] and torch.equal(out["logprobs"], ref)
    assert out["top_token_ids"].shape == out["top_logprobs"].shape == (2, 3, 2) and out["token_ranks"].shape == (2, 3)
    # entry j scores id j + 1 of the kept window from the row of the position before it: ids = the target (+ slot), values = that position
    assert out["top_token_ids"][0].tolist() == [[6, 7], [7, 8], [8, 9]] and out["token_ranks"].tolist() == [[5, 6, 7], [1, 2, 3]]
    assert out["top_logprobs"][1, :, 0].tolist() == [1.0, 2.0, 3.0]
    both = m.completion_logprobs(vis, ids, 2, None, 3, return_entropy=True, top_logprobs=2)
    assert sorted(both) == ["entropies", "logprobs", "token_ranks", "top_logprobs", "top_token_ids"] and both["entropies"].shape == (2, 3)
    # right padding: the rank of a pad is 0 (its target is -100); left padding: the row's own pass lands in the row
    right = m.completion_logprobs(vis, ids, 2, torch.tensor([[1] * 7, [1, 1, 1, 1, 1, 0, 0]]), 3, top_logprobs=2)
    assert right["token_ranks"].tolist() == [[5, 6, 7], [1, 0, 0]]
    eng.calls.clear()
    left = m.completion_logprobs(vis, ids, 2, torch.tensor([[1] * 7, [0, 0, 1, 1, 1, 1, 1]]), 3, top_logprobs=2)
    assert sorted(c["shape"][:2] for c in eng.calls) == [(1, 5), (1, 7)] and all(c["top_k"] == 2 for c in eng.calls)
    for name in out:
        assert torch.equal(left[name], out[name]), name
