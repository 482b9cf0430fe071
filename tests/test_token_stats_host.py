"""CPU: per-token statistics of the decode loop (sv_generate_stats) -- the C ABI surface and its argument checks, HipCausalLM.generate's
``output_token_logprobs`` refusals on a fake engine, and ``generate_im2svg_grpo(return_logprobs=True)`` over a scripted engine: the keys it
adds and the completion mask for rows that end at EOS, at the stop sequence and at the budget."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from starvector_amd import _lib
from starvector_amd.model import HipCausalLM, completion_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "starvector_hip.h")).read(), flags=re.S)


def _fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            out += [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", x)[-1] for x in decl.split(",")]
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_entry_point_is_exported_and_matches_the_header(lib):
    assert hasattr(lib, "sv_generate_stats")
    m = re.search(r"\bsv_generate_stats\s*\(([^;{}]*?)\)\s*;", _header(), flags=re.S)
    params = [p.strip() for p in m.group(1).split(",")]
    proto = _lib.PRODUCT_PROTOTYPES["sv_generate_stats"][1]
    assert len(params) == len(proto) == len(_lib.PRODUCT_PROTOTYPES["sv_generate_processed"][1]) + 1
    assert "sv_token_stats" in params[9] and "sv_generate_outputs" in params[8] and "sv_logits_processors" in params[7]
    assert proto[9]._type_ is _lib.SvTokenStats
    assert _fields("sv_token_stats") == [f[0] for f in _lib.SvTokenStats._fields_] == ["dev_logprob", "dev_logprob_processed", "dev_entropy", "ld"]
    assert C.sizeof(_lib.SvTokenStats) == 32


def test_abi_version_and_existing_structs_are_unchanged(lib):
    assert lib.sv_abi_version() == 9 == _lib.ABI_VERSION
    assert "#define SV_ABI_VERSION 9" in open(os.path.join(ROOT, "include", "starvector_hip.h")).read()
    assert _fields("sv_sampling") == [f[0] for f in _lib.SvSampling._fields_]
    assert _fields("sv_sampling")[-1] == "min_new_tokens" and C.sizeof(_lib.SvSampling) == 96
    assert _fields("sv_cb_request") == [f[0] for f in _lib.SvCbRequest._fields_]
    assert _fields("sv_cb_request")[-1] == "stop_any_ids" and C.sizeof(_lib.SvCbRequest) == 208
    assert _fields("sv_generate_outputs") == ["dev_scores", "dev_logits", "ld", "host_sequences_scores", "host_beam_indices"]
    assert C.sizeof(_lib.SvGenerateOutputs) == 40


def test_argument_checks_come_before_any_device_work(lib):
    """ld < max_new, all three pointers NULL and num_beams > 1 are SV_EINVAL with a message that names the cause -- with no engine at all."""
    def err():
        return lib.sv_last_error().decode()

    n = C.c_int32(0)
    p = C.c_void_p(64)                                         # never dereferenced: the checks come first
    sp = _lib.SvSampling(max_length=4 + 10, num_beams=1, temperature=1.0, top_p=1.0)

    def call(ts, sp=sp):
        return lib.sv_generate_stats(None, p, 2, None, 4, 1, C.byref(sp), None, None, C.byref(ts), p, C.byref(n), None)

    assert call(_lib.SvTokenStats(None, None, None, 10)) == -22 and "all NULL" in err()
    assert call(_lib.SvTokenStats(p, p, p, 9)) == -22 and "ld 9" in err() and "max_new 10" in err()
    beams = _lib.SvSampling(max_length=14, num_beams=2, temperature=1.0, top_p=1.0)
    assert call(_lib.SvTokenStats(p, p, p, 10), beams) == -22 and "num_beams 2" in err()
    assert lib.sv_generate_stats(None, p, 2, None, 4, 0, C.byref(sp), None, None, C.byref(_lib.SvTokenStats(p, p, p, 10)), p, C.byref(n),
                                 None) == -22 and "n_samples" in err()
    # a well-formed request reaches the engine check (no engine here), and stats = NULL is sv_generate_processed's path
    assert call(_lib.SvTokenStats(p, None, None, 10)) == -22 and "null engine" in err()
    assert lib.sv_generate_stats(None, p, 2, None, 4, 1, C.byref(sp), None, None, None, p, C.byref(n), None) == -22 and "null engine" in err()


# ---- HipCausalLM.generate on a fake engine ---------------------------------------------------------------------------------------------
class _Eng:
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
        if not (kw.get("return_outputs") or kw.get("token_stats")):
            return toks
        res = {"sequences": toks, "n_generated": toks.shape[1]}
        if kw.get("token_stats"):
            for i, k in enumerate(("token_logprobs", "token_logprobs_processed", "token_entropies")):
                res[k] = torch.full(toks.shape, -1.0 - i)
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


def test_output_token_logprobs_adds_three_fields_and_is_read_with_return_dict_only():
    lm = _lm()
    emb = torch.zeros(2, 3, 4)
    plain = lm.generate(inputs_embeds=emb, max_length=8, output_token_logprobs=True)          # like output_scores: ignored without the dict
    assert isinstance(plain, torch.Tensor) and "token_stats" not in lm._engine.calls[-1]
    for kw in (dict(), dict(do_sample=True, top_k=5, top_p=0.8, seed=3), dict(num_return_sequences=3, do_sample=True),
               dict(repetition_penalty=1.3, min_length=5), dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[4], [5, 6]]),
               dict(do_sample=True, min_p=0.1), dict(output_scores=True, output_logits=True)):
        out = lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True, output_token_logprobs=True, **kw)
        rows = 2 * kw.get("num_return_sequences", 1)
        assert lm._engine.calls[-1]["token_stats"] is True and lm._engine.calls[-1]["return_outputs"] is True
        assert out.sequences.shape == (rows, 5) and (rows != 2 or torch.equal(out.sequences, plain))
        for i, k in enumerate(("token_logprobs", "token_logprobs_processed", "token_entropies")):
            assert out[k].shape == (rows, 5) and float(out[k][0, 0]) == -1.0 - i and getattr(out, k) is out[k]
        assert (out.scores is not None) == bool(kw.get("output_scores")) and (out.logits is not None) == bool(kw.get("output_logits"))
    some = lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True, output_token_logprobs=("token_entropies",))
    assert lm._engine.calls[-1]["token_stats"] == ("token_entropies",)
    without = lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True)
    assert "token_logprobs" not in without.keys() and "token_stats" not in lm._engine.calls[-1]


def test_output_token_logprobs_refusals_name_the_combination():
    lm = _lm()
    emb = torch.zeros(2, 3, 4)
    kw = dict(inputs_embeds=emb, max_length=8, return_dict_in_generate=True, output_token_logprobs=True)
    with pytest.raises(NotImplementedError, match="output_token_logprobs with num_beams > 1"):
        lm.generate(num_beams=2, **kw)
    mask = torch.ones(2, 3, dtype=torch.long)
    mask[1, 0] = 0
    with pytest.raises(NotImplementedError, match="output_token_logprobs with a padded attention_mask"):
        lm.generate(attention_mask=mask, **kw)
    lm.batcher = object()
    with pytest.raises(NotImplementedError, match="output_token_logprobs with a batcher"):
        lm.generate(**kw)
    lm.batcher = None
    assert lm._engine.calls == []                                 # nothing reached the engine
    assert lm.generate(attention_mask=torch.ones(2, 3, dtype=torch.long), **kw)["token_entropies"].shape == (2, 5)


# ---- generate_im2svg_grpo over a scripted engine ---------------------------------------------------------------------------------------
def _build_model(script):
    """The real mirror classes over an engine whose 'decoder' returns the rows of `script(B, budget, eos, pad)`."""
    from starvector_amd.engine import EngineConfig
    from starvector_amd.model import ByteTokenizer, StarVectorConfig, StarVectorStarCoder

    tok = ByteTokenizer(49152)

    class Engine:
        device = 0

        def __init__(self):
            self.cfg = EngineConfig(image_size=28, patch_size=14, vit_width=4, hidden=8, vocab=len(tok))
            self.calls = []

        def encode_image(self, image):
            return image.float().mean(dim=(1, 2, 3)).view(-1, 1, 1).expand(-1, self.cfg.query_length, 4).to(torch.bfloat16)

        def adapter(self, h):
            return torch.cat([h, h], dim=-1)

        def embed_tokens(self, ids):
            return (ids.float().unsqueeze(-1) / 300.0).expand(-1, -1, 8).to(torch.bfloat16)

        def generate(self, inputs_embeds, max_length, n_samples=1, eos_token_id=0, pad_token_id=0, stop_ids=None, **kw):
            B, S, _ = inputs_embeds.shape
            self.calls.append(dict(kw, n_samples=n_samples))
            toks = script(B * n_samples, max_length - S, eos_token_id, pad_token_id, list(stop_ids or []))
            if not (kw.get("return_outputs") or kw.get("token_stats")):
                return toks
            res = {"sequences": toks, "n_generated": toks.shape[1]}
            if kw.get("token_stats"):
                base = -(torch.arange(toks.numel(), dtype=torch.float32).view(toks.shape) + 1) / 64
                full = dict(token_logprobs=base, token_logprobs_processed=base / 2, token_entropies=-base)
                res.update(full if kw["token_stats"] is True else {k: full[k] for k in kw["token_stats"]})
            return res

        def generate_shared(self, inputs_embeds, max_length, n_samples, **kw):
            return self.generate(inputs_embeds, max_length, n_samples=n_samples, **kw)

    engine = Engine()
    return StarVectorStarCoder(StarVectorConfig(), engine, tok), engine


def _images(n):
    return torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 3, 28, 28).contiguous()


def test_grpo_dict_is_the_references_three_keys_without_the_flag():
    model, eng = _build_model(lambda B, n, eos, pad, stop: torch.full((B, n), 65, dtype=torch.long))
    S0 = model.query_length + 4
    for kw in (dict(num_beams=1), dict(num_return_sequences=2), dict(num_beams=1, return_logprobs=False)):
        res = model.generate_im2svg_grpo({"image": _images(2)}, max_length=S0 + 6, **kw)
        assert list(res) == ["raw_svg", "outputs", "inputs_embeds"]
        assert "token_stats" not in eng.calls[-1] and "return_outputs" not in eng.calls[-1]
    with pytest.raises(NotImplementedError, match="output_token_logprobs with num_beams > 1"):
        model.generate_im2svg_grpo({"image": _images(2)}, max_length=S0 + 6, return_logprobs=True)      # the reference's default: 2 beams


def test_grpo_completion_mask_for_eos_stop_sequence_and_budget():
    ends = {}

    def script(B, n, eos, pad, stop):
        ends.update(eos=eos, pad=pad, stop=stop)
        L = ends["cols"]
        toks = torch.full((B, L), 65, dtype=torch.long)
        toks[1, 2] = eos                                          # row 1: its own EOS at column 2, pads behind it
        toks[1, 3:] = pad
        if ends["fire"]:                                          # row 0 ends with the stop sequence: the call ends there, for every row
            toks[0, L - len(stop):] = torch.tensor(stop)
        toks[3, L - 1] = eos                                      # row 3: EOS in the very last column
        return toks

    model, eng = _build_model(script)
    S0 = model.query_length + 4
    for fire, cols in ((True, 7), (False, 9)):                    # the stop sequence at column 6 of a budget of 9 | every column of the budget
        ends.update(fire=fire, cols=cols)
        res = model.generate_im2svg_grpo({"image": _images(2)}, max_length=S0 + 9, num_return_sequences=2, return_logprobs=True)
        assert list(res) == ["raw_svg", "outputs", "inputs_embeds", "logprobs", "entropies", "completion_mask"]
        assert eng.calls[-1]["token_stats"] == ("token_logprobs", "token_entropies")      # the processed log-prob is not asked for: it costs the most
        assert eng.calls[-1]["n_samples"] == 2
        assert len(ends["stop"]) >= 1 and ends["eos"] != 65
        new = res["outputs"][:, 4:]
        assert new.shape == (4, cols) and res["logprobs"].shape == res["entropies"].shape == res["completion_mask"].shape == (4, cols)
        want = torch.ones(4, cols, dtype=torch.int64)
        want[1, 3:] = 0                                           # EOS at column 2: three columns count, the pads do not
        assert torch.equal(res["completion_mask"], want)          # rows 0, 2 (stop sequence / budget) and 3 (EOS in the last column): all
        assert res["completion_mask"].sum(1).tolist() == [cols, 3, cols, cols]
        assert float(res["logprobs"][0, 0]) == -1 / 64 and float(res["entropies"][0, 0]) == 1 / 64


def test_completion_mask_counts_the_first_eos_only():
    toks = torch.tensor([[5, 0, 0, 0], [5, 6, 7, 8], [0, 1, 1, 1], [5, 6, 7, 0]])
    assert completion_mask(toks, 0).tolist() == [[1, 1, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 1, 1]]
