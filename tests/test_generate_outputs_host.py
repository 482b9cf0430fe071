"""CPU: HF structured generate outputs (return_dict_in_generate / output_scores / output_logits) -- the C ABI surface of
sv_generate_ex, compute_transition_scores against transformers, and HipCausalLM.generate's argument checks on a fake engine."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from starvector_amd import _lib
from starvector_amd.model import HipCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "starvector_hip.h")).read(), flags=re.S)


def test_outputs_struct_matches_ctypes_mirror_and_symbol_is_exported():
    body = re.search(r"typedef struct sv_generate_outputs \{(.*?)\} sv_generate_outputs;", _header(), flags=re.S).group(1)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", d)[-1] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.SvGenerateOutputs._fields_]
    assert names == ["dev_scores", "dev_logits", "ld", "host_sequences_scores", "host_beam_indices"]
    assert C.sizeof(_lib.SvGenerateOutputs) == 40
    assert "sv_generate_ex" in _lib.PRODUCT_PROTOTYPES and len(_lib.PRODUCT_PROTOTYPES["sv_generate_ex"][1]) == 9
    assert _lib.ABI_VERSION == 9
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    assert hasattr(lib, "sv_generate_ex")
    # argument checks before any device work: a null engine is rejected
    n = C.c_int32(0)
    assert lib.sv_generate_ex(None, None, 1, 1, None, None, None, C.byref(n), None) != 0


class _Eng:
    def __init__(self, vocab):
        self.cfg = types.SimpleNamespace(vocab=vocab)
        self.calls = []
        self.free = 1 << 40

    def mem_free_bytes(self):
        return self.free

    def generate(self, inputs_embeds, max_length, **kw):
        B, S, _ = inputs_embeds.shape
        self.calls.append(kw)
        toks = torch.arange(B * (max_length - S)).view(B, -1) % self.cfg.vocab
        if kw.get("return_outputs"):
            for k in ("scores_out", "logits_out"):
                if kw.get(k) is not None:
                    kw[k].fill_(0.5)
            return {"sequences": toks, "n_generated": toks.shape[1]}
        return toks


def _lm(vocab=11):
    lm = HipCausalLM.__new__(HipCausalLM)
    torch.nn.Module.__init__(lm)
    object.__setattr__(lm, "_engine", _Eng(vocab))
    lm.eos_token_id, lm.pad_token_id, lm.seed = 0, 1, 0
    lm.batcher = None
    return lm


def test_return_dict_false_returns_the_tensor_and_ignores_output_scores():
    lm = _lm()
    emb = torch.zeros(2, 3, 4)
    a = lm.generate(inputs_embeds=emb, max_length=8)
    b = lm.generate(inputs_embeds=emb, max_length=8, output_scores=True, output_logits=True)
    assert isinstance(a, torch.Tensor) and torch.equal(a, b)
    assert all("scores_out" not in kw and "return_outputs" not in kw for kw in lm._engine.calls)


def test_return_dict_sequences_and_slabs():
    lm = _lm()
    emb = torch.zeros(2, 3, 4)
    out = lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True)
    assert torch.equal(out.sequences, out["sequences"]) and out.sequences.shape == (2, 5)
    assert out.scores is None and out.logits is None
    out = lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True, output_scores=True, output_logits=True)
    assert len(out.scores) == len(out.logits) == out.sequences.shape[1] == 5
    assert out.scores[0].shape == (2, 11) and out.scores[0].dtype == torch.float32
    kw = lm._engine.calls[-1]
    assert kw["scores_out"].shape == (5, 2, 11) and kw["logits_out"].shape == (5, 2, 11)


def test_not_built_cases_raise():
    lm = _lm()
    emb = torch.zeros(2, 4, 4)
    mask = torch.tensor([[0, 1, 1, 1], [1, 1, 1, 1]])
    with pytest.raises(NotImplementedError):
        lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=8, return_dict_in_generate=True, output_scores=True)
    with pytest.raises(NotImplementedError):
        lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=8, return_dict_in_generate=True, output_logits=True)
    with pytest.raises(NotImplementedError):
        lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True, output_attentions=True)
    with pytest.raises(NotImplementedError):
        lm.generate(inputs_embeds=emb, max_length=8, return_dict_in_generate=True, output_hidden_states=True)
    assert lm._engine.calls == []


def test_slab_size_is_checked_before_generating():
    lm = _lm(vocab=49156)
    lm._engine.free = 1 << 30
    emb = torch.zeros(32, 2, 4)
    with pytest.raises(MemoryError, match=r"6\.44 GB"):          # 32 rows x 1024 columns x 49156 fp32, one slab
        lm.generate(inputs_embeds=emb, max_length=2 + 1024, return_dict_in_generate=True, output_scores=True)
    with pytest.raises(MemoryError, match=r"12\.89 GB"):
        lm.generate(inputs_embeds=emb, max_length=2 + 1024, return_dict_in_generate=True, output_scores=True, output_logits=True)
    assert lm._engine.calls == []


def _hf_transition_scores(V, sequences, scores, beam_indices, normalize):
    tr = pytest.importorskip("transformers")
    from transformers.generation.utils import GenerationMixin
    fake = types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=V, get_text_config=lambda: types.SimpleNamespace(vocab_size=V)))
    del tr
    return GenerationMixin.compute_transition_scores(fake, sequences, scores, beam_indices, normalize_logits=normalize)


@pytest.mark.parametrize("normalize", [False, True])
def test_compute_transition_scores_greedy_matches_hf(normalize):
    V, B, L = 13, 3, 6
    g = torch.Generator().manual_seed(0)
    scores = tuple(torch.randn(B, V, generator=g) for _ in range(L))
    seqs = torch.randint(0, V, (B, L), generator=g)
    lm = _lm(V)
    got = lm.compute_transition_scores(seqs, scores, normalize_logits=normalize)
    ref = _hf_transition_scores(V, seqs, scores, None, normalize)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("normalize", [False, True])
def test_compute_transition_scores_beam_matches_hf(normalize):
    V, B, nb, L = 17, 2, 3, 5
    g = torch.Generator().manual_seed(1)
    scores = tuple(torch.randn(B * nb, V, generator=g).log_softmax(-1) for _ in range(L))
    seqs = torch.randint(0, V, (B, L), generator=g)
    bi = torch.tensor([[0, 1, 2, 1, 0], [3, 5, 4, -1, -1]])
    lm = _lm(V)
    got = lm.compute_transition_scores(seqs, scores, bi, normalize_logits=normalize)
    ref = _hf_transition_scores(V, seqs, scores, bi, normalize)
    assert torch.equal(got, ref)
    assert (got[1, 3:] == 0).all()
