"""CPU: the ragged scoring pass (sv_forward_logprobs_ragged) -- the argument checks of the entry point and of the gather operator through the
built library, which come before any device work; header and binding agree on the new symbols; and the packing / scatter logic of
``completion_logprobs(..., unpadded=True)`` over a fake engine that records its calls."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from starvector_amd import _lib
from starvector_amd.engine import TokenLogprobs, TokenTopLogprobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(64)                                                 # never dereferenced: the checks come first


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_new_symbols(lib):
    head, dbg = _header("starvector_hip.h"), _header("starvector_hip_debug.h")
    for name, table, text in (("sv_forward_logprobs_ragged", _lib.PRODUCT_PROTOTYPES, head),
                              ("sv_op_gather_tail_rows_ragged", _lib.DEBUG_PROTOTYPES, dbg)):
        assert hasattr(lib, name) and name in table
        decl = re.search(r"int\s+%s\((.*?)\);" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(table[name][1]), name
    # sv_forward_topk's arguments with (host_lens, host_keep) in the place of (S, n_keep)
    rag, rect = _lib.PRODUCT_PROTOTYPES["sv_forward_logprobs_ragged"][1], _lib.PRODUCT_PROTOTYPES["sv_forward_topk"][1]
    assert len(rag) == len(rect) and rag[3] == rag[4] == C.POINTER(C.c_int32) and rag[:3] == rect[:3] and rag[5:] == rect[5:]
    assert "#define SV_ABI_VERSION 9" in head and lib.sv_abi_version() == _lib.ABI_VERSION == 9      # entry points only
    assert "BIT-IDENTICAL to sv_forward_topk" in open(os.path.join(ROOT, "include", "starvector_hip.h")).read()


def _call(lib, embeds=P, B=3, lens=(9, 20, 12), keep=(3, 5, 12), targets=P, t=1.0, outs=(P, P, None, None), k=0, ids=P, lps=P, rank=P):
    arr = lambda v: (C.c_int32 * len(v))(*v) if v is not None else None
    rc = lib.sv_forward_logprobs_ragged(None, embeds, B, arr(lens), arr(keep), targets, t, outs[0], outs[1], outs[2], outs[3], k, ids, lps, rank,
                                        None)
    return rc, lib.sv_last_error().decode()


@pytest.mark.parametrize("case, kw, words", [
    ("embeds NULL", dict(embeds=None), ["null embeds"]),
    ("lens NULL", dict(lens=None), ["null", "lengths"]),
    ("keep NULL", dict(keep=None), ["null", "keep"]),
    ("targets NULL", dict(targets=None), ["null", "targets"]),
    ("B = 0", dict(B=0), ["bad B=0"]),
    ("B < 0", dict(B=-2), ["bad B=-2"]),
    ("length 0", dict(lens=(9, 0, 12)), ["length 0 of sequence 1"]),
    ("keep 0", dict(keep=(3, 0, 12)), ["keep 0 of sequence 1", "1..its length 20"]),
    ("keep < 0", dict(keep=(-1, 5, 12)), ["keep -1 of sequence 0"]),
    ("keep > length", dict(keep=(3, 5, 13)), ["keep 13 of sequence 2", "1..its length 12"]),
    ("temperature 0", dict(t=0.0), ["temperature"]),
    ("temperature nan", dict(t=float("nan")), ["temperature"]),
    ("temperature inf", dict(t=float("inf")), ["temperature"]),
    ("k < 0", dict(k=-1), ["k=-1", "0..32"]),
    ("k > 32", dict(k=33), ["k=33", "0..32"]),
    ("ids NULL", dict(k=4, ids=None), ["k=4", "dev_topk_ids"]),
    ("list log-probs NULL", dict(k=4, lps=None), ["k=4", "dev_topk_logprobs"]),
    ("no output", dict(outs=(None, None, None, None)), ["every output pointer is null"]),
])
def test_entry_point_refusals_come_before_any_device_work(lib, case, kw, words):
    rc, msg = _call(lib, **kw)
    assert rc == -22 and msg.startswith("sv_forward_logprobs_ragged:"), (case, msg)
    for w in words:
        assert w in msg, (case, msg)


def test_well_formed_calls_reach_the_engine_check(lib):
    for kw in (dict(), dict(k=5), dict(k=32, rank=None), dict(k=4, outs=(None, None, None, None)), dict(k=0, ids=None, lps=None, rank=None),
               dict(outs=(None, None, None, P)), dict(B=1, lens=(7,), keep=(7,)), dict(keep=(1, 1, 1)), dict(t=0.7)):
        rc, msg = _call(lib, **kw)
        assert rc == -22 and "null engine" in msg, (kw, msg)


def test_gather_operator_refusals(lib):
    def op(h=P, out=P, B=4, D=64, desc=P, total=9):
        return lib.sv_op_gather_tail_rows_ragged(h, out, B, D, desc, total, None), lib.sv_last_error().decode()

    for kw in (dict(h=None), dict(out=None), dict(desc=None), dict(B=0), dict(D=60), dict(D=0), dict(total=3), dict(total=0)):
        rc, msg = op(**kw)
        assert rc == -22 and "sv_op_gather_tail_rows_ragged" in msg, (kw, msg)
    assert lib.sv_op_gather_tail_rows(P, P, 2, 4, 5, 64, None) == -22          # the rectangular operator keeps its signature


# ---- completion_logprobs(..., unpadded=True) over a fake engine ------------------------------------------------------------------------------
class _Eng:
    """Both scoring calls scripted so that placement shows in every field: a kept row's "position value" is the embedding value of the row
    itself; log-prob = 100 * value + target (0 at -100), entropy = value, ids = target + slot, list log-probs = value + slot / 10, rank = value."""

    def __init__(self):
        self.calls = []

    def embed_tokens(self, ids):
        return ids.float().unsqueeze(-1).expand(-1, -1, 4).to(torch.bfloat16)

    @staticmethod
    def _result(pos, targets, entropy, k):
        lp = torch.where(targets == -100, torch.zeros_like(pos), 100.0 * pos + targets.float())
        if not k:
            return TokenLogprobs(lp, torch.zeros_like(lp), pos.clone() if entropy else None, None)
        slot = torch.arange(k)
        rank = torch.where(targets == -100, torch.zeros_like(targets), pos.to(torch.int32))
        return TokenTopLogprobs(lp, torch.zeros_like(lp), pos.clone() if entropy else None, None, (targets.unsqueeze(-1) + slot).to(torch.int32),
                                pos.unsqueeze(-1) + slot.float() / 10, rank)

    def forward_logprobs(self, emb, targets, keep, temperature=1.0, entropy=False, argmax=False, **kw):
        self.calls.append(dict(kw, name="rect", shape=tuple(emb.shape), keep=keep))
        return self._result(emb[:, -keep:, 0].float(), targets, entropy, kw.get("top_k", 0))

    def forward_logprobs_ragged(self, embeds, targets, keep, lengths=None, temperature=1.0, entropy=False, argmax=False, **kw):
        assert embeds.dtype == torch.bfloat16 and embeds.dim() == 2 and embeds.shape[0] == sum(lengths)
        assert targets.dtype == torch.int32 and tuple(targets.shape) == (sum(keep),) and all(1 <= k <= n for k, n in zip(keep, lengths))
        self.calls.append(dict(kw, name="ragged", lengths=list(lengths), keep=list(keep), targets=targets.tolist(), temperature=temperature,
                               rows=embeds[:, 0].float().tolist()))
        pos, first = [], 0
        for n, k in zip(lengths, keep):
            pos.append(embeds[first + n - k:first + n, 0].float())
            first += n
        return self._result(torch.cat(pos), targets, entropy, kw.get("top_k", 0))


class _OldEng:
    """an engine from before the ragged scoring pass"""

    def __init__(self):
        self.inner = _Eng()
        self.embed_tokens = self.inner.embed_tokens
        self.forward_logprobs = self.inner.forward_logprobs


def _model(eng=None):
    from starvector_amd.model import StarVectorForCausalLM
    m = StarVectorForCausalLM.__new__(StarVectorForCausalLM)
    torch.nn.Module.__init__(m)
    eng = eng or _Eng()
    object.__setattr__(m, "engine", eng)
    object.__setattr__(m, "model", types.SimpleNamespace(_get_embeddings=eng.embed_tokens))
    return m, eng


VIS = torch.full((1, 2, 4), 9.0, dtype=torch.bfloat16)             # 2 visual positions, value 9
IDS = torch.tensor([[11, 12, 13, 14, 15, 16], [21, 22, 23, 24, 25, 26], [31, 32, 33, 34, 35, 36]])      # S = 8, L = 6
N = 4                                                              # scored tokens: positions 4 .. 7 = ids[:, 2:]


def _solo(m, ids_row, n):
    """the row alone, without pads, through the rectangular call (the fake engine's numbers depend on a row's own values only)"""
    return m.completion_logprobs(VIS, ids_row, 1, None, n, return_entropy=True, top_logprobs=2)


def test_right_padding_packs_the_real_rows_and_scatters_the_scored_entries():
    m, eng = _model()
    # row 0 full; row 1 ends after position 5 (two scored tokens); row 2 ends after position 2: before the scored window
    mask = torch.tensor([[1] * 8, [1] * 6 + [0] * 2, [1] * 3 + [0] * 5])
    out = m.completion_logprobs(VIS, IDS, 3, mask, N, temperature=0.5, return_entropy=True, top_logprobs=2, unpadded=True)
    assert [c["name"] for c in eng.calls] == ["ragged"]
    call = eng.calls[0]
    assert call["lengths"] == [8, 6, 3] and call["keep"] == [5, 3, 1] and call["top_k"] == 2 and call["temperature"] == 0.5
    assert call["rows"] == [9, 9, 11, 12, 13, 14, 15, 16, 9, 9, 21, 22, 23, 24, 9, 9, 31]          # no pad row goes down
    assert call["targets"] == [13, 14, 15, 16, -100, 23, 24, -100, -100]                          # the last kept row of a sequence predicts nothing
    assert sorted(out) == ["entropies", "logprobs", "token_ranks", "top_logprobs", "top_token_ids"]
    # entry j scores ids[:, 2 + j] from the row of the position before it
    assert out["logprobs"].tolist() == [[1213, 1314, 1415, 1516], [2223, 2324, 0, 0], [0, 0, 0, 0]]
    assert out["entropies"].tolist() == [[12, 13, 14, 15], [22, 23, 0, 0], [0, 0, 0, 0]]
    assert out["token_ranks"].tolist() == [[12, 13, 14, 15], [22, 23, 0, 0], [0, 0, 0, 0]]
    assert out["top_token_ids"][1].tolist() == [[23, 24], [24, 25], [-1, -1], [-1, -1]] and out["top_token_ids"][2].tolist() == [[-1, -1]] * 4
    assert out["top_logprobs"][1, :, 1].tolist() == pytest.approx([22.1, 23.1, 0, 0]) and float(out["top_logprobs"][2].abs().max()) == 0
    # every row equals the row alone without its pads
    for b, (real, c) in enumerate([(6, 4), (4, 2)]):
        solo = _solo(m, IDS[b:b + 1, :real], c)
        for key in out:
            assert torch.equal(out[key][b, :c], solo[key][0]), (b, key)
    # the result forms without the lists
    lp = m.completion_logprobs(VIS, IDS, 3, mask, N, unpadded=True)
    assert isinstance(lp, torch.Tensor) and "top_k" not in eng.calls[-1] and lp.tolist() == out["logprobs"].tolist()
    lp2, ent2 = m.completion_logprobs(VIS, IDS, 3, mask, N, return_entropy=True, unpadded=True)
    assert lp2.tolist() == lp.tolist() and ent2.tolist() == out["entropies"].tolist()


def test_left_padding_and_both_sides_are_one_ragged_call():
    m, eng = _model()
    # row 0 full; row 1 left-padded by 3 (the pads cover the visual prefix and one id); row 2: 1 pad in front, 2 behind
    mask = torch.tensor([[1] * 8, [0] * 3 + [1] * 5, [0] + [1] * 5 + [0] * 2])
    out = m.completion_logprobs(VIS, IDS, 3, mask, N, return_entropy=True, top_logprobs=2, unpadded=True)
    assert [c["name"] for c in eng.calls] == ["ragged"]                # one call whatever the pad counts
    call = eng.calls[0]
    assert call["lengths"] == [8, 5, 5] and call["keep"] == [5, 5, 3]
    assert call["rows"] == [9, 9, 11, 12, 13, 14, 15, 16, 22, 23, 24, 25, 26, 9, 31, 32, 33, 34]
    assert call["targets"] == [13, 14, 15, 16, -100, 23, 24, 25, 26, -100, 33, 34, -100]
    assert out["logprobs"].tolist() == [[1213, 1314, 1415, 1516], [2223, 2324, 2425, 2526], [3233, 3334, 0, 0]]
    assert out["token_ranks"][2].tolist() == [32, 33, 0, 0] and out["top_token_ids"][2, 2:].tolist() == [[-1, -1]] * 2
    # the default over the same mask: today's code, one rectangular call per pad group, never the ragged method
    eng.calls.clear()
    old = m.completion_logprobs(VIS, IDS, 3, mask, N, return_entropy=True, top_logprobs=2)
    assert [c["name"] for c in eng.calls] == ["rect"] * 3 and sorted(c["shape"][:2] for c in eng.calls) == [(1, 5), (1, 7), (1, 8)]
    assert old["logprobs"].tolist() == out["logprobs"].tolist() and old["token_ranks"].tolist() == out["token_ranks"].tolist()


def test_no_pads_means_the_rectangular_call_and_the_default_never_calls_the_ragged_method():
    m, eng = _model()
    ref = m.completion_logprobs(VIS, IDS, 3, None, N, top_logprobs=2)
    for mask in (None, torch.ones(3, 8, dtype=torch.long)):
        out = m.completion_logprobs(VIS, IDS, 3, mask, N, top_logprobs=2, unpadded=True)
        assert all(torch.equal(out[k], ref[k]) for k in ref)
    right = torch.tensor([[1] * 8, [1] * 6 + [0] * 2, [1] * 3 + [0] * 5])
    left = torch.tensor([[1] * 8, [0] * 3 + [1] * 5, [0] + [1] * 7])
    for mask in (right, left):
        m.completion_logprobs(VIS, IDS, 3, mask, N)
        m.completion_logprobs(VIS, IDS, 3, mask, N, unpadded=False)
    assert all(c["name"] == "rect" for c in eng.calls) and len(eng.calls) == 3 + 2 * (1 + 3)


def test_holes_bad_masks_and_an_engine_without_the_method_raise():
    m, eng = _model()
    with pytest.raises(NotImplementedError, match="holes"):
        m.completion_logprobs(VIS, IDS, 3, torch.tensor([[1] * 8, [1, 1, 0, 1, 1, 1, 1, 1], [1] * 8]), N, unpadded=True)
    with pytest.raises(ValueError, match="left padding"):
        m.completion_logprobs(VIS, IDS, 3, torch.tensor([[1] * 8, [0] * 4 + [1] * 4, [1] * 8]), N, unpadded=True)
    with pytest.raises(ValueError, match="all zeros"):
        m.completion_logprobs(VIS, IDS, 3, torch.tensor([[1] * 8, [0] * 8, [1] * 8]), N, unpadded=True)
    with pytest.raises(ValueError, match="does not cover"):
        m.completion_logprobs(VIS, IDS, 3, torch.ones(3, 7, dtype=torch.long), N, unpadded=True)
    assert eng.calls == []
    m2, old = _model(_OldEng())
    mask = torch.tensor([[1] * 8, [1] * 6 + [0] * 2, [1] * 8])
    with pytest.raises(NotImplementedError, match="forward_logprobs_ragged"):
        m2.completion_logprobs(VIS, IDS, 3, mask, N, unpadded=True)
    assert old.inner.calls == []                                       # nothing was scored another way instead
    assert m2.completion_logprobs(VIS, IDS, 3, mask, N).shape == (3, N)      # the default works on it as before
    assert m2.completion_logprobs(VIS, IDS, 3, None, N, unpadded=True).shape == (3, N)
