"""CPU: the shared-prefix scoring pass (sv_forward_logprobs_prefixed) -- the symbol and its prototype in the built library, the argument
checks that come before any device work, the host plan (sv_debug_prefix_plan) on hand-computed cases, and the packing / scatter logic of
``completion_logprobs(..., share_prefix=True)`` over a fake engine that records its calls."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from starvector_amd import _lib
from starvector_amd import engine as E
from starvector_amd.engine import TokenLogprobs, TokenTopLogprobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = C.c_void_p(64)                                               # never dereferenced: the checks come first
# StarVector-1B's decoder projections (N, K, act)
C_ATTN, C_PROJ, C_FC, DOWN = (2048 + 2 * 128, 2048, "none"), (2048, 2048, "none"), (8192, 2048, "gelu_tanh"), (2048, 8192, "none")


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
    for name, table, text in (("sv_forward_logprobs_prefixed", _lib.PRODUCT_PROTOTYPES, head), ("sv_debug_prefix_plan", _lib.DEBUG_PROTOTYPES, dbg),
                              ("sv_op_attn_prefill_prefixed", _lib.DEBUG_PROTOTYPES, dbg)):
        assert hasattr(lib, name) and name in table
        decl = re.search(r"int\s+%s\((.*?)\);" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(table[name][1]), name
    # sv_forward_logprobs_ragged's arguments with (prefixes, P, prefix lengths) in front of the embeddings and prefix_of in front of keep
    pre, rag = _lib.PRODUCT_PROTOTYPES["sv_forward_logprobs_prefixed"][1], _lib.PRODUCT_PROTOTYPES["sv_forward_logprobs_ragged"][1]
    assert len(pre) == len(rag) + 4 and pre[:1] + pre[4:7] + pre[8:] == rag
    assert lib.sv_abi_version() == _lib.ABI_VERSION                   # entry points only: an old binding keeps working
    text = open(os.path.join(ROOT, "include", "starvector_hip.h")).read()
    assert "SHARE PREFIXES" in text and "Refusal rule" in text and "Weight formats" in text


def _call(lib, prefixes=PTR, P=2, plens=(5, 7), embeds=PTR, B=3, lens=(9, 20, 12), prefix_of=(0, 1, 1), keep=(3, 5, 13), targets=PTR, t=1.0,
          outs=(PTR, PTR, None, None), k=0, ids=PTR, lps=PTR, rank=PTR):
    arr = lambda v: (C.c_int32 * len(v))(*v) if v is not None else None
    rc = lib.sv_forward_logprobs_prefixed(None, prefixes, P, arr(plens), embeds, B, arr(lens), arr(prefix_of), arr(keep), targets, t, outs[0],
                                          outs[1], outs[2], outs[3], k, ids, lps, rank, None)
    return rc, lib.sv_last_error().decode()


@pytest.mark.parametrize("case, kw, words", [
    ("prefixes NULL", dict(prefixes=None), ["null prefixes"]),
    ("prefix lengths NULL", dict(plens=None), ["null"]),
    ("embeds NULL", dict(embeds=None), ["null", "embeds"]),
    ("lens NULL", dict(lens=None), ["null", "lengths"]),
    ("prefix_of NULL", dict(prefix_of=None), ["null", "prefix_of"]),
    ("keep NULL", dict(keep=None), ["null", "keep"]),
    ("targets NULL", dict(targets=None), ["null", "targets"]),
    ("P = 0", dict(P=0), ["bad P=0"]),
    ("P > B", dict(P=2, B=1), ["bad P=2 / B=1"]),
    ("B < 0", dict(B=-2), ["B=-2"]),
    ("prefix length 0", dict(plens=(5, 0)), ["length 0 of prefix 1"]),
    ("length 0", dict(lens=(9, 0, 12)), ["length 0 of sequence 1"]),
    ("prefix_of < 0", dict(prefix_of=(0, -1, 1)), ["prefix_of -1 of sequence 1", "0..1"]),
    ("prefix_of = P", dict(prefix_of=(0, 2, 1)), ["prefix_of 2 of sequence 1", "0..1"]),
    ("prefix unused", dict(prefix_of=(1, 1, 1), keep=(3, 5, 12)), ["prefix 0 is used by no sequence"]),
    ("keep 0", dict(keep=(3, 0, 12)), ["keep 0 of sequence 1", "length + 1 (21)"]),
    ("keep > length + 1", dict(keep=(3, 5, 14)), ["keep 14 of sequence 2", "length + 1 (13)"]),
    ("temperature 0", dict(t=0.0), ["temperature"]),
    ("temperature nan", dict(t=float("nan")), ["temperature"]),
    ("k < 0", dict(k=-1), ["k=-1", "0..32"]),
    ("k > 32", dict(k=33), ["k=33", "0..32"]),
    ("ids NULL", dict(k=4, ids=None), ["k=4", "dev_topk_ids"]),
    ("list log-probs NULL", dict(k=4, lps=None), ["k=4", "dev_topk_logprobs"]),
    ("no output", dict(outs=(None, None, None, None)), ["every output pointer is null"]),
])
def test_entry_point_refusals_come_before_any_device_work(lib, case, kw, words):
    rc, msg = _call(lib, **kw)
    assert rc == -22 and msg.startswith("sv_forward_logprobs_prefixed:"), (case, msg)
    for w in words:
        assert w in msg, (case, msg)


def test_well_formed_calls_reach_the_engine_check(lib):
    for kw in (dict(), dict(k=5), dict(k=32, rank=None), dict(k=4, outs=(None, None, None, None)), dict(keep=(10, 21, 1)), dict(t=0.7),
               dict(P=1, plens=(257,), B=1, lens=(1,), prefix_of=(0,), keep=(2,))):          # (the remainder rule needs the engine's projections)
        rc, msg = _call(lib, **kw)
        assert rc == -22 and "null engine" in msg, (kw, msg)


def test_operator_and_plan_refusals(lib):
    arr = lambda *v: (C.c_int32 * len(v))(*v)
    op = lambda **kw: _op(lib, **kw)

    def _op(lib, qkv=PTR, out=PTR, stride=512, H=2, Hkv=1, dh=128, P=1, plens=(5,), B=2, lens=(3, 4), po=(0, 0), scale=0.1, window=0, q_off=0):
        return lib.sv_op_attn_prefill_prefixed(qkv, q_off, 256, 384, stride, out, P, arr(*plens), B, arr(*lens), arr(*po), H, Hkv, dh, scale, window, None), \
            lib.sv_last_error().decode()

    for kw in (dict(qkv=None), dict(out=None), dict(H=3, Hkv=2), dict(dh=96), dict(stride=380), dict(q_off=4), dict(stride=448), dict(scale=0.0),
               dict(window=-1), dict(P=0), dict(lens=(3, 0)), dict(po=(0, 1)), dict(P=2, plens=(5, 6), po=(0, 0))):
        rc, msg = op(**kw)
        assert rc == -22 and msg.startswith("sv_op_attn_prefill_prefixed:"), (kw, msg)
    buf, out4 = (C.c_int32 * 64)(), (C.c_int32 * 4)()
    plan = lambda *a: (lib.sv_debug_prefix_plan(*a), lib.sv_last_error().decode())
    assert plan(None, 1, arr(3), arr(0), 1, 64, 64, 0, 32, buf, buf, buf, 64, out4)[0] == -22
    assert "q_tile" in plan(arr(5), 1, arr(3), arr(0), 1, 64, 64, 0, 64, buf, buf, buf, 64, out4)[1]
    assert "capacity" in plan(arr(50), 1, arr(30), arr(0), 1, 64, 64, 0, 32, buf, buf, buf, 64, out4)[1]
    assert "used by no sequence" in plan(arr(5, 6), 2, arr(3, 3), arr(1, 1), 2, 64, 64, 0, 32, buf, buf, buf, 64, out4)[1]
    assert plan(arr(5), 1, arr(3), arr(0), 1, 64, 64, 0, 32, buf, buf, buf, 64, out4)[0] == 0 and list(out4) == [0, 1, -1, 8]


# ---- the host plan -----------------------------------------------------------------------------------------------------------------------
def test_plan_positions_are_solo_indices_and_blocks_start_at_the_straddling_tile():
    # packed: prefix 0 (5 rows) | prefix 1 (70 rows) | b0 own 3 of prefix 0 | b1 own 40 of prefix 1 | b2 own 60 of prefix 0 | b3 own 1 of prefix 1
    p = E.prefix_plan([5, 70], [3, 40, 60, 1], [0, 1, 0, 1], *C_PROJ)
    assert p["row_pos"] == list(range(5)) + list(range(70)) + [5, 6, 7] + list(range(70, 110)) + list(range(5, 65)) + [70]
    # tiles of 32 rows from solo index 0: b0 (T 8) tile 0; b1 (Pl 70, T 110) tiles 2..3 -- tile 2 = rows 64..95 straddles the prefix's end;
    # b2 (Pl 5, T 65) tiles 0..2; b3 (Pl 70, T 71) tile 2
    assert p["blocks"] == [(0, 0), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (3, 2)]
    assert p["rows"] == [] and p["refused"] is None
    # one head per block: tiles of 128 rows
    assert E.prefix_plan([130], [1, 127, 200], [0, 0, 0], *C_PROJ, q_tile=128)["blocks"] == [(0, 1), (1, 1), (1, 2), (2, 1), (2, 2)]
    # a prefix that ends on a tile boundary: the first listed tile is the first one of own rows alone
    assert E.prefix_plan([64], [1, 33], [0, 0], *C_PROJ)["blocks"] == [(0, 2), (1, 2), (1, 3)]


def test_plan_lists_remainder_rows_among_own_rows_only_and_never_a_prefix_by_its_own_length():
    assert all(E.gemm_seq_form(T, *DOWN) for T in (257, 258, 259, 515)) and not E.gemm_seq_form(260, *DOWN)       # what the cases below stand on
    assert not any(E.gemm_seq_form(T, *C_ATTN) for T in (257, 258, 259, 515))
    # prefixes of 5 and 257 rows = packed rows 0..4, 5..261; own rows from 262: b0 3 rows (T 8), b1 3 rows (T 260: no remainder), b2 254 rows
    # (T 259: its last 3 rows), b3 258 rows (T 515: its last 3 rows), b4 1 row of the 5-row prefix
    p = E.prefix_plan([5, 257], [3, 3, 254, 258, 1], [0, 1, 0, 1, 0], *DOWN)
    assert p["rows"] == [268 + 251, 268 + 252, 268 + 253, 522 + 255, 522 + 256, 522 + 257] and p["refused"] is None
    assert min(p["rows"]) >= 262, "a prefix row is listed"            # the 257-row prefix has a peel row as a sequence of its own: not here
    assert 5 + 256 not in p["rows"] and E.ragged_plan([5, 257], *DOWN)["rows"] == [5 + 256]
    assert E.prefix_plan([5, 257], [3, 3, 254, 258, 1], [0, 1, 0, 1, 0], *C_ATTN)["rows"] == []      # a projection without the form lists nothing
    # the listed rows are the solo run's: the same solo indices ragged_plan lists for the concatenations
    for pl, ln in ((255, 3), (256, 1), (250, 265), (5, 510), (257, 3), (1, 256)):
        got = E.prefix_plan([pl], [ln], [0], *DOWN)
        solo = E.ragged_plan([pl + ln], *DOWN)["rows"]
        assert got["refused"] is None and [got["row_pos"][r] for r in got["rows"]] == solo and all(r >= pl for r in got["rows"]), (pl, ln)
    assert len(E.prefix_plan([256], [1], [0], *DOWN)["rows"]) == 1 and len(E.prefix_plan([250], [265], [0], *DOWN)["rows"]) == 3


def test_plan_refuses_a_sequence_whose_remainder_rows_reach_into_its_prefix():
    # T = 258: two remainder rows, one own row; T = 259: three, two own rows
    assert E.prefix_plan([257], [1], [0], *DOWN)["refused"] == 0 and E.prefix_plan([257], [2], [0], *DOWN)["refused"] == 0
    assert E.prefix_plan([257], [3], [0], *DOWN)["refused"] is None          # T = 260
    assert E.prefix_plan([256], [1], [0], *DOWN)["refused"] is None          # T = 257: the one remainder row is the own row
    assert E.prefix_plan([257], [1], [0], *C_ATTN)["refused"] is None        # the projection does not take the form: nothing to refuse
    # the FIRST such sequence is named; the others are planned as usual
    p = E.prefix_plan([5, 257], [3, 2, 1, 254], [0, 1, 1, 0], *DOWN)
    assert p["refused"] == 1 and p["rows"] == [519, 520, 521]
    assert E.prefix_plan([512], [2, 3], [0, 0], *DOWN)["refused"] is None and E.prefix_plan([513], [1, 2], [0, 0], *DOWN)["refused"] == 0


# ---- completion_logprobs(..., share_prefix=True) over a fake engine --------------------------------------------------------------------------
class _Eng:
    """The scoring calls scripted so that placement shows in every field (as tests/test_ragged_scoring_host.py does): a kept row's value is the
    embedding value of the row itself; log-prob = 100 * value + target (0 at -100), entropy = value, ids = target + slot, rank = value."""

    def __init__(self, refused=()):
        self.calls, self.refused = [], set(refused)

    def embed_tokens(self, ids):
        return ids.float().unsqueeze(-1).expand(-1, -1, 4).to(torch.bfloat16)

    def prefix_refused(self, prefix_lengths, lengths, prefix_of):
        return [b for b in range(len(lengths)) if b in self.refused]

    @staticmethod
    def _result(pos, targets, entropy, k):
        lp = torch.where(targets == -100, torch.zeros_like(pos), 100.0 * pos + targets.float())
        if not k:
            return TokenLogprobs(lp, torch.zeros_like(lp), pos.clone() if entropy else None, None)
        slot = torch.arange(k)
        rank = torch.where(targets == -100, torch.zeros_like(targets), pos.to(torch.int32))
        return TokenTopLogprobs(lp, torch.zeros_like(lp), pos.clone() if entropy else None, None, (targets.unsqueeze(-1) + slot).to(torch.int32),
                                pos.unsqueeze(-1) + slot.float() / 10, rank)

    def forward_logprobs_ragged(self, embeds, targets, keep, lengths=None, temperature=1.0, entropy=False, argmax=False, **kw):
        self.calls.append(dict(kw, name="ragged", lengths=[int(x.shape[0]) for x in embeds], keep=list(keep), targets=targets.tolist()))
        pos = torch.cat([x[x.shape[0] - n:, 0].float() for x, n in zip(embeds, keep)])
        return self._result(pos, targets, entropy, kw.get("top_k", 0))

    def forward_logprobs_prefixed(self, prefixes, seqs, prefix_of, targets, keep, temperature=1.0, entropy=False, argmax=False, **kw):
        assert all(x.dtype == torch.bfloat16 and x.dim() == 2 for x in list(prefixes) + list(seqs)) and targets.dtype == torch.int32
        assert sorted(set(prefix_of)) == list(range(len(prefixes))) and all(1 <= k <= x.shape[0] + 1 for k, x in zip(keep, seqs))
        self.calls.append(dict(kw, name="prefixed", prefix_rows=[x[:, 0].float().tolist() for x in prefixes], prefix_of=list(prefix_of),
                               rows=[x[:, 0].float().tolist() for x in seqs], keep=list(keep), targets=targets.tolist(), temperature=temperature))
        cat = [torch.cat([prefixes[u], x]) for u, x in zip(prefix_of, seqs)]
        pos = torch.cat([x[x.shape[0] - n:, 0].float() for x, n in zip(cat, keep)])
        return self._result(pos, targets, entropy, kw.get("top_k", 0))


def _model(eng):
    from starvector_amd.model import StarVectorForCausalLM
    m = StarVectorForCausalLM.__new__(StarVectorForCausalLM)
    torch.nn.Module.__init__(m)
    object.__setattr__(m, "engine", eng)
    object.__setattr__(m, "model", types.SimpleNamespace(_get_embeddings=eng.embed_tokens))
    return m


VIS = torch.stack([torch.full((2, 4), 8.0), torch.full((2, 4), 9.0)]).to(torch.bfloat16)      # P = 2 images, 2 visual positions each
IDS = torch.tensor([[11, 12, 13, 14], [21, 22, 23, 24], [31, 32, 33, 34], [41, 42, 43, 44]])  # G = 2: rows 0, 2 -> image 0; rows 1, 3 -> image 1
MASK = torch.tensor([[1] * 6, [1] * 4 + [0] * 2, [1] * 6, [1] * 3 + [0] * 3])


def test_share_prefix_is_one_prefixed_call_over_the_stripped_rows():
    eng = _Eng()
    m = _model(eng)
    out = m.completion_logprobs(VIS, IDS, 2, MASK, 4, temperature=0.5, return_entropy=True, top_logprobs=2, share_prefix=True)
    assert [c["name"] for c in eng.calls] == ["prefixed"]
    call = eng.calls[0]
    assert call["prefix_rows"] == [[8, 8], [9, 9]] and call["prefix_of"] == [0, 1, 0, 1] and call["temperature"] == 0.5 and call["top_k"] == 2
    assert call["rows"] == [[11, 12, 13, 14], [21, 22], [31, 32, 33, 34], [41]]          # the visual rows are not repeated, no pad row goes down
    assert call["keep"] == [5, 3, 5, 2]                                                  # own length + 1: from the prefix's last row on
    assert call["targets"] == [11, 12, 13, 14, -100, 21, 22, -100, 31, 32, 33, 34, -100, 41, -100]
    assert sorted(out) == ["entropies", "logprobs", "token_ranks", "top_logprobs", "top_token_ids"]
    # entry 0 scores the first completion token from the prefix's last row
    assert out["logprobs"].tolist() == [[811, 1112, 1213, 1314], [921, 2122, 0, 0], [831, 3132, 3233, 3334], [941, 0, 0, 0]]
    assert out["entropies"].tolist() == [[8, 11, 12, 13], [9, 21, 0, 0], [8, 31, 32, 33], [9, 0, 0, 0]]
    assert out["top_token_ids"][3].tolist() == [[41, 42], [-1, -1], [-1, -1], [-1, -1]] and out["token_ranks"][1].tolist() == [9, 21, 0, 0]
    # it equals the unpadded pass over the repeated prefix, field by field
    ref_eng = _RaggedOnly()
    ref = _model(ref_eng).completion_logprobs(VIS, IDS, 2, MASK, 4, temperature=0.5, return_entropy=True, top_logprobs=2, unpadded=True)
    assert all(torch.equal(out[key], ref[key]) for key in ref)
    # fewer scored tokens, and the plain result forms
    lp = m.completion_logprobs(VIS, IDS, 2, MASK, 2, share_prefix=True)
    assert isinstance(lp, torch.Tensor) and eng.calls[-1]["keep"] == [3, 1, 3, 1] and "top_k" not in eng.calls[-1]
    assert lp.tolist() == [[1213, 1314], [0, 0], [3233, 3334], [0, 0]]
    lp2, ent2 = m.completion_logprobs(VIS, IDS, 2, None, None, return_entropy=True, share_prefix=True)
    assert lp2.shape == (4, 4) and eng.calls[-1]["keep"] == [5] * 4 and ent2[:, 0].tolist() == [8, 9, 8, 9]


class _RaggedOnly(_Eng):
    """the reference side: `unpadded=True` hands the ragged call ONE packed tensor and its lengths"""

    def forward_logprobs_ragged(self, embeds, targets, keep, lengths=None, **kw):
        seqs, first = [], 0
        for n in lengths:
            seqs.append(embeds[first:first + n])
            first += n
        return super().forward_logprobs_ragged(seqs, targets, keep, **kw)


def test_a_row_the_entry_point_would_refuse_is_scored_on_its_concatenation_in_the_same_call():
    eng = _Eng(refused=[1, 3])                                         # both rows of image 1: its prefix stays out of the prefixed call
    m = _model(eng)
    out = m.completion_logprobs(VIS, IDS, 2, MASK, 4, return_entropy=True, top_logprobs=2, share_prefix=True)
    assert [c["name"] for c in eng.calls] == ["prefixed", "ragged"]
    assert eng.calls[0]["prefix_rows"] == [[8, 8]] and eng.calls[0]["prefix_of"] == [0, 0] and eng.calls[0]["keep"] == [5, 5]
    assert eng.calls[1]["lengths"] == [4, 3] and eng.calls[1]["keep"] == [3, 2] and eng.calls[1]["targets"] == [21, 22, -100, 41, -100]
    whole = _model(_Eng()).completion_logprobs(VIS, IDS, 2, MASK, 4, return_entropy=True, top_logprobs=2, share_prefix=True)
    assert all(torch.equal(out[key], whole[key]) for key in whole)
    eng2 = _Eng(refused=[0, 1, 2, 3])
    all_ragged = _model(eng2).completion_logprobs(VIS, IDS, 2, MASK, 4, return_entropy=True, top_logprobs=2, share_prefix=True)
    assert [c["name"] for c in eng2.calls] == ["ragged"] and all(torch.equal(all_ragged[key], whole[key]) for key in whole)


def test_share_prefix_bad_masks_and_shapes_raise():
    eng = _Eng()
    m = _model(eng)
    with pytest.raises(NotImplementedError, match="holes"):
        m.completion_logprobs(VIS, IDS, 2, torch.tensor([[1] * 6, [1, 1, 0, 1, 1, 1], [1] * 6, [1] * 6]), 4, share_prefix=True)
    with pytest.raises(ValueError, match="left padding"):
        m.completion_logprobs(VIS, IDS, 2, torch.tensor([[1] * 6, [0] + [1] * 5, [1] * 6, [1] * 6]), 4, share_prefix=True)
    with pytest.raises(ValueError, match="end inside the visual prefix"):
        m.completion_logprobs(VIS, IDS, 2, torch.tensor([[1] * 6, [1] * 2 + [0] * 4, [1] * 6, [1] * 6]), 4, share_prefix=True)
    with pytest.raises(ValueError, match="does not cover"):
        m.completion_logprobs(VIS, IDS, 2, torch.ones(4, 5, dtype=torch.long), 4, share_prefix=True)
    with pytest.raises(ValueError, match="num_generations"):
        m.completion_logprobs(VIS, IDS, 3, MASK, 4, share_prefix=True)
    with pytest.raises(ValueError, match="num_logits_to_keep"):
        m.completion_logprobs(VIS, IDS, 2, MASK, 5, share_prefix=True)
    assert eng.calls == []
    old = types.SimpleNamespace(embed_tokens=eng.embed_tokens, forward_logprobs_ragged=eng.forward_logprobs_ragged)
    with pytest.raises(NotImplementedError, match="forward_logprobs_prefixed"):
        _model(old).completion_logprobs(VIS, IDS, 2, MASK, 4, share_prefix=True)
