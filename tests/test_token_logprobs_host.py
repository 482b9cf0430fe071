"""CPU: per-token log-probs of the scoring forward -- the host logic of StarVectorForCausalLM.completion_logprobs over a scripted
engine (shift, num_generations, padding), and the argument checks of sv_forward_logprobs / sv_op_logprob_rows /
sv_debug_set_score_chunk_rows through the built library, which come before any device work."""
import ctypes as C
import types

import pytest
import torch


class _Eng:
    """forward_logprobs scripted so that placement shows: logprob = 100 * (embedding value of the row's own position) + target id
    (0 where the target is -100, as the kernel does), entropy = the embedding value of the row's position."""

    def __init__(self):
        self.calls = []

    def embed_tokens(self, ids):
        return ids.float().unsqueeze(-1).expand(-1, -1, 4).to(torch.bfloat16)

    def forward_logprobs(self, emb, targets, keep, temperature=1.0, entropy=False, argmax=False):
        from starvector_amd.engine import TokenLogprobs
        assert emb.dtype == torch.bfloat16 and targets.dtype == torch.int32 and tuple(targets.shape) == (emb.shape[0], keep)
        self.calls.append((tuple(emb.shape), keep, float(temperature), bool(entropy)))
        pos = emb[:, -keep:, 0].float()
        lp = torch.where(targets == -100, torch.zeros_like(pos), 100.0 * pos + targets.float())
        return TokenLogprobs(lp, torch.zeros_like(lp), pos.clone() if entropy else None, None)


def _model():
    from starvector_amd.model import StarVectorForCausalLM
    m = StarVectorForCausalLM.__new__(StarVectorForCausalLM)
    torch.nn.Module.__init__(m)
    eng = _Eng()
    object.__setattr__(m, "engine", eng)
    object.__setattr__(m, "model", types.SimpleNamespace(_get_embeddings=eng.embed_tokens))
    return m, eng


VIS = torch.full((1, 3, 4), 9.0, dtype=torch.bfloat16)            # 3 visual positions, value 9
IDS = torch.tensor([[5, 6, 7, 8], [1, 2, 3, 4]])


def test_completion_logprobs_shift_and_prefix_repeat():
    m, eng = _model()
    out = m.completion_logprobs(VIS, IDS, 2, None, 3, temperature=0.5)
    # n + 1 = 4 rows kept of the 7 positions [9 9 9 | ids]; the visual prefix repeated for both completions
    assert eng.calls == [((2, 7, 4), 4, 0.5, False)]
    assert out.dtype == torch.float32 and out.shape == (2, 3)
    # out[b, j] scores id j + 1 of the kept window from the row of the position before it
    assert out.tolist() == [[100 * 5 + 6, 100 * 6 + 7, 100 * 7 + 8], [100 * 1 + 2, 100 * 2 + 3, 100 * 3 + 4]]
    # every completion token (n = 0 / None): the first one is predicted by the last visual position
    eng.calls.clear()
    out = m.completion_logprobs(VIS, IDS, 2, None, None)
    assert eng.calls == [((2, 7, 4), 5, 1.0, False)]
    assert out[0].tolist() == [100 * 9 + 5, 100 * 5 + 6, 100 * 6 + 7, 100 * 7 + 8]
    lp, ent = m.completion_logprobs(VIS, IDS, 2, torch.ones(2, 7, dtype=torch.long), 2, return_entropy=True)
    assert eng.calls[-1] == ((2, 7, 4), 3, 1.0, True)
    assert lp[1].tolist() == [100 * 2 + 3, 100 * 3 + 4] and ent[1].tolist() == [2, 3]
    # forward() itself is unchanged by the shared mask helper: the scripted engine has no forward_logits
    with pytest.raises(AttributeError):
        m.forward(VIS, IDS, 2, None, 3)


def test_completion_logprobs_padding():
    m, eng = _model()
    ref = m.completion_logprobs(VIS, IDS, 2, None, 3)
    # right padding: entries whose own token is a pad are 0, the others are untouched; one engine pass
    eng.calls.clear()
    right = torch.tensor([[1] * 7, [1, 1, 1, 1, 1, 0, 0]])
    out, ent = m.completion_logprobs(VIS, IDS, 2, right, 3, return_entropy=True)
    assert len(eng.calls) == 1
    assert out[0].tolist() == ref[0].tolist() and out[1].tolist() == [ref[1, 0].item(), 0.0, 0.0]
    assert ent[1].tolist() == [1.0, 0.0, 0.0]
    # left padding: the row is scored without its pads in its own pass -> the numbers of the unpadded row
    eng.calls.clear()
    left_ids = torch.tensor([[5, 6, 7, 8], [1, 2, 3, 4]])
    vis2 = torch.full((1, 3, 4), 9.0, dtype=torch.bfloat16)
    out = m.completion_logprobs(vis2, left_ids, 2, torch.tensor([[1] * 7, [0, 0, 1, 1, 1, 1, 1]]), 3)
    assert sorted(c[:2] for c in eng.calls) == [((1, 5, 4), 4), ((1, 7, 4), 4)]
    assert out.tolist() == ref.tolist()
    # a hole; kept rows reaching into the pads (the first scored token needs a real position before it); no real position
    with pytest.raises(NotImplementedError):
        m.completion_logprobs(VIS, IDS, 2, torch.tensor([[1] * 7, [1, 1, 0, 1, 1, 1, 1]]), 3)
    with pytest.raises(ValueError, match="left padding"):
        m.completion_logprobs(VIS, IDS, 2, torch.tensor([[1] * 7, [0, 0, 0, 0, 1, 1, 1]]), 3)
    m.completion_logprobs(VIS, IDS, 2, torch.tensor([[1] * 7, [0, 0, 0, 1, 1, 1, 1]]), 3)         # 3 pads + 3 + 1 rows = 7: fits
    with pytest.raises(ValueError, match="all zeros"):
        m.completion_logprobs(VIS, IDS, 2, torch.tensor([[1] * 7, [0] * 7]), 3)
    with pytest.raises(ValueError):
        m.completion_logprobs(VIS, IDS, 2, torch.ones(2, 6, dtype=torch.long), 3)                  # mask does not cover the inputs
    with pytest.raises(ValueError):
        m.completion_logprobs(VIS, IDS, 2, None, 5)                                                # more than the completion holds


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from starvector_amd import _lib
    return _lib.load()


def test_forward_logprobs_validation_precedes_device_work(lib):
    """NULL embeds / targets, n_keep outside 1..S, a temperature that is not finite and > 0, no output at all: SV_EINVAL with a
    message before the engine is even looked at (so the same checks run here, without a GPU)."""
    p = C.c_void_p(16)                                             # never dereferenced: the checks come first

    def call(embeds=p, S=8, n_keep=4, targets=p, t=1.0, outs=(p, p, None, None)):
        rc = lib.sv_forward_logprobs(None, embeds, 1, S, n_keep, targets, t, outs[0], outs[1], outs[2], outs[3], None)
        return rc, lib.sv_last_error().decode()

    rc, msg = call(embeds=None)
    assert rc == -22 and "null embeds" in msg
    rc, msg = call(targets=None)
    assert rc == -22 and "targets" in msg
    for S, n in [(8, 0), (8, 9), (8, -1), (0, 1)]:
        rc, msg = call(S=S, n_keep=n)
        assert rc == -22 and "n_keep" in msg, (S, n, msg)
    for t in (0.0, -1.0, float("inf"), float("nan")):
        rc, msg = call(t=t)
        assert rc == -22 and "temperature" in msg, (t, msg)
    rc, msg = call(outs=(None, None, None, None))
    assert rc == -22 and "output" in msg
    rc, msg = call()                                               # everything valid but the engine
    assert rc == -22 and "null engine" in msg
    rc, msg = call(outs=(None, None, None, p))                     # one output is enough
    assert rc == -22 and "null engine" in msg


def test_logprob_rows_and_chunk_rows_validation(lib):
    p = C.c_void_p(16)

    def op(logits=p, R=4, V=100, ld=104, targets=p, t=1.0, outs=(p, None, None, None)):
        rc = lib.sv_op_logprob_rows(logits, R, V, ld, targets, t, outs[0], outs[1], outs[2], outs[3], None, None)
        return rc, lib.sv_last_error().decode()

    assert op(logits=None)[0] == -22 and op(R=0)[0] == -22 and op(V=0)[0] == -22
    assert op(ld=96)[0] == -22                                     # ld < V
    rc, msg = op(ld=100)                                           # rows would not start 16-byte aligned
    assert rc == -22 and "multiple of 8" in msg
    assert op(logits=C.c_void_p(8))[0] == -22                      # base not 16-byte aligned
    rc, msg = op(targets=None)
    assert rc == -22 and "targets" in msg
    rc, msg = op(outs=(None, None, None, None))
    assert rc == -22 and "output" in msg
    for t in (0.0, float("nan"), float("inf")):
        rc, msg = op(t=t)
        assert rc == -22 and "temperature" in msg
    assert lib.sv_debug_set_score_chunk_rows(None, 256) == -22 and "null engine" in lib.sv_last_error().decode()
    for rows in (100, -256, 65536 + 256):
        assert lib.sv_debug_set_score_chunk_rows(None, rows) == -22 and "multiple of 256" in lib.sv_last_error().decode()
