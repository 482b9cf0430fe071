"""CPU: (1) the float32 attention reference of the prompt-pass operator tests (tests/attn_ref.py) against a per-row Python loop, so that
its mask cannot share an off-by-one with the kernel unnoticed; (2) sv_op_attention_prefill rejects every bad argument with SV_EINVAL and
a message before any device work (the pointers it is given here are never dereferenced)."""
import ctypes as C

import pytest
import torch

from tests.attn_ref import ref


def _loop_ref(q, k, v, H, Hkv, lens, causal, window, scale):
    """One query row and one head at a time, the visible keys listed by index."""
    hd = q.shape[1] // H
    out = torch.zeros(q.shape[0], H * hd)
    r0 = 0
    for S in lens:
        for i in range(S):
            if causal:
                first = max(0, i - window + 1) if window > 0 else 0
                keys = list(range(first, i + 1))
            else:
                keys = list(range(S))
            for h in range(H):
                kh = h // (H // Hkv)
                qi = q[r0 + i, h * hd:(h + 1) * hd]
                sc = torch.stack([(qi * k[r0 + j, kh * hd:(kh + 1) * hd]).sum() * scale for j in keys])
                m = sc.max()
                e = torch.exp(sc - m)
                p = (e / e.sum()).bfloat16().float()
                acc = torch.zeros(hd)
                for n, j in enumerate(keys):
                    acc += p[n] * v[r0 + j, kh * hd:(kh + 1) * hd]
                out[r0 + i, h * hd:(h + 1) * hd] = acc
        r0 += S
    return out


@pytest.mark.parametrize("H,Hkv,hd,lens,causal,window", [
    (4, 1, 8, [9], 1, 0),                    # multi-query, causal
    (4, 2, 8, [7, 1, 12], 1, 3),             # ragged, grouped heads, a window shorter than two of the sequences
    (2, 2, 8, [6, 10], 1, 1),                # window 1: every row sees itself alone
    (2, 2, 8, [5, 8], 1, 8),                 # a window equal to the longest sequence: nothing is cut
    (3, 3, 8, [6, 4], 0, 0),                 # unmasked, keys of the own sequence only
])
def test_reference_equals_a_per_row_loop(H, Hkv, hd, lens, causal, window):
    g = torch.Generator().manual_seed(H * 100 + sum(lens) + window)
    rows = sum(lens)
    q = (3 * torch.randn(rows, H * hd, generator=g)).bfloat16().float()
    k = torch.randn(rows, Hkv * hd, generator=g).bfloat16().float()
    v = torch.randn(rows, Hkv * hd, generator=g).bfloat16().float()
    got = ref(q, k, v, H, Hkv, lens, causal, window)
    want = _loop_ref(q, k, v, H, Hkv, lens, causal, window, hd ** -0.5)
    # float32 summation order only -- except where it moves a probability across a bf16 rounding boundary: one bf16 ulp of p (2^-8) times |v|
    err = (got - want).abs().max().item()
    assert err <= 2.0 ** -8 * v.abs().max().item() + 1e-5, err
    assert (got - want).abs().mean().item() <= 1e-4
    if window == 1:
        idx = torch.arange(H) // (H // Hkv)
        assert torch.equal(got.view(rows, H, hd), v.view(rows, Hkv, hd)[:, idx])
    if window >= max(lens):
        assert torch.equal(got, ref(q, k, v, H, Hkv, lens, causal, 0))


def test_reference_window_mask_by_hand():
    """One head, one-hot values: the output row IS the probability row, so the visible key set can be read off it."""
    S, W, hd = 7, 3, 8
    q = torch.zeros(S, hd)
    k = torch.zeros(S, hd)
    v = torch.zeros(S, hd)
    v[torch.arange(S), torch.arange(S)] = 1.0
    out = ref(q, k, v, 1, 1, [S], 1, W)
    for i in range(S):
        seen = [j for j in range(S) if out[i, j] > 0]
        assert seen == list(range(max(0, i - W + 1), i + 1)), (i, seen)
        assert float(out[i, i]) == float(torch.tensor(1.0 / len(seen)).bfloat16())
    two = ref(torch.cat([q, q[:4]]), torch.cat([k, k[:4]]), torch.cat([v, v[:4]]), 1, 1, [S, 4], 1, W)
    assert torch.equal(two[:S], out) and torch.equal(two[S:], out[:4])          # the second sequence starts over at its own row 0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from starvector_amd import _lib
    return _lib.load()


def test_attention_prefill_argument_validation_precedes_any_device_work(lib):
    p = C.c_void_p(16)                                                           # never dereferenced: the checks come first

    def call(qkv=p, q_off=0, k_off=256, v_off=384, stride=512, out=p, B=1, S=40, lens=None, H=2, Hkv=1, hd=128, causal=1, scale=0.1,
             window=0, last_rows=0):
        c_lens = (C.c_int32 * len(lens))(*lens) if lens is not None else None
        rc = lib.sv_op_attention_prefill(qkv, q_off, k_off, v_off, stride, out, B, S, c_lens, H, Hkv, hd, causal, scale, window, last_rows, None)
        return rc, lib.sv_last_error().decode()

    bad = [
        (dict(qkv=None), "null pointer"), (dict(out=None), "null pointer"),
        (dict(H=3, Hkv=2, stride=1024), "not a multiple"),
        (dict(hd=96), "head_dim"), (dict(hd=32), "head_dim"),
        (dict(q_off=4), "multiples of 8"), (dict(k_off=260), "multiples of 8"), (dict(v_off=380), "multiples of 8"),
        (dict(stride=516), "multiples of 8"), (dict(q_off=-8), "multiples of 8"),
        (dict(q_off=264), "beyond the row stride"),                             # (q columns may overlap k's: the row stride is the only bound)
        (dict(k_off=392), "beyond the row stride"), (dict(v_off=392), "beyond the row stride"), (dict(stride=504), "beyond the row stride"),
        (dict(H=6), "beyond the row stride"),
        (dict(window=-1), "window"), (dict(window=8, causal=0), "causal"),
        (dict(lens=[5, 7], B=2, causal=0), "causal"),
        (dict(lens=[5, 0], B=2), "length"), (dict(lens=[-3], B=1), "length"),
        (dict(last_rows=-1), "last_rows"),
        (dict(S=0), "S 0"), (dict(B=0), "bad shape"), (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"),
    ]
    for kw, msg in bad:
        rc, err = call(**kw)
        assert rc == -22 and msg in err and "sv_op_attention_prefill" in err, (kw, rc, err)
