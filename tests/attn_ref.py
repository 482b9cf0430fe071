"""A plain float32 restatement of the prompt-pass attention over packed rows: the comparator of tests/test_gpu_prefill_attention.py,
pinned itself against a per-row loop by tests/test_prefill_attention_host.py (CPU).  torch only: importable without the engine."""
import torch


def ref(q, k, v, H, Hkv, lens, causal, window, scale=None):
    """q [rows, H*hd], k / v [rows, Hkv*hd] float32 (bf16-exact values), rows = sum(lens): sequence b owns lens[b] consecutive rows.
    Query i of a sequence (i counted from the sequence's first row) sees keys j of the SAME sequence; causal: j <= i, and with
    window > 0 also j > i - window (window = 0: all).  Scores times scale (default hd ** -0.5), softmax in float32, probabilities
    rounded to bf16 before P.V, the result not rounded.  Query head h reads KV head h // (H // Hkv).  Returns [rows, H*hd] float32."""
    rows = q.shape[0]
    hd = q.shape[1] // H
    assert sum(lens) == rows and k.shape == v.shape == (rows, Hkv * hd) and H % Hkv == 0
    assert causal or not window
    scale = hd ** -0.5 if scale is None else scale
    out = torch.empty(rows, H * hd, dtype=torch.float32)
    r0 = 0
    for S in lens:
        qq = q[r0:r0 + S].float().view(S, H, hd).transpose(0, 1)                                          # [H, S, hd]
        kk = k[r0:r0 + S].float().view(S, Hkv, hd).transpose(0, 1).repeat_interleave(H // Hkv, dim=0)
        vv = v[r0:r0 + S].float().view(S, Hkv, hd).transpose(0, 1).repeat_interleave(H // Hkv, dim=0)
        s = qq @ kk.transpose(-1, -2) * scale
        if causal:
            i = torch.arange(S).view(S, 1)
            j = torch.arange(S).view(1, S)
            seen = j <= i
            if window > 0:
                seen = seen & (j > i - window)
            s = s.masked_fill(~seen, float("-inf"))
        p = torch.softmax(s, -1).bfloat16().float()
        out[r0:r0 + S] = (p @ vv).transpose(0, 1).reshape(S, H * hd)
        r0 += S
    return out
