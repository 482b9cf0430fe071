"""A torch restatement of the e4m3 KV cache's rule (include/starvector_hip.h, SV_KV_FP8_E4M3): the reference side of
tests/test_gpu_kv_fp8_ops.py and tests/test_gpu_kv_fp8.py, pinned by itself on the CPU in tests/test_kv_fp8_host.py.  torch only
(importable without the engine, runs on any device).

For every row of D bf16 values (one token, one KV head; K after RoPE, or V):
  amax = max |x| over the finite elements;  E = floor(log2(amax)) - 7 clamped to [-120, 120], E = 0 when amax = 0;
  code = e4m3_rne(x * 2^-E) (the multiply exact, nothing saturates: the scaled maximum lies in [128, 256));  non-finite x -> the NaN code;
  deq = e4m3(code) * 2^E, exactly a bf16 number."""
import torch

from tests import fp8_ref

NAN_CODE = 0x7F
E_MIN, E_MAX = -120, 120


def cast(y):
    """The cast of the rule on already scaled values (any float dtype): clamp to +-448, then torch's own round-to-nearest-even
    conversion.  Returns the uint8 codes."""
    return y.float().clamp(-fp8_ref.E4M3_MAX, fp8_ref.E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def exponents(x):
    """E of every row of x [..., D] (int64 [...])."""
    xf = x.float()
    amax = torch.where(torch.isfinite(xf), xf.abs(), torch.zeros_like(xf)).amax(-1)
    _, e = torch.frexp(amax.double())                        # amax = m * 2^e with m in [0.5, 1): floor(log2(amax)) = e - 1, exactly
    E = (e.long() - 1 - 7).clamp(E_MIN, E_MAX)
    return torch.where(amax > 0, E, torch.zeros_like(E))


def quant(x):
    """x [..., D] (bf16, or a float dtype holding bf16 values) -> (codes uint8 [..., D], E int64 [...])."""
    E = exponents(x)
    xd = x.double()
    finite = torch.isfinite(xd)
    y = torch.ldexp(torch.where(finite, xd, torch.zeros_like(xd)), -E[..., None])      # exact in float64
    codes = cast(y)
    return torch.where(finite, codes, torch.full_like(codes, NAN_CODE)), E


def deq(codes, E):
    """(codes, E) -> bf16 [..., D]: e4m3(code) * 2^E (exact; the NaN codes give NaN)."""
    v = fp8_ref.e4m3_table().to(codes.device)[codes.long()].double()
    return torch.ldexp(v, E[..., None]).float().to(torch.bfloat16)


def deq_quant(x):
    """What a later decode step reads where x was stored: bf16 [..., D]."""
    return deq(*quant(x))


def same_bits(a, b):
    """bf16 tensors equal bit for bit, a NaN matching any NaN (the payload of a NaN is not part of the rule)."""
    a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    nan = torch.isnan(a) & torch.isnan(b)
    return bool(((a.view(torch.int16) == b.view(torch.int16)) | nan).all())


# ---- designed rows ---------------------------------------------------------------------------------------------------
def exact_rows(N, D, g, j_lo=-8, j_hi=8):
    """Rows the quantiser has to reproduce without rounding: e4m3 values times 2^j[n], every |value| below 256 and one element per row in
    [128, 256) (codes 0x70 .. 0x77, either sign), so that E = j exactly.  Returns (x float32 [N, D] holding bf16 values, codes, j)."""
    code = torch.randint(0, 256, (N, D), generator=g, dtype=torch.int32)
    code = torch.where((code & 0x7F) > 0x77, code - 8, code)                           # magnitudes <= 240
    top = 0x70 + torch.randint(0, 8, (N,), generator=g, dtype=torch.int32) + 0x80 * torch.randint(0, 2, (N,), generator=g, dtype=torch.int32)
    code[torch.arange(N), torch.randint(0, D, (N,), generator=g)] = top
    j = torch.randint(j_lo, j_hi + 1, (N,), generator=g)
    x = torch.ldexp(fp8_ref.e4m3_table()[code.long()].double(), j[:, None]).float()
    assert bool((x.bfloat16().float() == x).all())
    return x, code.to(torch.uint8), j


def tie_rows(D, g, j=-3):
    """Rows whose elements all sit on midpoints between adjacent codes after scaling (every midpoint below 256 -- what a scaled row can
    hold -- in random order and sign, subnormal ones included), behind one element 2^7 that fixes E = j.  Returns x float32 [R, D]."""
    mid = fp8_ref.e4m3_midpoints()
    mid = mid[mid < 256]
    R = (mid.numel() + D - 2) // (D - 1)
    order = torch.randperm(mid.numel(), generator=g)
    pick = mid[order[torch.arange(R * (D - 1)) % mid.numel()]].view(R, D - 1)
    sgn = torch.randint(0, 2, (R, D - 1), generator=g).float() * 2 - 1
    x = torch.cat([torch.full((R, 1), 128.0), pick * sgn], 1) * 2.0 ** j
    assert bool((x.bfloat16().float() == x).all())
    return x


def special_rows(D, g):
    """(x float32 [R, D] holding bf16 values, names): the rows that exercise the rule's corners."""
    rn = lambda: torch.randn(D, generator=g).bfloat16().float()
    outlier = rn().clamp(-3.5, 3.5)
    outlier[D // 3] = -3.5 * 2.0 ** 10                       # the others land on the smallest normals, the subnormals and zero
    zero = torch.zeros(D)
    nonfinite = rn()
    nonfinite[1], nonfinite[D // 2], nonfinite[D - 2] = float("inf"), float("nan"), float("-inf")
    tiny = rn().clamp(-1, 1) * 2.0 ** -128                   # amax = bf16's smallest normal: E clamps at -120
    tiny[5] = 2.0 ** -126
    big = rn().clamp(-1, 1) * 2.0 ** 119                     # amax = 2^120: E = 113, no clamp yet
    big[7] = 2.0 ** 120
    huge = rn().clamp(-1, 1) * 2.0 ** 126                    # amax = 1.5 * 2^127: E clamps at 120
    huge[9] = -1.5 * 2.0 ** 127
    rows = torch.stack([outlier, zero, nonfinite, tiny, big, huge]).bfloat16().float()
    return rows, ["outlier", "all zero", "inf and nan", "amax 2^-126", "amax 2^120", "amax 1.5 * 2^127"]
