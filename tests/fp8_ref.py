"""The reference side of tests/test_gpu_fp8_ops.py: weight constructions, torch's own e4m3 quantisation, the stated layouts of the
quantiser's two images and float64 restatements of the fp8-weight Linears.  torch only (importable without the engine, runs on any
device); pinned by itself on the CPU in tests/test_fp8_ops_host.py.

Weight-only quantisation as sv_load_weight does it (csrc/gemm_pack.hip fp8_row_scale_kernel / pack_weight_fp8_kernel): one scale per
output row, scale[n] = max_k |W[n][k]| / 448 (1 for an all-zero row), q = e4m3_rne(W / scale) with the division in float32."""
import torch

BF16_1ULP = 2.0 ** -8
E4M3_MAX = 448.0


def e4m3_table():
    """The value of each of the 256 e4m3 codes (float32; the two NaN codes included)."""
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()


def e4m3_midpoints():
    """The 126 midpoints between adjacent non-negative finite codes c, c + 1 (c = 0 .. 125), ascending: 7 between subnormals (the first
    one between 0 and the smallest subnormal), 1 between the largest subnormal and the smallest normal, 118 between normals.  Each has
    at most 5 significant bits: exact in bf16.  RNE sends midpoint c to the EVEN one of the codes c, c + 1."""
    v = e4m3_table()[:0x7F].double()
    return ((v[:-1] + v[1:]) / 2).float()


def exact_weights(N, K, g, device="cpu"):          # (g: a generator of that device)
    """Weights the quantiser has to reproduce without rounding: W = q * 2^j[n] with q random e4m3 values (zeros and subnormals included,
    NaN codes replaced by +-448's codes), one element per row forced to +-448, j[n] random in -8 .. 8.  Then amax / 448 = 2^j exactly and
    W is exact in bf16 (4 significant bits, exponents inside -17 .. 16).  Returns (W float32 [N, K], q float32 [N, K], scale float32 [N])."""
    code = torch.randint(0, 256, (N, K), generator=g, device=device, dtype=torch.int32)
    code = torch.where((code & 0x7F) == 0x7F, code - 1, code)
    sign = torch.randint(0, 2, (N,), generator=g, device=device, dtype=torch.int32) * 0x80
    col = torch.randint(0, K, (N,), generator=g, device=device)
    code[torch.arange(N, device=device), col] = 0x7E + sign
    q = e4m3_table().to(device)[code]
    j = torch.randint(-8, 9, (N,), generator=g, device=device)
    scale = torch.ldexp(torch.ones(N, device=device), j)
    return q * scale[:, None], q, scale


def natural_weights(N, K, g, device="cpu", dtype=torch.bfloat16):
    """randn / sqrt(K) times a per-row factor in [0.5, 2] (neighbouring rows' maxima differ: a scale read from the wrong row shows), row
    min(3, N - 1) all zero (scale 1, q 0).  dtype bfloat16, or float32 for the quantiser's fp32 source."""
    W = torch.randn(N, K, generator=g, device=device) / K ** 0.5 * (0.5 + 1.5 * torch.rand(N, 1, generator=g, device=device))
    W[min(3, N - 1)] = 0
    return W.to(dtype)


def designed_quantiser_rows(K, g, f32):
    """Rows that probe the rounding of the quantiser, each with a power-of-two scale 2^j (one element is +-448 * 2^j) so that W / scale
    is exact and the expected code depends on the rounding rule alone.  Returns (rows float32 [R, K], names):
      ties          every element on a midpoint between adjacent codes (all 8 that touch a subnormal, then the rest in random order,
                    random signs): RNE goes to the even code, subnormals included
      outlier       one element 2^10 times the largest of the others: they land on the smallest normals, the subnormals and zero
      negative max  the row maximum is negative: the scale is its magnitude
      off-midpoint  (fp32 source only) midpoints moved by 1 .. 3 fp32 ulps to either side: not bf16 numbers -- a quantiser that rounds
                    its source to bf16 first lands on the midpoint and then on the even code, wrong for half of them"""
    mid = e4m3_midpoints()
    order = torch.cat([torch.arange(8), 8 + torch.randperm(mid.numel() - 8, generator=g)])
    pick = mid[order[torch.arange(K - 1) % mid.numel()]]
    sgn = lambda n: torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    ties = torch.cat([torch.tensor([E4M3_MAX]), pick * sgn(K - 1)]) * 2.0 ** -3
    outlier = torch.randn(K, generator=g).bfloat16().float().clamp(-3.5, 3.5)
    outlier[K // 3] = -3.5 * 2.0 ** 10
    neg = torch.randn(K, generator=g).bfloat16().float().clamp(-3, 3)
    neg[K - 5] = -7.0
    rows, names = [ties, outlier, neg], ["ties", "outlier", "negative max"]
    if f32:
        ulps = torch.randint(1, 4, (K - 1,), generator=g).float() * sgn(K - 1)
        off = pick * (1 + ulps * 2.0 ** -23)
        assert bool((off.bfloat16().float() == pick).all()) and bool((off != pick).all())
        rows.append(torch.cat([torch.tensor([-E4M3_MAX]), off * sgn(K - 1)]) * 2.0 ** 5)
        names.append("off-midpoint")
    return torch.stack(rows), names


def quantise(W):
    """torch's own cast: (scale float32 [N], q float32 [N, K] = the e4m3 values) of W [N, K] (any float dtype; computed in float32)."""
    Wf = W.float()
    amax = Wf.abs().amax(1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    return scale, (Wf / scale[:, None]).to(torch.float8_e4m3fn).float()


def dequantised(W):
    """(scale, float64 [N, K] = q * scale): the weight an fp8 Linear computes with."""
    scale, q = quantise(W)
    return scale, q.double() * scale.double()[:, None]


def wp_index(Npad, K):
    """The packed layout of a bf16 weight image (csrc/kernels.h, pack_weight_kernel) [Npad/32][K/16][64 lanes][8]: W[n][k] sits at
    (((n // 32) * (K // 16) + k // 16) * 64 + ((k // 8) & 1) * 32 + n % 32) * 8 + k % 8."""
    n = torch.arange(Npad)[:, None]
    k = torch.arange(K)[None, :]
    return (((n // 32) * (K // 16) + k // 16) * 64 + ((k // 8) & 1) * 32 + n % 32) * 8 + k % 8


def wq_index(Npad, K):
    """The decode image of an fp8 weight (csrc/kernels.h, pack_weight_fp8_kernel) [Npad/32][K/32][64 lanes][16 bytes], a lane's two
    consecutive k-steps of 8 codes each: W[n][k] sits at byte
    (((n // 32) * (K // 32) + k // 32) * 64 + ((k // 8) & 1) * 32 + n % 32) * 16 + ((k // 16) & 1) * 8 + k % 8."""
    n = torch.arange(Npad)[:, None]
    k = torch.arange(K)[None, :]
    return (((n // 32) * (K // 32) + k // 32) * 64 + ((k // 8) & 1) * 32 + n % 32) * 16 + ((k // 16) & 1) * 8 + k % 8


ACTS = {"none": lambda t: t, "gelu_tanh": lambda t: torch.nn.functional.gelu(t, approximate="tanh")}


def linear_ref(x, Wd, bias=None, residual=None, act="none", out_f32=False):
    """float64 restatement of the big-M Linear (tests/test_gpu_ops.py test_linear_mfma): x Wd^T + bias; an activation acts on the bf16-rounded
    Linear output; a residual is added to the bf16-rounded result.  Wd float64 (dequantised)."""
    y = x.double() @ Wd.T
    if bias is not None:
        y = y + bias.double()
    if out_f32:
        return y
    if act != "none":
        y = ACTS[act](y.bfloat16().double())
    if residual is not None:
        y = y.bfloat16().double() + residual.double()
    return y


def c_fc_ref(x, Wd, bias, act):
    """float64 restatement of the decode GEMM's c_fc epilogue: act(bf16(x Wd^T + bias))."""
    return ACTS[act]((x.double() @ Wd.T + bias.double()).bfloat16().double())


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.abs().max())


def mean_err(got, ref):
    return float((got.double() - ref.double()).abs().mean() / ref.abs().max())


# the project's own bounds for each output form (tests/test_gpu_ops.py, tests/test_gpu_fp8.py), as (max, mean) relative to max |ref|
BOUND_F32 = (2e-5, None)                      # fp32 outputs: accumulation order only
BOUND_BIG_M = (2.2 * BF16_1ULP, 6e-4)         # big-M bf16 outputs
BOUND_C_FC = (2.2 * BF16_1ULP, 1.5e-3)        # decode c_fc form
BOUND_LOGITS = (1.1 * BF16_1ULP, None)        # decode logits form (and every value a bf16 value)


def assert_within(got, ref, bound, what):
    r, m = rel_err(got, ref), mean_err(got, ref)
    print(f"[fp8 ops] {what}: max {r:.3e} (bound {bound[0]:.3e}), mean {m:.3e}" + (f" (bound {bound[1]:.1e})" if bound[1] else ""))
    assert r <= bound[0], (what, r)
    assert bound[1] is None or m <= bound[1], (what, m)
