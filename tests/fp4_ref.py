"""The reference side of the MXFP4 tests: the format restated in torch (csrc/kernels.h launch_pack_weight_mxfp4, include/starvector_hip.h
sv_config.weight_dtype), the stated layouts of the quantiser's images and weight constructions.  torch only (importable without the
engine, runs on any device); pinned by itself on the CPU in tests/test_mxfp4_host.py.

Weight-only quantisation per output row n and block of 32 consecutive k (K zero-padded to a multiple of 64): amax = max |W| of the block,
taken from the tensor as handed; amax == 0: E = 0, codes 0; else E = floor(log2(amax)) - 2 clamped to [-125, 125], stored as the byte
E + 127; q = W / 2^E rounded to {0, .5, 1, 1.5, 2, 3, 4, 6} with its sign, ties to the code with the even mantissa bit (= the even index),
magnitudes above 6 saturating.  Everything here is computed in float64, where W / 2^E is exact."""
import torch

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E2M1_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)          # between codes j and j + 1
E2M1_TIE_GOES_TO = (0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0)            # the even one of the two
GROUP = 1088                                                      # bytes of one (column tile, 64 k) group of the decode image


def e2m1_table(device="cpu"):
    return torch.tensor(E2M1, dtype=torch.float64, device=device)


def round_e2m1_index(a):
    """a >= 0 (float64) -> the index 0..7 of the nearest e2m1 magnitude; a on a midpoint -> the even index; above 6 -> 7."""
    mid = torch.tensor(E2M1_MIDPOINTS, dtype=torch.float64, device=a.device)
    idx = torch.bucketize(a, mid, right=False)                    # midpoints strictly below a: a tie lands on the lower code
    tie = (idx < 7) & (a == mid[idx.clamp(max=6)])
    return torch.where(tie & (idx % 2 == 1), idx + 1, idx)


def pow2(E):
    """2^E as float64 for an int64 tensor E in -1022 .. 1023, built from the bit pattern: exact on every device (a library pow need not be)."""
    return ((E.long() + 1023) << 52).view(torch.float64)


def _blocks(W):
    """W [N, K] -> float64 [N, Kpad / 32, 32], K zero-padded to a multiple of 64."""
    N, K = W.shape
    Kpad = (K + 63) // 64 * 64
    Wd = torch.zeros(N, Kpad, dtype=torch.float64, device=W.device)
    Wd[:, :K] = W.double()                                        # bf16 and fp32 are exact in float64: the source as handed
    return Wd.view(N, Kpad // 32, 32)


def block_exponents(W):
    """int64 [N, Kpad / 32]: E of every block."""
    amax = _blocks(W).abs().amax(-1)
    _, e = torch.frexp(amax)                                      # amax = m * 2^e, m in [0.5, 1): floor(log2(amax)) = e - 1
    E = (e.long() - 1 - 2).clamp(-125, 125)
    return torch.where(amax > 0, E, torch.zeros_like(E))


def quantise(W):
    """(scale bytes uint8 [N, Kpad / 32], values float64 [N, K] = the signed e2m1 numbers q) of W [N, K] (bf16 or float32)."""
    N, K = W.shape
    B = _blocks(W)
    E = block_exponents(W)
    a = B / pow2(E)[..., None]
    q = e2m1_table(W.device)[round_e2m1_index(a.abs())] * torch.where(a < 0, -1.0, 1.0)
    return (E + 127).to(torch.uint8), q.view(N, -1)[:, :K]


def dequantised(W):
    """(scale bytes, float64 [N, K] = q * 2^E): the weight an MXFP4 Linear computes with."""
    N, K = W.shape
    sc, q = quantise(W)
    E = (sc.long() - 127).repeat_interleave(32, dim=1)[:, :K]
    return sc, q * pow2(E)


def fake_quantize_mxfp4(w, cfg):
    """The engine's `weight_dtype = "mxfp4"` mode over a state dict, the key list of oracle.fake_quantize_fp8: every decoder Linear weight
    and the lm_head replaced by dequant(quant(W)), W taken as the bf16 tensor the engine is handed.  Embedding lookups keep their table.
    Returns a new dict (float32 values, each exactly a bf16 number)."""
    from oracle import starvector_oracle as O
    out = dict(w)
    pre = O.P_DEC2 if cfg.arch == "v2" else O.P_DEC
    keys = [O.K_LMH]
    for i in range(cfg.n_layer):
        if cfg.arch == "v2":
            b = f"{pre}layers.{i}."
            keys += [b + n for n in ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                                     "self_attn.o_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")]
        else:
            b = f"{pre}h.{i}."
            keys += [b + n for n in ("attn.c_attn.weight", "attn.c_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")]
    for k in keys:
        out[k] = dequantised(w[k].to(torch.bfloat16))[1].float()
    return out


# ---- the stated layouts -------------------------------------------------------------------------------------------------------------
def w4_code_index(Npad, K):
    """The decode image (csrc/kernels.h): groups [Npad/32][K/64] of 1088 bytes.  The code of W[n][k] sits in byte
    ((n // 32) * (K // 64) + k // 64) * 1088 + (((k // 8) & 1) * 32 + n % 32) * 16 + ((k // 16) & 3) * 4 + (k % 8) // 2, in the low nibble
    for even k and the high nibble for odd k.  Returns (byte index, shift) as int64 [Npad, K]."""
    n = torch.arange(Npad)[:, None]
    k = torch.arange(K)[None, :]
    byte = ((n // 32) * (K // 64) + k // 64) * GROUP + (((k // 8) & 1) * 32 + n % 32) * 16 + ((k // 16) & 3) * 4 + (k % 8) // 2
    return byte, ((k & 1) * 4).expand(Npad, K)


def w4_scale_index(Npad, K):
    """The scale byte of block (n, b = k // 32) sits at ((n // 32) * (K // 64) + b // 2) * 1088 + 1024 + (n % 32) * 2 + (b & 1).
    Returns int64 [Npad, K / 32]."""
    n = torch.arange(Npad)[:, None]
    b = torch.arange(K // 32)[None, :]
    return ((n // 32) * (K // 64) + b // 2) * GROUP + 1024 + (n % 32) * 2 + (b & 1)


def image_bytes(Npad, K):
    return Npad // 32 * (K // 64) * GROUP


def codes_of(q):
    """signed e2m1 values float64 -> the 4-bit codes uint8 (sign bit 8 for negative values; a zero is code 0)."""
    idx = torch.bucketize(q.abs(), e2m1_table(q.device))          # exact table values -> their index
    return (idx + torch.where(q < 0, 8, 0)).to(torch.uint8)


def decode_image_values(img, sc_plain, Npad, K):
    """Reads a raw decode image back through the stated layout: (values float64 [Npad, K] = the signed e2m1 numbers, scale bytes
    uint8 [Npad, K / 32] read from the image's own scale slots)."""
    img = img.cpu()
    byte, shift = w4_code_index(Npad, K)
    code = (img[byte].long() >> shift) & 15
    val = e2m1_table()[code & 7] * torch.where(code >= 8, -1.0, 1.0)
    return val, img[w4_scale_index(Npad, K)]


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def exact_weights(N, K, g, dtype=torch.bfloat16):
    """Weights the quantiser has to reproduce without rounding: per block random codes (zeros included) times 2^j, j random in -8 .. 8,
    one element of every block forced to +-4 or +-6 (then amax / 2^E lies in [4, 8) with E = j: the block's exponent IS j).  Exact in bf16
    (two significant bits).  Returns (W [N, K] dtype, q float64 [N, K], E int64 [N, K / 32])."""
    nb = K // 32
    code = torch.randint(0, 8, (N, nb, 32), generator=g)
    sgn = torch.randint(0, 2, (N, nb, 32), generator=g) * 2.0 - 1.0
    top = torch.randint(6, 8, (N, nb), generator=g)
    col = torch.randint(0, 32, (N, nb), generator=g)
    code.scatter_(2, col[..., None], top[..., None])
    q = e2m1_table()[code] * sgn
    j = torch.randint(-8, 9, (N, nb), generator=g)
    W = (q * pow2(j)[..., None]).view(N, K)
    assert bool((W.to(dtype).double() == W).all())
    return W.to(dtype), q.view(N, K), j


def natural_weights(N, K, g, dtype=torch.bfloat16):
    """randn / sqrt(K) times a per-row factor in [0.5, 2]; one all-zero block (row 0, block 1 when there is one) and one all-zero row
    (row min(3, N - 1)).  dtype bfloat16, or float32 for the quantiser's fp32 source."""
    W = torch.randn(N, K, generator=g) / K ** 0.5 * (0.5 + 1.5 * torch.rand(N, 1, generator=g))
    W[0, 32:64] = 0
    W[min(3, N - 1)] = 0
    return W.to(dtype)


def designed_rows(K, g, f32):
    """Rows that probe the rounding, built from 32-element blocks whose exponent is known by construction (one element is +-4 .. +-7.5
    times 2^j, so E = j), tiled over K.  Returns (rows float32 [R, K] -- every value a bf16 number unless f32 --, names):
      midpoints     every rounding midpoint with both signs (0.25 .. 5 -> the even code), next to a 6 that fixes the exponent
      outlier       one element 2^4 .. 2^5 times its neighbours: they land on 0 and 0.5
      negative max  the block maximum is negative
      saturate      magnitudes in (6, 8) * 2^E, which saturate to 6
      off-midpoint  (fp32 source only) midpoints moved by 1 .. 3 fp32 ulps to either side: not bf16 numbers -- a quantiser that rounds
                    its source to bf16 first lands on the midpoint and then on the even code, wrong for half of them"""
    mid = torch.tensor(E2M1_MIDPOINTS)
    nb = K // 32

    def tile(make):
        return torch.cat([make(b) for b in range(nb)])

    def midpoints(b):
        blk = torch.cat([mid, -mid, mid[torch.randint(0, 7, (17,), generator=g)] * (torch.randint(0, 2, (17,), generator=g) * 2.0 - 1.0)])
        blk = torch.cat([torch.tensor([6.0 if b % 2 else -6.0]), blk])[torch.randperm(32, generator=g)]
        return blk * 2.0 ** (b % 7 - 3)

    def outlier(b):
        blk = torch.randn(32, generator=g).clamp(-1, 1) * 0.25           # |.| <= 0.25 against an outlier of 5: q <= 0.5 * ... -> 0 or 0.5
        blk[b % 32] = 5.0
        return (blk * 2.0 ** (b % 5)).bfloat16().float()

    def negmax(b):
        blk = torch.randn(32, generator=g).clamp(-3, 3)
        blk[(3 * b) % 32] = -7.0
        return (blk * 2.0 ** -(b % 4)).bfloat16().float()

    def saturate(b):
        blk = 6.0 + 2.0 * (torch.arange(32) + 1) / 34.0                    # (6, 8)
        blk = blk * (torch.randint(0, 2, (32,), generator=g) * 2.0 - 1.0)
        return (blk * 2.0 ** (b % 3 - 1)).bfloat16().float()

    rows, names = [tile(midpoints), tile(outlier), tile(negmax), tile(saturate)], ["midpoints", "outlier", "negative max", "saturate"]
    if f32:
        def off(b):
            pick = mid[torch.randint(0, 7, (31,), generator=g)]
            ulps = torch.randint(1, 4, (31,), generator=g).float() * (torch.randint(0, 2, (31,), generator=g) * 2.0 - 1.0)
            o = pick * (1 + ulps * 2.0 ** -23)
            assert bool((o.bfloat16().float() == pick).all()) and bool((o != pick).all())
            o = o * (torch.randint(0, 2, (31,), generator=g) * 2.0 - 1.0)
            return torch.cat([torch.tensor([-6.0]), o]) * 2.0 ** (b % 6)
        rows.append(tile(off))
        names.append("off-midpoint")
    return torch.stack(rows), names
