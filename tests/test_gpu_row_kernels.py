"""-m gpu: the row kernels that assemble the prompt and carry the decode residual stream, each on its own through the C ABI (sv_op_*),
against plain torch on the CPU: rowops.hip's im2col, token assembly, embeddings, gathers, ragged positions, adapter norms, the packed
LayerNorm and the decode row update; engine_forward.hip's ragged_positions_kernel; engine_core.hip's pack_rows / unpack_rows.

Conventions of this file
  * every input is exactly representable in its format (bf16 tensors hold bf16 values, the split-K slabs are plain fp32);
  * every output buffer is handed in pre-filled with a sentinel (bf16 0x7FC1, a NaN no kernel here produces; int32 -7) and everything a
    kernel must not write -- padding rows of a fragment-order tile, the gaps a batch / sequence stride leaves, rows behind the last -- must
    still hold it afterwards;
  * fragment-order ("xp") buffers are read with xp_unpack, written here from the layout stated in csrc/common.h, never with
    unpack_rows_kernel;
  * kernels that only move values or add two bf16 numbers are held to the BITS of the reference; kernels that normalise are held, row by
    row, to one bf16 rounding of a float64 reference: max|err| <= 1.1 * 2^-8 * max|ref| over each row (2^-8: the largest relative error of
    one round-to-nearest to bf16; 1.1: the float32 statistics).  Per row, not per tensor: rows differ in scale by design here.
  * the eps cases feed rows of variance 4e-6, where eps = 1e-5 and eps = 1e-6 give outputs a factor 1.67 apart: a kernel (or an engine)
    that read the wrong eps, or none, cannot pass them.  Each first proves on the CPU that the reference with the OTHER eps is at
    least ten bounds away."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from starvector_amd import engine as E
from tests.gpu_util import bf, build_engine, dev, rel_err
from oracle import starvector_oracle as O

pytestmark = pytest.mark.gpu
BF16_1ULP = 2.0 ** -8
SENT = 0x7FC1                 # bf16 sentinel: a quiet NaN with payload 1
SENT_I32 = -7


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.int16).view(torch.bfloat16).to(dev())


def assert_bits(got, ref, what=""):
    """Bit for bit (NaN-safe, signed zeros told apart): `ref` is a bf16 tensor or float32 holding bf16 values."""
    g, r = bits(got).flatten(), bits(ref.to(torch.bfloat16)).flatten()
    assert g.numel() == r.numel(), (what, g.numel(), r.numel())
    bad = (g != r).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at flat index {int(bad[0])}"


def assert_sentinel(t, what=""):
    b = bits(t).flatten()
    bad = (b != SENT).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {b.numel()} elements that must stay untouched were written, first at {int(bad[0])}"


def assert_rows_close(got, ref64, what=""):
    """Every row within one bf16 rounding of the float64 reference, normalised by that row's own maximum."""
    g = got.detach().cpu().double().reshape(-1, got.shape[-1])
    r = ref64.double().reshape(-1, ref64.shape[-1])
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err, bound = (g - r).abs().amax(1), 1.1 * BF16_1ULP * r.abs().amax(1)
    worst = int((err / bound).argmax())
    print(f"[{what}] worst row {worst}: max|err| {float(err[worst]):.3e} = {float(err[worst] / bound[worst]):.3f} x its bound {float(bound[worst]):.3e}")
    assert bool((err <= bound).all()), f"{what}: row {worst} is {float(err[worst] / bound[worst]):.2f} bounds off"


def assert_far(ref_a, ref_b, what=""):
    """CPU only: two references at least ten bounds apart in EVERY row -- the case can tell them apart."""
    a, b = ref_a.double().reshape(-1, ref_a.shape[-1]), ref_b.double().reshape(-1, ref_b.shape[-1])
    gap, bound = (a - b).abs().amax(1), 1.1 * BF16_1ULP * a.abs().amax(1)
    assert bool((gap >= 10 * bound).all()), f"{what}: the case has no power, gap / bound = {float((gap / bound).min()):.2f}"


def xp_index(M, K):
    """csrc/common.h: x[mt*32 + m][k] of a fragment-order buffer with KS = K/16 k-steps sits at
    (((mt*KS + k//16) * 64) + ((k//8) & 1) * 32 + m) * 8 + k % 8."""
    r = torch.arange(M)[:, None]
    k = torch.arange(K)[None, :]
    mt, m, KS = r // 32, r % 32, K // 16
    return (((mt * KS + k // 16) * 64) + ((k // 8) & 1) * 32 + m) * 8 + k % 8


def xp_unpack(buf, M, K):
    return buf.detach().cpu().flatten()[xp_index(M, K)]


def xp_rest(buf, M, K):
    """The elements of the buffer that belong to no row < M."""
    flat = buf.detach().cpu().flatten()
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    keep[xp_index(M, K).flatten()] = False
    return flat[keep]


def xp_pack_cpu(x, total_rows=None):
    """Row-major bf16 [M, K] -> a sentinel-filled fragment-order buffer (CPU, from the stated layout)."""
    M, K = x.shape
    buf = torch.full((E.xp_elems(M if total_rows is None else total_rows, K),), SENT, dtype=torch.int16).view(torch.bfloat16)
    buf[xp_index(M, K).flatten()] = x.to(torch.bfloat16).flatten()
    return buf


def bf_add(a, b):
    return (a.float() + b.float()).bfloat16()


def rnd(g, *shape, std=1.0, mean=0.0):
    return (std * torch.randn(*shape, generator=g) + mean).bfloat16()


def affine(g, *shape):
    return rnd(g, *shape, std=0.1, mean=1.0), rnd(g, *shape, std=0.1)


def ln64(x, w, b, eps):
    return F.layer_norm(x.double(), (x.shape[-1],), w.double(), b.double(), eps)


def small_rows(g, M, D):
    """Zero-mean rows of standard deviation 2e-3 (variance 4e-6, between the two eps values), bf16-exact."""
    x = rnd(g, M, D, std=2e-3)
    var = x.double().var(1, unbiased=False)
    assert float(var.min()) > 3e-6 and float(var.max()) < 5e-6
    return x


EPS_PAIR = [(1e-5, 1e-6), (1e-6, 1e-5)]


# ---- bit-exact kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,P", [(2, 28, 14), (1, 32, 16), (3, 42, 14)])
def test_im2col_is_unfold_with_zero_padding_columns(B, S, P):
    """(2, 28, 14): K = 588 padded to 640, the 52 pad columns exactly +0; (1, 32, 16): K = 768, no padding; (3, 42, 14): a 3 x 3 grid, where
    a py / px or ky / kx swap shows."""
    g = torch.Generator().manual_seed(B * 100 + S)
    K = 3 * P * P
    Kpad = (K + 63) // 64 * 64
    img = rnd(g, B, 3, S, S)
    ref = F.unfold(img.float(), kernel_size=P, stride=P).transpose(1, 2).reshape(-1, K)       # [B * G * G][c * P * P + ky * P + kx]
    out = E.op_im2col(bf(img), P, Kpad, out=sentinel(ref.shape[0] + 1, Kpad))
    assert_bits(out[:-1, :K], ref, "patch columns")
    assert int(bits(out[:-1, K:]).abs().max() if Kpad > K else 0) == 0, "padding columns must be +0"
    assert_sentinel(out[-1], "the row behind the last patch")


@pytest.mark.parametrize("B,S0,D", [(3, 5, 64), (2, 3, 4608)])
def test_dec_embed_adds_the_position_of_a_row_inside_its_sequence(B, S0, D):
    g = torch.Generator().manual_seed(B + S0 + D)
    emb, table = rnd(g, B, S0, D), rnd(g, S0 + 2, D, std=0.3)
    out = E.op_dec_embed(bf(emb), bf(table), out=sentinel(B * S0 + 1, D))
    assert_bits(out[:-1], bf_add(emb, table[:S0][None]), "h")
    assert_sentinel(out[-1])


def test_dec_embed_ragged_rows_take_their_listed_positions():
    g = torch.Generator().manual_seed(9)
    pos = [0, 1, 2, 0, 1, 2, 3, 0, 1]                                          # packed sequences of 3, 4 and 2 rows
    D = 72
    emb, table = rnd(g, 1, len(pos), D), rnd(g, 6, D, std=0.3)
    out = E.op_dec_embed(bf(emb), bf(table), row_pos=torch.tensor(pos, dtype=torch.int32, device=dev()), out=sentinel(len(pos) + 1, D))
    assert_bits(out[:-1], bf_add(emb[0], table[pos]), "h")
    assert_sentinel(out[-1])


def test_gather_rows_plain_and_behind_the_visual_rows_of_a_prompt_buffer():
    g = torch.Generator().manual_seed(11)
    V, D = 11, 72
    table = rnd(g, V, D)
    ids = torch.tensor([0, V - 1, 3, 3, 0, 7], dtype=torch.int64)
    out = E.op_gather_rows(bf(table), ids.to(dev()), out=sentinel(ids.numel() + 1, D))
    assert_bits(out[:-1], table[ids], "plain")
    assert_sentinel(out[-1])
    # P = 2 prompt ids per sequence, written at row T = 3 of every sequence's [S0 = 5][D] block
    B, P, S0, T = 3, 2, 5, 3
    buf = sentinel(B, S0, D)
    E.op_gather_rows(bf(table), ids.to(dev()), per_seq=P, seq_stride=S0 * D, out=buf.view(-1)[T * D:])
    assert_bits(buf[:, T:T + P], table[ids].view(B, P, D), "per-sequence rows")
    assert_sentinel(buf[:, :T], "the visual rows")
    assert_sentinel(buf[:, T + P:], "the rows behind the prompt ids")


def test_gather_last_rows_rectangular_and_ragged():
    g = torch.Generator().manual_seed(12)
    D = 72
    h = rnd(g, 12, D)
    out = E.op_gather_last_rows(bf(h), B=3, S0=4, out=sentinel(4, D))
    assert_bits(out[:3], h[[3, 7, 11]], "rectangular")
    assert_sentinel(out[3])
    lens = [1, 4, 2]                                                           # packed rows 0 | 1..4 | 5..6
    out = E.op_gather_last_rows(bf(h), lens=lens, out=sentinel(4, D))
    assert_bits(out[:3], h[[0, 4, 6]], "ragged")
    assert_sentinel(out[3])


@pytest.mark.parametrize("n_keep", [1, 5])
def test_gather_tail_rows(n_keep):
    g = torch.Generator().manual_seed(13)
    B, S0, D = 2, 5, 72
    h = rnd(g, B, S0, D)
    out = E.op_gather_tail_rows(bf(h), n_keep, out=sentinel(B * n_keep + 1, D))
    assert_bits(out[:-1], h[:, S0 - n_keep:].reshape(-1, D), "tail rows")
    assert_sentinel(out[-1])


def test_gather_listed_rows_unordered_repeated_from_strided_rows():
    g = torch.Generator().manual_seed(14)
    R, ldx, D = 7, 80, 64
    x = rnd(g, R, ldx)
    rows = [5, 0, 5, 2, 6]
    out = E.op_gather_listed_rows(bf(x), torch.tensor(rows, dtype=torch.int32, device=dev()), D, out=sentinel(len(rows) + 1, D))
    assert_bits(out[:-1], x[rows, :D], "listed rows")
    assert_sentinel(out[-1])


def test_ragged_row_pos_and_ragged_positions():
    lens = [300, 1, 7]                                                         # 300 > the 256 threads of a block; a sequence of one row
    total = sum(lens)
    out = torch.full((total + 5,), SENT_I32, dtype=torch.int32, device=dev())
    E.op_ragged_row_pos(lens, out)
    ref = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens])
    assert torch.equal(out[:total].cpu(), ref)
    assert bool((out[total:].cpu() == SENT_I32).all())
    for rep, delta in ((1, 0), (3, -1), (70, 0)):                              # 3 * 70 = 210 entries: more than one 64-thread block
        n = len(lens) * rep
        out = torch.full((n + 5,), SENT_I32, dtype=torch.int32, device=dev())
        E.op_ragged_positions(lens, rep, delta, out)
        ref = torch.tensor(lens, dtype=torch.int32).repeat_interleave(rep) + delta
        assert torch.equal(out[:n].cpu(), ref), (rep, delta)
        assert bool((out[n:].cpu() == SENT_I32).all()), (rep, delta)


@pytest.mark.parametrize("K", [16, 64, 2048])
@pytest.mark.parametrize("M", [1, 32, 33, 64])
def test_pack_rows_and_unpack_rows_follow_the_stated_fragment_layout(M, K):
    g = torch.Generator().manual_seed(M * 3 + K)
    x = rnd(g, M, K)
    xp = E.op_pack_rows(bf(x), out=sentinel(E.xp_elems(M, K) + 16))
    assert_bits(xp_unpack(xp[:-16], M, K), x, "pack_rows against the stated layout")
    assert_sentinel(xp_rest(xp, M, K), "rows >= M of the last tile and the elements behind it")
    # unpack_rows: from a buffer packed HERE (independent of pack_rows_kernel), and the round trip
    y = E.op_unpack_rows(xp_pack_cpu(x).to(dev()), M, K, out=sentinel(M + 1, K))
    assert_bits(y[:M], x, "unpack_rows against the stated layout")
    assert_sentinel(y[M])
    assert_bits(E.op_unpack_rows(xp, M, K), x, "round trip")


# ---- the decode row update ------------------------------------------------------------------------------------------------------
def _row_update_residual(M, D, splitk, ldh, eps=1e-5, slab_std=1.0, h_std=1.5, h_mean=0.3, seed=0):
    """Runs the residual mode; returns (h read back row-major [M, D], the untouched rest of the h buffer, LN output rows, the untouched rest
    of the LN buffer) and the inputs (h0, ws, bias, gamma, beta) on the CPU."""
    g = torch.Generator().manual_seed(seed + M * 31 + D + splitk)
    rows_ws, ldws = (M + 31) // 32 * 32, D + 32           # whole 32-row tiles per slab, as the engine lays its slabs out (MT * 32)
    ws = slab_std * torch.randn(splitk, rows_ws, ldws, generator=g)
    bias = rnd(g, D, std=0.1 * slab_std)
    h0 = rnd(g, M, D, std=h_std, mean=h_mean)
    gam, bet = affine(g, D)
    if ldh:
        hbuf = sentinel(M + 2, D)
        hbuf[:M] = bf(h0)
    else:
        hbuf = xp_pack_cpu(h0).to(dev())
    xp_out = sentinel(E.xp_elems(M, D))
    E.op_row_update_ln(hbuf, bf(gam), bf(bet), xp_out, M, D, eps, ws=ws.to(dev()), bias=bf(bias), ldh=ldh)
    torch.cuda.synchronize()
    if ldh:
        h, h_rest = hbuf[:M].cpu(), hbuf[M:].cpu()
    else:
        h, h_rest = xp_unpack(hbuf, M, D), xp_rest(hbuf, M, D)
    return (h, h_rest, xp_unpack(xp_out, M, D), xp_rest(xp_out, M, D)), (h0, ws, bias, gam, bet)


def _residual_ref(h0, ws, bias, M, D):
    """fp32, the slabs in slab order: h = bf(h + bf(sum_s ws[s] + bias))."""
    v = torch.zeros(M, D)
    for s in range(ws.shape[0]):
        v = v + ws[s, :M, :D]
    return (h0.float() + (v + bias.float()).bfloat16().float()).bfloat16()


@pytest.mark.parametrize("ldh_is_D", [True, False], ids=["rowmajor", "fragment"])
@pytest.mark.parametrize("M,D", [(1, 64), (13, 2048), (33, 2048), (32, 4608), (5, 8192), (2, 9216)])
def test_row_update_residual_mode_sums_the_slabs_in_order(M, D, ldh_is_D):
    """h bit for bit, LayerNorm(h) within one rounding of float64, for 1, 3, 4, 5 and 8 slabs (3 and 5 run the clamped part of the kernel's
    groups of four: a slab summed twice shows as a wrong h).  D <= 2048: 256 threads per row, above: 1024; D = 9216 > 8192 takes that
    kernel's loop over more than one chunk per thread.  Slabs hold rows_ws = 32 * ceil(M / 32) rows of ldws = D + 32 floats: the
    engine's layout (a slab of 32 rows cannot hold the 33rd row of the (33, 2048) case)."""
    for splitk in (1, 3, 4, 5, 8):
        (h, h_rest, y, y_rest), (h0, ws, bias, gam, bet) = _row_update_residual(M, D, splitk, D if ldh_is_D else 0)
        what = f"M {M} D {D} splitk {splitk}"
        href = _residual_ref(h0, ws, bias, M, D)
        assert_bits(h, href, what + ": h")
        assert_sentinel(h_rest, what + ": rows >= M of h")
        assert_sentinel(y_rest, what + ": rows >= M of the LayerNorm output")
        assert_rows_close(y, ln64(href, gam, bet, 1e-5), what + ": LN")


@pytest.mark.parametrize("with_wpe", [True, False], ids=["wpe", "rotary"])
@pytest.mark.parametrize("M,D", [(5, 64), (33, 2048), (3, 4608), (2, 9216)])
def test_row_update_embedding_mode(M, D, with_wpe):
    g = torch.Generator().manual_seed(M + D)
    V, P = 19, 23
    wte, wpe = rnd(g, V, D), rnd(g, P, D, std=0.3)
    tok = torch.randint(0, V, (M,), generator=g)
    tok[0], tok[-1] = V - 1, 0
    pos = torch.randint(0, P, (M,), generator=g)
    pos[0], pos[-1] = P - 1, 0                                                  # not monotone
    gam, bet = affine(g, D)
    href = bf_add(wte[tok], wpe[pos]) if with_wpe else wte[tok]
    yref = ln64(href, gam, bet, 1e-5)
    for ldh in (D, 0):
        hbuf = sentinel(M + 2, D) if ldh else sentinel(E.xp_elems(M, D))
        xp_out = sentinel(E.xp_elems(M, D))
        E.op_row_update_ln(hbuf, bf(gam), bf(bet), xp_out, M, D, 1e-5, ldh=ldh, wte=bf(wte), wpe=bf(wpe) if with_wpe else None,
                           tokens=tok.int().to(dev()), positions=pos.int().to(dev()))
        torch.cuda.synchronize()
        h, h_rest = (hbuf[:M].cpu(), hbuf[M:].cpu()) if ldh else (xp_unpack(hbuf, M, D), xp_rest(hbuf, M, D))
        assert_bits(h, href, f"ldh {ldh}: h")
        assert_sentinel(h_rest, f"ldh {ldh}: rows >= M of h")
        assert_sentinel(xp_rest(xp_out, M, D), f"ldh {ldh}: rows >= M of the LayerNorm output")
        assert_rows_close(xp_unpack(xp_out, M, D), yref, f"ldh {ldh}: LN")


# ---- kernels within one bf16 rounding of float64 ----------------------------------------------------------------------------------
def _vit_embed_case(g, B, NP, Dv, ldp, x_std=1.0):
    patches = rnd(g, B * NP, ldp, std=x_std)
    cls, pos = rnd(g, Dv, std=x_std), rnd(g, NP + 1, Dv, std=0.3 * x_std)
    gam, bet = affine(g, Dv)
    tok = torch.cat([cls.expand(B, 1, Dv), patches[:, :Dv].reshape(B, NP, Dv)], 1)
    v = bf_add(tok, pos[None])                                                  # the reference rounds the sum before ln_pre
    return patches, cls, pos, gam, bet, v


@pytest.mark.parametrize("B,NP,Dv,pad", [(2, 4, 64, 0), (2, 4, 576, 0), (1, 3, 1024, 0), (3, 5, 2048, 0), (2, 4, 576, 64)])
def test_vit_embed_lnpre(B, NP, Dv, pad):
    """(2, 4, 64): 8 chunks, most lanes idle; 576: 72 chunks, the second round partly filled; (3, 5, 2048): the widest row the kernel takes,
    18 rows = 4 full blocks of 4 rows + 2; pad: patch rows ldp = Dv + 64 apart."""
    g = torch.Generator().manual_seed(B + NP + Dv + pad)
    patches, cls, pos, gam, bet, v = _vit_embed_case(g, B, NP, Dv, Dv + pad)
    out = E.op_vit_embed_lnpre(bf(patches), bf(cls), bf(pos), bf(gam), bf(bet), B, NP, Dv, 1e-5, out=sentinel(B * (NP + 1) + 1, Dv))
    assert_rows_close(out[:-1], ln64(v, gam, bet, 1e-5), "ln_pre")
    assert_sentinel(out[-1])


def test_vit_embed_lnpre_refuses_rows_wider_than_its_registers():
    x = sentinel(8, 2056)
    with pytest.raises(ValueError, match="2048"):
        E.op_vit_embed_lnpre(x, x[0], x, x[0], x[0], 1, 1, 2056, 1e-5)
    with pytest.raises(ValueError, match="multiple of 8"):
        E.op_vit_embed_lnpre(x, x[0], x, x[0], x[0], 1, 1, 60, 1e-5)
    with pytest.raises(ValueError, match="% 16"):
        E.op_layernorm_packed(x[:, :40], x[0], x[0])                            # packed outputs: whole k-steps of 16 columns


def _batchnorm_ref(x, w, b, rm, rv, eps):
    c = lambda t: t.double()[None, :, None]
    return (x.double() - c(rm)) / torch.sqrt(c(rv) + eps) * c(w) + c(b)


@pytest.mark.parametrize("B,Q,D", [(2, 5, 64), (3, 257, 128)])
def test_token_batchnorm_running_statistics_per_token(B, Q, D):
    """Running variances from 1e-6 to 4 (log-uniform): for the small ones eps = 1e-5 decides the scale.  Each token's row is scaled to its
    own running deviation, so that every row's output is of order one and a wrong statistic of ONE token is that row's failure."""
    g = torch.Generator().manual_seed(B + Q + D)
    rv = torch.exp(torch.linspace(torch.log(torch.tensor(1e-6)).item(), torch.log(torch.tensor(4.0)).item(), Q))[torch.randperm(Q, generator=g)].bfloat16()
    rm = (rv.float().sqrt() * torch.randn(Q, generator=g)).bfloat16()
    w, b = affine(g, Q)
    x = (rm.float()[None, :, None] + rv.float().sqrt()[None, :, None] * torch.randn(B, Q, D, generator=g)).bfloat16()
    stride = (Q + 2) * D
    out = E.op_token_batchnorm(bf(x), bf(w), bf(b), bf(rm), bf(rv), 1e-5, y_batch_stride=stride, out=sentinel(B, Q + 2, D))
    assert_rows_close(out[:, :Q], _batchnorm_ref(x, w, b, rm, rv, 1e-5), "batch norm")
    assert_sentinel(out[:, Q:], "the gap the batch stride leaves")


def test_plane_layernorm_into_a_strided_prompt_buffer():
    g = torch.Generator().manual_seed(17)
    B, Q, D = 3, 17, 256
    x = rnd(g, B, Q, D, std=2.0, mean=0.5)
    gam, bet = affine(g, Q, D)
    out = E.op_plane_layernorm(bf(x), bf(gam), bf(bet), 1e-5, y_batch_stride=(Q + 2) * D, out=sentinel(B, Q + 2, D))
    ref = F.layer_norm(x.double(), (Q, D), gam.double(), bet.double(), 1e-5)
    assert_rows_close(out[:, :Q], ref, "plane LN")
    assert_sentinel(out[:, Q:], "the gap the batch stride leaves")


@pytest.mark.parametrize("D", [64, 2048])
@pytest.mark.parametrize("M", [1, 5, 33, 64])
def test_layernorm_rows_packed_output(M, D):
    g = torch.Generator().manual_seed(M + D)
    x = rnd(g, M, D, std=2.0, mean=0.5) * torch.logspace(-2, 2, M)[:, None].bfloat16()       # rows of very different scale
    gam, bet = affine(g, D)
    out = E.op_layernorm_packed(bf(x), bf(gam), bf(bet), 1e-5, out=sentinel(E.xp_elems(M, D)))
    assert_rows_close(xp_unpack(out, M, D), ln64(x, gam, bet, 1e-5), "packed LN")
    assert_sentinel(xp_rest(out, M, D), "rows >= M")


# ---- eps: rows of variance 4e-6 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps,other", EPS_PAIR)
@pytest.mark.parametrize("packed", [False, True], ids=["rowmajor", "packed"])
def test_eps_layernorm_rows(packed, eps, other):
    g = torch.Generator().manual_seed(21)
    M, D = 5, 256
    x = small_rows(g, M, D)
    gam, bet = affine(g, D)
    ref = ln64(x, gam, bet, eps)
    assert_far(ref, ln64(x, gam, bet, other), "layernorm_rows")
    if packed:
        got = xp_unpack(E.op_layernorm_packed(bf(x), bf(gam), bf(bet), eps), M, D)
    else:
        got = E.op_layernorm(bf(x), bf(gam), bf(bet), eps)
    assert_rows_close(got, ref, f"eps {eps}")


@pytest.mark.parametrize("eps,other", EPS_PAIR)
def test_eps_plane_layernorm(eps, other):
    g = torch.Generator().manual_seed(22)
    B, Q, D = 2, 5, 64
    x = small_rows(g, B, Q * D).view(B, Q, D)
    gam, bet = affine(g, Q, D)
    ref = lambda e: F.layer_norm(x.double(), (Q, D), gam.double(), bet.double(), e).reshape(B, Q * D)      # one statistic per plane: a row = a plane
    assert_far(ref(eps), ref(other), "plane_layernorm")
    got = E.op_plane_layernorm(bf(x), bf(gam), bf(bet), eps, y_batch_stride=(Q + 2) * D, out=sentinel(B, Q + 2, D))
    assert_rows_close(got[:, :Q].reshape(B, Q * D), ref(eps), f"eps {eps}")


@pytest.mark.parametrize("eps,other", EPS_PAIR)
def test_eps_vit_embed_lnpre(eps, other):
    g = torch.Generator().manual_seed(23)
    B, NP, Dv = 2, 3, 576
    patches, cls, pos, gam, bet, v = _vit_embed_case(g, B, NP, Dv, Dv, x_std=1.9e-3)           # cls / patch + 0.3 x that: variance ~ 4e-6
    var = v.double().var(-1, unbiased=False)
    assert float(var.min()) > 3e-6 and float(var.max()) < 5e-6
    ref = ln64(v, gam, bet, eps)
    assert_far(ref, ln64(v, gam, bet, other), "vit_embed_lnpre")
    got = E.op_vit_embed_lnpre(bf(patches), bf(cls), bf(pos), bf(gam), bf(bet), B, NP, Dv, eps)
    assert_rows_close(got, ref, f"eps {eps}")


@pytest.mark.parametrize("eps,other", EPS_PAIR)
@pytest.mark.parametrize("mode", ["embedding", "residual"])
@pytest.mark.parametrize("D", [256, 4608], ids=["256threads", "1024threads"])
def test_eps_row_update(D, mode, eps, other):
    """Both thread variants, and both places the kernel reads its late arguments from: the embedding mode reads them first, the residual
    mode after its loads are in flight."""
    g = torch.Generator().manual_seed(24 + D)
    M = 3
    if mode == "embedding":
        wte = small_rows(g, 7, D)
        tok = torch.tensor([6, 0, 3])
        gam, bet = affine(g, D)
        href = wte[tok]
        xp_out = sentinel(E.xp_elems(M, D))
        E.op_row_update_ln(sentinel(M, D), bf(gam), bf(bet), xp_out, M, D, eps, ldh=D, wte=bf(wte), tokens=tok.int().to(dev()),
                           positions=torch.zeros(M, dtype=torch.int32, device=dev()))
        got = xp_unpack(xp_out, M, D)
    else:
        # two slabs of deviation 1.4e-3 each on h = 0: the row is bf(sum) of variance ~ 4e-6
        (h, _, got, _), (h0, ws, bias, gam, bet) = _row_update_residual(M, D, 2, D, eps=eps, slab_std=2e-3 / 2 ** 0.5, h_std=0.0, h_mean=0.0, seed=7)
        href = _residual_ref(h0, ws, bias, M, D)
        assert_bits(h, href, "h")
    var = href.double().var(1, unbiased=False)
    assert float(var.min()) > 3e-6 and float(var.max()) < 5e-6, var
    ref = ln64(href, gam, bet, eps)
    assert_far(ref, ln64(href, gam, bet, other), "row_update_ln")
    assert_rows_close(got, ref, f"eps {eps}")


@pytest.mark.parametrize("eps,other", EPS_PAIR)
def test_eps_token_batchnorm(eps, other):
    g = torch.Generator().manual_seed(25)
    B, Q, D = 2, 5, 64
    rv = torch.full((Q,), 4e-6).bfloat16()
    rm = rnd(g, Q, std=1e-3)
    w, b = affine(g, Q)
    x = (rm.float()[None, :, None] + 2e-3 * torch.randn(B, Q, D, generator=g)).bfloat16()
    ref = _batchnorm_ref(x, w, b, rm, rv, eps)
    assert_far(ref, _batchnorm_ref(x, w, b, rm, rv, other), "token_batchnorm")
    got = E.op_token_batchnorm(bf(x), bf(w), bf(b), bf(rm), bf(rv), eps).view(B, Q, D)
    assert_rows_close(got, ref, f"eps {eps}")


@pytest.mark.parametrize("eps,other", EPS_PAIR)
def test_eps_folded_layernorm_of_the_six_launch_layer(eps, other):
    """op_decode_proj_fold with a zero projection: h2 = h (rows of variance 4e-6), y = LN(h2; eps) Wf^T + bf without activation."""
    g = torch.Generator().manual_seed(26)
    M, D, Kp, Fo = 5, 256, 256, 512
    h = small_rows(g, M, D)
    gam, bet = affine(g, D)
    Wf, bf_ = rnd(g, Fo, D, std=D ** -0.5), rnd(g, Fo, std=0.1)
    ref = lambda e: ln64(h, gam, bet, e) @ Wf.double().T + bf_.double()
    assert_far(ref(eps), ref(other), "decode_proj_fold")
    h2, y = E.op_decode_proj_fold(torch.zeros(M, Kp, dtype=torch.bfloat16, device=dev()), torch.zeros(D, Kp, dtype=torch.bfloat16, device=dev()),
                                  torch.zeros(D, dtype=torch.bfloat16, device=dev()), bf(h), bf(gam), bf(bet), bf(Wf), bf(bf_), act="none", eps=eps)
    assert_bits(h2, h, "h2")
    assert_rows_close(y, ref(eps), f"eps {eps}")


def test_siglip_tower_normalises_with_vit_eps_not_ln_eps():
    """The engine hands SigLIP's tower vit_eps (1e-6), every other LayerNorm ln_eps (1e-5): one line of vision_forward.  With the patch embedding
    and the position table scaled by 2^-9 the first layer_norm1 sees rows of variance 3.9e-6 .. 7.0e-6 (mean 4.9e-6), and the oracle run with
    vit_eps := ln_eps lands rel_err = 0.463 from the right one (measured on the CPU; bf16 against fp32 oracle: 0.010) -- 15 times the 3e-2 that
    test_against_reference_goldens allows the encoder output.  The engine must meet the right oracle within that 3e-2 and stay farther than
    that from the swapped one."""
    cfg = dataclasses.replace(O.OracleConfig.tiny_v2(), vit_eps=1e-6, ln_eps=1e-5)
    w = O.make_weights(cfg, seed=4321)
    pe = O.P_VIT + "embeddings."
    for k in ("patch_embedding.weight", "patch_embedding.bias", "position_embedding.weight"):
        w[pe + k] = w[pe + k] * 2.0 ** -9                                        # a power of two: the weights stay bf16-exact
    img = O.synthetic_images(2, cfg.image_size, seed=91)
    x = O._patch_conv(img, w[pe + "patch_embedding.weight"], w[pe + "patch_embedding.bias"], cfg.patch_size).flatten(2).transpose(1, 2)
    var = (x.bfloat16().float() + w[pe + "position_embedding.weight"]).bfloat16().float().var(-1, unbiased=False)
    assert 2e-6 < float(var.min()) and float(var.max()) < 1e-5, (float(var.min()), float(var.max()))
    right = O.image_encoder_forward(w, cfg, img, "bf16")
    swapped = O.image_encoder_forward(w, dataclasses.replace(cfg, vit_eps=cfg.ln_eps), img, "bf16")
    assert rel_err(swapped, right) >= 5 * 3e-2
    eng = build_engine(cfg, w, max_batch=2, max_seq_len=64)
    try:
        enc = eng.encode_image(bf(img))
        torch.cuda.synchronize()
        e_right, e_swapped = rel_err(enc, right), rel_err(enc, swapped)
        print(f"[siglip eps] engine vs oracle {e_right:.3e}, vs the oracle with vit_eps := ln_eps {e_swapped:.3e}")
        assert e_right <= 3e-2, e_right
        assert e_swapped > 3e-2, e_swapped
    finally:
        eng.close()
