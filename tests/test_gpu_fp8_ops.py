"""-m gpu: the fp8 (e4m3) weight paths kernel by kernel -- the quantiser, the big-M kernels' column-scale epilogues (an fp8 engine's
prompt pass), the decode GEMM's c_fc and lm_head epilogues with fp8 weights -- through sv_op_pack_weight_fp8, sv_op_linear_fp8 and
sv_op_linear_skinny_epi_fp8.  The reference side is tests/fp8_ref.py (pinned on the CPU by tests/test_fp8_ops_host.py).

Two kinds of weights:
  (a) exact    W = q * 2^j[n], q random e4m3 values with one +-448 per row: the quantiser returns q and 2^j without rounding, and scaling
               by a power of two commutes with every float32 rounding, so an fp8 operator has to give THE BITS of the bf16 operator
               fed W wherever both sum in the same order.  Neighbouring columns' scales differ by factors of 2 .. 2^16: a scale read
               from another column is a gross error, not one inside a model-level tolerance.
  (b) natural  randn / sqrt(K) times a per-row factor in [0.5, 2], one all-zero row: held to a float64 restatement on
               dequant(quant(W)) built with torch's own float8_e4m3fn cast, inside the project's bounds for the same output form
               (fp8_ref.BOUND_*)."""
import ctypes as C

import pytest
import torch

from starvector_amd import _lib
from starvector_amd import engine as E
from tests import fp8_ref as R
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}[t.dtype])


def _gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def _weights(kind, N, K, g):
    """(W bf16 on the device, scale float32 [N] the op must return, dequantised float64 weight) of kind "exact" / "natural"."""
    if kind == "exact":
        W, q, scale = R.exact_weights(N, K, g, device=dev())
        return W.bfloat16(), scale, q.double() * scale.double()[:, None]
    W = R.natural_weights(N, K, g, device=dev())
    scale, Wd = R.dequantised(W.cpu())                                       # torch's cast on the host
    return W, scale.to(dev()), Wd.to(dev())


def _same_bits(a, b, what):
    ne = _bits(a) != _bits(b)
    if bool(ne.any()):
        first = ne.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} values differ, first at {first}: {a[tuple(first)].item()!r} != {b[tuple(first)].item()!r}")


# ---- the quantiser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["bf16", "f32"])
@pytest.mark.parametrize("N,K", [(33, 64), (516, 256), (520, 320)])
def test_quantiser_images_are_torchs_cast_in_the_stated_layouts(N, K, src):
    """fp8_row_scale_kernel + pack_weight_fp8_kernel as sv_load_weight launches them, both source types.  The scales are amax / 448 (1 for
    the zero row and the padding rows); the decode image, read through the stated layout and torch's float8_e4m3fn view, is torch's cast
    of W / scale by value (+-0 compare equal); the bf16 image holds the same values element for element; padding rows are zero.  Rows:
    natural weights (fp32 source: not rounded to bf16), 8 rows of exact weights, and fp8_ref.designed_quantiser_rows (ties on normal and
    subnormal midpoints, an outlier, a negative maximum and, fp32 source, values a few ulps off a midpoint that are no bf16 numbers)."""
    g = torch.Generator().manual_seed(N * 3 + K + (src == "f32"))
    f32 = src == "f32"
    W = R.natural_weights(N, K, g, dtype=torch.float32 if f32 else torch.bfloat16).float()
    W[8:16] = R.exact_weights(8, K, g)[0]
    rows, names = R.designed_quantiser_rows(K, g, f32)
    W[16:16 + len(names)] = rows
    W = W if f32 else W.bfloat16()
    assert f32 or torch.equal(W[16:16 + len(names)].float(), rows)           # the designed rows are exact in bf16
    sc, wq, wp = (t.cpu() for t in E.op_pack_weight_fp8(W.to(dev())))
    Npad = (N + 31) // 32 * 32
    ref_sc, ref_q = R.quantise(W)
    assert float(ref_sc[3]) == 1.0 and not bool(ref_q[3].any())
    assert torch.equal(sc[:N], ref_sc), (sc[:N] != ref_sc).nonzero()[:4]
    assert bool((sc[N:] == 1).all())
    codes = wq[R.wq_index(Npad, K)]                                           # [Npad, K] uint8
    assert not bool(((codes & 0x7F) == 0x7F).any()), "a NaN code"
    got_q = codes.view(torch.float8_e4m3fn).float()
    for i, name in enumerate(names):
        bad = (got_q[16 + i] != ref_q[16 + i]).nonzero().flatten().tolist()
        assert not bad, f"row '{name}': {len(bad)} codes differ from RNE, first k = {bad[0]}: W / scale = {float(W[16 + i, bad[0]].float() / ref_sc[16 + i])!r} -> {float(got_q[16 + i, bad[0]])}, expected {float(ref_q[16 + i, bad[0]])}"
    assert torch.equal(got_q[:N], ref_q), (got_q[:N] != ref_q).nonzero()[:4]
    got_p = wp[R.wp_index(Npad, K)].float()
    assert torch.equal(got_p, got_q)                                          # the prefill image = the decode image, element for element
    assert not bool(codes[N:].any()) and not bool(_bits(wp[R.wp_index(Npad, K)])[N:].any())


# ---- the big-M kernels' column-scale epilogues ------------------------------------------------------------------------------------
def _big_m_case(M, N, K, act, res, out_f32, forms, seq=0, seed=0):
    """op_linear_fp8 under every form of `forms` (sv_debug_set_gemm_form; -1 = the tuned choice) with the sequence structure `seq`
    (sv_debug_set_linear_seq_rows), both kinds of weights.  (a): the bits of op_linear on W in the same form; (b): inside the bounds.
    All forms agree bit for bit (as the bf16 forms do: test_gpu_ops.py), the returned scales are the reference's.  Returns the outputs."""
    g = _gen(M + N + K + seed)
    x = torch.randn(M, K, generator=g, device=dev()).bfloat16()
    b = None if out_f32 else (0.1 * torch.randn(N, generator=g, device=dev())).bfloat16()
    r = torch.randn(M, N, generator=g, device=dev()).bfloat16() if res else None
    outs = {}
    for kind in ("exact", "natural"):
        W, scale, Wd = _weights(kind, N, K, g)
        try:
            E.set_linear_seq_rows(seq)
            for form in forms:
                E.set_gemm_form(form)
                y, sc = E.op_linear_fp8(x, W, b, r, act=act, out_f32=out_f32)
                assert torch.equal(sc, scale), (kind, form)
                outs[kind, form] = y
                if kind == "exact":
                    _same_bits(y, E.op_linear(x, W, b, r, act=act, out_f32=out_f32), f"exact weights, form {form}: fp8 op vs bf16 op")
        finally:
            E.set_gemm_form(-1)
            E.set_linear_seq_rows(0)
        for form in forms[1:]:
            _same_bits(outs[kind, form], outs[kind, forms[0]], f"{kind} weights: form {form} vs form {forms[0]}")
        if seq <= 0:
            R.assert_within(outs[kind, forms[0]], R.linear_ref(x, Wd, b, r, act, out_f32), R.BOUND_F32 if out_f32 else R.BOUND_BIG_M,
                            f"big-M {kind} M={M} N={N} K={K} act={act} res={res} f32={out_f32}")
        outs[kind, "operands"] = (x, W, b, r, Wd)
    return outs


@pytest.mark.parametrize("N,act,res,out_f32", [(520, "none", False, False), (520, "gelu_tanh", False, False), (520, "none", True, False),
                                               (520, "gelu_tanh", True, False), (516, "none", True, False), (516, "gelu_tanh", False, False),
                                               (520, "none", False, True)])
def test_big_m_kernels_apply_the_column_scale(N, act, res, out_f32):
    """M = 326, K = 320 under forms 0 (gemm_bf16_kernel), 1 (gemm256_kernel), 2 (256 rows of it + 70 rows through gemm_tail_kernel) and
    the tuned choice.  N = 520 (N % 8 == 0) takes the tile kernels' LDS-strip epilogue, N = 516 their register epilogue, out_f32 the
    fp32 stores; with and without activation and residual."""
    _big_m_case(326, N, 320, act, res, out_f32, forms=(1, 0, 2, -1))


@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16_residual", "f32"])
def test_big_m_rows_a_sequence_leaves_over_its_tiles_with_the_column_scale(out_f32):
    """B = 3 sequences of S = 258 rows, N = K = 1024: the per-sequence form holds (asserted), so rows 256, 257 of every sequence take
    gemm_tailk_kernel (K split over 8 waves).  (a) the bits of op_linear on W with the same sequence structure; (b) inside the bounds;
    the compact form (the sequences' last rows on their own, set_linear_seq_rows(-S)) gives those rows' bits.  bf16 output with bias and
    residual as the engine's projections; the fp32 output shows that the remainder rows did take the other kernel: their bits differ
    from the call without the sequence structure (another summation order), which six rows of bf16 values cannot show."""
    B, S, N, K = 3, 258, 1024, 1024
    assert E.gemm_seq_form(S, N, K, "none")
    outs = _big_m_case(B * S, N, K, "none", not out_f32, out_f32, forms=(-1,), seq=S)
    for kind in ("exact", "natural"):
        x, W, b, r, Wd = outs[kind, "operands"]
        y = outs[kind, -1]
        R.assert_within(y, R.linear_ref(x, Wd, b, r, "none", out_f32), R.BOUND_F32 if out_f32 else R.BOUND_BIG_M,
                        f"big-M per-sequence form, {kind}, f32={out_f32}")
        plain = E.op_linear_fp8(x, W, b, r, out_f32=out_f32)[0]
        yb, pb = _bits(y).view(B, S, N), _bits(plain).view(B, S, N)
        assert torch.equal(yb[:, :256], pb[:, :256])                          # rows inside full tiles: the tile kernels' bits
        if out_f32:
            assert not torch.equal(yb[:, 256:], pb[:, 256:])
        xc = x.view(B, S, K)[:, -1].contiguous()
        rc = None if r is None else r.view(B, S, N)[:, -1].contiguous()
        try:
            E.set_linear_seq_rows(-S)
            yc = E.op_linear_fp8(xc, W, b, rc, out_f32=out_f32)[0]
            if kind == "exact":
                _same_bits(yc, E.op_linear(xc, W, b, rc, out_f32=out_f32), "compact last rows: fp8 op vs bf16 op")
        finally:
            E.set_linear_seq_rows(0)
        _same_bits(yc, y.view(B, S, N)[:, -1], f"compact last rows vs the full problem, {kind}")


def test_big_m_tuned_choice_with_the_column_scale():
    """(4136, 1032, 512) is above the tuner's threshold (M >= 1024, M * N >= 2^22): its key carries the column scale, so an fp8 Linear is
    timed and chosen apart from the bf16 one.  Whatever it picks gives the bits of form 1."""
    _big_m_case(4136, 1032, 512, "none", False, False, forms=(1, -1))


# ---- the decode GEMM's epilogues with fp8 weights ---------------------------------------------------------------------------------
ROWS = (1, 7, 32, 33, 40, 64)
FORMS = (0, 2, 3, 1)                 # sv_debug_set_skinny_form: the 33..64-row kernels (1 = the default, restored last)
COL_TILES = (1, 2, 3)


def _waves(rows, N, K, fp8):
    out = (C.c_int32 * 2)()
    E.check(_lib.load().sv_debug_skinny_plan(rows, N, K, 1, int(fp8), out), "sv_debug_skinny_plan")
    return int(out[0])


def _calls(op, rows, every_form):
    """As tests/test_gpu_batch_invariance.py: (label, first row, output) of the first M rows at every M of `rows` -- above 32 rows under
    every kernel form and column-tile count when every_form, else under the default form and every column-tile count at 64 rows --
    and of rows 32..63 as a call of their own."""
    for M in rows:
        if M <= 32:
            yield f"M={M}", 0, op(slice(0, M))
            continue
        try:
            for form in (FORMS if every_form else (1,)):
                E.set_skinny_form(form)
                for ct in (COL_TILES if every_form or M == 64 else (0,)):
                    E.set_op_col_tiles(ct)
                    yield f"M={M} form={form} col_tiles={ct}", 0, op(slice(0, M))
        finally:
            E.set_op_col_tiles(0)
            E.set_skinny_form(1)
    yield "rows 32..63", 32, op(slice(32, 64))


def _assert_rows_invariant(op, rows, every_form):
    """Every row has the same bits in every call that contains it; returns the 64-row result of the default form."""
    full = op(slice(0, 64))
    ref_bits = _bits(full)
    bad = []
    for label, r0, out in _calls(op, rows, every_form):
        same = (_bits(out) == ref_bits[r0:r0 + out.shape[0]]).all(dim=1)
        if not bool(same.all()):
            rws = [r0 + i for i in torch.nonzero(~same).flatten().tolist()]
            diff = int((_bits(out) != ref_bits[r0:r0 + out.shape[0]]).sum())
            bad.append(f"{label}: rows {rws[:6]}{'...' if len(rws) > 6 else ''} differ from the 64-row call ({diff} values)")
    assert not bad, "a row's bits depend on its batch or on the kernel form:\n  " + "\n  ".join(bad)
    return full


def _decode_case(N, K, act, rows, every_form, seed=0):
    """op_linear_skinny_epi_fp8 in the c_fc form (act given: bias, bf16, activation, bf16, fragment order) or the logits form (act None:
    bf16-rounded fp32 logits), both kinds of weights: every row the same bits in every call; the returned scales are the reference's;
    inside the bounds of the form; the logits are bf16 values.  (a) where sv_debug_skinny_plan gives bf16 and fp8 weights the same number
    of waves (K is cut the same way inside a block): the bits of op_linear_skinny_epi on W, at 64 and at 32 rows."""
    logits = act is None
    g = _gen(N + K + seed)
    x = torch.randn(64, K, generator=g, device=dev()).bfloat16()
    b = None if logits else (0.1 * torch.randn(N, generator=g, device=dev())).bfloat16()
    compared = 0
    for kind in ("exact", "natural"):
        W, scale, Wd = _weights(kind, N, K, g)

        def op(r):
            y, sc = E.op_linear_skinny_epi_fp8(x[r].contiguous(), W, b, act=act or "none", out_f32=logits)
            assert torch.equal(sc, scale), kind
            return y
        full = _assert_rows_invariant(op, rows, every_form)
        if logits:
            assert torch.equal(full, full.bfloat16().float())
            R.assert_within(full, x.double() @ Wd.T, R.BOUND_LOGITS, f"decode logits {kind} N={N} K={K}")
        else:
            R.assert_within(full, R.c_fc_ref(x, Wd, b, act), R.BOUND_C_FC, f"decode c_fc {act} {kind} N={N} K={K}")
        if kind == "exact":
            for M in (64, 32):
                if _waves(M, N, K, False) == _waves(M, N, K, True):
                    _same_bits(full[:M], E.op_linear_skinny_epi(x[:M].contiguous(), W, b, act=act or "none", out_f32=logits),
                               f"exact weights, {M} rows: fp8 op vs bf16 op")
                    compared += 1
    return compared


SMALL = [(N, K, act) for K in (256, 512, 1024, 2112, 2176) for N, act in ((5128, "gelu_tanh"), (5129, None), (520, "gelu_tanh"), (520, None))]
SMALL += [(5128, K, "none") for K in (256, 1024, 2112)]


@pytest.mark.parametrize("N,K,act", SMALL, ids=lambda v: str(v))
def test_decode_epilogues_with_fp8_weights_small_shapes(N, K, act):
    """M in 1, 7, 32, 33, 40, 64; above 32 rows every kernel form (0, 2, 3, 1) x column tiles (1, 2, 3).  K = 256: 8 waves of 2 k-steps,
    the register-only two-tile kernel (gemm_skinny_mt2_kernel<8, true, *>); K = 512 / 1024: the LDS-ring kernel at chunk depths 2 / 4
    (gemm_skinny_mt2x_kernel<true, *, 2 | 4>: scale and bias of the block's column tiles through LDS); K = 2112: 2 waves -- no two-tile
    kernel, gemm_skinny_fp8_kernel<2> with its long steady-state loop on both row tiles; K = 2176: 4 waves (gemm_skinny_fp8_kernel<4>,
    gemm_skinny_mt2_kernel<4, true, 1>).  <= 32 rows: gemm_skinny_fp8_kernel<8 | 4 | 2>.  N = 5128 / 5129: a ragged last column tile (and
    a ragged last block at 2 and 3 column tiles per block); N = 520: few blocks.

    Exact weights against the bf16 operator: the plans agree (8 waves both) at N = 5128 / 5129 with K = 256, 512, 1024, and there the bits
    ARE equal -- both kernels give wave w the k-steps [w * KS / 8, (w + 1) * KS / 8) in ascending order, add the waves' accumulators in
    wave order and share the epilogue (sk_store); the fp8 kernels scale each wave's accumulator before that sum, which a power of two
    commutes with.  At K = 2112 / 2176 fp8 weights take half the waves (a lane's 16 bytes hold two k-steps) and at N = 520 bf16 weights
    take 16 (a narrow output): another summation order by design, so only the tolerance holds there."""
    compared = _decode_case(N, K, act, ROWS, every_form=True)
    assert compared == (2 if N > 520 and K <= 1024 else 0)


ENGINE = [("8b c_fc", 18432, 4608, "gelu_tanh"), ("8b lm_head", 49157, 4608, None), ("1b c_fc", 8192, 2048, "gelu_tanh"),
          ("1b lm_head", 49156, 2048, None)]


@pytest.mark.parametrize("name,N,K,act", ENGINE, ids=[e[0] for e in ENGINE])
def test_decode_epilogues_with_fp8_weights_engine_shapes(name, N, K, act):
    """StarVector-8B's and -1B's c_fc and lm_head (BASELINE config 5 runs them at 64 rows): 32 and 64 rows in the default form, column
    tiles 1 .. 3 at 64.  Both plans are 8 waves here, so with exact weights the bits equal the bf16 operator's (the bf16 lm_head of
    StarVector-1B takes the persistent-block kernel, bit-identical to the one-tile kernel: test_gpu_ops.py)."""
    assert _decode_case(N, K, act, (32, 64), every_form=False, seed=1) == 2
