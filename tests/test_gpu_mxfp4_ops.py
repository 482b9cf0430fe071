"""GPU: the MXFP4 kernels of csrc/mxfp4/mxfp4.hip on their own, against the torch restatement of the format (tests/fp4_ref.py, pinned on
the CPU by tests/test_mxfp4_host.py): the quantiser's two images in their stated layouts, and the decode GEMM in its three output forms
against float64 on dequant(quant(W)) with the project's own bounds (tests/fp8_ref.py)."""
import functools

import pytest
import torch

from tests import fp4_ref as R
from tests import fp8_ref as F
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

QUANT_SHAPES = [(40, 64), (516, 256), (33, 4608)]
GEMM_SHAPES = [(32, 64, 256, 1), (7, 516, 256, 2), (3, 256, 1024, 8), (32, 2304, 2048, 4), (40, 2048, 8192, 4), (32, 5632, 4608, 2),
               (16, 49157, 2048, 1)]
COL_TILES = (1, 2, 4)                     # every value gemm_skinny_mxfp4_kernel is built for


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sources(N, K, f32):
    """name -> W [N, K] (bfloat16, or float32 for the fp32 source): exact, natural, natural with the designed rows on top."""
    dtype = torch.float32 if f32 else torch.bfloat16
    g = _gen(N * 7 + K + f32)
    rows, _ = R.designed_rows(K, g, f32)
    designed = R.natural_weights(N, K, g, dtype)
    designed[:rows.shape[0]] = rows.to(dtype)
    return {"exact": R.exact_weights(N, K, g, dtype)[0], "natural": R.natural_weights(N, K, g, dtype), "designed": designed}


@pytest.mark.parametrize("f32", [False, True], ids=["bf16-source", "fp32-source"])
@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_quantiser_images_are_the_restatement_in_the_stated_layouts(N, K, f32):
    from starvector_amd import engine as E
    Npad = (N + 31) // 32 * 32
    for name, W in _sources(N, K, f32).items():
        sc, w4, wp = E.op_pack_weight_mxfp4(W.to(dev()))
        sc, w4, wp = sc.cpu(), w4.cpu(), wp.cpu()
        ref_sc, ref_q = R.quantise(W)
        _, ref_d = R.dequantised(W)
        assert torch.equal(sc[:N], ref_sc), (name, "scale bytes")
        assert bool((sc[N:] == 127).all()), (name, "padding rows")
        val, img_sc = R.decode_image_values(w4, None, Npad, K)
        assert torch.equal(img_sc, sc), (name, "scale slots of the decode image")
        assert torch.equal(val[:N], ref_q), (name, "codes of the decode image", int((val[:N] != ref_q).sum()))
        assert not bool(val[N:].any()), (name, "padding rows of the decode image")
        # the bf16 image: dequantised(W) as bf16 (exact), in the packed layout of the bf16 weights (a rounded-to-zero value may keep either sign)
        got = wp[F.wp_index(Npad, K)]
        assert torch.equal(got[:N].double(), ref_d), (name, "bf16 image")
        assert torch.equal(ref_d.bfloat16().double(), ref_d) and not bool(got[N:].float().any()), name
        if name == "exact":
            assert torch.equal(got[:N].double(), W.double())


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """One problem per shape, shared by the tests below: inputs on the device, the float64 references computed once."""
    g = _gen(M + N + K)
    x = torch.randn(M, K, generator=g).bfloat16().to(dev())
    W = R.natural_weights(N, K, g)
    b = (0.1 * torch.randn(N, generator=g)).bfloat16().to(dev())
    sc, Wd = R.dequantised(W.to(dev()))
    xd = x.double()
    return dict(x=x, W=W.to(dev()), b=b, sc=sc, ref=xd @ Wd.T, ref_unq=xd @ W.to(dev()).double().T, Wd=Wd)


@pytest.mark.parametrize("M,N,K,sk", GEMM_SHAPES)
def test_decode_gemm_slabs_against_float64_on_the_dequantised_weights(M, N, K, sk):
    from starvector_amd import engine as E
    c = _case(M, N, K)
    ref = c["ref"] + c["b"].double()
    ys = []
    for ct in COL_TILES:
        y, sc = E.op_linear_skinny_mxfp4(c["x"], c["W"], c["b"], splitk=sk, col_tiles=ct)
        assert torch.equal(sc, c["sc"]), ct
        ys.append(y)
    F.assert_within(ys[0], ref, F.BOUND_F32, f"mxfp4 slabs {M}x{N}x{K} split-K {sk}")
    for ct, y in zip(COL_TILES[1:], ys[1:]):
        assert torch.equal(y, ys[0]), f"col_tiles {ct} moved the bits"
    # discriminating power: the output is the quantised model's, not x W^T with the weights as handed
    unq = c["ref_unq"] + c["b"].double()
    assert F.rel_err(ys[0], unq) > F.rel_err(ys[0], ref), (F.rel_err(ys[0], unq), F.rel_err(ys[0], ref))


@pytest.mark.parametrize("M,N,K,sk", GEMM_SHAPES)
def test_decode_gemm_epilogues_against_float64_on_the_dequantised_weights(M, N, K, sk):
    """The whole-K forms an mxfp4 engine launches for c_fc (bias + GELU, packed activations) and the lm_head (fp32 logits of bf16 values)."""
    from starvector_amd import engine as E
    c = _case(M, N, K)
    lg = [E.op_linear_skinny_epi_mxfp4(c["x"], c["W"], out_f32=True, col_tiles=ct)[0] for ct in COL_TILES]
    F.assert_within(lg[0], c["ref"], F.BOUND_LOGITS, f"mxfp4 logits {M}x{N}x{K}")
    assert torch.equal(lg[0].bfloat16().float(), lg[0])
    for ct, y in zip(COL_TILES[1:], lg[1:]):
        assert torch.equal(y, lg[0]), f"col_tiles {ct} moved the bits"
    if N % 8 == 0:
        ref = F.c_fc_ref(c["x"], c["Wd"], c["b"], "gelu_tanh")
        ys = [E.op_linear_skinny_epi_mxfp4(c["x"], c["W"], c["b"], act="gelu_tanh", col_tiles=ct)[0] for ct in COL_TILES]
        F.assert_within(ys[0], ref, F.BOUND_C_FC, f"mxfp4 c_fc {M}x{N}x{K}")
        for ct, y in zip(COL_TILES[1:], ys[1:]):
            assert torch.equal(y, ys[0]), f"col_tiles {ct} moved the bits"


@pytest.mark.parametrize("N,K,sk", [(516, 256, 2), (2048, 8192, 4)])
def test_rows_do_not_depend_on_the_batch(N, K, sk):
    """Rows 0..6 of a 40-row launch (two row tiles on grid.z) are the 7-row launch's, bit for bit; so are the two epilogue forms'."""
    from starvector_amd import engine as E
    c = _case(40, N, K)
    x40, x7 = c["x"], c["x"][:7].contiguous()
    for ct in COL_TILES:
        a = E.op_linear_skinny_mxfp4(x40, c["W"], c["b"], splitk=sk, col_tiles=ct)[0]
        b = E.op_linear_skinny_mxfp4(x7, c["W"], c["b"], splitk=sk, col_tiles=ct)[0]
        assert torch.equal(a[:7], b), ct
    a = E.op_linear_skinny_epi_mxfp4(x40, c["W"], out_f32=True)[0]
    assert torch.equal(a[:7], E.op_linear_skinny_epi_mxfp4(x7, c["W"], out_f32=True)[0])
    if N % 8:
        return
    a = E.op_linear_skinny_epi_mxfp4(x40, c["W"], c["b"], act="gelu_tanh")[0]
    assert torch.equal(a[:7], E.op_linear_skinny_epi_mxfp4(x7, c["W"], c["b"], act="gelu_tanh")[0])


def test_bad_arguments_are_refused():
    from starvector_amd import engine as E
    x = torch.zeros(4, 192, dtype=torch.bfloat16, device=dev())
    W = torch.zeros(32, 192, dtype=torch.bfloat16, device=dev())
    with pytest.raises(ValueError):
        E.op_linear_skinny_mxfp4(x, W)                                   # K = 192: no cut into whole groups for two waves
    x = torch.zeros(4, 256, dtype=torch.bfloat16, device=dev())
    W = torch.zeros(32, 256, dtype=torch.bfloat16, device=dev())
    with pytest.raises(ValueError):
        E.op_linear_skinny_mxfp4(x, W, col_tiles=3)
    with pytest.raises(ValueError):
        E.op_linear_skinny_mxfp4(x, W, splitk=4)                         # 4 k-steps per block
