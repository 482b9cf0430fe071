"""The decode output projection's row-half form (csrc/decode_cols.hip gemm_cols_resid_kernel<.., RH = 1>: 16 rows x 16 columns x whole K
per block, grid (N / 16, row halves)) against the 32-row form it replaces (cpb columns x 32 rows per block).  Every output element keeps
its wave's K chunks, its MFMA chain and the wave-order sum, so the two forms must agree BIT FOR BIT -- the op level here (SV_COLS_ROWHALF
= 0 then 1 around two calls of op_decode_proj_fold, the launch counter proving which form ran), the engine level in
tests/test_gpu_cols_rowhalf_engine.py."""
import functools

import pytest
import torch

from starvector_amd import engine as E
from tests.gpu_util import bf

pytestmark = pytest.mark.gpu

F = 64


@functools.lru_cache(maxsize=None)
def _operands(D, Kp):
    """N(0, 1) activations, N(0, 0.02) weights, fixed seeds; built once per shape, on the device, never modified."""
    g = torch.Generator().manual_seed(1000 * D + Kp)
    x = torch.randn(32, Kp, generator=g)
    h = torch.randn(32, D, generator=g)
    Wp = 0.02 * torch.randn(D, Kp, generator=g)
    bp = 0.02 * torch.randn(D, generator=g)
    gam = 1 + 0.1 * torch.randn(D, generator=g)
    bet = 0.1 * torch.randn(D, generator=g)
    Wf = 0.02 * torch.randn(F, D, generator=g)
    bf_ = 0.02 * torch.randn(F, generator=g)
    return tuple(bf(t) for t in (x, h, Wp, bp, gam, bet, Wf, bf_))


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("Kp", [32, 512, 2048])          # 32: one chunk, 15 of the 16 waves have none
@pytest.mark.parametrize("D", [96, 256, 2048])           # 96 = 6 column blocks of 16 (no multiple of 8): stays on the 32-row form
def test_row_half_form_gives_the_bits_of_the_32_row_form(monkeypatch, D, Kp):
    x, h, Wp, bp, gam, bet, Wf, bf_ = _operands(D, Kp)
    takes = D != 96
    for M in (1, 15, 16, 17, 32):                        # the row-half edges
        for bias in (bp, None):
            run = lambda: E.op_decode_proj_fold(x[:M].contiguous(), Wp, bias, h[:M].contiguous(), gam, bet, Wf, bf_)
            monkeypatch.setenv("SV_COLS_ROWHALF", "0")
            n0 = E.cols_rowhalf_launches()
            h2_old, y_old = run()
            n1 = E.cols_rowhalf_launches()
            monkeypatch.setenv("SV_COLS_ROWHALF", "1")
            h2_new, y_new = run()
            n2 = E.cols_rowhalf_launches()
            what = f"M {M} D {D} Kp {Kp} bias {bias is not None}"
            assert n1 == n0, f"{what}: SV_COLS_ROWHALF=0 ran the row-half form"
            halves = 1 if M <= 16 else 2
            want = (n1[0] + 1, n1[1] + halves) if takes else n1
            assert n2 == want, f"{what}: (row-half launches, row halves) went {n1} -> {n2}, expected {want}"
            assert torch.equal(_bits(h2_new), _bits(h2_old)), f"{what}: h2 differs"
            assert torch.equal(_bits(y_new), _bits(y_old)), f"{what}: y differs"
            assert bool(torch.isfinite(h2_new.float()).all()) and bool((h2_new != h[:M]).any())      # (the projection really ran)
