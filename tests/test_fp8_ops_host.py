"""CPU: the reference side of tests/test_gpu_fp8_ops.py holds by itself (tests/fp8_ref.py) -- the weight constructions do what
their docstrings claim under torch's own e4m3 cast, the stated layouts of the quantiser's images are the kernels' thread maps, and
a float32 emulation of each fp8-weight operator (exact products, float32 accumulation, the kernels' rounding points) sits inside
the bounds the GPU tests hold the kernels to."""
import pytest
import torch

from tests import fp8_ref as R


def test_torch_cast_is_rne_subnormals_included_and_saturates_above_the_tests_range():
    t = R.e4m3_table()
    finite = t[:0x7F]
    assert bool((finite[1:] > finite[:-1]).all()) and float(finite[-1]) == 448.0 and float(finite[1]) == 2.0 ** -9
    mid = R.e4m3_midpoints()
    code = mid.to(torch.float8_e4m3fn).view(torch.uint8).int()
    lo = torch.arange(126)
    assert torch.equal(code, lo + (lo & 1))                                   # the even one of (c, c + 1)
    up, down = torch.nextafter(mid, torch.tensor(1e9)), torch.nextafter(mid, torch.tensor(-1e9))
    assert torch.equal(up.to(torch.float8_e4m3fn).view(torch.uint8).int(), lo + 1)
    assert torch.equal(down.to(torch.float8_e4m3fn).view(torch.uint8).int(), lo)
    assert torch.equal((-mid).to(torch.float8_e4m3fn).float(), -mid.to(torch.float8_e4m3fn).float())
    # amax / 448 rounds, so |W| / scale can exceed 448 by an ulp: still 448 (torch gives NaN only from 464 on)
    edge = torch.tensor([448.0 * (1 + 2.0 ** -23), 463.9]).to(torch.float8_e4m3fn).float()
    assert edge.tolist() == [448.0, 448.0]


@pytest.mark.parametrize("N,K", [(33, 64), (520, 320)])
def test_exact_weights_quantise_without_rounding(N, K):
    g = torch.Generator().manual_seed(N + K)
    W, q, scale = R.exact_weights(N, K, g)
    assert torch.equal(W.bfloat16().float(), W)                                # exact in bf16
    assert bool((q.abs().amax(1) == 448).all()) and bool((q == 0).any()) and bool(((q != 0) & (q.abs() < 2.0 ** -6)).any())
    sc, qq = R.quantise(W.bfloat16())
    assert torch.equal(sc, scale) and torch.equal(qq, q)
    assert len(set(scale.tolist())) > 8 and float(scale.max() / scale.min()) >= 2.0 ** 12


@pytest.mark.parametrize("K", [64, 256, 320])
def test_designed_rows_have_power_of_two_scales_and_bite(K):
    g = torch.Generator().manual_seed(K)
    rows, names = R.designed_quantiser_rows(K, g, f32=True)
    assert names == ["ties", "outlier", "negative max", "off-midpoint"]
    sc, q = R.quantise(rows)
    assert sc.tolist() == [2.0 ** -3, 8.0, 2.0 ** -6, 32.0]
    assert torch.equal(rows[:3].bfloat16().float(), rows[:3]) and not torch.equal(rows[3].bfloat16().float(), rows[3])
    t = R.e4m3_table()
    # ties: every element but the first sits half-way between two codes, and the chosen code is even
    x = (rows[0] / sc[0])[1:].abs()
    code = q[0, 1:].abs().to(torch.float8_e4m3fn).view(torch.uint8).int()
    assert bool((code % 2 == 0).all())
    other = torch.where(t[code] > x, code - 1, code + 1)
    assert torch.equal((t[code] - x).abs(), (t[other] - x).abs())
    assert int((x < 2.0 ** -6).sum()) >= 7                                    # the subnormal midpoints are in every row
    # outlier: the other elements land below 0.5, some on subnormals, some on zero
    rest = torch.cat([q[1, : K // 3], q[1, K // 3 + 1:]]).abs()
    assert float(q[1, K // 3]) == -448 and float(rest.max()) <= 0.4375 and bool((rest < 2.0 ** -6).any())
    assert float(q[2, K - 5]) == -448
    # off-midpoint: rounding the source to bf16 first gives another code for about half of the elements
    early = R.quantise(rows[3:].bfloat16())[1][0]
    assert 0.25 * K < int((early != q[3]).sum()) < 0.75 * K


def _kernel_maps(Npad, K):
    """The thread maps of pack_weight_kernel / pack_weight_fp8_kernel as loops, element by element (csrc/gemm_pack.hip)."""
    KS = K // 16
    wp = torch.empty(Npad, K, dtype=torch.long)
    wq = torch.empty(Npad, K, dtype=torch.long)
    for nt in range(Npad // 32):
        for ks in range(KS):
            for lane in range(64):
                n, k0 = nt * 32 + (lane & 31), ks * 16 + (lane >> 5) * 8
                c = (nt * KS + ks) * 64 + lane                                 # one 16-byte chunk of 8 bf16 per (tile, k-step, lane)
                i = (nt * (KS // 2) + ks // 2) * 64 + lane                     # one 16-byte chunk of 16 codes per (tile, k-step pair, lane)
                for e in range(8):
                    wp[n, k0 + e] = c * 8 + e
                    wq[n, k0 + e] = i * 16 + (ks & 1) * 8 + e
    return wp, wq


@pytest.mark.parametrize("Npad,K", [(32, 64), (64, 128), (96, 320)])
def test_stated_layouts_are_the_kernels_thread_maps(Npad, K):
    wp, wq = _kernel_maps(Npad, K)
    assert torch.equal(R.wp_index(Npad, K), wp) and torch.equal(R.wq_index(Npad, K), wq)
    for idx in (wp, wq):
        assert torch.equal(idx.flatten().sort().values, torch.arange(Npad * K))


def _emulate(x, q, scale, bias):
    """What every fp8-weight kernel computes up to summation order: float32 sum of the exact products x * q, times the row scale, plus bias."""
    y = (x.float() @ q.T) * scale
    return y if bias is None else y + bias.float()


@pytest.mark.parametrize("kind", ["exact", "natural"])
def test_float32_emulation_of_the_operators_sits_inside_the_bounds(kind):
    M, N, K = 326, 520, 320
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).bfloat16()
    b = (0.1 * torch.randn(N, generator=g)).bfloat16()
    r = torch.randn(M, N, generator=g).bfloat16()
    W = R.exact_weights(N, K, g)[0].bfloat16() if kind == "exact" else R.natural_weights(N, K, g)
    scale, q = R.quantise(W)
    Wd = R.dequantised(W)[1]
    y = _emulate(x, q, scale, b)
    gelu = R.ACTS["gelu_tanh"]
    R.assert_within(_emulate(x, q, scale, None), R.linear_ref(x, Wd, out_f32=True), R.BOUND_F32, f"{kind} fp32 out")
    R.assert_within(y.bfloat16(), R.linear_ref(x, Wd, b), R.BOUND_BIG_M, f"{kind} big-M")
    got = (gelu(y.bfloat16().float()).bfloat16().float() + r.float()).bfloat16()
    R.assert_within(got, R.linear_ref(x, Wd, b, r, "gelu_tanh"), R.BOUND_BIG_M, f"{kind} big-M gelu + residual")
    R.assert_within(gelu(y[:64].bfloat16().float()).bfloat16(), R.c_fc_ref(x[:64], Wd, b, "gelu_tanh"), R.BOUND_C_FC, f"{kind} c_fc")
    lg = _emulate(x[:64], q, scale, None).bfloat16().float()
    R.assert_within(lg, x[:64].double() @ Wd.T, R.BOUND_LOGITS, f"{kind} logits")
