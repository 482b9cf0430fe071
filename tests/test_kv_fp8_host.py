"""CPU: the e4m3 KV cache's rule as tests/kv8_ref.py restates it, pinned on designed rows; the argument errors of sv_create_kv / sv_kv_info
that need no GPU; the page and pool arithmetic."""
import ctypes as C
import dataclasses

import pytest
import torch

from tests import fp8_ref, kv8_ref as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("D", [64, 128])
def test_exact_rows_are_reproduced(D):
    x, codes, j = R.exact_rows(64, D, _g(1), j_lo=-100, j_hi=100)
    q, E = R.quant(x.bfloat16())
    assert torch.equal(E, j)
    # (a -0 element keeps its sign bit; +-0 are the two zero codes)
    assert torch.equal(q, codes)
    assert R.same_bits(R.deq(q, E), x.bfloat16())


def test_the_cast_sends_every_midpoint_to_the_even_code():
    mid = fp8_ref.e4m3_midpoints()
    assert mid.numel() == 126
    for sign in (1.0, -1.0):
        c = R.cast(mid * sign).int() & 0x7F
        lo = torch.arange(126)
        even = torch.where(lo % 2 == 0, lo, lo + 1)
        assert torch.equal(c, even.int())
    assert int(R.cast(torch.tensor([1e9]))[0]) == 0x7E and int(R.cast(torch.tensor([-1e9]))[0]) == 0xFE      # the clamp


@pytest.mark.parametrize("D", [64, 128])
def test_tie_rows_round_to_even_under_the_row_scale(D):
    x = R.tie_rows(D, _g(2), j=-3)
    q, E = R.quant(x.bfloat16())
    assert bool((E == -3).all())
    assert bool(((q[:, 1:].int() & 1) == 0).all()), "a midpoint went to the odd code"
    tab = fp8_ref.e4m3_table()
    # the scaled element is the mean of the chosen code and one of its neighbours: it really was a tie
    c = q[:, 1:].long() & 0x7F
    y = x[:, 1:].abs().double() * 2.0 ** 3
    mean_lo = (tab[c].double() + tab[(c - 1).clamp(min=0)].double()) / 2
    mean_hi = (tab[c].double() + tab[c + 1].double()) / 2
    assert bool(((y == mean_lo) | (y == mean_hi)).all()) and bool((y != tab[c].double()).all())


def test_special_rows():
    x, names = R.special_rows(128, _g(3))
    q, E = R.quant(x.bfloat16())
    by = dict(zip(names, range(len(names))))
    assert E.tolist() == [11 - 7, 0, exp_of(x[by["inf and nan"]]), -120, 113, 120], E.tolist()
    d = R.deq(q, E).float()
    # outlier: the row maximum is exact; the others (|x| < 4, scaled by 2^-4 into the binade below 2^-2, whose step is 2^-6) are off by
    # half of 2^-6 * 2^4 at most, and some land on the subnormals or zero
    o = by["outlier"]
    assert float(d[o, 128 // 3]) == -3.5 * 2.0 ** 10
    assert float((d[o] - x[o]).abs().max()) <= 2.0 ** (4 - 6) / 2 and int((q[o].int() & 0x7F == 0).sum()) > 0
    assert bool((q[by["all zero"]] == 0).all()) and bool((d[by["all zero"]] == 0).all())
    n = by["inf and nan"]
    bad = ~torch.isfinite(x[n])
    assert int(bad.sum()) == 3 and bool((q[n][bad] == R.NAN_CODE).all()) and bool(torch.isnan(d[n][bad]).all())
    assert bool(torch.isfinite(d[n][~bad]).all()) and bool((q[n][~bad].int() & 0x7F != 0x7F).all())
    # the clamps: the maximum of each row survives exactly
    assert float(d[by["amax 2^-126"], 5]) == 2.0 ** -126 and float(d[by["amax 2^120"], 7]) == 2.0 ** 120
    assert float(d[by["amax 1.5 * 2^127"], 9]) == -1.5 * 2.0 ** 127
    for k in ("amax 2^-126", "amax 2^120", "amax 1.5 * 2^127"):
        assert bool(torch.isfinite(d[by[k]]).all())
    # nothing saturates: no code of a finite element is +-448 unless its scaled value is
    fin = torch.isfinite(x)
    assert bool(((q.int() & 0x7F)[fin] <= 0x78).all())
    # every dequantised value is a bf16 number by construction (deq returns bf16); the relative error of a normal code is 2^-4 at most
    big = fin & (x.abs() >= torch.ldexp(torch.ones(()), E[:, None] - 6).float())
    assert float(((d - x).abs() / x.abs())[big].max()) <= 2.0 ** -4


def exp_of(row):
    fin = row[torch.isfinite(row)]
    return int(torch.floor(torch.log2(fin.abs().max().double()))) - 7


def test_random_rows_error_bound():
    x = (torch.randn(256, 128, generator=_g(4)) * torch.logspace(-3, 3, 256)[:, None]).bfloat16()
    d = R.deq_quant(x)
    amax = x.float().abs().amax(-1, keepdim=True)
    # scaled values below 256 sit at most half of the top binade's step (16 / 2) from a code: 8 / 128 of amax at worst
    assert float(((d.float() - x.float()).abs() / amax).max()) <= 8.0 / 128


def test_create_kv_argument_errors_need_no_gpu():
    import __graft_entry__ as ge
    ge.build()
    from starvector_amd import _lib
    lib = _lib.load()
    err = lambda: lib.sv_last_error().decode()
    h = C.c_void_p()
    c = _lib.SvConfig()
    lib.sv_config_default_1b(C.byref(c))
    assert lib.sv_create_kv(None, 1, C.byref(h)) == -22 and "null" in err()
    assert lib.sv_create_kv(C.byref(c), 1, None) == -22
    for bad in (-1, 2, 7):
        assert lib.sv_create_kv(C.byref(c), bad, C.byref(h)) == -22 and "kv_dtype" in err(), err()
    c.vit_width = 1000                                       # the configuration checks of sv_create run for both formats
    assert lib.sv_create_kv(C.byref(c), 1, C.byref(h)) == -22 and lib.sv_create_kv(C.byref(c), 0, C.byref(h)) == -22
    assert lib.sv_kv_info(None, None, None, None) == -22 and "null" in err()
    assert lib.sv_debug_kv_read(None, 0, 0, 0, 1, None, None) == -22
    if not torch.cuda.is_available():
        lib.sv_config_default_1b(C.byref(c))
        assert lib.sv_create_kv(C.byref(c), 1, C.byref(h)) == -5 and "hipSetDevice" in err()


def test_page_and_pool_arithmetic():
    import starvector_amd as sva
    from starvector_amd.engine import kv_page_bytes, kv_pool_bytes, resolve_kv_dtype
    assert kv_page_bytes("bf16", 128) == 32768 and kv_page_bytes("fp8_e4m3", 128) == 16512
    assert kv_page_bytes("bf16", 64) == 16384 and kv_page_bytes("fp8", 64) == 8320
    for cfg in (sva.EngineConfig(), sva.EngineConfig.starvector_8b(max_batch=64),
                sva.EngineConfig(hidden=1024, n_head=16, n_inner=4096, max_batch=3, max_seq_len=130)):       # head_dim 128, 128, 64
        b = kv_pool_bytes(dataclasses.replace(cfg, kv_dtype="bf16"))
        f = kv_pool_bytes(dataclasses.replace(cfg, kv_dtype="fp8_e4m3"))
        dh = cfg.hidden // cfg.n_head
        assert f * (2 * dh) == b * (dh + 1)                  # 129 / 256 at head_dim 128, 65 / 128 at 64
        assert f <= 0.51 * b
    one = sva.EngineConfig(max_batch=32, max_seq_len=2048)
    assert kv_pool_bytes(one) == 24 * (32 * 32 + 1) * 32768
    assert resolve_kv_dtype("auto") == "bf16" and resolve_kv_dtype("fp8") == "fp8_e4m3" and resolve_kv_dtype("FP8_E4M3") == "fp8_e4m3"
    with pytest.raises(ValueError):
        resolve_kv_dtype("int8")


def test_python_surfaces_take_the_format(monkeypatch):
    from starvector_amd.engine import resolve_kv_dtype
    from starvector_amd.model import StarVectorConfig
    monkeypatch.delenv("SV_KV_DTYPE", raising=False)
    assert StarVectorConfig().engine_config().kv_dtype == "bf16"
    assert StarVectorConfig(kv_cache_dtype="fp8").engine_config().kv_dtype == "fp8_e4m3"
    monkeypatch.setenv("SV_KV_DTYPE", "fp8")
    assert resolve_kv_dtype(None) == "fp8_e4m3" and StarVectorConfig().engine_config().kv_dtype == "fp8_e4m3"
    assert StarVectorConfig(kv_cache_dtype="bf16").engine_config().kv_dtype == "bf16"
    from starvector_amd import vllm
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        vllm.LLM("nowhere", kv_cache_dtype="int8")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        vllm.LLM("nowhere", kv_cache_dtype="bf16")           # vLLM's own spelling of the default is "auto"
