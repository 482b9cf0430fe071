"""CPU: the MXFP4 restatement of tests/fp4_ref.py pins itself (the GPU tests hold the quantiser and the decode GEMM to it), the stated
layouts are bijections, the exactness the mode's contract rests on, and the plumbing that makes the format reachable: EngineConfig,
StarVectorConfig / from_pretrained, vllm.LLM(quantization=), serve --weight-dtype, the environment default, the C ABI's plan entry points."""
import ctypes as C

import pytest
import torch

from tests import fp4_ref as R
from tests.fp8_ref import wp_index


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_exact_weights_come_back_unchanged(dtype):
    W, q, E = R.exact_weights(40, 256, _gen(1), dtype)
    sc, qq = R.quantise(W)
    assert torch.equal(sc.long() - 127, E) and torch.equal(qq, q)
    assert torch.equal(R.dequantised(W)[1], W.double())


def test_every_midpoint_goes_to_the_even_code_with_both_signs():
    tab = R.e2m1_table()
    mid = torch.tensor(R.E2M1_MIDPOINTS, dtype=torch.float64)
    want = torch.tensor(R.E2M1_TIE_GOES_TO, dtype=torch.float64)
    assert torch.equal(tab[R.round_e2m1_index(mid)], want)
    assert torch.equal((tab[:-1] + tab[1:]) / 2, mid)                       # they ARE the midpoints of the table
    idx = R.round_e2m1_index(mid)
    assert bool((idx % 2 == 0).all())                                        # even index = even mantissa bit
    eps = 2.0 ** -40
    assert torch.equal(R.round_e2m1_index(mid - eps), torch.arange(7)) and torch.equal(R.round_e2m1_index(mid + eps), torch.arange(7) + 1)
    for j in (-3, 0, 5):                                                     # through quantise, next to a 6 that fixes the exponent
        row = torch.cat([torch.tensor([6.0]), mid.float(), -mid.float(), torch.zeros(17)]) * 2.0 ** j
        sc, q = R.quantise(row[None].bfloat16())
        assert int(sc[0, 0]) == 127 + j
        assert torch.equal(q[0, 1:8], want) and torch.equal(q[0, 8:15], -want)


def test_saturation_zero_blocks_and_exponent_clamps():
    row = torch.zeros(1, 64)
    row[0, 0], row[0, 1], row[0, 2] = 7.96875, -7.0, 6.5                      # amax / 2^E in [4, 8): above 6 saturates
    sc, q = R.quantise(row.bfloat16())
    assert sc.tolist() == [[127, 127]]                                      # E = 0; the all-zero block: byte 127, codes 0
    assert q[0, :3].tolist() == [6.0, -6.0, 6.0] and not bool(q[0, 32:].any())
    tiny = torch.full((1, 64), 2.0 ** -140, dtype=torch.float32)              # fp32 subnormal: E clamps to -125, everything rounds to 0
    sc, q = R.quantise(tiny)
    assert sc.tolist() == [[2, 2]] and not bool(q.any())
    big = torch.full((1, 64), 2.0 ** 127, dtype=torch.float32)
    sc, q = R.quantise(big)
    assert sc.tolist() == [[252, 252]] and bool((q == 4.0).all())            # E = 125, 2^127 / 2^125


def test_designed_rows_are_what_their_names_say():
    for f32 in (False, True):
        rows, names = R.designed_rows(256, _gen(2), f32)
        assert names[:4] == ["midpoints", "outlier", "negative max", "saturate"] and (len(names) == 5) == f32
        if not f32:
            assert torch.equal(rows.bfloat16().float(), rows)
        sc, q = R.quantise(rows if f32 else rows.bfloat16())
        assert set(q[1].abs().unique().tolist()) <= {0.0, 0.5, 4.0}          # the outlier's neighbours land on 0 and 0.5
        assert bool((q[3].abs() == 6.0).all())
        if f32:
            # rounding the source to bf16 first lands on the midpoints: a different (wrong) answer for a good share of the elements
            _, q16 = R.quantise(rows.bfloat16())
            assert float((q16[4] != q[4]).float().mean()) > 0.3


@pytest.mark.parametrize("Npad,K", [(64, 64), (32, 256), (544, 256)])
def test_the_layouts_are_bijections_onto_the_image(Npad, K):
    byte, shift = R.w4_code_index(Npad, K)
    nib = (byte * 2 + shift // 4).flatten()
    sc = R.w4_scale_index(Npad, K).flatten()
    groups = Npad // 32 * (K // 64)
    assert R.image_bytes(Npad, K) == groups * 1088
    assert nib.unique().numel() == Npad * K and sc.unique().numel() == Npad * K // 32
    used = torch.zeros(R.image_bytes(Npad, K), dtype=torch.int32)
    used.index_add_(0, byte.flatten(), torch.ones(Npad * K, dtype=torch.int32))
    used.index_add_(0, sc, torch.full((sc.numel(),), 2, dtype=torch.int32))
    assert bool((used == 2).all())                                           # two nibbles or one scale byte in every byte: 4.25 bits / weight
    assert R.image_bytes(Npad, K) * 8 / (Npad * K) == 4.25
    wp = wp_index(Npad, K).flatten()
    assert wp.unique().numel() == Npad * K and int(wp.max()) == Npad * K - 1
    # a lane's 16-byte load: four k-steps of 8 codes of ONE row, two MX blocks
    lane0 = (byte // 16 == byte[0, 0] // 16).nonzero()
    assert lane0[:, 0].unique().tolist() == [0] and sorted(lane0[:, 1].tolist()) == [16 * u + e for u in range(4) for e in range(8)]


def test_dequantised_natural_weights_are_bf16_numbers():
    for dtype in (torch.bfloat16, torch.float32):
        W = R.natural_weights(48, 512, _gen(3), dtype)
        sc, Wd = R.dequantised(W)
        assert torch.equal(Wd.bfloat16().double(), Wd)
        assert int(sc[0, 1]) == 127 and bool((sc[3] == 127).all()) and not bool(Wd[3].any())
        err = (Wd - W.double()).abs().view(48, -1, 32).amax(-1)
        amax = W.double().abs().view(48, -1, 32).amax(-1)
        assert bool((err <= amax / 4).all())                                 # half a step of the coarsest grid (2 * 2^E <= amax / 2), saturation included


def test_codes_round_trip_through_the_image_reader():
    W, q, E = R.exact_weights(32, 128, _gen(4))
    img = torch.zeros(R.image_bytes(32, 128), dtype=torch.uint8)
    byte, shift = R.w4_code_index(32, 128)
    img.index_put_((byte.flatten(),), (R.codes_of(q).long() << shift).flatten().to(torch.uint8), accumulate=True)
    img[R.w4_scale_index(32, 128)] = (E + 127).to(torch.uint8)
    val, sc = R.decode_image_values(img, None, 32, 128)
    assert torch.equal(val, q) and torch.equal(sc.long() - 127, E)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def test_engine_config_names_and_codes(monkeypatch):
    from starvector_amd import engine as E
    assert E.WEIGHT_DTYPES == {"bf16": 0, "fp8_e4m3": 1, "mxfp4": 2}
    assert [E.weight_dtype_code(n) for n in ("bf16", "fp8_e4m3", "fp8", "mxfp4", "MXFP4")] == [0, 1, 1, 2, 2]
    with pytest.raises(ValueError, match="weight_dtype"):
        E.resolve_weight_dtype("int4")
    monkeypatch.delenv("SV_WEIGHT_DTYPE", raising=False)
    assert E.resolve_weight_dtype(None) == "bf16"
    monkeypatch.setenv("SV_WEIGHT_DTYPE", "mxfp4")
    assert E.resolve_weight_dtype(None) == "mxfp4" and E.resolve_weight_dtype("bf16") == "bf16"
    monkeypatch.setenv("SV_WEIGHT_DTYPE", "nonsense")
    with pytest.raises(ValueError):
        E.resolve_weight_dtype(None)


def test_starvector_config_routes_the_format(monkeypatch):
    from starvector_amd.model import StarVectorConfig, config_from_checkpoint
    monkeypatch.delenv("SV_WEIGHT_DTYPE", raising=False)
    assert StarVectorConfig().engine_config().weight_dtype == "bf16"
    assert StarVectorConfig(weight_dtype="mxfp4").engine_config().weight_dtype == "mxfp4"
    assert StarVectorConfig(weight_dtype="fp8").engine_config().weight_dtype == "fp8_e4m3"
    v2 = StarVectorConfig(starcoder_model_name="bigcode/starcoder2-7b", image_encoder_type="siglip_384", weight_dtype="mxfp4")
    assert v2.engine_config().weight_dtype == "mxfp4"
    assert config_from_checkpoint({"weight_dtype": "mxfp4"}, {}).engine_config().weight_dtype == "mxfp4"
    with pytest.raises(ValueError, match="weight_dtype"):
        StarVectorConfig(weight_dtype="int4")
    monkeypatch.setenv("SV_WEIGHT_DTYPE", "fp8")
    assert StarVectorConfig().engine_config().weight_dtype == "fp8_e4m3"
    assert StarVectorConfig(weight_dtype="bf16").engine_config().weight_dtype == "bf16"          # the argument wins


class _Captured(Exception):
    pass


def test_from_pretrained_hands_the_format_to_the_engine(tmp_path, monkeypatch):
    from oracle import starvector_oracle as O
    from starvector_amd import model as M
    from tests.ckpt_util import write_reference_checkpoint
    cfg = O.OracleConfig.tiny()
    write_reference_checkpoint(str(tmp_path / "ckpt"), cfg, O.make_weights(cfg, seed=5))
    seen = []

    class Engine:
        def __init__(self, ecfg, device=None):
            seen.append(ecfg.weight_dtype)
            raise _Captured()

    monkeypatch.setattr(M, "HipEngine", Engine)
    monkeypatch.delenv("SV_WEIGHT_DTYPE", raising=False)
    for kw, want in (({}, "bf16"), ({"weight_dtype": "mxfp4"}, "mxfp4"), ({"weight_dtype": "fp8"}, "fp8_e4m3")):
        with pytest.raises(_Captured):
            M.StarVectorForCausalLM.from_pretrained(str(tmp_path / "ckpt"), byte_tokenizer_fallback=True, **kw)
        assert seen[-1] == want
    monkeypatch.setenv("SV_WEIGHT_DTYPE", "mxfp4")
    with pytest.raises(_Captured):
        M.StarVectorForCausalLM.from_pretrained(str(tmp_path / "ckpt"), byte_tokenizer_fallback=True)
    assert seen[-1] == "mxfp4"


def test_llm_quantization_routing_and_value_error(monkeypatch):
    from starvector_amd import model as M
    from starvector_amd import vllm as V
    seen = []

    def from_pretrained(path, tokenizer=None, **kw):
        seen.append(kw)
        raise _Captured()

    monkeypatch.setattr(M.StarVectorForCausalLM, "from_pretrained", staticmethod(from_pretrained))
    for q, want in ((None, None), ("fp8", "fp8_e4m3"), ("mxfp4", "mxfp4")):
        with pytest.raises(_Captured):
            V.LLM("/nowhere", quantization=q, max_num_seqs=4)
        assert seen[-1].get("weight_dtype") == want and seen[-1]["max_batch"] == 4
    n = len(seen)
    for bad in ("awq", "int4", "FP8", ""):
        with pytest.raises(ValueError, match="quantization"):
            V.LLM("/nowhere", quantization=bad)
    assert len(seen) == n                                                   # refused before anything is loaded


def test_serve_flag_reaches_the_loader(monkeypatch):
    from starvector_amd import serve as S
    seen = []

    def load(path, device="cuda", **kw):
        seen.append(kw)
        raise _Captured()

    monkeypatch.setattr(S, "load_pretrained_model", load)
    for wd, want in ((None, {}), ("mxfp4", {"weight_dtype": "mxfp4"})):
        with pytest.raises(_Captured):
            S.ModelWorker("http://c", "http://w", "id", True, "/nowhere/starvector-x", weight_dtype=wd)
        assert seen[-1] == want
    import inspect
    assert "--weight-dtype" in inspect.getsource(S.main)


def test_abi_plan_entry_points_take_the_format():
    from starvector_amd import _lib
    lib = _lib.load()
    out = (C.c_int32 * 2)()
    # waves are a function of (K, split-K) only: the same at 1, 33 and 64 rows; never two row tiles per block
    for K, sk, waves in ((256, 1, 4), (256, 2, 2), (1024, 8, 2), (2048, 4, 8), (4608, 2, 4), (4608, 1, 8), (18432, 8, 4), (18432, 4, 8), (192, 1, 0)):
        for rows in (1, 33, 64):
            assert lib.sv_debug_skinny_plan(rows, 2048, K, sk, 2, out) == 0
            assert (out[0], out[1]) == (waves, 0), (K, sk, rows, out[0], out[1])
    assert lib.sv_debug_skinny_plan(1, 2048, 256, 1, 3, out) != 0                # unknown format
    for rows in (1, 16, 33, 64):
        for N, K, whole in ((2304, 2048, 0), (2048, 8192, 0), (8192, 2048, 1), (4608, 18432, 0), (18432, 4608, 1), (49157, 2048, 1)):
            assert lib.sv_debug_decode_plan(rows, N, K, 2, whole, 256, out) == 0
            assert out[1] in (1, 2, 4) and (not whole or out[0] == 1)
            assert lib.sv_debug_skinny_plan(rows, N, K, out[0], 2, (C.c_int32 * 2)()) == 0
            w = (C.c_int32 * 2)()
            lib.sv_debug_skinny_plan(rows, N, K, out[0], 2, w)
            assert w[0] in (2, 4, 8)                                           # the plan's split-K has a kernel
    for name in ("sv_op_pack_weight_mxfp4", "sv_op_linear_skinny_mxfp4", "sv_op_linear_skinny_epi_mxfp4"):
        assert name in _lib.DEBUG_PROTOTYPES and hasattr(lib, name)
