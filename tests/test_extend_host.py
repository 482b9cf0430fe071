"""CPU: the extension pass's host side -- the plan as sv_debug_extend_plan states it (chunk schedules, remainder rows, attention tiles, page
groups), the argument checks of the new entry points that need no engine, and the Python plumbing of the row budget.  (The checks that
read the engine's contexts -- B against the cache, ctx + len > total, unknown contexts -- need an engine: tests/test_gpu_extend_ops.py.)"""
import ctypes as C
import os
from unittest import mock

import pytest

from starvector_amd import _lib, engine as E
from starvector_amd.model import StarVectorConfig

SHAPES_1B = {"c_attn": (2048 + 2 * 128, 2048, "none"), "c_proj": (2048, 2048, "none"), "c_fc": (8192, 2048, "gelu_tanh"),
             "down": (2048, 8192, "none")}
TOTALS = [257, 259, 515, 260, 256, 5]
BUDGETS = [32, 100, 256, 258]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _first_rows(lens):
    out, r0 = [], 0
    for n in lens:
        out.append(r0)
        r0 += n
    return out


@pytest.mark.parametrize("budget", [0] + BUDGETS)
def test_chunk_schedules_cover_every_row_exactly_once_and_in_order(budget):
    for lens in (TOTALS, TOTALS[::-1], [300], [1, 1, 1], [64, 64]):
        plan = E.extend_plan([0] * len(lens), lens, None, *SHAPES_1B["c_proj"], budget=budget)
        at, walked = [0] * len(lens), []
        for p in plan:
            rows = sum(n for _, _, n, _ in p["seqs"])
            assert 0 < rows <= (budget or rows), (budget, p)
            assert [b for b, *_ in p["seqs"]] == sorted(b for b, *_ in p["seqs"])
            assert [r for *_, r in p["seqs"]] == _first_rows([n for _, _, n, _ in p["seqs"]])      # packed back to back, in sequence order
            for b, ctx, n, _ in p["seqs"]:
                assert ctx == at[b] and n > 0, (budget, p)       # a pass continues where the last one stopped
                walked += [(b, ctx + j) for j in range(n)]
                at[b] += n
            assert p["fin"] == [b for b, ctx, n, _ in p["seqs"] if ctx + n == lens[b]]
            if budget:                                           # every pass but the last one is full
                assert rows == budget or p is plan[-1], (budget, p)
        assert walked == [(b, j) for b, n in enumerate(lens) for j in range(n)], (budget, lens)
        assert len(plan) == (-(-sum(lens) // budget) if budget else 1)


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", sorted(SHAPES_1B))
def test_remainder_rows_are_those_of_the_one_shot_ragged_plan(name, budget):
    N, K, act = SHAPES_1B[name]
    first = _first_rows(TOTALS)
    want = set(E.ragged_plan(TOTALS, N, K, act)["rows"])         # packed rows of the one-shot pass
    got = set()
    for p in E.extend_plan([0] * len(TOTALS), TOTALS, None, N, K, act, budget=budget):
        for r in p["rows"]:
            b, ctx, n, r0 = next(s for s in p["seqs"] if s[3] <= r < s[3] + s[2])
            got.add(first[b] + ctx + (r - r0))
    assert got == want, (name, budget)
    if name == "down":
        assert want, "the lengths reach the remainder form at this projection"


def test_a_boundary_inside_the_three_peel_rows_of_259():
    N, K, act = SHAPES_1B["c_proj"]
    assert E.gemm_seq_form(259, N, K, act)
    plan = E.extend_plan([0], [259], None, N, K, act, budget=258)
    assert [p["seqs"] for p in plan] == [[(0, 0, 258, 0)], [(0, 258, 1, 0)]]
    assert [p["rows"] for p in plan] == [[256, 257], [0]]       # two peel rows in the first pass, the third is the second pass's only row
    # the stated total decides, not the rows at hand: 258 rows of a 259-row sequence list 256 and 257, the same rows of a 260-row one nothing
    assert E.extend_plan([0], [258], [259], N, K, act)[0]["rows"] == [256, 257]
    assert E.extend_plan([0], [258], [260], N, K, act)[0]["rows"] == []
    assert E.extend_plan([0], [258], None, N, K, act)[0]["rows"] == ([256, 257] if E.gemm_seq_form(258, N, K, act) else [])
    assert E.extend_plan([256], [3], None, N, K, act)[0]["rows"] == [0, 1, 2]
    assert E.extend_plan([258], [1], [300], N, K, act)[0]["rows"] == []


@pytest.mark.parametrize("q_tile", [32, 128])
def test_attention_tiles_start_at_the_tile_that_straddles_the_context(q_tile):
    for ctx, n in ((0, 70), (31, 5), (32, 1), (33, 200), (127, 2), (128, 1), (129, 300), (255, 3)):
        p, = E.extend_plan([ctx], [n], None, *SHAPES_1B["c_attn"], q_tile=q_tile)
        assert p["tiles"] == [(0, t) for t in range(ctx // q_tile, (ctx + n - 1) // q_tile + 1)], (ctx, n, q_tile)
    # context-free sequences first (one ragged launch), then one run of tiles per sequence with a context
    p, = E.extend_plan([40, 0, 100], [30, 50, 1], None, *SHAPES_1B["c_attn"], q_tile=32)
    assert p["tiles"] == [(1, 0), (1, 1), (0, 1), (0, 2), (2, 3)]


def test_page_groups_written():
    for ctx in (31, 32, 33, 63, 64, 65):
        for n in (1, 31, 32, 70):
            p, = E.extend_plan([ctx], [n], None, *SHAPES_1B["c_attn"])
            assert p["groups"] == [(0, g) for g in range(ctx // 32, (ctx + n - 1) // 32 + 1)], (ctx, n)
    p, = E.extend_plan([31, 0, 64], [2, 0, 1], None, *SHAPES_1B["c_attn"])
    assert p["seqs"] == [(0, 31, 2, 0), (2, 64, 1, 2)] and p["groups"] == [(0, 0), (0, 1), (2, 2)]      # a length 0 takes no part


def test_argument_errors_before_any_device_work(lib):
    for name, n_args in (("sv_prefill_open", 3), ("sv_prefill_extend", 7), ("sv_set_prefill_chunk", 2), ("sv_debug_extend_plan", 12),
                         ("sv_debug_kv_gather", 6)):
        assert hasattr(lib, name) and len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert lib.sv_abi_version() == 9

    def err():
        return lib.sv_last_error().decode()
    p = C.c_void_p(16)                                              # never dereferenced: the checks come first
    good, zero, neg = (C.c_int32 * 3)(5, 0, 2), (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(5, -1, 2)
    small = (C.c_int32 * 3)(9, 9, 1)
    assert lib.sv_prefill_extend(None, None, 3, good, None, p, None) == -22 and "null" in err()
    assert lib.sv_prefill_extend(None, p, 3, None, None, p, None) == -22 and "null" in err()
    assert lib.sv_prefill_extend(None, p, 3, good, None, None, None) == -22 and "null" in err()
    assert lib.sv_prefill_extend(None, p, 0, good, None, p, None) == -22 and "B=0" in err()
    assert lib.sv_prefill_extend(None, p, 3, neg, None, p, None) == -22 and "length -1 of sequence 1" in err()
    assert lib.sv_prefill_extend(None, p, 3, zero, None, p, None) == -22 and "every length is 0" in err()
    assert lib.sv_prefill_extend(None, p, 3, good, small, p, None) == -22 and "total length 1 of sequence 2" in err()
    assert lib.sv_prefill_extend(None, p, 3, good, None, p, None) == -22 and "null engine" in err()
    assert lib.sv_prefill_open(None, 3, None) == -22 and "null" in err()
    assert lib.sv_prefill_open(None, 0, good) == -22 and "B=0" in err()
    assert lib.sv_prefill_open(None, 3, good) == -22 and "total length 0 of sequence 1" in err()
    assert lib.sv_prefill_open(None, 3, small) == -22 and "null engine" in err()
    assert lib.sv_set_prefill_chunk(None, 64) == -22 and "null engine" in err()
    assert lib.sv_debug_kv_gather(None, 0, 0, 1, p, None) == -22
    n, buf = C.c_int32(0), (C.c_int32 * 64)()
    args = (2048, 2048, 0, 32, buf)
    assert lib.sv_debug_extend_plan(None, good, None, 3, 0, *args, 64, C.byref(n)) == -22 and "null" in err()
    assert lib.sv_debug_extend_plan(zero, neg, None, 3, 0, *args, 64, C.byref(n)) == -22 and "sequence 1" in err()
    assert lib.sv_debug_extend_plan(good, good, small, 3, 0, *args, 64, C.byref(n)) == -22 and "total" in err()
    assert lib.sv_debug_extend_plan(zero, good, None, 3, -1, *args, 64, C.byref(n)) == -22 and "budget" in err()
    assert lib.sv_debug_extend_plan(zero, good, None, 3, 0, 2048, 2048, 0, 64, buf, 64, C.byref(n)) == -22 and "q_tile" in err()
    assert lib.sv_debug_extend_plan(zero, good, None, 3, 0, *args, 4, C.byref(n)) == -22 and "capacity" in err() and n.value > 4
    assert lib.sv_debug_extend_plan(zero, good, None, 3, 0, *args, 64, C.byref(n)) == 0 and buf[0] == 1


class _Lib:
    def __init__(self):
        self.calls = []

    def sv_set_prefill_chunk(self, h, rows):
        self.calls.append(rows)
        return 0


def test_python_plumbing_config_setter_environment_and_bad_values():
    assert E.EngineConfig().prefill_chunk_rows == 0
    eng = E.HipEngine.__new__(E.HipEngine)
    eng.lib, eng._h = _Lib(), None
    eng.set_prefill_chunk(2048)
    eng.set_prefill_chunk(0)
    assert eng.lib.calls == [2048, 0]
    for bad in (-1, "many", 1.5, True):
        with pytest.raises(ValueError, match="prefill_chunk_rows"):
            eng.set_prefill_chunk(bad)
        with pytest.raises(ValueError, match="prefill_chunk_rows"):
            StarVectorConfig(prefill_chunk_rows=bad)
    assert eng.lib.calls == [2048, 0]
    # the config carries the budget into the engine's config; None = the environment's default, else off
    with mock.patch.dict(os.environ, {}, clear=False):
        os.environ.pop("SV_PREFILL_CHUNK_ROWS", None)
        assert StarVectorConfig().engine_config().prefill_chunk_rows == 0
        assert StarVectorConfig(prefill_chunk_rows=4096).engine_config().prefill_chunk_rows == 4096
        os.environ["SV_PREFILL_CHUNK_ROWS"] = "1024"
        assert StarVectorConfig().engine_config().prefill_chunk_rows == 1024
        assert StarVectorConfig(prefill_chunk_rows=0).engine_config().prefill_chunk_rows == 0
        os.environ["SV_PREFILL_CHUNK_ROWS"] = "-3"
        with pytest.raises(ValueError, match="prefill_chunk_rows"):
            StarVectorConfig()
    # the serving flag
    from starvector_amd import serve
    import inspect
    assert "prefill_chunk_rows" in inspect.signature(serve.ModelWorker.__init__).parameters
