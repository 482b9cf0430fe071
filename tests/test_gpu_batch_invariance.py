"""-m gpu: a row's decode result does not depend on the batch around it.

The continuous-batching engine (engine_cb.hip), sv_generate and the two-row-tile kernels all rely on this rule.  Every decode GEMM
changes kernel at the 32 / 33-row boundary (launch_gemm_skinny: the one-tile kernel, the persistent lm_head or the c_fc tail split
at <= 32 rows; gemm_skinny_mt2* at 33..64), so a kernel that sums in another order on one side gives a row other bits when its
batch grows past 32.  Tokens and tolerance checks cannot see that; these tests compare bits (through integer views, so that NaN and
-0.0 count too) for every row across calls of 1 .. 64 rows, and keep each result inside the operator tolerances of test_gpu_ops.py
against a float64 restatement, so that a kernel that is consistently wrong cannot pass either.

Operator level: the real decode Linears of StarVector-1B / -8B, each form the engine runs (split-K partials with the engine's own
split factor, the c_fc epilogue with and without the tail split, the lm_head's fp32 logits and its folded arg-max, fp8 weights),
every 33..64-row kernel form and column-tile count.  Engine level: teacher-forced prefill + decode logits at B = 1 / 32 / 33 / 64
(8B dimensions bf16 and fp8, 1B dimensions), and a continuous batch whose bucket grows from 32 to 64 rows under a live request."""
import ctypes as C
import dataclasses

import pytest
import torch

from oracle import starvector_oracle as O
from oracle.hostinfo import host_cores
from starvector_amd import _lib
from starvector_amd import engine as E
from tests.gpu_util import build_engine, dev

pytestmark = pytest.mark.gpu
BF16_1ULP = 2.0 ** -8

# (N, K) of the decode Linears (W [N][K]): c_attn, c_proj, c_fc (gelu_tanh), down projection, lm_head
LINEARS = {
    "1b": {"c_attn": (2304, 2048), "c_proj": (2048, 2048), "c_fc": (8192, 2048), "down": (2048, 8192), "lm_head": (49156, 2048)},
    "8b": {"c_attn": (5632, 4608), "c_proj": (4608, 4608), "c_fc": (18432, 4608), "down": (4608, 18432), "lm_head": (49157, 4608)},
}
ROWS = (1, 7, 31, 32, 33, 40, 63, 64)
FORMS = (0, 2, 3, 1)                 # sv_debug_set_skinny_form: the 33..64-row kernels (1 = the default, restored last)
COL_TILES = (1, 2, 3)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan_splitk(N, K, fp8=False, whole_k=False):
    """The split-K factor sv_create picks for this Linear in a 64-row engine (sv_debug_decode_plan)."""
    out = (C.c_int32 * 2)()
    E.check(_lib.load().sv_debug_decode_plan(64, N, K, int(fp8), int(whole_k), _cus(), out), "sv_debug_decode_plan")
    return int(out[0])


def _operands(N, K, seed):
    g = torch.Generator(device=dev()).manual_seed(seed)
    x = torch.randn(64, K, generator=g, device=dev()).bfloat16()
    W = (torch.randn(N, K, generator=g, device=dev()) / K ** 0.5).bfloat16()
    b = (0.1 * torch.randn(N, generator=g, device=dev())).bfloat16()
    return x, W, b


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _mean(got, ref):
    return float((got.double() - ref).abs().mean() / ref.abs().max())


def _calls(op):
    """op(rows) -> output of a call on those rows of the 64-row x.  Yields (label, first row, output) for the first M rows at every
    M in ROWS -- at 33..64 rows under every kernel form and column-tile count -- and for rows 32..63 as a call of their own."""
    for M in ROWS:
        if M <= 32:
            yield f"M={M}", 0, op(slice(0, M))
            continue
        try:
            for form in FORMS:
                E.set_skinny_form(form)
                for ct in COL_TILES:
                    E.set_op_col_tiles(ct)
                    yield f"M={M} form={form} col_tiles={ct}", 0, op(slice(0, M))
        finally:
            E.set_op_col_tiles(0)
            E.set_skinny_form(1)
    yield "rows 32..63", 32, op(slice(32, 64))


def _assert_rows_invariant(op):
    """Every row has the same bits in every call that contains it; returns the 64-row result of the default form."""
    full = op(slice(0, 64))
    ref_bits = _bits(full)
    bad = []
    for label, r0, out in _calls(op):
        same = (_bits(out) == ref_bits[r0:r0 + out.shape[0]]).all(dim=1)
        if not bool(same.all()):
            rows = [r0 + i for i in torch.nonzero(~same).flatten().tolist()]
            diff = int((_bits(out) != ref_bits[r0:r0 + out.shape[0]]).sum())
            bad.append(f"{label}: rows {rows[:6]}{'...' if len(rows) > 6 else ''} differ from the 64-row call ({diff} values)")
    assert not bad, "a row's bits depend on its batch:\n  " + "\n  ".join(bad)
    return full


CASES = [(m, l) for m in ("1b", "8b") for l in ("c_attn", "c_proj", "c_fc", "down")]


@pytest.mark.parametrize("model,lin", CASES)
def test_split_k_partials_do_not_depend_on_the_batch(model, lin):
    """op_linear_skinny (fp32 slabs + the fixed-order split-K reduction) with the engine's split factor."""
    N, K = LINEARS[model][lin]
    sk = _plan_splitk(N, K)
    x, W, b = _operands(N, K, seed=N + K + 1)
    full = _assert_rows_invariant(lambda r: E.op_linear_skinny(x[r].contiguous(), W, b, splitk=sk))
    ref = x.double() @ W.double().T + b.double()
    assert _rel(full, ref) <= 1e-5, (sk, _rel(full, ref))


@pytest.mark.parametrize("model,lin", CASES)
def test_fp8_weight_partials_do_not_depend_on_the_batch(model, lin):
    """op_linear_skinny_fp8 (its own <= 32-row kernel, the two-row-tile kernels' fp8 path at 33..64) with the engine's split factor."""
    N, K = LINEARS[model][lin]
    sk = _plan_splitk(N, K, fp8=True)
    x, W, b = _operands(N, K, seed=N + K + 2)
    scales = {}

    def op(r):
        y, sc = E.op_linear_skinny_fp8(x[r].contiguous(), W, b, splitk=sk)
        scales.setdefault("sc", sc)
        return y
    full = _assert_rows_invariant(op)
    Wc = W.float().cpu()                                  # the scales as test_gpu_fp8.py states them (IEEE division on the host)
    amax = Wc.abs().amax(1)
    ref_sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert torch.equal(scales["sc"].cpu(), ref_sc)
    q = (Wc / ref_sc[:, None]).to(torch.float8_e4m3fn).double() * ref_sc[:, None].double()
    ref = x.double() @ q.to(dev()).T + b.double()
    assert _rel(full, ref) < 2e-5, (sk, _rel(full, ref))


@pytest.mark.parametrize("tailsplit", ["1", "0"])
@pytest.mark.parametrize("act", ["gelu_tanh", "none"])
@pytest.mark.parametrize("model", ["1b", "8b"])
def test_c_fc_epilogue_does_not_depend_on_the_batch(model, act, tailsplit, monkeypatch):
    """op_linear_skinny_epi, the c_fc form (bias, bf16, activation, bf16 into the packed activations): StarVector-8B's c_fc at
    <= 32 rows takes the tail split for the tiles beyond 2 x CUs with SV_TAILSPLIT=1 (off by default); at 33..64 rows it never does."""
    monkeypatch.setenv("SV_TAILSPLIT", tailsplit)
    N, K = LINEARS[model]["c_fc"]
    x, W, b = _operands(N, K, seed=N + K + 3)
    full = _assert_rows_invariant(lambda r: E.op_linear_skinny_epi(x[r].contiguous(), W, b, act=act))
    y = (x.double() @ W.double().T + b.double()).bfloat16().float()
    if act == "gelu_tanh":
        y = torch.nn.functional.gelu(y, approximate="tanh")
    y = y.double()
    assert _rel(full, y) <= 2.2 * BF16_1ULP and _mean(full, y) <= 1.5e-3, (_rel(full, y), _mean(full, y))


@pytest.mark.parametrize("model", ["1b", "8b"])
def test_lm_head_logits_and_selection_do_not_depend_on_the_batch(model):
    """op_linear_skinny_epi(out_f32): the lm_head's bf16-rounded fp32 logits (the persistent lm_head at one and two row tiles, the
    two-row-tile kernels).  op_lm_head_argmax (<= 32 rows): its logits are the same bits, and its folded arg-max is torch.argmax of
    the same rows' logits from a 33-row call."""
    V, K = LINEARS[model]["lm_head"]
    x, W, _ = _operands(V, K, seed=V + K + 4)
    full = _assert_rows_invariant(lambda r: E.op_linear_skinny_epi(x[r].contiguous(), W, out_f32=True))
    ref = x.double() @ W.double().T
    assert torch.equal(full, full.bfloat16().float())
    assert _rel(full, ref) <= 1.1 * BF16_1ULP, _rel(full, ref)
    lg33 = E.op_linear_skinny_epi(x[:33].contiguous(), W, out_f32=True)
    for M in (1, 7, 31, 32):
        lg, idx = E.op_lm_head_argmax(x[:M].contiguous(), W)
        assert torch.equal(_bits(lg), _bits(full[:M])), M
        assert torch.equal(idx, lg33[:M].argmax(-1).cpu()), M


def test_tail_split_runs_at_32_rows_only_and_gives_the_one_tile_bits(monkeypatch):
    """The launch counter of the tail split (sv_debug_tailsplit_launches) proves which side ran: StarVector-8B's c_fc at 32 rows takes
    it, at 33 rows and with SV_TAILSPLIT=0 it does not -- and all three give every row the same bits."""
    if _cus() != 256:
        pytest.skip("the split is sized on 2 x 256 block slots")
    N, K = LINEARS["8b"]["c_fc"]
    x, W, b = _operands(N, K, seed=N + K + 5)
    run = lambda M: E.op_linear_skinny_epi(x[:M].contiguous(), W, b, act="gelu_tanh")
    monkeypatch.setenv("SV_TAILSPLIT", "1")
    n0 = E.tailsplit_launches()
    split32 = run(32)
    n1 = E.tailsplit_launches()
    two33 = run(33)
    n2 = E.tailsplit_launches()
    monkeypatch.setenv("SV_TAILSPLIT", "0")
    one32 = run(32)
    n3 = E.tailsplit_launches()
    assert (n1 - n0, n2 - n1, n3 - n2) == (1, 0, 0)
    assert torch.equal(_bits(split32), _bits(one32))
    assert torch.equal(_bits(split32), _bits(two33[:32]))


# ---- engine level -----------------------------------------------------------------------------------------------------------
S0, STEPS = 40, 6


@pytest.fixture(scope="module")
def w8():
    torch.set_num_threads(host_cores())
    cfg = dataclasses.replace(O.OracleConfig.starvector_8b(), n_layer=1, vit_layers=1, eos_token_id=-1)
    return cfg, O.make_weights(cfg, seed=83)


def _teacher_forced_rows_invariant(eng, vocab, seed):
    ids = torch.randint(0, 4000, (64, S0), generator=torch.Generator().manual_seed(seed))
    toks = torch.randint(0, 4000, (64, STEPS), generator=torch.Generator().manual_seed(seed + 1), dtype=torch.int64)
    emb = eng.embed_tokens(ids.to(dev()))
    runs = {}
    for B in (64, 1, 32, 33):
        out = [eng.prefill(emb[:B].contiguous())]
        for t in range(STEPS):
            out.append(eng.decode_step(toks[:B, t].to(dev())))
        runs[B] = torch.stack(out)                     # [1 + STEPS, B, vocab]
    full = runs[64]
    assert full.shape == (1 + STEPS, 64, vocab) and bool(torch.isfinite(full).all())
    assert float(full.abs().max()) > 0
    bad = []
    for B in (1, 32, 33):
        diff = (_bits(runs[B]) != _bits(full[:, :B])).any(dim=2)      # [step, row]
        for t, r in torch.nonzero(diff).tolist():
            bad.append(f"B={B} {'prefill' if t == 0 else f'step {t}'} row {r}")
    assert not bad, "logits depend on the batch: " + ", ".join(bad[:12]) + (f" ... ({len(bad)})" if len(bad) > 12 else "")


@pytest.mark.parametrize("weight_dtype", ["bf16", "fp8_e4m3"])
def test_engine_8b_dims_teacher_forced_logits_do_not_depend_on_the_batch(w8, weight_dtype):
    """A 64-row engine at StarVector-8B's dimensions (one decoder layer): prefill and 6 teacher-forced decode steps at B = 1 / 32 / 33
    / 64 on the same 64 prompts and tokens -- every row's fp32 logits bit-identical in every batch that contains it."""
    cfg, w = w8
    eng = build_engine(cfg, w, max_batch=64, max_seq_len=64, weight_dtype=weight_dtype)
    try:
        _teacher_forced_rows_invariant(eng, cfg.vocab, seed=84)
    finally:
        eng.close()


def test_engine_1b_dims_teacher_forced_logits_do_not_depend_on_the_batch():
    """The same at StarVector-1B's dimensions, two decoder layers (the 6-launch layer, the fused MLP launch where the engine takes it)."""
    torch.set_num_threads(host_cores())
    cfg = dataclasses.replace(O.OracleConfig(), n_layer=2, vit_layers=1, eos_token_id=-1)
    w = O.make_weights(cfg, seed=85)
    eng = build_engine(cfg, w, max_batch=64, max_seq_len=64)
    try:
        _teacher_forced_rows_invariant(eng, cfg.vocab, seed=86)
    finally:
        eng.close()


def test_continuous_batch_growing_past_32_rows_keeps_a_live_request_on_its_solo_tokens(w8):
    """Request A runs alone for two steps, then 32 more join (the bucket grows from 32 to 64 rows while A is live) and leave again:
    A's greedy tokens equal `generate` of A alone."""
    cfg, w = w8
    eng = build_engine(cfg, w, max_batch=64, max_seq_len=64)
    try:
        ids = torch.randint(0, 4000, (33, S0), generator=torch.Generator().manual_seed(87))
        emb = eng.embed_tokens(ids.to(dev()))
        n_new = 20
        solo = eng.generate(emb[:1].contiguous(), max_length=S0 + n_new, eos_token_id=-1, pad_token_id=0).cpu()[0]
        assert solo.numel() == n_new
        a = eng.cb_admit(emb[:1].contiguous(), [dict(max_new_tokens=n_new, eos_token_id=-1)])[0]
        assert eng.cb_step(2) == 1
        others = eng.cb_admit(emb[1:33].contiguous(), [dict(max_new_tokens=8, eos_token_id=-1)] * 32)
        assert eng.cb_step(4) == 33                     # 33 live rows: the 64-row bucket
        while True:
            lv, _ = eng.cb_poll()
            if not any(lv[s] for s in others):
                break
            eng.cb_step(4)
        for s in others:
            eng.cb_release(s)
        while eng.cb_step(4) > 0:
            pass
        lv, st = eng.cb_poll()
        assert lv[a] == 0 and st[a] == n_new
        got = eng.cb_read(a, 0, n_new)
        assert torch.equal(got, solo), (got, solo)
        eng.cb_reset()
    finally:
        eng.close()
