"""GPU: the e4m3 KV cache (SV_KV_FP8_E4M3) kernel by kernel, over an engine's real paged pool -- the KVF = 1 forms of
kv_write_prefill_kernel and attn_decode_kernel (csrc/attention.hip) and kv_read_kernel (csrc/kv8/kv8.hip).

  * the quantiser: sv_debug_kv_load then sv_debug_kv_read against tests/kv8_ref.py bit for bit, designed and random rows;
  * the append: the row a decode step leaves at its position is kv8_ref of the step's own k_new (after RoPE) / v_new;
  * the attention against float32 softmax attention (tests/attn_ref.py) over deq(quant(K, V)) for the cached keys and the unquantised new
    token, at the kernel's own tolerance (the arithmetic is the bf16 kernel's), and beside a bf16-KV engine holding deq(quant(.));
  * stale codes and scale bytes behind a sequence's position contribute nothing; a 70-step walk across the page boundary.

Three geometries, helpers and engine configurations of tests/test_gpu_long_context.py: head_dim 128 MQA (16 / 1, 32 rows: 8 context splits,
4 key groups per block), head_dim 128 GQA (8 / 2, RoPE, a 96-key window), head_dim 64 MQA."""
from unittest import mock

import pytest
import torch

import starvector_amd as sva
from tests import attn_ref, kv8_ref as R
from tests.gpu_util import dev
from tests.test_gpu_long_context import _attn_engine, _kv_rows, _r, _rope_tables, _rot

pytestmark = pytest.mark.gpu

TOL = 2e-2                                            # the decode attention's tolerance in units of max|ref| (tests/test_gpu_long_context.py `_walk`)
SEQ = 1280
GEOMS = {                                             # H, n_kv, rows, head_dim, window
    "mqa128": (16, 1, 32, 128, 0),
    "gqa128": (8, 2, 8, 128, 96),
    "mqa64": (16, 1, 32, 64, 0),
}
_engines = {}


def _engine(geom, kv="fp8_e4m3"):
    """tests/test_gpu_long_context.py's attention engine of this geometry with the KV format swapped in (one per module and format)."""
    if (geom, kv) not in _engines:
        H, nkv, B, dh, W = GEOMS[geom]
        cfg = sva.EngineConfig
        with mock.patch.object(sva, "EngineConfig", lambda **kw: cfg(**kw, kv_dtype=kv)):
            _engines[geom, kv] = _attn_engine(H, nkv, B, SEQ, window=W, dh=dh)
        assert _engines[geom, kv].kv_info()["kv_dtype"] == kv
    return _engines[geom, kv]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def _rope(geom):
    H, nkv, B, dh, W = GEOMS[geom]
    return _rope_tables(SEQ, dh, 1e6) if (nkv > 1 or W) else None


def _row_pool(D, seed):
    """float32 [N, D] holding bf16 values: exact rows, tie rows, the rule's corners, random rows of very different magnitudes."""
    g = torch.Generator().manual_seed(seed)
    ex, _, _ = R.exact_rows(24, D, g, j_lo=-30, j_hi=30)
    sp, _ = R.special_rows(D, g)
    rnd = (torch.randn(40, D, generator=g) * torch.logspace(-4, 4, 40)[:, None]).bfloat16().float()
    return torch.cat([ex, R.tie_rows(D, g), sp, rnd])


def _tokens_from_pool(pool, B, S, nkv, seed):
    """[B, S, 2 * nkv * D] bf16: every (token, head, K or V) slot takes a row of the pool"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, pool.shape[0], (B, S, 2 * nkv), generator=g)
    return pool[idx].reshape(B, S, -1).to(torch.bfloat16)


# ---- the quantiser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
def test_quantiser_read_back_is_the_restatement(geom):
    """Rectangular loads of 1, 31, 32, 33, 64 and 65 tokens, and one 65-token load with those six lengths as dev_lens: what sv_debug_kv_read
    returns for every token of every row is kv8_ref.deq_quant of what was loaded, bit for bit."""
    H, nkv, B, dh, W = GEOMS[geom]
    eng = _engine(geom)
    pool = _row_pool(dh, 11)
    lens = [1, 31, 32, 33, 64, 65]
    for S in lens:
        kv = _tokens_from_pool(pool, 6, S, nkv, 100 + S)
        eng.debug_kv_load(0, kv.to(dev()))
        want = R.deq_quant(kv.view(6, S, 2 * nkv, dh)).view(6, S, -1)
        for b in range(6):
            got = eng.debug_kv_read(0, b, 0, S).cpu()
            assert R.same_bits(got, want[b]), f"{geom}: rectangular load of {S} tokens, row {b}"
    kv = _tokens_from_pool(pool, 6, 65, nkv, 99)
    eng.debug_kv_load(0, kv.to(dev()), lens=torch.tensor(lens, dtype=torch.int32, device=dev()))
    want = R.deq_quant(kv.view(6, 65, 2 * nkv, dh)).view(6, 65, -1)
    for b, n in enumerate(lens):
        got = eng.debug_kv_read(0, b, 0, n).cpu()
        assert R.same_bits(got, want[b, :n]), f"{geom}: load with dev_lens, row {b} ({n} tokens)"
    # the bf16 pool through the same read-back: the stored bits
    ref_eng = _engine(geom, "bf16")
    ref_eng.debug_kv_load(0, kv.to(dev()))
    assert R.same_bits(ref_eng.debug_kv_read(0, 3, 0, 65).cpu(), kv[3])
    assert R.same_bits(ref_eng.debug_kv_read(0, 5, 33, 32).cpu(), kv[5, 33:65])


# ---- the append ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
def test_appended_row_is_the_restatement_of_the_steps_own_row(geom):
    """After sv_debug_attn_decode(advance = 1) at positions 0, 31, 63 and 64 (a page's last and the next page's first slot), the row read
    back at the old position is kv8_ref of k_new (rotated where the configuration has RoPE) and v_new; its neighbours are untouched."""
    H, nkv, B, dh, W = GEOMS[geom]
    eng = _engine(geom)
    rope = _rope(geom)
    pool = _row_pool(dh, 21)
    pool = pool[torch.isfinite(pool).all(-1)]
    g = torch.Generator().manual_seed(22)
    for S in (0, 31, 63, 64):
        kv = _tokens_from_pool(pool, B, max(S, 1), nkv, 200 + S)[:, :S]
        eng.debug_kv_load(0, kv.to(dev()))
        # [B, 2 nkv, dh]: k heads | v heads; + 0.0: the step sums its c_attn slabs from +0, so a -0 input reaches the cache as +0
        new = pool[torch.randint(0, pool.shape[0], (B, 2 * nkv), generator=g)] + 0.0
        q = torch.randn(B, H * dh, generator=g)
        qkv = torch.cat([q, new.reshape(B, -1)], -1).float().contiguous()
        out = eng.debug_attn_decode(0, qkv.to(dev()), advance=True)
        kn, vn = new[:, :nkv], new[:, nkv:]
        if rope is not None:
            kn = _rot(kn.to(dev()), rope[0][S], rope[1][S]).cpu()
        want = R.deq_quant(torch.cat([kn, vn], 1)).view(B, -1)
        for b in (0, 1, B - 1):
            got = eng.debug_kv_read(0, b, 0, S + 1).cpu()
            assert R.same_bits(got[S], want[b]), f"{geom}: appended row at position {S}, row {b}"
            assert R.same_bits(got[:S], R.deq_quant(kv[b].view(S, 2 * nkv, dh)).view(S, 2 * nkv * dh)), f"{geom}: rows in front of position {S}"
        assert out.shape == (B, H * dh)                  # (rows of 2^127 in K and V: the step's own output is not the subject here)


# ---- the attention ---------------------------------------------------------------------------------------------------
def _needle_case(geom, L, seed):
    """q [B, H, dh], K / V [B, nkv, L, dh] float32 holding bf16 values (token L - 1 is the new one).  Keys are random with a per-key factor
    0.5 / 1 / 2 (K) and 2^-2 .. 2^2 (V) -- neighbouring keys' scales differ by factors of 2 -- and one key per 32-key group is a needle: K =
    24 e_d, V a one-hot marker whose amplitude depends on the token.  Every fourth head looks for the needle of one group (score 24 * 24 /
    sqrt(dh) against a few units for the rest); the other heads are peaked random queries."""
    H, nkv, B, dh, W = GEOMS[geom]
    g = torch.Generator().manual_seed(seed)
    k_fac = torch.ldexp(torch.ones(L), (torch.arange(L) % 3) - 1)
    v_fac = torch.ldexp(torch.ones(L), (torch.arange(L) * 3 % 5) - 2)
    K = (torch.randn(B, nkv, L, dh, generator=g) * k_fac[None, None, :, None]).bfloat16().float()
    V = (torch.randn(B, nkv, L, dh, generator=g) * v_fac[None, None, :, None]).bfloat16().float()
    q = torch.randn(B, H, dh, generator=g) * 3.0
    n_groups = (L + 31) // 32
    lo = max(0, L - W) if W else 0                                          # needles only where the window looks
    for b in range(B):
        for h in range(0, H, 4):
            grp = (b * 5 + h * 3) % n_groups
            tok = min(grp * 32 + (7 * grp + 3 + b) % 32, L - 1)
            if tok < lo:
                continue
            d = (grp * 13 + b + h) % dh
            kvh = h // (H // nkv)
            K[b, kvh, tok] = 0
            K[b, kvh, tok, d] = 24.0
            V[b, kvh, tok] = 0
            V[b, kvh, tok, (h * 8 + b) % dh] = (1.0 + tok % 7) * 2.0 ** (tok % 3)
            q[b, h] = 0
            q[b, h, d] = 24.0
    return q, K, V


def _reference(geom, q, K, V, rope, quantised=True):
    """attn_ref.ref for the query at the last key: the cached keys as deq(quant(.)), the new token unquantised (rotated with q where the
    configuration has RoPE: cached keys are stored rotated).  Returns ([B, H * dh] float32, the cache as the bf16 engine must hold it)."""
    H, nkv, B, dh, W = GEOMS[geom]
    L = K.shape[2]
    Kc, Vc = K.clone(), V.clone()
    if quantised and L > 1:
        Kc[:, :, :L - 1] = R.deq_quant(K[:, :, :L - 1]).float()
        Vc[:, :, :L - 1] = R.deq_quant(V[:, :, :L - 1]).float()
    qb, kn = _r(q), _r(K[:, :, L - 1])
    if rope is not None:
        cos, sin = rope[0][L - 1].cpu(), rope[1][L - 1].cpu()
        qb, kn = _rot(qb, cos, sin), _rot(kn, cos, sin)
    Kc[:, :, L - 1] = kn
    out = torch.empty(B, H * dh)
    for b in range(B):
        qq = torch.zeros(L, H * dh)
        qq[L - 1] = qb[b].reshape(-1)
        kk = Kc[b].permute(1, 0, 2).reshape(L, nkv * dh)
        vv = Vc[b].permute(1, 0, 2).reshape(L, nkv * dh)
        out[b] = attn_ref.ref(qq, kk, vv, H, nkv, [L], True, W)[L - 1]
    return out, Kc, Vc


def _launch(eng, geom, q, K, V):
    H, nkv, B, dh, W = GEOMS[geom]
    L = K.shape[2]
    eng.debug_kv_load(0, _kv_rows(K.to(dev()), V.to(dev()), L - 1))
    qkv = torch.cat([q.reshape(B, -1), K[:, :, L - 1].reshape(B, -1), V[:, :, L - 1].reshape(B, -1)], -1).float().contiguous()
    return eng.debug_attn_decode(0, qkv.to(dev()), advance=False).float().cpu()


CONTEXTS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1100]


@pytest.mark.parametrize("geom", list(GEOMS))
def test_attention_over_the_dequantised_cache(geom):
    """Contexts 1 .. 1100 (keys the query sees, the new token included): the group, page, second-split and six-wave-merge edges; the GQA
    geometry has a 96-key window, which context 200 crosses.  The fp8-KV engine, and a bf16-KV engine of the same configuration loaded with
    deq(quant(.)), both lie within TOL of the same reference; how many outputs are bit-equal and the largest difference are printed
    (profiles/kv_fp8.md records them).  A control: the reference over the UNquantised cache is further away than TOL at some context --
    the cases see the quantisation."""
    H, nkv, B, dh, W = GEOMS[geom]
    eng, ref_eng = _engine(geom), _engine(geom, "bf16")
    rope = _rope(geom)
    equal = total = 0
    worst_diff = worst = worst_unq = 0.0
    for L in CONTEXTS:
        q, K, V = _needle_case(geom, L, 300 + L)
        ref, Kc, Vc = _reference(geom, q, K, V, rope)
        scale = float(ref.abs().max())
        out = _launch(eng, geom, q, K, V)
        err = float((out - ref).abs().max())
        print(f"[kv fp8 attention {geom}] context {L}: |err| / max|ref| = {err / scale:.3e}")
        assert err <= TOL * scale, f"{geom} context {L}: fp8-KV attention off by {err:.3e} (max|ref| {scale:.3e}); row {int((out - ref).abs().amax(-1).argmax())}"
        Kb, Vb = Kc.clone(), Vc.clone()
        Kb[:, :, L - 1], Vb[:, :, L - 1] = K[:, :, L - 1], V[:, :, L - 1]       # the new token goes in as the step's own input
        out_b = _launch(ref_eng, geom, q, Kb, Vb)
        err_b = float((out_b - ref).abs().max())
        assert err_b <= TOL * scale, f"{geom} context {L}: bf16-KV attention over deq(quant(.)) off by {err_b:.3e}"
        equal += int((out.bfloat16().view(torch.int16) == out_b.bfloat16().view(torch.int16)).sum())
        total += out.numel()
        worst_diff = max(worst_diff, float((out - out_b).abs().max()) / scale)
        worst = max(worst, err / scale)
        if L > 1:
            unq, _, _ = _reference(geom, q, K, V, rope, quantised=False)
            worst_unq = max(worst_unq, float((out - unq).abs().max()) / float(unq.abs().max()))
    print(f"[kv fp8 attention {geom}] worst |err| / max|ref| {worst:.3e}; against the bf16-KV engine over deq(quant(.)): {equal} of {total} outputs "
          f"bit-equal, largest difference {worst_diff:.3e} of max|ref|; against the unquantised cache {worst_unq:.3e}")
    assert worst_unq > TOL, "the cases do not see the quantisation"


# ---- stale bytes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
def test_stale_codes_and_scales_behind_the_position_contribute_nothing(geom):
    """tests/test_gpu_safety.py's page-reuse case for codes AND scale bytes: a full-length load of rows that are NaN but for one element of
    1.5 * 2^127 leaves every slot of every page with NaN codes and the largest scale byte the quantiser writes; short sequences loaded over
    them and decoded must come out finite and within TOL (slots behind the position hold the stale bytes, in the new token's group too)."""
    H, nkv, B, dh, W = GEOMS[geom]
    eng = _engine(geom)
    rope = _rope(geom)
    junk = torch.full((B, SEQ - 1, 2 * nkv * dh), float("nan"))
    junk[..., ::dh] = -1.5 * 2.0 ** 127
    eng.debug_kv_load(0, junk.to(torch.bfloat16).to(dev()))
    got = eng.debug_kv_read(0, B - 1, SEQ - 3, 2).float().cpu()
    assert bool(torch.isnan(got[:, 1]).all()) and float(got[0, 0]) == -1.5 * 2.0 ** 127
    for L in (6, 41, 97):
        q, K, V = _needle_case(geom, L, 400 + L)
        ref, _, _ = _reference(geom, q, K, V, rope)
        out = _launch(eng, geom, q, K, V)
        assert bool(torch.isfinite(out).all()), f"{geom} context {L}: stale bytes reached the output"
        err, scale = float((out - ref).abs().max()), float(ref.abs().max())
        assert err <= TOL * scale, f"{geom} context {L} over stale pages: off by {err:.3e} (max|ref| {scale:.3e})"


# ---- walk ------------------------------------------------------------------------------------------------------------
def _ref64(q, K, V, W):
    """float64 decode attention of one row: q [H, dh], K / V [nkv, L, dh]; probabilities rounded to bf16 before P.V as the kernel has them"""
    H, dh = q.shape
    nkv, L = K.shape[0], K.shape[1]
    kk, vv = K.double().repeat_interleave(H // nkv, 0), V.double().repeat_interleave(H // nkv, 0)
    s = torch.einsum("hd,hld->hl", q.double(), kk) * dh ** -0.5
    if W and L > W:
        s[:, :L - W] = float("-inf")
    p = torch.softmax(s, -1).bfloat16().double()
    return torch.einsum("hl,hld->hd", p, vv).reshape(-1)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_walk_across_the_page_boundary(geom):
    """70 steps from context 60 with advance = 1: every step against a float64 replay that quantises each row as it enters the cache (the
    step's own row is seen unquantised, every later step reads kv8_ref of it)."""
    H, nkv, B, dh, W = GEOMS[geom]
    B = 4
    eng = _engine(geom)
    rope = _rope(geom)
    S, steps = 59, 70
    g = torch.Generator().manual_seed(500)
    K = (torch.randn(B, nkv, S + steps, dh, generator=g) * torch.ldexp(torch.ones(S + steps), torch.arange(S + steps) % 3 - 1)[None, None, :, None]).bfloat16().float()
    V = (torch.randn(B, nkv, S + steps, dh, generator=g) * torch.ldexp(torch.ones(S + steps), torch.arange(S + steps) * 3 % 5 - 2)[None, None, :, None]).bfloat16().float()
    eng.debug_kv_load(0, _kv_rows(K.to(dev()), V.to(dev()), S)[:B])
    Kc, Vc = K.clone(), V.clone()
    Kc[:, :, :S], Vc[:, :, :S] = R.deq_quant(K[:, :, :S]).float(), R.deq_quant(V[:, :, :S]).float()
    worst = 0.0
    for t in range(steps):
        pos = S + t
        q = torch.randn(B, H, dh, generator=g) * 3.0
        qkv = torch.cat([q.reshape(B, -1), K[:, :, pos].reshape(B, -1), V[:, :, pos].reshape(B, -1)], -1).float().contiguous()
        out = eng.debug_attn_decode(0, qkv.to(dev()), advance=True).float().cpu()
        qb, kn = _r(q), _r(K[:, :, pos])
        if rope is not None:
            cos, sin = rope[0][pos].cpu(), rope[1][pos].cpu()
            qb, kn = _rot(qb, cos, sin), _rot(kn, cos, sin)
        Kc[:, :, pos], Vc[:, :, pos] = kn, V[:, :, pos]
        ref = torch.stack([_ref64(qb[b], Kc[b, :, :pos + 1], Vc[b, :, :pos + 1], W) for b in range(B)]).float()
        err, scale = float((out - ref).abs().max()), float(ref.abs().max())
        worst = max(worst, err / scale)
        assert err <= TOL * scale, f"{geom} walk, context {pos + 1}: off by {err:.3e} (max|ref| {scale:.3e})"
        Kc[:, :, pos], Vc[:, :, pos] = R.deq_quant(kn).float(), R.deq_quant(V[:, :, pos]).float()      # what every later step reads
    print(f"[kv fp8 walk {geom}] contexts {S + 1}..{S + steps}: worst |err| / max|ref| = {worst:.3e}")
