"""GPU: the decode attention launch, whose blocks issue their critical-path requests first.

  * `attn_decode_kernel`: waves 4-7 request every c_attn slab and the bias at block start and sum them (slab order, then the bias)
    while waves 0-3 hold the block table and the KV stream alone.  The operator against the bf16-rounded float32 reference of
    tests/test_gpu_long_context.py (same walk, same tolerance) at the contexts where the roles of the waves change -- the empty cache,
    one key group, the first second split, the split cap, and (32 rows: 8 splits of 4 groups = 1024 keys) the contexts at which the
    upper waves start to own key groups and request them behind their slabs -- at head_dim 128 and 64, and grouped KV heads with RoPE
    and a small sliding window.  Then what one slab and a zero bias cannot see -- the slab stride, the slab order, the bias column:
    `sv_debug_attn_decode_slabs` with 1 / 4 / 8 slabs and a bias must give the BITS of the one-slab launch fed the row
    ((s0 + s1) + ...) + bias summed in float32 in that order, for the step itself and for the step behind it (which reads the K / V
    row that the first one appended from k_new | v_new)."""
import pytest
import torch

from tests.gpu_util import dev
from tests.test_gpu_long_context import _attn_engine, _kv_rows, _peaked_case, _r, _rope_tables, _walk

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(H, nkv, B, n_pos, window, dh):
    """one engine per attention geometry for the whole module (sv_debug_kv_load re-assigns the pages of every case)"""
    key = (H, nkv, B, n_pos, window, dh)
    if key not in _ENGINES:
        _ENGINES[key] = _attn_engine(H, nkv, B, n_pos, window=window, dh=dh)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _queries(n, B, H, dh, seed):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return [torch.randn(B, H, dh, generator=g, device=dev()) * 3.0 for _ in range(n)]


CONTEXTS = [(3, S) for S in (0, 31, 32, 127, 128, 256, 2047, 2048, 2049)] + [(32, S) for S in (1022, 1023, 1024, 1056, 1536)]


@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("B,S", CONTEXTS)
def test_one_slab_contexts_where_the_wave_roles_change(B, S, dh):
    """16 query heads on one KV head; two launches per cached length S (the second reads the row the first appended).  32 rows: 8
    splits of 4 key groups hold 1024 keys -- from context 1025 on a block has a fifth group and wave 4 owns it."""
    H = 16
    eng = _engine(H, 1, B, 2304, 0, dh)
    q, K, V = _peaked_case(B, H, 1, S + 2, 3.0, 9100 + S + dh, dh=dh)
    worst = _walk(eng, [q] + _queries(1, B, H, dh, 9101 + S), K, V, S, 2, 0, None, f"request order, B={B} head_dim {dh} S={S}")
    print(f"[decode attention, slabs from waves 4-7] B={B} head_dim {dh} context {S + 1}..{S + 2}: worst |err| / max|ref| = {worst:.3e}")


def test_one_slab_grouped_kv_rope_small_window():
    """12 query heads on 4 KV heads (3 live rows of the 16-row tile: the slab threads of rows 3-15 write zeros), RoPE in-kernel on q
    and k_new, sliding window 200: contexts 190 -> 197, the window start leaves key 0 inside a key group."""
    B, H, nkv, W, S, steps, dh = 16, 12, 4, 200, 189, 8, 128
    eng = _engine(H, nkv, B, 512, W, dh)
    q, K, V = _peaked_case(B, H, nkv, S + steps, 3.0, 9300, dh=dh)
    rope = _rope_tables(512, dh, 1e6)
    worst = _walk(eng, _queries(steps, B, H, dh, 9301), K, V, S, steps, W, rope, "request order, GQA 12/4 RoPE window 200")
    print(f"[decode attention, slabs from waves 4-7] GQA 12/4, RoPE, window 200, walk {S + 1}..{S + steps}: worst {worst:.3e}")


@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("splitk", [1, 4, 8])
@pytest.mark.parametrize("B,S", [(3, 37), (32, 37), (32, 1030)])
def test_slabs_and_bias_give_the_bits_of_their_float32_sum(B, S, splitk, dh):
    """The sum order is fixed (slab 0 .. splitk - 1, then the bias, in float32), so the launch fed `splitk` slabs and a bias must
    produce the bits of the launch fed that sum as one slab.  Context 38: the new token carries weight, so a wrong k_new / v_new
    column moves the output; context 1031 at 32 rows: the upper waves own a key group as well.  The second step (one slab on both
    sides, its query pointed at the new token's key) reads the K / V row the first step appended."""
    H = 16
    QKV = H * dh + 2 * dh
    eng = _engine(H, 1, B, 2304, 0, dh)
    q, K, V = _peaked_case(B, H, 1, S + 2, 3.0, 9500 + S + dh + splitk, dh=dh)
    g = torch.Generator(device=dev()).manual_seed(9501 + splitk)
    row = torch.cat([q.reshape(B, H * dh), K[:, 0, S], V[:, 0, S]], -1).float()
    # slabs that sum to about `row`: random parts of very different size (the order of the float32 adds matters), and a bias
    parts = torch.randn(splitk, B, QKV, generator=g, device=dev()) * torch.logspace(-2, 1, splitk, device=dev())[:, None, None]
    bias = (torch.randn(QKV, generator=g, device=dev()) * 0.5).to(torch.bfloat16)
    slabs = parts.clone()
    slabs[0] += row - parts.sum(0) - bias.float()
    slabs = slabs.contiguous()
    total = torch.zeros(B, QKV, device=dev())
    for s in range(splitk):
        total = total + slabs[s]                    # ((0 + s0) + s1) + ...: the kernel's order
    total = (total + bias.float()).contiguous()
    # second step: every head looks at the key the first step appended
    k1 = _r(total[:, H * dh:H * dh + dh])
    q2 = (k1 * (24.0 / k1.norm(dim=-1, keepdim=True)))[:, None, :].expand(B, H, dh)
    row2 = torch.cat([q2.reshape(B, H * dh), K[:, 0, S + 1], V[:, 0, S + 1]], -1).float().contiguous()

    kv = _kv_rows(K, V, S)
    eng.debug_kv_load(0, kv)
    a1 = eng.debug_attn_decode_slabs(0, slabs, bias, advance=True).clone()
    a2 = eng.debug_attn_decode(0, row2, advance=True).clone()
    eng.debug_kv_load(0, kv)
    b1 = eng.debug_attn_decode(0, total, advance=True).clone()
    b2 = eng.debug_attn_decode(0, row2, advance=True).clone()
    assert bool(torch.isfinite(b1.float()).all()) and float(b1.float().abs().max()) > 0
    d1 = int((a1.view(torch.int16) != b1.view(torch.int16)).sum())
    d2 = int((a2.view(torch.int16) != b2.view(torch.int16)).sum())
    print(f"[decode attention, {splitk} slab(s) + bias] B={B} head_dim {dh} context {S + 1}: {d1} / {d2} of {a1.numel()} outputs differ "
          f"from the one-slab launch (step / next step)")
    assert d1 == 0, f"{d1} outputs of the {splitk}-slab launch differ from the one-slab launch fed the float32 sum"
    assert d2 == 0, f"{d2} outputs of the NEXT step differ: the K / V row appended from the slabs is not the one-slab launch's"
    # the second step does look at the appended row: without it the answer is another one
    eng.debug_kv_load(0, kv)
    eng.debug_attn_decode(0, (total * 0.5).contiguous(), advance=True)
    c2 = eng.debug_attn_decode(0, row2, advance=True)
    assert not torch.equal(c2, b2), "the second step does not depend on the row the first one appended"
