"""-m gpu: attn_prefill_kernel in every form the engine's prompt pass launches it -- fused QKV rows (MQA with KV head stride 0, strided
KV heads), the sliding window, the trailing query tiles alone (last_rows) and the ragged form -- through sv_op_attention_prefill, against
the float32 reference of tests/attn_ref.py on the same bf16-exact inputs.

Tolerance: the one of test_gpu_ops.py::test_attention_prefill, |err| <= 3 * 2^-8 * max|ref| and mean |err| <= 1e-3 * max|ref| (the
probabilities and the output are each rounded to bf16).  Every windowed comparison carries its own control: the reference with the window
one key shorter and one key longer must differ from the reference by at least 10 x that tolerance, so that a window off by one key in
either direction cannot pass.  Where the engine promises bits (a row's result does not depend on which other tiles or sequences are in
the launch; window >= S is no window; window = 1 is the token's own V) the tests compare bits."""
import functools

import pytest
import torch

from starvector_amd import engine as E
from tests.attn_ref import ref
from tests.gpu_util import bf, dev

pytestmark = pytest.mark.gpu
TOL, MEAN_TOL = 3 * 2.0 ** -8, 1e-3
CONTROL = 10 * TOL
SENTINEL = 0x5A5A                                 # bit pattern the outputs are pre-filled with (as bf16: 1.5e16, never a result here)

# the smallest geometry of every kernel class: (query heads, KV heads, head_dim) -> query tile rows
GEOMS = {
    "1b_mqa_t32": (16, 1, 128),                   # multi-query: 32-row tiles, four heads per block, kv_head_stride 0
    "8b_gqa9_t128": (18, 2, 128),                 # 9 query heads per KV head: 128-row tiles, strided KV heads
    "hd64_t32": (8, 2, 64),
    "hd64_t128": (2, 2, 64),
}
GEOM_IDS = list(GEOMS)


def q_tile(H, Hkv):
    return 32 if (H // Hkv) % 4 == 0 and H % 4 == 0 else 128


def test_geometries_cover_both_tile_sizes_and_head_dims():
    assert {(q_tile(H, Hkv), hd) for H, Hkv, hd in GEOMS.values()} == {(32, 128), (128, 128), (32, 64), (128, 64)}


class Layout:
    """Column offsets of q / k / v inside a row of the fused buffer."""

    def __init__(self, H, Hkv, hd, pads=(0, 0, 0, 0)):
        self.q_off = pads[0]
        self.k_off = self.q_off + H * hd + pads[1]
        self.v_off = self.k_off + Hkv * hd + pads[2]
        self.stride = self.v_off + Hkv * hd + pads[3]


def fuse(q, k, v, lay, extra_rows=0):
    """[rows (+ extra_rows)][stride] bf16 on the device; every element that is not q / k / v is NaN, so a read of it shows."""
    rows = q.shape[0]
    buf = torch.full((rows + extra_rows, lay.stride), float("nan"))
    buf[:rows, lay.q_off:lay.q_off + q.shape[1]] = q
    buf[:rows, lay.k_off:lay.k_off + k.shape[1]] = k
    buf[:rows, lay.v_off:lay.v_off + v.shape[1]] = v
    return bf(buf)


def sentinel_out(rows, width):
    return torch.full((rows, width), SENTINEL, dtype=torch.int16, device=dev()).view(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def untouched(t):
    return bool((bits(t) == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def case(geom, lens, seed=0):
    """q (x 3: peaked scores, a few keys carry the mass), k, v: float32 CPU tensors holding bf16 values, packed rows."""
    H, Hkv, hd = GEOMS[geom]
    rows = sum(lens)
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + H + hd)
    q = (3 * torch.randn(rows, H * hd, generator=g)).bfloat16().float()
    k = torch.randn(rows, Hkv * hd, generator=g).bfloat16().float()
    v = torch.randn(rows, Hkv * hd, generator=g).bfloat16().float()
    return q, k, v


@functools.lru_cache(maxsize=None)
def case_ref(geom, lens, window, seed=0):
    """Computed once per (case, window), shared by the tests and never modified."""
    H, Hkv, _ = GEOMS[geom]
    return ref(*case(geom, lens, seed), H, Hkv, list(lens), 1, window)


def errs(got, want, scale=None):
    """(max, mean) |got - want| in units of max|want| (or of `scale`)."""
    got, want = got.float().cpu(), want.float()
    scale = float(want.abs().max()) if scale is None else scale
    d = (got - want).abs()
    return float(d.max()) / scale, float(d.mean()) / scale


def check_close(tag, got, want, scale=None):
    assert not torch.isnan(got.float()).any(), tag
    mx, mean = errs(got, want, scale)
    print(f"[{tag}] max err {mx * 256:.2f} x 2^-8, mean err {mean:.2e} (of max|ref|)")
    assert mx <= TOL and mean <= MEAN_TOL, (tag, mx, mean)
    return mx


def check_control(tag, want, shorter, longer):
    """The reference with the window one key shorter / longer is at least 10 tolerances away from the reference."""
    lo, hi = errs(shorter, want)[0], errs(longer, want)[0]
    print(f"[{tag}] control: window - 1 moves the reference by {lo / TOL:.1f} x tolerance, window + 1 by {hi / TOL:.1f} x")
    assert lo >= CONTROL and hi >= CONTROL, (tag, lo, hi)


def run(geom, qkv, lay, **kw):
    H, Hkv, hd = GEOMS[geom]
    out = E.op_attention_prefill(qkv, lay.q_off, lay.k_off, lay.v_off, H, Hkv, hd, **kw)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------
# the window against the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,W", [
    (70, 8),             # the window inside the first key tile
    (200, 64),           # a window of exactly one 64-key tile
    (200, 65),           # one key more
    (300, 100),          # the first key tile that is not skipped steps through 0, 1, 2, 3; in the 128-row classes the later waves of a block meet
                         # key tiles that lie wholly below their rows' window
    (515, 130),          # more than one 128-row block, S a multiple of nothing
])
@pytest.mark.parametrize("geom", GEOM_IDS)
def test_window_against_the_reference(geom, S, W):
    H, Hkv, hd = GEOMS[geom]
    B = 2
    lens = (S,) * B
    lay = Layout(H, Hkv, hd)                                                   # the engine's rows: q | k | v, nothing between
    got = run(geom, fuse(*case(geom, lens), lay), lay, B=B, S=S, window=W)
    want = case_ref(geom, lens, W)
    tag = f"window {geom} S={S} W={W}"
    check_control(tag, want, case_ref(geom, lens, W - 1), case_ref(geom, lens, W + 1))
    check_close(tag, got, want)


# ------------------------------------------------------------------------------------------------
# window edges placed by hand
# ------------------------------------------------------------------------------------------------
def needle_case(geom, S, W, shift):
    """Query rows i of interest look for ONE key, i - W + 1 + shift (shift 0: the oldest key inside the window, -1: the newest one
    outside): query and key are 24 x the same unit vector (score 576 * scale >= 50, every other score of the row ~ 0.2), the key's
    value row is zero but for a marker.  Returns q, k, v and {row: (key, [(kv head, column, amplitude)])}; rows whose key would
    lie before the sequence are left out (not wrapped)."""
    H, Hkv, hd = GEOMS[geom]
    g = torch.Generator().manual_seed(S * 31 + W + H)
    q = (3 * torch.randn(S, H * hd, generator=g)).bfloat16().float()
    k = (0.1 * torch.randn(S, Hkv * hd, generator=g)).bfloat16().float()
    v = torch.zeros(S, Hkv * hd)
    rows = sorted({63, 64, 127, 128, W - 1, W, S - 1})
    placed = {}
    for n, i in enumerate(rows):
        key = i - W + 1 + shift
        if key < 0 or i >= S:
            continue
        d = (11 * n + 3) % hd                                                  # one direction per row: the needles do not see each other
        q[i] = 0
        q[i].view(H, hd)[:, d] = 24.0
        k[key] = 0
        k[key].view(Hkv, hd)[:, d] = 24.0
        marks = []
        for kh in range(Hkv):
            col, amp = 8 * n + kh, 1.0 + (key % 7)                             # one column per (row, KV head)
            v[key, kh * hd + col] = amp
            marks.append((kh, col, amp))
        placed[i] = (key, marks)
    return q, k, v, placed


@pytest.mark.parametrize("S,W", [(300, 100), (200, 64), (200, 65)])
@pytest.mark.parametrize("geom", GEOM_IDS)
def test_window_edges_placed_by_hand(geom, S, W):
    H, Hkv, hd = GEOMS[geom]
    lay = Layout(H, Hkv, hd)
    group = H // Hkv
    for shift, present in [(0, True), (-1, False)]:
        q, k, v, placed = needle_case(geom, S, W, shift)
        assert len(placed) >= 4, placed
        want = ref(q, k, v, H, Hkv, [S], 1, W)
        # the control in the direction this case is about: one key fewer loses the needles, one key more admits them
        other = ref(q, k, v, H, Hkv, [S], 1, W - 1 if present else W + 1)
        moved = errs(other, want)[0]
        tag = f"needles {geom} S={S} W={W} {'inside' if present else 'outside'}"
        print(f"[{tag}] control: window {'- 1' if present else '+ 1'} moves the reference by {moved / TOL:.1f} x tolerance")
        assert moved >= CONTROL, (tag, moved)
        got = run(geom, fuse(q, k, v, lay), lay, B=1, S=S, window=W)
        check_close(tag, got, want)
        o = got.float().cpu().view(S, H, hd)
        for i, (key, marks) in placed.items():
            for kh, col, amp in marks:
                seen = o[i, kh * group:(kh + 1) * group, col]
                if present:                                                    # at full weight
                    assert ((seen - amp).abs() <= TOL * amp).all(), (tag, i, key, seen, amp)
                else:
                    assert (seen.abs() <= TOL * amp).all(), (tag, i, key, seen, amp)


# ------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOM_IDS)
def test_window_of_one_returns_the_tokens_own_value_bits(geom):
    H, Hkv, hd = GEOMS[geom]
    B, S = 2, 300
    q, k, v = case(geom, (S,) * B)
    lay = Layout(H, Hkv, hd)
    got = run(geom, fuse(q, k, v, lay), lay, B=B, S=S, window=1)
    idx = torch.arange(H) // (H // Hkv)
    want = v.view(B * S, Hkv, hd)[:, idx].reshape(B * S, H * hd).bfloat16()    # p = 1 exactly: the value row itself
    assert same_bits(got, want)


@pytest.mark.parametrize("geom", GEOM_IDS)
def test_window_at_or_above_the_length_gives_the_bits_of_no_window(geom):
    H, Hkv, hd = GEOMS[geom]
    B, S = 2, 300
    lay = Layout(H, Hkv, hd)
    qkv = fuse(*case(geom, (S,) * B), lay)
    full = run(geom, qkv, lay, B=B, S=S, window=0)
    check_close(f"no window {geom} S={S}", full, case_ref(geom, (S,) * B, 0))
    for W in (S, S + 1, 4096):
        assert same_bits(run(geom, qkv, lay, B=B, S=S, window=W), full), W


@pytest.mark.parametrize("pads", [(0, 0, 0, 0), (8, 16, 8, 24)], ids=["engine_rows", "padded_rows"])
@pytest.mark.parametrize("causal", [1, 0])
@pytest.mark.parametrize("geom", GEOM_IDS)
def test_fused_rows_give_the_bits_of_three_tensors(geom, causal, pads):
    """The same values through sv_op_attention (three contiguous tensors, the form test_attention_prefill pins) and as column ranges
    of one buffer, with NaN columns before, between and after them."""
    H, Hkv, hd = GEOMS[geom]
    B, S = 2, 257
    q, k, v = case(geom, (S,) * B)
    lay = Layout(H, Hkv, hd, pads)
    got = run(geom, fuse(q, k, v, lay), lay, B=B, S=S, causal=causal)
    three = E.op_attention(bf(q.view(B, S, -1)), bf(k.view(B, S, -1)), bf(v.view(B, S, -1)), H, Hkv, causal)
    assert not torch.isnan(got.float()).any()
    assert same_bits(got, three.view(B * S, H * hd))


# ------------------------------------------------------------------------------------------------
# last_rows: the trailing query tiles alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [129, 257, 300])
@pytest.mark.parametrize("geom", GEOM_IDS)
def test_last_rows_writes_the_trailing_tiles_only_with_the_bits_of_the_full_launch(geom, S):
    H, Hkv, hd = GEOMS[geom]
    B, W, tile = 2, 50, q_tile(H, Hkv)          # (a window short enough to cut most rows of the 129-row case too)
    lens = (S,) * B
    lay = Layout(H, Hkv, hd)
    qkv = fuse(*case(geom, lens), lay)
    for window in (0, W):
        want = case_ref(geom, lens, window)
        tag = f"last_rows {geom} S={S} W={window}"
        if window:
            check_control(tag, want, case_ref(geom, lens, window - 1), case_ref(geom, lens, window + 1))
        full = run(geom, qkv, lay, B=B, S=S, window=window)
        for last_rows in (1, 33, S):
            out = run(geom, qkv, lay, B=B, S=S, window=window, last_rows=last_rows, out=sentinel_out(B * S, H * hd))
            first = (S - last_rows) // tile * tile                             # first row of the first launched query tile
            o3, f3 = out.view(B, S, -1), full.view(B, S, -1)
            assert same_bits(o3[:, first:], f3[:, first:]), (tag, last_rows)
            assert untouched(o3[:, :first]), (tag, last_rows)
            scale = float(want.abs().max())
            check_close(f"{tag} last_rows={last_rows} last row", o3[:, S - 1], want.view(B, S, -1)[:, S - 1], scale)


# ------------------------------------------------------------------------------------------------
# the ragged form
# ------------------------------------------------------------------------------------------------
RAGGED = [(5, 31, 128, 129, 257, 300), (300, 129, 5, 257, 128, 31)]


@pytest.mark.parametrize("window", [0, 100])
@pytest.mark.parametrize("lens", RAGGED, ids=["ascending", "mixed"])
@pytest.mark.parametrize("geom", GEOM_IDS)
def test_ragged_form(geom, lens, window):
    H, Hkv, hd = GEOMS[geom]
    tile, rows, width = q_tile(H, Hkv), sum(lens), H * hd
    lay = Layout(H, Hkv, hd)
    PAD = 130                                                                  # rows behind the packed ones, in both buffers: never addressed
    qkv = fuse(*case(geom, lens), lay, extra_rows=PAD)
    want = case_ref(geom, lens, window)
    tag = f"ragged {geom} {'x'.join(map(str, lens))} W={window}"
    if window:
        check_control(tag, want, case_ref(geom, lens, window - 1), case_ref(geom, lens, window + 1))
    out = run(geom, qkv, lay, lens=lens, window=window, out=sentinel_out(rows + PAD, width))
    assert untouched(out[rows:]), tag
    check_close(tag, out[:rows], want)
    last = run(geom, qkv, lay, lens=lens, window=window, last_rows=1, out=sentinel_out(rows + PAD, width))
    r0 = 0
    for S in lens:
        # the sequence alone, as a rectangular launch over its own rows: the same bits
        solo = run(geom, qkv[r0:r0 + S], lay, B=1, S=S, window=window)
        assert same_bits(out[r0:r0 + S], solo), (tag, S)
        # the pruned list: the sequence's last query tile carries those bits, nothing else of the sequence is written
        first = (S - 1) // tile * tile
        assert same_bits(last[r0 + first:r0 + S], solo[first:]), (tag, S)
        assert untouched(last[r0:r0 + first]), (tag, S)
        r0 += S
    assert untouched(last[rows:]), tag
