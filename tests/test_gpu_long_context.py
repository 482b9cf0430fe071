"""GPU: parity at the contexts the reference and the benchmark actually reach.

The reference generates to max_length 7800 with StarVector-1B (configs/generation/hf/starvector-1b/im2svg.yaml:33) and 16000 with
StarVector-8B behind StarCoder2's sliding window of 4096 (configs/generation/hf/starvector-8b/im2svg.yaml:32,
starvector/model/llm/starcoder2.py:22-27); bench.py decodes contexts 260 -> 1283.  Two kinds of test:

  * THE OPERATOR: `attn_decode_kernel` on its own over an engine's real paged KV pool / block table / split plan
    (include/starvector_hip.h: sv_debug_kv_load, sv_debug_attn_decode), against float32 torch softmax attention with the oracle's cast
    points (gpt_bigcode/modeling_gpt_bigcode.py:151-226).  q is scaled so that the softmax is PEAKED (a handful of keys spread over all
    pages carry the mass): a missing, stale or misplaced key group moves the output by O(1), not by 1/L.  Contexts 0 .. 8191 (1B) and
    .. 16383 with the real window value 4096 (8B), walks across the 64-page boundary of the pre-loaded block table (4096 tokens), the
    split cap, the window start crossing key groups and pages, a ragged batch.
  * END TO END: BASELINE config 2 (StarVector-1B, B = 32) teacher-forced against the oracle in float32 on the GPU around contexts 1283
    (the bench's end), 4080 -> 4110 (the 64-page boundary) and 7780 -> 7800 (the reference's max_length); StarVector-8B dimensions two
    layers deep with sliding_window = 4096 at 4090 -> 4120; beam search's KV re-index across the 4096 boundary.  The oracle's prompt pass
    runs in row chunks (its attention scores are [rows, heads, S, S] float32).  With random weights the attention over thousands of keys
    is a small part of the residual stream, so every e2e case also PRINTS its own discriminating power: the oracle's logit change when one
    KV page of the far context is swapped for another (in units of the tolerance); the operator tests are what pins the kernel."""
import dataclasses
import gc
import math

import pytest
import torch

import starvector_amd as sva
from oracle import starvector_oracle as O
from tests.gpu_util import bf, build_engine, dev
from tests.test_gpu_e2e import LOGIT_TOL

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------
# the operator
# ------------------------------------------------------------------------------------------------------------------
def _r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _attn_engine(n_head, n_kv, max_batch, max_seq_len, window=0, dh=128):
    """An engine with the decoder's attention geometry (head_dim `dh`: 128, or 64 in tests/test_gpu_decoder_head_dim64.py) and everything
    else small: the attention test surface needs no weights (the caller supplies q / K / V)."""
    hidden = n_head * dh
    ec = sva.EngineConfig(image_size=28, patch_size=14, vit_width=128, vit_layers=1, vit_heads=2, hidden=hidden, n_layer=1,
                          n_head=n_head, n_inner=256, vocab=512, n_positions=max_seq_len, max_batch=max_batch,
                          max_seq_len=max_seq_len, arch="v2" if n_kv > 1 or window else "v1", n_kv_head=n_kv,
                          rope_theta=1e6, vit_mlp=256, sliding_window=window)
    return sva.HipEngine(ec)


def _rope_tables(n_pos, dh, theta):
    """Starcoder2RotaryEmbedding as the oracle restates it (oracle._rope): float32 angles, cos / sin rounded to bf16."""
    inv = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float32, device=dev()) / dh))
    fr = torch.arange(n_pos, dtype=torch.float32, device=dev())[:, None] * inv[None, :]
    emb = torch.cat([fr, fr], -1)
    return _r(emb.cos()), _r(emb.sin())


def _rot(x, cos, sin):
    h = x.shape[-1] // 2
    rh = torch.cat([-x[..., h:], x[..., :h]], -1)
    return _r(_r(x * cos) + _r(rh * sin))


def _ref_attention(q, K, V, pos, window):
    """q [B,H,dh], K/V [B,nkv,L,dh] (float32 holding bf16 values, new token included), pos [B] -> [B, H*dh].  Keys j with
    max(0, pos - window + 1) <= j <= pos (window 0 = all); softmax in float32, probabilities rounded to bf16 before P.V, output
    rounded to bf16 (the oracle's `_block` / `_block_v2`)."""
    B, H, dh = q.shape
    nkv, L = K.shape[1], K.shape[2]
    G = H // nkv
    kk, vv = K.repeat_interleave(G, 1), V.repeat_interleave(G, 1)
    s = torch.einsum("bhd,bhld->bhl", q, kk) * dh ** -0.5
    j = torch.arange(L, device=q.device)[None, None, :]
    p3 = pos[:, None, None]
    dead = j > p3
    if window:
        dead = dead | (j <= p3 - window)
    s = s.masked_fill(dead, float("-inf"))
    pr = _r(torch.softmax(s, -1))
    return _r(torch.einsum("bhl,bhld->bhd", pr, vv).reshape(B, H * dh))


def _peaked_case(B, H, nkv, L, sharp, seed, dh=128):
    g = torch.Generator(device=dev()).manual_seed(seed)
    K = _r(torch.randn(B, nkv, L, dh, generator=g, device=dev()))
    V = _r(torch.randn(B, nkv, L, dh, generator=g, device=dev()))
    q = torch.randn(B, H, dh, generator=g, device=dev()) * sharp            # scores ~ N(0, sharp^2): a few keys carry the mass
    return q, K, V


def _kv_rows(K, V, S):
    """[B, S, 2*nkv*dh] bf16: k heads | v heads of tokens 0..S-1."""
    B, nkv, _, dh = K.shape
    k = K[:, :, :S].permute(0, 2, 1, 3).reshape(B, S, nkv * dh)
    v = V[:, :, :S].permute(0, 2, 1, 3).reshape(B, S, nkv * dh)
    return torch.cat([k, v], -1).to(torch.bfloat16).contiguous()


def _walk(eng, q_all, K, V, S, steps, window, rope, tag, tol=2e-2):
    """Load tokens 0..S-1, then `steps` decode-attention launches for tokens S, S+1, ... (each appends its K / V row) against the
    reference over the same keys.  q_all [steps][B,H,dh] float32 (pre-RoPE), K / V hold the pre-RoPE new rows at index S + t; cached
    rows are taken as they are.  Returns the worst error in units of max|ref|."""
    B, nkv, _, dh = K.shape
    H = q_all[0].shape[1]
    eng.debug_kv_load(0, _kv_rows(K, V, S))
    Kc, Vc = K.clone(), V.clone()
    worst = 0.0
    for t in range(steps):
        pos = S + t
        q, kn, vn = q_all[t], K[:, :, pos], V[:, :, pos]                    # [B,H,dh], [B,nkv,dh]
        qkv = torch.cat([q.reshape(B, H * dh), kn.reshape(B, nkv * dh), vn.reshape(B, nkv * dh)], -1).float().contiguous()
        out = eng.debug_attn_decode(0, qkv, advance=True).float()
        qb, kb = _r(q), _r(kn)
        if rope is not None:
            cos, sin = rope[0][pos], rope[1][pos]
            qb, kb = _rot(qb, cos, sin), _rot(kb, cos, sin)
        Kc[:, :, pos] = kb
        Vc[:, :, pos] = _r(vn)
        ref = _ref_attention(qb, Kc[:, :, :pos + 1], Vc[:, :, :pos + 1], torch.full((B,), pos, device=dev()), window)
        scale = float(ref.abs().max())
        err = float((out - ref).abs().max())
        worst = max(worst, err / scale)
        assert err <= tol * scale, (f"[{tag}] context {pos + 1}: decode attention off by {err:.3e} (max|ref| {scale:.3e}, tolerance "
                                    f"{tol * scale:.3e}); row {int((out - ref).abs().amax(-1).argmax())}")
    return worst


@pytest.mark.parametrize("S", [0, 1, 31, 32, 63, 64, 127, 1282, 4095, 7799, 8190])
def test_decode_attention_1b_geometry_contexts(S):
    """StarVector-1B's attention (16 query heads on one KV head, B = 32: 8 context splits per sequence) at single contexts from the
    empty cache to the last position of the 8192 table; two launches each (the second reads the row the first appended)."""
    B, H = 32, 16
    eng = _attn_engine(H, 1, B, 8192)
    q, K, V = _peaked_case(B, H, 1, S + 2, 3.0, 100 + S)
    g = torch.Generator(device=dev()).manual_seed(7 + S)
    qs = [q, torch.randn(B, H, 128, generator=g, device=dev()) * 3.0]
    worst = _walk(eng, qs, K, V, S, 2, 0, None, f"1B attention S={S}")
    print(f"[decode attention 1B geometry] context {S + 1}..{S + 2}: worst |err| / max|ref| = {worst:.3e}")
    eng.close()


def test_decode_attention_1b_geometry_walk_across_the_64_page_boundary():
    """Contexts 4081 -> 4120: the block-table entries of pages >= 64 are not in the kernel's pre-loaded registers (attention.hip
    `page_of`), the new token's page changes at 4096, and every sequence runs at the split cap."""
    B, H, S, steps = 32, 16, 4080, 40
    eng = _attn_engine(H, 1, B, 8192)
    q, K, V = _peaked_case(B, H, 1, S + steps, 3.0, 4242)
    g = torch.Generator(device=dev()).manual_seed(4243)
    qs = [torch.randn(B, H, 128, generator=g, device=dev()) * 3.0 for _ in range(steps)]
    worst = _walk(eng, qs, K, V, S, steps, 0, None, "1B attention walk 4081..4120")
    print(f"[decode attention 1B geometry] walk 4081..4120 (page 63 -> 64): worst |err| / max|ref| = {worst:.3e}")
    eng.close()


def test_decode_attention_needle_on_every_page():
    """One key per page made the argmax of one head's scores (a 'needle'), its value row a one-hot marker: the output must carry every
    marker at full weight -- a page that is skipped, read twice or read from another sequence shows as a missing / foreign marker."""
    B, H, L = 32, 16, 8000
    eng = _attn_engine(H, 1, B, 8192)
    g = torch.Generator(device=dev()).manual_seed(99)
    K = _r(torch.randn(B, 1, L, 128, generator=g, device=dev()) * 0.1)
    V = torch.zeros(B, 1, L, 128, device=dev())
    n_pages = (L + 63) // 64
    q = torch.zeros(B, H, 128, device=dev())
    # head h of row b looks for the needle of page (b * 7 + h * 5) % n_pages; needle key = 24 * e_dir, query = 24 * e_dir: score 576/sqrt(128) = 51
    want = torch.zeros(B, H, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            pg = (b * 7 + h * 5) % n_pages
            tok = min(pg * 64 + (b * 3 + h) % 64, L - 2)
            d = (pg * 13 + b) % 128
            K[b, 0, tok] = 0
            K[b, 0, tok, d] = 24.0
            q[b, h, d] = 24.0
            V[b, 0, tok, (h * 8 + b) % 128] = 1.0 + (tok % 7)             # marker: position-dependent amplitude
            want[b, h] = tok
    worst = _walk(eng, [q], K, V, L - 1, 1, 0, None, "needles", tol=2e-2)
    print(f"[decode attention needles] {B * H} needles over {n_pages} pages: worst |err| / max|ref| = {worst:.3e}")
    eng.close()


def test_decode_attention_ragged_batch_positions():
    """Rows of ONE launch at different contexts (continuous batching, padded prompts): 6 .. 5990 keys in one batch of 32, so the
    active context splits, the groups per wave and the page counts all differ between the blocks of the launch."""
    B, H, L = 32, 16, 6100
    eng = _attn_engine(H, 1, B, 8192)
    q, K, V = _peaked_case(B, H, 1, L, 3.0, 555)
    pos = torch.tensor([5 + 193 * b for b in range(B)], dtype=torch.int32, device=dev())
    eng.debug_kv_load(0, _kv_rows(K, V, L - 1), lens=pos)
    idx = pos.long()
    rows = torch.arange(B, device=dev())
    kn, vn = K[rows, 0, idx], V[rows, 0, idx]                                # each row's new token sits at its own position
    qkv = torch.cat([q.reshape(B, H * 128), kn, vn], -1).float().contiguous()
    out = eng.debug_attn_decode(0, qkv, advance=False).float()
    ref = _ref_attention(_r(q), K, V, idx, 0)                                # keys above pos[b] are masked per row
    err = (out - ref).abs().amax(-1) / ref.abs().max()
    print(f"[decode attention 1B geometry] ragged batch, contexts {int(pos.min()) + 1}..{int(pos.max()) + 1}: worst {float(err.max()):.3e}")
    assert float(err.max()) <= 2e-2, f"row {int(err.argmax())} (context {int(pos[int(err.argmax())]) + 1}): {float(err.max()):.3e}"
    eng.close()


@pytest.mark.parametrize("S,steps", [(4070, 60), (8180, 24), (16350, 30)])
def test_decode_attention_8b_geometry_sliding_window_4096(S, steps):
    """StarVector-8B's attention: 36 query heads on 4 KV heads (9 per MFMA tile), RoPE applied in-kernel to q and the new k, and the REAL
    window value 4096 masking real keys: contexts 4071 -> 4130 (the window start leaves key 0, crosses key groups), 8181 -> 8204 and the end
    of the 16384-position table (window start crosses pages; groups / pages below the window are never read)."""
    B, H, nkv, W = 16, 36, 4, 4096
    eng = _attn_engine(H, nkv, B, 16384, window=W)
    q, K, V = _peaked_case(B, H, nkv, S + steps, 3.0, 8000 + S)
    g = torch.Generator(device=dev()).manual_seed(8001 + S)
    qs = [torch.randn(B, H, 128, generator=g, device=dev()) * 3.0 for _ in range(steps)]
    rope = _rope_tables(16384, 128, 1e6)
    worst = _walk(eng, qs, K, V, S, steps, W, rope, f"8B attention walk {S + 1}..{S + steps}")
    print(f"[decode attention 8B geometry, window 4096] walk {S + 1}..{S + steps}: worst |err| / max|ref| = {worst:.3e}")
    # control: the same keys WITHOUT the window give another answer (the window masks keys that carry mass)
    if S >= W:
        pos = S + steps - 1
        cos, sin = rope[0][pos], rope[1][pos]
        qb = _rot(_r(qs[-1]), cos, sin)
        Kc = K.clone()
        a = _ref_attention(qb, Kc[:, :, :pos + 1], V[:, :, :pos + 1], torch.full((B,), pos, device=dev()), W)
        b = _ref_attention(qb, Kc[:, :, :pos + 1], V[:, :, :pos + 1], torch.full((B,), pos, device=dev()), 0)
        assert float((a - b).abs().max()) > 0.2 * float(a.abs().max()), "the case does not exercise the window"
    eng.close()


@pytest.mark.parametrize("H,nkv,S,steps", [(36, 4, 248, 20), (36, 4, 1010, 6), (16, 1, 24, 16), (16, 1, 2040, 6)])
def test_decode_attention_full_64_row_batch_has_more_blocks_than_the_chip_has_cus(H, nkv, S, steps):
    """A 64-row engine launches 64 * n_kv * max_splits = 512 blocks of 8 waves at one block per CU: the blocks of a sequence's context
    splits are NOT all resident at once, so the split merge must not wait for a block that has not been dispatched (round 4's in-band
    hand-off did, and gave every row NaNs at the first context with two active splits: 8B geometry 257, profiles/diag_8b_fp8_r04.log).
    Walks across that first multi-split context for both geometries, and a context at the split cap."""
    B = 64
    W = 4096 if nkv > 1 else 0
    eng = _attn_engine(H, nkv, B, 4096, window=W)
    q, K, V = _peaked_case(B, H, nkv, S + steps, 3.0, 6400 + S)
    g = torch.Generator(device=dev()).manual_seed(6401 + S)
    qs = [torch.randn(B, H, 128, generator=g, device=dev()) * 3.0 for _ in range(steps)]
    rope = _rope_tables(4096, 128, 1e6) if nkv > 1 else None
    worst = _walk(eng, qs, K, V, S, steps, W, rope, f"64 rows, {H}/{nkv} heads, walk {S + 1}..{S + steps}")
    print(f"[decode attention, 64 rows, {H} heads on {nkv}] walk {S + 1}..{S + steps}: worst |err| / max|ref| = {worst:.3e}")
    eng.close()


def test_blocks_of_a_launch_go_round_robin_to_the_xcds():
    """The XCD-aware block -> tile mappings (slab GEMMs' (tile, K slice) assignment, the 256^2 GEMM's tile order) rest on the dispatcher dealing
    block L of a launch to XCD (L + c) % 8.  Where the blocks of a launch that fits the chip and of one that runs in rounds (the decode
    attention's footprint, 512 blocks) actually ran: `sv_debug_xcc_map`."""
    eng = _attn_engine(16, 1, 32, 4096)
    for heavy, n in [(False, 1024), (True, 512)]:
        m = eng.debug_xcc_map(n, heavy)
        rule = all(m[i] == m[i & 7] for i in range(n)) and len(set(m[:8])) == 8
        print(f"[xcd map] {n} blocks, {'attention footprint, 2 rounds' if heavy else 'light'}: first 16 -> {m[:16]}; block L on XCD map[L % 8]: {rule}")
        assert rule
    eng.close()


# ------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------
def _oracle_long(w, cfg, emb, n_new, rows_per_chunk):
    """Oracle greedy stream from a long prompt: the prompt pass in row chunks (scores are [rows, H, S, S] float32), then all rows
    decode together.  Returns (tokens [B, n_new], logits [B, n_new, V], cache)."""
    B = emb.shape[0]
    lgs, caches = [], []
    with torch.no_grad():
        for i in range(0, B, rows_per_chunk):
            lg, cache = O.decoder_prefill(w, cfg, emb[i:i + rows_per_chunk].float(), "bf16")
            lgs.append(lg)
            caches.append(cache)
            torch.cuda.empty_cache()
        logits = torch.cat(lgs, 0)
        cache = [(torch.cat([c[l][0] for c in caches], 0), torch.cat([c[l][1] for c in caches], 0)) for l in range(cfg.n_layer)]
        del caches
        toks, all_lg = [], []
        for t in range(n_new):
            sc = logits.float()
            all_lg.append(sc)
            nxt = sc.argmax(-1)
            toks.append(nxt)
            if t + 1 < n_new:
                logits, cache = O.decoder_decode_step(w, cfg, nxt, cache, "bf16")
    return torch.stack(toks, 1), torch.stack(all_lg, 1), cache


def _page_swap_sensitivity(w, cfg, cache, last_tok, o_next_logits, page_a, page_b, tol_abs):
    """The oracle's own logit change when KV page `page_a` (64 tokens) of every layer is replaced by page `page_b`: what a wrong block-table
    entry would do, in units of the test's tolerance."""
    sl_a, sl_b = slice(page_a * 64, page_a * 64 + 64), slice(page_b * 64, page_b * 64 + 64)
    bad = []
    for k, v in cache:
        k2, v2 = k.clone(), v.clone()
        if cfg.arch == "v2":
            k2[:, :, sl_a], v2[:, :, sl_a] = k[:, :, sl_b], v[:, :, sl_b]
        else:
            k2[:, sl_a], v2[:, sl_a] = k[:, sl_b], v[:, sl_b]
        bad.append((k2, v2))
    with torch.no_grad():
        lg, _ = O.decoder_decode_step(w, cfg, last_tok, bad, "bf16")
    return float((lg.float() - o_next_logits).abs().max()) / tol_abs


def _teacher_forced_long(eng, emb, o_toks, o_lg, tag, min_checked, max_near=0.1):
    """The engine is fed the oracle's tokens; logits within LOGIT_TOL * scale at every step, tokens exact outside twice that band."""
    B, n_new = o_toks.shape
    scale = float(o_lg.abs().max())
    band = 2 * LOGIT_TOL * scale
    top2 = o_lg.topk(2, -1).values
    margin = top2[..., 0] - top2[..., 1]
    worst, checked, near = 0.0, 0, 0
    for t in range(n_new):
        lg = (eng.prefill(emb) if t == 0 else eng.decode_step(o_toks[:, t - 1].contiguous())).float()
        err = (lg - o_lg[:, t]).abs().amax(-1)
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= LOGIT_TOL * scale, (f"[{tag}] step {t}: row {int(err.argmax())} logits off by {float(err.max()):.3e} "
                                                       f"(scale {scale:.3e}, tolerance {LOGIT_TOL * scale:.3e})")
        am = lg.argmax(-1)
        safe = margin[:, t] > band
        bad = safe & (am != o_toks[:, t])
        assert not bool(bad.any()), f"[{tag}] step {t}: rows {bad.nonzero().flatten().tolist()} differ from the oracle outside the band"
        checked += int(safe.sum())
        near += int((~safe & (am != o_toks[:, t])).sum())
    msg = (f"[{tag}] {n_new} steps x {B} rows: logits max|err| {worst:.3e} (scale {scale:.3e}, {worst / scale:.2e} relative); "
           f"{checked}/{B * n_new} positions token-exact outside the band, {near} near-tie flips inside it")
    print(msg)
    assert checked >= min_checked * B * n_new, msg
    assert near <= max_near * B * n_new, msg                       # in-band flips are legitimate near-ties, but a regression shows as more of them
    return worst / scale


@pytest.fixture(scope="module")
def config2():
    """BASELINE config 2's model (StarVector-1B, seed-1234 weights, B = 32) with the KV pool sized for the reference's max_length."""
    cfg = dataclasses.replace(O.OracleConfig(), eos_token_id=-1)
    w = O.make_weights(cfg, seed=1234)
    eng = build_engine(cfg, w, max_batch=32, max_seq_len=7808)
    w_dev = {k: v.to(dev()) for k, v in w.items() if "image_encoder" not in k and "image_projection" not in k}
    del w
    gc.collect()
    yield cfg, eng, w_dev
    eng.close()
    del w_dev
    gc.collect(); torch.cuda.empty_cache()


def _synthetic_prompt(B, S0, D, seed):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(B, S0, D, generator=g, device=dev()) * 0.5).to(torch.bfloat16)


@pytest.mark.parametrize("S0,n_new,chunk", [(1262, 24, 32), (4080, 32, 8), (7780, 20, 2)])
def test_config2_batch32_long_contexts(config2, S0, n_new, chunk):
    """Teacher-forced logits + tokens at contexts 1262 -> 1286 (bench.py's last step is context 1283), 4080 -> 4112 (across the 64-page
    block-table boundary) and 7780 -> 7800 (configs/generation/hf/starvector-1b/im2svg.yaml:33 max_length), B = 32."""
    cfg, eng, w_dev = config2
    B = 32
    emb = _synthetic_prompt(B, S0, cfg.hidden, 1000 + S0)
    o_toks, o_lg, cache = _oracle_long(w_dev, cfg, emb, n_new, chunk)
    tag = f"config2 B=32 context {S0}->{S0 + n_new}"
    # coverage floor: a synthetic N(0, 0.5) prompt leaves the random-init model with flatter logits than an image prompt does --
    # measured 28 / 28 / 33 % of the positions have a top-1/top-2 margin outside the band (217/768, 291/1024, 209/640; 18-35 in-band
    # near-tie flips); EVERY one of them must be token-exact and EVERY position's logits in tolerance
    _teacher_forced_long(eng, emb, o_toks, o_lg, tag, 0.2, max_near=0.06)
    # discriminating power of THIS case: swap one far page for another in the oracle's cache and look at its own logits
    with torch.no_grad():
        ref_next, _ = O.decoder_decode_step(w_dev, cfg, o_toks[:, -1], cache, "bf16")
    tol_abs = LOGIT_TOL * float(o_lg.abs().max())
    last_page = (S0 + n_new - 2) // 64
    sens = _page_swap_sensitivity(w_dev, cfg, cache, o_toks[:, -1], ref_next.float(), last_page - 1, 0, tol_abs)
    print(f"[{tag}] sensitivity: swapping KV page {last_page - 1} for page 0 in every layer moves the oracle's logits by {sens:.2f} x the "
          f"tolerance (random weights: attention over {S0} keys is a small part of the residual; the operator tests pin the kernel)")
    # free run from the same prompt: graph loop == eager teacher-forced stream wherever the margins are safe
    got = eng.generate(emb, max_length=S0 + n_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id).cpu()
    scale = float(o_lg.abs().max())
    top2 = o_lg.topk(2, -1).values
    margin = (top2[..., 0] - top2[..., 1]).cpu()
    o_cpu = o_toks.cpu()
    full = 0
    for b in range(B):
        diff = (got[b] != o_cpu[b]).nonzero()
        t = int(diff[0]) if diff.numel() else n_new
        assert t == n_new or float(margin[b, t]) <= 2 * LOGIT_TOL * scale, f"[{tag}] row {b} leaves the oracle at step {t} outside the band"
        full += t == n_new
    print(f"[{tag}] free run (hipGraph loop): {full}/{B} rows identical to the oracle for all {n_new} tokens")
    del cache
    gc.collect(); torch.cuda.empty_cache()


def test_config2_long_context_with_peaked_attention():
    """with random weights the attention over thousands of keys is a small part of the residual, and the case above at
    7780 -> 7800 moves by only ~1 x its tolerance when a far KV page is swapped -- it could not see the bug it is named for.  Same model, same
    context, but the QUERY rows of every c_attn (weight and bias) are multiplied by Q_GAIN in the engine and in the oracle alike: a peaked
    softmax, where a wrong page moves the oracle's own logits by several tolerances (asserted) while the engine still has to stay inside ONE
    (LOGIT_TOL, teacher-forced, every step, every row).  How peaked: tools/diag/peaked_sweep.py -- gain 1 / 1.5 / 2 / 3 / 4 gives a page-swap
    sensitivity of 1.0 / 1.3 / 1.7-2.8 / 3.9-9.0 / 21-30 x the tolerance, an engine error of 1.3 / 1.3 / 1.2 / 1.6 / 3.9e-2 of the scale and
    a distance of the ORACLE'S OWN bf16 and fp32 modes of 1.0 / 1.1 / 1.1 / 1.1 / 3.4e-2: beyond gain 3 the function itself amplifies
    roundings (any two correct bf16 implementations differ by more than the tolerance), so 2.5 is as discriminating as this test can be."""
    Q_GAIN, B, S0, n_new = 2.5, 8, 7780, 12
    cfg = dataclasses.replace(O.OracleConfig(), eos_token_id=-1)
    w = O.make_weights(cfg, seed=1234)
    D = cfg.hidden
    for i in range(cfg.n_layer):
        p = f"{O.P_DEC}h.{i}.attn.c_attn."
        w[p + "weight"][:D] = (w[p + "weight"][:D].float() * Q_GAIN).to(torch.bfloat16).to(w[p + "weight"].dtype)
        w[p + "bias"][:D] = (w[p + "bias"][:D].float() * Q_GAIN).to(torch.bfloat16).to(w[p + "bias"].dtype)
    eng = build_engine(cfg, w, max_batch=B, max_seq_len=7808)
    w_dev = {k: v.to(dev()) for k, v in w.items() if "image_encoder" not in k and "image_projection" not in k}
    del w
    gc.collect()
    emb = _synthetic_prompt(B, S0, cfg.hidden, 8780)
    o_toks, o_lg, cache = _oracle_long(w_dev, cfg, emb, n_new, 2)
    tag = f"config2 dims, B={B}, q x {Q_GAIN:g}, context {S0}->{S0 + n_new}"
    _teacher_forced_long(eng, emb, o_toks, o_lg, tag, 0.1, max_near=0.2)
    with torch.no_grad():
        ref_next, _ = O.decoder_decode_step(w_dev, cfg, o_toks[:, -1], cache, "bf16")
    tol_abs = LOGIT_TOL * float(o_lg.abs().max())
    last_page = (S0 + n_new - 2) // 64
    sens = [_page_swap_sensitivity(w_dev, cfg, cache, o_toks[:, -1], ref_next.float(), pg, 0, tol_abs) for pg in (last_page - 1, 61, 7)]
    print(f"[{tag}] sensitivity: swapping KV page {last_page - 1} / 61 / 7 for page 0 in every layer moves the oracle's logits by "
          f"{sens[0]:.1f} / {sens[1]:.1f} / {sens[2]:.1f} x the tolerance")
    assert min(sens) >= 1.5 and max(sens) >= 5.0, sens          # measured 16.5 / 2.1 / 5.2 (the unscaled case: ~1.0 each)
    eng.close()
    del w_dev, cache
    gc.collect(); torch.cuda.empty_cache()


def test_starvector_8b_dims_window_4096_at_long_context():
    """StarVector-8B dimensions (hidden 4608, 36 / 4 heads, RoPE, sliding_window = 4096 -- the real value), two StarCoder2 layers deep, B = 4:
    prompt of 4090 rows (the windowed prompt pass) then 30 decode steps to context 4120, where the window masks real keys."""
    cfg = dataclasses.replace(O.OracleConfig.starvector_8b(), eos_token_id=-1, n_layer=2, vit_layers=1)
    B, S0, n_new = 4, 4090, 30
    ec = sva.EngineConfig.starvector_8b(max_batch=B, max_seq_len=4160)
    ec.n_layer, ec.vit_layers = 2, 1
    eng = sva.HipEngine(ec)
    w_dev = {}
    for name, tns in O.iter_weights(cfg, seed=77, init="parity", device=dev()):
        eng.load_weight(name, tns.to(torch.bfloat16))
        if "image_encoder" not in name and "image_projection" not in name:
            w_dev[name] = tns
    eng.load_state_dict({})
    w_dev[O.K_LMH] = w_dev[O.embed_key(cfg)]
    emb = _synthetic_prompt(B, S0, cfg.hidden, 4608)
    o_toks, o_lg, cache = _oracle_long(w_dev, cfg, emb, n_new, 1)
    tag = "8B dims, 2 layers, window 4096, context 4090->4120"
    _teacher_forced_long(eng, emb, o_toks, o_lg, tag, 0.6)
    # the window matters here: the same oracle WITHOUT it gives other logits at the last step
    cfg_nw = dataclasses.replace(cfg, sliding_window=0)
    with torch.no_grad():
        a, _ = O.decoder_decode_step(w_dev, cfg, o_toks[:, -1], cache, "bf16")
        b, _ = O.decoder_decode_step(w_dev, cfg_nw, o_toks[:, -1], cache, "bf16")
    print(f"[{tag}] window on/off moves the oracle's logits by {float((a - b).abs().max()) / (LOGIT_TOL * float(o_lg.abs().max())):.2f} x the tolerance")
    eng.close()
    del w_dev, cache
    gc.collect(); torch.cuda.empty_cache()


def test_beam_search_kv_reindex_across_the_4096_boundary():
    """Beam search (num_beams 3) from a 4085-row prompt for 30 tokens: the beams' shared full pages, the private tail page and its copy when
    a beam changes parent run at block-table index 63 -> 64 (4096 tokens).  Tiny decoder with n_positions 8192 and a sharpened query
    projection (x8: peaked attention, so a stale tail page costs what it costs at short contexts); the recorded search is replayed
    through the oracle."""
    from tests.test_gpu_beam import _replay
    cfg = dataclasses.replace(O.OracleConfig.tiny(), n_positions=8192, eos_token_id=-1)
    w = O.make_weights(cfg, seed=4096)
    for i in range(cfg.n_layer):
        k = f"{O.P_DEC}h.{i}.attn.c_attn.weight"
        w[k] = w[k].clone()
        w[k][:cfg.hidden] *= 8.0
    B, nb, S0, n_new = 2, 3, 4085, 30
    eng = build_engine(cfg, w, B * nb, 4160)
    emb = _synthetic_prompt(B, S0, cfg.hidden, 31)
    toks = eng.generate(emb, max_length=S0 + n_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id, num_beams=nb, early_stopping=True).cpu()
    assert toks.shape == (B, n_new)
    hp, ht = eng.beam_history()
    assert (hp[1:] != torch.arange(nb).repeat(B)).any(), "case must exercise beams switching parents"
    short = _replay(w, cfg, emb.float().cpu(), nb, hp, ht)                    # the oracle on the host: 6 rows x 2 layers
    worst = max(short)
    print(f"[beam across 4096] worst shortfall {worst:.4f} nats over {n_new} steps at contexts {S0}..{S0 + n_new} (mean {sum(short) / len(short):.4f})")
    assert worst < 0.25, f"engine kept a continuation {worst:.3f} nats worse than the oracle's choice"
    assert torch.equal(eng.generate(emb, max_length=S0 + n_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id, num_beams=nb,
                                    early_stopping=True).cpu(), toks)
    eng.close()
