"""-m gpu: the whole hot path through the C ABI against (a) the golden vectors minted from the reference
and (b) the CPU oracle on the same seeded inputs; plus size-independent properties at StarVector-1B shapes.

Stated tolerances (floating point path, bf16 storage / fp32 accumulation):
  * module outputs vs the float32 reference golden: max|err| <= 3e-2 * max|ref|  (bf16 has 8 mantissa bits;
    23+24 layers of bf16 rounding);
  * logits vs the oracle's bf16 mode (same cast points): max|err| <= LOGIT_TOL * max|logit|, LOGIT_TOL = 1.8e-2
    = the worst error measured over ALL full-size cases on bf16 weights + 20 %: 1.52e-2 of the scale at BASELINE config 4
    (StarVector-8B, 16 rows, 578-row prompt, tests/test_gpu_configs45.py); config 2 at B = 32 measures 1.40e-2, its long contexts
    (259 .. 7800) 1.32e-2 .. 1.46e-2, 8B at 2 rows 1.25e-2 (profiles/pytest_gpu_r06_final.log).  At |logit| ~ 4.5 that is two bf16 ulps (the
    reference's own bf16 lm_head quantises logits at 2^-8 relative, so north_star's absolute 1e-3 is below the
    resolution of O(1) bf16 logits; DESIGN.md section "Parity").  fp8 weights (not a reference numerics mode; checked
    against oracle.fake_quantize_fp8): LOGIT_TOL_FP8 = 2.6e-2 = measured 2.13e-2 (StarVector-8B, full depth, 64 rows x 12 steps:
    config 5 at its batch size, tests/test_gpu_configs45.py; 1.77e-2 at 2 rows) + 20 %;
  * token ids: bit-exact wherever the oracle's top-1/top-2 margin exceeds twice the logit tolerance; a
    mismatch inside that band is a legitimate near-tie and is reported, anything outside fails."""
import dataclasses
import os

import pytest
import torch
from safetensors.torch import load_file

from oracle import starvector_oracle as O
from oracle.hostinfo import host_cores
from starvector_amd import engine as E
from tests.gpu_util import bf, build_engine, dev, rel_err

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1.8e-2
LOGIT_TOL_FP8 = 2.6e-2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(name):
    return load_file(os.path.join(ROOT, "tests", "golden", name + ".safetensors"))


def _teacher_forced_check(eng, emb, w, cfg, n_new):
    """Feed the ORACLE's greedy tokens step by step; at every step compare logits and argmax."""
    S0 = emb.shape[1]
    o_emb = emb.float().cpu()
    o_toks, o_lg = O.greedy_generate(w, cfg, o_emb, S0 + n_new, mode="bf16", return_logits=True)
    scale = float(o_lg.abs().max())
    top2 = o_lg.topk(2, -1).values
    margin = top2[..., 0] - top2[..., 1]
    worst, checked, near_ties = 0.0, 0, 0
    for t in range(o_toks.shape[1]):
        lg = eng.prefill(emb) if t == 0 else eng.decode_step(o_toks[:, t - 1].to(dev()))
        lg = lg.float().cpu()
        err = float((lg - o_lg[:, t]).abs().max())
        worst = max(worst, err)
        assert err <= LOGIT_TOL * scale, f"step {t}: logits off by {err:.3e} (scale {scale:.3e})"
        am = lg.argmax(-1)
        for b in range(am.shape[0]):
            if margin[b, t] > 2 * LOGIT_TOL * scale:
                assert am[b] == o_toks[b, t], f"row {b} step {t}: token {int(am[b])} != {int(o_toks[b, t])} at margin {margin[b, t]:.3e}"
                checked += 1
            elif am[b] != o_toks[b, t]:
                near_ties += 1
    return worst, scale, checked, near_ties, o_toks, margin


@pytest.mark.parametrize("name,norm", [("tiny_b3", "layer_norm"), ("tiny_bn_b2", "batch_norm")])
def test_against_reference_goldens(name, norm):
    g = _golden(name)
    seed, B, n_new = [int(x) for x in g["meta"]]
    cfg = dataclasses.replace(O.OracleConfig.tiny(), adapter_norm=norm)
    w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)
    eng = build_engine(cfg, w, max_batch=4, max_seq_len=64)
    enc = eng.encode_image(bf(g["image"]))
    vis = eng.adapter(enc)
    emb = torch.cat([vis, eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    logits0 = eng.prefill(emb)
    assert rel_err(enc, g["enc"]) <= 3e-2
    assert rel_err(vis, g["vis"]) <= 3e-2
    assert rel_err(emb, g["emb"]) <= 3e-2
    assert rel_err(logits0, g["logits0"]) <= 5e-2
    # embedding lookup is a pure gather of bf16-exact values: bit-exact
    assert torch.equal(emb[:, -2:].float().cpu(), w[O.P_DEC + "wte.weight"][g["prompt_ids"]])
    worst, scale, checked, near, o_toks, margin = _teacher_forced_check(eng, emb, w, cfg, n_new)
    assert checked > 0
    print(f"[{name}] logits max|err| {worst:.3e} (scale {scale:.3e}); {checked} token positions checked exactly, "
          f"{near} near-tie flips")
    if "wte" in g:
        # tiny_b3: the designed stream (fitted embedding table, margins >= 0.25 x the logit scale, 37 distinct tokens).  EVERY
        # position is checked, and the free-running engine reproduces HF generate token for token -- no margin filter.
        assert checked == B * n_new and near == 0
        toks = eng.generate(emb, max_length=emb.shape[1] + n_new, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id).cpu()
        assert torch.equal(toks, g["tokens"])
    eng.close()


def test_seven_launch_layer_mask_matches_the_golden():
    """SV_EXP_NO_LN_FOLD on the tiny golden engine, which takes the 6-launch layer by default (bf16, 3 rows, widths multiples of 32): the
    captured step grows by launches, and the 7-launch layer meets what the default mask meets in test_against_reference_goldens -- the
    oracle's logits within LOGIT_TOL at every teacher-forced step and HF generate's tokens.  Not compared bit for bit with mask 0: the fold
    re-rounds gamma * W."""
    g = _golden("tiny_b3")
    seed, B, n_new = [int(x) for x in g["meta"]]
    cfg = O.OracleConfig.tiny()
    w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)
    eng = build_engine(cfg, w, max_batch=4, max_seq_len=64)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    kw = dict(max_length=emb.shape[1] + n_new, eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id)
    assert torch.equal(eng.generate(emb, **kw).cpu(), g["tokens"])
    nodes6 = eng.step_plan()["graph_kernel_nodes"]
    eng.set_exp(E.Exp.NO_LN_FOLD)
    toks = eng.generate(emb, **kw).cpu()
    nodes7 = eng.step_plan()["graph_kernel_nodes"]
    print(f"[NO_LN_FOLD] kernel nodes per step: {nodes6} by default, {nodes7} with the switch ({cfg.n_layer} layers)")
    assert 0 < nodes6 < nodes7, "the tiny engine does not take the 6-launch layer by default"
    worst, scale, checked, near, o_toks, margin = _teacher_forced_check(eng, emb, w, cfg, n_new)
    print(f"[NO_LN_FOLD] logits max|err| {worst:.3e} (scale {scale:.3e}); {checked} token positions checked exactly")
    assert checked == B * n_new and near == 0
    assert torch.equal(toks, g["tokens"])
    eng.close()


def test_unknown_switch_bits_are_refused_and_the_skinny_form_survives_engine_creation():
    """sv_debug_set_exp with a bit that is no switch (a removed one; one past the known set) is SV_EINVAL and leaves the engine's mask as it
    was: the same tokens and the same step afterwards, under mask 0 and under a mask whose effect shows in the step plan.  The process-wide
    form of the 33..64-row decode GEMMs belongs to sv_debug_set_skinny_form alone: creating an engine no longer resets it."""
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=21)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(33, 256, generator=gen).bfloat16().float()
    W = (torch.randn(96, 256, generator=gen) / 16).bfloat16().float()
    known = int(E.Exp.known())
    try:
        E.set_skinny_form(0)
        before = E.op_linear_skinny(bf(x), bf(W), None, splitk=2)
        eng = build_engine(cfg, w, 4, 64)                                   # sv_create in between
        assert E.skinny_form() == 0, "sv_create changed the form sv_debug_set_skinny_form set"
        assert torch.equal(E.op_linear_skinny(bf(x), bf(W), None, splitk=2), before)
        emb = torch.cat([eng.adapter(eng.encode_image(bf(O.synthetic_images(2, cfg.image_size, seed=22)))),
                         eng.embed_tokens(torch.tensor([[7, 11]] * 2, device=dev()))], 1)
        kw = dict(max_length=emb.shape[1] + 8, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
        for mask in (E.Exp(0), E.Exp.SEPARATE_ARGMAX | E.Exp.NO_LN_FOLD):
            eng.set_exp(mask)
            toks, plan = eng.generate(emb, **kw).cpu(), eng.step_plan()
            for bad in (16, known | (1 << 20)):
                with pytest.raises(ValueError, match=str(bad & ~known)):    # the message names the offending bit
                    eng.set_exp(bad)
                assert torch.equal(eng.generate(emb, **kw).cpu(), toks) and eng.step_plan() == plan, (mask, bad)
        assert E.skinny_form() == 0                                         # nor does sv_debug_set_exp touch it
        eng.close()
    finally:
        E.set_skinny_form(1)


def test_generate_semantics_eos_pad_stop_on_device():
    """HF semantics restated on device: pad after EOS, the row-0 stop sequence ends the WHOLE batch, only new
    tokens are returned.  The golden comes from HF generate + the reference's StoppingCriteriaSub."""
    g = _golden("tiny_stop")
    seed, B, n_new, eos = [int(x) for x in g["meta"]]
    cfg = dataclasses.replace(O.OracleConfig.tiny(), eos_token_id=eos)
    w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)      # designed stream: margins >= 0.25 x the logit scale
    eng = build_engine(cfg, w, 4, 64)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    S0 = emb.shape[1]
    stop = g["stop_ids"].tolist()
    toks = eng.generate(emb, max_length=S0 + n_new, eos_token_id=eos, pad_token_id=cfg.pad_token_id, stop_ids=stop).cpu()
    assert torch.equal(toks, g["tokens"])                          # identical to HF generate, incl. early stop + pads
    assert toks.shape[1] == 11 and (toks[1] == cfg.pad_token_id).sum() == 6 and toks[0, -2:].tolist() == stop
    # structural semantics, restated:
    assert toks.shape[0] == B and 1 <= toks.shape[1] <= n_new
    for b in range(B):
        row = toks[b].tolist()
        if eos in row:
            i = row.index(eos)
            assert all(t == cfg.pad_token_id for t in row[i + 1:])  # pad after EOS
    if toks.shape[1] < n_new:                                       # ended early: row-0 stop fired or all rows finished
        r0 = toks[0].tolist()
        assert r0[-len(stop):] == stop or all((eos in toks[b].tolist()) for b in range(B))
    # budget semantics: max_length includes the prompt
    assert eng.generate(emb, max_length=S0 + 3, eos_token_id=-1, pad_token_id=0).shape == (B, 3)
    with pytest.raises(ValueError):
        eng.generate(emb, max_length=S0, eos_token_id=-1, pad_token_id=0)
    eng.close()


def test_generate_is_deterministic_graph_equals_eager_and_batch_invariant():
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=21)
    eng = build_engine(cfg, w, 8, 96)
    img = bf(O.synthetic_images(6, cfg.image_size, seed=22))
    prompt = torch.tensor([[7, 11]] * 6, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    S0 = emb.shape[1]
    kw = dict(max_length=S0 + 40, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    os.environ.pop("SV_NO_GRAPH", None)
    a = eng.generate(emb, **kw).cpu()
    assert eng.last_timing()["graph"], "decode step did not run as a hipGraph replay"
    assert eng.last_timing()["graph_steps"] == 1                   # 39 steps < 4 polling chunks of 32: one step per launch
    b = eng.generate(emb, **kw).cpu()
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        c = eng.generate(emb, **kw).cpu()
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    assert torch.equal(a, b) and torch.equal(a, c)                 # bit-exact integer streams
    # every sequence is independent: a row generated alone equals the same row inside the batch
    solo = eng.generate(emb[2:3].contiguous(), **kw).cpu()
    assert torch.equal(solo[0], a[2])
    # sync_every only changes when the host looks at the done flag, never the tokens
    assert torch.equal(a, eng.generate(emb, sync_every=3, **kw).cpu())
    # several steps per graph launch (round 6: a call with >= 4 polling chunks in front of it replays the step `sync_every` times per
    # hipGraphLaunch): 39 steps at sync_every 8 = 4 launches of the 8-step graph + 7 of the one-step graph -- the same tokens; greedy,
    # sampled, and with an EOS that ends rows in the middle of a chunk
    assert eng.last_timing()["graph_steps"] == 3                   # (the sync_every = 3 call above already ran 13 launches of a 3-step graph)
    m8 = eng.generate(emb, sync_every=8, **kw).cpu()
    assert eng.last_timing()["graph_steps"] == 8 and torch.equal(a, m8)
    assert torch.equal(a, eng.generate(emb, sync_every=8, **kw).cpu())          # the kept 8-step graph, replayed by the next call
    skw = dict(do_sample=True, temperature=1.0, top_p=0.9, top_k=20, seed=5)
    s1 = eng.generate(emb, sync_every=1, **skw, **kw).cpu()
    assert eng.last_timing()["graph_steps"] == 1
    s8 = eng.generate(emb, sync_every=8, **skw, **kw).cpu()
    assert eng.last_timing()["graph_steps"] == 8 and torch.equal(s1, s8)
    eos = int(a[1, 13])
    e1 = eng.generate(emb, sync_every=1, max_length=S0 + 40, eos_token_id=eos, pad_token_id=cfg.pad_token_id).cpu()
    e8 = eng.generate(emb, sync_every=8, max_length=S0 + 40, eos_token_id=eos, pad_token_id=cfg.pad_token_id).cpu()
    assert torch.equal(e1, e8)
    # the reference's row-0 stop sequence (starvector_base.py:9-20) firing inside a chunk of the 8-step graph: the call ends at the same column
    stop = [int(a[0, 17]), int(a[0, 18])]
    t1 = eng.generate(emb, sync_every=1, stop_ids=stop, **kw).cpu()
    t8 = eng.generate(emb, sync_every=8, stop_ids=stop, **kw).cpu()
    assert torch.equal(t1, t8) and t1.shape[1] <= 19
    eng.close()


def test_kept_graphs_are_kept_and_replaced_across_plain_sampled_and_lookup_calls():
    """The engine's graph slots through their keep and replace paths in ONE engine: a greedy call that builds the one-step and a 2-step graph
    (39 steps >= 4 x sync_every 2), the same call again (both replayed), two sampled calls (another key, then another seed: both plain graphs
    replaced), a lookup call (a slot of its own), the first call again (captured afresh).  Every call returns the tokens of the same call
    launched eagerly (SV_NO_GRAPH=1) on the same engine; the last call returns the first one's bit for bit."""
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=21)
    eng = build_engine(cfg, w, 32, 128)
    img = bf(O.synthetic_images(3, cfg.image_size, seed=22))
    prompt = torch.tensor([[7, 11]] * 3, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    kw = dict(max_length=emb.shape[1] + 40, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    skw = dict(do_sample=True, temperature=1.0, top_p=0.9, top_k=20)
    calls = {"greedy": lambda: eng.generate(emb, sync_every=2, **kw),
             "seed3": lambda: eng.generate(emb, seed=3, **skw, **kw),
             "seed4": lambda: eng.generate(emb, seed=4, **skw, **kw),
             "lookup": lambda: eng.generate_lookup(emb, num_draft_tokens=3, **kw)}
    order = ["greedy", "greedy", "seed3", "seed4", "lookup", "greedy"]
    os.environ.pop("SV_NO_GRAPH", None)
    got, steps, nodes = [], [], []
    for name in order:
        got.append(calls[name]().cpu())
        assert eng.last_timing()["graph"], f"{name}: the decode step did not run as a hipGraph replay"
        steps.append(eng.last_timing()["graph_steps"])
        nodes.append(eng.step_plan()["graph_kernel_nodes"])
    assert steps == [2, 2, 1, 1, 1, 2]          # (a sampled call at sync_every 32 and a lookup call launch one step per graph)
    assert nodes[0] > 0 and nodes[1] == nodes[0] and nodes[5] == nodes[0]
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        eager = {name: call().cpu() for name, call in calls.items()}
        assert not eng.last_timing()["graph"]
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    for name, toks in zip(order, got):
        assert toks.shape == (3, 40) and torch.equal(toks, eager[name]), name
    assert torch.equal(got[5], got[0]) and not torch.equal(eager["seed3"], eager["seed4"])
    eng.close()


def test_prompts_of_259_rows_are_batch_independent_with_the_per_sequence_remainder():
    """StarVector-1B's dimensions at reduced depth, 224 x 224 images -> 257 vision tokens + 2 prompt ids = 259 prompt rows: the GEMM remainder of every
    sequence (3 of 259 rows, 1 of 257 tokens) runs through the split-K remainder kernel where gemm_seq_form holds (round 6, gemm.hip).  Which kernel computes
    a row depends on its position in its SEQUENCE only: a request alone, at another place of the batch and in a batch of another size gives the same vision
    tokens, the same first-token logits and the same tokens, bit for bit; the pruned last prompt layer equals the full one (SV_EXP bit 32768);
    and against the batch-level remainder of rounds 2-5 (bit 4194304: another summation order for those rows -- some bf16 roundings downstream flip) the
    logits stay inside the suite's tolerance."""
    cfg = dataclasses.replace(O.OracleConfig(), n_layer=3, vit_layers=3, eos_token_id=-1)      # the defaults are StarVector-1B
    w = O.make_weights(cfg, seed=77)
    B = 5
    eng = build_engine(cfg, w, B, 259 + 24)
    img = bf(O.synthetic_images(B, cfg.image_size, seed=78))
    prompt = torch.tensor([[7, 11]] * B, device=dev())
    assert E.gemm_seq_form(259, cfg.hidden, cfg.hidden) and E.gemm_seq_form(257, cfg.vit_width, cfg.vit_width)

    def run(im, pr):
        enc = eng.encode_image(im)
        emb = torch.cat([eng.adapter(enc), eng.embed_tokens(pr)], 1)
        assert emb.shape[1] == 259
        lg = eng.prefill(emb).float().cpu()
        toks = eng.generate(emb, max_length=259 + 12, eos_token_id=-1, pad_token_id=cfg.pad_token_id).cpu()
        return enc.cpu(), lg, toks

    enc_a, lg_a, tok_a = run(img, prompt)
    enc_s, lg_s, tok_s = run(img[3:4].contiguous(), prompt[3:4].contiguous())                       # alone
    assert torch.equal(enc_s[0].view(torch.int16), enc_a[3].view(torch.int16))
    assert torch.equal(lg_s[0], lg_a[3]) and torch.equal(tok_s[0], tok_a[3])
    perm = torch.tensor([4, 2, 0], device=dev())                                                   # another batch size, another order
    enc_p, lg_p, tok_p = run(img[perm].contiguous(), prompt[perm].contiguous())
    for i, j in enumerate(perm.tolist()):
        assert torch.equal(enc_p[i].view(torch.int16), enc_a[j].view(torch.int16))
        assert torch.equal(lg_p[i], lg_a[j]) and torch.equal(tok_p[i], tok_a[j])
    try:
        eng.set_exp(32768)                                                                          # the last prompt layer on all rows
        _, lg_full, tok_full = run(img, prompt)
        assert torch.equal(lg_full, lg_a) and torch.equal(tok_full, tok_a)
        eng.set_exp(4194304)                                                                        # the batch-level remainder (whole-K order for every row)
        _, lg_old, _ = run(img, prompt)
    finally:
        eng.set_exp(0)
    d = float((lg_old - lg_a).abs().max() / lg_a.abs().max())
    print(f"[seq remainder e2e] 1B dims, 3 + 3 layers, B = {B}: solo / permuted / pruned-vs-full bit-identical; per-sequence vs batch-level remainder: "
          f"first-token logits differ by {d:.2e} of max|logit|")
    assert d < LOGIT_TOL
    eng.close()


def test_sampling_path_runs_and_respects_nucleus():
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=31)
    eng = build_engine(cfg, w, 4, 64)
    img = bf(O.synthetic_images(2, cfg.image_size, seed=32))
    prompt = torch.tensor([[7, 11]] * 2, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    S0 = emb.shape[1]
    s1 = eng.generate(emb, max_length=S0 + 12, do_sample=True, temperature=0.7, top_p=0.9, eos_token_id=-1, pad_token_id=0, seed=5).cpu()
    s2 = eng.generate(emb, max_length=S0 + 12, do_sample=True, temperature=0.7, top_p=0.9, eos_token_id=-1, pad_token_id=0, seed=5).cpu()
    s3 = eng.generate(emb, max_length=S0 + 12, do_sample=True, temperature=0.7, top_p=0.9, eos_token_id=-1, pad_token_id=0, seed=6).cpu()
    assert torch.equal(s1, s2) and not torch.equal(s1, s3) and s1.shape == (2, 12)
    # first sampled token must lie in the oracle's nucleus of the prefill logits
    lg = eng.prefill(emb).float().cpu()
    probs = O.top_p_filtered_probs(lg, 0.7, 0.9)
    # allow the boundary token: compare against a slightly wider nucleus
    wide = O.top_p_filtered_probs(lg, 0.7, 0.93)
    for b in range(2):
        assert wide[b, s1[b, 0]] > 0
    # top_p -> 0 degenerates to greedy
    greedy = eng.generate(emb, max_length=S0 + 12, eos_token_id=-1, pad_token_id=0).cpu()
    tiny_p = eng.generate(emb, max_length=S0 + 12, do_sample=True, temperature=1.0, top_p=1e-6, eos_token_id=-1, pad_token_id=0).cpu()
    assert torch.equal(greedy, tiny_p)
    eng.close()


def test_drop_in_api_generate_im2svg():
    """The reference's public call sequence (scripts/quickstart.py:9-19) on the mirror classes."""
    import starvector_amd as sva
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=41)
    scfg = sva.StarVectorConfig(image_size=cfg.image_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.n_layer,
                                num_attention_heads=cfg.n_head, vocab_size=cfg.vocab - 4, n_inner=cfg.n_inner,
                                n_positions=cfg.n_positions, max_length=cfg.n_positions, vit_width=cfg.vit_width,
                                vit_layers=cfg.vit_layers, vit_heads=cfg.vit_heads, max_batch=4)
    model = sva.StarVectorForCausalLM(scfg, state_dict={k: v.to(torch.bfloat16) for k, v in w.items()})
    model.eval()
    from PIL import Image
    pil = Image.new("RGB", (cfg.image_size, cfg.image_size), (200, 30, 30))
    image = model.process_images([pil, pil])
    batch = {"image": torch.cat(image, 0).to(dev())}
    S0 = model.model.query_length + 4                                  # '<svg' = 4 byte tokens
    out = model.generate_im2svg(batch, max_length=S0 + 10, num_beams=1, use_nucleus_sampling=False)
    assert isinstance(out, list) and len(out) == 2 and all(isinstance(s, str) for s in out)
    assert all(s.startswith("<svg") for s in out)                      # prompt ids are prepended (starvector_base.py:256)
    assert out[0] == out[1]                                            # identical images -> identical streams
    res = model.model.generate_im2svg_grpo(batch, max_length=S0 + 10, num_beams=1, use_nucleus_sampling=False)
    assert res["outputs"].shape == (2, 4 + 10) and res["inputs_embeds"].shape == (2, S0, cfg.hidden)
    many = model.model.generate_im2svg_grpo(batch, max_length=S0 + 10, num_return_sequences=2, use_nucleus_sampling=True,
                                            temperature=1.0, top_p=0.95)            # GRPO sampling: 2 sequences per image
    assert many["outputs"].shape == (4, 4 + 10) and len(many["raw_svg"]) == 4
    assert not torch.equal(many["outputs"][0], many["outputs"][1])     # copies of one image are sampled independently
    dflt = model.generate_im2svg(batch, max_length=S0 + 10)            # the reference's defaults: num_beams=2 + nucleus sampling
    assert len(dflt) == 2 and all(s.startswith("<svg") for s in dflt)
    beams = model.generate_im2svg(batch, max_length=S0 + 10, num_beams=2, use_nucleus_sampling=False)
    assert len(beams) == 2 and beams[0] == beams[1] and beams[0].startswith("<svg")
    # text2svg (starvector_base.py:297-330 by intent): caption ids + <svg-start> -> new token ids, budget = max_length - prompt
    cap = {"caption": ["a red square", "a red square"], "image": batch["image"]}
    t2s = model.model.generate_text2svg(cap, max_length=13 + 9, num_beams=1, use_nucleus_sampling=False)
    assert t2s.shape[0] == 2 and 1 <= t2s.shape[1] <= 9 and torch.equal(t2s[0], t2s[1])
    # captions of different lengths: the tokenizer pads, HF masks the pads and numbers positions by cumsum(mask) -- i.e. every
    # row behaves like the same row alone (pinned against HF on CPU); the mirror generates the rows group by group
    caps = ["short", "a much longer caption", "short"]
    mixed = model.model.generate_text2svg({"caption": caps, "image": batch["image"]}, max_length=40, num_beams=1,
                                          use_nucleus_sampling=False)
    padded_len = max(len(c.encode()) for c in caps) + 1                 # longest caption + <svg-start>
    assert mixed.shape == (3, 40 - padded_len) and torch.equal(mixed[0], mixed[2])
    for i in (0, 1):
        solo = model.model.generate_text2svg({"caption": [caps[i]], "image": batch["image"][:1]},
                                             max_length=len(caps[i].encode()) + 1 + mixed.shape[1], num_beams=1,
                                             use_nucleus_sampling=False)
        assert torch.equal(solo[0], mixed[i])
    # module-level operator signatures
    enc = model.model.image_encoder(batch["image"].to(torch.bfloat16))
    assert enc.shape == (2, model.model.query_length, cfg.vit_width)
    assert model.model.image_projection(enc).shape == (2, model.model.query_length, cfg.hidden)
    with pytest.raises(ValueError):
        model.model.image_encoder(batch["image"].to(torch.bfloat16)[:, :, :8])
    with pytest.raises(ValueError):
        model.model.image_encoder(torch.zeros(1, 3, cfg.image_size, cfg.image_size))      # CPU tensor: no CPU path


def _stream_equal_until_band(got, o_toks, margin, band):
    """A free-running stream may leave the oracle's only AT a position whose top-1/top-2 margin is inside the tolerance band
    (a legitimate bf16 near-tie; after it the two contexts differ and nothing can be compared).  Returns, per row, the
    number of leading positions that are identical."""
    n = []
    for b in range(got.shape[0]):
        diff = (got[b] != o_toks[b]).nonzero()
        t = int(diff[0]) if diff.numel() else got.shape[1]
        if t < got.shape[1]:
            assert margin[b, t] <= band, (f"row {b} step {t}: engine token {int(got[b, t])} != oracle {int(o_toks[b, t])} "
                                          f"at margin {float(margin[b, t]):.3e} (band {band:.3e}); leading identical positions of "
                                          f"the rows before it: {n} of {got.shape[1]}")
        n.append(t)
    return n


def test_starvector_1b_shapes_against_oracle():
    """BASELINE config 2 shapes (StarVector-1B, bf16), B = 2, 130 new tokens: the context runs 259 -> 389, i.e. through the
    KV page boundaries at 320 and 384.  Teacher-forced logits at EVERY step against the oracle (bf16 cast points); token ids
    bit-exact at every position whose margin clears the band, which must be >= 95 % of the 260 positions; the free-running
    engine stream equals the oracle's up to the first in-band position; the same free-running check with a repetition
    penalty (a diverse stream: random-init greedy streams repeat one token)."""
    torch.set_num_threads(host_cores())
    cfg = dataclasses.replace(O.OracleConfig(), eos_token_id=-1)
    w = O.make_weights(cfg, seed=1234)
    B, n_new = 2, 130
    eng = build_engine(cfg, w, max_batch=2, max_seq_len=259 + n_new + 8)
    img = O.synthetic_images(B, 224, seed=1235)
    prompt = torch.tensor([[7, 11]] * B)
    enc = eng.encode_image(bf(img))
    vis = eng.adapter(enc)
    emb = torch.cat([vis, eng.embed_tokens(prompt.to(dev()))], 1)
    S0 = emb.shape[1]
    assert S0 == 259 and S0 + n_new > 384
    o_enc = O.image_encoder_forward(w, cfg, img, "bf16")
    o_vis = O.adapter_forward(w, cfg, o_enc, "bf16")
    e1, e2 = rel_err(enc, o_enc), rel_err(vis, o_vis)
    print(f"[1b] encoder rel err {e1:.3e}, adapter rel err {e2:.3e}")
    assert e1 <= 4e-2 and e2 <= 4e-2
    worst, scale, checked, near, o_toks, margin = _teacher_forced_check(eng, emb, w, cfg, n_new)
    print(f"[1b] {n_new} steps x {B} rows: logits max|err| {worst:.3e} (scale {scale:.3e}); {checked}/{B * n_new} positions "
          f"token-exact outside the band, {near} near-tie flips inside it; min margin {float(margin.min()):.3e}")
    assert checked >= 0.95 * B * n_new
    kw = dict(max_length=S0 + n_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    got = eng.generate(emb, **kw).cpu()
    lead = _stream_equal_until_band(got, o_toks, margin, 2 * LOGIT_TOL * scale)
    print(f"[1b] free-running greedy stream == oracle for the first {lead} positions per row (of {n_new}); a row may only "
          f"leave the oracle's stream at an in-band near-tie")
    # a diverse stream: repetition penalty 1.3 (HF RepetitionPenaltyLogitsProcessor, pinned by tests/golden/tiny_reppen)
    n2, pen = 24, 1.3
    p_toks, p_sc = O.greedy_generate(w, cfg, emb.float().cpu(), S0 + n2, mode="bf16", return_logits=True, repetition_penalty=pen)
    top2 = p_sc.topk(2, -1).values
    got2 = eng.generate(emb, max_length=S0 + n2, eos_token_id=-1, pad_token_id=cfg.pad_token_id, repetition_penalty=pen).cpu()
    lead2 = _stream_equal_until_band(got2, p_toks, top2[..., 0] - top2[..., 1], 2 * LOGIT_TOL * float(p_sc.abs().max()))
    print(f"[1b] repetition_penalty {pen}: {len(set(p_toks.flatten().tolist()))} distinct tokens; stream == oracle for the first {lead2} positions")
    eng.close()


def _rms(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())


def _comparator_case(cfg, w, img, prompt, n_steps, tag):
    """errors against the float32 oracle of (a) the engine and (b) a REAL bf16 execution of the same modules by torch on this
    GPU (ATen / rocBLAS bf16 kernels; the decoder is HF's own class): the engine may not be further from float32 than
    1.5 x what torch's bf16 is (relative RMS; the maxima are reported too)."""
    from tests.gpu_util import hf_decoder_bf16, hf_teacher_forced_logits
    B = img.shape[0]
    o_enc = O.image_encoder_forward(w, cfg, img)
    o_vis = O.adapter_forward(w, cfg, o_enc)
    o_emb = O.prepare_generation_inputs(w, cfg, img, prompt)
    o_toks, o_lg = O.greedy_generate(w, cfg, o_emb, o_emb.shape[1] + n_steps, return_logits=True)       # float32 reference
    wb = {k: v.to(torch.bfloat16).to(dev()) for k, v in w.items() if not k.startswith("model.svg_transformer")}
    with torch.no_grad():
        t_enc = O.image_encoder_forward(wb, cfg, bf(img), "native")
        t_vis = O.adapter_forward(wb, cfg, t_enc, "native")
    lm = hf_decoder_bf16(cfg, w)
    wte = lm.get_input_embeddings()
    t_emb = torch.cat([t_vis, wte(prompt.to(dev()))], 1)
    t_lg = hf_teacher_forced_logits(lm, t_emb, wte, o_toks)
    del lm
    eng = build_engine(cfg, w, max_batch=max(B, 2), max_seq_len=o_emb.shape[1] + n_steps + 8)
    e_enc = eng.encode_image(bf(img))
    e_vis = eng.adapter(e_enc)
    e_emb = torch.cat([e_vis, eng.embed_tokens(prompt.to(dev()))], 1)
    rows = [eng.prefill(e_emb).float().cpu()]
    for t in range(1, o_toks.shape[1]):
        rows.append(eng.decode_step(o_toks[:, t - 1].to(dev())).float().cpu())
    e_lg = torch.stack(rows, 1)
    eng.close()
    out = {}
    for name, e, t, o in (("encoder", e_enc, t_enc, o_enc), ("adapter", e_vis, t_vis, o_vis), ("logits", e_lg, t_lg, o_lg)):
        re_, rt_ = _rms(e, o), _rms(t, o)
        me_, mt_ = rel_err(e, o), rel_err(t, o)
        out[name] = (re_, rt_, me_, mt_)
        print(f"[{tag}] {name:8s} vs float32: engine rms {re_:.3e} max {me_:.3e} | torch bf16 rms {rt_:.3e} max {mt_:.3e} | ratio {re_ / rt_:.2f}")
    return out


def test_engine_error_against_real_bf16_execution():
    """The tolerance is not self-chosen: a real torch.bfloat16 run of the reference's modules on the same GPU sets it."""
    torch.set_num_threads(host_cores())
    g = _golden("tiny_b3")
    seed, B, n_new = [int(x) for x in g["meta"]]
    cfg = O.OracleConfig.tiny()
    w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)
    res = _comparator_case(cfg, w, g["image"], g["prompt_ids"], n_new, "tiny")
    for name, (re_, rt_, me_, mt_) in res.items():
        assert re_ <= 1.5 * rt_, f"{name}: engine rms error {re_:.3e} > 1.5 x torch-bf16's {rt_:.3e}"
        assert me_ <= 2.5 * mt_, f"{name}: engine max error {me_:.3e} > 2.5 x torch-bf16's {mt_:.3e}"
    # StarVector-1B dims, one image, prefill + 6 teacher-forced steps
    cfg1 = dataclasses.replace(O.OracleConfig(), eos_token_id=-1)
    w1 = O.make_weights(cfg1, seed=1234)
    res = _comparator_case(cfg1, w1, O.synthetic_images(1, 224, seed=1235), torch.tensor([[7, 11]]), 7, "1b")
    for name, (re_, rt_, me_, mt_) in res.items():
        assert re_ <= 1.5 * rt_, f"1b {name}: engine rms error {re_:.3e} > 1.5 x torch-bf16's {rt_:.3e}"
        assert me_ <= 2.5 * mt_, f"1b {name}: engine max error {me_:.3e} > 2.5 x torch-bf16's {mt_:.3e}"


def test_full_size_properties_batch32():
    """Size-independent properties at the benchmark's full size (B=32, StarVector-1B): determinism,
    graph == eager, batch-invariance of a row, token range."""
    cfg = O.OracleConfig()
    w = O.make_weights(cfg, seed=7, init="std002")
    eng = build_engine(cfg, w, max_batch=64, max_seq_len=259 + 40)
    del w
    img = bf(O.synthetic_images(32, 224, seed=8))
    prompt = torch.tensor([[7, 11]] * 32, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    S0 = emb.shape[1]
    assert S0 == 259
    kw = dict(max_length=S0 + 32, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    a = eng.generate(emb, **kw).cpu()
    assert a.shape == (32, 32) and int(a.min()) >= 0 and int(a.max()) < cfg.vocab
    assert torch.equal(a, eng.generate(emb, **kw).cpu())
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        assert torch.equal(a, eng.generate(emb, **kw).cpu())
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    assert torch.equal(a[17], eng.generate(emb[17:18].contiguous(), **kw).cpu()[0])
    # batch 64 (BASELINE config 5's rows per GPU): the decode GEMMs run two row tiles per block (weights streamed once);
    # same tokens as with one tile per block, and a row of the second tile equals its solo run
    ids = torch.randint(0, cfg.vocab - 8, (64, 8), generator=torch.Generator().manual_seed(3)).to(dev())
    e64 = eng.embed_tokens(ids)
    kw64 = dict(max_length=8 + 24, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    t64 = eng.generate(e64, **kw64).cpu()
    assert t64.shape == (64, 24) and len({tuple(r.tolist()) for r in t64}) > 32
    for b in (5, 40, 63):
        assert torch.equal(t64[b], eng.generate(e64[b:b + 1].contiguous(), **kw64).cpu()[0]), b
    eng.close()


def test_more_than_one_row_tile_and_short_prompts():
    """B > 32 exercises the second 32-row tile of every decode kernel (BASELINE configs 3/5 use up to 64 rows per
    GPU); a text-only prompt (no visual rows) exercises S0 much smaller than a KV page."""
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=51)
    B = 40
    eng = build_engine(cfg, w, max_batch=B, max_seq_len=96)
    img = bf(O.synthetic_images(B, cfg.image_size, seed=52))
    prompt = torch.tensor([[7, 11]] * B, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    S0 = emb.shape[1]
    kw = dict(max_length=S0 + 20, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    full = eng.generate(emb, **kw).cpu()
    assert full.shape == (B, 20)
    for b in (0, 31, 32, 39):                                   # rows of both tiles equal their solo runs
        assert torch.equal(full[b], eng.generate(emb[b:b + 1].contiguous(), **kw).cpu()[0]), b
    # teacher-forced logits of row 35 (second tile) against the oracle
    o_toks, o_lg = O.greedy_generate(w, cfg, emb[35:36].float().cpu(), S0 + 6, mode="bf16", return_logits=True)
    lg0 = eng.prefill(emb)[35].float().cpu()
    assert float((lg0 - o_lg[0, 0]).abs().max()) <= LOGIT_TOL * float(o_lg.abs().max())
    # short prompt: 3 token embeddings only (generate_text2svg-style input)
    ids = torch.tensor([[5, 9, 13]] * 2, device=dev())
    e3 = eng.embed_tokens(ids)
    t3 = eng.generate(e3, max_length=3 + 70, eos_token_id=-1, pad_token_id=0).cpu()     # crosses a 64-token page
    assert t3.shape == (2, 70) and torch.equal(t3[0], t3[1])
    o3 = O.greedy_generate(w, cfg, e3[:1].float().cpu(), 3 + 4, mode="bf16", return_logits=True)[1]
    l3 = eng.prefill(e3)[0].float().cpu()
    assert float((l3 - o3[0, 0]).abs().max()) <= LOGIT_TOL * float(o3.abs().max())
    eng.close()


def _gen_with_env(env, cfg, w, emb_cpu, n_new):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = build_engine(cfg, w, max_batch=4, max_seq_len=96)       # the pipeline is chosen at sv_create
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    emb = emb_cpu.to(dev())
    toks = eng.generate(emb, max_length=emb.shape[1] + n_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id).cpu()
    return eng, emb, toks


def test_starvector_8b_op_graph_against_reference_golden():
    """SURVEY.md section 8a row a13 at reduced shapes: SigLIP tower (conv bias, no class token, GELU-tanh, post LN) +
    StarCoder2 decoder (fused q|k|v from three tensors, RoPE, GQA with 3 query heads per KV head, no position
    table).  Golden = HF SiglipVisionModel + Starcoder2ForCausalLM.generate (tests/golden/tiny_v2_b2)."""
    g = _golden("tiny_v2_b2")
    seed, B, n_new = [int(x) for x in g["meta"]]
    cfg = O.OracleConfig.tiny_v2()
    w = O.make_weights(cfg, seed=seed)
    eng = build_engine(cfg, w, max_batch=4, max_seq_len=96)
    enc = eng.encode_image(bf(g["image"]))
    vis = eng.adapter(enc)
    emb = torch.cat([vis, eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    assert enc.shape == (B, cfg.query_length, cfg.vit_width) and cfg.query_length == 16
    assert rel_err(enc, g["enc"]) <= 3e-2 and rel_err(vis, g["vis"]) <= 3e-2 and rel_err(emb, g["emb"]) <= 3e-2
    assert rel_err(eng.prefill(emb), g["logits0"]) <= 5e-2
    worst, scale, checked, near, o_toks, margin = _teacher_forced_check(eng, emb, w, cfg, n_new)
    assert checked > 0
    print(f"[tiny_v2] logits max|err| {worst:.3e} (scale {scale:.3e}); {checked} token positions checked exactly, {near} near-tie flips")
    # determinism + graph == eager + a longer decode crossing a KV page with RoPE positions
    kw = dict(max_length=emb.shape[1] + 70, eos_token_id=-1, pad_token_id=0)
    a = eng.generate(emb, **kw).cpu()
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        b2 = eng.generate(emb, **kw).cpu()
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    assert a.shape == (B, 70) and torch.equal(a, b2)
    assert torch.equal(a[1], eng.generate(emb[1:2].contiguous(), **kw).cpu()[0])
    eng.close()


def _assert_stream_vs_hf(got, hf_tokens, w, cfg, g):
    """HF's golden stream is the float32 oracle's stream (asserted); its float32 top-1/top-2 margins say where a correct bf16
    implementation may legitimately pick the other token.  Returns the leading identical positions per row."""
    o_emb = O.prepare_generation_inputs(w, cfg, g["image"], g["prompt_ids"])
    n = hf_tokens.shape[1]
    f_toks, f_lg = O.greedy_generate(w, cfg, o_emb, o_emb.shape[1] + n, return_logits=True)
    assert torch.equal(f_toks, hf_tokens), "the float32 oracle no longer reproduces HF's golden stream"
    top2 = f_lg.topk(2, -1).values
    return _stream_equal_until_band(got, hf_tokens, top2[..., 0] - top2[..., 1], 2 * LOGIT_TOL * float(f_lg.abs().max()))


def test_starcoder2_sliding_window():
    """StarCoder2 attends to the last `sliding_window` keys (4096 in bigcode/starcoder2-7b; 24 here).  Teacher-forced
    logits against the windowed oracle (pinned to HF by tests/golden/tiny_v2_window) for 80 steps: the window start
    moves through key groups and across a KV page, so skipped groups, skipped pages and the partially masked first
    group are all exercised.  An engine without the window must NOT pass the same check."""
    g = _golden("tiny_v2_window")
    seed, B, n_new, W = [int(x) for x in g["meta"]]
    cfg = dataclasses.replace(O.OracleConfig.tiny_v2(), sliding_window=W, eos_token_id=-1)
    w = O.make_weights(cfg, seed=seed)
    eng = build_engine(cfg, w, max_batch=4, max_seq_len=128)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    S0 = emb.shape[1]
    worst, scale, checked, near, o_toks, margin = _teacher_forced_check(eng, emb, w, cfg, 80)
    print(f"[v2 window] W={W} S0={S0}: logits max|err| {worst:.3e} (scale {scale:.3e}) over 80 steps; {checked} exact, {near} near-tie flips")
    assert checked > 0
    got = eng.generate(emb, max_length=S0 + n_new, eos_token_id=-1, pad_token_id=0).cpu()
    same = sum(int(torch.equal(got[b], g["tokens"][b])) for b in range(B))
    print(f"[v2 window] {same}/{B} streams identical to HF's windowed generate")
    # asserted, not only printed: the float32 oracle's stream IS HF's (pinned), and every engine stream equals it or leaves it
    # AT a position where the float32 margin is inside the band (a bf16 near-tie; the oracle's own bf16 mode flips there too)
    lead = _assert_stream_vs_hf(got, g["tokens"], w, cfg, g)
    assert same == sum(1 for t in lead if t == n_new), f"identical streams {same} vs leading positions {lead} of {n_new}"
    eng.close()
    full = build_engine(dataclasses.replace(cfg, sliding_window=0), w, max_batch=4, max_seq_len=128)
    with pytest.raises(AssertionError):
        _teacher_forced_check(full, emb, w, cfg, 80)            # full attention drifts from the windowed oracle
    full.close()
    # a prompt LONGER than the window (W = 8 < S0): the prompt pass itself is windowed (key tiles below a block's window are
    # skipped, rows that have seen no key yet keep empty statistics), then the windowed decode continues from that cache
    cfg8 = dataclasses.replace(cfg, sliding_window=8)
    small = build_engine(cfg8, w, max_batch=4, max_seq_len=128)
    assert S0 > 8
    worst8, scale8, checked8, near8, _, _ = _teacher_forced_check(small, emb, w, cfg8, 24)
    print(f"[v2 window] W=8 < S0={S0}: logits max|err| {worst8:.3e} (scale {scale8:.3e}); {checked8} exact, {near8} near-tie flips")
    assert checked8 > 0
    got8 = small.generate(emb, max_length=S0 + g["tokens_w8"].shape[1], eos_token_id=-1, pad_token_id=0).cpu()
    print(f"[v2 window] W=8: {sum(int(torch.equal(got8[b], g['tokens_w8'][b])) for b in range(B))}/{B} streams identical to HF's "
          "generate with the window inside the prompt pass")
    _assert_stream_vs_hf(got8, g["tokens_w8"], w, cfg8, g)      # asserts: departures from HF's stream only at in-band near-ties
    small.close()


def test_streaming_callback_and_hf_streamer():
    """Tokens are handed to the host in bursts of `sync_every` steps while the hipGraph loop keeps running: the streamed
    columns, concatenated, are exactly the returned tokens -- also when EOS / the row-0 stop ends generation early.  The
    mirror feeds a HF-style streamer (put / end), which the reference's worker builds but never gets called."""
    g = _golden("tiny_stop")
    seed, B, n_new, eos = [int(x) for x in g["meta"]]
    cfg = dataclasses.replace(O.OracleConfig.tiny(), eos_token_id=eos)
    w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)
    eng = build_engine(cfg, w, max_batch=4, max_seq_len=96)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    S0 = emb.shape[1]
    for kw in (dict(eos_token_id=-1), dict(eos_token_id=eos, stop_ids=g["stop_ids"].tolist())):
        chunks = []
        toks = eng.generate(emb, max_length=S0 + 40, pad_token_id=cfg.pad_token_id, sync_every=4,
                            on_tokens=lambda t, c0: chunks.append((c0, t.clone())), **kw).cpu()
        assert len(chunks) >= 2 and chunks[0][0] == 0
        assert [c0 for c0, _ in chunks] == [sum(t.shape[1] for _, t in chunks[:i]) for i in range(len(chunks))]   # contiguous
        assert torch.equal(torch.cat([t for _, t in chunks], 1), toks)
        assert torch.equal(toks, eng.generate(emb, max_length=S0 + 40, pad_token_id=cfg.pad_token_id, **kw).cpu())
    with pytest.raises(ValueError):
        eng.generate(emb, max_length=S0 + 8, eos_token_id=-1, pad_token_id=0, num_beams=2, on_tokens=lambda t, c0: None)
    eng.close()

    import starvector_amd as sva

    class Streamer:                                         # the protocol of transformers.generation.streamers
        def __init__(self):
            self.values, self.ended = [], False

        def put(self, value):
            self.values.append(value.clone())

        def end(self):
            self.ended = True

    c0 = O.OracleConfig.tiny()
    w0 = O.make_weights(c0, seed=41)
    scfg = sva.StarVectorConfig(image_size=c0.image_size, hidden_size=c0.hidden, num_hidden_layers=c0.n_layer,
                                num_attention_heads=c0.n_head, vocab_size=c0.vocab - 4, n_inner=c0.n_inner,
                                n_positions=c0.n_positions, max_length=c0.n_positions, vit_width=c0.vit_width,
                                vit_layers=c0.vit_layers, vit_heads=c0.vit_heads, max_batch=4)
    model = sva.StarVectorForCausalLM(scfg, state_dict={k: v.to(torch.bfloat16) for k, v in w0.items()})
    from PIL import Image
    batch = {"image": model.process_images([Image.new("RGB", (c0.image_size, c0.image_size), (20, 200, 30))])[0]}
    st = Streamer()
    S0 = model.model.query_length + 4
    res = model.model.generate_im2svg_grpo(batch, max_length=S0 + 20, num_beams=1, use_nucleus_sampling=False, streamer=st)
    assert st.ended and st.values[0].shape == (1, 0)                       # empty prompt ids first, like HF with inputs_embeds
    streamed = torch.stack(st.values[1:], 1)
    assert torch.equal(streamed.to(res["outputs"].device), res["outputs"][:, 4:])


def test_scoring_forward_logits():
    """sv_forward_logits / StarVectorForCausalLM.forward (starvector_arch.py:161-184): bf16 logits of the last n positions
    against the oracle (bf16 cast points; pinned to HF by tests/golden/tiny_forward) and the HF golden itself."""
    import starvector_amd as sva
    g = _golden("tiny_forward")
    seed, B, n_ids = [int(x) for x in g["meta"]]
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=seed)
    eng = build_engine(cfg, w, max_batch=4, max_seq_len=64)
    vis = eng.adapter(eng.encode_image(bf(g["image"])))
    emb = torch.cat([vis, eng.embed_tokens(g["ids"].to(dev()))], 1)
    S = emb.shape[1]
    got = eng.forward_logits(emb, 5)
    assert got.shape == (B, 5, cfg.vocab) and got.dtype == torch.bfloat16
    ora = O.decoder_forward_logits(w, cfg, emb.float().cpu(), 5, mode="bf16")
    scale = float(ora.abs().max())
    assert float((got.float().cpu() - ora).abs().max()) <= LOGIT_TOL * scale
    assert rel_err(got, g["logits_keep5"]) <= 5e-2                                  # and the fp32 HF golden
    full = eng.forward_logits(emb, 0)
    assert full.shape == (B, S, cfg.vocab)
    assert torch.equal(full[:, -5:].cpu().view(torch.int16), got.cpu().view(torch.int16))
    # the last position agrees with the prefill logits (different GEMM kernel, same arithmetic up to summation order)
    assert float((full[:, -1].float() - eng.prefill(emb).float()).abs().max()) <= LOGIT_TOL * scale
    # argmax of position t predicts the completion token t+1 the same way for both paths where margins allow
    eng.close()
    # the mirror's forward(): visual prefix repeated num_generations times + completion ids
    scfg = sva.StarVectorConfig(image_size=cfg.image_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.n_layer,
                                num_attention_heads=cfg.n_head, vocab_size=cfg.vocab - 4, n_inner=cfg.n_inner,
                                n_positions=cfg.n_positions, max_length=cfg.n_positions, vit_width=cfg.vit_width,
                                vit_layers=cfg.vit_layers, vit_heads=cfg.vit_heads, max_batch=4)
    model = sva.StarVectorForCausalLM(scfg, state_dict={k: v.to(torch.bfloat16) for k, v in w.items()})
    v1 = model.model.image_projection(model.model.image_encoder(bf(g["image"][:1])))
    ids = g["ids"].to(dev())
    out = model(v1, ids, 2, torch.ones(2, v1.shape[1] + ids.shape[1], device=dev()), 4)
    assert out.logits.shape == (2, 4, cfg.vocab) and out.loss is None
    ref = model.engine.forward_logits(torch.cat([v1.repeat(2, 1, 1), model.model._get_embeddings(ids)], 1), 4)
    assert torch.equal(out.logits.view(torch.int16), ref.view(torch.int16))
    # left-padded row (mask 0 0 1 ... 1): HF masks the padded keys and numbers positions by cumsum(mask) - 1, i.e. the row is
    # scored as the row without its pads; the unpadded row of the same call keeps its own logits; right pads change nothing
    S = v1.shape[1] + ids.shape[1]
    mask = torch.ones(2, S, device=dev())
    mask[0, :2] = 0
    mask[1, -1] = 0
    out = model(v1, ids, 2, mask, 4)
    emb2 = torch.cat([v1.repeat(2, 1, 1), model.model._get_embeddings(ids)], 1)
    alone = model.engine.forward_logits(emb2[:1, 2:].contiguous(), 4)
    assert torch.equal(out.logits[0].view(torch.int16), alone[0].view(torch.int16)), "left-padded row != the row without its pads"
    assert torch.equal(out.logits[1].view(torch.int16), ref[1].view(torch.int16)), "unpadded row changed by its neighbour's padding"
    ora = O.decoder_forward_logits(w, cfg, emb2[:1, 2:].float().cpu(), 4, mode="bf16")
    assert float((out.logits[0].float().cpu() - ora[0]).abs().max()) <= LOGIT_TOL * float(ora.abs().max())
    # HF itself on the masked batch with the pinned version's position rule (fp32 golden, oracle/make_golden.py::run_forward_case)
    assert rel_err(out.logits[0], g["logits_leftpad2_row0_keep5"][-4:]) <= 5e-2
    full = model(v1, ids, 2, mask, None).logits
    assert full.shape == (2, S, cfg.vocab) and float(full[0, :2].abs().max()) == 0.0
    assert torch.equal(full[0, -4:].view(torch.int16), alone[0].view(torch.int16))


def test_starvector_8b_dims_one_layer_against_oracle():
    """BASELINE config 4 / 5 DIMENSIONS against the CPU oracle (the full 32-layer model is 29 GB of float32 on the host; one
    layer is not): siglip_384 geometry (576 tokens, 1 tower layer) + ONE StarCoder2-7B layer at D = 4608, 36 query / 4 KV heads,
    F = 18432, sliding window 4096, + the tied lm_head over V = 49157 (llm/starcoder2.py:22-27).  Every kernel shape of the 8B
    decode and prefill path is the real one: K = 4608 / 18432 GEMMs, GQA with 9 query heads per KV head, RoPE, the [576 x 4608]
    adapter LayerNorm.  Teacher-forced logits at every step, token ids exact outside the band, prompt crossing 9 KV pages."""
    torch.set_num_threads(host_cores())
    cfg = dataclasses.replace(O.OracleConfig.starvector_8b(), n_layer=1, vit_layers=1, eos_token_id=-1)
    w = O.make_weights(cfg, seed=77)
    B, n_new = 2, 8
    eng = build_engine(cfg, w, max_batch=2, max_seq_len=578 + 72)
    img = O.synthetic_images(B, 384, seed=78)
    prompt = torch.tensor([[7, 11]] * B)
    enc = eng.encode_image(bf(img))
    vis = eng.adapter(enc)
    emb = torch.cat([vis, eng.embed_tokens(prompt.to(dev()))], 1)
    assert emb.shape == (B, 578, 4608)
    o_enc = O.image_encoder_forward(w, cfg, img, "bf16")
    o_vis = O.adapter_forward(w, cfg, o_enc, "bf16")
    e1, e2 = rel_err(enc, o_enc), rel_err(vis, o_vis)
    print(f"[8b dims] siglip rel err {e1:.3e}, adapter rel err {e2:.3e}")
    assert e1 <= 3e-2 and e2 <= 3e-2
    worst, scale, checked, near, o_toks, margin = _teacher_forced_check(eng, emb, w, cfg, n_new)
    print(f"[8b dims] {n_new} steps x {B} rows: logits max|err| {worst:.3e} (scale {scale:.3e}); {checked}/{B * n_new} positions "
          f"token-exact outside the band, {near} near-tie flips inside it")
    assert checked >= 0.85 * B * n_new, f"only {checked}/{B * n_new} positions are margin-safe and token-exact"
    # a longer free run crosses the 640-token KV page boundary with RoPE positions: deterministic, graph == eager
    kw = dict(max_length=578 + 70, eos_token_id=-1, pad_token_id=0)
    a = eng.generate(emb, **kw).cpu()
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        assert torch.equal(a, eng.generate(emb, **kw).cpu())
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    assert torch.equal(a[1], eng.generate(emb[1:2].contiguous(), **kw).cpu()[0])
    eng.close()


def test_starvector_8b_dims_64_row_engine_short_contexts():
    """A 64-row engine at StarVector-8B's dimensions (BASELINE config 5: text2svg, short prompts): rows x KV heads = 256 fill the chip,
    so a context of up to 8 key groups stays in one attention block (no partial results / merge) and longer ones split; the decode
    GEMMs run the two-row-tile kernel with the engine's (split-K, column tiles) plan.  Text-only prompt of 250 tokens + 12 new tokens:
    the context crosses 256 -> the attention switches from one block to two splits on the way.  Teacher-forced against the oracle."""
    torch.set_num_threads(host_cores())
    cfg = dataclasses.replace(O.OracleConfig.starvector_8b(), n_layer=1, vit_layers=1, eos_token_id=-1)
    w = O.make_weights(cfg, seed=79)
    B, n_new, S0 = 3, 12, 250
    eng = build_engine(cfg, w, max_batch=64, max_seq_len=320)
    ids = torch.randint(0, 4000, (B, S0), generator=torch.Generator().manual_seed(80))
    emb = eng.embed_tokens(ids.to(dev()))
    assert emb.shape == (B, S0, 4608)
    worst, scale, checked, near, o_toks, margin = _teacher_forced_check(eng, emb, w, cfg, n_new)
    print(f"[8b dims, 64-row engine] {n_new} steps x {B} rows: logits max|err| {worst:.3e} (scale {scale:.3e}); "
          f"{checked}/{B * n_new} positions token-exact outside the band, {near} near-tie flips inside it")
    assert checked >= 0.8 * B * n_new, f"only {checked}/{B * n_new} positions are margin-safe and token-exact"
    # a row does not depend on the batch around it (same splits, same plan: constants of the engine), graph == eager
    kw = dict(max_length=S0 + n_new, eos_token_id=-1, pad_token_id=0)
    a = eng.generate(emb, **kw).cpu()
    assert torch.equal(a[2], eng.generate(emb[2:3].contiguous(), **kw).cpu()[0])
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        assert torch.equal(a, eng.generate(emb, **kw).cpu())
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    eng.close()


def test_starvector_8b_full_size_properties():
    """BASELINE config 4 shapes (siglip_384 + starcoder2-7b: 7.2 B parameters, 36 query / 4 KV heads, D 4608):
    the CPU oracle cannot run this size in test time, so the full size is covered by size-independent properties -
    bit-exact determinism, graph == eager, batch invariance of a row, token range, and the top-p sampling path."""
    import starvector_amd as sva
    cfg = O.OracleConfig.starvector_8b()
    eng = sva.HipEngine(sva.EngineConfig.starvector_8b(max_batch=4, max_seq_len=640))
    for name, tns in O.iter_weights(cfg, seed=3, init="std002"):          # streamed: never 29 GB of fp32 at once
        eng.load_weight(name, tns)
    eng.load_state_dict({})
    img = bf(O.synthetic_images(3, 384, seed=4))
    prompt = torch.tensor([[7, 11]] * 3, device=dev())
    enc = eng.encode_image(img)
    emb = torch.cat([eng.adapter(enc), eng.embed_tokens(prompt)], 1)
    assert enc.shape == (3, 576, 1024) and emb.shape == (3, 578, 4608) and not torch.isnan(emb.float()).any()
    kw = dict(max_length=578 + 24, eos_token_id=-1, pad_token_id=0)
    a = eng.generate(emb, **kw).cpu()
    assert a.shape == (3, 24) and int(a.min()) >= 0 and int(a.max()) < cfg.vocab
    assert torch.equal(a, eng.generate(emb, **kw).cpu())
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        assert torch.equal(a, eng.generate(emb, **kw).cpu())
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    assert torch.equal(a[2], eng.generate(emb[2:3].contiguous(), **kw).cpu()[0])
    s = eng.generate(emb, do_sample=True, temperature=1.0, top_p=0.95, seed=9, **kw).cpu()
    assert s.shape == (3, 24) and torch.equal(s, eng.generate(emb, do_sample=True, temperature=1.0, top_p=0.95, seed=9, **kw).cpu())
    print(f"[8b] timing {eng.last_timing()}")
    eng.close()


def test_row_update_and_c_attn_as_one_launch_at_starvector_8b_widths():
    """Round 5, VERDICT r04 item 3 (one of the 1B launches carried to the wide model): StarVector-8B's decode layer is the 7-launch layer
    (row-major residual stream, hidden 4608: a 1024-thread row update, a c_attn of 176 tiles x 4 K slices with NINE k-steps per wave); the
    fused launch there is rowln_cattn_kernel<9, true> -- the wide row role on a block's 512 threads with the 1024-thread kernel's reduction
    tree, 704 GEMM blocks behind 32 row blocks.  8B widths, 4 decoder layers, SV_EXP 16384 on a non-exclusive engine: teacher-forced logits,
    greedy and sampled tokens at 16 / 11 rows and a single row (too few attention threads for the pattern stores: falls back by itself) are
    IDENTICAL to the two launches."""
    import starvector_amd as sva
    ec = sva.EngineConfig.starvector_8b(max_batch=16, max_seq_len=578 + 80)
    ec.n_layer, ec.vit_layers = 4, 1
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=17)
    B = 16
    g = torch.Generator().manual_seed(3)
    img = torch.randn(B, 3, 384, 384, generator=g).to(torch.bfloat16).to(dev())
    prompt = torch.tensor([[7, 11]] * B, dtype=torch.long, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1).contiguous()
    S0 = emb.shape[1]
    kw = dict(max_length=S0 + 60, eos_token_id=-1, pad_token_id=0)
    runs = {}
    for mask in (0, 16384):
        eng.set_exp(mask)
        lg = [eng.prefill(emb)]
        tok = lg[0].argmax(-1)
        for _ in range(6):
            lg.append(eng.decode_step(tok))
            tok = lg[-1].argmax(-1)
        toks = eng.generate(emb, **kw).cpu()
        assert eng.last_timing()["graph"]
        small = eng.generate(emb[:11].contiguous(), **kw).cpu()
        one = eng.generate(emb[5:6].contiguous(), **kw).cpu()
        samp = eng.generate(emb, do_sample=True, temperature=1.0, top_p=0.95, top_k=50, seed=3, **kw).cpu()
        again = eng.generate(emb, **kw).cpu()
        runs[mask] = (torch.stack(lg).cpu(), toks, small, one, samp, again)
    eng.set_exp(0)
    ref = runs[0]
    assert torch.isfinite(ref[0].float()).all() and ref[4].unique().numel() > 16
    for k, what in enumerate(["teacher-forced logits", "tokens (16 rows)", "tokens (11 rows)", "tokens (1 row)", "sampled tokens", "second call"]):
        assert torch.equal(runs[16384][k], ref[k]), f"8B widths, SV_EXP 16384: {what} differ from the two launches"
    eng.close()
    own = sva.HipEngine(dataclasses.replace(ec, exclusive_device=True))           # the deployment: on by itself, same tokens
    own.load_random_weights(seed=17)
    emb2 = torch.cat([own.adapter(own.encode_image(img)), own.embed_tokens(prompt)], 1).contiguous()
    assert torch.equal(own.generate(emb2, **kw).cpu(), ref[1])
    assert torch.equal(own.generate(emb2, do_sample=True, temperature=1.0, top_p=0.95, top_k=50, seed=3, **kw).cpu(), ref[4])
    own.close()


def test_repetition_penalty_on_device():
    """starvector_base.py:237 -> HF RepetitionPenaltyLogitsProcessor, restated on device (bitmap of generated ids).
    Property: an overwhelming penalty never lets a token with a positive logit repeat; parity: the engine's stream equals
    the oracle's (pinned to HF by tests/golden/tiny_reppen) up to the first near-tie."""
    g = _golden("tiny_reppen")
    seed, B, n_new = [int(x) for x in g["meta"]]
    pen = float(g["penalty"])
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=seed)
    eng = build_engine(cfg, w, 4, 96)
    emb = torch.cat([eng.adapter(eng.encode_image(bf(g["image"]))), eng.embed_tokens(g["prompt_ids"].to(dev()))], 1)
    S0 = emb.shape[1]
    kw = dict(max_length=S0 + n_new, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    got = eng.generate(emb, repetition_penalty=pen, **kw).cpu()
    free = eng.generate(emb, **kw).cpu()
    assert got.shape == (B, n_new) and not torch.equal(got, free)
    o_toks, o_sc = O.greedy_generate(w, cfg, emb.float().cpu(), S0 + n_new, mode="bf16", return_logits=True,
                                     repetition_penalty=pen)
    top2 = o_sc.topk(2, -1).values
    margin = top2[..., 0] - top2[..., 1]
    tol = 2 * LOGIT_TOL * float(o_sc.abs().max())
    for b in range(B):
        for t in range(n_new):
            if got[b, t] != o_toks[b, t]:
                assert margin[b, t] <= tol, f"row {b} step {t}: mismatch at margin {margin[b, t]:.3e}"
                break
    huge = eng.generate(emb, repetition_penalty=1e6, max_length=S0 + 40, eos_token_id=-1, pad_token_id=cfg.pad_token_id).cpu()
    for b in range(B):
        assert len(set(huge[b].tolist())) == 40            # all distinct: positive logits exist for unseen ids
    # sampling path with the penalty runs and is reproducible
    s1 = eng.generate(emb, do_sample=True, temperature=0.8, top_p=0.9, seed=3, repetition_penalty=pen, **kw).cpu()
    assert torch.equal(s1, eng.generate(emb, do_sample=True, temperature=0.8, top_p=0.9, seed=3, repetition_penalty=pen, **kw).cpu())
    eng.close()


def test_non_finite_logits_are_an_error_not_a_memory_fault():
    """A row of logits with no finite value (NaN weights here) has no argmax: the selection kernels must not hand their
    out-of-range sentinel to the next step's embedding gather (that was a GPU memory fault), and the call must fail loudly
    instead of returning made-up tokens.  The engine stays usable afterwards."""
    cfg = O.OracleConfig.tiny()
    w = O.make_weights(cfg, seed=5)
    bad = dict(w)
    k = O.P_DEC + "ln_f.weight"
    bad[k] = torch.full_like(w[k], float("nan"))
    eng = build_engine(cfg, bad, 4, 96)
    img = bf(O.synthetic_images(2, cfg.image_size, seed=6))
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(torch.tensor([[7, 11]] * 2, device=dev()))], 1)
    S0 = emb.shape[1]
    for kw in (dict(), dict(do_sample=True, temperature=1.0, top_p=0.9, seed=3)):
        with pytest.raises(RuntimeError, match="no finite value"):
            eng.generate(emb, max_length=S0 + 12, eos_token_id=-1, pad_token_id=0, **kw)
    with pytest.raises(RuntimeError, match="no finite value"):
        eng.cb_admit(emb[:1].contiguous(), [dict(max_new_tokens=8)])
        eng.cb_step(4)
    eng.cb_reset()
    eng.close()
    good = build_engine(cfg, w, 4, 96)                       # same process, healthy weights: unaffected
    emb = torch.cat([good.adapter(good.encode_image(img)), good.embed_tokens(torch.tensor([[7, 11]] * 2, device=dev()))], 1)
    assert good.generate(emb, max_length=S0 + 12, eos_token_id=-1, pad_token_id=0).shape == (2, 12)
    good.close()


def test_from_pretrained_reference_format_directory_matches_hf_generate(tmp_path):
    """scripts/quickstart.py:9-19 end to end on a checkpoint DIRECTORY in the reference's format (config.json + sharded safetensors under
    train/util.py:71's key names, written by tests/ckpt_util.py): `StarVectorForCausalLM.from_pretrained` -> `.cuda().eval()` ->
    `generate_im2svg`.  The weights are tests/golden/tiny_b3's (designed greedy stream), so the NEW token ids must equal HF generate's,
    token for token, through the public API; then the quickstart's own kwargs (beam-sample, repetition penalty) run on the same model."""
    import starvector_amd as sva
    from starvector_amd.model import ByteTokenizer
    from tests.ckpt_util import write_reference_checkpoint
    g = _golden("tiny_b3")
    seed, B, n_new = [int(x) for x in g["meta"]]
    cfg = O.OracleConfig.tiny()
    w = O.apply_fixture_weights(O.make_weights(cfg, seed=seed), cfg, g)
    d = str(tmp_path / "starvector-tiny-im2svg")
    write_reference_checkpoint(d, cfg, w, n_shards=2, torch_dtype="bfloat16")
    prompt_ids = g["prompt_ids"][0].tolist()

    class Tok(ByteTokenizer):                       # the golden's prompt ids stand for '<svg' (the StarCoder tokenizer is gated / offline)
        def encode(self, text, add_special_tokens=False):
            return list(prompt_ids) if text == "<svg" else super().encode(text, add_special_tokens)

    with pytest.raises(FileNotFoundError, match="tokenizer"):
        sva.StarVectorForCausalLM.from_pretrained(d)                       # no tokenizer files, no silent stand-in
    model = sva.StarVectorForCausalLM.from_pretrained(d, torch_dtype="auto", tokenizer=Tok(cfg.vocab - 4))
    model.cuda()
    model.eval()
    batch = {"image": g["image"].to(torch.float16).to(dev())}              # the quickstart hands the image over as float16
    S0 = model.model.query_length + len(prompt_ids)
    res = model.model.generate_im2svg_grpo(batch, max_length=S0 + n_new, num_beams=1, use_nucleus_sampling=False)
    assert res["outputs"].shape == (B, len(prompt_ids) + n_new)
    assert torch.equal(res["outputs"][:, :len(prompt_ids)].cpu(), g["prompt_ids"])
    assert torch.equal(res["outputs"][:, len(prompt_ids):].cpu(), g["tokens"]), "from_pretrained + generate != HF generate on the golden"
    svgs = model.generate_im2svg(batch, max_length=S0 + n_new, num_beams=1, use_nucleus_sampling=False)
    assert isinstance(svgs, list) and len(svgs) == B and all(isinstance(s, str) for s in svgs)
    # the quickstart's literal call: one un-batched image, the reference's defaults (num_beams 2 + nucleus sampling) and its kwargs
    one = {"image": g["image"][0].to(torch.float16).to(dev())}
    raw_svg = model.generate_im2svg(one, max_length=S0 + 12, temperature=1.5, length_penalty=-1, repetition_penalty=3.1)[0]
    assert isinstance(raw_svg, str)
    # a float16 checkpoint (configs/generation/hf/starvector-1b/im2svg.yaml:16) loads too: converted at the boundary, with a warning
    d16 = str(tmp_path / "starvector-tiny-fp16")
    write_reference_checkpoint(d16, cfg, w, n_shards=1, torch_dtype="float16")
    m16 = sva.StarVectorForCausalLM.from_pretrained(d16, tokenizer=Tok(cfg.vocab - 4))
    r16 = m16.model.generate_im2svg_grpo(batch, max_length=S0 + n_new, num_beams=1, use_nucleus_sampling=False)
    # fp16 storage only flushes the few weights below its subnormal range (|w| < 6e-8); the designed margins are 0.25 x the logit scale
    assert torch.equal(r16["outputs"].cpu(), res["outputs"].cpu())
    model.engine.close()
    m16.engine.close()


def test_fused_mlp_launch_equals_the_two_launches_bit_for_bit():
    """Round-4 experiment (SV_EXP bit 128, mlp_fused.hip mlp_fused_kernel): c_fc + GELU + down projection of a decode layer as ONE launch of
    256 co-resident blocks with an in-launch hand-off (write-through stores, one ticket per K slice, bounded polling).  Per-wave k
    ranges, MFMA order, reduction order and epilogues are those of the two kernels it replaces, so logits and tokens must be IDENTICAL
    bit for bit -- at BASELINE config 2's size (the geometry it is built for), eager and under the hipGraph loop."""
    import starvector_amd as sva
    B = 32
    eng = sva.HipEngine(sva.EngineConfig(max_batch=B, max_seq_len=259 + 160))
    eng.load_random_weights(seed=7)
    g = torch.Generator().manual_seed(3)
    img = torch.randn(B, 3, 224, 224, generator=g).to(torch.bfloat16).to(dev())
    prompt = torch.tensor([[7, 11]] * B, dtype=torch.long, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    runs = {}
    for mask in (0, 128):
        eng.set_exp(mask)
        lg = [eng.prefill(emb)]
        tok = lg[0].argmax(-1)
        for _ in range(6):
            lg.append(eng.decode_step(tok))
            tok = lg[-1].argmax(-1)
        toks = eng.generate(emb, max_length=emb.shape[1] + 150, eos_token_id=-1, pad_token_id=49152)
        assert eng.last_timing()["graph"]
        runs[mask] = (torch.stack(lg).cpu(), toks.cpu())
    eng.set_exp(0)
    assert torch.equal(runs[0][0], runs[128][0]), "fused MLP launch changes the logits"
    assert torch.equal(runs[0][1], runs[128][1]), "fused MLP launch changes the token stream"
    assert runs[0][1].unique().numel() > 8                                  # not a degenerate stream
    eng.close()
    # an engine that owns its GPU (sv_config.exclusive_device) runs the fused launch by default: same tokens again
    own = sva.HipEngine(sva.EngineConfig(max_batch=B, max_seq_len=259 + 160, exclusive_device=True))
    own.load_random_weights(seed=7)
    emb2 = torch.cat([own.adapter(own.encode_image(img)), own.embed_tokens(prompt)], 1)
    toks = own.generate(emb2, max_length=emb2.shape[1] + 150, eos_token_id=-1, pad_token_id=49152).cpu()
    assert torch.equal(toks, runs[0][1])
    own.close()


@pytest.mark.parametrize("norm", ["layer_norm", "batch_norm"])
def test_prepare_inputs_writes_the_prefill_buffer_directly(norm):
    """a1 (starvector_base.py:203-221): `prepare_inputs` = torch.cat([adapter(enc), wte(prompt ids)], 1) bit for bit, without the ATen
    concatenation kernel (both adapter norms; the drop-in `_prepare_generation_inputs` goes through it)."""
    cfg = dataclasses.replace(O.OracleConfig.tiny(), adapter_norm=norm)
    w = O.make_weights(cfg, seed=77)
    eng = build_engine(cfg, w, max_batch=4, max_seq_len=64)
    img = O.synthetic_images(3, cfg.image_size, seed=5)
    ids = torch.tensor([[7, 11, 13], [2, 3, 4], [500, 1, 9]], dtype=torch.long, device=dev())
    enc = eng.encode_image(bf(img))
    want = torch.cat([eng.adapter(enc), eng.embed_tokens(ids)], 1)
    got = eng.prepare_inputs(enc, ids)
    assert got.shape == want.shape and torch.equal(got, want)
    with pytest.raises(ValueError):
        eng.prepare_inputs(enc, ids[:2])
    eng.close()


def test_ttft_stage_profile_accounts_for_the_pass():
    """sv_profile_ttft (the bench line's `ttft_breakdown_ms`): every stage of image -> first token is priced, the
    stages add up to the first-to-last-event span (minus the event-pair time of each interval), and the call leaves the engine
    usable with the KV cache of that prompt (a decode step continues from it exactly as after sv_prefill)."""
    cfg = dataclasses.replace(O.OracleConfig.tiny(), eos_token_id=-1)
    w = O.make_weights(cfg, seed=31)
    eng = build_engine(cfg, w, max_batch=4, max_seq_len=64)
    img = bf(O.synthetic_images(3, cfg.image_size, seed=32))
    ids = torch.tensor([[7, 11, 13]] * 3, dtype=torch.long, device=dev())
    tp = eng.profile_ttft(img, ids, iters=2)
    stages = {k: tp[k] for k in eng.TTFT_STAGES}
    print(f"[ttft profile, tiny] {', '.join(f'{k} {v * 1e3:.0f} us' for k, v in stages.items())}; first to last event {tp['first_to_last_event_ms'] * 1e3:.0f} us")
    assert all(v >= 0 for v in stages.values()) and stages["encoder_gemm"] > 0 and stages["prefill_gemm"] > 0 and stages["lm_head"] > 0
    n_int = sum(tp["launches"].values())
    assert n_int > 20
    total = sum(stages.values())
    span = tp["first_to_last_event_ms"]
    assert total <= span + 1e-3 and total >= span - n_int * (tp["event_pair_overhead_ms"] + 2e-3), (total, span, n_int)
    # the cache it leaves = sv_prefill's: the next decode step gives the same logits as after a plain prompt pass
    emb = eng.prepare_inputs(eng.encode_image(img), ids)
    tok = torch.tensor([5, 6, 7], device=dev())
    eng.profile_ttft(img, ids, iters=1)
    a = eng.decode_step(tok)
    eng.prefill(emb)
    assert torch.equal(a, eng.decode_step(tok))
    # text2svg: no encoder / adapter stages
    t2 = eng.profile_ttft(None, ids, iters=1)
    assert t2["encoder_gemm"] == 0 and t2["adapter_gemm"] == 0 and t2["prefill_gemm"] > 0
    eng.close()


def test_folded_greedy_selection_equals_the_argmax_launch_token_for_token():
    """Round 5: a plain greedy sv_generate selects inside the lm_head launch (one launch less per decode step).  SV_EXP bit 1024 puts
    the separate argmax launch back: the token streams must be IDENTICAL -- BASELINE config 2's size, graph and eager, a batch that is
    not a multiple of anything (rows >= B of the row tile take no part), EOS / pad bookkeeping after a row finishes, and the modes
    that must NOT take the folded path (repetition penalty, min_length hold, sampling) unchanged."""
    import starvector_amd as sva
    B = 32
    eng = sva.HipEngine(sva.EngineConfig(max_batch=B, max_seq_len=259 + 200))
    eng.load_random_weights(seed=11)
    g = torch.Generator().manual_seed(5)
    img = torch.randn(B, 3, 224, 224, generator=g).to(torch.bfloat16).to(dev())
    prompt = torch.tensor([[7, 11]] * B, dtype=torch.long, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    S0 = emb.shape[1]
    kw = dict(max_length=S0 + 180, eos_token_id=-1, pad_token_id=49152)
    eng.set_exp(1024)
    ref = eng.generate(emb, **kw).cpu()
    # an EOS id that row 3 meets for the first time at some step >= 20 (random-init rows repeat tokens: search for one)
    t_eos = next(t for t in range(20, 170) if int(ref[3, t]) not in ref[3, :t].tolist())
    eos = int(ref[3, t_eos])
    ref_eos = eng.generate(emb, max_length=S0 + 180, eos_token_id=eos, pad_token_id=49152).cpu()
    ref13 = eng.generate(emb[:13].contiguous(), **kw).cpu()
    ref_pen = eng.generate(emb, repetition_penalty=1.3, **kw).cpu()
    eng.set_exp(0)
    got = eng.generate(emb, **kw).cpu()
    assert eng.last_timing()["graph"]
    assert torch.equal(got, ref), "folded greedy selection changes the token stream"
    assert ref.unique().numel() > 8
    assert torch.equal(eng.generate(emb, max_length=S0 + 180, eos_token_id=eos, pad_token_id=49152).cpu(), ref_eos)
    if ref_eos.shape[1] > t_eos:                                # (the batch may have ended earlier: every row met the id before t_eos)
        assert int(ref_eos[3, t_eos]) == eos and bool((ref_eos[3, t_eos + 1:] == 49152).all())
    assert torch.equal(eng.generate(emb[:13].contiguous(), **kw).cpu(), ref13)
    assert torch.equal(ref13, ref[:13])                         # a row does not depend on the batch around it
    assert torch.equal(eng.generate(emb, repetition_penalty=1.3, **kw).cpu(), ref_pen)
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        assert torch.equal(eng.generate(emb, **kw).cpu(), ref)
        assert not eng.last_timing()["graph"]
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    # back-to-back calls re-arm the key slots: a second identical call, then a sampled one, then greedy again
    assert torch.equal(eng.generate(emb, **kw).cpu(), ref)
    eng.generate(emb, do_sample=True, temperature=1.0, top_p=0.9, top_k=50, seed=3, **kw)
    assert torch.equal(eng.generate(emb, **kw).cpu(), ref)
    eng.close()


def test_step_bookkeeping_inside_the_lm_head_launch_equals_the_finish_launch(monkeypatch):
    """Round 6, fifth session: a greedy step whose selection rides in the persistent lm_head launch also does its bookkeeping there (the
    last block of the grid, elected by a ticket, decodes the keys and runs what finish_step_kernel runs: tokens out, EOS / pad, the stop
    sequence on row 0, the step counter, the end of the call) -- one launch less per step.  SV_FINISH_FOLD=0 puts the launch back: the
    streams must be IDENTICAL, with rows ending at different steps, with a stop sequence that fires inside a multi-step graph, at batches
    1 / 5 / 32, over repeated calls (the ticket and the key slots re-arm).  The reference semantics: HF generate's _sample bookkeeping
    (transformers generation/utils.py) under /root/reference/starvector/model/models/starvector_base.py:223-241."""
    import starvector_amd as sva
    B = 32
    eng = sva.HipEngine(sva.EngineConfig(max_batch=B, max_seq_len=259 + 200))
    eng.load_random_weights(seed=13)
    g = torch.Generator().manual_seed(9)
    img = torch.randn(B, 3, 224, 224, generator=g).to(torch.bfloat16).to(dev())
    prompt = torch.tensor([[7, 11]] * B, dtype=torch.long, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    S0 = emb.shape[1]
    kw = dict(max_length=S0 + 170, pad_token_id=49152)
    monkeypatch.setenv("SV_FINISH_FOLD", "0")
    ref = eng.generate(emb, eos_token_id=-1, **kw).cpu()
    n_unfolded = eng.step_plan()["graph_kernel_nodes"]
    t_eos = next(t for t in range(20, 160) if int(ref[3, t]) not in ref[3, :t].tolist())
    eos = int(ref[3, t_eos])
    r0 = ref[0].tolist()                                        # a pair row 0 emits for the first time at some step >= 60 (random-init rows repeat tokens)
    t_stop = next(t for t in range(60, 160) if all((r0[u], r0[u + 1]) != (r0[t], r0[t + 1]) for u in range(t)))
    stop = [r0[t_stop], r0[t_stop + 1]]
    ref_eos = eng.generate(emb, eos_token_id=eos, **kw).cpu()
    ref_stop = eng.generate(emb, eos_token_id=-1, stop_ids=stop, **kw).cpu()
    ref5 = eng.generate(emb[:5].contiguous(), eos_token_id=eos, **kw).cpu()
    ref1 = eng.generate(emb[:1].contiguous(), eos_token_id=-1, **kw).cpu()
    monkeypatch.setenv("SV_FINISH_FOLD", "1")
    for rep in range(2):
        got = eng.generate(emb, eos_token_id=-1, **kw).cpu()
        assert eng.last_timing()["graph"] and eng.step_plan()["greedy_in_lm_head"]
        assert eng.step_plan()["graph_kernel_nodes"] == n_unfolded - 1, "the bookkeeping launch is still in the captured step"
        assert torch.equal(got, ref)
        assert torch.equal(eng.generate(emb, eos_token_id=eos, **kw).cpu(), ref_eos)
        assert torch.equal(eng.generate(emb, eos_token_id=-1, stop_ids=stop, **kw).cpu(), ref_stop)
        assert torch.equal(eng.generate(emb[:5].contiguous(), eos_token_id=eos, **kw).cpu(), ref5)
        assert torch.equal(eng.generate(emb[:1].contiguous(), eos_token_id=-1, **kw).cpu(), ref1)
    assert ref_stop.shape[1] == t_stop + 2, "the stop sequence did not end the call where row 0 completes it"
    monkeypatch.setenv("SV_NO_GRAPH", "1")
    assert torch.equal(eng.generate(emb, eos_token_id=eos, **kw).cpu(), ref_eos)
    assert not eng.last_timing()["graph"]
    print(f"[finish fold] {n_unfolded} -> {n_unfolded - 1} kernel nodes per captured step; streams identical (EOS at step {t_eos} of row 3, stop sequence "
          f"ends the call after {ref_stop.shape[1]} of {ref.shape[1]} tokens)")
    eng.close()


def test_fused_row_update_launch_blocks_resident_per_cu():
    """the fused row update + c_attn launch waits on blocks of its own grid -- the narrow form (StarVector-1B) needs two blocks per CU
    resident, the wide form's (StarVector-8B) first round is three per CU.  That is the compiler's register allocation, not host arithmetic:
    sv_create asks the runtime (hipOccupancyMaxActiveBlocksPerMultiprocessor) and turns the launch off below that; here the numbers are pinned."""
    import ctypes as C
    from starvector_amd import _lib
    lib = _lib.load()
    got = {}
    for wide in (0, 1):
        n = C.c_int32(0)
        assert lib.sv_debug_rowln_occupancy(wide, C.byref(n)) == 0
        got[wide] = n.value
    print(f"[rowln_cattn occupancy] blocks per CU: narrow {got[0]}, wide {got[1]}")
    assert got[0] >= 2 and got[1] >= 3


def test_row_update_and_c_attn_as_one_launch_bit_for_bit():
    """Round 5 (rowops.hip rowln_cattn_kernel, SV_EXP bit 16384 on a non-exclusive engine): the row update and the c_attn projection
    behind it as ONE launch -- 32 row blocks publish the LayerNorm output with write-through stores, the 288 GEMM blocks hold their
    whole weight share in registers from t = 0 and poll the activations in band (the buffer carries the 0xFFFF'FFFF pattern from a
    memset node / the attention launch of the layer before).  Same per-wave k ranges, MFMA and reduction order as the two kernels:
    logits and tokens must be IDENTICAL -- alone, together with the fused MLP launch, at 32 / 13 / 1 rows, under the graph and eager,
    with EOS bookkeeping, with sampling, through sv_decode_step, and back to back (the pattern is re-armed every step)."""
    import starvector_amd as sva
    B = 32
    eng = sva.HipEngine(sva.EngineConfig(max_batch=B, max_seq_len=259 + 200))
    eng.load_random_weights(seed=13)
    g = torch.Generator().manual_seed(9)
    img = torch.randn(B, 3, 224, 224, generator=g).to(torch.bfloat16).to(dev())
    prompt = torch.tensor([[7, 11]] * B, dtype=torch.long, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    S0 = emb.shape[1]
    kw = dict(max_length=S0 + 170, eos_token_id=-1, pad_token_id=49152)
    runs = {}
    for mask in (0, 16384, 128, 128 + 16384):
        eng.set_exp(mask)
        lg = [eng.prefill(emb)]
        tok = lg[0].argmax(-1)
        for _ in range(5):
            lg.append(eng.decode_step(tok))
            tok = lg[-1].argmax(-1)
        toks = eng.generate(emb, **kw)
        assert eng.last_timing()["graph"]
        small = eng.generate(emb[:13].contiguous(), **kw)
        one = eng.generate(emb[5:6].contiguous(), **kw)
        if mask & 16384:       # (round 6: below 10 rows the attention grid has no room for the pattern; the output projection's launch arms the buffer instead)
            assert eng.step_plan()["rowln_cattn_fused"], "a 1-row call fell back to the two launches"
        samp = eng.generate(emb, do_sample=True, temperature=1.0, top_p=0.9, top_k=50, seed=3, **kw)
        again = eng.generate(emb, **kw)
        runs[mask] = (torch.stack(lg).cpu(), toks.cpu(), small.cpu(), one.cpu(), samp.cpu(), again.cpu())
    eng.set_exp(16384)
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        eager = eng.generate(emb, **kw).cpu()
        assert not eng.last_timing()["graph"]
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    eng.set_exp(0)
    ref = runs[0]
    assert ref[1].unique().numel() > 8
    assert torch.equal(ref[1], ref[5]) and torch.equal(ref[2], ref[1][:13]) and torch.equal(ref[3][0], ref[1][5])
    for mask in (16384, 128, 128 + 16384):
        for k, what in enumerate(["teacher-forced logits", "tokens (32 rows)", "tokens (13 rows)", "tokens (1 row)", "sampled tokens", "second call"]):
            assert torch.equal(runs[mask][k], ref[k]), f"SV_EXP {mask}: {what} differ from the unfused launches"
    assert torch.equal(eager, ref[1])
    eng.close()
    # an engine that owns its GPU runs both fused launches by default: same tokens again -- and again through the KEPT hipGraph with a
    # prompt pass in between (round 5: the first form fed the prompt pass's ln_f through the polled buffer with plain stores and armed it
    # with a memset node; bench.py's third call then read a stale line of it out of an L2 -> NaN logits.  The buffer is now touched with
    # write-through stores / L1-bypassing loads only, and this is the sequence that found it: several identical long calls)
    own = sva.HipEngine(sva.EngineConfig(max_batch=B, max_seq_len=259 + 700, exclusive_device=True))
    own.load_random_weights(seed=13)
    emb2 = torch.cat([own.adapter(own.encode_image(img)), own.embed_tokens(prompt)], 1)
    assert torch.equal(own.generate(emb2, **kw).cpu(), ref[1])
    kw_long = dict(max_length=S0 + 690, eos_token_id=-1, pad_token_id=49152)
    first = own.generate(emb2, **kw_long).cpu()
    assert torch.equal(first[:, :170], ref[1])
    for _ in range(3):
        emb3 = own.prepare_inputs(own.encode_image(img), prompt)
        assert torch.equal(own.generate(emb3, **kw_long).cpu(), first) and own.last_timing()["graph"]
    own.close()
