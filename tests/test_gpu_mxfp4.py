"""GPU: MXFP4 decoder weights through the engine (`weight_dtype="mxfp4"`).

The contract (DESIGN.md "MXFP4 decoder weights"): every dequantised weight is exactly a bf16 number, so an mxfp4 engine over W computes what a
bf16 engine computes over dequant(quant(W)) = tests/fp4_ref.fake_quantize_mxfp4(W), except for the K-summation order of the decode GEMMs.
Engine A is the mxfp4 engine over W; engine B is the bf16 engine over the fake-quantised weights, created with SV_EXP = 2 (the 7-launch
decode layer an mxfp4 engine runs: the 6-launch layer folds LayerNorm's gamma into c_fc and re-rounds the product, other numerics)."""
import dataclasses
import os

import pytest
import torch

from oracle import starvector_oracle as O
from tests import fp4_ref as R
from tests.fp8_ref import BOUND_LOGITS
from tests.gpu_util import bf, build_engine, dev
from tests.test_gpu_e2e import LOGIT_TOL, _teacher_forced_check

pytestmark = pytest.mark.gpu
SEED = 55        # checked on the CPU with the oracle over fake_quantize_mxfp4(W): 5 (v1) / 3 (v2) of 72 positions inside the margin band
STEPS = 24


def _bf16_engine_7_launch(cfg, w, **kw):
    old = os.environ.get("SV_EXP")
    os.environ["SV_EXP"] = "2"                                  # read once at sv_create
    try:
        return build_engine(cfg, w, **kw)
    finally:
        os.environ.pop("SV_EXP", None) if old is None else os.environ.__setitem__("SV_EXP", old)


@pytest.fixture(scope="module", params=["v1", "v2"])
def pair(request):
    cfg = O.OracleConfig.tiny() if request.param == "v1" else O.OracleConfig.tiny_v2()
    cfg = dataclasses.replace(cfg, eos_token_id=-1)
    w = O.make_weights(cfg, seed=SEED)
    wq = R.fake_quantize_mxfp4(w, cfg)
    a = build_engine(cfg, w, max_batch=24, max_seq_len=112, weight_dtype="mxfp4")          # 24 rows: three sequences of K + 1 = 8 lookup rows
    b = _bf16_engine_7_launch(cfg, wq, max_batch=24, max_seq_len=112)
    img = bf(O.synthetic_images(3, cfg.image_size, seed=56))
    prompt = torch.tensor([[7, 11]] * 3, device=dev())
    emb = torch.cat([a.adapter(a.encode_image(img)), a.embed_tokens(prompt)], 1)
    yield dict(arch=request.param, cfg=cfg, w=w, wq=wq, a=a, b=b, emb=emb)
    a.close()
    b.close()


def test_prompt_pass_and_teacher_forced_decode_against_the_bf16_engine_over_the_dequantised_weights(pair):
    a, b, emb = pair["a"], pair["b"], pair["emb"]
    la, lb = a.prefill(emb).float(), b.prefill(emb).float()
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), "the prompt pass runs the bf16 image of the same values: same bits"
    left_out, total, worst = 0, 0, 0.0
    for t in range(STEPS):
        scale = float(lb.abs().max())
        err = float((la - lb).abs().max()) / scale
        worst = max(worst, err)
        print(f"[mxfp4 {pair['arch']}] step {t}: max |A - B| / max |B| = {err:.3e} (bound {BOUND_LOGITS[0]:.3e})")
        assert err <= BOUND_LOGITS[0], (t, err)
        top2 = lb.topk(2, -1).values
        clear = (top2[:, 0] - top2[:, 1]) > 2 * BOUND_LOGITS[0] * scale      # either logit may move by the bound
        assert torch.equal(la.argmax(-1)[clear], lb.argmax(-1)[clear]), t
        left_out += int((~clear).sum())
        total += clear.numel()
        tok = lb.argmax(-1)                                                  # B's greedy token feeds both engines
        la, lb = a.decode_step(tok).float(), b.decode_step(tok).float()
    print(f"[mxfp4 {pair['arch']}] worst {worst:.3e}; {left_out} of {total} positions inside the margin band")
    assert left_out * 4 <= total


def test_against_the_oracle_over_the_fake_quantised_weights(pair):
    a, emb, cfg = pair["a"], pair["emb"], pair["cfg"]
    worst, scale, checked, near, _, _ = _teacher_forced_check(a, emb, pair["wq"], cfg, STEPS)
    print(f"[mxfp4 {pair['arch']}] logits max|err| {worst:.3e} vs the fake-quantised oracle (scale {scale:.3e}, LOGIT_TOL {LOGIT_TOL}); "
          f"{checked} exact, {near} near-tie flips")
    assert checked > 0
    # ... and it really is the quantised model: the unquantised oracle is farther away
    lg_q = O.decoder_prefill(pair["wq"], cfg, emb.float().cpu(), "bf16")[0]
    lg_b = O.decoder_prefill(pair["w"], cfg, emb.float().cpu(), "bf16")[0]
    got = a.prefill(emb).float().cpu()
    assert float((got - lg_q).abs().max()) < float((got - lg_b).abs().max())


def test_generation_deterministic_graph_eager_lookup_and_continuous_batch(pair):
    a, emb, cfg = pair["a"], pair["emb"], pair["cfg"]
    kw = dict(max_length=emb.shape[1] + 70, eos_token_id=-1, pad_token_id=cfg.pad_token_id)
    plain = a.generate(emb, **kw).cpu()
    assert plain.shape == (3, 70) and torch.equal(plain, a.generate(emb, **kw).cpu())
    os.environ["SV_NO_GRAPH"] = "1"
    try:
        assert torch.equal(plain, a.generate(emb, **kw).cpu()), "graph != eager"
    finally:
        os.environ.pop("SV_NO_GRAPH", None)
    # greedy prompt-lookup decoding, K = 7: K + 1 rows per sequence through the same kernels
    assert torch.equal(a.generate_lookup(emb, num_draft_tokens=7, **kw).cpu(), plain), "lookup != plain"
    # a 3-request continuous batch against the solo calls
    solo = [a.generate(emb[i:i + 1].contiguous(), **kw).cpu()[0].tolist() for i in range(3)]
    assert solo == plain.tolist()
    a.cb_reset()
    try:
        slots = a.cb_admit(emb.contiguous(), [dict(max_new_tokens=70, eos_token_id=-1)] * 3)
        for _ in range(200):
            if not any(a.cb_poll()[0][s] for s in slots):
                break
            a.cb_step(8)
        live, steps = a.cb_poll()
        assert not any(live[s] for s in slots)
        for i, s in enumerate(slots):
            assert a.cb_read(s, 0, steps[s]).tolist() == solo[i], f"continuous batch request {i}"
    finally:
        a.cb_reset()


def test_row_0_does_not_depend_on_the_batch_at_8b_dimensions():
    """2 decoder layers at StarVector-8B's dimensions (hidden 4608, n_inner 18432), a 64-row mxfp4 engine: row 0's teacher-forced fp32 logits
    over 4 decode steps are bit-identical at B = 1, 32, 33 and 64 (row tiles ride on grid.z of one kernel: by construction)."""
    from oracle.hostinfo import host_cores
    torch.set_num_threads(host_cores())
    cfg = dataclasses.replace(O.OracleConfig.starvector_8b(), n_layer=2, vit_layers=1, eos_token_id=-1)
    w = O.make_weights(cfg, seed=83)
    eng = build_engine(cfg, w, max_batch=64, max_seq_len=64, weight_dtype="mxfp4")
    try:
        ids = torch.randint(0, 4000, (64, 40), generator=torch.Generator().manual_seed(84))
        toks = torch.randint(0, 4000, (64, 4), generator=torch.Generator().manual_seed(85), dtype=torch.int64)
        emb = eng.embed_tokens(ids.to(dev()))
        runs = {}
        for B in (64, 1, 32, 33):
            out = [eng.prefill(emb[:B].contiguous())[0]]
            for t in range(4):
                out.append(eng.decode_step(toks[:B, t].to(dev()))[0])
            runs[B] = torch.stack(out).float()
        assert bool(torch.isfinite(runs[64]).all()) and float(runs[64].abs().max()) > 0
        for B in (1, 32, 33):
            assert torch.equal(runs[B].view(torch.int32), runs[64].view(torch.int32)), f"row 0 at B = {B} differs from B = 64"
    finally:
        eng.close()


def test_a_k_without_a_fitting_cut_is_refused_at_create():
    """n_inner = 1088: the down projection's K is 68 k-steps, which no wave count cuts into whole groups of 4 for two waves or more."""
    import starvector_amd as sva
    cfg = O.OracleConfig.tiny()
    ec = sva.EngineConfig(image_size=cfg.image_size, patch_size=cfg.patch_size, vit_width=cfg.vit_width, vit_layers=cfg.vit_layers,
                          vit_heads=cfg.vit_heads, adapter_norm=cfg.adapter_norm, hidden=cfg.hidden, n_layer=cfg.n_layer, n_head=cfg.n_head,
                          n_inner=1088, vocab=cfg.vocab, n_positions=cfg.n_positions, max_batch=4, max_seq_len=64, weight_dtype="mxfp4")
    with pytest.raises(NotImplementedError, match=r"mlp\.c_proj K=1088"):        # SV_ENOTSUP
        sva.HipEngine(ec)
    sva.HipEngine(dataclasses.replace(ec, weight_dtype="bf16")).close()          # the shape itself is fine


def test_from_pretrained_and_llm_generate_with_mxfp4_on_a_checkpoint(tmp_path, capfd):
    """The format is reachable from what a user calls: `from_pretrained(path, weight_dtype="mxfp4")` and `LLM(path, quantization="mxfp4")` on a
    checkpoint directory in the reference's format; both say once that the mode is not the reference's precision, and agree on the greedy tokens."""
    import numpy as np
    from PIL import Image
    from starvector_amd import vllm as VL
    from starvector_amd.model import StarVectorForCausalLM
    from tests.ckpt_util import write_reference_checkpoint
    cfg = O.OracleConfig.tiny()
    path = str(tmp_path / "ckpt")
    write_reference_checkpoint(path, cfg, O.make_weights(cfg, seed=21))
    llm = VL.LLM(model=path, max_num_seqs=4, max_model_len=min(96, cfg.n_positions), byte_tokenizer_fallback=True, quantization="mxfp4")
    assert llm.engine.cfg.weight_dtype == "mxfp4"
    err = capfd.readouterr().err
    assert err.count("decoder weights quantised to mxfp4") == 1 and "not the reference's precision" in err
    rng = np.random.default_rng(3)
    inputs = [{"prompt": "<image-start>", "multi_modal_data": {"image": Image.fromarray(rng.integers(0, 255, (40, 48, 3), dtype=np.uint8))}}]
    sp = VL.SamplingParams(n=1, temperature=0.0, max_tokens=12, ignore_eos=True)
    toks = list(llm.generate(inputs, sp, use_tqdm=False)[0].outputs[0].token_ids)
    assert len(toks) == 12
    emb = llm.prepare(inputs, [sp])[0]["emb"]
    llm.engine.cb_reset()
    model = StarVectorForCausalLM.from_pretrained(path, weight_dtype="mxfp4", byte_tokenizer_fallback=True)
    assert model.engine.cfg.weight_dtype == "mxfp4"
    got = model.engine.generate(emb, max_length=emb.shape[1] + 12, eos_token_id=-1, pad_token_id=cfg.pad_token_id).cpu()[0].tolist()
    assert got == toks
    with pytest.raises(ValueError, match="quantization"):
        VL.LLM(model=path, quantization="int4", byte_tokenizer_fallback=True)
