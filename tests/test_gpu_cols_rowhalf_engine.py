"""Engine level of tests/test_gpu_cols_rowhalf.py: the greedy token block of 24 decode steps must not depend on which form of the output
projection ran (SV_COLS_ROWHALF) -- eager and through the captured step graph, at 1 / 16 / 17 / 32 rows (one row half up to 16 rows), on
the small engine of tests/test_gpu_e2e.py and on an engine that owns its GPU (exclusive_device: the fused launches, whose pattern buffers
the output projection's launch arms at small batches).  A captured graph keeps its choice, so each setting gets its own engine; the launch
counter proves which form each engine ran.  (The write-through output stores measured beside the row-half form, DESIGN section 3j, lost
their A/B and left no switch behind: there is no second setting to cross this one with.)"""
import pytest
import torch

import starvector_amd as sva
from oracle import starvector_oracle as O
from starvector_amd import engine as E
from tests.gpu_util import build_engine, dev

pytestmark = pytest.mark.gpu

STEPS = 24
BATCHES = (1, 16, 17, 32)


def _tiny():
    cfg = O.OracleConfig.tiny()
    eng = build_engine(cfg, O.make_weights(cfg, seed=5), max_batch=32, max_seq_len=64)
    return eng, cfg.image_size, cfg.pad_token_id


def _own_gpu():
    eng = sva.HipEngine(sva.EngineConfig(max_batch=32, max_seq_len=259 + 32, exclusive_device=True))
    eng.load_random_weights(seed=13)
    return eng, 224, 49152


def _token_blocks(monkeypatch, make, rowhalf):
    """{(batch, graph?): tokens} of one engine built and run under SV_COLS_ROWHALF = rowhalf, and the row-half launches it made."""
    monkeypatch.setenv("SV_COLS_ROWHALF", str(rowhalf))
    eng, size, pad = make()
    g = torch.Generator().manual_seed(9)
    img = torch.randn(32, 3, size, size, generator=g).to(torch.bfloat16).to(dev())
    prompt = torch.tensor([[7, 11]] * 32, dtype=torch.long, device=dev())
    emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
    kw = dict(max_length=emb.shape[1] + STEPS, eos_token_id=-1, pad_token_id=pad)
    out = {}
    n0 = E.cols_rowhalf_launches()
    for graph in (False, True):
        if graph:
            monkeypatch.delenv("SV_NO_GRAPH", raising=False)
        else:
            monkeypatch.setenv("SV_NO_GRAPH", "1")
        for B in BATCHES:
            out[B, graph] = eng.generate(emb[:B].contiguous(), **kw).cpu()
            assert bool(eng.last_timing()["graph"]) == graph
    n1 = E.cols_rowhalf_launches()
    plan = eng.step_plan()
    eng.close()
    return out, (n1[0] - n0[0], n1[1] - n0[1]), plan


@pytest.mark.parametrize("make", [_tiny, _own_gpu], ids=["small_engine", "exclusive_device"])
def test_greedy_tokens_do_not_depend_on_the_output_projection_form(monkeypatch, make):
    old, n_old, _ = _token_blocks(monkeypatch, make, 0)
    assert n_old == (0, 0), "SV_COLS_ROWHALF=0 ran the row-half form"
    assert old[32, True].unique().numel() > 4                     # not a degenerate stream
    for key, ref in old.items():
        assert ref.shape == (key[0], ref.shape[1]) and torch.equal(old[key[0], True], old[key[0], False])
    new, n_new, plan = _token_blocks(monkeypatch, make, 1)
    # eager: one launch per layer and step; a batch of at most 16 rows runs ONE row half (1 and 16 of the four batches)
    assert 0 < n_new[0] < n_new[1] < 2 * n_new[0], f"row-half launches {n_new}: the form did not run, or not with one half up to 16 rows"
    if make is _own_gpu:
        assert plan["rowln_cattn_fused"] and plan["mlp_fused"], f"the engine that owns its GPU did not run the fused launches: {plan}"
    for key, ref in old.items():
        assert torch.equal(new[key], ref), f"batch {key[0]}, graph {key[1]}: tokens differ between the forms"
