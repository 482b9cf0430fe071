#!/usr/bin/env python3
"""Time to first token and tokens per second of a text2svg-like padded batch through `HipCausalLM.generate`: 64 prompts with lengths
drawn uniformly from 8 .. 96 (seeded), 256 new tokens, greedy and num_beams = 2, at StarVector-1B dimensions and at StarVector-8B
dimensions with fp8 weights (BASELINE config 5's call).  On an engine with the ragged prompt pass the padded mask is one prompt pass
(and, under beams, one search); without it the mirror runs one prompt pass / one search per distinct length.  The script is the same on
both, so two commits can be compared on one box:

    python tools/ragged_ttft.py --out profiles/ragged_ttft_<commit>.json [--models 1b,8b] [--new 256] [--rows 64] [--repeats 3]

Random weights (the timing does not depend on their values), EOS disabled so every row runs its whole budget.  TTFT is measured with a
one-token call (prompt pass + first selection), tokens per second over the full call; the median of --repeats runs after one warm-up."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import starvector_amd as sva                                     # noqa: E402
from starvector_amd.model import HipCausalLM                     # noqa: E402


def build(model, rows, beams, max_seq_len):
    if model == "8b":
        ec = sva.EngineConfig.starvector_8b(max_batch=rows * beams, max_seq_len=max_seq_len)
        ec.weight_dtype = "fp8_e4m3"
    else:
        ec = sva.EngineConfig(max_batch=rows * beams, max_seq_len=max_seq_len)
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=1234)
    return ec, eng


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", default="1b,8b")
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    rng = random.Random(a.seed)
    lens = [rng.randint(8, 96) for _ in range(a.rows)]
    S = max(lens)
    res = {"rows": a.rows, "new_tokens": a.new, "lengths": lens, "distinct_lengths": len(set(lens)), "runs": []}
    dev = torch.device("cuda", 0)
    for model in a.models.split(","):
        for beams in (1, 2):
            ec, eng = build(model, a.rows, beams, S + a.new + 8)
            lm = HipCausalLM(eng, eos_token_id=-1, pad_token_id=0)
            g = torch.Generator().manual_seed(a.seed)
            emb = torch.zeros(a.rows, S, ec.hidden, dtype=torch.bfloat16, device=dev)
            mask = torch.zeros(a.rows, S, dtype=torch.long, device=dev)
            for b, n in enumerate(lens):                         # left padding, as the 8B tokenizer pads
                emb[b, S - n:] = (torch.randn(n, ec.hidden, generator=g) * 0.5).to(torch.bfloat16).to(dev)
                mask[b, S - n:] = 1
            passes = getattr(eng, "prompt_passes", None)
            p0 = passes() if passes else None
            ttft, ttft_all = timed(lambda: lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=S + 1, num_beams=beams), a.repeats)
            per_call = (passes() - p0) // (a.repeats + 1) if passes else None
            full, full_all = timed(lambda: lm.generate(inputs_embeds=emb, attention_mask=mask, max_length=S + a.new, num_beams=beams), a.repeats)
            run = {"model": model, "num_beams": beams, "ttft_ms": ttft * 1e3, "ttft_ms_all": [t * 1e3 for t in ttft_all],
                   "tokens_per_s": a.rows * a.new / full, "full_s_all": full_all, "prompt_passes_per_call": per_call}
            print(json.dumps(run), flush=True)
            res["runs"].append(run)
            eng.close()
            del lm, eng
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
