#!/usr/bin/env python3
"""Added time per decode step of HF's per-step outputs (sv_generate_ex: output_scores + output_logits) at StarVector-1B, B = 32, random
weights, fixed-length calls: the same call with and without the two [max_new, 32, 49156] fp32 slabs, interleaved, median of N.
    python tools/capture_cost.py [--new-tokens 256] [--reps 5] > profiles/capture_cost.log"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import starvector_amd as sva  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    B, n, S0 = a.batch, a.new_tokens, 16
    ec = sva.EngineConfig(max_batch=B, max_seq_len=S0 + n)
    ec.exclusive_device = True
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=1234, std=0.02)
    ids = torch.randint(0, 49152, (B, S0), generator=torch.Generator().manual_seed(0)).cuda()
    emb = eng.embed_tokens(ids)
    V = ec.vocab
    slabs = dict(scores_out=torch.empty(n, B, V, device="cuda"), logits_out=torch.empty(n, B, V, device="cuda"))
    modes = {"greedy": dict(), "top-k 50 + top-p 0.95 sampling": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, seed=3)}
    print(f"StarVector-1B dims, random weights, B = {B}, {n} new tokens per call (EOS off), {a.reps} interleaved reps; "
          f"outputs = scores + logits slabs ({2 * B * V * 4 / 1e6:.1f} MB written per step)")
    for name, kw in modes.items():
        t = {False: [], True: []}
        toks = {}
        for r in range(a.reps + 1):
            for cap in (False, True):
                extra = dict(slabs, return_outputs=True) if cap else {}
                o = eng.generate(emb, max_length=S0 + n, eos_token_id=-1, pad_token_id=0, **kw, **extra)
                torch.cuda.synchronize()
                toks[cap] = o["sequences"] if cap else o
                lt = eng.last_timing()
                if r > 0:                                        # rep 0: graph capture + instantiation of both keys
                    t[cap].append(lt["decode_ms"] * 1e3 / max(lt["decode_steps"], 1))
        same = torch.equal(toks[False], toks[True])
        base, cap = statistics.median(t[False]), statistics.median(t[True])
        print(f"{name:32s} plain {base:8.1f} us/step   with outputs {cap:8.1f} us/step   added {cap - base:6.1f} us/step   "
              f"tokens identical: {same}   (plain {['%.1f' % x for x in t[False]]}, outputs {['%.1f' % x for x in t[True]]})")
    eng.close()


if __name__ == "__main__":
    main()
