#!/usr/bin/env python3
"""Time per decode step and launches per step of a roll-out that returns the top-k lists (sv_generate_topk) at StarVector-1B, B = 32, random
weights, fixed-length calls: plain ("off"), the three statistics ("stats"), the lists alone with k = 1, 5, 20, 32 under the raw distribution with
the rank ("tk1" ... "tk32"), k = 20 under the processed distribution ("tk20p") and k = 20 beside the statistics ("stats+tk20").  The engine
keeps ONE captured step, so each form runs one warm-up call (capture + instantiation) and then `reps` timed calls; the forms take turns `rounds`
times.  Median over all timed calls.  Then the scoring pass (forward_logprobs) over 32 x 256 kept positions with and without top_k = 20, and one
launch of the row function on 32 random rows (the selection arm) and on 32 flat rows (the arm of k arg-max rounds), host clock around launch + synchronise.
    python tools/token_topk_cost.py [--new-tokens 256] [--reps 3] [--rounds 2] [--forms off,stats,tk1,tk5,tk20,tk32,tk20p,stats+tk20]
`--forms off` runs on a build without the lists as well (the same figures of the parent commit)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import starvector_amd as sva  # noqa: E402

FORMS = {"off": {}, "stats": dict(token_stats=True),
         "tk1": dict(token_topk=1), "tk5": dict(token_topk=5), "tk20": dict(token_topk=20), "tk32": dict(token_topk=32),
         "tk20p": dict(token_topk=dict(k=20, source="processed")), "stats+tk20": dict(token_stats=True, token_topk=20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--score-reps", type=int, default=5)
    a = ap.parse_args()
    forms = a.forms.split(",")
    B, n, S0 = a.batch, a.new_tokens, 16
    ec = sva.EngineConfig(max_batch=B, max_seq_len=S0 + n)
    ec.exclusive_device = True
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=1234, std=0.02)
    ids = torch.randint(0, 49152, (B, S0), generator=torch.Generator().manual_seed(0)).cuda()
    emb = eng.embed_tokens(ids)
    modes = {"greedy": dict(), "top-k 50 + top-p 0.95 sampling": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, seed=3)}
    print(f"StarVector-1B dims, random weights, B = {B}, {n} new tokens per call (EOS off); per form 1 warm-up + {a.reps} timed calls, "
          f"{a.rounds} rounds; forms: {forms}")
    for name, kw in modes.items():
        t = {f: [] for f in forms}
        nodes, toks = {}, {}
        for _ in range(a.rounds):
            for f in forms:
                for r in range(a.reps + 1):
                    o = eng.generate(emb, max_length=S0 + n, eos_token_id=-1, pad_token_id=0, **kw, **FORMS[f])
                    torch.cuda.synchronize()
                    lt = eng.last_timing()
                    if r == 0:                                   # the warm-up call captured this form's step
                        nodes[f] = eng.step_plan()["graph_kernel_nodes"]
                    else:
                        t[f].append(lt["decode_ms"] * 1e3 / max(lt["decode_steps"], 1))
                toks[f] = o["sequences"] if isinstance(o, dict) else o
        for f in forms:
            med = statistics.median(t[f])
            print(f"{name:32s} {f:10s} {med:8.1f} us/step  {nodes[f]:4d} launches/step  added {med - statistics.median(t[forms[0]]):7.1f} us/step  "
                  f"tokens identical to '{forms[0]}': {torch.equal(toks[f], toks[forms[0]])}  ({['%.1f' % x for x in t[f]]})")
    # the scoring pass: 32 sequences, the last 256 positions of each kept (8192 rows of logits: two lm_head chunks)
    x = eng.embed_tokens(torch.randint(0, 49152, (B, S0 + n), generator=torch.Generator().manual_seed(1)).cuda())
    tg = torch.randint(0, 49152, (B, n), generator=torch.Generator().manual_seed(2)).to(torch.int32).cuda()
    for label, kw in (("forward_logprobs", {}), ("forward_logprobs top_k=20", dict(top_k=20))):
        if kw and not any(f.startswith(("tk", "stats+")) for f in forms):
            continue                                             # a build without the lists
        ms = []
        for r in range(a.score_reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.forward_logprobs(x, tg, n, 0.7, **kw)            # blocks until the pass has finished
            if r:
                ms.append((time.perf_counter() - t0) * 1e3)
        print(f"scoring pass {B} x {n} positions  {label:28s} {statistics.median(ms):8.2f} ms  ({['%.2f' % v for v in ms]})")
    # the two arms of row_topk on 32 fp32 rows of the vocabulary's width (sv_op_token_topk: one launch, then a stream synchronise): random rows take
    # the selection, a row of one value everywhere -- every column a candidate -- takes k rounds of block arg-max, one sweep of the row per slot
    if any(f.startswith(("tk", "stats+")) for f in forms):
        from starvector_amd.engine import op_token_topk
        V = ec.vocab
        rows = {"random rows (selection)": torch.randn(B, V, generator=torch.Generator().manual_seed(4)).cuda(),
                "flat rows (k arg-max rounds)": torch.zeros(B, V).cuda()}
        tok = torch.zeros(B, dtype=torch.int32).cuda()
        for label, r in rows.items():
            for k in (1, 5, 32):
                us = []
                for i in range(a.score_reps * 4 + 2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    op_token_topk(r, tok, k, 0.7)
                    if i >= 2:
                        us.append((time.perf_counter() - t0) * 1e6)
                print(f"row_topk launch, {B} x {V} fp32  {label:30s} k = {k:2d}  {statistics.median(us):8.1f} us  (min {min(us):.1f})")
    eng.close()


if __name__ == "__main__":
    main()
