#!/usr/bin/env python3
"""Time per decode step and launches per step of a roll-out with per-token statistics (sv_generate_stats) at StarVector-1B, B = 32, random
weights, fixed-length calls -- four forms of the same call: plain ("off"), with the three [32, max_new] statistics tensors ("stats"), with
the log-prob and the entropy alone ("stats2": what generate_im2svg_grpo(return_logprobs=True) asks for), and with HF's per-step outputs, the
two [max_new, 32, 49156] fp32 slabs ("slabs").  The engine keeps ONE captured step, so each form runs one warm-up
call (capture + instantiation) and then `reps` timed calls; the forms take turns `rounds` times.  Median over all timed calls.
    python tools/token_stats_cost.py [--new-tokens 256] [--reps 3] [--rounds 2] [--forms off,stats,stats2,slabs] > profiles/token_stats_cost.log
`--forms off` runs on a build without the statistics as well (the same figure of the parent commit)."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--forms", default="off,stats,stats2,slabs")
    a = ap.parse_args()
    forms = a.forms.split(",")
    B, n, S0 = a.batch, a.new_tokens, 16
    ec = sva.EngineConfig(max_batch=B, max_seq_len=S0 + n)
    ec.exclusive_device = True
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=1234, std=0.02)
    ids = torch.randint(0, 49152, (B, S0), generator=torch.Generator().manual_seed(0)).cuda()
    emb = eng.embed_tokens(ids)
    V = ec.vocab
    extra = {"off": {}, "stats": dict(token_stats=True), "stats2": dict(token_stats=("token_logprobs", "token_entropies"))}
    if "slabs" in forms:
        extra["slabs"] = dict(scores_out=torch.empty(n, B, V, device="cuda"), logits_out=torch.empty(n, B, V, device="cuda"), return_outputs=True)
    modes = {"greedy": dict(), "top-k 50 + top-p 0.95 sampling": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, seed=3)}
    print(f"StarVector-1B dims, random weights, B = {B}, {n} new tokens per call (EOS off); per form 1 warm-up + {a.reps} timed calls, "
          f"{a.rounds} rounds; forms: {forms}")
    for name, kw in modes.items():
        t = {f: [] for f in forms}
        nodes, toks = {}, {}
        for _ in range(a.rounds):
            for f in forms:
                for r in range(a.reps + 1):
                    o = eng.generate(emb, max_length=S0 + n, eos_token_id=-1, pad_token_id=0, **kw, **extra[f])
                    torch.cuda.synchronize()
                    lt = eng.last_timing()
                    if r == 0:                                   # the warm-up call captured this form's step
                        nodes[f] = eng.step_plan()["graph_kernel_nodes"]
                    else:
                        t[f].append(lt["decode_ms"] * 1e3 / max(lt["decode_steps"], 1))
                toks[f] = o["sequences"] if isinstance(o, dict) else o
        for f in forms:
            med = statistics.median(t[f])
            print(f"{name:32s} {f:6s} {med:8.1f} us/step  {nodes[f]:4d} launches/step  added {med - statistics.median(t[forms[0]]):7.1f} us/step  "
                  f"tokens identical to '{forms[0]}': {torch.equal(toks[f], toks[forms[0]])}  ({['%.1f' % x for x in t[f]]})")
    eng.close()


if __name__ == "__main__":
    main()
