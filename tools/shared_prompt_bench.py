"""Time to first token and decode step of a B x G sampling call on three routes, interleaved in one process per case:

  (a) repeated   generate on the prompts repeated G times (B * G rows through the prompt pass)
  (b) shared     generate_shared: one prompt pass over the B prompts, the fork launch, B * G decode rows
  (c) plain      generate on the B prompts, one sample each (for scale: the prompt pass (b) runs)

StarVector-1B shapes with bench.py's synthetic weights, 259-row prompts (257 image rows + 2 prompt ids), 64 new tokens, EOS off.
TTFT is sv_last_timing's (prompt pass + first token, host wall clock around a stream synchronise), the step time its decode wall
clock over the decode steps.  The engine keeps ONE captured decode graph, keyed by the decode rows and the sampling parameters, and
captures it inside the decode wall clock when the key changes: (c) has other rows than (a) and (b), which share a key.  So every
route is called TWICE back to back and only the second call is timed -- its graph is the kept one for every route alike -- and the
order of (a) and (b) alternates between rounds.  Prints one JSON line per case.

    python tools/shared_prompt_bench.py                 # both cases, each in a child process under its own time limit
    python tools/shared_prompt_bench.py --case 4 8      # one case, in this process
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(4, 8), (1, 32)]
S0, N_NEW = 259, 64


def run_case(B, G, rounds, warmup):
    import torch
    import starvector_amd as sva
    ec = sva.EngineConfig(max_batch=B * G, max_seq_len=S0 + N_NEW)
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=1234)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(B, S0, ec.hidden, generator=g) * 0.5).to(torch.bfloat16).to(torch.device("cuda", eng.device))
    rep = x.repeat_interleave(G, dim=0).contiguous()
    kw = dict(max_length=S0 + N_NEW, do_sample=True, temperature=0.9, top_p=0.95, top_k=50, seed=7, eos_token_id=-1)
    routes = {"repeated": lambda: eng.generate(rep, **kw), "shared": lambda: eng.generate_shared(x, n_samples=G, **kw),
              "plain": lambda: eng.generate(x, **kw)}
    ttft = {k: [] for k in routes}
    step = {k: [] for k in routes}
    same = None
    for r in range(warmup + rounds):
        outs = {}
        order = ["repeated", "shared", "plain"] if r % 2 == 0 else ["shared", "repeated", "plain"]
        for name in order:                                     # interleaved: every round runs the three routes
            fn = routes[name]
            fn()                                               # untimed: leaves this route's decode graph as the kept one
            outs[name] = fn()
            t = eng.last_timing()
            if r >= warmup:
                ttft[name].append(t["ttft_ms"])
                step[name].append(1e3 * t["decode_ms"] / max(t["decode_steps"], 1))
        same = bool(torch.equal(outs["repeated"], outs["shared"])) if same is None else same and bool(torch.equal(outs["repeated"], outs["shared"]))
    eng.close()

    def stat(v):
        return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    return {"B": B, "G": G, "S0": S0, "new_tokens": N_NEW, "rounds": rounds, "tokens_equal": same,
            "ttft_ms": {k: stat(v) for k, v in ttft.items()}, "step_us": {k: stat(v) for k, v in step.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs=2, type=int, metavar=("B", "G"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=280, help="seconds a case may take")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case[0], a.case[1], a.rounds, a.warmup)), flush=True)
        return 0
    for B, G in CASES:                                         # every GPU step under its own limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", str(B), str(G),
               "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(f"case B={B} G={G} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
