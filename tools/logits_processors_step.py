"""Decode step time of a greedy call with a token ban next to the same call with a repetition penalty: both take the separate selection
launch, the ban adds ban_tokens_kernel (processors.hip) in front of it.

StarVector-1B shapes with bench.py's synthetic weights, batch 32, 259-row prompts, 1024 new tokens, EOS off.  The step time is
sv_last_timing's decode wall clock over the decode steps.  The engine keeps one captured decode graph per parameter set, built inside the
decode wall clock: every route is called twice back to back and only the second call is timed; the routes alternate between rounds.  On a
tree without generate_processed only the repetition-penalty route runs.  Prints one JSON line.

    python tools/logits_processors_step.py [--rounds 5] [--ngram 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, S0, N_NEW = 32, 259, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ngram", type=int, default=3)
    a = ap.parse_args()
    import torch
    import starvector_amd as sva
    ec = sva.EngineConfig(max_batch=B, max_seq_len=S0 + N_NEW)
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=1234)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(B, S0, ec.hidden, generator=g) * 0.5).to(torch.bfloat16).to(torch.device("cuda", eng.device))
    kw = dict(max_length=S0 + N_NEW, eos_token_id=-1)
    routes = {"plain_greedy": lambda: eng.generate(x, **kw),
              "repetition_penalty_1.1": lambda: eng.generate(x, repetition_penalty=1.1, **kw)}
    if hasattr(eng, "generate_processed"):
        routes[f"no_repeat_ngram_{a.ngram}"] = lambda: eng.generate_processed(x, no_repeat_ngram_size=a.ngram, **kw)
    step = {k: [] for k in routes}
    nodes = {}
    for r in range(a.rounds):
        for name in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            routes[name]()                                      # untimed: leaves this route's decode graph as the kept one
            routes[name]()
            t = eng.last_timing()
            step[name].append(1e3 * t["decode_ms"] / max(t["decode_steps"], 1))
            nodes[name] = eng.step_plan()["graph_kernel_nodes"]
    eng.close()
    print(json.dumps({"batch": B, "S0": S0, "new_tokens": N_NEW, "rounds": a.rounds,
                      "step_us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                  for k, v in step.items()},
                      "graph_kernel_nodes": nodes}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
