"""Prompt-lookup drafting in the continuous batch (sv_cb_set_lookup) against the same batch with drafting off, alternating in ONE process so
that every arm sees the same box:

  off          the continuous batch as it is: one token per request and step
  rejected K   drafting with forced drafts that are all wrong: one token per request and verification step of (K + 1) rows per request -- its
               step time over off's is what verification costs when nothing is accepted (the pre-write launch per layer, wider rows, and the
               selection kernel's one pass)
  accepted K   drafting with each request's own continuation as drafts: K + 1 tokens per request and step, K + 1 selection passes IN SEQUENCE
               inside the slot's block -- the ceiling, and the price of sequential selection

StarVector-1B shapes with bench.py's synthetic weights, `live` requests of one 259-row prompt each on an engine of `rows` rows, `new` tokens
per request, EOS off; greedy, and top-k 50 / top-p 0.9 sampling with one seed per request.  The stream of random weights is not SVG: a
natural-draft arm would say nothing about real checkpoints, and there is none here.  Time = host wall clock around the sv_cb_step calls of a
run (8 steps per call, until no request is live); step time = that over the steps the calls ran.  The engine keeps its captured steps per
drafting setting, so every arm runs twice back to back and only the second run is timed.  Every arm's tokens are compared with off's.
Prints one JSON line per arm and a markdown table.

    python tools/cb_lookup_bench.py [--new 1024] [--rows 32,64] [--live 1,4,5] [--K 3,7] [--rounds 3] [--modes greedy,sample]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S0 = 259
STEPS_PER_CALL = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=1024)
    ap.add_argument("--rows", default="32,64")
    ap.add_argument("--live", default="1,4,5")
    ap.add_argument("--K", default="3,7")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="greedy,sample")
    a = ap.parse_args()
    import torch
    import starvector_amd as sva
    rows_out = []
    for rows in [int(v) for v in a.rows.split(",")]:
        ec = sva.EngineConfig(max_batch=rows, max_seq_len=S0 + a.new)
        eng = sva.HipEngine(ec)
        eng.load_random_weights(seed=1234)
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(1, S0, ec.hidden, generator=g) * 0.5).to(torch.bfloat16).to(torch.device("cuda", eng.device))

        def run(n, K, forced, sel):
            """(tokens per request, wall ms, steps the calls ran, totals)"""
            eng.cb_reset()
            eng.cb_set_lookup_drafts(forced)
            eng.cb_set_lookup(K)
            reqs = [dict(max_new_tokens=a.new, eos_token_id=-1, pad_token_id=49152, seed=7 + i, **sel) for i in range(n)]
            slots = eng.cb_admit([x[0]] * n, reqs)
            torch.cuda.synchronize()
            t0, calls = time.perf_counter(), 0
            while True:
                calls += 1
                if eng.cb_step(STEPS_PER_CALL) == 0:
                    break
            ms = 1e3 * (time.perf_counter() - t0)
            toks = [eng.cb_read(s, 0, a.new).tolist() for s in slots]
            totals = eng.cb_lookup_counts(-1)
            eng.cb_reset()
            return toks, ms, calls * STEPS_PER_CALL, totals

        for mode in a.modes.split(","):
            sel = dict(do_sample=True, top_k=50, top_p=0.9, temperature=1.0) if mode == "sample" else {}
            for n in [int(v) for v in a.live.split(",")]:
                plain = run(n, 0, None, sel)[0]
                arms = {"off": (0, None)}
                for K in [int(v) for v in a.K.split(",")]:
                    if n * (K + 1) > rows:
                        continue
                    arms[f"rejected{K}"] = (K, [[(t + 1) % 49152 for t in p] for p in plain])
                    arms[f"accepted{K}"] = (K, plain)
                res = {k: dict(ms=[], steps=0, totals=None, same=True) for k in arms}
                for _ in range(a.rounds):
                    for name, (K, forced) in arms.items():
                        run(n, K, forced, sel)                 # untimed: captures this arm's step graphs
                        toks, ms, steps, totals = run(n, K, forced, sel)
                        res[name]["same"] = res[name]["same"] and toks == plain
                        res[name].update(steps=steps, totals=totals)
                        res[name]["ms"].append(ms)
                base = statistics.median(res["off"]["ms"]) / res["off"]["steps"]
                for name, v in res.items():
                    ms = statistics.median(v["ms"])
                    out = dict(rows=rows, mode=mode, live=n, arm=name, new_tokens=a.new, steps_run=v["steps"], drafted=v["totals"]["drafted"],
                               accepted=v["totals"]["accepted"], tokens_equal_off=v["same"], wall_ms=round(ms, 3),
                               wall_ms_min_max=[round(min(v["ms"]), 3), round(max(v["ms"]), 3)], step_us=round(1e3 * ms / v["steps"], 1),
                               step_over_off=round(ms / v["steps"] / base, 4), tok_per_s_per_request=round(1e3 * (a.new - 1) / ms, 1), rounds=a.rounds)
                    rows_out.append(out)
                    print(json.dumps(out), flush=True)
        eng.close()
    print("\n| rows | mode | live | arm | steps run | accepted / drafted | step (us) | step / off step | tok/s per request | wall ms (min .. max) | tokens == off |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for o in rows_out:
        print(f"| {o['rows']} | {o['mode']} | {o['live']} | {o['arm']} | {o['steps_run']} | {o['accepted']} / {o['drafted']} | {o['step_us']} | "
              f"{o['step_over_off']} | {o['tok_per_s_per_request']} | {o['wall_ms_min_max'][0]} .. {o['wall_ms_min_max'][1]} | {o['tokens_equal_off']} |")


if __name__ == "__main__":
    main()
