"""What the continuous batch's prefix cache (sv_cb_set_prefix_cache) costs and saves at admit, in ONE process so that every arm sees the same box:

  off    the cache off: the admit as it is without the feature (on a tree without the entry point this is the only arm: the same script run
         there gives the parent's admit on the same box)
  miss   the cache on, prompts nobody has brought before: the admit's ordinary prompt pass plus the digest launch, its copy to the host and the
         host's table work -- miss over off is what the feature costs a request that gains nothing
  hit    the cache on, the same prompts admitted and released before: every full page but the last-row's is reused and the prompt pass computes
         only the rows behind them

StarVector-1B shapes: 32 prompts of 259 rows; StarVector-8B shapes: 16 prompts of 578 rows (576 visual + 2), bench.py's synthetic weights,
one sv_cb_admit_ragged call for all of them, 8 new tokens per request, EOS off.  Time = host wall clock around the admit call (it is
synchronous: the first token of every request is selected when it returns; it includes the binding's packing of the prompts into one
buffer, a device copy that is the same in every arm), median and min .. max over the rounds after one untimed round per
arm.  `step` = host wall clock of sv_cb_step(8) / 8 with all admitted requests live, cache off and on.  Prints one JSON line per arm and a
markdown table.

    python tools/prefix_cache_bench.py [--models 1b,8b] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS_PER_CALL = 8
SHAPES = {"1b": (32, 259), "8b": (16, 578)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="1b,8b")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    import starvector_amd as sva
    out_rows = []
    for model in a.models.split(","):
        n, S0 = SHAPES[model]
        ec = sva.EngineConfig.starvector_8b(max_batch=n, max_seq_len=1024) if model == "8b" else sva.EngineConfig(max_batch=n, max_seq_len=1024)
        eng = sva.HipEngine(ec)
        eng.load_random_weights(seed=1234)
        has = hasattr(eng, "cb_set_prefix_cache")
        dev = torch.device("cuda", eng.device)
        reqs = [dict(max_new_tokens=64, eos_token_id=-1, pad_token_id=0) for _ in range(n)]

        def prompts(seed):
            g = torch.Generator().manual_seed(seed)
            return list((torch.randn(n, S0, ec.hidden, generator=g) * 0.5).to(torch.bfloat16).to(dev))

        def admit(xs, steps=0):
            """(admit ms, step us or None, info); the requests are released afterwards"""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            slots = eng.cb_admit(xs, reqs)
            ms = 1e3 * (time.perf_counter() - t0)
            us = None
            if steps:
                eng.cb_step(STEPS_PER_CALL)              # untimed: captures the bucket's graph
                t0 = time.perf_counter()
                for _ in range(steps):
                    eng.cb_step(STEPS_PER_CALL)
                us = 1e6 * (time.perf_counter() - t0) / (steps * STEPS_PER_CALL)
            info = eng.cb_prefix_cache_info() if has else None
            for s in slots:
                eng.cb_release(s)
            return ms, us, info

        arms = ["off"] + (["miss", "hit"] if has else [])
        res = {k: dict(ms=[], us=[], info=None) for k in arms}
        seed = 100
        for arm in arms:
            eng.cb_reset()
            if has:
                eng.cb_set_prefix_cache(arm != "off")
            same = prompts(7)
            admit(same)                                  # untimed: workspaces, and the donor of the hit arm
            for r in range(a.rounds):
                seed += 1
                ms, us, info = admit(same if arm == "hit" else prompts(seed), steps=4 if arm != "miss" else 0)
                res[arm]["ms"].append(ms)
                if us is not None:
                    res[arm]["us"].append(us)
                res[arm]["info"] = info
        eng.cb_reset()
        if has:
            eng.cb_set_prefix_cache(False)
        base = statistics.median(res["off"]["ms"])
        for arm in arms:
            v = res[arm]
            ms = statistics.median(v["ms"])
            o = dict(model=model, prompts=n, rows=S0, arm=arm, admit_ms=round(ms, 3), admit_ms_min_max=[round(min(v["ms"]), 3), round(max(v["ms"]), 3)],
                     admit_over_off=round(ms / base, 4), step_us=round(statistics.median(v["us"]), 1) if v["us"] else None,
                     step_us_min_max=[round(min(v["us"]), 1), round(max(v["us"]), 1)] if v["us"] else None, info=v["info"], rounds=a.rounds)
            out_rows.append(o)
            print(json.dumps(o), flush=True)
        eng.close()
    print("\n| model | prompts x rows | arm | admit ms (min .. max) | admit / off | decode step us (min .. max) | pages reused / looked up |")
    print("|---|---|---|---|---|---|---|")
    for o in out_rows:
        i = o["info"] or {}
        st = f"{o['step_us']} ({o['step_us_min_max'][0]} .. {o['step_us_min_max'][1]})" if o["step_us"] is not None else "-"
        print(f"| {o['model']} | {o['prompts']} x {o['rows']} | {o['arm']} | {o['admit_ms']} ({o['admit_ms_min_max'][0]} .. {o['admit_ms_min_max'][1]}) | "
              f"{o['admit_over_off']} | {st} | {i.get('reused', '-')} / {i.get('lookups', '-')} |")


if __name__ == "__main__":
    main()
