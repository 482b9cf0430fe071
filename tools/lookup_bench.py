"""Prompt-lookup speculative decoding against the plain greedy call, alternating in ONE process so that every arm sees the same box:

  plain        generate: one token per decode step
  rejected K   generate_lookup with forced drafts that are all wrong: one token per verification step of K + 1 rows -- its step time over
               plain's is what verification costs when nothing is accepted (the pre-write launch per layer, the lookup step, wider rows)
  accepted K   generate_lookup with the plain call's own continuation as drafts: K + 1 tokens per step, the ceiling
  natural K    generate_lookup drafting by n-gram lookup over the model's own stream, with its measured acceptance

StarVector-1B shapes with bench.py's synthetic weights, one 259-row prompt, 1024 new tokens, EOS off.  The stream of random weights is not
SVG: the natural arm's acceptance says nothing about real checkpoints.  Step time = sv_last_timing's decode wall clock over the steps
the call ran.  The engine keeps ONE captured verification step, keyed by K and the call's parameters, and captures it inside the decode wall
clock when the key changes: every arm is therefore called TWICE back to back and only the second call is timed; `rounds` rounds run all arms in turn.
Every lookup arm's tokens are compared with the plain call's.  Prints one JSON line per arm and a markdown table.

--sample: the same arms for SAMPLED decoding (top_k 50, top_p 0.9, a fixed seed; --penalty 1.1 adds the repetition penalty): plain is
generate(do_sample=True, ...), the lookup arms are generate_lookup_sampled with the same selection, the forced drafts are the plain sampled
call's own tokens (accepted) and those tokens + 1 (rejected).  --penalty without --sample: greedy under the penalty.  The natural arm's
acceptance under sampling on random weights says even less than the greedy one.

    python tools/lookup_bench.py [--new 1024] [--rounds 3] [--shared] [--only plain,rejected7] [--sample] [--penalty 1.1]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S0 = 259


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shared", action="store_true", help="exclusive_device off: no fused row-update + c_attn / MLP launches")
    ap.add_argument("--only", default="", help="comma-separated arm names")
    ap.add_argument("--sample", action="store_true", help="sampled decoding: top_k 50, top_p 0.9, seed 7 (generate_lookup_sampled)")
    ap.add_argument("--penalty", type=float, default=1.0, help="repetition_penalty of every arm (generate_lookup_sampled)")
    a = ap.parse_args()
    import torch
    import starvector_amd as sva
    ec = sva.EngineConfig(max_batch=16, max_seq_len=S0 + a.new, exclusive_device=not a.shared)
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=1234)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1, S0, ec.hidden, generator=g) * 0.5).to(torch.bfloat16).to(torch.device("cuda", eng.device))
    kw = dict(max_length=S0 + a.new, eos_token_id=-1, pad_token_id=49152)
    sel = dict(do_sample=True, top_k=50, top_p=0.9, temperature=1.0, seed=7) if a.sample else {}
    if a.penalty != 1.0:
        sel["repetition_penalty"] = a.penalty
    kw.update(sel)
    call_lookup = eng.generate_lookup_sampled if sel else eng.generate_lookup
    plain = eng.generate(x, **kw).cpu()
    stream = plain[0].tolist()
    wrong = [(t + 1) % 49152 for t in stream]

    def lookup(K, forced):
        def run():
            eng.set_lookup_drafts(None if forced is None else [forced])
            try:
                return call_lookup(x, num_draft_tokens=K, return_counts=True, **kw)
            finally:
                eng.set_lookup_drafts(None)
        return run
    arms = {"plain": lambda: (eng.generate(x, **kw), dict(steps=a.new - 1, drafted=0, accepted=0)),
            "rejected3": lookup(3, wrong), "rejected7": lookup(7, wrong), "rejected15": lookup(15, wrong),
            "accepted3": lookup(3, stream), "accepted7": lookup(7, stream), "accepted15": lookup(15, stream),
            "natural7": lookup(7, None)}
    if a.only:
        arms = {k: v for k, v in arms.items() if k in a.only.split(",")}
    res = {k: dict(ms=[], steps=0, drafted=0, accepted=0, same=True) for k in arms}
    for r in range(a.rounds):
        for name, fn in arms.items():
            fn()                                               # untimed: leaves this arm's captured step as the kept one
            toks, c = fn()
            t = eng.last_timing()
            res[name]["same"] = res[name]["same"] and bool(torch.equal(toks.cpu(), plain))
            res[name].update(steps=c["steps"], drafted=c["drafted"], accepted=c["accepted"])
            res[name]["ms"].append(t["decode_ms"])
    base = statistics.median(res["plain"]["ms"]) / (a.new - 1) if "plain" in res else None
    rows = []
    for name, v in res.items():
        ms = statistics.median(v["ms"])
        step_us = 1e3 * ms / max(v["steps"], 1)
        out = dict(arm=name, new_tokens=a.new, steps=v["steps"], drafted=v["drafted"], accepted=v["accepted"], tokens_equal_plain=v["same"],
                   decode_ms=round(ms, 3), step_us=round(step_us, 1), tokens_per_step=round((a.new - 1) / max(v["steps"], 1), 3),
                   tok_per_s=round(1e3 * (a.new - 1) / ms, 1), step_over_plain=round(step_us / (1e3 * base), 4) if base else None,
                   exclusive_device=not a.shared, rounds=a.rounds, sample=a.sample, repetition_penalty=a.penalty)
        rows.append(out)
        print(json.dumps(out))
    print("\n| arm | steps | tokens / step | accepted / drafted | step (us) | step / plain step | tok/s | tokens == plain |")
    print("|---|---|---|---|---|---|---|---|")
    for o in rows:
        print(f"| {o['arm']} | {o['steps']} | {o['tokens_per_step']} | {o['accepted']} / {o['drafted']} | {o['step_us']} | {o['step_over_plain']} | "
              f"{o['tok_per_s']} | {o['tokens_equal_plain']} |")
    eng.close()


if __name__ == "__main__":
    main()
