#!/usr/bin/env python3
"""Continuous-batching step cost by sampler arm, in ONE process (1B dimensions, random weights): HF-mode sampling (the path before
vLLM semantics), vLLM mode with every field neutral, min_p only, penalties + logit bias, and everything on.  The arms alternate
round by round (`--rounds` x `--steps` timed decode steps each) so that clock drift spreads over all of them.
    python tools/cb_sampling_ab.py [--live 32] [--steps 256] [--rounds 4] > profiles/cb_sampling_ab.log"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import starvector_amd as sva  # noqa: E402
from bench import synthetic_images  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--live", type=int, default=32)
ap.add_argument("--steps", type=int, default=256, help="timed decode steps per arm per round")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--per-call", type=int, default=32, help="decode steps per cb_step call (one graph launch)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
warm = 2 * a.per_call
budget = a.steps + warm + 8
ec = sva.EngineConfig(max_batch=a.live, max_seq_len=259 + budget + 8)
ec.exclusive_device = True
eng = sva.HipEngine(ec)
eng.load_random_weights(seed=1234)
img = synthetic_images(torch, a.live, 224, seed=0).to(dev)
prompt = [7, 11]
emb = eng.prepare_inputs(eng.encode_image(img), torch.tensor([prompt] * a.live, dtype=torch.long, device=dev))

samp = dict(max_new_tokens=budget, eos_token_id=-1, pad_token_id=49152, do_sample=True, temperature=0.8, top_p=0.95, top_k=0)
pen = dict(repetition_penalty=1.1, frequency_penalty=0.3, presence_penalty=0.2, prompt_ids=prompt,
           logit_bias={49151: -100.0, 10: 0.5, 20: 0.5, 30: -0.5, 40: 1.0})
ARMS = {
    "hf": dict(samp),
    "vllm_neutral": dict(samp, semantics="vllm"),
    "min_p": dict(samp, semantics="vllm", min_p=0.05),
    "penalties_bias": dict(samp, semantics="vllm", **pen),
    "all_on": dict(samp, semantics="vllm", min_p=0.05, min_new_tokens=budget // 2, stop_any_ids=[49150, 49149], **pen),
}
times = {k: [] for k in ARMS}
live_end = {}
for r in range(a.rounds):
    for name, req in ARMS.items():
        eng.cb_reset()
        eng.cb_admit(emb, [dict(req, seed=1000 * r + i) for i in range(a.live)])
        eng.cb_step(warm)                                       # graph capture (first round), warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while n < a.steps:
            live = eng.cb_step(a.per_call)
            n += a.per_call
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / n * 1e6)
        live_end[name] = live
eng.cb_reset()
base = sum(times["hf"]) / len(times["hf"])
for name, ts in times.items():
    m = sum(ts) / len(ts)
    print(json.dumps({"arm": name, "live": a.live, "steps": a.steps * a.rounds, "us_per_step": round(m, 1),
                      "rounds_us": [round(t, 1) for t in ts], "vs_hf_pct": round(100 * (m / base - 1), 2),
                      "live_at_end": live_end[name]}))
eng.close()
