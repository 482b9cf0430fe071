#!/usr/bin/env python3
"""Decode-step time vs context length (StarVector-1B shapes, B=32): generate N tokens, then profile one
step by kernel class at the context the generation ended on.  --kv-dtype / --weight-dtype / --model 8b / --batch: the same sweep with the
e4m3 KV cache, quantised decoder weights, StarVector-8B shapes (image 384, sliding window 4096) or another batch."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import starvector_amd as sva  # noqa: E402
from bench import synthetic_images  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8", "fp8_e4m3"], help="KV-cache format (EngineConfig.kv_dtype)")
ap.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8", "fp8_e4m3", "mxfp4"])
ap.add_argument("--model", default="1b", choices=["1b", "8b"])
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--new-tokens", type=int, nargs="+", default=[2, 512, 1024, 2048, 4096], help="tokens generated behind the prompt, one row each")
args = ap.parse_args()

dev = torch.device("cuda", 0)
B = args.batch
if args.model == "8b":
    cfg = sva.EngineConfig.starvector_8b(max_batch=B, max_seq_len=576 + 2 + max(args.new_tokens) + 4)
else:
    cfg = sva.EngineConfig(max_batch=B, max_seq_len=259 + max(args.new_tokens) + 4)
cfg.weight_dtype, cfg.kv_dtype = args.weight_dtype, args.kv_dtype
eng = sva.HipEngine(cfg)
eng.load_random_weights(seed=1)
print(json.dumps({"model": args.model, "batch": B, "weight_dtype": cfg.weight_dtype, **eng.kv_info()}), flush=True)
img = synthetic_images(torch, B, cfg.image_size, seed=2).to(dev)
prompt = torch.tensor([[7, 11]] * B, dtype=torch.long, device=dev)
emb = torch.cat([eng.adapter(eng.encode_image(img)), eng.embed_tokens(prompt)], 1)
S0 = emb.shape[1]
for n_new in args.new_tokens:
    eng.generate(emb, max_length=S0 + n_new, eos_token_id=-1, pad_token_id=49152)          # first call of a length: graph capture
    eng.generate(emb, max_length=S0 + n_new, eos_token_id=-1, pad_token_id=49152)
    tm = eng.last_timing()
    # per-class HIP-event time at the context the generation ended on: the MEDIAN of three profile calls (one call's event deltas came out
    # wrong once, cause not established: profiles/ctx_sweep_r03.log's 1283 row)
    profs = [eng.profile_decode_step(B, iters=5) for _ in range(3)]
    med = {k: sorted(p[k]["ms_per_step"] for p in profs)[1] for k in profs[0] if isinstance(profs[0][k], dict)}
    print(json.dumps({"ctx_end": S0 + n_new, "avg_us_per_step": round(tm["decode_ms"] / max(tm["decode_steps"], 1) * 1e3, 1),
                      "ttft_ms": round(tm["ttft_ms"], 2), "at_ctx_end_ms": {k: round(v, 4) for k, v in med.items()},
                      "others_chain_ms": round(sorted(p["others_chain_ms_per_step"] for p in profs)[1], 4),
                      "gemm_chain_ms": round(sorted(p["skinny_chain_ms_per_step"] for p in profs)[1], 4)}), flush=True)
