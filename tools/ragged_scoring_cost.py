#!/usr/bin/env python3
"""Time of the scoring pass over completions of different lengths, padded and ragged, on the same inputs: StarVector-1B dimensions, random
weights, B = 32 right-padded rows whose lengths are spread evenly between a quarter and the whole of S = 2048 (shuffled), the first `--prefix`
rows of every row the visual prefix and the rest its completion, every completion token scored -- the calls completion_logprobs makes for a
right-padded roll-out batch.
  padded   forward_logprobs over [B][S] with n_keep = S - prefix + 1: pads go through every layer and the lm_head (the call of the parent commit)
  ragged   forward_logprobs_ragged over the packed rows, row b keeping its own lens[b] - prefix + 1 rows (completion_logprobs(..., unpadded=True))
Host clock around a call that blocks until the pass has finished; one warm-up call per form (workspaces, GEMM tuning), then the two forms take
turns `--reps` times; median.  Beside the times: the share of the padded call's rows that are pads, layers (sum(lens) / (B * S)) and lm_head
(sum(keep) / (B * n_keep)) -- the ratios the saving is to be read against.
    python tools/ragged_scoring_cost.py [--batch 32] [--seq 2048] [--reps 5] [--prefix 256] [--top-k 0] [--out profiles/ragged_scoring.md]"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import starvector_amd as sva  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prefix", type=int, default=256)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_scoring.md"))
    a = ap.parse_args()
    B, S = a.batch, a.seq
    lens = [S // 4 + (S - S // 4) * b // max(B - 1, 1) for b in range(B)]          # a quarter .. the whole of S, evenly
    random.Random(0).shuffle(lens)                                                 # rows arrive in any order
    if not 0 < a.prefix < min(lens):
        ap.error(f"--prefix must be in 1..{min(lens) - 1}")
    keep = [n - a.prefix + 1 for n in lens]
    n_pad = S - a.prefix + 1
    ec = sva.EngineConfig(max_batch=B, max_seq_len=S)
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=1234, std=0.02)
    g = torch.Generator().manual_seed(0)
    emb = eng.embed_tokens(torch.randint(0, ec.vocab, (B, S), generator=g).cuda())
    mask = torch.arange(S).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)
    packed = emb[mask.cuda()].contiguous()
    tg_pad = torch.randint(0, ec.vocab, (B, n_pad), generator=g).to(torch.int32).cuda()
    tg_rag = torch.randint(0, ec.vocab, (sum(keep),), generator=g).to(torch.int32).cuda()
    kw = dict(top_k=a.top_k) if a.top_k else {}
    forms = {"padded": lambda: eng.forward_logprobs(emb, tg_pad, n_pad, 0.7, **kw),
             "ragged": lambda: eng.forward_logprobs_ragged(packed, tg_rag, keep, lengths=lens, temperature=0.7, **kw)}
    ms = {f: [] for f in forms}
    for r in range(a.reps + 1):
        for f, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                  # blocks until the pass has finished
            if r:
                ms[f].append((time.perf_counter() - t0) * 1e3)
    med = {f: statistics.median(v) for f, v in ms.items()}
    layer_share, head_share = sum(lens) / (B * S), sum(keep) / (B * n_pad)
    lines = [
        "# Scoring pass over completions of different lengths: padded against ragged",
        "",
        f"`tools/ragged_scoring_cost.py`: StarVector-1B dimensions, random weights, B = {B} right-padded rows, S = {S}, lengths {min(lens)} .. {max(lens)} "
        f"(sum {sum(lens)}), a prefix of {a.prefix} rows and every completion token scored (kept rows: padded {B} x {n_pad}, ragged {sum(keep)}), "
        f"top_k = {a.top_k}, temperature 0.7.  Host clock around the blocking call, 1 warm-up + {a.reps} timed calls per form, taking turns; median.",
        "",
        "| form | ms per call | calls |",
        "|---|---|---|",
    ] + [f"| {f} | {med[f]:.2f} | {' '.join('%.2f' % v for v in ms[f])} |" for f in forms] + [
        "",
        f"ragged / padded time: {med['ragged'] / med['padded']:.3f}",
        f"rows through the layers, ragged / padded: {layer_share:.3f} ({100 * (1 - layer_share):.1f} % of the padded call's rows are pads)",
        f"rows through the lm_head, ragged / padded: {head_share:.3f}",
        "",
    ]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
