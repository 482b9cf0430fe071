#!/usr/bin/env python3
"""Time of GRPO's log-prob pass with the visual prefix shared, against the call of the parent commit, on the same inputs: StarVector-1B decoder
dimensions (full depth unless --layers), random weights, P images of `--prefix` visual rows, G completions of L rows per image.
  ragged     forward_logprobs_ragged over the P * G concatenations cat(prefix, completion): every prefix goes through the layers G times (the baseline:
             what completion_logprobs(..., unpadded=True) calls today)
  prefixed   forward_logprobs_prefixed over the P prefixes and the P * G completions: every prefix goes through the layers once
Both keep L + 1 rows per sequence (every completion token scored: the prefix's last row predicts the first one), and -- to split the layers from
the lm_head -- both are also timed keeping ONE row per sequence.  Host clock around a call that blocks until the pass has finished; one warm-up call
per form (workspaces, GEMM tuning), then the two forms take turns `--reps` times; median.  Beside each timing: the share of the baseline's rows the
prefixed call does not compute, (G - 1) * Pl / (G * (Pl + L)).
    python tools/prefix_scoring_sweep.py [--images 4] [--prefix 257] [--reps 7] [--layers 0] [--commit ID] [--box NAME] [--out profiles/prefix_scoring.md]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import starvector_amd as sva  # noqa: E402


def commit_id(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--prefix", type=int, default=257)
    ap.add_argument("--generations", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--completions", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--layers", type=int, default=0, help="decoder layers (0 = StarVector-1B's full depth)")
    ap.add_argument("--commit", default="")
    ap.add_argument("--box", default="", help="name of the machine for the report (default: what the runtime calls device 0)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_scoring.md"))
    a = ap.parse_args()
    P, Pl = a.images, a.prefix
    B_max, T_max = P * max(a.generations), Pl + max(a.completions)
    ec = sva.EngineConfig(vit_layers=1, max_batch=B_max, max_seq_len=T_max, **({"n_layer": a.layers} if a.layers else {}))
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=1234, std=0.02)
    g = torch.Generator().manual_seed(0)
    rows = []
    for L in a.completions:
        for G in a.generations:
            B = P * G
            prefixes = [(0.02 * torch.randn(Pl, ec.hidden, generator=g)).to(torch.bfloat16).cuda() for _ in range(P)]
            seqs = list(eng.embed_tokens(torch.randint(0, ec.vocab, (B, L), generator=g).cuda()))
            prefix_of = [b % P for b in range(B)]
            cats = [torch.cat([prefixes[u], x]) for u, x in zip(prefix_of, seqs)]
            refused = eng.prefix_refused([Pl] * P, [L] * B, prefix_of)
            if refused:
                raise SystemExit(f"L = {L}: the prefixed call refuses these shapes (remainder rows in the prefix); choose another --prefix / completion length")
            med = {}
            for keep_name, keep in (("all", [L + 1] * B), ("one", [1] * B)):
                tg = torch.randint(0, ec.vocab, (sum(keep),), generator=g).to(torch.int32).cuda()
                forms = {"ragged": lambda: eng.forward_logprobs_ragged(cats, tg, keep, temperature=0.7),
                         "prefixed": lambda: eng.forward_logprobs_prefixed(prefixes, seqs, prefix_of, tg, keep, temperature=0.7)}
                ms = {f: [] for f in forms}
                for r in range(a.reps + 1):
                    for f in (list(forms) if r % 2 else list(reversed(forms))):      # alternating order
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        forms[f]()                                    # blocks until the pass has finished
                        if r:
                            ms[f].append((time.perf_counter() - t0) * 1e3)
                for f in forms:
                    med[f, keep_name] = statistics.median(ms[f])
            removed = (G - 1) * Pl / (G * (Pl + L))
            rows.append((L, G, B * (Pl + L), P * Pl + B * L, removed, med))
            print(rows[-1], flush=True)
    lines = [
        "# GRPO's log-prob pass: the visual prefix once per image against once per completion",
        "",
        f"`tools/prefix_scoring_sweep.py` on {a.box or torch.cuda.get_device_name(0)}, commit {commit_id(a.commit)}: StarVector-1B decoder dimensions, {ec.n_layer} layers, "
        f"bf16 random weights, P = {P} images of {Pl} visual rows, G completions of L rows each.  `ragged` = `forward_logprobs_ragged` over the P * G "
        "concatenations (the baseline: the call of the parent commit), `prefixed` = `forward_logprobs_prefixed`; temperature 0.7, no lists.  "
        f"Host clock around the blocking call, 1 warm-up + {a.reps} timed calls per form in alternating order; median, ms.  `all`: L + 1 rows kept per "
        "sequence (every completion token scored); `one`: one row kept per sequence (the layers without the lm_head's share).",
        "",
        "| L | G | rows ragged | rows prefixed | rows removed | ragged all | prefixed all | prefixed / ragged | ragged one | prefixed one | prefixed / ragged |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for L, G, r_rag, r_pre, removed, med in rows:
        lines.append(f"| {L} | {G} | {r_rag} | {r_pre} | {100 * removed:.1f} % | {med['ragged', 'all']:.2f} | {med['prefixed', 'all']:.2f} | "
                     f"{med['prefixed', 'all'] / med['ragged', 'all']:.3f} | {med['ragged', 'one']:.2f} | {med['prefixed', 'one']:.2f} | "
                     f"{med['prefixed', 'one'] / med['ragged', 'one']:.3f} |")
    lines += ["",
              "`all` minus `one` is the lm_head + log-prob share of a call; it is the same work in both forms (the same kept rows), so the saving shows "
              "in full in the `one` columns and diluted by that share in the `all` columns.  The prefixed call also writes no KV page.", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
