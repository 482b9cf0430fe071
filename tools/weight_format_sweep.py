#!/usr/bin/env python3
"""Decode step time per decoder weight format (bf16, fp8, mxfp4) -> profiles/mxfp4_weights.md.

    python tools/weight_format_sweep.py [--out profiles/mxfp4_weights.md] [--models 1b,8b] [--batches 1,16,32,64] [--no-col-tiles]

One process, one GPU.  Per model (StarVector-1B / -8B, text2svg shapes: 32 caption ids + <svg-start>, no image encoder, random weights
drawn on the GPU) and batch B: the three engines are built side by side, each runs `generate` of 128 new tokens once (warm-up and graph
capture) and then three timed times, the format order alternating between the repeats; the figure is decode_ms / decode_steps of
`last_timing()` (device events around the decode loop), every repeat listed.  Greedy, EOS disabled, exclusive_device on (one process per GPU,
the deployment bench.py measures).

Beside it, for every decode Linear of the two models (StarVector-8B's c_fc and down projection first) at 16 and 64 rows: the kernel time
of gemm_skinny_mxfp4_kernel per launch for every col_tiles value, through the operators sv_op_linear_skinny_epi_mxfp4 / sv_op_linear_skinny_mxfp4, read from a `rocprofv3 --kernel-trace`
of a child process of this script (--col-tiles-child: a fresh process, the profiler in a run of its own)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMATS = ("bf16", "fp8_e4m3", "mxfp4")
NEW_TOKENS, CAPTION_TOKENS, REPEATS = 128, 32, 3
CT_VALUES, CT_CALLS = (1, 2, 4), 12
# (name, N, K, form): the decode Linears of StarVector-1B and -8B; form = "slabs" (split-K partials), "act" (c_fc: whole K, bias + GELU) or
# "logits" (lm_head: whole K, fp32 rows).  The issue's pair -- 8B c_fc and down projection -- first.
CT_LINEARS = (("8b c_fc", 18432, 4608, "act"), ("8b down", 4608, 18432, "slabs"), ("8b c_attn", 5632, 4608, "slabs"),
              ("8b c_proj", 4608, 4608, "slabs"), ("8b lm_head", 49157, 4608, "logits"),
              ("1b c_fc", 8192, 2048, "act"), ("1b down", 2048, 8192, "slabs"), ("1b c_attn", 2304, 2048, "slabs"),
              ("1b c_proj", 2048, 2048, "slabs"), ("1b lm_head", 49156, 2048, "logits"))
CT_ROWS = (16, 64)


def step_sweep(models, batches, log):
    import torch
    import starvector_amd as sva
    dev = torch.device("cuda", 0)
    rows = []
    for model in models:
        for B in batches:
            engines = {}
            for fmt in FORMATS:
                ec = sva.EngineConfig.starvector_8b(max_batch=B, max_seq_len=16) if model == "8b" else sva.EngineConfig(max_batch=B)
                ec.max_seq_len = CAPTION_TOKENS + 1 + NEW_TOKENS
                ec.weight_dtype = fmt
                ec.exclusive_device = True
                eng = sva.HipEngine(ec, device=0)
                eng.load_random_weights(seed=1234, std=0.02)
                engines[fmt] = eng
            g = torch.Generator().manual_seed(0)
            caps = torch.randint(1, 49152, (B, CAPTION_TOKENS), generator=g)
            prompt = torch.cat([caps, torch.full((B, 1), 49152 + 1, dtype=torch.long)], 1).to(dev)
            pad = 0 if model == "8b" else 49152

            def run(eng):
                emb = eng.embed_tokens(prompt)
                out = eng.generate(emb, max_length=CAPTION_TOKENS + 1 + NEW_TOKENS, eos_token_id=-1, pad_token_id=pad)
                torch.cuda.synchronize()
                tm = eng.last_timing()
                assert tuple(out.shape) == (B, NEW_TOKENS) and tm["decode_steps"] > 0, (out.shape, tm)
                return 1e3 * tm["decode_ms"] / tm["decode_steps"], bool(tm["graph"])

            for fmt in FORMATS:
                run(engines[fmt])                                   # warm-up + graph capture
            times = {fmt: [] for fmt in FORMATS}
            graph = {}
            for rep in range(REPEATS):
                for fmt in (FORMATS if rep % 2 == 0 else FORMATS[::-1]):
                    us, gr = run(engines[fmt])
                    times[fmt].append(us)
                    graph[fmt] = gr
            for fmt in FORMATS:
                rows.append(dict(model=model, B=B, fmt=fmt, us=times[fmt], graph=graph[fmt]))
                log(f"{model} B={B} {fmt}: " + ", ".join(f"{u:.0f}" for u in times[fmt]) + f" us/step (graph {graph[fmt]})")
                engines[fmt].close()
            torch.cuda.empty_cache()
    return rows


def col_tiles_child():
    """The launches the profiler watches, in a fixed order: per Linear, per col_tiles value, 1 + CT_CALLS operator calls at 16 rows."""
    import ctypes as C
    import torch
    from starvector_amd import _lib
    from starvector_amd import engine as E
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = {}
    for name, N, K, form in CT_LINEARS:
        g = torch.Generator(device=dev).manual_seed(N + K)
        W = (torch.randn(N, K, generator=g, device=dev) / K ** 0.5).bfloat16()
        for rows in CT_ROWS:
            x = torch.randn(rows, K, generator=g, device=dev).bfloat16()
            out = (C.c_int32 * 2)()
            E.check(_lib.load().sv_debug_decode_plan(rows, N, K, 2, int(form != "slabs"), cus, out), "sv_debug_decode_plan")
            plan[f"{name} {rows}"] = dict(splitk=int(out[0]), picked=int(out[1]))
            for ct in CT_VALUES:
                for _ in range(1 + CT_CALLS):
                    if form == "slabs":
                        E.op_linear_skinny_mxfp4(x, W, None, splitk=int(out[0]), col_tiles=ct)
                    else:
                        E.op_linear_skinny_epi_mxfp4(x, W, None, act="gelu_tanh" if form == "act" else "none", out_f32=form == "logits", col_tiles=ct)
    torch.cuda.synchronize()
    print("CT_PLAN " + json.dumps(plan))


def col_tiles_probe(log):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--col-tiles-child"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        plan = json.loads([l for l in r.stdout.splitlines() if l.startswith("CT_PLAN ")][-1][8:])
        launches = []
        for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(fn) as f:
                for row in csv.DictReader(f):
                    if "gemm_skinny_mxfp4_kernel" in (row.get("Kernel_Name") or ""):
                        launches.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    launches.sort()
    per = 1 + CT_CALLS
    want = per * len(CT_VALUES) * len(CT_LINEARS) * len(CT_ROWS)
    if len(launches) != want:
        raise RuntimeError(f"{len(launches)} launches of gemm_skinny_mxfp4_kernel in the trace, {want} expected")
    res, i = [], 0
    for name, N, K, form in CT_LINEARS:
        for rows in CT_ROWS:
            pl = plan[f"{name} {rows}"]
            for ct in CT_VALUES:
                d = sorted(x[1] for x in launches[i + 1:i + per])         # the first call of each group is the warm-up
                i += per
                res.append(dict(linear=name, rows=rows, N=N, K=K, form=form, splitk=pl["splitk"], picked=pl["picked"], col_tiles=ct,
                                median_us=d[len(d) // 2] / 1e3, min_us=d[0] / 1e3, max_us=d[-1] / 1e3))
                log(f"{name} rows {rows} N={N} K={K} split-K {pl['splitk']} col_tiles {ct}: median {d[len(d) // 2] / 1e3:.1f} us "
                    f"(min {d[0] / 1e3:.1f}, max {d[-1] / 1e3:.1f}, {len(d)} launches)")
    return res


def box():
    import torch
    p = torch.cuda.get_device_properties(0)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip()
        dirty = bool(subprocess.run(["git", "status", "--porcelain"], capture_output=True, text=True, cwd=ROOT).stdout.strip())
    except OSError:
        commit, dirty = "", False
    return dict(gpu=p.name, cus=p.multi_processor_count, hip=torch.version.hip, torch=torch.__version__,
                commit=(commit + (" + working tree" if dirty else "")) or "not a git checkout (the parent of the commit that adds this file)")


def write_md(path, info, rows, ct):
    med = lambda v: sorted(v)[len(v) // 2]
    L = ["# Decoder weight formats: decode step time (tools/weight_format_sweep.py)", "",
         f"Box: {info['gpu']}, {info['cus']} CUs, HIP {info['hip']}, torch {info['torch']}.  Commit: {info['commit']}.  {time.strftime('%Y-%m-%d')}.", "",
         f"text2svg shapes ({CAPTION_TOKENS} caption ids + <svg-start>), random weights, greedy, EOS disabled, {NEW_TOKENS} new tokens, "
         "exclusive_device on; one process, the three engines side by side, one warm-up call, then three timed calls per format with the "
         "format order alternating.  us per decode step = decode_ms / decode_steps of last_timing(); median (every repeat).", "",
         "| model | rows | bf16 | fp8_e4m3 | mxfp4 | mxfp4 / fp8 | mxfp4 / bf16 |", "|---|---|---|---|---|---|---|"]
    by = {(r["model"], r["B"], r["fmt"]): r["us"] for r in rows}
    for model, B in sorted({(r["model"], r["B"]) for r in rows}):
        c = [by[(model, B, f)] for f in FORMATS]
        cell = lambda v: f"{med(v):.0f} ({', '.join(f'{u:.0f}' for u in v)})"
        L.append(f"| {model} | {B} | {cell(c[0])} | {cell(c[1])} | {cell(c[2])} | {med(c[2]) / med(c[1]):.3f} | {med(c[2]) / med(c[0]):.3f} |")
    L += ["", "bf16 engines run the fused decode launches where they apply (6-launch layer, row update + c_attn, fused MLP); fp8 and mxfp4 run "
          "the 7-launch layer with the separate lm_head launch.", ""]
    if ct:
        L += ["## col_tiles of gemm_skinny_mxfp4_kernel per decode Linear", "",
              f"Kernel time per launch from a rocprofv3 kernel trace of a child process, {CT_CALLS} launches per value after one warm-up, through "
              "sv_op_linear_skinny_mxfp4 (slabs: split-K partials with sv_create's split factor) and sv_op_linear_skinny_epi_mxfp4 (act: whole K, "
              "GELU epilogue; logits: whole K, fp32 rows).  `picked` marks what pick_decode_plan chooses for the shape; `*` the fastest median.", "",
              "| Linear | rows | N | K | form | split-K | col_tiles | median us | min | max | pick_decode_plan |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        best = {}
        for r in ct:
            k = (r["linear"], r["rows"])
            if k not in best or r["median_us"] < best[k]:
                best[k] = r["median_us"]
        for r in ct:
            star = " *" if r["median_us"] == best[(r["linear"], r["rows"])] else ""
            L.append(f"| {r['linear']} | {r['rows']} | {r['N']} | {r['K']} | {r['form']} | {r['splitk']} | {r['col_tiles']} | {r['median_us']:.1f}{star} | "
                     f"{r['min_us']:.1f} | {r['max_us']:.1f} | {'picked' if r['picked'] == r['col_tiles'] else ''} |")
        L.append("")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4_weights.md"))
    ap.add_argument("--models", default="1b,8b")
    ap.add_argument("--batches", default="1,16,32,64")
    ap.add_argument("--no-col-tiles", action="store_true")
    ap.add_argument("--no-steps", action="store_true", help="only the col_tiles table")
    ap.add_argument("--col-tiles-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.col_tiles_child:
        return col_tiles_child()
    import torch
    if not torch.cuda.is_available():
        sys.exit("weight_format_sweep: no GPU -- nothing is measured without one")
    log = lambda s: print("[weight_format_sweep] " + s, flush=True)
    rows = [] if args.no_steps else step_sweep([m for m in args.models.split(",") if m], [int(b) for b in args.batches.split(",") if b], log)
    ct, err = None, None
    if not args.no_col_tiles:
        try:
            ct = col_tiles_probe(log)
        except Exception as e:                        # the step table is written either way; the failure is the exit status
            err = e
    write_md(args.out, box(), rows, ct)
    log(f"wrote {args.out}")
    if err is not None:
        sys.exit(f"weight_format_sweep: the col_tiles probe failed: {err}")


if __name__ == "__main__":
    main()
