"""What the prompt-pass row budget (sv_set_prefill_chunk) costs and saves; the numbers of profiles/chunked_prefill.md.

  --ttft     StarVector-1B dimensions, full depth, random weights: the prompt pass of 32 x 259 rows (BASELINE config 2's) under every --budgets value,
             median of --iters passes timed with events around sv_prefill
  --memory   StarVector-8B dimensions (--layers decoder layers): device memory taken by the FIRST prompt pass of 16 x 2048 rows (torch.cuda.mem_get_info
             around it: the prompt-pass workspaces and the gathered K | V rows), one engine per --budgets value
  --gather   one extension of 256 rows behind a 2048-token context at 1B and 8B dimensions, both pool formats: run under
             `rocprofv3 --kernel-trace --stats` and read kv_gather_kernel's time; prints the bytes one launch moves
"""
import argparse
import dataclasses
import statistics

import torch

import starvector_amd as sva


def _engine(model, layers, max_batch, max_seq_len, kv="bf16", seed=4321):
    if model == "8b":
        ec = sva.EngineConfig.starvector_8b(max_batch=max_batch, max_seq_len=max_seq_len)
        ec = dataclasses.replace(ec, vit_layers=1, kv_dtype=kv, **({"n_layer": layers} if layers else {}))
    else:
        ec = sva.EngineConfig(vit_layers=1, max_batch=max_batch, max_seq_len=max_seq_len, kv_dtype=kv, **({"n_layer": layers} if layers else {}))
    eng = sva.HipEngine(ec)
    eng.load_random_weights(seed=seed)
    return ec, eng


def _rows(n, hidden, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, hidden, generator=g) * 0.5).to(torch.bfloat16).cuda()


def ttft(args):
    ec, eng = _engine("1b", args.layers, 32, 512)
    x = _rows(32 * 259, ec.hidden).view(32, 259, ec.hidden)
    ref = None
    for budget in args.budgets:
        eng.set_prefill_chunk(budget)
        for _ in range(2):
            lg = eng.prefill(x)
        ref = lg.clone() if ref is None else ref
        ms = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.prefill(x)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        passes = eng.prompt_passes()
        eng.prefill(x)
        print(f"[ttft] 32 x 259 rows, budget {budget}: median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms over {args.iters} passes; "
              f"{eng.prompt_passes() - passes} pass(es) per call; logits equal to the first budget's: {torch.equal(lg, ref)}")
    eng.close()


def memory(args):
    for budget in args.budgets:
        ec, eng = _engine("8b", args.layers or 4, 16, 2112)
        eng.set_prefill_chunk(budget)
        x = _rows(16 * 2048, ec.hidden).view(16, 2048, ec.hidden)
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        eng.prefill(x)
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
        print(f"[memory] 8B dimensions, 16 x 2048 rows, budget {budget}: the first prompt pass took {(free0 - free1) / 2**20:.0f} MiB of device memory")
        eng.close()
        del eng, x
        torch.cuda.empty_cache()


def gather(args):
    ctx, own = 2048, 256
    for model in ("1b", "8b"):
        for kv in ("bf16", "fp8_e4m3"):
            ec, eng = _engine(model, args.layers or 4, 4, ctx + own + 64, kv)
            n_kv = ec.n_kv_head if ec.arch == "v2" else 1
            dh = ec.hidden // ec.n_head
            x = _rows(4 * (ctx + own), ec.hidden)
            for _ in range(args.iters):      # every round re-opens: the same 2048-token context behind every second extension
                eng.prefill_open([ctx + own] * 4)
                eng.prefill_extend(x[:4 * ctx], [ctx] * 4, [ctx + own] * 4)
                eng.prefill_extend(x[4 * ctx:], [own] * 4, [ctx + own] * 4)
            torch.cuda.synchronize()
            read = 4 * ctx * n_kv * (2 * dh * (1 if kv != "bf16" else 2) + (2 if kv != "bf16" else 0))
            written = 4 * ctx * n_kv * 2 * dh * 2
            print(f"[gather] {model} {kv}: one kv_gather_kernel launch of the second extension (4 sequences x {ctx} tokens, {n_kv} KV head(s), head_dim {dh}) "
                  f"reads {read} B of pages and writes {written} B of rows = {(read + written) / 1e6:.3f} MB; {ec.n_layer} launches per extension")
            eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ttft", action="store_true")
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--budgets", type=int, nargs="+", default=[0, 2048, 4096])
    ap.add_argument("--layers", type=int, default=0, help="decoder layers (0: the model's own for --ttft, 4 otherwise)")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if a.ttft:
        ttft(a)
    if a.memory:
        memory(a)
    if a.gather:
        gather(a)
