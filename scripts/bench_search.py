#!/usr/bin/env python3
"""Embedding-search benchmark (BASELINE config 5 shape): synthetic
SSCD-like index, chunked GEMM kNN + per-shard top-k.

Single process = one shard. Under torchrun (one rank per GPU) each rank
holds index_size vectors and the [k,2] candidate all-gather merges ranks
(dcr_amd.search.distributed_knn) — 8 GPUs => 8x index at the same wall
time plus one latency-bound gather.

Prints one JSON line: queries*index dot-products/sec (GEMM-bound).

--arms (single GPU) instead alternates three arms in one process on the same
seeded unit-norm data, for every --queries-list entry:

  library  sharded_topk with DCR_FUSED_SEARCH=0: bf16 GEMM + topk + re-rank
  fused    sharded_topk with the fused candidate pass (ops.topk_sim) + re-rank
  kernel   the HIP top-k kernel alone on bf16 operands converted beforehand,
           m = k + 4 as sharded_topk asks for

Each round times every arm once, device-synchronised; rounds repeat until
every arm has --min-seconds of timed work (at least --min-rounds). Prints one
JSON line per shape: median and min seconds per arm, algorithmic TFLOP/s =
2*Q*N*D / median, peak device memory of one call above the resident inputs,
and the share of rows where the fused arm returns the library arm's indices.
--sweep adds the kernel alone at forced stripe counts (0 = the launcher's
rule), alternated the same way. --arms needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import time

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch


def _unit(n, d, seed, device):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g).to(device)
    return torch.nn.functional.normalize(x, dim=-1)


def _alternate(arms, args):
    """Rounds of every arm once, synchronised; {name: [seconds]}."""
    times = {k: [] for k in arms}
    rounds = 0
    while rounds < args.min_rounds or \
            min(sum(t) for t in times.values()) < args.min_seconds:
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
        rounds += 1
        if rounds >= args.max_rounds:
            break
    return times


def bench_arms(queries, args, shard, device):
    from dcr_amd import ops
    from dcr_amd.search import sharded_topk

    query = _unit(queries, args.dim, 7, device)
    m = args.k + 4
    qb, xb = query.bfloat16(), shard.bfloat16()
    kern = ops.ext().topk_sim

    def with_env(flag):
        def run():
            os.environ["DCR_FUSED_SEARCH"] = flag
            return sharded_topk(query, shard, k=args.k, chunk=args.chunk)
        return run

    arms = {"library": with_env("0"), "fused": with_env("1"),
            "kernel": lambda: kern(qb, xb, m)}
    outs, peak = {}, {}
    for k, fn in arms.items():           # warm-up, outputs, peak memory
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
        outs[k] = out[1].cpu()
        del out
    n0 = ops.dispatch_counts["topk_sim"]
    times = _alternate(arms, args)
    rounds = len(times["fused"])
    chunks = -(-shard.shape[0] // args.chunk)
    assert ops.dispatch_counts["topk_sim"] == n0 + rounds * chunks, \
        "the fused arm did not run the HIP kernel"

    flop = 2.0 * queries * shard.shape[0] * args.dim
    res = {"metric": "search_arms", "queries": queries,
           "index_size": shard.shape[0], "dim": args.dim, "k": args.k,
           "chunk": args.chunk, "rounds": rounds,
           "inputs_gb": round((query.numel() + shard.numel()) * 4 / 2 ** 30, 3),
           "fused_rows_equal_library": round(
               (outs["fused"] == outs["library"]).all(dim=1).float().mean().item(), 4),
           "arms": {}}
    for k in arms:
        med = statistics.median(times[k])
        res["arms"][k] = {"sec_median": round(med, 5),
                          "sec_min": round(min(times[k]), 5),
                          "algo_tflops": round(flop / med / 1e12, 1),
                          "peak_mem_gb": round(peak[k] / 2 ** 30, 3)}
    print(json.dumps(res), flush=True)

    if args.sweep:
        sweep = {f"stripes_{s}": (lambda s=s: kern(qb, xb, m, s))
                 for s in args.sweep_stripes}
        for fn in sweep.values():
            fn()
        st = _alternate(sweep, args)
        print(json.dumps({
            "metric": "search_stripe_sweep", "queries": queries,
            "index_size": shard.shape[0], "dim": args.dim, "m": m,
            "rounds": len(next(iter(st.values()))),
            "sec_median": {k: round(statistics.median(v), 5) for k, v in st.items()},
            "sec_min": {k: round(min(v), 5) for k, v in st.items()}}), flush=True)


def main_arms(args):
    if not torch.cuda.is_available():
        sys.exit("bench_search.py --arms needs a GPU: no timing is taken on a CPU")
    from dcr_amd import ops
    ops.require_hip("topk_sim")
    device = torch.device("cuda", 0)
    shard = _unit(args.index_size, args.dim, 8, device)
    for queries in args.queries_list:
        bench_arms(queries, args, shard, device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", action="store_true",
                    help="alternate library / fused / kernel arms (one GPU)")
    ap.add_argument("--sweep", action="store_true",
                    help="with --arms: the kernel alone at forced stripe counts")
    ap.add_argument("--queries-list", type=int, nargs="*",
                    default=[10_000, 1_000])
    ap.add_argument("--sweep-stripes", type=int, nargs="*",
                    default=[0, 1, 2, 4, 6, 8, 12, 16, 24, 32, 64])
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--min-rounds", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=200)
    ap.add_argument("--index-size", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--bf16", action="store_true",
                    help="bf16 GEMM + fp32 re-rank (sharded_topk "
                         "compute_dtype) — expect ~2x the fp32 rate")
    args = ap.parse_args()
    if args.arms:
        return main_arms(args)

    from dcr_amd.parallel import dist as dist_utils
    from dcr_amd.search import distributed_knn

    rank, world, local = dist_utils.init_distributed_mode(gate_print=False)
    use_cuda = torch.cuda.is_available()
    device = torch.device("cuda", local) if use_cuda else torch.device("cpu")

    g = torch.Generator().manual_seed(7 + rank)
    shard = torch.randn(args.index_size, args.dim, generator=g).to(device)
    shard = torch.nn.functional.normalize(shard, dim=-1)
    gq = torch.Generator().manual_seed(7)
    query = torch.randn(args.queries, args.dim, generator=gq).to(device)
    query = torch.nn.functional.normalize(query, dim=-1)

    cd = torch.bfloat16 if args.bf16 else None
    v, i = distributed_knn(query, shard, k=args.k, chunk=args.chunk,
                           compute_dtype=cd)  # warmup
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.repeat):
        v, i = distributed_knn(query, shard, k=args.k, chunk=args.chunk,
                               compute_dtype=cd)
    if use_cuda:
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.repeat

    if rank == 0:
        dots = args.queries * args.index_size * world
        print(json.dumps({
            "metric": "knn_dotproducts_per_sec",
            "value": round(dots / dt, 1),
            "tflops": round(2 * dots * args.dim / dt / 1e12, 2),
            "index_size": args.index_size * world,
            "queries": args.queries,
            "dim": args.dim,
            "k": args.k,
            "sec_per_search": round(dt, 4),
            "n_gpus": world,
            "dtype": "bf16_rerank" if args.bf16 else "fp32",
        }))


if __name__ == "__main__":
    main()
