#!/usr/bin/env python3
"""Patch max-similarity benchmark (split-product retrieval, stype='cross').

Arms, alternated in one process on the same seeded unit-norm features:

  composite   the einsum("ncp,mcq->nmpq").amax((2,3)) formula on the device
              in fp32, rows chunked so the [chunk, M, P, Q] block stays
              under --composite-gb
  fused_bf16  dcr_amd.ops.patch_maxsim(precision="bf16"), fp32 features in
  fused_high  dcr_amd.ops.patch_maxsim(precision="high"), fp32 features in
  kernel_bf16 / kernel_high
              the HIP kernel alone on operands transformed beforehand

Each round times every arm once, device-synchronised; rounds repeat until
every arm has --min-seconds of timed work (at least --min-rounds). Prints
one JSON line per shape: median and min seconds per arm, algorithmic
TFLOP/s = 2*N*P*M*Q*C / median (for the high arms also "mfma_tflops", the
same with the 3x contraction the kernel really runs), peak device memory
of one call of each arm above the resident inputs, and the max abs
difference of each fused arm against the composite.

Needs a GPU: exits with an error instead of timing anything on a CPU.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch
import torch.nn.functional as F

# (name, N, M, P, Q, C)
SHAPES = {
    "sscd_trunk": (512, 4096, 49, 49, 2048),
    "vit_b16": (256, 2048, 196, 196, 768),
}


def composite(fa, fb, chunk):
    """The composite formula of einsum_in_chunks(stype='cross'), [N, C, P] in."""
    sims = []
    for i in range(0, fa.shape[0], chunk):
        a = fa[i:i + chunk].float()
        sims.append(torch.einsum("ncp,mcq->nmpq", a, fb.float()).amax(dim=(2, 3)))
    return torch.cat(sims, dim=0)


def bench_shape(name, N, M, P, Q, C, args, dev):
    from dcr_amd import ops
    from dcr_amd.ops.functional import maxsim_operands

    g = torch.Generator().manual_seed(7)
    a = F.normalize(torch.randn(N, P, C, generator=g), dim=-1).to(dev)
    b = F.normalize(torch.randn(M, Q, C, generator=g), dim=-1).to(dev)
    fa = a.transpose(1, 2).contiguous()          # [N, C, P], the caller's layout
    fb = b.transpose(1, 2).contiguous()
    chunk = max(1, min(N, int(args.composite_gb * 2 ** 30) // (M * P * Q * 4)))
    ab, bb = maxsim_operands(a, b, "bf16")
    ah, bh = maxsim_operands(a, b, "high")
    kern = ops.ext().patch_maxsim

    arms = {
        "composite": lambda: composite(fa, fb, chunk),
        "fused_bf16": lambda: ops.patch_maxsim(a, b, precision="bf16"),
        "fused_high": lambda: ops.patch_maxsim(a, b, precision="high"),
        "kernel_bf16": lambda: kern(ab, bb),
        "kernel_high": lambda: kern(ah, bh),
    }

    # warm-up, outputs and peak memory: one call of each arm
    outs, peak = {}, {}
    for k, fn in arms.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
        outs[k] = out.float().cpu()
        del out
    n0 = ops.dispatch_counts["patch_maxsim"]

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
    assert ops.dispatch_counts["patch_maxsim"] == n0 + 2 * rounds, \
        "the fused arms did not run the HIP kernel"

    flop = 2.0 * N * P * M * Q * C
    res = {"metric": "patch_maxsim", "shape": name, "N": N, "M": M, "P": P,
           "Q": Q, "C": C, "rounds": rounds, "composite_chunk": chunk,
           "inputs_gb": round((a.numel() + b.numel()) * 4 / 2 ** 30, 3),
           "arms": {}}
    for k in arms:
        med = statistics.median(times[k])
        r = {"sec_median": round(med, 5), "sec_min": round(min(times[k]), 5),
             "algo_tflops": round(flop / med / 1e12, 1),
             "peak_mem_gb": round(peak[k] / 2 ** 30, 3)}
        if k.endswith("high"):
            r["mfma_tflops"] = round(3 * flop / med / 1e12, 1)
        if k != "composite":
            r["max_abs_diff_vs_composite"] = float(
                (outs[k] - outs["composite"]).abs().max())
        res["arms"][k] = r
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES),
                    choices=list(SHAPES))
    ap.add_argument("--composite-gb", type=float, default=8.0,
                    help="cap of the composite arm's [chunk, M, P, Q] block")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--min-rounds", type=int, default=3)
    ap.add_argument("--max-rounds", type=int, default=200)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_maxsim.py needs a GPU: no timing is taken on a CPU")
    from dcr_amd import ops
    ops.require_hip("patch_maxsim")
    dev = torch.device("cuda", 0)
    for name in args.shapes:
        bench_shape(name, *SHAPES[name], args, dev)


if __name__ == "__main__":
    main()
