#!/usr/bin/env python3
"""Split-product benchmark (split-product retrieval, stype='': aligned chunks
of a flat embedding or aligned patches of a feature map).

Arms, alternated in one process on the same seeded features, every group
L2-normalised:

  composite   the einsum(...).amax formula on the device in fp32, in the
              caller's layout ('ngl,mgl->nmg' on [N, c, D/c] chunks of a flat
              embedding, 'ncp,mcp->nmp' on [N, C, P] patch maps), rows
              chunked so the [chunk, M, G] block stays under --composite-gb
  fused_bf16  dcr_amd.ops.split_product(precision="bf16"), fp32 features in
  fused_high  dcr_amd.ops.split_product(precision="high"), fp32 features in
  kernel_bf16 / kernel_high
              the HIP kernel alone on operands transformed beforehand

Each round times every arm once, device-synchronised; rounds repeat until
every arm has --min-seconds of timed work (at least --min-rounds). Prints
one JSON line per shape: median and min seconds per arm, algorithmic
TFLOP/s = 2*N*M*G*L / median (for the high arms also "mfma_tflops", the
same with the 3x contraction the kernel really runs), peak device memory
of one call of each arm above the resident inputs, and the max abs
difference of each fused arm against the composite.

--sweep adds one JSON line per shape with the kernel alone at forced split
counts (0 = the launcher's rule), alternated the same way, and checks that
every count returns the bits of the rule's result.

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

# name: (N, M, G, L, layout of the composite arm)
SHAPES = {
    "flat_sscd": (4096, 65536, 8, 64, "chunks"),
    "sscd_trunk": (512, 4096, 49, 2048, "patches"),
    "vit_b16": (256, 2048, 196, 768, "patches"),
}
SWEEP = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 49, 64, 98, 196)


def composite(fa, fb, chunk, layout):
    eq = "ngl,mgl->nmg" if layout == "chunks" else "ncp,mcp->nmp"
    sims = []
    for i in range(0, fa.shape[0], chunk):
        sims.append(torch.einsum(eq, fa[i:i + chunk].float(),
                                 fb.float()).amax(dim=2))
    return torch.cat(sims, dim=0)


def timed_rounds(arms, args):
    """Alternate the arms; {name: [seconds]} and the number of rounds."""
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
    return times, rounds


def bench_shape(name, N, M, G, L, layout, args, dev):
    from dcr_amd import ops
    from dcr_amd.ops.functional import split_product_operands

    g = torch.Generator().manual_seed(7)
    a = F.normalize(torch.randn(N, G, L, generator=g), dim=-1).to(dev)
    b = F.normalize(torch.randn(M, G, L, generator=g), dim=-1).to(dev)
    if layout == "chunks":
        fa, fb = a, b
    else:                                  # [N, C, P], the caller's layout
        fa = a.transpose(1, 2).contiguous()
        fb = b.transpose(1, 2).contiguous()
    chunk = max(1, min(N, int(args.composite_gb * 2 ** 30) // (M * G * 4)))
    ab, bb = split_product_operands(a, b, "bf16")
    ah, bh = split_product_operands(a, b, "high")
    kern = ops.ext().split_product

    arms = {
        "composite": lambda: composite(fa, fb, chunk, layout),
        "fused_bf16": lambda: ops.split_product(a, b, precision="bf16"),
        "fused_high": lambda: ops.split_product(a, b, precision="high"),
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
    n0 = ops.dispatch_counts["split_product"]
    times, rounds = timed_rounds(arms, args)
    assert ops.dispatch_counts["split_product"] == n0 + 2 * rounds, \
        "the fused arms did not run the HIP kernel"

    flop = 2.0 * N * M * G * L
    res = {"metric": "split_product", "shape": name, "N": N, "M": M, "G": G,
           "L": L, "rounds": rounds, "composite_chunk": chunk,
           "inputs_gb": round((a.numel() + b.numel()) * 4 / 2 ** 30, 3),
           "output_gb": round(N * M * 4 / 2 ** 30, 3), "arms": {}}
    for k in arms:
        med = statistics.median(times[k])
        r = {"sec_median": round(med, 6), "sec_min": round(min(times[k]), 6),
             "algo_tflops": round(flop / med / 1e12, 1),
             "peak_mem_gb": round(peak[k] / 2 ** 30, 3)}
        if k.endswith("high"):
            r["mfma_tflops"] = round(3 * flop / med / 1e12, 1)
        if k != "composite":
            r["max_abs_diff_vs_composite"] = float(
                (outs[k] - outs["composite"]).abs().max())
        res["arms"][k] = r
    print(json.dumps(res), flush=True)

    if not args.sweep:
        return
    for prec, (x, y) in (("bf16", (ab, bb)), ("high", (ah, bh))):
        counts = [s for s in SWEEP if s <= G]
        want = kern(x, y).view(torch.int32)
        for s in counts:
            assert torch.equal(kern(x, y, s).view(torch.int32), want), \
                f"splits={s} changed the result"
        sw = {str(s): (lambda s=s: kern(x, y, s)) for s in counts}
        times, rounds = timed_rounds(sw, args)
        print(json.dumps({
            "metric": "split_product_sweep", "shape": name, "operands": prec,
            "tiles": ((N + 127) // 128) * ((M + 127) // 128), "G": G,
            "rounds": rounds,
            "ms_median_by_splits": {
                k: round(statistics.median(t) * 1e3, 4)
                for k, t in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES),
                    choices=list(SHAPES))
    ap.add_argument("--composite-gb", type=float, default=8.0,
                    help="cap of the composite arm's [chunk, M, G] block")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--min-rounds", type=int, default=3)
    ap.add_argument("--max-rounds", type=int, default=200)
    ap.add_argument("--sweep", action="store_true",
                    help="also time the kernel alone at forced split counts")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_splitsim.py needs a GPU: no timing is taken on a CPU")
    from dcr_amd import ops
    ops.require_hip("split_product")
    dev = torch.device("cuda", 0)
    for name in args.shapes:
        bench_shape(name, *SHAPES[name], args, dev)


if __name__ == "__main__":
    main()
