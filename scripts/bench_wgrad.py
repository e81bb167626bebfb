#!/usr/bin/env python3
"""linear_wgrad (gemm.hip) against the library's weight gradient, per linear
shape of the SD-2.1 UNet at bs16 256px.

Column 1: native dw alone against `dy.t() @ x` alone (no cast, no sum on the
library side). Column 2, the biased case: native dw+db against the library
product plus the native column sum (`colsum`) that the default path runs for
the bias gradient today.

Operands rotate through a pool larger than the 256 MB last-level cache, so
no call finds its inputs resident: cache-resident per-call timings did not
reproduce in-model times (profiles/r06_prof_after.md). Each figure is the
mean over `--reps` windows; min and max over the windows are printed so a
difference can be set against the scatter. The byte floor is the operand
and result bytes at the rate adamw_bf16 reaches in the same run.

`--sweep` times forced (tile, split) pairs per shape: the data behind the
launcher's rule. The whole-model profile, not this script, decides what is
dispatched."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from dcr_amd import ops

BF16 = torch.bfloat16
POOL_BYTES = 320 << 20

SHAPES = [  # (M, N, K, what)
    (16384, 320, 320, "L0 q/k/v/out/proj_in/proj_out"),
    (16384, 2560, 320, "L0 GEGLU proj"),
    (16384, 320, 1280, "L0 ff.net.2"),
    (4096, 640, 640, "L1 q/k/v/out/proj_in/proj_out"),
    (4096, 5120, 640, "L1 GEGLU proj"),
    (4096, 640, 2560, "L1 ff.net.2"),
    (1024, 1280, 1280, "L2 q/k/v/out/proj_in/proj_out"),
    (1024, 10240, 1280, "L2 GEGLU proj"),
    (1024, 1280, 5120, "L2 ff.net.2"),
    (1232, 320, 1024, "L0 context k/v"),
    (1232, 640, 1024, "L1 context k/v"),
    (1232, 1280, 1024, "L2 context k/v"),
]


def make_pool(M, N, K):
    pair = (M * N + M * K) * 2
    n = max(2, POOL_BYTES // pair + 1)
    return [(torch.randn(M, N, device="cuda").to(BF16),
             torch.randn(M, K, device="cuda").to(BF16)) for _ in range(n)]


def timeit(fn, pool, reps):
    """fn(dy, x) over the pool; (mean, min, max) us per call over `reps`
    windows of at least 64 calls, whole passes through the pool (device time
    between events)"""
    passes = max(1, -(-64 // len(pool)))
    for dy, x in pool[:3]:
        fn(dy, x)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(passes):
            for dy, x in pool:
                fn(dy, x)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / (passes * len(pool)) * 1e3)
    return sum(out) / len(out), min(out), max(out)


def adamw_rate(m):
    n = 64 * 1024 * 1024
    p = torch.randn(n, device="cuda").to(BF16)
    g = torch.randn(n, device="cuda").to(BF16)
    master = p.float()
    mm, vv = torch.zeros_like(master), torch.zeros_like(master)
    for _ in range(3):
        m.adamw_step_bf16(p, g, master, mm, vv, 1e-5, 0.9, 0.999, 1e-8, 1e-2, 1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        m.adamw_step_bf16(p, g, master, mm, vv, 1e-5, 0.9, 0.999, 1e-8, 1e-2, 1)
    e1.record()
    torch.cuda.synchronize()
    rate = n * 30 / (e0.elapsed_time(e1) / 10 * 1e-3)
    print(f"adamw_bf16: {rate / 1e12:.2f} TB/s (the byte-floor rate below)")
    return rate


def fmt(t):
    return f"{t[0]:7.1f} [{t[1]:6.1f},{t[2]:6.1f}]"


def compare(m, rate, reps, shapes):
    print("us per call: mean [min,max] over windows\n"
          f"{'shape':<22} {'floor':>6} | {'native dw':>22} {'lib dy.t()@x':>22} "
          f"{'x':>5} | {'native dw+db':>22} {'lib + colsum':>22} {'x':>5}")
    for M, N, K, what in shapes:
        pool = make_pool(M, N, K)
        floor = ((M * N + M * K + N * K) * 2) / rate * 1e6
        nat = timeit(lambda dy, x: m.linear_wgrad(dy, x, False), pool, reps)
        lib = timeit(lambda dy, x: dy.t() @ x, pool, reps)
        natb = timeit(lambda dy, x: m.linear_wgrad(dy, x, True), pool, reps)
        libb = timeit(lambda dy, x: (dy.t() @ x, m.colsum(dy)), pool, reps)
        print(f"{M}x{N}x{K:<10} {floor:6.1f} | {fmt(nat)} {fmt(lib)} "
              f"{lib[0] / nat[0]:5.2f} | {fmt(natb)} {fmt(libb)} "
              f"{libb[0] / natb[0]:5.2f}   {what}", flush=True)
        del pool


def sweep(m, reps, shapes):
    print("\n== sweep: native dw+db, us per call (mean) by tile and split; "
          "slab MB in brackets")
    for M, N, K, what in shapes:
        pool = make_pool(M, N, K)
        nchunks = (M + 127) // 128
        print(f"{M}x{N}x{K}  {what}")
        for tile in (64, 128):
            tiles = -(-N // tile) * -(-K // 64)
            cells = []
            for split in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64):
                if split > nchunks or tiles * split > 8192:
                    continue
                t = timeit(lambda dy, x: m.linear_wgrad(dy, x, True, split, tile),
                           pool, reps)
                cells.append(f"s{split}:{t[0]:.1f}({split * N * K * 4 / 1e6:.1f})")
            print(f"  tile {tile:>3} ({tiles:>4} tiles): " + "  ".join(cells), flush=True)
        del pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--shapes", default="",
                    help="comma list of indices into SHAPES (default: all)")
    args = ap.parse_args()
    m = ops.ext()
    assert m is not None, "build the extension first"
    assert torch.cuda.is_available(), "needs the GPU"
    shapes = [SHAPES[int(i)] for i in args.shapes.split(",")] if args.shapes else SHAPES
    rate = adamw_rate(m)
    compare(m, rate, args.reps, shapes)
    if args.sweep:
        sweep(m, args.reps, shapes)


if __name__ == "__main__":
    main()
