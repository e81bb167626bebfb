#!/usr/bin/env python3
"""Per-kernel A/B for LayerNorm backward, NHWC GroupNorm backward and the
bias-gradient column sums at the SD-2.1 bs16 256px shapes.

Each line prints time, bytes moved (from the shape), achieved TB/s and the
time against its byte bound at the rate adamw_bf16 reaches in the same run.
`--parent DIR` loads a second build of the extension (a checkout of the
parent commit, built) and adds the ratio to it plus a bit-comparison of dx;
the column sums are compared with the aten reductions they replace."""
import argparse
import importlib.util
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from dcr_amd import ops

BF16 = torch.bfloat16


def timeit(fn, n=50):
    """mean us per call, device time between two events"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def load_parent(root):
    so = Path(root) / "dcr_amd" / "ops" / "_dcr_hip.so"
    spec = importlib.util.spec_from_file_location("_dcr_hip", str(so))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def line(name, us, nbytes, rate, extra=""):
    bound = nbytes / rate * 1e6
    print(f"{name:<44} {us:8.1f} us  {nbytes / 1e6:8.2f} MB  "
          f"{nbytes / us / 1e6:5.2f} TB/s  {us / bound:5.2f}x bound {extra}")


def adamw_rate(m):
    n = 64 * 1024 * 1024
    p = torch.randn(n, device="cuda").to(BF16)
    g = torch.randn(n, device="cuda").to(BF16)
    master = p.float()
    mm, vv = torch.zeros_like(master), torch.zeros_like(master)
    us = timeit(lambda: m.adamw_step_bf16(p, g, master, mm, vv, 1e-5, 0.9,
                                          0.999, 1e-8, 1e-2, 1), n=10)
    nbytes = n * 30   # p r/w 4, g 2, master/m/v r/w 8 each
    rate = nbytes / (us * 1e-6)
    print(f"adamw_bf16 {n} elems: {us:.0f} us, {rate / 1e12:.2f} TB/s (the byte-bound rate below)")
    return rate


def bench_ln(m, parent, rate):
    print("\n== LayerNorm backward (bf16 x, bf16 w): 3 * M * N * 2 bytes")
    for M, N in [(16384, 320), (4096, 640), (1024, 1280)]:
        x = torch.randn(M, N, device="cuda").to(BF16)
        dy = torch.randn(M, N, device="cuda").to(BF16)
        w = torch.randn(N, device="cuda").to(BF16)
        b = torch.randn(N, device="cuda").to(BF16)
        _, mean, rstd = m.layernorm_fwd(x, w, b, 1e-5)
        nbytes = 3 * M * N * 2
        us = timeit(lambda: m.layernorm_bwd(dy, x, w, mean, rstd))
        extra = ""
        if parent is not None:
            pus = timeit(lambda: parent.layernorm_bwd(dy, x, w, mean, rstd))
            same = torch.equal(m.layernorm_bwd(dy, x, w, mean, rstd)[0],
                               parent.layernorm_bwd(dy, x, w, mean, rstd)[0])
            extra = f"parent {pus:.1f} us -> {pus / us:.2f}x, dx bits equal: {same}"
        line(f"ln_bwd {M}x{N}", us, nbytes, rate, extra)
        for blocks in (64, 128, 256, 512, 1024, 2048):
            if blocks * 8 > M:
                continue
            bus = timeit(lambda: m.layernorm_bwd(dy, x, w, mean, rstd, blocks))
            print(f"    blocks={blocks:<5} (slab {blocks * 2 * N * 4 / 1e6:.2f} MB) {bus:8.1f} us")


GN_SHAPES = [  # (C, H) of every GroupNorm input in the SD-2.1 UNet at bs16 256px
    (320, 32), (320, 16), (640, 16), (640, 8), (1280, 8), (1280, 4),
    (2560, 4), (2560, 8), (1920, 8), (1920, 16), (1280, 16), (960, 16),
    (960, 32), (640, 32)]


def bench_gn(m, parent, rate):
    print("\n== NHWC GroupNorm+SiLU backward (bf16, N=16, G=32): 5 * N*HW*C * 2 bytes")
    cl = torch.channels_last
    for C, H in GN_SHAPES:
        x = torch.randn(16, C, H, H, device="cuda").to(BF16).contiguous(memory_format=cl)
        dy = torch.randn(16, C, H, H, device="cuda").to(BF16).contiguous(memory_format=cl)
        w = torch.randn(C, device="cuda").to(BF16)
        b = torch.randn(C, device="cuda").to(BF16)
        _, mean, rstd = m.groupnorm_silu_nhwc_fwd(x, w, b, 32, 1e-5, True)
        nbytes = 5 * x.numel() * 2
        us = timeit(lambda: m.groupnorm_silu_nhwc_bwd(dy, x, w, b, mean, rstd, 32, True))
        extra = ""
        if parent is not None:
            pus = timeit(lambda: parent.groupnorm_silu_nhwc_bwd(dy, x, w, b, mean, rstd, 32, True))
            a = m.groupnorm_silu_nhwc_bwd(dy, x, w, b, mean, rstd, 32, True)[0]
            p1 = parent.groupnorm_silu_nhwc_bwd(dy, x, w, b, mean, rstd, 32, True)[0]
            p2 = parent.groupnorm_silu_nhwc_bwd(dy, x, w, b, mean, rstd, 32, True)[0]
            extra = (f"parent {pus:.1f} us -> {pus / us:.2f}x, dx bits equal: "
                     f"{torch.equal(a, p1)} (parent vs parent: {torch.equal(p1, p2)})")
        line(f"gn_nhwc_bwd C{C} {H}x{H}", us, nbytes, rate, extra)


def bench_colsum(m, rate):
    print("\n== colsum vs dy.sum(0) (bf16): rows * C * 2 bytes")
    for rows, C in [(16384, 320), (16384, 1280), (16384, 2560), (4096, 640),
                    (4096, 2560), (4096, 5120), (1024, 1280), (1024, 5120),
                    (1024, 10240), (256, 1280), (1232, 1024), (64, 1280), (16, 1280)]:
        dy = torch.randn(rows, C, device="cuda").to(BF16)
        us = timeit(lambda: m.colsum(dy))
        aus = timeit(lambda: dy.sum(0))
        line(f"colsum {rows}x{C}", us, rows * C * 2, rate,
             f"aten {aus:.1f} us -> {aus / us:.2f}x")
    print("\n== colsum_grouped vs dy.sum((2,3)) + convolution_backward's bias sum")
    cl = torch.channels_last
    for C, H in [(320, 32), (640, 16), (1280, 8), (1280, 4), (640, 32), (320, 16)]:
        dy = torch.randn(16, C, H, H, device="cuda").to(BF16).contiguous(memory_format=cl)
        dy3 = dy.permute(0, 2, 3, 1).reshape(16, H * H, C)
        us = timeit(lambda: m.colsum_grouped(dy3))
        aus = timeit(lambda: (dy.sum(dim=(2, 3)), dy.sum(dim=(0, 2, 3))))
        line(f"colsum_grouped 16x{H}x{H}x{C}", us, dy.numel() * 2, rate,
             f"aten (2 sums) {aus:.1f} us -> {aus / us:.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None,
                    help="root of a built checkout of the parent commit")
    args = ap.parse_args()
    m = ops.ext()
    assert m is not None, "build the extension first"
    parent = load_parent(args.parent) if args.parent else None
    rate = adamw_rate(m)
    bench_ln(m, parent, rate)
    bench_gn(m, parent, rate)
    bench_colsum(m, rate)


if __name__ == "__main__":
    main()
