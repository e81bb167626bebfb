#!/usr/bin/env python3
"""A/B the fp32-state AdamW kernels (elementwise.hip) against the FP8-state
kernels (adamw8.hip) at the SD-2.1 UNet arena size and at 8 M elements.
Same process, alternating rounds, each kernel on its own arenas and state;
prints the median ms per call and the effective GB/s over the bytes each
kernel really moves."""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from dcr_amd import ops

HYP = (5e-6, 0.9, 0.999, 1e-8, 1e-2)  # lr, betas, eps, wd


def unet_numel() -> int:
    """Trainable elements of the SD-2.1 UNet = FusedAdamW's arena size."""
    from dcr_amd.models import UNet2DConditionModel, UNetConfig
    with torch.device("meta"):
        unet = UNet2DConditionModel(UNetConfig.sd21())
    return sum(p.numel() for p in unet.parameters())


def bytes_moved(kind: str, bf16: bool, n: int) -> float:
    """HBM bytes of one call. fp32 params: grad in, param in+out; bf16:
    grad in, param out, master in+out. Plus both moments in+out."""
    nb = (n + 255) // 256
    arenas = (2 + 2 + 8) * n if bf16 else (4 + 8) * n
    if kind == "fp32":
        return arenas + 16 * n
    return arenas + 4 * nb * 256 + 16 * nb


def make(n: int, bf16: bool):
    """Arenas and state of ONE kernel (each timed kernel gets its own, so
    none sees state or a step count left behind by another)."""
    dev = torch.device("cuda", 0)
    dt = torch.bfloat16 if bf16 else torch.float32
    nb = (n + 255) // 256
    gen = torch.Generator(device=dev).manual_seed(0)
    t = {
        "p": torch.randn(n, device=dev, generator=gen).to(dt),
        "g": (1e-3 * torch.randn(n, device=dev, generator=gen)).to(dt),
        "nb": nb,
    }
    if bf16:
        t["master"] = t["p"].float()
    return t


def callers(m, n, bf16):
    dev = torch.device("cuda", 0)
    a, b = make(n, bf16), make(n, bf16)
    a["m"] = torch.zeros(n, device=dev)
    a["v"] = torch.zeros(n, device=dev)
    for k in ("mq", "rq"):
        b[k] = torch.zeros(b["nb"] * 256, dtype=torch.uint8, device=dev)
    for k in ("mabs", "rabs"):
        b[k] = torch.zeros(b["nb"], device=dev)
    sa, sb = [0], [0]

    def fp32():
        sa[0] += 1
        if bf16:
            m.adamw_step_bf16(a["p"], a["g"], a["master"], a["m"], a["v"], *HYP, sa[0])
        else:
            m.adamw_step(a["p"], a["g"], a["m"], a["v"], *HYP, sa[0])

    def fp8():
        sb[0] += 1
        if bf16:
            m.adamw8_step_bf16(b["p"], b["g"], b["master"], b["mq"], b["mabs"],
                               b["rq"], b["rabs"], *HYP, sb[0])
        else:
            m.adamw8_step(b["p"], b["g"], b["mq"], b["mabs"], b["rq"],
                          b["rabs"], *HYP, sb[0])

    return {"fp32": fp32, "fp8": fp8}


def time_calls(fn, calls):
    """Device time of each of `calls` back-to-back launches (events)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for i in range(calls):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(calls)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="timed calls per round")
    ap.add_argument("--rounds", type=int, default=3,
                    help="alternating rounds per kernel (>= 20 timed calls in all)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=None)
    args = ap.parse_args()
    assert args.calls * args.rounds >= 20, "median of at least 20 timed calls"
    assert torch.cuda.is_available(), "needs the GPU: no timing without one"
    m = ops.require_hip("adamw8")
    sizes = args.sizes or [unet_numel(), 8 * 1024 * 1024]
    for n in sizes:
        for bf16 in (True, False):
            fns = callers(m, n, bf16)
            for fn in fns.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    ms[k] += time_calls(fn, args.calls)
            base = statistics.median(ms["fp32"])
            tag = "bf16+master" if bf16 else "fp32 params"
            for k in fns:
                med = statistics.median(ms[k])
                gb = bytes_moved("fp32" if k == "fp32" else "fp8", bf16, n) / 1e9
                print(f"n={n} {tag:11s} {k:4s}: median {med:7.3f} ms "
                      f"(min {min(ms[k]):.3f}, max {max(ms[k]):.3f}; "
                      f"{len(ms[k])} calls)  {gb:6.2f} GB  "
                      f"{gb / med * 1e3:6.0f} GB/s  {base / med:.2f}x vs fp32 state")
            del fns
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
