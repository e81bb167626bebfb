#!/usr/bin/env python3
"""A/B the SD-1.x (head_dim 40/80/160) attention fwd+bwd on an MI355X.

One process, variants alternated, every shape warmed up, each timing a
host clock around a window of >= 0.5 s of work that ends in a device
synchronise, each row repeated 3 times to show the spread:

* gen        ops.attention with grad -> attn_fwd_gen_lse + attn_bwd_gen
* composite  the same call under DCR_ATTN_GEN_BWD=0 (fp32 GEMM + softmax
             + GEMM, autograd keeps the [B,H,Lq,Lk] matrices) -- the
             yardstick: what ran before the gen backward existed
* sdpa       F.scaled_dot_product_attention (informational)

Peak memory is the allocator's high-water mark over one fwd+bwd, above
what was allocated before it (inputs and upstream grad excluded).
Outputs and grads of gen and composite are compared at the timed sizes.

--train-step adds an SD-1.4 256 px bs-16 pure-bf16 Trainer.train_step
pair (gate on / gate off, alternated) on a resident synthetic batch.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch
import torch.nn.functional as F

from dcr_amd import ops

B, H = 16, 8
SHAPES = [  # (D, Lq, Lk): SD-1.4 bs-16 256 px training shapes + 512 px level 0
    (40, 1024, 1024), (40, 1024, 77),
    (80, 256, 256), (80, 256, 77),
    (160, 64, 64), (160, 64, 77),
    (160, 16, 16), (160, 16, 77),
    (40, 4096, 4096),
]
WINDOW_S = 0.5
REPEATS = 3


def _sync_time(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def _iters_for_window(fn):
    """warm up, then size the window to >= WINDOW_S from a short probe"""
    for _ in range(3):
        fn()
    t = _sync_time(fn, 3)
    return max(3, int(WINDOW_S / t) + 1)


def _peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() /
            b.float().abs().max().clamp_min(1e-12)).item()


def bench_shapes():
    print(f"# attention fwd+bwd, bf16, B={B} H={H}, layout blhd; ms per "
          f"fwd+bwd over a >= {WINDOW_S} s synchronised window; "
          f"{REPEATS} alternated repeats")
    print("# D Lq Lk | variant | ms (repeats) | peak MiB above inputs")
    for (D, Lq, Lk) in SHAPES:
        torch.manual_seed(D + Lq + Lk)
        mk = lambda L: torch.randn(B, L, H, D, device="cuda").to(torch.bfloat16)
        q, k, v, g = mk(Lq), mk(Lk), mk(Lk), mk(Lq)
        qp, kp, vp, gp = (t.permute(0, 2, 1, 3).contiguous() for t in (q, k, v, g))
        scale = D ** -0.5

        def run_ops(gate, keep=None):
            os.environ["DCR_ATTN_GEN_BWD"] = gate
            leaves = [t.detach().requires_grad_(True) for t in (q, k, v)]
            out = ops.attention(*leaves, layout="blhd")
            out.backward(g)
            if keep is not None:
                keep[:] = [out.detach()] + [t.grad for t in leaves]

        def run_sdpa():
            leaves = [t.detach().requires_grad_(True) for t in (qp, kp, vp)]
            out = F.scaled_dot_product_attention(*leaves, scale=scale)
            out.backward(gp)

        variants = [("gen", lambda: run_ops("1")),
                    ("composite", lambda: run_ops("0")),
                    ("sdpa", run_sdpa)]

        r_gen, r_cmp = [], []
        run_ops("1", r_gen)
        run_ops("0", r_cmp)
        errs = " ".join(f"{n}={_rel(a, b):.2e}" for n, a, b in
                        zip(("o", "dQ", "dK", "dV"), r_gen, r_cmp))
        del r_gen, r_cmp

        iters = {name: _iters_for_window(fn) for name, fn in variants}
        times = {name: [] for name, _ in variants}
        for _ in range(REPEATS):
            for name, fn in variants:
                times[name].append(_sync_time(fn, iters[name]) * 1e3)
        peaks = {name: _peak_mib(fn) for name, fn in variants[:2]}

        for name, _ in variants:
            ts = " ".join(f"{t:.3f}" for t in times[name])
            pk = f"{peaks[name]:.1f}" if name in peaks else "-"
            print(f"D{D} Lq{Lq} Lk{Lk} | {name:9s} | {ts} | {pk}")
        best = {n: min(t) for n, t in times.items()}
        print(f"D{D} Lq{Lq} Lk{Lk} | composite/gen {best['composite'] / best['gen']:.2f}x "
              f"sdpa/gen {best['sdpa'] / best['gen']:.2f}x (best of {REPEATS}) | "
              f"gen vs composite max-abs/max-abs: {errs}")
        sys.stdout.flush()
    os.environ.pop("DCR_ATTN_GEN_BWD", None)


def bench_train_step(steps):
    from dcr_amd.train import TrainConfig, Trainer
    cfg = TrainConfig(model_size="sd14", synthetic_data=True, synthetic_size=16,
                      resolution=256, train_batch_size=16,
                      mixed_precision="pure_bf16", channels_last=True,
                      dataloader_num_workers=0, max_train_steps=10 ** 6, seed=0,
                      output_dir="/tmp/dcr_bench_attn_gen_out")
    tr = Trainer(cfg, device=torch.device("cuda", 0))
    # as bench.py: skip MIOpen's exhaustive find (the convs are the same in
    # both variants; the search would only add minutes before the windows)
    torch.backends.cudnn.benchmark = False
    batch = next(iter(tr.dataloader))
    batch = {k_: (v_.cuda() if torch.is_tensor(v_) else v_)
             for k_, v_ in batch.items()}

    def step():
        tr.train_step(batch)

    print(f"# SD-1.4 256 px bs16 pure_bf16 channels_last Trainer.train_step, "
          f"resident synthetic batch; ms per step over {steps}-step "
          f"synchronised windows; {REPEATS} alternated repeats")
    gates = [("gen (DCR_ATTN_GEN_BWD unset)", "1"), ("composite (=0)", "0")]
    for _, gate in gates:                       # warm up both paths
        os.environ["DCR_ATTN_GEN_BWD"] = gate
        for _ in range(3):
            step()
    times = {n: [] for n, _ in gates}
    peaks = {}
    counts = {}
    for _ in range(REPEATS):
        for name, gate in gates:
            os.environ["DCR_ATTN_GEN_BWD"] = gate
            c0 = dict(ops.dispatch_counts)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            times[name].append(_sync_time(step, steps) * 1e3)
            peaks[name] = torch.cuda.max_memory_allocated() / 2 ** 20
            counts[name] = {k_: ops.dispatch_counts[k_] - c0.get(k_, 0)
                            for k_ in ("attention_gen", "attention_gen_bwd",
                                       "attention_math")}
    for name, _ in gates:
        ts = " ".join(f"{t:.2f}" for t in times[name])
        print(f"train_step | {name} | ms/step {ts} | peak allocated "
              f"{peaks[name]:.0f} MiB | dispatches per window {counts[name]}")
    a, b = (min(times[n]) for n, _ in gates)
    print(f"train_step | composite/gen {b / a:.3f}x (best of {REPEATS}); "
          f"imgs/s gen {16e3 / a:.1f} composite {16e3 / b:.1f}")
    os.environ.pop("DCR_ATTN_GEN_BWD", None)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--train-step", action="store_true",
                    help="also time the SD-1.4 train step, gate on/off")
    ap.add_argument("--train-steps", type=int, default=8,
                    help="steps per timed train-step window")
    ap.add_argument("--no-shapes", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: no CPU fallback"
    print(f"# device {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if not args.no_shapes:
        bench_shapes()
    if args.train_step:
        bench_train_step(args.train_steps)


if __name__ == "__main__":
    main()
