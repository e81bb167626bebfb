#!/usr/bin/env python3
"""A/B the VAE mid-block attention (one 512-d head, forward) on an MI355X.

One process, candidates alternated, every shape warmed up, each timing a
host clock around a window of >= 0.5 s of work that ends in a device
synchronise, each row repeated 3 times to show the spread:

* native     ops.attention under no_grad -> attn_fwd_d512
* composite  the same call under DCR_ATTN_D512=0 (fp32 GEMM + softmax +
             GEMM on a materialised [B,H,Lq,Lk] score matrix) -- the
             yardstick: what ran before the kernel existed
* sdpa       bf16 F.scaled_dot_product_attention (informational)

Shapes: B16 L1024 (the frozen-VAE encode of the 256 px bs-16 training
step) and B4 L4096 (a 512 px decode batch). FLOPs = 4*B*Lq*Lk*512. Peak
memory is the allocator's high-water mark over one call, above what was
allocated before it (inputs excluded).

--decode adds a 512 px SD VAE decode (bs 1, bf16, channels_last), gate on
and off alternated, with the dispatch counts of one decode.
--train-step adds the SD-2.1 256 px bs-16 pure-bf16 Trainer.train_step
(gate on / gate off, alternated) on a resident synthetic batch.
--decode-only GATE runs just three such decodes with DCR_ATTN_D512=GATE,
for a kernel trace of their own.
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

D, H = 512, 1
SHAPES = [(16, 1024), (4, 4096)]    # (B, L): training encode, 512 px decode
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


def _spread(ts):
    return (max(ts) - min(ts)) / min(ts) * 100.0


@torch.no_grad()
def bench_shapes():
    print(f"# attention forward, bf16, one head of {D}, layout blhd, no_grad; "
          f"ms per call over a >= {WINDOW_S} s synchronised window; "
          f"{REPEATS} alternated repeats")
    print("# B L | candidate | ms (repeats) | spread % | TF/s (best) | "
          "peak MiB above inputs")
    for (B, L) in SHAPES:
        torch.manual_seed(B + L)
        mk = lambda: torch.randn(B, L, H, D, device="cuda").to(torch.bfloat16)
        q, k, v = mk(), mk(), mk()
        qp, kp, vp = (t.permute(0, 2, 1, 3).contiguous() for t in (q, k, v))
        scale = D ** -0.5
        flop = 4.0 * B * L * L * D

        def run_ops(gate):
            os.environ["DCR_ATTN_D512"] = gate
            return ops.attention(q, k, v, layout="blhd")

        def run_sdpa():
            return F.scaled_dot_product_attention(qp, kp, vp, scale=scale)

        cands = [("native", lambda: run_ops("1")),
                 ("composite", lambda: run_ops("0")),
                 ("sdpa", run_sdpa)]

        c0 = dict(ops.dispatch_counts)
        o_nat, o_cmp = run_ops("1"), run_ops("0")
        assert ops.dispatch_counts["attention_d512"] == c0.get("attention_d512", 0) + 1
        assert ops.dispatch_counts["attention_math"] == c0.get("attention_math", 0) + 1
        err = _rel(o_nat, o_cmp)
        del o_nat, o_cmp

        iters = {name: _iters_for_window(fn) for name, fn in cands}
        times = {name: [] for name, _ in cands}
        for _ in range(REPEATS):
            for name, fn in cands:
                times[name].append(_sync_time(fn, iters[name]) * 1e3)
        peaks = {name: _peak_mib(fn) for name, fn in cands}

        for name, _ in cands:
            ts = times[name]
            print(f"B{B} L{L} | {name:9s} | "
                  f"{' '.join(f'{t:.4f}' for t in ts)} | {_spread(ts):.1f} | "
                  f"{flop / (min(ts) * 1e-3) / 1e12:.1f} | {peaks[name]:.1f}")
        best = {n: min(t) for n, t in times.items()}
        print(f"B{B} L{L} | {flop / 1e9:.1f} GFLOP | composite/native "
              f"{best['composite'] / best['native']:.2f}x sdpa/native "
              f"{best['sdpa'] / best['native']:.2f}x (best of {REPEATS}) | "
              f"native vs composite max-abs/max-abs: {err:.2e}")
        sys.stdout.flush()
    os.environ.pop("DCR_ATTN_D512", None)


def _sd_vae_and_latent():
    from dcr_amd.models import AutoencoderKL, VAEConfig
    torch.manual_seed(0)
    vae = AutoencoderKL(VAEConfig.sd()).cuda().to(torch.bfloat16) \
        .to(memory_format=torch.channels_last).eval()
    z = torch.randn(1, 4, 64, 64, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    return vae, z


@torch.no_grad()
def bench_decode():
    vae, z = _sd_vae_and_latent()
    decode = lambda: vae.decode(z).sample
    print(f"# SD VAE decode, 512 px, bs 1, bf16 channels_last (L=4096); ms per "
          f"decode over a >= {WINDOW_S} s synchronised window; "
          f"{REPEATS} alternated repeats")
    gates = [("native (DCR_ATTN_D512 unset)", "1"), ("composite (=0)", "0")]
    iters, counts, peaks, times = {}, {}, {}, {n: [] for n, _ in gates}
    for name, gate in gates:
        os.environ["DCR_ATTN_D512"] = gate
        iters[name] = _iters_for_window(decode)
        c0 = dict(ops.dispatch_counts)
        decode()
        counts[name] = {k_: ops.dispatch_counts[k_] - c0.get(k_, 0)
                        for k_ in ("attention_d512", "attention_math")}
    for _ in range(REPEATS):
        for name, gate in gates:
            os.environ["DCR_ATTN_D512"] = gate
            times[name].append(_sync_time(decode, iters[name]) * 1e3)
    for name, gate in gates:
        os.environ["DCR_ATTN_D512"] = gate
        peaks[name] = _peak_mib(decode)
    for name, _ in gates:
        ts = times[name]
        print(f"decode512 | {name} | ms {' '.join(f'{t:.3f}' for t in ts)} | "
              f"spread {_spread(ts):.1f} % | peak {peaks[name]:.0f} MiB above "
              f"weights | dispatches per decode {counts[name]}")
    a, b = (min(times[n]) for n, _ in gates)
    print(f"decode512 | composite/native {b / a:.3f}x (best of {REPEATS})")
    os.environ.pop("DCR_ATTN_D512", None)


def bench_train_step(steps):
    from dcr_amd.train import TrainConfig, Trainer
    cfg = TrainConfig(model_size="sd21", synthetic_data=True, synthetic_size=16,
                      resolution=256, train_batch_size=16,
                      mixed_precision="pure_bf16", channels_last=True,
                      dataloader_num_workers=0, max_train_steps=10 ** 6, seed=0,
                      output_dir="/tmp/dcr_bench_attn_d512_out")
    tr = Trainer(cfg, device=torch.device("cuda", 0))
    # as bench.py: skip MIOpen's exhaustive find (same convs on both sides)
    torch.backends.cudnn.benchmark = False
    batch = next(iter(tr.dataloader))
    batch = {k_: (v_.cuda() if torch.is_tensor(v_) else v_)
             for k_, v_ in batch.items()}
    step = lambda: tr.train_step(batch)

    print(f"# SD-2.1 256 px bs16 pure_bf16 channels_last Trainer.train_step "
          f"(frozen-VAE encode inside), resident synthetic batch; ms per step "
          f"over {steps}-step synchronised windows; {REPEATS} alternated repeats")
    gates = [("native (DCR_ATTN_D512 unset)", "1"), ("composite (=0)", "0")]
    for _, gate in gates:                       # warm up both paths
        os.environ["DCR_ATTN_D512"] = gate
        for _ in range(3):
            step()
    times, counts = {n: [] for n, _ in gates}, {}
    for _ in range(REPEATS):
        for name, gate in gates:
            os.environ["DCR_ATTN_D512"] = gate
            c0 = dict(ops.dispatch_counts)
            times[name].append(_sync_time(step, steps) * 1e3)
            counts[name] = {k_: ops.dispatch_counts[k_] - c0.get(k_, 0)
                            for k_ in ("attention_d512", "attention_math")}
    for name, _ in gates:
        ts = times[name]
        print(f"train_step | {name} | ms/step {' '.join(f'{t:.2f}' for t in ts)} "
              f"| spread {_spread(ts):.1f} % | dispatches per window {counts[name]}")
    a, b = (min(times[n]) for n, _ in gates)
    print(f"train_step | composite/native {b / a:.4f}x (best of {REPEATS})")
    os.environ.pop("DCR_ATTN_D512", None)


@torch.no_grad()
def decode_only(gate):
    os.environ["DCR_ATTN_D512"] = gate
    vae, z = _sd_vae_and_latent()
    for _ in range(3):
        vae.decode(z).sample
    torch.cuda.synchronize()
    print(f"decode512 x3 with DCR_ATTN_D512={gate}: dispatch counts "
          f"{dict(ops.dispatch_counts)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--decode", action="store_true",
                    help="also time a 512 px SD VAE decode, gate on/off")
    ap.add_argument("--train-step", action="store_true",
                    help="also time the SD-2.1 256 px train step, gate on/off")
    ap.add_argument("--train-steps", type=int, default=8,
                    help="steps per timed train-step window")
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--decode-only", choices=["0", "1"], default=None,
                    help="only run three 512 px decodes with this gate value")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: no CPU fallback"
    # the conv solver is the same on both sides; skip MIOpen's exhaustive find
    torch.backends.cudnn.benchmark = False
    if args.decode_only is not None:
        decode_only(args.decode_only)
        return
    print(f"# device {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if not args.no_shapes:
        bench_shapes()
    if args.decode:
        bench_decode()
    if args.train_step:
        bench_train_step(args.train_steps)


if __name__ == "__main__":
    main()
