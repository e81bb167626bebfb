#!/usr/bin/env python3
"""The optimizer tail alone at the real arena: gather -> norm/clip -> AdamW.

Parameter shapes come from tests/golden/sd21_state_dict_manifest.json (the
SD-2.1 UNet, 865,910,724 elements, bf16 + fp32 master); the gradients are
seeded synthetic tensors of their own, as autograd hands them over. Two arms,
alternated in one process:

  old  DCR_FUSED_GRAD_TAIL=0: _foreach_copy_, vector_norm + host compare
       (+ mul_ when clipping), adamw_bf16_kernel<false>
  new  grad_gather_kernel with fused sum of squares, sumsq_finalize_kernel,
       adamw_bf16_kernel<true> reading the device record

Every section is timed on the wall clock between device synchronisations, so
host work (the Python loop over parameters, the pointer table) counts; `tail`
is the three sections back to back with one synchronisation at the end.
--grad-scale 1e-5 keeps the norm below max_norm, 1e-3 clips on every call
(as the benchmark's randomly initialised model does). The sweep times
grad_gather alone (device events) over the virtual-block size CH and the
grid."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch

from dcr_amd import ops
from dcr_amd.ops import adamw as adamw_mod
from dcr_amd.ops.adamw import FusedAdamW

MAX_NORM = 1.0


def unet_shapes():
    man = json.loads((ROOT / "tests/golden/sd21_state_dict_manifest.json").read_text())
    shapes = dict(man["unet"])
    last = shapes.pop("conv_out.bias")      # registered last in the model
    return list(shapes.values()) + [last]


def build(dtype, scale):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    params, grads = [], []
    for s in unet_shapes():
        params.append(torch.nn.Parameter(
            (0.02 * torch.randn(*s, device=dev, generator=gen)).to(dtype)))
        grads.append((scale * torch.randn(*s, device=dev, generator=gen)).to(dtype))
    return FusedAdamW(params), params, grads


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def one_call(opt, params, grads, m, new, split):
    """One optimizer tail; returns section times (split) or the whole."""
    os.environ["DCR_FUSED_GRAD_TAIL"] = "1" if new else "0"
    for p, g in zip(params, grads):
        p.grad = g

    def adamw_new():
        rec = opt._norm_rec
        opt.step_count += 1
        m.adamw_step_bf16_clip(opt.flat_param, opt.flat_grad, opt.master,
                               opt.exp_avg, opt.exp_avg_sq, opt.lr, opt.beta1,
                               opt.beta2, opt.eps, opt.weight_decay,
                               opt.step_count, rec)
        opt.arena_written()

    if new:
        secs = [opt.gather_grads, lambda: opt._norm_record(m, MAX_NORM), adamw_new]
    else:
        secs = [opt.gather_grads, lambda: opt.clip_grad_norm_(MAX_NORM), opt.step]
    if split:
        out = [sync_ms(f) for f in secs]
    else:
        out = [sync_ms(lambda: [f() for f in secs])]
    opt.zero_grad()
    return out


def sweep(opt, params, grads, m, calls):
    n = opt.numel
    es = opt.flat_grad.element_size()
    views = opt._grad_views
    print("\nsweep: grad_gather + fused sum of squares, device time "
          f"(median of {calls}), {2 * n * es / 1e9:.2f} GB per call")
    print("| CH | grid | virtual blocks | ms | TB/s |")
    print("|---:|---:|---:|---:|---:|")
    for ch in (8192, 16384, 32768, 65536):
        nvb = sum((p.numel() + ch - 1) // ch for p in params)
        partials = torch.empty(nvb, device=opt.flat_grad.device)
        for grid in (1024, 2048, 4096, 8192):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * calls)]
            for i in range(calls + 2):
                if i >= 2:
                    ev[2 * (i - 2)].record()
                assert m.grad_gather(opt.flat_grad, views, grads, partials, ch, grid) == []
                if i >= 2:
                    ev[2 * (i - 2) + 1].record()
            torch.cuda.synchronize()
            ms = statistics.median(ev[2 * i].elapsed_time(ev[2 * i + 1])
                                   for i in range(calls))
            print(f"| {ch} | {grid} | {nvb} | {ms:.3f} | {2 * n * es / ms / 1e9:.2f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grad-scale", type=float, nargs="*", default=[1e-5, 1e-3])
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: no timing without one"
    m = ops.require_hip("grad_tail")
    dtype = torch.bfloat16
    for scale in args.grad_scale:
        opt, params, grads = build(dtype, scale)
        n, es = opt.numel, opt.flat_grad.element_size()
        gb = {"gather": 2 * n * es / 1e9, "norm": n * es / 1e9,
              "adamw": (2 * es + 8 + 16) * n / 1e9}
        for new in (False, True):
            for _ in range(args.warmup):
                one_call(opt, params, grads, m, new, True)
        sec = {False: [], True: []}
        tail = {False: [], True: []}
        for _ in range(args.rounds):
            for new in (False, True):
                sec[new].append(one_call(opt, params, grads, m, new, True))
                tail[new].append(one_call(opt, params, grads, m, new, False)[0])
        norm = float(opt._norm_rec[1])
        # bytes per arm: the old norm reads the arena (and mul_ reads and
        # writes it when clipping); the new norm reads only the partials;
        # the new AdamW also writes the arena back when clipping
        clips = norm > MAX_NORM
        nb = {False: gb["norm"] * (3 if clips else 1),
              True: 4 * opt._nvb_all / 1e9}
        ab = {False: gb["adamw"],
              True: gb["adamw"] + (n * es / 1e9 if clips else 0.0)}
        print(f"\nn={n} bf16+master grad-scale {scale:g}: norm {norm:.4g} "
              f"({'clips' if norm > MAX_NORM else 'no clip'}), "
              f"CH={adamw_mod.GATHER_CH}, median of {args.rounds} alternated rounds")
        print("| arm | gather ms | norm ms | adamw ms (min..max) | tail ms (min..max) "
              "| gather GB | norm GB | adamw GB | gather TB/s | adamw TB/s |")
        print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
        for new in (False, True):
            g_, n_, a_ = (statistics.median(r[i] for r in sec[new]) for i in range(3))
            t_ = tail[new]
            al = [r[2] for r in sec[new]]
            print(f"| {'new' if new else 'old'} | {g_:.3f} | {n_:.3f} "
                  f"| {a_:.3f} ({min(al):.3f}..{max(al):.3f}) "
                  f"| {statistics.median(t_):.3f} ({min(t_):.3f}..{max(t_):.3f}) "
                  f"| {gb['gather']:.2f} | {nb[new]:.2f} | {ab[new]:.2f} "
                  f"| {gb['gather'] / g_:.2f} | {ab[new] / a_:.2f} |")
        if not args.no_sweep and scale == args.grad_scale[0]:
            sweep(opt, params, grads, m, calls=10)
        del opt, params, grads
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
