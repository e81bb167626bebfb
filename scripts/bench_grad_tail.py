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
grid.

--arms picks what runs (default: all):

  tail32  the two arms above, fp32 moments
  tail8   the same two arms with FP8 moments (state_bits=8): old is
          DCR_FUSED_GRAD_TAIL=0 (vector_norm + host compare, mul_ when
          clipping, adamw8_kernel<bf16, false>), new is the native tail with
          adamw8_kernel<bf16, true>
  accum   one non-sync micro-step's gradient hand-over into an arena that
          already holds a gradient: old `_foreach_add_` (switch 0), new the
          add-mode grad_gather_kernel launch; gather_grads() end to end

For tail8 and accum a verdict line says whether the new median is below the
old median by more than the old arm's own min..max spread in this run."""
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


def build(dtype, scale, state_bits=32):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    params, grads = [], []
    for s in unet_shapes():
        params.append(torch.nn.Parameter(
            (0.02 * torch.randn(*s, device=dev, generator=gen)).to(dtype)))
        grads.append((scale * torch.randn(*s, device=dev, generator=gen)).to(dtype))
    return FusedAdamW(params, state_bits=state_bits), params, grads


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
        if opt.state_bits == 8:
            m.adamw8_step_bf16_clip(opt.flat_param, opt.flat_grad, opt.master,
                                    opt.exp_avg_q, opt.exp_avg_absmax,
                                    opt.exp_avg_sq_q, opt.exp_avg_sq_absmax,
                                    opt.lr, opt.beta1, opt.beta2, opt.eps,
                                    opt.weight_decay, opt.step_count, rec)
        else:
            m.adamw_step_bf16_clip(opt.flat_param, opt.flat_grad, opt.master,
                                   opt.exp_avg, opt.exp_avg_sq, opt.lr,
                                   opt.beta1, opt.beta2, opt.eps,
                                   opt.weight_decay, opt.step_count, rec)
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


def verdict(what, old, new):
    """The condition of the comparison: new median below old median by more
    than the old arm's own min..max spread."""
    mo, mn = statistics.median(old), statistics.median(new)
    spread = max(old) - min(old)
    print(f"{what}: old median {mo:.3f} ms (spread {spread:.3f}), new median "
          f"{mn:.3f} ms, gain {mo - mn:.3f} ms: "
          f"{'MET' if mo - mn > spread else 'NOT MET'}")


def accum_arm(args, dtype):
    """A non-sync micro-step's hand-over: every parameter already gathered
    once this cycle, so gather_grads() adds."""
    opt, params, grads = build(dtype, 1e-3)
    n, es = opt.numel, opt.flat_grad.element_size()

    def hand_over(new):
        os.environ["DCR_FUSED_GRAD_TAIL"] = "1" if new else "0"
        for p, g in zip(params, grads):
            p.grad = g
        return sync_ms(opt.gather_grads)

    hand_over(True)                     # first gather of the cycle: the copy
    assert len(opt._gathered) == len(params)
    for new in (False, True):
        for _ in range(args.warmup):
            hand_over(new)
    c0 = dict(ops.dispatch_counts)
    ms = {False: [], True: []}
    for _ in range(args.rounds):
        for new in (False, True):
            ms[new].append(hand_over(new))
    assert ops.dispatch_counts["grad_gather_add"] - c0.get("grad_gather_add", 0) \
        == args.rounds
    assert ops.dispatch_counts["grad_gather_fallback"] == c0.get("grad_gather_fallback", 0)
    gbytes = 3 * n * es / 1e9           # read gradient, read and write arena
    print(f"\naccumulation hand-over, n={n} bf16, {gbytes:.2f} GB per call, "
          f"median of {args.rounds} alternated rounds")
    print("| arm | gather_grads ms (min..max) | TB/s |")
    print("|---|---:|---:|")
    for new in (False, True):
        t_ = ms[new]
        md = statistics.median(t_)
        print(f"| {'new: add-mode launch' if new else 'old: _foreach_add_'} "
              f"| {md:.3f} ({min(t_):.3f}..{max(t_):.3f}) | {gbytes / md:.2f} |")
    verdict("accum hand-over", ms[False], ms[True])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grad-scale", type=float, nargs="*", default=[1e-5, 1e-3])
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--arms", nargs="*", default=["tail32", "tail8", "accum"],
                    choices=["tail32", "tail8", "accum"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: no timing without one"
    m = ops.require_hip("grad_tail")
    dtype = torch.bfloat16
    tails = [(b, sc) for b in (32, 8) if f"tail{b}" in args.arms
             for sc in args.grad_scale]
    for bits, scale in tails:
        opt, params, grads = build(dtype, scale, bits)
        n, es = opt.numel, opt.flat_grad.element_size()
        # AdamW bytes per element: grad read, param write, master read and
        # write, and the moments: 2 x fp32 read and write, or 2 x (one code
        # byte + 4 B of absmax per 256) read and write
        state = 16 if bits == 32 else 4 + 16 / 256
        gb = {"gather": 2 * n * es / 1e9, "norm": n * es / 1e9,
              "adamw": (2 * es + 8 + state) * n / 1e9}
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
        print(f"\nn={n} bf16+master, {bits}-bit state, grad-scale {scale:g}: norm {norm:.4g} "
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
        if bits == 8:
            verdict(f"8-bit tail, {'clips' if clips else 'no clip'}",
                    tail[False], tail[True])
        if not args.no_sweep and (bits, scale) == tails[0] and bits == 32:
            sweep(opt, params, grads, m, calls=10)
        del opt, params, grads
        torch.cuda.empty_cache()
    if "accum" in args.arms:
        accum_arm(args, dtype)


if __name__ == "__main__":
    main()
