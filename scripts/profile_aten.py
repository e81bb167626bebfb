#!/usr/bin/env python3
"""Attribute the remaining aten glue (direct copies / fills / reduces) in
the train step to python-level ops via torch.profiler (rocprofv3 gives
kernel names only). Run on a GPU box; prints the top CPU-op table with
input shapes so the copy sources are identifiable.

--kernels REGEX additionally names, for every launch of a kernel whose name
matches, the op that launched it: op name, input shapes, the enclosing ops
(autograd node, custom Function) and the first dcr_amd source line on the
Python stack; one row per distinct source, launches per step."""
import argparse
import re
import sys
from collections import defaultdict
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch
from torch.profiler import profile, ProfilerActivity

from dcr_amd.train import TrainConfig, Trainer

STEPS = 2


def kernel_sources(prof, pattern):
    rx = re.compile(pattern)
    rows = defaultdict(lambda: [0, 0.0, set()])
    for e in prof.events():
        ks = [k for k in getattr(e, "kernels", []) if rx.search(k.name)]
        if not ks:
            continue
        chain, p = [], e.cpu_parent
        while p is not None and len(chain) < 3:
            chain.append(p.name[:60])
            p = p.cpu_parent
        src = next((f.strip()[:90] for f in (e.stack or []) if "dcr_amd" in f), "")
        key = (e.name[:40], str(e.input_shapes)[:70], " < ".join(chain), src)
        rows[key][0] += len(ks)
        rows[key][1] += sum(k.duration for k in ks)
        rows[key][2].update(k.name[:50] for k in ks)
    print(f"\nlaunches of kernels matching /{pattern}/, by source "
          f"({STEPS} steps profiled)")
    print("| launches/step | us/step | op | input shapes | enclosing ops | source | kernel |")
    print("|---:|---:|---|---|---|---|---|")
    tot_n = tot_us = 0
    for key, (n, us, names) in sorted(rows.items(), key=lambda kv: -kv[1][0]):
        tot_n += n
        tot_us += us
        print(f"| {n / STEPS:.1f} | {us / STEPS:.1f} | {key[0]} | {key[1]} | {key[2]} "
              f"| {key[3]} | {'; '.join(sorted(names))} |")
    print(f"| {tot_n / STEPS:.1f} | {tot_us / STEPS:.1f} | total | | | | |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", nargs="*", default=[],
                    help="kernel-name regexes to attribute to their source ops")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = True
    cfg = TrainConfig(
        model_size="sd21", synthetic_data=True, synthetic_size=64,
        resolution=256, train_batch_size=16, mixed_precision="pure_bf16",
        dataloader_num_workers=0, max_train_steps=10**9, seed=1234,
        learning_rate=5e-6, lr_warmup_steps=0, channels_last=True,
        output_dir="/tmp/prof_aten_out")
    tr = Trainer(cfg, device=torch.device("cuda", 0))
    batch = next(iter(tr.dataloader))
    for _ in range(4):
        tr.train_step(batch)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA],
                 record_shapes=True, with_stack=bool(args.kernels)) as prof:
        for _ in range(STEPS):
            tr.train_step(batch)
        torch.cuda.synchronize()
    print(prof.key_averages(group_by_input_shape=True).table(
        sort_by="self_cuda_time_total", row_limit=45, max_name_column_width=55))
    for pattern in args.kernels:
        kernel_sources(prof, pattern)


if __name__ == "__main__":
    main()
