#!/usr/bin/env python3
"""Flagship benchmark: SD-2.1 256px finetune step (imgs/sec), BASELINE.json.

Measures the reference's canonical train config
(/root/reference/README.md:27-35: SD-2.1, 256px, bs16/GPU, bf16) on
random-init weights + synthetic data (no network), full train step:
VAE encode -> add_noise -> text encode -> UNet fwd -> MSE -> backward
(bucketed RCCL all-reduce for N>1) -> grad clip -> fused AdamW.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W]
                       [--dump-outputs DIR] [--full]
For N>1 the driver launches this under torch.distributed.run with one
rank per GPU (RANK/LOCAL_RANK/WORLD_SIZE read from env).

Rank 0 prints ONE JSON line with the whole-job aggregate imgs/sec.

A plain run sets up, warms up, times the K steps and prints the result
line; nothing else. --dump-outputs DIR additionally writes what the last
timed step computed (see dump_outputs) so two builds can be compared
output for output. --full is where measurements beyond the headline
figure belong; none exist yet, and the headline path is the same with
and without it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import torch

# --dump-outputs: at most this many elements per sampled array (4 MiB of
# float32 each, far under the 64 MB cap for the whole dump)
DUMP_SAMPLE = 1 << 20
DUMP_SEED = 1234


def dump_outputs(out_dir, trainer, loss) -> None:
    """Write what the last timed train step computed as float32 .npy files.

    loss.npy          the value train_step() returned to its caller
    grad_sample.npy   the UNet gradient as that step's optimizer left it
                      (clipped in place by the host-scalar AdamW; the
                      device-state AdamW fuses the clip and leaves it raw)
    param_sample.npy  the UNet weights after that step's AdamW update
                      (fp32 master copy where the run keeps one)

    The two flat arrays hold ~865M elements each for SD-2.1, so a fixed
    seeded sample of DUMP_SAMPLE positions is stored (everything, when the
    model is smaller than that). Same arguments -> same positions.
    """
    import numpy as np

    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    opt = trainer.optimizer
    idx = None
    if opt.numel > DUMP_SAMPLE:
        g = torch.Generator().manual_seed(DUMP_SEED)
        idx = torch.randint(0, opt.numel, (DUMP_SAMPLE,), generator=g)
        idx = idx.sort().values.to(opt.flat_param.device)

    def save(name, t):
        np.save(out / f"{name}.npy",
                t.detach().to(device="cpu", dtype=torch.float32).numpy())

    def sample(flat):
        return flat if idx is None else flat.index_select(0, idx)

    save("loss", loss.reshape(1))
    save("grad_sample", sample(opt.flat_grad))
    save("param_sample",
         sample(opt.master if opt.master is not None else opt.flat_param))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--model", type=str, default="sd21", choices=["sd21", "tiny"])
    # defaults = the measured-fastest configuration on MI355X
    # (pure bf16 params + fp32-master AdamW; NHWC convs): see BASELINE.md
    ap.add_argument("--precision", type=str, default="pure_bf16",
                    choices=["bf16", "pure_bf16", "no"])
    ap.add_argument("--channels-last", dest="channels_last", action="store_true",
                    default=True)
    ap.add_argument("--no-channels-last", dest="channels_last",
                    action="store_false")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one "
                         "computed as DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="also run whatever the benchmark measures beyond "
                         "the headline figure; off by default (nothing "
                         "sits behind it yet: every run so far does only "
                         "what the headline needs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    from dcr_amd.parallel import dist as dist_utils
    from dcr_amd.train import TrainConfig, Trainer

    rank, world, local = dist_utils.init_distributed_mode(gate_print=False)
    if world == 1 and args.gpus > 1:
        print("warning: --gpus > 1 but not launched under torchrun; running 1 rank",
              file=sys.stderr)
    n_gpus = world if world > 1 else 1

    use_cuda = torch.cuda.is_available()
    # local % device_count: lets a world-2 smoke run share one leased GPU
    # (RCCL multi-rank-per-device) without a special path
    device = torch.device("cuda", local % max(torch.cuda.device_count(), 1)) \
        if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)

    cfg = TrainConfig(
        model_size=args.model,
        synthetic_data=True,
        synthetic_size=args.batch_size * 4,
        resolution=args.resolution,
        train_batch_size=args.batch_size,
        mixed_precision=args.precision if use_cuda else "no",
        dataloader_num_workers=0,
        max_train_steps=10**9,
        seed=1234,
        class_prompt="instancelevel_blip",
        duplication="nodup",
        output_dir="/tmp/dcr_bench_out",
        channels_last=args.channels_last,
    )
    trainer = Trainer(cfg, device=device)
    trainer.unet.train()
    # The trainer switches on MIOpen's exhaustive find, which benchmarks
    # every solver for every conv shape at the first step: 20 s of a run
    # with warm kernel caches, 80 s with cold ones, against ~1 s of timed
    # steps. A plain run skips the search: MIOpen then takes each solver
    # from the user's find database, which __graft_entry__.build() fills
    # on a GPU host. DCR_CONV_BENCHMARK=1 searches here as before, and so
    # does the graph-replayed run, which is left exactly as it was.
    want_graph = use_cuda and n_gpus == 1 \
        and os.environ.get("DCR_HIPGRAPH", "0") == "1"
    if use_cuda and not want_graph \
            and os.environ.get("DCR_CONV_BENCHMARK") != "1":
        torch.backends.cudnn.benchmark = False

    # fixed synthetic batch of the training shape, resident on device
    g = torch.Generator().manual_seed(1234 + rank)
    batch = {
        "pixel_values": (torch.rand(args.batch_size, 3, args.resolution,
                                    args.resolution, generator=g) * 2 - 1).to(device),
        "input_ids": trainer.tokenizer(
            [f"An image of sample {i} rank {rank}" for i in range(args.batch_size)],
            truncation=True, padding="max_length",
            max_length=trainer.tokenizer.model_max_length,
            return_tensors="pt").input_ids.to(device),
    }

    def step():
        return trainer.train_step(batch, sync_gradients=True)

    for _ in range(args.warmup):
        step()

    # Whole-step hipGraph capture after the MIOpen-find warmup; timed
    # steps then replay it (1-GPU only). Opt-in with DCR_HIPGRAPH=1: on
    # the current ROCm stack the replayed step goes non-finite from its
    # second replay (loss, gradient and weights NaN in --dump-outputs)
    # while the eager step with the same batch stays finite; the runs are
    # recorded in profiles/r03_graph_nan/. A rate measured on that is not
    # a rate of the workload. Any capture failure falls back to the eager
    # step so the bench always completes.
    if want_graph:
        try:
            trainer.enable_hipgraph(batch)
            step()  # one replay outside the timed window
        except Exception as e:  # noqa: BLE001
            print(f"hipGraph capture unavailable ({type(e).__name__}: {e}); "
                  f"benching the eager step", file=sys.stderr)

    if dist_utils.is_dist():
        dist_utils.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    if use_cuda:
        torch.cuda.synchronize()
    if dist_utils.is_dist():
        dist_utils.barrier()
    elapsed = time.perf_counter() - t0

    # max over ranks (slowest rank defines job time)
    if dist_utils.is_dist():
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if use_cuda else None)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    phases = trainer.prof.summary()
    if phases and rank == 0:
        print("phase ms/step:", json.dumps({k: round(v, 2) for k, v in phases.items()}),
              file=sys.stderr)

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, trainer, loss)

    ms_per_step = elapsed / args.steps * 1000.0
    imgs_per_sec = args.batch_size * n_gpus * args.steps / elapsed

    if rank == 0:
        print(json.dumps({
            "metric": "sd21_256px_finetune_imgs_per_sec",
            "value": round(imgs_per_sec, 3),
            "unit": "imgs/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if use_cuda else "fp32",
            "data": "synthetic",
            "config": {
                "model": "sd2.1-unet-865M-random-init" if args.model == "sd21"
                         else "tiny-unet",
                "global_batch": args.batch_size * n_gpus,
                "resolution": args.resolution,
                "seq_len": 77,
                "parallelism": f"dp{n_gpus}",
                "optimizer": "fused_adamw",
            },
        }))


if __name__ == "__main__":
    main()
    # explicit teardown: a rank exiting with the group alive can race the
    # store shutdown under torchrun and turn a finished bench into a
    # non-zero exit
    import torch.distributed as _dist
    if _dist.is_available() and _dist.is_initialized():
        _dist.destroy_process_group()
