"""Is the hipGraph-replayed train step still the eager train step?

Drives the trainer exactly as bench.py's graph run does (SD-2.1, 256px,
bs16, pure bf16, NHWC, MIOpen find on, 3 eager warm-up steps, capture,
replays) and prints after every step whether loss, flat gradient and
weights are finite. When the gradient first goes non-finite it lists the
parameters whose gradient holds the bad elements.

    python scripts/graph_replay_check.py            # graph replay
    CHECK_GRAPH=0 python scripts/graph_replay_check.py   # eager, same batch
    CHECK_SEED=7 CHECK_LRWARM=0 ...                 # other seed / constant lr

Recorded runs: profiles/r03_graph_nan/.
"""
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dcr_amd.train import TrainConfig, Trainer  # noqa: E402

device = torch.device("cuda", 0)
torch.cuda.set_device(device)
cfg = TrainConfig(model_size="sd21", synthetic_data=True, synthetic_size=64,
                  resolution=256, train_batch_size=16,
                  mixed_precision="pure_bf16", dataloader_num_workers=0,
                  max_train_steps=10**9,
                  seed=int(os.environ.get("CHECK_SEED", "1234")),
                  lr_warmup_steps=int(os.environ.get("CHECK_LRWARM", "5000")),
                  output_dir="/tmp/dcr_bench_out", channels_last=True)
trainer = Trainer(cfg, device=device)  # sets cudnn.benchmark = True
if os.environ.get("CHECK_FIND") == "0":
    torch.backends.cudnn.benchmark = False
trainer.unet.train()
g = torch.Generator().manual_seed(1234)
batch = {
    "pixel_values": (torch.rand(16, 3, 256, 256, generator=g) * 2 - 1).to(device),
    "input_ids": trainer.tokenizer(
        [f"An image of sample {i} rank 0" for i in range(16)],
        truncation=True, padding="max_length",
        max_length=trainer.tokenizer.model_max_length,
        return_tensors="pt").input_ids.to(device),
}
opt = trainer.optimizer
names = [(n, p) for n, p in trainer.unet.named_parameters() if p.requires_grad]


def report(tag, loss):
    torch.cuda.synchronize()
    ok = bool(torch.isfinite(opt.flat_grad).all())
    print(f"{tag}: loss={float(loss):.5f} grad_finite={ok} "
          f"weights_finite={bool(torch.isfinite(opt.master).all())}", flush=True)
    return ok


def blame():
    bad = [k for k, (_, p) in enumerate(names)
           if not bool(torch.isfinite(opt._view_of[id(p)]).all())]
    print(f"  non-finite gradient in {len(bad)} of {len(names)} parameters")
    for k in bad:
        v = opt._view_of[id(names[k][1])]
        print(f"    {names[k][0]} shape={tuple(v.shape)} "
              f"bad_elements={int((~torch.isfinite(v)).sum())}")


for i in range(3):
    report(f"eager warm-up {i}", trainer.train_step(batch))
graph = os.environ.get("CHECK_GRAPH", "1") != "0"
if graph:
    trainer.enable_hipgraph(batch)
for i in range(8):
    ok = report(f"{'replay' if graph else 'eager'} {i}",
                trainer.train_step(batch))
    if not ok:
        blame()
        break
