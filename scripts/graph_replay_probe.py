"""PyTorch-only probe: does a captured graph replay correctly on reused memory?

No dcr_amd code. The body is a chain of bf16 matmuls and column sums
(`sum(0)` over 65536 rows is a multi-block reduction that starts from a
zero-filled semaphore buffer) and leaves NaN-filled blocks behind in the
graph's memory pool. Inputs never change, so every replay must reproduce
the eager result. Recorded output: profiles/r03_graph_nan/.

    python scripts/graph_replay_probe.py [thread_local|global]
"""
import sys

import torch

mode = sys.argv[1] if len(sys.argv) > 1 else "thread_local"
dev = torch.device("cuda", 0)
torch.manual_seed(0)
x = torch.randn(16 * 4096, 320, device=dev, dtype=torch.bfloat16)
w = torch.randn(320, 320, device=dev, dtype=torch.bfloat16)


def body():
    outs = []
    h = x
    for _ in range(6):
        h = (h @ w) * 0.05
        outs.append(h.sum(0))
        t = torch.full_like(h, float("nan"))  # garbage for the next user
        del t
    return torch.stack(outs)


ref = body()
torch.cuda.synchronize()
s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    for _ in range(2):
        body()
torch.cuda.current_stream().wait_stream(s)
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g, capture_error_mode=mode):
    out = body()
for i in range(4):
    g.replay()
    torch.cuda.synchronize()
    err = (out.float() - ref.float()).abs().max().item()
    print(f"mode={mode} replay {i}: nonfinite={int((~torch.isfinite(out)).sum())} "
          f"max_err_vs_eager={err:.4g} (max |eager| {ref.float().abs().max().item():.4g})",
          flush=True)
