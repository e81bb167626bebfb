"""Bucketed gradient all-reduce with backward overlap (RCCL over xGMI).

Replaces the reference's accelerate-managed DDP
(/root/reference/diff_train.py:514-520,656) with an
explicit design for MI355X topology: each GPU has 7 point-to-point xGMI
links (≈153 GB/s each), so ring all-reduce is per-link bound — buckets
are sized (default 64 MiB) so per-bucket all-reduce launched DURING
backward hides under the remaining backward compute, and RCCL spreads
channels over the links.

Works with FusedAdamW's flat gradient arena: each bucket hook batch-
copies its params' autograd grads into the contiguous arena slice
(gather_grads) and all-reduces that slice — no per-param add kernels,
no flatten/unflatten traffic. Gradient accumulation parity
(diff_train.py:618): set `require_backward_grad_sync=False` on non-sync
micro-steps to skip collectives entirely.
"""
from __future__ import annotations

from typing import List, Optional

import torch.distributed as dist

from ..ops.adamw import FusedAdamW
from . import dist as dist_utils


class _Bucket:
    __slots__ = ("start", "end", "params", "pending", "work")

    def __init__(self, start: int, end: int, params: list):
        self.start = start
        self.end = end
        self.params = params
        self.pending = len(params)
        self.work = None


class GradBucketAllReduce:
    """Overlapped bucketed all-reduce over FusedAdamW's flat grad buffer."""

    def __init__(self, optimizer: FusedAdamW, bucket_mb: float = 64.0,
                 process_group: Optional[object] = None):
        self.opt = optimizer
        self.pg = process_group
        self.world = dist_utils.get_world_size()
        self.require_backward_grad_sync = True
        self.buckets: List[_Bucket] = []
        self._param_bucket = {}
        self._enabled = self.world > 1 and dist.is_initialized()

        if not self._enabled:
            return

        # broadcast initial flat params so every rank starts identical;
        # in pure-bf16 mode the fp32 master was cloned from the PRE-broadcast
        # rank-local weights (per-rank init seeds) and is the source of truth
        # for every update — refresh it or ranks diverge from step 1
        dist.broadcast(self.opt.flat_param, src=0, group=self.pg)
        if self.opt.master is not None:
            self.opt.master.copy_(self.opt.flat_param.float())

        bucket_elems = int(bucket_mb * 1024 * 1024 /
                           self.opt.flat_grad.element_size())
        # Buckets are contiguous param runs in REVERSE registration order:
        # backward produces grads roughly output->input, i.e. reverse order,
        # so the last-registered bucket completes (and launches) first.
        cur_params, cur_start, cur_end = [], None, None
        runs = list(zip(self.opt.params, self.opt.offsets))
        for p, off in reversed(runs):
            n = p.numel()
            if cur_start is None:
                cur_params, cur_start, cur_end = [p], off, off + n
            else:
                cur_params.append(p)
                cur_start = off
            if cur_end - cur_start >= bucket_elems:
                self._push_bucket(cur_start, cur_end, cur_params)
                cur_params, cur_start, cur_end = [], None, None
        if cur_params:
            self._push_bucket(cur_start, cur_end, cur_params)

        for p in self.opt.params:
            p.register_post_accumulate_grad_hook(self._hook)

    def _push_bucket(self, start, end, params):
        b = _Bucket(start, end, list(params))
        self.buckets.append(b)
        for p in params:
            self._param_bucket[id(p)] = b

    def _launch(self, b: _Bucket):
        # batched copy of this bucket's autograd grads into the arena
        # slice, then SUM all-reduce + post-scale (bf16 grads: pre-divide
        # would lose mantissa)
        # no fused sum of squares here: the all-reduce changes the values
        self.opt.gather_grads(b.params, sumsq=False)
        self.opt.arena_written()
        sl = self.opt.flat_grad[b.start:b.end]
        b.work = dist.all_reduce(sl, group=self.pg, async_op=True)

    def _hook(self, param):
        if not self.require_backward_grad_sync:
            return
        b = self._param_bucket[id(param)]
        b.pending -= 1
        if b.pending == 0:
            self._launch(b)

    def finalize(self):
        """Call after backward(), before optimizer.step()."""
        # any grads not yet moved by a bucket hook (world 1: all of them)
        self.opt.gather_grads()
        self.opt._ensure_cold_slices()
        if not self._enabled or not self.require_backward_grad_sync:
            self._reset()
            return
        for b in self.buckets:
            if b.work is None and b.pending > 0:
                # params that never produced grads this step (e.g. frozen path)
                self._launch(b)
        launched = any(b.work is not None for b in self.buckets)
        for b in self.buckets:
            if b.work is not None:
                b.work.wait()
        if launched and self.world > 1:
            self.opt.arena_written()
            self.opt.flat_grad.div_(self.world)
        self._reset()

    def _reset(self):
        for b in self.buckets:
            b.pending = len(b.params)
            b.work = None
