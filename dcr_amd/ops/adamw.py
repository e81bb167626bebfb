"""Flat-buffer fused AdamW for MI355X.

Reference behavior: torch.optim.AdamW over ~865M UNet params
(/root/reference/diff_train.py:435-446; betas 0.9/0.999, eps 1e-8,
weight_decay 1e-2). Instead of ~700 per-tensor kernel launches per step,
this optimizer re-parameterizes the model so that

* every parameter tensor is a VIEW into one contiguous flat buffer,
* gradients land in one contiguous flat arena via ``gather_grads()``
  (autograd owns per-param grads; no per-param adds): on the GPU one
  ``grad_gather_kernel`` launch copies the whole list and takes its sum of
  squares on the way, and accumulation micro-steps add through the same
  kernel's add mode (ops/hip/grad_tail.hip); gradients whose layout differs
  from their arena view go through ``copy_`` / ``add_``,
* Adam state (m, v) are two more flat buffers,

so one step is ONE elementwise HIP kernel over four flat arrays —
HBM-bound by design (~8 TB/s on MI355X), and the flat grad buffer doubles
as the bucket arena for RCCL all-reduce (dcr_amd/parallel/ddp.py).
``clip_and_step()`` is the training step's tail: the global-norm clip
coefficient stays on the device and the AdamW kernel (fp32 or FP8 state)
applies it, so the host never waits for the norm. ``DCR_FUSED_GRAD_TAIL=0``
(read per call) restores the ``_foreach_copy_`` / ``_foreach_add_`` /
``vector_norm`` / host-compare path.

Flatten AFTER moving the model to its device; ``p.data`` is replaced by
buffer views.

``state_bits=8`` (``--use_8bit_adam``) holds both moments as block-scaled
FP8 instead of fp32 — 2 B + 8 B/256 of state per parameter instead of 8 B.
The format (normative; checkpoints and ops/hip/adamw8.hip depend on it):

* a quantisation block is 256 consecutive elements of the flat arena
  (blocks ignore parameter boundaries), ``nblocks = ceil(numel / 256)``;
* per moment: codes ``uint8[nblocks*256]`` + ``absmax float32[nblocks]``;
  padding bytes past ``numel`` are 0 and stay 0;
* codes are OCP FP8 e4m3fn (``torch.float8_e4m3fn``: max 448, no inf):
  ``code = e4m3fn_rne(clamp(x * (448/absmax), -448, 448))``, ``absmax`` the
  block's ``max|x|``; dequantise as ``float(code) * (absmax/448)``; a block
  whose ``448/absmax`` is not finite (``absmax == 0``, or below ~1.3e-36
  where the scale overflows) is a zero block: codes 0, absmax 0;
* the first moment is stored as is, the second as ``r = sqrt(v)`` (halves
  the dynamic range a block spans; sign bit always 0).

One step dequantises, updates in fp32 with the UNquantised ``m'``/``v'``,
and requantises; rounding is to nearest even, deterministic.
"""
from __future__ import annotations

import os
from typing import Iterable, List, Tuple

import torch

from . import use_hip, require_hip, count_dispatch

# grad_gather_kernel's virtual block: elements of one parameter per block,
# and the grid (0: min(virtual blocks, 8192)). Sweep: ops/hip/README.md.
GATHER_CH = 16384
GATHER_GRID = 0

QBLOCK = 256
FP8_MAX = 448.0
STATE_FORMAT = {"state_bits": 8, "qblock": QBLOCK, "codec": "e4m3fn_absmax",
                "second_moment": "sqrt"}


def fused_grad_tail_enabled() -> bool:
    return os.environ.get("DCR_FUSED_GRAD_TAIL", "1") != "0"


def _nblocks(numel: int) -> int:
    return (numel + QBLOCK - 1) // QBLOCK


def _sqrt_rn(x: torch.Tensor) -> torch.Tensor:
    """Correctly rounded fp32 square root (through fp64), as the kernel's
    sqrtf is; torch's vectorised CPU sqrt is off by one ulp now and then."""
    return x.double().sqrt().float()


@torch.no_grad()
def quantize_blockwise(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Flat tensor -> (codes uint8[nblocks*256], absmax float32[nblocks]) in
    the format of the module docstring. The FP8 cast itself runs on the CPU
    (``.to(torch.float8_e4m3fn)``); results come back on ``x``'s device."""
    dev = x.device
    x = x.detach().reshape(-1).float()
    nb = _nblocks(x.numel())
    xp = torch.zeros(nb * QBLOCK, dtype=torch.float32, device=dev)
    xp[: x.numel()] = x
    xp = xp.view(nb, QBLOCK)
    absmax = xp.abs().amax(dim=1)
    # a true division: `448 / tensor` is reciprocal-then-multiply in torch,
    # one rounding too many to agree with the kernel at FP8 rounding ties
    scale = torch.full_like(absmax, FP8_MAX).div(absmax)
    # the scale is not finite for absmax == 0 and for absmax below
    # 448/FLT_MAX (~1.3e-36), where 0 * inf would put NaN codes on the
    # block's zeros: such a block is stored as a zero block (codes 0 — not
    # the 0x80 of a negative zero — and absmax 0). A NaN absmax stays NaN.
    ok = torch.isfinite(scale)
    scale = torch.where(ok, scale, torch.zeros_like(scale))
    y = (xp * scale[:, None]).clamp_(-FP8_MAX, FP8_MAX)
    codes = y.cpu().to(torch.float8_e4m3fn).view(torch.uint8).to(dev)
    codes = torch.where(ok[:, None], codes, torch.zeros_like(codes))
    absmax = torch.where(ok | absmax.isnan(), absmax, torch.zeros_like(absmax))
    return codes.reshape(-1).contiguous(), absmax.contiguous()


@torch.no_grad()
def dequantize_blockwise(codes: torch.Tensor, absmax: torch.Tensor,
                         numel: int) -> torch.Tensor:
    """Inverse of quantize_blockwise: float32[numel]."""
    dev = codes.device
    nb = absmax.numel()
    if codes.numel() != nb * QBLOCK or _nblocks(numel) != nb:
        raise ValueError(
            f"dequantize_blockwise: {codes.numel()} codes / {nb} blocks do "
            f"not describe {numel} elements")
    f = codes.detach().cpu().contiguous().view(torch.float8_e4m3fn).float().to(dev)
    out = f.view(nb, QBLOCK) * (absmax.float() / FP8_MAX)[:, None]
    return out.reshape(-1)[:numel].contiguous()


class FusedAdamW:
    def __init__(
        self,
        params: Iterable[torch.nn.Parameter],
        lr: float = 5e-6,
        betas=(0.9, 0.999),
        eps: float = 1e-8,
        weight_decay: float = 1e-2,
        device_state: bool = False,
        max_grad_norm: float = 1.0,
        state_bits: int = 32,
    ):
        if state_bits not in (32, 8):
            raise ValueError(f"FusedAdamW: state_bits must be 32 or 8, got {state_bits}")
        if state_bits == 8 and device_state:
            raise ValueError(
                "FusedAdamW: no device-state (graph-capturable) step exists "
                "for 8-bit optimizer state; use device_state=False")
        self.state_bits = state_bits
        self.lr = lr
        self.beta1, self.beta2 = betas
        self.eps = eps
        self.weight_decay = weight_decay
        self.step_count = 0
        self.max_grad_norm = max_grad_norm

        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("FusedAdamW: no trainable parameters")
        device = self.params[0].device
        dtype = self.params[0].dtype
        for p in self.params:
            if p.device != device or p.dtype != dtype:
                raise ValueError("FusedAdamW requires uniform param dtype/device")

        total = sum(p.numel() for p in self.params)
        self.flat_param = torch.empty(total, device=device, dtype=dtype)
        self.flat_grad = torch.zeros(total, device=device, dtype=dtype)
        if state_bits == 8:
            # block-scaled FP8 moments (module docstring); no fp32 arenas
            nb = _nblocks(total)
            self.exp_avg = self.exp_avg_sq = None
            self.exp_avg_q = torch.zeros(nb * QBLOCK, device=device, dtype=torch.uint8)
            self.exp_avg_absmax = torch.zeros(nb, device=device, dtype=torch.float32)
            self.exp_avg_sq_q = torch.zeros(nb * QBLOCK, device=device, dtype=torch.uint8)
            self.exp_avg_sq_absmax = torch.zeros(nb, device=device, dtype=torch.float32)
        else:
            self.exp_avg = torch.zeros(total, device=device, dtype=torch.float32)
            self.exp_avg_sq = torch.zeros(total, device=device, dtype=torch.float32)
        # pure-bf16 training: bf16 model params/grads + fp32 master copy
        self.master = None
        if dtype == torch.bfloat16:
            self.master = torch.empty(total, device=device, dtype=torch.float32)

        # Re-parameterize: params become views of flat_param. Grads are NOT
        # pre-assigned as arena views: with p.grad set, autograd's
        # AccumulateGrad issues one small `add_` kernel per parameter
        # (~700 launch-bound kernels, ~3.5 ms/step measured in the round-1
        # profile). Leaving p.grad unset lets autograd hand over the
        # computed tensor for free; gather_grads() then moves them into
        # the arena in a handful of batched _foreach kernels.
        offset = 0
        self.offsets: List[int] = []
        self._grad_views: List[torch.Tensor] = []
        for p in self.params:
            n = p.numel()
            sl = self.flat_param[offset : offset + n]
            gl = self.flat_grad[offset : offset + n]
            if (p.data.dim() == 4 and not p.data.is_contiguous()
                    and p.data.is_contiguous(
                        memory_format=torch.channels_last)):
                # channels_last conv weights: store in NHWC memory order
                # and view back with channels_last strides — a plain
                # view_as() would silently revert them to NCHW, making
                # every conv pay a per-call weight relayout (measured
                # ~2 ms/step of aten::copy_, profile_aten r02c8) and
                # de-eligibilizing the native conv kernel for every
                # TRAINED module (the frozen VAE was the only one
                # actually running it)
                K, C, Hh, Ww = p.data.shape
                sl.copy_(p.data.permute(0, 2, 3, 1).reshape(-1))
                p.data = sl.view(K, Hh, Ww, C).permute(0, 3, 1, 2)
                self._grad_views.append(
                    gl.view(K, Hh, Ww, C).permute(0, 3, 1, 2))
            else:
                sl.copy_(p.data.reshape(-1))
                p.data = sl.view_as(p.data)
                self._grad_views.append(gl.view_as(p.data))
            self.offsets.append(offset)
            offset += n
        self.numel = total
        self._view_of = {id(p): v for p, v in zip(self.params, self._grad_views)}
        self._gathered: set = set()
        if self.master is not None:
            self.master.copy_(self.flat_param.float())

        # native gradient tail (ops/hip/grad_tail.hip): per-virtual-block
        # sums of squares, the {sumsq, norm, coef} device record, and
        # whether `_partials` currently holds the sums of what is in the
        # arena (see arena_written())
        self._nvb_all = sum((p.numel() + GATHER_CH - 1) // GATHER_CH
                            for p in self.params)
        self._partials = None
        self._norm_rec = None
        self._sumsq_valid = False

        # device-state mode (round-2 draft, DCR_DEV_ADAMW=1): all per-step
        # scalars live in hyper[8] on device so the whole optimizer tail is
        # hipGraph-capturable — see elementwise.hip adamw_dev section.
        # hyper = {lr, b1^t, b2^t, inv_bc1, inv_bc2, clip_coef, gnorm_sq, t}
        self.hyper = None
        if device_state and device.type == "cuda":
            self.hyper = torch.tensor([lr, 1, 1, 1, 1, 1, 0, 0],
                                      dtype=torch.float32, device=device)

    # -- torch.optim-ish surface ------------------------------------------
    def zero_grad(self, set_to_none: bool = False):
        # the arena-wide zero exists so slices whose params produce no
        # grad read 0 — when EVERY param was gathered last cycle (the
        # normal training case) the next cycle's first gather per param
        # is a copy, so the zero is skippable (1.7 GB write saved).
        # _ensure_cold_slices() covers the rare dynamic-graph case where
        # a later cycle leaves some params ungathered.
        self.arena_written()
        if len(self._gathered) != len(self.params):
            self.flat_grad.zero_()
            self._skipped_zero = False
        else:
            self._skipped_zero = True
        self._gathered.clear()
        for p in self.params:
            p.grad = None

    def _ensure_cold_slices(self):
        """After the final gather of a cycle whose zero was skipped, any
        param that produced no grad this cycle still holds LAST cycle's
        grad in its arena slice — zero exactly those."""
        if not getattr(self, "_skipped_zero", False):
            return
        if len(self._gathered) == len(self.params):
            return
        stale = [self._view_of[id(p)] for p in self.params
                 if id(p) not in self._gathered]
        if stale:
            self.arena_written()
            torch._foreach_zero_(stale)
        self._skipped_zero = False

    def arena_written(self):
        """Declare that ``flat_grad`` holds, or is about to hold, values the
        fused sum of squares did not see. EVERY site that writes the arena
        outside ``grad_gather_kernel``'s own full-coverage copy calls this:
        add-mode gathers (the kernel's add mode takes no sum, and
        ``_foreach_add_`` has none), partial gathers, the per-parameter
        fallback copy / add, ``_ensure_cold_slices``' zeroing, ``zero_grad``,
        the clip's ``mul_`` and the clipped store-back of the AdamW kernels
        (fp32 and FP8 state), and outside this
        class the bucket all-reduce and ``div_`` of
        ``GradBucketAllReduce`` and the fp16 scaler's ``mul_`` in
        ``Trainer.train_step``. A new writer of the arena must call it too:
        ``clip_and_step`` then takes the standalone sum-of-squares pass
        instead of trusting a sum of values that are no longer there."""
        self._sumsq_valid = False

    def _native_tail(self):
        """The extension when the native gather / norm / clip path applies to
        this call, else None (CPU, switch off, or stream capture: a captured
        copy of the pinned pointer table would replay stale pointers)."""
        if not self.flat_grad.is_cuda or not fused_grad_tail_enabled():
            return None
        if torch.cuda.is_current_stream_capturing():
            return None
        return require_hip("grad_tail")

    def _get_partials(self) -> torch.Tensor:
        if self._partials is None:
            self._partials = torch.empty(
                max(self._nvb_all, 1), dtype=torch.float32,
                device=self.flat_grad.device)
        return self._partials

    @torch.no_grad()
    def gather_grads(self, params=None, sumsq: bool = True):
        """Move autograd-produced p.grad tensors into the flat arena (first
        gather per param after zero_grad is a copy over the slice; later
        gathers — gradient accumulation micro-steps — add). Called
        per-bucket by the DDP engine (before each bucket's all-reduce,
        with ``sumsq=False``: the all-reduce changes the values) and by
        finalize().

        On the GPU the copies are one ``grad_gather_kernel`` launch; a
        gradient whose dtype or memory layout differs from its arena view
        is copied with ``copy_``. When one call copies EVERY parameter that
        way and ``sumsq`` is on, the kernel also leaves the arena's sum of
        squares in ``_partials`` and the validity flag is set. The adds are
        one launch of the same kernel in add mode (``dst = T(float(dst) +
        float(src))``, the rounded add of ``_foreach_add_``), with ``add_``
        for a gradient the kernel does not take; an add never leaves a valid
        sum, so the step after accumulation takes the standalone pass. A call
        that copies some parameters and adds to others issues both launches.
        Without the native path (CPU, switch off, stream capture) the copies
        use ``_foreach_copy_`` and the adds ``_foreach_add_``."""
        m = self._native_tail()
        copy_d, copy_s, add_d, add_s = [], [], [], []
        for p in (params if params is not None else self.params):
            g = p.grad
            if g is None:
                continue
            view = self._view_of[id(p)]
            if g.dtype != view.dtype:
                g = g.to(view.dtype)
            if id(p) in self._gathered:
                add_d.append(view)
                add_s.append(g)
            else:
                copy_d.append(view)
                copy_s.append(g)
                self._gathered.add(id(p))
            p.grad = None
        if copy_d or add_d:
            self.arena_written()
        if copy_d and m is not None:
            fused = (sumsq and params is None and not add_d
                     and len(copy_d) == len(self.params))
            rejected = m.grad_gather(
                self.flat_grad, copy_d, copy_s,
                self._get_partials() if fused else None,
                GATHER_CH, GATHER_GRID)
            count_dispatch('grad_gather')
            for i in rejected:
                count_dispatch('grad_gather_fallback')
                copy_d[i].copy_(copy_s[i])
            self._sumsq_valid = fused and not rejected
        elif copy_d:
            if self.flat_grad.is_cuda:
                count_dispatch('grad_gather_foreach')
            torch._foreach_copy_(copy_d, copy_s)
        if add_d and m is not None:
            rejected = m.grad_gather(self.flat_grad, add_d, add_s, None,
                                     GATHER_CH, GATHER_GRID, True)
            count_dispatch('grad_gather_add')
            for i in rejected:
                count_dispatch('grad_gather_fallback')
                add_d[i].add_(add_s[i])
        elif add_d:
            torch._foreach_add_(add_d, add_s)

    @torch.no_grad()
    def step(self, lr: float | None = None):
        self.gather_grads()  # no-op when finalize() already ran
        self._ensure_cold_slices()
        if lr is not None:
            self.lr = lr
        self.step_count += 1
        t = self.step_count
        if self.state_bits == 8:
            self._step8(t)
            return
        if use_hip(self.flat_param):
            m = require_hip("adamw")
            if m is not None:
                count_dispatch('adamw')
                if self.master is not None:
                    m.adamw_step_bf16(
                        self.flat_param, self.flat_grad, self.master,
                        self.exp_avg, self.exp_avg_sq, self.lr, self.beta1,
                        self.beta2, self.eps, self.weight_decay, t)
                else:
                    m.adamw_step(
                        self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq,
                        self.lr, self.beta1, self.beta2, self.eps, self.weight_decay, t,
                    )
                return
        # reference implementation (CPU tests / debug fallback)
        bc1 = 1.0 - self.beta1 ** t
        bc2 = 1.0 - self.beta2 ** t
        g = self.flat_grad.float()
        self.exp_avg.mul_(self.beta1).add_(g, alpha=1 - self.beta1)
        self.exp_avg_sq.mul_(self.beta2).addcmul_(g, g, value=1 - self.beta2)
        denom = (self.exp_avg_sq / bc2).sqrt_().add_(self.eps)
        upd = (self.exp_avg / bc1) / denom
        if self.master is not None:
            self.master.add_(upd + self.weight_decay * self.master, alpha=-self.lr)
            self.flat_param.copy_(self.master.to(self.flat_param.dtype))
        else:
            self.flat_param.add_(
                (upd + self.weight_decay * self.flat_param.float()).to(self.flat_param.dtype),
                alpha=-self.lr,
            )

    def _step8(self, t: int):
        """One step on block-scaled FP8 state (format: module docstring)."""
        if use_hip(self.flat_param):
            m = require_hip("adamw8")
            if m is not None:
                count_dispatch('adamw8')
                if self.master is not None:
                    m.adamw8_step_bf16(
                        self.flat_param, self.flat_grad, self.master,
                        self.exp_avg_q, self.exp_avg_absmax,
                        self.exp_avg_sq_q, self.exp_avg_sq_absmax, self.lr,
                        self.beta1, self.beta2, self.eps, self.weight_decay, t)
                else:
                    m.adamw8_step(
                        self.flat_param, self.flat_grad,
                        self.exp_avg_q, self.exp_avg_absmax,
                        self.exp_avg_sq_q, self.exp_avg_sq_absmax, self.lr,
                        self.beta1, self.beta2, self.eps, self.weight_decay, t)
                return
        # reference implementation (CPU tests / debug fallback). Every
        # multiply and add is its own torch op (no `alpha=`/addcmul, which
        # fuse into FMAs on some CPU paths) and the scalars are formed in
        # double then rounded once — the kernel does the same, so the two
        # agree to the last bit (sqrt and divide round correctly on both).
        n = self.numel
        inv_bc1 = 1.0 / (1.0 - self.beta1 ** t)
        inv_bc2 = 1.0 / (1.0 - self.beta2 ** t)
        g = self.flat_grad.float()
        m_ = dequantize_blockwise(self.exp_avg_q, self.exp_avg_absmax, n)
        r_ = dequantize_blockwise(self.exp_avg_sq_q, self.exp_avg_sq_absmax, n)
        m_ = m_.mul(self.beta1).add(g.mul(1.0 - self.beta1))
        v_ = r_.mul(r_).mul(self.beta2).add(g.mul(g).mul(1.0 - self.beta2))
        denom = _sqrt_rn(v_.mul(inv_bc2)).add(self.eps)
        w = self.master if self.master is not None else self.flat_param
        upd = m_.mul(inv_bc1).div(denom).add(w.mul(self.weight_decay))
        w.copy_(w.sub(upd.mul(self.lr)))
        if self.master is not None:
            self.flat_param.copy_(self.master.to(self.flat_param.dtype))
        q, a = quantize_blockwise(m_)
        self.exp_avg_q.copy_(q)
        self.exp_avg_absmax.copy_(a)
        q, a = quantize_blockwise(_sqrt_rn(v_))
        self.exp_avg_sq_q.copy_(q)
        self.exp_avg_sq_absmax.copy_(a)

    def state_nbytes(self) -> int:
        """Bytes held in moment state: codes + scales, or the two fp32 arenas."""
        if self.state_bits == 8:
            ts = (self.exp_avg_q, self.exp_avg_absmax,
                  self.exp_avg_sq_q, self.exp_avg_sq_absmax)
        else:
            ts = (self.exp_avg, self.exp_avg_sq)
        return sum(t.numel() * t.element_size() for t in ts)

    @torch.no_grad()
    def step_dev(self, lr: float | None = None):
        """Device-state step (clip INCLUDED — do not call clip_grad_norm_
        separately): 3 stream-ordered kernels reading every scalar from the
        hyper buffer; capturable into a hipGraph. The only host work is the
        4-byte lr write when the schedule moves."""
        assert self.hyper is not None, "built without device_state=True"
        self.gather_grads()  # no-op when finalize() already ran
        self._ensure_cold_slices()
        if lr is not None and lr != self.lr:
            self.lr = lr
            self.hyper[0].fill_(lr)  # outside any captured graph
        self.step_count += 1
        m = require_hip("adamw")
        count_dispatch('adamw_dev')
        m.adamw_step_dev(self.flat_param, self.flat_grad, self.master,
                         self.exp_avg, self.exp_avg_sq, self.hyper,
                         self.beta1, self.beta2, self.eps, self.weight_decay,
                         self.max_grad_norm)

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """Global L2 grad clip (reference: diff_train.py:657-663, max 1.0).
        fp32 accumulation via the dtype arg — `.float()` would
        materialize a full fp32 copy of the 1.7 GB bf16 arena first
        (~1 ms/step, profile_aten r02c8).

        This call always takes aten's norm over the arena and reads it on
        the host, also right after a gather that left a valid fused sum of
        squares: a caller of ``clip_grad_norm_`` + ``step`` pays for the norm
        a second time. The training step uses ``clip_and_step``."""
        self.gather_grads()  # no-op when finalize() already ran
        self._ensure_cold_slices()
        if self.flat_grad.is_cuda:
            count_dispatch('grad_norm_aten')
        norm = torch.linalg.vector_norm(self.flat_grad, dtype=torch.float32)
        scale = max_norm / (norm + 1e-6)
        if float(norm) > max_norm:
            self.arena_written()
            self.flat_grad.mul_(scale.to(self.flat_grad.dtype))
        return norm

    def _norm_record(self, m, max_norm: float) -> torch.Tensor:
        """Device record {sumsq, norm, coef} of the arena as it stands: from
        the gather's fused partials when they are valid, else from the
        standalone pass over the same virtual-block partition (same bits)."""
        if self._norm_rec is None:
            self._norm_rec = torch.zeros(3, dtype=torch.float32,
                                         device=self.flat_grad.device)
        partials = self._get_partials()
        if not self._sumsq_valid:
            count_dispatch('grad_sumsq')
            m.grad_sumsq(self.flat_grad, self._grad_views, partials,
                         GATHER_CH, GATHER_GRID)
            self._sumsq_valid = True
        count_dispatch('grad_norm_finalize')
        m.sumsq_finalize(partials, self._nvb_all, float(max_norm),
                         self._norm_rec)
        return self._norm_rec

    @torch.no_grad()
    def clip_and_step(self, max_norm: float, lr: float | None = None) -> torch.Tensor:
        """``clip_grad_norm_(max_norm)`` followed by ``step(lr)`` with no
        host read in between: the norm and the clip coefficient stay in a
        device record, and the AdamW kernel applies the coefficient, storing
        the clipped gradient back into the arena when it is not 1, so the
        arena, parameters, master copy and moments end as the two calls
        leave them. Returns the gradient norm as a 0-dim device tensor (a
        view of the record: the next call overwrites it). 8-bit state runs
        the same tail with ``adamw8_kernel<P, true>``. CPU,
        ``DCR_FUSED_GRAD_TAIL=0`` and stream capture take the two calls.

        ``max_norm`` means what it means to ``clip_grad_norm_``, on every
        path: the gradient is scaled whenever ``norm > max_norm``, so
        ``max_norm = 0`` does NOT switch clipping off, it zeroes the
        gradient, and a negative ``max_norm`` flips its sign."""
        m = self._native_tail()
        if m is None:
            norm = self.clip_grad_norm_(max_norm)
            self.step(lr=lr)
            return norm
        self.gather_grads()  # no-op when finalize() already ran
        self._ensure_cold_slices()
        rec = self._norm_record(m, max_norm)
        if lr is not None:
            self.lr = lr
        self.step_count += 1
        if self.state_bits == 8:
            count_dispatch('adamw8')
            count_dispatch('adamw8_clip')
            state = (self.exp_avg_q, self.exp_avg_absmax, self.exp_avg_sq_q,
                     self.exp_avg_sq_absmax, self.lr, self.beta1, self.beta2,
                     self.eps, self.weight_decay, self.step_count, rec)
            if self.master is not None:
                m.adamw8_step_bf16_clip(self.flat_param, self.flat_grad,
                                        self.master, *state)
            else:
                m.adamw8_step_clip(self.flat_param, self.flat_grad, *state)
            self.arena_written()  # the kernel stores the clipped gradient back
            return rec[1]
        count_dispatch('adamw')
        count_dispatch('adamw_clip')
        if self.master is not None:
            m.adamw_step_bf16_clip(
                self.flat_param, self.flat_grad, self.master, self.exp_avg,
                self.exp_avg_sq, self.lr, self.beta1, self.beta2, self.eps,
                self.weight_decay, self.step_count, rec)
        else:
            m.adamw_step_clip(
                self.flat_param, self.flat_grad, self.exp_avg,
                self.exp_avg_sq, self.lr, self.beta1, self.beta2, self.eps,
                self.weight_decay, self.step_count, rec)
        self.arena_written()  # the kernel stores the clipped gradient back
        return rec[1]

    # -- checkpointing -----------------------------------------------------
    def state_dict(self):
        if self.state_bits == 8:
            d = {
                "step": self.step_count,
                "lr": self.lr,
                "flat_param": self.flat_param,
                "exp_avg_q": self.exp_avg_q,
                "exp_avg_absmax": self.exp_avg_absmax,
                "exp_avg_sq_q": self.exp_avg_sq_q,
                "exp_avg_sq_absmax": self.exp_avg_sq_absmax,
                "format": dict(STATE_FORMAT),
            }
            if self.master is not None:
                d["master"] = self.master
            return d
        d = {
            "step": self.step_count,
            "lr": self.lr,
            "exp_avg": self.exp_avg,
            "exp_avg_sq": self.exp_avg_sq,
            "flat_param": self.flat_param,
        }
        if self.master is not None:
            d["master"] = self.master
        if self.hyper is not None:
            d["hyper"] = self.hyper
        return d

    def _check_8bit_sd(self, sd):
        """Validate a checkpoint when either side holds 8-bit state; raises
        ValueError before anything is modified."""
        n, nb = self.numel, _nblocks(self.numel)
        fmt = sd.get("format")
        if sd["flat_param"].numel() != n:
            raise ValueError(
                f"FusedAdamW.load_state_dict: checkpoint has "
                f"{sd['flat_param'].numel()} params, optimizer has {n}")
        if "master" in sd and sd["master"].numel() != n:
            raise ValueError("FusedAdamW.load_state_dict: master numel mismatch")
        if fmt is None:
            for k in ("exp_avg", "exp_avg_sq"):
                if k not in sd or sd[k].numel() != n:
                    raise ValueError(
                        f"FusedAdamW.load_state_dict: fp32-state checkpoint "
                        f"needs '{k}' of {n} elements")
            return
        if fmt.get("codec") != STATE_FORMAT["codec"]:
            raise ValueError(f"FusedAdamW.load_state_dict: unknown codec "
                             f"{fmt.get('codec')!r}")
        if fmt.get("qblock") != QBLOCK:
            raise ValueError(f"FusedAdamW.load_state_dict: unknown qblock "
                             f"{fmt.get('qblock')!r}")
        if fmt.get("state_bits") != 8 or \
                fmt.get("second_moment") != STATE_FORMAT["second_moment"]:
            raise ValueError(f"FusedAdamW.load_state_dict: unknown state "
                             f"format {fmt!r}")
        for k, want in (("exp_avg_q", nb * QBLOCK), ("exp_avg_absmax", nb),
                        ("exp_avg_sq_q", nb * QBLOCK), ("exp_avg_sq_absmax", nb)):
            if k not in sd or sd[k].numel() != want:
                raise ValueError(
                    f"FusedAdamW.load_state_dict: '{k}' must hold {want} "
                    f"elements for numel {n}")

    def _load_moments(self, sd):
        fmt = sd.get("format")
        if self.state_bits == 8:
            if fmt is not None:            # 8 -> 8: copy
                for k in ("exp_avg_q", "exp_avg_absmax",
                          "exp_avg_sq_q", "exp_avg_sq_absmax"):
                    getattr(self, k).copy_(sd[k])
            else:                          # 32 -> 8: quantise (v as sqrt)
                q, a = quantize_blockwise(sd["exp_avg"].cpu())
                self.exp_avg_q.copy_(q)
                self.exp_avg_absmax.copy_(a)
                q, a = quantize_blockwise(_sqrt_rn(sd["exp_avg_sq"].cpu().float()))
                self.exp_avg_sq_q.copy_(q)
                self.exp_avg_sq_absmax.copy_(a)
        else:                              # 8 -> 32: dequantise, v = r*r
            self.exp_avg.copy_(dequantize_blockwise(
                sd["exp_avg_q"].cpu(), sd["exp_avg_absmax"].cpu(), self.numel))
            r = dequantize_blockwise(
                sd["exp_avg_sq_q"].cpu(), sd["exp_avg_sq_absmax"].cpu(), self.numel)
            self.exp_avg_sq.copy_(r * r)

    @torch.no_grad()
    def load_state_dict(self, sd):
        if self.state_bits == 8 or sd.get("format") is not None:
            self._check_8bit_sd(sd)
            self.step_count = sd["step"]
            self.lr = sd["lr"]
            self._load_moments(sd)
        else:
            self.step_count = sd["step"]
            self.lr = sd["lr"]
            self.exp_avg.copy_(sd["exp_avg"])
            self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.flat_param.copy_(sd["flat_param"])
        if self.hyper is not None and "hyper" in sd:
            self.hyper.copy_(sd["hyper"])
        if self.master is not None:
            if "master" in sd:
                self.master.copy_(sd["master"])
            else:
                self.master.copy_(self.flat_param.float())
