"""Linear-layer dispatch: library forward/dgrad, native weight gradient
where the library's starves the GPU, native bias gradient.

The reference runs every UNet linear (QKV/out projections, GEGLU
FeedForward matmuls, proj_in/out) through the vendor BLAS. Here:

* forward and dgrad stay with rocBLAS/Tensile: the in-tree 128x128 MFMA
  kernel (`gemm_bf16`) reaches 0.42-0.59x of it on the SD-2.1 shapes
  (scripts/bench_gemm.py).
* the weight gradient dy.T @ x goes to `linear_wgrad` (gemm.hip: split
  contraction, fp32 slab, ordered reduction, fused bias gradient) for the
  shapes `_native_wgrad_rule(M, N, K)` accepts. The library runs one
  workgroup per 64x64 tile of dW over all M rows, so the 320x320 layers
  with 16384 rows occupy 25 of 256 CUs for 102 us; the native pair of
  launches takes 19 us (scripts/bench_wgrad.py, operands rotated through a
  pool larger than the last-level cache; table and sweep in
  dcr_amd/ops/hip/README.md). Measured wins, native dw against dy.t() @ x
  alone / native dw+db against library + colsum: 16384x320x320 5.6x / 6.0x,
  16384x320x1280 3.2x / 3.3x, 16384x2560x320 1.16x / 1.35x, 4096x640x640
  1.38x / 1.69x, 1232x320x1024 1.50x (bias-free). Measured losses, left
  with the library: 4096x640x2560 0.72x, 4096x5120x640 0.44x, every
  1024-row level-2 shape 0.18-0.61x, 1232x640x1024 0.89x, 1232x1280x1024
  0.82x. In the model the step went from 68.0-68.3 to 63.2-63.4 ms
  (profiles/r07_prof_*.md). DCR_NATIVE_WGRAD=0, read per call, restores
  the library weight gradient exactly.
* elsewhere the bias gradient alone is native: reduce.hip's column sum
  replaces the aten reduction. DCR_NATIVE_BIAS_GRAD=0, read per call, turns
  that off.

All of the above is one autograd Function, `_DefaultLinear`; bias-free
linears reach it only for the native weight gradient.

The older `gemm_bf16(ta=1, tb=1)` weight gradient (two-byte transposed
gathers, fp32 atomics into a zero-filled workspace + finalize) measured
83 us at 16384x320x320 and lost in the whole-model profile
(profiles/r02_prof_head.md); it stays behind DCR_NATIVE_GEMM=1 (hybrid)
and DCR_NATIVE_GEMM=full (all three passes native, benching only).
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import use_hip, require_hip, count_dispatch


def _mode() -> str:
    return os.environ.get("DCR_NATIVE_GEMM", "0")


def _wgrad_eligible(x2d: torch.Tensor, weight: torch.Tensor) -> bool:
    M, K = x2d.shape
    N = weight.shape[0]
    return (x2d.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and K % 8 == 0 and N % 8 == 0 and M % 8 == 0 and M >= 4096)


def _bias_grad_enabled() -> bool:
    return os.environ.get("DCR_NATIVE_BIAS_GRAD", "1") != "0"


# Below this many rows of dy the native column sum is not dispatched. The
# only such linears in the UNet are the [16, C] time-embedding projections:
# scripts/bench_norms.py measured 4.1 us native against 5.1 us aten at
# 16x1280 (profiles/r06_bench_norms.log): 1 us per call, 26 calls a step,
# less than the host time a Python autograd Function adds to each of them
# in the eager step (reasoned, not measured in the model). From 256 rows up
# the kernel measured 1.2-3.6x the aten reduction.
_BIAS_GRAD_MIN_ROWS = 64


def _native_wgrad_enabled() -> bool:
    return os.environ.get("DCR_NATIVE_WGRAD", "1") != "0"


# linear_wgrad (gemm.hip) takes dw (+ db) where the library's weight
# gradient starves the GPU: it runs one workgroup per 64x64 tile of dW, each
# walking all M rows, so with fewer tiles than the 256 CUs its time is set
# by M alone (about 6.7 ns a row: 108 us at 16384 rows, 28 us at 4096)
# whatever N and K are. The native pair of launches costs about 14 us at
# the least, and its time grows with the operand re-reads, that is with
# the tile count. Measured with scripts/bench_wgrad.py (module docstring):
# up to 100 tiles it wins from 1232 rows on; between 100 and 256 tiles only
# the 16384-row GEGLU projection was measured to win, the 1232-row context
# projection with 160 tiles was not; above 256 tiles the library wins.
_WGRAD_SMALL_TILES, _WGRAD_SMALL_MIN_ROWS = 100, 1024
_WGRAD_MAX_TILES, _WGRAD_MIN_ROWS = 256, 8192


def _native_wgrad_rule(M: int, N: int, K: int) -> bool:
    if N % 8 or K % 8 or M * max(N, K) >= 1 << 30:   # the kernel's limits
        return False
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    if tiles <= _WGRAD_SMALL_TILES:
        return M >= _WGRAD_SMALL_MIN_ROWS
    return tiles <= _WGRAD_MAX_TILES and M >= _WGRAD_MIN_ROWS


class _DefaultLinear(torch.autograd.Function):
    """Default path: library GEMMs for forward and dgrad, exactly the ones
    autograd issues for F.linear. With `native_wgrad`, dw and db come from
    one linear_wgrad call (split-contraction MFMA kernel + ordered slab
    reduction); otherwise dw is the library's dy.T @ x and the bias gradient
    the native column-sum kernel instead of an aten reduction."""

    @staticmethod
    def forward(ctx, x, weight, bias, native_wgrad):
        y = F.linear(x, weight, bias)
        ctx.save_for_backward(x, weight)
        ctx.native_wgrad = native_wgrad
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (dy2 @ weight).view(x.shape)
        if ctx.native_wgrad and ctx.needs_input_grad[1]:
            m = require_hip("linear_wgrad")
            count_dispatch("linear_wgrad")
            out = m.linear_wgrad(dy2.contiguous(),
                                 x.reshape(-1, x.shape[-1]).contiguous(),
                                 bool(ctx.needs_input_grad[2]))
            dw = out[0]
            if ctx.needs_input_grad[2]:
                db = out[1]
            return dx, dw, db, None
        if ctx.needs_input_grad[1]:
            dw = dy2.t() @ x.reshape(-1, x.shape[-1])
        if ctx.needs_input_grad[2]:
            m = require_hip("colsum")
            count_dispatch("bias_grad")
            db = m.colsum(dy2.contiguous())
        return dx, dw, db, None


class _HybridLinear(torch.autograd.Function):
    """rocBLAS fwd/dgrad, native MFMA wgrad (+fused dbias)."""

    @staticmethod
    def forward(ctx, x2d, weight, bias):
        y = F.linear(x2d, weight, bias)
        ctx.save_for_backward(x2d, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x2d, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dy @ weight if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1]:
            m = require_hip("gemm_bf16")
            count_dispatch("gemm_wgrad")
            want_db = ctx.has_bias and ctx.needs_input_grad[2]
            if want_db:
                dw, db = m.gemm_bf16(dy, x2d, None, True, True, True)
                db = db.to(dy.dtype)
            else:
                (dw,) = m.gemm_bf16(dy, x2d, None, True, True, False)
        elif ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0)
        return dx, dw, db


class _FullNativeLinear(torch.autograd.Function):
    """All three passes on gemm.hip (DCR_NATIVE_GEMM=full — benching)."""

    @staticmethod
    def forward(ctx, x2d, weight, bias):
        m = require_hip("gemm_bf16")
        count_dispatch("gemm")
        (y,) = m.gemm_bf16(x2d, weight, bias, False, False, False)
        ctx.save_for_backward(x2d, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x2d, weight = ctx.saved_tensors
        m = require_hip("gemm_bf16")
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            (dx,) = m.gemm_bf16(dy, weight, None, False, True, False)
        dw = db = None
        if ctx.needs_input_grad[1]:
            if ctx.has_bias and ctx.needs_input_grad[2]:
                dw, db = m.gemm_bf16(dy, x2d, None, True, True, True)
                db = db.to(dy.dtype)
            else:
                (dw,) = m.gemm_bf16(dy, x2d, None, True, True, False)
        return dx, dw, db


def dcr_linear(x: torch.Tensor, weight: torch.Tensor,
               bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.linear with the native MFMA wgrad in its measured-win regime."""
    mode = _mode()
    if mode != "0" and use_hip(x) and torch.is_grad_enabled() \
            and weight.requires_grad:
        x2d = x.reshape(-1, x.shape[-1])
        if _wgrad_eligible(x2d, weight):
            fn = _FullNativeLinear if mode == "full" else _HybridLinear
            y = fn.apply(x2d.contiguous(), weight.contiguous(), bias)
            return y.reshape(*x.shape[:-1], weight.shape[0])
    if use_hip(x) and torch.is_grad_enabled() \
            and not torch.is_autocast_enabled():
        rows = x.numel() // x.shape[-1]
        if weight.requires_grad and _native_wgrad_enabled() \
                and x.dtype == weight.dtype == torch.bfloat16 \
                and (bias is None or bias.dtype == torch.bfloat16) \
                and _native_wgrad_rule(rows, weight.shape[0], weight.shape[1]):
            return _DefaultLinear.apply(x, weight, bias, True)
        if bias is not None and bias.requires_grad and _bias_grad_enabled() \
                and x.dtype == weight.dtype == bias.dtype \
                and x.dtype in (torch.bfloat16, torch.float16, torch.float32) \
                and rows >= _BIAS_GRAD_MIN_ROWS:
            return _DefaultLinear.apply(x, weight, bias, False)
    return F.linear(x, weight, bias)


class DcrLinear(nn.Linear):
    """nn.Linear routing through dcr_linear (state-dict compatible with
    nn.Linear and so with the diffusers checkpoint naming)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        return dcr_linear(x, self.weight, self.bias)
