"""Functional op wrappers: HIP kernels on GPU, PyTorch reference on CPU.

Each op corresponds to a fused hot spot of the SD-2.1 finetune / sampling
loop the reference runs through libraries:

* ``group_norm_silu``  — every ResNet-block norm in UNet/VAE
  (reference: diffusers ResnetBlock2D, /root/reference/diff_train.py:644).
* ``layer_norm``       — transformer blocks in UNet + CLIP text encoder.
* ``geglu``            — UNet transformer FeedForward gate.
* ``attention``        — self/cross attention (flash-style HIP kernel).
* ``add_noise`` / ``get_velocity`` — DDPM scheduler math
  (reference: diff_train.py:632,650).
* ``cfg_combine``      — classifier-free guidance in sampling.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import use_hip, require_hip, count_dispatch


# --------------------------------------------------------------------------
# GroupNorm (+ optional fused SiLU)
# --------------------------------------------------------------------------
class _GroupNormSiLUNHWC(torch.autograd.Function):
    """channels_last path: stats/apply kernels over the native NHWC walk
    (dcr_amd/ops/hip/norms_nhwc.hip) — no transpose round-trips."""

    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, apply_silu):
        m = require_hip("group_norm_silu_nhwc")
        count_dispatch('groupnorm_nhwc')
        y, mean, rstd = m.groupnorm_silu_nhwc_fwd(x, weight, bias, num_groups,
                                                  eps, apply_silu)
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        ctx.num_groups = num_groups
        ctx.apply_silu = apply_silu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mean, rstd = ctx.saved_tensors
        m = require_hip("group_norm_silu_nhwc")
        dx, dw, db = m.groupnorm_silu_nhwc_bwd(
            dy.contiguous(memory_format=torch.channels_last), x, weight, bias,
            mean, rstd, ctx.num_groups, ctx.apply_silu)
        return dx, dw, db, None, None, None


class _GroupNormSiLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, apply_silu):
        m = require_hip("group_norm_silu")
        if m is None:  # debug fallback on GPU
            return _gn_silu_ref(x, weight, bias, num_groups, eps, apply_silu)
        count_dispatch('groupnorm')
        y, mean, rstd = m.groupnorm_silu_fwd(x, weight, bias, num_groups, eps, apply_silu)
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        ctx.num_groups = num_groups
        ctx.apply_silu = apply_silu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mean, rstd = ctx.saved_tensors
        m = require_hip("group_norm_silu")
        dx, dw, db = m.groupnorm_silu_bwd(
            dy.contiguous(), x, weight, bias, mean, rstd, ctx.num_groups, ctx.apply_silu
        )
        return dx, dw, db, None, None, None


def _gn_silu_ref(x, weight, bias, num_groups, eps, apply_silu):
    # fp32 accumulation regardless of input dtype (matches HIP kernel numerics)
    y = F.group_norm(x.float(), num_groups, weight.float(), bias.float(), eps)
    if apply_silu:
        y = F.silu(y)
    return y.to(x.dtype)


def group_norm_silu(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    num_groups: int = 32,
    eps: float = 1e-5,
    apply_silu: bool = True,
) -> torch.Tensor:
    if use_hip(x):
        if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) \
                and not x.is_contiguous() and x.shape[1] % 4 == 0:
            return _GroupNormSiLUNHWC.apply(x, weight, bias, num_groups, eps,
                                            apply_silu)
        return _GroupNormSiLU.apply(x.contiguous(), weight, bias, num_groups, eps, apply_silu)
    return _gn_silu_ref(x, weight, bias, num_groups, eps, apply_silu)


# --------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        m = require_hip("layer_norm")
        if m is None:
            return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)
        count_dispatch('layernorm')
        y, mean, rstd = m.layernorm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        m = require_hip("layer_norm")
        dx, dw, db = m.layernorm_bwd(dy.contiguous(), x, weight, mean, rstd)
        return dx, dw, db, None


def layer_norm(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    eps: float = 1e-5,
) -> torch.Tensor:
    if use_hip(x):
        return _LayerNorm.apply(x.contiguous(), weight, bias, eps)
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


# --------------------------------------------------------------------------
# GEGLU: out = a * gelu(g) with [a, g] = split(x, 2, dim=-1)
# --------------------------------------------------------------------------
class _GEGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        m = require_hip("geglu")
        if m is None:
            a, g = x.chunk(2, dim=-1)
            return a * F.gelu(g)
        count_dispatch('geglu')
        y = m.geglu_fwd(x)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        m = require_hip("geglu")
        return m.geglu_bwd(dy.contiguous(), x)


def geglu(x: torch.Tensor) -> torch.Tensor:
    """x[..., :N] * gelu(x[..., N:]) — exact (erf) GELU."""
    if use_hip(x):
        return _GEGLU.apply(x.contiguous())
    a, g = x.chunk(2, dim=-1)
    return a * F.gelu(g)


# --------------------------------------------------------------------------
# Attention (hand-written CDNA4 flash kernel). q,k,v: [B, H, L, D].
# --------------------------------------------------------------------------
class _FlashAttention(torch.autograd.Function):
    """bf16 flash attention, head_dim 64 (dcr_amd/ops/hip/attention.hip)."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal):
        m = require_hip("attn")
        count_dispatch('attention')
        # schedule dispatch (measured, gpurun_out/r02c7): the swapped-QK^T
        # in-register-softmax v4 wins at Lq >= 256 (1.17x @256, 1.27x
        # @1024, 1.73x @4096 vs v1); the 64x64-tile v1 stays for short
        # sequences and CLIP's causal 77. v4's LSE is bit-identical so
        # the shared FlashAttention-2 backward applies to both.
        # DCR_ATTN_V2/V3: env-gated draft schedules (A/B only).
        if os.environ.get("DCR_ATTN_V3") == "1":
            fwd = m.attn_fwd_v3
        elif os.environ.get("DCR_ATTN_V2") == "1":
            fwd = m.attn_fwd_v2
        elif q.shape[1] >= 256 and os.environ.get("DCR_ATTN_V4", "1") != "0":
            fwd = m.attn_fwd_v4
        else:
            fwd = m.attn_fwd
        o, lse = fwd(q, k, v, scale, causal)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        ctx.causal = causal
        return o

    @staticmethod
    def backward(ctx, dO):
        q, k, v, o, lse = ctx.saved_tensors
        m = require_hip("attn")
        # measured dispatch (gpurun_out/r02c16): the swapped-operand v4
        # backward wins for self-attention (1.27x @256, 1.13x @1024,
        # 1.56x @4096 vs v1) and loses at tiny L / 77-token cross-attn
        # where its 256-row blocks starve. DCR_ATTN_BWD_V4=0/1 overrides.
        env = os.environ.get("DCR_ATTN_BWD_V4", "")
        use_v4 = (env == "1") if env in ("0", "1") \
            else (q.shape[1] >= 256 and k.shape[1] >= 256)
        bwd = m.attn_bwd_v4 if use_v4 else m.attn_bwd
        dQ, dK, dV = bwd(q, k, v, o, dO.contiguous(), lse,
                         ctx.scale, ctx.causal)
        return dQ, dK, dV, None, None


class _FlashAttentionGen(torch.autograd.Function):
    """bf16 flash attention for the SD-1.x head dims 40/80/160 with grad
    (attn_fwd_gen_kernel + attn_bwd_*_gen_kernel in attention.hip).
    q,k,v: [B, L, H, D] or packed [BH, L, D], contiguous."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal):
        m = require_hip("attn_gen")
        count_dispatch('attention_gen')
        o, lse = m.attn_fwd_gen_lse(q, k, v, scale, causal)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        ctx.causal = causal
        return o

    @staticmethod
    def backward(ctx, dO):
        q, k, v, o, lse = ctx.saved_tensors
        m = require_hip("attn_gen_bwd")
        count_dispatch('attention_gen_bwd')
        dQ, dK, dV = m.attn_bwd_gen(q, k, v, o, dO.contiguous(), lse,
                                    ctx.scale, ctx.causal)
        return dQ, dK, dV, None, None


def _attention_math(q, k, v, scale, causal):
    """Composite path (rocBLAS GEMMs + native softmax) for shapes no HIP
    kernel covers: fp32 inputs, the tiny config's D=32, D=512 when causal
    or with grad (the VAE's frozen no-grad head has attn_fwd_d512; here
    only under DCR_ATTN_D512=0) and 40/80/160 with grad under
    DCR_ATTN_GEN_BWD=0. No Triton."""
    count_dispatch('attention_math')
    s = (q.float() @ k.float().transpose(-2, -1)) * scale
    if causal:
        Lq, Lk = q.shape[-2], k.shape[-2]
        mask = torch.ones(Lq, Lk, dtype=torch.bool, device=q.device).tril_()
        s = s.masked_fill(~mask, float("-inf"))
    p = s.softmax(dim=-1)
    return (p @ v.float()).to(q.dtype)


def attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool = False,
    scale: Optional[float] = None,
    layout: str = "bhld",
) -> torch.Tensor:
    """layout "bhld": q,k,v are [B, H, L, D]. layout "blhd": [B, L, H, D] —
    the transpose-free layout the models use (the flash kernel walks it
    with a strided row pitch, so no head-split permute copies happen)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if use_hip(q):
        if q.dtype == torch.bfloat16 and q.shape[-1] == 64 and k.shape[-1] == 64:
            if layout == "blhd":
                return _FlashAttention.apply(q.contiguous(), k.contiguous(),
                                             v.contiguous(), scale, causal)
            shp = q.shape
            out = _FlashAttention.apply(
                q.reshape(-1, shp[-2], 64).contiguous(),
                k.reshape(-1, k.shape[-2], 64).contiguous(),
                v.reshape(-1, v.shape[-2], 64).contiguous(),
                scale, causal)
            return out.reshape(shp)
        needs_grad = torch.is_grad_enabled() and (
            q.requires_grad or k.requires_grad or v.requires_grad)
        if q.dtype == torch.bfloat16 and q.shape[-1] in (40, 80, 160) \
                and k.shape[-1] == q.shape[-1] \
                and not (needs_grad and
                         os.environ.get("DCR_ATTN_GEN_BWD", "1") == "0"):
            # SD-1.x head dims: sampling (sd_mitigation / diff_inference)
            # runs the forward kernel without an LSE; with grad the same
            # kernel writes the LSE and the gen backward kernels follow.
            # No length threshold: fwd+bwd measured 3.5-6.4x the composite
            # path at every SD-1.4 bs-16 training shape, 16x16 to 4096x4096
            # (profiles/r05_attn_gen_bwd.log). DCR_ATTN_GEN_BWD=0 sends the
            # grad case to the composite path (A/B in one process).
            if needs_grad:
                fwd = lambda a, b, c: _FlashAttentionGen.apply(a, b, c, scale, causal)
            else:
                m = require_hip("attn_gen")
                count_dispatch('attention_gen')
                fwd = lambda a, b, c: m.attn_fwd_gen(a, b, c, scale, causal)
            if layout == "blhd":
                return fwd(q.contiguous(), k.contiguous(), v.contiguous())
            d = q.shape[-1]
            shp = q.shape
            out = fwd(q.reshape(-1, shp[-2], d).contiguous(),
                      k.reshape(-1, k.shape[-2], d).contiguous(),
                      v.reshape(-1, v.shape[-2], d).contiguous())
            return out.reshape(shp)
        if q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 \
                and v.dtype == torch.bfloat16 \
                and q.shape[-1] == 512 and k.shape[-1] == 512 \
                and v.shape == k.shape \
                and not causal and not needs_grad \
                and os.environ.get("DCR_ATTN_D512", "1") != "0":
            # the VAE mid-block's single 512-d head (frozen VAE: forward
            # only). DCR_ATTN_D512=0 restores the composite path, read per
            # call so one process can A/B.
            m = require_hip("attn_d512")
            count_dispatch('attention_d512')
            if layout == "blhd":
                return m.attn_fwd_d512(q.contiguous(), k.contiguous(),
                                       v.contiguous(), scale)
            shp = q.shape
            out = m.attn_fwd_d512(q.reshape(-1, shp[-2], 512).contiguous(),
                                  k.reshape(-1, k.shape[-2], 512).contiguous(),
                                  v.reshape(-1, v.shape[-2], 512).contiguous(),
                                  scale)
            return out.reshape(shp)
        if layout == "blhd":
            out = _attention_math(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                                  v.permute(0, 2, 1, 3), scale, causal)
            return out.permute(0, 2, 1, 3)
        return _attention_math(q, k, v, scale, causal)
    if layout == "blhd":
        out = F.scaled_dot_product_attention(
            q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3),
            is_causal=causal, scale=scale)
        return out.permute(0, 2, 1, 3)
    return F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=scale)


# --------------------------------------------------------------------------
# Diffusion scheduler math (no autograd needed: inputs are leaves w/o grad)
# --------------------------------------------------------------------------
def _gather_sqrt(alphas_cumprod: torch.Tensor, t: torch.Tensor, ndim: int):
    ac = alphas_cumprod.to(torch.float32).gather(0, t)
    shape = [t.shape[0]] + [1] * (ndim - 1)
    sqrt_ac = ac.sqrt().view(shape)
    sqrt_1mac = (1.0 - ac).sqrt().view(shape)
    return sqrt_ac, sqrt_1mac


def add_noise(
    x0: torch.Tensor, noise: torch.Tensor, alphas_cumprod: torch.Tensor, t: torch.Tensor
) -> torch.Tensor:
    """x_t = sqrt(ac_t) x0 + sqrt(1-ac_t) noise, per-sample t."""
    from . import ext

    m = ext()
    if use_hip(x0) and m is not None:
        count_dispatch('add_noise')
        ac = alphas_cumprod if (alphas_cumprod.device == x0.device and
                                alphas_cumprod.dtype == torch.float32) \
            else alphas_cumprod.to(x0.device, torch.float32)
        return m.add_noise(x0.contiguous(), noise.contiguous(), ac,
                           t.contiguous())
    sa, sb = _gather_sqrt(alphas_cumprod.to(x0.device), t, x0.dim())
    return (sa * x0.float() + sb * noise.float()).to(x0.dtype)


def get_velocity(
    x0: torch.Tensor, noise: torch.Tensor, alphas_cumprod: torch.Tensor, t: torch.Tensor
) -> torch.Tensor:
    """v = sqrt(ac_t) noise - sqrt(1-ac_t) x0 (v-prediction target)."""
    from . import ext

    m = ext()
    if use_hip(x0) and m is not None:
        ac = alphas_cumprod if (alphas_cumprod.device == x0.device and
                                alphas_cumprod.dtype == torch.float32) \
            else alphas_cumprod.to(x0.device, torch.float32)
        return m.get_velocity(x0.contiguous(), noise.contiguous(), ac,
                              t.contiguous())
    sa, sb = _gather_sqrt(alphas_cumprod.to(x0.device), t, x0.dim())
    return (sa * noise.float() - sb * x0.float()).to(x0.dtype)


def _dense(t: torch.Tensor) -> bool:
    """dense (no holes) in ANY layout — elementwise kernels walk raw memory."""
    if t.is_contiguous():
        return True
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)


def lincomb(x: torch.Tensor, y: torch.Tensor, a: float, b: float,
            z: Optional[torch.Tensor] = None, c: float = 0.0) -> torch.Tensor:
    """out = a*x + b*y (+ c*z) — one fused HIP kernel; the DDIM and
    DPM-Solver++ sampler updates are expressed through this."""
    from . import ext

    m = ext()
    if use_hip(x) and m is not None and x.numel() % 4 == 0 \
            and _dense(x) and x.stride() == y.stride() \
            and (z is None or z.stride() == x.stride()):
        count_dispatch('lincomb')
        return m.lincomb(x, y, z, float(a), float(b), float(c))
    out = a * x.float() + b * y.float()
    if z is not None:
        out = out + c * z.float()
    return out.to(x.dtype)


# --------------------------------------------------------------------------
# Patch max-similarity (split-product retrieval, stype="cross")
# --------------------------------------------------------------------------
def _bf16_split(x: torch.Tensor):
    """x (fp32) as hi + lo with both in bf16: hi = bf16(x), lo = bf16(x - hi).
    hi + lo carries 16 significand bits of x."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def _maxsim_operand(x: torch.Tensor, precision: str, side: str) -> torch.Tensor:
    """The bf16 [rows, patches, K'] operand the kernel contracts.

    "bf16": x rounded to bf16, K' = C. "high": the K-concatenation
    [hi | hi | lo] for side "a" and [hi | lo | hi] for side "b", K' = 3C, so
    one fp32-accumulating product sums hi.hi + hi.lo + lo.hi. C is padded
    with zeros to a multiple of 8 first."""
    pad = -x.shape[-1] % 8
    if precision == "bf16":
        x = x.to(torch.bfloat16)
        if pad:
            x = F.pad(x, (0, pad))
        return x.contiguous()
    x = x.float()
    if pad:
        x = F.pad(x, (0, pad))
    hi, lo = _bf16_split(x)
    parts = (hi, hi, lo) if side == "a" else (hi, lo, hi)
    return torch.cat(parts, dim=-1)


def maxsim_operands(a: torch.Tensor, b: torch.Tensor, precision: str = "high"):
    """(A', B') in bf16 as `patch_maxsim` hands them to the kernel."""
    if precision not in ("high", "bf16"):
        raise ValueError(f"precision must be 'high' or 'bf16', not {precision!r}")
    return _maxsim_operand(a, precision, "a"), _maxsim_operand(b, precision, "b")


def _maxsim_ref(a2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """CPU path: fp32 products of the transformed operands, max over patch
    pairs. One row of `a` at a time, so the intermediate is [M*Q, P] and the
    way callers chunk the rows cannot change a bit of the result."""
    n, p, k = a2.shape
    m, q, _ = b2.shape
    bf = b2.float().reshape(m * q, k)
    out = torch.empty(n, m, dtype=torch.float32, device=a2.device)
    for i in range(n):
        s = bf @ a2[i].float().t()               # [M*Q, P]
        out[i] = s.reshape(m, q * p).amax(dim=1)
    return out


def patch_maxsim(a: torch.Tensor, b: torch.Tensor, *, precision: str = "high",
                 chunk: Optional[int] = None) -> torch.Tensor:
    """out[n, m] = max over patch pairs (p, q) of <a[n, p, :], b[m, q, :]>.

    a [N, P, C], b [M, Q, C], any float dtype; returns fp32 [N, M]. On the
    GPU one fused kernel (dcr_amd/ops/hip/maxsim.hip) contracts in bf16 MFMA
    with fp32 accumulation and reduces the scores without storing them.
    precision="bf16" rounds both operands to bf16; "high" (default) contracts
    the bf16 hi/lo split of both (3x the FLOPs, fp32-grade scores). `chunk`
    is the number of rows of `a` per launch (bounds the transformed copy of
    `a`); it does not change the result. CPU tensors take the same operand
    transformation and an fp32 matmul."""
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != b.shape[2]:
        raise ValueError("patch_maxsim: a [N, P, C] and b [M, Q, C] expected, "
                         f"got {tuple(a.shape)} and {tuple(b.shape)}")
    if precision not in ("high", "bf16"):
        raise ValueError(f"precision must be 'high' or 'bf16', not {precision!r}")
    if chunk is not None and chunk < 1:
        raise ValueError("patch_maxsim: chunk must be >= 1")
    n, m = a.shape[0], b.shape[0]
    if n == 0 or m == 0:
        return torch.empty(n, m, dtype=torch.float32, device=a.device)
    if a.shape[1] == 0 or b.shape[1] == 0 or a.shape[2] == 0:
        raise ValueError("patch_maxsim: P, Q and C must be >= 1")
    step = n if chunk is None else chunk
    b2 = _maxsim_operand(b, precision, "b")
    run = _maxsim_ref
    if use_hip(a):
        mod = require_hip("patch_maxsim")
        if mod is not None:  # None: debug fallback on GPU
            count_dispatch('patch_maxsim')
            run = mod.patch_maxsim
    outs = [run(_maxsim_operand(a[i:i + step], precision, "a"), b2)
            for i in range(0, n, step)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


# --------------------------------------------------------------------------
# Split product (split-product retrieval, stype="": aligned chunks / patches)
# --------------------------------------------------------------------------
def split_product_operands(a: torch.Tensor, b: torch.Tensor,
                           precision: str = "high"):
    """(A', B') in bf16 as `split_product` hands them to the kernel: the
    `patch_maxsim` transformation of every group's last dim, [N, G, L']."""
    return maxsim_operands(a, b, precision)


def _split_ref(a2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """CPU path: fp32 products of the transformed operands, max over groups.
    One row of `a` at a time (a batched matrix-vector product over the
    groups), so the way callers chunk the rows cannot change a bit."""
    n = a2.shape[0]
    bf = b2.float().transpose(0, 1)                  # [G, M, L']
    out = torch.empty(n, b2.shape[0], dtype=torch.float32, device=a2.device)
    for i in range(n):
        s = torch.bmm(bf, a2[i].float().unsqueeze(2))    # [G, M, 1]
        out[i] = s.squeeze(2).amax(dim=0)
    return out


def split_product(a: torch.Tensor, b: torch.Tensor, *, precision: str = "high",
                  chunk: Optional[int] = None) -> torch.Tensor:
    """out[n, m] = max over groups g of <a[n, g, :], b[m, g, :]>.

    a [N, G, L], b [M, G, L], any float dtype and strides; returns fp32
    [N, M]. G chunks of a flat embedding (L = D / G) or G patches of L
    channels. On the GPU one fused kernel (dcr_amd/ops/hip/splitsim.hip)
    contracts group by group in bf16 MFMA with fp32 accumulation and keeps
    the running max in registers: the [N, M, G] block is never stored.
    `precision` and `chunk` are `patch_maxsim`'s: "bf16" rounds both
    operands, "high" (default) contracts their bf16 hi/lo split; `chunk` is
    the number of rows of `a` per launch (bounds the transformed copy of
    `a`) and does not change the result. CPU tensors take the same operand
    transformation and fp32 products. A NaN group score is dropped by the
    kernel's max unless all of an entry's groups are NaN; non-finite inputs
    are outside the contract."""
    if a.dim() != 3 or b.dim() != 3 or a.shape[1:] != b.shape[1:]:
        raise ValueError("split_product: a [N, G, L] and b [M, G, L] expected, "
                         f"got {tuple(a.shape)} and {tuple(b.shape)}")
    if precision not in ("high", "bf16"):
        raise ValueError(f"precision must be 'high' or 'bf16', not {precision!r}")
    if chunk is not None and chunk < 1:
        raise ValueError("split_product: chunk must be >= 1")
    n, m = a.shape[0], b.shape[0]
    if n == 0 or m == 0:
        return torch.empty(n, m, dtype=torch.float32, device=a.device)
    if a.shape[1] == 0 or a.shape[2] == 0:
        raise ValueError("split_product: G and L must be >= 1")
    step = n if chunk is None else chunk
    b2 = _maxsim_operand(b, precision, "b")
    run = _split_ref
    if use_hip(a):
        mod = require_hip("split_product")
        if mod is not None:  # None: debug fallback on GPU
            count_dispatch('split_product')
            run = mod.split_product
    outs = [run(_maxsim_operand(a[i:i + step], precision, "a"), b2)
            for i in range(0, n, step)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


# --------------------------------------------------------------------------
# Top-k similarity search (embedding search)
# --------------------------------------------------------------------------
TOPK_SIM_MAX_K = 16   # list capacity of the fused kernel


def topk_sim_operands(q: torch.Tensor, x: torch.Tensor, precision: str = "high"):
    """(Q', X') in bf16 as `topk_sim` hands them to the kernel."""
    if precision not in ("high", "bf16"):
        raise ValueError(f"precision must be 'high' or 'bf16', not {precision!r}")
    return _maxsim_operand(q, precision, "a"), _maxsim_operand(x, precision, "b")


def _topk_sim_ref(q2: torch.Tensor, x2: torch.Tensor, k: int):
    """CPU path: fp32 products of the transformed operands, then the ordering
    rule: higher score first, the lower index first among equal scores, NaN
    never taken. Columns are in index order already, so one stable descending
    sort is the stable-by-index-then-stable-by-score order."""
    xf = x2.float()
    vals, idxs = [], []
    for i in range(0, q2.shape[0], 1024):
        s = q2[i:i + 1024].float() @ xf.t()
        s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
        v, ix = torch.sort(s, dim=1, descending=True, stable=True)
        vals.append(v[:, :k].contiguous())
        idxs.append(ix[:, :k].contiguous())
    return torch.cat(vals, dim=0), torch.cat(idxs, dim=0)


def topk_sim(q: torch.Tensor, x: torch.Tensor, k: int, *,
             precision: str = "bf16"):
    """The k best rows of x for every row of q by dot product.

    q [Nq, D], x [Nx, D], any float dtype; returns (scores fp32 [Nq, k],
    idx int64 [Nq, k]), higher score first and the lower index first among
    equal scores; a NaN score is never returned. On the GPU one fused kernel
    (dcr_amd/ops/hip/topk_sim.hip) contracts in bf16 MFMA with fp32
    accumulation and keeps the k best per row in registers: the [Nq, Nx]
    score matrix is never stored, and the result does not depend on how the
    caller chunks the query rows. precision="bf16" rounds both operands to
    bf16; "high" contracts the bf16 hi/lo split of both (3x the FLOPs,
    fp32-grade scores). The kernel holds k <= 16. CPU tensors take the same
    operand transformation and an fp32 matmul."""
    if q.dim() != 2 or x.dim() != 2 or q.shape[1] != x.shape[1] \
            or q.shape[1] == 0:
        raise ValueError("topk_sim: q [Nq, D] and x [Nx, D] with D >= 1 "
                         f"expected, got {tuple(q.shape)} and {tuple(x.shape)}")
    if precision not in ("high", "bf16"):
        raise ValueError(f"precision must be 'high' or 'bf16', not {precision!r}")
    k = int(k)
    if k < 1:
        raise ValueError("topk_sim: k must be >= 1")
    if k > x.shape[0]:
        raise ValueError(f"topk_sim: k = {k} exceeds the {x.shape[0]} index rows")
    if q.shape[0] == 0:
        return (torch.empty(0, k, dtype=torch.float32, device=q.device),
                torch.empty(0, k, dtype=torch.long, device=q.device))
    if use_hip(q):
        if k > TOPK_SIM_MAX_K:
            raise ValueError(
                f"topk_sim: the fused kernel holds k <= {TOPK_SIM_MAX_K}, got "
                f"{k}; callers fall back to the library path (matmul + topk)")
        mod = require_hip("topk_sim")
        if mod is not None:  # None: debug fallback on GPU
            count_dispatch('topk_sim')
            scores, idx = mod.topk_sim(_maxsim_operand(q, precision, "a"),
                                       _maxsim_operand(x, precision, "b"), k)
            return scores, idx
    return _topk_sim_ref(_maxsim_operand(q, precision, "a"),
                         _maxsim_operand(x, precision, "b"), k)


def cfg_combine(eps_uncond: torch.Tensor, eps_text: torch.Tensor, scale: float) -> torch.Tensor:
    """Classifier-free guidance: eps_u + s * (eps_t - eps_u)."""
    from . import ext

    m = ext()
    if use_hip(eps_uncond) and m is not None \
            and eps_uncond.stride() == eps_text.stride() \
            and _dense(eps_uncond):
        return m.cfg_combine(eps_uncond, eps_text, float(scale))
    return eps_uncond + scale * (eps_text - eps_uncond)
