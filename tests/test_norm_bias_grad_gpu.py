"""LayerNorm / NHWC GroupNorm backward without aten glue, the conv forward's
bf16 bias, and the native bias-gradient column sums (reduce.hip).

References are plain PyTorch in fp32 on the same (bf16-valued) inputs.
Norm tolerances are those of tests/test_ops_gpu.py. The column-sum bound
per output element is one rounding to the output dtype plus fp32
accumulation: |out - ref| <= 2^-8 |ref| + 1e-5 sum|x| for bf16 (2^-8 is a
bf16 ulp bound; fp32: 1e-6 |ref| + 1e-5 sum|x|)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ext():
    from dcr_amd import ops
    m = ops.ext()
    assert m is not None, "HIP extension must be present on GPU box"
    return m


def _close(out, ref, rtol):
    scale = ref.abs().max().item() + 1e-6
    err = (out.float() - ref.float()).abs().max().item()
    assert err < rtol * scale, f"err={err:.4g} scale={scale:.4g} rtol={rtol}"


def _rel(out, ref):
    return ((out.float() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------- LN backward
@pytest.mark.parametrize("shape", [(1, 320), (5, 52), (33, 320), (515, 640),
                                   (1030, 1280), (9, 2048), (7, 2052)])
@pytest.mark.parametrize("xdt,wdt", [(BF16, BF16), (BF16, F32), (F32, F32)])
def test_layernorm_bwd(ext, shape, xdt, wdt):
    torch.manual_seed(20)
    M, N = shape
    x = torch.randn(M, N, device="cuda").to(xdt)
    dy = torch.randn(M, N, device="cuda").to(xdt)
    w = (torch.randn(N, device="cuda") * 0.5 + 1).to(wdt)
    b = torch.randn(N, device="cuda").to(wdt)

    xr = x.float().requires_grad_(True)
    wr = w.float().requires_grad_(True)
    br = b.float().requires_grad_(True)
    F.layer_norm(xr, (N,), wr, br, 1e-5).backward(dy.float())

    _, mean, rstd = ext.layernorm_fwd(x, w, b, 1e-5)
    dx, dw, db = ext.layernorm_bwd(dy, x, w, mean, rstd)
    assert dx.dtype == xdt and dw.dtype == wdt and db.dtype == wdt
    tol_x, tol_w = (1e-4, 1e-4) if xdt == F32 else (3e-2, 3e-2)
    _close(dx, xr.grad, tol_x)
    rw, rb = _rel(dw, wr.grad), _rel(db, br.grad)
    print(f"ln_bwd {shape} {xdt} {wdt}: rel dw={rw:.3g} db={rb:.3g}")
    assert rw < tol_w and rb < tol_w

    if N <= 2048 and N % 4 == 0:    # v2: slab + fixed-order reduce
        dx2, dw2, db2 = ext.layernorm_bwd(dy, x, w, mean, rstd)
        assert _bits_equal(dx, dx2) and _bits_equal(dw, dw2) and _bits_equal(db, db2)


# ------------------------------------------------------ GN NHWC backward
@pytest.mark.parametrize("shape", [(2, 320, 8, 8, 32), (3, 96, 7, 9, 8),
                                   (1, 1280, 4, 4, 32), (2, 2560, 8, 8, 32)])
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("xdt,wdt", [(BF16, BF16), (BF16, F32), (F32, F32)])
def test_groupnorm_nhwc_bwd(ext, shape, silu, xdt, wdt):
    torch.manual_seed(21)
    N, C, H, W, G = shape
    cl = torch.channels_last
    x = torch.randn(N, C, H, W, device="cuda").to(xdt).contiguous(memory_format=cl)
    dy = torch.randn(N, C, H, W, device="cuda").to(xdt).contiguous(memory_format=cl)
    w = (torch.randn(C, device="cuda") * 0.5 + 1).to(wdt)
    b = (torch.randn(C, device="cuda") * 0.1).to(wdt)

    xr = x.float().contiguous().requires_grad_(True)
    wr = w.float().requires_grad_(True)
    br = b.float().requires_grad_(True)
    ref = F.group_norm(xr, G, wr, br, 1e-5)
    if silu:
        ref = F.silu(ref)
    ref.backward(dy.float().contiguous())

    _, mean, rstd = ext.groupnorm_silu_nhwc_fwd(x, w, b, G, 1e-5, silu)
    dx, dw, db = ext.groupnorm_silu_nhwc_bwd(dy, x, w, b, mean, rstd, G, silu)
    assert dw.dtype == wdt and db.dtype == wdt and dx.dtype == xdt
    atol_x, tol_w = (1e-4, 1e-4) if xdt == F32 else (5e-2, 3e-2)
    ex = (dx.float() - xr.grad).abs().max().item()
    rw, rb = _rel(dw, wr.grad), _rel(db, br.grad)
    print(f"gn_bwd {shape} silu={silu} {xdt} {wdt}: dx={ex:.3g} dw={rw:.3g} db={rb:.3g}")
    assert ex < atol_x
    assert rw < tol_w and rb < tol_w

    dx2, dw2, db2 = ext.groupnorm_silu_nhwc_bwd(dy, x, w, b, mean, rstd, G, silu)
    assert _bits_equal(dx, dx2) and _bits_equal(dw, dw2) and _bits_equal(db, db2)


# ------------------------------------------------------- conv forward bias
def _small_ints(lo, hi, *shape):
    """Integer-valued bf16: every product and partial sum of the convs below
    is exact in fp32, so split-K atomics and the library's split weight
    gradient give the same bits in any summation order and a bit comparison
    sees only what the test is about."""
    return torch.randint(lo, hi + 1, shape, device="cuda").to(BF16)


def _conv_inputs(N, C, H, K):
    torch.manual_seed(22)
    cl = torch.channels_last
    x = _small_ints(-2, 2, N, C, H, H).contiguous(memory_format=cl)
    w = _small_ints(-1, 1, K, C, 3, 3).contiguous(memory_format=cl)
    bias = torch.randn(K, device="cuda", dtype=BF16)
    res = torch.randn(N, K, H, H, device="cuda", dtype=BF16).contiguous(memory_format=cl)
    temb = torch.randn(N, K, device="cuda", dtype=BF16)
    return x, w, bias, res, temb


@pytest.mark.parametrize("shape", [(2, 64, 8, 64), (16, 320, 32, 320)])
@pytest.mark.parametrize("fused", [False, True])
def test_conv_fwd_bf16_bias_bit_identical(ext, shape, fused):
    x, w, bias, res, temb = _conv_inputs(*shape)
    r, t = (res, temb) if fused else (None, None)
    y_bf = ext.conv2d_nhwc_fwd_v2(x, w, bias, 1, 1, r, t)
    y_f32 = ext.conv2d_nhwc_fwd_v2(x, w, bias.float(), 1, 1, r, t)
    assert _bits_equal(y_bf, y_f32)


# ------------------------------------------------------------- column sums
def _colsum_check(out, x2d_f32, dtype):
    """out [C] against the fp32 column sum of x2d_f32 [rows, C]"""
    ref = x2d_f32.sum(0)
    sabs = x2d_f32.abs().sum(0)
    r = 2.0 ** -8 if dtype == BF16 else 1e-6
    bound = r * ref.abs() + 1e-5 * sabs
    err = (out.float() - ref).abs()
    worst = (err - bound).max().item()
    assert worst <= 0, f"column-sum bound missed by {worst:.4g}"


@pytest.mark.parametrize("rows", [1, 7, 130, 4099])
@pytest.mark.parametrize("C", [8, 320, 1288])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_colsum(ext, rows, C, dtype):
    torch.manual_seed(23)
    x = torch.randn(rows, C, device="cuda").to(dtype)
    out = ext.colsum(x)
    assert out.dtype == dtype and out.shape == (C,)
    _colsum_check(out, x.float(), dtype)
    assert _bits_equal(out, ext.colsum(x))


@pytest.mark.parametrize("HW", [1, 16, 65])
@pytest.mark.parametrize("K", [64, 320])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_colsum_grouped(ext, HW, K, dtype):
    torch.manual_seed(24)
    N = 3
    x = torch.randn(N, HW, K, device="cuda").to(dtype)
    out_n, out = ext.colsum_grouped(x)
    assert out_n.dtype == dtype and out_n.shape == (N, K) and out.shape == (K,)
    for n in range(N):
        _colsum_check(out_n[n], x[n].float(), dtype)
    # [C]: fp32 sum over n of the unrounded per-sample sums
    ref = x.float().sum(1).sum(0)
    sabs = x.float().abs().sum((0, 1))
    r = 2.0 ** -8 if dtype == BF16 else 1e-6
    assert ((out.float() - ref).abs() - (r * ref.abs() + 1e-5 * sabs)).max().item() <= 0
    out_n2, out2 = ext.colsum_grouped(x)
    assert _bits_equal(out_n, out_n2) and _bits_equal(out, out2)


# --------------------------------------------------------- autograd wiring
def _grads(module, inputs, g, extra=()):
    for p in list(module.parameters()) + list(inputs) + list(extra):
        p.grad = None
    y = module(*inputs) if not extra else module(inputs[0], res=extra[0], temb=extra[1])
    (y * g).sum().backward()
    out = [p.grad.clone() for p in module.parameters()]
    out += [t.grad.clone() for t in list(inputs) + list(extra)]
    return out


def test_linear_bias_grad_wiring(monkeypatch):
    from dcr_amd import ops
    from dcr_amd.ops.linear import DcrLinear
    torch.manual_seed(25)
    lin = DcrLinear(320, 640).to("cuda", BF16)
    x = torch.randn(2, 33, 320, device="cuda", dtype=BF16, requires_grad=True)
    g = torch.randn(2, 33, 640, device="cuda", dtype=BF16)

    monkeypatch.setenv("DCR_NATIVE_BIAS_GRAD", "0")
    dw0, db0, dx0 = _grads(lin, [x], g)
    monkeypatch.setenv("DCR_NATIVE_BIAS_GRAD", "1")
    before = ops.dispatch_counts["bias_grad"]
    dw1, db1, dx1 = _grads(lin, [x], g)
    assert ops.dispatch_counts["bias_grad"] == before + 1
    assert _bits_equal(dw0, dw1) and _bits_equal(dx0, dx1)
    g2 = g.float().reshape(-1, 640)      # dy of (y * g).sum() is g
    _colsum_check(db1, g2, BF16)
    _colsum_check(db0, g2, BF16)


def test_conv_bias_grad_wiring(monkeypatch):
    from dcr_amd import ops
    from dcr_amd.ops.conv import Conv2d
    torch.manual_seed(26)
    cl = torch.channels_last
    conv = Conv2d(64, 64, 3, padding=1).to("cuda", BF16).to(memory_format=cl)
    with torch.no_grad():       # exact sums: see _small_ints
        conv.weight.copy_(_small_ints(-1, 1, 64, 64, 3, 3))
    x = _small_ints(-2, 2, 2, 64, 8, 8).contiguous(
        memory_format=cl).requires_grad_(True)
    res = torch.randn(2, 64, 8, 8, device="cuda", dtype=BF16).contiguous(
        memory_format=cl).requires_grad_(True)
    temb = torch.randn(2, 64, device="cuda", dtype=BF16, requires_grad=True)
    g = _small_ints(-2, 2, 2, 64, 8, 8).contiguous(memory_format=cl)

    monkeypatch.setenv("DCR_NATIVE_BIAS_GRAD", "0")
    dw0, db0, dx0, dr0, dt0 = _grads(conv, [x], g, (res, temb))
    monkeypatch.setenv("DCR_NATIVE_BIAS_GRAD", "1")
    before = ops.dispatch_counts["bias_grad"]
    dw1, db1, dx1, dr1, dt1 = _grads(conv, [x], g, (res, temb))
    assert ops.dispatch_counts["bias_grad"] == before + 1
    assert _bits_equal(dw0, dw1) and _bits_equal(dx0, dx1) and _bits_equal(dr0, dr1)
    # bias terms (dbias, and d_temb = the per-sample bias): column-sum bound
    g3 = g.float().permute(0, 2, 3, 1).reshape(2, 64, 64)   # [N, HW, K]
    for n in range(2):
        _colsum_check(dt1[n], g3[n], BF16)
        _colsum_check(dt0[n], g3[n], BF16)
    _colsum_check(db1, g3.reshape(-1, 64), BF16)
    _colsum_check(db0, g3.reshape(-1, 64), BF16)


# ------------------------------------------------------------ launch counts
def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    from torch.autograd import DeviceType
    fn()                                  # warm: module load, allocator
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]


def _no_glue(names):
    assert not [n for n in names if "FillFunctor" in n or "copy_kernel" in n], names


def test_launch_counts(ext):
    torch.manual_seed(27)
    x = torch.randn(515, 640, device="cuda", dtype=BF16)
    dy = torch.randn_like(x)
    w = torch.randn(640, device="cuda", dtype=BF16)
    b = torch.randn(640, device="cuda", dtype=BF16)
    _, mean, rstd = ext.layernorm_fwd(x, w, b, 1e-5)
    names = _device_kernels(lambda: ext.layernorm_bwd(dy, x, w, mean, rstd))
    print("layernorm_bwd:", names)
    assert len(names) <= 2
    _no_glue(names)

    cl = torch.channels_last
    gx = torch.randn(2, 320, 8, 8, device="cuda", dtype=BF16).contiguous(memory_format=cl)
    gdy = torch.randn_like(gx)
    gw = torch.randn(320, device="cuda", dtype=BF16)
    gb = torch.randn(320, device="cuda", dtype=BF16)
    _, gm, gr = ext.groupnorm_silu_nhwc_fwd(gx, gw, gb, 32, 1e-5, True)
    names = _device_kernels(
        lambda: ext.groupnorm_silu_nhwc_bwd(gdy, gx, gw, gb, gm, gr, 32, True))
    print("groupnorm_silu_nhwc_bwd:", names)
    assert len(names) <= 3
    _no_glue(names)

    cx, cw, cb, _, _ = _conv_inputs(16, 320, 32, 320)
    names = _device_kernels(lambda: ext.conv2d_nhwc_fwd_v2(cx, cw, cb, 1, 1))
    print("conv2d_nhwc_fwd_v2:", names)
    assert len(names) == 1
    _no_glue(names)
