"""Split-contraction MFMA weight gradient for the linear layers
(gemm.hip linear_wgrad): dw[N,K] = dy[M,N]^T x[M,K], db[N] = sum_m dy[m,n].

Exact check: integer-valued bf16 inputs in [-3, 3] with M <= 4096 keep every
fp32 partial sum an integer below 2^24 (|sum| <= 9 * 4096), so the fp32
result is exact in any summation order and the kernel must reproduce
ref_fp32.to(bf16) bit for bit. Random check: the suite's _close at 2e-2
against the fp32 product. Operands are the first M rows of larger NaN-filled
buffers, so a read past M shows up as NaN. N != K and the data is not
symmetric, so a transposed result cannot pass."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16

# (M, N, K, forced split; 0 = the launcher's rule)
CASES = [
    (256, 64, 64, 0),        # one tile
    (520, 72, 136, 0),       # ragged M, N and K; K % 8 only
    (2056, 320, 64, 1),
    (2056, 320, 64, 2),
    (2056, 320, 64, 5),      # 17 chunks of 128 rows: slices of 4,4,4,4,1
    (2056, 320, 64, 1000),   # clamped to the 17 chunks
    (1232, 320, 1024, 0),
]


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


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _in_nan_buffer(t):
    """t as the first rows of a larger NaN-filled buffer."""
    M, C = t.shape
    buf = torch.full((M + 300, C), float("nan"), device=t.device, dtype=t.dtype)
    buf[:M] = t
    return buf[:M]


@pytest.mark.parametrize("M,N,K,split", CASES)
@pytest.mark.parametrize("tile", [0, 128])
def test_linear_wgrad_exact(ext, M, N, K, split, tile):
    g = torch.Generator(device="cuda").manual_seed(31)
    dy = _in_nan_buffer(torch.randint(-3, 4, (M, N), device="cuda", generator=g).to(BF16))
    x = _in_nan_buffer(torch.randint(-3, 4, (M, K), device="cuda", generator=g).to(BF16))
    ref_dw = (dy.float().t() @ x.float()).to(BF16)
    ref_db = dy.float().sum(0).to(BF16)

    dw, db = ext.linear_wgrad(dy, x, True, split, tile)
    assert dw.shape == (N, K) and db.shape == (N,) and dw.dtype == BF16
    assert torch.equal(dw, ref_dw)
    assert torch.equal(db, ref_db)
    (dw_only,) = ext.linear_wgrad(dy, x, False, split, tile)
    assert torch.equal(dw_only, ref_dw)


@pytest.mark.parametrize("M,N,K,split", CASES)
def test_linear_wgrad_random(ext, M, N, K, split):
    torch.manual_seed(32)
    dy = _in_nan_buffer(torch.randn(M, N, device="cuda", dtype=BF16) * 0.5)
    x = _in_nan_buffer(torch.randn(M, K, device="cuda", dtype=BF16) * 0.1 + 0.05)
    dw, db = ext.linear_wgrad(dy, x, True, split)
    _close(dw, dy.float().t() @ x.float(), 2e-2)
    _close(db, dy.float().sum(0), 2e-2)
    # plain stores and an ordered reduction: bit-reproducible
    dw2, db2 = ext.linear_wgrad(dy, x, True, split)
    assert _bits_equal(dw, dw2) and _bits_equal(db, db2)


def _linear_grads(x, w, b, g):
    from dcr_amd.ops.linear import dcr_linear
    for t in (x, w, b):
        if t is not None:
            t.grad = None
    y = dcr_linear(x, w, b)
    y.backward(g)
    return y, x.grad, w.grad, (b.grad if b is not None else None)


@pytest.mark.parametrize("with_bias", [True, False])
def test_dcr_linear_native_wgrad(ext, monkeypatch, with_bias):
    from dcr_amd.ops import dispatch_counts
    from dcr_amd.ops.linear import _native_wgrad_rule
    monkeypatch.delenv("DCR_NATIVE_GEMM", raising=False)
    torch.manual_seed(33)
    B, L, N, K = 2, 2048, 320, 192
    assert _native_wgrad_rule(B * L, N, K)
    x = (torch.randn(B, L, K, device="cuda", dtype=BF16) * 0.5).requires_grad_(True)
    w = (torch.randn(N, K, device="cuda", dtype=BF16) * 0.1).requires_grad_(True)
    b = torch.randn(N, device="cuda", dtype=BF16).requires_grad_(True) \
        if with_bias else None
    g = torch.randn(B, L, N, device="cuda", dtype=BF16)

    monkeypatch.setenv("DCR_NATIVE_WGRAD", "1")
    before = dispatch_counts["linear_wgrad"]
    y, dx, dw, db = _linear_grads(x, w, b, g)
    assert dispatch_counts["linear_wgrad"] == before + 1

    xf = x.detach().float().requires_grad_(True)
    wf = w.detach().float().requires_grad_(True)
    bf = b.detach().float().requires_grad_(True) if with_bias else None
    F.linear(xf, wf, bf).backward(g.float())
    _close(dx, xf.grad, 2e-2)
    _close(dw, wf.grad, 2e-2)
    if with_bias:
        _close(db, bf.grad, 2e-2)

    # switched off: the library's weight gradient, bit for bit
    monkeypatch.setenv("DCR_NATIVE_WGRAD", "0")
    before = dispatch_counts["linear_wgrad"]
    _, dx0, dw0, db0 = _linear_grads(x, w, b, g)
    assert dispatch_counts["linear_wgrad"] == before
    dy2, x2 = g.reshape(-1, N), x.detach().reshape(-1, K)
    assert _bits_equal(dw0, dy2.t() @ x2)
    assert _bits_equal(dx0, dx)
    if with_bias:
        _close(db0, bf.grad, 2e-2)
