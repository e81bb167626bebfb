"""Fused patch max-similarity kernel (dcr_amd/ops/hip/maxsim.hip).

Kernel checks compare against the fp64 einsum of the SAME bf16 operands the
kernel is handed (rounded, or hi/lo-concatenated). A bf16 x bf16 product is
exact in fp32, so only the fp32 accumulation differs: K' * 2^-23 for
unit-norm rows, K' the contracted length. End-to-end checks compare against
the fp64 einsum of the original fp32 inputs with the CPU-test bounds
(tests/test_maxsim_cpu.py)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (N, M, P, Q, C)
SHAPES = [
    (5, 7, 49, 49, 64),       # segments straddle every tile boundary, ragged tails
    (4, 6, 3, 5, 96),         # P != Q
    (2, 3, 7, 7, 72),         # C % 8 == 0 only: MFMA and BK contraction tails
    (7, 9, 49, 49, 256),      # 343 x 441 scores: several tiles both ways
    (2, 2, 196, 196, 768),    # ViT-B/16 patch grid
    (3, 3, 49, 49, 2048),     # SSCD trunk width, long contraction
    (1, 1, 1, 1, 8),          # minimum
    (300, 2, 1, 1, 64),       # P = Q = 1: one segment per score
]


@pytest.fixture(scope="module")
def ops():
    from dcr_amd import ops as o
    assert o.ext() is not None, "HIP extension must be present on GPU box"
    return o


def _unit(n, p, c, seed):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(n, p, c, generator=g), dim=-1).to(DEV)


def _ref64(a, b):
    """fp64 max over patch pairs, one row of a at a time (bounded memory)."""
    bd = b.double()
    return torch.stack([torch.einsum("pc,mqc->mpq", x.double(), bd).amax((1, 2))
                        for x in a])


def _kernel(ops, a2, b2):
    """The kernel alone: bf16 operands pass through precision='bf16' as is."""
    assert a2.dtype == torch.bfloat16 and b2.dtype == torch.bfloat16
    return ops.patch_maxsim(a2, b2, precision="bf16")


@pytest.mark.parametrize("precision", ["bf16", "high"])
@pytest.mark.parametrize("N,M,P,Q,C", SHAPES)
def test_kernel_vs_fp64_of_same_operands(ops, N, M, P, Q, C, precision):
    from dcr_amd.ops.functional import maxsim_operands
    a, b = _unit(N, P, C, 1), _unit(M, Q, C, 2)
    a2, b2 = maxsim_operands(a, b, precision)
    out = _kernel(ops, a2, b2)
    assert out.dtype == torch.float32 and out.shape == (N, M)
    tol = a2.shape[-1] * 2.0 ** -23
    err = (out.double() - _ref64(a2, b2)).abs().max().item()
    print(f"{precision} {(N, M, P, Q, C)}: K'={a2.shape[-1]} err={err:.3e} "
          f"tol={tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("N,M,P,Q,C", [(5, 7, 49, 49, 64), (2, 3, 7, 7, 72)])
def test_exact_integers(ops, N, M, P, Q, C):
    """Entries in {-2..2}: every partial sum is a small integer, exact in
    fp32 in any order. A and B are drawn differently (B is mostly
    non-positive), so a row/column swap or a transposed output shows."""
    g = torch.Generator().manual_seed(3)
    a = torch.randint(-2, 3, (N, P, C), generator=g).to(DEV, torch.bfloat16)
    b = torch.randint(-2, 2, (M, Q, C), generator=g).to(DEV, torch.bfloat16)
    out = _kernel(ops, a, b)
    ref = _ref64(a, b)
    assert out.shape == (N, M)
    assert torch.equal(out.double(), ref)


def test_all_negative_scores(ops):
    """Positive a, negative b: every score is < 0, so a padded zero (rows or
    columns past the end, zero-filled staging) reaching a max would show."""
    N, M, P, Q, C = 5, 7, 49, 49, 64
    a = _unit(N, P, C, 4).abs()
    b = -_unit(M, Q, C, 5).abs()
    a2, b2 = a.bfloat16(), b.bfloat16()
    out = _kernel(ops, a2, b2)
    assert bool((out < 0).all())
    assert (out.double() - _ref64(a2, b2)).abs().max().item() <= C * 2.0 ** -23


def test_planted_corner_matches(ops):
    """A copy of one patch planted at a corner (p*, q*) of the P x Q block
    must be found: an off-by-one segment bound loses it (~0.5 instead of 1)."""
    N = M = 4
    P = Q = 49
    C = 64
    a, b = _unit(N, P, C, 6), _unit(M, Q, C, 7)
    corners = [(0, 0), (0, Q - 1), (P - 1, 0), (P - 1, Q - 1)]
    for n, (ps, qs) in enumerate(corners):
        b[n, qs] = a[n, ps]
    a2, b2 = a.bfloat16(), b.bfloat16()
    out = _kernel(ops, a2, b2)
    ref = _ref64(a2, b2)
    d = out.diagonal()
    assert (d - 1).abs().max().item() <= 2.0 ** -7
    assert (out.double() - ref).abs().max().item() <= C * 2.0 ** -23
    off = out[~torch.eye(N, dtype=torch.bool, device=DEV)]
    assert off.max().item() < 0.9


@pytest.mark.parametrize("precision,bound", [
    ("bf16", lambda C: 2.0 ** -8 + C * 2.0 ** -23),
    ("high", lambda C: 2.0 ** -16 + 3 * C * 2.0 ** -23)])
def test_modes_end_to_end(ops, precision, bound):
    N, M, P, Q, C = 5, 7, 49, 49, 64
    a, b = _unit(N, P, C, 8), _unit(M, Q, C, 9)
    out = ops.patch_maxsim(a, b, precision=precision)
    err = (out.double() - _ref64(a, b)).abs().max().item()
    print(f"{precision}: err={err:.3e} bound={bound(C):.3e}")
    assert err <= bound(C)
    # like with like: the CPU path rounds the same way
    cpu = ops.patch_maxsim(a.cpu(), b.cpu(), precision=precision)
    k = (C if precision == "bf16" else 3 * C)
    assert (out.cpu() - cpu).abs().max().item() <= 2 * k * 2.0 ** -23


@pytest.mark.parametrize("precision", ["bf16", "high"])
def test_deterministic_and_chunk_neutral(ops, precision):
    N, M, P, Q, C = 7, 9, 49, 49, 256
    a, b = _unit(N, P, C, 10), _unit(M, Q, C, 11)
    first = ops.patch_maxsim(a, b, precision=precision)
    again = ops.patch_maxsim(a, b, precision=precision)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    chunked = ops.patch_maxsim(a, b, precision=precision, chunk=2)
    assert torch.equal(first.view(torch.int32), chunked.view(torch.int32))


def test_wrapper_inputs(ops):
    """fp32 and non-contiguous inputs, C that needs padding, empty N or M."""
    a, b = _unit(4, 6, 20, 12), _unit(3, 5, 20, 13)
    ref = _ref64(a, b)
    out = ops.patch_maxsim(a, b)
    assert (out.double() - ref).abs().max().item() <= 2.0 ** -16 + 72 * 2.0 ** -23
    at = a.transpose(1, 2).contiguous().transpose(1, 2)
    assert not at.is_contiguous()
    assert torch.equal(ops.patch_maxsim(at, b), out)
    e = ops.patch_maxsim(a[:0], b)
    assert e.shape == (0, 3) and e.dtype == torch.float32 and e.is_cuda
    assert ops.patch_maxsim(a, b[:0]).shape == (4, 0)


def test_binding_rejects_bad_operands(ops):
    m = ops.ext()
    a = _unit(2, 3, 16, 14).bfloat16()
    b = _unit(2, 3, 16, 15).bfloat16()
    with pytest.raises(RuntimeError):
        m.patch_maxsim(a.float(), b.float())          # dtype
    with pytest.raises(RuntimeError):
        m.patch_maxsim(a.transpose(0, 1), b)          # contiguity
    with pytest.raises(RuntimeError):
        m.patch_maxsim(a[..., :12].contiguous(), b[..., :12].contiguous())
    with pytest.raises(RuntimeError):
        m.patch_maxsim(a, b[..., :8].contiguous())    # C mismatch


def test_einsum_in_chunks_dispatch(ops):
    from dcr_amd.retrieval.similarity import einsum_in_chunks
    g = torch.Generator().manual_seed(16)
    fa = F.normalize(torch.randn(5, 32, 9, generator=g), dim=1).to(DEV)
    fb = F.normalize(torch.randn(4, 32, 9, generator=g), dim=1).to(DEV)
    n0 = ops.dispatch_counts["patch_maxsim"]
    plain = einsum_in_chunks(fa, fb, chunk=2, stype="")
    assert ops.dispatch_counts["patch_maxsim"] == n0
    cross = einsum_in_chunks(fa, fb, chunk=2, stype="cross")
    assert ops.dispatch_counts["patch_maxsim"] == n0 + 1
    want = torch.einsum("ncp,mcq->nmpq", fa.double(), fb.double()).amax((2, 3))
    assert cross.shape == (5, 4) and cross.dtype == torch.float32
    assert (cross.double() - want).abs().max().item() <= \
        2.0 ** -16 + 3 * 32 * 2.0 ** -23
    assert bool((cross >= plain - 1e-5).all())   # all pairs >= aligned pairs
