"""Fused split-product kernel (dcr_amd/ops/hip/splitsim.hip).

Kernel checks compare against the fp64 einsum of the SAME bf16 operands the
kernel is handed (rounded, or hi/lo-concatenated). A bf16 x bf16 product is
exact in fp32, so only the fp32 accumulation differs: L' * 2^-23 for
unit-norm groups, L' the contracted length of a group. Every group of the
inputs is L2-normalised, so per-group scores are O(1). End-to-end checks
compare against the fp64 einsum of the original fp32 inputs with the
CPU-test bounds (tests/test_split_product_cpu.py)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (N, M, G, L)
SHAPES = [
    (1, 1, 1, 8),             # minimum
    (5, 7, 8, 64),            # one k-step per group in bf16, three in high
    (130, 129, 3, 72),        # several tiles both ways, ragged tails, group
                              # end inside a k-step
    (4, 6, 64, 8),            # group shorter than an MFMA chunk
    (9, 5, 5, 24),            # small ragged case, group shorter than a chunk
    (2, 3, 196, 768),         # ViT patch map
    (3, 3, 49, 2048),         # SSCD trunk
    (300, 2, 1, 64),          # G = 1 equals a plain GEMM
]


@pytest.fixture(scope="module")
def ops():
    from dcr_amd import ops as o
    assert o.ext() is not None, "HIP extension must be present on GPU box"
    return o


def _unit(n, g, l, seed):
    gen = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(n, g, l, generator=gen), dim=-1).to(DEV)


def _ref64(a, b):
    """fp64 max over groups, one row of a at a time (bounded memory)."""
    bd = b.double()
    return torch.stack([torch.einsum("gl,mgl->mg", x.double(), bd).amax(1)
                        for x in a])


def _kernel(ops, a2, b2, splits=0):
    assert a2.dtype == torch.bfloat16 and b2.dtype == torch.bfloat16
    return ops.ext().split_product(a2, b2, splits)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("precision", ["bf16", "high"])
@pytest.mark.parametrize("N,M,G,L", SHAPES)
def test_kernel_vs_fp64_of_same_operands(ops, N, M, G, L, precision):
    from dcr_amd.ops.functional import split_product_operands
    a, b = _unit(N, G, L, 1), _unit(M, G, L, 2)
    a2, b2 = split_product_operands(a, b, precision)
    out = _kernel(ops, a2, b2)
    assert out.dtype == torch.float32 and out.shape == (N, M)
    tol = a2.shape[-1] * 2.0 ** -23
    err = (out.double() - _ref64(a2, b2)).abs().max().item()
    print(f"{precision} {(N, M, G, L)}: L'={a2.shape[-1]} err={err:.3e} "
          f"tol={tol:.3e}")
    assert err <= tol
    if G == 1:
        gemm = a2[:, 0].double() @ b2[:, 0].double().t()
        assert (out.double() - gemm).abs().max().item() <= tol


@pytest.mark.parametrize("N,M,G,L", [(5, 7, 3, 72), (4, 6, 64, 8)])
def test_exact_integers(ops, N, M, G, L):
    """Entries in {-2..2}: every partial sum is a small integer, exact in
    fp32 in any order. A and B are drawn differently (B is mostly
    non-positive), so a k-step that reads into the neighbouring group or a
    transposed output shows."""
    gen = torch.Generator().manual_seed(3)
    a = torch.randint(-2, 3, (N, G, L), generator=gen).to(DEV, torch.bfloat16)
    b = torch.randint(-2, 2, (M, G, L), generator=gen).to(DEV, torch.bfloat16)
    ref = _ref64(a, b)
    for splits in (0, 1, G):
        out = _kernel(ops, a, b, splits)
        assert out.shape == (N, M)
        assert torch.equal(out.double(), ref), splits


@pytest.mark.parametrize("splits", [1, 2])
def test_all_negative_scores(ops, splits):
    """Positive a, negative b: every score is < 0, so a running max started
    at 0 or a padded zero reaching a max would show."""
    N, M, G, L = 130, 129, 3, 72
    a2 = _unit(N, G, L, 4).abs().bfloat16()
    b2 = (-_unit(M, G, L, 5).abs()).bfloat16()
    out = _kernel(ops, a2, b2, splits)
    assert bool((out < 0).all())
    assert (out.double() - _ref64(a2, b2)).abs().max().item() <= L * 2.0 ** -23


def test_planted_match(ops):
    """A unit chunk copied into the first group (even rows) or the last group
    (odd rows) only must be found: the diagonal is 1, everything else is the
    best of G random 64-d cosines."""
    N, G, L = 6, 5, 64
    a, b = _unit(N, G, L, 6), _unit(N, G, L, 7)
    for n in range(N):
        g = 0 if n % 2 == 0 else G - 1
        b[n, g] = a[n, g]
    a2, b2 = a.bfloat16(), b.bfloat16()
    for splits in (1, G):
        out = _kernel(ops, a2, b2, splits)
        d = out.diagonal()
        assert (d - 1).abs().max().item() <= 2.0 ** -7
        off = out[~torch.eye(N, dtype=torch.bool, device=DEV)]
        assert off.max().item() < d.min().item()
        assert off.max().item() < 0.9
        assert (out.double() - _ref64(a2, b2)).abs().max().item() \
            <= L * 2.0 ** -23


@pytest.mark.parametrize("precision", ["bf16", "high"])
@pytest.mark.parametrize("N,M,G,L", [(5, 7, 8, 64), (9, 5, 5, 24),
                                     (130, 129, 3, 72)])
def test_bit_identical(ops, N, M, G, L, precision):
    """Repeated calls, row chunking and any split count return the same
    bits: every group's dot product runs the same k-step sequence and the
    combine is an exact max."""
    from dcr_amd.ops.functional import split_product_operands
    a, b = _unit(N, G, L, 8), _unit(M, G, L, 9)
    first = ops.split_product(a, b, precision=precision)
    again = ops.split_product(a, b, precision=precision)
    assert torch.equal(_bits(first), _bits(again))
    chunked = ops.split_product(a, b, precision=precision, chunk=2)
    assert torch.equal(_bits(first), _bits(chunked))
    a2, b2 = split_product_operands(a, b, precision)
    for splits in (1, 2, 3, G):
        if splits <= G:
            forced = _kernel(ops, a2, b2, splits)
            assert torch.equal(_bits(first), _bits(forced)), splits


@pytest.mark.parametrize("precision,bound", [
    ("bf16", lambda L: 2.0 ** -8 + L * 2.0 ** -23),
    ("high", lambda L: 2.0 ** -16 + 3 * L * 2.0 ** -23)])
def test_modes_end_to_end(ops, precision, bound):
    N, M, G, L = 5, 7, 8, 64
    a, b = _unit(N, G, L, 10), _unit(M, G, L, 11)
    n0 = ops.dispatch_counts["split_product"]
    out = ops.split_product(a, b, precision=precision)
    assert ops.dispatch_counts["split_product"] == n0 + 1
    err = (out.double() - _ref64(a, b)).abs().max().item()
    print(f"{precision}: err={err:.3e} bound={bound(L):.3e}")
    assert err <= bound(L)
    # like with like: the CPU path rounds the same way
    cpu = ops.split_product(a.cpu(), b.cpu(), precision=precision)
    k = (L if precision == "bf16" else 3 * L)
    assert (out.cpu() - cpu).abs().max().item() <= 2 * k * 2.0 ** -23


def test_wrapper_inputs(ops):
    """fp32 and non-contiguous inputs, L that needs padding, empty N or M."""
    a, b = _unit(6, 7, 20, 12), _unit(5, 7, 20, 13)
    ref = _ref64(a, b)
    out = ops.split_product(a, b)
    assert (out.double() - ref).abs().max().item() <= 2.0 ** -16 + 72 * 2.0 ** -23
    at = a.transpose(1, 2).contiguous().transpose(1, 2)
    assert not at.is_contiguous()
    assert torch.equal(ops.split_product(at, b), out)
    assert torch.equal(ops.split_product(a.double(), b.double()), out)
    e = ops.split_product(a[:0], b)
    assert e.shape == (0, 5) and e.dtype == torch.float32 and e.is_cuda
    assert ops.split_product(a, b[:0]).shape == (6, 0)


def test_binding_rejects_bad_operands(ops):
    m = ops.ext()
    a = _unit(2, 3, 16, 14).bfloat16()
    b = _unit(2, 3, 16, 15).bfloat16()
    bad = [
        lambda: m.split_product(a.float(), b.float()),            # dtype
        lambda: m.split_product(a.cpu(), b.cpu()),                # device
        lambda: m.split_product(a.transpose(0, 1), b),            # contiguity
        lambda: m.split_product(a[0], b),                         # rank
        lambda: m.split_product(a[..., :12].contiguous(),
                                b[..., :12].contiguous()),        # L % 8
        lambda: m.split_product(a, b[..., :8].contiguous()),      # L mismatch
        lambda: m.split_product(a, b[:, :2].contiguous()),        # G mismatch
        lambda: m.split_product(a, b, -1),                        # splits < 0
        lambda: m.split_product(a, b, 4),                         # splits > G
    ]
    off = torch.empty(2 * 3 * 16 + 4, dtype=torch.bfloat16, device=DEV)[4:] \
        .view(2, 3, 16)
    bad.append(lambda: m.split_product(off, b))                   # alignment
    for f in bad:
        with pytest.raises(RuntimeError):
            f()
    out = m.split_product(a, b, 3)                                # still sound
    assert (out.double() - _ref64(a, b)).abs().max().item() <= 16 * 2.0 ** -23


def test_einsum_in_chunks_dispatch(ops, monkeypatch):
    from dcr_amd.retrieval.similarity import einsum_in_chunks
    gen = torch.Generator().manual_seed(16)
    fa = F.normalize(torch.randn(5, 32, 9, generator=gen), dim=1).to(DEV)
    fb = F.normalize(torch.randn(4, 32, 9, generator=gen), dim=1).to(DEV)
    want = torch.einsum("ncp,mcp->nmp", fa.double(), fb.double()).amax(2)
    bound = 2.0 ** -16 + 3 * 32 * 2.0 ** -23
    n0 = ops.dispatch_counts["split_product"]
    plain = einsum_in_chunks(fa, fb, chunk=2, stype="")
    assert ops.dispatch_counts["split_product"] == n0 + 1
    assert plain.shape == (5, 4) and plain.dtype == torch.float32
    assert (plain.double() - want).abs().max().item() <= bound
    monkeypatch.setenv("DCR_FUSED_SPLITSIM", "0")
    eins = einsum_in_chunks(fa, fb, chunk=2, stype="")
    assert ops.dispatch_counts["split_product"] == n0 + 1
    assert (eins.double() - want).abs().max().item() <= bound
    monkeypatch.delenv("DCR_FUSED_SPLITSIM")
    einsum_in_chunks(fa, fb, chunk=2, stype="", precision="bf16")
    assert ops.dispatch_counts["split_product"] == n0 + 2
