"""Fused top-k similarity kernel (dcr_amd/ops/hip/topk_sim.hip) and its
consumers in dcr_amd.search.

Ordering rule under test: higher score first, the lower index first among
equal scores. Exact checks use integer-valued bf16 inputs (every product and
partial sum is a small integer, exact in fp32 in any order) against the CPU
reference bit for bit. On random unit-norm inputs neighbouring scores are
closer than the accumulation error, so set equality against a reference is
not a valid check; every row is instead checked against the fp64 product of
the SAME bf16 operands with tol = K' * 2^-23 (bf16 x bf16 products are exact
in fp32, only the accumulation differs; K' is the contracted length):
indices distinct and in range, |score_j - ref[idx_j]| <= tol, scores
non-increasing, and every index not returned has ref <= score_k + 2*tol."""
import functools
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from dcr_amd import ops as o
    assert o.ext() is not None, "HIP extension must be present on GPU box"
    return o


def _kernel(ops, q2, x2, m, stripes=0):
    assert q2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16
    return ops.ext().topk_sim(q2, x2, m, stripes)


@functools.lru_cache(maxsize=None)
def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(n, d, generator=g), dim=-1).to(DEV)


@functools.lru_cache(maxsize=None)
def _int_case(nq, nx, d):
    """Integer operands in {-2..2} and the CPU reference's top 16 (or Nx)."""
    from dcr_amd import ops
    g = torch.Generator().manual_seed(3)
    q = torch.randint(-2, 3, (nq, d), generator=g).to(torch.bfloat16)
    x = torch.randint(-2, 3, (nx, d), generator=g).to(torch.bfloat16)
    rv, ri = ops.topk_sim(q, x, min(16, nx), precision="bf16")
    return q.to(DEV), x.to(DEV), rv, ri


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])


def _check_rows(scores, idx, ref, tol):
    """The tolerance-aware check of the module docstring, every row."""
    nq, k = idx.shape
    nx = ref.shape[1]
    assert scores.dtype == torch.float32 and idx.dtype == torch.int64
    assert scores.shape == (nq, k)
    assert bool(((idx >= 0) & (idx < nx)).all())
    srt = idx.sort(dim=1).values
    assert bool((srt[:, 1:] > srt[:, :-1]).all()), "duplicate index"
    err = (scores.double() - ref.gather(1, idx)).abs().max().item()
    assert bool((scores[:, 1:] <= scores[:, :-1]).all())
    rest = ref.clone().scatter_(1, idx, float("-inf"))
    over = (rest.max(dim=1).values - scores[:, -1].double()).max().item() \
        if k < nx else float("-inf")
    print(f"err={err:.3e} tol={tol:.3e} best-missed-minus-kth={over:.3e}")
    assert err <= tol
    assert over <= 2 * tol


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("nq,nx,d,k,stripes", [
    (130, 300, 40, 1, 0), (130, 300, 40, 4, 0), (130, 300, 40, 16, 0),
    (1, 16, 8, 16, 0),
    (70, 1000, 72, 10, 1), (70, 1000, 72, 10, 3), (70, 1000, 72, 10, 8),
    (5, 20, 64, 16, 3),
    (5, 264, 64, 16, 3),      # last stripe holds 8 columns: fewer than k
    (5, 300, 64, 8, 0),       # list capacity 8
])
def test_exact_integers(ops, nq, nx, d, k, stripes):
    q, x, rv, ri = _int_case(nq, nx, d)
    v, i = _kernel(ops, q, x, k, stripes)
    assert v.shape == (nq, k) and i.dtype == torch.int64
    assert torch.equal(i.cpu(), ri[:, :k])
    assert torch.equal(_bits(v.cpu()), _bits(rv[:, :k]))


def test_planted_ties(ops):
    """Copies of one query at rows 5 (first wave half of tile 0), 70 (the
    other half of the same tile), 200 (another tile) and 900 (another
    stripe): equal scores must come back lowest index first."""
    q = _unit(3, 64, 20).bfloat16()
    x = _unit(1000, 64, 21).bfloat16().clone()
    for r in (5, 70, 200, 900):
        x[r] = q[1]
    v, i = _kernel(ops, q, x, 4, 3)
    assert i[1].tolist() == [5, 70, 200, 900]
    assert len(set(_bits(v[1]).tolist())) == 1
    assert abs(v[1, 0].item() - 1.0) < 2.0 ** -6


# ---------------------------------------------------------------- tolerance
@pytest.mark.parametrize("precision", ["bf16", "high"])
@pytest.mark.parametrize("nq,nx,d,k", [(130, 300, 40, 16), (70, 520, 512, 10),
                                       (3, 257, 2048, 4)])
def test_kernel_vs_fp64_of_same_operands(ops, nq, nx, d, k, precision):
    from dcr_amd.ops.functional import topk_sim_operands
    q2, x2 = topk_sim_operands(_unit(nq, d, 1), _unit(nx, d, 2), precision)
    assert q2.shape[1] == (d if precision == "bf16" else 3 * d)
    v, i = _kernel(ops, q2, x2, k)
    ref = q2.double() @ x2.double().t()
    _check_rows(v, i, ref, q2.shape[1] * 2.0 ** -23)


def test_padding_cannot_win(ops):
    """Every score is negative, Nx = 100: a zero from a padded column or a
    zero-staged row reaching a list would beat them all."""
    nq, nx, d = 70, 100, 64
    q = _unit(nq, d, 4).abs()
    noise = _unit(nx, d, 5).abs()
    x = -F.normalize(q[torch.arange(nx, device=DEV) % nq] + 0.1 * noise, dim=-1)
    q2, x2 = q.bfloat16(), x.bfloat16()
    ref = q2.double() @ x2.double().t()
    assert ref.max().item() < 0
    for stripes in (0, 1):
        v, i = _kernel(ops, q2, x2, 16, stripes)
        assert bool((i < nx).all()) and bool((v < 0).all())
        _check_rows(v, i, ref, d * 2.0 ** -23)


def test_bit_reproducible(ops):
    nq, nx, d, k = 200, 1000, 72, 10
    q2, x2 = _unit(nq, d, 6).bfloat16(), _unit(nx, d, 7).bfloat16()
    first = _kernel(ops, q2, x2, k)
    assert _same(first, _kernel(ops, q2, x2, k))
    assert _same(first, _kernel(ops, q2, x2, k, 1))
    assert _same(first, _kernel(ops, q2, x2, k, 3))
    a = _kernel(ops, q2[:72].contiguous(), x2, k)
    b = _kernel(ops, q2[72:].contiguous(), x2, k)
    assert _same(first, (torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]])))


def test_high_end_to_end(ops):
    nq, nx, d = 70, 520, 64
    q, x = _unit(nq, d, 8), _unit(nx, d, 9)
    n0 = ops.dispatch_counts["topk_sim"]
    v, i = ops.topk_sim(q, x, 5, precision="high")
    assert ops.dispatch_counts["topk_sim"] == n0 + 1
    ref = q.double() @ x.double().t()
    _check_rows(v, i, ref, 2.0 ** -16 + 3 * d * 2.0 ** -23)
    with pytest.raises(ValueError, match="library path"):
        ops.topk_sim(q, x, 17)


# ---------------------------------------------------------------- consumers
def test_sharded_topk_fused(ops, monkeypatch):
    from dcr_amd.search import sharded_topk
    nq, nx, d, k = 256, 4096, 64, 10
    q, shard = _unit(nq, d, 30), _unit(nx, d, 31)
    monkeypatch.setenv("DCR_FUSED_SEARCH", "1")
    n0 = ops.dispatch_counts["topk_sim"]
    v, i = sharded_topk(q, shard, k=k)
    assert ops.dispatch_counts["topk_sim"] > n0
    sel = torch.einsum("qd,qkd->qk", q, shard[i])
    assert (v - sel).abs().max().item() <= 1e-6
    # chunking must not change the result
    vc, ic = sharded_topk(q, shard, k=k, chunk=1000)
    assert torch.equal(ic, i) and (vc - v).abs().max().item() <= 1e-6

    monkeypatch.setenv("DCR_FUSED_SEARCH", "0")
    n1 = ops.dispatch_counts["topk_sim"]
    v0, i0 = sharded_topk(q, shard, k=k)
    assert ops.dispatch_counts["topk_sim"] == n1
    sel0 = torch.einsum("qd,qkd->qk", q, shard[i0])
    assert (v0 - sel0).abs().max().item() <= 1e-6

    top = (q @ shard.t()).topk(k + 1, dim=1).values
    clear = (top[:, k - 1] - top[:, k]) > 1e-4
    frac = clear.float().mean().item()
    print(f"rows with a clear 10th/11th gap: {frac:.3f}")
    assert frac >= 0.95
    assert torch.equal(i[clear], i0[clear])
    assert (v[clear] - v0[clear]).abs().max().item() <= 1e-6


def test_sharded_topk_allocates_no_score_matrix(ops, monkeypatch):
    from dcr_amd.search import sharded_topk
    monkeypatch.setenv("DCR_FUSED_SEARCH", "1")
    nq, nx, d, k = 2048, 65536, 64, 10
    q, shard = _unit(nq, d, 32), _unit(nx, d, 33)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    v, i = sharded_topk(q, shard, k=k)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"peak above the inputs: {extra / 2 ** 20:.1f} MiB")
    assert extra < nq * nx * 4 // 8
    assert v.shape == (nq, k) and bool((i >= 0).all()) and bool((i < nx).all())


def test_stream_top1_precisions(ops, tmp_path):
    from dcr_amd.search import stream_top1
    rng = np.random.default_rng(0)
    D = 16
    q = rng.normal(size=(4, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    files = []
    for n, (row, src) in enumerate([(7, 0), (3, 2)]):
        c = rng.normal(size=(50, D)).astype(np.float32)
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        c[row] = q[src]
        f = tmp_path / f"embedding_{n}.pkl"
        with open(f, "wb") as fh:
            pickle.dump({"features": c,
                         "indexes": [f"c{n}:{i}" for i in range(50)]}, fh)
        files.append(f)
    n0 = ops.dispatch_counts["topk_sim"]
    got = {p: stream_top1(torch.from_numpy(q), files, device=DEV, precision=p)
           for p in (None, "bf16", "fp32")}
    assert ops.dispatch_counts["topk_sim"] == n0 + 4   # 2 chunks x 2 fused runs
    s32, k32 = got["fp32"]
    assert k32[0] == "c0:7" and k32[2] == "c1:3"
    assert s32[0] > 0.999 and s32[2] > 0.999
    for p in (None, "bf16"):
        s, keys = got[p]
        assert keys == k32
        assert np.abs(s - s32).max() <= 1e-6


# ---------------------------------------------------------------- arguments
def test_binding_rejects_bad_arguments(ops):
    m = ops.ext()
    q = _unit(4, 16, 40).bfloat16()
    x = _unit(20, 16, 41).bfloat16()
    bad = [
        lambda: m.topk_sim(q.float(), x.float(), 1),              # dtype
        lambda: m.topk_sim(q.cpu(), x.cpu(), 1),                  # device
        lambda: m.topk_sim(q.t(), x, 1),                          # contiguity
        lambda: m.topk_sim(q[0], x, 1),                           # rank
        lambda: m.topk_sim(q, x[:, :8].contiguous(), 1),          # D mismatch
        lambda: m.topk_sim(q[:, :12].contiguous(),
                           x[:, :12].contiguous(), 1),            # D % 8
        lambda: m.topk_sim(q, x, 0),                              # m < 1
        lambda: m.topk_sim(q, x, 17),                             # m > 16
        lambda: m.topk_sim(q, x[:5].contiguous(), 6),             # m > Nx
        lambda: m.topk_sim(q, x, 1, -1),                          # stripes
    ]
    flat = torch.zeros(4 + 20 * 16, dtype=torch.bfloat16, device=DEV)
    off = flat[4:].view(20, 16)                                   # 8-byte offset
    assert off.is_contiguous() and off.data_ptr() % 16 == 8
    bad.append(lambda: m.topk_sim(q, off, 1))                     # alignment
    for fn in bad:
        with pytest.raises(RuntimeError):
            fn()
    # Nx >= 2^31 without the 34 GB: a stride-0 view (the size check comes
    # before the contiguity check). The grid-size check needs 2^30 query
    # rows of real memory and is not exercised here.
    with pytest.raises(RuntimeError, match="2\\^31"):
        m.topk_sim(q, x[:1].expand(2 ** 31, 16), 1)
    v, i = m.topk_sim(q, x, 3)                                    # still sound
    assert v.shape == (4, 3) and bool((i >= 0).all())
