"""ops.topk_sim on the CPU (reference path) and the search consumers' CPU
behaviour: the ordering rule against a brute-force Python sort on integer
inputs (exact scores, plentiful ties), the error cases, and that the CPU
paths of stream_top1 / sharded_topk / the CLI are what they were."""
import importlib.util
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def _ints(n, d, seed, lo=-2, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, (n, d), generator=g).float()


def _brute(q, x, k):
    """Python sort by (-score, index); scores are exact integers."""
    s = (q.double() @ x.double().t()).tolist()
    vals, idxs = [], []
    for row in s:
        order = sorted(range(len(row)), key=lambda c: (-row[c], c))[:k]
        idxs.append(order)
        vals.append([row[c] for c in order])
    return torch.tensor(vals, dtype=torch.float32), torch.tensor(idxs)


@pytest.mark.parametrize("precision", ["bf16", "high"])
@pytest.mark.parametrize("nq,nx,d,k", [(7, 50, 8, 1), (13, 300, 40, 16),
                                       (3, 16, 12, 16), (5, 90, 5, 40)])
def test_reference_matches_brute_force(nq, nx, d, k, precision):
    from dcr_amd import ops
    q, x = _ints(nq, d, 1), _ints(nx, d, 2)
    v, i = ops.topk_sim(q, x, k, precision=precision)
    rv, ri = _brute(q, x, k)
    assert v.dtype == torch.float32 and i.dtype == torch.int64
    assert v.shape == (nq, k) and i.shape == (nq, k)
    # ties are plentiful: the test means something
    full = (q @ x.t()).tolist()
    assert any(len(set(row)) < len(row) for row in full)
    assert torch.equal(i, ri)
    assert torch.equal(v, rv)


def test_nan_is_never_returned():
    from dcr_amd import ops
    q, x = _ints(4, 8, 3), _ints(20, 8, 4)
    x[5, 0] = float("nan")
    v, i = ops.topk_sim(q, x, 19)
    assert not bool((i == 5).any())
    assert not bool(torch.isnan(v).any())


def test_errors():
    from dcr_amd import ops
    q, x = _ints(4, 8, 5), _ints(20, 8, 6)
    with pytest.raises(ValueError):
        ops.topk_sim(q[0], x, 1)                      # 1-D query
    with pytest.raises(ValueError):
        ops.topk_sim(q, x[:, :4], 1)                  # D mismatch
    with pytest.raises(ValueError):
        ops.topk_sim(q, x, 0)                         # k < 1
    with pytest.raises(ValueError):
        ops.topk_sim(q, x, 21)                        # k > Nx
    with pytest.raises(ValueError):
        ops.topk_sim(q, x, 1, precision="fp32")       # unknown precision
    v, i = ops.topk_sim(q[:0], x, 3)
    assert v.shape == (0, 3) and i.shape == (0, 3)


def _two_chunks(tmp_path):
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
    return torch.from_numpy(q), files


def test_stream_top1_cpu_precision_default_is_fp32(tmp_path):
    from dcr_amd.search import stream_top1
    q, files = _two_chunks(tmp_path)
    s0, k0 = stream_top1(q, files, device="cpu", precision=None)
    s1, k1 = stream_top1(q, files, device="cpu", precision="fp32")
    assert k0 == k1 and np.array_equal(s0, s1)
    assert k0[0] == "c0:7" and k0[2] == "c1:3"
    assert s0[0] > 0.999 and s0[2] > 0.999
    # a CPU device takes the GEMM path whatever the precision says
    s2, k2 = stream_top1(q, files, device="cpu", precision="high",
                         query_chunks=2)
    assert k2 == k0 and np.array_equal(s2, s0)
    with pytest.raises(ValueError):
        stream_top1(q, files, device="cpu", precision="fp64")


def test_cli_parses_search_precision():
    spec = importlib.util.spec_from_file_location(
        "similarity_search_cli", ROOT / "embedding_search" / "similarity_search.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--generation_embedding", "g.pkl", "--laion_embedding_folder", "l",
            "--dump_path", "o.pkl"]
    p = mod.build_parser()
    assert p.parse_args(base).search_precision == "high"
    for name in ("high", "bf16", "fp32"):
        assert p.parse_args(base + ["--search_precision", name]) \
            .search_precision == name
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--search_precision", "fp64"])


def test_sharded_topk_cpu_ignores_fused_switch(monkeypatch):
    from dcr_amd import ops
    from dcr_amd.search import sharded_topk
    g = torch.Generator().manual_seed(7)
    q = torch.nn.functional.normalize(torch.randn(9, 32, generator=g), dim=1)
    shard = torch.nn.functional.normalize(torch.randn(200, 32, generator=g), dim=1)
    n0 = ops.dispatch_counts["topk_sim"]
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("DCR_FUSED_SEARCH", flag)
        out[flag] = [sharded_topk(q, shard, k=3, chunk=64),
                     sharded_topk(q, shard, k=3, chunk=64,
                                  compute_dtype=torch.bfloat16)]
    for a, b in zip(out["0"], out["1"]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert ops.dispatch_counts["topk_sim"] == n0
