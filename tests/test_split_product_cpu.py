"""Split product (dcr_amd.ops.split_product) on the CPU: the operand
transformations the HIP kernel is fed, checked against an fp64 einsum, and
the retrieval paths that call it.

Bounds are tests/test_maxsim_cpu.py's, for unit-norm contraction vectors
(every group is L2-normalised): 2^-8 + L 2^-23 for bf16 (two roundings of
2^-9 relative), 2^-16 + 3L 2^-23 for the hi/lo split (16 significand bits
kept, only lo.lo dropped); fp32 accumulation over K' terms is given
K' 2^-23, twice its worst case."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dcr_amd.ops import split_product
from dcr_amd.ops.functional import _bf16_split, split_product_operands
from dcr_amd.retrieval.similarity import einsum_in_chunks

ROOT = Path(__file__).resolve().parent.parent

# (N, M, G, L)
SHAPES = [(1, 1, 1, 8), (5, 7, 8, 64), (130, 129, 3, 72), (4, 6, 64, 8),
          (9, 5, 5, 24), (6, 5, 7, 20)]


def _unit(n, g, l, seed):
    gen = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(n, g, l, generator=gen), dim=-1)


def _ref64(a, b):
    return torch.einsum("ngl,mgl->nmg", a.double(), b.double()).amax(2)


def _bound(precision, L):
    if precision == "bf16":
        return 2.0 ** -8 + L * 2.0 ** -23
    return 2.0 ** -16 + 3 * L * 2.0 ** -23


@pytest.mark.parametrize("precision", ["bf16", "high"])
@pytest.mark.parametrize("N,M,G,L", SHAPES)
def test_split_product_cpu_vs_fp64(N, M, G, L, precision):
    a, b = _unit(N, G, L, 1), _unit(M, G, L, 2)
    out = split_product(a, b, precision=precision)
    assert out.dtype == torch.float32 and out.shape == (N, M)
    err = (out.double() - _ref64(a, b)).abs().max().item()
    print(f"{precision} {(N, M, G, L)}: err={err:.3e} "
          f"bound={_bound(precision, L):.3e}")
    assert err <= _bound(precision, L)


def test_operands_layout():
    """Per group: L padded to 8, [hi | hi | lo] x [hi | lo | hi]."""
    a, b = _unit(2, 3, 20, 3), _unit(3, 3, 20, 4)
    a2, b2 = split_product_operands(a, b, "high")
    assert a2.shape == (2, 3, 72) and b2.shape == (3, 3, 72)
    assert a2.dtype == torch.bfloat16 and a2.is_contiguous()
    ah, al = _bf16_split(a)
    bh, bl = _bf16_split(b)
    assert torch.equal(a2[..., :20], ah) and torch.equal(a2[..., 24:44], ah)
    assert torch.equal(a2[..., 48:68], al)
    assert torch.equal(b2[..., :20], bh) and torch.equal(b2[..., 24:44], bl)
    assert torch.equal(b2[..., 48:68], bh)
    assert a2[..., 20:24].abs().max() == 0 and b2[..., 68:].abs().max() == 0
    a1, b1 = split_product_operands(a, b, "bf16")
    assert a1.shape == (2, 3, 24) and torch.equal(a1[..., :20], ah)
    with pytest.raises(ValueError):
        split_product_operands(a, b, "fp8")


@pytest.mark.parametrize("precision", ["bf16", "high"])
def test_chunk_is_bitwise_neutral(precision):
    a, b = _unit(7, 5, 40, 5), _unit(6, 5, 40, 6)
    full = split_product(a, b, precision=precision)
    for chunk in (1, 2, 3, 7, 100):
        assert torch.equal(split_product(a, b, precision=precision,
                                         chunk=chunk), full)


def test_empty_and_bad_arguments():
    a, b = _unit(3, 4, 16, 7), _unit(2, 4, 16, 8)
    e = split_product(a[:0], b)
    assert e.shape == (0, 2) and e.dtype == torch.float32
    e = split_product(a, b[:0], precision="bf16")
    assert e.shape == (3, 0) and e.dtype == torch.float32
    with pytest.raises(ValueError):
        split_product(a, b, precision="fp8")
    with pytest.raises(ValueError):
        split_product(a, b[..., :8])                  # L mismatch
    with pytest.raises(ValueError):
        split_product(a, b[:, :3])                    # G mismatch
    with pytest.raises(ValueError):
        split_product(a[0], b)                        # 2-D
    with pytest.raises(ValueError):
        split_product(a, b, chunk=0)
    with pytest.raises(ValueError):
        split_product(a[:, :0], b[:, :0])             # G = 0


def test_input_dtypes_and_strides():
    a, b = _unit(3, 4, 16, 9), _unit(2, 4, 16, 10)
    ref = split_product(a, b)
    at = a.transpose(1, 2).contiguous().transpose(1, 2)   # non-contiguous
    assert not at.is_contiguous()
    assert torch.equal(split_product(at, b), ref)
    assert torch.equal(split_product(a.double(), b.double()), ref)
    assert torch.equal(split_product(a.bfloat16(), b.bfloat16()),
                       split_product(a, b, precision="bf16"))


def test_one_group_is_a_matmul():
    a, b = _unit(4, 1, 32, 11), _unit(5, 1, 32, 12)
    out = split_product(a, b)
    want = a[:, 0].double() @ b[:, 0].double().t()
    assert (out.double() - want).abs().max().item() <= _bound("high", 32)


@pytest.mark.parametrize("stype", ["cross", ""])
def test_einsum_in_chunks_cpu_unchanged(stype):
    gen = torch.Generator().manual_seed(13)
    fa = F.normalize(torch.randn(7, 24, 6, generator=gen), dim=1)
    fb = F.normalize(torch.randn(5, 24, 6, generator=gen), dim=1)
    sims = []
    for i in range(0, 7, 3):
        x = fa[i:i + 3].float()
        if stype == "cross":
            s = torch.einsum("ncp,mcq->nmpq", x, fb.float()).amax(dim=(2, 3))
        else:
            s = torch.einsum("ncp,mcp->nmp", x, fb.float()).amax(dim=2)
        sims.append(s)
    want = torch.cat(sims, dim=0)
    from dcr_amd import ops
    n0 = ops.dispatch_counts["split_product"]
    assert torch.equal(einsum_in_chunks(fa, fb, chunk=3, stype=stype), want)
    assert torch.equal(einsum_in_chunks(fa, fb, chunk=3, stype=stype,
                                        precision="bf16"), want)
    assert ops.dispatch_counts["split_product"] == n0


def _image_dirs(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    qdir, vdir = tmp_path / "gens", tmp_path / "train"
    qdir.mkdir()
    vdir.mkdir()
    for d, n in ((qdir, 3), (vdir, 4)):
        for i in range(n):
            Image.fromarray(rng.integers(0, 255, (64, 64, 3)).astype(np.uint8)) \
                .save(d / f"{i}.png")
    return qdir, vdir


def _run_cli(monkeypatch, tmp_path, qdir, vdir, extra):
    """diff_retrieval.main() in this process, recording the flat embeddings
    it extracted (query first, then train)."""
    import diff_retrieval as dr
    seen = []
    real = dr.extract_features

    def recording(*a, **k):
        f = real(*a, **k)
        seen.append(f.detach().cpu().clone())
        return f

    out = tmp_path / "s"
    monkeypatch.setattr(dr, "extract_features", recording)
    monkeypatch.setattr(sys, "argv", [
        "diff_retrieval.py", "--query_dir", str(qdir), "--val_dir", str(vdir),
        "--pt_style", "sscd", "-b", "4", "-j", "0", "--imsize", "64", "-ssp",
        str(out), "--skip_fid", "--noeval", "--similarity_metric",
        "splitloss"] + extra)
    dr.main()
    return seen, out


@pytest.mark.timeout(600)
@pytest.mark.parametrize("flag", ["--num_loss_chunks", "--numpatches"])
def test_cli_num_loss_chunks(monkeypatch, tmp_path, flag):
    """c chunks of the flat embedding: rearrange 'b (c p) -> b c p', einsum
    'ncp,mcp->nmc', max over c (the reference's splitloss)."""
    qdir, vdir = _image_dirs(tmp_path)
    c = 8
    seen, out = _run_cli(monkeypatch, tmp_path, qdir, vdir, [flag, str(c)])
    q = F.normalize(seen[0].double(), dim=1)
    v = F.normalize(seen[1].double(), dim=1)
    d = q.shape[1]
    qc, vc = q.reshape(-1, c, d // c), v.reshape(-1, c, d // c)
    want = torch.einsum("ncp,mcp->nmc", qc, vc).amax(2)
    want_tt = torch.einsum("ncp,mcp->nmc", vc, vc).amax(2)
    sim = torch.load(out / "similarity.pth")
    sim_tt = torch.load(out / "similarity_wtrain.pth")
    assert sim.shape == (3, 4) and sim_tt.shape == (4, 4)
    # chunks of a unit vector have norm <= 1; F.normalize in fp32 adds 2^-23
    bound = _bound("high", d // c) + 2.0 ** -22
    assert (sim.double() - want).abs().max().item() <= bound
    assert (sim_tt.double() - want_tt).abs().max().item() <= bound
    # it is not the plain dot product
    assert (sim.double() - q @ v.t()).abs().max().item() > 1e-3


@pytest.mark.timeout(600)
def test_cli_rejects_non_dividing_chunks(monkeypatch, tmp_path):
    qdir, vdir = _image_dirs(tmp_path)
    with pytest.raises(ValueError, match=r"512.*\b7\b"):
        _run_cli(monkeypatch, tmp_path, qdir, vdir, ["--num_loss_chunks", "7"])


def test_retrieval_cli_help_texts():
    r = subprocess.run([sys.executable, str(ROOT / "diff_retrieval.py"),
                        "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = " ".join(r.stdout.split())
    assert "c > 1 slices the flat" in text
    assert "overrides --num_loss_chunks" in text
