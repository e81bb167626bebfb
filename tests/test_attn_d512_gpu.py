"""Flash attention forward for the VAE mid-block's single 512-d head
(attn_fwd_d512_kernel in dcr_amd/ops/hip/attention.hip), from the raw
binding up to AutoencoderKL encode/decode.

Reference: fp32 scaled_dot_product_attention on the same bf16 inputs.
Tolerance: the project's forward tolerance (test_flash_attention_fwd,
test_ops_attention_grad_dispatch) — max-abs error below 2e-2 of the
reference's max-abs."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

D = 512
B, H = 2, 2
# (Lq, Lk): one full tile; a quarter-filled tile; partial tiles on both
# axes; multiple q tiles with a 13-key second key tile; a 2-row tail after
# two full tiles; five key tiles for the running rescale.
SHAPES = [(64, 64), (16, 16), (100, 33), (256, 77), (130, 130), (320, 320)]
KINDS = ["randn", "ramp"]


def _close(out, ref, rtol):
    scale = ref.abs().max().item() + 1e-6
    err = (out.float() - ref.float()).abs().max().item()
    assert err < rtol * scale, f"err={err:.4g} scale={scale:.4g} rtol={rtol}"


@pytest.fixture(scope="module")
def ext():
    from dcr_amd import ops
    m = ops.ext()
    assert m is not None, "HIP extension must be present on GPU box"
    return m


_CASES = {}


def _case(Lq, Lk, kind="randn", b=B, h=H):
    """bf16 inputs [b,L,h,512] and the fp32 SDPA reference in the same
    layout, computed once per case and shared read-only. kind "ramp"
    scales the keys by linspace(0.5, 4, Lk) along the key axis, so the
    running max keeps rising from tile to tile and the softmax is sharp."""
    key = (Lq, Lk, kind, b, h)
    if key not in _CASES:
        gen = torch.Generator(device="cuda").manual_seed(Lq * 7 + Lk * 3 + b)
        mk = lambda L: torch.randn(b, L, h, D, device="cuda", generator=gen)
        q, k, v = mk(Lq), mk(Lk), mk(Lk)
        if kind == "ramp":
            k = k * torch.linspace(0.5, 4.0, Lk, device="cuda").view(1, Lk, 1, 1)
        q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
        scale = 1.0 / D ** 0.5
        ref = F.scaled_dot_product_attention(
            q.permute(0, 2, 1, 3).float(), k.permute(0, 2, 1, 3).float(),
            v.permute(0, 2, 1, 3).float(), scale=scale).permute(0, 2, 1, 3)
        _CASES[key] = (q, k, v, scale, ref.contiguous())
    return _CASES[key]


# ---------------------------------------------------------------- 1. binding
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_attn_fwd_d512(ext, Lq, Lk, kind):
    q, k, v, scale, ref = _case(Lq, Lk, kind)
    o = ext.attn_fwd_d512(q, k, v, scale)
    assert o.dtype == torch.bfloat16
    assert o.shape == q.shape
    assert torch.isfinite(o.float()).all()
    _close(o, ref, 2e-2)


# ---------------------------------------------------------------- 2. packed
def test_attn_fwd_d512_packed_equals_4d(ext):
    q, k, v, scale, _ = _case(100, 33)
    o4 = ext.attn_fwd_d512(q, k, v, scale)
    pk = lambda t: t.permute(0, 2, 1, 3).reshape(B * H, t.shape[1], D).contiguous()
    o3 = ext.attn_fwd_d512(pk(q), pk(k), pk(v), scale)
    assert o3.shape == (B * H, 100, D)
    # the layout only changes the row stride of the loads and stores; the
    # arithmetic and its order are the same, so the results are bit-equal
    assert torch.equal(o3, pk(o4))


# ---------------------------------------------------------------- 3. checks
def test_attn_fwd_d512_host_checks(ext):
    """Every one of these is refused by a TORCH_CHECK before any launch."""
    q, k, v, scale, _ = _case(64, 64)
    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=dt)
    with pytest.raises(RuntimeError):       # D=256
        ext.attn_fwd_d512(mk(2, 64, 2, 256), mk(2, 64, 2, 256),
                          mk(2, 64, 2, 256), scale)
    with pytest.raises(RuntimeError):       # fp32
        ext.attn_fwd_d512(q.float(), k.float(), v.float(), scale)
    with pytest.raises(RuntimeError):       # non-contiguous q
        qn = mk(2, 2, 64, D).permute(0, 2, 1, 3)
        assert not qn.is_contiguous()
        ext.attn_fwd_d512(qn, k, v, scale)
    with pytest.raises(RuntimeError):       # k and v of different shapes
        ext.attn_fwd_d512(q, k, mk(2, 32, 2, D), scale)
    with pytest.raises(RuntimeError):       # q and k of different rank
        ext.attn_fwd_d512(q, mk(4, 64, D), mk(4, 64, D), scale)
    with pytest.raises(RuntimeError):       # q and k of different H
        ext.attn_fwd_d512(q, mk(2, 64, 1, D), mk(2, 64, 1, D), scale)


# ---------------------------------------------------------------- 4. dispatch
def _counts():
    from dcr_amd.ops import dispatch_counts
    return (dispatch_counts["attention_d512"], dispatch_counts["attention_math"])


def _to_layout(t, layout):
    return t if layout == "blhd" else t.permute(0, 2, 1, 3).contiguous()


@pytest.mark.parametrize("layout", ["blhd", "bhld"])
def test_ops_attention_dispatch_d512(ext, monkeypatch, layout):
    from dcr_amd import ops
    monkeypatch.delenv("DCR_ATTN_D512", raising=False)
    q, k, v, _, ref = _case(100, 33)
    ql, kl, vl = (_to_layout(t, layout) for t in (q, k, v))
    n0, m0 = _counts()
    with torch.no_grad():
        out = ops.attention(ql, kl, vl, layout=layout)
    assert _counts() == (n0 + 1, m0)
    assert out.shape == ql.shape and out.dtype == torch.bfloat16
    _close(out if layout == "blhd" else out.permute(0, 2, 1, 3), ref, 2e-2)


def test_ops_attention_d512_env_gate(ext, monkeypatch):
    """DCR_ATTN_D512=0 (read per call) restores the composite path."""
    from dcr_amd import ops
    q, k, v, _, ref = _case(100, 33)
    monkeypatch.setenv("DCR_ATTN_D512", "0")
    n0, m0 = _counts()
    with torch.no_grad():
        out = ops.attention(q, k, v, layout="blhd")
    assert _counts() == (n0, m0 + 1)
    _close(out, ref, 2e-2)
    # and back, in the same process
    monkeypatch.setenv("DCR_ATTN_D512", "1")
    with torch.no_grad():
        out = ops.attention(q, k, v, layout="blhd")
    assert _counts() == (n0 + 1, m0 + 1)
    _close(out, ref, 2e-2)


def test_ops_attention_d512_grad_stays_composite(ext, monkeypatch):
    from dcr_amd import ops
    monkeypatch.delenv("DCR_ATTN_D512", raising=False)
    q, k, v, _, ref = _case(100, 33)
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    n0, m0 = _counts()
    out = ops.attention(*leaves, layout="blhd")
    out.float().sum().backward()
    assert _counts() == (n0, m0 + 1)
    _close(out, ref, 2e-2)
    for t in leaves:
        assert t.grad is not None and torch.isfinite(t.grad.float()).all()


def test_ops_attention_d512_causal_stays_composite(ext, monkeypatch):
    from dcr_amd import ops
    monkeypatch.delenv("DCR_ATTN_D512", raising=False)
    q, k, v, scale, _ = _case(64, 64)
    n0, m0 = _counts()
    with torch.no_grad():
        out = ops.attention(q, k, v, causal=True, layout="blhd")
    assert _counts() == (n0, m0 + 1)
    ref = F.scaled_dot_product_attention(
        q.permute(0, 2, 1, 3).float(), k.permute(0, 2, 1, 3).float(),
        v.permute(0, 2, 1, 3).float(), is_causal=True, scale=scale)
    _close(out.permute(0, 2, 1, 3), ref, 2e-2)


def test_ops_attention_d512_fp32_stays_composite(ext, monkeypatch):
    from dcr_amd import ops
    monkeypatch.delenv("DCR_ATTN_D512", raising=False)
    q, k, v, _, ref = _case(64, 64)
    n0, m0 = _counts()
    with torch.no_grad():
        out = ops.attention(q.float(), k.float(), v.float(), layout="blhd")
    assert _counts() == (n0, m0 + 1)
    assert out.dtype == torch.float32
    _close(out, ref, 2e-2)


# ---------------------------------------------------------------- 5. memory
def test_ops_attention_d512_no_l2_allocation(ext, monkeypatch):
    """One fp32 score matrix (L*L*4 = 16 MiB at L=2048) is the least the
    composite path allocates; the native path needs the 2 MiB output."""
    from dcr_amd import ops
    monkeypatch.delenv("DCR_ATTN_D512", raising=False)
    L = 2048
    q, k, v, _, ref = _case(L, L, b=1, h=1)
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = ops.attention(q, k, v, layout="blhd")
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base
    assert extra < L * L * 4, f"peak extra {extra} B >= {L * L * 4} B"
    _close(out, ref, 2e-2)


# ---------------------------------------------------------------- 6. mid block
@pytest.mark.parametrize("channels_last", [False, True])
def test_vae_attention_block(ext, monkeypatch, channels_last):
    from dcr_amd.models.vae import VAEAttention
    torch.manual_seed(0)
    blk = VAEAttention(512, 32).cuda().to(torch.bfloat16)
    x = torch.randn(2, 512, 10, 13, device="cuda").bfloat16()   # L = 130
    if channels_last:
        blk = blk.to(memory_format=torch.channels_last)
        x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        monkeypatch.setenv("DCR_ATTN_D512", "0")
        ref = blk(x)
        monkeypatch.delenv("DCR_ATTN_D512")
        n0, m0 = _counts()
        out = blk(x)
    assert _counts() == (n0 + 1, m0)
    assert out.shape == x.shape
    _close(out, ref, 2e-2)


# ---------------------------------------------------------------- 7. whole VAE
def test_sd_vae_encode_decode(ext, monkeypatch):
    """SD VAE encode of a 64x64 image and decode of an 8x8 latent (L=64):
    one native attention each, none on the composite path, and the same
    result as the gated composite run.

    Bounds (max-abs error over the reference's max-abs). The encode holds
    the project's 2e-2: native against composite measured 0.96e-2 and
    1.16e-2. The decode does not: the layers after the attention amplify
    the difference to 1.6e-2 and 2.1e-2 in two runs of the same process
    (the composite run is itself not bit-reproducible from run to run).
    The composite path's own bf16 decode against an fp32 copy of the VAE on
    the same latent measured 1.76e-2 and 1.90e-2 (the native path's
    1.55e-2 and 1.75e-2), so the decode bound is 2 x 1.90e-2 = 3.8e-2."""
    from dcr_amd.models import AutoencoderKL, VAEConfig
    # an earlier Trainer leaves MIOpen's exhaustive conv search on, which
    # costs minutes at these new conv shapes; no assertion depends on it
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    torch.manual_seed(0)
    vae = AutoencoderKL(VAEConfig.sd()).cuda().to(torch.bfloat16) \
        .to(memory_format=torch.channels_last).eval()
    img = torch.randn(1, 3, 64, 64, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    lat = torch.randn(1, 4, 8, 8, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)

    def run():
        with torch.no_grad():
            return (vae.encode(img).latent_dist.mode(), vae.decode(lat).sample)

    monkeypatch.setenv("DCR_ATTN_D512", "0")
    ref_enc, ref_dec = run()
    monkeypatch.delenv("DCR_ATTN_D512")
    n0, m0 = _counts()
    with torch.no_grad():
        enc = vae.encode(img).latent_dist.mode()
        assert _counts() == (n0 + 1, m0)
        dec = vae.decode(lat).sample
        assert _counts() == (n0 + 2, m0)
    assert enc.shape == (1, 4, 8, 8) and dec.shape == (1, 3, 64, 64)
    assert torch.isfinite(enc.float()).all() and torch.isfinite(dec.float()).all()
    rel = lambda a, b: ((a.float() - b.float()).abs().max() /
                        b.float().abs().max()).item()
    print(f"native vs composite: enc {rel(enc, ref_enc):.3e} "
          f"dec {rel(dec, ref_dec):.3e}")
    _close(enc, ref_enc, 2e-2)
    _close(dec, ref_dec, 3.8e-2)
