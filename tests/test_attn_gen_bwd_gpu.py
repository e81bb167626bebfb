"""Flash attention backward for the SD-1.x head dims 40/80/160
(attn_bwd_*_gen_kernel in dcr_amd/ops/hip/attention.hip), from the raw
bindings up to Trainer(model_size="sd14").

Gradient tolerance: the project's own for the D=64 backward
(test_attn_bwd_v4_matches_ref) — max-abs error below 3e-2 of the
reference's max-abs, for each of dQ, dK and dV, against fp32
scaled_dot_product_attention autograd."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DIMS = [40, 80, 160]
# (Lq, Lk, causal): partial tiles on both axes, a second key tile with 13
# valid keys, a quarter-filled single tile, a causal diagonal with a
# 2-row tail; B*H > 1 for the head stride; randn data for the transposes.
SHAPES = [(64, 64, False), (100, 33, False), (256, 77, False),
          (16, 16, False), (130, 130, True), (64, 64, True)]
B, H = 2, 3


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


def _case(D, Lq, Lk, causal):
    """bf16 inputs [B,L,H,D] and the fp32 SDPA reference grads (same
    layout), computed once per shape and shared read-only."""
    key = (D, Lq, Lk, causal)
    if key not in _CASES:
        gen = torch.Generator(device="cuda").manual_seed(D * 1000 + Lq * 3 + Lk)
        mk = lambda L: torch.randn(B, L, H, D, device="cuda", generator=gen
                                   ).to(torch.bfloat16)
        q, k, v, g = mk(Lq), mk(Lk), mk(Lk), mk(Lq)
        scale = 1.0 / D ** 0.5
        qf, kf, vf = (t.permute(0, 2, 1, 3).float().requires_grad_(True)
                      for t in (q, k, v))
        of = F.scaled_dot_product_attention(qf, kf, vf, is_causal=causal,
                                            scale=scale)
        of.backward(g.permute(0, 2, 1, 3).float())
        ref = tuple(t.grad.permute(0, 2, 1, 3).contiguous()
                    for t in (qf, kf, vf))
        _CASES[key] = (q, k, v, g, scale, of.detach().permute(0, 2, 1, 3), ref)
    return _CASES[key]


# ---------------------------------------------------------------- 1. lse
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("Lq,Lk,causal", SHAPES)
def test_attn_fwd_gen_lse(ext, D, Lq, Lk, causal):
    q, k, v, _, scale, _, _ = _case(D, Lq, Lk, causal)
    o0 = ext.attn_fwd_gen(q, k, v, scale, causal)
    o, lse = ext.attn_fwd_gen_lse(q, k, v, scale, causal)
    assert torch.equal(o, o0)
    assert lse.shape == (B * H, Lq) and lse.dtype == torch.float32
    assert torch.isfinite(lse).all()
    # natural-log LSE of the scaled scores
    s = torch.einsum("blhd,bmhd->bhlm", q.float(), k.float()) * scale
    if causal:
        s = s.masked_fill(~torch.ones(Lq, Lk, dtype=torch.bool,
                                      device="cuda").tril_(), float("-inf"))
    torch.testing.assert_close(lse, s.logsumexp(-1).reshape(B * H, Lq),
                               rtol=1e-3, atol=1e-3)


# ---------------------------------------------------------------- 2. grads
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("Lq,Lk,causal", SHAPES)
def test_attn_bwd_gen_matches_ref(ext, D, Lq, Lk, causal):
    q, k, v, g, scale, _, (rq, rk, rv) = _case(D, Lq, Lk, causal)
    o, lse = ext.attn_fwd_gen_lse(q, k, v, scale, causal)
    dQ, dK, dV = ext.attn_bwd_gen(q, k, v, o, g, lse, scale, causal)
    assert dQ.shape == q.shape and dK.shape == k.shape and dV.shape == v.shape
    assert dQ.dtype == dK.dtype == dV.dtype == torch.bfloat16
    for name, got, ref in (("dQ", dQ, rq), ("dK", dK, rk), ("dV", dV, rv)):
        err = (got.float() - ref).abs().max().item() / ref.abs().max().item()
        print(f"D={D} Lq={Lq} Lk={Lk} causal={causal} {name} rel_err={err:.3e}")
    _close(dQ, rq, 3e-2)
    _close(dK, rk, 3e-2)
    _close(dV, rv, 3e-2)


def test_attn_bwd_gen_packed_3d(ext):
    """[BH, L, D] packed layout (H=1 stride) gives the 4-D layout's grads."""
    D, Lq, Lk = 80, 100, 33
    q, k, v, g, scale, _, (rq, rk, rv) = _case(D, Lq, Lk, False)
    pk = lambda t: t.permute(0, 2, 1, 3).reshape(B * H, t.shape[1], D).contiguous()
    o, lse = ext.attn_fwd_gen_lse(pk(q), pk(k), pk(v), scale, False)
    dQ, dK, dV = ext.attn_bwd_gen(pk(q), pk(k), pk(v), o, pk(g), lse, scale, False)
    _close(dQ, pk(rq), 3e-2)
    _close(dK, pk(rk), 3e-2)
    _close(dV, pk(rv), 3e-2)


def test_attn_bwd_gen_shape_checks(ext):
    q, k, v, g, scale, _, _ = _case(40, 64, 64, False)
    o, lse = ext.attn_fwd_gen_lse(q, k, v, scale, False)
    with pytest.raises(RuntimeError):
        ext.attn_bwd_gen(q, k, v, o, g[:, :32].contiguous(), lse, scale, False)
    with pytest.raises(RuntimeError):
        ext.attn_bwd_gen(q, k, v, o, g, lse[:, :32].contiguous(), scale, False)
    with pytest.raises(RuntimeError):
        ext.attn_bwd_gen(q, k, v, o.float(), g, lse, scale, False)
    q64 = torch.randn(2, 64, 3, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ext.attn_fwd_gen_lse(q64, q64, q64, 0.125, False)


# ---------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("D", DIMS)
def test_attn_bwd_gen_deterministic(ext, D):
    q, k, v, g, scale, _, _ = _case(D, 256, 77, False)
    o, lse = ext.attn_fwd_gen_lse(q, k, v, scale, False)
    a = ext.attn_bwd_gen(q, k, v, o, g, lse, scale, False)
    b = ext.attn_bwd_gen(q, k, v, o, g, lse, scale, False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- 4. dispatch
def _run_ops_attention(q, k, v, g, causal, layout):
    """ops.attention fwd+bwd on leaf copies; g is [B,L,H,D]. The upstream
    grad is made non-contiguous (a transposed view of a dense tensor)."""
    from dcr_amd import ops
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    if layout == "bhld":
        ins = [t.permute(0, 2, 1, 3) for t in leaves]
        out = ops.attention(*ins, causal=causal, layout="bhld")
        up = g.permute(0, 2, 1, 3)               # non-contiguous [B,H,L,D]
    else:
        out = ops.attention(*leaves, causal=causal, layout="blhd")
        up = g.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not up.is_contiguous()
    out.backward(up)
    return out, [t.grad for t in leaves]


@pytest.mark.parametrize("layout", ["blhd", "bhld"])
@pytest.mark.parametrize("D,Lq,Lk,causal", [(40, 100, 33, False),
                                            (80, 130, 130, True),
                                            (160, 16, 16, False)])
def test_ops_attention_grad_dispatch(ext, monkeypatch, layout, D, Lq, Lk, causal):
    from dcr_amd.ops import dispatch_counts
    monkeypatch.delenv("DCR_ATTN_GEN_BWD", raising=False)
    q, k, v, g, _, oref, (rq, rk, rv) = _case(D, Lq, Lk, causal)
    c0 = dict(dispatch_counts)
    out, (dq, dk, dv) = _run_ops_attention(q, k, v, g, causal, layout)
    assert dispatch_counts["attention_gen"] == c0.get("attention_gen", 0) + 1
    assert dispatch_counts["attention_gen_bwd"] == c0.get("attention_gen_bwd", 0) + 1
    assert dispatch_counts["attention_math"] == c0.get("attention_math", 0)
    oo = out if layout == "blhd" else out.permute(0, 2, 1, 3)
    _close(oo, oref, 2e-2)
    _close(dq, rq, 3e-2)
    _close(dk, rk, 3e-2)
    _close(dv, rv, 3e-2)


def test_ops_attention_env_gate_composite(ext, monkeypatch):
    """DCR_ATTN_GEN_BWD=0 (read per call) forces the composite path."""
    from dcr_amd.ops import dispatch_counts
    D, Lq, Lk = 40, 100, 33
    q, k, v, g, _, _, (rq, rk, rv) = _case(D, Lq, Lk, False)
    monkeypatch.setenv("DCR_ATTN_GEN_BWD", "0")
    c0 = dict(dispatch_counts)
    _, (dq, dk, dv) = _run_ops_attention(q, k, v, g, False, "blhd")
    assert dispatch_counts["attention_math"] == c0.get("attention_math", 0) + 1
    assert dispatch_counts["attention_gen"] == c0.get("attention_gen", 0)
    assert dispatch_counts["attention_gen_bwd"] == c0.get("attention_gen_bwd", 0)
    _close(dq, rq, 3e-2)
    _close(dk, rk, 3e-2)
    _close(dv, rv, 3e-2)
    # and back, in the same process
    monkeypatch.setenv("DCR_ATTN_GEN_BWD", "1")
    _run_ops_attention(q, k, v, g, False, "blhd")
    assert dispatch_counts["attention_gen_bwd"] == c0.get("attention_gen_bwd", 0) + 1
    # the gate does not touch the no-grad path
    monkeypatch.setenv("DCR_ATTN_GEN_BWD", "0")
    from dcr_amd import ops
    g0 = dispatch_counts["attention_gen"]
    with torch.no_grad():
        ops.attention(q, k, v, layout="blhd")
    assert dispatch_counts["attention_gen"] == g0 + 1


@pytest.mark.parametrize("D,dtype", [(32, torch.bfloat16), (40, torch.float32)])
def test_ops_attention_other_shapes_stay_composite(ext, monkeypatch, D, dtype):
    from dcr_amd import ops
    from dcr_amd.ops import dispatch_counts
    monkeypatch.delenv("DCR_ATTN_GEN_BWD", raising=False)
    torch.manual_seed(D)
    q, k, v = (torch.randn(2, 20, 3, D, device="cuda", dtype=dtype,
                           requires_grad=True) for _ in range(3))
    c0 = dict(dispatch_counts)
    ops.attention(q, k, v, layout="blhd").float().sum().backward()
    assert dispatch_counts["attention_math"] == c0.get("attention_math", 0) + 1
    assert dispatch_counts["attention_gen"] == c0.get("attention_gen", 0)
    assert dispatch_counts["attention_gen_bwd"] == c0.get("attention_gen_bwd", 0)
    assert q.grad is not None and torch.isfinite(q.grad).all()


# ---------------------------------------------------------------- 5. checkpoint
def test_grad_checkpointing_equal(ext, monkeypatch):
    from torch.utils.checkpoint import checkpoint
    from dcr_amd import ops
    monkeypatch.delenv("DCR_ATTN_GEN_BWD", raising=False)
    q, k, v, g, _, _, _ = _case(80, 100, 33, False)

    def run(ckpt):
        leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        fn = lambda a, b, c: ops.attention(a, b, c, layout="blhd")
        out = checkpoint(fn, *leaves, use_reentrant=False) if ckpt \
            else fn(*leaves)
        out.backward(g)
        return [t.grad for t in leaves]

    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 6. UNet
def _reduced_sd1x_unet_config():
    """SD-1.x UNet cut to three levels: 8 heads at 320/640/1280 channels,
    so head dims 40, 80 and 160 (mid block) all occur."""
    from dcr_amd.models import UNetConfig
    return UNetConfig(
        sample_size=16, block_out_channels=(320, 640, 1280),
        down_block_types=("CrossAttnDownBlock2D",) * 3,
        up_block_types=("CrossAttnUpBlock2D",) * 3,
        layers_per_block=1, attention_head_dim=(8, 8, 8),
        cross_attention_dim=768, use_linear_projection=False)


def test_reduced_sd1x_unet_fwd_bwd(ext, monkeypatch):
    from dcr_amd.models import UNet2DConditionModel
    from dcr_amd.ops import dispatch_counts
    monkeypatch.delenv("DCR_ATTN_GEN_BWD", raising=False)
    # an earlier Trainer leaves MIOpen's exhaustive conv search on, which
    # costs minutes at these new conv shapes; no assertion depends on it
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    torch.manual_seed(0)
    unet = UNet2DConditionModel(_reduced_sd1x_unet_config()).cuda() \
        .to(torch.bfloat16)
    x = torch.randn(2, 4, 16, 16, device="cuda").bfloat16()
    ctx = torch.randn(2, 77, 768, device="cuda").bfloat16()
    math0 = dispatch_counts["attention_math"]
    bwd0 = dispatch_counts["attention_gen_bwd"]
    out = unet(x, torch.tensor([10, 500], device="cuda"), ctx)
    out.float().pow(2).mean().backward()
    assert dispatch_counts["attention_math"] == math0
    assert dispatch_counts["attention_gen_bwd"] > bwd0
    seen = 0
    for name, p in unet.named_parameters():
        if name.endswith(("to_q.weight", "to_k.weight", "to_v.weight")):
            seen += 1
            assert p.grad is not None, name
            assert torch.isfinite(p.grad).all(), name
            assert p.grad.abs().max() > 0, name
    # q/k/v x self+cross x (3 down + 1 mid + 6 up) transformer blocks
    assert seen == 3 * 2 * 10


# ---------------------------------------------------------------- 7. Trainer
def test_trainer_sd14_reduced(ext, tmp_path, monkeypatch):
    from dcr_amd.ops import dispatch_counts
    from dcr_amd.train import TrainConfig, Trainer
    monkeypatch.delenv("DCR_ATTN_GEN_BWD", raising=False)
    cfg_path = tmp_path / "unet_config.json"
    cfg_path.write_text(_reduced_sd1x_unet_config().to_json())
    cfg = TrainConfig(model_size="sd14", unet_from_scratch="yes",
                      unet_config=str(cfg_path), synthetic_data=True,
                      synthetic_size=4, resolution=128, train_batch_size=2,
                      mixed_precision="pure_bf16", channels_last=True,
                      dataloader_num_workers=0, max_train_steps=2, seed=0,
                      learning_rate=1e-4, lr_warmup_steps=1,
                      output_dir=str(tmp_path / "out"))
    tr = Trainer(cfg, device=torch.device("cuda", 0))
    # the Trainer turns on MIOpen's exhaustive conv search, tens of seconds
    # at the first step; nothing asserted here depends on the conv solver
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    assert tr.unet.config.block_out_channels == (320, 640, 1280)
    assert tr.text_encoder.config.hidden_size == 768
    before = tr.optimizer.flat_param.detach().clone()
    bwd0 = dispatch_counts["attention_gen_bwd"]
    batch = next(iter(tr.dataloader))
    losses = [tr.train_step(batch) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(torch.isfinite(l) for l in losses)
    assert not torch.equal(tr.optimizer.flat_param, before)
    assert dispatch_counts["attention_gen_bwd"] > bwd0
