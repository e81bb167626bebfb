"""adamw8.hip (AdamW with block-scaled FP8 state) on MI355X against the
CPU reference step of FusedAdamW(state_bits=8)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LR, WD, STEPS = 1e-3, 1e-2, 3
# one pass of a full grid covers 8192 workgroups x 4 waves x 256 elements;
# the last size needs a second grid-stride pass and keeps a partial block
SIZES = [1, 255, 256, 257, 64 * 256 + 37, 8192 * 4 * 256 + 293]
CODE_MISMATCH_CAP = 0.005


@functools.lru_cache(maxsize=None)
def _problem(n, bf16, seed=0):
    """(p0, grads) — shared, never modified in place."""
    gen = torch.Generator().manual_seed(seed)
    scale = 10 ** (-3 * torch.rand(n, generator=gen))
    mu = 0.1 * scale * torch.randn(n, generator=gen)
    p0 = torch.randn(n, generator=gen)
    grads = [mu + scale * torch.randn(n, generator=gen) for _ in range(STEPS)]
    if bf16:
        p0 = p0.bfloat16()
        grads = [g.bfloat16() for g in grads]
    return p0, grads


def _state(opt):
    return {k: getattr(opt, k).detach().cpu().clone() for k in
            ("exp_avg_q", "exp_avg_absmax", "exp_avg_sq_q", "exp_avg_sq_absmax")}


def _weights(opt):
    w = opt.master if opt.master is not None else opt.flat_param
    return w.detach().cpu().clone()


@functools.lru_cache(maxsize=None)
def _cpu_reference(n, bf16):
    """Per step: (weights, state) of the CPU reference; computed once per
    (size, variant) and shared by every test that needs it."""
    from dcr_amd.ops.adamw import FusedAdamW
    p0, grads = _problem(n, bf16)
    param = torch.nn.Parameter(p0.clone())
    opt = FusedAdamW([param], lr=LR, weight_decay=WD, state_bits=8)
    out = []
    for g in grads:
        param.grad = g.clone()
        opt.step()
        opt.zero_grad()
        out.append((_weights(opt), _state(opt)))
    return out


def _check_codes(name, got, want, n):
    """At most 0.5 % of the bytes differ, and only to the adjacent code."""
    diff = got != want
    share = diff.float().mean().item()
    print(f"  {name}: {int(diff.sum())} of {got.numel()} codes differ "
          f"({100 * share:.4f} %)")
    assert share <= CODE_MISMATCH_CAP, (name, share)
    if diff.any():
        a, b = got[diff].int(), want[diff].int()
        assert ((a & 0x80) == (b & 0x80)).all(), f"{name}: sign flipped"
        assert ((a - b).abs() == 1).all(), f"{name}: not the adjacent code"
    assert not got[n:].any(), f"{name}: padding bytes not 0"


def _check_step(step, w, st, ref_w, ref_st, n):
    print(f" step {step}: max |w - ref| = {(w - ref_w).abs().max().item():.3e}")
    if step == 1:
        # zero state in, so no codes are involved yet
        assert (w - ref_w).abs().max().item() <= 1e-5
    for k in ("exp_avg_absmax", "exp_avg_sq_absmax"):
        rel = ((st[k] - ref_st[k]).abs() / ref_st[k].abs().clamp_min(1e-45)).max()
        print(f"  {k}: max rel diff {rel.item():.3e}")
        assert (st[k] - ref_st[k]).abs().le(1e-6 * ref_st[k].abs()).all(), k
    for k in ("exp_avg_q", "exp_avg_sq_q"):
        _check_codes(k, st[k], ref_st[k], n)
    assert not (st["exp_avg_sq_q"] & 0x80).any(), "sqrt(v) code with sign bit"
    if step == STEPS:
        d = (w - ref_w).abs()
        share = (d > 1e-5).float().mean().item()
        print(f"  weights off by > 1e-5: {100 * share:.4f} %, max {d.max().item():.3e}")
        assert share <= CODE_MISMATCH_CAP
        assert d.max().item() <= 10 * LR * 3


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_cpu_reference(n, bf16):
    """Both kernels, 3 steps against the CPU reference.

    The kernel forms its scalars like the reference and compiles with FP
    contraction off. Measured on MI355X, every size and both variants:
    weights and both absmax arrays equal the reference bit for bit, and
    0 of the codes differ (0.0000 %; the cap is 0.5 %)."""
    from dcr_amd import ops
    m = ops.require_hip("adamw8")
    ref = _cpu_reference(n, bf16)
    p0, grads = _problem(n, bf16)
    nb = (n + 255) // 256
    dev = torch.device("cuda", 0)
    p = p0.to(dev)
    master = p.float() if bf16 else None
    mq = torch.zeros(nb * 256, dtype=torch.uint8, device=dev)
    rq = torch.zeros(nb * 256, dtype=torch.uint8, device=dev)
    mabs = torch.zeros(nb, dtype=torch.float32, device=dev)
    rabs = torch.zeros(nb, dtype=torch.float32, device=dev)
    for t, g in enumerate(grads, start=1):
        g = g.to(dev)
        if bf16:
            m.adamw8_step_bf16(p, g, master, mq, mabs, rq, rabs,
                               LR, 0.9, 0.999, 1e-8, WD, t)
        else:
            m.adamw8_step(p, g, mq, mabs, rq, rabs,
                          LR, 0.9, 0.999, 1e-8, WD, t)
        w = (master if bf16 else p).cpu()
        st = {"exp_avg_q": mq.cpu(), "exp_avg_absmax": mabs.cpu(),
              "exp_avg_sq_q": rq.cpu(), "exp_avg_sq_absmax": rabs.cpu()}
        _check_step(t, w, st, ref[t - 1][0], ref[t - 1][1], n)
        if bf16:
            assert torch.equal(p.cpu(), master.cpu().bfloat16())


def test_tiny_moments_become_zero_blocks_not_nan():
    """m' ~ 1e-37 makes 448/absmax overflow: the block, padding included,
    must come out as a zero block exactly as in the CPU reference."""
    from dcr_amd import ops
    from dcr_amd.ops.adamw import FusedAdamW
    m = ops.require_hip("adamw8")
    dev = torch.device("cuda", 0)
    n = 256 + 3
    g = torch.zeros(n)
    g[3], g[5], g[256] = 1e-36, -1e-37, 1e-36
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(1))
    param = torch.nn.Parameter(p0.clone())
    opt = FusedAdamW([param], lr=LR, weight_decay=WD, state_bits=8)
    p = p0.to(dev)
    mq = torch.full((512,), 0, dtype=torch.uint8, device=dev)
    rq = torch.zeros_like(mq)
    mabs = torch.zeros(2, device=dev)
    rabs = torch.zeros(2, device=dev)
    for t in (1, 2):
        param.grad = g.clone()
        opt.step()
        opt.zero_grad()
        m.adamw8_step(p, g.to(dev), mq, mabs, rq, rabs, LR, 0.9, 0.999, 1e-8, WD, t)
        assert not mq.any() and not rq.any()
        assert not mabs.any() and not rabs.any()
        assert torch.equal(mq.cpu(), opt.exp_avg_q)
        assert torch.equal(mabs.cpu(), opt.exp_avg_absmax)
        assert torch.isfinite(p).all()
        assert (p.cpu() - opt.flat_param).abs().max().item() <= 1e-5


def test_binding_rejects_wrong_state_shapes():
    from dcr_amd import ops
    m = ops.require_hip("adamw8")
    dev = torch.device("cuda", 0)
    n = 300
    p = torch.zeros(n, device=dev)
    g = torch.zeros(n, device=dev)
    q = torch.zeros(512, dtype=torch.uint8, device=dev)
    a = torch.zeros(2, device=dev)
    args = (LR, 0.9, 0.999, 1e-8, WD, 1)
    m.adamw8_step(p, g, q, a, q.clone(), a.clone(), *args)
    with pytest.raises(RuntimeError):       # codes one block short
        m.adamw8_step(p, g, q[:256], a, q.clone(), a.clone(), *args)
    with pytest.raises(RuntimeError):       # absmax too long
        m.adamw8_step(p, g, q, torch.zeros(3, device=dev), q.clone(), a.clone(), *args)
    with pytest.raises(RuntimeError):       # codes not uint8
        m.adamw8_step(p, g, q.float(), a, q.clone(), a.clone(), *args)
    with pytest.raises(RuntimeError):       # bf16 params into the fp32 entry
        m.adamw8_step(p.bfloat16(), g, q, a, q.clone(), a.clone(), *args)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_optimizer_dispatches_adamw8_and_matches_cpu(bf16):
    """FusedAdamW(state_bits=8) on the GPU over a small two-layer model:
    counts 'adamw8' (never 'adamw') and follows the same optimizer on the
    CPU under the conditions of the kernel test. Both sides get the
    gradients of the CPU model, so only the optimizer is compared."""
    from dcr_amd import ops
    from dcr_amd.ops.adamw import FusedAdamW
    torch.manual_seed(0)
    dtype = torch.bfloat16 if bf16 else torch.float32

    def make():
        return torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.GELU(),
                                   torch.nn.Linear(53, 11))
    cpu = make()
    gpu = make()
    gpu.load_state_dict(cpu.state_dict())
    cpu.to(dtype)
    gpu.to(torch.device("cuda", 0), dtype=dtype)
    oc = FusedAdamW(cpu.parameters(), lr=LR, weight_decay=WD, state_bits=8)
    og = FusedAdamW(gpu.parameters(), lr=LR, weight_decay=WD, state_bits=8)
    n = oc.numel
    assert og.exp_avg_q.is_cuda and og.exp_avg_q.dtype == torch.uint8
    a8, a32 = ops.dispatch_counts["adamw8"], ops.dispatch_counts["adamw"]
    x = torch.randn(19, 37).to(dtype)
    y = torch.randn(19, 11).to(dtype)
    for t in range(1, STEPS + 1):
        torch.nn.functional.mse_loss(cpu(x).float(), y.float()).backward()
        for pc, pg in zip(cpu.parameters(), gpu.parameters()):
            pg.grad = pc.grad.to(pg.device)
        oc.step()
        og.step()
        oc.zero_grad()
        og.zero_grad()
        _check_step(t, _weights(og), _state(og), _weights(oc), _state(oc), n)
    assert ops.dispatch_counts["adamw8"] == a8 + STEPS
    assert ops.dispatch_counts["adamw"] == a32
    # the model's parameters are views of the arena the kernel wrote
    assert torch.equal(next(gpu.parameters()).detach().reshape(-1),
                       og.flat_param[:37 * 53])


def test_tiny_train_step_8bit_adam_gpu(tmp_path):
    from dcr_amd import ops
    from dcr_amd.train import TrainConfig, Trainer
    cfg = TrainConfig(model_size="tiny", synthetic_data=True, synthetic_size=4,
                      resolution=64, train_batch_size=2,
                      mixed_precision="pure_bf16", use_8bit_adam=True,
                      dataloader_num_workers=0, max_train_steps=2, seed=0,
                      learning_rate=1e-4, lr_warmup_steps=1,
                      output_dir=str(tmp_path / "o"))
    tr = Trainer(cfg, device=torch.device("cuda", 0))
    assert tr.optimizer.state_bits == 8 and tr.optimizer.exp_avg is None
    a8, a32 = ops.dispatch_counts["adamw8"], ops.dispatch_counts["adamw"]
    before = tr.optimizer.master.clone()
    loss = tr.train_step(next(iter(tr.dataloader)))
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert not torch.equal(tr.optimizer.master, before), "params did not move"
    assert torch.equal(tr.optimizer.flat_param, tr.optimizer.master.bfloat16())
    assert ops.dispatch_counts["adamw8"] == a8 + 1
    assert ops.dispatch_counts["adamw"] == a32
    assert tr.optimizer.exp_avg_absmax.max().item() > 0
    with pytest.raises(AssertionError, match="8-bit"):
        tr.enable_hipgraph(next(iter(tr.dataloader)))
