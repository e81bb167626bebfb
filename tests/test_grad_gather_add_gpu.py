"""Add mode of grad_gather_kernel (ops/hip/grad_tail.hip): gradient
accumulation micro-steps add into the flat arena in one launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
SENTINEL = -7.0
GAP = 5


def _ext():
    from dcr_amd.ops import require_hip
    return require_hip("grad_tail")


def _ch():
    from dcr_amd.ops.adamw import GATHER_CH
    return GATHER_CH


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _width(src_ptr, dst_ptr, es):
    d = (src_ptr - dst_ptr) % 16
    for w in (16, 8, 4, 2):
        if d % w == 0 and w >= es:
            return w
    raise AssertionError((src_ptr, dst_ptr))


def _layout(dtype, seed=0):
    """Hand-built arena of random values: (arena, views, grads, gap_at).
    Entry kinds: a flat count, the gap of unowned elements (sentinels), a
    channels-last 4-D weight, and a [K,C,1,1] weight whose gradient carries
    contiguous / channels-last strides. Gradients are random, not integers:
    every add rounds."""
    CH = _ch()
    plan = [1, CH + 1, 4, 2 * CH + 3, 7, CH - 1, 8, 320, "gap", 11520, CH,
            "cl4d", "k1_contig", "k1_cl"]
    dev = torch.device("cuda", 0)
    g_ = torch.Generator(device="cpu").manual_seed(seed)

    def values(*shape):
        return torch.randn(*shape, generator=g_)

    sizes = []
    for e in plan:
        sizes.append({"gap": GAP, "cl4d": 4 * 6 * 3 * 3, "k1_contig": 32,
                      "k1_cl": 32}.get(e, e))
    arena = (3.0 * values(sum(sizes))).to(dev, dtype)
    views, grads, off = [], [], 0
    gap_at = None
    for e, n in zip(plan, sizes):
        sl = arena[off:off + n]
        if e == "gap":
            gap_at = off
            sl.fill_(SENTINEL)
        elif e == "cl4d":
            views.append(sl.view(4, 3, 3, 6).permute(0, 3, 1, 2))
            grads.append(values(4, 6, 3, 3).to(dev, dtype).contiguous(
                memory_format=torch.channels_last))
        elif e in ("k1_contig", "k1_cl"):
            views.append(sl.view(8, 4, 1, 1))
            g = torch.empty_strided(
                (8, 4, 1, 1), (4, 1, 1, 1) if e == "k1_contig" else (4, 1, 4, 4),
                device=dev, dtype=dtype)
            g.copy_(values(8, 4, 1, 1))
            grads.append(g)
        else:
            views.append(sl)
            grads.append(values(n).to(dev, dtype))
        off += n
    return arena, views, grads, gap_at


def _views_on(other, arena, views):
    return [other.as_strided(v.size(), v.stride(),
                             v.storage_offset() - arena.storage_offset())
            for v in views]


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_mode_is_foreach_add(dtype):
    m = _ext()
    arena, views, grads, gap_at = _layout(dtype)
    es = arena.element_size()
    widths = {_width(g.data_ptr(), v.data_ptr(), es) for g, v in zip(grads, views)}
    assert widths == ({16, 8, 4, 2} if es == 2 else {16, 8, 4}), widths
    assert grads[-1].stride() != views[-1].stride()   # [K,C,1,1], other tuple
    start = arena.clone()
    ref = arena.clone()
    torch._foreach_add_(_views_on(ref, arena, views), grads)
    assert not torch.equal(_bits(ref), _bits(start))
    arena2 = start.clone()
    views2 = _views_on(arena2, arena, views)
    rejected = m.grad_gather(arena, views, grads, None, _ch(), 0, True)
    torch.cuda.synchronize()
    assert rejected == []
    assert torch.equal(_bits(arena), _bits(ref))
    assert (arena[gap_at:gap_at + GAP] == SENTINEL).all()
    # a small grid walks several virtual blocks per block: same result
    assert m.grad_gather(arena2, views2, grads, None, _ch(), 3, add=True) == []
    torch.cuda.synchronize()
    assert torch.equal(_bits(arena2), _bits(ref))


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_mode_takes_no_partials_and_copy_mode_is_unchanged(dtype):
    m = _ext()
    arena, views, grads, _ = _layout(dtype, seed=1)
    nvb = sum((v.numel() + _ch() - 1) // _ch() for v in views)
    partials = torch.zeros(nvb, device=arena.device)
    with pytest.raises(RuntimeError):
        m.grad_gather(arena, views, grads, partials, _ch(), 0, True)
    # the six-argument positional call is still the copy
    ref = arena.clone()
    torch._foreach_copy_(_views_on(ref, arena, views), grads)
    assert m.grad_gather(arena, views, grads, None, _ch(), 0) == []
    torch.cuda.synchronize()
    assert torch.equal(_bits(arena), _bits(ref))


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_mode_rejects_other_dtype_and_strides(dtype):
    m = _ext()
    dev = torch.device("cuda", 0)
    g_ = torch.Generator(device="cpu").manual_seed(2)
    arena = torch.randn(320 + 37 + 72, generator=g_).to(dev, dtype)
    views = [arena[:320].view(16, 20), arena[320:357], arena[357:].view(9, 8)]
    other = torch.float32 if dtype == torch.bfloat16 else torch.float64
    grads = [torch.randn(20, 16, generator=g_).to(dev, dtype).t(),   # strides
             torch.randn(37, generator=g_).to(dev, other),           # dtype
             torch.randn(9, 8, generator=g_).to(dev, dtype)]
    start = arena.clone()
    rejected = m.grad_gather(arena, views, grads, None, _ch(), 0, True)
    torch.cuda.synchronize()
    assert rejected == [0, 1]
    assert torch.equal(_bits(arena[:357]), _bits(start[:357]))
    want = start[357:].view(9, 8).clone().add_(grads[2])
    assert torch.equal(_bits(arena[357:].view(9, 8)), _bits(want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_grads_add_fallback(dtype, monkeypatch):
    """Through FusedAdamW.gather_grads: a second gradient with other strides
    takes add_, the rest the add-mode launch; equal to _foreach_add_."""
    from dcr_amd.ops import FusedAdamW, dispatch_counts
    dev = torch.device("cuda", 0)

    def arm(switch):
        monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", switch)
        g_ = torch.Generator(device="cpu").manual_seed(3)
        ps = [torch.nn.Parameter(torch.randn(16, 20, generator=g_).to(dev, dtype)),
              torch.nn.Parameter(torch.randn(37, generator=g_).to(dev, dtype)),
              torch.nn.Parameter(torch.randn(9, 8, generator=g_).to(dev, dtype))]
        opt = FusedAdamW(ps)
        for rnd in range(2):
            gs = [torch.randn(20, 16, generator=g_).to(dev, dtype).t(),
                  torch.randn(37, generator=g_).to(dev, dtype),
                  torch.randn(9, 8, generator=g_).to(dev, dtype)]
            for p, g in zip(ps, gs):
                p.grad = g
            opt.gather_grads()
        torch.cuda.synchronize()
        assert not opt._sumsq_valid
        return opt.flat_grad.clone()

    g0 = arm("0")
    c0 = dict(dispatch_counts)
    g1 = arm("1")
    assert dispatch_counts["grad_gather_add"] == c0.get("grad_gather_add", 0) + 1
    # one rejected entry in the copy round, one in the add round
    assert dispatch_counts["grad_gather_fallback"] == \
        c0.get("grad_gather_fallback", 0) + 2
    assert torch.equal(_bits(g0), _bits(g1))


# ---------------------------------------------------------------- optimizer
def _shapes():
    return [(33, 7), (_ch() + 5,), (8, 4, 3, 3), (1,), (12,)]


def _make_opt(dtype, state_bits, seed=0):
    from dcr_amd.ops import FusedAdamW
    dev = torch.device("cuda", 0)
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g_).to(dev, dtype))
          for s in _shapes()]
    return FusedAdamW(ps, lr=1e-2, state_bits=state_bits), ps


def _int_grads(dtype, seed):
    dev = torch.device("cuda", 0)
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randint(-2, 3, s, generator=g_).float().to(dev, dtype)
            for s in _shapes()]


def _state(opt):
    ts = {"param": opt.flat_param, "grad": opt.flat_grad}
    if opt.state_bits == 8:
        ts.update(exp_avg_q=opt.exp_avg_q, exp_avg_absmax=opt.exp_avg_absmax,
                  exp_avg_sq_q=opt.exp_avg_sq_q,
                  exp_avg_sq_absmax=opt.exp_avg_sq_absmax)
    else:
        ts.update(exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq)
    if opt.master is not None:
        ts["master"] = opt.master
    return ts


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("state_bits", [32, 8])
def test_accumulation_cycles_match_the_switch_off(dtype, state_bits, monkeypatch):
    """Two cycles of three micro-steps of integer gradients (sums and their
    squares stay exact), a gather after each, then clip_and_step."""
    from dcr_amd.ops import dispatch_counts

    def arm(switch):
        monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", switch)
        opt, ps = _make_opt(dtype, state_bits)
        norms, per_cycle = [], []
        for cycle in range(2):
            c0 = dict(dispatch_counts)
            for micro in range(3):
                for p, g in zip(ps, _int_grads(dtype, 30 + 3 * cycle + micro)):
                    p.grad = g
                opt.gather_grads()
                assert all(p.grad is None for p in ps)
            norms.append(float(opt.clip_and_step(1.0)))
            opt.zero_grad()
            per_cycle.append({k: dispatch_counts[k] - c0.get(k, 0)
                              for k in ("grad_gather", "grad_gather_add",
                                        "grad_sumsq", "grad_norm_aten",
                                        "grad_gather_fallback")})
        torch.cuda.synchronize()
        return opt, norms, per_cycle

    ref, rn, rc = arm("0")
    new, nn_, nc = arm("1")
    assert nn_ == rn
    assert all(n > 1.0 for n in nn_)
    sa, sb = _state(ref), _state(new)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k].view(torch.uint8), sb[k].view(torch.uint8)), k
    for c in nc:
        assert c == {"grad_gather": 1, "grad_gather_add": 2, "grad_sumsq": 1,
                     "grad_norm_aten": 0, "grad_gather_fallback": 0}
    for c in rc:
        assert c["grad_gather_add"] == 0 and c["grad_norm_aten"] == 1


# ------------------------------------------------------------------ trainer
def test_tiny_trainer_accumulates_through_the_arena(tmp_path, monkeypatch):
    """One accumulation cycle (micro-step + sync step) per arm. Backward is
    not run-to-run reproducible, so the arms are compared with the
    tolerances of test_tiny_train_step_switch_on_and_off."""
    from dcr_amd import ops
    from dcr_amd.train import TrainConfig, Trainer

    cfg = TrainConfig(model_size="tiny", synthetic_data=True,
                      synthetic_size=4, resolution=64, train_batch_size=2,
                      mixed_precision="pure_bf16", channels_last=True,
                      gradient_accumulation_steps=2,
                      dataloader_num_workers=0, max_train_steps=2, seed=0,
                      output_dir=str(tmp_path / "o"))
    tr = Trainer(cfg, device=torch.device("cuda", 0))
    batch = next(iter(tr.dataloader))
    opt = tr.optimizer
    start = (opt.flat_param.clone(), opt.master.clone())

    def arm(switch):
        monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", switch)
        opt.flat_param.copy_(start[0])
        opt.master.copy_(start[1])
        opt.exp_avg.zero_()
        opt.exp_avg_sq.zero_()
        opt.step_count = 0
        tr.global_step = 0
        torch.manual_seed(1234)
        ops.dispatch_counts.clear()
        losses = [float(tr.train_step(batch, sync_gradients=False))]
        assert all(p.grad is None for p in opt.params)
        assert len(opt._gathered) == len(opt.params)
        assert tr.global_step == 0
        losses.append(float(tr.train_step(batch, sync_gradients=True)))
        torch.cuda.synchronize()
        assert tr.global_step == 1
        return (losses, opt.flat_grad.float().cpu().numpy(),
                opt.master.cpu().numpy(), dict(ops.dispatch_counts))

    l0, g0, p0, c0 = arm("0")
    l1, g1, p1, c1 = arm("1")
    assert c1.get("grad_gather_add", 0) >= 1 and c1.get("grad_gather") == 1
    assert c1.get("grad_sumsq") == 1 and c1.get("grad_norm_aten", 0) == 0
    assert c1.get("adamw_clip") == 1
    assert c0.get("grad_gather_add", 0) == 0 and c0.get("grad_gather", 0) == 0
    assert np.isfinite(l0).all() and np.isfinite(l1).all()
    assert np.allclose(l0, l1, rtol=1e-2)
    assert np.linalg.norm(g0) > 0
    assert np.linalg.norm(g0 - g1) <= 0.05 * np.linalg.norm(g0)
    assert np.abs(p0 - p1).max() <= 4e-5
