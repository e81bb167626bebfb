"""Native gradient tail (ops/hip/grad_tail.hip + the clip-aware AdamW):
one-launch gather with a fused sum of squares, device-side clip."""
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


def _layout(dtype, integer=False, seed=0):
    """Hand-built arena: (arena, views, grads). Entry kinds: a flat count, the
    gap of unowned elements, a channels-last 4-D weight, and a [K,C,1,1]
    weight whose gradient carries contiguous / channels-last strides."""
    CH = _ch()
    plan = [1, CH + 1, 4, 2 * CH + 3, 7, CH - 1, 8, 320, "gap", 11520, CH,
            "cl4d", "k1_contig", "k1_cl"]
    dev = torch.device("cuda", 0)
    g_ = torch.Generator(device="cpu").manual_seed(seed)

    def values(*shape):
        if integer:
            return torch.randint(-1, 3, shape, generator=g_).float()
        return torch.randn(*shape, generator=g_)

    sizes = []
    for e in plan:
        sizes.append({"gap": GAP, "cl4d": 4 * 6 * 3 * 3, "k1_contig": 32,
                      "k1_cl": 32}.get(e, e))
    arena = torch.full((sum(sizes),), SENTINEL, device=dev, dtype=dtype)
    views, grads, off = [], [], 0
    gap_at = None
    for e, n in zip(plan, sizes):
        sl = arena[off:off + n]
        if e == "gap":
            gap_at = off
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


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_is_a_copy(dtype):
    m = _ext()
    arena, views, grads, gap_at = _layout(dtype)
    es = arena.element_size()
    widths = {_width(g.data_ptr(), v.data_ptr(), es) for g, v in zip(grads, views)}
    assert widths == ({16, 8, 4, 2} if es == 2 else {16, 8, 4}), widths
    assert grads[-1].stride() != views[-1].stride()   # [K,C,1,1], other tuple
    ref = arena.clone()
    ref_views = [ref.as_strided(v.size(), v.stride(),
                                v.storage_offset() - arena.storage_offset())
                 for v in views]
    torch._foreach_copy_(ref_views, grads)
    rejected = m.grad_gather(arena, views, grads, None, _ch(), 0)
    torch.cuda.synchronize()
    assert rejected == []
    assert torch.equal(_bits(arena), _bits(ref))
    assert (arena[gap_at:gap_at + GAP] == SENTINEL).all()
    # a small grid walks several virtual blocks per block: same result
    arena2 = torch.full_like(arena, SENTINEL)
    views2 = [arena2.as_strided(v.size(), v.stride(), v.storage_offset())
              for v in views]
    assert m.grad_gather(arena2, views2, grads, None, _ch(), 3) == []
    assert torch.equal(_bits(arena2), _bits(ref))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_fallback_for_other_dtype_or_strides(dtype, monkeypatch):
    """Through FusedAdamW.gather_grads: a gradient of another dtype is
    converted first (as before), one with other strides takes copy_."""
    from dcr_amd.ops import FusedAdamW, dispatch_counts
    monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", "1")
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(16, 20, device=dev, dtype=dtype)),
          torch.nn.Parameter(torch.randn(37, device=dev, dtype=dtype)),
          torch.nn.Parameter(torch.randn(9, 8, device=dev, dtype=dtype))]
    opt = FusedAdamW(ps)
    other = torch.float32 if dtype == torch.bfloat16 else torch.float64
    gs = [torch.randn(20, 16, device=dev, dtype=dtype).t(),      # strides
          torch.randn(37, device=dev, dtype=other),              # dtype
          torch.randn(9, 8, device=dev, dtype=dtype)]
    ps[1].grad_dtype = None      # allow a gradient of another dtype
    for p, g in zip(ps, gs):
        p.grad = g
    fb0 = dispatch_counts["grad_gather_fallback"]
    opt.gather_grads()
    torch.cuda.synchronize()
    assert dispatch_counts["grad_gather_fallback"] == fb0 + 1
    assert not opt._sumsq_valid
    want = torch.cat([g.to(dtype).contiguous().reshape(-1) for g in gs])
    assert torch.equal(_bits(opt.flat_grad), _bits(want))


def _sumsq(m, arena, views, grads, max_norm=1.0, fused=True, grid=0):
    nvb = sum((v.numel() + _ch() - 1) // _ch() for v in views)
    partials = torch.full((nvb,), float("nan"), device=arena.device)
    if fused:
        assert m.grad_gather(arena, views, grads, partials, _ch(), grid) == []
    else:
        assert m.grad_sumsq(arena, views, partials, _ch(), grid) == nvb
    rec = torch.zeros(3, device=arena.device)
    m.sumsq_finalize(partials, nvb, max_norm, rec)
    return rec.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sumsq_exact_on_integers(dtype):
    m = _ext()
    arena, views, grads, _ = _layout(dtype, integer=True)
    exact = sum(int((g.double() ** 2).sum().item()) for g in grads)
    assert 0 < exact < 2 ** 24
    rec = _sumsq(m, arena, views, grads)
    assert rec[0].item() == float(exact)
    assert rec[1].item() == float(np.float32(np.sqrt(np.float64(exact))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sumsq_bound_repeatable_and_same_standalone(dtype):
    """Error bound from the reduction in grad_tail.hip, all terms >= 0.
    Per lane: head + CH/(16 B group)/256 groups + tail sequential adds
    (bf16: 1 + 8 + 1, fp32: 1 + 16 + 1), the pairwise tree inside a group
    (bf16: 3, fp32: 2), one rounding of each fp32 square (bf16 squares are
    exact), 6 wave-shuffle levels, 4 waves added in order, and the final
    rounding of the fp64 total to fp32: 24 (bf16) / 32 (fp32) roundings,
    each relative 2^-24."""
    m = _ext()
    assert _ch() == 16384, "the chain lengths above are for CH = 16384"
    depth = 24 if dtype == torch.bfloat16 else 32
    bound = (1.0 + 2.0 ** -24) ** depth - 1.0
    arena, views, grads, _ = _layout(dtype, seed=3)
    ref = sum((g.double() ** 2).sum().item() for g in grads)
    a = _sumsq(m, arena, views, grads)
    print(f"sumsq {a[0].item()!r} fp64 {ref!r} rel "
          f"{abs(a[0].item() - ref) / ref:.3e} bound {bound:.3e}")
    assert abs(a[0].item() - ref) <= bound * ref
    b = _sumsq(m, arena, views, grads)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    c = _sumsq(m, arena, views, grads, fused=False)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    d = _sumsq(m, arena, views, grads, fused=False, grid=5)
    assert torch.equal(a.view(torch.int32), d.view(torch.int32))


# ---------------------------------------------------------------- optimizer
def _shapes():
    return [(33, 7), (_ch() + 5,), (8, 4, 3, 3), (1,), (12,)]


def _make_opt(dtype, seed=0):
    from dcr_amd.ops import FusedAdamW
    dev = torch.device("cuda", 0)
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g_).to(dev, dtype))
          for s in _shapes()]
    return FusedAdamW(ps, lr=1e-2), ps


def _int_grads(dtype, seed, ones=None):
    """Integer-valued gradients: every partial sum of squares is exact in
    fp32, so aten's norm and the native one are the same bits. `ones`: only
    that many elements are 1, the rest 0 (norm = sqrt(ones))."""
    dev = torch.device("cuda", 0)
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    left = ones
    for s in _shapes():
        if ones is None:
            g = torch.randint(-2, 3, s, generator=g_).float()
        else:
            g = torch.zeros(s)
            k = min(left, g.numel(), 7)
            g.view(-1)[:k] = 1.0
            left -= k
        out.append(g.to(dev, dtype))
    assert ones is None or left == 0
    return out


def _state(opt):
    ts = {"param": opt.flat_param, "grad": opt.flat_grad,
          "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}
    if opt.master is not None:
        ts["master"] = opt.master
    return ts


def _assert_same_state(a, b):
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(_bits(sa[k]), _bits(sb[k])), k


def _run(opt, ps, grads_per_step, max_norm, monkeypatch, switch, mutate=None):
    """clip + step once per entry of grads_per_step; switch '0' is the
    parent's sequence (clip_grad_norm_ then step)."""
    monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", switch)
    norms = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.clone()
        if mutate is not None:
            mutate(opt, ps, grads)
        if switch == "0":
            n = opt.clip_grad_norm_(max_norm)
            opt.step()
        else:
            n = opt.clip_and_step(max_norm)
        norms.append(float(n))
        opt.zero_grad()
    return norms


CLIP_CASES = {
    # name: (ones, max_norm); ones=None -> random integers in [-2, 2], norm ~ 184
    "above": (None, 1.0),
    "below": (None, 1.0e6),
    "equal": (16, 4.0),      # norm exactly 4: strict '>' does not clip
    "zero": (None, 0.0),     # today: norm > 0 holds, the scale is 0
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clip_and_step_matches_parent_sequence(dtype, case, monkeypatch):
    from dcr_amd.ops import dispatch_counts
    ones, max_norm = CLIP_CASES[case]
    steps = [_int_grads(dtype, 10, ones), _int_grads(dtype, 11, ones)]
    ref, rps = _make_opt(dtype)
    new, nps = _make_opt(dtype)
    rn = _run(ref, rps, steps, max_norm, monkeypatch, "0")
    c0 = dict(dispatch_counts)
    nn_ = _run(new, nps, steps, max_norm, monkeypatch, "1")
    assert nn_ == rn
    if case == "equal":
        assert rn == [4.0, 4.0]
    if case == "zero":   # what clip_grad_norm_(0) does today: gradient -> 0
        assert not ref.flat_grad.any()
    _assert_same_state(ref, new)
    assert dispatch_counts["grad_gather"] == c0.get("grad_gather", 0) + 2
    assert dispatch_counts["adamw_clip"] == c0.get("adamw_clip", 0) + 2
    assert dispatch_counts["grad_sumsq"] == c0.get("grad_sumsq", 0)
    assert dispatch_counts["grad_norm_aten"] == c0.get("grad_norm_aten", 0)
    assert dispatch_counts["grad_gather_foreach"] == c0.get("grad_gather_foreach", 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_and_step_nan_gradient(dtype, monkeypatch):
    steps = [_int_grads(dtype, 12), _int_grads(dtype, 13)]
    steps[0][1][5] = float("nan")
    ref, rps = _make_opt(dtype)
    new, nps = _make_opt(dtype)
    _run(ref, rps, steps, 1.0, monkeypatch, "0")
    _run(new, nps, steps, 1.0, monkeypatch, "1")
    torch.cuda.synchronize()
    sa, sb = _state(ref), _state(new)
    bad = 0
    for k in sa:
        fa, fb = torch.isfinite(sa[k].float()), torch.isfinite(sb[k].float())
        assert torch.equal(fa, fb), k
        bad += int((~fa).sum())
    assert bad > 0


def _add_mode(opt, ps, grads):
    opt.gather_grads()
    for p, g in zip(ps, grads):
        p.grad = g.clone()          # second micro-step: the gather adds


def _simulated_div(opt, ps, grads):
    opt.gather_grads()
    opt.arena_written()
    opt.flat_grad.div_(2)           # integers / 2: exact in bf16 and fp32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("how", ["add", "cold", "div"])
def test_stale_sum_takes_the_standalone_pass(dtype, how, monkeypatch):
    from dcr_amd.ops import dispatch_counts
    full = [_int_grads(dtype, 20), _int_grads(dtype, 21)]
    mutate = None
    if how == "add":
        mutate = _add_mode
    elif how == "div":
        mutate = _simulated_div
    else:       # second cycle: two parameters produce no gradient
        full[1][0] = None
        full[1][3] = None
    ref, rps = _make_opt(dtype)
    new, nps = _make_opt(dtype)
    rn = _run(ref, rps, full, 1.0, monkeypatch, "0", mutate)
    c0 = dict(dispatch_counts)
    nn_ = _run(new, nps, full, 1.0, monkeypatch, "1", mutate)
    want = 1 if how == "cold" else 2
    assert dispatch_counts["grad_sumsq"] == c0.get("grad_sumsq", 0) + want
    assert dispatch_counts["grad_norm_aten"] == c0.get("grad_norm_aten", 0)
    assert nn_ == rn
    _assert_same_state(ref, new)


def test_tiny_train_step_switch_on_and_off(tmp_path, monkeypatch):
    """Two tiny train steps per arm. Backward is not run-to-run
    reproducible, so the arms are compared with the tolerances
    tests/test_bench_contract.py uses for two runs of one build."""
    from dcr_amd import ops
    from dcr_amd.train import TrainConfig, Trainer

    cfg = TrainConfig(model_size="tiny", synthetic_data=True,
                      synthetic_size=4, resolution=64, train_batch_size=2,
                      mixed_precision="pure_bf16", channels_last=True,
                      dataloader_num_workers=0, max_train_steps=2, seed=0,
                      output_dir=str(tmp_path / "o"))
    tr = Trainer(cfg, device=torch.device("cuda", 0))
    batch = next(iter(tr.dataloader))
    opt = tr.optimizer
    start = (opt.flat_param.clone(), opt.master.clone())

    def arm(switch):
        # one Trainer serves both arms: back to the initial weights, zero
        # moments, step 0 and the same noise / timestep draws
        monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", switch)
        opt.flat_param.copy_(start[0])
        opt.master.copy_(start[1])
        opt.exp_avg.zero_()
        opt.exp_avg_sq.zero_()
        opt.step_count = 0
        tr.global_step = 0
        torch.manual_seed(1234)
        ops.dispatch_counts.clear()
        losses = [float(tr.train_step(batch)), float(tr.train_step(batch))]
        torch.cuda.synchronize()
        return (losses, opt.flat_grad.float().cpu().numpy(),
                opt.master.cpu().numpy(), dict(ops.dispatch_counts))

    l0, g0, p0, c0 = arm("0")
    l1, g1, p1, c1 = arm("1")
    assert c1.get("grad_gather") == 2 and c1.get("grad_norm_finalize") == 2
    assert c1.get("adamw_clip") == 2 and c1.get("adamw") == 2
    assert c1.get("grad_sumsq", 0) == 0 and c1.get("grad_gather_fallback", 0) == 0
    assert c1.get("grad_gather_foreach", 0) == 0 and c1.get("grad_norm_aten", 0) == 0
    assert c0.get("grad_gather", 0) == 0 and c0.get("adamw_clip", 0) == 0
    assert c0.get("grad_gather_foreach") == 2 and c0.get("grad_norm_aten") == 2
    assert np.isfinite(l0).all() and np.isfinite(l1).all()
    assert np.allclose(l0, l1, rtol=1e-2)
    assert np.linalg.norm(g0) > 0
    assert np.linalg.norm(g0 - g1) <= 0.05 * np.linalg.norm(g0)
    assert np.abs(p0 - p1).max() <= 4e-5
