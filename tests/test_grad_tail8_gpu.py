"""Native gradient tail with FP8 optimizer state: the clip-aware
adamw8_kernel<P, true> (ops/hip/adamw8.hip) behind FusedAdamW.clip_and_step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
FLAT_N = 3 * 256 + 5     # partial last quantisation block, length % 4 != 0
SENTINEL = -7.0


def _ext():
    from dcr_amd.ops import require_hip
    return require_hip("grad_tail")


def _ch():
    from dcr_amd.ops.adamw import GATHER_CH
    return GATHER_CH


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


SHAPES = {
    "multi": lambda: [(33, 7), (_ch() + 5,), (8, 4, 3, 3), (1,), (12,)],
    "flat": lambda: [(FLAT_N,)],
}


def _make_opt(dtype, layout, device="cuda", seed=0):
    from dcr_amd.ops import FusedAdamW
    dev = torch.device(device, 0) if device == "cuda" else torch.device("cpu")
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g_).to(dev, dtype))
          for s in SHAPES[layout]()]
    return FusedAdamW(ps, lr=1e-2, state_bits=8), ps


def _int_grads(dtype, layout, seed, ones=None):
    """Integer-valued gradients (on the CPU; _run moves them): every partial
    sum of squares is exact in fp32, so aten's norm and the native one are the
    same bits. `ones`: only that many elements are 1, the rest 0."""
    g_ = torch.Generator(device="cpu").manual_seed(seed)
    shapes = SHAPES[layout]()
    out = []
    left = ones
    for s in shapes:
        if ones is None:
            g = torch.randint(-2, 3, s, generator=g_).float()
        else:
            g = torch.zeros(s)
            k = min(left, g.numel(), 7 if len(shapes) > 1 else left)
            g.view(-1)[:k] = 1.0
            left -= k
        out.append(g.to(dtype))
    assert ones is None or left == 0
    return out


def _state(opt):
    ts = {"param": opt.flat_param, "grad": opt.flat_grad,
          "exp_avg_q": opt.exp_avg_q, "exp_avg_absmax": opt.exp_avg_absmax,
          "exp_avg_sq_q": opt.exp_avg_sq_q,
          "exp_avg_sq_absmax": opt.exp_avg_sq_absmax}
    if opt.master is not None:
        ts["master"] = opt.master
    return ts


def _assert_same_state(a, b):
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(_bits(sa[k]).cpu(), _bits(sb[k]).cpu()), k


def _run(opt, ps, grads_per_step, max_norm, monkeypatch, switch):
    """clip + step once per entry of grads_per_step; switch '0' is the
    parent's sequence (clip_grad_norm_ then step), also what the CPU runs."""
    monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", switch)
    norms = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = g.to(p.device).clone()
        if switch == "0":
            n = opt.clip_grad_norm_(max_norm)
            opt.step()
        else:
            n = opt.clip_and_step(max_norm)
        norms.append(float(n))
        opt.zero_grad()
    return norms


CLIP_CASES = {
    # name: (ones, max_norm); ones=None -> random integers in [-2, 2]
    "above": (None, 1.0),
    "below": (None, 1.0e6),
    "equal": (16, 4.0),      # norm exactly 4: strict '>' does not clip
    "zero": (None, 0.0),     # norm > 0 holds, the scale is 0
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", list(SHAPES))
@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clip_and_step8_matches_parent_sequence_and_cpu(dtype, layout, case,
                                                        monkeypatch):
    from dcr_amd.ops import dispatch_counts
    ones, max_norm = CLIP_CASES[case]
    steps = [_int_grads(dtype, layout, 10, ones),
             _int_grads(dtype, layout, 11, ones)]
    ref, rps = _make_opt(dtype, layout)
    new, nps = _make_opt(dtype, layout)
    cpu, cps = _make_opt(dtype, layout, device="cpu")
    rn = _run(ref, rps, steps, max_norm, monkeypatch, "0")
    c0 = dict(dispatch_counts)
    nn_ = _run(new, nps, steps, max_norm, monkeypatch, "1")
    c1 = dict(dispatch_counts)
    cn = _run(cpu, cps, steps, max_norm, monkeypatch, "0")
    assert nn_ == rn
    assert nn_ == cn
    if case == "equal":
        assert rn == [4.0, 4.0]
    if case == "zero":
        assert not ref.flat_grad.any()
    _assert_same_state(ref, new)
    # the CPU step is the kernel's bit-exact twin: no tolerance
    _assert_same_state(cpu, new)
    # padding bytes of the code arrays past numel stay 0
    for q in (new.exp_avg_q, new.exp_avg_sq_q):
        assert q.numel() % 256 == 0 and q.numel() >= new.numel
        assert not q[new.numel:].any()
    if case != "zero":       # a zeroed gradient leaves zero moments
        assert new.exp_avg_q[: new.numel].any()

    def d(k):
        return c1.get(k, 0) - c0.get(k, 0)
    assert d("adamw8_clip") == 2 and d("adamw8") == 2
    assert d("grad_gather") == 2
    assert d("grad_norm_aten") == 0
    assert d("grad_gather_foreach") == 0
    assert d("grad_sumsq") == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_clipped_store_back_stays_inside_the_arena(dtype):
    """The binding alone on hand-built buffers: with coef != 1 the arena
    becomes `g.mul_(coef.to(dtype))`, and the elements directly after the
    FLAT_N-element gradient, parameter and master slices are not touched."""
    m = _ext()
    dev = torch.device("cuda", 0)
    n, pad = FLAT_N, 16
    g_ = torch.Generator(device="cpu").manual_seed(5)
    bufs = {}
    for k, dt in (("p", dtype), ("g", dtype), ("master", torch.float32)):
        bufs[k] = torch.full((n + pad,), SENTINEL, device=dev, dtype=dt)
    g0 = torch.randint(-2, 3, (n,), generator=g_).float().to(dev, dtype)
    p0 = torch.randn(n, generator=g_).to(dev, dtype)
    bufs["g"][:n] = g0
    bufs["p"][:n] = p0
    bufs["master"][:n] = p0.float()
    nb = (n + 255) // 256
    mq = torch.zeros(nb * 256, device=dev, dtype=torch.uint8)
    rq = torch.zeros(nb * 256, device=dev, dtype=torch.uint8)
    mabs = torch.zeros(nb, device=dev)
    rabs = torch.zeros(nb, device=dev)
    coef = torch.tensor(0.3, device=dev)
    rec = torch.stack([torch.tensor(0.0, device=dev),
                       torch.tensor(0.0, device=dev), coef])
    hyper = (1e-2, 0.9, 0.999, 1e-8, 1e-2, 1)
    if dtype == torch.bfloat16:
        m.adamw8_step_bf16_clip(bufs["p"][:n], bufs["g"][:n],
                                bufs["master"][:n], mq, mabs, rq, rabs,
                                *hyper, rec)
    else:
        m.adamw8_step_clip(bufs["p"][:n], bufs["g"][:n], mq, mabs, rq, rabs,
                           *hyper, rec)
    torch.cuda.synchronize()
    want = g0.clone().mul_(coef.to(dtype))
    assert torch.equal(_bits(bufs["g"][:n]), _bits(want))
    assert not torch.equal(_bits(want), _bits(g0))
    assert (bufs["g"][n:] == SENTINEL).all()
    assert (bufs["p"][n:] == SENTINEL).all()
    if dtype == torch.bfloat16:
        assert (bufs["master"][n:] == SENTINEL).all()
        assert not torch.equal(bufs["master"][:n], p0.float())
    assert not torch.equal(_bits(bufs["p"][:n]), _bits(p0))
    assert not mq[n:].any() and not rq[n:].any()
    assert mq[:n].any() and rq[:n].any()


def _finite(t):
    if t.dtype == torch.uint8:      # FP8 codes: 0x7f / 0xff are NaN
        t = t.cpu().view(torch.float8_e4m3fn)
    return torch.isfinite(t.float()).cpu()


@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_and_step8_nan_gradient(dtype, monkeypatch):
    steps = [_int_grads(dtype, "multi", 12), _int_grads(dtype, "multi", 13)]
    steps[0][1][5] = float("nan")
    ref, rps = _make_opt(dtype, "multi")
    new, nps = _make_opt(dtype, "multi")
    _run(ref, rps, steps, 1.0, monkeypatch, "0")
    _run(new, nps, steps, 1.0, monkeypatch, "1")
    torch.cuda.synchronize()
    sa, sb = _state(ref), _state(new)
    bad = 0
    for k in sa:
        fa, fb = _finite(sa[k]), _finite(sb[k])
        assert torch.equal(fa, fb), k
        bad += int((~fa).sum())
    assert bad > 0


def test_tiny_train_step_8bit_takes_the_native_tail(tmp_path, monkeypatch):
    from dcr_amd import ops
    from dcr_amd.train import TrainConfig, Trainer

    monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", "1")
    cfg = TrainConfig(model_size="tiny", synthetic_data=True,
                      synthetic_size=4, resolution=64, train_batch_size=2,
                      mixed_precision="pure_bf16", channels_last=True,
                      use_8bit_adam=True, dataloader_num_workers=0,
                      max_train_steps=2, seed=0,
                      output_dir=str(tmp_path / "o"))
    tr = Trainer(cfg, device=torch.device("cuda", 0))
    assert tr.optimizer.state_bits == 8
    batch = next(iter(tr.dataloader))
    ops.dispatch_counts.clear()
    losses = [float(tr.train_step(batch)), float(tr.train_step(batch))]
    torch.cuda.synchronize()
    c = dict(ops.dispatch_counts)
    assert c.get("adamw8_clip") == 2 and c.get("adamw8") == 2
    assert c.get("grad_norm_aten", 0) == 0
    assert c.get("grad_gather") == 2 and c.get("grad_norm_finalize") == 2
    assert np.isfinite(losses).all()
    assert torch.isfinite(tr.optimizer.master).all()
