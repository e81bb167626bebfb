"""FusedAdamW(state_bits=8) / --use_8bit_adam on the CPU: the block-scaled
FP8 state format, the reference step, checkpoints, trainer and CLI."""
import copy
import importlib.util
import math
from pathlib import Path

import pytest
import torch

from dcr_amd.ops.adamw import (FusedAdamW, QBLOCK, dequantize_blockwise,
                               quantize_blockwise)
from dcr_amd.train import TrainConfig, Trainer, validate

ROOT = Path(__file__).resolve().parent.parent


def _nblocks(n):
    return (n + QBLOCK - 1) // QBLOCK


def _grad_problem(n, seed):
    """Per-element gradient scales over three decades with a small mean:
    g_t = mu + scale * randn."""
    gen = torch.Generator().manual_seed(seed)
    scale = 10 ** (-3 * torch.rand(n, generator=gen))
    mu = 0.1 * scale * torch.randn(n, generator=gen)
    p0 = torch.randn(n, generator=gen)

    def grad():
        return mu + scale * torch.randn(n, generator=gen)

    return p0, grad


def _opt(p0, dtype=torch.float32, **kw):
    param = torch.nn.Parameter(p0.clone().to(dtype))
    kw.setdefault("lr", 1e-3)
    kw.setdefault("weight_decay", 1e-2)
    return param, FusedAdamW([param], **kw)


def _step(param, opt, g):
    param.grad = g.to(param.dtype)
    opt.step()
    opt.zero_grad()


# ---------------------------------------------------------------- 1. format
@pytest.mark.parametrize("d", [0, 2, 4, 6, 8])
def test_roundtrip_within_format_bound(d):
    """|dq(q(x)) - x| <= max(half an ulp of 3 mantissa bits, half the
    subnormal spacing), elementwise, with 1e-4 slack for the fp32 scales."""
    gen = torch.Generator().manual_seed(d)
    x = torch.randn(4096, 256, generator=gen) * \
        10 ** (-d * torch.rand(4096, 256, generator=gen))
    codes, absmax = quantize_blockwise(x.reshape(-1))
    assert codes.dtype == torch.uint8 and codes.numel() == x.numel()
    assert absmax.dtype == torch.float32 and absmax.numel() == 4096
    assert torch.equal(absmax, x.abs().amax(dim=1))
    y = dequantize_blockwise(codes, absmax, x.numel()).view_as(x)
    assert torch.isfinite(y).all()
    bound = (1 + 1e-4) * torch.maximum(
        2.0 ** -4 * x.abs(), (2.0 ** -10 * absmax / 448)[:, None])
    ratio = ((y - x).abs() / bound).max().item()
    print(f"d={d}: worst error/bound {ratio:.5f}")
    assert ratio <= 1.0


def test_zero_block_tiny_block_and_partial_block():
    x = torch.zeros(3 * 256)
    x[256:512] = -0.0                       # negative zeros are still code 0
    x[512 + 17] = 1e-30                     # lone tiny value round-trips
    codes, absmax = quantize_blockwise(x)
    assert torch.equal(codes[:512], torch.zeros(512, dtype=torch.uint8))
    assert absmax[0] == 0 and absmax[1] == 0
    y = dequantize_blockwise(codes, absmax, x.numel())
    assert torch.equal(y[:512], torch.zeros(512))
    assert y[512 + 17].item() == pytest.approx(1e-30, rel=1e-6)
    assert (y[512:] != 0).sum() == 1

    x = torch.randn(257)
    codes, absmax = quantize_blockwise(x)
    assert codes.numel() == 512 and absmax.numel() == 2
    assert torch.equal(codes[257:], torch.zeros(255, dtype=torch.uint8))
    assert absmax[1] == x[256].abs()
    y = dequantize_blockwise(codes, absmax, 257)
    assert y.numel() == 257
    # the block max takes code 448: exact up to the rounding of absmax/448
    assert y[256].item() == pytest.approx(x[256].item(), rel=1e-6)


def test_block_below_scale_overflow_is_a_zero_block():
    """448/absmax overflows below ~1.3e-36; the block's zeros (padding too)
    must not turn into NaN codes: it is stored as a zero block."""
    x = torch.zeros(256 + 3)
    x[3] = 1e-37
    x[5] = -1e-38
    x[256] = 1e-37                          # partial block with padding
    codes, absmax = quantize_blockwise(x)
    assert not codes.any()
    assert torch.equal(absmax, torch.zeros(2))
    y = dequantize_blockwise(codes, absmax, x.numel())
    assert torch.equal(y, torch.zeros_like(x))
    # just above the overflow the block is kept, zeros stay code 0
    x = torch.zeros(256)
    x[3] = 2e-36
    codes, absmax = quantize_blockwise(x)
    assert absmax[0] == x[3] and codes[3] == 0x7E
    assert int((codes != 0).sum()) == 1
    y = dequantize_blockwise(codes, absmax, 256)
    assert torch.isfinite(y).all() and y[3].item() == pytest.approx(2e-36, rel=1e-5)


def test_decaying_first_moment_never_goes_nan():
    """Zero gradients after one step: m decays by 0.9 per step through the
    scale-overflow window (~step 800) down to nothing; state and params
    stay finite all the way."""
    p0 = torch.randn(300, generator=torch.Generator().manual_seed(0))
    param, opt = _opt(p0, state_bits=8, weight_decay=0.0)
    _step(param, opt, torch.full((300,), 1e-3))
    zero = torch.zeros(300)
    for _ in range(900):
        _step(param, opt, zero)
    assert torch.isfinite(opt.flat_param).all()
    assert torch.isfinite(opt.exp_avg_absmax).all()
    assert not opt.exp_avg_q.any() and not opt.exp_avg_absmax.any()
    m = dequantize_blockwise(opt.exp_avg_q, opt.exp_avg_absmax, 300)
    assert torch.equal(m, torch.zeros(300))


def test_codes_are_ocp_e4m3fn():
    """448 -> 0x7e, 1.0 -> 0x38 (bias 7; FNUZ would give 0x40)."""
    x = torch.zeros(256)
    x[0], x[1], x[2] = 448.0, 1.0, -1.0
    codes, absmax = quantize_blockwise(x)
    assert absmax[0] == 448
    assert codes[:3].tolist() == [0x7E, 0x38, 0xB8]


# ------------------------------------------------- 2. first step from zero
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_first_step_matches_torch_adamw(dtype):
    """State is zero, and the update uses the unquantised m', v': step 1 is
    plain AdamW. bf16 params are compared on the fp32 master."""
    n = 5 * 256 + 37
    p0, grad = _grad_problem(n, seed=3)
    p0 = p0.to(dtype).float()
    g = grad().to(dtype)
    param, opt = _opt(p0, dtype, state_bits=8)
    _step(param, opt, g)
    ref = torch.nn.Parameter(p0.clone())
    topt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=1e-2)
    ref.grad = g.float()
    topt.step()
    got = opt.master if dtype == torch.bfloat16 else opt.flat_param
    err = (got - ref.detach()).abs().max().item()
    print(f"{dtype}: first-step max abs diff {err:.3e}")
    assert err <= 1e-6
    if dtype == torch.bfloat16:
        assert torch.equal(opt.flat_param, opt.master.to(torch.bfloat16))


# --------------------------------------------------- 3. 50-step fidelity
@pytest.mark.parametrize("bf16_grads", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fidelity_50_steps_vs_torch_adamw(seed, bf16_grads):
    """Relative deviation of the 50-step parameter displacement from
    torch.optim.AdamW in fp32, ||(p8-p0)-(p32-p0)|| / ||p32-p0||.
    Measured: 0.0609-0.0616 with fp32 gradients and 0.0611-0.0618 with
    bf16-rounded ones, seeds 0-2. Bound 0.10."""
    n = 64 * 256 + 37
    p0, grad = _grad_problem(n, seed)
    param, opt = _opt(p0, state_bits=8)
    ref = torch.nn.Parameter(p0.clone())
    topt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=1e-2)
    for _ in range(50):
        g = grad()
        if bf16_grads:
            g = g.bfloat16().float()
        _step(param, opt, g)
        ref.grad = g.clone()
        topt.step()
    d32 = ref.detach() - p0
    d8 = opt.flat_param - p0
    rel = ((d8 - d32).norm() / d32.norm()).item()
    print(f"seed {seed} bf16_grads={bf16_grads}: relative deviation {rel:.4f}")
    assert rel < 0.10


# ------------------------------------------------------- 4. state_dict
def _snapshot(opt):
    return {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v))
            for k, v in opt.state_dict().items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _run(n, steps, seed, dtype=torch.float32, **kw):
    p0, grad = _grad_problem(n, seed)
    param, opt = _opt(p0, dtype, **kw)
    for _ in range(steps):
        _step(param, opt, grad())
    return param, opt, grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_state_dict_8_to_8_bit_exact(dtype):
    n = 3 * 256 + 5
    pa, oa, grad = _run(n, 3, seed=5, dtype=dtype, state_bits=8)
    sd = oa.state_dict()
    want = {"step", "lr", "flat_param", "exp_avg_q", "exp_avg_absmax",
            "exp_avg_sq_q", "exp_avg_sq_absmax", "format"}
    if dtype == torch.bfloat16:
        want.add("master")
    assert set(sd) == want
    assert sd["format"] == {"state_bits": 8, "qblock": 256,
                            "codec": "e4m3fn_absmax", "second_moment": "sqrt"}
    sd = _snapshot(oa)
    pb, ob = _opt(torch.zeros(n), dtype, state_bits=8)
    ob.load_state_dict(sd)
    _same(_snapshot(ob), sd)
    g = grad()
    _step(pa, oa, g)
    _step(pb, ob, g)
    _same(_snapshot(oa), _snapshot(ob))


def test_state_dict_32_to_8_quantises():
    n = 3 * 256 + 5
    _, o32, _ = _run(n, 3, seed=6)
    sd = _snapshot(o32)
    _, o8 = _opt(torch.zeros(n), state_bits=8)
    o8.load_state_dict(sd)
    q, a = quantize_blockwise(sd["exp_avg"])
    assert torch.equal(o8.exp_avg_q, q) and torch.equal(o8.exp_avg_absmax, a)
    q, a = quantize_blockwise(sd["exp_avg_sq"].double().sqrt().float())
    assert torch.equal(o8.exp_avg_sq_q, q) and torch.equal(o8.exp_avg_sq_absmax, a)
    assert o8.step_count == 3 and torch.equal(o8.flat_param, sd["flat_param"])


def test_state_dict_8_to_32_dequantises():
    n = 3 * 256 + 5
    _, o8, _ = _run(n, 3, seed=7, state_bits=8)
    sd = _snapshot(o8)
    _, o32 = _opt(torch.zeros(n))
    o32.load_state_dict(sd)
    m = dequantize_blockwise(sd["exp_avg_q"], sd["exp_avg_absmax"], n)
    r = dequantize_blockwise(sd["exp_avg_sq_q"], sd["exp_avg_sq_absmax"], n)
    assert torch.equal(o32.exp_avg, m) and torch.equal(o32.exp_avg_sq, r * r)
    assert o32.step_count == 3 and torch.equal(o32.flat_param, sd["flat_param"])


@pytest.mark.parametrize("case,bits", [
    ("numel", 8), ("codec", 8), ("qblock", 8), ("numel32", 8),
    ("numel", 32), ("codec", 32), ("qblock", 32)])
def test_bad_checkpoint_raises_and_modifies_nothing(case, bits):
    n = 3 * 256 + 5
    if case == "numel32":                   # fp32-state checkpoint, wrong size
        _, src, _ = _run(n + 256, 2, seed=8)
    else:
        _, src, _ = _run(n + 256 if case == "numel" else n, 2, seed=8,
                         state_bits=8)
    sd = _snapshot(src)
    if case == "codec":
        sd["format"]["codec"] = "e5m2_absmax"
    if case == "qblock":
        sd["format"]["qblock"] = 128
    _, dst, _ = _run(n, 1, seed=9, state_bits=bits)
    before = _snapshot(dst)
    with pytest.raises(ValueError):
        dst.load_state_dict(sd)
    _same(_snapshot(dst), before)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_32bit_state_dict_keys_unchanged(dtype):
    _, opt, _ = _run(300, 1, seed=10, dtype=dtype)
    want = {"step", "lr", "exp_avg", "exp_avg_sq", "flat_param"}
    if dtype == torch.bfloat16:
        want.add("master")
    sd = opt.state_dict()
    assert set(sd) == want
    assert sd["exp_avg"] is opt.exp_avg and sd["exp_avg_sq"] is opt.exp_avg_sq
    assert opt.state_bits == 32


# ------------------------------------------------ 5. memory and guards
def test_state_nbytes_and_no_fp32_moment_arenas():
    n = 1000 * 256 + 37
    nb = _nblocks(n)
    _, o8 = _opt(torch.zeros(n), torch.bfloat16, state_bits=8)
    assert o8.state_nbytes() == 2 * nb * 256 + 8 * nb
    big32 = [k for k, v in vars(o8).items() if torch.is_tensor(v)
             and v.dtype == torch.float32 and v.numel() >= n]
    assert big32 == ["master"]
    assert o8.exp_avg is None and o8.exp_avg_sq is None

    _, o8f = _opt(torch.zeros(n), state_bits=8)
    big32 = {k for k, v in vars(o8f).items() if torch.is_tensor(v)
             and v.dtype == torch.float32 and v.numel() >= n}
    assert big32 == {"flat_param", "flat_grad"}   # the fp32 model itself

    _, o32 = _opt(torch.zeros(n))
    assert o32.state_nbytes() == 8 * n


def test_constructor_guards():
    p = torch.nn.Parameter(torch.zeros(10))
    with pytest.raises(ValueError):
        FusedAdamW([p], device_state=True, state_bits=8)
    with pytest.raises(ValueError):
        FusedAdamW([p], state_bits=16)


# --------------------------------------------------- 6. trainer and CLI
def tiny_cfg(tmp_path, **kw):
    base = dict(model_size="tiny", synthetic_data=True, synthetic_size=8,
                resolution=64, train_batch_size=2, mixed_precision="no",
                dataloader_num_workers=0, max_train_steps=4, seed=0,
                learning_rate=1e-4, lr_warmup_steps=1,
                output_dir=str(tmp_path / "out"))
    base.update(kw)
    return TrainConfig(**base)


def test_trainer_8bit_loss_decreases(tmp_path):
    tr = Trainer(tiny_cfg(tmp_path, use_8bit_adam=True),
                 device=torch.device("cpu"))
    assert tr.optimizer.state_bits == 8
    batch = next(iter(tr.dataloader))
    losses = [tr.train_step(batch).item() for _ in range(8)]
    assert all(math.isfinite(l) for l in losses)
    assert losses[-1] < losses[0], losses
    assert tr.optimizer.exp_avg_absmax.max() > 0


def test_trainer_8bit_resume_bit_faithful(tmp_path):
    """4 straight steps == 2 steps -> checkpoint -> resume -> 2 steps."""
    dev = torch.device("cpu")
    tr_a = Trainer(tiny_cfg(tmp_path, seed=11, use_8bit_adam=True), device=dev)
    batch = next(iter(tr_a.dataloader))
    for _ in range(4):
        tr_a.train_step(batch)

    tr_b = Trainer(tiny_cfg(tmp_path, seed=11, use_8bit_adam=True), device=dev)
    b2 = next(iter(tr_b.dataloader))
    assert torch.equal(batch["pixel_values"], b2["pixel_values"])
    for _ in range(2):
        tr_b.train_step(b2)
    tr_b.save_checkpoint(tmp_path / "ck")

    tr_c = Trainer(tiny_cfg(tmp_path, seed=99, use_8bit_adam=True), device=dev)
    tr_c.load_checkpoint(tmp_path / "ck")
    assert tr_c.global_step == 2
    for _ in range(2):
        tr_c.train_step(b2)
    assert torch.allclose(tr_a.optimizer.flat_param, tr_c.optimizer.flat_param,
                          atol=1e-6), \
        (tr_a.optimizer.flat_param - tr_c.optimizer.flat_param).abs().max()
    assert torch.equal(tr_a.optimizer.exp_avg_q, tr_c.optimizer.exp_avg_q)


def test_trainer_resume_across_state_formats(tmp_path):
    """state.pt of an fp32-state run resumes with the flag and back."""
    dev = torch.device("cpu")
    tr32 = Trainer(tiny_cfg(tmp_path, seed=3), device=dev)
    batch = next(iter(tr32.dataloader))
    for _ in range(2):
        tr32.train_step(batch)
    tr32.save_checkpoint(tmp_path / "ck32")
    tr8 = Trainer(tiny_cfg(tmp_path, seed=3, use_8bit_adam=True), device=dev)
    tr8.load_checkpoint(tmp_path / "ck32")
    assert tr8.global_step == 2 and tr8.optimizer.step_count == 2
    assert torch.isfinite(tr8.train_step(batch))
    tr8.save_checkpoint(tmp_path / "ck8")
    tr32b = Trainer(tiny_cfg(tmp_path, seed=3), device=dev)
    tr32b.load_checkpoint(tmp_path / "ck8")
    assert tr32b.global_step == 3
    assert torch.isfinite(tr32b.train_step(batch))


def _diff_train():
    spec = importlib.util.spec_from_file_location(
        "_diff_train_cli", str(ROOT / "diff_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flag_sets_config(monkeypatch):
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    cli = _diff_train()
    cfg = cli.config_from_args(cli.parse_args(
        ["--synthetic_data", "--use_8bit_adam"]))
    assert cfg.use_8bit_adam is True
    cfg = cli.config_from_args(cli.parse_args(["--synthetic_data"]))
    assert cfg.use_8bit_adam is False
    assert TrainConfig().use_8bit_adam is False


def test_validate_rejects_device_state_combo(monkeypatch, tmp_path):
    monkeypatch.setenv("DCR_DEV_ADAMW", "1")
    with pytest.raises(ValueError):
        validate(tiny_cfg(tmp_path, use_8bit_adam=True))
    validate(tiny_cfg(tmp_path))            # the flag off: still accepted
    monkeypatch.delenv("DCR_DEV_ADAMW")
    validate(tiny_cfg(tmp_path, use_8bit_adam=True))


def test_output_dir_mangling_ignores_flag(tmp_path):
    from dcr_amd.train import mangle_output_dir
    assert mangle_output_dir(tiny_cfg(tmp_path, use_8bit_adam=True)) == \
        mangle_output_dir(tiny_cfg(tmp_path))
