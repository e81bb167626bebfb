"""CPU side of the native gradient tail: clip_and_step falls back to
clip_grad_norm_ + step, and every arena writer clears the validity flag
of the fused sum of squares through FusedAdamW.arena_written()."""
import pytest
import torch

from dcr_amd.ops import FusedAdamW, dispatch_counts
from dcr_amd.parallel.ddp import GradBucketAllReduce

NEW_COUNTERS = ("grad_gather", "grad_sumsq", "grad_norm_finalize",
                "adamw_clip", "grad_gather_fallback")


def _make(dtype=torch.float32, seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dtype))
          for s in [(5, 3), (17,), (2, 3, 1, 1)]]
    return FusedAdamW(ps, lr=1e-2, **kw), ps


def _grads(ps, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=g).to(p.dtype) * 3 for p in ps]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("state_bits", [32, 8])
@pytest.mark.parametrize("max_norm", [1.0, 1e6])
def test_clip_and_step_is_clip_then_step_on_cpu(dtype, state_bits, max_norm):
    ref, rps = _make(dtype, state_bits=state_bits)
    new, nps = _make(dtype, state_bits=state_bits)
    before = {k: dispatch_counts[k] for k in NEW_COUNTERS}
    for step in range(2):
        for ps in (rps, nps):
            for p, g in zip(ps, _grads(ps, 10 + step)):
                p.grad = g
        rn = ref.clip_grad_norm_(max_norm)
        ref.step(lr=2e-2)
        nn_ = new.clip_and_step(max_norm, lr=2e-2)
        assert torch.equal(rn, nn_)
        assert torch.equal(ref.flat_grad, new.flat_grad)
        assert torch.equal(ref.flat_param, new.flat_param)
        ref.zero_grad()
        new.zero_grad()
    assert new.lr == 2e-2 and new.step_count == 2
    if state_bits == 32:
        assert torch.equal(ref.exp_avg, new.exp_avg)
        assert torch.equal(ref.exp_avg_sq, new.exp_avg_sq)
    else:
        assert torch.equal(ref.exp_avg_q, new.exp_avg_q)
    # no native op ran, and the flag never claims a sum that was not taken
    assert {k: dispatch_counts[k] for k in NEW_COUNTERS} == before
    assert not new._sumsq_valid


def test_switch_is_read_per_call(monkeypatch):
    from dcr_amd.ops.adamw import fused_grad_tail_enabled
    monkeypatch.delenv("DCR_FUSED_GRAD_TAIL", raising=False)
    assert fused_grad_tail_enabled()
    monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", "0")
    assert not fused_grad_tail_enabled()
    monkeypatch.setenv("DCR_FUSED_GRAD_TAIL", "1")
    assert fused_grad_tail_enabled()
    opt, _ = _make()
    assert opt._native_tail() is None      # CPU arena: never native


def _armed(opt):
    """Pretend a full fused gather just ran."""
    opt._sumsq_valid = True
    return opt


def test_every_arena_writer_clears_the_flag():
    opt, ps = _make()
    gs = _grads(ps, 1)

    # copy-mode and add-mode gathers
    for p, g in zip(ps, gs):
        p.grad = g
    _armed(opt).gather_grads()
    assert not opt._sumsq_valid
    for p, g in zip(ps, gs):
        p.grad = g
    _armed(opt).gather_grads()                      # second gather: adds
    assert not opt._sumsq_valid
    assert torch.equal(opt.flat_grad, 2 * torch.cat([g.reshape(-1) for g in gs]))
    # a gather with nothing to move writes nothing
    _armed(opt).gather_grads()
    assert opt._sumsq_valid

    # the clip's mul_, only when it clips
    _armed(opt).clip_grad_norm_(1e9)
    assert opt._sumsq_valid
    _armed(opt).clip_grad_norm_(1e-3)
    assert not opt._sumsq_valid

    # zero_grad, then a partial cycle whose cold slices get zeroed
    _armed(opt).zero_grad()
    assert not opt._sumsq_valid
    ps[0].grad = gs[0]
    opt.gather_grads()
    _armed(opt)._ensure_cold_slices()
    assert not opt._sumsq_valid
    assert not opt.flat_grad[ps[0].numel():].any()
    # nothing stale left: no write
    _armed(opt)._ensure_cold_slices()
    assert opt._sumsq_valid


def test_bucket_allreduce_sites_clear_the_flag(monkeypatch):
    """_launch (the all-reduce rewrites the slice) and finalize's div_, with
    a stand-in for the collective: a world of 2 without a process group."""
    import torch.distributed as dist
    from dcr_amd.parallel.ddp import _Bucket

    class _Work:
        def wait(self):
            pass

    opt, ps = _make()
    ddp = GradBucketAllReduce(opt)
    calls = []
    orig = opt.arena_written
    monkeypatch.setattr(opt, "arena_written",
                        lambda: (calls.append(1), orig())[1])
    monkeypatch.setattr(dist, "all_reduce", lambda *a, **k: _Work())
    monkeypatch.setattr(ddp, "_enabled", True)
    monkeypatch.setattr(ddp, "world", 2)
    b = _Bucket(0, opt.numel, list(ps))
    ddp.buckets.append(b)

    _armed(opt)
    ddp._launch(b)                    # nothing to gather: still invalidates
    assert not opt._sumsq_valid and calls

    opt.flat_grad.fill_(4.0)
    _armed(opt)
    ddp.finalize()                    # waits for b.work, then div_(world)
    assert not opt._sumsq_valid
    assert torch.equal(opt.flat_grad, torch.full_like(opt.flat_grad, 2.0))
