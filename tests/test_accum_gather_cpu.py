"""Gradient accumulation hands every micro-step's gradient to the flat arena
(Trainer.train_step with sync_gradients=False gathers after backward)."""
import torch

from dcr_amd.train import TrainConfig, Trainer


def tiny_cfg(tmp_path, name, **kw):
    base = dict(model_size="tiny", synthetic_data=True, synthetic_size=8,
                resolution=64, train_batch_size=2, mixed_precision="no",
                dataloader_num_workers=0, max_train_steps=4, seed=0,
                learning_rate=1e-4, lr_warmup_steps=1,
                gradient_accumulation_steps=2,
                output_dir=str(tmp_path / name))
    base.update(kw)
    return TrainConfig(**base)


def test_non_sync_micro_step_leaves_no_grad_behind(tmp_path):
    tr = Trainer(tiny_cfg(tmp_path, "a"), device=torch.device("cpu"))
    opt = tr.optimizer
    b = next(iter(tr.dataloader))
    p0 = opt.flat_param.clone()
    tr.train_step(b, sync_gradients=False)
    assert all(p.grad is None for p in opt.params)
    assert len(opt._gathered) == len(opt.params)
    assert opt.flat_grad.any()
    assert torch.equal(opt.flat_param, p0)
    # the explicit call of the older idiom finds nothing left to move
    g1 = opt.flat_grad.clone()
    opt.gather_grads()
    assert torch.equal(opt.flat_grad, g1)
    # a second micro-step adds into the arena and again leaves no p.grad
    tr.train_step(b, sync_gradients=False)
    assert all(p.grad is None for p in opt.params)
    assert not torch.equal(opt.flat_grad, g1)


def test_accumulation_same_bits_as_explicit_gather(tmp_path):
    """Micro-step, then sync step, against the same two backward passes
    with an explicit gather_grads() in between: same arena, same parameters,
    bit for bit."""
    tr_a = Trainer(tiny_cfg(tmp_path, "a"), device=torch.device("cpu"))
    tr_b = Trainer(tiny_cfg(tmp_path, "b"), device=torch.device("cpu"))
    tr_b.optimizer.flat_param.copy_(tr_a.optimizer.flat_param)
    b = next(iter(tr_a.dataloader))
    p0 = tr_a.optimizer.flat_param.clone()

    torch.manual_seed(7)
    tr_a.train_step(b, sync_gradients=False)
    # the micro-step itself has moved its gradient into the arena
    g_half_a = tr_a.optimizer.flat_grad.clone()
    assert all(p.grad is None for p in tr_a.optimizer.params)
    torch.manual_seed(8)
    tr_a.train_step(b, sync_gradients=True)

    torch.manual_seed(7)
    tr_b.train_step(b, sync_gradients=False)
    tr_b.optimizer.gather_grads()
    g_half = tr_b.optimizer.flat_grad.clone()
    torch.manual_seed(8)
    tr_b.train_step(b, sync_gradients=True)

    assert g_half.any()
    assert torch.equal(g_half_a, g_half)
    assert not torch.equal(tr_a.optimizer.flat_param, p0)
    assert torch.equal(tr_a.optimizer.flat_grad, tr_b.optimizer.flat_grad)
    assert not torch.equal(tr_a.optimizer.flat_grad, g_half)
    assert torch.equal(tr_a.optimizer.flat_param, tr_b.optimizer.flat_param)
    assert torch.equal(tr_a.optimizer.exp_avg, tr_b.optimizer.exp_avg)
    assert tr_a.global_step == tr_b.global_step == 1
