"""--model_size sd14 plumbing: CLI choices, the size-name -> configs helper,
and the CPU fallback of ops.attention at an SD-1.x head dim."""
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent


def test_diff_train_accepts_sd14():
    sys.path.insert(0, str(ROOT))
    try:
        import diff_train
    finally:
        sys.path.pop(0)
    args = diff_train.parse_args(["--model_size", "sd14", "--synthetic_data"])
    cfg = diff_train.config_from_args(args)
    assert cfg.model_size == "sd14"
    assert (cfg.prediction_type or "epsilon") == "epsilon"
    with pytest.raises(SystemExit):
        diff_train.parse_args(["--model_size", "sd15x"])


def test_diff_inference_help_lists_sd14():
    r = subprocess.run([sys.executable, str(ROOT / "diff_inference.py"), "--help"],
                       capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stdout.replace("\n", " ").split("--") if
            l.startswith("model_size")]
    assert line and "sd14" in line[0] and "sd21" in line[0] and "tiny" in line[0]


def test_model_configs_sd14():
    from dcr_amd.models import (CLIPTextConfig, UNetConfig, VAEConfig,
                                model_configs)
    u, v, t = model_configs("sd14")
    assert u.attention_head_dim == (8, 8, 8, 8)
    assert u.cross_attention_dim == 768
    assert u.use_linear_projection is False
    assert u == UNetConfig.sd14()
    assert t == CLIPTextConfig.sd14() and t.hidden_size == 768
    assert v == VAEConfig.sd()
    # head dims of the family: channels / heads per level
    assert [c // h for c, h in zip(u.block_out_channels, u.attention_head_dim)] \
        == [40, 80, 160, 160]


def test_model_configs_existing_names_unchanged():
    from dcr_amd.models import (CLIPTextConfig, MODEL_SIZES, UNetConfig,
                                VAEConfig, model_configs)
    assert model_configs("sd21") == (UNetConfig.sd21(), VAEConfig.sd(),
                                     CLIPTextConfig.sd21())
    assert model_configs("tiny") == (UNetConfig.tiny(), VAEConfig.tiny(),
                                     CLIPTextConfig.tiny())
    assert set(MODEL_SIZES) == {"sd21", "sd14", "tiny"}
    with pytest.raises(ValueError):
        model_configs("sd3")


def test_trainer_unet_config_overrides_sd14(tmp_path, monkeypatch):
    """--unet_from_scratch yes --unet_config keeps overriding the UNet
    config; VAE / text encoder still come from the size name."""
    from dcr_amd.models import UNetConfig
    from dcr_amd.train import TrainConfig, Trainer
    p = tmp_path / "unet_config.json"
    p.write_text(UNetConfig.tiny().to_json())
    calls = []
    import dcr_amd.train.trainer as trainer_mod
    real = trainer_mod.model_configs

    def tiny_but_recorded(size):
        calls.append(size)
        return real("tiny")     # keep the CPU test small: only the name is checked

    monkeypatch.setattr(trainer_mod, "model_configs", tiny_but_recorded)
    cfg = TrainConfig(model_size="sd14", unet_from_scratch="yes",
                      unet_config=str(p), synthetic_data=True,
                      synthetic_size=4, resolution=64, train_batch_size=2,
                      mixed_precision="no", dataloader_num_workers=0,
                      max_train_steps=1, seed=0,
                      output_dir=str(tmp_path / "out"))
    tr = Trainer(cfg, device=torch.device("cpu"))
    assert calls == ["sd14"]
    assert tr.unet.config == UNetConfig.tiny()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("layout", ["blhd", "bhld"])
def test_cpu_attention_d40_with_grad_matches_sdpa(dtype, layout):
    from dcr_amd import ops
    torch.manual_seed(0)
    Bn, Hn, Lq, Lk, D = 2, 3, 20, 13, 40
    shape = (lambda L: (Bn, L, Hn, D)) if layout == "blhd" \
        else (lambda L: (Bn, Hn, L, D))
    q, k, v = (torch.randn(shape(L), dtype=dtype, requires_grad=True)
               for L in (Lq, Lk, Lk))
    out = ops.attention(q, k, v, layout=layout)
    g = torch.randn_like(out)
    out.backward(g)

    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    tr = (lambda t: t.permute(0, 2, 1, 3)) if layout == "blhd" else (lambda t: t)
    ref = tr(F.scaled_dot_product_attention(tr(q2), tr(k2), tr(v2),
                                            scale=1.0 / D ** 0.5))
    ref.backward(g)
    assert torch.equal(out, ref)
    for a, b in zip((q, k, v), (q2, k2, v2)):
        assert torch.equal(a.grad, b.grad)
