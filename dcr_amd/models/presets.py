"""Stock architectures by name: the one place that maps a ``--model_size``
value to the (UNet, VAE, text-encoder) configs built when no checkpoint
directory is given (trainer, diff_inference, sd_mitigation)."""
from __future__ import annotations

from typing import Tuple

from .clip_text import CLIPTextConfig
from .unet import UNetConfig
from .vae import VAEConfig

MODEL_SIZES = ("sd21", "sd14", "tiny")


def model_configs(size: str) -> Tuple[UNetConfig, VAEConfig, CLIPTextConfig]:
    """sd21: stabilityai/stable-diffusion-2-1 (head_dim 64, 1024-d text).
    sd14: CompVis/stable-diffusion-v1-4 and v1-5 (8 heads per level, i.e.
    head dims 40/80/160; 768-d CLIP ViT-L text; same VAE as sd21).
    tiny: same topology at small widths, for CPU tests."""
    if size == "sd21":
        return UNetConfig.sd21(), VAEConfig.sd(), CLIPTextConfig.sd21()
    if size == "sd14":
        return UNetConfig.sd14(), VAEConfig.sd(), CLIPTextConfig.sd14()
    if size == "tiny":
        return UNetConfig.tiny(), VAEConfig.tiny(), CLIPTextConfig.tiny()
    raise ValueError(f"unknown model_size {size!r}; choose from {MODEL_SIZES}")
