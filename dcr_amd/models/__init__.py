from .unet import UNet2DConditionModel, UNetConfig
from .vae import AutoencoderKL, VAEConfig, DiagonalGaussianDistribution
from .clip_text import CLIPTextModel, CLIPTextConfig
from .presets import MODEL_SIZES, model_configs

__all__ = [
    "UNet2DConditionModel", "UNetConfig",
    "AutoencoderKL", "VAEConfig", "DiagonalGaussianDistribution",
    "CLIPTextModel", "CLIPTextConfig",
    "MODEL_SIZES", "model_configs",
]
