"""MI355X-native denoising engine for Transformer Latent Diffusion (drop-in for the reference's
``Denoiser`` / ``DiffusionGenerator`` / ``DiffusionTransformer`` hot path)."""
from .configs import ClipConfig, DenoiserConfig, DenoiserLoad, LTDConfig, VaeConfig, config_100m  # noqa: F401
from .denoiser import Denoiser  # noqa: F401
from .diffusion import ContinuousBatcher, DiffusionGenerator, DiffusionTransformer, RequestBatcher, SamplerSession, latent_mask  # noqa: F401
from .sharded import generate_latents_from_sharded, generate_latents_requests_sharded  # noqa: F401
from .vae import AutoencoderKLDecoder, VaeDecoderConfig  # noqa: F401
from .vae_encoder import AutoencoderKL, AutoencoderKLEncoder, DiagonalGaussianDistribution, VaeEncoderConfig, encode_image  # noqa: F401
from .clip_text import ClipTextConfig, ClipTextEncoder  # noqa: F401
from .clip_tokenizer import ClipTokenizer  # noqa: F401
from .clip_image import Clip, ClipImageEncoder, ClipVisionConfig, clip_preprocess, clip_score, clip_visual_from_transformers  # noqa: F401
from . import opt_groups  # noqa: F401
from . import metrics  # noqa: F401
from .metrics import FeatureBank, FeatureMoments, cmmd, frechet_distance, mmd2  # noqa: F401
from .train import EvalLoss, TrainConfig, Trainer, eval_plan  # noqa: F401
from .data import DeviceLatentDataset, dequantize_latents, quantize_latents  # noqa: F401
from .weights import flatten_state_dict, param_layout, unflatten  # noqa: F401

__all__ = ["ClipConfig", "DenoiserConfig", "DenoiserLoad", "LTDConfig", "VaeConfig", "config_100m", "Denoiser",
           "DiffusionGenerator", "DiffusionTransformer", "RequestBatcher", "ContinuousBatcher", "SamplerSession", "AutoencoderKLDecoder", "VaeDecoderConfig",
           "AutoencoderKL", "AutoencoderKLEncoder", "DiagonalGaussianDistribution", "VaeEncoderConfig", "encode_image", "ClipTextConfig", "ClipTextEncoder", "ClipTokenizer", "Clip", "ClipImageEncoder", "ClipVisionConfig", "clip_preprocess", "clip_score", "clip_visual_from_transformers", "TrainConfig", "Trainer", "EvalLoss", "eval_plan",
           "flatten_state_dict", "param_layout", "unflatten", "latent_mask", "generate_latents_from_sharded", "generate_latents_requests_sharded",
           "DeviceLatentDataset", "quantize_latents", "dequantize_latents", "opt_groups",
           "metrics", "FeatureBank", "FeatureMoments", "cmmd", "frechet_distance", "mmd2"]
