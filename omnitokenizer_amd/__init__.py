"""omnitokenizer_amd -- MI355X-native (gfx950 HIP) encode/decode path of OmniTokenizer.

    from omnitokenizer_amd import OmniTokenizer_VQGAN     # drop-in for the reference class
    from omnitokenizer_amd.gpt import GPT, sample_with_past, sample_with_past_cfg   # LM consumer
    from omnitokenizer_amd import psnr_ssim, calculate_psnr, calculate_ssim          # reconstruction metrics
"""
from .config import OmniTokConfig, make_args  # noqa: F401

__all__ = ["OmniTokenizer_VQGAN", "GPT", "OmniTokConfig", "make_args", "psnr_ssim", "calculate_psnr", "calculate_ssim"]


def __getattr__(name):
    if name == "OmniTokenizer_VQGAN":
        from .vqgan import OmniTokenizer_VQGAN
        return OmniTokenizer_VQGAN
    if name == "GPT":
        from .gpt import GPT
        return GPT
    if name in ("psnr_ssim", "calculate_psnr", "calculate_ssim"):
        from . import metrics
        return getattr(metrics, name)
    raise AttributeError(name)
