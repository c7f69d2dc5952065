"""omnitokenizer_amd -- MI355X-native (gfx950 HIP) encode/decode path of OmniTokenizer.

    from omnitokenizer_amd import OmniTokenizer_VQGAN     # drop-in for the reference class
    from omnitokenizer_amd.gpt import GPT, sample_with_past, sample_with_past_cfg   # LM consumer
    from omnitokenizer_amd import psnr_ssim, calculate_psnr, calculate_ssim          # reconstruction metrics
    from omnitokenizer_amd import InceptionI3d, get_fvd_logits, frechet_distance      # FVD (omnitokenizer_amd.fvd)
"""
from .config import OmniTokConfig, make_args  # noqa: F401

__all__ = ["OmniTokenizer_VQGAN", "GPT", "OmniTokConfig", "make_args", "psnr_ssim", "calculate_psnr", "calculate_ssim",
           "InceptionI3d", "load_fvd_model", "get_fvd_logits", "frechet_distance", "compute_fvd"]


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
    if name == "InceptionI3d":
        from .i3d import InceptionI3d
        return InceptionI3d
    if name in ("load_fvd_model", "get_fvd_logits", "frechet_distance", "compute_fvd"):
        from . import fvd
        return getattr(fvd, name)
    raise AttributeError(name)
