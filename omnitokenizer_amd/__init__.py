"""omnitokenizer_amd -- MI355X-native (gfx950 HIP) encode/decode path of OmniTokenizer.

    from omnitokenizer_amd import OmniTokenizer_VQGAN     # drop-in for the reference class
    from omnitokenizer_amd.gpt import GPT, sample_with_past, sample_with_past_cfg   # LM consumer
    from omnitokenizer_amd import fp8_dequantized         # what GPT.set_decode_quant("fp8") steps with, as a state dict
    from omnitokenizer_amd import fp8_quantize_rows       # the row rule of both fp8 switches (GPT.set_decode_quant, GPT.set_cache_quant)
    from omnitokenizer_amd import psnr_ssim, calculate_psnr, calculate_ssim          # reconstruction metrics
    from omnitokenizer_amd import InceptionI3d, get_fvd_logits, frechet_distance      # FVD (omnitokenizer_amd.fvd)
    from omnitokenizer_amd import InceptionV3, load_fid_inception, compute_fid       # FID (omnitokenizer_amd.fid)
    from omnitokenizer_amd import LPIPS, load_lpips, lpips_frames                    # LPIPS (omnitokenizer_amd.lpips)
    from omnitokenizer_amd import reconstruction_losses                              # validation losses (omnitokenizer_amd.losses)
    from omnitokenizer_amd import token_cross_entropy                                # LM validation (omnitokenizer_amd.lm_losses)
    from omnitokenizer_amd import resize_frames, images_to_pixels, center_crop_arr   # Pillow-exact resize (omnitokenizer_amd.frames)
    from omnitokenizer_amd import DiT, DiT_models, load_dit                           # DiT denoiser (omnitokenizer_amd.dit)
    from omnitokenizer_amd import create_diffusion, generate_images                  # its sampler (omnitokenizer_amd.diffusion)
    from omnitokenizer_amd import create_ddim_diffusion, DDIMDiffusion, ddim_timesteps   # ... and the DDIM sampler
    from omnitokenizer_amd import Latte, Latte_models, load_latte, generate_videos   # Latte video denoiser (omnitokenizer_amd.latte)
"""
from .config import OmniTokConfig, make_args  # noqa: F401

# omnitokenizer_amd.fid's drop-ins (its Frechet distance is calculate_frechet_distance, on statistics; fvd's is
# frechet_distance, on embeddings)
_FID_NAMES = ("load_fid_inception", "calculate_activation_statistics", "calculate_frechet_distance",
              "compute_statistics_of_path", "calculate_fid_given_paths", "save_fid_stats", "compute_fid")

__all__ = ["OmniTokenizer_VQGAN", "GPT", "OmniTokConfig", "make_args", "psnr_ssim", "calculate_psnr", "calculate_ssim",
           "InceptionI3d", "load_fvd_model", "get_fvd_logits", "frechet_distance", "compute_fvd",
           "InceptionV3"] + list(_FID_NAMES) + ["LPIPS", "load_lpips", "lpips_frames", "reconstruction_losses",
                                           "token_cross_entropy", "resize_frames", "images_to_pixels", "center_crop_arr",
                                           "DiT", "DiT_models", "load_dit", "create_diffusion", "generate_images",
                                           "create_ddim_diffusion", "DDIMDiffusion", "ddim_timesteps",
                                           "Latte", "Latte_models", "load_latte", "get_1d_sincos_temp_embed", "generate_videos",
                                           "fp8_dequantized", "fp8_quantize_rows"]


def __getattr__(name):
    if name == "OmniTokenizer_VQGAN":
        from .vqgan import OmniTokenizer_VQGAN
        return OmniTokenizer_VQGAN
    if name == "GPT":
        from .gpt import GPT
        return GPT
    if name in ("fp8_dequantized", "fp8_quantize_rows"):
        from . import gpt
        return getattr(gpt, name)
    if name in ("psnr_ssim", "calculate_psnr", "calculate_ssim"):
        from . import metrics
        return getattr(metrics, name)
    if name == "InceptionI3d":
        from .i3d import InceptionI3d
        return InceptionI3d
    if name in ("load_fvd_model", "get_fvd_logits", "frechet_distance", "compute_fvd"):
        from . import fvd
        return getattr(fvd, name)
    if name == "InceptionV3":
        from .inception import InceptionV3
        return InceptionV3
    if name in _FID_NAMES:
        from . import fid
        return getattr(fid, name)
    if name in ("LPIPS", "load_lpips", "lpips_frames"):
        from . import lpips
        return getattr(lpips, name)
    if name == "reconstruction_losses":
        from . import losses
        return losses.reconstruction_losses
    if name == "token_cross_entropy":
        from . import lm_losses
        return lm_losses.token_cross_entropy
    if name in ("resize_frames", "images_to_pixels", "center_crop_arr"):
        from . import frames
        return getattr(frames, name)
    if name in ("DiT", "DiT_models", "load_dit"):
        from . import dit
        return getattr(dit, name)
    if name in ("Latte", "Latte_models", "load_latte", "get_1d_sincos_temp_embed"):
        from . import latte
        return getattr(latte, name)
    if name in ("create_diffusion", "generate_images", "generate_videos", "create_ddim_diffusion", "DDIMDiffusion", "ddim_timesteps"):
        from . import diffusion
        return getattr(diffusion, name)
    raise AttributeError(name)
