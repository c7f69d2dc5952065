"""FVD on the device: a drop-in for the reference's OmniTokenizer/fvd/fvd.py (what vqgan_eval.py:103, 141-164 calls).

    i3d = load_fvd_model(device, "i3d_pretrained_400.pt")   # the weight file is the caller's: nothing ships with the package
    real = get_fvd_logits(frames_real, i3d, device)          # uint8 [B, T, H, W, 3]: numpy (the reference's input) or a CUDA
    fake = get_fvd_logits(frames_fake, i3d, device)          #   tensor, e.g. decode_frames(..., layout="thwc"); no host trip
    fvd = frechet_distance(real, fake)                       # fp64 on the CPU, the reference's formula

preprocess (bilinear resize to 224 x 224 and 2 v / 255 - 1) and the network run in csrc/i3d.hip (omnitokenizer_amd/i3d.py).
frechet_distance is 400 x 400 work and stays in torch: fp64 on the CPU, unbiased cov, the svd square root with the eps = 1e-10
cutoff and trace_sqrt_product, as in the reference.
"""
from __future__ import annotations

import numpy as np
import torch

from .i3d import InceptionI3d, check_input_size, preprocess_frames

MAX_BATCH = 16
TARGET_RESOLUTION = (224, 224)


def _frames_tensor(videos, device) -> torch.Tensor:
    """numpy / torch uint8 [B, T, H, W, 3] -> the same frames as a uint8 tensor on `device` (a CUDA device)"""
    if isinstance(videos, np.ndarray):
        if videos.dtype != np.uint8:
            raise TypeError(f"videos: dtype {videos.dtype}, expected np.uint8 in {{0, ..., 255}}")
        videos = torch.from_numpy(np.ascontiguousarray(videos))
    elif not isinstance(videos, torch.Tensor):
        raise TypeError(f"videos must be a numpy array or a tensor, got {type(videos).__name__}")
    if videos.dtype != torch.uint8:
        raise TypeError(f"videos: dtype {videos.dtype}, expected uint8 in {{0, ..., 255}}")
    if videos.dim() != 5 or videos.shape[4] != 3:
        raise ValueError(f"videos must be [B, T, H, W, 3], got shape {tuple(videos.shape)}")
    check_input_size(videos.shape[1], *TARGET_RESOLUTION)
    device = torch.device(device) if device is not None else (videos.device if videos.is_cuda else None)
    if device is None or device.type != "cuda":
        raise RuntimeError(f"FVD runs on the GPU: device {device} (there is no CPU path)")
    return videos.to(device, non_blocking=True).contiguous()


def preprocess(videos, target_resolution=TARGET_RESOLUTION, device=None) -> torch.Tensor:
    """fvd.py preprocess: uint8 [B, T, H, W, 3] -> fp32 [B, 3, T, *target_resolution] in [-1, 1] on the GPU"""
    x = preprocess_frames(_frames_tensor(videos, device), tuple(target_resolution))
    return x[..., :3].permute(0, 4, 1, 2, 3).contiguous()


def get_logits(i3d: InceptionI3d, videos: torch.Tensor, device=None) -> torch.Tensor:
    """fvd.py get_logits: i3d over [B, 3, T, H, W] fp32 videos, MAX_BATCH clips at a time"""
    if device is not None:
        videos = videos.to(device)
    with torch.no_grad():
        return torch.cat([i3d(videos[i:i + MAX_BATCH]) for i in range(0, videos.shape[0], MAX_BATCH)])


def get_fvd_logits(videos, i3d: InceptionI3d, device=None) -> torch.Tensor:
    """fvd.py get_fvd_logits: uint8 [B, T, H, W, 3] (numpy or tensor) -> I3D logits [B, 400] on the GPU.  The frames are
    resized straight into the channels-last layout the network reads."""
    x = preprocess_frames(_frames_tensor(videos, device), TARGET_RESOLUTION)
    with torch.no_grad():
        return i3d.forward_channels_last(x)


def load_fvd_model(device, path: str) -> InceptionI3d:
    """fvd.py load_fvd_model, with the weight file's path as an argument (the reference reads i3d_pretrained_400.pt next to
    its module)"""
    i3d = InceptionI3d(400, in_channels=3)
    i3d.load_state_dict(torch.load(path, map_location="cpu"))
    return i3d.to(device).eval()


# https://github.com/tensorflow/gan/blob/de4b8da3853058ea380a6152bd3bd454013bf619/tensorflow_gan/python/eval/classifier_metrics.py
def _symmetric_matrix_square_root(mat, eps=1e-10):
    u, s, v = torch.svd(mat)
    si = torch.where(s < eps, s, torch.sqrt(s))
    return torch.matmul(torch.matmul(u, torch.diag(si)), v.t())


def trace_sqrt_product(sigma, sigma_v):
    sqrt_sigma = _symmetric_matrix_square_root(sigma)
    sqrt_a_sigmav_a = torch.matmul(sqrt_sigma, torch.matmul(sigma_v, sqrt_sigma))
    return torch.trace(_symmetric_matrix_square_root(sqrt_a_sigmav_a))


def cov(m, rowvar=False):
    """the unbiased covariance of fvd.py cov"""
    if m.dim() > 2:
        raise ValueError("m has more than 2 dimensions")
    if m.dim() < 2:
        m = m.view(1, -1)
    if not rowvar and m.size(0) != 1:
        m = m.t()
    fact = 1.0 / (m.size(1) - 1)
    m_center = m - torch.mean(m, dim=1, keepdim=True)
    return fact * m_center.matmul(m_center.t()).squeeze()


def frechet_distance(x1, x2) -> torch.Tensor:
    """fvd.py frechet_distance in fp64 on the CPU: x1 [N1, ...], x2 [N2, ...] embeddings (any device, any float dtype)
    -> a 0-d float64 tensor"""
    x1 = torch.as_tensor(x1).detach().to("cpu", torch.float64).flatten(start_dim=1)
    x2 = torch.as_tensor(x2).detach().to("cpu", torch.float64).flatten(start_dim=1)
    m, m_w = x1.mean(dim=0), x2.mean(dim=0)
    sigma, sigma_w = cov(x1, rowvar=False), cov(x2, rowvar=False)
    sqrt_trace_component = trace_sqrt_product(sigma, sigma_w)
    trace = torch.trace(sigma + sigma_w) - 2.0 * sqrt_trace_component
    mean = torch.sum((m - m_w) ** 2)
    return trace + mean


def compute_fvd(real, samples, i3d: InceptionI3d, device=None) -> torch.Tensor:
    """fvd.py compute_fvd: real, samples uint8 [N, T, H, W, 3] -> FVD (fp64, CPU)"""
    return frechet_distance(get_fvd_logits(real, i3d, device), get_fvd_logits(samples, i3d, device))
