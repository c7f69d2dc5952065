"""FID on the device: drop-ins for the reference's evaluation/pytorch-fid (fid_score.py), which vqgan_eval.py's image branch
runs on its folders of input and reconstruction PNGs.

    model = load_fid_inception("cuda", "pt_inception-2015-12-05-6726825d.pth")   # the weight file is the caller's
    act = get_activations(images, model)            # paths (read with PIL), numpy / CUDA uint8 [N, H, W, 3] (e.g.
                                                    #   decode_frames(ids, True): no host round trip) or fp32 [N, 3, H, W]
    fid = compute_fid(real_u8, fake_u8, model)      # or calculate_fid_given_paths([dir_a, dir_b], 50, "cuda", 2048, model=...)

The preprocess (u8 / 255, bilinear resize to 299, 2 x - 1), the network and the spatial mean of dims < 2048 run in
csrc/inception.hip (omnitokenizer_amd/inception.py); the activations come back once, as the reference's fp64 [N, dims]
array.  The statistics (np.mean, np.cov) and the Frechet distance (scipy.linalg.sqrtm, with the eps offset fallback and the
imaginary-part check) are 2048 x 2048 work in fp64 on the CPU, as in the reference.
"""
from __future__ import annotations

import os
import pathlib
from typing import Optional

import numpy as np
import torch

from .inception import BLOCK_INDEX_BY_DIM, InceptionV3, preprocess_images, spatial_mean

IMAGE_EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp", "JPEG"}


def load_fid_inception(device, path: str, dims: int = 2048) -> InceptionV3:
    """InceptionV3([BLOCK_INDEX_BY_DIM[dims]]) with the FID weights read from `path` (the .pth file, or a state_dict of
    the wrapper); nothing is downloaded"""
    if dims not in BLOCK_INDEX_BY_DIM:
        raise ValueError(f"dims {dims}: one of {sorted(BLOCK_INDEX_BY_DIM)}")
    model = InceptionV3([BLOCK_INDEX_BY_DIM[dims]])
    model.load_state_dict(torch.load(path, map_location="cpu"))
    return model.to(device).eval()


def _device(device, model: InceptionV3) -> torch.device:
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda":
        raise RuntimeError(f"FID runs on the GPU: device {device} (there is no CPU path)")
    return device


def _read_images(files) -> np.ndarray:
    from PIL import Image
    arrs = [np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8) for f in files]
    if len({a.shape for a in arrs}) != 1:
        raise ValueError("get_activations: the images of one batch must share a size (as the reference's DataLoader needs)")
    return np.stack(arrs)


def _as_tensor(images, device: torch.device) -> torch.Tensor:
    """numpy / tensor uint8 [N, H, W, 3] or fp32 [N, 3, H, W] -> a tensor on `device` (no copy if it is there already)"""
    if isinstance(images, np.ndarray):
        images = torch.from_numpy(np.ascontiguousarray(images))
    if not isinstance(images, torch.Tensor):
        raise TypeError(f"images must be a list of paths, a numpy array or a tensor, got {type(images).__name__}")
    if images.dtype == torch.uint8:
        if images.dim() != 4 or images.shape[3] != 3:
            raise ValueError(f"uint8 images must be [N, H, W, 3], got {tuple(images.shape)}")
    elif images.dtype == torch.float32:
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"float32 images must be [N, 3, H, W] in [0, 1], got {tuple(images.shape)}")
    else:
        raise TypeError(f"images: dtype {images.dtype}, expected uint8 [N, H, W, 3] or float32 [N, 3, H, W]")
    return images.to(device, non_blocking=True)


def _batch_features(model: InceptionV3, batch: torch.Tensor) -> torch.Tensor:
    """[n, dims] fp32 on the device: the model's first output block, spatially averaged unless it is 1 x 1 already"""
    if not model.resize_input:
        H, W = (batch.shape[1], batch.shape[2]) if batch.dtype == torch.uint8 else (batch.shape[2], batch.shape[3])
        from .inception import check_input_size
        check_input_size(H, W, model.last_needed_block)
    if batch.dtype == torch.uint8 and (batch.stride(3) != 1 or batch.stride(2) != 3 or
                                       batch.stride(0) != batch.shape[1] * batch.stride(1)):
        batch = batch.contiguous()
    x = preprocess_images(batch, model.resize_input, model.normalize_input)
    f = model.forward_channels_last(x)[0]            # channels-last [n, h, w, C]
    return f.reshape(f.shape[0], -1) if f.shape[1] == f.shape[2] == 1 else spatial_mean(f)


def get_activations(images, model: InceptionV3, batch_size: int = 50, dims: int = 2048, device=None,
                    num_workers: int = 1) -> np.ndarray:
    """fid_score.get_activations: the fp64 [N, dims] activations of `model`'s first output block.  `images` is a list of
    image files (read with PIL, .convert("RGB"), as the reference does), a uint8 [N, H, W, 3] array or tensor (CUDA
    tensors stay on the device) or fp32 [N, 3, H, W] in [0, 1].  num_workers is accepted for the reference's signature."""
    if dims not in BLOCK_INDEX_BY_DIM:
        raise ValueError(f"dims {dims}: one of {sorted(BLOCK_INDEX_BY_DIM)}")
    if model.output_blocks[0] != BLOCK_INDEX_BY_DIM[dims]:
        raise ValueError(f"dims {dims} is block {BLOCK_INDEX_BY_DIM[dims]}; the model's first output block is "
                         f"{model.output_blocks[0]}")
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size}")
    dev = _device(device, model)
    is_files = isinstance(images, (list, tuple))
    n = len(images) if is_files else int(images.shape[0])
    batch_size = min(batch_size, max(n, 1))
    tensor = None if is_files else _as_tensor(images, dev)
    out = torch.empty((n, dims), device=dev, dtype=torch.float32)
    with torch.no_grad(), torch.cuda.device(dev):
        for i in range(0, n, batch_size):
            if is_files:
                batch = torch.from_numpy(_read_images(images[i:i + batch_size])).to(dev)
            else:
                batch = tensor[i:i + batch_size]
            out[i:i + batch.shape[0]] = _batch_features(model, batch)
    return out.cpu().numpy().astype(np.float64)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """fid_score.calculate_frechet_distance: ||mu1 - mu2||^2 + tr(S1) + tr(S2) - 2 tr(sqrtm(S1 S2)) in fp64 on the CPU
    (scipy.linalg.sqrtm; where the product's square root is not finite, eps is added to both diagonals; an imaginary
    part above 1e-3 on the diagonal is an error)"""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape:
        raise ValueError(f"mean vectors of different lengths: {mu1.shape} vs {mu2.shape}")
    if sigma1.shape != sigma2.shape:
        raise ValueError(f"covariances of different shapes: {sigma1.shape} vs {sigma2.shape}")
    d = mu1 - mu2
    root, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(root).all():
        print(f"FID: the square root of the covariance product is not finite; adding {eps} to both diagonals")
        off = np.eye(sigma1.shape[0]) * eps
        root = linalg.sqrtm((sigma1 + off).dot(sigma2 + off))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(root.imag))}")
        root = root.real
    return float(d.dot(d) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(root))


def calculate_activation_statistics(images, model: InceptionV3, batch_size: int = 50, dims: int = 2048, device=None,
                                    num_workers: int = 1):
    """fid_score.calculate_activation_statistics: (mu, sigma) = np.mean and np.cov(rowvar=False) of the activations"""
    act = get_activations(images, model, batch_size, dims, device, num_workers)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def _image_files(path) -> list:
    path = pathlib.Path(path)
    files = sorted(f for ext in IMAGE_EXTENSIONS for f in path.glob(f"*/*.{ext}"))
    if not files:
        files = sorted(f for ext in IMAGE_EXTENSIONS for f in path.glob(f"*.{ext}"))
    if not files:
        raise ValueError(f"no images under {path}")
    return files


def compute_statistics_of_path(path, model: InceptionV3, batch_size: int = 50, dims: int = 2048, device=None,
                               num_workers: int = 1):
    """fid_score.compute_statistics_of_path: (mu, sigma) of a .npz with mu and sigma, or of the images of a folder
    (those one level down if there are any, else those in it; sorted by path)"""
    path = str(path)
    if path.endswith(".npz"):
        with np.load(path) as f:
            return f["mu"][:], f["sigma"][:]
    return calculate_activation_statistics(_image_files(path), model, batch_size, dims, device, num_workers)


def _model_for(dims: int, model, weights, device, paths) -> Optional[InceptionV3]:
    if model is not None or all(str(p).endswith(".npz") for p in paths):
        return model
    if weights is None:
        raise ValueError("pass model= (an InceptionV3) or weights= (the path of the FID Inception weights): nothing is "
                         "downloaded")
    return load_fid_inception(device, weights, dims)


def calculate_fid_given_paths(paths, batch_size: int, device, dims: int, num_workers: int = 1, *, model=None,
                              weights=None) -> float:
    """fid_score.calculate_fid_given_paths: the FID of two folders or .npz files.  The reference downloads its weights;
    here the caller passes the model, or the weight file's path"""
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError(f"Invalid path: {p}")
    model = _model_for(dims, model, weights, device, paths)
    m1, s1 = compute_statistics_of_path(paths[0], model, batch_size, dims, device, num_workers)
    m2, s2 = compute_statistics_of_path(paths[1], model, batch_size, dims, device, num_workers)
    return calculate_frechet_distance(m1, s1, m2, s2)


def save_fid_stats(paths, batch_size: int, device, dims: int, num_workers: int = 1, *, model=None, weights=None):
    """fid_score.save_fid_stats: the statistics of the folder paths[0] into the new .npz paths[1] (mu, sigma)"""
    if not os.path.exists(paths[0]):
        raise RuntimeError(f"Invalid path: {paths[0]}")
    if os.path.exists(paths[1]):
        raise RuntimeError(f"Existing output file: {paths[1]}")
    model = _model_for(dims, model, weights, device, paths[:1])
    m1, s1 = compute_statistics_of_path(paths[0], model, batch_size, dims, device, num_workers)
    np.savez_compressed(paths[1], mu=m1, sigma=s1)


def compute_fid(real, fake, model: InceptionV3, dims: int = 2048, batch_size: int = 50, device=None) -> float:
    """FID of two image sets (uint8 [N, H, W, 3] numpy or CUDA, fp32 [N, 3, H, W] in [0, 1], or lists of files)"""
    m1, s1 = calculate_activation_statistics(real, model, batch_size, dims, device)
    m2, s2 = calculate_activation_statistics(fake, model, batch_size, dims, device)
    return calculate_frechet_distance(m1, s1, m2, s2)
