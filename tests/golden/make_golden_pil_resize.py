#!/usr/bin/env python
"""Writes tests/golden/pilresize_*.npz with the installed Pillow: the fixtures of tests/test_pil_resize_cpu.py and
tests/test_gpu_pil_resize.py (omnitokenizer_amd.frames.resize_frames / images_to_pixels / center_crop_arr on
csrc/resize_pil.hip).  Neither Pillow nor the reference is needed where the fixtures are read.

    python tests/golden/make_golden_pil_resize.py

Every file holds
    u8        uint8 input, [H, W, 3] (or [F, H, Wfull, 3] for the video case, of which columns col0 .. col0 + W are the clip)
    size      (h, w) Pillow is asked for, interpolation (a string), pil_version
    out       Pillow's bytes: Image.fromarray(frame).resize((w, h), filter) of every selected frame, then the crop window
              where crop / crop_size are stored; for kind == "center_crop_arr" the result of the DiT / Latte loaders'
              center_crop_arr(image, image_size) (Diffusion/DiT/train.py:92-110: BOX halvings, BICUBIC, center crop)
and the ImageDataset cases (data.py:83-99, kind == "imagedataset") also
    pixels    fp32 [3, h, w] = np.float32(out) / np.float32(255) - np.float32(0.5): torch's ToTensor + Normalize(0.5, 1.0)
              arithmetic (one IEEE fp32 division, one subtraction), which is what frames_to_pixels' resize="none" /
              norm="totensor" mode is pinned to.
Content is uniform noise unless the case says otherwise.
"""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "box": Image.BOX}
ALL = ("bicubic", "bilinear", "box")

# name: (H, W), (h, w), filters, content
CASES = {
    "down": ((37, 53), (16, 16), ALL, "noise"),
    "extremes": ((37, 53), (16, 16), ALL, "extremes"),
    "up_16_24": ((16, 16), (24, 24), ALL, "noise"),
    "up_7x5_16": ((7, 5), (16, 16), ALL, "noise"),
    "skip_v": ((64, 48), (64, 32), ALL, "noise"),
    "skip_v_33": ((33, 33), (33, 20), ("bicubic",), "noise"),
    "skip_h_33": ((33, 33), (20, 33), ("bicubic",), "noise"),
    "one_row": ((1, 9), (4, 4), ALL, "noise"),
    "taps501_v": ((1000, 31), (8, 8), ("bicubic",), "noise"),
    "taps501_h": ((31, 1000), (8, 8), ("bicubic",), "noise"),
    "tiles": ((129, 257), (96, 96), ("bicubic", "bilinear"), "noise"),
    "halve_48": ((48, 48), (24, 24), ("box",), "noise"),
    "halve_50": ((50, 50), (25, 25), ("box",), "noise"),
}
IMAGEDATASET = {("down", "bicubic"), ("tiles", "bicubic")}   # Resize((R, R), bicubic) + ToTensor + Normalize(0.5, 1.0)


def content(rng, shape, kind):
    if kind == "extremes":
        return (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def pil_resize(u8, size, interpolation):
    return np.asarray(Image.fromarray(u8).resize((size[1], size[0]), FILTERS[interpolation]))


def center_crop_arr(u8, image_size):
    """uint8 [H, W, 3] -> [image_size, image_size, 3]: the chain of frames.center_crop_arr with pil_resize() as every resize
    step (the same loop as tests/pil_resize_oracle.center_crop_arr, which has the numpy restatement in Pillow's place)"""
    while min(u8.shape[0], u8.shape[1]) >= 2 * image_size:
        u8 = pil_resize(u8, (u8.shape[0] // 2, u8.shape[1] // 2), "box")
    scale = image_size / min(u8.shape[0], u8.shape[1])
    u8 = pil_resize(u8, (round(u8.shape[0] * scale), round(u8.shape[1] * scale)), "bicubic")
    top, left = (u8.shape[0] - image_size) // 2, (u8.shape[1] - image_size) // 2
    return np.ascontiguousarray(u8[top:top + image_size, left:left + image_size])


def to_pixels(out):
    return np.ascontiguousarray((out.astype(np.float32) / np.float32(255) - np.float32(0.5)).transpose(2, 0, 1))


def fixtures():
    """name -> dict of arrays; deterministic (one generator per case, seeded by the case's position)"""
    fx = {}
    for i, (case, (hw, size, filters, kind)) in enumerate(CASES.items()):
        u8 = content(np.random.default_rng(1000 + i), hw + (3,), kind)
        for f in filters:
            d = dict(u8=u8, size=np.array(size), interpolation=f, kind="resize", out=pil_resize(u8, size, f))
            if (case, f) in IMAGEDATASET:
                d.update(kind="imagedataset", pixels=to_pixels(d["out"]))
            fx[f"pilresize_{case}_{f}"] = d
    # 3 output frames of a 40 x 72 clip -> 32 x 32: source frames 1, 3, 5 of a column-cropped view (row stride > 3 * W)
    rng = np.random.default_rng(2000)
    base = content(rng, (6, 40, 80, 3), "noise")
    col0, W, start, step = 5, 72, 1, 2
    out = np.stack([pil_resize(np.ascontiguousarray(base[t, :, col0:col0 + W]), (32, 32), "bicubic")
                    for t in range(start, 6, step)])
    fx["pilresize_video_bicubic"] = dict(u8=base, col0=np.array(col0), width=np.array(W), frame_start=np.array(start),
                                         sample_every_n_frames=np.array(step), size=np.array((32, 32)),
                                         interpolation="bicubic", kind="video", out=out)
    # train-time resizecrop: Resize((96, 96)) of a 70 x 90 image, RandomCrop(64) at the drawn offsets (5, 17)
    u8 = content(np.random.default_rng(2001), (70, 90, 3), "noise")
    full = pil_resize(u8, (96, 96), "bicubic")
    out = np.ascontiguousarray(full[5:5 + 64, 17:17 + 64])
    fx["pilresize_crop_bicubic"] = dict(u8=u8, size=np.array((96, 96)), crop=np.array((5, 17)), crop_size=np.array(64),
                                        interpolation="bicubic", kind="imagedataset", out=out, pixels=to_pixels(out))
    for j, hw in enumerate([(150, 97), (64, 64)]):
        u8 = content(np.random.default_rng(2010 + j), hw + (3,), "noise")
        fx[f"pilresize_cca_{hw[0]}x{hw[1]}"] = dict(u8=u8, image_size=np.array(32), kind="center_crop_arr",
                                                    out=center_crop_arr(u8, 32))
    return fx


def main():
    for name, d in fixtures().items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, pil_version=PIL.__version__, **d)
        print(f"{name}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
