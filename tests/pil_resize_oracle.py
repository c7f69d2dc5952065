"""Numpy restatement of Pillow's 8-bit resampler, Image.resize(size, filter) on an RGB image (whole-image box,
reducing_gap=None; src/libImaging/Resample.c), for the bicubic, bilinear and box filters.  It is what csrc/resize_pil.hip
computes and what the tests compare with where Pillow itself is not installed; Pillow is never imported here.

Everything is IEEE double arithmetic, one rounding per operation (numpy scalars do not fuse), in Pillow's order:

    scale = in / out;  fs = max(scale, 1);  support = S * fs;  ksize = int(ceil(support)) * 2 + 1
    center = (xx + 0.5) * scale;  ss = 1 / fs
    xmin = max(int(center - support + 0.5), 0);  xmax = min(int(center + support + 0.5), in) - xmin
    w[x] = filter((x + xmin - center + 0.5) * ss);  w /= sum(w) (summed in index order, if it is not 0)
    k[x] = int(w[x] * 2**22 -+ 0.5)   (truncation; - for w < 0)

One pass: out = clamp((2**21 + sum(u8[xmin + x] * k[x])) >> 22, 0, 255) in int32.  The horizontal pass runs first and
writes uint8, the vertical pass runs over its result, and a pass whose output size equals its input size is skipped.
"""
import math

import numpy as np

BICUBIC, BILINEAR, BOX = 0, 1, 2
FILTERS = {"bicubic": BICUBIC, "bilinear": BILINEAR, "box": BOX}
SUPPORT = {BICUBIC: 2.0, BILINEAR: 1.0, BOX: 0.5}
PRECISION_BITS = 22


def _filter(f, x):
    D = np.float64
    if f == BICUBIC:
        a = D(-0.5)
        x = abs(x)
        if x < 1.0:
            return ((a + D(2.0)) * x - (a + D(3.0))) * x * x + D(1.0)
        if x < 2.0:
            return (((x - D(5.0)) * x + D(8.0)) * x - D(4.0)) * a
        return D(0.0)
    if f == BILINEAR:
        x = abs(x)
        return D(1.0) - x if x < 1.0 else D(0.0)
    return D(1.0) if -0.5 < x <= 0.5 else D(0.0)


def coeffs(in_size, out_size, f):
    """(ksize, k int32 [out, ksize] (zero past a row's taps), bounds int32 [out, 2] = (xmin, number of taps))"""
    D = np.float64
    scale = D(in_size) / D(out_size)
    fs = scale if scale > 1.0 else D(1.0)
    support = D(SUPPORT[f]) * fs
    ksize = int(math.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    ss = D(1.0) / fs
    for xx in range(out_size):
        center = (D(xx) + D(0.5)) * scale
        xmin = max(int(center - support + D(0.5)), 0)      # int(): truncation toward zero
        xmax = min(int(center + support + D(0.5)), in_size) - xmin
        w = [_filter(f, (D(x + xmin) - center + D(0.5)) * ss) for x in range(xmax)]
        ww = D(0.0)
        for v in w:
            ww = ww + v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(D(-0.5) + v * D(4194304.0)) if v < 0 else int(D(0.5) + v * D(4194304.0))
        bounds[xx] = (xmin, xmax)
    return ksize, k, bounds


def _pass(img, out_size, f, axis):
    """one pass along `axis` of a uint8 [..., H, W, 3] array"""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img
    _, k, bounds = coeffs(in_size, out_size, f)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        kk = k[xx, :n].reshape((n,) + (1,) * (src.ndim - 1))
        acc = np.int32(1 << (PRECISION_BITS - 1)) + (src[xmin:xmin + n] * kk).sum(0, dtype=np.int32)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, size, interpolation="bicubic"):
    """uint8 [..., H, W, 3] -> [..., size[0], size[1], 3]: Image.resize((size[1], size[0]), filter) of every frame"""
    f = FILTERS[interpolation] if isinstance(interpolation, str) else interpolation
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    return np.ascontiguousarray(_pass(_pass(img, size[1], f, -2), size[0], f, -3))


def center_crop_arr(img, image_size):
    """the DiT / Latte loaders' center_crop_arr on a uint8 [H, W, 3] array -> [image_size, image_size, 3]"""
    while min(img.shape[0], img.shape[1]) >= 2 * image_size:
        img = resize(img, (img.shape[0] // 2, img.shape[1] // 2), "box")
    scale = image_size / min(img.shape[0], img.shape[1])
    img = resize(img, (round(img.shape[0] * scale), round(img.shape[1] * scale)), "bicubic")
    top, left = (img.shape[0] - image_size) // 2, (img.shape[1] - image_size) // 2
    return np.ascontiguousarray(img[top:top + image_size, left:left + image_size])
