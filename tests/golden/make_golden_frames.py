"""Generates tests/golden/frames_*.npz: the reference's OWN uint8 -> fp32 input conversions on seeded uint8 clips, for
omnitokenizer_amd.frames (csrc/frames.hip).  Runs the UNMODIFIED reference (imported read-only through
oracle/ref_harness.py) in the build container only:

    python tests/golden/make_golden_frames.py

  frames_pre_*  OmniTokenizer/data.py:305-350 `preprocess(video, resolution, sequence_length, sample_every_n_frames)`
                (u / 255, bilinear resize of the short side, center crop, - 0.5), on the CPU in fp32
  frames_vn_*   the decord dataset path, data.py:228-232: the crop of VideoRandomSquareCrop (offsets drawn by the reference's
                own random.randint under a seed), then video_utils.py VideoNorm (/255 only if the clip's max is above 1, - 0.5)

Each fixture stores the uint8 input `u8` [F,H,W,3], the reference's output `ref` [3,F_out,R,R] and the parameters
(resolution, sequence_length (-1: none), sample_every_n_frames, crop_top, crop_left).  The stubs below replace
packages the two modules import but whose code the two functions never run (data loaders, tokenizers, codecs).
"""
import os
import random
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

# name, (F, H, W), resolution, sequence_length, sample_every_n_frames
PRE_CASES = [
    ("frames_pre_wide_down", (5, 72, 128), 64, None, 1),      # h < w, downscale (72x128 -> 64x114)
    ("frames_pre_tall_up", (2, 96, 80), 128, None, 1),        # h > w, upscale (96x80 -> 154x128)
    ("frames_pre_square_up", (2, 48, 48), 64, None, 1),       # square, upscale
    ("frames_pre_same", (2, 64, 128), 64, None, 1),           # resize size == source size: exact copy, then the crop
    ("frames_pre_odd", (1, 300, 301), 128, None, 1),          # odd sizes, downscale
    ("frames_pre_seq", (9, 40, 72), 32, 7, 2),               # sequence_length + sample_every_n_frames: frames 0 2 4 6
    ("frames_pre_image", (1, 72, 128), 64, None, 1),         # an image: a clip of one frame
]
# name, (F, H, W), crop size, byte range (high exclusive)
VN_CASES = [
    ("frames_vn_video", (5, 72, 128), 64, 256),
    ("frames_vn_binary", (5, 40, 48), 32, 2),                 # every byte 0 or 1: VideoNorm does not divide by 255
    ("frames_vn_image", (1, 64, 96), 64, 256),
]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference_frames():
    """(preprocess, VideoNorm, VideoRandomSquareCrop) of the unmodified reference."""
    rh.install_stubs()
    for name in ("h5py", "decord", "ftfy", "imagenet_stubs", "timm.data", "torchvision.datasets"):
        _stub(name)
    sys.modules["decord"].VideoReader = object
    sys.modules["decord"].cpu = lambda *a: None
    sys.modules["decord"].bridge = types.SimpleNamespace(set_bridge=lambda *a: None)
    _stub("transformers", BertTokenizer=object)
    _stub("imagenet_stubs.imagenet_2012_labels", label_to_name=lambda i: str(i))
    _stub("timm.data.transforms", _pil_interp=lambda m: m)
    _stub("torchvision.datasets.video_utils", VideoClips=object)
    tvt = sys.modules["torchvision.transforms"]
    tvt.functional = _stub("torchvision.transforms.functional", pad=None, resize=None)
    tv = sys.modules["torchvision"]
    tv.datasets = sys.modules["torchvision.datasets"]
    tv.io = _stub("torchvision.io", read_video=None)
    sys.modules["pytorch_lightning"].LightningDataModule = object
    import importlib
    vu = importlib.import_module("OmniTokenizer.video_utils")
    data = importlib.import_module("OmniTokenizer.data")
    return data.preprocess, vu.VideoNorm, vu.VideoRandomSquareCrop


def main():
    preprocess, VideoNorm, VideoRandomSquareCrop = load_reference_frames()
    torch.set_num_threads(1)
    total = 0
    for i, (name, shape, res, seq, every) in enumerate(PRE_CASES):
        u8 = np.random.default_rng(100 + i).integers(0, 256, size=shape + (3,), dtype=np.uint8)
        ref = preprocess(torch.from_numpy(u8), res, sequence_length=seq, sample_every_n_frames=every)["video"]
        total += _save(name, u8, ref, res, -1 if seq is None else seq, every, -1, -1)
    for i, (name, shape, res, hi) in enumerate(VN_CASES):
        u8 = np.random.default_rng(200 + i).integers(0, hi, size=shape + (3,), dtype=np.uint8)
        random.seed(300 + i)
        cropper = VideoRandomSquareCrop(res)
        # the offsets the cropper draws (its own random.randint calls, replayed from the same seed)
        state = random.getstate()
        top, left = random.randint(0, shape[1] - res), random.randint(0, shape[2] - res)
        random.setstate(state)
        frames = cropper(u8)
        assert np.array_equal(frames, u8[:, top:top + res, left:left + res])
        # data.py:228-232
        vid = torch.from_numpy(np.ascontiguousarray(frames)).float().permute(0, 3, 1, 2)
        ref = VideoNorm()(vid).permute(1, 0, 2, 3).contiguous()
        total += _save(name, u8, ref, res, -1, 1, top, left)
    print(f"total {total / 1e6:.2f} MB")


def _save(name, u8, ref, res, seq, every, top, left):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, u8=u8, ref=ref.numpy().astype(np.float32), resolution=res, sequence_length=seq,
                        sample_every_n_frames=every, crop_top=top, crop_left=left)
    size = os.path.getsize(path)
    print(f"{name}: u8 {u8.shape} -> ref {tuple(ref.shape)}, {size / 1e3:.0f} kB")
    return size


if __name__ == "__main__":
    main()
