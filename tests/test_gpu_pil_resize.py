"""GPU: the Pillow-exact resize (csrc/resize_pil.hip; frames.resize_frames / images_to_pixels / center_crop_arr and
OmniTokenizer_VQGAN.encode_images) against Pillow's own bytes (tests/golden/pilresize_*.npz, written by
make_golden_pil_resize.py) and the numpy restatement of the algorithm (tests/pil_resize_oracle.py).  Every comparison is
equality: there is no tolerance anywhere."""
import glob
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import frames as fr
from tests import pil_resize_oracle as oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "pilresize_*.npz")))
RESIZE = [n for n in FIXTURES if "_cca_" not in n]
CCA = [n for n in FIXTURES if "_cca_" in n]
IMAGEDATASET = ["pilresize_down_bicubic", "pilresize_tiles_bicubic", "pilresize_crop_bicubic"]


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _resize_fixture(g, out="uint8", stream=None):
    """resize_frames on one fixture as its parameters say -> [F_out or nothing, h, w, 3] (uint8) on the CPU"""
    size, interp = tuple(int(v) for v in g["size"]), str(g["interpolation"])
    u8 = torch.from_numpy(g["u8"]).cuda()
    kw = {}
    if "crop" in g:
        kw.update(crop=[tuple(int(v) for v in g["crop"])], crop_size=int(g["crop_size"]))
    if str(g["kind"]) == "video":
        c0, w = int(g["col0"]), int(g["width"])
        clip = u8[:, :, c0:c0 + w]               # a view: row stride 3 * 80 > 3 * W, rows start at odd byte offsets
        assert not clip.is_contiguous()
        return fr.resize_frames([clip], size, interpolation=interp, frame_start=int(g["frame_start"]),
                                sample_every_n_frames=int(g["sample_every_n_frames"]), out=out)[0]
    return fr.resize_frames([u8], size, True, interpolation=interp, out=out, **kw)[0]


def test_fixture_list_is_complete():
    assert len(RESIZE) == 28 and len(CCA) == 2 and set(IMAGEDATASET) <= set(RESIZE)


@pytest.mark.parametrize("name", RESIZE)
def test_resize_frames_equals_pillow(name):
    g = _load(name)
    got = _resize_fixture(g)
    want = torch.from_numpy(g["out"])
    assert got.dtype == torch.uint8 and got.shape == want.shape
    got = got.cpu()
    assert torch.equal(got, want), f"{name}: {(got != want).sum().item()} of {want.numel()} bytes differ"


@pytest.mark.parametrize("name", IMAGEDATASET)
def test_images_to_pixels_equals_imagedataset(name):
    g = _load(name)
    assert str(g["kind"]) == "imagedataset"
    u8 = torch.from_numpy(g["u8"]).cuda()
    if "crop" in g:   # the train-time resizecrop
        x = fr.images_to_pixels([u8], int(g["crop_size"]), resize_to=int(g["size"][0]), crop=[tuple(int(v) for v in g["crop"])])
    else:
        x = fr.images_to_pixels(u8[None], int(g["size"][0]))
    want = torch.from_numpy(g["pixels"])
    assert x.dtype == torch.float32 and x.shape == (1,) + want.shape
    assert torch.equal(x[0].cpu(), want), name


@pytest.mark.parametrize("name", ["pilresize_down_bicubic", "pilresize_tiles_bilinear", "pilresize_halve_50_box",
                                  "pilresize_video_bicubic", "pilresize_crop_bicubic", "pilresize_skip_h_33_bicubic"])
def test_out_pixels_equals_totensor_of_out_uint8(name):
    g = _load(name)
    u8 = _resize_fixture(g, out="uint8")
    px = _resize_fixture(g, out="pixels")
    is_image = u8.dim() == 3
    want = fr.frames_to_pixels(u8[None], is_image, resize="none", norm="totensor")[0]
    assert px.shape == want.shape and torch.equal(px, want), name


SHAPES33 = [(20, 27), (16, 16), (9, 40), (33, 18)]   # a downscale, a copy, mixed up / down, odd sizes: all -> 16 x 16


def test_ragged_batch_of_33_equals_single_calls_and_the_oracle():
    rng = np.random.default_rng(33)
    imgs = [rng.integers(0, 256, SHAPES33[i % 4] + (3,), dtype=np.uint8) for i in range(33)]   # one more than a launch carries
    dev = [torch.from_numpy(a).cuda() for a in imgs]
    got = fr.resize_frames(dev, (16, 16), True)
    assert got.shape == (33, 16, 16, 3)
    for i in range(33):
        assert torch.equal(got[i:i + 1], fr.resize_frames([dev[i]], (16, 16), True)), i
        assert np.array_equal(got[i].cpu().numpy(), oracle.resize(imgs[i], (16, 16), "bicubic")), i


# The horizontal pass takes a row in chunks of at most 256 output pixels (fewer where the source segment of 256 would not
# fit the staged span: the host narrows the chunk, to a multiple of 4 or to 1..3), re-staging LDS for each; the vertical
# pass walks a row 256 pixels at a time.  No Pillow fixture is that wide, so these compare with the numpy restatement:
# (H, W) -> (h, w), interpolation, crop (top, left) and crop_size (h, w) or None
WIDE = [
    ("two_chunks", (20, 700), (12, 301), "bicubic", None, None),        # 256 + 45 pixels: a ragged last lane group
    ("skipped_horizontal", (20, 301), (12, 301), "bicubic", None, None),  # the copy, two chunks
    ("skipped_vertical", (12, 700), (12, 301), "bilinear", None, None),
    ("upscale_three_chunks", (5, 100), (4, 600), "bilinear", None, None),
    ("crop_of_two_chunks", (20, 700), (12, 301), "box", (1, 3), (9, 290)),  # chunks start at column 3 of the resized row
    ("chunk_16", (5, 6000), (4, 40), "bicubic", None, None),            # 601 taps: chunks of 16, 16, 8 output pixels
    ("chunk_3", (5, 6000), (4, 12), "bicubic", None, None),             # 2001 taps: chunks of 3 (byte stores, one lane)
    ("chunk_1", (3, 9000), (3, 5), "box", None, None),                  # 1801 taps: chunks of 1
]


@pytest.mark.parametrize("name,hw,size,interp,crop,crop_size", WIDE, ids=[w[0] for w in WIDE])
def test_rows_of_several_chunks_equal_the_oracle(name, hw, size, interp, crop, crop_size):
    u8 = np.random.default_rng(len(name) + hw[1]).integers(0, 256, hw + (3,), dtype=np.uint8)
    want = oracle.resize(u8, size, interp)
    kw = {}
    if crop is not None:
        want = np.ascontiguousarray(want[crop[0]:crop[0] + crop_size[0], crop[1]:crop[1] + crop_size[1]])
        kw.update(crop=[crop], crop_size=crop_size)
    dev = torch.from_numpy(u8).cuda()
    got = fr.resize_frames([dev], size, True, interpolation=interp, **kw)
    assert got.shape == (1,) + want.shape
    got = got[0].cpu()
    assert torch.equal(got, torch.from_numpy(want)), f"{name}: {(got.numpy() != want).sum()} of {want.size} bytes differ"
    px = fr.resize_frames([dev], size, True, interpolation=interp, out="pixels", **kw)
    assert torch.equal(px, fr.frames_to_pixels(got[None].cuda(), True, resize="none", norm="totensor")), name


def test_clips_of_different_chunk_widths_in_one_launch():
    rng = np.random.default_rng(77)   # chunks of 256 + 45 and of 168 + 133 output pixels in the same group
    imgs = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in [(20, 700), (5, 6000)]]
    got = fr.resize_frames([torch.from_numpy(a).cuda() for a in imgs], (4, 301), True).cpu().numpy()
    for i, a in enumerate(imgs):
        assert np.array_equal(got[i], oracle.resize(a, (4, 301), "bicubic")), i


def test_two_fixtures_batched_equal_the_single_calls():
    a, b = _load("pilresize_down_bicubic"), _load("pilresize_up_7x5_16_bicubic")
    ua, ub = torch.from_numpy(a["u8"]).cuda(), torch.from_numpy(b["u8"]).cuda()
    for out in ("uint8", "pixels"):
        both = fr.resize_frames([ua, ub], (16, 16), True, out=out)
        assert torch.equal(both[0:1], fr.resize_frames([ua], (16, 16), True, out=out))
        assert torch.equal(both[1:2], fr.resize_frames([ub], (16, 16), True, out=out))
    both = fr.resize_frames([ua, ub], (16, 16), True).cpu()
    assert torch.equal(both[0], torch.from_numpy(a["out"])) and torch.equal(both[1], torch.from_numpy(b["out"]))


def test_non_default_stream_equals_default_stream():
    g = _load("pilresize_tiles_bicubic")
    u8 = torch.from_numpy(g["u8"]).cuda()
    want = fr.resize_frames([u8], (96, 96), True, out="pixels")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = fr.resize_frames([u8], (96, 96), True, out="pixels")
    s.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", CCA)
def test_center_crop_arr_equals_the_loaders(name):
    g = _load(name)
    got = fr.center_crop_arr([torch.from_numpy(g["u8"]).cuda()], int(g["image_size"]))
    want = torch.from_numpy(g["out"])
    assert got.dtype == torch.uint8 and got.shape == (1,) + want.shape
    assert torch.equal(got[0].cpu(), want), name


def test_center_crop_arr_batches_images_of_different_sizes():
    gs = [_load(n) for n in CCA]
    got = fr.center_crop_arr([torch.from_numpy(g["u8"]).cuda() for g in gs], 32).cpu()
    for i, g in enumerate(gs):
        assert torch.equal(got[i], torch.from_numpy(g["out"])), i


def test_encode_images_equals_encode_of_images_to_pixels():
    from tests.test_gpu_frames import _model
    m = _model(64)
    rng = np.random.default_rng(5)
    imgs = [torch.from_numpy(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).cuda() for hw in [(90, 70), (64, 64), (150, 97)]]
    ids = m.encode_images(imgs)
    x = fr.images_to_pixels(imgs, 64)
    assert x.shape == (3, 3, 64, 64)
    assert torch.equal(ids, m.encode(x, True))
    emb, ids2 = m.encode_images(imgs, include_embeddings=True)
    assert torch.equal(ids2, ids) and emb.shape[0] == 3
    with pytest.raises(RuntimeError, match="model on"):
        m.encode_images([i.cpu() for i in imgs])


def test_fake_implementation_matches_real_outputs():
    clips = [torch.randint(0, 256, (3, 20, 27, 3), dtype=torch.uint8, device="cuda"),
             torch.randint(0, 256, (4, 33, 18, 3), dtype=torch.uint8, device="cuda")]
    geom = [0, 1, 0, 0, 16, 16, 1, 1, 0, 0, 16, 16]
    for kind in (0, 1):
        torch.library.opcheck(torch.ops.omnitok.frames_resize_pil.default, (clips, geom, 2, 16, 16, 0, kind),
                              test_utils=("test_schema", "test_faketensor"))
