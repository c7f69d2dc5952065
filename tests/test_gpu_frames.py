"""GPU (-m gpu): frames in, frames out (csrc/frames.hip, omnitokenizer_amd/frames.py, OmniTokenizer_VQGAN.encode_frames /
decode_frames) against the reference's own conversions (tests/golden/frames_*.npz, make_golden_frames.py) and against
encode() / decode() of the same pixels."""
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import frames as fr
from tests.test_gpu_e2e import assert_ids_match_or_near_tie

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRE = ["frames_pre_wide_down", "frames_pre_tall_up", "frames_pre_square_up", "frames_pre_same", "frames_pre_odd",
       "frames_pre_seq", "frames_pre_image"]
VN = ["frames_vn_video", "frames_vn_binary", "frames_vn_image"]


def _fix(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    seq = int(g["sequence_length"])
    return dict(u8=torch.from_numpy(g["u8"]), ref=torch.from_numpy(g["ref"]), R=int(g["resolution"]),
                seq=None if seq < 0 else seq, every=int(g["sample_every_n_frames"]),
                crop=(int(g["crop_top"]), int(g["crop_left"])))


def _to_frames_ref(x, layout):
    """the reference's conversion (vqgan_eval.py:141-148) on the device, in the requested layout"""
    u = ((x + 0.5).clamp(0, 1) * 255).to(torch.uint8)
    if layout == "thwc":
        u = u.permute(0, 2, 3, 1) if u.dim() == 4 else u.permute(0, 2, 3, 4, 1)
    return u.contiguous()


@pytest.mark.parametrize("name", VN)
def test_mode_none_videonorm_bit_identical(name):
    f = _fix(name)
    x = fr.frames_to_pixels(f["u8"][None].cuda(), resize="none", norm="videonorm", resolution=f["R"], crop=[f["crop"]])
    assert x.shape == (1,) + tuple(f["ref"].shape) and x.dtype == torch.float32
    assert torch.equal(x[0].cpu(), f["ref"]), name


@pytest.mark.parametrize("name", ["frames_vn_image", "frames_vn_binary", "frames_pre_odd"])
def test_mode_none_totensor_on_images(name):
    """ToTensor + Normalize(0.5, 1.0): u / 255 - 0.5 for every byte, bytes 0 / 1 included"""
    u8 = _fix(name)["u8"][0]                  # [H, W, 3]
    imgs = torch.stack([u8, u8.flip(0)])
    x = fr.frames_to_pixels(imgs.cuda(), True, norm="totensor")
    want = imgs.permute(0, 3, 1, 2).float().div(255) - 0.5
    assert x.shape == want.shape and torch.equal(x.cpu(), want)


@pytest.mark.parametrize("name", PRE)
def test_mode_bilinear_vs_preprocess(name):
    f = _fix(name)
    x = fr.frames_to_pixels(f["u8"][None].cuda(), resize="bilinear", resolution=f["R"], sequence_length=f["seq"],
                            sample_every_n_frames=f["every"])[0].cpu()
    assert x.shape == f["ref"].shape
    err = (x - f["ref"]).abs().max().item()
    assert err <= 1e-6, f"{name}: max abs error {err:.2e}"
    H, W = f["u8"].shape[1:3]
    if fr.preprocess_size(H, W, f["R"]) == (H, W):
        assert torch.equal(x, f["ref"]), name


def _ragged_clips():
    clips = [_fix(n)["u8"].cuda() for n in ("frames_pre_wide_down", "frames_pre_tall_up", "frames_vn_video", "frames_pre_seq")]
    # a strided view on the device: a frame subset and a crop whose rows start at odd byte offsets
    clips.append(clips[3][1:, 3:, 5:])
    return clips


@pytest.mark.parametrize("resize", ["none", "bilinear"])
def test_ragged_batch_equals_per_clip_calls(resize):
    clips = _ragged_clips()
    clips = (clips * 8)[:37]    # more clips than one launch carries (32)
    kw = dict(resize=resize, resolution=32, sequence_length=2, sample_every_n_frames=1)
    if resize == "none":
        kw["crop"] = [(i % 5, (3 * i) % 7) for i in range(len(clips))]
    x = fr.frames_to_pixels(clips, **kw)
    assert x.shape == (len(clips), 3, 2, 32, 32)
    for i, c in enumerate(clips):
        kw1 = dict(kw, crop=[kw["crop"][i]]) if "crop" in kw else kw
        assert torch.equal(x[i:i + 1], fr.frames_to_pixels([c], **kw1)), i
    # the frame step and start reach the right source frames
    c = clips[3]
    a = fr.frames_to_pixels([c], resize=resize, resolution=32, frame_start=1, sample_every_n_frames=3, norm="totensor"
                            if resize == "none" else None)
    b = fr.frames_to_pixels([c[1::3].contiguous()], resize=resize, resolution=32, norm="totensor" if resize == "none" else None)
    assert torch.equal(a, b)


# ---- the engine ----------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(res, use_vae=False):
    key = (res, use_vae)
    if key not in _MODELS:
        from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
        from omnitokenizer_amd.config import OmniTokConfig
        args = make_args(2, resolution=res, use_vae=use_vae)
        m = OmniTokenizer_VQGAN(args)
        m.load_state_dict(synth.synth_state_dict(OmniTokConfig.from_args(args), seed=0), strict=True)
        _MODELS[key] = m.cuda().eval()
    return _MODELS[key]


# fixture, model resolution, is_image, resize
ENCODE_CASES = [("frames_vn_video", 64, False, "none"), ("frames_vn_image", 64, True, "none"),
                ("frames_pre_wide_down", 64, False, "bilinear"), ("frames_pre_image", 64, True, "bilinear"),
                ("frames_pre_odd", 128, True, "bilinear")]


@pytest.mark.parametrize("name,res,is_image,resize", ENCODE_CASES)
def test_encode_frames_vs_encode_of_reference_pixels(name, res, is_image, resize):
    f = _fix(name)
    m = _model(res)
    u8 = torch.stack([f["u8"], f["u8"].flip(2)])          # [2, F, H, W, 3]: the clip and its mirror image (mode none)
    if resize == "none":
        R = f["R"]
        crop = [f["crop"], (f["crop"][0], u8.shape[3] - R - f["crop"][1])]
        # ToTensor-style pixels of the crops on the CPU (= VideoNorm for clips with a byte > 1); the first is the fixture
        ref = torch.stack([(u8[i, :, t:t + R, l:l + R].float().div(255) - 0.5).permute(3, 0, 1, 2)
                           for i, (t, l) in enumerate(crop)])
        assert torch.equal(ref[0], f["ref"])
        kw = dict(resize="none", resolution=R, crop=crop)
    else:
        u8 = torch.stack([f["u8"], f["u8"]])
        ref = torch.stack([f["ref"], f["ref"]])
        kw = dict(resize="bilinear", resolution=f["R"])
    u8 = u8.cuda()
    if is_image:
        u8, ref = u8[:, 0], ref[:, :, 0]
    ids, z = m.encode_frames(u8, is_image, return_latents=True, **kw)
    ids_ref, z_ref = m.encode(ref.cuda(), is_image, return_latents=True)
    if resize == "none":
        assert torch.equal(ids, ids_ref) and torch.equal(z, z_ref), name
    else:
        assert (z - z_ref).abs().max().item() < 1e-3
        assert_ids_match_or_near_tie(ids, ids_ref.cpu(), z, m.codebook.embeddings.data.cpu(), name)
    emb, ids2 = m.encode_frames(u8, is_image, include_embeddings=True, **kw)
    assert torch.equal(ids2, ids) and emb.shape[0] == 2


def test_encode_frames_vae_returns_the_latents_of_encode():
    f = _fix("frames_vn_video")
    m = _model(64, use_vae=True)
    u8 = f["u8"][None].cuda()
    kw = dict(resolution=64, crop=[f["crop"]])
    z = m.encode_frames(u8, False, sample_posterior=False, **kw)
    z_ref = m.encode(f["ref"][None].cuda(), False, sample_posterior=False)
    assert torch.equal(z, z_ref)
    torch.manual_seed(7)
    zs = m.encode_frames(u8, False, **kw)
    torch.manual_seed(7)
    assert torch.equal(zs, m.encode(f["ref"][None].cuda(), False))


def test_encode_frames_errors_match_encode():
    m = _model(64)
    u8 = _fix("frames_pre_tall_up")["u8"]     # 2 frames: (2 - 1) % temporal_patch_size != 0
    with pytest.raises(AssertionError):
        m.encode_frames(u8[None].cuda(), False, resize="bilinear")
    with pytest.raises(RuntimeError, match="GPU|model on"):
        m.encode_frames(u8[None], False, resize="bilinear")
    bad = torch.full((1, 2, 8, 8), m.n_codes, dtype=torch.int64, device="cuda")
    with pytest.raises(IndexError):
        m.decode_frames(bad, False)


def _adversarial():
    k = torch.arange(256, dtype=torch.float32)
    edges = k / 255 - 0.5                       # exact k/255 - 0.5 boundaries (as torch rounds them)
    up = torch.nextafter(edges, torch.full_like(edges, 2.0))
    down = torch.nextafter(edges, torch.full_like(edges, -2.0))
    tiny = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 5e-39, -0.5, 0.5, -0.5000001, 0.5000001, -0.50000006,
                         0.50000006, 1e30, -1e30, 3.4e38, -3.4e38, 1.0, -1.0, 7.5, -7.5])
    v = torch.cat([edges, up, down, tiny, torch.rand(4096) * 1.2 - 0.6])
    n = 2 * 3 * 3 * 24 * 20
    v = torch.cat([v, torch.randn(n) * 0.4])[:n]
    return v.reshape(2, 3, 3, 24, 20)


@pytest.mark.parametrize("layout", ["thwc", "cthw"])
def test_pixels_to_frames_adversarial(layout):
    torch.manual_seed(0)
    x = _adversarial().cuda()
    assert torch.equal(fr.pixels_to_frames(x, layout), _to_frames_ref(x, layout))
    img = x[:, :, 0]
    assert torch.equal(fr.pixels_to_frames(img, layout), _to_frames_ref(img, layout))
    odd = x[:, :, :, :23, :19].contiguous()         # H * W % 4 != 0: the scalar path
    assert torch.equal(fr.pixels_to_frames(odd, layout), _to_frames_ref(odd, layout))
    big = (torch.rand(1, 3, 2, 64, 80, device="cuda") * 1.4 - 0.7)   # several full 1024-pixel blocks per plane
    assert torch.equal(fr.pixels_to_frames(big, layout), _to_frames_ref(big, layout))
    nonfinite = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0], device="cuda").repeat(3 * 4).reshape(1, 3, 1, 4, 4)
    u = fr.pixels_to_frames(nonfinite, "cthw")
    assert torch.equal(u[nonfinite.isfinite().logical_not()], torch.zeros_like(u[nonfinite.isfinite().logical_not()]))


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict_fp32"])
@pytest.mark.parametrize("layout", ["thwc", "cthw"])
def test_decode_frames_equals_conversion_of_decode(strict, layout):
    m = _model(64)
    f = _fix("frames_vn_video")
    if strict:
        m.set_option("gemm_mode", 0)
        m.set_option("attn_mode", 0)
    try:
        for is_image, x in ((False, f["ref"][None]), (True, f["ref"][None, :, 0])):
            ids = m.encode(x.cuda(), is_image)
            rec = m.decode(ids, is_image)
            u = m.decode_frames(ids, is_image, layout=layout)
            assert torch.equal(u, _to_frames_ref(rec, layout))
            assert torch.equal(fr.pixels_to_frames(rec, layout), u)
    finally:
        m.set_option("gemm_mode", -1)
        m.set_option("attn_mode", -1)


def test_decode_frames_vae():
    m = _model(64, use_vae=True)
    f = _fix("frames_vn_video")
    z = m.encode(f["ref"][None].cuda(), False, sample_posterior=False)
    zl = z.permute(0, 2, 3, 4, 1)
    assert torch.equal(m.decode_frames(zl, False), _to_frames_ref(m.decode(zl, False), "thwc"))
    zi = m.encode(f["ref"][None, :, 0].cuda(), True, sample_posterior=False)
    assert torch.equal(m.decode_frames(zi, True, layout="cthw"), _to_frames_ref(m.decode(zi, True), "cthw"))


def test_fake_implementations_match_real_outputs():
    clips = [c for c in _ragged_clips()[:3]]
    geom = [0, 1, 0, 0, 0, 0] * 3
    real = torch.ops.omnitok.frames_to_pixels(clips, geom, 2, 32, 32, 0, 0)
    meta = torch.ops.omnitok.frames_to_pixels([torch.empty(c.shape, dtype=torch.uint8, device="meta") for c in clips], geom,
                                              2, 32, 32, 0, 0)
    assert meta.shape == real.shape and meta.dtype == real.dtype == torch.float32
    x = torch.rand(2, 3, 5, 16, 24, device="cuda") - 0.5
    for layout in (0, 1):
        r = torch.ops.omnitok.pixels_to_frames(x, layout)
        mt = torch.ops.omnitok.pixels_to_frames(x.to("meta"), layout)
        assert mt.shape == r.shape and mt.dtype == r.dtype == torch.uint8
        torch.library.opcheck(torch.ops.omnitok.pixels_to_frames.default, (x, layout),
                              test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.omnitok.frames_to_pixels.default, (clips, geom, 2, 32, 32, 0, 0),
                          test_utils=("test_schema", "test_faketensor"))
