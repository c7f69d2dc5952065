"""Generates tests/golden/val_*.npz: what the UNMODIFIED reference's VQGAN.forward(x) -- the branch validation_step runs,
OmniTokenizer/omnitokenizer.py:330-407, 520-525 -- returns on seeded synthetic weights and inputs, for
OmniTokenizer_VQGAN.forward(x) / validation_step (omnitokenizer_amd/vqgan.py, csrc/losses.hip).  Runs in the build container
only (the reference is located through oracle/ref_harness.py, read-only):

    python tests/golden/make_golden_validation.py

What the maker does around the reference, none of it arithmetic:
  perceptual_model   ref_harness stubs LPIPS (it is off the encode/decode path), so the reference's own LPIPS
                     (modules/lpips.py, loaded as make_golden_lpips.py loads it, synthetic weights of seed LPIPS_SEED) is
                     assigned to model.perceptual_model after construction
  Tensor.cuda        forward calls .cuda() on the drawn frame indices (:401); it is the identity for the duration of the call
  torch.randint / torch.randn   wrapped to RECORD what forward draws: the frame index per clip, the posterior noise
  Tensor.float       in the fp64 run of a spatial_pos='rel' (stage 1) model only, .float() widens to fp64 instead: the reference's learned relative position bias
                     casts its integer offsets with .float() (modules/attention.py:577), which a .double() model cannot take

Every case runs twice from the same seed: the model in fp32, and a second instance after .double() on the widened input.
The maker asserts that both runs drew the same indices / noise and that their ids agree on EVERY position (the commitment
bound of tests/test_gpu_validation.py needs flip-free fixtures).  Stored per case:
  stage, mode, overrides, batch, frames, weight_seed, input_seed, lpips_seed, draw_seed, state_crc, input_crc
  frame_idx [B] (videos without apply_allframes), noise (use_vae), x_resized (gen_upscale: the x the losses see)
  recon_loss32/64, perceptual32/64 (un-reduced), x_recon32, x_recon64_resid (x_recon64 = x_recon32 + resid to 1e-12; on the
  non-l1 path both carry the +0.5 of logits_laplace's in-place shift), x_shifted (1 if the reference shifted its input)
  VQ: ids, z32, z64_resid (b t h w c, what Codebook.forward is fed), commitment32/64, perplexity32/64
  VAE: moments32, moments64_resid, kl32/64
  fp64_run: 0 for the external codebook (VectorQuantize narrows its input with .float(), a .double() model cannot run):
  its "64" entries are the fp32 run's values
  lpips_val64 [N], lpips_res64 [N, 5]: the reference's LPIPS in fp64 on the fp32 run's own frames (widened), un-weighted, with
  its per-slice means
  l1_64, mse_64, laplace_64: the three raw means of the fp64 run, recomputed here in fp64 from its x and x_recon

The reference cannot run a gen_upscale VIDEO through this branch: :386 reads `frames` before it is assigned
(UnboundLocalError).  main() asserts that it still raises; the gen_upscale fixture is therefore an image batch.
"""
import importlib.util
import os
import sys
import tempfile
import warnings
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from oracle import ref_harness as rh  # noqa: E402
from omnitokenizer_amd.config import make_args, OmniTokConfig  # noqa: E402
from omnitokenizer_amd import synth  # noqa: E402
from omnitokenizer_amd.lpips import to_torchvision  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LPIPS_SEED = 23
# name, stage, attention mode, overrides, batch, frames (1 = image), input seed, seed of forward's own draws
CASES = [
    ("val_s2_sdpa_r64_img_l1", 2, "sdpa", dict(resolution=64), 2, 1, 1234, 7),
    ("val_s2_sdpa_r64_vid_l1", 2, "sdpa", dict(resolution=64), 1, 5, 1234, 7),
    # two clips, and a draw seed for which forward picks two different, non-zero frames: a gather that ignored frame_idx
    # or indexed it by the wrong clip would not pass (asserted in run_case)
    ("val_s2_sdpa_r64_vid_b2_l1", 2, "sdpa", dict(resolution=64), 2, 5, 1234, 13),
    ("val_s2_sdpa_r64_vid_mse", 2, "sdpa", dict(resolution=64, recon_loss_type="mse", logitslaplace_weight=0.5,
                                               apply_allframes=True), 1, 5, 1234, 7),
    ("val_s1_legacy_r64_vid", 1, "legacy", dict(resolution=64), 1, 5, 1234, 7),
    ("val_vae_s2_sdpa_r64_vid", 2, "sdpa", dict(resolution=64, use_vae=True, kl_weight=1e-4), 1, 5, 1234, 7),
    ("val_genup2_r64_img", 2, "sdpa", dict(resolution=64, gen_upscale=2), 1, 1, 1234, 7),
    ("val_ext_s2_sdpa_r64_img", 2, "sdpa", dict(resolution=64, use_external_codebook=True), 2, 1, 1234, 7),
]


def load_make_golden_lpips():
    spec = importlib.util.spec_from_file_location("make_golden_lpips", os.path.join(OUT, "make_golden_lpips.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Draws:
    """torch.randint / torch.randn / Tensor.cuda for the duration of one reference forward"""

    def __init__(self, widen_float=False):
        self.randint, self.randn, self.widen_float = [], [], widen_float

    def __enter__(self):
        self._ri, self._rn, self._cuda, self._float = torch.randint, torch.randn, torch.Tensor.cuda, torch.Tensor.float
        if self.widen_float:
            torch.Tensor.float = lambda t, *a, **k: t.double()

        def randint(*a, **k):
            r = self._ri(*a, **k)
            self.randint.append(r.clone())
            return r

        def randn(*a, **k):
            r = self._rn(*a, **k)
            self.randn.append(r.clone())
            return r

        torch.randint, torch.randn = randint, randn
        torch.Tensor.cuda = lambda t, *a, **k: t
        return self

    def __exit__(self, *exc):
        torch.randint, torch.randn, torch.Tensor.cuda, torch.Tensor.float = self._ri, self._rn, self._cuda, self._float


def run_once(args, mode, sd, lpips_cls, x, dtype, draw_seed):
    model = rh.build_reference_model(args)
    msg = model.load_state_dict(sd, strict=False)
    assert not msg.unexpected_keys, msg.unexpected_keys
    model.perceptual_model = lpips_cls().eval()
    want = synth.synth_lpips_state_dict(LPIPS_SEED)
    got = model.perceptual_model.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in got)
    model = model.to(dtype)
    taps = {}
    if model.use_vae:
        model.pre_vq_conv.register_forward_hook(lambda m, i, o: taps.__setitem__("moments", o.detach().clone()))
    else:
        model.codebook.register_forward_pre_hook(lambda m, i: taps.__setitem__("z", i[0].detach().clone()))
    xin = x.to(dtype).clone()   # logits_laplace shifts its arguments in place
    torch.manual_seed(draw_seed)
    with torch.no_grad(), rh.attention_mode(mode), Draws(widen_float=dtype == torch.float64 and args.spatial_pos == "rel") as d:
        recon_loss, x_recon, vq, perc = model(xin)
    out = dict(recon_loss=recon_loss, x_recon=x_recon, vq=vq, perceptual=perc, x_after=xin, draws=d, taps=taps,
               call_cnt=getattr(model.codebook, "call_cnt", None) if not model.use_vae else None)
    return out


def raw_means64(x, x_recon):
    """the three means in fp64, logits_laplace's formula (omnitokenizer.py:23-30) without its in-place shift"""
    x, r = x.double(), x_recon.double()
    lap = ((1 - 2 * 0.1) * (x + 0.5) + 0.1) - ((1 - 2 * 0.1) * (r + 0.5) + 0.1)
    return (r - x).abs().mean().item(), ((r - x) ** 2).mean().item(), lap.abs().mean().item()


def run_case(ref_lpips, name, stage, mode, overrides, batch, frames, input_seed, draw_seed):
    args = make_args(stage, **overrides)
    cfg = OmniTokConfig.from_args(args, attention_mode=mode)
    sd = synth.synth_state_dict(cfg, seed=0)
    is_image = frames == 1
    res = cfg.resolution
    x = synth.synth_image(batch, res, seed=input_seed) if is_image else synth.synth_video(batch, frames, res, seed=input_seed)
    r32 = run_once(args, mode, sd, ref_lpips.LPIPS, x, torch.float32, draw_seed)
    # VectorQuantize.forward narrows its input with x.float() and compares it with its own (then fp64) codebook: the
    # external quantiser has no fp64 run.  Its fixture carries the fp32 run's values, widened, under the "64" names.
    fp64_run = not args.use_external_codebook
    r64 = run_once(args, mode, sd, ref_lpips.LPIPS, x, torch.float64, draw_seed) if fp64_run else dict(r32)
    if not fp64_run:
        r64["x_recon"] = r32["x_recon"].double()
    l1_path = args.recon_loss_type == "l1"
    shift = 0.0 if l1_path else 0.5
    out = dict(stage=stage, mode=mode, overrides=repr(overrides), batch=batch, frames=frames, weight_seed=0,
               input_seed=input_seed, lpips_seed=LPIPS_SEED, draw_seed=draw_seed,
               state_crc=np.uint32(synth.state_checksum(sd)), input_crc=np.uint32(zlib.crc32(x.numpy().tobytes())),
               x_shifted=np.int32(not l1_path), fp64_run=np.int32(fp64_run))
    # what forward drew
    for a, b in zip(r32["draws"].randint, r64["draws"].randint):
        assert torch.equal(a, b)
    for a, b in zip(r32["draws"].randn, r64["draws"].randn):
        assert torch.equal(a, b)
    if not is_image:
        assert len(r32["draws"].randint) == 1
        if not args.apply_allframes:
            out["frame_idx"] = r32["draws"].randint[0].numpy().astype(np.int64)
            if batch > 1:
                assert len(set(out["frame_idx"].tolist())) == batch and out["frame_idx"].min() > 0, \
                    f"{name}: drew {out['frame_idx']}: choose a draw seed that gives distinct non-zero frames"
    else:
        assert not r32["draws"].randint
    if args.use_vae:
        assert len(r32["draws"].randn) == 1
        out["noise"] = r32["draws"].randn[0].numpy()
    else:
        assert not r32["draws"].randn
    # the reference's in-place shift of its own input, and of what it returns
    assert torch.equal(r32["x_after"], x + shift)
    x_seen64 = x.double()
    if args.gen_upscale is not None:
        import torch.nn.functional as F
        up = dict(scale_factor=args.gen_upscale, mode="bilinear", align_corners=True)
        out["x_resized"] = F.interpolate(x, **up).numpy()
        x_seen64 = F.interpolate(x.double(), **up)
    for tag, r in (("32", r32), ("64", r64)):
        out["recon_loss" + tag] = r["recon_loss"].numpy()
        out["perceptual" + tag] = r["perceptual"].numpy()
        assert r["recon_loss"].dim() == 0 and r["perceptual"].dim() == 4
    xr32, xr64 = r32["x_recon"], r64["x_recon"]
    assert xr32.dtype == torch.float32 and xr64.dtype == torch.float64
    out["x_recon32"] = xr32.numpy()
    out["x_recon64_resid"] = (xr64 - xr32.double()).float().numpy()
    out["l1_64"], out["mse_64"], out["laplace_64"] = raw_means64(x_seen64, xr64 - shift)
    if args.use_vae:
        m32, m64 = r32["taps"]["moments"], r64["taps"]["moments"]
        out["moments32"] = m32.numpy()
        out["moments64_resid"] = (m64 - m32.double()).float().numpy()
        out["kl32"], out["kl64"] = r32["vq"]["commitment_loss"].numpy(), r64["vq"]["commitment_loss"].numpy()
        assert set(r32["vq"]) == {"commitment_loss"}
        extra = f"kl {out['kl64']:.6e}"
    else:
        ids32, ids64 = r32["vq"]["encodings"], r64["vq"]["encodings"]
        flips = int((ids32 != ids64).sum())
        assert flips == 0, f"{name}: {flips} ids differ between the fp32 and the fp64 run: choose another seed"
        out["ids"] = ids32.numpy().astype(np.int16)
        out["commitment32"], out["commitment64"] = (r["vq"]["commitment_loss"].numpy() for r in (r32, r64))
        out["perplexity32"], out["perplexity64"] = (r["vq"]["perplexity"].numpy() for r in (r32, r64))
        if not args.use_external_codebook:
            z32, z64 = (r["taps"]["z"].permute(0, 2, 3, 4, 1).contiguous() for r in (r32, r64))
            out["z32"] = z32.numpy()
            out["z64_resid"] = (z64 - z32.double()).float().numpy()
            assert r32["call_cnt"] == 1
        extra = f"commitment {float(out['commitment64']):.6e} perplexity {float(out['perplexity64']):.3f}"
    # the perceptual term alone: the reference's LPIPS in fp64 on the fp32 run's OWN frames (widened), with the per-slice
    # means its forward computes (spatial_average, recorded) -- what the bar of tests/test_gpu_lpips.py is built from
    xa, ra = r32["x_after"], xr32
    if "x_resized" in out:
        xa = torch.from_numpy(out["x_resized"])
    if is_image:
        fa, fb = xa, ra
    elif args.apply_allframes:
        fa, fb = (t.permute(0, 2, 1, 3, 4).reshape(-1, 3, *t.shape[-2:]) for t in (xa, ra))
    else:
        idx = torch.from_numpy(out["frame_idx"]).reshape(-1, 1, 1, 1, 1).repeat(1, 3, 1, *xa.shape[-2:])
        fa, fb = torch.gather(xa, 2, idx).squeeze(2), torch.gather(ra, 2, idx).squeeze(2)
    recorded = []
    spatial_average = ref_lpips.spatial_average
    ref_lpips.spatial_average = lambda t, keepdim=True: (lambda r: (recorded.append(r.clone()), r)[1])(spatial_average(t, keepdim=keepdim))
    try:
        with torch.no_grad():
            val = ref_lpips.LPIPS().eval().double()(fa.double(), fb.double())
    finally:
        ref_lpips.spatial_average = spatial_average
    n = fa.shape[0]
    out["lpips_res64"] = torch.cat([r.view(n, 1) for r in recorded], 1).numpy()
    out["lpips_val64"] = val.view(n).numpy()
    assert out["lpips_res64"].shape == (n, 5)
    assert np.abs(out["lpips_val64"] * args.perceptual_weight - out["perceptual32"].reshape(-1)).max() < 1e-4
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB, recon_loss {float(out['recon_loss64']):.6e} "
          f"(fp32 run off by {abs(float(out['recon_loss32']) - float(out['recon_loss64'])):.1e}), perceptual "
          f"{out['perceptual64'].reshape(-1)[:3]}, {extra}, frame_idx {out.get('frame_idx')}")
    assert os.path.getsize(path) < (1 << 20), path


def assert_reference_genup_video_raises(lpips_cls):
    args = make_args(2, resolution=64, gen_upscale=2)
    model = rh.build_reference_model(args)
    model.perceptual_model = lpips_cls().eval()
    try:
        with torch.no_grad(), Draws():
            model(synth.synth_video(1, 5, 64, seed=1234))
    except UnboundLocalError:
        return
    raise SystemExit("the reference now runs a gen_upscale video through forward(x): add the video fixture")


def main():
    assert rh.reference_available(), "run in the build container (needs the reference)"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rh.install_stubs()
    mgl = load_make_golden_lpips()
    mgl.WEIGHT_SEED = LPIPS_SEED
    with tempfile.TemporaryDirectory() as tmp:
        vgg_pth = os.path.join(tmp, "vgg.pth")
        torch.save(to_torchvision(synth.synth_lpips_state_dict(LPIPS_SEED))[1], vgg_pth)
        ref_lpips = mgl.load_reference(vgg_pth)
        only = sys.argv[1] if len(sys.argv) > 1 else None
        for c in CASES:
            if only is None or only in c[0]:
                run_case(ref_lpips, *c)
        if only is None:
            assert_reference_genup_video_raises(ref_lpips.LPIPS)


if __name__ == "__main__":
    main()
