"""Generates tests/golden/lpips_*.npz: the reference's OWN LPIPS values (OmniTokenizer/modules/lpips.py, taming's VGG16
LPIPS, the tokenizer's perceptual model) on seeded images and seeded synthetic weights, for omnitokenizer_amd.lpips
(csrc/lpips.hip).  Runs the UNMODIFIED reference file, located through oracle/ref_harness.py (read-only) and loaded by file
path, in the build container only:

    python tests/golden/make_golden_lpips.py

The stand-ins, none of them arithmetic:
  torchvision   a minimal module whose models.vgg16(pretrained=True) returns torchvision's VGG16 `features` layout (cfg D:
                indices 0..30, Conv2d(3 x 3, pad 1) / ReLU(inplace=True) / MaxPool2d(2, 2), torchvision's registration order)
                filled from synth.synth_lpips_state_dict(WEIGHT_SEED)
  requests      a module whose every function raises (lpips.py imports it for its download)
  get_ckpt_path the loaded module's is replaced by one that returns a temporary vgg.pth holding the synthetic lin weights
main() asserts that the stand-ins served every load.

Images: synth.synth_fid_images with the stored seeds, uint8 [n, H, W, 3], turned into the tokenizer's range as
x = float(u) / 255 + SHIFT (SHIFT = -0.5) in fp32, NCHW; the second image of a pair is the same content plus N(0, NOISE^2)
("noise"), an unrelated image ("other") or the first image itself ("same").  Per case:
  res32 / res64 [n, 5]   the per-slice spatial means the reference's forward computes (its spatial_average, recorded),
                         fp32 run and model.double() run (inputs widened to fp64)
  val32 / val64 [n]      LPIPS.forward's output
  rms [5]                the RMS of each slice's output (fp32 run, both images): the synthetic weights keep it O(1)
lpips_keys.npz holds the reference's LPIPS().state_dict() key set and shapes.
"""
import importlib.util
import os
import sys
import tempfile
import time
import types
import warnings

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from oracle import ref_harness as rh  # noqa: E402
from omnitokenizer_amd import synth  # noqa: E402
from omnitokenizer_amd.lpips import to_torchvision  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
WEIGHT_SEED = 23
NOISE = 0.03
SHIFT = -0.5
# name -> (H, W, seed, second image: "noise" | "other" | "same", second seed, pairs)
CASES = {"lpips_16x16": (16, 16, 61, "other", 62, 3),
         "lpips_50x70": (50, 70, 63, "noise", 64, 3),
         "lpips_64x64": (64, 64, 65, "noise", 66, 4),
         "lpips_256x256": (256, 256, 67, "noise", 68, 3),
         "lpips_same_32x32": (32, 32, 69, "same", 0, 2),
         "lpips_light_40x40": (40, 40, 71, "noise", 72, 2)}


def case_images(H, W, seed, mode, seed2, n):
    """the uint8 [n, H, W, 3] pair of a case"""
    a = synth.synth_fid_images(n, H, W, seed)
    if mode == "noise":
        b = synth.synth_fid_images(n, H, W, seed, NOISE, seed2)
    elif mode == "other":
        b = synth.synth_fid_images(n, H, W, seed2)
    else:
        b = a.copy()
    return a, b


def to_input(u: np.ndarray) -> torch.Tensor:
    """uint8 [n, H, W, 3] -> fp32 [n, 3, H, W]: float(u) / 255 + SHIFT, each step in fp32"""
    return torch.from_numpy(u).permute(0, 3, 1, 2).to(torch.float32) / 255 + SHIFT


# ---- the stand-ins -------------------------------------------------------------------------------------------------------

VGG_CALLS, CKPT_CALLS = [], []
CFG_D = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]


class VGG(nn.Module):
    """torchvision's VGG16 `features` (make_layers(cfg D), no batch norm); the classifier is not needed by LPIPS"""

    def __init__(self):
        super().__init__()
        layers, c = [], 3
        for v in CFG_D:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(c, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                c = v
        self.features = nn.Sequential(*layers)


def vgg16(pretrained=False, **kwargs):
    if not pretrained:
        raise RuntimeError("stand-in vgg16: LPIPS asks for pretrained=True")
    m = VGG()
    vgg, _ = to_torchvision(synth.synth_lpips_state_dict(WEIGHT_SEED))
    missing, unexpected = m.load_state_dict(vgg, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    VGG_CALLS.append(1)
    return m


def _no_network(*args, **kwargs):
    raise RuntimeError("make_golden_lpips: no code path may download anything")


def install_modules():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    tv = module("torchvision", __version__="0.17.1")
    tv.models = module("torchvision.models", vgg16=vgg16)
    module("requests", get=_no_network, request=_no_network, Session=_no_network)


def load_reference(vgg_pth: str):
    install_modules()
    path = os.path.join(rh.REFERENCE_ROOT, "OmniTokenizer", "modules", "lpips.py")
    spec = importlib.util.spec_from_file_location("ref_lpips", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_lpips"] = mod
    spec.loader.exec_module(mod)

    def get_ckpt_path(name, root, check=False):
        assert name == "vgg_lpips", name
        CKPT_CALLS.append(name)
        return vgg_pth

    mod.get_ckpt_path = get_ckpt_path
    mod.download = _no_network
    return mod


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with tempfile.TemporaryDirectory() as tmp:
        vgg_pth = os.path.join(tmp, "vgg.pth")
        torch.save(to_torchvision(synth.synth_lpips_state_dict(WEIGHT_SEED))[1], vgg_pth)
        ref = load_reference(vgg_pth)
        model = ref.LPIPS().eval()
        model64 = ref.LPIPS().eval().double()
    assert len(VGG_CALLS) == 2 and CKPT_CALLS == ["vgg_lpips"] * 2, (VGG_CALLS, CKPT_CALLS)
    sd = model.state_dict()
    want = synth.synth_lpips_state_dict(WEIGHT_SEED)
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in sd)
    np.savez_compressed(os.path.join(OUT, "lpips_keys.npz"), keys=np.array(list(sd)),
                        shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]))

    recorded = []
    spatial_average = ref.spatial_average

    def recording(x, keepdim=True):
        r = spatial_average(x, keepdim=keepdim)
        recorded.append(r.clone())   # LPIPS.forward's `val += res[l]` adds into res[0] in place
        return r

    ref.spatial_average = recording   # LPIPS.forward looks it up at call time
    sq = {}
    for k in range(1, 6):
        getattr(model.net, f"slice{k}").register_forward_hook(
            lambda mod, inp, o, k=k: sq.setdefault(k, []).append((o.double().pow(2).sum().item(), o.numel())))
    with torch.no_grad():
        for name, (H, W, seed, mode, seed2, n) in CASES.items():
            t0 = time.time()
            a, b = (to_input(u) for u in case_images(H, W, seed, mode, seed2, n))
            out = dict(H=H, W=W, seed=seed, mode=mode, seed2=seed2, n=n, noise=NOISE, shift=SHIFT, weight_seed=WEIGHT_SEED)
            sq.clear()
            recorded.clear()
            val32 = model(a, b)
            out["res32"] = torch.cat([r.view(n, 1) for r in recorded], 1).numpy()
            out["val32"] = val32.view(n).numpy()
            out["rms"] = np.array([np.sqrt(sum(s for s, _ in sq[k]) / sum(c for _, c in sq[k])) for k in range(1, 6)])
            recorded.clear()
            val64 = model64(a.double(), b.double())
            out["res64"] = torch.cat([r.view(n, 1) for r in recorded], 1).numpy()
            out["val64"] = val64.view(n).numpy()
            assert out["res32"].dtype == np.float32 and out["res64"].dtype == np.float64
            np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
            err = np.abs(out["val32"] - out["val64"]).max()
            print(f"{name}: {time.time() - t0:.0f} s, val64 {out['val64']}, slice rms {out['rms']}, "
                  f"|val32 - val64| max {err:.2e}")


if __name__ == "__main__":
    main()
