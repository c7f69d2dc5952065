#!/usr/bin/env python
"""The DDIM sampler against the ancestral one, in one session (the conventions of tools/dit_bench.py: device events, medians).

    python tools/ddim_bench.py --out profiles/ddim_bench.json

  kernels          omnitok_dit_ddim_step (eta 0: no noise; eta 0.5: with noise; the reverse step) and omnitok_dit_p_sample alone at the
                   DiT-XL/2 latent of 16 samples, [16, 8, 32, 32] with a learned-range model output: ms per call (10 back-to-back calls
                   per timed event pair), the bytes each must move and the fraction of the HBM peak that makes.  The tensors are 0.5 MiB
                   each: the calls are bound by the launch, not by memory, and the fractions say so.
  generate_images  DiT-XL/2 (seeded random weights, fp32, the default formats) with the --use_vae tokenizer at 256 x 256, 8 labels with
                   classifier-free guidance = 16 streams: create_diffusion("250") + the ancestral sampler (timed first and again at the end)
                   against create_ddim_diffusion("ddim50") + sample_method="ddim", eta 0.  The ratio is the step count's: the per-step
                   cost is the denoiser's in both.  Sample quality is NOT assessed: the weights are random.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_TBS = 8.0


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="DiT-XL/2")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--ddpm-respacing", default="250")
    ap.add_argument("--ddim-respacing", default="ddim50")
    ap.add_argument("--skip-generate", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ddim_bench needs the GPU: there is nothing to measure without it")
    from omnitokenizer_amd import _lib
    from omnitokenizer_amd.diffusion import create_ddim_diffusion, create_diffusion, generate_images
    from tests import dit_ref

    lib = _lib.load()
    P = ctypes.c_void_p
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    B, C, HW = 2 * a.images, 8, 32 * 32
    x, noise, mo = (torch.randn(B, c, 32, 32, device="cuda", generator=g) for c in (C, C, 2 * C))
    out, xs = torch.empty_like(x), torch.empty_like(x)
    ddpm, ddim = create_diffusion(a.ddpm_respacing), create_ddim_diffusion(a.ddim_respacing)
    t = torch.full((B,), ddim.num_timesteps // 2, device="cuda", dtype=torch.int64)
    tabs = {"p": torch.from_numpy(ddpm.coefficient_table()).cuda(), 0.0: torch.from_numpy(ddim.ddim_coefficient_table(0.0)).cuda(),
            0.5: torch.from_numpy(ddim.ddim_coefficient_table(0.5)).cuda()}

    def ddim_call(eta, reverse):
        n = P(noise.data_ptr()) if eta > 0 and not reverse else None
        return lambda: _lib.check(lib.omnitok_dit_ddim_step(P(mo.data_ptr()), P(x.data_ptr()), n, P(tabs[eta].data_ptr()), ddim.num_timesteps,
                                                            P(t.data_ptr()), B, C, HW, 1, 0, int(reverse), P(out.data_ptr()), P(xs.data_ptr()), st))

    def p_sample_call():
        _lib.check(lib.omnitok_dit_p_sample(P(mo.data_ptr()), P(x.data_ptr()), P(noise.data_ptr()), P(tabs["p"].data_ptr()), ddpm.num_timesteps,
                                            P(t.data_ptr()), B, C, HW, 1, 0, P(out.data_ptr()), P(xs.data_ptr()), st))

    elem = B * C * HW * 4
    # tensors moved: x, eps (+ noise) in, x_out and pred_xstart out; p_sample also reads the variance half
    ops = {"ddim_step_eta0": (ddim_call(0.0, False), 4 * elem), "ddim_step_eta0.5": (ddim_call(0.5, False), 5 * elem),
           "ddim_reverse_step": (ddim_call(0.0, True), 4 * elem), "p_sample": (p_sample_call, 6 * elem)}
    kernels = {}
    for name, (fn, nbytes) in ops.items():
        def rep(fn=fn):
            for _ in range(10):
                fn()
        med, lo, hi = timed(rep, 3, 20)
        tbs = nbytes / (med / 10 * 1e-3) / 1e12
        kernels[name] = {"ms_per_call": round(med / 10, 5), "ms_per_call_min_max": [round(lo / 10, 5), round(hi / 10, 5)], "bytes": nbytes,
                         "tb_per_s": round(tbs, 4), "frac_of_hbm_peak": round(tbs / PEAK_HBM_TBS, 5)}
    res = {"bench": "ddim", "device": torch.cuda.get_device_name(0), "latent": [B, C, 32, 32], "learned_range": True,
           "peak_hbm_tb_per_s": PEAK_HBM_TBS, "kernels": kernels,
           "kernels_note": "10 back-to-back calls per timed pair of device events; 0.5 MiB per tensor: launch-bound, not memory-bound"}

    if not a.skip_generate:
        from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
        from omnitokenizer_amd.config import OmniTokConfig
        from omnitokenizer_amd.dit import DiT_models
        args = make_args(2, resolution=256, use_vae=True)
        vae = OmniTokenizer_VQGAN(args)
        vae.load_state_dict(synth.synth_state_dict(OmniTokConfig.from_args(args), seed=0), strict=True)
        vae = vae.cuda().eval()
        m = DiT_models[a.model](input_size=32, in_channels=8, num_classes=1000)
        cfg = dict(input_size=32, patch_size=m.patch_size, in_channels=8, hidden_size=m.hidden_size, depth=m.depth, num_heads=m.num_heads,
                   mlp_ratio=4.0, class_dropout_prob=0.1, num_classes=1000, learn_sigma=True)
        m.load_state_dict(dit_ref.make_weights(cfg, 1), strict=True)
        m = m.cuda().eval()
        labels = torch.arange(a.images, device="cuda") % 1000

        def wall(diffusion, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            imgs = generate_images(m, diffusion, vae, labels, cfg_scale=4.0, seed=0, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, imgs

        wall(create_diffusion("4"))                                          # warm-up: workspaces, the decode
        wall(create_ddim_diffusion("ddim4"), sample_method="ddim")
        first, ref = wall(ddpm)
        ddim_ms, imgs = wall(ddim, sample_method="ddim", eta=0.0)
        ddim_ms2, again = wall(ddim, sample_method="ddim", eta=0.0)
        last, ref2 = wall(ddpm)
        assert torch.equal(imgs, again) and torch.equal(ref, ref2) and imgs.shape == (a.images, 256, 256, 3)
        res["generate_images"] = {
            "model": a.model, "images": a.images, "streams": B, "cfg_scale": 4.0, "formats": "fp32 (the defaults)",
            "ddpm": {"respacing": a.ddpm_respacing, "steps": ddpm.num_timesteps, "ms_first": round(first, 2), "ms_last": round(last, 2),
                     "ms_per_step": round(min(first, last) / ddpm.num_timesteps, 3)},
            "ddim": {"respacing": a.ddim_respacing, "steps": ddim.num_timesteps, "eta": 0.0, "ms": [round(ddim_ms, 2), round(ddim_ms2, 2)],
                     "ms_per_step": round(min(ddim_ms, ddim_ms2) / ddim.num_timesteps, 3)},
            "speedup": round(min(first, last) / min(ddim_ms, ddim_ms2), 3),
            "note": "the ratio is the step count's (the decode is in both); sample quality was not assessed: random weights, no checkpoint",
        }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
