"""Generates tests/golden/ddim_loop.npz from the reference's own diffusion packages (Diffusion/DiT/diffusion and
Diffusion/Latte/diffusion), in fp64.

    python tests/golden/make_golden_ddim.py /path/to/OmniTokenizer-reference

Run once where the reference tree exists; the fixture holds DATA only (inputs, the reference's outputs, its tables) and the tests read
nothing else.  The reference draws a step's noise with torch.randn_like whatever eta is (gaussian_diffusion.py:551); it is patched
to replay the recorded draws.

  x0, step_noise                  the start and the 10 draws of the 4-D loops (DiT package), [3,4,5,5]
  dit_eta{0,0.5,1}_{clip,noclip}  ddim_sample_loop_progressive with "ddim10" and tests/dit_ref.py's toy model: the 10 samples
  dit_reverse                     ddim_reverse_sample walked from x0 at t = 0 up to t = 9, eta 0, clip off
  latte_x0, latte_step_noise, latte_eta{0,0.5}_noclip
                                  the same from the Latte package over [2,3,4,5,5] with tests/latte_ref.py's toy model
  cpu_fp32_err_<trajectory>       the max-abs error of the same loop run in fp32 by torch on the CPU through tests/ddim_ref.py with
                                  this package's coefficient table, against that fp64 trajectory: the yardstick of the GPU's error (4 x)
  <respacing>/timestep_map, alphas_cumprod, alphas_cumprod_prev, alphas_cumprod_next
                                  for "ddim10", "ddim50" and "10,15,20" (key s10_15_20), fp64
  ddim_timesteps/<count>          space_timesteps(1000, "ddim<count>") sorted, counts 7, 10, 25, 50, 250; ddim_timesteps/no_stride:
                                  the counts for which the reference raises ValueError (300)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import ddim_ref, dit_ref, latte_ref  # noqa: E402

RESPACING = "ddim10"
DIT_SHAPE = (3, 4, 5, 5)
LATTE_SHAPE = (2, 3, 4, 5, 5)


def eta_tag(eta):
    return f"eta{eta:g}"


def reference_package(ref_root, name):
    """The `diffusion` package of Diffusion/<name>: both are called `diffusion`, so the other one is dropped from sys.modules first."""
    for mod in [m for m in sys.modules if m == "diffusion" or m.startswith("diffusion.")]:
        del sys.modules[mod]
    path = os.path.join(ref_root, "Diffusion", name)
    sys.path.insert(0, path)
    try:
        import diffusion
        assert os.path.dirname(os.path.dirname(os.path.abspath(diffusion.__file__))) == os.path.abspath(path)
        return diffusion
    finally:
        sys.path.remove(path)


def replaying(noise):
    """torch.randn_like replaced by the rows of `noise` in order, for the length of a `with`."""
    class Patch:
        def __enter__(self):
            draws = iter(torch.from_numpy(noise))
            self.orig = torch.randn_like
            torch.randn_like = lambda x: next(draws).to(x.dtype)

        def __exit__(self, *exc):
            torch.randn_like = self.orig
    return Patch()


def cpu_fp32_error(ours, toy, coef, x0, noise, traj, clip, eta, reverse=False):
    """The loop in fp32 on the CPU through ddim_ref.ddim_step against the reference's fp64 trajectory."""
    n = ours.num_timesteps
    x = torch.from_numpy(x0).float()
    err = 0.0
    for k, i in enumerate(range(n) if reverse else range(n - 1, -1, -1)):
        tt = torch.full((x0.shape[0],), ours.timestep_map[i], dtype=torch.int64)
        draw = torch.from_numpy(noise[k]).float() if eta > 0 and not reverse else None
        x, _ = ddim_ref.ddim_step(coef[i], toy(x, tt), x, draw, True, clip, reverse)
        err = max(err, float((x.double() - torch.from_numpy(traj[k])).abs().max()))
    assert np.isfinite(err) and err > 0, err
    return err


def main(ref_root):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    ours = create_ddim_diffusion(RESPACING)
    out = {"respacing": np.array(RESPACING)}
    rng = np.random.default_rng(177)

    for pkg, prefix, shape, toy, cases in (
            ("DiT", "dit", DIT_SHAPE, dit_ref.toy_model, [(eta, clip) for eta in (0.0, 0.5, 1.0) for clip in (True, False)]),
            ("Latte", "latte", LATTE_SHAPE, latte_ref.toy_model, [(0.0, False), (0.5, False)])):
        ref = reference_package(ref_root, pkg)
        d = ref.create_diffusion(RESPACING)
        assert d.timestep_map == ours.timestep_map
        x0 = rng.normal(size=shape)
        noise = rng.normal(size=(d.num_timesteps, *shape))
        names = ("x0", "step_noise") if prefix == "dit" else ("latte_x0", "latte_step_noise")
        out[names[0]], out[names[1]] = x0, noise
        for eta, clip in cases:
            with replaying(noise):
                traj = np.stack([o["sample"].numpy() for o in d.ddim_sample_loop_progressive(
                    toy, shape, noise=torch.from_numpy(x0), clip_denoised=clip, device="cpu", eta=eta)])
            key = f"{prefix}_{eta_tag(eta)}_{'clip' if clip else 'noclip'}"
            assert traj.dtype == np.float64 and traj.shape == (d.num_timesteps, *shape)
            out[key] = traj
            out[f"cpu_fp32_err_{key}"] = np.float64(cpu_fp32_error(ours, toy, ours.ddim_coefficient_table(eta), x0, noise, traj, clip, eta))
            print(key, "max|x|", float(np.abs(traj).max()), "cpu fp32 err", float(out[f"cpu_fp32_err_{key}"]))
        if prefix == "dit":
            x, traj = torch.from_numpy(x0), []
            with torch.no_grad():
                for i in range(d.num_timesteps):
                    x = d.ddim_reverse_sample(toy, x, torch.tensor([i] * shape[0]), clip_denoised=False, eta=0.0)["sample"]
                    traj.append(x.numpy())
            traj = np.stack(traj)
            out["dit_reverse"] = traj
            out["cpu_fp32_err_dit_reverse"] = np.float64(cpu_fp32_error(ours, toy, ours.ddim_coefficient_table(0.0), x0, noise, traj, False,
                                                                        0.0, reverse=True))
            print("dit_reverse max|x|", float(np.abs(traj).max()), "cpu fp32 err", float(out["cpu_fp32_err_dit_reverse"]))
            # ---- tables and the striding, from the DiT package ---------------------------------------------------------------------
            for key, resp in (("ddim10", "ddim10"), ("ddim50", "ddim50"), ("s10_15_20", "10,15,20")):
                t = ref.create_diffusion(resp)
                out[f"{key}/timestep_map"] = np.asarray(t.timestep_map, dtype=np.int64)
                for n in ("alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next"):
                    out[f"{key}/{n}"] = np.asarray(getattr(t, n), dtype=np.float64)
            from diffusion.respace import space_timesteps
            no_stride = []
            for count in (7, 10, 25, 50, 250, 300):
                try:
                    out[f"ddim_timesteps/{count}"] = np.asarray(sorted(space_timesteps(1000, f"ddim{count}")), dtype=np.int64)
                except ValueError:
                    no_stride.append(count)
            assert no_stride == [300]
            out["ddim_timesteps/no_stride"] = np.asarray(no_stride, dtype=np.int64)

    np.savez_compressed(os.path.join(HERE, "ddim_loop.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
