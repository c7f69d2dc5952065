"""The DDIM step of the reference's gaussian_diffusion.py:513-598 restated in torch, the counterpart of dit_ref.p_sample: the
yardstick of tests/test_gpu_ddim.py and of the cpu_fp32_err_* figures in tests/golden/ddim_loop.npz."""
import torch


def ddim_step(coef_row, model_out, x, noise, learned_range, clip, reverse):
    """One timestep shared by the batch.  coef_row: the 8 scalars of omnitokenizer_amd.diffusion.DDIMDiffusion.ddim_coefficient_table
    (fp32 values, as the reference's fp32 scalar chain leaves them); the arithmetic runs in model_out's dtype.  x [N,C,H,W] or
    [N,F,C,H,W]: the eps half is the first C channels of dim -3.  noise may be None (taken as absent, not as zeros) and is not read
    under reverse.  Returns (sample, pred_xstart)."""
    dtype = model_out.dtype
    k = [torch.tensor(float(v), dtype=torch.float32).to(dtype) for v in coef_row]
    x = x.to(dtype)
    C = x.shape[-3]
    eps = model_out.narrow(-3, 0, C) if learned_range else model_out
    xs = k[0] * x - k[1] * eps
    if clip:
        xs = xs.clamp(-1, 1)
    e = (k[0] * x - xs) / k[1]  # the reference re-derives eps from pred_xstart (_predict_eps_from_xstart)
    if reverse:
        return xs * k[5] + k[6] * e, xs
    sample = xs * k[2] + k[3] * e
    if noise is not None:
        sample = sample + k[4] * noise.to(dtype)
    return sample, xs
