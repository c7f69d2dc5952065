"""The ancestral sampler of the reference's Diffusion/DiT/diffusion package on the MI355X: `create_diffusion` with the reference's
signature, and of the object it returns what sample.py / sample_ddp.py use -- p_sample_loop, p_sample, timestep_map,
num_timesteps.  Diffusion/Latte/diffusion is the same package with 5-D video latents [N,F,C,H,W]; p_sample takes both.

    from omnitokenizer_amd.diffusion import create_diffusion, generate_images
    diffusion = create_diffusion("250")
    samples = diffusion.p_sample_loop(model.forward_with_cfg, z.shape, z, clip_denoised=False,
                                      model_kwargs=dict(y=y, cfg_scale=4.0), device=z.device)

Built: epsilon prediction, LEARNED_RANGE or fixed variances, the linear schedule, space_timesteps with its section form
("10,15,20").  The coefficient tables are computed on the host in fp64 exactly as the reference's numpy does (respacing
included) and rounded to fp32 where _extract_into_tensor rounds them (gaussian_diffusion.py:861-874); one step is one model call
plus ONE element-wise kernel (omnitok_dit_p_sample).  Everything else raises NotImplementedError with the reference line.

The DDIM sampler (gaussian_diffusion.py:513-680, the Latte scripts' `--sample_method ddim`) and the "ddimN" striding come on an object
of their own, because create_diffusion("ddimN") and SpacedDiffusion.ddim_* are pinned as refused:

    diffusion = create_ddim_diffusion("ddim50")            # a DDIMDiffusion; the reference: create_diffusion("ddim50")
    samples = diffusion.ddim_sample_loop(model.forward_with_cfg, z.shape, z, clip_denoised=False,
                                         model_kwargs=dict(y=y, cfg_scale=4.0), device=z.device, eta=0.0)
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check

_REF = "Diffusion/DiT/diffusion/"


def space_timesteps(num_timesteps, section_counts):
    """respace.py:12-62: the timesteps of the original process to keep, for a count per equally sized section."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            raise NotImplementedError(f"the 'ddimN' striding ({_REF}respace.py:32-39) belongs to the DDIM sampler, which is not built")
        section_counts = [int(x) for x in section_counts.split(",")]
    size_per = num_timesteps // len(section_counts)
    extra = num_timesteps % len(section_counts)
    start_idx = 0
    all_steps = []
    for i, section_count in enumerate(section_counts):
        size = size_per + (1 if i < extra else 0)
        if size < section_count:
            raise ValueError(f"cannot divide section of {size} steps into {section_count}")
        frac_stride = 1 if section_count <= 1 else (size - 1) / (section_count - 1)
        cur_idx = 0.0
        for _ in range(section_count):
            all_steps.append(start_idx + round(cur_idx))
            cur_idx += frac_stride
        start_idx += size
    return set(all_steps)


def linear_betas(num_diffusion_timesteps):
    """get_named_beta_schedule("linear") (gaussian_diffusion.py:106-115): Ho et al.'s schedule scaled to any step count."""
    scale = 1000 / num_diffusion_timesteps
    return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)


def _not_built(what, where):
    raise NotImplementedError(f"{what} is not built ({_REF}{where})")


class SpacedDiffusion:
    """respace.py:65-129 over gaussian_diffusion.py:144-201: the respaced process and its fp64 tables."""

    COEF_NAMES = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
                  "posterior_log_variance_clipped", "log_betas", "fixed_log_variance", "nonzero_mask")

    def __init__(self, use_timesteps, betas, learn_sigma=True, sigma_small=False):
        self.use_timesteps = set(use_timesteps)
        self.original_num_steps = len(betas)
        self.learn_sigma = bool(learn_sigma)
        self.sigma_small = bool(sigma_small)
        base_cumprod = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64), axis=0)
        last = 1.0
        new_betas, self.timestep_map = [], []
        for i, ac in enumerate(base_cumprod):
            if i in self.use_timesteps:
                new_betas.append(1 - ac / last)
                last = ac
                self.timestep_map.append(i)
        betas = np.array(new_betas, dtype=np.float64)
        assert betas.ndim == 1 and (betas > 0).all() and (betas <= 1).all()
        self.betas = betas
        self.num_timesteps = int(betas.shape[0])
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:])) \
            if len(self.posterior_variance) > 1 else np.array([])
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
        if self.num_timesteps < 2:
            raise ValueError("the sampler needs at least two timesteps (the reference's clipped log variance is empty below)")
        self._dev_tables = {}

    # ---- the per-timestep scalars of one ancestral step ---------------------------------------------------------------------
    def coefficient_table(self) -> np.ndarray:
        """[num_timesteps, 8] fp32, the columns of COEF_NAMES (include/omnitok_dit.h, omnitok_dit_p_sample): each fp64 table
        rounded to fp32 as _extract_into_tensor's .float() does.  The fixed log variance is FIXED_LARGE's
        log(append(posterior_variance[1], betas[1:])) or, with sigma_small, the clipped posterior one (gaussian_diffusion.py:295-306)."""
        fixed = self.posterior_log_variance_clipped if self.sigma_small else \
            np.log(np.append(self.posterior_variance[1], self.betas[1:]))
        cols = [self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod, self.posterior_mean_coef1,
                self.posterior_mean_coef2, self.posterior_log_variance_clipped, np.log(self.betas), fixed,
                (np.arange(self.num_timesteps) != 0).astype(np.float64)]
        return np.stack(cols, axis=1).astype(np.float32)

    def _table_on(self, device):
        key = str(device)
        if key not in self._dev_tables:
            self._dev_tables[key] = (torch.from_numpy(self.coefficient_table()).to(device).contiguous(),
                                     torch.tensor(self.timestep_map, device=device, dtype=torch.int64))
        return self._dev_tables[key]

    # ---- sampling ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _refuse(denoised_fn=None, cond_fn=None):
        if denoised_fn is not None:
            _not_built("denoised_fn", "gaussian_diffusion.py:310-315")
        if cond_fn is not None:
            _not_built("cond_fn (classifier guidance)", "gaussian_diffusion.py:346-356, 414-415")

    def _model_call(self, model, x, t, model_kwargs):
        """What p_sample and the DDIM steps share in front of their kernel: the argument checks, the model call with
        timestep_map[t] (respace.py:124-129) and the check of its output's shape.  Returns x and the model output as contiguous fp32,
        t as int64 on x's device, and (B, frames, C)."""
        if x.device.type != "cuda":
            raise RuntimeError(f"x is on {x.device}: the sampler runs on the GPU only")
        if x.dim() not in (4, 5):
            raise ValueError(f"x must be [N,C,H,W] or [N,F,C,H,W], got {tuple(x.shape)}")
        x = x.float().contiguous()
        B, frames, C = x.shape[0], (x.shape[1] if x.dim() == 5 else 1), x.shape[-3]
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        if tuple(t.shape) != (B,):
            raise ValueError(f"t must be [{B}]")
        model_output = model(x, self._table_on(x.device)[1][t], **(model_kwargs or {}))
        if isinstance(model_output, tuple):
            model_output = model_output[0]
        want = (*x.shape[:-3], C * (2 if self.learn_sigma else 1), *x.shape[-2:])
        if tuple(model_output.shape) != want:
            raise ValueError(f"model output {tuple(model_output.shape)}, expected {want}")
        return x, t, model_output.float().contiguous(), (B, frames, C)

    @staticmethod
    def _step_noise(noise, x):
        if noise is None:
            return torch.randn_like(x)
        if noise.shape != x.shape or noise.device != x.device:
            raise ValueError("noise must have x's shape and device")
        return noise.float().contiguous()

    @torch.no_grad()
    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, noise=None):
        """gaussian_diffusion.py:376-417.  x [N,C,H,W] fp32 on the GPU, t [N] indices of the RESPACED process; the model is called
        with timestep_map[t] (respace.py:124-129).  noise: this step's normal draw (default torch.randn_like(x)).
        Video latents x [N,F,C,H,W] (Diffusion/Latte/diffusion/gaussian_diffusion.py:277-291): the model returns [N,F,2C | C,H,W],
        split on dim 2, and the update runs over the N F frames with each sample's t repeated F times.
        Returns {"sample", "pred_xstart"}."""
        self._refuse(denoised_fn, cond_fn)
        x, t, model_output, (B, frames, C) = self._model_call(model, x, t, model_kwargs)
        coef = self._table_on(x.device)[0]
        noise = self._step_noise(noise, x)
        sample, xstart = torch.empty_like(x), torch.empty_like(x)
        if x.dim() == 5:
            t = t.repeat_interleave(frames)
        P = ctypes.c_void_p
        check(_lib.load().omnitok_dit_p_sample(P(model_output.data_ptr()), P(x.data_ptr()), P(noise.data_ptr()), P(coef.data_ptr()),
                                               self.num_timesteps, P(t.data_ptr()), B * frames, C, x.shape[-2] * x.shape[-1],
                                               int(self.learn_sigma),
                                               int(bool(clip_denoised)), P(sample.data_ptr()), P(xstart.data_ptr()),
                                               torch.cuda.current_stream().cuda_stream), "dit_p_sample")
        return {"sample": sample, "pred_xstart": xstart}

    @torch.no_grad()
    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False, step_noise=None):
        """gaussian_diffusion.py:464-511.  step_noise: [num_timesteps, *shape] -- row k is the draw of the k-th step taken
        (timestep num_timesteps - 1 - k) -- or a callable step_noise(k, shape, device); it replaces the per-step torch.randn."""
        self._refuse(denoised_fn, cond_fn)

        def step(img, t, kwargs, eps):
            return self.p_sample(model, img, t, clip_denoised=clip_denoised, model_kwargs=kwargs, noise=eps)

        yield from self._loop(step, model, shape, noise, model_kwargs, device, progress, step_noise)

    def _loop(self, step, model, shape, noise, model_kwargs, device, progress, step_noise):
        """The loop of p_sample_loop_progressive and ddim_sample_loop_progressive around step(img, t, model_kwargs, draw)."""
        if device is None:
            owner = getattr(model, "__self__", model)
            device = next(owner.parameters()).device
        device = torch.device(device)
        assert isinstance(shape, (tuple, list))
        img = noise if noise is not None else torch.randn(*shape, device=device)
        if step_noise is not None and not callable(step_noise) and tuple(step_noise.shape) != (self.num_timesteps, *shape):
            raise ValueError(f"step_noise must be [{self.num_timesteps}, *shape]")
        owner = getattr(model, "__self__", None)
        fast = owner is not None and hasattr(owner, "check_range") and getattr(model, "__name__", "") in ("forward", "forward_with_cfg")
        kwargs = dict(model_kwargs or {})
        if fast:
            kwargs["check_range"] = False  # one read-back after the loop instead of a host synchronisation per step
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for k, i in enumerate(indices):
            t = torch.full((shape[0],), i, device=device, dtype=torch.int64)
            if step_noise is None:
                eps = None
            elif callable(step_noise):
                eps = step_noise(k, tuple(shape), device)
            else:
                eps = step_noise[k].to(device)
            out = step(img, t, kwargs, eps)
            yield out
            img = out["sample"]
        if fast:
            owner.check_range()

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                      device=None, progress=False, step_noise=None):
        """gaussian_diffusion.py:419-462: all rows of the batch, as the reference returns them (with classifier-free guidance the
        caller `chunk`s the null half away)."""
        final = None
        for sample in self.p_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                                     cond_fn=cond_fn, model_kwargs=model_kwargs, device=device, progress=progress,
                                                     step_noise=step_noise):
            final = sample
        return final["sample"]

    # ---- what this class refuses: the DDIM sampler is DDIMDiffusion's (create_ddim_diffusion), the rest is not built ---------------
    def ddim_sample(self, *a, **k):
        _not_built("DDIM sampling", "gaussian_diffusion.py:513-560")

    def ddim_reverse_sample(self, *a, **k):
        _not_built("DDIM sampling", "gaussian_diffusion.py:562-598")

    def ddim_sample_loop(self, *a, **k):
        _not_built("DDIM sampling", "gaussian_diffusion.py:600-631")

    def ddim_sample_loop_progressive(self, *a, **k):
        _not_built("DDIM sampling", "gaussian_diffusion.py:633-680")

    def training_losses(self, *a, **k):
        _not_built("training_losses (DiT training)", "gaussian_diffusion.py:715-787")

    def calc_bpd_loop(self, *a, **k):
        _not_built("calc_bpd_loop", "gaussian_diffusion.py:805-858")


def ddim_timesteps(num_timesteps, count):
    """respace.py:32-39, the "ddimN" striding: range(0, num_timesteps, i) for the first integer stride i that keeps `count` steps."""
    for i in range(1, num_timesteps):
        if len(range(0, num_timesteps, i)) == count:
            return set(range(0, num_timesteps, i))
    raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")


class DDIMDiffusion(SpacedDiffusion):
    """A SpacedDiffusion with the DDIM sampler of gaussian_diffusion.py:513-680 next to the ancestral one: ddim_sample,
    ddim_reverse_sample (DDIM inversion), ddim_sample_loop and ddim_sample_loop_progressive with the reference's signatures plus this
    package's noise= / step_noise= arguments.  One step is one model call plus ONE element-wise kernel (omnitok_dit_ddim_step)."""

    DDIM_COEF_NAMES = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "sqrt_alphas_cumprod_prev", "sqrt_one_minus_prev_sigma2",
                       "sigma_nonzero", "sqrt_alphas_cumprod_next", "sqrt_one_minus_alphas_cumprod_next", "unused")

    def __init__(self, use_timesteps, betas, learn_sigma=True, sigma_small=False):
        super().__init__(use_timesteps, betas, learn_sigma=learn_sigma, sigma_small=sigma_small)
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self._ddim_dev_tables = {}

    @staticmethod
    def _eta(eta):
        eta = float(eta)
        if not np.isfinite(eta) or eta < 0:
            raise ValueError(f"eta must be finite and >= 0, got {eta}")
        return eta

    def ddim_coefficient_table(self, eta=0.0) -> np.ndarray:
        """[num_timesteps, 8] fp32, the columns of DDIM_COEF_NAMES (include/omnitok_dit.h, omnitok_dit_ddim_step).  The reference's
        _extract_into_tensor returns fp32 whatever x's dtype is, so its per-timestep scalars (gaussian_diffusion.py:543-558, 590-596)
        are an fp32 chain; it is done here, in numpy float32 from the fp64 tables rounded once, in the reference's operation order.
        Every operation is correctly rounded (IEEE), which is what torch's CPU tensors give for + - * / and, in all but about one
        element of a hundred of a long table, for its vectorised sqrt (tests/test_ddim_cpu.py).  A negative radicand in 1 - alpha_bar_prev - sigma^2 (a NaN in the reference) raises ValueError."""
        f32 = np.float32
        eta = f32(self._eta(eta))
        ab, abp, abn = (v.astype(f32) for v in (self.alphas_cumprod, self.alphas_cumprod_prev, self.alphas_cumprod_next))
        one = f32(1.0)
        sigma = eta * np.sqrt((one - abp) / (one - ab)) * np.sqrt(one - ab / abp)
        radicand = one - abp - sigma ** 2
        if not (radicand >= 0).all():
            bad = int(np.argmin(radicand >= 0))
            raise ValueError(f"eta {float(eta)}: 1 - alpha_bar_prev - sigma^2 = {float(radicand[bad])} < 0 at timestep {bad}")
        cols = [self.sqrt_recip_alphas_cumprod.astype(f32), self.sqrt_recipm1_alphas_cumprod.astype(f32), np.sqrt(abp), np.sqrt(radicand),
                sigma * (np.arange(self.num_timesteps) != 0).astype(f32), np.sqrt(abn), np.sqrt(one - abn),
                np.zeros(self.num_timesteps, f32)]
        table = np.stack(cols, axis=1)
        assert table.dtype == f32
        return table

    def _ddim_table_on(self, device, eta):
        key = (str(device), self._eta(eta))
        if key not in self._ddim_dev_tables:
            self._ddim_dev_tables[key] = torch.from_numpy(self.ddim_coefficient_table(eta)).to(device).contiguous()
        return self._ddim_dev_tables[key]

    def _ddim_step(self, model, x, t, clip_denoised, model_kwargs, eta, noise, reverse):
        x, t, model_output, (B, frames, C) = self._model_call(model, x, t, model_kwargs)
        coef = self._ddim_table_on(x.device, eta)
        # eta == 0 and the reverse step read no noise: none is drawn and none is passed
        noise = self._step_noise(noise, x) if eta > 0 and not reverse else None
        sample, xstart = torch.empty_like(x), torch.empty_like(x)
        if x.dim() == 5:
            t = t.repeat_interleave(frames)
        P = ctypes.c_void_p
        check(_lib.load().omnitok_dit_ddim_step(P(model_output.data_ptr()), P(x.data_ptr()), P(noise.data_ptr()) if noise is not None else None,
                                                P(coef.data_ptr()), self.num_timesteps, P(t.data_ptr()), B * frames, C,
                                                x.shape[-2] * x.shape[-1], int(self.learn_sigma), int(bool(clip_denoised)), int(reverse),
                                                P(sample.data_ptr()), P(xstart.data_ptr()), torch.cuda.current_stream().cuda_stream),
              "dit_ddim_step")
        return {"sample": sample, "pred_xstart": xstart}

    @torch.no_grad()
    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0, noise=None):
        """gaussian_diffusion.py:513-560: x_{t-1} from x_t.  x, t, the model call and the video form as p_sample.  noise: this step's
        normal draw, read only when eta > 0 (default torch.randn_like(x)); with eta == 0 nothing is drawn.
        Returns {"sample", "pred_xstart"}."""
        self._refuse(denoised_fn, cond_fn)
        return self._ddim_step(model, x, t, clip_denoised, model_kwargs, self._eta(eta), noise, False)

    @torch.no_grad()
    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0):
        """gaussian_diffusion.py:562-598: x_{t+1} from x_t by the reverse ODE (DDIM inversion); eta must be 0, where the reference
        asserts."""
        self._refuse(denoised_fn, cond_fn)
        if eta != 0.0:
            raise ValueError("Reverse ODE only for deterministic path (eta must be 0)")
        return self._ddim_step(model, x, t, clip_denoised, model_kwargs, 0.0, None, True)

    @torch.no_grad()
    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0, step_noise=None):
        """gaussian_diffusion.py:633-680.  step_noise as in p_sample_loop_progressive, consulted only when eta > 0."""
        self._refuse(denoised_fn, cond_fn)
        eta = self._eta(eta)
        self.ddim_coefficient_table(eta)  # a refused eta raises before the first model call

        def step(img, t, kwargs, eps):
            return self.ddim_sample(model, img, t, clip_denoised=clip_denoised, model_kwargs=kwargs, eta=eta, noise=eps)

        yield from self._loop(step, model, shape, noise, model_kwargs, device, progress, step_noise if eta > 0 else None)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                         device=None, progress=False, eta=0.0, step_noise=None):
        """gaussian_diffusion.py:600-631: all rows of the batch, as p_sample_loop returns them."""
        final = None
        for sample in self.ddim_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                                        cond_fn=cond_fn, model_kwargs=model_kwargs, device=device, progress=progress,
                                                        eta=eta, step_noise=step_noise):
            final = sample
        return final["sample"]


def _process(cls, stride, timestep_respacing, noise_schedule, sigma_small, predict_xstart, learn_sigma, diffusion_steps):
    if noise_schedule != "linear":
        _not_built(f"the {noise_schedule!r} noise schedule", "gaussian_diffusion.py:116-122")
    if predict_xstart:
        _not_built("predict_xstart (ModelMeanType.START_X)", "gaussian_diffusion.py:317-318")
    betas = linear_betas(diffusion_steps)
    if timestep_respacing is None or timestep_respacing == "":
        timestep_respacing = [diffusion_steps]
    return cls(stride(diffusion_steps, timestep_respacing), betas, learn_sigma=learn_sigma, sigma_small=sigma_small)


def create_diffusion(timestep_respacing, noise_schedule="linear", use_kl=False, sigma_small=False, predict_xstart=False,
                     learn_sigma=True, rescale_learned_sigmas=False, diffusion_steps=1000):
    """diffusion/__init__.py:10-46.  use_kl / rescale_learned_sigmas only choose a training loss there and are accepted."""
    return _process(SpacedDiffusion, space_timesteps, timestep_respacing, noise_schedule, sigma_small, predict_xstart, learn_sigma,
                    diffusion_steps)


def create_ddim_diffusion(timestep_respacing, noise_schedule="linear", use_kl=False, sigma_small=False, predict_xstart=False,
                          learn_sigma=True, rescale_learned_sigmas=False, diffusion_steps=1000):
    """create_diffusion for the DDIM sampler: the same signature and refusals, "ddimN" (respace.py:32-39) accepted next to "250" and
    "10,15,20", a DDIMDiffusion returned.  create_diffusion("ddimN") itself stays refused."""
    def stride(num_timesteps, section_counts):
        if isinstance(section_counts, str) and section_counts.startswith("ddim"):
            return ddim_timesteps(num_timesteps, int(section_counts[len("ddim"):]))
        return space_timesteps(num_timesteps, section_counts)

    return _process(DDIMDiffusion, stride, timestep_respacing, noise_schedule, sigma_small, predict_xstart, learn_sigma, diffusion_steps)


def _check_sample_method(diffusion, sample_method):
    if sample_method not in ("ddpm", "ddim"):
        raise ValueError(f"sample_method must be 'ddpm' or 'ddim', got {sample_method!r}")
    if sample_method == "ddim" and not isinstance(diffusion, DDIMDiffusion):
        raise TypeError("sample_method='ddim' needs a DDIMDiffusion: build it with create_ddim_diffusion")


def _run_sampler(diffusion, sample_method, eta, sample_fn, z, model_kwargs, device, gen):
    """--sample_method of the Latte scripts (sample/sample.py:100-107): "ddpm" is p_sample_loop, "ddim" ddim_sample_loop, both with
    clip_denoised=False.  The per-step draws come from `gen` in step order; DDIM with eta == 0 draws none."""
    def draw(k, shape, dev):
        return torch.randn(*shape, device=dev, generator=gen)

    if sample_method == "ddim":
        return diffusion.ddim_sample_loop(sample_fn, z.shape, z, clip_denoised=False, model_kwargs=model_kwargs, device=device,
                                          eta=eta, step_noise=draw)
    return diffusion.p_sample_loop(sample_fn, z.shape, z, clip_denoised=False, model_kwargs=model_kwargs, device=device,
                                   step_noise=draw)


@torch.no_grad()
def generate_images(dit, diffusion, vae, labels, cfg_scale=1.5, seed=0, sample_method="ddpm", eta=0.0):
    """The body of sample_ddp.py:136-163 in one call: labels [n] int64 on the GPU -> uint8 images [n,H,W,3].
    z ~ N(0, 1) from a generator seeded with `seed` on the model's device; with cfg_scale > 1 the batch is doubled with the null
    class (num_classes) and run through forward_with_cfg; p_sample_loop with clip_denoised=False; the null half is dropped;
    vae.decode(samples / 0.18215, is_image=True); frames.pixels_to_frames, this package's uint8 conversion (the script's own is
    clamp(255 x + 128, 0, 255) truncated: half a grey level above it).
    sample_method="ddim" (with a DDIMDiffusion from create_ddim_diffusion, else TypeError) runs ddim_sample_loop(eta=eta) instead:
    with eta == 0 the generator is consumed for z only, with eta > 0 for one more normal draw per step, in step order."""
    from .frames import pixels_to_frames
    _check_sample_method(diffusion, sample_method)
    if cfg_scale < 1.0:
        raise ValueError("In almost all cases, cfg_scale be >= 1.0")
    device = dit.device
    labels = labels.to(device=device, dtype=torch.int64)
    n = labels.shape[0]
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    z = torch.randn(n, dit.in_channels, dit.input_size, dit.input_size, device=device, generator=gen)
    using_cfg = cfg_scale > 1.0
    if using_cfg:
        z = torch.cat([z, z], 0)
        y = torch.cat([labels, torch.full((n,), dit.num_classes, device=device, dtype=torch.int64)], 0)
        model_kwargs, sample_fn = dict(y=y, cfg_scale=cfg_scale), dit.forward_with_cfg
    else:
        model_kwargs, sample_fn = dict(y=labels), dit.forward

    samples = _run_sampler(diffusion, sample_method, eta, sample_fn, z, model_kwargs, device, gen)
    if using_cfg:
        samples, _ = samples.chunk(2, dim=0)
    pixels = vae.decode((samples / 0.18215).contiguous(), is_image=True)
    return pixels_to_frames(pixels)


@torch.no_grad()
def generate_videos(latte, diffusion, vae, labels, cfg_scale=7.0, seed=0, sample_method="ddpm", eta=0.0):
    """The loop body of Diffusion/Latte/sample/sample_ddp.py:148-211 in one call: labels [n] int64 on the GPU (an int n, or None
    with n = 1, for a model without labels, extras == 1) -> uint8 videos [n,F_pixels,H,W,3].
    z ~ N(0, 1) of shape [n, latte.num_frames, in_channels, s, s] from a generator seeded with `seed` on the model's device; with
    cfg_scale > 1 the batch is doubled with the null class (num_classes: the script's literal 101 is UCF-101's) and run through
    forward_with_cfg; p_sample_loop with clip_denoised=False; the null half is dropped; the latents go channel-last
    ("b f c h w -> b f h w c", :202) into vae.decode(samples / 0.18215, is_image=False); frames.pixels_to_frames, which is the
    script's own uint8 conversion (:207).
    sample_method="ddim", eta: the scripts' --sample_method ddim (sample/sample.py:100-107), as in generate_images."""
    from .frames import pixels_to_frames
    _check_sample_method(diffusion, sample_method)
    if cfg_scale < 1.0:
        raise ValueError("In almost all cases, cfg_scale be >= 1.0")
    device = latte.device
    conditional = latte.extras == 2
    if conditional:
        if labels is None:
            raise ValueError("labels are required: the model has extras == 2")
        labels = labels.to(device=device, dtype=torch.int64)
        n = labels.shape[0]
    else:
        n = 1 if labels is None else (int(labels) if isinstance(labels, int) else labels.shape[0])
        labels = None
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    z = torch.randn(n, latte.num_frames, latte.in_channels, latte.input_size, latte.input_size, device=device, generator=gen)
    using_cfg = cfg_scale > 1.0
    if using_cfg:
        z = torch.cat([z, z], 0)
        y = torch.cat([labels, torch.full((n,), latte.num_classes, device=device, dtype=torch.int64)], 0) if conditional else None
        model_kwargs, sample_fn = dict(y=y, cfg_scale=cfg_scale), latte.forward_with_cfg
    else:
        model_kwargs, sample_fn = dict(y=labels), latte.forward

    samples = _run_sampler(diffusion, sample_method, eta, sample_fn, z, model_kwargs, device, gen)
    if using_cfg:
        samples, _ = samples.chunk(2, dim=0)
    pixels = vae.decode((samples / 0.18215).permute(0, 1, 3, 4, 2).contiguous(), is_image=False)
    return pixels_to_frames(pixels)
