"""Generates tests/golden/dit_*.npz from the reference's own code (Diffusion/DiT/models.py and its diffusion package), in fp64.

    python tests/golden/make_golden_dit.py /path/to/OmniTokenizer-reference

Run once where the reference tree exists; the fixtures hold DATA only (inputs, the reference's outputs, its tables) and the tests
read nothing else.  The reference's models.py imports PatchEmbed, Attention and Mlp from timm, which this tree does not depend on:
a stand-in module with these three classes (a few lines each, written here after timm's documented behaviour) is placed in
sys.modules before the import.  Weights are NOT stored: tests/dit_ref.py make_weights regenerates them from the seed on both sides.

  dit_model_{a,b}.npz  x, t, y; forward and forward_with_cfg of the reference in fp64 (model.double()); cpu_fp32_err_*: the
                       max-abs error of tests/dit_ref.py run in fp32 by torch on the CPU against the same fp64 outputs -- the
                       yardstick of the GPU's error bar (4 x)
  dit_tables.npz       per respacing "250", "50", "10,15,20": timestep_map and the fp64 tables of the respaced process; the
                       reference's pos_embed for (128, grid 6)
  dit_loop.npz         a 10-step p_sample_loop trajectory in fp64 with the closed-form toy model of dit_ref.py and recorded
                       step noise, clip_denoised on and off, with the fp32-on-CPU error of dit_ref.p_sample over the same steps
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import dit_ref  # noqa: E402

CFG_SCALE = 4.0
LOOP_SHAPE = (3, 4, 5, 5)
LOOP_RESPACING = "10"


def timm_stand_in():
    class PatchEmbed(nn.Module):
        def __init__(self, img_size, patch_size, in_chans, embed_dim, bias=True):
            super().__init__()
            self.patch_size = (patch_size, patch_size)
            self.num_patches = (img_size // patch_size) ** 2
            self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size, bias=bias)

        def forward(self, x):
            return self.proj(x).flatten(2).transpose(1, 2)

    class Attention(nn.Module):
        def __init__(self, dim, num_heads=8, qkv_bias=False, **kw):
            super().__init__()
            self.num_heads = num_heads
            self.scale = (dim // num_heads) ** -0.5
            self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
            self.proj = nn.Linear(dim, dim)

        def forward(self, x):
            B, N, C = x.shape
            qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
            q, k, v = qkv.unbind(0)
            attn = ((q * self.scale) @ k.transpose(-2, -1)).softmax(dim=-1)
            return self.proj((attn @ v).transpose(1, 2).reshape(B, N, C))

    class Mlp(nn.Module):
        def __init__(self, in_features, hidden_features=None, act_layer=nn.GELU, drop=0.0):
            super().__init__()
            self.fc1 = nn.Linear(in_features, hidden_features)
            self.act = act_layer()
            self.fc2 = nn.Linear(hidden_features, in_features)

        def forward(self, x):
            return self.fc2(self.act(self.fc1(x)))

    vt = types.ModuleType("timm.models.vision_transformer")
    vt.PatchEmbed, vt.Attention, vt.Mlp = PatchEmbed, Attention, Mlp
    timm, models = types.ModuleType("timm"), types.ModuleType("timm.models")
    timm.models, models.vision_transformer = models, vt
    sys.modules.update({"timm": timm, "timm.models": models, "timm.models.vision_transformer": vt})


def main(ref_root):
    timm_stand_in()
    sys.path.insert(0, os.path.join(ref_root, "Diffusion", "DiT"))
    import models as ref_models
    from diffusion import create_diffusion as ref_create_diffusion

    # ---- the two models --------------------------------------------------------------------------------------------------------
    for name, cfg in dit_ref.MODELS.items():
        w32 = dit_ref.make_weights(cfg, dit_ref.SEEDS[name])
        model = ref_models.DiT(**cfg)
        missing = model.load_state_dict(w32, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        model = model.double().eval()
        # the embedding is fp32 in the reference whatever the model's dtype (models.py:52-56); its MLP then needs the model's dtype
        emb = model.t_embedder.timestep_embedding
        model.t_embedder.timestep_embedding = lambda t, dim, _e=emb: _e(t, dim).double()
        x, t, y = (torch.from_numpy(v) for v in dit_ref.make_inputs(name))
        with torch.no_grad():
            fwd = model.forward(x.double(), t, y)
            cfgo = model.forward_with_cfg(x.double(), t, y, CFG_SCALE)
            f32 = dit_ref.forward(w32, cfg, x, t, y)
            c32 = dit_ref.forward_with_cfg(w32, cfg, x, t, y, CFG_SCALE)
        out = dict(x=x.numpy(), t=t.numpy(), y=y.numpy(), cfg_scale=np.float64(CFG_SCALE), forward=fwd.numpy(),
                   forward_with_cfg=cfgo.numpy(), cpu_fp32_err_forward=np.float64((f32.double() - fwd).abs().max()),
                   cpu_fp32_err_forward_with_cfg=np.float64((c32.double() - cfgo).abs().max()))
        np.savez_compressed(os.path.join(HERE, f"dit_model_{name}.npz"), **out)
        print(name, "max|out|", float(fwd.abs().max()), "cpu fp32 err", out["cpu_fp32_err_forward"], out["cpu_fp32_err_forward_with_cfg"])

    # ---- the respaced tables ---------------------------------------------------------------------------------------------------
    tables = {}
    names = ("betas", "alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
             "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")
    for key, resp in (("250", "250"), ("50", "50"), ("s10_15_20", "10,15,20")):
        d = ref_create_diffusion(resp)
        tables[f"{key}/timestep_map"] = np.asarray(d.timestep_map, dtype=np.int64)
        for n in names:
            tables[f"{key}/{n}"] = np.asarray(getattr(d, n), dtype=np.float64)
    tables["pos_embed_128_6"] = ref_models.get_2d_sincos_pos_embed(128, 6)
    np.savez_compressed(os.path.join(HERE, "dit_tables.npz"), **tables)

    # ---- the sampling loop -----------------------------------------------------------------------------------------------------
    from omnitokenizer_amd.diffusion import create_diffusion
    d = ref_create_diffusion(LOOP_RESPACING)
    ours = create_diffusion(LOOP_RESPACING).coefficient_table()
    rng = np.random.default_rng(77)
    x0 = rng.normal(size=LOOP_SHAPE)
    noise = rng.normal(size=(d.num_timesteps, *LOOP_SHAPE))
    loop = dict(x0=x0, step_noise=noise, respacing=np.array(LOOP_RESPACING))
    for clip in (True, False):
        draws = iter(torch.from_numpy(noise))
        orig = torch.randn_like
        torch.randn_like = lambda x: next(draws).to(x.dtype)  # the reference draws its step noise here (gaussian_diffusion.py:410)
        try:
            traj = [o["sample"].numpy() for o in d.p_sample_loop_progressive(
                dit_ref.toy_model, LOOP_SHAPE, noise=torch.from_numpy(x0), clip_denoised=clip, device="cpu")]
        finally:
            torch.randn_like = orig
        traj = np.stack(traj)
        # the same loop in fp32 on the CPU through dit_ref.p_sample: the yardstick of the GPU's error
        x = torch.from_numpy(x0).float()
        err = 0.0
        for k, i in enumerate(range(d.num_timesteps - 1, -1, -1)):
            tt = torch.full((LOOP_SHAPE[0],), d.timestep_map[i], dtype=torch.int64)
            x, _ = dit_ref.p_sample(ours[i], dit_ref.toy_model(x, tt), x, torch.from_numpy(noise[k]).float(), True, clip)
            err = max(err, float((x.double() - torch.from_numpy(traj[k])).abs().max()))
        tag = "clip" if clip else "noclip"
        loop[f"trajectory_{tag}"] = traj
        loop[f"cpu_fp32_err_{tag}"] = np.float64(err)
        print("loop", tag, "max|x|", float(np.abs(traj).max()), "cpu fp32 err", err)
    np.savez_compressed(os.path.join(HERE, "dit_loop.npz"), **loop)


if __name__ == "__main__":
    main(sys.argv[1])
