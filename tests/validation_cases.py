"""The val_*.npz fixtures (tests/golden/make_golden_validation.py): config, weights and inputs rebuilt from their seeds."""
import ast
import os
import zlib

import numpy as np
import torch

from omnitokenizer_amd import synth
from omnitokenizer_amd.config import OmniTokConfig, make_args

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VAL_CASES = ["val_s2_sdpa_r64_img_l1", "val_s2_sdpa_r64_vid_l1", "val_s2_sdpa_r64_vid_b2_l1", "val_s2_sdpa_r64_vid_mse",
             "val_s1_legacy_r64_vid", "val_vae_s2_sdpa_r64_vid", "val_genup2_r64_img", "val_ext_s2_sdpa_r64_img"]


class ValCase:
    def __init__(self, name):
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.g, self.name = g, name
        self.stage, self.mode = int(g["stage"]), str(g["mode"])
        self.overrides = ast.literal_eval(str(g["overrides"]))
        self.batch, self.frames = int(g["batch"]), int(g["frames"])
        self.is_image = self.frames == 1
        self.args = make_args(self.stage, **self.overrides)
        self.cfg = OmniTokConfig.from_args(self.args, attention_mode=self.mode)
        self.sd = synth.synth_state_dict(self.cfg, seed=int(g["weight_seed"]))
        assert synth.state_checksum(self.sd) == int(g["state_crc"]), "synthetic weight generator drifted from the fixtures"
        res, seed = self.cfg.resolution, int(g["input_seed"])
        self.x = synth.synth_image(self.batch, res, seed) if self.is_image else synth.synth_video(self.batch, self.frames, res, seed)
        assert zlib.crc32(self.x.numpy().tobytes()) == int(g["input_crc"]), "synthetic input drifted"
        self.lpips_sd = synth.synth_lpips_state_dict(int(g["lpips_seed"]))
        self.is_vae, self.is_ext = bool(self.args.use_vae), bool(self.args.use_external_codebook)
        self.l1_path = self.args.recon_loss_type == "l1"
        self.shift = 0.0 if self.l1_path else 0.5
        self.fp64_run = bool(int(g["fp64_run"]))
        self.frame_idx = torch.from_numpy(g["frame_idx"]) if "frame_idx" in g.files else None
        self.noise = torch.from_numpy(g["noise"]) if "noise" in g.files else None
        # the x the losses see: resized under gen_upscale
        self.x_seen = torch.from_numpy(g["x_resized"]) if "x_resized" in g.files else self.x
        self.x_recon32 = torch.from_numpy(g["x_recon32"])
        self.x_recon64 = self.x_recon32.double() + torch.from_numpy(g["x_recon64_resid"]).double()

    def wide(self, key):
        """fp64 tensor stored as fp32 value + fp32 residual"""
        return torch.from_numpy(self.g[key + "32"]).double() + torch.from_numpy(self.g[key + "64_resid"]).double()

    def scalar(self, key):
        return float(self.g[key])
