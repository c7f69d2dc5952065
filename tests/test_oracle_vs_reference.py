"""CPU: the oracle against the reference's own outputs on small cases, stored by tests/golden/make_golden.py (refcheck_*.npz);
also checks the synthetic state_dict covers exactly the reference's path keys, with the reference's shapes and dtypes."""
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import omnitok_oracle as orc
from oracle import c_oracle
from omnitokenizer_amd import synth
from omnitokenizer_amd.config import OmniTokConfig, make_args
from tests.helpers import GOLDEN


@pytest.mark.parametrize("stage,mode", [(2, "sdpa"), (1, "legacy")])
def test_live_reference_vs_oracle(stage, mode):
    g = np.load(os.path.join(GOLDEN, f"refcheck_s{stage}_{mode}_r64.npz"))
    args = make_args(stage, resolution=64)
    cfg = OmniTokConfig.from_args(args, attention_mode=mode)
    sd = synth.synth_state_dict(cfg, seed=int(g["weight_seed"]))
    assert synth.state_checksum(sd) == int(g["state_crc"]), "synthetic weights drifted from the golden fixture"
    keys = g["keys"].tolist()
    assert set(keys) == set(sd.keys())
    dims = iter(g["dims"].tolist())
    for k, nd, dt in zip(keys, g["ndims"].tolist(), g["dtypes"].tolist()):
        shape = tuple(next(dims) for _ in range(nd))
        assert tuple(sd[k].shape) == shape and str(sd[k].dtype) == dt, k
    x = synth.synth_video(1, 9, 64, seed=int(g["x_seed"]))
    assert zlib.crc32(x.contiguous().numpy().tobytes()) == int(g["x_crc"]), "synthetic input drifted from the golden fixture"
    ids_ref = torch.from_numpy(g["ids"].astype(np.int64))
    rec_ref = torch.from_numpy(g["recon"])
    with torch.no_grad():
        ids = orc.encode(sd, x, False, cfg)
        rec = orc.decode(sd, ids_ref, False, cfg)
    assert torch.equal(ids, ids_ref)
    assert (rec - rec_ref).abs().max().item() < 2e-5


def test_reference_codebook_vs_c_oracle_random():
    g = np.load(os.path.join(GOLDEN, "refcheck_codebook_8192.npz"))
    assert np.array_equal(c_oracle.vq_argmin(g["z"], g["codebook"]), g["ids"].astype(np.int64))
