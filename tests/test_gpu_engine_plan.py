"""GPU (-m gpu): the launch census of the engine -- WHICH data flow every block of an encode + decode took.

The e2e tests compare results with bars that every flow of the engine meets (plane GEMM, fp16 split, bf16x3, fp32 MFMA), so a
dispatch slip that sends a block down a fallback flow passes them, only slower and with other low bits.  Here every entry of a
matrix (fixture x engine mode, and the default mode with one data-flow option switched off) runs one encode and one decode with
the engine's timing on and compares timing_report() -- per kernel family the number of launches and the summed `work` the call
sites declare -- with tests/golden/engine_plans.json (tests/golden/make_golden_engine_plans.py).  `calls` must match exactly,
`work` to a relative 1e-6: the report prints it with %.6e, so that is the print precision, not a tolerance on arithmetic.
Times are ignored.
"""
import functools
import json
import os

import pytest
import torch

from tests.helpers import E2E_CASES, EXT_CASES, FULL_CASES, GOLDEN, HEAVY_CASES, VAE_CASES, VARIANT_CASES, GoldenCase
from tests.test_gpu_e2e import ENGINE_MODES

pytestmark = pytest.mark.gpu

PLANS = os.path.join(GOLDEN, "engine_plans.json")

# process options an entry may set, with the value every entry starts from and is left at ("pl_min_tokens" is pinned to 0 here
# whatever OMNITOK_TEST_PL_MIN_TOKENS says: the recorded plans are those of the default data flow)
DEFAULTS = dict(gemm_mode=2, attn_mode=1, gemm_pl=1, pl_min_tokens=0, qkv_pl=1, attn_window_mode=1, temporal_fused=1,
                attn_vpack=1, prevq_fuse=1, temporal_chunk=0)

SMALL = [c for c in E2E_CASES + VARIANT_CASES + HEAVY_CASES if "_r64_" in c or "_r128_" in c]
MODE_CASES = SMALL + FULL_CASES + [VAE_CASES[1], EXT_CASES[1]]
MODES = ENGINE_MODES + [(1, 1, 0)]
# the default mode with one option off: a small clip (8 x 8 grid), a 16 x 16 grid (the packed spatial q|k|v launch needs 256
# rows per clip), an image (single-token temporal blocks) and the two full-length clips (fused temporal stage, plane to_pixels)
OPTION_CASES = ["s2_sdpa_r64_vid", "s2_sdpa_r128_vid_16k", "s2_sdpa_r64_img"] + FULL_CASES
OPTIONS = [dict(qkv_pl=0), dict(attn_window_mode=0), dict(temporal_fused=0), dict(attn_vpack=0, gemm_pl=0), dict(prevq_fuse=0),
           dict(pl_min_tokens=1 << 30)]
# the chunked temporal branch needs chunk < B and 256-row clips; at T' = 5 the fused temporal stage comes first, so the
# full-length clip reaches it with that stage off
CHUNK_ENTRIES = [("s2_sdpa_r128_vid_16k", dict(temporal_chunk=1), 2), ("s2_sdpa_r256_vid17", dict(temporal_chunk=1), 2),
                 ("s2_sdpa_r256_vid17", dict(temporal_chunk=1, temporal_fused=0), 2)]


def entry_id(name, opts, clips):
    return name + "|" + ",".join(f"{k}={v}" for k, v in sorted(opts.items())) + (f"|x{clips}" if clips else "")


def matrix():
    """[(id, fixture, options, clips)]; clips > 0: the fixture's first clip repeated to that batch."""
    out = []
    for name in MODE_CASES:
        for gm, am, pl in MODES:
            out.append((name, dict(gemm_mode=gm, attn_mode=am, gemm_pl=pl), 0))
    for name in OPTION_CASES:
        for opts in OPTIONS:
            out.append((name, dict(opts), 0))
    out += CHUNK_ENTRIES
    return [(entry_id(*e),) + tuple(e) for e in out]


MATRIX = matrix()


@functools.lru_cache(maxsize=None)
def golden_case(name):
    return GoldenCase(name)


def build_model(case):
    from omnitokenizer_amd import OmniTokenizer_VQGAN
    m = OmniTokenizer_VQGAN(case.args, attention_mode=case.mode)
    missing = m.load_state_dict(case.sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.cuda().eval()


def run_entry(m, c, opts, clips):
    """One encode + one decode of fixture `c` on model `m` under the process options `opts`.  Returns (census, tensors):
    {family: {"calls", "work"}} of the two calls together, and what they returned."""
    from omnitokenizer_amd import _lib

    def rep(t):
        return t[:1].repeat(clips, *([1] * (t.dim() - 1))).contiguous() if clips else t
    x = rep(c.x).cuda()
    out = {}
    try:
        for k, v in {**DEFAULTS, **opts}.items():
            _lib.set_option(k, v)
        m.set_timing(True)
        m.timing_report()   # drop whatever an earlier call recorded
        if c.is_vae:
            z, mom = m.encode(x, c.is_image, noise=rep(c.noise), return_moments=True)
            out.update(z=z, moments=mom)
            out["recon"] = m.decode(rep(c.decode_input()).cuda(), c.is_image)
        else:
            ids, z = m.encode(x, c.is_image, return_latents=True)
            out.update(ids=ids, z=z)
            out["recon"] = m.decode(rep(c.ids).cuda(), c.is_image)
        report = m.timing_report()
    finally:
        m.set_timing(False)
        for k, v in DEFAULTS.items():
            _lib.set_option(k, v)
        _lib.set_option("pl_min_tokens", int(os.environ.get("OMNITOK_TEST_PL_MIN_TOKENS", "0")))  # tests/conftest.py
    census = {k: dict(calls=r["calls"], work=r["work"]) for k, r in sorted(report.items())}
    return census, {k: t.cpu() for k, t in out.items()}


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(case):
        key = (case.stage, case.mode, tuple(sorted(case.overrides.items())), case.profile)
        if key not in cache:
            cache[key] = build_model(case)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def plans():
    with open(PLANS) as f:
        return json.load(f)["plans"]


def test_matrix_and_recorded_plans_name_the_same_entries(plans):
    assert sorted(plans) == sorted(e[0] for e in MATRIX)


@pytest.mark.parametrize("eid,name,opts,clips", MATRIX, ids=[e[0] for e in MATRIX])
def test_launch_census_matches_the_recorded_plan(models, plans, eid, name, opts, clips):
    c = golden_case(name)
    census, out = run_entry(models(c), c, opts, clips)
    want = plans[eid]
    print(eid, {k: v["calls"] for k, v in census.items()})
    assert {k: v["calls"] for k, v in census.items()} == {k: v["calls"] for k, v in want.items()}, eid
    for k, v in census.items():
        assert abs(v["work"] - want[k]["work"]) <= 1e-6 * abs(want[k]["work"]), (eid, k, v["work"], want[k]["work"])
    assert all(torch.isfinite(t).all() for t in out.values() if t.is_floating_point())
