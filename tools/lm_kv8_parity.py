#!/usr/bin/env python
"""What a bf16 and an fp8 K/V cache cost the logits, for users choosing the knob (profiles/lm_kv8_parity.json).  Not a test bar.

Per golden model (tests/golden/gpt_hd*.npz, synthetic weights): the fp32-cache engine samples up to 64 positions greedily after a
4-token prefix; the same 3 sequences are then teacher-forced, one decode step per position, through an fp32-cache, a bf16-cache
(GPT.set_cache_format) and an fp8-cache engine (GPT.set_cache_quant), all with fp32 weights.  Recorded per cache, over the sampled
positions: the largest |logit - fp32-cache logit|, the largest |logit| for scale, and how often the top-1 token and the top-5 set
agree with the fp32-cache engine's.
    python tools/lm_kv8_parity.py OUT.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from omnitokenizer_amd import gpt as og  # noqa: E402
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case  # noqa: E402


def make(sd, dims):
    V, BS, L, H, C = dims
    m = og.GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    m.load_state_dict({k: v for k, v in sd.items() if k != "vtokens_pos_emb"}, strict=True)
    return m.cuda().eval()


def stepped(m, seq):
    m.reset_streams(seq.shape[0], seq.shape[1] + 2)
    out = torch.stack([m.step(seq[:, t].contiguous()) for t in range(seq.shape[1])], 1)
    m.check_overflow()
    return out


def main():
    out_path = sys.argv[1]
    rec = []
    for name in GPT_CASES:
        g, sd, dims = load_gpt_case(name)
        V, BS, L, H, C = dims
        n = min(64, BS - 4 - 1)
        x = torch.from_numpy(g["idx"])[:3, :4].cuda()
        m32 = make(sd, dims)
        new = og.sample_with_past(x, m32, n, sample_logits=False)
        seq = torch.cat([x, new], 1)[:, :4 + n]
        ref = stepped(m32, seq)[:, 3:3 + n]          # the logits that chose the n sampled tokens
        row = {"model": name, "n_layer": L, "n_head": H, "head_dim": C // H, "positions": n, "streams": 3,
               "max_abs_logit": round(float(ref.abs().max()), 4)}
        for arm, m in (("bf16", make(sd, dims).set_cache_format("bf16")), ("fp8", make(sd, dims).set_cache_quant("fp8"))):
            lg = stepped(m, seq)[:, 3:3 + n]
            t5a, t5b = lg.topk(5, -1).indices.sort(-1).values, ref.topk(5, -1).indices.sort(-1).values
            row[arm] = {"max_logit_diff": float(f"{float((lg - ref).abs().max()):.4e}"),
                        "top1_agreement": round(float((lg.argmax(-1) == ref.argmax(-1)).float().mean()), 4),
                        "top5_set_agreement": round(float((t5a == t5b).all(-1).float().mean()), 4)}
        rec.append(row)
        print(json.dumps(row), flush=True)
    with open(out_path, "w") as f:
        json.dump({"what": "logits of a bf16 / fp8 K/V cache against the fp32-cache engine, fp32 weights, teacher-forced decode steps "
                           "over greedily sampled positions (tools/lm_kv8_parity.py)", "device": torch.cuda.get_device_name(0),
                   "models": rec}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
