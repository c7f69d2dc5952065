"""TEST HELPER: what a PF_W16 prefill (omnitok_lm_set_prefill_format) computes, restated on the CPU in fp32 or fp64.

It is the oracle's forward (oracle/gpt_oracle.py: forward / block / attention) with two changes: the weights are `rounded(sd, fmt)`
(the five matrix families of a 16-bit engine), and the input of every nn.Linear -- ln1's rows, the merged attention output, ln2's
rows, FC1's GELU output and ln_f's rows -- passes through .to(fmt) first: one rounding to nearest even, torch's bits.  Everything
else (embedding, residual stream, LayerNorm statistics, softmax, biases) stays in the working dtype `dt`.
"""
import math

import torch
import torch.nn.functional as F

FMT = {"bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
MATRICES = (".attn.key.weight", ".attn.query.weight", ".attn.value.weight", ".attn.proj.weight", ".mlp.0.weight", ".mlp.2.weight")


def rounded(sd, fmt):
    dt = FMT[fmt][1]
    return {k: (v.to(dt).float() if k == "head.weight" or k.endswith(MATRICES) else v) for k, v in sd.items()}


def forward(sd, idx, n_head, fmt, dt=torch.float64):
    """sd: fp32 state_dict (unrounded).  Returns (logits [B, T, V], k0, v0 [B, n_head, T, head_dim] of layer 0), all in dt."""
    f16 = FMT[fmt][1]
    sd = {k: v.to(dt) for k, v in rounded(sd, fmt).items()}

    def rnd(t):
        return t.to(f16).to(dt)

    x = F.embedding(idx, sd["tok_emb.weight"])
    B, T, C = x.shape
    x = x + sd["pos_emb"][:, :T]
    hs = C // n_head
    n_layer = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool))
    k0 = v0 = None
    for i in range(n_layer):
        p = f"blocks.{i}"
        h = rnd(F.layer_norm(x, (C,), sd[f"{p}.ln1.weight"], sd[f"{p}.ln1.bias"]))
        k = F.linear(h, sd[f"{p}.attn.key.weight"], sd[f"{p}.attn.key.bias"]).view(B, T, n_head, hs).transpose(1, 2)
        q = F.linear(h, sd[f"{p}.attn.query.weight"], sd[f"{p}.attn.query.bias"]).view(B, T, n_head, hs).transpose(1, 2)
        v = F.linear(h, sd[f"{p}.attn.value.weight"], sd[f"{p}.attn.value.bias"]).view(B, T, n_head, hs).transpose(1, 2)
        if i == 0:
            k0, v0 = k, v
        att = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(hs))
        att = att.masked_fill(~mask, float("-inf"))
        y = (F.softmax(att, dim=-1) @ v).transpose(1, 2).contiguous().view(B, T, C)
        x = x + F.linear(rnd(y), sd[f"{p}.attn.proj.weight"], sd[f"{p}.attn.proj.bias"])
        h = rnd(F.layer_norm(x, (C,), sd[f"{p}.ln2.weight"], sd[f"{p}.ln2.bias"]))
        h = rnd(F.gelu(F.linear(h, sd[f"{p}.mlp.0.weight"], sd[f"{p}.mlp.0.bias"])))
        x = x + F.linear(h, sd[f"{p}.mlp.2.weight"], sd[f"{p}.mlp.2.bias"])
    x = rnd(F.layer_norm(x, (C,), sd["ln_f.weight"], sd["ln_f.bias"]))
    return F.linear(x, sd["head.weight"]), k0, v0


def reference(sd, idx, n_head, fmt):
    """(logits64, k0_64, v0_64, d_ref): the fp64 restatement and d_ref = max |restatement in fp32 - restatement in fp64| over the
    logits -- the reference's own sensitivity to last-bit differences upstream of the discontinuous 16-bit roundings."""
    l64, k64, v64 = forward(sd, idx, n_head, fmt, torch.float64)
    l32, _, _ = forward(sd, idx, n_head, fmt, torch.float32)
    return l64, k64, v64, float((l32.double() - l64).abs().max())
