"""GPU (-m gpu): the batched prefill resolves the engine's switches (weight format, prefill format, prefill attention, attention
operands) once per call, so a switch flipped between two prefills on ONE engine must give the bits of a fresh engine built with that
switch: no stage may keep the form, the workspace layout or a flag of the call before.  Bitwise (torch.equal), so no tolerance."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

# hd 64; B x T crosses a 256-key chunk of the rows mode, a 128-query block and a 32-key tile of the tiled mode, with a ragged tail
V, BS, L, H, C = 512, 320, 2, 4, 256
B, T = 2, 300

# (weight format, prefill format, attention, operands): every stop changes what at least one stage of the layer loop launches
WALK = [("fp32", "fp32", "rows", "fp32"),
        ("fp32", "fp32", "tiled", "fp32"),
        ("fp32", "fp32", "tiled", "bf16"),
        ("fp32", "fp32", "rows", "fp32"),
        ("bf16", "w16", "tiled", "fp16")]


def _new_gpt(sd):
    from omnitokenizer_amd.gpt import GPT
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.cuda().eval()


def _state_dict():
    from omnitokenizer_amd.gpt import GPT
    g = torch.Generator().manual_seed(5)
    sd = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C).state_dict()
    out = {}
    for k, t in sd.items():
        r = torch.randn(t.shape, generator=g)
        ln_gain = k.endswith("weight") and (".ln" in k or k.startswith("ln_f"))
        out[k] = 1.0 + 0.1 * r if ln_gain else 0.05 * r
    return out


def _apply(m, stop):
    wfmt, pfmt, attn, aop = stop
    return m.set_weight_format(wfmt).set_prefill_format(pfmt).set_prefill_attention(attn).set_prefill_attention_operands(aop)


def _run(m, idx, nxt):
    """prefill logits [B, T, V] and the logits of one decode step after it"""
    m.reset_streams(B, T + 1)
    pre = m.prefill(idx, want_logits=True)
    step = m.step(nxt)
    m.check_overflow()
    return pre.clone(), step.clone()


def test_a_switch_flipped_on_one_engine_gives_a_fresh_engines_bits():
    sd = _state_dict()
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(0, V, (B, T), generator=g).cuda()
    nxt = torch.randint(0, V, (B,), generator=g).cuda()
    walker = _new_gpt(sd)
    seen = []
    for stop in WALK:
        pre, step = _run(_apply(walker, stop), idx, nxt)
        fresh_pre, fresh_step = _run(_apply(_new_gpt(sd), stop), idx, nxt)
        assert torch.isfinite(pre).all() and torch.isfinite(step).all(), stop
        assert torch.equal(pre, fresh_pre), stop
        assert torch.equal(step, fresh_step), stop
        seen.append((stop, pre))
    # every switch of the walk is live: the stops differ from each other wherever their settings do
    for i, (si, pi) in enumerate(seen):
        for sj, pj in seen[i + 1:]:
            assert torch.equal(pi, pj) == (si == sj), (si, sj)

    # the two refused combinations, with the engine's messages, on the engine that just ran the last stop
    _apply(walker, ("bf16", "w16", "rows", "fp16"))
    walker.reset_streams(B, T + 1)
    with pytest.raises(RuntimeError) as ei:
        walker.prefill(idx, want_logits=True)
    assert ("lm_prefill: 16-bit attention operands (omnitok_lm_set_prefill_attention_operands) need the tiled attention: set "
            "omnitok_lm_set_prefill_attention to OMNITOK_LM_PA_TILED (it is OMNITOK_LM_PA_ROWS), or the operands back to "
            "OMNITOK_LM_AOP_FP32") in str(ei.value)
    _apply(walker, ("fp32", "w16", "tiled", "fp32"))
    walker.reset_streams(B, T + 1)
    with pytest.raises(RuntimeError) as ei:
        walker.prefill(idx, want_logits=True)
    assert ("lm_prefill: prefill format OMNITOK_LM_PF_W16 (omnitok_lm_set_prefill_format) needs the packed 16-bit weight images: "
            "set omnitok_lm_set_weight_format to OMNITOK_LM_W_BF16 or OMNITOK_LM_W_FP16 (it is OMNITOK_LM_W_FP32), or the prefill "
            "format back to OMNITOK_LM_PF_FP32") in str(ei.value)
    # ... and the engine runs on once the combination is legal again
    pre, step = _run(_apply(walker, WALK[0]), idx, nxt)
    assert torch.equal(pre, seen[0][1])
