#!/usr/bin/env python
"""One guided denoising step of Latte on the engine, and its temporal-attention kernel alone against the rearranging alternative.

    python tools/latte_bench.py --out profiles/latte_bench.json

Two shapes, seeded random weights, B = 2 (one video and its null-class twin), 256 tokens per frame:
  omnitokenizer   Latte-XL/2-omnitokenizer: 8 latent channels, F = 5 latent frames (17 pixel frames through the tokenizer's VAE)
  sd1.4           Latte-XL/2: 4 latent channels, F = 16
Reported per shape:
  step_ms         median of the timed steps after warm-up, device events around each; one step = forward_with_cfg + the p_sample
                  update over the B F frames
  --linear-format bf16 | fp16: the block linears of both kinds of block on the 16-bit MFMA (Latte.set_linear_format); step_ms is then
                  the 16-bit step and fp32_step_ms the default format's, timed first in the same session on the same model
  --attention-format bf16 | fp16: the spatial blocks' attention operands on the 16-bit MFMA (Latte.set_attention_format); step_ms is
                  then the step with that attention and fp32_attention_step_ms the same linear format's step with the fp32 attention,
                  timed just before it in the same session.  `split` then holds attention16 (omnitok_dit_attn16 over the B F frames,
                  writing what the engine has it write), attention_fp32 (omnitok_dit_attn at the same shape, same session) and, under
                  a 16-bit linear format, round16_attention with the calls it still has (the temporal blocks')
  temporal_attn   omnitok_latte_attn_temporal alone at the model's shape (qkv [B F N, 3 D] in (b f) n order): median ms per call
                  over batches of calls, and the achieved bytes/s against ONE read of qkv plus ONE write of out
  rearranged      what the kernel replaces: the copy '(b f) n d -> (b n) f d' of qkv, omnitok_dit_attn with N = F on it, and the copy
                  of its output back -- the three together and each alone -- with the max abs difference of the two results
  clock / power   the shader clock and board power sampled over the timed windows (tools/gpu_power.py)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "omnitokenizer": dict(model="Latte-XL/2-omnitokenizer", num_frames=5, in_channels=8),
    "sd1.4": dict(model="Latte-XL/2", num_frames=16, in_channels=4),
}


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def per_call(fn, calls, warmup, steps):
    """median / min / max ms of ONE call, from timed batches of `calls` back-to-back calls"""
    def batch():
        for _ in range(calls):
            fn()
    return [round(v / calls, 5) for v in timed(batch, warmup, steps)]


def bench_shape(name, spec, a, lib):
    from omnitokenizer_amd import _lib
    from omnitokenizer_amd.diffusion import create_diffusion
    from omnitokenizer_amd.latte import Latte_models
    P = ctypes.c_void_p
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    B, F, C = 2, spec["num_frames"], spec["in_channels"]
    m = Latte_models[spec["model"]](input_size=32, num_frames=F, num_classes=101, extras=2,
                                    **({} if "omnitokenizer" in spec["model"] else {"in_channels": C})).cuda().eval()
    for k, v in m.state_dict(keep_vars=True).items():  # every block contributes; the values do not change the time
        if k not in ("pos_embed", "temp_embed"):
            v.data.copy_(torch.randn(v.shape, device="cuda", generator=g) * 0.02)
    z = torch.randn(B // 2, F, C, 32, 32, device="cuda", generator=g)
    z = torch.cat([z, z])
    y = torch.tensor([7, 101], device="cuda")
    noise = torch.randn(B, F, C, 32, 32, device="cuda", generator=g)
    d = create_diffusion("250")
    t = torch.full((B,), 125, device="cuda", dtype=torch.int64)
    kw = dict(y=y, cfg_scale=7.0, check_range=False)

    def step():
        return d.p_sample(m.forward_with_cfg, z, t, clip_denoised=False, model_kwargs=kw, noise=noise)["sample"]

    with torch.no_grad():
        assert torch.isfinite(step()).all()
        m.check_range()
        step_ms = fp32_ms = timed(step, a.warmup, a.steps)
        if a.linear_format != "fp32":
            ref = step()
            m.set_linear_format(a.linear_format)
            diff16 = float((step() - ref).abs().max())
            m.check_range()
            step_ms = timed(step, a.warmup, a.steps)
        if a.attention_format != "fp32":
            ref, a32_ms = step(), step_ms
            m.set_attention_format(a.attention_format)
            diff_a16 = float((step() - ref).abs().max())
            m.check_range()
            step_ms = timed(step, a.warmup, a.steps)

    # ---- the temporal attention alone, and the rearranging alternative ------------------------------------------------------------
    D, heads, N = m.hidden_size, m.num_heads, (32 // m.patch_size) ** 2
    hd, rows = D // heads, B * F * N
    qkv = torch.randn(rows, 3 * D, device="cuda", generator=g)
    out = torch.empty(rows, D, device="cuda")
    qkv_t, out_t, out2 = torch.empty(rows, 3 * D, device="cuda"), torch.empty(rows, D, device="cuda"), torch.empty(rows, D, device="cuda")

    def strided():
        _lib.check(lib.omnitok_latte_attn_temporal(P(qkv.data_ptr()), B, F, N, heads, hd, P(out.data_ptr()), st))

    def copy_in():   # '(b f) n d -> (b n) f d'
        qkv_t.view(B, N, F, 3 * D).copy_(qkv.view(B, F, N, 3 * D).transpose(1, 2))

    def tiled():
        _lib.check(lib.omnitok_dit_attn(P(qkv_t.data_ptr()), B * N, F, heads, hd, P(out_t.data_ptr()), st))

    def copy_out():  # '(b n) f d -> (b f) n d'
        out2.view(B, F, N, D).copy_(out_t.view(B, N, F, D).transpose(1, 2))

    def rearranged():
        copy_in()
        tiled()
        copy_out()

    strided()
    rearranged()
    torch.cuda.synchronize()
    diff = float((out - out2).abs().max())
    calls = a.calls
    res_strided = per_call(strided, calls, 2, a.steps)
    res_re = per_call(rearranged, calls, 2, a.steps)
    parts = {k: per_call(f, calls, 2, a.steps)[0] for k, f in (("copy_in", copy_in), ("dit_attn_N_eq_F", tiled), ("copy_out", copy_out))}
    nbytes = rows * 4 * D * 4   # one read of qkv [rows, 3 D] + one write of out [rows, D], fp32
    extra = {} if a.linear_format == "fp32" else {
        "fp32_step_ms": round(fp32_ms[0], 4), "fp32_step_ms_min_max": [round(fp32_ms[1], 4), round(fp32_ms[2], 4)],
        "speedup_over_fp32_step": round(fp32_ms[0] / step_ms[0], 3), "max_abs_diff_to_fp32_step": diff16}
    if a.attention_format != "fp32":   # the spatial attention alone: B F sequences of N tokens, both kernels in this session
        codes = {"bf16": 1, "fp16": 2}
        lin16 = a.linear_format != "fp32"
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        a16 = torch.empty(rows, D, device="cuda", dtype=torch.int16)
        o32, o16, ofmt = (None, P(a16.data_ptr()), codes[a.linear_format]) if lin16 else (P(out.data_ptr()), None, 0)

        def spatial16():
            _lib.check(lib.omnitok_dit_attn16(P(qkv.data_ptr()), B * F, N, heads, hd, codes[a.attention_format], o32, o16, ofmt,
                                              P(flag.data_ptr()), st))

        def spatial32():
            _lib.check(lib.omnitok_dit_attn(P(qkv.data_ptr()), B * F, N, heads, hd, P(out.data_ptr()), st))

        def round16():
            _lib.check(lib.omnitok_dit_round16(P(out.data_ptr()), codes[a.linear_format], P(a16.data_ptr()), rows * D, P(flag.data_ptr()), st))

        r16, r32 = per_call(spatial16, calls, 2, a.steps), per_call(spatial32, calls, 2, a.steps)
        split = {"attention16": {"ms_per_call": r16[0], "ms_min_max": r16[1:], "calls_per_forward": m.depth // 2,
                                 "writes": "the packed operand of attn.proj" if lin16 else "fp32"},
                 "attention_fp32": {"ms_per_call": r32[0], "ms_min_max": r32[1:], "calls_per_forward": 0,
                                    "kernel": "omnitok_dit_attn at the same shape, same session"}}
        if lin16:
            rr = per_call(round16, calls, 2, a.steps)
            split["round16_attention"] = {"ms_per_call": rr[0], "ms_min_max": rr[1:], "calls_per_forward": m.depth // 2,
                                          "note": "behind the temporal attention only; the spatial blocks' pass is not launched"}
        extra.update({"split": split, "attention16_speedup_over_fp32_kernel": round(r32[0] / r16[0], 3),
                      "fp32_attention_step_ms": round(a32_ms[0], 4),
                      "fp32_attention_step_ms_min_max": [round(a32_ms[1], 4), round(a32_ms[2], 4)],
                      "speedup_over_fp32_attention_step": round(a32_ms[0] / step_ms[0], 3),
                      "max_abs_diff_to_fp32_attention_step": diff_a16})
    return {
        **extra, "linear_format": a.linear_format, "attention_format": a.attention_format,
        "model": spec["model"], "B": B, "frames": F, "tokens": N, "in_channels": C, "rows": rows, "hidden": D, "heads": heads,
        "head_dim": hd, "step_ms": round(step_ms[0], 4), "step_ms_min_max": [round(step_ms[1], 4), round(step_ms[2], 4)],
        "steps_timed": a.steps,
        "temporal_attn": {"ms_per_call": res_strided[0], "ms_min_max": res_strided[1:], "calls_per_forward": m.depth // 2,
                          "bytes_one_read_one_write": nbytes, "achieved_GBps": round(nbytes / (res_strided[0] * 1e-3) / 1e9, 1),
                          "sequences": B * N * heads},
        "rearranged": {"ms_per_call": res_re[0], "ms_min_max": res_re[1:], "parts_ms": parts,
                       "max_abs_diff_to_strided": diff},
        "strided_speedup_over_rearranged": round(res_re[0] / res_strided[0], 3),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="omnitokenizer,sd1.4")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50, help="kernel calls per timed batch")
    ap.add_argument("--linear-format", default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--attention-format", default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latte_bench needs the GPU: there is nothing to measure without it")
    from omnitokenizer_amd import _lib
    from tools import gpu_power
    lib = _lib.load()
    idle = gpu_power.snapshot()
    x = torch.randn(8192, 8192, device="cuda")
    for _ in range(20):
        x @ x
    busy = gpu_power.snapshot()
    torch.cuda.synchronize()
    del x
    files, hw = gpu_power.pick_hwmon(idle, busy, pci=gpu_power.pci_address(torch.cuda.current_device()))
    res = {"bench": "latte_step", "device": torch.cuda.get_device_name(0), "shapes": {},
           "arithmetic": "fp32" if a.linear_format == "fp32" else
           f"block linears {a.linear_format} operands on v_mfma_f32_32x32x16, fp32 accumulate; everything else fp32"}
    if a.attention_format != "fp32":
        res["arithmetic"] += (f"; spatial attention operands {a.attention_format} on v_mfma_f32_32x32x16, fp32 softmax and accumulate "
                              "(the temporal attention stays fp32)")
    for name in a.shapes.split(","):
        smp = gpu_power.Sampler(files) if files else None
        if smp:
            smp.start()
        res["shapes"][name] = bench_shape(name, SHAPES[name], a, lib)
        if smp:
            smp.stop()
            res["shapes"][name]["clock_power"] = smp.summary()
        torch.cuda.empty_cache()
    res["hwmon"] = hw if hw else "not readable: clock and power not measured"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
