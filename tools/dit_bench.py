#!/usr/bin/env python
"""One denoising step of DiT-XL/2 on the engine against the fp32 PyTorch restatement on the same GPU, in the same session.

    python tools/dit_bench.py --out profiles/dit_bench.json

The workload: DiT-XL/2 at input_size 32, 8 latent channels (the --use_vae tokenizer's), seeded random weights, 8 images with
classifier-free guidance = 16 streams x 256 tokens = 4096 rows; one step = forward_with_cfg + the p_sample update.  Reported:
  step_ms            median of >= 20 steps after warm-up, device events around each step
  torch_step_ms      the same step through tests/dit_ref.py in fp32 by torch on this GPU (what a user would otherwise run)
  split              each operator alone at the model's shapes through its stand-alone entry point, x its calls per forward; their sum
                     is not the step (no launch gaps, warm caches): it says where the time goes
  --linear-format    bf16 | fp16: the block linears on the 16-bit MFMA (DiT.set_linear_format).  step_ms is then the 16-bit step and
                     fp32_step_ms the default format's, timed first in the same session; the split times omnitok_dit_gemm16 per
                     epilogue and the producers of its packed operands, and block_gemms is held against the 16-bit MFMA peak
  --attention-format bf16 | fp16: the attention's operands on the 16-bit MFMA (DiT.set_attention_format).  step_ms is then the step
                     with that attention and fp32_attention_step_ms the same linear format's step with the fp32 attention, timed just
                     before it in the same session; the split times omnitok_dit_attn16 (`attention16`, writing what the engine has it
                     write: the packed operand of attn.proj under a 16-bit linear format, which drops `round16_attention`), and
                     attention_fp32 holds omnitok_dit_attn's time in the same session
  attention          the attention kernel's useful FLOP (4 B heads N^2 hd: both products, the dead 3/4 of head_dim 72's third output
                     block not counted) over its time, as a fraction of the fp32-input MFMA peak
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

PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_16BIT_MFMA_TFLOPS = 2500.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="DiT-XL/2")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--torch-steps", type=int, default=20)
    ap.add_argument("--linear-format", default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--attention-format", default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lin16 = a.linear_format != "fp32"
    attn16 = a.attention_format != "fp32"
    if not torch.cuda.is_available():
        raise SystemExit("dit_bench needs the GPU: there is nothing to measure without it")
    from omnitokenizer_amd import _lib
    from omnitokenizer_amd.dit import DiT_models
    from omnitokenizer_amd.diffusion import create_diffusion
    from tests import dit_ref

    m = DiT_models[a.model](input_size=32, in_channels=8, num_classes=1000)
    cfg = dict(input_size=32, patch_size=m.patch_size, in_channels=8, hidden_size=m.hidden_size, depth=m.depth,
               num_heads=m.num_heads, mlp_ratio=4.0, class_dropout_prob=0.1, num_classes=1000, learn_sigma=True)
    w = dit_ref.make_weights(cfg, 1)
    m.load_state_dict(w, strict=True)
    m = m.cuda().eval()
    wd = {k: v.cuda() for k, v in w.items()}
    n = a.images
    B = 2 * n
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    z = torch.randn(n, 8, 32, 32, device="cuda", generator=g)
    z = torch.cat([z, z])
    y = torch.cat([torch.arange(n, device="cuda") % 1000, torch.full((n,), 1000, device="cuda")])
    noise = torch.randn(B, 8, 32, 32, device="cuda", generator=g)
    d = create_diffusion("250")
    t = torch.full((B,), 125, device="cuda", dtype=torch.int64)
    kw = dict(y=y, cfg_scale=4.0, check_range=False)

    def engine_step():
        return d.p_sample(m.forward_with_cfg, z, t, clip_denoised=False, model_kwargs=kw, noise=noise)["sample"]

    coef = d.coefficient_table()[125]
    tmap = torch.tensor(d.timestep_map, device="cuda")

    def torch_step():
        out = dit_ref.forward_with_cfg(wd, cfg, z, tmap[t], y, 4.0)
        return dit_ref.p_sample(coef, out, z, noise, True, False)[0]

    with torch.no_grad():
        ours, ref = engine_step(), torch_step()
        diff = float((ours - ref).abs().max())
        step = fp32_step = timed(engine_step, a.warmup, a.steps)
        if lin16:
            m.set_linear_format(a.linear_format)
            diff16 = float((engine_step() - ours).abs().max())
            step = timed(engine_step, a.warmup, a.steps)
        if attn16:
            before, a32_step = engine_step(), step
            m.set_attention_format(a.attention_format)
            diff_a16 = float((engine_step() - before).abs().max())
            step = timed(engine_step, a.warmup, a.steps)
        tstep = timed(torch_step, a.warmup, a.torch_steps)

    # ---- the split: each operator alone at the model's shapes -------------------------------------------------------------------
    lib = _lib.load()
    P = ctypes.c_void_p
    st = torch.cuda.current_stream().cuda_stream
    D, F, N, H, hd, L = m.hidden_size, m.mlp_hidden, (32 // m.patch_size) ** 2, m.num_heads, m.hidden_size // m.num_heads, m.depth
    M = B * N
    modN = L * 6 * D + 2 * D
    PC = m.patch_size ** 2 * 16
    buf = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    X, Y, QKV, H1, mod = buf(M, D), buf(M, D), buf(M, 3 * D), buf(M, F), buf(B, modN) * 0.1
    O, O3, OF, OL = torch.empty(M, D, device="cuda"), torch.empty(M, 3 * D, device="cuda"), torch.empty(M, F, device="cuda"), \
        torch.empty(M, PC, device="cuda")
    Wqkv, Wp, W1, W2, Wf, bias = buf(3 * D, D), buf(D, D), buf(F, D), buf(D, F), buf(PC, D), buf(max(3 * D, F, modN))  # the widest N

    def gemm(A, W, C, Mr, Nc, K):
        assert A.numel() >= Mr * K and W.numel() == Nc * K and C.numel() == Mr * Nc and bias.numel() >= Nc, "operand smaller than the GEMM"
        desc = _lib.OmnitokRowGemm(a=A.data_ptr(), lda=K, w=W.data_ptr(), ldw=K, bias=bias.data_ptr(), c=C.data_ptr(), ldc=Nc, M=Mr,
                                   N=Nc, K=K, flags=1)
        return lambda: _lib.check(lib.omnitok_gemm(ctypes.byref(desc), st))

    xin, wpe, pos = buf(B, 8, 32, 32), buf(D, 8, m.patch_size, m.patch_size), buf(N, D)
    img = torch.empty(B, 16, 32, 32, device="cuda")
    ops = {
        "patch_embed": (1, lambda: lib.omnitok_dit_patch_embed(P(xin.data_ptr()), B, P(wpe.data_ptr()), P(bias.data_ptr()), P(pos.data_ptr()),
                                                               B, 8, 32, m.patch_size, D, P(O.data_ptr()), st)),
        "ln_modulate": (2 * L + 1, lambda: lib.omnitok_dit_ln_modulate(P(X.data_ptr()), P(mod.data_ptr()), P(mod.data_ptr() + 4 * D), modN,
                                                                       M, N, D, P(O.data_ptr()), st)),
        "gemm_qkv": (L, gemm(X, Wqkv, O3, M, 3 * D, D)),
        "attention": (L, lambda: lib.omnitok_dit_attn(P(QKV.data_ptr()), B, N, H, hd, P(O.data_ptr()), st)),
        "gemm_proj": (L, gemm(X, Wp, O, M, D, D)),
        "gate_residual": (2 * L, lambda: lib.omnitok_dit_gate_residual(P(Y.data_ptr()), P(X.data_ptr()), P(mod.data_ptr()), modN, M, N, D, st)),
        "gemm_fc1": (L, gemm(X, W1, OF, M, F, D)),
        "gelu_tanh": (L, lambda: lib.omnitok_dit_gelu_tanh(P(H1.data_ptr()), M * F, st)),
        "gemm_fc2": (L, gemm(H1, W2, O, M, D, F)),
        "gemm_modulation": (1, gemm(X, buf(modN, D), torch.empty(B, modN, device="cuda"), B, modN, D)),
        "gemm_final": (1, gemm(X, Wf, OL, M, PC, D)),
        "unpatchify": (1, lambda: lib.omnitok_dit_unpatchify(P(OL.data_ptr()), B, N, m.patch_size, 16, P(img.data_ptr()), st)),
    }
    if lin16:  # the block's four GEMMs with their epilogues, and the passes that round their A operands
        code, dt = {"bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}[a.linear_format]
        X16, H16, O16 = (buf(M, D) * 0.5).to(dt), (buf(M, F) * 0.5).to(dt), torch.empty(M, F, device="cuda", dtype=dt)
        W16 = {k: (v * 0.02).to(dt) for k, v in (("qkv", Wqkv), ("proj", Wp), ("fc1", W1), ("fc2", W2))}
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        gate = P(mod.data_ptr() + 8 * D)

        def gemm16(A, W, epi, y32, y16, Nc, K):
            gated = epi == 2
            return lambda: _lib.check(lib.omnitok_dit_gemm16(P(A.data_ptr()), P(W.data_ptr()), code, P(bias.data_ptr()), epi, y32, y16,
                                                             gate if gated else None, modN if gated else 0, N if gated else 0,
                                                             P(Y.data_ptr()) if gated else None, M, Nc, K, P(flag.data_ptr()), st))

        for k in ("gemm_qkv", "gemm_proj", "gate_residual", "gemm_fc1", "gelu_tanh", "gemm_fc2"):
            del ops[k]
        ops.update({
            "ln_modulate16": (2 * L, lambda: lib.omnitok_dit_ln_modulate16(P(X.data_ptr()), P(mod.data_ptr()), P(mod.data_ptr() + 4 * D), modN,
                                                                           M, N, D, code, P(O16.data_ptr()), P(flag.data_ptr()), st)),
            "round16_attention": (L, lambda: lib.omnitok_dit_round16(P(X.data_ptr()), code, P(O16.data_ptr()), M * D, P(flag.data_ptr()), st)),
            "gemm16_qkv_bias": (L, gemm16(X16, W16["qkv"], 0, P(O3.data_ptr()), None, 3 * D, D)),
            "gemm16_proj_gate_residual": (L, gemm16(X16, W16["proj"], 2, None, None, D, D)),
            "gemm16_fc1_gelu16": (L, gemm16(X16, W16["fc1"], 1, None, P(O16.data_ptr()), F, D)),
            "gemm16_fc2_gate_residual": (L, gemm16(H16, W16["fc2"], 2, None, None, D, F)),
        })
        ops["ln_modulate"] = (1, ops["ln_modulate"][1])  # the final layer's
    if attn16:  # what the engine launches: into the packed A16 under a 16-bit linear format (no round pass), else fp32
        acode = {"bf16": 1, "fp16": 2}[a.attention_format]
        aflag = torch.zeros(1, dtype=torch.int32, device="cuda")
        A16 = torch.empty(M, D, device="cuda", dtype=torch.int16)
        o32, o16, ofmt = (None, P(A16.data_ptr()), {"bf16": 1, "fp16": 2}[a.linear_format]) if lin16 else (P(O.data_ptr()), None, 0)
        attn_fp32 = ops.pop("attention")[1]
        ops.pop("round16_attention", None)
        ops["attention16"] = (L, lambda: lib.omnitok_dit_attn16(P(QKV.data_ptr()), B, N, H, hd, acode, o32, o16, ofmt, P(aflag.data_ptr()),
                                                                st))
        ops["attention_fp32"] = (0, attn_fp32)  # not part of this forward: the yardstick, timed in the same session
    split = {}
    for name, (calls, fn) in ops.items():
        def rep(fn=fn):
            for _ in range(10):
                fn()
        print("split:", name, file=sys.stderr, flush=True)
        med, _, _ = timed(rep, 2, 10)
        split[name] = {"ms_per_call": round(med / 10, 5), "calls_per_forward": calls, "ms_per_forward": round(med / 10 * calls, 4)}
    attn_ms = split["attention16" if attn16 else "attention"]["ms_per_call"]
    attn_flop = 4.0 * B * H * N * N * hd
    gemm_flop = 2.0 * M * D * (3 * D + D + 2 * F) * L
    gemm_ms = sum(v["ms_per_forward"] for k, v in split.items() if k.startswith("gemm16_" if lin16 else ("gemm_qkv", "gemm_proj", "gemm_fc")))
    peak = PEAK_16BIT_MFMA_TFLOPS if lin16 else PEAK_F32_MFMA_TFLOPS
    tiles = {k: ((M + 127) // 128) * ((nc + 127) // 128) for k, nc in (("qkv", 3 * D), ("proj", D), ("fc1", F), ("fc2", D))}
    res = {
        "bench": "dit_step", "model": a.model, "input_size": 32, "in_channels": 8, "images": n, "streams": B, "rows": M,
        "device": torch.cuda.get_device_name(0), "linear_format": a.linear_format, "attention_format": a.attention_format,
        "arithmetic": (f"block linears {a.linear_format} operands on v_mfma_f32_32x32x16, fp32 accumulate; everything else fp32" if lin16
                       else "fp32 (v_mfma_f32_32x32x2_f32 GEMMs and attention)"),
        "step_ms": round(step[0], 4), "step_ms_min_max": [round(step[1], 4), round(step[2], 4)], "steps_timed": a.steps,
        "torch_step_ms": round(tstep[0], 4), "torch_step_ms_min_max": [round(tstep[1], 4), round(tstep[2], 4)],
        "torch_baseline": "tests/dit_ref.py forward_with_cfg + p_sample in fp32 through torch on the same GPU, same session "
                          f"(allow_tf32 {torch.backends.cuda.matmul.allow_tf32})",
        "speedup_over_torch": round(tstep[0] / step[0], 3), "max_abs_diff_to_torch_step": diff,
        "split": split, "split_sum_ms": round(sum(v["ms_per_forward"] for v in split.values()), 4),
        "attention": {"useful_flop": attn_flop, "tflops": round(attn_flop / (attn_ms * 1e-3) / 1e12, 2),
                      "frac_of_f32_mfma_peak": round(attn_flop / (attn_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)},
        "block_gemms": {"flop": gemm_flop, "ms_per_forward": round(gemm_ms, 4), "tflops": round(gemm_flop / (gemm_ms * 1e-3) / 1e12, 2),
                        ("frac_of_16bit_mfma_peak" if lin16 else "frac_of_f32_mfma_peak"): round(gemm_flop / (gemm_ms * 1e-3) / 1e12 / peak, 4)},
        "peak_f32_mfma_tflops": PEAK_F32_MFMA_TFLOPS,
    }
    if lin16:
        res.update({"fp32_step_ms": round(fp32_step[0], 4), "fp32_step_ms_min_max": [round(fp32_step[1], 4), round(fp32_step[2], 4)],
                    "speedup_over_fp32_step": round(fp32_step[0] / step[0], 3), "max_abs_diff_to_fp32_step": diff16,
                    "peak_16bit_mfma_tflops": PEAK_16BIT_MFMA_TFLOPS, "gemm16_tiles_128x128": tiles, "compute_units": 256})
    if attn16:
        a32 = split.pop("attention_fp32")["ms_per_call"]
        res["split_sum_ms"] = round(sum(v["ms_per_forward"] for v in split.values()), 4)
        res["arithmetic"] += f"; attention operands {a.attention_format} on v_mfma_f32_32x32x16, fp32 softmax and accumulate"
        res["attention"]["frac_of_16bit_mfma_peak"] = round(attn_flop / (attn_ms * 1e-3) / 1e12 / PEAK_16BIT_MFMA_TFLOPS, 4)
        res.update({"attention_fp32": {"ms_per_call": a32, "ms_per_forward": round(a32 * L, 4), "kernel": "omnitok_dit_attn, same session"},
                    "attention16_speedup_over_fp32_kernel": round(a32 / attn_ms, 3),
                    "fp32_attention_step_ms": round(a32_step[0], 4),
                    "fp32_attention_step_ms_min_max": [round(a32_step[1], 4), round(a32_step[2], 4)],
                    "speedup_over_fp32_attention_step": round(a32_step[0] / step[0], 3), "max_abs_diff_to_fp32_attention_step": diff_a16,
                    "peak_16bit_mfma_tflops": PEAK_16BIT_MFMA_TFLOPS})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
