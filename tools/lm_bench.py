#!/usr/bin/env python
"""Tokens/s of the LM consumer's sampling loop (sample_with_past) on the MI355X, reference k600
LM shape by default (scripts/lm_train/train_k600.sh: vocab 8192, block 5120, 24 layers, 16 heads,
1536 wide), synthetic weights.  One JSON line: throughput, per-step time at the start / end of the
sequence, the HBM roofline of a step (weight bytes + K/V bytes read) and a CPU baseline (the oracle's
KV-cached step on the host, bounded sample).
    python tools/lm_bench.py [--batch 1] [--steps 512] [--ctx 0] [--weights fp32|bf16|fp16] [--kv fp32|bf16|fp16] [--also 8] [--no-cpu-baseline]
                             [--max-streams 16] [--streams-format fp32|w16] [--decode-quant none|fp8]
                             [--cache-quant none|fp8]
--kv8-session OUT.json: the cache-quant record instead (GPT.set_cache_quant; profiles/lm_kv8_bench.json): see kv8_session.
--fp8-session OUT.json: the decode-quant record instead (GPT.set_decode_quant; profiles/lm_fp8.json): see fp8_session.
--streams-session OUT.json: the many-stream record instead (GPT.set_max_streams; profiles/lm_streams_bench.json): the bare decode step
(graph replay) of B in --session-batches streams at --session-ctx cached tokens, fp32 weights + fp32 cache first, then bf16 + bf16,
and of 8 and 16 streams once more with "lm_streams_min" 1 (the many-stream kernel below its default threshold).  The cache lengths
are set on the device, nothing is prefilled: a step's time depends on how many rows it reads, not on what they hold.
With --streams-format w16 the session is the record of GPT.set_streams_format instead (profiles/lm_streams16_bench.json): bf16 weights +
bf16 cache only; per context the "fp32" streams format first (every batch, and the 8 / 16-stream cells as above: the yardstick, the
path as it was), then "w16" at the batches of 17 and more streams, then "fp32" once more at those batches (the end of the session);
and the bare GEMMs at the model's five shapes and B = 32, 64, 128: omnitok_lm_gemm_streams (fp32-input MFMA over bf16 weights), then
omnitok_lm_gemm16 at M = B (the prefill kernel), then omnitok_lm_gemm_streams16, 10 back-to-back launches per timed call.
--prefill-session OUT.json: the batched-prefill record (GPT.set_prefill_format; profiles/lm_prefill16_bench.json): per weight format
bf16 then fp16, GPT.forward and GPT.token_losses at (B, T) in --prefill-shapes with the fp32 prefill first and the "w16" prefill after
it, and the bare omnitok_lm_gemm16 at the model's five GEMM shapes with M = the largest B * T.  --prefill-attention rows,tiled adds the
attention mode (GPT.set_prefill_attention; profiles/lm_prefill_attn_bench.json) as the outermost arm per shape, in the order given (the
default "rows" alone is the record as it was); --prefill-weights picks the weight formats; --prefill-attention-operands fp32,bf16,fp16
adds the operand format of the tiled attention (GPT.set_prefill_attention_operands; profiles/lm_prefill_attn16_bench.json) as the
INNERMOST arm, in the order given, under the attention mode "tiled" only (the default "fp32" alone is the record as it was).
--attn-kernel-session OUT.json: the bare attention kernels instead, no model: omnitok_lm_attn_prefill, then omnitok_lm_attn_prefill16
with bf16, then fp16 operands, on the same standard-normal qkv at every BxTxHEADSxHEAD_DIM of --attn-shapes, 6 calls each, the median
of the last 5 by device events (run it under `rocprofv3 --kernel-trace --stats -- python tools/lm_bench.py ...` for the kernels' own
times)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from omnitokenizer_amd import gpt as og  # noqa: E402
from omnitokenizer_amd.synth import synth_gpt_state  # noqa: E402

PEAK_HBM_GBS = 8000.0
PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_16BIT_MFMA_TFLOPS = 2500.0


def fp8_session(a, sd, dims):
    """The record of GPT.set_decode_quant (profiles/lm_fp8.json): the bare decode step (graph replay) of B in --session-batches
    streams at --session-ctx cached tokens on four engines over the same weights -- fp32 weights + fp32 cache and bf16 + bf16, each
    with the switch off and with "fp8" -- ALTERNATED: five rounds, every round times each arm once, the median per arm.  The cache
    lengths are set on the device, nothing is prefilled."""
    V, BS, L, H, C = dims
    hd = C // H
    batches = [int(b) for b in a.session_batches.split(",")]
    ctxs = [int(c) for c in a.session_ctx.split(",")]
    arms = [("fp32", "none"), ("fp32", "fp8"), ("bf16", "none"), ("bf16", "fp8")]
    models = {}
    for fmt, dq in arms:
        m = og.GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
        m.load_state_dict(sd, strict=True)
        models[fmt, dq] = m.cuda().eval().set_weight_format(fmt).set_cache_format(fmt).set_decode_quant(dq)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cells = []
    for ctx in ctxs:
        for m in models.values():
            m.set_cache_format(m.cache_format)     # drops the cache: reset_streams allocates exactly ctx + 64 positions
            m.reset_streams(max(batches), ctx + 64)
        for B in batches:
            replays = {k: m.graph_step(B)[2] for k, m in models.items()}

            def one_round(k, n):
                m = models[k]
                e0.record()
                for _ in range(n):
                    m._pos[:B] = ctx
                    m._len[:B] = ctx
                    replays[k]()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / n
            nrep = max(5, min(50, int(100.0 / max(max(one_round(k, 3) for k in arms), 1e-3))))
            rounds = {k: [] for k in arms}
            for _ in range(5):
                for k in arms:
                    rounds[k].append(one_round(k, nrep))
            for (fmt, dq), r in rounds.items():
                r = sorted(r)
                m = models[fmt, dq]
                m.check_overflow()
                weight_bytes = float(m.step_weight_bytes())
                kv_bytes = 2.0 * L * B * H * (ctx + 1) * hd * (4.0 if fmt == "fp32" else 2.0)
                cells.append({"weights": fmt, "kv": fmt, "decode_quant": dq, "ctx": ctx, "streams": B, "step_ms": round(r[2], 4),
                              "step_ms_min_max": [round(r[0], 4), round(r[-1], 4)], "replays_per_round": nrep,
                              "weight_bytes": weight_bytes, "kv_bytes": kv_bytes,
                              "hbm_gbs": round((weight_bytes + kv_bytes) / (r[2] * 1e-3) / 1e9, 1),
                              "hbm_frac": round((weight_bytes + kv_bytes) / (r[2] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)})
                print(json.dumps(cells[-1]), flush=True)
    ms = {(c["weights"], c["decode_quant"], c["ctx"], c["streams"]): c["step_ms"] for c in cells}
    ratios = [{"ctx": ctx, "streams": B, "fp8_vs_bf16": round(ms["bf16", "none", ctx, B] / ms["bf16", "fp8", ctx, B], 3),
               "fp8_vs_fp32": round(ms["fp32", "none", ctx, B] / ms["fp32", "fp8", ctx, B], 3)} for ctx in ctxs for B in batches]
    return {"workload": f"GPT {L}x{C} ({H} heads, head_dim {hd}), vocab {V}, block {BS}: bare decode step (graph replay)",
            "method": "four engines over the same synthetic weights, arms alternated inside each of 5 rounds, median per arm; "
                      "speedups are step_ms(switch off) / step_ms(fp8) at the same weight and cache format",
            "device": torch.cuda.get_device_name(0), "peak_hbm_gbs": PEAK_HBM_GBS, "cells": cells, "fp8_speedup": ratios}


def kv8_session(a, sd, dims):
    """The record of GPT.set_cache_quant (profiles/lm_kv8_bench.json): bf16 weights over three caches -- fp32, bf16 (the yardstick:
    the code as it was) and fp8 -- as three engines over the same weights.  Per cell the bare decode step (graph replay; the cache
    lengths are set on the device, nothing is prefilled), arms ALTERNATED inside each of 1 dropped + 5 timed rounds, the median per
    arm; then the attention launch alone: the exported entry of that cache (partials + merge) at the cell's shape, rotating over
    four layers' worth of slabs, 1 dropped + 5 timed rounds of 24 launches.  Cells: --session-ctx x --session-batches on 16-stream
    engines, then --kv8-many streams at the last context on engines of max(--kv8-many) streams, where the fp32 cache is timed on its
    own first (the three caches do not fit side by side) and bf16 / fp8 alternate.  The first cell is repeated at the end: the
    session's drift."""
    import ctypes
    from omnitokenizer_amd import _lib
    V, BS, L, H, C = dims
    hd = C // H
    batches = [int(b) for b in a.session_batches.split(",")]
    ctxs = [int(c) for c in a.session_ctx.split(",")]
    many = [int(b) for b in a.kv8_many.split(",") if b]
    arms = ["fp32", "bf16", "fp8"]
    elem = {"fp32": 4.0, "bf16": 2.0, "fp8": 1.0}
    models = {}
    for arm in arms:
        m = og.GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval().set_weight_format("bf16")
        models[arm] = m.set_cache_quant("fp8") if arm == "fp8" else m.set_cache_format(arm)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lib = _lib.load()
    cells = []

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def drop(ms_):
        for m in ms_:
            m.set_cache_format(m.cache_format)     # drops the cache: reset_streams allocates exactly ctx + 64 positions

    def attn_ms(arm, B, ctx):
        """median ms of one attention launch pair of `arm`'s exported entry: B streams, ctx cached tokens, max_len ctx + 64"""
        ml, NS = ctx + 64, 4
        dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp8": torch.uint8}[arm]
        kc = [torch.zeros(B, H, ml, hd, dtype=dt, device="cuda") for _ in range(NS)]
        vc = [torch.zeros(B, H, ml, hd, dtype=dt, device="cuda") for _ in range(NS)]
        sc = [torch.ones(2, B, H, ml, device="cuda") for _ in range(NS if arm == "fp8" else 0)]
        qkv = torch.randn(B, 3 * C, device="cuda")
        cl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
        scratch = torch.empty(B * H * ((ml + 255) // 256) * (2 + hd), device="cuda")
        out = torch.empty(B, C, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def launch(i):
            if arm == "fp32":
                rc = lib.omnitok_lm_attn_decode(p(qkv), p(kc[i]), p(vc[i]), p(cl), B, H, hd, ml, p(scratch), p(out), st)
            elif arm == "bf16":
                rc = lib.omnitok_lm_attn_decode_kv16(p(qkv), p(kc[i]), p(vc[i]), 1, p(cl), B, H, hd, ml, p(scratch), p(out), st)
            else:
                rc = lib.omnitok_lm_attn_decode_kv8(p(qkv), p(kc[i]), p(vc[i]), p(sc[i][0]), p(sc[i][1]), p(cl), B, H, hd, ml,
                                                    p(scratch), p(out), st)
            _lib.check(rc, "attention entry")
        rounds = []
        for _ in range(6):
            e0.record()
            for i in range(24):
                launch(i % NS)
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) / 24)
        return sorted(rounds[1:])[2]

    def cell(ctx, B, group, note=None):
        replays = {k: models[k].graph_step(B)[2] for k in group}

        def one_round(k, n):
            m = models[k]
            e0.record()
            for _ in range(n):
                m._pos[:B] = ctx
                m._len[:B] = ctx
                replays[k]()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        nrep = max(3, min(50, int(100.0 / max(max(one_round(k, 2) for k in group), 1e-3))))
        rounds = {k: [] for k in group}
        for _ in range(6):
            for k in group:
                rounds[k].append(one_round(k, nrep))
        for k in group:
            r = sorted(rounds[k][1:])
            m = models[k]
            m.check_overflow()
            kv_bytes = 2.0 * L * B * H * (ctx + 1) * (hd * elem[k] + (4.0 if k == "fp8" else 0.0))     # read by one step, scales included
            cells.append({"weights": "bf16", "cache": k, "ctx": ctx, "streams": B, "max_streams": m.max_streams,
                          "max_len": m._cache_shape[1], "step_ms": round(r[2], 4), "step_ms_min_max": [round(r[0], 4), round(r[-1], 4)],
                          "replays_per_round": nrep, "cache_bytes_allocated": m.cache_bytes(), "kv_bytes_read": kv_bytes,
                          "weight_bytes": float(m.step_weight_bytes()),
                          "step_hbm_frac": round((m.step_weight_bytes() + kv_bytes) / (r[2] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                          **({"note": note} if note else {})})
            print(json.dumps(cells[-1]), flush=True)

    def attn_cells(ctx, B, tag=None):
        for k in arms:
            ms = attn_ms(k, B, ctx)
            byts = 2.0 * B * H * (ctx + 1) * (hd * elem[k] + (4.0 if k == "fp8" else 0.0))
            for c in cells:
                if (c["cache"], c["ctx"], c["streams"], c.get("note")) == (k, ctx, B, tag):
                    c.update({"attn_launch_ms": round(ms, 5), "attn_bytes": byts, "attn_gbs": round(byts / (ms * 1e-3) / 1e9, 1),
                              "attn_hbm_frac": round(byts / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)})

    for ctx in ctxs:
        drop(models.values())
        for m in models.values():
            m.reset_streams(max(batches), ctx + 64)
        for B in batches:
            cell(ctx, B, arms)
    if ctxs[-1] != ctxs[0]:      # the first cell again, in a cache of its own size like the first time
        drop(models.values())
        for m in models.values():
            m.reset_streams(max(batches), ctxs[0] + 64)
    cell(ctxs[0], batches[0], arms, note="first cell again")
    drop(models.values())
    if many:
        ctx, NB = ctxs[-1], max(many)
        for m in models.values():
            m.set_max_streams(NB)
        for group in (["fp32"], ["bf16", "fp8"]):
            try:
                for k in group:
                    models[k].reset_streams(NB, ctx + 64)
                for B in many:
                    cell(ctx, B, group)
            except Exception as exc:     # a cache the device cannot hold: recorded, not fatal
                cells.append({"weights": "bf16", "cache": "+".join(group), "ctx": ctx, "skipped": f"{NB} streams x {ctx + 64} tokens: {exc}"})
            drop(models[k] for k in group)
    for ctx in ctxs:
        for B in batches:
            attn_cells(ctx, B)
    for B in many:
        attn_cells(ctxs[-1], B)
    ms = {(c["cache"], c["ctx"], c["streams"]): c for c in cells if "step_ms" in c and "note" not in c}
    verdict = []
    for (k, ctx, B), c in ms.items():
        if k == "fp8" and ("bf16", ctx, B) in ms:
            y = ms["bf16", ctx, B]
            verdict.append({"ctx": ctx, "streams": B, "bf16_cache_ms": y["step_ms"], "fp8_cache_ms": c["step_ms"],
                            "step_speedup": round(y["step_ms"] / c["step_ms"], 3), "fp8_gained": bool(c["step_ms"] < y["step_ms"]),
                            **({"attn_speedup": round(y["attn_launch_ms"] / c["attn_launch_ms"], 3)} if "attn_launch_ms" in c and "attn_launch_ms" in y else {})})
    return {"metric": "LM decode step (graph replay) over an fp32 / bf16 / fp8 K/V cache, bf16 weights", "unit": "ms per step",
            "workload": f"GPT {L}x{C} ({H} heads, head_dim {hd}), vocab {V}, block {BS}",
            "protocol": "graph replay, pos / cache_len reset before every replay, arms alternated inside each of 1 dropped + 5 timed "
                        "rounds, median per arm; the yardstick is the bf16 cache (the code as it was); attn_*: the exported attention "
                        "entry alone (partials + merge launches) at the cell's shape over 4 rotating slab pairs, 1 dropped + 5 timed "
                        "rounds of 24 launches; cache contents not prefilled",
            "device": torch.cuda.get_device_name(0), "peak_hbm_gbs": PEAK_HBM_GBS, "cells": cells, "fp8_vs_bf16_cache": verdict,
            "did_not_gain": [f"ctx {v['ctx']} x {v['streams']} streams" for v in verdict if not v["fp8_gained"]]}


def streams_session(a, m, dims):
    """One session over (format, cached tokens, streams): see the module docstring.  Returns the record."""
    from omnitokenizer_amd import _lib
    V, BS, L, H, C = dims
    hd = C // H
    batches = [int(b) for b in a.session_batches.split(",")]
    ctxs = [int(c) for c in a.session_ctx.split(",")]
    NB = max(batches)
    m.set_max_streams(NB)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    default_min = _lib.get_option("lm_streams_min")
    flop_per_stream = 2.0 * (12.0 * C * C * L + V * C)
    cells = []

    def time_cell(B, length):
        """median ms of 5 rounds of nrep graph replays of the B-stream step at cache length `length` (a first round is dropped)"""
        _, _, replay = m.graph_step(B)

        def one_round(n):
            e0.record()
            for _ in range(n):
                m._pos[:B] = length
                m._len[:B] = length
                replay()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        first = one_round(3)
        nrep = max(5, min(50, int(250.0 / max(first, 1e-3))))
        rounds = sorted(one_round(nrep) for _ in range(5))
        return rounds[2], [round(rounds[0], 4), round(rounds[-1], 4)], nrep

    sf16 = a.streams_format == "w16"
    fmts = ("bf16",) if sf16 else ("fp32", "bf16")     # the fp32 arm first
    for fmt in fmts:
        m.set_weight_format(fmt).set_cache_format(fmt)
        weight_bytes = float(m.step_weight_bytes())
        kv_elem = 4.0 if fmt == "fp32" else 2.0
        for ctx in ctxs:
            # a cache sized for this context, as `--ctx` runs allocate it: the attention launch covers the whole cache, and a
            # workgroup has requested its chunk's rows before it learns that the stream ends in front of them
            m.set_cache_format(fmt)      # drops the cache: the next reset_streams allocates exactly ctx + 64 positions
            try:
                m.reset_streams(NB, ctx + 64)
            except Exception as exc:     # a cache the device cannot hold: recorded, not fatal
                cells.append({"weights": fmt, "kv": fmt, "ctx": ctx, "skipped": f"cache for {NB} streams x {ctx + 64} tokens: {exc}"})
                continue
            arms = [(B, default_min, "fp32") for B in batches] + [(B, 1, "fp32") for B in (8, 16) if B in batches and B < default_min]
            if sf16:
                many = [B for B in batches if B >= default_min]
                arms += [(B, default_min, "w16") for B in many] + [(B, default_min, "fp32 again") for B in many]
            for B, smin, sf in arms:
                _lib.set_option("lm_streams_min", smin)
                m.set_streams_format(sf.split()[0])     # (drops the graphs: the kernels are chosen when the step is captured)
                try:
                    ms, spread, nrep = time_cell(B, ctx)
                finally:
                    _lib.set_option("lm_streams_min", default_min)
                    m._graphs = {}
                m.check_overflow()
                kv_bytes = 2.0 * L * B * H * (ctx + 1) * hd * kv_elem
                cells.append({"weights": fmt, "kv": fmt, "ctx": ctx, "streams": B, "lm_streams_min": smin,
                              **({"streams_format": sf} if sf16 else {}),
                              "path": "many-stream 16-bit MFMA GEMM" if sf == "w16" else "many-stream MFMA GEMM" if B >= smin else "VALU GEMV, groups of 8",
                              "max_len": m._cache_shape[1], "step_ms": round(ms, 4), "step_ms_min_max": spread,
                              "replays_per_round": nrep,
                              "tokens_s": round(B / (ms * 1e-3), 1), "weight_bytes": weight_bytes, "kv_bytes": kv_bytes,
                              "frac_hbm": round((weight_bytes + kv_bytes) / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                              # the step's GEMM FLOPs over the WHOLE step's time (attention, LayerNorm and every launch boundary
                              # included) against the f32-MFMA peak: a rate of the step, not of the GEMM kernels
                              "step_gemm_flops_over_f32_mfma_peak": round(B * flop_per_stream / (ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)})
                print(json.dumps(cells[-1]), flush=True)
    m.set_streams_format("fp32")
    # the yardstick: a B-stream step against B / 16 steps of 16 streams (the <= 16-stream path, untouched)
    verdict, sf_verdict = [], []
    for fmt in fmts:
        for ctx in ctxs:
            def cell(B, smin=default_min, sf="fp32"):
                return next((c for c in cells if c.get("weights") == fmt and c.get("ctx") == ctx and c.get("streams") == B
                             and c.get("lm_streams_min") == smin and c.get("streams_format", "fp32") == sf), None)
            for B in (batches if sf16 else []):
                first, w16, again = cell(B), cell(B, sf="w16"), cell(B, sf="fp32 again")
                if first and w16 and again:
                    sf_verdict.append({"weights": fmt, "ctx": ctx, "streams": B, "fp32_first_ms": first["step_ms"],
                                       "w16_ms": w16["step_ms"], "fp32_again_ms": again["step_ms"],
                                       "speedup": round(min(first["step_ms"], again["step_ms"]) / w16["step_ms"], 3),
                                       "w16_faster": bool(w16["step_ms"] < min(first["step_ms"], again["step_ms"]))})
            base = cell(16)
            for B in batches:
                c = cell(B)
                if base and c and B > 16:
                    verdict.append({"weights": fmt, "ctx": ctx, "streams": B, "step_ms": c["step_ms"],
                                    "steps_of_16_ms": round(base["step_ms"] * B / 16, 4),
                                    "speedup": round(base["step_ms"] * B / 16 / c["step_ms"], 3)})
    extra = {"w16_vs_fp32": sf_verdict, "gemms": streams_gemms(a, dims), "device": device_state()} if sf16 else {}
    return {**extra, "metric": "LM decode step (graph replay), many streams per engine", "unit": "ms per step",
            "config": {"workload": f"GPT {L}x{C} ({H} heads, head_dim {hd}), vocab {V}, block {BS}", "max_streams": NB,
                       "peak_hbm_gbs": PEAK_HBM_GBS, "peak_f32_mfma_tflops": PEAK_F32_MFMA_TFLOPS,
                       "protocol": "graph replay, pos / cache_len reset before every replay, 1 dropped + 5 timed rounds, median; "
                                   "fp32 arm first; cache contents not prefilled; the timed window includes the two small device fills that "
                                   "reset pos / cache_len before each replay (the same in every cell, as in the tool's other records: "
                                   "ratios stand, absolute times are high by those two launches)",
                       "frac_hbm": "(weight bytes + K/V bytes of the cached tokens) / step time / peak_hbm_gbs",
                       "step_gemm_flops_over_f32_mfma_peak": "2 B (12 C^2 L + V C) FLOP / WHOLE step time / peak: a rate of the step, "
                                                             "attention and LayerNorm launches included, not of the GEMM kernels"},
            "cells": cells, "vs_steps_of_16": verdict}


def device_state():
    """clock and power of the device as rocm-smi reports them after the session, or the reason they could not be read"""
    import subprocess
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=60)
        return json.loads(r.stdout) if r.returncode == 0 else {"not_readable": f"rocm-smi exit {r.returncode}: {r.stderr.strip()[:200]}"}
    except Exception as exc:
        return {"not_readable": f"{type(exc).__name__}: {exc}"}


def streams_gemms(a, dims):
    """The bare many-stream GEMMs at the model's five shapes, bf16: see the module docstring.  Returns the cells."""
    import ctypes
    from omnitokenizer_amd import _lib
    V, BS, L, H, C = dims
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    default_min = _lib.get_option("lm_streams_min")
    fmt = og.WEIGHT_FORMATS["bf16"]
    cells = []
    for what, N, K, act in (("qkv", 3 * C, C, 0), ("proj", C, C, 0), ("fc1 (GELU)", 4 * C, C, 1), ("fc2", C, 4 * C, 0), ("head", V, C, 0)):
        w = ((torch.rand(N, K, device="cuda") * 2 - 1) * 0.02).to(torch.bfloat16)
        bias = torch.zeros(N, device="cuda")
        for B in (32, 64, 128):
            x32 = torch.rand(B, K, device="cuda") * 2 - 1
            x16 = x32.to(torch.bfloat16)
            y32 = torch.empty(B, N, device="cuda")
            y16 = torch.empty(B, N, device="cuda", dtype=torch.bfloat16)
            o32, o16 = (None, y16) if act else (y32, None)      # FC1 writes the 16-bit operand of FC2 in both 16-bit kernels
            calls = {"gemm_streams (fp32 MFMA)": lambda: lib.omnitok_lm_gemm_streams(P(x32), P(w), fmt, P(bias), None, None, None, P(y32), B, N, K,
                                                                                     act, stream),
                     "gemm16 (M = B)": lambda: lib.omnitok_lm_gemm16(P(x16), P(w), fmt, P(bias), None, P(o32), P(o16), B, N, K, act, None, stream),
                     "gemm_streams16": lambda: lib.omnitok_lm_gemm_streams16(P(x16), P(w), fmt, P(bias), None, P(o32), P(o16), B, N, K, act, None,
                                                                            stream)}
            cell = {"gemm": what, "B": B, "N": N, "K": K, "weight_mb": round(N * K * 2 / 1e6, 2), "gflop": round(2.0 * B * N * K / 1e9, 3)}
            for name, fn in calls.items():
                ms = []
                for _ in range(6):
                    e0.record()
                    for _ in range(10):
                        _lib.check(fn(), name)
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1) / 10)
                last = sorted(ms[1:])
                cell[name + " us"] = round(last[2] * 1e3, 2)
                cell[name + " us_min_max"] = [round(last[0] * 1e3, 2), round(last[-1] * 1e3, 2)]
            cell["streams16_over_fp32_mfma"] = round(cell["gemm_streams (fp32 MFMA) us"] / cell["gemm_streams16 us"], 2)
            cell["streams16_over_gemm16"] = round(cell["gemm16 (M = B) us"] / cell["gemm_streams16 us"], 2)
            cells.append(cell)
            print(json.dumps(cell), flush=True)
        del w
    assert _lib.get_option("lm_streams_min") == default_min
    return cells


def attn_kernel_session(a):
    """The bare prefill-attention kernels, fp32 operands first: see the module docstring.  Returns the record."""
    import ctypes
    from omnitokenizer_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    cells = []
    for B, T, H, hd in (tuple(int(v) for v in s.split("x")) for s in a.attn_shapes.split(",")):
        C = H * hd
        qkv = torch.randn(B * T, 3 * C, generator=torch.Generator().manual_seed(5)).cuda()
        out = torch.empty(B * T, C, device="cuda")
        flop = 4.0 * (T * (T + 1) / 2) * C * B
        calls = {"fp32": lambda: lib.omnitok_lm_attn_prefill(P(qkv), B, T, H, hd, P(out), None, 0, None, stream)}
        for op in ("bf16", "fp16"):
            calls[op] = lambda op=op: lib.omnitok_lm_attn_prefill16(P(qkv), B, T, H, hd, og.WEIGHT_FORMATS[op], P(out), None, 0, None, stream)
        base = None
        for op, fn in calls.items():
            ms = []
            for _ in range(6):
                e0.record()
                _lib.check(fn(), "lm_attn_prefill")
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            last = sorted(ms[1:])
            med = last[len(last) // 2]
            base = med if op == "fp32" else base
            cells.append({"B": B, "T": T, "heads": H, "head_dim": hd, "operands": op, "ms": round(med, 4),
                          "ms_min_max": [round(last[0], 4), round(last[-1], 4)], "first_call_ms": round(ms[0], 4),
                          "tflops": round(flop / (med * 1e-3) / 1e12, 1), "fp32_over_this": round(base / med, 3)})
            print(json.dumps(cells[-1]), flush=True)
        del qkv, out
    return {"metric": "bare prefill attention kernels (omnitok_lm_attn_prefill, omnitok_lm_attn_prefill16)", "unit": "ms per call",
            "config": {"protocol": "one process; per shape fp32 operands first, then bf16, then fp16, on the same standard-normal qkv, fp32 output; "
                                   "device events around each call, 6 calls, the median (min, max) of the last 5",
                       "tflops": "4 (T (T + 1) / 2) C B FLOP / call time"},
            "cells": cells}


def prefill_session(a, m, dims):
    """One session over (weight format, prefill format, shape): see the module docstring.  Returns the record."""
    import ctypes
    from omnitokenizer_amd import _lib
    V, BS, L, H, C = dims
    lib = _lib.load()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.prefill_shapes.split(",")]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, reps):
        """median ms of `reps` calls after one dropped call, and the (min, max)"""
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        out.sort()
        return out[len(out) // 2], [round(out[0], 3), round(out[-1], 3)]

    cells, gemms = [], []
    gen = torch.Generator().manual_seed(3)
    fmts = a.prefill_weights.split(",")
    modes = a.prefill_attention.split(",")
    aops = a.prefill_attention_operands.split(",")
    arms = [(mode, pf, aop) for mode in modes for pf in ("fp32", "w16") for aop in (aops if mode == "tiled" else ["fp32"])]
    aop0 = "fp32" if "fp32" in aops else aops[0]   # the operand format of the tiled cells the older verdicts compare
    for fmt in fmts:
        m.set_weight_format(fmt)
        for B, T in shapes:
            M = B * T
            flop = 2.0 * M * (12.0 * C * C * L + V * C)
            idx = torch.randint(0, V, (B, T), generator=gen).cuda()
            tg = torch.randint(0, V, (B, T), generator=gen).cuda()
            for mode, pf, aop in arms:    # the first mode first, in it the fp32 arm first, in it the operand formats in the order given
                m.set_prefill_attention(mode)
                m.set_prefill_format(pf)
                m.set_prefill_attention_operands(aop)
                peak = PEAK_F32_MFMA_TFLOPS if pf == "fp32" else PEAK_16BIT_MFMA_TFLOPS
                cell = {"weights": fmt, "prefill": pf, "attention": mode, **({"operands": aop} if aops != ["fp32"] else {}),
                        "B": B, "T": T, "gemm_flop": flop}
                for name, fn in (("forward", lambda: m(idx)), ("token_losses", lambda: m.token_losses(idx, tg))):
                    ms, spread = timed(fn, a.prefill_reps)
                    cell[name + "_ms"] = round(ms, 3)
                    cell[name + "_ms_min_max"] = spread
                    cell[name + "_tflops"] = round(flop / (ms * 1e-3) / 1e12, 1)
                    cell[name + "_frac_of_peak"] = round(flop / (ms * 1e-3) / 1e12 / peak, 4)
                cell["peak_tflops"] = peak
                m.check_overflow()
                cells.append(cell)
                print(json.dumps(cell), flush=True)
            del idx, tg
        # the bare GEMM at the model's shapes, M = the largest B * T: operands uniform in [-1, 1) / 0.02 x that, not zeros
        M = max(B * T for B, T in shapes)
        dt = torch.bfloat16 if fmt == "bf16" else torch.float16
        stream = torch.cuda.current_stream().cuda_stream
        total = 0.0
        for what, N, K, y16, per_model in (("qkv", 3 * C, C, False, L), ("proj", C, C, False, L), ("fc1 (GELU, 16-bit out)", 4 * C, C, True, L),
                                            ("fc2", C, 4 * C, False, L), ("head", V, C, False, 1)):
            x = (torch.rand(M, K, device="cuda") * 2 - 1).to(dt)
            w = ((torch.rand(N, K, device="cuda") * 2 - 1) * 0.02).to(dt)
            bias = torch.zeros(N, device="cuda")
            y = torch.empty(M, N, device="cuda", dtype=dt if y16 else torch.float32)
            P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

            def call():
                for _ in range(10):
                    _lib.check(lib.omnitok_lm_gemm16(P(x), P(w), og.WEIGHT_FORMATS[fmt], P(bias), None, None if y16 else P(y),
                                                     P(y) if y16 else None, M, N, K, int(y16), None, stream), "lm_gemm16")
            ms, spread = timed(call, a.prefill_reps)
            ms /= 10
            tf = 2.0 * M * N * K / (ms * 1e-3) / 1e12
            total += per_model * ms
            gemms.append({"weights": fmt, "gemm": what, "M": M, "N": N, "K": K, "ms": round(ms, 4),
                          "ms_min_max": [round(v / 10, 4) for v in spread], "tflops": round(tf, 1),
                          "frac_of_16bit_peak": round(tf / PEAK_16BIT_MFMA_TFLOPS, 4), "calls_per_forward": per_model})
            print(json.dumps(gemms[-1]), flush=True)
            del x, w, y
        for mode in modes:
            big = next(c for c in cells if c["weights"] == fmt and c["prefill"] == "w16" and c["attention"] == mode and c["B"] * c["T"] == M
                       and c.get("operands", "fp32") == (aop0 if mode == "tiled" else "fp32"))
            gemms.append({"weights": fmt, "M": M, "gemm_ms_per_forward": round(total, 3), "forward_ms": big["forward_ms"],
                          "non_gemm_ms_per_forward": round(big["forward_ms"] - total, 3), **({"attention": mode} if len(modes) > 1 else {})})
            print(json.dumps(gemms[-1]), flush=True)
    m.set_prefill_format("fp32").set_prefill_attention("rows").set_prefill_attention_operands("fp32")

    def cell_of(fmt, pf, mode, B, T, aop=None):
        aop = aop or (aop0 if mode == "tiled" else "fp32")
        return next(c for c in cells if (c["weights"], c["prefill"], c["attention"], c["B"], c["T"], c.get("operands", "fp32"))
                    == (fmt, pf, mode, B, T, aop))
    verdict, attn_verdict, aop_verdict = [], [], []
    for fmt in fmts:
        for B, T in shapes:
            for mode in modes:
                f32, w16 = (cell_of(fmt, pf, mode, B, T) for pf in ("fp32", "w16"))
                verdict.append({"weights": fmt, "B": B, "T": T, **({"attention": mode} if len(modes) > 1 else {}),
                                "forward_speedup": round(f32["forward_ms"] / w16["forward_ms"], 3),
                                "token_losses_speedup": round(f32["token_losses_ms"] / w16["token_losses_ms"], 3),
                                "w16_faster": bool(w16["forward_ms"] < f32["forward_ms"] and w16["token_losses_ms"] < f32["token_losses_ms"])})
            if "rows" in modes and "tiled" in modes:
                for pf in ("fp32", "w16"):
                    r, t = cell_of(fmt, pf, "rows", B, T), cell_of(fmt, pf, "tiled", B, T)
                    attn_verdict.append({"weights": fmt, "prefill": pf, "B": B, "T": T, "rows_forward_ms": r["forward_ms"],
                                         "tiled_forward_ms": t["forward_ms"], "forward_speedup": round(r["forward_ms"] / t["forward_ms"], 3),
                                         "token_losses_speedup": round(r["token_losses_ms"] / t["token_losses_ms"], 3)})
            if "tiled" in modes and "fp32" in aops:
                for pf in ("fp32", "w16"):
                    base = cell_of(fmt, pf, "tiled", B, T)
                    for aop in (o for o in aops if o != "fp32"):
                        c = cell_of(fmt, pf, "tiled", B, T, aop)
                        aop_verdict.append({"weights": fmt, "prefill": pf, "B": B, "T": T, "operands": aop, "fp32_operands_forward_ms": base["forward_ms"],
                                            "forward_ms": c["forward_ms"], "forward_speedup": round(base["forward_ms"] / c["forward_ms"], 3),
                                            "token_losses_speedup": round(base["token_losses_ms"] / c["token_losses_ms"], 3)})
    extra = {"tiled_vs_rows": attn_verdict} if attn_verdict else {}
    if aop_verdict:
        extra["operands_16bit_vs_fp32"] = aop_verdict
    return {**extra, "metric": "LM batched prefill (GPT.forward / GPT.token_losses), fp32 prefill vs the 16-bit MFMA prefill", "unit": "ms per call",
            "config": {"workload": f"GPT {L}x{C} ({H} heads, head_dim {C // H}), vocab {V}, block {BS}",
                       "peak_f32_mfma_tflops": PEAK_F32_MFMA_TFLOPS, "peak_16bit_mfma_tflops": PEAK_16BIT_MFMA_TFLOPS,
                       "protocol": f"one process; per weight format {' then '.join(fmts)}, per shape the attention mode(s) {' then '.join(modes)}, in each "
                                   f"the fp32 prefill first, then w16{'' if aops == ['fp32'] else ', in each (tiled mode) the attention operands ' + ' then '.join(aops)}; device events "
                                   f"around each call, 1 dropped + {a.prefill_reps} timed calls, median (min, max beside it); bare GEMMs: 10 "
                                   "back-to-back launches per timed call on uniform random operands",
                       "tflops": "2 M (12 C^2 L + V C) FLOP of the six GEMM families / WHOLE call time (embedding, LayerNorm, attention, "
                                 "cross-entropy and every launch boundary included): a rate of the call, not of the GEMM kernels",
                       "non_gemm_ms_per_forward": "forward_ms of the w16 arm minus the bare GEMM times x their calls per forward"},
            "cells": cells, "gemm16": gemms, "w16_vs_fp32": verdict}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--ctx", type=int, default=0, help="tokens already in the cache before timing (prefilled)")
    ap.add_argument("--vocab", type=int, default=8192)
    ap.add_argument("--block", type=int, default=5120)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--embd", type=int, default=1536)
    ap.add_argument("--option", action="append", default=[], metavar="NAME=INT", help="omnitok_set_option switch (A/B)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-also", action="store_true", help="skip the 8-stream line (B = 1 runs only)")
    ap.add_argument("--also", default="8", metavar="B[,B..]", help="stream counts of the extra lines of a B = 1 run (default 8; up to --max-streams)")
    ap.add_argument("--weights", choices=("fp32", "bf16", "fp16"), default="fp32",
                    help="format of the matrices a decode step streams (GPT.set_weight_format)")
    ap.add_argument("--kv", choices=("fp32", "bf16", "fp16"), default="fp32", help="format of the K/V cache (GPT.set_cache_format)")
    ap.add_argument("--decode-quant", choices=("none", "fp8"), default="none",
                    help="weight-only quantisation of the decode step of up to 16 streams (GPT.set_decode_quant)")
    ap.add_argument("--cache-quant", choices=("none", "fp8"), default="none",
                    help="fp8 K/V cache with a scale per cached row (GPT.set_cache_quant)")
    ap.add_argument("--kv8-session", metavar="OUT.json", help="write the cache-quant record (kv8_session: --session-batches, default "
                    "1,2,4,8,16, x --session-ctx, then --kv8-many streams) and exit")
    ap.add_argument("--kv8-many", default="64,128", metavar="B[,B..]", help="stream counts of the many-stream cells of --kv8-session")
    ap.add_argument("--fp8-session", metavar="OUT.json", help="write the decode-quant record (fp8_session: --session-batches, "
                                                              "--session-ctx) and exit")
    ap.add_argument("--max-streams", type=int, default=16, help="streams per engine (GPT.set_max_streams, up to 128): the limit of "
                                                                 "--batch and of every --also count")
    ap.add_argument("--streams-format", choices=("fp32", "w16"), default="fp32",
                    help="GEMMs of a step of more than 16 streams (GPT.set_streams_format; w16 needs --weights bf16|fp16); with "
                         "--streams-session: the record of the w16 format against the fp32 one")
    ap.add_argument("--streams-session", metavar="OUT.json", help="write the many-stream record (see above) and exit")
    ap.add_argument("--session-batches", default="8,16,32,64,128")
    ap.add_argument("--session-ctx", default="0,4608")
    ap.add_argument("--prefill-session", metavar="OUT.json", help="write the batched-prefill record (see above) and exit")
    ap.add_argument("--prefill-shapes", default="1x5120,8x5120", metavar="BxT[,BxT..]")
    ap.add_argument("--prefill-reps", type=int, default=5)
    ap.add_argument("--prefill-weights", default="bf16,fp16", metavar="FMT[,FMT]")
    ap.add_argument("--prefill-attention", default="rows", metavar="MODE[,MODE]", help="rows | tiled | rows,tiled (GPT.set_prefill_attention)")
    ap.add_argument("--prefill-attention-operands", default="fp32", metavar="FMT[,FMT]",
                    help="fp32 | bf16 | fp16, comma-separated: the innermost arm of the tiled mode (GPT.set_prefill_attention_operands)")
    ap.add_argument("--attn-kernel-session", metavar="OUT.json", help="write the bare attention kernels' record (see above) and exit")
    ap.add_argument("--attn-shapes", default="1x5120x16x96,8x5120x16x96,8x5120x12x128,8x5120x24x64", metavar="BxTxHEADSxHEAD_DIM[,..]")
    a = ap.parse_args()
    if a.attn_kernel_session:
        rec = attn_kernel_session(a)
        with open(a.attn_kernel_session, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps({"written": a.attn_kernel_session}), flush=True)
        return
    V, BS, L, H, C = a.vocab, a.block, a.layers, a.heads, a.embd
    for kv in a.option:
        from omnitokenizer_amd import _lib
        _lib.set_option(kv.partition("=")[0], int(kv.partition("=")[2]))
    sd = synth_gpt_state(V, BS, L, H, C, seed=0)
    m = og.GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    m.load_state_dict(sd, strict=True)
    if a.kv8_session:
        if a.session_batches == ap.get_default("session_batches"):
            a.session_batches = "1,2,4,8,16"
        rec = kv8_session(a, sd, (V, BS, L, H, C))
        with open(a.kv8_session, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps({"written": a.kv8_session, "did_not_gain": rec["did_not_gain"]}), flush=True)
        return
    if a.fp8_session:
        rec = fp8_session(a, sd, (V, BS, L, H, C))
        with open(a.fp8_session, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps({"written": a.fp8_session, "fp8_speedup": rec["fp8_speedup"]}), flush=True)
        return
    m = m.cuda().eval().set_weight_format(a.weights).set_cache_format(a.kv).set_max_streams(a.max_streams)
    m.set_decode_quant(a.decode_quant).set_cache_quant(a.cache_quant)
    if a.prefill_session:
        rec = prefill_session(a, m, (V, BS, L, H, C))
        with open(a.prefill_session, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps({"written": a.prefill_session, "w16_vs_fp32": rec["w16_vs_fp32"]}), flush=True)
        return
    if a.streams_session:
        rec = streams_session(a, m, (V, BS, L, H, C))
        with open(a.streams_session, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps({"written": a.streams_session, "vs_steps_of_16": rec["vs_steps_of_16"], **({"w16_vs_fp32": rec["w16_vs_fp32"]} if "w16_vs_fp32" in rec else {})}), flush=True)
        return
    m.set_streams_format(a.streams_format)
    B = a.batch
    g = torch.Generator().manual_seed(1)
    cond = torch.randint(0, V, (B, 1 + a.ctx), generator=g).cuda()
    # prefill a.ctx tokens (not timed), then time `steps` sampled tokens
    torch.manual_seed(0)
    og.sample_with_past(cond, m, 8, top_k=2048, top_p=0.9, use_graph=not a.no_graph)  # warm-up + graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = og.sample_with_past(cond, m, a.steps, top_k=2048, top_p=0.9, use_graph=not a.no_graph)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the prefill of ctx tokens is inside dt: measure it alone and subtract
    t1 = time.perf_counter()
    og.sample_with_past(cond, m, 1, top_k=2048, top_p=0.9, use_graph=not a.no_graph)
    torch.cuda.synchronize()
    t_prefill = time.perf_counter() - t1
    dt_sample = max(dt - t_prefill, 1e-9)
    # the bare decode step (graph replay only, no token selection) at the final context length
    idx_buf, logits_buf, replay = m.graph_step(B)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nrep = 50

    def time_step(replay_fn, nb, length):
        """ms per bare decode step at cache length `length`: median of 5 rounds of nrep replays, and the rounds' (min, max)"""
        rounds = []
        for _ in range(6):  # the first round warms up and is dropped
            e0.record()
            for _ in range(nrep):
                m._pos[:nb] = length
                m._len[:nb] = length
                replay_fn()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) / nrep)
        rounds = sorted(rounds[1:])
        return rounds[2], [round(rounds[0], 4), round(rounds[-1], 4)]

    step_ms, step_spread = time_step(replay, B, a.ctx + a.steps)
    hd = C // H
    weight_bytes = float(m.step_weight_bytes())
    kv_elem = 4.0 if a.kv == "fp32" else 2.0  # bytes per cached K/V element
    if a.cache_quant == "fp8":                # a byte, and its share of the row's fp32 scale
        kv_elem = 1.0 + 4.0 / hd
    kv_bytes = 2.0 * L * B * H * (a.ctx + a.steps) * hd * kv_elem
    out_json = {
        "metric": "LM sampled tokens/sec (sample_with_past, top-k 2048 / top-p 0.9)",
        "value": round(B * a.steps / dt_sample, 1), "unit": "tokens/s", "n_gpus": 1, "batch_streams": B,
        "steps": a.steps, "ctx": a.ctx, "ms_per_token_step": round(dt_sample / a.steps * 1e3, 4),
        "dtype": "f32", "weights": a.weights, "kv": a.kv, "decode_quant": a.decode_quant, "cache_quant": a.cache_quant, "streams_format": a.streams_format, "data": "synthetic",
        "config": {"workload": f"GPT {L}x{C} ({H} heads, head_dim {hd}), vocab {V}, block {BS}; B={B} streams, "
                               f"{a.ctx} cached tokens + {a.steps} sampled"},
        "roofline": {"kernel": "decode step (graph replay) at the final context", "bound": "hbm",
                     "achieved": round((weight_bytes + kv_bytes) / (step_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS,
                     "unit": "GB/s", "step_ms": round(step_ms, 4), "step_ms_min_max": step_spread,
                     "weight_bytes": weight_bytes, "kv_bytes": kv_bytes,
                     "traffic": None},
        "kv_cache_gb": round(m.cache_bytes() / 2**30, 2),
        "prefill_ms": round(t_prefill * 1e3, 2),  # a.ctx prefix tokens (batched prefill) + 1 sampled token
    }
    out_json["roofline"]["frac"] = round(out_json["roofline"]["achieved"] / PEAK_HBM_GBS, 4)
    try:  # memory-side traffic of one step from the committed PMC pass (default model shape, B = 1 only)
        pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["lm_step_b1"]
        if (V, BS, L, H, C, B) == (8192, 5120, 24, 16, 1536, 1):
            out_json["roofline"]["traffic"] = pmc["read_bytes"] + pmc["write_bytes"]
            out_json["roofline"]["traffic_source"] = pmc["source"]
    except Exception:
        pass
    for B8 in ([int(b) for b in a.also.split(",")] if B == 1 and not a.no_also else []):
        # the same model with 8 (--also) streams sampled together (one pass over the weights per step serves all of them)
        n8 = min(a.steps, 128)
        cond8 = torch.randint(0, V, (B8, 1 + a.ctx), generator=g).cuda()
        og.sample_with_past(cond8, m, 8, top_k=2048, top_p=0.9, use_graph=not a.no_graph)
        torch.cuda.synchronize()
        t8 = time.perf_counter()
        og.sample_with_past(cond8, m, n8, top_k=2048, top_p=0.9, use_graph=not a.no_graph)
        torch.cuda.synchronize()
        dt8 = time.perf_counter() - t8
        t9 = time.perf_counter()   # the prefill of the ctx prefix is inside dt8: measure it alone (+ 1 token) and subtract
        og.sample_with_past(cond8, m, 1, top_k=2048, top_p=0.9, use_graph=not a.no_graph)
        torch.cuda.synchronize()
        dt8 = max(dt8 - (time.perf_counter() - t9), 1e-9)
        # the bare decode step of the 8 streams at the final context
        _, _, replay8 = m.graph_step(B8)
        torch.cuda.synchronize()
        step8, spread8 = time_step(replay8, B8, a.ctx + n8)
        kv8 = 2.0 * L * B8 * H * (a.ctx + n8) * hd * kv_elem
        out_json.setdefault("also", {})[f"b{B8}"] = {"batch_streams": B8, "steps": n8, "tokens_s": round(B8 * n8 / dt8, 1),
                                   "ms_per_token_step": round(dt8 / n8 * 1e3, 4), "step_ms": round(step8, 4),
                                                     "step_ms_min_max": spread8, "kv_bytes": kv8,
                                                     "frac_hbm": round((weight_bytes + kv8) / (step8 * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
    if not a.no_cpu_baseline:
        from oracle import gpt_oracle as go  # the CPU oracle is only the baseline / checker here
        torch.set_num_threads(min(32, os.cpu_count() or 1))
        x = cond.cpu()[:1, -1:]
        with torch.no_grad():
            _, cache = go.forward_with_past(sd, cond.cpu()[:1, :min(1 + a.ctx, 64)], H, None)
            n, spent = 0, 0.0
            while n < 3 or (spent < 15.0 and n < 200):
                t = time.perf_counter()
                lg, cache = go.forward_with_past(sd, x, H, cache, position=cache[0][0].shape[2])
                spent += time.perf_counter() - t
                n += 1
        out_json["cpu_baseline"] = {"value": round(n / spent, 2), "unit": "tokens/s", "cores": torch.get_num_threads(),
                                    "kind": "port", "sample": f"{n} KV-cached oracle steps (1 stream, context "
                                                              f"{cache[0][0].shape[2]}), torch CPU fp32"}
    print(json.dumps(out_json), flush=True)


if __name__ == "__main__":
    main()
