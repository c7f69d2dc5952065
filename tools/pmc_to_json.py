#!/usr/bin/env python
"""Builds profiles/pmc_traffic.json -- the counter-derived fields bench.py prints next to its live HIP-event
numbers -- from the per-kernel summaries of three rocprofv3 --pmc passes (tools/pmc_collect.sh):

    python tools/pmc_to_json.py <FETCH_SIZE.csv> <WRITE_SIZE.csv> <SQ_VALU_MFMA_BUSY_CYCLES.csv> <tag> > pmc_traffic.json

FETCH_SIZE / WRITE_SIZE are KB per dispatch; on gfx950 FETCH_SIZE counts half of the bytes of wide coalesced reads
(MI355X_MICROARCH.md, HBM section): x2.  Matrix-pipe busy = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x
1024 SIMDs).  The file is stamped with the sha256 of omnitokenizer_amd/csrc (tools/pmc_to_json.py csrc_digest):
bench.py prints the fields only when the stamp matches the sources the loaded library was built from."""
import csv
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bench.py family -> substrings that identify its kernel in the rocprofv3 kernel names (pmc_summary.short())
FAMILIES = {
    "gemm_ff_in": ["gemm_pl_kernel<1,"],          # GEGLU epilogue: FF-in only
    "gemm_out": ["gemm_pl_kernel<2,"],            # full-row residual + LayerNorm epilogue: the out-projections
    "gemm_qk_pack": ["gemm_pl_kernel<4,"],        # spatial and window q|k launches (packed Q / K)
    "gemm_v_pack": ["gemm_pl_kernel<3,"],         # spatial and window v launches (packed V)
    "gemm_pixels": ["gemm_pl_kernel<5,"],         # to_pixels with the un-patchify store
    "gemm_t_scores": ["gemm_plt_kernel<6>", "gemm_pl_kernel<6,"],       # fused temporal stage, launch 1: q|k GEMM -> softmax weights (r05)
    "gemm_t_pv": ["gemm_plt_kernel<7>", "gemm_pl_kernel<7,"],           # fused temporal stage, launch 2: V GEMM -> attention output planes (r05)
    # the fp32 epilogue serves FF-out (16 launches, K = 1408) AND the temporal / window q|k|v launches (10, K = 512): one
    # kernel name, so the counters cannot be split per family -- reported under its own key, not as gemm_ff_out
    "gemm_f32_epilogue_mixed": ["gemm_pl_kernel<0,"],
    "attn_spatial": ["attn_spatial_h2w_kernel", "attn_spatial_h2x_kernel"],   # default: h2w
    "attn_temporal": ["attn_temporal_reg"],
    "attn_window": ["attn_window_h2_kernel", "attn_window_kernel"],
    "vq_argmin": ["vq_screen_kernel", "vq_argmin_kernel"],   # r05 default: the screened search
    "peg3d": ["peg3d_wide_kernel", "peg2d_wide_kernel", "peg3d_lds_kernel"],   # r04: the 64-channel kernel at C3 (5 planes)
    "pre_vq": ["layernorm_prevq_kernel", "pre_vq_kernel"],
    "stats_pack": ["stats_pack_kernel"],
}


def csrc_digest(root=ROOT):
    d = os.path.join(root, "omnitokenizer_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h", ".cpp")):
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()


def load(path):
    return list(csv.DictReader(open(path)))


def pick(rows, pats, col):
    """dispatch-weighted mean of `col` over the kernels matching a family"""
    num = den = 0.0
    for r in rows:
        if any(p in r["kernel"] for p in pats) and r.get(col) not in (None, "", "nan"):
            n = float(r["dispatches"])
            num += float(r[col]) * n
            den += n
    return num / den if den else None


def main():
    fetch, write, mfma, tag = load(sys.argv[1]), load(sys.argv[2]), load(sys.argv[3]), sys.argv[4]
    fam = {}
    for name, pats in FAMILIES.items():
        rd, wr = pick(fetch, pats, "mean_FETCH_SIZE"), pick(write, pats, "mean_WRITE_SIZE")
        busy, act = pick(mfma, pats, "mean_SQ_VALU_MFMA_BUSY_CYCLES"), pick(mfma, pats, "mean_GRBM_GUI_ACTIVE")
        if rd is None and busy is None:
            continue
        e = {}
        if rd is not None and wr is not None:
            e.update(read_bytes=round(rd * 1024 * 2), write_bytes=round(wr * 1024),
                     source=f"profiles/{tag}_pmc_FETCH_SIZE.csv / {tag}_pmc_WRITE_SIZE.csv (rocprofv3 --pmc FETCH_SIZE and "
                            "--pmc WRITE_SIZE in separate passes of `bench.py --steps 1`, KB per dispatch, FETCH x2 gfx950 "
                            "correction, WRITE_SIZE uncalibrated)")
        if busy is not None and act:
            e.update(mfma_busy_pct=round(100.0 * busy / (act / 8.0 * 1024.0), 1),
                     mfma_source=f"profiles/{tag}_pmc_SQ_VALU_MFMA_BUSY_CYCLES.csv (SQ_VALU_MFMA_BUSY_CYCLES / "
                                 "(GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs))")
            wc = pick(mfma, pats, "mean_SQ_WAVE_CYCLES")
            if wc:
                for c in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"):
                    v = pick(mfma, pats, "mean_" + c)
                    if v is not None:
                        e[c.lower() + "_frac_of_wave_cycles"] = round(v / wc, 3)
        fam[name] = e
    try:
        head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except Exception:
        head = None
    out = {"stamp": {"csrc_sha256": csrc_digest(), "git_head": head, "tag": tag,
                     "note": "bench.py nulls the counter-derived fields when csrc_sha256 differs from the tree it runs in"},
           "gemm_mode_2": fam,
           "power_limit_evidence": {
               "source": "profiles/r03_gemm_limiter_probe.txt",
               "reading": "the board sits at its 1400 W cap: removing every stall of the plane GEMM (barrier + DMA wait) cuts its "
                          "cycles by 20 % and the clock drops by 18 % -- same wall time; what raises the rate is less data moved "
                          "per flop",
               "ff_in_tflops": {"plane_gemm": 352, "no_barrier_no_wait": 354, "no_l2_to_lds_traffic": 414,
                                "no_traffic_no_barrier": 424, "h2_fp32_operand": 330, "h2_fused_layernorm_r02": 300},
               "mfma_stream_only_tflops": 424}}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "csrc_digest":
        print(csrc_digest())
    else:
        main()
