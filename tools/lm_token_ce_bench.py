"""Times the LM validation kernels on the GPU (device events, alternating arms, medians of repeated windows):

  token_ce            omnitok_lm_token_ce on [N, V] fp32 logits, whole op (three launches + output allocations): once on ONE
                      tensor (re-read from the Infinity Cache when it fits) and once rotating over enough copies to exceed
                      the 256 MB cache several times, so that every read comes from HBM; only the second is set against the
                      8 TB/s HBM peak
  torch               F.cross_entropy + topk(5) on the same logits (what the reference's shared_step runs)
  token_losses        GPT.token_losses at lm_loss_chunk_rows = R against R >= B * T (one head GEMM), on a synthetic LM

    python tools/lm_token_ce_bench.py [--rows 5120] [--vocab 9217] [--out profiles/lm_token_ce.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def alternate(arms, iters, reps):
    """{name: [seconds per call, one per window]}: the arms take turns, `reps` windows each"""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            out[k].append(window(fn, iters))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5120)
    ap.add_argument("--vocab", type=int, default=9217)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lm", default="1,5120,9217,4,8,512", help="B,T,V,layers,heads,n_embd of the token_losses arm")
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    from omnitokenizer_amd import _lib, lm_losses
    from omnitokenizer_amd.gpt import GPT
    from oracle import gpt_oracle as go
    lines = [f"device {torch.cuda.get_device_name(0)}; medians of {a.reps} windows (min .. max), arms alternating"]
    N, V = a.rows, a.vocab
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(N, V, generator=g) * 3).cuda()
    tg = torch.randint(0, V, (N,), generator=g).cuda()
    # same results first
    out = lm_losses.token_cross_entropy(logits, tg)
    ref = F.cross_entropy(logits.double(), tg)
    top5 = logits.topk(5, -1).indices
    lines.append(f"N {N} V {V}: loss {float(out['loss']):.7f} (fp64 torch {float(ref):.7f}); acc5 {out['acc5'].item():.4f} "
                 f"(torch topk {100.0 * float((top5 == tg[:, None]).any(-1).sum()) / N:.4f})")

    def torch_arm():
        F.cross_entropy(logits, tg)
        logits.topk(5, 1, True, True)

    nbytes = N * V * 4
    ncopy = max(2, -(-4 * (256 << 20) // nbytes))       # at least 1 GiB in rotation
    copies = [logits] + [logits.clone() for _ in range(ncopy - 1)]
    turn = [0]

    def cold_arm():
        turn[0] = (turn[0] + 1) % ncopy
        torch.ops.omnitok.token_ce(copies[turn[0]], tg)

    def torch_cold_arm():
        turn[0] = (turn[0] + 1) % ncopy
        F.cross_entropy(copies[turn[0]], tg)
        copies[turn[0]].topk(5, 1, True, True)

    t = alternate({"token_ce, one tensor": lambda: torch.ops.omnitok.token_ce(logits, tg),
                   f"token_ce, {ncopy} tensors in turn": cold_arm, "torch ce + topk(5), one tensor": torch_arm,
                   f"torch ce + topk(5), {ncopy} in turn": torch_cold_arm}, a.iters, a.reps)
    for k, v in t.items():
        med = statistics.median(v)
        extra = ""
        if k.startswith("token_ce, one"):
            extra = f"; {nbytes / med / 1e12:.2f} TB/s of logits read ({nbytes / 1e6:.0f} MB: from the Infinity Cache, not an HBM figure)"
        elif k.startswith("token_ce"):
            extra = f"; {nbytes / med / 1e12:.2f} TB/s of logits read from HBM ({ncopy * nbytes / 1e6:.0f} MB in rotation) = " \
                    f"{100 * nbytes / med / HBM_PEAK:.0f} % of the 8 TB/s peak, whole op"
        lines.append(f"  {k:36s} {med * 1e6:9.1f} us ({min(v) * 1e6:.1f} .. {max(v) * 1e6:.1f}){extra}")
    lines.append("  (the op allocates its outputs and a 128 KiB workspace and launches 3 kernels per call)")
    # token_losses: blocks of R rows against one head GEMM
    B, T, Vl, L, H, C = (int(x) for x in a.lm.split(","))
    m = GPT(argparse.Namespace(), Vl, T + 1, n_layer=L, n_head=H, n_embd=C)
    m.load_state_dict(go.synth_gpt_state(Vl, T + 1, L, H, C, seed=3), strict=True)
    m = m.cuda().eval()
    idx = torch.randint(0, Vl, (B, T), generator=g).cuda()
    tgl = torch.randint(0, Vl, (B, T), generator=g).cuda()
    before = _lib.get_option("lm_loss_chunk_rows")

    def arm(R):
        def f():
            _lib.set_option("lm_loss_chunk_rows", R)
            m.token_losses(idx, tgl)
        return f

    def logits_arm():
        lg, _ = m(idx)
        F.cross_entropy(lg.view(-1, Vl), tgl.view(-1))
        lg.view(-1, Vl).topk(5, 1, True, True)
    try:
        t = alternate({f"token_losses R={a.chunk}": arm(a.chunk), f"token_losses R={B * T} (one GEMM)": arm(B * T),
                       "forward + torch ce + topk(5)": logits_arm}, max(a.iters // 20, 3), a.reps)
    finally:
        _lib.set_option("lm_loss_chunk_rows", before)
    lines.append(f"LM B {B} T {T} V {Vl} layers {L} heads {H} n_embd {C} (whole call, host synchronisation included):")
    for k, v in t.items():
        lines.append(f"  {k:34s} {statistics.median(v) * 1e3:9.3f} ms ({min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
