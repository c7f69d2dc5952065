"""GPU (-m gpu): bf16 / fp16 weight matrices in the LM decode step (omnitok_lm_set_weight_format, GPT.set_weight_format).

"W rounded" below is what a 16-bit engine computes with: `rounded(sd, fmt)` applies .to(fmt).float() on the CPU to the five matrix
families a step streams (q/k/v, proj, mlp.0, mlp.2, head) and leaves every other tensor alone.  The rounded weights are exact in
fp32, so every tolerance is the fp32 path's own: LOGIT_TOL for whole-model logits, test_gemv's 2e-5 sqrt(K / 1536) for one GEMV."""
import argparse
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import gpt_oracle as go
from tests import error_bounds as eb
from tests import lm_validation_bounds as lb
from tests.test_gpu_lm import LOGIT_TOL, rnd
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu
FMT = {"bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
MATRICES = (".attn.key.weight", ".attn.query.weight", ".attn.value.weight", ".attn.proj.weight", ".mlp.0.weight", ".mlp.2.weight")


def rounded(sd, fmt):
    dt = FMT[fmt][1]
    return {k: (v.to(dt).float() if k == "head.weight" or k.endswith(MATRICES) else v) for k, v in sd.items()}


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib
    return _lib.load()


def make_gpt(sd, dims, fmt="fp32"):
    from omnitokenizer_amd.gpt import GPT
    V, BS, L, H, C = dims
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.cuda().eval().set_weight_format(fmt)


# ---- kernel level ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def gemv_weights(N, K, fmt):
    """test_gemv's weight matrix, rounded by torch: (packed 16-bit tensor on the device, its fp32 values on the host)"""
    w16 = rnd(N, K, seed=2, scale=0.05).to(FMT[fmt][1])
    return w16.cuda(), w16.float()


@pytest.mark.parametrize("B", [1, 2, 3, 5, 8, 11])
@pytest.mark.parametrize("N,K", [(1536, 1536), (1000, 1536), (1536, 6144), (2048, 2048), (1000, 8192), (20000, 1536), (300, 256),
                                 (8193, 768)])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_gemv_w16(lib, fmt, N, K, B):
    """omnitok_lm_gemv_w16 against F.linear on the rounded weights in the three forms of test_gemv: every K-sliced configuration
    (K = 1536 / 2048: one chunk per wave, 6144 / 8192: four), the ragged row split (N = 1000), more than one workgroup per CU
    (N = 20000), and the row kernel with odd N; groups of 8 / 4 / 2 / 1 streams."""
    x, bias, res = rnd(B, K, seed=1), rnd(N, seed=3), rnd(B, N, seed=4)
    g, beta = rnd(K, seed=5, scale=0.1) + 1.0, rnd(K, seed=6, scale=0.1)
    wd, w = gemv_weights(N, K, fmt)
    f = FMT[fmt][0]
    s = torch.cuda.current_stream().cuda_stream
    xd, bd, rd, gd, betad = (t.cuda() for t in (x, bias, res, g, beta))
    tol = 2e-5 * math.sqrt(K / 1536)
    y = torch.empty(B, N, device="cuda")
    assert lib.omnitok_lm_gemv_w16(_p(xd), _p(wd), f, _p(bd), None, None, None, _p(y), B, N, K, 0, s) == 0
    e0 = (y.cpu() - F.linear(x, w, bias)).abs().max().item()
    assert lib.omnitok_lm_gemv_w16(_p(xd), _p(wd), f, _p(bd), None, _p(gd), _p(betad), _p(y), B, N, K, 1, s) == 0
    e1 = (y.cpu() - F.gelu(F.linear(F.layer_norm(x, (K,), g, beta), w, bias))).abs().max().item()
    y = rd.clone()
    assert lib.omnitok_lm_gemv_w16(_p(xd), _p(wd), f, None, _p(y), None, None, _p(y), B, N, K, 0, s) == 0
    e2 = (y.cpu() - (F.linear(x, w) + res)).abs().max().item()
    print(f"{fmt} B {B} N {N} K {K}: plain {e0:.2e} ln+gelu {e1:.2e} residual {e2:.2e} (tol {tol:.2e})")
    assert e0 < tol and e1 < tol and e2 < tol


def test_gemv_w16_fp16_subnormal_weights(lib):
    """Weights at scale 1e-6: most are fp16 subnormals (below 2^-14 = 6.1e-5).  The outputs are ~1e-5, under test_gemv's absolute
    tolerance whatever the kernel does, so the bar here is the forward bound of an fp32 dot product of K fused terms in any order,
    |y - y64| <= gamma(K + 1) sum_k |x_k w_k| (Higham, Accuracy and Stability, (3.5); + 1 for the bias add): ~1e-9 against the
    ~1e-5 a flushed subnormal would cost."""
    N, K, B = 300, 256, 5
    w16 = rnd(N, K, seed=2, scale=1e-6).to(torch.float16)
    w = w16.float()
    sub = (w.abs() < 2.0 ** -14) & (w != 0)
    assert float(sub.float().mean()) > 0.9
    x, bias = rnd(B, K, seed=1), rnd(N, seed=3, scale=1e-5)
    y = torch.empty(B, N, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert lib.omnitok_lm_gemv_w16(_p(x.cuda()), _p(w16.cuda()), 2, _p(bias.cuda()), None, None, None, _p(y), B, N, K, 0, s) == 0
    y64 = F.linear(x.double(), w.double(), bias.double())
    bar = eb.gamma(K + 1) * (F.linear(x.double().abs(), w.double().abs()) + bias.double().abs())
    err = (y.cpu().double() - y64).abs()
    print(f"fp16 subnormal weights: max err {float(err.max()):.2e}, smallest bar {float(bar.min()):.2e}, |y| up to {float(y64.abs().max()):.2e}")
    assert (err <= bar).all()


@pytest.mark.parametrize("fmt,N,K,scale", [("bf16", 300, 256, 0.05), ("bf16", 1536, 1536, 0.05), ("bf16", 1000, 6144, 0.05),
                                           ("fp16", 300, 256, 1e-6), ("fp16", 1536, 1536, 0.05), ("fp16", 1536, 1536, 1e-6),
                                           ("fp16", 1000, 6144, 1e-6)])
def test_gemv_w16_one_hot_is_exact(lib, fmt, N, K, scale):
    """x one-hot at column k: y[:, n] must EQUAL the rounded weight w[n, k] -- no summation, so the widening is checked exactly, for
    every column (both halves of a dword, every lane, every wave slice) of the row kernel (K = 256) and the K-sliced kernel (one
    and four chunks per wave); scale 1e-6: fp16 subnormals through each of them.
    Covered: the widening of torch-rounded bits (the packed tensor here is torch's).  NOT covered here: the packed image that
    lm_round_w16_kernel writes -- no entry point exports it.  Its fp32 write-back is compared bit for bit in
    test_rounding_is_torchs and the packed halves come from the same values, but the packed image itself is only seen through the
    stepped logits (test_decode_reads_the_rounded_values, test_ksliced_path_in_the_engine, within LOGIT_TOL)."""
    w16 = rnd(N, K, seed=2, scale=scale).to(FMT[fmt][1])
    wd, want = w16.cuda(), w16.cuda().float().t().contiguous()    # want[k, n] = w[n, k]
    eye = torch.eye(K, device="cuda")
    y = torch.empty(K, N, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for k0 in range(0, K, 8):   # 8 streams per call, stream b one-hot at column k0 + b
        assert lib.omnitok_lm_gemv_w16(_p(eye[k0:k0 + 8]), _p(wd), FMT[fmt][0], None, None, None, None, _p(y[k0:k0 + 8]), 8, N, K,
                                       0, s) == 0
    assert torch.equal(y, want)
    assert float((want != 0).float().mean()) > 0.95


# ---- engine level: the golden models (row kernel) ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    """per (golden model, format), computed once: the 16-bit engine on sd, the fp32 engine on rounded(sd), and -- in the shape of
    test_prefill_equals_steps -- stepped and prefilled logits of both, the fp32 engine's on the unrounded sd, and the oracle's."""
    cache, plain = {}, {}

    def run(m, idx, nxt, T):
        m.reset_streams(3, T + 4)
        stepped = torch.stack([m.step(idx[:, t].contiguous()) for t in range(T)], 1)
        after_steps = m.step(nxt)
        m.reset_streams(3, T + 4)
        batched = m.prefill(idx, want_logits=True)
        after_prefill = m.step(nxt)
        return dict(stepped=stepped, after_steps=after_steps, batched=batched, after_prefill=after_prefill)

    def get(name, fmt):
        if (name, fmt) not in cache:
            g, sd, dims = load_gpt_case(name)
            V, BS, L, H, C = dims
            T = min(BS - 2, 40)
            idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11)).cuda()
            nxt = torch.randint(0, V, (3,), generator=torch.Generator().manual_seed(12)).cuda()
            if name not in plain:
                plain[name] = run(make_gpt(sd, dims), idx, nxt, T)
            rsd = rounded(sd, fmt)
            m16, m32r = make_gpt(sd, dims, fmt), make_gpt(rsd, dims)
            ref = go.forward(rsd, torch.cat([idx.cpu(), nxt.cpu()[:, None]], 1), H)
            cache[name, fmt] = dict(g=g, sd=sd, rsd=rsd, H=H, T=T, idx=idx, nxt=nxt, m16=m16, w16=run(m16, idx, nxt, T),
                                    w32r=run(m32r, idx, nxt, T), w32=plain[name], ref=ref)
        return cache[name, fmt]
    return get


def dmax(a, b):
    return (a.cpu() - b.cpu()).abs().max().item()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", GPT_CASES)
def test_rounding_is_torchs(cases, name, fmt):
    """Prefill logits of a 16-bit engine loaded with sd are BIT-equal to those of an fp32 engine loaded with rounded(sd): the same
    GEMM on the same values -- the device rounding gives torch's bits in every matrix, the concatenated q/k/v included."""
    c = cases(name, fmt)
    assert c["m16"].weight_format == fmt
    assert torch.equal(c["w16"]["batched"], c["w32r"]["batched"])


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", GPT_CASES)
def test_decode_reads_the_rounded_values(cases, name, fmt):
    c = cases(name, fmt)
    a, T = c["w16"], c["T"]
    errs = {"own prefill": max(dmax(a["stepped"], a["batched"]), dmax(a["after_steps"], a["after_prefill"])),
            "oracle on rounded": max(dmax(a["stepped"], c["ref"][:, :T]), dmax(a["after_steps"], c["ref"][:, T])),
            "stepped fp32 engine on rounded": max(dmax(a["stepped"], c["w32r"]["stepped"]),
                                                  dmax(a["after_steps"], c["w32r"]["after_steps"]))}
    live = dmax(a["stepped"], c["w32"]["stepped"])
    print(f"{name} {fmt}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"; vs fp32 on unrounded weights {live:.2e}")
    for k, v in errs.items():
        assert v < LOGIT_TOL, k
    # the feature is live: the rounding moves the logits by more than the tolerance
    assert live > LOGIT_TOL


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", GPT_CASES)
def test_greedy_sampling_is_token_equal(cases, name, fmt):
    from omnitokenizer_amd import gpt as og
    c = cases(name, fmt)
    x = torch.from_numpy(c["g"]["idx"])[:, :4]
    ref_tok, ref_logits = go.sample_with_past(c["rsd"], x, c["H"], 10, sample_logits=False, return_logits=True)
    top2 = ref_logits.topk(2, -1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    print(f"{name} {fmt}: smallest top-1 / top-2 gap of the oracle {gap:.2e}")
    assert gap > 2 * LOGIT_TOL   # precondition: no argmax within the logits' tolerance of a tie
    for use_graph in (False, True):
        tok = og.sample_with_past(x.cuda(), c["m16"], 10, sample_logits=False, use_graph=use_graph)
        assert torch.equal(tok.cpu(), ref_tok), f"greedy tokens differ (graph={use_graph})"


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", GPT_CASES)
def test_token_losses_equal_cross_entropy_of_prefill_logits(cases, name, fmt):
    """omnitok_lm_prefill_loss at R >= B * T on a 16-bit engine: every output equals token_cross_entropy on that engine's prefill
    logits bit for bit (both read the rounded fp32 image through the same GEMM)."""
    from omnitokenizer_amd import lm_losses as ll
    c = cases(name, fmt)
    m, idx = c["m16"], c["idx"]
    tg = torch.randint(0, m.vocab_size, tuple(idx.shape), generator=torch.Generator().manual_seed(13))
    tg[:, :2] = -1
    tg = tg.cuda()
    assert idx.numel() <= 2048
    want = ll.token_cross_entropy(c["w16"]["batched"], tg)
    out = m.token_losses(idx, tg)
    for k in want:
        assert torch.equal(out[k], want[k]), k


# ---- engine level: the K-sliced kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("C,H", [(1536, 16), (2048, 16)])
def test_ksliced_path_in_the_engine(C, H, fmt):
    """The golden models only reach the row kernel: a 1-layer model at n_embd 1536 / 2048 runs the K-sliced 16-bit kernels inside the
    step -- the attention merge in the proj GEMV's prologue, one and four chunks per wave, groups of 8 / 2 + 1 / 1 streams --
    against the oracle on rounded weights."""
    V, BS, L = 300, 48, 1
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=23)
    rsd = rounded(sd, fmt)
    m = make_gpt(sd, (V, BS, L, H, C), fmt)
    idx = torch.randint(0, V, (8, 18), generator=torch.Generator().manual_seed(24))
    ref = go.forward(rsd, idx, H)     # streams are independent: the first B rows serve every B
    for B in (1, 3, 8):
        xb = idx[:B].cuda()
        m.reset_streams(B, 20)
        lg = [m.prefill(xb[:, :12].contiguous(), want_logits=True)]
        lg += [m.step(xb[:, t].contiguous())[:, None] for t in range(12, 18)]
        err = dmax(torch.cat(lg, 1), ref[:B])
        print(f"C {C} {fmt} B {B}: {err:.2e}")
        assert err < LOGIT_TOL


# ---- range, switching, Net2NetTransformer -------------------------------------------------------------------------------------
SMALL = (300, 48, 1, 4, 256)


def test_fp16_overflow_is_refused_by_name():
    V, BS, L, H, C = SMALL
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=25)
    sd["blocks.0.mlp.0.weight"][5, 7] = 1e5
    m = make_gpt(sd, SMALL, "fp16")
    with pytest.raises(ValueError, match=r"blocks\.0\.mlp\.0\.weight"):
        m._sync_engine()
    idx = torch.randint(0, V, (2, 20), generator=torch.Generator().manual_seed(26)).cuda()
    # the refused engine holds half-rounded images: the C ABI takes no finalize in another format until the weights are set again
    from omnitokenizer_amd import _lib
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    assert lib.omnitok_lm_set_weight_format(m._engine, FMT["bf16"][0]) == 0
    assert lib.omnitok_lm_finalize(m._engine, stream) != 0 and b"released by a previous finalize" in lib.omnitok_last_error()
    with pytest.raises(ValueError, match=r"blocks\.0\.mlp\.0\.weight"):   # ... and it stays refused: nothing half-loaded runs
        m(idx)
    logits, _ = m.set_weight_format("bf16")(idx)
    assert torch.isfinite(logits).all()
    want, _ = make_gpt(rounded(sd, "bf16"), SMALL)(idx)
    assert torch.equal(logits, want)


def test_switching_formats_leaves_the_parameters_alone():
    from omnitokenizer_amd import gpt as og
    V, BS, L, H, C = SMALL
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=27)
    m = make_gpt(sd, SMALL)
    idx = torch.randint(0, V, (2, 20), generator=torch.Generator().manual_seed(28)).cuda()
    runs = []
    for fmt in ("fp32", "bf16", "fp32"):
        assert m.set_weight_format(fmt) is m
        logits, _ = m(idx)
        tok, lg = og.sample_with_past(idx[:, :4], m, 6, sample_logits=False, use_graph=True, return_logits=True)
        runs.append((logits.clone(), tok.clone(), lg.clone()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))
    assert dmax(runs[0][0], runs[1][0]) > LOGIT_TOL and not torch.equal(runs[0][2], runs[1][2])
    for k, v in m.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v.cpu(), sd[k]), k


def test_net2net_validation_step_in_bf16():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
    from omnitokenizer_amd.config import OmniTokConfig
    from omnitokenizer_amd.lm_transformer import Net2NetTransformer
    targs = make_args(2, resolution=64)
    cfg = OmniTokConfig.from_args(targs)
    tok = OmniTokenizer_VQGAN(targs)
    tok.load_state_dict(synth.synth_state_dict(cfg, seed=0), strict=True)
    n_cls, L, H, C = 10, 2, 4, 256
    args = argparse.Namespace(class_cond_dim=n_cls, unconditional=False, vtokens=False, block_size=80, n_layer=L, n_head=H, n_embd=C,
                              vtokens_pos=False, n_unmasked=0, starts_with_sos=False, class_first=False, lm_weight_format="bf16")
    net = Net2NetTransformer(args, first_stage_model=tok, first_stage_key="video", cond_stage_key="label")
    assert net.transformer.weight_format == "bf16"
    V = net.transformer.vocab_size
    gsd = go.synth_gpt_state(V, 80, L, H, C, seed=6)
    net.load_state_dict({f"transformer.{k}": v for k, v in gsd.items()}, strict=True)
    net = net.cuda().eval()
    batch = {"video": synth.synth_image(2, 64, seed=21).cuda(), "label": torch.tensor([3, 7]).cuda()}
    out = net.validation_step(batch, 0)
    assert net.transformer.weight_format == "bf16" and set(out) == {"val/loss", "val/acc1", "val/acc5"}
    # the oracle on rounded weights over the same teacher-forced sequence
    cz, z, prefix = net._teacher_forced_sequence(*net.get_xc(batch))
    ref = go.forward(rounded(gsd, "bf16"), cz[:, :-1].cpu(), H)[:, prefix:].reshape(-1, V)
    tflat = z.reshape(-1).cpu().long()
    loss64 = float(lb.nll64(ref, tflat).mean())
    bar = lb.loss_bar(lb.nll_bar(ref, tflat), tflat, loss64) + LOGIT_TOL   # (test_token_losses_vs_reference_golden's)
    plain = float(lb.nll64(go.forward(gsd, cz[:, :-1].cpu(), H)[:, prefix:].reshape(-1, V), tflat).mean())
    print(f"val/loss {float(out['val/loss']):.6f} vs oracle on rounded weights {loss64:.6f} (bar {bar:.2e}); on fp32 weights {plain:.6f}")
    assert abs(float(out["val/loss"]) - loss64) <= bar
