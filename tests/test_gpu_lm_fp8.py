"""GPU (-m gpu): weight-only fp8 (e4m3fn, one power-of-two scale per output row) in the LM decode step of up to 16 streams
(omnitok_lm_set_decode_quant, GPT.set_decode_quant; the contract: include/omnitok_lm.h).

The restatement is torch's on the CPU: omnitokenizer_amd.gpt.fp8_quantize_rows (the scale rule and .to(torch.float8_e4m3fn)) and
fp8_dequantized (the state dict with the five matrix families replaced by s * q), itself held to a scalar loop in
tests/test_lm_fp8_abi.py.  s * q is exact in fp32 and so is the scaling of a finished sum by a power of two, so an fp8 step is an
fp32 dot product with the values s * q in some order and every tolerance below is the fp32 path's own: LOGIT_TOL for whole-model
logits, test_gemv's 2e-5 sqrt(K / 1536) for one GEMV (weights of the same magnitude, scale 0.05)."""
import argparse
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import gpt_oracle as go
from tests.test_gpu_lm import LOGIT_TOL, rnd
from tests.test_lm_fp8_abi import boundary_rows
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib
    return _lib.load()


def quantize(w):
    """torch's restatement: (codes uint8 [N, K], scales fp32 [N], s * q fp32 [N, K]), on the CPU"""
    from omnitokenizer_amd.gpt import fp8_quantize_rows
    q, s = fp8_quantize_rows(w)
    return q.view(torch.uint8), s, q.float() * s[:, None]


def make_gpt(sd, dims, quant="none", fmt="fp32", kv="fp32"):
    from omnitokenizer_amd.gpt import GPT
    V, BS, L, H, C = dims
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.cuda().eval().set_weight_format(fmt).set_cache_format(kv).set_decode_quant(quant)


def dmax(a, b):
    return (a.cpu() - b.cpu()).abs().max().item()


# ---- the quantiser -----------------------------------------------------------------------------------------------------------------
def device_quantize(lib, w):
    wd = w.cuda()
    N, K = w.shape
    q = torch.full((N, K), 0x55, dtype=torch.uint8, device="cuda")
    s = torch.full((N,), -1.0, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.omnitok_lm_quantize_fp8(_p(wd), _p(q), _p(s), N, K, _p(flag), torch.cuda.current_stream().cuda_stream) == 0
    return q.cpu(), s.cpu(), int(flag.item())


def test_quantizer_is_torchs(lib):
    """Byte-equal and scale-equal to torch on rows at every boundary of the rule and of the format (tests/test_lm_fp8_abi.py,
    boundary_rows: an all-zero row, amax exactly 448 2^e and one ulp above, m exactly 0.875 and one ulp above, rounding ties,
    subnormal results down to half the smallest one, -0.0, scales up to 220 octaves apart, fp32 subnormals and fp32's maximum),
    then on rows long enough for every thread of the row's workgroup to loop (K = 1536, 6144), scaled over 40 octaves."""
    names, w = boundary_rows()
    big = [w]
    for K, seed in ((1536, 41), (6144, 42)):
        r = rnd(37, K, seed=seed) * torch.logspace(-6, 6, 37)[:, None]
        r[5, 7:900] = 0.0
        r[6] = 0.0
        big.append(r)
    for mat in big:
        codes, s, _ = quantize(mat)
        assert not ((codes & 0x7F) == 0x7F).any()        # the restatement itself never makes the NaN code (nothing saturates)
        q, sc, flag = device_quantize(lib, mat)
        assert flag == 0
        bad = (sc != s).nonzero().flatten().tolist()
        assert not bad, f"scales differ in rows {[names[i] if mat is w else i for i in bad]}"
        bad = (q != codes).any(1).nonzero().flatten().tolist()
        assert not bad, f"codes differ in rows {[names[i] if mat is w else i for i in bad]}"


@pytest.mark.parametrize("what", ["nan", "inf", "-inf"])
def test_quantizer_flags_non_finite_rows(lib, what):
    """A NaN or an infinity raises the flag; the finite rows of the same call are still torch's bytes."""
    w = rnd(9, 512, seed=43)
    codes, s, _ = quantize(w)
    w[4, 300] = float(what)
    q, sc, flag = device_quantize(lib, w)
    assert flag == 1
    keep = [r for r in range(9) if r != 4]
    assert torch.equal(q[keep], codes[keep]) and torch.equal(sc[keep], s[keep])


# ---- the GEMV ------------------------------------------------------------------------------------------------------------------------
_weights = {}


def gemv_weights(N, K):
    """test_gemv's weight matrix, quantised by torch: (codes and scales on the device, s * q on the host), made once per shape"""
    if (N, K) not in _weights:
        codes, s, w = quantize(rnd(N, K, seed=2, scale=0.05))
        _weights[N, K] = (codes.cuda(), s.cuda(), w)
    return _weights[N, K]


@pytest.mark.parametrize("B", [1, 3, 8, 11])
@pytest.mark.parametrize("N,K", [(300, 256), (1536, 1536), (1000, 6144), (8193, 768)])
def test_gemv_fp8(lib, N, K, B):
    """omnitok_lm_gemv_fp8 against F.linear on s * q in the three forms of test_gemv_w16: the row kernel with odd N (K = 256, 768),
    both K-sliced configurations (one and four chunks per wave) and the ragged row split (N = 1000); groups of 8 / 2 / 1 streams."""
    x, bias, res = rnd(B, K, seed=1), rnd(N, seed=3), rnd(B, N, seed=4)
    g, beta = rnd(K, seed=5, scale=0.1) + 1.0, rnd(K, seed=6, scale=0.1)
    qd, sd, w = gemv_weights(N, K)
    s = torch.cuda.current_stream().cuda_stream
    xd, bd, rd, gd, betad = (t.cuda() for t in (x, bias, res, g, beta))
    tol = 2e-5 * math.sqrt(K / 1536)
    y = torch.empty(B, N, device="cuda")
    assert lib.omnitok_lm_gemv_fp8(_p(xd), _p(qd), _p(sd), _p(bd), None, None, None, _p(y), B, N, K, 0, s) == 0
    e0 = (y.cpu() - F.linear(x, w, bias)).abs().max().item()
    assert lib.omnitok_lm_gemv_fp8(_p(xd), _p(qd), _p(sd), _p(bd), None, _p(gd), _p(betad), _p(y), B, N, K, 1, s) == 0
    e1 = (y.cpu() - F.gelu(F.linear(F.layer_norm(x, (K,), g, beta), w, bias))).abs().max().item()
    y = rd.clone()
    assert lib.omnitok_lm_gemv_fp8(_p(xd), _p(qd), _p(sd), None, _p(y), None, None, _p(y), B, N, K, 0, s) == 0
    e2 = (y.cpu() - (F.linear(x, w) + res)).abs().max().item()
    print(f"fp8 B {B} N {N} K {K}: plain {e0:.2e} ln+gelu {e1:.2e} residual {e2:.2e} (tol {tol:.2e})")
    assert e0 < tol and e1 < tol and e2 < tol


def one_hot_columns(lib, qd, sd, N, K):
    """y[k, n] of the GEMV with x one-hot at column k, for every k: 8 streams per call"""
    eye = torch.eye(K, device="cuda")
    y = torch.empty(K, N, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for k0 in range(0, K, 8):
        assert lib.omnitok_lm_gemv_fp8(_p(eye[k0:k0 + 8]), _p(qd), _p(sd), None, None, None, None, _p(y[k0:k0 + 8]), 8, N, K, 0, s) == 0
    return y


@pytest.mark.parametrize("N,K", [(300, 256), (1536, 1536), (1000, 6144)])
def test_gemv_fp8_one_hot_is_exact(lib, N, K):
    """x one-hot at column k: y[:, n] must EQUAL s[n] float(q[n, k]) -- no rounding anywhere (the other terms are +0, the scale a
    power of two) -- for every column: every byte of a dword, every lane, every wave slice and the scale, in the row kernel
    (K = 256) and both K-sliced configurations, on rows whose magnitudes (and so scales) run over 17 octaves."""
    w = rnd(N, K, seed=2) * torch.pow(2.0, (torch.arange(N) % 17 - 8).float())[:, None]
    codes, s, want = quantize(w)
    assert len(set(s.tolist())) >= 17
    y = one_hot_columns(lib, codes.cuda(), s.cuda(), N, K)
    assert torch.equal(y.cpu(), want.t())
    assert float((want != 0).float().mean()) > 0.95


def test_gemv_fp8_widens_every_code(lib):
    """One K = 256 matrix made from bytes: dword d of the image holds the codes number d, d + 67, d + 134 and d + 201 (mod 254) of the
    254 non-NaN ones, so each code stands in every byte position, next to three other codes; checked by one-hot against torch's
    float8_e4m3fn -> float32, with a different power-of-two scale per row.  Subnormals and both zeros included (a -0 weight gives
    +0 -- it is added to +0 --, which compares equal)."""
    N, K = 16, 256
    allc = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
    assert allc.numel() == 254
    p = torch.arange(N * K)
    codes = allc[(p // 4 + 67 * (p % 4)) % 254].reshape(N, K)
    for byte in range(4):
        assert set(codes.reshape(-1, 4)[:, byte].tolist()) == set(allc.tolist())
    s = torch.pow(2.0, torch.arange(N).float() - 8)
    want = codes.view(torch.float8_e4m3fn).float() * s[:, None]
    assert torch.isfinite(want).all()
    y = one_hot_columns(lib, codes.cuda(), s.cuda(), N, K)
    assert torch.equal(y.cpu(), want.t())


# ---- the engine: the golden models (row kernel) -----------------------------------------------------------------------------------
def run(m, idx, nxt, T):
    m.reset_streams(3, T + 4)
    stepped = torch.stack([m.step(idx[:, t].contiguous()) for t in range(T)], 1)
    after_steps = m.step(nxt)
    m.reset_streams(3, T + 4)
    batched = m.prefill(idx, want_logits=True)
    after_prefill = m.step(nxt)
    return dict(stepped=stepped, after_steps=after_steps, batched=batched, after_prefill=after_prefill)


@pytest.fixture(scope="module")
def cases():
    """per golden model, computed once: the fp8 engine on sd, the fp32 engine on fp8_dequantized(sd), the fp32 engine on sd --
    stepped and prefilled logits of each -- and the oracle on fp8_dequantized(sd)."""
    from omnitokenizer_amd import fp8_dequantized
    cache = {}

    def get(name):
        if name not in cache:
            g, sd, dims = load_gpt_case(name)
            V, BS, L, H, C = dims
            T = min(BS - 2, 24)
            idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11)).cuda()
            nxt = torch.randint(0, V, (3,), generator=torch.Generator().manual_seed(12)).cuda()
            dsd = fp8_dequantized(sd)
            m8 = make_gpt(sd, dims, "fp8")
            ref = go.forward(dsd, torch.cat([idx.cpu(), nxt.cpu()[:, None]], 1), H)
            cache[name] = dict(g=g, sd=sd, dsd=dsd, dims=dims, T=T, idx=idx, nxt=nxt, m8=m8, q8=run(m8, idx, nxt, T),
                               w32d=run(make_gpt(dsd, dims), idx, nxt, T), w32=run(make_gpt(sd, dims), idx, nxt, T), ref=ref)
        return cache[name]
    return get


@pytest.mark.parametrize("name", GPT_CASES)
def test_steps_read_the_fp8_values(cases, name):
    c = cases(name)
    a, T = c["q8"], c["T"]
    assert c["m8"].decode_quant == "fp8" and c["m8"].weight_format == "fp32"
    errs = {"stepped fp32 engine on s*q": max(dmax(a["stepped"], c["w32d"]["stepped"]), dmax(a["after_steps"], c["w32d"]["after_steps"])),
            "oracle on s*q": max(dmax(a["stepped"], c["ref"][:, :T]), dmax(a["after_steps"], c["ref"][:, T]))}
    live = dmax(a["stepped"], c["w32"]["stepped"])
    print(f"{name} fp8: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"; vs fp32 on the unquantised weights {live:.2e}")
    for k, v in errs.items():
        assert v < LOGIT_TOL, k
    assert live > LOGIT_TOL      # the feature is live: the quantisation moves the logits by more than the tolerance


@pytest.mark.parametrize("name", GPT_CASES)
def test_prefill_is_untouched(cases, name):
    """The batched prefill keeps the weight format's arithmetic: BIT-equal logits with the switch on and off.  (The step after it
    reads the fp8 image over the prefill's cache: not the default engine's bits.)"""
    c = cases(name)
    assert torch.equal(c["q8"]["batched"], c["w32"]["batched"])
    assert not torch.equal(c["q8"]["after_prefill"], c["w32"]["after_prefill"])


def test_switching_back_restores_the_default_bits(cases):
    c = cases(GPT_CASES[0])
    m = make_gpt(c["sd"], c["dims"], "fp8")
    first = run(m, c["idx"], c["nxt"], c["T"])
    assert torch.equal(first["stepped"], c["q8"]["stepped"])
    assert m.set_decode_quant("none") is m and m.decode_quant == "none"
    again = run(m, c["idx"], c["nxt"], c["T"])
    for k, v in c["w32"].items():
        assert torch.equal(again[k], v), k
    for k, v in m.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v.cpu(), c["sd"][k]), k


@pytest.mark.parametrize("name", GPT_CASES)
def test_graph_capture_equals_eager(cases, name):
    from omnitokenizer_amd import gpt as og
    c = cases(name)
    x = torch.from_numpy(c["g"]["idx"])[:, :4].cuda()
    out = {g: og.sample_with_past(x, c["m8"], 10, sample_logits=False, use_graph=g, return_logits=True) for g in (False, True)}
    c["m8"].check_overflow()
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    plain = og.sample_with_past(x, make_gpt(c["sd"], c["dims"]), 10, sample_logits=False, use_graph=True, return_logits=True)
    assert not torch.equal(out[True][1], plain[1])                      # ... and it is the fp8 step that was captured


def test_guided_sampling_runs_with_2b_rows(cases):
    from omnitokenizer_amd import gpt as og
    c = cases(GPT_CASES[0])
    V = c["dims"][0]
    cls = torch.tensor([3, 7, 11]).cuda()[:, None]                      # 2 B = 6 rows: a group of 4 and a group of 2 streams
    out = {g: og.sample_with_past_cfg(cls.clone(), c["m8"], 8, sample_logits=False, cfg_ratio=1.5, use_graph=g, return_logits=True)
           for g in (False, True)}
    c["m8"].check_overflow()
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    tok, lg = out[True]
    assert tok.shape == (3, 8) and lg.shape == (3, 8, V) and torch.isfinite(lg).all() and int(tok.min()) >= 0 and int(tok.max()) < V
    # the blended logits (1 + t) l_c - t l_u of an fp32 engine on s * q: (1 + 2 t) = 4 logit tolerances
    ref = og.sample_with_past_cfg(cls.clone(), make_gpt(c["dsd"], c["dims"]), 8, sample_logits=False, cfg_ratio=1.5, return_logits=True)
    if torch.equal(ref[0], tok):                                        # (same tokens: the same contexts at every step)
        assert dmax(lg, ref[1]) < 4 * LOGIT_TOL


def test_image_is_made_from_the_fp32_originals(cases):
    """bf16 weights + a bf16 cache + fp8: steps from empty streams read only the fp8 image (every matrix product of a step), so
    their logits are BIT-equal to an engine with fp32 weights and the same cache format -- the image does not see the 16-bit
    rounding of the other images.  The prefill does run on the bf16 values."""
    c = cases(GPT_CASES[0])
    a = make_gpt(c["sd"], c["dims"], "fp8", fmt="bf16", kv="bf16")
    b = make_gpt(c["sd"], c["dims"], "fp8", fmt="fp32", kv="bf16")
    ra, rb = run(a, c["idx"], c["nxt"], c["T"]), run(b, c["idx"], c["nxt"], c["T"])
    assert (a.weight_format, a.cache_format, a.decode_quant) == ("bf16", "bf16", "fp8")
    assert torch.equal(ra["stepped"], rb["stepped"]) and torch.equal(ra["after_steps"], rb["after_steps"])
    assert not torch.equal(ra["batched"], rb["batched"])


def test_many_stream_steps_are_untouched(cases):
    """set_max_streams(24): a 24-stream step runs the many-stream GEMMs on the weight format's image, bit-equal with and without
    the switch; a 3-stream step of the same engines differs."""
    c = cases(GPT_CASES[0])
    V = c["dims"][0]
    idx = torch.randint(0, V, (24, 6), generator=torch.Generator().manual_seed(14)).cuda()
    out = {}
    for quant in ("none", "fp8"):
        m = make_gpt(c["sd"], c["dims"], quant).set_max_streams(24)
        m.reset_streams(24, 8)
        many = torch.stack([m.step(idx[:, t].contiguous()) for t in range(6)], 1)
        m.reset_streams(3, 8)
        few = torch.stack([m.step(idx[:3, t].contiguous()) for t in range(6)], 1)
        out[quant] = (many, few)
    assert torch.equal(out["none"][0], out["fp8"][0])
    assert dmax(out["none"][1], out["fp8"][1]) > LOGIT_TOL


@pytest.mark.parametrize("key,value", [("blocks.0.mlp.0.weight", float("inf")), ("blocks.0.attn.key.weight", float("nan")),
                                       ("head.weight", float("-inf"))])
def test_non_finite_weight_is_refused_by_name(key, value):
    V, BS, L, H, C = dims = (300, 48, 1, 4, 256)
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=25)
    good = sd[key][5, 7].item()
    sd[key][5, 7] = value
    m = make_gpt(sd, dims, "fp8")
    idx = torch.randint(0, V, (2, 20), generator=torch.Generator().manual_seed(26)).cuda()
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        m(idx)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):     # ... and it stays refused: nothing half-loaded runs
        m.reset_streams(2, 24)
    sd[key][5, 7] = good
    m.load_state_dict(sd, strict=True)
    logits, _ = m(idx)
    assert torch.isfinite(logits).all()


# ---- the engine: the K-sliced kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H", [(1536, 16), (2048, 16)])
def test_ksliced_path_in_the_engine(C, H):
    """The golden models only reach the row kernel: a 1-layer model at n_embd 1536 / 2048 runs the K-sliced fp8 kernels inside the
    step -- the attention merge in the proj GEMV's prologue, one and four chunks per wave, groups of 8 / 2 + 1 / 1 streams --
    against the oracle on s * q."""
    from omnitokenizer_amd import fp8_dequantized
    V, BS, L = 300, 48, 1
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=23)
    m = make_gpt(sd, (V, BS, L, H, C), "fp8")
    idx = torch.randint(0, V, (8, 14), generator=torch.Generator().manual_seed(24))
    ref = go.forward(fp8_dequantized(sd), idx, H)     # streams are independent: the first B rows serve every B
    for B in (1, 3, 8):
        xb = idx[:B].cuda()
        m.reset_streams(B, 16)
        lg = torch.stack([m.step(xb[:, t].contiguous()) for t in range(14)], 1)
        err = dmax(lg, ref[:B])
        print(f"C {C} fp8 B {B}: {err:.2e}")
        assert err < LOGIT_TOL
