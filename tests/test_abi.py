"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/omnitok.h
declares (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def test_header_symbols_exported(lib):
    from omnitokenizer_amd import _lib
    hdr = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("omnitok.h", "omnitok_lm.h", "omnitok_debug.h", "omnitok_comm.h"))
    # the measurement-only entry points live in their own header, outside the drop-in boundary
    assert "omnitok_debug_" not in open(os.path.join(ROOT, "include", "omnitok.h")).read()
    declared = set(re.findall(r"\b(omnitok_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"omnitok_stream_t"}
    assert len(declared) >= 30
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(raw, name), f"{name} declared in omnitok.h but not exported"
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)


def test_version_and_argument_errors_without_gpu(lib):
    assert b"gfx950" in lib.omnitok_version()
    # argument validation happens before any HIP call, so it is testable on the CPU
    from omnitokenizer_amd._lib import OmnitokRowGemm
    rc = lib.omnitok_gemm(ctypes.byref(OmnitokRowGemm(M=1, N=1, K=1)), None)
    assert rc == -1 and b"null" in lib.omnitok_last_error()
    rc = lib.omnitok_rope_table(0, 64, 10000.0, None, None)
    assert rc == -1


def test_rope_table_host_matches_oracle(lib):
    import torch
    from omnitokenizer_amd import ops
    from oracle import omnitok_oracle as orc
    for n in (64, 1024):
        cos, sin = ops.rope_table(n)
        rc, rs = orc.rope_table(n)
        assert (cos - rc).abs().max().item() < 1e-6 and (sin - rs).abs().max().item() < 1e-6


def test_product_refuses_cpu_tensors(lib):
    import torch
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, ops
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.layernorm(torch.zeros(4, 512), torch.ones(512))
    m = OmniTokenizer_VQGAN(make_args(2, resolution=64)).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode(torch.zeros(1, 3, 64, 64), True)


def test_state_dict_contract(lib):
    """Same key set / shapes as the reference's path; off-path keys are ignored on load."""
    import torch
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
    from omnitokenizer_amd.config import OmniTokConfig
    for stage in (1, 2):
        args = make_args(stage, resolution=64)
        cfg = OmniTokConfig.from_args(args)
        m = OmniTokenizer_VQGAN(args)
        spec = synth.path_state_spec(cfg)
        sd = m.state_dict()
        assert list(sd.keys()) == list(spec.keys())
        assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
        src = synth.synth_state_dict(cfg, seed=1)
        src["video_discriminator.main.0.weight"] = torch.zeros(3)
        src["perceptual_model.net.x"] = torch.zeros(1)
        res = m.load_state_dict(src, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert torch.equal(m.codebook.embeddings.data, src["codebook.embeddings"])
        assert m.codebook.n_codes == cfg.n_codes and m.n_codes == cfg.n_codes and not m.use_vae
        assert m.encoder.image_size == (64, 64)


def test_config_rejects_unbuilt_variants():
    from omnitokenizer_amd import make_args
    from omnitokenizer_amd.config import OmniTokConfig
    # in the DECODER 'n'/'r' Up blocks make the reference itself raise (omnitokenizer.py:1078; in the encoder
    # they run and are built, see below); GroupNorm(32) over the cnn decoder's 3 channels cannot be
    # constructed (base.py:274); the external VectorQuantize exists for codebook_type 'vq' only
    # (omnitokenizer.py:139-140)
    for bad in (dict(dec_block="tntt"), dict(dec_block="trtt"), dict(dec_block="tatt"), dict(enc_block="ttxw"),
                dict(patch_embed="cnn", norm_type="group"), dict(patch_embed="conv"),
                dict(use_external_codebook=True, codebook_type="lfq"),
                dict(use_external_codebook=True, use_vae=True), dict(dim_head=32)):
        with pytest.raises((NotImplementedError, ValueError)):
            OmniTokConfig.from_args(make_args(2, **bad))
    assert OmniTokConfig.from_args(make_args(2, use_vae=True)).use_vae
    c = OmniTokConfig.from_args(make_args(2, defer_spatial_pool=True, defer_temporal_pool=True, gen_upscale=2))
    assert (c.enc_patch_size, c.enc_temporal_patch_size, c.dec_patch_size, c.enc_grid_divisor) == (4, 2, 8, 2)
    c = OmniTokConfig.from_args(make_args(2, patch_embed="cnn", defer_spatial_pool=True, enc_block="tawl"))
    assert (c.enc_patch_size, c.dec_patch_size, c.enc_grid_divisor) == (8, 8, 4)  # defer_* ignored for cnn
    # encoder-side Up blocks (reference attention.py:116-150, 640-645): enc_block="ttnw" runs in the reference
    c = OmniTokConfig.from_args(make_args(2, enc_block="trnw"))
    assert (c.enc_grid_multiplier, c.enc_grid_divisor) == (4, 1)


def test_vae_state_dict_contract(lib):
    """--use_vae: pre_vq_conv emits mean|logvar (reference omnitokenizer.py:149-153)."""
    import torch
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    m = OmniTokenizer_VQGAN(make_args(2, resolution=64, use_vae=True))
    assert m.use_vae
    assert tuple(m.state_dict()["pre_vq_conv.1.weight"].shape) == (16, 512)
    assert tuple(m.state_dict()["pre_vq_conv.1.bias"].shape) == (16,)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode(torch.zeros(1, 3, 64, 64), True)


def test_load_from_pl_checkpoint(tmp_path, lib):
    """PL-style checkpoints ({state_dict, hyper_parameters: {args}}, reference omnitokenizer.py:208,
    download.py:49) load through the drop-in class, off-path entries dropped, stale Namespaces
    back-filled like the reference's hasattr() defaults (omnitokenizer.py:70-98)."""
    import argparse
    import torch
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
    from omnitokenizer_amd.config import OmniTokConfig
    args = make_args(1, resolution=64)
    cfg = OmniTokConfig.from_args(args)
    sd = dict(synth.synth_state_dict(cfg, seed=7))
    sd["image_discriminator.main.0.weight"] = torch.zeros(3)
    sd["perceptual_model.net.slice1.0.weight"] = torch.zeros(3)
    old = argparse.Namespace(**{k: v for k, v in vars(args).items()
                                if k not in ("enc_block", "dec_block", "twod_window_size", "spatial_pos", "use_vae",
                                             "defer_temporal_pool", "defer_spatial_pool", "gen_upscale")})
    path = tmp_path / "tok.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": {"args": old}}, path)
    m = OmniTokenizer_VQGAN.load_from_checkpoint(str(path), attention_mode="legacy")
    assert m.cfg.enc_block == "tttt" and m.cfg.window_size == 4 and m.cfg.spatial_pos == "rel"  # back-filled
    assert m.cfg.attention_mode == "legacy" and not m.use_vae
    got = m.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items() if k in got)
    from omnitokenizer_amd.vqgan import load_vqgan
    m2 = load_vqgan("omnitokenizer", str(path))
    assert not m2.training and m2.latent_shape == (4, 16, 16)  # (17 // 1, 64, 64) // (4, 4, 4)
    assert not any(k.startswith(("image_discriminator", "perceptual_model")) for k in got)


def test_torch_custom_ops_registered_with_schemas(lib):
    """the operators are schema-registered PyTorch custom ops (omnitok::*), with fake
    (shape-inference) kernels so that they trace without a GPU."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from omnitokenizer_amd import ops
    assert ops.CUSTOM_OPS_REGISTERED
    assert str(torch.ops.omnitok.vq_argmin.default._schema) == "omnitok::vq_argmin(Tensor z, Tensor codebook) -> Tensor"
    for name in ("linear", "layernorm", "attn_spatial", "attn_window", "attn_temporal", "peg3d"):
        assert hasattr(torch.ops.omnitok, name)
    with FakeTensorMode():
        z, E = torch.empty(10, 3, 8, device="cuda"), torch.empty(8192, 8, device="cuda")
        ids = torch.ops.omnitok.vq_argmin(z, E)
        assert tuple(ids.shape) == (10, 3) and ids.dtype == torch.int64
        y = torch.ops.omnitok.linear(torch.empty(7, 512, device="cuda"), torch.empty(192, 512, device="cuda"), None)
        assert tuple(y.shape) == (7, 192)
        q = torch.empty(2048, 512, device="cuda")
        assert tuple(torch.ops.omnitok.attn_spatial(q, q, q, 1024, 8).shape) == (2048, 512)
        # the rest of the operator set
        s64 = torch.empty(64, device="cuda")
        assert tuple(torch.ops.omnitok.attn_spatial_h2(q, q, q, 1024, 8, s64, s64).shape) == (2048, 512)
        assert tuple(torch.ops.omnitok.linear_geglu(q, torch.empty(2816, 512, device="cuda")).shape) == (2048, 1408)
        vid = torch.empty(2, 3, 17, 256, 256, device="cuda")
        assert tuple(torch.ops.omnitok.patchify_ln(vid, 1, 4, 4, 8).shape) == (2 * 4 * 1024, 3 * 4 * 64)
        assert tuple(torch.ops.omnitok.pre_vq(q, torch.empty(8, 512, device="cuda"), torch.empty(8, device="cuda")).shape) \
            == (2048, 8)
        idl = torch.empty(2, 5, 32, 32, dtype=torch.int64, device="cuda")
        w, b = torch.empty(512, 8, device="cuda"), torch.empty(512, device="cuda")
        assert tuple(torch.ops.omnitok.dequant_post_vq(idl, torch.empty(8192, 8, device="cuda"), w, b).shape) == (2, 5, 32, 32, 512)
        assert tuple(torch.ops.omnitok.gather_rows(idl, torch.empty(8192, 512, device="cuda")).shape) == (2, 5, 32, 32, 512)
    for name in ("unpatchify", "qk_prep"):   # in-place operators: schema carries the mutation
        assert "!)" in str(getattr(torch.ops.omnitok, name).default._schema)


def test_vqgan_encode_decode_are_registered_operators():
    """OmniTokenizer_VQGAN.encode / decode run through omnitok::vqgan_encode / vqgan_decode; their fake
    implementations infer the shapes of every configuration family without a GPU."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    cases = [(dict(), (2, 3, 17, 256, 256), (2, 5, 32, 32)),
             (dict(enc_block="tawl", resolution=128), (1, 3, 5, 128, 128), (1, 2, 4, 4)),
             (dict(enc_block="ttnw", resolution=64), (1, 3, 5, 64, 64), (1, 2, 16, 16)),
             (dict(defer_spatial_pool=True, defer_temporal_pool=True, resolution=128), (1, 3, 9, 128, 128), (1, 3, 16, 16)),
             (dict(gen_upscale=2, resolution=64), (1, 3, 5, 64, 64), (1, 2, 8, 8))]
    for over, xs, ids_shape in cases:
        m = OmniTokenizer_VQGAN(make_args(2, **over))
        with FakeTensorMode():
            x = torch.empty(*xs, device="cuda")
            ids, emb, z = torch.ops.omnitok.vqgan_encode(x, m._handle, True, True)
            assert tuple(ids.shape) == ids_shape and ids.dtype == torch.int64
            assert tuple(emb.shape) == (ids_shape[0], 8) + ids_shape[1:] and tuple(z.shape) == ids_shape + (8,)
            pix = torch.ops.omnitok.vqgan_decode(ids, m._handle)
            # the decoder works from the latent grid: pooling / Up blocks of the encoder are not undone
            side = ids_shape[2] * m.cfg.dec_patch_size * (2 if over.get("defer_spatial_pool") else 1)
            assert tuple(pix.shape) == (xs[0], 3, xs[2], side, side), (over, pix.shape)
    with FakeTensorMode(), pytest.raises(RuntimeError, match="handle"):
        torch.ops.omnitok.vqgan_decode(torch.empty(1, 1, 8, 8, dtype=torch.int64, device="cuda"), 10 ** 9)
    with pytest.raises(NotImplementedError):   # CPU tensors: the operator exists for the GPU only (no fallback)
        torch.ops.omnitok.vqgan_decode(torch.empty(1, 1, 8, 8, dtype=torch.int64), 10 ** 9)


def test_lm_argument_errors_without_gpu(lib):
    """include/omnitok_lm.h: configuration / argument validation happens before any HIP call."""
    from omnitokenizer_amd._lib import OmnitokLmConfig
    h = ctypes.c_void_p()
    bad = OmnitokLmConfig(100, 16, 1, 3, 300)           # head_dim 100
    assert lib.omnitok_lm_create(ctypes.byref(bad), ctypes.byref(h)) != 0
    assert b"head_dim" in lib.omnitok_last_error()
    assert lib.omnitok_lm_create(None, ctypes.byref(h)) == -1
    ok = OmnitokLmConfig(8192, 5120, 24, 16, 1536)
    assert lib.omnitok_lm_create(ctypes.byref(ok), ctypes.byref(h)) == 0
    try:
        assert lib.omnitok_lm_step(h, None, None, None, 1, None, 1, None) == -1       # null pointers
        assert lib.omnitok_lm_alloc_cache(h, 17, 64) == -1                             # more than 16 streams
        assert lib.omnitok_lm_alloc_cache(h, 1, 9000) == -1                            # beyond 8192 positions
        assert lib.omnitok_lm_gemv(None, None, None, None, None, None, None, 1, 8, 256, 0, None) == -1
        shape = (ctypes.c_int64 * 2)(7, 7)
        x = ctypes.c_float(0)
        assert lib.omnitok_lm_set_weight(h, b"tok_emb.weight", ctypes.byref(x), shape, 2, None) == -1  # shape mismatch
        assert b"tok_emb.weight" in lib.omnitok_last_error()
        assert lib.omnitok_lm_set_weight(h, b"blocks.0.attn.mask", ctypes.byref(x), shape, 2, None) == 1  # ignored
    finally:
        lib.omnitok_lm_destroy(h)


def test_missing_library_fails_loudly(lib, monkeypatch):
    """No CPU / PyTorch fallback: without libomnitok.so the product raises instead of computing."""
    from omnitokenizer_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libomnitok.so")
    with pytest.raises(_lib.OmnitokError, match="no CPU fallback"):
        _lib.load()


def test_new_entry_points_validate_arguments_without_gpu(lib):
    """Argument validation of the round-2 entry points happens before any HIP call (status -1 + a message)."""
    import ctypes as C
    one = C.c_void_p(256)  # any non-null, 16-byte aligned value: the checks fire before it is dereferenced
    f = C.c_float
    # attn_pack: n_tokens not a multiple of 32; non-positive bounds
    pack = dict(q=256, ldq=512, k=256, v=256, ldkv=1024, seqs=1, heads=8, q_scale=256, k_scale=256, scale=8.0, q_bound=8.0,
                k_bound=1.0, v_bound=1.0, qp=256, kp=256, vp=256)
    assert lib.omnitok_attn_pack(C.byref(_attn_desc(**pack, n_tokens=48)), None) == -1
    assert b"attn_pack" in lib.omnitok_last_error()
    for bound in ("q_bound", "k_bound"):
        assert lib.omnitok_attn_pack(C.byref(_attn_desc(**{**pack, "n_tokens": 64, bound: 0.0})), None) == -1
        assert b"bounds" in lib.omnitok_last_error()
    # attn_spatial_h2: N not a multiple of 64
    h2 = _attn_desc(qp=256, kp=256, vp=256, out=256, ldo=512, seqs=1, n_tokens=96, heads=8, q_bound=8.0, k_bound=1.0, v_bound=1.0)
    assert lib.omnitok_attn_spatial_h2(C.byref(h2), None) == -1
    # lm_select: non-positive temperature, sampling without uniforms, top_p <= 0
    assert lib.omnitok_lm_select(one, None, 1, 100, f(0.0), f(1.0), f(0.0), -1, f(1.0), 0, None, one, None, None, None) == -1
    assert b"temperature" in lib.omnitok_last_error()
    assert lib.omnitok_lm_select(one, None, 1, 100, f(1.0), f(1.0), f(0.0), 10, f(0.9), 1, None, one, None, None, None) == -1
    assert lib.omnitok_lm_select(one, None, 1, 100, f(1.0), f(1.0), f(0.0), 10, f(0.0), 0, None, one, None, None, None) == -1
    # gather_rows / layernorm with the fused transpose: rows must be whole (a, c) groups; in-place is refused
    assert lib.omnitok_gather_rows_transposed(one, one, 10, one, 100, 3, 7, 512, None, None) == -1
    assert lib.omnitok_layernorm_transposed(one, one, None, one, 2, 3, 4, 512, f(1e-5), None) == -1
    # set_workspace: pointer / size mismatch and alignment are rejected on a null engine too
    assert lib.omnitok_engine_set_workspace(None, None, 0) == -1
    # plane GEMM: null argument block / null operands, the LayerNorm epilogue's full-row rule; per-engine options
    from omnitokenizer_amd._lib import OmnitokPlGemm
    assert lib.omnitok_gemm_pl(None, None) == -1
    g = OmnitokPlGemm()
    g.a = g.w = g.w_scale = g.c = g.out_planes = g.ln_gamma = 256
    g.M, g.N, g.K, g.ldc, g.epilogue, g.out_planes_k, g.out_bound = 64, 256, 512, 256, 2, 256, 30.0
    assert lib.omnitok_gemm_pl(C.byref(g), None) == -1 and b"512" in lib.omnitok_last_error()
    g.epilogue, g.N = 7, 512
    assert lib.omnitok_gemm_pl(C.byref(g), None) == -1
    assert lib.omnitok_pl_pack_weight(one, 512, 500, 512, 512, one, one, None) == -1   # N % 32
    assert lib.omnitok_pl_planes_bytes(1000, 512, 256) == 1024 * 512 * 4 and lib.omnitok_pl_planes_bytes(10, 500, 256) == -1
    assert lib.omnitok_engine_set_option(None, b"gemm_mode", 1) == -1


# the nearest-code entry points of csrc/vq.hip: argument names in call order (the stream, always last, is passed as NULL)
VQ_ENTRIES = {
    "omnitok_vq_argmin": "z packed ee n n_codes ids",
    "omnitok_vq_argmin_screened": "z packed ee screen n n_codes ids",
    "omnitok_vq_argmax_cos": "z packed n n_codes ids",
    "omnitok_vq_argmin_cdist": "z packed ee n n_codes ids",
    "omnitok_vq_prepare": "codebook n_codes cdim packed ee",
    "omnitok_vq_screen_prepare": "codebook ee n_codes cdim screen",
}
_VQ_SIZES = dict(n=64, n_codes=8192, cdim=8)
_VQ_PREPARE = " need cdim == 8, n_codes % 32 == 0"
# pointers whose 16-byte alignment the entry checks (ids and the arguments of omnitok_vq_prepare are not among them: a misaligned
# one passes every check and would reach the kernel)
_VQ_ALIGNED = {"omnitok_vq_argmin": "z packed ee", "omnitok_vq_argmin_screened": "z packed ee screen",
               "omnitok_vq_argmax_cos": "z packed", "omnitok_vq_argmin_cdist": "z packed ee", "omnitok_vq_prepare": "",
               "omnitok_vq_screen_prepare": "screen"}


def _vq_call(lib, name, **over):
    """(status, message) of `name` on sizes that pass every check and pointers 256 (non-null, 16-byte aligned, never
    dereferenced: each case below fails a check, and the checks come before the first HIP call), with `over` replaced."""
    args = [over.get(k, _VQ_SIZES.get(k, 256)) for k in VQ_ENTRIES[name].split()]
    return getattr(lib, name)(*args, None), lib.omnitok_last_error().decode()


@pytest.mark.parametrize("name", sorted(VQ_ENTRIES))
def test_vq_entry_points_host_checks(lib, name):
    """Status and omnitok_last_error() text of every host check of the four search entries and the two prepare entries, as
    commit 3751f52 (the last with one copy of the checks per entry) returned them: a null pointer in each position, n_codes 0 /
    33 / 32800, cdim 4, a pointer at address 8, and n == 0 ahead of every check.  n_codes 32800 is left out for the two prepare
    entries: they have no upper bound, so the call passes its checks and launches on the fake addresses."""
    short = name[len("omnitok_"):]
    prepare = name.endswith("prepare")
    pointers = [p for p in VQ_ENTRIES[name].split() if p not in _VQ_SIZES]
    for p in pointers:
        assert _vq_call(lib, name, **{p: None}) == (-1, f"{short}: null pointer"), p
    for n_codes in (0, 33) if prepare else (0, 33, 32800):
        want = f"{short}:{_VQ_PREPARE}" if prepare else f"{short}: n_codes={n_codes} unsupported"
        assert _vq_call(lib, name, n_codes=n_codes) == (-1, want), n_codes
    if prepare:
        assert _vq_call(lib, name, cdim=4) == (-1, f"{short}:{_VQ_PREPARE}")
    for p in _VQ_ALIGNED[name].split():
        want = f"{short}:{_VQ_PREPARE}" if prepare else f"{short}: unaligned"
        assert _vq_call(lib, name, **{p: 8}) == (-1, want), p
    if not prepare:   # an empty batch is done before anything is looked at
        assert _vq_call(lib, name, n=0, n_codes=33, **{p: None for p in pointers})[0] == 0
    # order of the checks: null pointer, then the sizes, then alignment
    assert _vq_call(lib, name, **{pointers[0]: None}, n_codes=33)[1] == f"{short}: null pointer"
    if not prepare:
        assert _vq_call(lib, name, z=8, n_codes=33)[1] == f"{short}: n_codes=33 unsupported"


ROW_GEMMS = ("omnitok_gemm", "omnitok_gemm_x3", "omnitok_gemm_h2")


def _row_gemm(name, **fields):
    """A descriptor whose required pointers are a non-null, 16-byte aligned dummy: every check fires before a dereference."""
    from omnitokenizer_amd._lib import OmnitokRowGemm
    weight = dict(w_planes=256, w_scale=256) if name == "omnitok_gemm_h2" else dict(w=256)
    return OmnitokRowGemm(**{**dict(a=256, c=256, M=64, N=64, K=64, a_bound=1.0), **weight, **fields})


@pytest.mark.parametrize("name", ROW_GEMMS)
def test_row_gemm_descriptor_layout_and_null_checks(lib, name):
    """omnitok_row_gemm through ctypes: the size fields land where the C struct has them (the message echoes them), and a NULL
    descriptor or NULL operand is refused -- all before the first HIP call."""
    fn = getattr(lib, name)
    assert fn(ctypes.byref(_row_gemm(name, M=7, N=5, K=-3)), None) == -1
    assert b"M=7 N=5 K=-3" in lib.omnitok_last_error()
    assert fn(None, None) == -1
    assert fn(ctypes.byref(_row_gemm(name, a=None)), None) == -1 and b"null pointer" in lib.omnitok_last_error()


def test_row_gemm_h2_fields_echoed(lib):
    """Fields behind the sizes: a_rows_per_clip (int64 after a float, a pointer and an int) and N under the GEGLU flag."""
    one = ctypes.c_float(1.0)
    g = _row_gemm("omnitok_gemm_h2", a_bound_dev=ctypes.addressof(one), a_rows_per_clip=100)
    assert lib.omnitok_gemm_h2(ctypes.byref(g), None) == -1 and b"(100)" in lib.omnitok_last_error()
    g = _row_gemm("omnitok_gemm_h2", flags=4, N=96)
    assert lib.omnitok_gemm_h2(ctypes.byref(g), None) == -1 and b"96" in lib.omnitok_last_error()


@pytest.mark.parametrize("name,field", [("omnitok_gemm", "w_planes"), ("omnitok_gemm", "ln_stats"), ("omnitok_gemm", "split_col"),
                                        ("omnitok_gemm", "v_planes"), ("omnitok_gemm_x3", "w_planes"),
                                        ("omnitok_gemm_x3", "v_planes"), ("omnitok_gemm_h2", "w")])
def test_row_gemm_refuses_fields_the_kernel_does_not_implement(lib, name, field):
    g = _row_gemm(name, **{field: 256})
    assert getattr(lib, name)(ctypes.byref(g), None) == -1
    err = lib.omnitok_last_error()
    assert field.encode() in err and name[len("omnitok_"):].encode() + b":" in err, err


def test_row_gemm_vpack_entry_point_is_gone(lib):
    """The packed-V epilogue is omnitok_gemm_h2 with v_planes set; header, library and binding agree on the symbol set."""
    from omnitokenizer_amd import _lib
    assert "omnitok_gemm_h2_vpack" not in _lib.EXPORTED_SYMBOLS
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), "omnitok_gemm_h2_vpack")
    hdr = open(os.path.join(ROOT, "include", "omnitok.h")).read()
    assert "omnitok_gemm_h2_vpack" not in hdr
    declared = set(re.findall(r"\b(omnitok_gemm[a-z0-9_]*)\s*\(", hdr))
    assert declared == {n for n in _lib.EXPORTED_SYMBOLS if n.startswith("omnitok_gemm")}
    # v_planes under a precondition the packed-V epilogue does not meet (a flag set) is refused, as before
    g = _row_gemm("omnitok_gemm_h2", v_planes=256, flags=1, bias=256)
    assert lib.omnitok_gemm_h2(ctypes.byref(g), None) == -1 and b"packed-V" in lib.omnitok_last_error()


def _attn_desc(**fields):
    from omnitokenizer_amd._lib import OmnitokAttnDesc
    return OmnitokAttnDesc(**fields)


# per entry point: a descriptor that passes every argument check (pointers are a non-null, 16-byte aligned dummy: every check
# fires before a dereference)
_ROWS = dict(q=256, ldq=128, k=256, v=256, ldkv=256)
_PLANES = dict(qp=256, kp=256, vp=256)
_PREP = dict(q_scale=256, k_scale=256, scale=8.0)
_BOUNDS = dict(q_bound=8.0, k_bound=1.0, v_bound=1.0)
_OUT = dict(out=256, ldo=128)
ATTN_OK = {
    "omnitok_qk_prep": dict(**_ROWS, **_PREP, seqs=1, n_tokens=64, heads=2),
    "omnitok_attn_pack": dict(**_ROWS, **_PLANES, **_PREP, **_BOUNDS, seqs=1, n_tokens=64, heads=2),
    "omnitok_attn_spatial": dict(**_ROWS, **_OUT, seqs=1, n_tokens=64, heads=2),
    "omnitok_attn_spatial_h2": dict(**_PLANES, **_BOUNDS, **_OUT, seqs=1, n_tokens=64, heads=2),
    "omnitok_attn_window": dict(q=256, ldq=384, bias_dense=256, **_OUT, seqs=1, gh=8, gw=8, heads=2),
    "omnitok_attn_window_h2": dict(**_PLANES, **_BOUNDS, bias_dense=256, **_OUT, seqs=1, gh=8, gw=8, heads=2),
    "omnitok_attn_temporal": dict(**_ROWS, **_PREP, **_OUT, seqs=16, n_tokens=5, heads=2, causal=1),
}


def _attn_call(lib, name, **fields):
    """(status, message) of entry point `name` on ATTN_OK[name] with `fields` replaced."""
    rc = getattr(lib, name)(ctypes.byref(_attn_desc(**{**ATTN_OK[name], **fields})), None)
    return rc, lib.omnitok_last_error()


@pytest.mark.parametrize("name,fields,echo", [
    ("omnitok_attn_spatial", dict(bias_table=256, gh=3, gw=5), b"bias grid 3x5 != N=64"),
    ("omnitok_attn_spatial_h2", dict(bias_table=256, gh=3, gw=5), b"bias grid 3x5 != N=64"),
    ("omnitok_attn_window", dict(gh=12, gw=8), b"grid 12x8"),
    ("omnitok_attn_window_h2", dict(gh=12, gw=8), b"grid 12x8"),
    ("omnitok_attn_temporal", dict(n_tokens=0), b"T=0"),
    ("omnitok_attn_pack", dict(n_tokens=48), b"48 rows of 48-token"),
    ("omnitok_qk_prep", dict(ldq=6), b"unaligned")])
def test_attn_descriptor_layout(lib, name, fields, echo):
    """omnitok_attn_desc through ctypes: fields late in the struct (the geometry sits behind every pointer, float and int64) land
    where the C struct has them -- the message of the check they fail echoes them."""
    rc, err = _attn_call(lib, name, **fields)
    assert rc == -1 and echo in err and name[len("omnitok_"):].encode() + b":" in err, err


@pytest.mark.parametrize("name", sorted(ATTN_OK))
def test_attn_null_descriptor_and_operand_refused(lib, name):
    """A NULL descriptor and a NULL required operand are refused before the first HIP call."""
    short = name[len("omnitok_"):].encode()
    assert getattr(lib, name)(None, None) == -1
    assert short + b": null descriptor" in lib.omnitok_last_error()
    for operand in ("q", "qp"):
        if operand in ATTN_OK[name]:
            rc, err = _attn_call(lib, name, **{operand: None})
            assert rc == -1 and short + b": null pointer" in err, err
    if "out" in ATTN_OK[name]:
        rc, err = _attn_call(lib, name, out=None)
        assert rc == -1 and short + b": null pointer" in err, err


ATTN_REFUSED = {
    "omnitok_attn_spatial": "qp kp vp out_planes bias_dense alibi_slopes causal",
    "omnitok_attn_spatial_h2": "q k v bias_dense alibi_slopes causal",
    "omnitok_attn_window": "k v qp kp vp bias_table alibi_slopes causal v_bound_dev",
    "omnitok_attn_window_h2": "q k v bias_table alibi_slopes causal v_bound_dev",
    "omnitok_attn_temporal": "qp kp vp bias_table bias_dense rope_cos rope_sin",
    "omnitok_qk_prep": "bias_table bias_dense alibi_slopes causal out out_planes",
    "omnitok_attn_pack": "bias_table bias_dense alibi_slopes causal out out_planes",
}


@pytest.mark.parametrize("name,field", [(n, f) for n, fs in sorted(ATTN_REFUSED.items()) for f in fs.split()])
def test_attn_refuses_fields_the_kernel_does_not_implement(lib, name, field):
    rc, err = _attn_call(lib, name, **{field: 256})
    assert rc == -1 and f"{name[len('omnitok_'):]}: {field} is set".encode() in err, err


def test_attn_planes_entry_points_are_gone(lib):
    """The plane outputs are out_planes of the seven entry points; header, library and binding agree on the symbol set."""
    from omnitokenizer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "omnitok.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for gone in ("omnitok_attn_spatial_h2_planes", "omnitok_attn_window_planes", "omnitok_attn_temporal_planes"):
        assert gone not in _lib.EXPORTED_SYMBOLS and not hasattr(raw, gone) and gone not in hdr, gone
    declared = set(re.findall(r"\b(omnitok_(?:attn[a-z0-9_]*|qk_prep))\s*\(", hdr))
    assert declared == set(ATTN_OK)
    assert declared == {n for n in _lib.EXPORTED_SYMBOLS if n.startswith("omnitok_attn") or n == "omnitok_qk_prep"}


@pytest.mark.parametrize("name,fields,message", [
    ("omnitok_attn_temporal", dict(out_planes=256, out_scale=256, v_bound=1.0, n_tokens=18),
     b"attn_temporal: plane output needs out_scale, T <= 17, cols % 16 == 0 and a bound of |v|"),
    ("omnitok_attn_window", dict(out_planes=256, out_bound=0.0), b"attn_window: plane output needs a bound"),
    ("omnitok_attn_spatial_h2", dict(out_planes=256, out_scale=None), b"attn_spatial_h2: plane output needs out_scale")])
def test_attn_plane_output_preconditions(lib, name, fields, message):
    """out_planes selects what the _planes entry points did, under their preconditions and with their messages."""
    rc, err = _attn_call(lib, name, **fields)
    assert rc == -1 and message in err, err


def test_attn_spatial_h2_refuses_retired_variants(lib):
    """"attn_h2_variant" takes 6 (64 queries per wave), 3 (32 queries per wave) or the measurement arms 4, 5, 7 of the first; every
    other value -- the retired arms 0, 1, 2 among them -- is refused by the entry point as its last argument check, so before the
    first HIP call."""
    from omnitokenizer_amd import _lib
    try:
        for v in (0, 1, 2, -1, 8):
            _lib.set_option("attn_h2_variant", v)
            rc, err = _attn_call(lib, "omnitok_attn_spatial_h2")
            assert rc == -1 and f"attn_h2_variant={v},".encode() in err and b"6, 3 and" in err, (v, err)
            # last among the checks: a descriptor that fails an earlier one reports that one
            rc, err = _attn_call(lib, "omnitok_attn_spatial_h2", n_tokens=48)
            assert rc == -1 and b"N=48" in err, (v, err)
        for v in (6, 3, 4, 5, 7):
            _lib.set_option("attn_h2_variant", v)
            rc, err = _attn_call(lib, "omnitok_attn_spatial_h2", seqs=0)
            assert rc == 0, (v, err)
    finally:
        _lib.set_option("attn_h2_variant", 6)


# every option a test or tool sets and then has to restore: the LM decode step's kernel choices and the stats_pack form
READABLE_OPTIONS = ("gemm_mode", "attn_mode", "gemm_pl", "pl_min_tokens", "temporal_chunk", "prevq_fuse", "pl_cfg", "pl_tail",
                    "sp_small_blocks", "lm_wide_u", "lm_balance", "lm_ksliced", "lm_mfma", "lm_mfma_mult", "lm_ks_deep",
                    "lm_attn_short", "lm_attn_waves")


@pytest.mark.parametrize("name", READABLE_OPTIONS)
def test_option_reads_back_what_was_set(lib, name):
    """omnitok_get_option returns the value omnitok_set_option stored, for every readable option (the lm_* options and
    sp_small_blocks could be set but not read, so tests restored hard-coded values)."""
    from omnitokenizer_amd import _lib
    before = _lib.get_option(name)
    try:
        for v in (before + 7, 0, 3, before):
            _lib.set_option(name, v)
            assert _lib.get_option(name) == v, (name, v)
    finally:
        _lib.set_option(name, before)
    assert _lib.get_option(name) == before
    v = ctypes.c_int(-12345)
    assert lib.omnitok_get_option(b"lm_no_such_option", ctypes.byref(v)) == -1 and v.value == -12345
    assert b"lm_no_such_option" in lib.omnitok_last_error()


def test_option_table_settable_readable_and_retired_names(lib):
    """The one option table behind omnitok_set_option / omnitok_get_option: every readable option round-trips, the minimum of
    lm_loss_chunk_rows holds, the retired ablation switches are unknown names, and a settable option outside the readable subset
    still cannot be read."""
    readable = ["gemm_mode", "attn_mode", "gemm_pl", "pl_min_tokens", "temporal_chunk", "prevq_fuse", "pl_cfg", "pl_tail",
                "sp_small_blocks", "lm_wide_u", "lm_balance", "lm_ksliced", "lm_mfma", "lm_mfma_mult", "lm_ks_deep",
                "lm_attn_short", "lm_attn_waves", "lm_loss_chunk_rows"]
    for name in readable:
        before, v = ctypes.c_int(), ctypes.c_int()
        assert lib.omnitok_get_option(name.encode(), ctypes.byref(before)) == 0, name
        try:
            assert lib.omnitok_set_option(name.encode(), before.value + 5) == 0, name
            assert lib.omnitok_get_option(name.encode(), ctypes.byref(v)) == 0 and v.value == before.value + 5, name
        finally:
            assert lib.omnitok_set_option(name.encode(), before.value) == 0
        assert lib.omnitok_get_option(name.encode(), ctypes.byref(v)) == 0 and v.value == before.value, name

    rows = ctypes.c_int()
    assert lib.omnitok_get_option(b"lm_loss_chunk_rows", ctypes.byref(rows)) == 0 and rows.value >= 1
    assert lib.omnitok_set_option(b"lm_loss_chunk_rows", 0) == -1
    assert b"lm_loss_chunk_rows 0, expected at least 1" in lib.omnitok_last_error()
    v = ctypes.c_int()
    assert lib.omnitok_get_option(b"lm_loss_chunk_rows", ctypes.byref(v)) == 0 and v.value == rows.value

    # the three retired switches, the retired arm selector of the VQ search and a made-up name
    for name in b"h2_dbg x3_dbg attn_h2_dbg vq_variant no_such_option".split():
        assert lib.omnitok_set_option(name, 1) == -1, name
        assert b"unknown option " + name in lib.omnitok_last_error(), name

    v = ctypes.c_int(-12345)   # settable, but outside the readable subset (not set here: its value could not be restored)
    assert lib.omnitok_get_option(b"gemm_variant", ctypes.byref(v)) == -1 and v.value == -12345
    assert b"gemm_variant is not a readable option" in lib.omnitok_last_error()
