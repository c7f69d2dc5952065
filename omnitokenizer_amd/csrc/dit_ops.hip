// DiT denoiser: the small kernels around the GEMMs and the attention (index: dit_common.h).  Every kernel computes an output
// element from its own sample's data in an order fixed by the shapes of ONE sample: results do not depend on the batch.
#include "dit_common.h"

#include <cmath>

namespace omnitok {

// ---- patch embed + pos_embed ------------------------------------------------------------------------------------------------
// out[b N + n][d] = bias[d] + sum_k w[d][k] * patch[k] + pos[n][d], k = (c, i, j) as the conv weight [D, C, p, p] lies in memory.
// K = p p C is 16 or 32 in practice: a workgroup stages PE_TOK patches in LDS, thread d walks its weight row once (64 .. 128
// contiguous bytes) and feeds PE_TOK fmaf chains in k order.
constexpr int PE_TOK = 8;
constexpr int PE_KMAX = 512;

__global__ __launch_bounds__(256) void dit_patch_embed_kernel(const float *__restrict__ x, int x_batch, const float *__restrict__ w,
                                                              const float *__restrict__ bias, const float *__restrict__ pos, int64_t M,
                                                              int N, int C, int H, int p, int D, float *__restrict__ out) {
    __shared__ float patch[PE_TOK][PE_KMAX];
    const int K = C * p * p, gw = H / p;
    const int64_t m0 = (int64_t)blockIdx.x * PE_TOK;
    for (int id = threadIdx.x; id < PE_TOK * K; id += 256) {
        const int tk = id / K, k = id - tk * K;
        const int64_t m = m0 + tk;
        float v = 0.0f;
        if (m < M) {
            const int b = (int)(m / N), n = (int)(m - (int64_t)b * N);
            const int hp = n / gw, wp = n - hp * gw;
            const int c = k / (p * p), ij = k - c * p * p, i = ij / p, j = ij - i * p;
            v = x[(((int64_t)(b % x_batch) * C + c) * H + hp * p + i) * H + wp * p + j];
        }
        patch[tk][k] = v;
    }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) {
        float acc[PE_TOK];
#pragma unroll
        for (int tk = 0; tk < PE_TOK; ++tk) acc[tk] = 0.0f;
        const float *wr = w + (int64_t)d * K;
        for (int k = 0; k < K; ++k) {
            const float wk = wr[k];
#pragma unroll
            for (int tk = 0; tk < PE_TOK; ++tk) acc[tk] = fmaf(wk, patch[tk][k], acc[tk]);
        }
        const float bd = bias[d];
#pragma unroll
        for (int tk = 0; tk < PE_TOK; ++tk) {
            const int64_t m = m0 + tk;
            if (m < M) out[m * D + d] = (acc[tk] + bd) + pos[(m % N) * D + d];
        }
    }
}

// ---- conditioning --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dit_silu_f(float v) { return v / (1.0f + expf(-v)); }

__global__ void dit_cond_gather_kernel(const float *__restrict__ table, const int64_t *__restrict__ t, int B, float *__restrict__ temb,
                                       int *__restrict__ flag) {
    const int b = blockIdx.x;
    if (b >= B) return;
    int64_t tv = t[b];
    if (tv < 0 || tv >= DIT_T_STEPS) {
        if (threadIdx.x == 0) atomicOr(flag, DIT_FLAG_T_RANGE);
        tv = tv < 0 ? 0 : DIT_T_STEPS - 1;
    }
    for (int i = threadIdx.x; i < DIT_T_FREQ; i += blockDim.x) temb[(int64_t)b * DIT_T_FREQ + i] = table[tv * DIT_T_FREQ + i];
}

__global__ void dit_silu_kernel(float *__restrict__ x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = dit_silu_f(x[i]);
}

__global__ void dit_cond_combine_kernel(const float *__restrict__ temb2, const float *__restrict__ ytable, int y_rows,
                                        const int64_t *__restrict__ y, int B, int D, float *__restrict__ c, int *__restrict__ flag) {
    const int b = blockIdx.x;
    if (b >= B) return;
    if (!ytable) {  // no labels: c = silu(t_emb)
        for (int d = threadIdx.x; d < D; d += blockDim.x) c[(int64_t)b * D + d] = dit_silu_f(temb2[(int64_t)b * D + d]);
        return;
    }
    int64_t yv = y[b];
    if (yv < 0 || yv >= y_rows) {
        if (threadIdx.x == 0) atomicOr(flag, DIT_FLAG_Y_RANGE);
        yv = yv < 0 ? 0 : y_rows - 1;
    }
    for (int d = threadIdx.x; d < D; d += blockDim.x) c[(int64_t)b * D + d] = dit_silu_f(temb2[(int64_t)b * D + d] + ytable[yv * D + d]);
}

// ---- LayerNorm (eps 1e-6, no affine) * (1 + scale[b]) + shift[b] -------------------------------------------------------------------
// One wave per row: pass 1 the mean, pass 2 the variance around it, pass 3 the store (the row stays in L1 / L2 between them).
// OT = float: the fp32 row.  OT = lm_bf16 / lm_fp16 (omnitok_dit_ln_modulate16): the same values rounded once into a packed row, the A
// operand of dit_gemm16_kernel; a finite value that leaves the fp16 range raises DIT_FLAG_F16_RANGE in *flag.
template <typename OT>
__global__ __launch_bounds__(256) void dit_ln_modulate_kernel(const float *__restrict__ x, const float *__restrict__ shift,
                                                              const float *__restrict__ scale, int64_t ld_mod, int64_t rows, int n_tokens,
                                                              int D, void *__restrict__ out_, int *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;  // wave-uniform
    const int64_t b = r / n_tokens;
    const f32x4 *xr = reinterpret_cast<const f32x4 *>(x + r * D);
    const int n4 = D / 4;
    float s = 0.0f;
    for (int i = lane; i < n4; i += 64) {
        const f32x4 v = xr[i];
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = wave_allsum(s) / (float)D;
    float q = 0.0f;
    for (int i = lane; i < n4; i += 64) {
        const f32x4 v = xr[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float dv = v[e] - mean;
            q = fmaf(dv, dv, q);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_allsum(q) / (float)D + 1e-6f);
    const f32x4 *sh = reinterpret_cast<const f32x4 *>(shift + b * ld_mod);
    const f32x4 *sc = reinterpret_cast<const f32x4 *>(scale + b * ld_mod);
    bool inf = false;
    for (int i = lane; i < n4; i += 64) {
        const f32x4 v = xr[i], a = sc[i], c = sh[i];
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = fmaf((v[e] - mean) * rstd, 1.0f + a[e], c[e]);
        if constexpr (__is_same(OT, float))
            reinterpret_cast<f32x4 *>(static_cast<float *>(out_) + r * D)[i] = y;
        else
            reinterpret_cast<u32x2 *>(static_cast<unsigned short *>(out_) + r * D)[i] = dit_round16x4<OT>(y, inf);
    }
    if constexpr (__is_same(OT, lm_fp16))
        if (inf) atomicOr(flag, DIT_FLAG_F16_RANGE);
}

// ---- fp32 -> packed 16-bit, round to nearest even (the attention output in front of proj; the weight images at finalize) ---------------
template <typename OT>
__global__ void dit_round16_kernel(const float *__restrict__ src, unsigned short *__restrict__ dst, int64_t n4, int *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    bool inf = false;
    reinterpret_cast<u32x2 *>(dst)[i] = dit_round16x4<OT>(reinterpret_cast<const f32x4 *>(src)[i], inf);
    if constexpr (__is_same(OT, lm_fp16))
        if (inf) atomicOr(flag, DIT_FLAG_F16_RANGE);
}

// ---- x += gate[b] * y ---------------------------------------------------------------------------------------------------------------
__global__ void dit_gate_residual_kernel(float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ gate, int64_t ld_gate,
                                         int64_t rows, int n_tokens, int D) {
    const int n4 = D / 4;
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= rows * n4) return;
    const int64_t r = id / n4;
    const int i = (int)(id - r * n4);
    const f32x4 g = reinterpret_cast<const f32x4 *>(gate + (r / n_tokens) * ld_gate)[i];
    const f32x4 yv = reinterpret_cast<const f32x4 *>(y)[id];
    f32x4 xv = reinterpret_cast<f32x4 *>(x)[id];
#pragma unroll
    for (int e = 0; e < 4; ++e) xv[e] = fmaf(g[e], yv[e], xv[e]);
    reinterpret_cast<f32x4 *>(x)[id] = xv;
}

// ---- GELU, tanh form (dit_common.h) ----------------------------------------------------------------------------------------------------
__global__ void dit_gelu_tanh_kernel(float *__restrict__ x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    x[i] = dit_gelu_tanh_f(x[i]);
}

// ---- unpatchify: lin[(b, hp, wp)][(i, j, c)] -> out[b][c][hp p + i][wp p + j] -------------------------------------------------------------
__global__ void dit_unpatchify_kernel(const float *__restrict__ lin, int64_t total, int gw, int p, int Cout, float *__restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int H = gw * p;
    const int wcol = (int)(id % H);
    const int64_t r1 = id / H;
    const int hrow = (int)(r1 % H);
    const int64_t r2 = r1 / H;
    const int c = (int)(r2 % Cout);
    const int64_t b = r2 / Cout;
    const int hp = hrow / p, i = hrow - hp * p, wp = wcol / p, j = wcol - wp * p;
    out[id] = lin[((b * gw + hp) * gw + wp) * ((int64_t)p * p * Cout) + (i * p + j) * Cout + c];
}

// ---- classifier-free guidance on channels [0, nc) (models.py:262-266) ----------------------------------------------------------------------
__global__ void dit_cfg_blend_kernel(float *__restrict__ out, int half, int Cout, int nc, int64_t HW, float s) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)half * nc * HW) return;
    const int64_t b = id / (nc * HW), rest = id - b * nc * HW;
    const int64_t ic = b * Cout * HW + rest, iu = (b + half) * Cout * HW + rest;
    const float cond = out[ic], uncond = out[iu];
    const float g = uncond + no_fuse(s * (cond - uncond));  // torch's three roundings
    out[ic] = g;
    out[iu] = g;
}

// ---- p_sample ----------------------------------------------------------------------------------------------------------------------------------
__global__ void dit_p_sample_kernel(const float *__restrict__ mo, const float *__restrict__ x, const float *__restrict__ noise,
                                    const float *__restrict__ coef, int n_steps, const int64_t *__restrict__ t, int64_t total, int C,
                                    int64_t HW, int learned, int clip, float *__restrict__ x_prev, float *__restrict__ pred_xstart) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int64_t chw = (int64_t)C * HW;
    const int64_t b = id / chw, rest = id - b * chw;
    int64_t tv = t[b];
    tv = tv < 0 ? 0 : (tv >= n_steps ? n_steps - 1 : tv);
    const float *k = coef + tv * 8;
    const int64_t mo_b = b * (learned ? 2 : 1) * chw;
    const float eps = mo[mo_b + rest], xv = x[id];
    float logvar = k[6];
    if (learned) {
        const float frac = (mo[mo_b + chw + rest] + 1.0f) / 2.0f;
        logvar = frac * k[5] + (1.0f - frac) * k[4];
    }
    float xs = k[0] * xv - k[1] * eps;
    if (clip) xs = fminf(fmaxf(xs, -1.0f), 1.0f);
    const float mean = k[2] * xs + k[3] * xv;
    if (pred_xstart) pred_xstart[id] = xs;
    x_prev[id] = mean + k[7] * expf(0.5f * logvar) * noise[id];
}

// ---- ddim_step -----------------------------------------------------------------------------------------------------------------------------------
// gaussian_diffusion.py:513-598 behind the model call.  One element: contraction is off and every fused multiply-add is written
// out, so the scalar and the float4 kernel give the same bits and a row does not depend on which of them its call took.
// k: the row of DDIMDiffusion.ddim_coefficient_table (omnitok_dit.h).  n is read only where has_noise.
__device__ __forceinline__ float dit_ddim_elem(const float *__restrict__ k, float xv, float eps, float n, bool has_noise, bool clip,
                                               bool reverse, float *xs_out) {
#pragma clang fp contract(off)
    float xs = fmaf(k[0], xv, -(k[1] * eps));
    if (clip) xs = fminf(fmaxf(xs, -1.0f), 1.0f);
    const float e = fmaf(k[0], xv, -xs) / k[1];  // re-derived from pred_xstart: not eps under clip
    *xs_out = xs;
    if (reverse) return fmaf(k[6], e, xs * k[5]);
    const float mean = fmaf(k[3], e, xs * k[2]);
    return has_noise ? fmaf(k[4], n, mean) : mean;
}

__device__ __forceinline__ const float *dit_ddim_row(const float *__restrict__ coef, int n_steps, const int64_t *__restrict__ t, int64_t b) {
    int64_t tv = t[b];
    tv = tv < 0 ? 0 : (tv >= n_steps ? n_steps - 1 : tv);
    return coef + tv * 8;
}

__global__ void dit_ddim_step_kernel(const float *__restrict__ mo, const float *__restrict__ x, const float *__restrict__ noise,
                                     const float *__restrict__ coef, int n_steps, const int64_t *__restrict__ t, int64_t total, int64_t chw,
                                     int mo_mul, int clip, int reverse, float *__restrict__ x_out, float *__restrict__ pred_xstart) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int64_t b = id / chw, rest = id - b * chw;
    const float *k = dit_ddim_row(coef, n_steps, t, b);
    float xs;
    const float out = dit_ddim_elem(k, x[id], mo[b * mo_mul * chw + rest], noise ? noise[id] : 0.0f, noise != nullptr, clip, reverse, &xs);
    if (pred_xstart) pred_xstart[id] = xs;
    x_out[id] = out;
}

// chw % 4 == 0 and 16-byte aligned pointers: four elements of one sample per thread, total4 = B chw / 4
__global__ void dit_ddim_step4_kernel(const float *__restrict__ mo, const float *__restrict__ x, const float *__restrict__ noise,
                                      const float *__restrict__ coef, int n_steps, const int64_t *__restrict__ t, int64_t total4, int64_t chw,
                                      int mo_mul, int clip, int reverse, float *__restrict__ x_out, float *__restrict__ pred_xstart) {
    const int64_t id4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id4 >= total4) return;
    const int64_t id = id4 * 4;
    const int64_t b = id / chw, rest = id - b * chw;
    const float *k = dit_ddim_row(coef, n_steps, t, b);
    const float4 xv = *reinterpret_cast<const float4 *>(x + id);
    const float4 ev = *reinterpret_cast<const float4 *>(mo + b * mo_mul * chw + rest);
    float4 nv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (noise) nv = *reinterpret_cast<const float4 *>(noise + id);
    float4 xs, out;
    out.x = dit_ddim_elem(k, xv.x, ev.x, nv.x, noise != nullptr, clip, reverse, &xs.x);
    out.y = dit_ddim_elem(k, xv.y, ev.y, nv.y, noise != nullptr, clip, reverse, &xs.y);
    out.z = dit_ddim_elem(k, xv.z, ev.z, nv.z, noise != nullptr, clip, reverse, &xs.z);
    out.w = dit_ddim_elem(k, xv.w, ev.w, nv.w, noise != nullptr, clip, reverse, &xs.w);
    if (pred_xstart) *reinterpret_cast<float4 *>(pred_xstart + id) = xs;
    *reinterpret_cast<float4 *>(x_out + id) = out;
}

static inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

int dit_cond_gather(const float *table, const int64_t *t, int B, float *temb, int *flag, hipStream_t stream) {
    hipLaunchKernelGGL(dit_cond_gather_kernel, dim3((unsigned)B), dim3(256), 0, stream, table, t, B, temb, flag);
    OT_LAUNCH_CHECK("dit_cond_gather");
    return OMNITOK_OK;
}

int dit_silu(float *x, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(dit_silu_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, x, n);
    OT_LAUNCH_CHECK("dit_silu");
    return OMNITOK_OK;
}

int dit_cond_combine(const float *temb2, const float *ytable, int y_rows, const int64_t *y, int B, int D, float *c, int *flag,
                     hipStream_t stream) {
    hipLaunchKernelGGL(dit_cond_combine_kernel, dim3((unsigned)B), dim3(256), 0, stream, temb2, ytable, y_rows, y, B, D, c, flag);
    OT_LAUNCH_CHECK("dit_cond_combine");
    return OMNITOK_OK;
}

int dit_cfg_blend(float *out, int B, int Cout, int channels, int64_t HW, float s, hipStream_t stream) {
    const int half = B / 2, nc = Cout < channels ? Cout : channels;
    hipLaunchKernelGGL(dit_cfg_blend_kernel, dim3(blocks_for((int64_t)half * nc * HW, 256)), dim3(256), 0, stream, out, half, Cout, nc, HW, s);
    OT_LAUNCH_CHECK("dit_cfg_blend");
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

// the grid of every kernel here is a 32-bit count of 256-thread workgroups
#define DIT_CHECK_GRID(who, elems) OT_CHECK_ARG((elems) / 256 < (1ll << 31) - 1, "%s: too many elements (%lld)", who, (long long)(elems))

extern "C" int omnitok_dit_patch_embed(const float *x, int x_batch, const float *w, const float *bias, const float *pos, int B, int C,
                                       int H, int p, int D, float *out, omnitok_stream_t stream) {
    OT_CHECK_ARG(x && w && bias && pos && out, "dit_patch_embed: null pointer");
    OT_CHECK_ARG(B >= 1 && C >= 1 && p >= 1 && H >= p && D >= 1 && x_batch >= 1 && x_batch <= B,
                 "dit_patch_embed: B %d, C %d, H %d, p %d, D %d, x_batch %d", B, C, H, p, D, x_batch);
    OT_CHECK_ARG(H % p == 0, "dit_patch_embed: input_size %d is not a multiple of patch_size %d", H, p);
    OT_CHECK_ARG((int64_t)p * p * C <= PE_KMAX, "dit_patch_embed: p * p * C = %lld (<= %d)", (long long)p * p * C, PE_KMAX);
    const int N = (H / p) * (H / p);
    const int64_t M = (int64_t)B * N;
    DIT_CHECK_GRID("dit_patch_embed", M * 256 / PE_TOK);
    hipLaunchKernelGGL(dit_patch_embed_kernel, dim3(blocks_for(M, PE_TOK)), dim3(256), 0, static_cast<hipStream_t>(stream), x, x_batch, w,
                       bias, pos, M, N, C, H, p, D, out);
    OT_LAUNCH_CHECK("dit_patch_embed");
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_ln_modulate(const float *x, const float *shift, const float *scale, int64_t ld_mod, int64_t rows, int n_tokens,
                                       int D, float *out, omnitok_stream_t stream) {
    OT_CHECK_ARG(x && shift && scale && out, "dit_ln_modulate: null pointer");
    OT_CHECK_ARG(rows >= 1 && n_tokens >= 1 && D >= 4 && D % 4 == 0 && ld_mod % 4 == 0 && ld_mod >= 0,
                 "dit_ln_modulate: rows %lld, n_tokens %d, D %d (%% 4 == 0), ld_mod %lld (%% 4 == 0)", (long long)rows, n_tokens, D,
                 (long long)ld_mod);
    OT_CHECK_ARG(aligned16(x) && aligned16(shift) && aligned16(scale) && aligned16(out), "dit_ln_modulate: unaligned pointer (16 bytes)");
    DIT_CHECK_GRID("dit_ln_modulate", rows * 64);
    hipLaunchKernelGGL(dit_ln_modulate_kernel<float>, dim3(blocks_for(rows, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, shift,
                       scale, ld_mod, rows, n_tokens, D, out, nullptr);
    OT_LAUNCH_CHECK("dit_ln_modulate");
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_ln_modulate16(const float *x, const float *shift, const float *scale, int64_t ld_mod, int64_t rows,
                                         int n_tokens, int D, int fmt, void *out16, int *flag, omnitok_stream_t stream) {
    OT_CHECK_ARG(fmt == OMNITOK_DIT_LIN_BF16 || fmt == OMNITOK_DIT_LIN_FP16, "dit_ln_modulate16: fmt %d (OMNITOK_DIT_LIN_BF16 | _FP16)", fmt);
    OT_CHECK_ARG(x && shift && scale && out16 && (flag || fmt != OMNITOK_DIT_LIN_FP16), "dit_ln_modulate16: null pointer");
    OT_CHECK_ARG(rows >= 1 && n_tokens >= 1 && D >= 4 && D % 4 == 0 && ld_mod % 4 == 0 && ld_mod >= 0,
                 "dit_ln_modulate16: rows %lld, n_tokens %d, D %d (%% 4 == 0), ld_mod %lld (%% 4 == 0)", (long long)rows, n_tokens, D,
                 (long long)ld_mod);
    OT_CHECK_ARG(aligned16(x) && aligned16(shift) && aligned16(scale) && aligned16(out16) && (reinterpret_cast<uintptr_t>(flag) & 3) == 0,
                 "dit_ln_modulate16: unaligned pointer (16 bytes)");
    DIT_CHECK_GRID("dit_ln_modulate16", rows * 64);
    if (fmt == OMNITOK_DIT_LIN_BF16)
        hipLaunchKernelGGL(dit_ln_modulate_kernel<lm_bf16>, dim3(blocks_for(rows, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                           shift, scale, ld_mod, rows, n_tokens, D, out16, flag);
    else
        hipLaunchKernelGGL(dit_ln_modulate_kernel<lm_fp16>, dim3(blocks_for(rows, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                           shift, scale, ld_mod, rows, n_tokens, D, out16, flag);
    OT_LAUNCH_CHECK("dit_ln_modulate16");
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_round16(const float *src, int fmt, void *dst16, int64_t n, int *flag, omnitok_stream_t stream) {
    OT_CHECK_ARG(fmt == OMNITOK_DIT_LIN_BF16 || fmt == OMNITOK_DIT_LIN_FP16, "dit_round16: fmt %d (OMNITOK_DIT_LIN_BF16 | _FP16)", fmt);
    OT_CHECK_ARG(src && dst16 && (flag || fmt != OMNITOK_DIT_LIN_FP16), "dit_round16: null pointer");
    OT_CHECK_ARG(n >= 4 && n % 4 == 0, "dit_round16: n %lld (%% 4 == 0)", (long long)n);
    OT_CHECK_ARG(aligned16(src) && aligned16(dst16) && (reinterpret_cast<uintptr_t>(flag) & 3) == 0, "dit_round16: unaligned pointer (16 bytes)");
    DIT_CHECK_GRID("dit_round16", n / 4);
    unsigned short *dst = static_cast<unsigned short *>(dst16);
    if (fmt == OMNITOK_DIT_LIN_BF16)
        hipLaunchKernelGGL(dit_round16_kernel<lm_bf16>, dim3(blocks_for(n / 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src, dst,
                           n / 4, flag);
    else
        hipLaunchKernelGGL(dit_round16_kernel<lm_fp16>, dim3(blocks_for(n / 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src, dst,
                           n / 4, flag);
    OT_LAUNCH_CHECK("dit_round16");
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_gate_residual(float *x, const float *y, const float *gate, int64_t ld_gate, int64_t rows, int n_tokens, int D,
                                         omnitok_stream_t stream) {
    OT_CHECK_ARG(x && y && gate, "dit_gate_residual: null pointer");
    OT_CHECK_ARG(rows >= 1 && n_tokens >= 1 && D >= 4 && D % 4 == 0 && ld_gate % 4 == 0 && ld_gate >= 0,
                 "dit_gate_residual: rows %lld, n_tokens %d, D %d (%% 4 == 0), ld_gate %lld (%% 4 == 0)", (long long)rows, n_tokens, D,
                 (long long)ld_gate);
    OT_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(gate), "dit_gate_residual: unaligned pointer (16 bytes)");
    const int64_t n = rows * (D / 4);
    DIT_CHECK_GRID("dit_gate_residual", n);
    hipLaunchKernelGGL(dit_gate_residual_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, gate, ld_gate,
                       rows, n_tokens, D);
    OT_LAUNCH_CHECK("dit_gate_residual");
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_gelu_tanh(float *x, int64_t n, omnitok_stream_t stream) {
    OT_CHECK_ARG(x && n >= 1, "dit_gelu_tanh: null pointer or n %lld", (long long)n);
    DIT_CHECK_GRID("dit_gelu_tanh", n);
    hipLaunchKernelGGL(dit_gelu_tanh_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, n);
    OT_LAUNCH_CHECK("dit_gelu_tanh");
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_unpatchify(const float *lin, int B, int N, int p, int Cout, float *out, omnitok_stream_t stream) {
    OT_CHECK_ARG(lin && out, "dit_unpatchify: null pointer");
    OT_CHECK_ARG(B >= 1 && N >= 1 && p >= 1 && Cout >= 1, "dit_unpatchify: B %d, N %d, p %d, Cout %d", B, N, p, Cout);
    const int gw = (int)lround(sqrt((double)N));
    OT_CHECK_ARG(gw * gw == N, "dit_unpatchify: N %d is not a square", N);
    const int64_t total = (int64_t)B * Cout * N * p * p;
    DIT_CHECK_GRID("dit_unpatchify", total);
    hipLaunchKernelGGL(dit_unpatchify_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), lin, total, gw, p,
                       Cout, out);
    OT_LAUNCH_CHECK("dit_unpatchify");
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_p_sample(const float *model_out, const float *x, const float *noise, const float *coef, int n_steps,
                                    const int64_t *t, int B, int C, int64_t HW, int learned_range, int clip, float *x_prev,
                                    float *pred_xstart, omnitok_stream_t stream) {
    OT_CHECK_ARG(model_out && x && noise && coef && t && x_prev, "dit_p_sample: null pointer");
    OT_CHECK_ARG(n_steps >= 1 && B >= 1 && C >= 1 && HW >= 1, "dit_p_sample: n_steps %d, B %d, C %d, HW %lld", n_steps, B, C, (long long)HW);
    const int64_t total = (int64_t)B * C * HW;
    DIT_CHECK_GRID("dit_p_sample", total);
    hipLaunchKernelGGL(dit_p_sample_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), model_out, x, noise,
                       coef, n_steps, t, total, C, HW, learned_range != 0, clip != 0, x_prev, pred_xstart);
    OT_LAUNCH_CHECK("dit_p_sample");
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_ddim_step(const float *model_out, const float *x, const float *noise, const float *coef, int n_steps,
                                     const int64_t *t, int B, int C, int64_t HW, int learned_range, int clip, int reverse, float *x_out,
                                     float *pred_xstart, omnitok_stream_t stream) {
    OT_CHECK_ARG(model_out, "dit_ddim_step: model_out is null");
    OT_CHECK_ARG(x, "dit_ddim_step: x is null");
    OT_CHECK_ARG(coef, "dit_ddim_step: coef is null");
    OT_CHECK_ARG(t, "dit_ddim_step: t is null");
    OT_CHECK_ARG(x_out, "dit_ddim_step: x_out is null");
    OT_CHECK_ARG(n_steps >= 1, "dit_ddim_step: n_steps %d (>= 1)", n_steps);
    OT_CHECK_ARG(B >= 1, "dit_ddim_step: B %d (>= 1)", B);
    OT_CHECK_ARG(C >= 1, "dit_ddim_step: C %d (>= 1)", C);
    OT_CHECK_ARG(HW >= 1, "dit_ddim_step: HW %lld (>= 1)", (long long)HW);
    OT_CHECK_ARG(HW <= INT64_MAX / C / B, "dit_ddim_step: too many elements (B %d, C %d, HW %lld)", B, C, (long long)HW);
    const int64_t chw = (int64_t)C * HW, total = (int64_t)B * chw;
    DIT_CHECK_GRID("dit_ddim_step", total);
    if (reverse) noise = nullptr;
    const int mo_mul = learned_range ? 2 : 1;
    const bool vec = chw % 4 == 0 && aligned16(model_out) && aligned16(x) && aligned16(noise) && aligned16(x_out) && aligned16(pred_xstart);
    if (vec)
        hipLaunchKernelGGL(dit_ddim_step4_kernel, dim3(blocks_for(total / 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), model_out, x,
                           noise, coef, n_steps, t, total / 4, chw, mo_mul, clip != 0, reverse != 0, x_out, pred_xstart);
    else
        hipLaunchKernelGGL(dit_ddim_step_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), model_out, x,
                           noise, coef, n_steps, t, total, chw, mo_mul, clip != 0, reverse != 0, x_out, pred_xstart);
    OT_LAUNCH_CHECK("dit_ddim_step");
    return OMNITOK_OK;
}
