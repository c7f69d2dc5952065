// LPIPS (the reference's OmniTokenizer/modules/lpips.py, taming's VGG16 LPIPS: the tokenizer's perceptual model): the
// input path and the per-slice head.  The VGG16 trunk between them is omnitok_conv2d / omnitok_maxpool2d of
// csrc/inception.hip, unchanged (include/omnitok.h "LPIPS").
//
//   lpips_preprocess_kernel   one operand (omnitok_metrics_operand: any b / t / c / h / w strides, fp32 or uint8) ->
//     out[n, H, W, 4] fp32 channels-last, image (b, t) = row b * F + t - i0; channel 3 = 0, so the first conv reads whole
//     16-byte taps.  Each step rounded in fp32, in this order:
//       v = x + shift (fp32) or v = u / 255 (common.h's table) + shift (uint8); then min(max(v, 0), 1) if clamp;
//       v = 2 v - 1 if OMNITOK_LPIPS_NORMALIZE (lpips' normalize=True);
//       v = (v - shift_c) / scale_c, a true division (ScalingLayer.forward; shift_c, scale_c from the checkpoint).
//     Equal bits to the same torch ops on the explicitly converted fp32 tensor.
//
//   lpips_layer_kernel   one VGG slice's head, feats[2N, h, w, C] (image n paired with image N + n).  Per pixel, 16 lanes
//     own the pixel; lane l holds the 16-byte channel groups c4 = l, l + 16, l + 32, ... in that order:
//       sa = sum_c a_c^2, sb = sum_c b_c^2      lane partials in (c4, component) order, then a xor butterfly over the 16
//                                               lanes (offsets 8, 4, 2, 1); every lane ends with the same bits
//       na = sqrt(sa) + 1e-10, nb likewise       normalize_tensor's norm_factor + eps
//       v  = sum_c w_c * ((a_c / na - b_c / nb)^2)   the same lane order and butterfly; all fp32, no contraction
//     An all-zero pixel gives na = 1e-10 and a_c / na = 0: 0, not NaN.  The spatial mean: the pixels of a pair are cut
//     into strips of LP_STRIP consecutive pixels; group g of a strip's block adds pixels g, g + 16, ... of the strip, in
//     order, to an fp64 sum; the 16 group sums are added in order into work[n][strip].
//   lpips_mean_kernel   one thread per pair: the strip sums in order, / (h w) in fp64 -> res[n][layer].
//   lpips_finalize_kernel   val[n] = fp32(((((res0 + res1) + res2) + res3) + res4)) (LPIPS.forward's val += res[l]).
// The strips depend on h and w alone, so a pair's scores do not depend on N, on a chunking of the batch or on the grid.
#include "common.h"

#include <math.h>

namespace omnitok {

__constant__ U8Unit k_lpips_unit = make_u8_unit();

constexpr int LP_THREADS = 256;
constexpr int LP_LANES = 16;                         // lanes per pixel
constexpr int LP_GROUPS = LP_THREADS / LP_LANES;     // pixels in flight per block
constexpr int LP_STRIP = 64;                         // pixels per strip (4 per group): enough blocks on 16 x 16 maps
constexpr int LP_MAX_C = 512;
constexpr int LP_MAX_J = LP_MAX_C / 4 / LP_LANES;    // 16-byte groups per lane at C = 512

struct LpOp {
    const void *p;
    int64_t s[5];
    int u8, clamp;
    float shift;
};

// grid (ceil(H W / 256), n)
__global__ __launch_bounds__(256) void lpips_preprocess_kernel(const LpOp o, int F, int H, int W, int i0, int normalize,
                                                               float sh0, float sh1, float sh2, float sc0, float sc1,
                                                               float sc2, float *__restrict__ out) {
#pragma clang fp contract(off)
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= H * W) return;
    const int y = px / W, x = px - y * W;
    const int64_t i = (int64_t)i0 + blockIdx.y;
    const int64_t b = i / F, t = i - b * F;
    const int64_t base = b * o.s[0] + t * o.s[1] + (int64_t)y * o.s[3] + (int64_t)x * o.s[4];
    const float sh[3] = {sh0, sh1, sh2}, sc[3] = {sc0, sc1, sc2};
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t off = base + c * o.s[2];
        float v = o.u8 ? k_lpips_unit.v[static_cast<const uint8_t *>(o.p)[off]] : static_cast<const float *>(o.p)[off];
        v = v + o.shift;
        if (o.clamp) v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
        if (normalize) v = 2.0f * v - 1.0f;
        r[c] = (v - sh[c]) / sc[c];
    }
    r[3] = 0.0f;
    *reinterpret_cast<f32x4 *>(out + ((int64_t)blockIdx.y * H * W + px) * 4) = r;
}

__device__ __forceinline__ float lp_group_sum(float v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = LP_LANES / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

// grid (nstrips, N)
__global__ __launch_bounds__(LP_THREADS) void lpips_layer_kernel(const float *__restrict__ feats, int N, int hw, int C4,
                                                                 const float *__restrict__ lin_w, int nstrips,
                                                                 double *__restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[LP_GROUPS];
    const int tid = threadIdx.x, lane = tid % LP_LANES, g = tid / LP_LANES;
    const int strip = blockIdx.x, n = blockIdx.y;
    const int p1 = min(hw, (strip + 1) * LP_STRIP);
    const float *fa = feats + (int64_t)n * hw * C4 * 4;
    const float *fb = feats + (int64_t)(N + n) * hw * C4 * 4;
    f32x4 w[LP_MAX_J];
#pragma unroll
    for (int j = 0; j < LP_MAX_J; ++j) {
        const int c4 = lane + LP_LANES * j;
        w[j] = c4 < C4 ? *reinterpret_cast<const f32x4 *>(lin_w + 4 * c4) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    double acc = 0.0;
    for (int p = strip * LP_STRIP + g; p < p1; p += LP_GROUPS) {  // trip count uniform over the 16 lanes of a group
        f32x4 a[LP_MAX_J], b[LP_MAX_J];
        float sa = 0.0f, sb = 0.0f;
#pragma unroll
        for (int j = 0; j < LP_MAX_J; ++j) {
            const int c4 = lane + LP_LANES * j;
            if (c4 < C4) {
                a[j] = *reinterpret_cast<const f32x4 *>(fa + ((int64_t)p * C4 + c4) * 4);
                b[j] = *reinterpret_cast<const f32x4 *>(fb + ((int64_t)p * C4 + c4) * 4);
            } else {
                a[j] = b[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
#pragma unroll
        for (int j = 0; j < LP_MAX_J; ++j) {
            if (lane + LP_LANES * j >= C4) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sa = sa + a[j][k] * a[j][k];
                sb = sb + b[j][k] * b[j][k];
            }
        }
        sa = lp_group_sum(sa);
        sb = lp_group_sum(sb);
        const float na = sqrtf(sa) + 1e-10f, nb = sqrtf(sb) + 1e-10f;
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < LP_MAX_J; ++j) {
            if (lane + LP_LANES * j >= C4) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = a[j][k] / na - b[j][k] / nb;
                s = s + w[j][k] * (d * d);
            }
        }
        acc += (double)lp_group_sum(s);
    }
    if (lane == 0) red[g] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < LP_GROUPS; ++k) t += red[k];
        part[(int64_t)n * nstrips + strip] = t;
    }
}

// one thread per pair
__global__ __launch_bounds__(256) void lpips_mean_kernel(const double *__restrict__ part, int N, int nstrips, int hw,
                                                         int layer, double *__restrict__ res) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double t = 0.0;
    for (int k = 0; k < nstrips; ++k) t += part[(int64_t)n * nstrips + k];
    res[(int64_t)n * 5 + layer] = t / (double)hw;
}

__global__ __launch_bounds__(256) void lpips_finalize_kernel(const double *__restrict__ res, int N, float *__restrict__ val) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const double *r = res + (int64_t)n * 5;
    val[n] = (float)((((r[0] + r[1]) + r[2]) + r[3]) + r[4]);
}

static int lp_strips(int h, int w) { return (int)(((int64_t)h * w + LP_STRIP - 1) / LP_STRIP); }

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_lpips_preprocess(const omnitok_metrics_operand *src, int B, int F, int H, int W, int i0, int n,
                                        int flags, const float *shift, const float *scale, float *out,
                                        omnitok_stream_t stream_) {
    OT_CHECK_ARG((flags & ~OMNITOK_LPIPS_NORMALIZE) == 0, "lpips_preprocess: flags 0x%x", flags);
    OT_CHECK_ARG(B >= 0 && F >= 1 && (int64_t)B * F <= (1ll << 31) - 1, "lpips_preprocess: bad sizes B %d F %d", B, F);
    OT_CHECK_ARG(H >= OMNITOK_LPIPS_MIN_SIZE && W >= OMNITOK_LPIPS_MIN_SIZE && (int64_t)H * W <= (1ll << 28),
                 "lpips_preprocess: %d x %d frames: at least 16 x 16 (the reference's fifth slice needs four 2 x 2 pools)", H,
                 W);
    OT_CHECK_ARG(i0 >= 0 && n >= 0 && n <= 65535 && (int64_t)i0 + n <= (int64_t)B * F,
                 "lpips_preprocess: images [%d, %d + %d) outside the %lld of the operand (at most 65535 per call)", i0, i0, n,
                 (long long)B * F);
    OT_CHECK_ARG(src, "lpips_preprocess: null pointer (operand)");
    OT_CHECK_ARG(src->dtype == OMNITOK_METRICS_F32 || src->dtype == OMNITOK_METRICS_U8,
                 "lpips_preprocess: element type %d", src->dtype);
    for (int k = 0; k < 5; ++k)
        OT_CHECK_ARG(src->stride[k] >= 0, "lpips_preprocess: negative stride %lld (dim %d)", (long long)src->stride[k], k);
    OT_CHECK_ARG(src->clamp == 0 || src->clamp == 1, "lpips_preprocess: clamp %d, expected 0 or 1", src->clamp);
    OT_CHECK_ARG(__builtin_isfinite(src->shift), "lpips_preprocess: shift is not finite");
    OT_CHECK_ARG(shift && scale, "lpips_preprocess: null pointer (ScalingLayer shift / scale)");
    for (int c = 0; c < 3; ++c)
        OT_CHECK_ARG(__builtin_isfinite(shift[c]) && __builtin_isfinite(scale[c]) && scale[c] != 0.0f,
                     "lpips_preprocess: ScalingLayer channel %d: shift %g, scale %g (finite, scale non-zero)", c,
                     (double)shift[c], (double)scale[c]);
    if (n == 0) return OMNITOK_OK;
    OT_CHECK_ARG(src->data && out, "lpips_preprocess: null pointer");
    OT_CHECK_ARG(aligned16(out), "lpips_preprocess: out must be 16-byte aligned");
    LpOp o{};
    o.p = src->data;
    for (int k = 0; k < 5; ++k) o.s[k] = src->stride[k];
    o.u8 = src->dtype == OMNITOK_METRICS_U8;
    o.clamp = src->clamp;
    o.shift = src->shift;
    const dim3 grid((unsigned)(((int64_t)H * W + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(lpips_preprocess_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), o, F, H, W, i0,
                       (flags & OMNITOK_LPIPS_NORMALIZE) ? 1 : 0, shift[0], shift[1], shift[2], scale[0], scale[1],
                       scale[2], out);
    OT_LAUNCH_CHECK("lpips_preprocess");
    return OMNITOK_OK;
}

extern "C" int64_t omnitok_lpips_workspace(int N, int h, int w) {
    if (N < 0 || h < 1 || w < 1 || (int64_t)h * w > (1ll << 28)) return -1;
    return (int64_t)N * lp_strips(h, w) * (int64_t)sizeof(double);
}

extern "C" int omnitok_lpips_layer(const float *feats, int N, int h, int w, int C, const float *lin_w, int layer, void *work,
                                   size_t work_bytes, double *res, omnitok_stream_t stream_) {
    OT_CHECK_ARG(N >= 0 && N <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= (1ll << 28),
                 "lpips_layer: bad sizes N %d h %d w %d", N, h, w);
    OT_CHECK_ARG(C >= 4 && C <= LP_MAX_C && C % 4 == 0, "lpips_layer: C %d outside 4..512 or not a multiple of 4", C);
    OT_CHECK_ARG(layer >= 0 && layer < 5, "lpips_layer: layer %d outside 0..4", layer);
    if (N == 0) return OMNITOK_OK;
    OT_CHECK_ARG(feats && lin_w && res, "lpips_layer: null pointer");
    OT_CHECK_ARG(aligned16(feats) && aligned16(lin_w), "lpips_layer: feats and lin_w must be 16-byte aligned");
    OT_CHECK_ARG(2ll * N * h * w * C < (1ll << 40), "lpips_layer: too large");
    const int64_t need = omnitok_lpips_workspace(N, h, w);
    OT_CHECK_ARG(work, "lpips_layer: null pointer (work, %lld bytes needed)", (long long)need);
    OT_CHECK_ARG(work_bytes >= (size_t)need, "lpips_layer: workspace of %zu bytes, %lld needed", work_bytes, (long long)need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int nstrips = lp_strips(h, w);
    double *part = static_cast<double *>(work);
    hipLaunchKernelGGL(lpips_layer_kernel, dim3((unsigned)nstrips, (unsigned)N), dim3(LP_THREADS), 0, stream, feats, N, h * w,
                       C / 4, lin_w, nstrips, part);
    OT_LAUNCH_CHECK("lpips_layer");
    hipLaunchKernelGGL(lpips_mean_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const double *>(part), N, nstrips, h * w, layer, res);
    OT_LAUNCH_CHECK("lpips_mean");
    return OMNITOK_OK;
}

extern "C" int omnitok_lpips_finalize(const double *res, int N, float *val, omnitok_stream_t stream_) {
    OT_CHECK_ARG(N >= 0, "lpips_finalize: N %d", N);
    if (N == 0) return OMNITOK_OK;
    OT_CHECK_ARG(res && val, "lpips_finalize: null pointer");
    hipLaunchKernelGGL(lpips_finalize_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), res, N, val);
    OT_LAUNCH_CHECK("lpips_finalize");
    return OMNITOK_OK;
}
