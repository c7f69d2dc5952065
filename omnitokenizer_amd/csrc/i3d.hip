// I3D (InceptionI3d of the reference's fvd/pytorch_i3d.py), the feature net of FVD: its four kernel families.  Activations
// are fp32 and channels-last, [B, T, H, W, C]; every layer reads a channel slice of its input and writes a channel slice of
// its output (include/omnitok.h "I3D").
//
//   i3d_preprocess_kernel   uint8 [B, T, H, W, 3] -> fp32 [B, T, R_h, R_w, 4]: fvd.py preprocess, i.e.
//     F.interpolate(float(u), (R_h, R_w), 'bilinear', align_corners=False), then 2 * v / 255 - 1 (each step rounded in fp32),
//     channel 3 = 0.  The source index / lambda arithmetic and the tap order are those of frames.hip's BILINEAR mode, on the
//     values 0..255 instead of u / 255; where the size does not change the taps are (v, 1, 0) and the result is exact.
//
//   conv3d_same_kernel<WMT, WNT, WN> (csrc/convnet_common.h, shared with csrc/inception.hip)   one Unit3D: TF "same" padding (Unit3D.compute_pad: the front gets pad // 2, the back the
//     rest), conv3d, the folded BatchNorm's bias and an optional ReLU, as an implicit GEMM on v_mfma_f32_32x32x2_f32:
//       M = output positions (b, t, h, w), N = Cout, K = taps x Cin, k = tap * Cin + ci, tap = (dt * kh + dh) * kw + dw.
//     A (BM x 32) is gathered from the input on the fly (zeros outside it: the pad); B is the packed weight [Cout][Kpad].
//     The tile / LDS / K-permutation design is gemm.hip's: 4 waves as 2 x 2, wave tile (32 WMT) x (32 WNT), BK = 32,
//     register-staged double buffer (the next step's loads are issued before this step's MFMAs), LDS rows of 36 floats.
//     A thread loads one 16-byte group of 4 consecutive k (one tap, 4 channels: Cin % 4 == 0) for BM / 32 rows; its
//     (tap, ci) advances incrementally, so there is no division in the K loop.  Every output element is one MFMA chain over
//     k = 0 .. Kpad in the same order whatever the tile, the grid or B: a clip's outputs do not depend on the batch.
//     The epilogue adds the bias, applies the ReLU (NaN stays NaN) and routes columns n < split to (y, y_off) and the rest
//     to (y2, y2_off): an Inception module's three 1x1x1 convs of one input are one launch.
//
//   maxpool3d_same_kernel   MaxPool3dSamePadding: F.pad with zeros, then max_pool3d.  Taps in (t, h, w) order, torch's
//     rule `v > m || isnan(v)` from m = -inf: bit-identical to torch.
//
//   i3d_head_kernel   AvgPool3d([2, 7, 7], stride 1) (sum of the 98 taps in (t, h, w) order, / 98), the logits 1x1x1 conv
//     with bias (a k-ordered fma chain over C) and the mean over the pooled time steps (sum in t order, / T'): one block
//     per (clip, h', w').
#include "convnet_common.h"

namespace omnitok {

// TF "same" padding of one dimension (Unit3D.compute_pad / MaxPool3dSamePadding.compute_pad) and the extent it gives
static void same_pad(int s, int k, int stride, int &front, int &out) {
    const int r = s % stride;
    const int pad = std::max(k - (r == 0 ? stride : r), 0);
    front = pad / 2;
    out = (s + pad - k) / stride + 1;
}

// ---- preprocess --------------------------------------------------------------------------------------------------------

// grid (ceil(R_h * R_w / 256), T, B): one thread per output pixel
__global__ __launch_bounds__(256) void i3d_preprocess_kernel(const uint8_t *__restrict__ src, int T, int H, int W, int Rh,
                                                              int Rw, float sh, float sw, float *__restrict__ out) {
#pragma clang fp contract(off)
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= Rh * Rw) return;
    const int y = px / Rw, x = px % Rw;
    const int t = blockIdx.y, b = blockIdx.z;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    pre_src(sh, y, H, Rh, y0, y1, wy0, wy1);
    pre_src(sw, x, W, Rw, x0, x1, wx0, wx1);
    const uint8_t *f = src + ((int64_t)b * T + t) * H * W * 3;
    const uint8_t *r0 = f + (int64_t)y0 * W * 3, *r1 = f + (int64_t)y1 * W * 3;
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = pre_lerp((float)r0[3 * x0 + c], (float)r0[3 * x1 + c], wx0, wx1);
        const float bot = pre_lerp((float)r1[3 * x0 + c], (float)r1[3 * x1 + c], wx0, wx1);
        const float v = pre_lerp(top, bot, wy0, wy1);
        o[c] = 2.0f * v / 255.0f - 1.0f;
    }
    o[3] = 0.0f;
    *reinterpret_cast<f32x4 *>(out + (((int64_t)b * T + t) * Rh * Rw + px) * 4) = o;
}

// ---- max pool ----------------------------------------------------------------------------------------------------------

struct MpArgs {
    const float *x;
    float *y;
    int T, H, W, C4, kt, kh, kw, st, sh, sw, pt, ph, pw, To, Ho, Wo;
    int64_t n;  // B * To * Ho * Wo * C4
};

__device__ __forceinline__ float mp_take(float m, float v) { return (v > m || isnan(v)) ? v : m; }

__global__ __launch_bounds__(256) void maxpool3d_same_kernel(const MpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int c4 = (int)(i % a.C4);
    int64_t r = i / a.C4;
    const int wo = (int)(r % a.Wo);
    r /= a.Wo;
    const int ho = (int)(r % a.Ho);
    r /= a.Ho;
    const int to = (int)(r % a.To);
    const int64_t b = r / a.To;
    const float *xb = a.x + b * a.T * a.H * a.W * (int64_t)a.C4 * 4 + 4 * c4;
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int dt = 0; dt < a.kt; ++dt) {
        const int ti = to * a.st - a.pt + dt;
        for (int dh = 0; dh < a.kh; ++dh) {
            const int yi = ho * a.sh - a.ph + dh;
            for (int dw = 0; dw < a.kw; ++dw) {
                const int xi = wo * a.sw - a.pw + dw;
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};  // F.pad's zeros
                if ((unsigned)ti < (unsigned)a.T && (unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W)
                    v = *reinterpret_cast<const f32x4 *>(xb + (((int64_t)ti * a.H + yi) * a.W + xi) * a.C4 * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) m[c] = mp_take(m[c], v[c]);
            }
        }
    }
    *reinterpret_cast<f32x4 *>(a.y + i * 4) = m;
}

// ---- head --------------------------------------------------------------------------------------------------------------

constexpr int HD_MAX_C = 2048;     // channels the pooled vector of one step may have (LDS)
constexpr int HD_MAX_SLOTS = 4;    // classes per thread: num_classes <= 1024

// grid (Hp * Wp, B), 256 threads
__global__ __launch_bounds__(256) void i3d_head_kernel(const float *__restrict__ x, int T, int H, int W, int C,
                                                       const float *__restrict__ wt, const float *__restrict__ bias, int ncls,
                                                       float *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float pooled[HD_MAX_C];
    const int Tp = T - 1, Hp = H - 6, Wp = W - 6;
    const int pos = blockIdx.x, b = blockIdx.y;
    const int py = pos / Wp, pxx = pos % Wp;
    const float *xb = x + (int64_t)b * T * H * W * C;
    float sum[HD_MAX_SLOTS] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = 0; t < Tp; ++t) {
        for (int c = threadIdx.x; c < C; c += 256) {
            float s = 0.0f;
            for (int dt = 0; dt < 2; ++dt)
                for (int dh = 0; dh < 7; ++dh)
                    for (int dw = 0; dw < 7; ++dw)
                        s += xb[(((int64_t)(t + dt) * H + py + dh) * W + pxx + dw) * C + c];
            pooled[c] = s / 98.0f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < HD_MAX_SLOTS; ++j) {
            const int n = threadIdx.x + 256 * j;
            if (n >= ncls) break;
            float acc = 0.0f;
            for (int k = 0; k < C; ++k) acc = __builtin_fmaf(pooled[k], wt[(int64_t)k * ncls + n], acc);
            sum[j] += acc + bias[n];
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < HD_MAX_SLOTS; ++j) {
        const int n = threadIdx.x + 256 * j;
        if (n >= ncls) break;
        out[(((int64_t)b * ncls + n) * Hp + py) * Wp + pxx] = sum[j] / (float)Tp;
    }
}

}  // namespace omnitok

using namespace omnitok;

extern "C" void omnitok_same_pad(int s, int k, int stride, int *front, int *out) {
    int f = 0, o = 0;
    if (s >= 1 && k >= 1 && stride >= 1) same_pad(s, k, stride, f, o);
    if (front) *front = f;
    if (out) *out = o;
}

extern "C" int64_t omnitok_conv3d_packed_ldw(int Cin, int kt, int kh, int kw) {
    if (Cin < 4 || Cin % 4 || kt < 1 || kh < 1 || kw < 1 || kt > 7 || kh > 7 || kw > 7 || Cin > (1 << 16)) return -1;
    const int64_t K = (int64_t)kt * kh * kw * Cin;
    return (K + CV_BK - 1) / CV_BK * CV_BK;
}

extern "C" int omnitok_i3d_preprocess(const uint8_t *frames, int B, int T, int H, int W, int R_h, int R_w, float *out,
                                      omnitok_stream_t stream_) {
    OT_CHECK_ARG(B >= 0 && B <= 65535 && T >= 1 && T <= 65535 && H >= 1 && W >= 1 && R_h >= 1 && R_w >= 1 &&
                     (int64_t)H * W <= (1ll << 30) && (int64_t)R_h * R_w <= (1ll << 30),
                 "i3d_preprocess: bad sizes B %d T %d H %d W %d -> %d x %d", B, T, H, W, R_h, R_w);
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG(frames && out, "i3d_preprocess: null pointer");
    OT_CHECK_ARG(aligned16(out), "i3d_preprocess: out must be 16-byte aligned");
    const float sh = (float)H / (float)R_h, sw = (float)W / (float)R_w;  // torch's area_pixel_compute_scale
    const dim3 grid((unsigned)(((int64_t)R_h * R_w + 255) / 256), (unsigned)T, (unsigned)B);
    hipLaunchKernelGGL(i3d_preprocess_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), frames, T, H, W, R_h,
                       R_w, sh, sw, out);
    OT_LAUNCH_CHECK("i3d_preprocess");
    return OMNITOK_OK;
}

extern "C" int omnitok_conv3d_same(const omnitok_conv3d *c, omnitok_stream_t stream_) {
    OT_CHECK_ARG(c, "conv3d_same: null descriptor");
    OT_CHECK_ARG(c->B >= 0 && c->T >= 1 && c->H >= 1 && c->W >= 1 && c->Cout >= 1 && c->Cout <= 65536,
                 "conv3d_same: bad sizes B %d T %d H %d W %d Cout %d", c->B, c->T, c->H, c->W, c->Cout);
    const int64_t ldw = omnitok_conv3d_packed_ldw(c->Cin, c->kt, c->kh, c->kw);
    OT_CHECK_ARG(ldw > 0, "conv3d_same: Cin %d must be a positive multiple of 4 and the kernel %d x %d x %d within 1..7",
                 c->Cin, c->kt, c->kh, c->kw);
    OT_CHECK_ARG(c->st >= 1 && c->st <= 4 && c->sh >= 1 && c->sh <= 4 && c->sw >= 1 && c->sw <= 4,
                 "conv3d_same: strides %d x %d x %d outside 1..4", c->st, c->sh, c->sw);
    OT_CHECK_ARG(c->relu == 0 || c->relu == 1, "conv3d_same: relu %d", c->relu);
    CvArgs a{};
    a.T = c->T;
    a.H = c->H;
    a.W = c->W;
    a.ldw = ldw;
    a.kt = c->kt;
    a.kh = c->kh;
    a.kw = c->kw;
    a.st = c->st;
    a.sh = c->sh;
    a.sw = c->sw;
    same_pad(c->T, c->kt, c->st, a.pt, a.To);
    same_pad(c->H, c->kh, c->sh, a.ph, a.Ho);
    same_pad(c->W, c->kw, c->sw, a.pw, a.Wo);
    OT_CHECK_ARG(a.To >= 1 && a.Ho >= 1 && a.Wo >= 1, "conv3d_same: empty output");  // "same" padding: never, for sizes >= 1
    if (int rc = conv_args(c, "conv3d_same", c->B, a)) return rc;
    if (c->B == 0) return OMNITOK_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // the tile by Cout alone: 128 columns unless 64 pads less (a clip's results never depend on the tile)
    const int pad128 = (c->Cout + 127) / 128 * 128, pad64 = (c->Cout + 63) / 64 * 64;
    if (pad64 < pad128) return conv_launch<4, 1>(a, (a.M + 255) / 256, stream);
    return conv_launch<2, 2>(a, (a.M + 127) / 128, stream);
}

extern "C" int omnitok_maxpool3d_same(const float *x, int B, int T, int H, int W, int C, int kt, int kh, int kw, int st,
                                      int sh, int sw, float *y, omnitok_stream_t stream_) {
    OT_CHECK_ARG(B >= 0 && T >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "maxpool3d_same: bad sizes B %d T %d H %d "
                 "W %d C %d (C a positive multiple of 4)", B, T, H, W, C);
    OT_CHECK_ARG(kt >= 1 && kt <= 7 && kh >= 1 && kh <= 7 && kw >= 1 && kw <= 7 && st >= 1 && st <= 4 && sh >= 1 &&
                     sh <= 4 && sw >= 1 && sw <= 4,
                 "maxpool3d_same: kernel %d x %d x %d / stride %d x %d x %d outside 1..7 / 1..4", kt, kh, kw, st, sh, sw);
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG(x && y, "maxpool3d_same: null pointer");
    OT_CHECK_ARG(aligned16(x) && aligned16(y), "maxpool3d_same: x and y must be 16-byte aligned");
    MpArgs a{};
    a.x = x;
    a.y = y;
    a.T = T;
    a.H = H;
    a.W = W;
    a.C4 = C / 4;
    a.kt = kt;
    a.kh = kh;
    a.kw = kw;
    a.st = st;
    a.sh = sh;
    a.sw = sw;
    same_pad(T, kt, st, a.pt, a.To);
    same_pad(H, kh, sh, a.ph, a.Ho);
    same_pad(W, kw, sw, a.pw, a.Wo);
    OT_CHECK_ARG(a.To >= 1 && a.Ho >= 1 && a.Wo >= 1, "maxpool3d_same: empty output");
    a.n = (int64_t)B * a.To * a.Ho * a.Wo * a.C4;
    OT_CHECK_ARG((int64_t)B * T * H * W * C < (1ll << 40) && (a.n + 255) / 256 <= 0x7fffffff, "maxpool3d_same: too large");
    hipLaunchKernelGGL(maxpool3d_same_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), a);
    OT_LAUNCH_CHECK("maxpool3d_same");
    return OMNITOK_OK;
}

extern "C" int omnitok_i3d_head(const float *x, int B, int T, int H, int W, int C, const float *w_t, const float *bias,
                                int num_classes, float *out, omnitok_stream_t stream_) {
    OT_CHECK_ARG(B >= 0 && B <= 65535 && T >= 2 && H >= 7 && W >= 7 && C >= 1 && C <= HD_MAX_C,
                 "i3d_head: bad sizes B %d T %d H %d W %d C %d (T >= 2, H and W >= 7, C <= %d)", B, T, H, W, C, HD_MAX_C);
    OT_CHECK_ARG(num_classes >= 1 && num_classes <= 256 * HD_MAX_SLOTS, "i3d_head: num_classes %d outside 1..%d",
                 num_classes, 256 * HD_MAX_SLOTS);
    OT_CHECK_ARG((int64_t)(H - 6) * (W - 6) <= 0x7fffffff && (int64_t)B * T * H * W * C < (1ll << 40), "i3d_head: too large");
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG(x && w_t && bias && out, "i3d_head: null pointer");
    hipLaunchKernelGGL(i3d_head_kernel, dim3((unsigned)((H - 6) * (W - 6)), (unsigned)B), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x, T, H, W, C, w_t, bias, num_classes, out);
    OT_LAUNCH_CHECK("i3d_head");
    return OMNITOK_OK;
}
