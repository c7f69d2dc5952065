// Inception V3 (the FID feature net of the reference's evaluation/pytorch-fid, inception.py): its layer set around the
// implicit-GEMM convolution of csrc/convnet_common.h.  Activations are fp32 and channels-last, [N, H, W, C]; a conv reads a
// channel slice of its input and writes channel slices of its outputs (include/omnitok.h "Inception V3").
//
//   fid_preprocess_kernel<U8>   uint8 [N, H, W, 3] (rows `ld` bytes apart) or fp32 [N, 3, H, W] -> fp32 [N, R_h, R_w, 4]:
//     InceptionV3.forward's input path after ToTensor: v = u / 255 (common.h's table: ToTensor's division), then
//     F.interpolate(v, (R_h, R_w), 'bilinear', align_corners=False) if resize, then 2 * v - 1 if normalize, each step
//     rounded in fp32 and in that order (not I3D's order: I3D resizes 0..255 and scales after).  The source index / lambda
//     arithmetic and the tap order are i3d.hip's (pre_src / pre_lerp); where the size does not change the taps are
//     (v, 1, 0) and the result equals torch's bits.  Channel 3 = 0, so the first conv reads whole 16-byte taps.
//
//   omnitok_conv2d   BasicConv2d with its BatchNorm folded: conv3d_same_kernel with T = kt = 1, the explicit (pad_h, pad_w)
//     as its front pads and the floor output extent (the back pad is implicit: taps past the input read zeros).  The
//     epilogue adds the bias and applies the ReLU; the column split routes an Inception module's sibling 1x1 branches of one
//     input to two tensors in one launch.  The tile is chosen by the layer's shape alone: Cout <= 32 (Conv2d_1a / 2a) takes
//     the 4 x 1 wave layout (256 x 32 tiles), which leaves no MFMA column idle; maps of at most 17 x 17 take 64 x 64 tiles.
//
//   maxpool2d_kernel   max_pool2d(k, s, p): -inf padding (out-of-image taps are skipped), floor sizing; taps in (dy, dx)
//     order with torch's rule `v > m || isnan(v)` from m = -inf: bit-identical to torch, NaN included.  Writes a channel
//     slice, so B's and D's pool branch lands in the module output.
//
//   avgpool2d_kernel   avg_pool2d(k, s, p, count_include_pad=False): the fp32 sum of the in-image taps in (dy, dx) order
//     from 0, divided by their count.
//
//   spatial_mean_kernel   adaptive_avg_pool2d(x, 1) over [N, h, w, C] -> [N, C]: the fp32 sum over positions in (y, x)
//     order from 0, divided by h * w.
#include "convnet_common.h"

namespace omnitok {

__constant__ U8Unit kFidUnit = make_u8_unit();

// ---- preprocess --------------------------------------------------------------------------------------------------------

// grid (ceil(R_h * R_w / 256), N): one thread per output pixel.  U8: src is uint8 [N, H, W, 3] with rows ld bytes apart;
// else fp32 [N, 3, H, W] dense.
template <bool U8>
__global__ __launch_bounds__(256) void fid_preprocess_kernel(const void *__restrict__ src_, int64_t ld, int H, int W, int Rh,
                                                             int Rw, float sh, float sw, int resize, int normalize,
                                                             float *__restrict__ out) {
#pragma clang fp contract(off)
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= Rh * Rw) return;
    const int y = px / Rw, x = px % Rw;
    const int64_t b = blockIdx.y;
    auto tap = [&](int c, int yy, int xx) -> float {
        if constexpr (U8) {
            const uint8_t *s = static_cast<const uint8_t *>(src_) + b * H * ld;
            return kFidUnit.v[s[(int64_t)yy * ld + 3 * xx + c]];
        } else {
            const float *s = static_cast<const float *>(src_) + (b * 3 + c) * H * W;
            return s[(int64_t)yy * W + xx];
        }
    };
    f32x4 o;
    if (resize) {
        int y0, y1, x0, x1;
        float wy0, wy1, wx0, wx1;
        pre_src(sh, y, H, Rh, y0, y1, wy0, wy1);
        pre_src(sw, x, W, Rw, x0, x1, wx0, wx1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = pre_lerp(tap(c, y0, x0), tap(c, y0, x1), wx0, wx1);
            const float bot = pre_lerp(tap(c, y1, x0), tap(c, y1, x1), wx0, wx1);
            o[c] = pre_lerp(top, bot, wy0, wy1);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = tap(c, y, x);
    }
    if (normalize) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = 2.0f * o[c] - 1.0f;
    }
    o[3] = 0.0f;
    *reinterpret_cast<f32x4 *>(out + (b * Rh * Rw + px) * 4) = o;
}

// ---- pools -------------------------------------------------------------------------------------------------------------

struct Pool2dArgs {
    const float *x;
    float *y;
    int64_t y_cs;
    int y_off;
    int H, W, C4, k, s, p, Ho, Wo;
    int64_t n;  // N * Ho * Wo * C4
};

__device__ __forceinline__ float mp2_take(float m, float v) { return (v > m || isnan(v)) ? v : m; }

// one thread per (n, ho, wo, 4 channels)
__global__ __launch_bounds__(256) void maxpool2d_kernel(const Pool2dArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int c4 = (int)(i % a.C4);
    int64_t r = i / a.C4;
    const int wo = (int)(r % a.Wo);
    r /= a.Wo;
    const int ho = (int)(r % a.Ho);
    const int64_t b = r / a.Ho;
    const float *xb = a.x + b * a.H * a.W * (int64_t)a.C4 * 4 + 4 * c4;
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int dh = 0; dh < a.k; ++dh) {
        const int yi = ho * a.s - a.p + dh;
        if ((unsigned)yi >= (unsigned)a.H) continue;
        for (int dw = 0; dw < a.k; ++dw) {
            const int xi = wo * a.s - a.p + dw;
            if ((unsigned)xi >= (unsigned)a.W) continue;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(xb + ((int64_t)yi * a.W + xi) * a.C4 * 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) m[c] = mp2_take(m[c], v[c]);
        }
    }
    float *dst = a.y + (((b * a.Ho + ho) * a.Wo + wo) * a.y_cs + a.y_off + 4 * c4);
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[c] = m[c];
}

__global__ __launch_bounds__(256) void avgpool2d_kernel(const Pool2dArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int c4 = (int)(i % a.C4);
    int64_t r = i / a.C4;
    const int wo = (int)(r % a.Wo);
    r /= a.Wo;
    const int ho = (int)(r % a.Ho);
    const int64_t b = r / a.Ho;
    const float *xb = a.x + b * a.H * a.W * (int64_t)a.C4 * 4 + 4 * c4;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    int cnt = 0;
    for (int dh = 0; dh < a.k; ++dh) {
        const int yi = ho * a.s - a.p + dh;
        if ((unsigned)yi >= (unsigned)a.H) continue;
        for (int dw = 0; dw < a.k; ++dw) {
            const int xi = wo * a.s - a.p + dw;
            if ((unsigned)xi >= (unsigned)a.W) continue;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(xb + ((int64_t)yi * a.W + xi) * a.C4 * 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c] = s[c] + v[c];
            ++cnt;
        }
    }
    const float d = (float)cnt;
    float *dst = a.y + (((b * a.Ho + ho) * a.Wo + wo) * a.y_cs + a.y_off + 4 * c4);
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[c] = s[c] / d;
}

// grid (ceil(C4 / 256), N): one thread per (image, 4 channels); consecutive threads read consecutive 16-byte groups
__global__ __launch_bounds__(256) void spatial_mean_kernel(const float *__restrict__ x, int HW, int C4,
                                                           float *__restrict__ y) {
#pragma clang fp contract(off)
    const int c4 = blockIdx.x * 256 + threadIdx.x;
    if (c4 >= C4) return;
    const int64_t b = blockIdx.y;
    const float *xb = x + b * HW * (int64_t)C4 * 4 + 4 * c4;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int p = 0; p < HW; ++p) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(xb + (int64_t)p * C4 * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = s[c] + v[c];
    }
    const float d = (float)HW;
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = s[c] / d;
    *reinterpret_cast<f32x4 *>(y + (b * C4 + c4) * 4) = o;
}

// floor output extent of a (k, s, p) window over s_in; 0 where there is none
static int pool_out(int s_in, int k, int s, int p) {
    const int span = s_in + 2 * p - k;
    return span < 0 ? 0 : span / s + 1;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_fid_preprocess(const void *src, int dtype, int64_t ld, int N, int H, int W, int R_h, int R_w,
                                      int flags, float *out, omnitok_stream_t stream_) {
    OT_CHECK_ARG(dtype == OMNITOK_FID_U8_NHWC || dtype == OMNITOK_FID_F32_NCHW, "fid_preprocess: dtype %d", dtype);
    OT_CHECK_ARG((flags & ~(OMNITOK_FID_RESIZE | OMNITOK_FID_NORMALIZE)) == 0, "fid_preprocess: flags %d", flags);
    OT_CHECK_ARG(N >= 0 && N <= 65535 && H >= 1 && W >= 1 && R_h >= 1 && R_w >= 1 && (int64_t)H * W <= (1ll << 28) &&
                     (int64_t)R_h * R_w <= (1ll << 28),
                 "fid_preprocess: bad sizes N %d H %d W %d -> %d x %d", N, H, W, R_h, R_w);
    const bool resize = flags & OMNITOK_FID_RESIZE;
    OT_CHECK_ARG(resize || (R_h == H && R_w == W), "fid_preprocess: without resize the output is the input's %d x %d, not "
                 "%d x %d", H, W, R_h, R_w);
    if (dtype == OMNITOK_FID_U8_NHWC)
        OT_CHECK_ARG(ld >= 3ll * W && ld <= (1ll << 30), "fid_preprocess: row stride %lld below 3 W = %d", (long long)ld,
                     3 * W);
    if (N == 0) return OMNITOK_OK;
    OT_CHECK_ARG(src && out, "fid_preprocess: null pointer");
    OT_CHECK_ARG(aligned16(out), "fid_preprocess: out must be 16-byte aligned");
    const float sh = (float)H / (float)R_h, sw = (float)W / (float)R_w;  // torch's area_pixel_compute_scale
    const dim3 grid((unsigned)(((int64_t)R_h * R_w + 255) / 256), (unsigned)N);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int nz = (flags & OMNITOK_FID_NORMALIZE) ? 1 : 0;
    if (dtype == OMNITOK_FID_U8_NHWC)
        hipLaunchKernelGGL(fid_preprocess_kernel<true>, grid, dim3(256), 0, stream, src, ld, H, W, R_h, R_w, sh, sw,
                           (int)resize, nz, out);
    else
        hipLaunchKernelGGL(fid_preprocess_kernel<false>, grid, dim3(256), 0, stream, src, ld, H, W, R_h, R_w, sh, sw,
                           (int)resize, nz, out);
    OT_LAUNCH_CHECK("fid_preprocess");
    return OMNITOK_OK;
}

extern "C" int omnitok_conv2d_out(int s, int k, int stride, int pad) {
    if (s < 1 || k < 1 || stride < 1 || pad < 0) return 0;
    return pool_out(s, k, stride, pad);
}

extern "C" int omnitok_conv2d(const omnitok_conv2d_desc *c, omnitok_stream_t stream_) {
    OT_CHECK_ARG(c, "conv2d: null descriptor");
    OT_CHECK_ARG(c->N >= 0 && c->H >= 1 && c->W >= 1 && c->Cout >= 1 && c->Cout <= 65536,
                 "conv2d: bad sizes N %d H %d W %d Cout %d", c->N, c->H, c->W, c->Cout);
    const int64_t ldw = omnitok_conv3d_packed_ldw(c->Cin, 1, c->kh, c->kw);
    OT_CHECK_ARG(ldw > 0, "conv2d: Cin %d must be a positive multiple of 4 and the kernel %d x %d within 1..7", c->Cin, c->kh,
                 c->kw);
    OT_CHECK_ARG(c->sh >= 1 && c->sh <= 4 && c->sw >= 1 && c->sw <= 4, "conv2d: strides %d x %d outside 1..4", c->sh, c->sw);
    OT_CHECK_ARG(c->ph >= 0 && c->ph < c->kh && c->pw >= 0 && c->pw < c->kw, "conv2d: padding %d x %d outside 0..kernel - 1",
                 c->ph, c->pw);
    OT_CHECK_ARG(c->relu == 0 || c->relu == 1, "conv2d: relu %d", c->relu);
    const int Ho = pool_out(c->H, c->kh, c->sh, c->ph), Wo = pool_out(c->W, c->kw, c->sw, c->pw);
    OT_CHECK_ARG(Ho >= 1 && Wo >= 1, "conv2d: empty output (%d x %d input, kernel %d x %d, padding %d x %d)", c->H, c->W,
                 c->kh, c->kw, c->ph, c->pw);
    CvArgs a{};
    a.T = 1;
    a.H = c->H;
    a.W = c->W;
    a.ldw = ldw;
    a.kt = 1;
    a.kh = c->kh;
    a.kw = c->kw;
    a.st = 1;
    a.sh = c->sh;
    a.sw = c->sw;
    a.pt = 0;
    a.ph = c->ph;
    a.pw = c->pw;
    a.To = 1;
    a.Ho = Ho;
    a.Wo = Wo;
    if (int rc = conv_args(c, "conv2d", c->N, a)) return rc;
    if (c->N == 0) return OMNITOK_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // the tile by the layer's shape alone (Cout and the per-image output extent; an image's results never depend on it):
    // 256 x 32 for Cout <= 32; 64 x 64 on maps of at most 17 x 17 (Mixed_6*, Mixed_7*: few rows per image, so larger tiles
    // leave CUs idle); else conv3d_same's rule
    if (c->Cout <= 32) return conv_launch<2, 1, 1>(a, (a.M + 255) / 256, stream, "conv2d");
    if ((int64_t)Ho * Wo <= 17 * 17) return conv_launch<1, 1, 2>(a, (a.M + 63) / 64, stream, "conv2d");
    const int pad128 = (c->Cout + 127) / 128 * 128, pad64 = (c->Cout + 63) / 64 * 64;
    if (pad64 < pad128) return conv_launch<4, 1>(a, (a.M + 255) / 256, stream, "conv2d");
    return conv_launch<2, 2>(a, (a.M + 127) / 128, stream, "conv2d");
}

static int pool2d(const char *what, bool is_max, const float *x, int N, int H, int W, int C, int k, int s, int p, float *y,
                  int64_t y_cs, int y_off, hipStream_t stream) {
    OT_CHECK_ARG(N >= 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "%s: bad sizes N %d H %d W %d C %d (C a positive "
                 "multiple of 4)", what, N, H, W, C);
    OT_CHECK_ARG(k >= 1 && k <= 7 && s >= 1 && s <= 4 && p >= 0 && 2 * p <= k, "%s: kernel %d / stride %d / padding %d "
                 "outside 1..7 / 1..4 / 0..kernel / 2", what, k, s, p);
    OT_CHECK_ARG(y_off >= 0 && y_off % 4 == 0 && y_cs % 4 == 0 && y_off + C <= y_cs, "%s: output channels [%d, %d) outside "
                 "the %lld per position, or not 16-byte groups", what, y_off, y_off + C, (long long)y_cs);
    Pool2dArgs a{};
    a.Ho = pool_out(H, k, s, p);
    a.Wo = pool_out(W, k, s, p);
    OT_CHECK_ARG(a.Ho >= 1 && a.Wo >= 1, "%s: empty output (%d x %d input, kernel %d)", what, H, W, k);
    if (N == 0) return OMNITOK_OK;
    OT_CHECK_ARG(x && y, "%s: null pointer", what);
    OT_CHECK_ARG(aligned16(x) && aligned16(y), "%s: x and y must be 16-byte aligned", what);
    a.x = x;
    a.y = y;
    a.y_cs = y_cs;
    a.y_off = y_off;
    a.H = H;
    a.W = W;
    a.C4 = C / 4;
    a.k = k;
    a.s = s;
    a.p = p;
    a.n = (int64_t)N * a.Ho * a.Wo * a.C4;
    OT_CHECK_ARG((int64_t)N * H * W * C < (1ll << 40) && (int64_t)N * a.Ho * a.Wo * y_cs < (1ll << 40) &&
                     (a.n + 255) / 256 <= 0x7fffffff,
                 "%s: too large", what);
    const dim3 grid((unsigned)((a.n + 255) / 256));
    if (is_max)
        hipLaunchKernelGGL(maxpool2d_kernel, grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(avgpool2d_kernel, grid, dim3(256), 0, stream, a);
    OT_LAUNCH_CHECK(what);
    return OMNITOK_OK;
}

extern "C" int omnitok_maxpool2d(const float *x, int N, int H, int W, int C, int k, int s, int p, float *y, int64_t y_cs,
                                 int y_off, omnitok_stream_t stream) {
    return pool2d("maxpool2d", true, x, N, H, W, C, k, s, p, y, y_cs, y_off, static_cast<hipStream_t>(stream));
}

extern "C" int omnitok_avgpool2d(const float *x, int N, int H, int W, int C, int k, int s, int p, float *y, int64_t y_cs,
                                 int y_off, omnitok_stream_t stream) {
    return pool2d("avgpool2d", false, x, N, H, W, C, k, s, p, y, y_cs, y_off, static_cast<hipStream_t>(stream));
}

extern "C" int omnitok_spatial_mean(const float *x, int N, int H, int W, int C, float *y, omnitok_stream_t stream_) {
    OT_CHECK_ARG(N >= 0 && N <= 65535 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && (int64_t)H * W <= (1 << 24),
                 "spatial_mean: bad sizes N %d H %d W %d C %d (C a positive multiple of 4)", N, H, W, C);
    if (N == 0) return OMNITOK_OK;
    OT_CHECK_ARG(x && y, "spatial_mean: null pointer");
    OT_CHECK_ARG(aligned16(x) && aligned16(y), "spatial_mean: x and y must be 16-byte aligned");
    OT_CHECK_ARG((int64_t)N * H * W * C < (1ll << 40), "spatial_mean: too large");
    const int C4 = C / 4;
    hipLaunchKernelGGL(spatial_mean_kernel, dim3((unsigned)((C4 + 255) / 256), (unsigned)N), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), x, H * W, C4, y);
    OT_LAUNCH_CHECK("spatial_mean");
    return OMNITOK_OK;
}
