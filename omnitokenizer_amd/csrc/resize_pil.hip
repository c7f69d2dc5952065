// Pillow-exact image resize on the device: Image.resize(size, BICUBIC | BILINEAR | BOX) of 8-bit RGB frames (Pillow's
// src/libImaging/Resample.c, whole-image box, reducing_gap=None), which is what torchvision's Resize does to a PIL image
// (the reference's ImageDataset, data.py:83-99) and what the DiT / Latte loaders' center_crop_arr is made of.  The 8-bit
// resampler is integer arithmetic on 22-bit fixed-point coefficients that come from a few double-precision + - * /, so
// the result is Pillow's, byte for byte.  No arithmetic is shared with frames.hip.
//
//   One axis (in -> out samples, filter support S: bicubic 2, bilinear 1, box 0.5), IEEE double, no contraction:
//     scale = in / out;  fs = max(scale, 1);  support = S * fs;  ksize = (int)ceil(support) * 2 + 1;  ss = 1 / fs
//     center = (xx + 0.5) * scale
//     xmin = max((int)(center - support + 0.5), 0);  n = min((int)(center + support + 0.5), in) - xmin
//     w[x] = filter((x + xmin - center + 0.5) * ss);  w[x] /= (w[0] + w[1] + ...) if that sum is not 0
//     k[x] = (int)(w[x] * 2^22 -+ 0.5)        (truncation; - for w < 0);  k[x] = 0 for n <= x < ksize
//   rp_coeff_row() is that text, once, for the host (omnitok_pil_resize_coeffs, the CPU tests) and the device (the
//   prologue kernel): fp64 + - * /, ceil and the double -> int32 conversion are correctly rounded / truncating on both.
//   One pass, per channel: out = clamp((2^21 + sum u8[xmin + x] * k[x]) >> 22, 0, 255), int32, arithmetic shift.
//
//   Three launches per group of RP_CLIPS clips (their descriptors travel in the kernel arguments: no copy, no
//   synchronisation, so a call can be captured in a graph), all state in the caller's workspace:
//     rp_coeffs_kernel      k[out][ksize] and bounds[out][2] of both axes of every clip
//     rp_horizontal_kernel  source rows -> uint8 intermediate; only the rows the vertical pass reads and the columns of the
//                           crop window.  One wave per row: the source row segment of a chunk of output pixels is staged
//                           in LDS as whole aligned dwords (as frames.hip does: the dword that holds a valid byte lies in
//                           the same aligned word of the allocation), 4 output pixels per lane, a run-time tap loop
//                           each, 12 bytes stored as 3 dwords.
//     rp_vertical_kernel    intermediate -> output.  One wave per output row, 4 pixels (3 dwords per tap row) per lane,
//                           the row's coefficients are wave-uniform.  Epilogue PIXELS: unit[u] - 0.5f (make_u8_unit(),
//                           the bits of ToTensor + Normalize(0.5, 1.0)) to planar fp32 by 16-byte stores; U8: the bytes.
//   A pass whose output size equals its input size copies (Pillow skips it).  The clamp of the horizontal pass is part of
//   the result: the intermediate is uint8.
//   Every index read from a table is clamped to the staged segment / the intermediate's rows before it is used.
#include "common.h"

#include <math.h>

namespace omnitok {

__constant__ U8Unit k_rp_unit = make_u8_unit();

constexpr int RP_CLIPS = 32;       // clips per launch
constexpr int RP_ROWS = 4;         // rows per 256-thread block, one per wave
constexpr int RP_CHUNK = 256;      // output pixels per wave pass (4 per lane)
constexpr int RP_SPAN_PX = 3411;   // most source pixels of one staged row segment ...
constexpr int RP_SPAN_MAX = 2600;  // ... and its dwords (3 bytes a pixel + alignment): 41.6 KB of LDS per block at most
constexpr int RP_BITS = 22;        // Pillow's PRECISION_BITS

struct RpClip {
    const uint8_t *src;
    int64_t fstride, rstride;
    int64_t off;   // of this clip's tables and intermediate in the workspace (rp_layout)
    int H, W, f0, fstep, top, left, rh, rw;
    int ksw, ksh;  // taps per table row; 0: the pass is skipped (a copy)
    int chunk;     // output pixels per horizontal wave pass
    int row0, nrows;  // source rows the vertical pass reads
};
struct RpArgs {
    RpClip c[RP_CLIPS];
    uint8_t *work;
    void *out;
    int F_out, R_h, R_w, clip0, filter, span;
};

// where a clip's parts lie from work + c.off: kh[rw][ksw], bh[rw][2], kv[rh][ksh], bv[rh][2] (int32), then the
// intermediate [F_out][rows][pitch] bytes, 16-byte aligned
struct RpLayout {
    int64_t kh, bh, kv, bv, mid, end;
};
__host__ __device__ inline int rp_pitch(int w) { return 12 * ((w + 3) / 4); }  // whole 4-pixel lane groups
__host__ __device__ inline RpLayout rp_layout(int H, int rh, int rw, int ksw, int ksh, int F_out) {
    RpLayout l;
    l.kh = 0;
    l.bh = l.kh + 4 * (int64_t)rw * ksw;
    l.kv = l.bh + (ksw ? 8 * (int64_t)rw : 0);
    l.bv = l.kv + 4 * (int64_t)rh * ksh;
    l.mid = (l.bv + (ksh ? 8 * (int64_t)rh : 0) + 15) & ~(int64_t)15;
    l.end = (l.mid + (int64_t)F_out * H * rp_pitch(rw) + 15) & ~(int64_t)15;
    return l;
}

// A product that is rounded before it feeds an addition or a subtraction: the device back end may contract a * b +- c
// whatever the pragma says (common.h no_fuse), so such a product passes through an empty asm there.  The host pass honours
// the pragma.  These are the products inside the filter polynomials, `center` (it feeds center -+ support and x - center)
// and the filter's argument (it feeds 1 - x in the bilinear filter).  w * 2^22 needs none: scaling by a power of two is
// exact, so a fused and an unfused + 0.5 round the same number.
__host__ __device__ inline double rp_rnd(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#endif
    return x;
}

__host__ __device__ inline double rp_filter(int f, double x) {
#pragma clang fp contract(off)
    if (f == OMNITOK_RESIZE_BICUBIC) {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) {  // ((a + 2) * x - (a + 3)) * x * x + 1
            double t = rp_rnd((a + 2.0) * x) - (a + 3.0);
            t = t * x;
            return rp_rnd(t * x) + 1.0;
        }
        if (x < 2.0) {  // (((x - 5) * x + 8) * x - 4) * a
            double t = rp_rnd((x - 5.0) * x) + 8.0;
            t = rp_rnd(t * x) - 4.0;
            return t * a;
        }
        return 0.0;
    }
    if (f == OMNITOK_RESIZE_BILINEAR) {
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    }
    return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
}

struct RpAxis {
    double scale, support, ss;
    int ksize;
};
__host__ __device__ inline RpAxis rp_axis(int in, int out, int f) {
#pragma clang fp contract(off)
    RpAxis a;
    a.scale = (double)in / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = (f == OMNITOK_RESIZE_BICUBIC ? 2.0 : f == OMNITOK_RESIZE_BILINEAR ? 1.0 : 0.5) * fs;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    a.ss = 1.0 / fs;
    return a;
}
// first tap and number of taps of output sample xx
__host__ __device__ inline void rp_bounds(const RpAxis &a, int in, int xx, int &xmin, int &n) {
#pragma clang fp contract(off)
    const double center = rp_rnd(((double)xx + 0.5) * a.scale);
    xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > in) xmax = in;
    n = xmax - xmin;
}
// k[ksize] and bounds[2] of output sample xx.  The weights are evaluated twice (the sum, then the quotients) instead of
// being kept: the same operations on the same operands give the same doubles.
__host__ __device__ inline void rp_coeff_row(const RpAxis &a, int in, int f, int xx, int32_t *k, int32_t *bounds) {
#pragma clang fp contract(off)
    int xmin, n;
    rp_bounds(a, in, xx, xmin, n);
    const double center = rp_rnd(((double)xx + 0.5) * a.scale);
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww = ww + rp_filter(f, rp_rnd(((double)(x + xmin) - center + 0.5) * a.ss));
    int x = 0;
    for (; x < n; ++x) {
        double w = rp_filter(f, rp_rnd(((double)(x + xmin) - center + 0.5) * a.ss));
        if (ww != 0.0) w = w / ww;
        k[x] = w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
    }
    for (; x < a.ksize; ++x) k[x] = 0;
    bounds[0] = xmin;
    bounds[1] = n;
}

// grid (ceil(longest axis of the group / 256), 2, clips): blockIdx.y 0 = the horizontal table, 1 = the vertical one
__global__ __launch_bounds__(256) void rp_coeffs_kernel(const RpArgs a) {
    const RpClip &c = a.c[blockIdx.z];
    const bool vert = blockIdx.y != 0;
    const int in = vert ? c.H : c.W, out = vert ? c.rh : c.rw, ks = vert ? c.ksh : c.ksw;
    const int xx = blockIdx.x * 256 + threadIdx.x;
    if (ks == 0 || xx >= out) return;
    const RpLayout l = rp_layout(c.H, c.rh, c.rw, c.ksw, c.ksh, a.F_out);
    uint8_t *base = a.work + c.off;
    int32_t *k = reinterpret_cast<int32_t *>(base + (vert ? l.kv : l.kh)) + (int64_t)xx * ks;
    int32_t *b = reinterpret_cast<int32_t *>(base + (vert ? l.bv : l.bh)) + 2 * xx;
    rp_coeff_row(rp_axis(in, out, a.filter), in, a.filter, xx, k, b);
}

__device__ __forceinline__ unsigned rp_clip8(int acc) {
    const int v = acc >> RP_BITS;  // arithmetic shift
    return (unsigned)min(max(v, 0), 255);
}

// one wave per intermediate row; grid (ceil(most rows of the group / RP_ROWS), F_out, clips), a.span dwords of LDS a wave
__global__ __launch_bounds__(256) void rp_horizontal_kernel(const RpArgs a) {
    extern __shared__ unsigned rp_span[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int z = blockIdx.z, t = blockIdx.y;
    const RpClip &c = a.c[z];
    if ((int)blockIdx.x * RP_ROWS >= c.nrows) return;  // block-uniform
    const int r = blockIdx.x * RP_ROWS + wave;
    const bool row_ok = r < c.nrows;
    const bool skip = c.ksw == 0;
    const RpLayout l = rp_layout(c.H, c.rh, c.rw, c.ksw, c.ksh, a.F_out);
    uint8_t *base = a.work + c.off;
    const int32_t *kh = reinterpret_cast<const int32_t *>(base + l.kh);
    const int32_t *bh = reinterpret_cast<const int32_t *>(base + l.bh);
    const int pitch = rp_pitch(a.R_w);
    uint8_t *mrow = base + l.mid + ((int64_t)t * c.nrows + (row_ok ? r : 0)) * pitch;
    const uint8_t *srow = c.src + (int64_t)(c.f0 + t * c.fstep) * c.fstride + (int64_t)(c.row0 + (row_ok ? r : 0)) * c.rstride;
    unsigned *span = rp_span + wave * a.span;
    const int span_px = (4 * a.span - 6) / 3;  // pixels that fit behind any alignment shift
    for (int x0 = 0; x0 < a.R_w; x0 += c.chunk) {  // trip count uniform over the block
        const int n = min(c.chunk, a.R_w - x0);
        const int X0 = c.left + x0;  // in the resized frame
        int cs, ce;                  // source pixels [cs, ce) of this chunk
        if (skip) {
            cs = X0;
            ce = X0 + n;
        } else {
            cs = bh[2 * X0];
            ce = bh[2 * (X0 + n - 1)] + bh[2 * (X0 + n - 1) + 1];
        }
        cs = min(max(cs, 0), c.W - 1);
        ce = min(min(max(ce, cs + 1), c.W), cs + span_px);
        __syncthreads();  // the previous pass is done with span[]
        int shift = 0;
        if (row_ok) {
            const uintptr_t b = reinterpret_cast<uintptr_t>(srow + 3 * (int64_t)cs);
            const unsigned *d = reinterpret_cast<const unsigned *>(b & ~(uintptr_t)3);
            shift = (int)(b & 3);
            const int nd = min((shift + 3 * (ce - cs) + 3) >> 2, a.span);
            for (int i = lane; i < nd; i += 64) span[i] = d[i];
        }
        __syncthreads();
        const uint8_t *sb = reinterpret_cast<const uint8_t *>(span) + shift;
        const int px = 4 * lane;
        if (!row_ok || px >= n) continue;
        unsigned u[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u[j][0] = u[j][1] = u[j][2] = 0u;
            if (px + j >= n) continue;
            const int x = X0 + px + j;
            if (skip) {
                const uint8_t *p = sb + 3 * (x - cs);
                u[j][0] = p[0]; u[j][1] = p[1]; u[j][2] = p[2];
            } else {
                const int xmin = min(max(bh[2 * x], cs), ce - 1);
                const int cnt = min(min(bh[2 * x + 1], c.ksw), ce - xmin);
                const int32_t *kp = kh + (int64_t)x * c.ksw;
                const uint8_t *p = sb + 3 * (xmin - cs);
                int a0 = 1 << (RP_BITS - 1), a1 = a0, a2 = a0;
                for (int i = 0; i < cnt; ++i) {
                    const int kk = kp[i];
                    a0 += (int)p[3 * i] * kk;
                    a1 += (int)p[3 * i + 1] * kk;
                    a2 += (int)p[3 * i + 2] * kk;
                }
                u[j][0] = rp_clip8(a0); u[j][1] = rp_clip8(a1); u[j][2] = rp_clip8(a2);
            }
        }
        uint8_t *dst = mrow + 3 * (x0 + px);
        if (px + 4 <= n && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
            unsigned *dd = reinterpret_cast<unsigned *>(dst);  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            dd[0] = u[0][0] | u[0][1] << 8 | u[0][2] << 16 | u[1][0] << 24;
            dd[1] = u[1][1] | u[1][2] << 8 | u[2][0] << 16 | u[2][1] << 24;
            dd[2] = u[2][2] | u[3][0] << 8 | u[3][1] << 16 | u[3][2] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (px + j < n)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) dst[3 * j + ch] = (uint8_t)u[j][ch];
        }
    }
}

// one wave per output row; grid (ceil(R_h / RP_ROWS), F_out, clips)
template <int KIND>
__global__ __launch_bounds__(256) void rp_vertical_kernel(const RpArgs a) {
    __shared__ float unit[256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int z = blockIdx.z, t = blockIdx.y;
    const RpClip &c = a.c[z];
    if (KIND == OMNITOK_RESIZE_OUT_PIXELS) {
        unit[threadIdx.x] = k_rp_unit.v[threadIdx.x];
        __syncthreads();
    }
    const int y = __builtin_amdgcn_readfirstlane(blockIdx.x * RP_ROWS + wave);
    if (y >= a.R_h) return;
    const bool skip = c.ksh == 0;
    const RpLayout l = rp_layout(c.H, c.rh, c.rw, c.ksw, c.ksh, a.F_out);
    const uint8_t *base = a.work + c.off;
    const int Y = c.top + y;  // in the resized frame
    int r0 = Y - c.row0, cnt = 1;
    const int32_t *kp = nullptr;
    if (!skip) {
        const int32_t *bv = reinterpret_cast<const int32_t *>(base + l.bv);
        r0 = bv[2 * Y] - c.row0;
        cnt = bv[2 * Y + 1];
        kp = reinterpret_cast<const int32_t *>(base + l.kv) + (int64_t)Y * c.ksh;
    }
    r0 = min(max(r0, 0), c.nrows - 1);
    cnt = min(min(cnt, skip ? 1 : c.ksh), c.nrows - r0);
    const int pitch = rp_pitch(a.R_w);
    const uint8_t *m0 = base + l.mid + ((int64_t)t * c.nrows + r0) * pitch;
    const int64_t plane = (int64_t)a.F_out * a.R_h * a.R_w;
    for (int px = 4 * lane; px < a.R_w; px += RP_CHUNK) {
        const unsigned *p = reinterpret_cast<const unsigned *>(m0 + 3 * px);
        unsigned u[12];
        if (skip) {
            const unsigned w0 = p[0], w1 = p[1], w2 = p[2];
#pragma unroll
            for (int b = 0; b < 12; ++b) u[b] = ((b < 4 ? w0 : b < 8 ? w1 : w2) >> (8 * (b & 3))) & 0xFFu;
        } else {
            int acc[12];
#pragma unroll
            for (int b = 0; b < 12; ++b) acc[b] = 1 << (RP_BITS - 1);
            for (int i = 0; i < cnt; ++i) {
                const int kk = kp[i];
                const unsigned w0 = p[0], w1 = p[1], w2 = p[2];
                p += pitch >> 2;
#pragma unroll
                for (int b = 0; b < 12; ++b)
                    acc[b] += (int)(((b < 4 ? w0 : b < 8 ? w1 : w2) >> (8 * (b & 3))) & 0xFFu) * kk;
            }
#pragma unroll
            for (int b = 0; b < 12; ++b) u[b] = rp_clip8(acc[b]);
        }
        // u[3 * j + ch]: pixel px + j, channel ch
        if (KIND == OMNITOK_RESIZE_OUT_PIXELS) {
            float *dst = static_cast<float *>(a.out) + (int64_t)(a.clip0 + z) * 3 * plane + ((int64_t)t * a.R_h + y) * a.R_w + px;
            if (px + 4 <= a.R_w && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (plane & 3) == 0) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    *reinterpret_cast<f32x4 *>(dst + ch * plane) = f32x4{unit[u[ch]] - 0.5f, unit[u[3 + ch]] - 0.5f,
                                                                        unit[u[6 + ch]] - 0.5f, unit[u[9 + ch]] - 0.5f};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (px + j < a.R_w)
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) dst[ch * plane + j] = unit[u[3 * j + ch]] - 0.5f;
            }
        } else {
            uint8_t *dst = static_cast<uint8_t *>(a.out) +
                           ((((int64_t)(a.clip0 + z) * a.F_out + t) * a.R_h + y) * a.R_w + px) * 3;
            if (px + 4 <= a.R_w && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
                unsigned *dd = reinterpret_cast<unsigned *>(dst);
#pragma unroll
                for (int q = 0; q < 3; ++q) dd[q] = u[4 * q] | u[4 * q + 1] << 8 | u[4 * q + 2] << 16 | u[4 * q + 3] << 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (px + j < a.R_w)
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) dst[3 * j + ch] = (uint8_t)u[3 * j + ch];
            }
        }
    }
}

static const char *const RP_FILTER_NAMES[] = {"bicubic", "bilinear", "box"};

// the checks of one clip that need no output size (shared by the workspace function), and its tap counts
static int rp_check_clip(const char *fn, const omnitok_frames_desc &d, int i, int F_out, int filter, int &ksw, int &ksh) {
    OT_CHECK_ARG(d.frames, "%s: clip %d: null frames pointer", fn, i);
    OT_CHECK_ARG(d.F >= 1 && d.H >= 1 && d.W >= 1, "%s: clip %d: bad size %dx%dx%d", fn, i, d.F, d.H, d.W);
    OT_CHECK_ARG(d.row_stride >= 3 * (int64_t)d.W && (d.F == 1 || d.frame_stride >= d.row_stride * (d.H - 1) + 3 * (int64_t)d.W),
                 "%s: clip %d: strides (%lld, %lld) bytes do not fit %dx%d x 3 frames", fn, i, (long long)d.frame_stride,
                 (long long)d.row_stride, d.H, d.W);
    OT_CHECK_ARG(d.frame_start >= 0 && d.frame_step >= 1 && d.frame_start + (int64_t)(F_out - 1) * d.frame_step < d.F,
                 "%s: clip %d: frames %d + k * %d for k < %d run past F = %d", fn, i, d.frame_start, d.frame_step, F_out, d.F);
    OT_CHECK_ARG(d.resize_h >= 1 && d.resize_w >= 1, "%s: clip %d: resize to %dx%d (sizes must be >= 1)", fn, i, d.resize_h,
                 d.resize_w);
    ksw = d.W == d.resize_w ? 0 : rp_axis(d.W, d.resize_w, filter).ksize;
    ksh = d.H == d.resize_h ? 0 : rp_axis(d.H, d.resize_h, filter).ksize;
    OT_CHECK_ARG(ksw <= OMNITOK_RESIZE_MAX_TAPS && ksh <= OMNITOK_RESIZE_MAX_TAPS,
                 "%s: clip %d: %dx%d -> %dx%d %s needs %d taps per sample, more than the cap of %d", fn, i, d.H, d.W,
                 d.resize_h, d.resize_w, RP_FILTER_NAMES[filter], ksw > ksh ? ksw : ksh, OMNITOK_RESIZE_MAX_TAPS);
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_pil_resize_coeffs(int in_size, int out_size, int filter, int *ksize, int32_t *k, int32_t *bounds) {
    OT_CHECK_ARG(filter >= OMNITOK_RESIZE_BICUBIC && filter <= OMNITOK_RESIZE_BOX, "pil_resize_coeffs: filter %d", filter);
    OT_CHECK_ARG(in_size >= 1 && out_size >= 1, "pil_resize_coeffs: bad sizes %d -> %d", in_size, out_size);
    OT_CHECK_ARG(ksize, "pil_resize_coeffs: null ksize pointer");
    const RpAxis a = rp_axis(in_size, out_size, filter);
    *ksize = a.ksize;
    if (!k) return OMNITOK_OK;
    OT_CHECK_ARG(bounds, "pil_resize_coeffs: null bounds pointer");
    for (int xx = 0; xx < out_size; ++xx) rp_coeff_row(a, in_size, filter, xx, k + (int64_t)xx * a.ksize, bounds + 2 * xx);
    return OMNITOK_OK;
}

extern "C" int64_t omnitok_frames_resize_pil_workspace(const omnitok_frames_desc *desc, int B, int F_out, int filter) {
    const char *fn = "frames_resize_pil_workspace";
    OT_CHECK_ARG(filter >= OMNITOK_RESIZE_BICUBIC && filter <= OMNITOK_RESIZE_BOX, "%s: filter %d", fn, filter);
    OT_CHECK_ARG(B >= 0 && F_out >= 1 && F_out <= 65535, "%s: bad sizes B %d F_out %d", fn, B, F_out);
    if (B == 0) return 0;
    OT_CHECK_ARG(desc, "%s: null pointer (desc)", fn);
    int64_t total = 0;
    for (int i = 0; i < B; ++i) {
        int ksw, ksh;
        if (int rc = rp_check_clip(fn, desc[i], i, F_out, filter, ksw, ksh)) return rc;
        total += rp_layout(desc[i].H, desc[i].resize_h, desc[i].resize_w, ksw, ksh, F_out).end;
    }
    return total;
}

extern "C" int omnitok_frames_resize_pil(const omnitok_frames_desc *desc, int B, int F_out, int R_h, int R_w, int filter,
                                         int out_kind, void *work, int64_t work_bytes, void *out, omnitok_stream_t stream_) {
    const char *fn = "frames_resize_pil";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(filter >= OMNITOK_RESIZE_BICUBIC && filter <= OMNITOK_RESIZE_BOX, "%s: filter %d", fn, filter);
    OT_CHECK_ARG(out_kind == OMNITOK_RESIZE_OUT_PIXELS || out_kind == OMNITOK_RESIZE_OUT_U8, "%s: out kind %d", fn, out_kind);
    OT_CHECK_ARG(B >= 0 && F_out >= 1 && F_out <= 65535 && R_h >= 1 && R_w >= 1, "%s: bad sizes B %d F_out %d R_h %d R_w %d",
                 fn, B, F_out, R_h, R_w);
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG(desc && work && out, "%s: null pointer (desc %p, work %p, out %p)", fn, (const void *)desc, work, out);
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 15) == 0, "%s: work %p is not 16-byte aligned", fn, work);
    int64_t need = 0;
    for (int i = 0; i < B; ++i) {
        const omnitok_frames_desc &d = desc[i];
        int ksw, ksh;
        if (int rc = rp_check_clip(fn, d, i, F_out, filter, ksw, ksh)) return rc;
        OT_CHECK_ARG(d.crop_top >= 0 && d.crop_left >= 0 && d.crop_top + (int64_t)R_h <= d.resize_h &&
                         d.crop_left + (int64_t)R_w <= d.resize_w,
                     "%s: clip %d: crop window %dx%d at (%d, %d) outside the %dx%d resized frame", fn, i, R_h, R_w, d.crop_top,
                     d.crop_left, d.resize_h, d.resize_w);
        need += rp_layout(d.H, d.resize_h, d.resize_w, ksw, ksh, F_out).end;
    }
    OT_CHECK_ARG(work_bytes >= need, "%s: workspace of %lld bytes is too small, %lld needed (omnitok_frames_resize_pil_workspace)",
                 fn, (long long)work_bytes, (long long)need);
    int64_t off = 0;
    for (int c0 = 0; c0 < B; c0 += RP_CLIPS) {
        const int n = B - c0 < RP_CLIPS ? B - c0 : RP_CLIPS;
        RpArgs a{};
        int max_axis = 0, max_rows = 0, span = 0;
        for (int i = 0; i < n; ++i) {
            const omnitok_frames_desc &d = desc[c0 + i];
            RpClip &c = a.c[i];
            c.src = d.frames;
            c.fstride = d.frame_stride;
            c.rstride = d.row_stride;
            c.H = d.H; c.W = d.W;
            c.f0 = d.frame_start; c.fstep = d.frame_step;
            c.top = d.crop_top; c.left = d.crop_left;
            c.rh = d.resize_h; c.rw = d.resize_w;
            int px;  // source pixels one horizontal wave pass stages
            if (d.W == d.resize_w) {
                c.ksw = 0;
                c.chunk = RP_CHUNK;
                px = RP_CHUNK;
            } else {
                // a chunk of m output pixels reads at most scale * (m - 1) + 2 * support + 1 source pixels (rp_bounds)
                const RpAxis ax = rp_axis(d.W, d.resize_w, filter);
                c.ksw = ax.ksize;
                const double fixed = 2.0 * ax.support + 2.0;
                int m = (int)(((double)RP_SPAN_PX - fixed) / ax.scale) + 1;
                m = m > RP_CHUNK ? RP_CHUNK : m;
                if (m >= 4) m &= ~3;
                c.chunk = m < 1 ? 1 : m;
                px = (int)ceil(ax.scale * (c.chunk - 1) + fixed);
                px = px > RP_SPAN_PX ? RP_SPAN_PX : px;
            }
            px = px > d.W ? d.W : px;
            const int dwords = (3 * px + 6 + 3) / 4;
            span = dwords > span ? dwords : span;
            if (d.H == d.resize_h) {
                c.ksh = 0;
                c.row0 = d.crop_top;
                c.nrows = R_h;
            } else {
                const RpAxis ay = rp_axis(d.H, d.resize_h, filter);
                c.ksh = ay.ksize;
                int y0, n0, y1, n1;
                rp_bounds(ay, d.H, d.crop_top, y0, n0);
                rp_bounds(ay, d.H, d.crop_top + R_h - 1, y1, n1);
                c.row0 = y0;
                c.nrows = y1 + n1 - y0;
                if (c.nrows < 1) c.nrows = 1;
            }
            c.off = off;
            off += rp_layout(d.H, d.resize_h, d.resize_w, c.ksw, c.ksh, F_out).end;
            if (c.ksw && d.resize_w > max_axis) max_axis = d.resize_w;
            if (c.ksh && d.resize_h > max_axis) max_axis = d.resize_h;
            max_rows = c.nrows > max_rows ? c.nrows : max_rows;
        }
        a.work = static_cast<uint8_t *>(work);
        a.out = out;
        a.F_out = F_out; a.R_h = R_h; a.R_w = R_w; a.clip0 = c0; a.filter = filter;
        a.span = span > RP_SPAN_MAX ? RP_SPAN_MAX : span;
        if (max_axis > 0) {
            hipLaunchKernelGGL(rp_coeffs_kernel, dim3((unsigned)((max_axis + 255) / 256), 2u, (unsigned)n), dim3(256), 0, stream, a);
            OT_LAUNCH_CHECK("rp_coeffs");
        }
        hipLaunchKernelGGL(rp_horizontal_kernel, dim3((unsigned)((max_rows + RP_ROWS - 1) / RP_ROWS), (unsigned)F_out, (unsigned)n),
                           dim3(256), (size_t)a.span * RP_ROWS * sizeof(unsigned), stream, a);
        OT_LAUNCH_CHECK("rp_horizontal");
        const dim3 grid((unsigned)((R_h + RP_ROWS - 1) / RP_ROWS), (unsigned)F_out, (unsigned)n);
        if (out_kind == OMNITOK_RESIZE_OUT_PIXELS)
            hipLaunchKernelGGL(rp_vertical_kernel<OMNITOK_RESIZE_OUT_PIXELS>, grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL(rp_vertical_kernel<OMNITOK_RESIZE_OUT_U8>, grid, dim3(256), 0, stream, a);
        OT_LAUNCH_CHECK("rp_vertical");
    }
    return OMNITOK_OK;
}
