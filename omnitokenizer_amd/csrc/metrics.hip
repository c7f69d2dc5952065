// Reconstruction metrics: PSNR and SSIM of every (clip, frame) of two videos in [0, 1], with the arithmetic of the
// reference's evaluation/common_metrics_on_video_quality: calculate_psnr.py img_psnr and calculate_ssim.py ssim /
// calculate_ssim_function.  The operands are read in place through strides (include/omnitok.h omnitok_metrics_operand).
//
//   frame_metrics_kernel<SSIM>  one 256-thread block per (column tile, row strip) of one (clip, frame, channel) plane.
//     A tile is 256 input columns (one per thread) and the 246 SSIM output columns they cover; a strip is 32 SSIM output
//     rows.  The partition depends on H and W alone (mt_strips / mt_tiles).
//     PSNR  every input element is read once per block; the block's own rows and columns (strips and tiles split the plane
//           without overlap) add rnd32(rnd32(a - b)^2) to an fp64 sum, in row order per thread.
//     SSIM  fp64 throughout (fp32 and u8 / 255 widen exactly).  The window of cv2.getGaussianKernel(11, 1.5) (host, in
//           fp64, cv2's formula) is applied separably, only over the valid (H - 10) x (W - 10) region:
//           vertical   each thread keeps the 14 input rows (a, b) of 4 output rows of its column in registers and forms the
//                      5 maps a, b, a^2, b^2, ab with 11 taps each (fma, taps in order);
//           horizontal the 4 x 5 vertical rows go through LDS (42 KiB, bank-conflict free: mt_swz);
//                      wave q takes output row q, lane l its 4 output columns 4l .. 4l + 3 from the 14 staged columns
//                      4l .. 4l + 13 of each map (11 taps in order);
//           then the reference's map ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), each
//           operation rounded on its own, summed in fp64 per thread.
//     The two sums of a block are reduced in a fixed order (a shuffle tree per wave, then the waves in order) into the
//     workspace.
//   frame_metrics_finalize_kernel  one thread per (clip, frame): the partial sums in a fixed order (channel, then strip
//     and tile), per-channel SSIM = sum / ((H - 10)(W - 10)), frame SSIM = ((s0 + s1) + s2) / 3 (the reference's mean
//     of three), mse = sum / (3 H W), PSNR = 100 if mse < 1e-10 else 20 log10(1 / sqrt(mse)), in fp64.
// A clip's scores therefore never depend on B, F or the other clips of the batch.
#include "common.h"

#include <math.h>

namespace omnitok {

__constant__ U8Unit k_metrics_unit = make_u8_unit();

constexpr int MT_THREADS = 256;
constexpr int MT_TILE = MT_THREADS - 10;  // SSIM output columns per tile: the 256 input columns of the tile, one per thread
constexpr int MT_STRIP = 32;              // SSIM output rows per strip
constexpr int MT_RB = 4;                  // output rows per step, one per wave in the horizontal pass
constexpr int MT_WIN = MT_RB + 10;        // input rows a step reads
constexpr int MT_LD = 264;                // doubles per staged row and map: 256 + what lane 61's reads (4 * 61 + 13) pass

static_assert(MT_RB == MT_THREADS / 64, "one output row per wave in the horizontal pass");

struct MtOp {
    const void *p;
    int64_t s[5];
    int u8, clamp;
    float shift;
};
struct MtArgs {
    MtOp a, b;
    double g[11];
    double *part;  // [B][F][3][nparts] x {SSIM map sum, d^2 sum}
    int H, W, ntiles, nparts;
};

static int mt_strips(int H) { return H <= 10 ? 1 : (H - 10 + MT_STRIP - 1) / MT_STRIP; }
static int mt_tiles(int W) { return W <= 10 ? 1 : (W - 10 + MT_TILE - 1) / MT_TILE; }

// LDS column of staged column c: consecutive columns (the ds_write_b64 of the vertical pass) and column 4l + k of lanes
// l = 0..31 / 32..63 (the ds_read_b64 of the horizontal pass, any k) fall on distinct banks
__device__ __forceinline__ int mt_swz(int c) { return c ^ ((c >> 5) & 3); }

__device__ __forceinline__ uint32_t mt_raw(const MtOp &o, int64_t off) {
    return o.u8 ? (uint32_t) static_cast<const uint8_t *>(o.p)[off]
                : __float_as_uint(static_cast<const float *>(o.p)[off]);
}

// the operand's value in [0, 1]: u / 255 (table), or x + shift then torch.clamp(., 0, 1) in fp32 (NaN stays NaN)
__device__ __forceinline__ float mt_value(const MtOp &o, uint32_t raw, const float *unit) {
#pragma clang fp contract(off)
    if (o.u8) return unit[raw];
    float v = __uint_as_float(raw) + o.shift;
    if (o.clamp) v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    return v;
}

// calculate_ssim.py ssim(): one map value from the 5 filtered maps (mu1, mu2, E[a^2], E[b^2], E[ab]), no contraction
__device__ __forceinline__ double mt_ssim(const double (&h)[5]) {
#pragma clang fp contract(off)
    constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double mu1_sq = h[0] * h[0], mu2_sq = h[1] * h[1], mu1_mu2 = h[0] * h[1];
    const double s1 = h[2] - mu1_sq, s2 = h[3] - mu2_sq, s12 = h[4] - mu1_mu2;
    return ((2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
}

// grid (nstrips * ntiles, 3 * F, B)
template <bool SSIM>
__global__ __launch_bounds__(MT_THREADS) void frame_metrics_kernel(const MtArgs a) {
#pragma clang fp contract(off)
    __shared__ float unit[256];
    __shared__ double rows[SSIM ? MT_RB : 1][5][SSIM ? MT_LD : 1];
    __shared__ double red[2][MT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strip = blockIdx.x / a.ntiles, tile = blockIdx.x - strip * a.ntiles;
    const int ch = blockIdx.y % 3, t = blockIdx.y / 3, b = blockIdx.z;
    const int H = a.H, W = a.W;
    const int r0 = strip * MT_STRIP, c0 = tile * MT_TILE, col = c0 + tid;
    const int nstrips = gridDim.x / a.ntiles;
    const int psnr_r1 = strip == nstrips - 1 ? H : r0 + MT_STRIP;              // PSNR rows [r0, psnr_r1) of the strip
    const bool in_col = col < W;
    const bool psnr_col = in_col && (tile == a.ntiles - 1 || tid < MT_TILE);  // PSNR columns [c0, c0 + 246) of the tile
    unit[tid] = k_metrics_unit.v[tid];
    const int64_t ccol = in_col ? col : 0;
    const int64_t pa = (int64_t)b * a.a.s[0] + (int64_t)t * a.a.s[1] + (int64_t)ch * a.a.s[2] + ccol * a.a.s[4];
    const int64_t pb = (int64_t)b * a.b.s[0] + (int64_t)t * a.b.s[1] + (int64_t)ch * a.b.s[2] + ccol * a.b.s[4];
    double d2 = 0.0, ssum = 0.0;
    // raw elements of input row r of this thread's column (0 outside the plane: those feed no kept output)
    auto fetch = [&](int r, uint32_t &ua, uint32_t &ub) {
        ua = ub = 0u;
        if (in_col && r < H) {
            ua = mt_raw(a.a, pa + (int64_t)r * a.a.s[3]);
            ub = mt_raw(a.b, pb + (int64_t)r * a.b.s[3]);
        }
    };
    // their values; the PSNR sum of the block's own elements
    auto take = [&](int r, uint32_t ua, uint32_t ub, double &x, double &y) {
        const float fa = mt_value(a.a, ua, unit), fb = mt_value(a.b, ub, unit);
        if (psnr_col && r >= r0 && r < psnr_r1) {
            const float d = fa - fb;
            d2 += (double)no_fuse(d * d);
        }
        x = fa;
        y = fb;
    };
    if constexpr (SSIM) {
        if (tid < 8 * MT_RB * 5) rows[tid / 40][tid / 8 % 5][256 + tid % 8] = 0.0;  // read only for outputs that are not kept
    }
    __syncthreads();  // unit[]
    if constexpr (!SSIM) {
        for (int r = r0; r < psnr_r1; ++r) {
            uint32_t ua, ub;
            double x, y;
            fetch(r, ua, ub);
            take(r, ua, ub, x, y);
        }
    } else {
        const int out_r1 = min(r0 + MT_STRIP, H - 10);  // SSIM output rows [r0, out_r1) of the strip
        const int out_c = min(MT_TILE, W - 10 - c0);    // SSIM output columns [c0, c0 + out_c) of the tile
        const int nsteps = (out_r1 - r0 + MT_RB - 1) / MT_RB;
        double wa[MT_WIN], wb[MT_WIN];  // input rows r0 + 4n + j of step n
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            uint32_t ua, ub;
            fetch(r0 + j, ua, ub);
            take(r0 + j, ua, ub, wa[j], wb[j]);
        }
        uint32_t na[MT_RB], nb[MT_RB];
#pragma unroll
        for (int q = 0; q < MT_RB; ++q) fetch(r0 + 10 + q, na[q], nb[q]);
        for (int n = 0; n < nsteps; ++n) {  // trip count uniform over the block
            const int rb = r0 + 10 + MT_RB * n;
#pragma unroll
            for (int q = 0; q < MT_RB; ++q) take(rb + q, na[q], nb[q], wa[10 + q], wb[10 + q]);
            if (n + 1 < nsteps) {
#pragma unroll
                for (int q = 0; q < MT_RB; ++q) fetch(rb + MT_RB + q, na[q], nb[q]);
            }
            double acc[MT_RB][5];
#pragma unroll
            for (int o = 0; o < MT_RB; ++o)
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
#pragma unroll
            for (int j = 0; j < MT_WIN; ++j) {
                const double x = wa[j], y = wb[j], xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
                for (int o = 0; o < MT_RB; ++o) {
                    const int k = j - o;
                    if (k < 0 || k > 10) continue;
                    const double g = a.g[k];
                    acc[o][0] = __builtin_fma(g, x, acc[o][0]);
                    acc[o][1] = __builtin_fma(g, y, acc[o][1]);
                    acc[o][2] = __builtin_fma(g, xx, acc[o][2]);
                    acc[o][3] = __builtin_fma(g, yy, acc[o][3]);
                    acc[o][4] = __builtin_fma(g, xy, acc[o][4]);
                }
            }
            __syncthreads();  // the previous step's horizontal pass is done with rows[]
#pragma unroll
            for (int o = 0; o < MT_RB; ++o)
#pragma unroll
                for (int m = 0; m < 5; ++m) rows[o][m][mt_swz(tid)] = acc[o][m];
            __syncthreads();
            const int oc = 4 * lane;
            if (r0 + MT_RB * n + wave < out_r1 && oc < out_c) {
                double h[4][5];
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    double v[14];
#pragma unroll
                    for (int k = 0; k < 14; ++k) v[k] = rows[wave][m][mt_swz(oc + k)];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k < 11; ++k) s = __builtin_fma(a.g[k], v[j + k], s);
                        h[j][m] = s;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double m = mt_ssim(h[j]);
                    ssum += oc + j < out_c ? m : 0.0;
                }
            }
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                wa[j] = wa[j + MT_RB];
                wb[j] = wb[j + MT_RB];
            }
        }
    }
    // fixed-order block reduction
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ssum += __shfl_xor(ssum, off);
        d2 += __shfl_xor(d2, off);
    }
    if (lane == 0) {
        red[0][wave] = ssum;
        red[1][wave] = d2;
    }
    __syncthreads();
    if (tid == 0) {
        double *p = a.part + (((int64_t)b * gridDim.y + blockIdx.y) * a.nparts + blockIdx.x) * 2;
        p[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        p[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// one thread per (clip, frame) i = b * F + t
__global__ __launch_bounds__(256) void frame_metrics_finalize_kernel(const double *__restrict__ part, int64_t n_frames,
                                                                     int nparts, int H, int W, int flags,
                                                                     double *__restrict__ psnr, double *__restrict__ ssim) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_frames) return;
    const double *p = part + i * 3 * nparts * 2;
    double s[3], d2 = 0.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        s[ch] = 0.0;
        for (int k = 0; k < nparts; ++k) {
            s[ch] += p[(ch * nparts + k) * 2];
            d2 += p[(ch * nparts + k) * 2 + 1];
        }
    }
    if (flags & OMNITOK_METRICS_SSIM) {
        if (H < 11 || W < 11) {
            ssim[i] = __builtin_nan("");
        } else {
            const double n = (double)(H - 10) * (double)(W - 10);
            ssim[i] = ((s[0] / n + s[1] / n) + s[2] / n) / 3.0;
        }
    }
    if (flags & OMNITOK_METRICS_PSNR) {
        const double mse = d2 / (double)(3 * (int64_t)H * W);
        psnr[i] = mse < 1e-10 ? 100.0 : 20.0 * log10(1.0 / sqrt(mse));
    }
}

// cv2.getGaussianKernel(11, 1.5) in fp64, cv2's own formula: t_i = exp((-0.5 / sigma^2) x x), x = i - 5, times 1 / sum t
static void gaussian11(double g[11]) {
    const double sigma = 1.5, scale2x = -0.5 / (sigma * sigma);
    double sum = 0.0;
    for (int i = 0; i < 11; ++i) {
        const double x = i - 5.0;
        g[i] = exp(scale2x * x * x);
        sum += g[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < 11; ++i) g[i] *= sum;
}

static int check_operand(const omnitok_metrics_operand *o, const char *name) {
    OT_CHECK_ARG(o, "frame_metrics: null pointer (operand %s)", name);
    OT_CHECK_ARG(o->data, "frame_metrics: operand %s: null pointer (data)", name);
    OT_CHECK_ARG(o->dtype == OMNITOK_METRICS_F32 || o->dtype == OMNITOK_METRICS_U8, "frame_metrics: operand %s: element type %d",
                 name, o->dtype);
    OT_CHECK_ARG(o->stride[4] == 1 || o->stride[4] == 3, "frame_metrics: operand %s: w stride %lld, expected 1 or 3", name,
                 (long long)o->stride[4]);
    for (int k = 0; k < 4; ++k)
        OT_CHECK_ARG(o->stride[k] >= 0, "frame_metrics: operand %s: negative stride %lld (dim %d)", name,
                     (long long)o->stride[k], k);
    OT_CHECK_ARG(o->clamp == 0 || o->clamp == 1, "frame_metrics: operand %s: clamp %d, expected 0 or 1", name, o->clamp);
    OT_CHECK_ARG(__builtin_isfinite(o->shift), "frame_metrics: operand %s: shift is not finite", name);
    OT_CHECK_ARG(o->dtype == OMNITOK_METRICS_F32 || (o->shift == 0.0f && o->clamp == 0),
                 "frame_metrics: operand %s: a uint8 operand takes no shift or clamp", name);
    return OMNITOK_OK;
}

static MtOp mt_op(const omnitok_metrics_operand *o) {
    MtOp m{};
    m.p = o->data;
    for (int k = 0; k < 5; ++k) m.s[k] = o->stride[k];
    m.u8 = o->dtype == OMNITOK_METRICS_U8;
    m.clamp = o->clamp;
    m.shift = o->shift;
    return m;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int64_t omnitok_frame_metrics_workspace(int B, int F, int H, int W) {
    if (B < 0 || F < 1 || H < 1 || W < 1) return -1;
    return (int64_t)B * F * 3 * mt_strips(H) * mt_tiles(W) * 2 * (int64_t)sizeof(double);
}

extern "C" int omnitok_frame_metrics(const omnitok_metrics_operand *a, const omnitok_metrics_operand *b, int B, int F, int H,
                                     int W, int flags, double *psnr, double *ssim, void *work, size_t work_bytes,
                                     omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(flags != 0 && (flags & ~(OMNITOK_METRICS_PSNR | OMNITOK_METRICS_SSIM)) == 0, "frame_metrics: flags 0x%x",
                 flags);
    OT_CHECK_ARG(B >= 0 && B <= 65535 && F >= 1 && F <= 65535 / 3 && H >= 1 && W >= 1,
                 "frame_metrics: bad sizes B %d F %d H %d W %d", B, F, H, W);
    if (B == 0) return OMNITOK_OK;
    if (int rc = check_operand(a, "a")) return rc;
    if (int rc = check_operand(b, "b")) return rc;
    OT_CHECK_ARG(!(flags & OMNITOK_METRICS_PSNR) || psnr, "frame_metrics: null pointer (psnr output)");
    OT_CHECK_ARG(!(flags & OMNITOK_METRICS_SSIM) || ssim, "frame_metrics: null pointer (ssim output)");
    const int64_t need = omnitok_frame_metrics_workspace(B, F, H, W);
    OT_CHECK_ARG(work, "frame_metrics: null pointer (work, %lld bytes needed)", (long long)need);
    OT_CHECK_ARG(work_bytes >= (size_t)need, "frame_metrics: workspace of %zu bytes, %lld needed", work_bytes, (long long)need);
    MtArgs args{};
    args.a = mt_op(a);
    args.b = mt_op(b);
    gaussian11(args.g);
    args.part = static_cast<double *>(work);
    args.H = H;
    args.W = W;
    args.ntiles = mt_tiles(W);
    args.nparts = mt_strips(H) * args.ntiles;
    const dim3 grid((unsigned)args.nparts, (unsigned)(3 * F), (unsigned)B);
    if ((flags & OMNITOK_METRICS_SSIM) && H >= 11 && W >= 11)
        hipLaunchKernelGGL(frame_metrics_kernel<true>, grid, dim3(MT_THREADS), 0, stream, args);
    else
        hipLaunchKernelGGL(frame_metrics_kernel<false>, grid, dim3(MT_THREADS), 0, stream, args);
    OT_LAUNCH_CHECK("frame_metrics");
    const int64_t n_frames = (int64_t)B * F;
    hipLaunchKernelGGL(frame_metrics_finalize_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const double *>(work), n_frames, args.nparts, H, W, flags, psnr, ssim);
    OT_LAUNCH_CHECK("frame_metrics_finalize");
    return OMNITOK_OK;
}
