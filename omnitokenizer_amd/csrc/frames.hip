// Frames in, frames out: uint8 video frames <-> the fp32 pixels the encode / decode path reads and writes.
// Memory-bound streaming kernels; no arithmetic is shared with the tokenizer's own kernels.
//
//   frames_to_pixels  uint8 [F, H, W, 3] clips (one descriptor each: pointer, strides, frame range, crop; a ragged batch of
//                     different native sizes is one launch) -> fp32 [B, 3, F_out, R_h, R_w], the layout omnitok_encode reads.
//     NONE      p = unit[u] - 0.5f, unit[i] = float(i) / 255.0f folded by the compiler at build time (IEEE division, the
//               bits torch's CPU division gives; no division on the device).  Bit-identical to ToTensor + Normalize(0.5, 1)
//               and to the reference's VideoNorm (video_utils.py:33-58).  With OMNITOK_FRAMES_VIDEONORM a pre-pass flags the
//               clips with a cropped byte > 1; the others are not divided (p = float(u) - 0.5f), VideoNorm's rule.
//     BILINEAR  preprocess (data.py:305-350): F.interpolate(u / 255, (rh, rw), 'bilinear', align_corners=False), the crop,
//               then - 0.5.  The fp32 arithmetic (torch's CPU rule, with the contractions fixed as stated):
//                 scale  = float(in) / float(out)                              (host, correctly rounded)
//                 src    = max(fma(scale, float(dst) + 0.5f, -0.5f), 0)         (one fma)
//                 i0     = min(floor(src), in - 1), i1 = i0 + (i0 < in - 1), l1 = clamp(src - i0, 0, 1), l0 = 1 - l1
//                 in == out: i0 = i1 = dst, l0 = 1, l1 = 0 (torch's copy case: the result is then exact)
//                 row    = fma(v[i1], lx1, rnd(v[i0] * lx0))                      (width taps, left then right)
//                 p      = fma(bottom_row, ly1, rnd(top_row * ly0)) - 0.5f       (height taps, top then bottom)
//               where v = unit[u] and rnd() is a product rounded on its own (no_fuse).  torch's own result depends on the
//               kernel it dispatches to (separable or not, thread count); this one stays within 1e-6 of it.
//     Source bytes are staged in LDS as whole aligned dwords (one wave per output row, 4 output pixels per lane): each
//     source row segment is read by coalesced dword loads, the 3-byte pixels are picked from LDS, and each of the three
//     output planes is written by 16-byte stores.  The dword that holds a valid byte lies in the same aligned 4-byte word
//     of the allocation, so the up to 3 bytes read past either end of a segment never leave it.
//
//   pixels_to_frames  fp32 [B, 3, F, H, W] -> uint8, u = (uint8) trunc(min(max(x + 0.5f, 0), 1) * 255.0f), each step rounded
//                     in fp32 (vqgan_eval.py:141-148, utils.py:225-229), non-finite x -> 0.  THWC: every lane packs its 4
//                     pixels' 12 interleaved bytes into 3 dwords, which go through LDS so that each store instruction of a
//                     wave writes 256 contiguous bytes; CTHW: one dword per lane and channel.
#include "common.h"

namespace omnitok {

__constant__ U8Unit k_u8_unit = make_u8_unit();

constexpr int FR_CLIPS = 32;    // clips per launch: their descriptors travel in the kernel arguments
constexpr int FR_ROWS = 4;      // output rows per 256-thread block, one per wave
constexpr int FR_CHUNK = 256;   // output pixels per wave pass (4 per lane)
constexpr int FR_SPAN_NONE = 200;       // dwords of one staged source row segment: 3 * 256 bytes + alignment
constexpr int FR_SPAN_BILINEAR = 512;   // ... bilinear: the chunk is narrowed on the host so that its taps fit
constexpr int FR_MAX_DOWNSCALE = 200;   // bilinear: source / resized width above this is refused (a chunk of 4 must fit)

struct FrClip {
    const uint8_t *src;
    int64_t fstride, rstride;
    int F, H, W, f0, fstep, top, left, rh, rw, chunk;
    float sh, sw;
};
struct FrArgs {
    FrClip c[FR_CLIPS];
    float *out;
    unsigned *any_gt1;
    int F_out, R_h, R_w, clip0;
};

// torch's compute_source_index_and_lambda (align_corners=False), arithmetic as stated in the header
__device__ __forceinline__ void lin_src(float scale, int dst, int in, int out, int &i0, int &i1, float &l0, float &l1) {
#pragma clang fp contract(off)
    if (in == out) {
        i0 = i1 = dst;
        l0 = 1.0f;
        l1 = 0.0f;
        return;
    }
    float s = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
    s = s < 0.0f ? 0.0f : s;
    i0 = min((int)floorf(s), in - 1);
    l1 = fminf(fmaxf(s - (float)i0, 0.0f), 1.0f);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l0 = 1.0f - l1;
}

__device__ __forceinline__ float lerp_taps(float a, float b, float w0, float w1) {
#pragma clang fp contract(off)
    return __builtin_fmaf(b, w1, no_fuse(a * w0));
}

// one wave per output row; grid (ceil(R_h / FR_ROWS), F_out, clips of this launch)
template <int MODE, bool VN>
__global__ __launch_bounds__(256) void frames_to_pixels_kernel(const FrArgs a) {
#pragma clang fp contract(off)
    constexpr int SPAN = MODE == OMNITOK_FRAMES_BILINEAR ? FR_SPAN_BILINEAR : FR_SPAN_NONE;
    constexpr int NR = MODE == OMNITOK_FRAMES_BILINEAR ? 2 : 1;
    __shared__ float unit[256];
    __shared__ unsigned span[FR_ROWS][NR][SPAN];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int z = blockIdx.z, t = blockIdx.y;
    const FrClip &c = a.c[z];
    unit[tid] = k_u8_unit.v[tid];
    const int y = blockIdx.x * FR_ROWS + wave;
    const bool row_ok = y < a.R_h;
    const bool raw = VN && a.any_gt1[z] == 0u;  // VideoNorm: no byte > 1 in the clip -> not divided by 255
    const uint8_t *frame = c.src + (int64_t)(c.f0 + t * c.fstep) * c.fstride;
    int r[2];
    float wy0 = 1.0f, wy1 = 0.0f;
    if (MODE == OMNITOK_FRAMES_BILINEAR)
        lin_src(c.sh, c.top + y, c.H, c.rh, r[0], r[1], wy0, wy1);
    else
        r[0] = r[1] = c.top + y;
    const int64_t plane = (int64_t)a.F_out * a.R_h * a.R_w;
    float *o = a.out + (int64_t)(a.clip0 + z) * 3 * plane + ((int64_t)t * a.R_h + (row_ok ? y : 0)) * a.R_w;
    const int chunk = MODE == OMNITOK_FRAMES_BILINEAR ? c.chunk : FR_CHUNK;
    const uint8_t *sb[NR];
    for (int x0 = 0; x0 < a.R_w; x0 += chunk) {  // trip count uniform over the block
        const int n = min(chunk, a.R_w - x0);
        int cs, ce;
        if (MODE == OMNITOK_FRAMES_BILINEAR) {
            int j0, j1;
            float u0, u1;
            lin_src(c.sw, c.left + x0, c.W, c.rw, cs, j1, u0, u1);
            lin_src(c.sw, c.left + x0 + n - 1, c.W, c.rw, j0, ce, u0, u1);
        } else {
            cs = c.left + x0;
            ce = cs + n - 1;
        }
        __syncthreads();  // the previous pass is done with span[] (and unit[] is written)
        if (row_ok) {
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const uintptr_t b = reinterpret_cast<uintptr_t>(frame + (int64_t)r[k] * c.rstride + 3 * (int64_t)cs);
                const unsigned *d = reinterpret_cast<const unsigned *>(b & ~(uintptr_t)3);
                const int shift = (int)(b & 3);
                const int nd = min((shift + 3 * (ce - cs + 1) + 3) >> 2, SPAN);
                for (int i = lane; i < nd; i += 64) span[wave][k][i] = d[i];
                sb[k] = reinterpret_cast<const uint8_t *>(span[wave][k]) + shift;
            }
        }
        __syncthreads();
        const int px = 4 * lane;
        if (!row_ok || px >= n) continue;
        float v[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + px + j;
            if (MODE == OMNITOK_FRAMES_BILINEAR) {
                int i0 = cs, i1 = cs;  // lanes past the chunk's end read in-range taps and store nothing
                float wx0 = 1.0f, wx1 = 0.0f;
                if (px + j < n) lin_src(c.sw, c.left + x, c.W, c.rw, i0, i1, wx0, wx1);
                const int o0 = 3 * (i0 - cs), o1 = 3 * (i1 - cs);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float top = lerp_taps(unit[sb[0][o0 + ch]], unit[sb[0][o1 + ch]], wx0, wx1);
                    const float bot = lerp_taps(unit[sb[1][o0 + ch]], unit[sb[1][o1 + ch]], wx0, wx1);
                    v[ch][j] = lerp_taps(top, bot, wy0, wy1) - 0.5f;
                }
            } else {
                const int o0 = 3 * (px + j);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const unsigned u = sb[0][o0 + ch];
                    v[ch][j] = (raw ? (float)u : unit[u]) - 0.5f;
                }
            }
        }
        float *dst = o + x0 + px;
        if (px + 4 <= n && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                *reinterpret_cast<f32x4 *>(dst + ch * plane) = f32x4{v[ch][0], v[ch][1], v[ch][2], v[ch][3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (px + j < n)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) dst[ch * plane + j] = v[ch][j];
        }
    }
}

// VideoNorm pre-pass: any_gt1[clip] = 1 if a byte of the clip's cropped window (selected frames) exceeds 1.  Same grid as
// the mode-NONE kernel; any_gt1 is zeroed before it.  Only stores of 1 race, so no atomics are needed.
__global__ __launch_bounds__(256) void frames_any_gt1_kernel(const FrArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int z = blockIdx.z, t = blockIdx.y;
    const int y = blockIdx.x * FR_ROWS + wave;
    if (y >= a.R_h || *reinterpret_cast<volatile const unsigned *>(a.any_gt1 + z)) return;
    const FrClip &c = a.c[z];
    const uintptr_t b = reinterpret_cast<uintptr_t>(c.src + (int64_t)(c.f0 + t * c.fstep) * c.fstride +
                                                    (int64_t)(c.top + y) * c.rstride + 3 * (int64_t)c.left);
    const unsigned *d = reinterpret_cast<const unsigned *>(b & ~(uintptr_t)3);
    const int shift = (int)(b & 3), nbytes = 3 * a.R_w;
    const int nd = (shift + nbytes + 3) >> 2;
    bool hit = false;
    for (int i = lane; i < nd; i += 64) {
        const unsigned w = d[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int at = 4 * i + k - shift;
            hit |= at >= 0 && at < nbytes && ((w >> (8 * k)) & 0xFFu) > 1u;
        }
    }
    if (hit) a.any_gt1[z] = 1u;
}

__device__ __forceinline__ unsigned to_u8(float x) {
#pragma clang fp contract(off)
    if (!__builtin_isfinite(x)) return 0u;
    float v = x + 0.5f;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    v = no_fuse(v) * 255.0f;
    return (unsigned)v;  // v_cvt_u32_f32: truncation
}

// grid (ceil(HW / 1024), F, B), 4 pixels per lane.  VEC: HW % 4 == 0, x 16-byte and out 4-byte aligned
template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(256) void pixels_to_frames_kernel(const float *__restrict__ x, uint8_t *__restrict__ out, int F,
                                                               int64_t HW) {
    __shared__ unsigned stage[3 * 256];
    const int f = blockIdx.y, b = blockIdx.z;
    const int64_t pblock = (int64_t)blockIdx.x * 1024, p = pblock + 4 * threadIdx.x;
    const int64_t plane = (int64_t)F * HW;
    const float *xin = x + (int64_t)b * 3 * plane + (int64_t)f * HW + p;
    unsigned u[3][4];
    if (VEC && p + 4 <= HW) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(xin + ch * plane);
#pragma unroll
            for (int j = 0; j < 4; ++j) u[ch][j] = to_u8(v[j]);
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int j = 0; j < 4; ++j) u[ch][j] = p + j < HW ? to_u8(xin[ch * plane + j]) : 0u;
    }
    if (LAYOUT == OMNITOK_LAYOUT_THWC) {
        uint8_t *ob = out + ((int64_t)b * F + f) * HW * 3;
        if (VEC && pblock + 1024 <= HW) {  // block-uniform: every pixel of the block is in range
            // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            stage[3 * threadIdx.x + 0] = u[0][0] | u[1][0] << 8 | u[2][0] << 16 | u[0][1] << 24;
            stage[3 * threadIdx.x + 1] = u[1][1] | u[2][1] << 8 | u[0][2] << 16 | u[1][2] << 24;
            stage[3 * threadIdx.x + 2] = u[2][2] | u[0][3] << 8 | u[1][3] << 16 | u[2][3] << 24;
            __syncthreads();
            unsigned *od = reinterpret_cast<unsigned *>(ob + 3 * pblock);
#pragma unroll
            for (int k = 0; k < 3; ++k) od[threadIdx.x + 256 * k] = stage[threadIdx.x + 256 * k];
        } else {
            for (int j = 0; j < 4; ++j)
                if (p + j < HW)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) ob[3 * (p + j) + ch] = (uint8_t)u[ch][j];
        }
    } else {
        uint8_t *ob = out + (int64_t)b * 3 * plane + (int64_t)f * HW + p;
        if (VEC && p + 4 <= HW) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                *reinterpret_cast<unsigned *>(ob + ch * plane) = u[ch][0] | u[ch][1] << 8 | u[ch][2] << 16 | u[ch][3] << 24;
        } else {
            for (int j = 0; j < 4; ++j)
                if (p + j < HW)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) ob[ch * plane + j] = (uint8_t)u[ch][j];
        }
    }
}

// widest bilinear chunk (multiple of 4, >= 4) whose source taps fit one staged row: span <= sw * (n - 1) + 3 pixels
static int bilinear_chunk(float sw) {
    const int max_px = (4 * FR_SPAN_BILINEAR - 3 - 3) / 3 - 3;  // alignment shift + the floor's slack
    int n = (int)((double)max_px / (sw > 1.0f ? (double)sw : 1.0)) + 1;
    n = n > FR_CHUNK ? FR_CHUNK : n;
    n &= ~3;
    return n < 4 ? 4 : n;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_frames_to_pixels(const omnitok_frames_desc *desc, int B, int F_out, int R_h, int R_w, int mode,
                                        int flags, void *work, float *pixels_out, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(mode == OMNITOK_FRAMES_NONE || mode == OMNITOK_FRAMES_BILINEAR, "frames_to_pixels: mode %d", mode);
    OT_CHECK_ARG((flags & ~OMNITOK_FRAMES_VIDEONORM) == 0, "frames_to_pixels: unknown flags 0x%x", flags);
    const bool vn = flags & OMNITOK_FRAMES_VIDEONORM;
    OT_CHECK_ARG(!vn || mode == OMNITOK_FRAMES_NONE, "frames_to_pixels: OMNITOK_FRAMES_VIDEONORM applies to mode NONE only");
    OT_CHECK_ARG(B >= 0 && F_out >= 1 && F_out <= 65535 && R_h >= 1 && R_w >= 1,
                 "frames_to_pixels: bad sizes B %d F_out %d R_h %d R_w %d", B, F_out, R_h, R_w);
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG(desc && pixels_out, "frames_to_pixels: null pointer (desc %p, pixels_out %p)", (const void *)desc,
                 (void *)pixels_out);
    OT_CHECK_ARG(!vn || work, "frames_to_pixels: null work pointer (OMNITOK_FRAMES_VIDEONORM needs 4 * B bytes)");
    for (int i = 0; i < B; ++i) {
        const omnitok_frames_desc &d = desc[i];
        OT_CHECK_ARG(d.frames, "frames_to_pixels: clip %d: null frames pointer", i);
        OT_CHECK_ARG(d.F >= 1 && d.H >= 1 && d.W >= 1, "frames_to_pixels: clip %d: bad size %dx%dx%d", i, d.F, d.H, d.W);
        OT_CHECK_ARG(d.row_stride >= 3 * (int64_t)d.W && (d.F == 1 || d.frame_stride >= d.row_stride * (d.H - 1) + 3 * (int64_t)d.W),
                     "frames_to_pixels: clip %d: strides (%lld, %lld) bytes do not fit %dx%d x 3 frames", i,
                     (long long)d.frame_stride, (long long)d.row_stride, d.H, d.W);
        OT_CHECK_ARG(d.frame_start >= 0 && d.frame_step >= 1 &&
                         d.frame_start + (int64_t)(F_out - 1) * d.frame_step < d.F,
                     "frames_to_pixels: clip %d: frames %d + k * %d for k < %d run past F = %d", i, d.frame_start,
                     d.frame_step, F_out, d.F);
        if (mode == OMNITOK_FRAMES_NONE) {
            OT_CHECK_ARG(d.crop_top >= 0 && d.crop_left >= 0 && d.crop_top + (int64_t)R_h <= d.H &&
                             d.crop_left + (int64_t)R_w <= d.W,
                         "frames_to_pixels: clip %d: crop window %dx%d at (%d, %d) outside the %dx%d source", i, R_h, R_w,
                         d.crop_top, d.crop_left, d.H, d.W);
        } else {
            OT_CHECK_ARG(d.resize_h >= 1 && d.resize_w >= 1 && d.crop_top >= 0 && d.crop_left >= 0 &&
                             d.crop_top + (int64_t)R_h <= d.resize_h && d.crop_left + (int64_t)R_w <= d.resize_w,
                         "frames_to_pixels: clip %d: crop window %dx%d at (%d, %d) outside the %dx%d resized frame", i, R_h,
                         R_w, d.crop_top, d.crop_left, d.resize_h, d.resize_w);
            OT_CHECK_ARG(d.W <= (int64_t)FR_MAX_DOWNSCALE * d.resize_w,
                         "frames_to_pixels: clip %d: width %d -> %d is a downscale by more than %d", i, d.W, d.resize_w,
                         FR_MAX_DOWNSCALE);
        }
    }
    if (vn)
        if (int rc = device_fill_u32(work, 0u, B, stream)) return rc;
    for (int c0 = 0; c0 < B; c0 += FR_CLIPS) {
        const int n = B - c0 < FR_CLIPS ? B - c0 : FR_CLIPS;
        FrArgs a{};
        for (int i = 0; i < n; ++i) {
            const omnitok_frames_desc &d = desc[c0 + i];
            FrClip &c = a.c[i];
            c.src = d.frames;
            c.fstride = d.frame_stride;
            c.rstride = d.row_stride;
            c.F = d.F; c.H = d.H; c.W = d.W;
            c.f0 = d.frame_start; c.fstep = d.frame_step;
            c.top = d.crop_top; c.left = d.crop_left;
            c.rh = d.resize_h; c.rw = d.resize_w;
            if (mode == OMNITOK_FRAMES_BILINEAR) {
                c.sh = (float)d.H / (float)d.resize_h;  // torch's area_pixel_compute_scale (no scale_factor given)
                c.sw = (float)d.W / (float)d.resize_w;
                c.chunk = bilinear_chunk(c.sw);
            }
        }
        a.out = pixels_out;
        a.any_gt1 = vn ? static_cast<unsigned *>(work) + c0 : nullptr;
        a.F_out = F_out; a.R_h = R_h; a.R_w = R_w; a.clip0 = c0;
        const dim3 grid((unsigned)((R_h + FR_ROWS - 1) / FR_ROWS), (unsigned)F_out, (unsigned)n);
        if (mode == OMNITOK_FRAMES_BILINEAR) {
            hipLaunchKernelGGL((frames_to_pixels_kernel<OMNITOK_FRAMES_BILINEAR, false>), grid, dim3(256), 0, stream, a);
        } else if (vn) {
            hipLaunchKernelGGL(frames_any_gt1_kernel, grid, dim3(256), 0, stream, a);
            OT_LAUNCH_CHECK("frames_any_gt1");
            hipLaunchKernelGGL((frames_to_pixels_kernel<OMNITOK_FRAMES_NONE, true>), grid, dim3(256), 0, stream, a);
        } else {
            hipLaunchKernelGGL((frames_to_pixels_kernel<OMNITOK_FRAMES_NONE, false>), grid, dim3(256), 0, stream, a);
        }
        OT_LAUNCH_CHECK("frames_to_pixels");
    }
    return OMNITOK_OK;
}

extern "C" int omnitok_pixels_to_frames(const float *pixels, int B, int C, int F, int H, int W, int layout, uint8_t *out,
                                        omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(C == 3, "pixels_to_frames: C = %d, expected 3 channels", C);
    OT_CHECK_ARG(layout == OMNITOK_LAYOUT_THWC || layout == OMNITOK_LAYOUT_CTHW, "pixels_to_frames: layout %d", layout);
    OT_CHECK_ARG(B >= 0 && B <= 65535 && F >= 1 && F <= 65535 && H >= 1 && W >= 1,
                 "pixels_to_frames: bad sizes B %d F %d H %d W %d", B, F, H, W);
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG(pixels && out, "pixels_to_frames: null pointer (pixels %p, out %p)", (const void *)pixels, (void *)out);
    const int64_t HW = (int64_t)H * W;
    const bool vec = HW % 4 == 0 && aligned16(pixels) && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    const dim3 grid((unsigned)((HW + 1023) / 1024), (unsigned)F, (unsigned)B);
#define P2F(L, V) hipLaunchKernelGGL((pixels_to_frames_kernel<L, V>), grid, dim3(256), 0, stream, pixels, out, F, HW)
    if (layout == OMNITOK_LAYOUT_THWC) {
        if (vec) P2F(OMNITOK_LAYOUT_THWC, true); else P2F(OMNITOK_LAYOUT_THWC, false);
    } else {
        if (vec) P2F(OMNITOK_LAYOUT_CTHW, true); else P2F(OMNITOK_LAYOUT_CTHW, false);
    }
#undef P2F
    OT_LAUNCH_CHECK("pixels_to_frames");
    return OMNITOK_OK;
}
