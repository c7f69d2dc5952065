// What csrc/i3d.hip and csrc/inception.hip share (LPIPS's VGG16 trunk runs on the latter's conv): the implicit-GEMM
// convolution of I3D's Unit3D (and of Inception V3's BasicConv2d, as T = kt = 1 with explicit padding) with the host side of
// its two entry points, and the bilinear source arithmetic of their preprocess kernels.  The design is described at the top
// of csrc/i3d.hip.
#pragma once
#include "gemm_common.h"

namespace omnitok {

constexpr int CV_BK = 32;
constexpr int CV_LDT = 36;  // LDS row: 32 floats + 4 of padding (gemm.hip: conflict-free ds_read_b128 fragments)

struct CvArgs {
    const float *x;
    int64_t x_cs;
    int x_off;
    int T, H, W, Cin;
    const float *w;
    int64_t ldw;
    const float *bias;
    int N, kt, kh, kw, st, sh, sw, pt, ph, pw;
    int To, Ho, Wo;
    int64_t M;
    int nk, nbn;
    float *y;
    int64_t y_cs;
    int y_off;
    float *y2;
    int64_t y2_cs;
    int y2_off, split, relu;
};

// WN: waves along N.  2 is the 2 x 2 layout (BM = 64 WMT, BN = 64 WNT); 1 is 4 x 1 (BM = 128 WMT, BN = 32 WNT), for a
// narrow N that would leave half the MFMA columns of a 64-wide tile idle.
template <int WMT, int WNT, int WN = 2>
__global__ __launch_bounds__(256, 2) void conv3d_same_kernel(const CvArgs p) {
    static_assert(WN == 1 || WN == 2, "4 waves as (4 / WN) x WN");
    constexpr int BM = 32 * WMT * (4 / WN), BN = 32 * WNT * WN;
    constexpr int RA = BM / 32, RB = BN / 32;  // 16-byte groups per thread and K step
    constexpr int STAGE = (BM + BN) * CV_LDT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int r32 = lane & 31, hi = lane >> 5;
    const int lid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int64_t bm = lid / p.nbn;
    const int bn = lid % p.nbn;

    const int lrow = tid >> 3, lc4 = tid & 7;
    // rows of A this thread gathers: the clip's base position and the front-padded input corner of the output position
    int64_t abase[RA];
    int at[RA], ah[RA], aw[RA];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        int64_t m = bm * BM + lrow + 32 * i;
        const bool ok = m < p.M;
        if (!ok) m = 0;
        const int wo = (int)(m % p.Wo);
        int64_t r = m / p.Wo;
        const int ho = (int)(r % p.Ho);
        r /= p.Ho;
        const int to = (int)(r % p.To);
        const int64_t b = r / p.To;
        abase[i] = b * p.T * p.H * p.W;
        at[i] = ok ? to * p.st - p.pt : -(1 << 20);  // a row past M reads nothing (every tap is "outside")
        ah[i] = ho * p.sh - p.ph;
        aw[i] = wo * p.sw - p.pw;
    }
    const float *wp[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        int n = bn * BN + lrow + 32 * i;
        if (n > p.N - 1) n = p.N - 1;
        wp[i] = p.w + (int64_t)n * p.ldw + lc4 * 4;
    }
    // this thread's k = step * 32 + 4 lc4 as (tap = (dt, dh, dw), ci), advanced incrementally
    int ci = lc4 * 4, dt = 0, dh = 0, dw = 0;
    auto k_norm = [&]() {
        while (ci >= p.Cin) {
            ci -= p.Cin;
            if (++dw == p.kw) {
                dw = 0;
                if (++dh == p.kh) {
                    dh = 0;
                    ++dt;
                }
            }
        }
    };
    k_norm();

    const int st_off = lrow * CV_LDT + lc4 * 4;
    f32x4 ra[RA], rb[RB];
    auto gload = [&](int k0) {
        const bool tap_ok = dt < p.kt;  // k < K (the packed weight is zero up to Kpad as well)
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const int ti = at[i] + dt, yi = ah[i] + dh, xi = aw[i] + dw;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (tap_ok && (unsigned)ti < (unsigned)p.T && (unsigned)yi < (unsigned)p.H && (unsigned)xi < (unsigned)p.W)
                v = *reinterpret_cast<const f32x4 *>(p.x + (abase[i] + ((int64_t)ti * p.H + yi) * p.W + xi) * p.x_cs +
                                                     p.x_off + ci);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) rb[i] = *reinterpret_cast<const f32x4 *>(wp[i] + k0);
        ci += CV_BK;
        k_norm();
    };
    auto lstore = [&](int buf) {
        float *As = smem + buf * STAGE;
        float *Bs = As + BM * CV_LDT;
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<f32x4 *>(As + st_off + i * 32 * CV_LDT) = ra[i];
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4 *>(Bs + st_off + i * 32 * CV_LDT) = rb[i];
    };

    f32x16 acc[WMT][WNT];
#pragma unroll
    for (int i = 0; i < WMT; ++i)
#pragma unroll
        for (int j = 0; j < WNT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    gload(0);
    lstore(0);
    __syncthreads();
    const int a_frag_off = (wm * 32 * WMT + r32) * CV_LDT + hi * 16;
    const int b_frag_off = (wn * 32 * WNT + r32) * CV_LDT + hi * 16;
    for (int kt = 0; kt < p.nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < p.nk) gload((kt + 1) * CV_BK);
        const float *As = smem + buf * STAGE;
        const float *Bs = As + BM * CV_LDT;
        f32x4 af[WMT][4], bf[WNT][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int mb = 0; mb < WMT; ++mb)
                af[mb][j] = *reinterpret_cast<const f32x4 *>(As + a_frag_off + mb * 32 * CV_LDT + 4 * j);
#pragma unroll
            for (int nb = 0; nb < WNT; ++nb)
                bf[nb][j] = *reinterpret_cast<const f32x4 *>(Bs + b_frag_off + nb * 32 * CV_LDT + 4 * j);
        }
        // MFMA step (j, e): k = 4 j + e (lanes 0-31) and 16 + 4 j + e (lanes 32-63), for A and B alike
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mb = 0; mb < WMT; ++mb)
#pragma unroll
                    for (int nb = 0; nb < WNT; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mb][j][e], bf[nb][j][e], acc[mb][nb], 0, 0, 0);
        if (kt + 1 < p.nk) lstore(buf ^ 1);
        __syncthreads();
    }

#pragma unroll
    for (int nb = 0; nb < WNT; ++nb) {
        const int n = bn * BN + wn * 32 * WNT + nb * 32 + r32;
        if (n >= p.N) continue;
        const float bias = p.bias[n];
        float *dst;
        int64_t cs;
        if (n < p.split) {
            dst = p.y + p.y_off + n;
            cs = p.y_cs;
        } else {
            dst = p.y2 + p.y2_off + (n - p.split);
            cs = p.y2_cs;
        }
#pragma unroll
        for (int mb = 0; mb < WMT; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = bm * BM + wm * 32 * WMT + mb * 32 + mfma32_row(r, hi);
                if (m >= p.M) continue;
                float v = acc[mb][nb][r] + bias;
                if (p.relu && v < 0.0f) v = 0.0f;
                dst[m * cs] = v;
            }
    }
}

__device__ __forceinline__ void pre_src(float scale, int dst, int in, int out, int &i0, int &i1, float &l0, float &l1) {
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

__device__ __forceinline__ float pre_lerp(float a, float b, float w0, float w1) {
#pragma clang fp contract(off)
    return __builtin_fmaf(b, w1, no_fuse(a * w0));
}

// one launch of the kernel over nbm row tiles (the caller's BM); `what` names the entry point in errors
template <int WMT, int WNT, int WN = 2>
static int conv_launch(const CvArgs &a, int64_t nbm, hipStream_t stream, const char *what = "conv3d_same") {
    constexpr int BM = 32 * WMT * (4 / WN), BN = 32 * WNT * WN;
    constexpr int lds = 2 * (BM + BN) * CV_LDT * 4;
    const void *k = reinterpret_cast<const void *>(conv3d_same_kernel<WMT, WNT, WN>);
    if (int rc = set_max_dynamic_lds(k, lds)) return rc;
    CvArgs p = a;
    p.nbn = (a.N + BN - 1) / BN;
    const int64_t tiles = nbm * p.nbn;
    OT_CHECK_ARG(tiles <= 0x7fffffff, "%s: %lld tiles", what, (long long)tiles);
    hipLaunchKernelGGL((conv3d_same_kernel<WMT, WNT, WN>), dim3((unsigned)tiles), dim3(256), lds, stream, p);
    OT_LAUNCH_CHECK(what);
    return OMNITOK_OK;
}

// What omnitok_conv3d_same and omnitok_conv2d check and fill alike, for a descriptor D (omnitok_conv3d, omnitok_conv2d_desc)
// whose sizes, kernel, strides and padding the caller has checked and written to `a` with the output grid and ldw: the
// channel windows of x, y and y2, then (unless batch == 0: nothing is read, so null pointers are fine, and the caller returns)
// the pointers, the rest of `a` and the size limit.
template <class D>
static int conv_args(const D *c, const char *what, int batch, CvArgs &a) {
    OT_CHECK_ARG(c->x_off >= 0 && c->x_off % 4 == 0 && c->x_cs % 4 == 0 && c->x_off + c->Cin <= c->x_cs,
                 "%s: input channels [%d, %d) outside the %lld per position, or not 16-byte groups", what, c->x_off,
                 c->x_off + c->Cin, (long long)c->x_cs);
    OT_CHECK_ARG(c->split >= 1 && c->split <= c->Cout, "%s: split %d outside 1..Cout (%d)", what, c->split, c->Cout);
    OT_CHECK_ARG(c->y_off >= 0 && c->y_off + c->split <= c->y_cs, "%s: output channels [%d, %d) outside the %lld per "
                 "position", what, c->y_off, c->y_off + c->split, (long long)c->y_cs);
    if (c->split < c->Cout)
        OT_CHECK_ARG(c->y2_off >= 0 && c->y2_off + (c->Cout - c->split) <= c->y2_cs, "%s: second output channels [%d, %d) "
                     "outside the %lld per position", what, c->y2_off, c->y2_off + c->Cout - c->split, (long long)c->y2_cs);
    if (batch == 0) return OMNITOK_OK;
    OT_CHECK_ARG(c->x && c->w && c->bias && c->y && (c->split == c->Cout || c->y2), "%s: null pointer", what);
    OT_CHECK_ARG(aligned16(c->x) && aligned16(c->w), "%s: x and w must be 16-byte aligned", what);
    a.x = c->x;
    a.x_cs = c->x_cs;
    a.x_off = c->x_off;
    a.Cin = c->Cin;
    a.w = c->w;
    a.bias = c->bias;
    a.N = c->Cout;
    a.M = (int64_t)batch * a.To * a.Ho * a.Wo;
    OT_CHECK_ARG((int64_t)batch * a.T * a.H * a.W * c->x_cs < (1ll << 40) && a.M * std::max(c->y_cs, c->y2_cs) < (1ll << 40),
                 "%s: tensors too large", what);
    a.nk = (int)(a.ldw / CV_BK);
    a.y = c->y;
    a.y_cs = c->y_cs;
    a.y_off = c->y_off;
    a.y2 = c->y2;
    a.y2_cs = c->y2_cs;
    a.y2_off = c->y2_off;
    a.split = c->split;
    a.relu = c->relu;
    return OMNITOK_OK;
}

}  // namespace omnitok
