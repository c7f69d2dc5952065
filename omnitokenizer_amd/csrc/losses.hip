// Validation losses of the reference's VQGAN.forward(x) (omnitokenizer.py:388-394, 372-377; modules/codebook.py:93), as
// streaming reductions that read every operand once:
//
//   recon_losses_kernel   x, x_recon [B][n] -> per item  sum |xr - x|,  sum (xr - x)^2,  sum |xl - rl|  with
//                         xl = 0.8f * (x + 0.5f) + 0.1f, rl likewise from xr (logits_laplace, eps = 0.1)
//   commitment_kernel     z [N][c], ids [N], E [n_codes][c] -> sum (z - E[id])^2, the code row gathered in the kernel
//   kl_kernel             moments [B][2][m] (mean | logvar) -> per item  sum ((mu^2 + exp(lv)) - 1) - lv,
//                         lv = min(max(logvar, -30), 20)
//
// Every summand is formed in fp32, operation by operation as torch forms it (no contraction: products pass no_fuse), then
// widened and added in fp64.  The one exception is exp(lv) of the KL term: it is the device's fp64 exp rounded to fp32,
// which is the correctly rounded fp32 exponential except where the fp64 result lies within its own error (under 1 ulp of
// fp64) of an fp32 rounding boundary.  torch's fp32 exp (SLEEF on the CPU, the device's expf on a GPU) is faithfully but
// not correctly rounded, so that summand can differ from the reference's by one fp32 ulp of exp(lv); every other
// operation of every summand is the reference's own.
//
// Partition: an item is cut into P parts, P = ceil(G / B) with G = 8 blocks per CU (at most LS_MAX_GRID), never more parts
// than the item has 256-thread rounds.  Block (p, b) walks item b's 16-byte groups p * 256 + tid, + P * 256, ...; each thread
// adds its summands in that order, the 64 lanes of a wave are combined by a xor butterfly, the 4 waves in order through
// LDS, and the block's sums go to work[(b * P + p) * K + k].  The up to 6 elements of an item outside its 16-byte groups
// are taken by threads 0..5 of part 0.  losses_finalize_kernel adds the P partials of every (b, k) in index order, then the B
// item sums in index order.  No atomics: the result depends on (shape, CU count) alone.
#include "common.h"

#include <math.h>

namespace omnitok {

constexpr int LS_THREADS = 256;
constexpr int LS_MAX_GRID = 4096;
constexpr int LS_BLOCKS_PER_CU = 8;
constexpr int LS_UNROLL = 4;

// the 16-byte groups of elements [s, s + n) of a 16-byte aligned array: [a0, a1) in elements; none if vec is off
struct LsSpan {
    int64_t s, a0, a1, e;
};
__device__ __forceinline__ LsSpan ls_span(int64_t s, int64_t n, int vec) {
    LsSpan sp;
    sp.s = s;
    sp.e = s + n;
    sp.a0 = vec ? min((s + 3) & ~(int64_t)3, sp.e) : sp.e;
    sp.a1 = vec ? max(sp.e & ~(int64_t)3, sp.a0) : sp.e;
    if (!vec) sp.a0 = sp.a1 = s;  // everything is "tail": [a1, e)
    return sp;
}

template <int K>
__device__ __forceinline__ void ls_block_reduce(double (&acc)[K], double *__restrict__ part) {
    __shared__ double red[K][LS_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
        if (lane == 0) red[k][wave] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * K + k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    }
}

// the three summands of one element pair, each operation rounded in fp32 as torch rounds it
template <int FLAGS>
__device__ __forceinline__ void recon_terms(float x, float r, double (&acc)[3]) {
#pragma clang fp contract(off)
    const float d = r - x;
    if (FLAGS & OMNITOK_LOSS_L1) acc[0] += (double)fabsf(d);
    if (FLAGS & OMNITOK_LOSS_MSE) acc[1] += (double)no_fuse(d * d);
    if (FLAGS & OMNITOK_LOSS_LAPLACE) {
        const float xs = x + 0.5f, rs = r + 0.5f;
        const float xl = no_fuse(0.8f * xs) + 0.1f, rl = no_fuse(0.8f * rs) + 0.1f;
        acc[2] += (double)fabsf(xl - rl);
    }
}

// grid (P, B)
template <int FLAGS>
__global__ __launch_bounds__(LS_THREADS) void recon_losses_kernel(const float *__restrict__ x, const float *__restrict__ xr,
                                                                  int64_t n, int vec, double *__restrict__ part) {
#pragma clang fp contract(off)
    const LsSpan sp = ls_span((int64_t)blockIdx.y * n, n, vec);
    const int64_t nvec = (sp.a1 - sp.a0) >> 2, stride = (int64_t)gridDim.x * LS_THREADS;
    const f32x4 *xv = reinterpret_cast<const f32x4 *>(x + sp.a0), *rv = reinterpret_cast<const f32x4 *>(xr + sp.a0);
    double acc[3] = {0.0, 0.0, 0.0};
    int64_t v = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    for (; v + (LS_UNROLL - 1) * stride < nvec; v += LS_UNROLL * stride) {
        f32x4 a[LS_UNROLL], b[LS_UNROLL];
#pragma unroll
        for (int u = 0; u < LS_UNROLL; ++u) {
            a[u] = __builtin_nontemporal_load(xv + v + u * stride);
            b[u] = __builtin_nontemporal_load(rv + v + u * stride);
        }
#pragma unroll
        for (int u = 0; u < LS_UNROLL; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) recon_terms<FLAGS>(a[u][j], b[u][j], acc);
    }
    for (; v < nvec; v += stride) {
        const f32x4 a = __builtin_nontemporal_load(xv + v), b = __builtin_nontemporal_load(rv + v);
#pragma unroll
        for (int j = 0; j < 4; ++j) recon_terms<FLAGS>(a[j], b[j], acc);
    }
    // elements outside the 16-byte groups: [s, a0) and [a1, e) (everything when vec is off)
    if (vec) {
        if (blockIdx.x == 0) {
            const int64_t nh = sp.a0 - sp.s, nt = sp.e - sp.a1;
            if (threadIdx.x < nh) recon_terms<FLAGS>(x[sp.s + threadIdx.x], xr[sp.s + threadIdx.x], acc);
            else if (threadIdx.x - nh < nt) recon_terms<FLAGS>(x[sp.a1 + threadIdx.x - nh], xr[sp.a1 + threadIdx.x - nh], acc);
        }
    } else {
        for (int64_t i = sp.s + (int64_t)blockIdx.x * LS_THREADS + threadIdx.x; i < sp.e; i += stride)
            recon_terms<FLAGS>(x[i], xr[i], acc);
    }
    ls_block_reduce<3>(acc, part);
}

// F.mse_loss(z, embeddings)'s summand
__device__ __forceinline__ double commit_term(float z, float e) {
#pragma clang fp contract(off)
    const float d = z - e;
    return (double)no_fuse(d * d);
}

// grid (P, 1).  z [N][c], c % 4 == 0 when vec.  An id outside [0, n_codes) reads nothing and makes the sum NaN.
__global__ __launch_bounds__(LS_THREADS) void commitment_kernel(const float *__restrict__ z, const int64_t *__restrict__ ids,
                                                                const float *__restrict__ E, int64_t N, int c, int n_codes,
                                                                int vec, double *__restrict__ part) {
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)gridDim.x * LS_THREADS, first = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    double acc[1] = {0.0};
    if (vec) {
        const int gpr = c >> 2;  // 16-byte groups per row
        const int64_t nvec = N * gpr;
        const f32x4 *zv = reinterpret_cast<const f32x4 *>(z);
        for (int64_t v = first; v < nvec; v += stride) {
            const int64_t tok = v / gpr;
            const int g = (int)(v - tok * gpr);
            const int64_t id = ids[tok];
            const f32x4 a = __builtin_nontemporal_load(zv + v);
            if ((uint64_t)id < (uint64_t)n_codes) {
                const f32x4 e = *reinterpret_cast<const f32x4 *>(E + id * c + 4 * g);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[0] += commit_term(a[j], e[j]);
            } else {
                acc[0] = __builtin_nan("");
            }
        }
    } else {
        const int64_t total = N * c;
        for (int64_t i = first; i < total; i += stride) {
            const int64_t tok = i / c;
            const int64_t id = ids[tok];
            if ((uint64_t)id < (uint64_t)n_codes) acc[0] += commit_term(z[i], E[id * c + (i - tok * c)]);
            else acc[0] = __builtin_nan("");
        }
    }
    ls_block_reduce<1>(acc, part);
}

// DiagonalGaussianDistribution.kl()'s summand: torch.pow(mean, 2) + var - 1.0 - logvar, left to right
__device__ __forceinline__ double kl_term(float mu, float logvar) {
#pragma clang fp contract(off)
    const float lv = fminf(fmaxf(logvar, -30.0f), 20.0f);  // torch.clamp; a NaN stays a NaN through the sum below
    const float var = (float)exp((double)lv);
    const float t = ((no_fuse(mu * mu) + var) - 1.0f) - (logvar != logvar ? logvar : lv);
    return (double)t;
}

// grid (P, B).  moments [B][2][m]: item b's means at b * 2m, its log-variances at b * 2m + m
__global__ __launch_bounds__(LS_THREADS) void kl_kernel(const float *__restrict__ mom, int64_t m, int vec,
                                                        double *__restrict__ part) {
#pragma clang fp contract(off)
    const float *mu = mom + (int64_t)blockIdx.y * 2 * m, *lv = mu + m;
    const int64_t stride = (int64_t)gridDim.x * LS_THREADS, first = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    double acc[1] = {0.0};
    if (vec) {  // m % 4 == 0 and a 16-byte aligned base: both halves of every item are aligned
        const f32x4 *mv = reinterpret_cast<const f32x4 *>(mu), *lvv = reinterpret_cast<const f32x4 *>(lv);
        for (int64_t v = first; v < (m >> 2); v += stride) {
            const f32x4 a = __builtin_nontemporal_load(mv + v), b = __builtin_nontemporal_load(lvv + v);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[0] += kl_term(a[j], b[j]);
        }
    } else {
        for (int64_t i = first; i < m; i += stride) acc[0] += kl_term(mu[i], lv[i]);
    }
    ls_block_reduce<1>(acc, part);
}

// one block: out[b][k] = part[b][0][k] + part[b][1][k] + ... in index order; total[k] = out[0][k] + out[1][k] + ...
__global__ __launch_bounds__(LS_THREADS) void losses_finalize_kernel(const double *__restrict__ part, int B, int P, int K,
                                                                     double *__restrict__ out, double *__restrict__ total) {
    for (int i = threadIdx.x; i < B * K; i += LS_THREADS) {
        const int b = i / K, k = i - b * K;
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += part[((int64_t)b * P + p) * K + k];
        out[i] = s;
    }
    __syncthreads();  // out[] was written by this block's own threads
    if (total && threadIdx.x < K) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += out[b * K + threadIdx.x];
        total[threadIdx.x] = s;
    }
}

// parts per item for B items of `rounds` 256-thread rounds each
static int ls_parts(int B, int64_t rounds, int *P) {
    int cus = 0;
    if (int rc = current_device_cus(&cus)) return rc;
    int G = cus * LS_BLOCKS_PER_CU;
    if (G > LS_MAX_GRID) G = LS_MAX_GRID;
    if (G < 1) G = 1;
    int64_t p = (G + B - 1) / B;
    if (p > rounds) p = rounds;
    if (p < 1) p = 1;
    *P = (int)p;
    return OMNITOK_OK;
}

static int ls_check_work(const char *what, int B, void *work, size_t work_bytes) {
    const int64_t need = omnitok_losses_workspace(B);
    OT_CHECK_ARG(need >= 0, "%s: bad batch %d", what, B);
    OT_CHECK_ARG(work, "%s: null pointer (work, %lld bytes needed)", what, (long long)need);
    OT_CHECK_ARG(work_bytes >= (size_t)need, "%s: workspace of %zu bytes, %lld needed", what, work_bytes, (long long)need);
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 7) == 0, "%s: workspace is not 8-byte aligned", what);
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int64_t omnitok_losses_workspace(int B) {
    if (B < 1 || B > 65535) return -1;
    // B * P partial triples with B * P < B + LS_MAX_GRID
    return ((int64_t)B + LS_MAX_GRID) * 3 * (int64_t)sizeof(double);
}

extern "C" int omnitok_recon_losses(const float *x, const float *x_recon, int B, int64_t n, int flags, double *sums,
                                    double *total, void *work, size_t work_bytes, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int all = OMNITOK_LOSS_L1 | OMNITOK_LOSS_MSE | OMNITOK_LOSS_LAPLACE;
    OT_CHECK_ARG(flags != 0 && (flags & ~all) == 0, "recon_losses: flags 0x%x", flags);
    OT_CHECK_ARG(B >= 1 && B <= 65535 && n >= 1, "recon_losses: bad sizes B %d n %lld", B, (long long)n);
    OT_CHECK_ARG(x && x_recon, "recon_losses: null pointer (x / x_recon)");
    OT_CHECK_ARG(sums, "recon_losses: null pointer (sums output)");
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(x_recon) & 3) == 0,
                 "recon_losses: operands are not 4-byte aligned");
    if (int rc = ls_check_work("recon_losses", B, work, work_bytes)) return rc;
    const int vec = aligned16(x) && aligned16(x_recon);
    int P = 1;
    if (int rc = ls_parts(B, (n / 4 + LS_THREADS - 1) / LS_THREADS, &P)) return rc;
    const dim3 grid((unsigned)P, (unsigned)B);
    double *part = static_cast<double *>(work);
#define LS_CASE(F)                                                                                                   \
    case F:                                                                                                          \
        hipLaunchKernelGGL(recon_losses_kernel<F>, grid, dim3(LS_THREADS), 0, stream, x, x_recon, n, vec, part);     \
        break;
    switch (flags) {
        LS_CASE(1) LS_CASE(2) LS_CASE(3) LS_CASE(4) LS_CASE(5) LS_CASE(6) LS_CASE(7)
    }
#undef LS_CASE
    OT_LAUNCH_CHECK("recon_losses");
    hipLaunchKernelGGL(losses_finalize_kernel, dim3(1), dim3(LS_THREADS), 0, stream, part, B, P, 3, sums, total);
    OT_LAUNCH_CHECK("losses_finalize");
    return OMNITOK_OK;
}

extern "C" int omnitok_commitment_sum(const float *z, const int64_t *ids, const float *codebook, int64_t n_tokens, int c,
                                      int n_codes, double *sum, void *work, size_t work_bytes, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(n_tokens >= 1 && c >= 1 && n_codes >= 1, "commitment_sum: bad sizes n_tokens %lld c %d n_codes %d",
                 (long long)n_tokens, c, n_codes);
    OT_CHECK_ARG(z && ids && codebook, "commitment_sum: null pointer (z / ids / codebook)");
    OT_CHECK_ARG(sum, "commitment_sum: null pointer (sum output)");
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(z) & 3) == 0 && (reinterpret_cast<uintptr_t>(codebook) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(ids) & 7) == 0,
                 "commitment_sum: operands are not aligned to their element size");
    if (int rc = ls_check_work("commitment_sum", 1, work, work_bytes)) return rc;
    const int vec = c % 4 == 0 && aligned16(z) && aligned16(codebook);
    const int64_t units = vec ? n_tokens * (c / 4) : n_tokens * c;
    int P = 1;
    if (int rc = ls_parts(1, (units + LS_THREADS - 1) / LS_THREADS, &P)) return rc;
    double *part = static_cast<double *>(work);
    hipLaunchKernelGGL(commitment_kernel, dim3((unsigned)P), dim3(LS_THREADS), 0, stream, z, ids, codebook, n_tokens, c,
                       n_codes, vec, part);
    OT_LAUNCH_CHECK("commitment_sum");
    hipLaunchKernelGGL(losses_finalize_kernel, dim3(1), dim3(LS_THREADS), 0, stream, part, 1, P, 1, sum,
                       static_cast<double *>(nullptr));
    OT_LAUNCH_CHECK("losses_finalize");
    return OMNITOK_OK;
}

extern "C" int omnitok_kl_sum(const float *moments, int B, int64_t m, double *sums, double *total, void *work,
                              size_t work_bytes, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(B >= 1 && B <= 65535 && m >= 1, "kl_sum: bad sizes B %d m %lld", B, (long long)m);
    OT_CHECK_ARG(moments, "kl_sum: null pointer (moments)");
    OT_CHECK_ARG(sums, "kl_sum: null pointer (sums output)");
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(moments) & 3) == 0, "kl_sum: moments are not 4-byte aligned");
    if (int rc = ls_check_work("kl_sum", B, work, work_bytes)) return rc;
    const int vec = m % 4 == 0 && aligned16(moments);
    int P = 1;
    if (int rc = ls_parts(B, ((vec ? m / 4 : m) + LS_THREADS - 1) / LS_THREADS, &P)) return rc;
    double *part = static_cast<double *>(work);
    hipLaunchKernelGGL(kl_kernel, dim3((unsigned)P, (unsigned)B), dim3(LS_THREADS), 0, stream, moments, m, vec, part);
    OT_LAUNCH_CHECK("kl_sum");
    hipLaunchKernelGGL(losses_finalize_kernel, dim3(1), dim3(LS_THREADS), 0, stream, part, B, P, 1, sums, total);
    OT_LAUNCH_CHECK("losses_finalize");
    return OMNITOK_OK;
}
