// Token cross-entropy and top-k hits of the LM validation step (reference lm_transformer.py:308-321: F.cross_entropy and
// utils.accuracy(topk=(1, 5)) on [N, V] logits), as ONE read of the logits:
//
//   ce_rows_small_kernel  V <= 1024: a wave per row, the row in 16 registers per lane (dword loads, any alignment), the maximum
//                         first, then s = sum exp(l_j - m): the plain two-phase form with a single memory pass
//   ce_rows_kernel        V >  1024: a 256-thread workgroup per row.  A row need not be 16-byte aligned (V = 9217, 17409 are odd):
//                         its first (0..3) and last (0..3) elements are peeled off as scalars, the rest are 16-byte loads, four in
//                         flight per thread.  Every lane keeps an online (max, sum) pair, rescaled when its maximum grows; at the
//                         end the row maximum m is found (exact), every lane rescales ONCE to m, and the sums are added lanes by
//                         xor butterfly, waves 0..3 in order
//   both                  l_t is read first; rank = #{l_j > l_t} + #{j < t : l_j == l_t} is counted in the same pass (integers);
//                         nll = (m + log s) - l_t in fp32.  t < 0: nll 0, rank -1 (ignored); t >= V: nll NaN, rank V, nothing read
//   ce_reduce_kernel      nll / rank [N] -> per workgroup (sum nll, counted, rank == 0, rank < 5) over a contiguous segment of rows,
//   ce_final_kernel       ... and the workgroups' partials added in index order.  fp64, no atomics: equal bits on every call
//
// Grids come from the CU count and walk the rows by grid stride; row offsets are 64-bit.  HBM / L2 bound: one expf per element
// plus one per 16 elements for the rescale.
#include "common.h"
#include "../../include/omnitok_lm.h"

#include <math.h>

namespace omnitok {

constexpr int CE_THREADS = 256;
constexpr int CE_WAVES = CE_THREADS / 64;
constexpr int CE_BLOCKS_PER_CU = 8;
constexpr int CE_MAX_GRID = 4096;
constexpr int CE_SMALL_REGS = 16;
constexpr int CE_SMALL_V = 64 * CE_SMALL_REGS;  // the widest row a wave holds in registers
constexpr int CE_UNROLL = 4;                    // 16-byte loads in flight per thread

__device__ __forceinline__ float ce_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float ce_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int ce_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// does entry j with value x come before the target (value lt at index t) in a descending, lowest-index-first order
__device__ __forceinline__ int ce_beats(float x, int j, float lt, int t) { return (x > lt) | ((x == lt) & (j < t)); }

// rows that read no logits: 1 = handled
__device__ __forceinline__ bool ce_row_without_logits(int64_t t, int V, bool writer, float *nll, int32_t *rank) {
    if (t >= 0 && t < V) return false;
    if (writer) {
        *nll = t < 0 ? 0.0f : __builtin_nanf("");
        *rank = t < 0 ? -1 : V;
    }
    return true;
}

// grid-stride over rows, one wave each
__global__ __launch_bounds__(CE_THREADS) void ce_rows_small_kernel(const float *__restrict__ logits, int64_t ld,
                                                                   const int64_t *__restrict__ targets, int64_t N, int V,
                                                                   float *__restrict__ nll, int32_t *__restrict__ rank) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t row = (int64_t)blockIdx.x * CE_WAVES + wave; row < N; row += (int64_t)gridDim.x * CE_WAVES) {
        const int64_t t64 = targets[row];
        if (ce_row_without_logits(t64, V, lane == 0, nll + row, rank + row)) continue;
        const int t = (int)t64;
        const float *p = logits + row * ld;
        const float lt = p[t];
        float x[CE_SMALL_REGS];
        float m = -INFINITY;
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < CE_SMALL_REGS; ++k) {
            const int j = lane + 64 * k;
            x[k] = j < V ? p[j] : -INFINITY;
            m = fmaxf(m, x[k]);
            cnt += j < V ? ce_beats(x[k], j, lt, t) : 0;
        }
        m = ce_wave_max(m);
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < CE_SMALL_REGS; ++k)
            if (64 * k < V) s += lane + 64 * k < V ? expf(x[k] - m) : 0.0f;
        s = ce_wave_sum(s);
        cnt = ce_wave_sum(cnt);
        if (lane == 0) {
            nll[row] = (m + logf(s)) - lt;
            rank[row] = cnt;
        }
    }
}

// n more elements into a lane's online (m, s): s = sum exp(x - m) over what the lane has seen
template <int n>
__device__ __forceinline__ void ce_absorb(float &m, float &s, const float (&x)[n]) {
#pragma clang fp contract(off)
    float cmax = x[0];
#pragma unroll
    for (int k = 1; k < n; ++k) cmax = fmaxf(cmax, x[k]);
    if (cmax > m) {
        s = s * expf(m - cmax);  // m = -inf: 0 * 0
        m = cmax;
    }
    const float base = m > -INFINITY ? m : 0.0f;  // nothing but -inf so far: every term is exp(-inf) = 0
#pragma unroll
    for (int k = 0; k < n; ++k) s += expf(x[k] - base);
}

// grid-stride over rows, one workgroup each
__global__ __launch_bounds__(CE_THREADS) void ce_rows_kernel(const float *__restrict__ logits, int64_t ld,
                                                             const int64_t *__restrict__ targets, int64_t N, int V,
                                                             float *__restrict__ nll, int32_t *__restrict__ rank) {
#pragma clang fp contract(off)
    __shared__ float red_m[CE_WAVES], red_s[CE_WAVES];
    __shared__ int red_c[CE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t row = blockIdx.x; row < N; row += gridDim.x) {
        const int64_t t64 = targets[row];
        if (ce_row_without_logits(t64, V, tid == 0, nll + row, rank + row)) continue;  // the same branch in every thread
        const int t = (int)t64;
        const float *p = logits + row * ld;
        const float lt = p[t];
        // [0, head) scalars | nvec 16-byte groups | [tail0, V) scalars
        const int head = min(V, (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2));
        const int nvec = (V - head) >> 2, tail0 = head + 4 * nvec;
        const f32x4 *pv = reinterpret_cast<const f32x4 *>(p + head);
        float m = -INFINITY, s = 0.0f;
        int cnt = 0;
        int v = tid;
        for (; v + (CE_UNROLL - 1) * CE_THREADS < nvec; v += CE_UNROLL * CE_THREADS) {
            f32x4 a[CE_UNROLL];
#pragma unroll
            for (int u = 0; u < CE_UNROLL; ++u) a[u] = __builtin_nontemporal_load(pv + v + u * CE_THREADS);
            float x[4 * CE_UNROLL];
#pragma unroll
            for (int u = 0; u < CE_UNROLL; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    x[4 * u + k] = a[u][k];
                    cnt += ce_beats(a[u][k], head + 4 * (v + u * CE_THREADS) + k, lt, t);
                }
            ce_absorb(m, s, x);
        }
        for (; v < nvec; v += CE_THREADS) {
            const f32x4 a = __builtin_nontemporal_load(pv + v);
            const float x[4] = {a[0], a[1], a[2], a[3]};
#pragma unroll
            for (int k = 0; k < 4; ++k) cnt += ce_beats(x[k], head + 4 * v + k, lt, t);
            ce_absorb(m, s, x);
        }
        {  // the up to 6 elements outside the 16-byte groups: threads 0 .. 5
            const int j = tid < head ? tid : tail0 + (tid - head);
            if (j < V && (tid < head || j >= tail0)) {
                const float x[1] = {p[j]};
                cnt += ce_beats(x[0], j, lt, t);
                ce_absorb(m, s, x);
            }
        }
        // the row maximum (exact), then every lane's sum rescaled to it once
        const float wm = ce_wave_max(m);
        if (lane == 0) red_m[wave] = wm;
        __syncthreads();
        const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        float sl = m == M ? s : s * expf(m - M);
        sl = ce_wave_sum(sl);
        cnt = ce_wave_sum(cnt);
        if (lane == 0) {
            red_s[wave] = sl;
            red_c[wave] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
            const float S = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
            nll[row] = (M + logf(S)) - lt;
            rank[row] = ((red_c[0] + red_c[1]) + red_c[2]) + red_c[3];
        }
        // the next row writes red_m only after every thread passed the second barrier, red_s / red_c only after the next first one
    }
}

// workgroup p: rows [p * L, min(N, (p + 1) * L)) -> part[p][4]
__global__ __launch_bounds__(CE_THREADS) void ce_reduce_kernel(const float *__restrict__ nll, const int32_t *__restrict__ rank,
                                                               int64_t N, int64_t L, int V, double *__restrict__ part) {
    __shared__ double red[4][CE_WAVES];
    const int64_t r0 = (int64_t)blockIdx.x * L, r1 = min(N, r0 + L);
    double sum = 0.0;
    int64_t counted = 0, top1 = 0, top5 = 0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += CE_THREADS) {
        const int r = rank[i];
        if (r < 0) continue;  // ignored row
        sum += (double)nll[i];
        counted += 1;
        top1 += r == 0 && r < V;
        top5 += r < 5 && r < V;  // rank == V marks an invalid target
    }
    double acc[4] = {sum, (double)counted, (double)top1, (double)top5};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
        if (lane == 0) red[k][wave] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        part[(int64_t)blockIdx.x * 4 + k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    }
}

__global__ void ce_final_kernel(const double *__restrict__ part, int P, double *__restrict__ sums) {
    if (threadIdx.x < 4) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += part[(int64_t)p * 4 + threadIdx.x];
        sums[threadIdx.x] = s;
    }
}

static int ce_grid(int64_t units, int *grid) {
    int cus = 0;
    if (int rc = current_device_cus(&cus)) return rc;
    int64_t g = (int64_t)cus * CE_BLOCKS_PER_CU;
    if (g > CE_MAX_GRID) g = CE_MAX_GRID;
    if (g > units) g = units;
    if (g < 1) g = 1;
    *grid = (int)g;
    return OMNITOK_OK;
}

int lm_token_ce_rows(const float *logits, int64_t ld, const int64_t *targets, int64_t N, int V, float *nll, int32_t *rank,
                     hipStream_t stream) {
    OT_CHECK_ARG(N >= 1 && N <= ((int64_t)1 << 31) && V >= 1 && ld >= V, "lm_token_ce: bad sizes N %lld V %d ld %lld",
                 (long long)N, V, (long long)ld);
    OT_CHECK_ARG(logits && targets && nll && rank, "lm_token_ce: null pointer (logits / targets / nll / rank)");
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 3) == 0 && (reinterpret_cast<uintptr_t>(targets) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(nll) & 3) == 0 && (reinterpret_cast<uintptr_t>(rank) & 3) == 0,
                 "lm_token_ce: operands are not aligned to their element size");
    int grid = 1;
    if (V <= CE_SMALL_V) {
        if (int rc = ce_grid((N + CE_WAVES - 1) / CE_WAVES, &grid)) return rc;
        hipLaunchKernelGGL(ce_rows_small_kernel, dim3((unsigned)grid), dim3(CE_THREADS), 0, stream, logits, ld, targets, N, V,
                           nll, rank);
    } else {
        if (int rc = ce_grid(N, &grid)) return rc;
        hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)grid), dim3(CE_THREADS), 0, stream, logits, ld, targets, N, V, nll,
                           rank);
    }
    OT_LAUNCH_CHECK("lm_token_ce_rows");
    return OMNITOK_OK;
}

int lm_token_ce_reduce(const float *nll, const int32_t *rank, int64_t N, int V, double *sums, void *work, int64_t work_bytes,
                       hipStream_t stream) {
    const int64_t need = omnitok_lm_token_ce_workspace(N);
    OT_CHECK_ARG(need >= 0 && V >= 1, "lm_token_ce: bad sizes N %lld V %d", (long long)N, V);
    OT_CHECK_ARG(nll && rank && sums, "lm_token_ce: null pointer (nll / rank / sums)");
    OT_CHECK_ARG(work, "lm_token_ce: null pointer (work, %lld bytes needed)", (long long)need);
    OT_CHECK_ARG(work_bytes >= need, "lm_token_ce: workspace of %lld bytes, %lld needed", (long long)work_bytes,
                 (long long)need);
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 7) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7) == 0,
                 "lm_token_ce: workspace / sums are not 8-byte aligned");
    int grid = 1;
    if (int rc = ce_grid((N + CE_THREADS - 1) / CE_THREADS, &grid)) return rc;
    const int64_t L = (N + grid - 1) / grid;
    const int P = (int)((N + L - 1) / L);  // workgroups with at least one row
    double *part = static_cast<double *>(work);
    hipLaunchKernelGGL(ce_reduce_kernel, dim3((unsigned)P), dim3(CE_THREADS), 0, stream, nll, rank, N, L, V, part);
    OT_LAUNCH_CHECK("lm_token_ce_reduce");
    hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(64), 0, stream, part, P, sums);
    OT_LAUNCH_CHECK("lm_token_ce_final");
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int64_t omnitok_lm_token_ce_workspace(int64_t N) {
    if (N < 1 || N > ((int64_t)1 << 31)) return -1;
    return (int64_t)CE_MAX_GRID * 4 * (int64_t)sizeof(double);  // one partial quadruple per workgroup of the reduction
}

extern "C" int omnitok_lm_token_ce(const float *logits, int64_t ld, const int64_t *targets, int64_t N, int V, float *nll,
                                   int32_t *rank, double *sums, void *work, int64_t work_bytes, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // every argument is checked before the first launch
    OT_CHECK_ARG(sums && work, "lm_token_ce: null pointer (sums / work)");
    OT_CHECK_ARG(omnitok_lm_token_ce_workspace(N) >= 0 && work_bytes >= omnitok_lm_token_ce_workspace(N),
                 "lm_token_ce: N %lld rows, workspace of %lld bytes (omnitok_lm_token_ce_workspace)", (long long)N,
                 (long long)work_bytes);
    if (int rc = lm_token_ce_rows(logits, ld, targets, N, V, nll, rank, stream)) return rc;
    return lm_token_ce_reduce(nll, rank, N, V, sums, work, work_bytes, stream);
}
