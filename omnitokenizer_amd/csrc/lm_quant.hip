// LM decode: the fp8 (e4m3fn) quantiser of omnitok_lm_set_decode_quant and its export omnitok_lm_quantize_fp8 (index: lm_common.h)
#include "lm_common.h"

namespace omnitok {

// One workgroup per row.  Pass 1: the row's amax as the unsigned maximum of the fp32 patterns without their sign -- for finite
// values that order is the order of |w|, and a NaN or an infinity (pattern >= 0x7F800000) wins it, so the same maximum says whether
// the row is finite.  The exponent e of the scale comes from that pattern by integer arithmetic (lm_fp8_scale_exp, lm_common.h).
// Pass 2 reads the row again (L2), scales by 2^-e with
// v_ldexp_f32 (exact) and converts with v_cvt_pk_fp8_f32: one round to nearest even, subnormal results kept; no value exceeds 448, so
// the instruction's behaviour out of range never matters.
__global__ __launch_bounds__(256) void lm_quantize_fp8_kernel(const float *__restrict__ w, unsigned *__restrict__ q8,
                                                              float *__restrict__ scale, int K, int seg_rows,
                                                              int *__restrict__ flags) {
    __shared__ unsigned s_max[4];
    const int n = blockIdx.x, tid = threadIdx.x, k4n = K >> 2;
    const f32x4 *row = reinterpret_cast<const f32x4 *>(w + (int64_t)n * K);
    unsigned m = 0u;
    for (int i = tid; i < k4n; i += 256) {
        const f32x4 v = row[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float f = v[e];  // (a scalar copy: __builtin_bit_cast of a vector ELEMENT reads element 0 with this compiler)
            const unsigned a = __builtin_bit_cast(unsigned, f) & 0x7FFFFFFFu;
            m = a > m ? a : m;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, s);
        m = o > m ? o : m;
    }
    if ((tid & 63) == 0) s_max[tid >> 6] = m;
    __syncthreads();
    const unsigned a01 = s_max[0] > s_max[1] ? s_max[0] : s_max[1], a23 = s_max[2] > s_max[3] ? s_max[2] : s_max[3];
    const unsigned amax = a01 > a23 ? a01 : a23;
    const int e = lm_fp8_scale_exp(amax);  // (lm_common.h: shared with the K/V cache's append and scatter)
    if (tid == 0) {
        scale[n] = lm_fp8_scale(e);
        if (amax >= 0x7F800000u && flags) flags[n / seg_rows] = 1;
    }
    unsigned *out = q8 + (int64_t)n * k4n;
    for (int i = tid; i < k4n; i += 256) {
        const f32x4 v = row[i];
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(v[0], -e), __builtin_ldexpf(v[1], -e), 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(v[2], -e), __builtin_ldexpf(v[3], -e), p, true);
        out[i] = (unsigned)p;
    }
}

int lm_quantize_fp8(const float *w, void *q8, float *scale, int N, int K, int seg_rows, int *flags, hipStream_t stream) {
    hipLaunchKernelGGL(lm_quantize_fp8_kernel, dim3((unsigned)N), dim3(256), 0, stream, w, static_cast<unsigned *>(q8), scale, K, seg_rows,
                       flags);
    OT_LAUNCH_CHECK("lm_quantize_fp8");
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_lm_quantize_fp8(const float *w, void *q8, float *scale, int N, int K, int *flag, omnitok_stream_t stream_) {
    OT_CHECK_ARG(w && q8 && scale, "lm_quantize_fp8: null pointer");
    OT_CHECK_ARG(N > 0 && K > 0 && K % 4 == 0, "lm_quantize_fp8: bad sizes N=%d K=%d (K %% 4 == 0)", N, K);
    OT_CHECK_ARG(aligned16(w) && aligned16(q8), "lm_quantize_fp8: unaligned");
    return lm_quantize_fp8(w, q8, scale, N, K, N, flag, static_cast<hipStream_t>(stream_));
}
