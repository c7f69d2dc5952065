// Latte denoiser: the two small operators it adds to the DiT's (index: latte_common.h).
#include "latte_common.h"

#include <cmath>

namespace omnitok {

// ---- x[(b F + f) N + n, :] += temp_embed[f, :] ------------------------------------------------------------------------------------------
// Its own pass after block 0's MLP residual (latte.py:358-363): the sum is rounded where the reference rounds it.
__global__ void latte_add_temp_embed_kernel(float *__restrict__ x, const float *__restrict__ temp, int64_t total4, int F, int N, int D) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total4) return;
    const int n4 = D / 4;
    const int64_t r = id / n4;
    const int i = (int)(id - r * n4), f = (int)((r / N) % F);
    const f32x4 tv = reinterpret_cast<const f32x4 *>(temp + (int64_t)f * D)[i];
    f32x4 xv = reinterpret_cast<f32x4 *>(x)[id];
#pragma unroll
    for (int e = 0; e < 4; ++e) xv[e] += tv[e];
    reinterpret_cast<f32x4 *>(x)[id] = xv;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_latte_add_temp_embed(float *x, const float *temp_embed, int B, int F, int N, int D, omnitok_stream_t stream) {
    OT_CHECK_ARG(x && temp_embed, "latte_add_temp_embed: null pointer");
    OT_CHECK_ARG(B >= 1 && F >= 1 && N >= 1 && D >= 4 && D % 4 == 0, "latte_add_temp_embed: B %d, F %d, N %d, D %d (%% 4 == 0)", B, F, N, D);
    OT_CHECK_ARG(aligned16(x) && aligned16(temp_embed), "latte_add_temp_embed: unaligned pointer (16 bytes)");
    const int64_t total4 = (int64_t)B * F * N * (D / 4);
    OT_CHECK_ARG(total4 / 256 < (1ll << 31) - 1, "latte_add_temp_embed: too many elements (%lld)", (long long)total4 * 4);
    hipLaunchKernelGGL(latte_add_temp_embed_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       temp_embed, total4, F, N, D);
    OT_LAUNCH_CHECK("latte_add_temp_embed");
    return OMNITOK_OK;
}

extern "C" int omnitok_latte_cfg_blend(float *out, int images, int Cout, int channels, int64_t HW, float scale, omnitok_stream_t stream) {
    OT_CHECK_ARG(out, "latte_cfg_blend: null pointer");
    OT_CHECK_ARG(images >= 2 && images % 2 == 0 && Cout >= 1 && channels >= 1 && HW >= 1,
                 "latte_cfg_blend: images %d (even), Cout %d, channels %d, HW %lld", images, Cout, channels, (long long)HW);
    OT_CHECK_ARG(std::isfinite(scale), "latte_cfg_blend: scale is not finite");
    OT_CHECK_ARG((int64_t)(images / 2) * Cout * HW / 256 < (1ll << 31) - 1, "latte_cfg_blend: too many elements");
    return dit_cfg_blend(out, images, Cout, channels, HW, scale, static_cast<hipStream_t>(stream));
}
