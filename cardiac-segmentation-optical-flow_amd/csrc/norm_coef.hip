// Normalisations whose [B][3][C] table {mean, scale, shift} does not come from statistics of the map, and the apply pass that takes a table
// and the activation's slope as data -- the pieces nnU-Net's trainer variants (BatchNorm in eval mode, no normalisation, LeakyReLU(0.2),
// Mish) add to the norms of norm.hip.  Both are bandwidth kernels: one read and one write of the map, coefficients wave-uniform.
#include "common.h"

namespace cf {

// BatchNorm in eval mode: y = (x - running_mean) * gamma / sqrt(running_var + eps) + beta, the same for every sample; written once per
// sample so that the table has cf_group_norm_coef's layout and every consumer of one takes the other.  The quotient is formed in fp64
// and rounded once.
__global__ void __launch_bounds__(256) bn_coef_kernel(const float* __restrict__ rmean, const float* __restrict__ rvar, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, int B, int C, float* __restrict__ coef) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    float* o = coef + (long)b * 3 * C + c;
    o[0] = rmean[c];
    o[C] = (float)((gamma ? (double)gamma[c] : 1.0) / sqrt((double)rvar[c] + (double)eps));
    o[2 * C] = beta ? beta[c] : 0.f;
}

// x * tanh(softplus(x)) with e = exp(x): tanh(log(1 + e)) = ((1 + e)^2 - 1) / ((1 + e)^2 + 1) = n / (n + 2), n = e (e + 2): no
// cancellation on either side (n -> 0 for x -> -inf, and the quotient is 1 in fp32 long before e overflows: from x = 20 on, softplus's
// own threshold in torch, the value is x itself).
__device__ __forceinline__ float mish_f(float v) {
    if (v > 20.f) return v;
    const float e = expf(v);
    const float n = e * (e + 2.f);
    return v * (n / (n + 2.f));
}

__device__ __forceinline__ float coef_act(float v, int act, float slope) {
    if (act == CF_ACT_LRELU) return v > 0.f ? v : v * slope;
    if (act == CF_ACT_MISH) return mish_f(v);
    return act_apply(v, act);
}

// out = act((x - mean) * scale + shift) over the B * C rows of HW values.  The unit of work is (row, chunk of 256 W-wide accesses) and
// belongs to one wave; units are grid-strided.  W = 4: a row starts at any 4-byte address (HW odd, a view), so every row has a scalar
// head up to its first 16-byte boundary, a float4 body and a scalar tail; head and tail ride with the row's first chunk.  x and out
// share the row offset, so they share the head whenever the two base addresses agree modulo 16 -- the host picks W = 1 otherwise.
template <int W>
__global__ void __launch_bounds__(256) coef_apply_kernel(const float* __restrict__ x, const float* __restrict__ coef, float* __restrict__ out,
                                                         long rows, int C, int HW, int cpr, int act, float slope) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const long units = rows * cpr;
    for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (long)gridDim.x * 4) {
        const long row = u / cpr;
        const int ch = (int)(u - row * cpr);
        float m = 0.f, sc = 1.f, sh = 0.f;
        if (coef) {
            const long b = row / C;
            const float* t = coef + b * 3 * C + (row - b * C);
            m = t[0]; sc = t[C]; sh = t[2 * C];
        }
        const float* xr = x + row * HW;
        float* orow = out + row * HW;
        if constexpr (W == 4) {
            int head = (int)((4 - ((reinterpret_cast<uintptr_t>(xr) >> 2) & 3)) & 3);
            if (head > HW) head = HW;
            const int nv = (HW - head) >> 2, tail0 = head + 4 * nv;
            if (ch == 0) {
                if (lane < head) orow[lane] = coef_act((xr[lane] - m) * sc + sh, act, slope);
                if (tail0 + lane < HW) orow[tail0 + lane] = coef_act((xr[tail0 + lane] - m) * sc + sh, act, slope);
            }
            const int v1 = min(nv, (ch + 1) * 256);
            for (int v = ch * 256 + lane; v < v1; v += 64) {
                f32x4 q = *reinterpret_cast<const f32x4*>(xr + head + 4 * v);
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = coef_act((q[j] - m) * sc + sh, act, slope);
                *reinterpret_cast<f32x4*>(orow + head + 4 * v) = q;
            }
        } else {
            const int e1 = min(HW, (ch + 1) * 256);
            for (int e = ch * 256 + lane; e < e1; e += 64) orow[e] = coef_act((xr[e] - m) * sc + sh, act, slope);
        }
    }
}

}  // namespace cf

using namespace cf;

extern "C" int cf_batch_norm_coef(const float* running_mean, const float* running_var, const float* gamma, const float* beta, float eps, int B,
                                  int C, float* coef, void* stream) {
    CF_REQUIRE(running_mean && running_var && coef, "null pointer");
    CF_REQUIRE(B > 0 && C > 0 && (long)B * C < (1L << 31), "bad shape B=%d C=%d", B, C);
    CF_REQUIRE(eps >= 0.f, "eps %g < 0", (double)eps);
    hipLaunchKernelGGL(bn_coef_kernel, dim3((unsigned)(((long)B * C + 255) / 256)), dim3(256), 0, as_stream(stream), running_mean, running_var, gamma,
                       beta, eps, B, C, coef);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

// host code, no launch: 1 when cf_coef_apply's index arithmetic holds the shape (HW and the chunk count of a row in an int; rows, units
// and element offsets in a long with room for the grid stride), else 0
extern "C" int cf_coef_apply_ok(int B, int C, long HW) {
    if (B <= 0 || C <= 0 || HW <= 0 || HW > (1L << 30)) return 0;
    const long rows = (long)B * C;
    return rows <= (1L << 40) / HW ? 1 : 0;          // B * C * HW <= 2^40 elements: units <= elements, far inside a long
}

extern "C" int cf_coef_apply(const float* x, const float* coef, int act, float slope, float* out, int B, int C, int HW, void* stream) {
    CF_REQUIRE(x && out, "null pointer");
    CF_REQUIRE(cf_coef_apply_ok(B, C, HW) == 1, "bad shape B=%d C=%d HW=%d", B, C, HW);
    CF_REQUIRE(act >= CF_ACT_NONE && act <= CF_ACT_MISH, "bad activation %d", act);
    CF_REQUIRE(act != CF_ACT_LRELU || slope >= 0.f, "LeakyReLU slope %g < 0", (double)slope);
    CF_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 3) == 0, "x and out must be 4-byte aligned");
    const bool vec = ((reinterpret_cast<uintptr_t>(x) ^ reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const long rows = (long)B * C;
    const int per = vec ? 4 : 1;
    int cpr = (int)(((long)HW / per + 255) / 256);
    if (cpr < 1) cpr = 1;
    const long units = rows * cpr;
    long blocks = (units + 3) / 4;
    const long cap = (long)device_cu_count() * 16;
    if (blocks > cap) blocks = cap;
    hipStream_t s = as_stream(stream);
    if (vec) hipLaunchKernelGGL(coef_apply_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, x, coef, out, rows, C, HW, cpr, act, slope);
    else hipLaunchKernelGGL(coef_apply_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, x, coef, out, rows, C, HW, cpr, act, slope);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
