// Training-only passes around the convolutions: InstanceNorm + LeakyReLU backward, the deep-supervision DC + CE loss, gradient clipping
// and Nesterov SGD.  Every cross-workgroup sum is a second launch that adds partials in a fixed order (fp64); no atomics, no waiting.
// Built with -ffp-contract=off: the optimizer's element chain is torch's, rounding by rounding (its fused multiply-adds are written out).
#include "common.h"

namespace cf {

// fixed-order block sum of NV doubles per thread: wave shuffles, then wave 0 adds the four wave results in wave order
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* sm /* [4][NV] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double s = v[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
        if (lane == 0) sm[wave * NV + i] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = sm[i] + sm[NV + i] + sm[2 * NV + i] + sm[3 * NV + i];
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------- InstanceNorm + LeakyReLU backward
__device__ __forceinline__ void plane_coef(const double* ws, long plane, int HW, float eps, float* mean, float* rstd) {
    const double invL = 1.0 / (double)HW;
    const double m = ws[2 * plane] * invL;
    double var = ws[2 * plane + 1] * invL - m * m;
    if (var < 0.0) var = 0.0;
    *mean = (float)m;                                   // the forward apply pass's own two numbers
    *rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// one block per plane: bws[plane] = {sum dz, sum dz * xhat}, dz = dy * (z > 0 ? 1 : slope), z = gamma * xhat + beta
__global__ void __launch_bounds__(256) norm_act_bwd_stats_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 const double* __restrict__ ws, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, double* __restrict__ bws, int C, int HW,
                                                                 float eps, float slope) {
    __shared__ double sm[8];
    const long plane = blockIdx.x;
    const int c = (int)(plane % C);
    float mean, rstd;
    plane_coef(ws, plane, HW, eps, &mean, &rstd);
    const float g = gamma[c], bb = beta[c];
    const float* xp = x + plane * HW;
    const float* dp = dy + plane * HW;
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < HW; i += 256) {
        const float xh = (xp[i] - mean) * rstd;
        const float z = xh * g + bb;
        const float dz = z > 0.f ? dp[i] : dp[i] * slope;
        v[0] += (double)dz;
        v[1] += (double)dz * (double)xh;
    }
    block_sum<2>(v, sm);
    if (threadIdx.x == 0) {
        bws[2 * plane] = v[0];
        bws[2 * plane + 1] = v[1];
    }
}

// dx = gamma * rstd * (dz - mean(dz) - xhat * mean(dz * xhat)); block 0 of every b = 0 plane also adds the planes' sums over the batch, in
// batch order, into dgamma / dbeta
__global__ void __launch_bounds__(256) norm_act_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 const double* __restrict__ ws, const double* __restrict__ bws,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float* __restrict__ dx, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, int B, int C, int HW, float eps, float slope,
                                                                 int segs) {
    const long plane = blockIdx.x / segs;
    const int seg = blockIdx.x % segs;
    const int c = (int)(plane % C);
    float mean, rstd;
    plane_coef(ws, plane, HW, eps, &mean, &rstd);
    const float g = gamma[c], bb = beta[c];
    const float m1 = (float)(bws[2 * plane] / (double)HW), m2 = (float)(bws[2 * plane + 1] / (double)HW);
    const float gr = g * rstd;
    const float* xp = x + plane * HW;
    const float* dp = dy + plane * HW;
    float* op = dx + plane * HW;
    for (int i = seg * 256 + threadIdx.x; i < HW; i += segs * 256) {
        const float xh = (xp[i] - mean) * rstd;
        const float z = xh * g + bb;
        const float dz = z > 0.f ? dp[i] : dp[i] * slope;
        op[i] = gr * ((dz - m1) - xh * m2);
    }
    if (plane < C && seg == 0 && threadIdx.x == 0) {
        double s1 = 0.0, s2 = 0.0;
        for (int b = 0; b < B; ++b) {
            s1 += bws[2 * ((long)b * C + c)];
            s2 += bws[2 * ((long)b * C + c) + 1];
        }
        dbeta[c] = (float)s1;
        dgamma[c] = (float)s2;
    }
}

// ---------------------------------------------------------------------------------------------- DC + CE loss
constexpr int LOSS_MAXK = 16;

template <int K>
__device__ __forceinline__ float softmax_k(const float* lp, long cstride, float (&pr)[K]) {
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        pr[k] = lp[k * cstride];
        mx = fmaxf(mx, pr[k]);
    }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        pr[k] = expf(pr[k] - mx);
        den += pr[k];
    }
    const float inv = 1.0f / den;
#pragma unroll
    for (int k = 0; k < K; ++k) pr[k] *= inv;
    return logf(den) + mx;   // log-sum-exp
}

// part[block][1 + 3K] = {sum of -log p[y], then per class sum p * y, sum p, sum y} over the block's pixels
template <int K>
__global__ void __launch_bounds__(256) loss_reduce_kernel(const float* __restrict__ logits, const int* __restrict__ target,
                                                          double* __restrict__ part, long N, int HW) {
    __shared__ double sm[4 * (1 + 3 * K)];
    double v[1 + 3 * K];
#pragma unroll
    for (int i = 0; i < 1 + 3 * K; ++i) v[i] = 0.0;
    for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long)gridDim.x * 256) {
        const long b = n / HW;
        const float* lp = logits + (b * K) * HW + (n - b * HW);
        float pr[K];
        const float lse = softmax_k<K>(lp, HW, pr);
        const int y = target[n];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k == y) {
                v[0] += (double)(lse - lp[(long)k * HW]);
                v[1 + 3 * k] += (double)pr[k];
                v[3 + 3 * k] += 1.0;
            }
            v[2 + 3 * k] += (double)pr[k];
        }
    }
    block_sum<1 + 3 * K>(v, sm);
    if (threadIdx.x == 0)
        for (int i = 0; i < 1 + 3 * K; ++i) part[(long)blockIdx.x * (1 + 3 * K) + i] = v[i];
}

// one block: partials added in block order; coef[2k] = a_k, coef[2k+1] = b_k with d(dice term)/dp_k = a_k * y_k + b_k; *loss += weight * l
__global__ void __launch_bounds__(64) loss_final_kernel(const double* __restrict__ part, int nblocks, int K, long N, float smooth,
                                                        float weight, float* __restrict__ coef, float* __restrict__ loss,
                                                        float* __restrict__ loss_out) {
    __shared__ double tot[1 + 3 * LOSS_MAXK];
    const int nv = 1 + 3 * K;
    if ((int)threadIdx.x < nv) {
        double s = 0.0;
        for (int b = 0; b < nblocks; ++b) s += part[(long)b * nv + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double dcsum = 0.0;
        coef[0] = 0.f;
        coef[1] = 0.f;   // do_bg = False
        for (int k = 1; k < K; ++k) {
            const double tp = tot[1 + 3 * k], sp = tot[2 + 3 * k], sy = tot[3 + 3 * k];
            const double nom = 2.0 * tp + (double)smooth, den = sp + sy + (double)smooth + 1e-8;   // 2tp + fp + fn = sum p + sum y
            dcsum += nom / den;
            coef[2 * k] = (float)(-2.0 / ((K - 1) * den));
            coef[2 * k + 1] = (float)(nom / ((K - 1) * den * den));
        }
        const double l = tot[0] / (double)N + 1.0 - dcsum / (K - 1);
        if (loss_out) *loss_out = (float)l;
        *loss += weight * (float)l;
    }
}

template <int K>
__global__ void __launch_bounds__(256) loss_grad_kernel(const float* __restrict__ logits, const int* __restrict__ target,
                                                        const float* __restrict__ coef, float* __restrict__ dlogits, long N, int HW,
                                                        float weight) {
    float ca[K], cb[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        ca[k] = coef[2 * k];
        cb[k] = coef[2 * k + 1];
    }
    const float invN = 1.0f / (float)N;
    for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long)gridDim.x * 256) {
        const long b = n / HW;
        const long off = (b * K) * HW + (n - b * HW);
        float pr[K], gk[K];
        softmax_k<K>(logits + off, HW, pr);
        const int y = target[n];
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            gk[k] = (k == y ? ca[k] : 0.f) + cb[k];
            dot += gk[k] * pr[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float ce = (pr[k] - (k == y ? 1.f : 0.f)) * invN;
            dlogits[off + (long)k * HW] = weight * (pr[k] * (gk[k] - dot) + ce);
        }
    }
}

template <int K>
static void loss_launch(const float* logits, const int* target, double* part, float* coef, float* dlogits, float* loss, float* loss_out, long N,
                        int HW, int nblocks, float smooth, float weight, hipStream_t s) {
    hipLaunchKernelGGL(loss_reduce_kernel<K>, dim3(nblocks), dim3(256), 0, s, logits, target, part, N, HW);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, s, part, nblocks, K, N, smooth, weight, coef, loss, loss_out);
    if (dlogits) hipLaunchKernelGGL(loss_grad_kernel<K>, dim3(flat_grid(N, 256)), dim3(256), 0, s, logits, target, coef, dlogits, N, HW, weight);
}

static int loss_blocks(long N) {
    long nb = (N + 256 * 8 - 1) / (256 * 8);
    return (int)(nb < 1 ? 1 : nb > 512 ? 512 : nb);
}

// ---------------------------------------------------------------------------------------------- clipping and Nesterov SGD
// table[t] = {offset, size, has_grad} (int64) of tensor t in the flat arenas

// one block per tensor: tnorm[t] = its 2-norm (fp64 sum, rounded to fp32 as torch's per-tensor norm is)
__global__ void __launch_bounds__(256) grad_norm_tensor_kernel(const float* __restrict__ grad, const long* __restrict__ table,
                                                               float* __restrict__ tnorm) {
    __shared__ double sm[4];
    const long off = table[3 * blockIdx.x], n = table[3 * blockIdx.x + 1];
    double v[1] = {0.0};
    if (table[3 * blockIdx.x + 2])
        for (long i = threadIdx.x; i < n; i += 256) {
            const double g = (double)grad[off + i];
            v[0] += g * g;
        }
    block_sum<1>(v, sm);
    if (threadIdx.x == 0) tnorm[blockIdx.x] = (float)sqrt(v[0]);
}

// out[0] = total norm (the 2-norm of the tensors' norms, in table order), out[1] = min(1, max_norm / (total + 1e-6))
__global__ void grad_norm_final_kernel(const float* __restrict__ tnorm, const long* __restrict__ table, int T, float max_norm,
                                       float* __restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    double s = 0.0;
    for (int t = 0; t < T; ++t)
        if (table[3 * t + 2]) s += (double)tnorm[t] * (double)tnorm[t];
    const float total = (float)sqrt(s);
    const float c = (1.0f / (total + 1e-6f)) * max_norm;   // torch's max_norm / tensor is tensor.reciprocal() * max_norm: two roundings
    out[0] = total;
    out[1] = c < 1.0f ? c : 1.0f;
}

__global__ void __launch_bounds__(256) sgd_nesterov_kernel(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ mom,
                                                           const long* __restrict__ table, const float* __restrict__ clip, float lr, float wd,
                                                           float mu, int first) {
    const long off = table[3 * blockIdx.y], n = table[3 * blockIdx.y + 1];
    if (!table[3 * blockIdx.y + 2]) return;
    const float c = clip[1];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        // torch's chain, rounding by rounding: mul_(clip); add(p, alpha = wd), add(buf, alpha = mu) and add_(g, alpha = -lr) are one fused
        // multiply-add each (ATen's a + alpha * b), buf.mul_(mu).add_(g) is a rounded product and a rounded sum
        const float p = param[off + i];
        float g = grad[off + i] * c;
        g = fmaf(wd, p, g);
        const float b = first ? g : mu * mom[off + i] + g;
        mom[off + i] = b;
        g = fmaf(mu, b, g);
        param[off + i] = fmaf(-lr, g, p);
    }
}

}  // namespace cf

using namespace cf;

extern "C" int cf_norm_act_bwd(const float* x, const float* dy, const double* ws, const float* gamma, const float* beta, float* dx,
                               float* dgamma, float* dbeta, double* bws, int B, int C, int HW, float eps, float slope, void* stream) {
    CF_REQUIRE(x && dy && ws && gamma && beta && dx && dgamma && dbeta && bws, "null pointer");
    CF_REQUIRE(B > 0 && C > 0 && HW > 0 && (long)B * C < (1L << 24), "bad shape B=%d C=%d HW=%d", B, C, HW);
    hipStream_t s = as_stream(stream);
    const int planes = B * C;
    hipLaunchKernelGGL(norm_act_bwd_stats_kernel, dim3(planes), dim3(256), 0, s, x, dy, ws, gamma, beta, bws, C, HW, eps, slope);
    CF_CHECK_LAUNCH();
    int segs = (HW + 256 * 8 - 1) / (256 * 8);
    if (segs > 64) segs = 64;
    hipLaunchKernelGGL(norm_act_bwd_apply_kernel, dim3((unsigned)((long)planes * segs)), dim3(256), 0, s, x, dy, ws, bws, gamma, beta, dx,
                       dgamma, dbeta, B, C, HW, eps, slope, segs);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_dc_ce_loss_blocks(long N) {
    CF_REQUIRE(N > 0, "bad pixel count");
    return loss_blocks(N);
}

extern "C" int cf_dc_ce_loss(const float* logits, const int* target, float* dlogits, float* loss, float* loss_out, float* coef, double* part,
                             int B, int K, int HW, float smooth, float weight, void* stream) {
    CF_REQUIRE(logits && target && loss && coef && part, "null pointer");
    CF_REQUIRE(B > 0 && HW > 0 && K >= 2 && K <= LOSS_MAXK, "bad shape B=%d K=%d HW=%d (2 <= K <= %d)", B, K, HW, LOSS_MAXK);
    const long N = (long)B * HW;
    const int nb = loss_blocks(N);
    hipStream_t s = as_stream(stream);
#define CF_LOSS_CASE(KK) case KK: loss_launch<KK>(logits, target, part, coef, dlogits, loss, loss_out, N, HW, nb, smooth, weight, s); break;
    switch (K) {
        CF_LOSS_CASE(2) CF_LOSS_CASE(3) CF_LOSS_CASE(4) CF_LOSS_CASE(5) CF_LOSS_CASE(6) CF_LOSS_CASE(7) CF_LOSS_CASE(8) CF_LOSS_CASE(9)
        CF_LOSS_CASE(10) CF_LOSS_CASE(11) CF_LOSS_CASE(12) CF_LOSS_CASE(13) CF_LOSS_CASE(14) CF_LOSS_CASE(15) CF_LOSS_CASE(16)
    }
#undef CF_LOSS_CASE
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_grad_norm(const float* grad, const long* table, int T, float max_norm, float* tnorm, float* out, void* stream) {
    CF_REQUIRE(grad && table && tnorm && out, "null pointer");
    CF_REQUIRE(T > 0 && T < 65536, "bad tensor count %d", T);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(grad_norm_tensor_kernel, dim3(T), dim3(256), 0, s, grad, table, tnorm);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(64), 0, s, tnorm, table, T, max_norm, out);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_sgd_nesterov(float* param, const float* grad, float* mom, const long* table, int T, long max_size, const float* clip,
                               float lr, float wd, float mu, int first, void* stream) {
    CF_REQUIRE(param && grad && mom && table && clip, "null pointer");
    CF_REQUIRE(T > 0 && T < 65536 && max_size > 0, "bad tensor table T=%d max_size=%ld", T, max_size);
    long nb = (max_size + 256 * 4 - 1) / (256 * 4);
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(sgd_nesterov_kernel, dim3((unsigned)nb, (unsigned)T), dim3(256), 0, as_stream(stream), param, grad, mom, table, clip,
                       lr, wd, mu, first);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
