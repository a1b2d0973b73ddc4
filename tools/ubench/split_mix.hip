// Micro-benchmark: issue cost of the fp32 -> f16 hi/lo split beside MFMAs, plain form against common.h's v_cvt_pk_f16_f32 + v_fma_mix*_f16
// form.  The register-operand MFMA loop of mfma_mix.hip (12 v_mfma_f32_32x32x16_f16 per iteration into 4 accumulators) with, per iteration,
// K splits of eight values whose hi / lo vectors ARE the MFMA operands (so nothing can be dropped or hoisted: the eight inputs pass through
// an empty asm statement before every split).  K = 0 is the bare loop; MFMA = false is the split alone (VALU issue rate).
// Prints clocks per iteration per wave and, from the difference to K = 0, clocks per split value.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../cardiac-segmentation-optical-flow_amd/csrc split_mix.hip -o split_mix
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include "common.h"
typedef float f32x16 __attribute__((ext_vector_type(16)));
using cf::f16x8;

template <bool NEW>
__device__ __forceinline__ void split8(const float (&v)[8], f16x8& hi, f16x8& lo) {
    if (NEW) {
        cf::split8_f16(v, hi, lo);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const _Float16 h = (_Float16)v[j];
            hi[j] = h;
            lo[j] = (_Float16)(v[j] - (float)h);
        }
    }
}

template <int K, bool NEW, bool MFMA>
__global__ void __launch_bounds__(256, 1) k(float* out, unsigned long long* ticks, int iters, const f16x8* __restrict__ gbuf, const float* __restrict__ xin) {
    f32x16 acc[4];
    for (int t = 0; t < 4; ++t) for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int lane = threadIdx.x & 63;
    f16x8 op[10];
    for (int i = 0; i < 10; ++i) op[i] = gbuf[i * 64 + lane];
    float x[8];
    for (int j = 0; j < 8; ++j) x[j] = xin[j * 256 + threadIdx.x];
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int g = 0; g < K; ++g) {
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(x[j]));
            split8<NEW>(x, op[2 * g], op[2 * g + 1]);
        }
        if (MFMA) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(op[1], op[2 + 2 * t], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(op[0], op[3 + 2 * t], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(op[0], op[2 + 2 * t], acc[t], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2 * K; ++i) asm volatile("" ::"v"(op[i]));
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    float s = 0;
    for (int t = 0; t < 4; ++t) for (int r = 0; r < 16; ++r) s += acc[t][r];
    for (int i = 0; i < 10; ++i) s += (float)op[i][0];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) ticks[0] = t1 - t0;
}

static double base_clk[2][3];   // [MFMA][waves per SIMD]: clocks per iteration of the K = 0 loop

template <int K, bool NEW, bool MFMA>
static void run(float* d, unsigned long long* dt, const f16x8* g, const float* x, hipEvent_t e0, hipEvent_t e1) {
    for (int wps = 1; wps <= 2; ++wps) {
        const int blocks = 256 * wps, iters = 40000 / wps;
        float ms = 0;
        for (int rep = 0; rep < 2; ++rep) {
            hipEventRecord(e0);
            hipLaunchKernelGGL((k<K, NEW, MFMA>), dim3(blocks), dim3(256), 0, 0, d, dt, iters, g, x);
            hipEventRecord(e1);
            if (hipEventSynchronize(e1) != hipSuccess) { printf("launch failed\n"); exit(1); }
            hipEventElapsedTime(&ms, e0, e1);
        }
        unsigned long long ticks = 0;
        hipMemcpy(&ticks, dt, 8, hipMemcpyDeviceToHost);
        const double clk = (double)ticks / iters;           // per iteration of one wave (wps waves share the SIMD)
        if (K == 0) base_clk[MFMA][wps] = clk;
        printf("%-5s %-4s K=%d (%2d values / iteration)  waves/SIMD %d: %8.2f ms  %8.1f clocks / iteration", MFMA ? "mfma" : "valu", K == 0 ? "-" : NEW ? "mix" : "plain", K,
               8 * K, wps, ms, clk);
        if (K) printf("  %+7.2f clocks / value over K=0", (clk - base_clk[MFMA][wps]) / (8 * K));
        printf("\n");
        fflush(stdout);
    }
}

int main() {
    float *d, *x;
    unsigned long long* dt;
    f16x8* g;
    hipMalloc(&d, 512 * 256 * 4);
    hipMalloc(&dt, 8);
    hipMalloc(&g, 640 * sizeof(f16x8));
    hipMalloc(&x, 8 * 256 * 4);
    _Float16* h = (_Float16*)malloc(640 * 16);
    float* hx = (float*)malloc(8 * 256 * 4);
    srand(1);
    for (int i = 0; i < 640 * 8; ++i) h[i] = (_Float16)(((rand() % 2001) - 1000) * 1e-3f);
    for (int i = 0; i < 8 * 256; ++i) hx[i] = ((rand() % 200001) - 100000) * 1e-5f;
    hipMemcpy(g, h, 640 * 16, hipMemcpyHostToDevice);
    hipMemcpy(x, hx, 8 * 256 * 4, hipMemcpyHostToDevice);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    run<0, false, true>(d, dt, g, x, e0, e1);
    run<1, false, true>(d, dt, g, x, e0, e1);
    run<1, true, true>(d, dt, g, x, e0, e1);
    run<2, false, true>(d, dt, g, x, e0, e1);
    run<2, true, true>(d, dt, g, x, e0, e1);
    run<4, false, true>(d, dt, g, x, e0, e1);
    run<4, true, true>(d, dt, g, x, e0, e1);
    run<0, false, false>(d, dt, g, x, e0, e1);
    run<4, false, false>(d, dt, g, x, e0, e1);
    run<4, true, false>(d, dt, g, x, e0, e1);
    return 0;
}
