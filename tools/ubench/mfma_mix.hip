// Micro-benchmark: how much of the sustained f16 MFMA rate do operand fetches cost?  The MFMA loop of mfma_rate.hip (random operands,
// 12 MFMAs per iteration into 4 accumulators) with, per iteration, NL ds_read_b128 from a 32 KB LDS image and NG global_load_dwordx4 from
// an L2-resident 1 MB buffer feeding the operands (so that the loads cannot be dropped).  The convolution kernel's four-wave shape has
// NL = 8, NG = 2 per 12 MFMAs.  Reports TFLOP/s (dense f16) and the clock.
//
// Second part (`shape` rows): a loop over pairs of those k-steps (2 NL + 2 NG fetches, then 24 x v_mfma_f32_32x32x16_f16) against the same
// fetches followed by 48 x v_mfma_f32_16x16x32_f16 into the 16 blocks of the same four 32x32 tiles, K = 32 spanning the two k-steps of the
// pair: equal output tile, equal MACs and equal operand fetches per MAC, only the MFMA shape differs.  Random and zero operands, the two
// shapes alternating launch by launch; the in-kernel clock is d(s_memtime) / d(s_memrealtime) x 100 MHz, median over workgroups.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int NL, int NG>
__global__ void __launch_bounds__(256, 1) k(float* out, unsigned long long* ticks, int iters, const f16x8* __restrict__ gbuf) {
    __shared__ f16x8 lds[2048];   // 32 KB
    for (int i = threadIdx.x; i < 2048; i += 256) lds[i] = gbuf[i];
    __syncthreads();
    f32x16 acc[4];
    for (int t = 0; t < 4; ++t) for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f16x8 a0 = gbuf[lane], a1 = gbuf[64 + lane];
    f16x8 b[8];
    for (int i = 0; i < 8; ++i) b[i] = gbuf[128 + i * 64 + lane];
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; ++it) {
        const int base = (it * 131 + wave * 257) & 1023;
        if (NG >= 1) a0 = gbuf[((base * 64 + blockIdx.x * 64) & 65535) + lane];
        if (NG >= 2) a1 = gbuf[((base * 64 + 4096 + blockIdx.x * 64) & 65535) + lane];
#pragma unroll
        for (int i = 0; i < NL; ++i) b[i] = lds[((base + i * 64) & 1023) + lane + (i & 1) * 1024 - ((i & 1) ? 64 : 0)];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b[2 * t], acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b[2 * t + 1], acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b[2 * t], acc[t], 0, 0, 0);
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    float s = 0;
    for (int t = 0; t < 4; ++t) for (int r = 0; r < 16; ++r) s += acc[t][r];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) ticks[0] = t1 - t0;
}

template <int NL, int NG>
static void run(float* d, unsigned long long* dt, const f16x8* g, hipEvent_t e0, hipEvent_t e1) {
    for (int wps = 1; wps <= 3; ++wps) {
        const int blocks = 256 * wps, iters = 60000 / wps;
        float ms = 0;
        for (int rep = 0; rep < 2; ++rep) {
            hipEventRecord(e0);
            hipLaunchKernelGGL((k<NL, NG>), dim3(blocks), dim3(256), 0, 0, d, dt, iters, g);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1);
        }
        unsigned long long ticks = 0;
        hipMemcpy(&ticks, dt, 8, hipMemcpyDeviceToHost);
        const double mfma = (double)blocks * 4 * iters * 12;
        const double tf = mfma * 2.0 * 32 * 32 * 16 / (ms * 1e-3) * 1e-12;
        printf("ds_read_b128 %d + global dwordx4 %d per 12 MFMAs, waves/SIMD %d: %7.2f ms  %7.1f TFLOP/s  clock %.3f GHz  %.1f clocks per MFMA per SIMD\n", NL, NG, wps,
               ms, tf, (double)ticks / (ms * 1e6), (double)ticks / ((double)iters * 12 * wps));
        fflush(stdout);
    }
}

// In-place 16x16x32 accumulate.  Through the builtin this compiler gives each chain of the unrolled loop a shared scratch tuple and rotates the
// 16 accumulators through it (60 v_accvgpr_mov and 30 s_nop per iteration), which would be measured instead of the shape.  Callers keep
// dependent MFMAs at least four apart, as the builtin form of the 32x32x16 loop does.
static __device__ __forceinline__ void mfma16(f32x4& c, const f16x8& a, const f16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

// a[p][2], b[p][8]: the operands of k-step p of the pair.  SHAPE 32 runs k's twelve MFMAs on each k-step.  SHAPE 16 reads a[.][x] as the
// two row halves and b[.][2t], b[.][2t+1] as the column halves of K = 32 operands (which 16 bytes a lane holds is a matter of LDS addressing,
// not of rate) and gives each 16x16 block three MFMAs.
template <int SHAPE, int NL, int NG>
__global__ void __launch_bounds__(256, 1) kp(float* out, unsigned long long* stamps, int iters, const f16x8* __restrict__ gbuf, int zero) {
    __shared__ f16x8 lds[2048];   // 32 KB
    const f16x8* src = gbuf + (zero ? 65536 + 4096 : 0);
    for (int i = threadIdx.x; i < 2048; i += 256) lds[i] = src[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f16x8 a[2][2], b[2][8];
    for (int p = 0; p < 2; ++p) {
        a[p][0] = src[p * 1024 + lane], a[p][1] = src[p * 1024 + 64 + lane];
        for (int i = 0; i < 8; ++i) b[p][i] = src[p * 1024 + 128 + i * 64 + lane];
    }
    f32x16 acc32[SHAPE == 32 ? 4 : 1];
    f32x4 acc16[SHAPE == 16 ? 16 : 1];
    if (SHAPE == 32) { for (int t = 0; t < 4; ++t) for (int r = 0; r < 16; ++r) acc32[t][r] = 0.f; }
    else             { for (int t = 0; t < 16; ++t) for (int r = 0; r < 4; ++r) acc16[t][r] = 0.f; }
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int base = ((2 * it + p) * 131 + wave * 257) & 1023;
            if (NG >= 1) a[p][0] = src[((base * 64 + blockIdx.x * 64) & 65535) + lane];
            if (NG >= 2) a[p][1] = src[((base * 64 + 4096 + blockIdx.x * 64) & 65535) + lane];
#pragma unroll
            for (int i = 0; i < NL; ++i) b[p][i] = lds[((base + i * 64) & 1023) + lane + (i & 1) * 1024 - ((i & 1) ? 64 : 0)];
        }
        __builtin_amdgcn_sched_barrier(0);
        if (SHAPE == 32) {
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    acc32[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[p][1], b[p][2 * t], acc32[t], 0, 0, 0);
                    acc32[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[p][0], b[p][2 * t + 1], acc32[t], 0, 0, 0);
                    acc32[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[p][0], b[p][2 * t], acc32[t], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int q = 0; q < 3; ++q)   // the three products of k, each over the tile's four independent blocks
#pragma unroll
                    for (int ij = 0; ij < 4; ++ij) mfma16(acc16[t * 4 + ij], a[ij >> 1][q == 0], b[ij & 1][2 * t + (q == 1)]);
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (SHAPE == 16)   // the compiler sees no MFMA in mfma16 to pad after: one builtin MFMA per block stands between mfma16 and the reads below
        for (int n = 0; n < 16; ++n) acc16[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0][0], b[0][0], acc16[n], 0, 0, 0);
    float s = 0;
    if (SHAPE == 32) { for (int t = 0; t < 4; ++t) for (int r = 0; r < 16; ++r) s += acc32[t][r]; }
    else             { for (int t = 0; t < 16; ++t) for (int r = 0; r < 4; ++r) s += acc16[t][r]; }
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0) { stamps[2 * blockIdx.x] = t1 - t0; stamps[2 * blockIdx.x + 1] = r1 - r0; }
}

static int cmp_d(const void* x, const void* y) { const double a = *(const double*)x, b = *(const double*)y; return a < b ? -1 : a > b; }

// three back-to-back launches, the last one timed; cycles and clock are medians over the workgroups of that launch
template <int SHAPE, int NL, int NG>
static void shape_row(float* d, unsigned long long* dst, const f16x8* g, int wps, int zero, int round, hipEvent_t e0, hipEvent_t e1) {
    const int blocks = 256 * wps, iters = 120000 / wps;
    float ms = 0;
    for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL((kp<SHAPE, NL, NG>), dim3(blocks), dim3(256), 0, 0, d, dst, iters, g, zero);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
    }
    static unsigned long long st[2 * 768];
    static double tk[768], ck[768];
    hipMemcpy(st, dst, sizeof(unsigned long long) * 2 * blocks, hipMemcpyDeviceToHost);
    for (int i = 0; i < blocks; ++i) { tk[i] = (double)st[2 * i]; ck[i] = (double)st[2 * i] / (double)st[2 * i + 1] * 0.1; }
    qsort(tk, blocks, sizeof(double), cmp_d);
    qsort(ck, blocks, sizeof(double), cmp_d);
    const double mac = (double)blocks * 4 * iters * 24 * 32 * 32 * 16;
    printf("shape %s  ds_read_b128 %d + global dwordx4 %d per 12 32x32x16 equivalents  waves/SIMD %d  %s  round %d  %7.2f ms : %7.1f TFLOP/s  wave cycles %.4e (%.2f per equivalent per SIMD)  in-kernel clock %.3f GHz\n",
           SHAPE == 32 ? "32x32x16" : "16x16x32", NL, NG, wps, zero ? "zeros " : "random", round, ms, mac * 2.0 / (ms * 1e-3) * 1e-12, tk[blocks / 2],
           tk[blocks / 2] / ((double)iters * 24 * wps), ck[blocks / 2]);
    fflush(stdout);
}

template <int NL, int NG>
static void shape_rows(float* d, unsigned long long* dst, const f16x8* g, hipEvent_t e0, hipEvent_t e1) {
    for (int wps = 1; wps <= 3; ++wps)
        for (int zero = 0; zero < 2; ++zero)
            for (int round = 0; round < 3; ++round) {
                shape_row<32, NL, NG>(d, dst, g, wps, zero, round, e0, e1);
                shape_row<16, NL, NG>(d, dst, g, wps, zero, round, e0, e1);
            }
}

int main() {
    float* d;
    unsigned long long* dt;
    f16x8* g;
    hipMalloc(&d, 256 * 3 * 256 * 4);
    hipMalloc(&dt, 8);
    hipMalloc(&g, 2 * (65536 + 4096) * sizeof(f16x8));   // the random image, then a zero image of the same size
    hipMemset(g, 0, 2 * (65536 + 4096) * sizeof(f16x8));
    const size_t n = 65536 + 4096;
    _Float16* h = (_Float16*)malloc(n * 16);
    srand(1);
    for (size_t i = 0; i < n * 8; ++i) h[i] = (_Float16)(((rand() % 2001) - 1000) * 1e-3f);
    hipMemcpy(g, h, n * 16, hipMemcpyHostToDevice);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    run<0, 0>(d, dt, g, e0, e1);
    run<4, 0>(d, dt, g, e0, e1);
    run<8, 0>(d, dt, g, e0, e1);
    run<0, 2>(d, dt, g, e0, e1);
    run<4, 2>(d, dt, g, e0, e1);
    run<8, 2>(d, dt, g, e0, e1);
    unsigned long long* dst;
    hipMalloc(&dst, sizeof(unsigned long long) * 2 * 768);
    shape_rows<8, 0>(d, dst, g, e0, e1);   // every B operand re-read from LDS
    shape_rows<8, 2>(d, dst, g, e0, e1);   // the convolution's fetches
    return 0;
}
