// The stem DoubleConv of the flow encoders (nnunet/lib/utils.py:1182-1215 with a 1x1 `downsample`; query_encoder 1 -> 64, memory_encoder
// 6 -> 64): conv1 (3x3 pad 1) and downsample[0] (1x1) read the same few-channel input, so ONE launch stages the thread's input
// neighbourhood once and writes both raw maps with the GroupNorm statistics of each.  Same thread layout as conv_small_cin_kernel
// (conv_direct.hip): a thread owns one output column of PY rows, its (PY + 2) x 3 x CIN neighbourhood sits in registers (the 1x1 branch
// reads its centre column), the weights of the current output channel are wave-uniform scalar loads, every store is a 256-byte row segment
// per wave, statistics go registers -> shuffles -> LDS (a slot per wave, summed in wave order) -> ONE fp64 atomic pair per (group, map) and block.  Exact fp32; the 3x3 sum of an
// output is formed in conv_small_cin_kernel's order (bias, then ci / ky / kx), the 1x1 sum likewise (bias, then ci), so each map is
// bit-equal to that kernel's.  Roofline: the two Cout-channel writes (algorithmic bytes = 4 * B * H * W * (Cin + 2 * Cout)).  Measured at
// 256 x 256 -> 2 x 64 (profiles/flow_stem_head_bench.md): CIN = 1 moves its 2.16 GB (B = 64) at 5.1-6.4 TB/s, 0.34-0.42 ms against 0.41 ms for
// the two launches it replaces, and nothing at B = 128 (0.84 ms either way: both forms already write at the rate the box takes); CIN = 6 is
// not write-bound but on the side of its 60 FMAs per output pair (3.3-3.6 TB/s, 0.64 / 1.25 ms at B = 64 / 128 against 0.63 / 1.29 ms for the MFMA 3x3 + direct 1x1).
// Two rows of a channel per v_pk_fma_f32 (weights broadcast by op_sel) gave bit-equal maps and no time (0.72 ms at B = 64): not kept.
#include "common.h"
#include "conv.h"
#include "profile.h"

namespace cf {

// STORE_R false (cf_stem_block_y): r is formed and summed into ws_r as before but never written -- its one consumer, the block's final
// apply pass, recomputes it from x (cf_group_norm_apply_res_stem, norm.hip), so the launch writes one Cout-channel map instead of two.
template <int CIN, int PY, bool STORE_R>
__global__ void __launch_bounds__(256) stem_block_kernel(const float* __restrict__ x, const float* __restrict__ w3, const float* __restrict__ b3,
                                                         const float* __restrict__ w1, const float* __restrict__ b1, float* __restrict__ y,
                                                         float* __restrict__ r, int H, int W, int Cout, int groups,
                                                         double* __restrict__ ws_y, double* __restrict__ ws_r) {
    constexpr int NR = PY + 2;
    __shared__ float red[2][4][64 * 2];       // [map][wave][group (<= 64)]: sum, sum of squares of each wave
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64 + tx, y0 = (blockIdx.y * 4 + ty) * PY, b = blockIdx.z;
    const long HW = (long)H * W;
    const float* xb = x + (long)b * CIN * HW;
    float* yb = y + (long)b * Cout * HW;
    float* rb = STORE_R ? r + (long)b * Cout * HW : nullptr;
    float in[CIN][NR][3];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
        for (int rr = 0; rr < NR; ++rr)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int yy = y0 + rr - 1, xx = x0 + c - 1;
                in[ci][rr][c] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? xb[ci * HW + (long)yy * W + xx] : 0.f;
            }
    bool ok[PY];
#pragma unroll
    for (int rr = 0; rr < PY; ++rr) ok[rr] = x0 < W && y0 + rr < H;
    const int cpg = Cout / groups;
    for (int g = 0; g < groups; ++g) {
        float ys = 0.f, yq = 0.f, rs = 0.f, rq = 0.f;
        for (int c = 0; c < cpg; ++c) {
            const int co = g * cpg + c;
            const float* w3c = w3 + (long)co * CIN * 9;         // wave-uniform: scalar loads
            const float* w1c = w1 + (long)co * CIN;
            const float bv3 = b3 ? b3[co] : 0.f, bv1 = b1 ? b1[co] : 0.f;
            float wr[CIN * 9], wp[CIN];
#pragma unroll
            for (int k = 0; k < CIN * 9; ++k) wr[k] = w3c[k];
#pragma unroll
            for (int k = 0; k < CIN; ++k) wp[k] = w1c[k];
#pragma unroll
            for (int rr = 0; rr < PY; ++rr) {
                float acc = bv3, pacc = bv1;
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) acc = fmaf(wr[(ci * 3 + ky) * 3 + kx], in[ci][rr + ky][kx], acc);
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci) pacc = fmaf(wp[ci], in[ci][rr + 1][1], pacc);
                if (ok[rr]) {
                    const long o = (long)co * HW + (long)(y0 + rr) * W + x0;
                    yb[o] = acc;
                    if (STORE_R) rb[o] = pacc;
                    ys += acc;
                    yq += acc * acc;
                    rs += pacc;
                    rq += pacc * pacc;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            ys += __shfl_xor(ys, o, 64);
            yq += __shfl_xor(yq, o, 64);
            rs += __shfl_xor(rs, o, 64);
            rq += __shfl_xor(rq, o, 64);
        }
        if (tx == 0) {
            red[0][ty][2 * g] = ys;
            red[0][ty][2 * g + 1] = yq;
            red[1][ty][2 * g] = rs;
            red[1][ty][2 * g + 1] = rq;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 4 * groups; k += 256) {
        const int m = k >= 2 * groups, j = k - m * 2 * groups;
        // the four waves' sums in wave order, whichever finished first: a block's contribution is the same bits in every run and in both
        // forms of the kernel, so two runs differ by the order of the fp64 atomics alone
        atomicAdd(&(m ? ws_r : ws_y)[2L * b * groups + j], (double)(((red[m][0][j] + red[m][1][j]) + red[m][2][j]) + red[m][3][j]));
    }
}

template <int CIN, int PY, bool STORE_R>
static void launch_stem_block(const float* x, const float* w3, const float* b3, const float* w1, const float* b1, float* y, float* r, int B, int H,
                              int W, int Cout, int groups, double* ws_y, double* ws_r, hipStream_t s) {
    dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 4 * PY - 1) / (4 * PY)), (unsigned)B);
    hipLaunchKernelGGL((stem_block_kernel<CIN, PY, STORE_R>), grid, dim3(256), 0, s, x, w3, b3, w1, b1, y, r, H, W, Cout, groups, ws_y, ws_r);
}

}  // namespace cf

using namespace cf;

extern "C" int cf_stem_block_ok(int B, int Cin, int H, int W, int Cout, int gn_groups) {
    return (Cin == 1 || Cin == 6) && B > 0 && B < 65536 && H > 0 && W > 0 && (H + 7) / 8 < 65536 && Cout > 0 && gn_groups > 0 && gn_groups <= 64 &&
                   Cout % gn_groups == 0 && (double)Cout * H * W < 2147483648.0
               ? 1 : 0;
}

static int stem_block_call(const char* who, const float* x, const float* w3, const float* b3, const float* w1, const float* b1, float* y, float* r, int B,
                           int Cin, int H, int W, int Cout, double* ws_y, double* ws_r, int gn_groups, void* stream) {
    const int groups = gn_groups < 0 ? -gn_groups : gn_groups;      // negative: the caller's workspaces are already zero
    if (cf_stem_block_ok(B, Cin, H, W, Cout, groups) != 1) {
        char msg[384];
        snprintf(msg, sizeof(msg),
                 "%s: built for Cin 1 or 6, <= 64 statistics groups dividing Cout, one output sample below 2^31 elements: B=%d Cin=%d H=%d W=%d Cout=%d groups=%d",
                 who, B, Cin, H, W, Cout, groups);
        set_error(msg);
        return CF_ERR_ARG;
    }
    hipStream_t s = as_stream(stream);
    if (gn_groups > 0 && (hipMemsetAsync(ws_y, 0, 2L * B * groups * sizeof(double), s) != hipSuccess ||
                          hipMemsetAsync(ws_r, 0, 2L * B * groups * sizeof(double), s) != hipSuccess)) {
        set_error(std::string(who) + ": memset failed");
        return CF_ERR_LAUNCH;
    }
    if (r) {
        if (Cin == 1) launch_stem_block<1, 8, true>(x, w3, b3, w1, b1, y, r, B, H, W, Cout, groups, ws_y, ws_r, s);
        else launch_stem_block<6, 4, true>(x, w3, b3, w1, b1, y, r, B, H, W, Cout, groups, ws_y, ws_r, s);
    } else {
        if (Cin == 1) launch_stem_block<1, 8, false>(x, w3, b3, w1, b1, y, nullptr, B, H, W, Cout, groups, ws_y, ws_r, s);
        else launch_stem_block<6, 4, false>(x, w3, b3, w1, b1, y, nullptr, B, H, W, Cout, groups, ws_y, ws_r, s);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string(who) + ": launch failed: " + hipGetErrorString(e));
        return CF_ERR_LAUNCH;
    }
    return CF_OK;
}

extern "C" int cf_stem_block(const float* x, const float* w3, const float* b3, const float* w1, const float* b1, float* y, float* r, int B, int Cin,
                             int H, int W, int Cout, double* ws_y, double* ws_r, int gn_groups, void* stream) {
    CF_REQUIRE(x && w3 && w1 && y && r && ws_y && ws_r, "null pointer");
    CF_REQUIRE(x != y && x != r && y != r && ws_y != ws_r, "aliased pointers");
    return stem_block_call("cf_stem_block", x, w3, b3, w1, b1, y, r, B, Cin, H, W, Cout, ws_y, ws_r, gn_groups, stream);
}

extern "C" int cf_stem_block_y(const float* x, const float* w3, const float* b3, const float* w1, const float* b1, float* y, int B, int Cin, int H,
                               int W, int Cout, double* ws_y, double* ws_r, int gn_groups, void* stream) {
    CF_REQUIRE(x && w3 && w1 && y && ws_y && ws_r, "null pointer");
    CF_REQUIRE(x != y && ws_y != ws_r, "aliased pointers");
    return stem_block_call("cf_stem_block_y", x, w3, b3, w1, b1, y, nullptr, B, Cin, H, W, Cout, ws_y, ws_r, gn_groups, stream);
}
