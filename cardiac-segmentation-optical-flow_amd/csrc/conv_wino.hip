// 3x3 / stride 1 / pad 1 convolution as a ROW Winograd F(2,3) on the f16 MFMA with the 3-term hi/lo operand split of conv_f16s.hip.
//
// Why: the 128- and 256-channel layers run at the board's power limit with the matrix pipe busy (profiles/r03_power_probe.txt,
// r03_conv_sq_pmc.txt): what moves them is fewer matrix instructions per output, not a tighter schedule.  Along x, two output columns
// (2u, 2u + 1) of one row need the four input columns d0..d3 = x[2u - 1 .. 2u + 2]:
//
//     V = B^T d = (d0 - d2,  d1 + d2,  d2 - d1,  d1 - d3)                (fp32 additions, BEFORE the hi/lo split)
//     U = G g   = (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2)       (per (co, ci, ky), on the host in fp64, packed like the direct weights)
//     M_j = sum over (ci, ky) of U_j[co][ci][ky] * V_j[ci][row + ky][u]  (four GEMMs, j = position 0..3: the MFMA work)
//     y[2u] = M0 + M1 + M2,   y[2u + 1] = M1 - M2 - M3                   (two adds per output in the accumulator registers)
//
// i.e. 4 x 3 = 12 MFMA k-steps per pair of output columns and 16-channel chunk where the direct form needs 2 x 9 = 18: 1.5x fewer
// MFMAs for the same result.  ky stays a direct sum, so nothing is exchanged between waves and the output transform needs no LDS.
// Numerics (tools/winograd_eval.py --row): max |err| / max|y| 2-8e-7 against fp64 at 128 / 256 channels, the same as the direct
// 3-term form and as an fp32 convolution.
//
// Structure (one workgroup = 4 waves = 128 output channels x NTW x 64 output pixels):
//   * wave w owns m-tile w (32 output channels) and ALL four positions of NTW "unit tiles" (32 column pairs each): 4 x NTW x 16
//     accumulator registers.  NTW = 4: 256 accumulators, one wave per SIMD (512 registers), a weight fragment pair feeds 12 MFMAs
//     and 8 ds_read_b128 feed the same 12 -- exactly the operand traffic per MFMA of conv_f16s' best 128-channel shape;
//     NTW = 2: 128 accumulators, two workgroups per CU.
//   * LDS holds V (not the raw patch): [patch row][position][unit] records of 80 bytes ([hi c0..15 | lo c0..15 | 16 B pad]); the odd
//     multiple of 16 B keeps every ds_read_b128 lane group on 16 distinct slots.  Two buffers, one barrier per chunk.
//   * staging: a lane loads one aligned quad of columns for 4 channels (buffer_load_dwordx4), its two neighbour columns come from the
//     adjacent lanes by DPP row shifts (the tile's outermost columns from one extra dword load of the row's first / last lane; in the persistent kernel from edge lanes of their own, see its lane map), the transform is
//     7 additions per quad and channel, then the usual split and two ds_write_b64 per (position, unit).
//   * weights: packed on the host in fragment order [m-tile][chunk][ky][position][hi|lo], loaded L2 -> registers two steps ahead.
// Reference layers: DoubleConv / ConvBlocks (nnunet/lib/utils.py:1182-1215), ConvDropoutNormNonlin (generic_UNet.py:26-69), ConvGRUCell
// (convGRU.py:57-66) at >= 128 output channels.
//
// The file, top to bottom: the activation switch both accumulator layouts share (wino_activate); conv_wino_kernel<NTW, PRE>, one tile per
// workgroup; conv_wino_ps_kernel<PRE, M16>, persistent, with its staging waves and its MFMA waves in the 32x32x16 or the 16x16x32 form; the
// host half -- WinoPlan / wino_plan name what one launch will be (argument gate, route level, form, MFMA shape, geometry, LDS, grid) as a pure
// function of the ConvParams; the probes read that plan and launch_plan executes it.
#include <hip/hip_fp16.h>
#include <stdlib.h>

#include "conv.h"
#include "profile.h"

namespace cf {
namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct WinoGeom {
    int TW, UW, RT, TH, PH, QW;   // tile columns (32 | 16), column pairs ("units") per tile row, rows per 32-unit tile, tile rows, patch rows, aligned quads per tile row
    int LINE, ROWP;               // LDS bytes per (patch row, position) line and per patch row (UW = 8: + 128 B so that rows alternate bank halves)
    int tiles_x, tiles_y;
    int nchunk, c1_pad;
    int ntask;                    // PH * QW * 4 staging tasks (4 channels x 4 columns) per chunk
};
// Timing experiments (clock build, make clock ABL=n -> -DCF_WINO_ABLATE=n; wrong results by design): 1 = staging waves skip transform + LDS
// writes, 2 = MFMA waves skip the weight-fragment loads, 3 = MFMA waves skip the V-record reads, 4 = staging waves skip the global loads.
// Compile-time on purpose: a run-time knob made every load conditional and the compiler's counted waits collapsed to vmcnt(0).

constexpr int W_REC = 80, W_CK = 16, W_NSTEP = 12;
constexpr int PS_NBUF = 4;        // LDS V buffers of the persistent kernel (one barrier per pair of chunks)
CF_CLOCK_DECL(g_clock_wino)
#ifdef CF_CLOCK_STAMPS
// phase totals of the persistent kernel (shader clocks, lane 0 of MFMA wave 0 and of staging wave 4 of every workgroup):
// [0] MFMA: barrier wait, [1] MFMA: chunk compute, [2] MFMA: epilogue + item setup, [3] staging: transform + LDS write, [4] staging: load issue,
// [5] staging: barrier wait, [6] workgroups, [7] chunks; inside [2]: [8] output transform + bias + activation, [9] stores + sums, [10] statistics
__device__ unsigned long long g_wino_phase[12];
#define WINO_T() __builtin_amdgcn_s_memtime()
#define WINO_ADD(i, v) do { if (lane == 0 && (wave == 0 || wave == 4)) atomicAdd(&g_wino_phase[i], (unsigned long long)(v)); } while (0)
#else
#define WINO_T() 0ULL
#define WINO_ADD(i, v) do { } while (0)
#endif

// value of the lane one below / above inside its row of 16 lanes (DPP row_shr:1 / row_shl:1); the row's first / last lane keeps `own`
__device__ __forceinline__ float from_lane_below(float v) {
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x111, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_lane_above(float v) {
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x101, 0xf, 0xf, false));
}

// Accumulators of every kernel form as a flat list of N vectors of type V per position: f32x16 [4][NTW] in the 32x32x16 forms, f32x4v [4][8]
// in the 16x16x32 form, whose vector a16(nt, ub, cbk) is (unit tile, unit block, channel block).
__device__ constexpr int a16(int nt, int ub, int cbk) { return nt * 4 + ub * 2 + cbk; }

// activation over the accumulator registers (acc[0], acc[1]: the two output columns of a pair), for both layouts: ONE workgroup-uniform
// switch with the element loops inside (with the switch inside the unrolled element loop the epilogue was tens of KB of instructions,
// conv_f16s.hip)
template <int ACT, class V, int N>
__device__ __forceinline__ void wino_act_loop(V (&acc)[4][N]) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int r = 0; r < (int)(sizeof(V) / sizeof(float)); ++r) {
                acc[e][i][r] = act_apply(acc[e][i][r], ACT);
                __builtin_amdgcn_sched_barrier(0);      // one element at a time: these cold paths must not set the kernel's register count
            }
}

template <class V, int N>
__device__ __forceinline__ void wino_activate(V (&acc)[4][N], int act) {
    switch (act) {
        case CF_ACT_GELU: wino_act_loop<CF_ACT_GELU>(acc); break;
        case CF_ACT_RELU: wino_act_loop<CF_ACT_RELU>(acc); break;
        case CF_ACT_LRELU: wino_act_loop<CF_ACT_LRELU>(acc); break;
        case CF_ACT_TANH: wino_act_loop<CF_ACT_TANH>(acc); break;
        case CF_ACT_SIGMOID: wino_act_loop<CF_ACT_SIGMOID>(acc); break;
        default: break;
    }
}

template <int NTW, int PRE>
__global__ void __launch_bounds__(256, NTW == 4 ? 1 : 2)
conv_wino_kernel(const ConvParams p, const WinoGeom g, const _Float16* __restrict__ wpk) {
    constexpr int REC = W_REC, CK = W_CK, NSTEP = W_NSTEP;
    constexpr int VT = NTW == 4 ? 2 : 1;          // staging tasks per thread (host: ntask <= 256 * VT)
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    CF_CLOCK_BEGIN();

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int mt = blockIdx.y * 4 + wave;

    // ---- tile decode, XCD-banded: the workgroups of one XCD walk a contiguous band of tiles (vertically adjacent tiles share halo rows in its L2)
    int bid = blockIdx.x;
    {
        const int nb = gridDim.x;
        const int xcd = bid & 7, qn = nb >> 3, rn = nb & 7;
        bid = ((xcd < rn) ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (bid >> 3);
    }
    const int tx = bid % g.tiles_x;
    const int t2 = bid / g.tiles_x;
    const int ty = t2 % g.tiles_y;
    const int b = t2 / g.tiles_y;
    const int x0 = tx * g.TW, y0 = ty * g.TH;
    const int HW = p.H * p.W;
    const unsigned HW4 = (unsigned)HW * 4u;
    const int buf_bytes = g.PH * g.ROWP;
    const bool do_stats = p.gn_ws != nullptr;

    // ---- staging tasks: (channel group of 4, patch row, quad q): columns x0 + 4q .. x0 + 4q + 3 of input row y0 - 1 + py
    // per-sample buffer resources (one sample of each input < 2 GiB, host-checked): out-of-range offsets read as 0 = the zero padding
    const __amdgpu_buffer_rsrc_t rsrc1 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x1 + (long)b * p.C1 * HW), 0, (int)((long)p.C1 * HW * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc2 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x2 ? p.x2 + (long)b * p.C2 * HW : p.x1), 0, p.x2 ? (int)((long)p.C2 * HW * 4) : 0, 0x00020000);
    unsigned v_off[VT], e_off[VT], v_c4[VT];
    int v_lds[VT];
    bool v_has[VT], v_first[VT], v_last[VT];
#pragma unroll
    for (int t = 0; t < VT; ++t) {
        const int task = tid + t * 256;
        v_has[t] = task < g.ntask;
        // lane order (q, channel group, patch row): 16 consecutive lanes write 8 units x 2 channel groups -> 2-way LDS bank conflicts on the
        // ds_write_b64 (with the patch row second it was 4-way: a row is 1280 banks = 0 mod 32; SQ_LDS_BANK_CONFLICT was 35 % of the LDS cycles)
        const int q = task % g.QW;
        const int r = task / g.QW;
        const int cg = r & 3, py = r >> 2;
        const int iy = y0 - 1 + py;
        const bool row_ok = v_has[t] && (unsigned)iy < (unsigned)p.H;
        v_first[t] = q == 0;
        v_last[t] = q == g.QW - 1;
        v_off[t] = row_ok ? (unsigned)(iy * p.W + x0 + 4 * q) * 4u : OOB;
        const int ecol = v_first[t] ? x0 - 1 : x0 + g.TW;
        e_off[t] = (row_ok && (v_first[t] || v_last[t]) && (unsigned)ecol < (unsigned)p.W) ? (unsigned)(iy * p.W + ecol) * 4u : OOB;
        v_c4[t] = (unsigned)cg * 4u;
        v_lds[t] = py * g.ROWP + 2 * q * REC + cg * 8;
    }

    auto issue_loads = [&](int chunk, f32x4v (&stg)[VT][4], float (&edg)[VT][4]) {
        const int c0 = chunk * CK;
        const bool in1 = c0 < g.c1_pad;                        // workgroup-uniform
        const unsigned cb = (unsigned)(in1 ? c0 : c0 - g.c1_pad);
        const unsigned clim = (unsigned)(in1 ? p.C1 : p.C2);   // channels at or past it are the zero-weight tail: never fetched
#pragma unroll
        for (int t = 0; t < VT; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned ch = cb + v_c4[t] + (unsigned)j;
                const bool ok = ch < clim;
                const unsigned off = ok ? v_off[t] + ch * HW4 : OOB;
                const unsigned eo = ok ? e_off[t] + ch * HW4 : OOB;
                if (in1) {
                    stg[t][j] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc1, off, 0, 0));
                    edg[t][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc1, eo, 0, 0));
                } else {
                    stg[t][j] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc2, off, 0, 0));
                    edg[t][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc2, eo, 0, 0));
                }
            }
        }
    };

    // PRE: x1 is a raw convolution output; its GroupNorm / InstanceNorm + activation is applied between the load and the transform, from
    // the {mean, scale, shift} table of this sample staged once in LDS behind the two V buffers.  Padding stays exactly zero.
    const float* ctab = reinterpret_cast<const float*>(lds + 2 * buf_bytes);
    const int ctab_n = g.nchunk * CK;
    auto pre_apply = [&](float v, float cm, float ca, float cs, bool valid) -> float {
        v = (v - cm) * ca + cs;
        v = p.in_slope < 0.f ? gelu_as(v) : (v > 0.f ? v : v * p.in_slope);
        return valid ? v : 0.f;
    };
    auto write_stage = [&](int chunk, const f32x4v (&stg)[VT][4], const float (&edg)[VT][4]) {
#pragma unroll
        for (int t = 0; t < VT; ++t) {
            unsigned char* base = lds + (chunk & 1) * buf_bytes + v_lds[t];
            f32x4v cm = {0.f, 0.f, 0.f, 0.f}, ca = cm, cs = cm;
            if (PRE) {
                const int c0 = chunk * CK + (int)v_c4[t];
                cm = *reinterpret_cast<const f32x4v*>(ctab + c0);
                ca = *reinterpret_cast<const f32x4v*>(ctab + ctab_n + c0);
                cs = *reinterpret_cast<const f32x4v*>(ctab + 2 * ctab_n + c0);
            }
            const bool valid = v_off[t] != OOB, evalid = e_off[t] != OOB;
            f16x4 hi[2][4], lo[2][4];      // [unit 2q | 2q + 1][position] over the 4 channels
            float va[4][4], vb[4][4];      // [position][channel]
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float c0 = stg[t][j][0], c1 = stg[t][j][1], c2 = stg[t][j][2], c3 = stg[t][j][3], e = edg[t][j];
                if (PRE) {
                    c0 = pre_apply(c0, cm[j], ca[j], cs[j], valid);
                    c1 = pre_apply(c1, cm[j], ca[j], cs[j], valid);
                    c2 = pre_apply(c2, cm[j], ca[j], cs[j], valid);
                    c3 = pre_apply(c3, cm[j], ca[j], cs[j], valid);
                    e = pre_apply(e, cm[j], ca[j], cs[j], evalid);
                }
                // every lane takes part in the shifts (uniform control flow): quads of one patch row sit in consecutive lanes of a DPP row
                float left = from_lane_below(c3), right = from_lane_above(c0);
                left = v_first[t] ? e : left;
                right = v_last[t] ? e : right;
                va[0][j] = left - c1, va[1][j] = c0 + c1, va[2][j] = c1 - c0, va[3][j] = c0 - c2;      // unit 2q:     d = (left, c0, c1, c2)
                vb[0][j] = c1 - c3, vb[1][j] = c2 + c3, vb[2][j] = c3 - c2, vb[3][j] = c2 - right;     // unit 2q + 1: d = (c1, c2, c3, right)
            }
            // split after the channel loop: a packed pair is two adjacent channels of one position
#pragma unroll
            for (int pos = 0; pos < 4; ++pos) {
                split4_f16(va[pos][0], va[pos][1], va[pos][2], va[pos][3], hi[0][pos], lo[0][pos]);
                split4_f16(vb[pos][0], vb[pos][1], vb[pos][2], vb[pos][3], hi[1][pos], lo[1][pos]);
            }
            if (v_has[t]) {
#pragma unroll
                for (int pos = 0; pos < 4; ++pos)
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        *reinterpret_cast<f16x4*>(base + pos * g.LINE + u * REC) = hi[u][pos];
                        *reinterpret_cast<f16x4*>(base + pos * g.LINE + u * REC + CK * 2) = lo[u][pos];
                    }
            }
        }
    };

    f32x4v stg[VT][4];
    float edg[VT][4];
    issue_loads(0, stg, edg);

    // ---- per-lane B-fragment offsets: unit tile nt, lane l31 -> (tile row nt * RT + l31 / UW, unit l31 % UW)
    int b_off[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) b_off[nt] = (nt * g.RT + l31 / g.UW) * g.ROWP + (l31 % g.UW) * REC + half * 16;

    f32x16 acc[4][NTW];
#pragma unroll
    for (int pos = 0; pos < 4; ++pos)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[pos][nt][r] = 0.f;

    // packed weights: fragment (mt, chunk, step = ky * 4 + position, part) = 64 lanes x 8 halves
    const f16x8* wfrag = reinterpret_cast<const f16x8*>(wpk) + (long)mt * g.nchunk * (NSTEP * 2) * 64 + lane;
    // fragment register ring, prefetched D steps ahead (NSTEP % R == 0 keeps the slots static).  NTW = 2: a step is only 6 MFMAs (~190
    // clocks), so three steps ahead to cover an L2 round trip under load; NTW = 4: 12 MFMAs per step, two steps
    constexpr int R = NTW == 2 ? 4 : 3, D = R - 1;
    f16x8 aH[R] = {}, aL[R] = {};
    auto load_a = [&](int chunk, int step, int slot) {
        const f16x8* wc = wfrag + ((long)chunk * NSTEP + step) * 2 * 64;
        aH[slot] = wc[0];
        aL[slot] = wc[64];
    };
#pragma unroll
    for (int s = 0; s < D; ++s) load_a(0, s, s % R);
    if (PRE) {
        float* ct = reinterpret_cast<float*>(lds + 2 * buf_bytes);
        for (int k = tid; k < 3 * ctab_n; k += 256) {
            const int which = k / ctab_n, c = k - which * ctab_n;
            ct[k] = c < p.C1 ? p.in_norm[((long)b * 3 + which) * p.C1 + c] : 0.f;
        }
        __syncthreads();
    }
    write_stage(0, stg, edg);
    __syncthreads();

    // B fragments (V records) one step ahead in a second register set (NTW = 2: 16 more registers; with two waves per SIMD a read issued
    // right in front of its MFMA left the pipe idle for the LDS latency twice per step).  NTW = 4 has no registers left for it.
    constexpr int BP = NTW == 2 ? 1 : 0;
    f16x8 bH[BP + 1][NTW], bL[BP + 1][NTW];
    auto load_b = [&](const unsigned char* xb, int step, int set) {
        const int toff = (step >> 2) * g.ROWP + (step & 3) * g.LINE;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            const unsigned char* rp = xb + b_off[nt] + toff;
            bH[set][nt] = *reinterpret_cast<const f16x8*>(rp);
            bL[set][nt] = *reinterpret_cast<const f16x8*>(rp + CK * 2);
        }
    };

    for (int c = 0; c < g.nchunk; ++c) {
        const bool more = c + 1 < g.nchunk;
        const int cn = more ? c + 1 : c;
        const unsigned char* xb = lds + (c & 1) * buf_bytes;
        if (BP) load_b(xb, 0, 0);
#pragma unroll
        for (int step = 0; step < NSTEP; ++step) {
            // every load is unconditional (the last chunk re-reads itself) and pinned here, so the waits come out counted (conv_f16s.hip)
            if (step + D < NSTEP) load_a(c, step + D, (step + D) % R);
            else load_a(cn, step + D - NSTEP, (step + D) % R);
            if (step == 0) issue_loads(cn, stg, edg);
            if (BP) { if (step + 1 < NSTEP) load_b(xb, step + 1, (step + 1) & 1); }
            else load_b(xb, step, 0);
            __builtin_amdgcn_sched_barrier(0);
            const int pos = step & 3;       // compile-time after unrolling
            const int set = BP ? (step & 1) : 0;
            const f16x8 ah = aH[step % R], al = aL[step % R];
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                acc[pos][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bH[set][nt], acc[pos][nt], 0, 0, 0);
                acc[pos][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bL[set][nt], acc[pos][nt], 0, 0, 0);
                acc[pos][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bH[set][nt], acc[pos][nt], 0, 0, 0);
            }
        }
        if (more) write_stage(c + 1, stg, edg);
        __syncthreads();
    }

    // ---- output transform in the accumulator registers: acc[0] <- y[2u], acc[1] <- y[2u + 1]
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float m0 = acc[0][nt][r], m1 = acc[1][nt][r], m2 = acc[2][nt][r], m3 = acc[3][nt][r];
            acc[0][nt][r] = (m0 + m1) + m2;
            acc[1][nt][r] = (m1 - m2) - m3;
        }

    // ---- epilogue: value = act(alpha * y + bias) (+ res); optional fused GroupNorm statistics of the stored values (conv_f16s.hip)
    float ssum[16], ssq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { ssum[r] = 0.f; ssq[r] = 0.f; }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        float bv = 0.f;
        if (p.bias && co < p.Cout) bv = p.bias[co];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            acc[0][nt][r] = p.alpha * acc[0][nt][r] + bv;
            acc[1][nt][r] = p.alpha * acc[1][nt][r] + bv;
        }
    }
    wino_activate(acc, p.act);      // workgroup-uniform; the ConvGRU gates (sigmoid / tanh) are the main users on this path
    constexpr unsigned OOB_CH = 0x40000000u;
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(
        p.out + ((long)b * p.out_ctotal + p.out_coff) * (long)HW, 0, (int)((long)(p.out_ctotal - p.out_coff) * HW * 4), 0x00020000);
    unsigned o_off[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        int li = l31;
        asm volatile("" : "+v"(li));                       // keep the address math below the main loop
        const int oy = y0 + nt * g.RT + li / g.UW, ox = x0 + 2 * (li % g.UW);
        o_off[nt] = (unsigned)(oy * p.W + ox) * 4u;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool co_ok = co < p.Cout;
        const unsigned ochan = co_ok ? (unsigned)co * HW4 : OOB_CH;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            float v0 = acc[0][nt][r], v1 = acc[1][nt][r];
            if (p.res) {                                    // rare (SingleConv residuals)
                if (co_ok) {
                    const float* rp = p.res + ((long)b * p.Cout + co) * HW + (o_off[nt] >> 2);
                    v0 += rp[0];
                    v1 += rp[1];
                }
            }
            u32x2 pk;
            pk[0] = __builtin_bit_cast(unsigned, v0);
            pk[1] = __builtin_bit_cast(unsigned, v1);
            __builtin_amdgcn_raw_buffer_store_b64(pk, rs_out, o_off[nt] + ochan, 0, 0);
            const float m0 = co_ok ? v0 : 0.f, m1 = co_ok ? v1 : 0.f;
            ssum[r] += m0 + m1;
            ssq[r] += m0 * m0 + m1 * m1;
        }
    }
    if (do_stats) {
        xreduce16(ssum, lane);      // common.h: DPP + v_permlane16_swap, no LDS traffic
        xreduce16(ssq, lane);
        // workgroup-level combine in LDS (the V buffers are free now), then ONE fp64 atomic pair per (group, workgroup)
        // (fp64 from the wave's per-channel totals on, as in conv_f16s.hip)
        double* red = reinterpret_cast<double*>(lds);  // [128 channels][2]
        __syncthreads();
        red[tid] = 0.0;
        __syncthreads();
        if ((lane & 1) == 0) {
            const int r = ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
            const int cl = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            atomicAdd(&red[2 * cl], (double)ssum[0]);
            atomicAdd(&red[2 * cl + 1], (double)ssq[0]);
        }
        __syncthreads();
        if (tid < 128) {
            const int co = blockIdx.y * 128 + tid;
            const int cpg = p.Cout / p.gn_groups;
            if (co < p.Cout && (tid == 0 || co % cpg == 0)) {
                int n = cpg - co % cpg;               // channels of this group from co on
                if (n > 128 - tid) n = 128 - tid;
                if (n > p.Cout - co) n = p.Cout - co;
                double s1 = 0.0, s2 = 0.0;
                for (int j = 0; j < n; ++j) { s1 += red[2 * (tid + j)]; s2 += red[2 * (tid + j) + 1]; }
                double* w = p.gn_ws + 2L * ((long)b * p.gn_groups + co / cpg);
                atomicAdd(w, s1);
                atomicAdd(w + 1, s2);
            }
        }
    }
    CF_CLOCK_END(g_clock_wino);
}

// =====================================================================================================================================
// Persistent, wave-specialised form (the default where a layer has enough tiles): one workgroup per CU = 4 MFMA waves (one per SIMD,
// 128 accumulators each: m-tile w x 4 positions x 2 unit tiles) + 4 staging waves (one per SIMD), walking a band of (128-channel block,
// tile) items of its XCD.  Why: in the kernel above the transform / split / LDS-write stream (4.8 vector instructions per MFMA,
// SQ_INSTS_VALU / SQ_INSTS_MFMA in profiles/r04_pmc_conv_wino.txt) sits in the SAME waves as the MFMAs and the matrix pipe is busy 53 %
// of the wave cycles where the direct kernel reaches 84 %.  Here
//   * the MFMA waves issue nothing but weight-fragment loads (three steps ahead), V-record reads (one step ahead) and MFMAs, one barrier
//     per 16-channel chunk, and run the item's epilogue (output transform, bias, activation, 32 eight-byte stores per lane, statistics by
//     shuffles + one fp64 atomic pair per group -- no LDS, no barrier);
//   * the staging waves run the chunk stream ACROSS item boundaries, two chunks of loads in flight (two register sets), up to two LDS buffers
//     ahead of the MFMA waves (four V buffers);
//   * ONE barrier per PAIR of chunks: barrier j = "chunks 2j, 2j + 1 are in LDS" for the MFMA waves and "chunks 2j - 2, 2j - 1 have been read"
//     for the staging waves (which then overwrite those buffers with chunks 2j + 2, 2j + 3); both roles execute ceil(N / 2) barriers.  (With a
//     barrier per chunk and two buffers the MFMA waves waited 500-700 clocks per chunk; with pairs they wait 170-270 -- and compute 300 clocks
//     longer per chunk, because the staging wave of their SIMD is now busy beside them: the layer times moved by 0 ... +4 %.  The CU, and on data
//     the board's power limit, are what is shared; the synchronisation was not the cost.)
// Where its clocks go (make clock + tools/wino_phases.py, profiles/r04_wino_phases.txt), per 16-channel chunk of 72 MFMAs = 2 304 clocks:
// MFMA wave 3 270 in the chunk loop (2 560 without the weight-fragment loads, make clock ABL=2) + 1 110 of epilogue at 8 chunks per item
// (the stores are issue-bound: ~8 700 clocks per item) + 300-500 at the barrier; staging wave ~2 800 for ~200 vector instructions beside
// the MFMA wave of its SIMD (4 600-5 100 with the GELU of a deferred normalisation, which then sets the pace).  Two variants were built
// and measured against this one and lost: the epilogue handed to the staging waves through an LDS buffer (their stores sit in the same
// in-order vmcnt queue as the staged loads), and a 4 + 2 + 2 split with dedicated epilogue waves (two staging waves with two tasks each
// get ~6 vector-instruction slots per MFMA of their SIMD and fall behind): -8 ... -25 %.
// Wave priorities (s_setprio 3 on one role, whole kernel or epilogue only): staging waves high = -8 % on plain layers, +<= 1 % with a deferred
// normalisation; MFMA waves high = no change.  The epilogue (~8 000 clocks per item: output transform 1 500, stores + sums 3 200, statistics
// 2 200) is ~800 vector instructions on a SIMD shared with a staging wave; dwordx4 instead of dwordx2 stores did not move it.
// Deferred normalisation: the {mean, scale, shift} quads come straight from global memory with the chunk's loads (no LDS table: items of a
// band cross samples).
struct StageRegs {
    f32x4v stg[4];
    f32x4v cm, ca, cs;
};

template <int PRE, int M16>
__global__ void __launch_bounds__(512, 2)
conv_wino_ps_kernel(const ConvParams p, const WinoGeom g, const _Float16* __restrict__ wpk) {
    constexpr int NTW = 2, REC = W_REC, CK = W_CK, NSTEP = W_NSTEP;
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    CF_CLOCK_BEGIN();

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;

    // ---- this workgroup's items: band of its XCD (blocks b and b + 8 share an XCD: speed only), interleaved with the XCD's other workgroups
    const int xcd = blockIdx.x & 7, wgi = blockIdx.x >> 3, nwgx = gridDim.x >> 3;
    const int ntiles = g.tiles_x * g.tiles_y * p.B;
    const int nitems = ntiles * ((p.Cout + 127) / 128);
    const int band_lo = (int)((long)nitems * xcd / 8), band_hi = (int)((long)nitems * (xcd + 1) / 8);
    if (band_lo + wgi >= band_hi) return;
    const int n_my = (band_hi - band_lo - wgi + nwgx - 1) / nwgx;
    auto decode = [&](int i, int& cb, int& b, int& y0, int& x0) {
        const int item = band_lo + wgi + i * nwgx;
        cb = item / ntiles;
        int t = item - cb * ntiles;
        const int tx = t % g.tiles_x;
        t /= g.tiles_x;
        const int ty = t % g.tiles_y;
        b = t / g.tiles_y;
        y0 = ty * g.TH;
        x0 = tx * g.TW;
    };
    const int HW = p.H * p.W;
    const unsigned HW4 = (unsigned)HW * 4u;
    const int buf_bytes = g.PH * g.ROWP;
    const int N = n_my * g.nchunk;                        // chunks of this workgroup's stream

    if (wave >= 4) {
        // ============================================================================================================ staging waves (4 .. 7)
        // Lane map.  Each of the four waves takes a quarter of the 4 PH (patch row, channel group) rows = PH rows: PH * QW MAIN lanes (q
        // fastest, as in conv_wino_kernel, so a row of quads sits inside a 16-lane DPP row) and behind them 2 PH EDGE lanes, one per row and side.
        //   TW = 32: 6 rows x 8 quads = lanes 0 .. 47, edge lanes 48 .. 59;   TW = 16: 10 rows x 4 quads = lanes 0 .. 39, edge lanes 40 .. 59.
        // An edge lane loads the aligned quad that holds its row's edge column (left: x0 - 4 .. x0 - 1, right: x0 + TW .. x0 + TW + 3) with the
        // offsets of a main lane, so the activations every lane issues for its four columns activate the edge value too; it writes nothing to
        // LDS.  The row's first / last quad lane fetches the activated value with ds_bpermute_b32.  (Before: every lane loaded and activated
        // a fifth "edge" value per channel that only first / last lanes use -- one GELU in five -- and with ntask = 192 wave 7 had no task.)
        constexpr int VT = 1;
        const int nmain = g.PH * g.QW, el = lane - nmain;
        const bool is_main = lane < nmain, is_edge = !is_main && el < 2 * g.PH;
        const bool eleft = is_edge && (el & 1) == 0;
        bool has[VT], first[VT], last[VT];
        unsigned c4[VT];
        int v_lds[VT], t_py[VT], t_q[VT], e_src[VT];
#pragma unroll
        for (int t = 0; t < VT; ++t) {
            const int q = is_main ? lane % g.QW : 0;
            const int lr = is_main ? lane / g.QW : (is_edge ? el >> 1 : 0);
            const int r = (wave - 4) * g.PH + lr;
            const int cg = r & 3, py = r >> 2;
            has[t] = is_main;
            first[t] = is_main && q == 0;
            last[t] = is_main && q == g.QW - 1;
            c4[t] = (unsigned)cg * 4u;
            v_lds[t] = py * g.ROWP + 2 * q * REC + cg * 8;
            t_py[t] = py;
            t_q[t] = q;
            e_src[t] = (nmain + 2 * lr + (last[t] ? 1 : 0)) * 4;        // ds_bpermute address of the row's edge lane (left; right for the last quad)
        }

        int ld_i = 0, ld_c = 0, ld_b = 0;                 // the next chunk to load: item, chunk, its sample
        unsigned v_off[VT];
        __amdgpu_buffer_rsrc_t rsrc1, rsrc2;
        auto setup = [&](int i) __attribute__((always_inline)) {
            int cb, b, y0, x0;
            decode(i, cb, b, y0, x0);
#pragma unroll
            for (int t = 0; t < VT; ++t) {
                const int iy = y0 - 1 + t_py[t];
                // an edge lane's quad lies wholly inside the row or wholly outside it (W % TW == 0): outside, the lane is parked like a row
                // outside the image -- load offset AND coefficient offsets out of range, so its value stays (0 - 0) * 0 + 0 = 0 through both activations
                const int col = is_main ? x0 + 4 * t_q[t] : (eleft ? x0 - 4 : x0 + g.TW);
                const bool ok = (is_main || is_edge) && (unsigned)iy < (unsigned)p.H && (unsigned)col < (unsigned)p.W;
                v_off[t] = ok ? (unsigned)(iy * p.W + col) * 4u + c4[t] * HW4 : OOB;
            }
            // per-sample resources: offsets at or past C * HW * 4 (the zero-weight channel tail of a chunk, parked lanes) read as 0
            rsrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x1 + (long)b * p.C1 * HW), 0, (int)((long)p.C1 * HW * 4), 0x00020000);
            rsrc2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x2 ? p.x2 + (long)b * p.C2 * HW : p.x1), 0,
                                                      p.x2 ? (int)((long)p.C2 * HW * 4) : 0, 0x00020000);
            ld_b = b;
        };
        auto issue = [&](StageRegs (&R)[VT]) __attribute__((always_inline)) {   // loads chunk (ld_i, ld_c) and advances the cursor (saturating: every call loads)
#if defined(CF_WINO_ABLATE) && CF_WINO_ABLATE == 4
            return;
#endif
            const int c0 = ld_c * CK;
            const bool in1 = c0 < g.c1_pad;
            const unsigned cb = (unsigned)(in1 ? c0 : c0 - g.c1_pad);
#pragma unroll
            for (int t = 0; t < VT; ++t) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned ch = (cb + (unsigned)j) * HW4;               // scalar
                    if (in1) {
                        R[t].stg[j] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc1, v_off[t] + ch, 0, 0));
                    } else {
                        R[t].stg[j] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc2, v_off[t] + ch, 0, 0));
                    }
                }
                if (PRE) {
                    const int c = c0 + (int)c4[t];                               // C1 % 4 == 0 (host): a quad is wholly inside or wholly the padded tail
                    const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in_norm + (long)ld_b * 3 * p.C1), 0,
                                                                                        3 * p.C1 * 4, 0x00020000);
                    // rows (and edge quads) outside the image take ZERO coefficients: their loads read 0, (0 - 0) * 0 + 0 = 0 and both activations
                    // map 0 to 0, so the padding stays exactly zero without a select per value
                    const unsigned o = (c < p.C1 && v_off[t] < OOB) ? (unsigned)c * 4u : OOB;
                    R[t].cm = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rn, o, 0, 0));
                    R[t].ca = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rn, o + (unsigned)p.C1 * 4u, 0, 0));
                    R[t].cs = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rn, o + (unsigned)p.C1 * 8u, 0, 0));
                }
            }
            if (ld_c + 1 < g.nchunk) ++ld_c;
            else if (ld_i + 1 < n_my) { ld_c = 0; ++ld_i; setup(ld_i); }
        };
        auto pre_apply = [&](float v, float cm, float ca, float cs) -> float {
            v = (v - cm) * ca + cs;
            return p.in_slope < 0.f ? gelu_as(v) : (v > 0.f ? v : v * p.in_slope);
        };
        auto write = [&](const StageRegs (&RR)[VT], int gc) __attribute__((always_inline)) {
#if defined(CF_WINO_ABLATE) && CF_WINO_ABLATE == 1
            return;
#endif
#pragma unroll
            for (int t = 0; t < VT; ++t) {
                const StageRegs& R = RR[t];
                unsigned char* base = lds + (gc & (PS_NBUF - 1)) * buf_bytes + v_lds[t];
                f16x4 hi[2][4], lo[2][4];
                float va[4][4], vb[4][4];      // [position][channel]
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float c0 = R.stg[j][0], c1 = R.stg[j][1], c2 = R.stg[j][2], c3 = R.stg[j][3];
                    if (PRE) {
                        c0 = pre_apply(c0, R.cm[j], R.ca[j], R.cs[j]);
                        c1 = pre_apply(c1, R.cm[j], R.ca[j], R.cs[j]);
                        c2 = pre_apply(c2, R.cm[j], R.ca[j], R.cs[j]);
                        c3 = pre_apply(c3, R.cm[j], R.ca[j], R.cs[j]);
                    }
                    // the row's edge lane holds the column beside the tile: last of its quad on the left, first on the right
                    const float e = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(e_src[t], __builtin_bit_cast(int, eleft ? c3 : c0)));
                    float left = from_lane_below(c3), right = from_lane_above(c0);
                    left = first[t] ? e : left;
                    right = last[t] ? e : right;
                    va[0][j] = left - c1, va[1][j] = c0 + c1, va[2][j] = c1 - c0, va[3][j] = c0 - c2;
                    vb[0][j] = c1 - c3, vb[1][j] = c2 + c3, vb[2][j] = c3 - c2, vb[3][j] = c2 - right;
                }
#pragma unroll
                for (int pos = 0; pos < 4; ++pos) {
                    split4_f16(va[pos][0], va[pos][1], va[pos][2], va[pos][3], hi[0][pos], lo[0][pos]);
                    split4_f16(vb[pos][0], vb[pos][1], vb[pos][2], vb[pos][3], hi[1][pos], lo[1][pos]);
                }
                if (has[t]) {
#pragma unroll
                    for (int pos = 0; pos < 4; ++pos)
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            *reinterpret_cast<f16x4*>(base + pos * g.LINE + u * REC) = hi[u][pos];
                            *reinterpret_cast<f16x4*>(base + pos * g.LINE + u * REC + CK * 2) = lo[u][pos];
                        }
                }
            }
        };
        StageRegs A[VT], B[VT];
        setup(0);
        issue(A);
        issue(B);
        unsigned long long tw = 0, ti = 0, tb = 0;
        (void)tw; (void)ti; (void)tb;
        // Both halves of the body are UNCONDITIONAL (an odd stream is padded by one chunk: the cursor saturates and the extra chunk lands in a
        // buffer nobody reads any more).  With the second half under `if (gc + 1 < N)` the loop header had a predecessor on which set B had not
        // been re-issued, and the compiler's wait for set A there came out as vmcnt(0).
        // ONE barrier per PAIR of chunks, four LDS buffers: barrier j says "chunks 2j, 2j + 1 are in LDS" to the MFMA waves and "chunks 2j - 2,
        // 2j - 1 have been read" to these waves, which then overwrite those two buffers with chunks 2j + 2, 2j + 3.  With a barrier per chunk and
        // two buffers the roles ran in lockstep one chunk apart: the MFMA waves paid every chunk's jitter at a barrier (500-700 clocks per
        // chunk) and these waves could get only one chunk ahead during an item's epilogue (profiles/r04_wino_phases.txt).
        for (int gc = 0; gc < N; gc += 2) {
            unsigned long long t0 = WINO_T();
            write(A, gc);
            unsigned long long t1 = WINO_T();
            issue(A);                                     // chunk gc + 2 (or the stream's last chunk again)
            unsigned long long t2 = WINO_T();
            tw += t1 - t0; ti += t2 - t1;
            t0 = WINO_T();
            write(B, gc + 1);
            t1 = WINO_T();
            issue(B);
            t2 = WINO_T();
            __syncthreads();
            const unsigned long long t3 = WINO_T();
            tw += t1 - t0; ti += t2 - t1; tb += t3 - t2;
        }
        WINO_ADD(3, tw); WINO_ADD(4, ti); WINO_ADD(5, tb);
        return;
    }

    if constexpr (M16) {
        // ================================================================================================ MFMA waves, 16x16x32 form
        // The same three split products with v_mfma_f32_16x16x32_f16 (profiles/mfma_shape_f16.txt: the chip holds a 1.13-1.18x higher clock
        // under this shape on data).  K = 32 is the two 16-channel chunks of one barrier pair: lane l = 16 kg + l15 takes k-group kg & 1
        // (8 channels) of chunk gc + (kg >> 1).  The V records are the M operand (rows = units), the weights the N operand (columns =
        // channels), so a lane's four accumulator registers are four adjacent units of one row for ONE channel: eight adjacent output
        // columns = two dwordx4 stores, no lane swap, and bias / statistics are per lane instead of per register.
        //   V operand: unit 16 ub + l15 of unit tile nt: the record's 16 bytes at (kg & 1) * 16 (hi; lo at + 32) in buffer (gc & 3) + (kg >> 1)
        //   W operand: channel 16 cbk + l15: the 16 bytes of lane (kg & 1) * 32 + 16 cbk + l15 of the 32x32x16 fragment of chunk c + (kg >> 1)
        //              (pack_conv_weight_wino's order [m-tile][chunk][step][hi|lo][lane = h * 32 + r][8], h = the k-group: nothing repacked)
        //   D: acc[pos][a16(nt, ub, cbk)][r] = unit 16 ub + 4 kg + r, channel 16 cbk + l15
        // 24 MFMAs of 16 clocks per step and pair of chunks against 2 x 6 x 32 before; 8 ds_read_b128 and 4 global dwordx4 per step and
        // pair, as before.  The item's chunk count is even (host).
        const int l15 = lane & 15, kg = lane >> 4;
        int a_off[NTW][2];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int ub = 0; ub < 2; ++ub) {
                const int u = ub * 16 + l15;
                a_off[nt][ub] = (nt * g.RT + u / g.UW) * g.ROWP + (u % g.UW) * REC + (kg & 1) * 16 + (kg >> 1) * buf_bytes;
            }
        const long mt_stride = (long)g.nchunk * (NSTEP * 2) * 64;             // f16x8 units per m-tile
        const f16x8* const wbase = reinterpret_cast<const f16x8*>(wpk) + (kg >> 1) * (NSTEP * 2 * 64) + (kg & 1) * 32 + l15;
        constexpr int R = 2;                                                   // weight ring: the next step's fragments load during this step
        f16x8 wH[R][2] = {}, wL[R][2] = {};
        auto load_w = [&](const f16x8* wc, int step, int slot) {
#pragma unroll
            for (int cbk = 0; cbk < 2; ++cbk) {
                wH[slot][cbk] = wc[(step * 2) * 64 + cbk * 16];
                wL[slot][cbk] = wc[(step * 2 + 1) * 64 + cbk * 16];
            }
        };
        f16x8 vH[NTW][2] = {}, vL[NTW][2] = {};                               // the unit tile is the double buffer: nt = 1 loads while nt = 0 computes
        auto load_v = [&](const unsigned char* xb, int step, int nt) {
            const int toff = (step >> 2) * g.ROWP + (step & 3) * g.LINE;
#pragma unroll
            for (int ub = 0; ub < 2; ++ub) {
                const unsigned char* rp = xb + a_off[nt][ub] + toff;
                vH[nt][ub] = *reinterpret_cast<const f16x8*>(rp);
                vL[nt][ub] = *reinterpret_cast<const f16x8*>(rp + CK * 2);
            }
        };
        f32x4v acc[4][8];
        int cb, b, y0, x0;
        decode(0, cb, b, y0, x0);
        const f16x8* wf = wbase + (long)(cb * 4 + wave) * mt_stride;
        load_w(wf, 0, 0);
        int cb_n = cb, b_n = b, y0_n = y0, x0_n = x0;
        for (int i = 0; i < n_my; ++i) {
            cb = cb_n; b = b_n; y0 = y0_n; x0 = x0_n;
            const int mt = cb * 4 + wave;
            wf = wbase + (long)mt * mt_stride;
            if (i + 1 < n_my) decode(i + 1, cb_n, b_n, y0_n, x0_n);
            const f16x8* wf_next = wbase + (long)(cb_n * 4 + wave) * mt_stride;
#pragma unroll
            for (int pos = 0; pos < 4; ++pos)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                    for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                        for (int cbk = 0; cbk < 2; ++cbk) acc[pos][a16(nt, ub, cbk)] = f32x4v{0.f, 0.f, 0.f, 0.f};

            for (int c = 0; c < g.nchunk; c += 2) {
                const int gc = i * g.nchunk + c;                               // even: nchunk is
                const f16x8* wc = wf + (long)c * NSTEP * 2 * 64;
                const f16x8* wn = (c + 2 < g.nchunk) ? wc + 2 * NSTEP * 2 * 64 : wf_next;   // the next pair of the stream (the last one re-reads the item's first)
                __syncthreads();                                               // chunks gc and gc + 1 are in LDS
                const unsigned char* xb = lds + (gc & (PS_NBUF - 1)) * buf_bytes;
                load_v(xb, 0, 0);
#pragma unroll
                for (int step = 0; step < NSTEP; ++step) {
                    const int pos = step & 3, slot = step & 1;
                    if (step + 1 < NSTEP) load_w(wc, step + 1, slot ^ 1);
                    else load_w(wn, 0, slot ^ 1);
                    load_v(xb, step, 1);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) {
                        // the products in the order of the 32x32x16 form (W lo x V hi, W hi x V lo, W hi x V hi), each over the four independent blocks
#pragma unroll
                        for (int q = 0; q < 3; ++q)
#pragma unroll
                            for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                                for (int cbk = 0; cbk < 2; ++cbk)
                                    acc[pos][a16(nt, ub, cbk)] = __builtin_amdgcn_mfma_f32_16x16x32_f16(q == 1 ? vL[nt][ub] : vH[nt][ub], q == 0 ? wL[slot][cbk] : wH[slot][cbk],
                                                                                                   acc[pos][a16(nt, ub, cbk)], 0, 0, 0);
                        if (nt == 0) {
                            if (step + 1 < NSTEP) load_v(xb, step + 1, 0);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
            }

            // ---- epilogue of item i: the meaning of conv_wino_ps_kernel's 32x32x16 epilogue in this lane layout
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                    for (int cbk = 0; cbk < 2; ++cbk)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float m0 = acc[0][a16(nt, ub, cbk)][r], m1 = acc[1][a16(nt, ub, cbk)][r], m2 = acc[2][a16(nt, ub, cbk)][r], m3 = acc[3][a16(nt, ub, cbk)][r];
                            acc[0][a16(nt, ub, cbk)][r] = (m0 + m1) + m2;
                            acc[1][a16(nt, ub, cbk)][r] = (m1 - m2) - m3;
                        }
            bool co_ok[2];
            unsigned ochan[2];
            constexpr unsigned OOB_CH = 0x40000000u;
#pragma unroll
            for (int cbk = 0; cbk < 2; ++cbk) {
                const int co = mt * 32 + cbk * 16 + l15;
                co_ok[cbk] = co < p.Cout;
                ochan[cbk] = co_ok[cbk] ? (unsigned)co * HW4 : OOB_CH;
                const float bv = p.bias ? p.bias[co_ok[cbk] ? co : p.Cout - 1] : 0.f;
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                    for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            acc[0][a16(nt, ub, cbk)][r] = p.alpha * acc[0][a16(nt, ub, cbk)][r] + bv;
                            acc[1][a16(nt, ub, cbk)][r] = p.alpha * acc[1][a16(nt, ub, cbk)][r] + bv;
                        }
            }
            wino_activate(acc, p.act);
            const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(
                p.out + ((long)b * p.out_ctotal + p.out_coff) * (long)HW, 0, (int)((long)(p.out_ctotal - p.out_coff) * HW * 4), 0x00020000);
            float ssum[2] = {0.f, 0.f}, ssq[2] = {0.f, 0.f};
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int ub = 0; ub < 2; ++ub) {
                    const int u = ub * 16 + 4 * kg;                            // the lane's four units: one row (UW is 8 or 16)
                    const int oy = y0 + nt * g.RT + u / g.UW, ox = x0 + 2 * (u % g.UW);
                    const unsigned o_off = (unsigned)(oy * p.W + ox) * 4u;
#pragma unroll
                    for (int cbk = 0; cbk < 2; ++cbk) {
                        float v[8];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            v[2 * r] = acc[0][a16(nt, ub, cbk)][r];
                            v[2 * r + 1] = acc[1][a16(nt, ub, cbk)][r];
                        }
                        if (p.res) {
                            if (co_ok[cbk]) {
                                const float* rp = p.res + ((long)b * p.Cout + (mt * 32 + cbk * 16 + l15)) * HW + (o_off >> 2);
#pragma unroll
                                for (int k = 0; k < 8; ++k) v[k] += rp[k];
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float m0 = co_ok[cbk] ? v[2 * r] : 0.f, m1 = co_ok[cbk] ? v[2 * r + 1] : 0.f;
                            ssum[cbk] += m0 + m1;
                            ssq[cbk] += m0 * m0 + m1 * m1;
                        }
                        u32x4 pk0, pk1;
#pragma unroll
                        for (int k = 0; k < 4; ++k) { pk0[k] = __builtin_bit_cast(unsigned, v[k]); pk1[k] = __builtin_bit_cast(unsigned, v[4 + k]); }
                        __builtin_amdgcn_raw_buffer_store_b128(pk0, rs_out, o_off + ochan[cbk], 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b128(pk1, rs_out, o_off + 16u + ochan[cbk], 0, 0);
                    }
                }
            if (p.gn_ws) {
                // per-channel totals of the wave: over the registers (above) and the lane bits 4 and 5 (kg) in fp32, fp64 from there on, as in
                // the 32x32x16 form.  Lanes with kg odd then carry channel block 1, so that lane bit 4 is bit 4 of the channel cl = 16 (kg & 1) + l15.
#pragma unroll
                for (int cbk = 0; cbk < 2; ++cbk) {
                    ssum[cbk] += __shfl_xor(ssum[cbk], 16, 64);
                    ssum[cbk] += __shfl_xor(ssum[cbk], 32, 64);
                    ssq[cbk] += __shfl_xor(ssq[cbk], 16, 64);
                    ssq[cbk] += __shfl_xor(ssq[cbk], 32, 64);
                }
                double s1 = (kg & 1) ? ssum[1] : ssum[0], s2 = (kg & 1) ? ssq[1] : ssq[0];
                const int cpg = p.Cout / p.gn_groups;
                const int cl = 16 * (kg & 1) + l15;
                const bool pow2 = (cpg & (cpg - 1)) == 0;
                int k = 0;
                if (pow2 && cpg > 1) { s1 += __shfl_xor(s1, 1, 64); s2 += __shfl_xor(s2, 1, 64); k = 1; }
                if (pow2 && cpg > 2) { s1 += __shfl_xor(s1, 2, 64); s2 += __shfl_xor(s2, 2, 64); k = 2; }
                if (pow2 && cpg > 4) { s1 += __shfl_xor(s1, 4, 64); s2 += __shfl_xor(s2, 4, 64); k = 3; }
                if (pow2 && cpg > 8) { s1 += __shfl_xor(s1, 8, 64); s2 += __shfl_xor(s2, 8, 64); k = 4; }
                if (pow2 && cpg > 16) { s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64); k = 5; }
                const int span = pow2 ? (1 << k) : 1;                        // channels whose total this lane now holds
                const int co = mt * 32 + cl;
                if (kg < 2 && (cl & (span - 1)) == 0 && co < p.Cout) {
                    double* w = p.gn_ws + 2L * ((long)b * p.gn_groups + co / cpg);
                    atomicAdd(w, s1);
                    atomicAdd(w + 1, s2);
                }
            }
        }
        CF_CLOCK_END(g_clock_wino);
        return;
    } else {
    // =================================================================================================================== MFMA waves
    int b_off[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) b_off[nt] = (nt * g.RT + l31 / g.UW) * g.ROWP + (l31 % g.UW) * REC + half * 16;
    const long mt_stride = (long)g.nchunk * (NSTEP * 2) * 64;             // f16x8 units per m-tile
    const f16x8* const wbase = reinterpret_cast<const f16x8*>(wpk) + lane;
    // weight-fragment ring, three steps ahead (a six-slot ring -- five steps, ~960 MFMA clocks -- took the chunk from 3 270 to 2 890 clocks
    // in the variant whose epilogue ran in other waves, profiles/r04_wino_phases.txt, but does not fit beside this role's epilogue registers)
    constexpr int R = 4, D = R - 1;
    f16x8 aH[R] = {}, aL[R] = {};
    auto load_a = [&](const f16x8* wc, int slot) {
#if defined(CF_WINO_ABLATE) && CF_WINO_ABLATE == 2
        return;
#endif
        aH[slot] = wc[0];
        aL[slot] = wc[64];
    };
    f16x8 bH[2][NTW] = {}, bL[2][NTW] = {};
    auto load_b = [&](const unsigned char* xb, int step, int set) {
#if defined(CF_WINO_ABLATE) && CF_WINO_ABLATE == 3
        return;
#endif
        const int toff = (step >> 2) * g.ROWP + (step & 3) * g.LINE;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            const unsigned char* rp = xb + b_off[nt] + toff;
            bH[set][nt] = *reinterpret_cast<const f16x8*>(rp);
            bL[set][nt] = *reinterpret_cast<const f16x8*>(rp + CK * 2);
        }
    };
    f32x16 acc[4][NTW];
    int cb, b, y0, x0;
    decode(0, cb, b, y0, x0);
    const f16x8* wf = wbase + (long)(cb * 4 + wave) * mt_stride;
#pragma unroll
    for (int s = 0; s < D; ++s) load_a(wf + (long)s * 2 * 64, s % R);

    unsigned long long tm_wait = 0, tm_comp = 0, tm_epi = 0, tm_e1 = 0, tm_e2 = 0, tm_e3 = 0, tm_mark = WINO_T();
    (void)tm_wait; (void)tm_comp; (void)tm_epi; (void)tm_mark;
    int cb_n = cb, b_n = b, y0_n = y0, x0_n = x0;          // the item after the current one (decoded once per item)
    for (int i = 0; i < n_my; ++i) {
        cb = cb_n; b = b_n; y0 = y0_n; x0 = x0_n;
        const int mt = cb * 4 + wave;
        wf = wbase + (long)mt * mt_stride;
        if (i + 1 < n_my) decode(i + 1, cb_n, b_n, y0_n, x0_n);
        const f16x8* wf_next = wbase + (long)(cb_n * 4 + wave) * mt_stride;
#pragma unroll
        for (int pos = 0; pos < 4; ++pos)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[pos][nt][r] = 0.f;

        for (int c = 0; c < g.nchunk; ++c) {
            const int gc = i * g.nchunk + c;
            const f16x8* wc = wf + (long)c * NSTEP * 2 * 64;
            const f16x8* wn = (c + 1 < g.nchunk) ? wc + NSTEP * 2 * 64 : wf_next;      // the next chunk of the stream (the last one re-reads itself)
            {
                const unsigned long long ta = WINO_T();
                if (c == 0) tm_epi += ta - tm_mark; else tm_comp += ta - tm_mark;
                if ((gc & 1) == 0) __syncthreads();       // chunks gc and gc + 1 are in LDS (one barrier per pair: see the staging loop)
                tm_mark = WINO_T();
                tm_wait += tm_mark - ta;
            }
            const unsigned char* xb = lds + (gc & (PS_NBUF - 1)) * buf_bytes;
            load_b(xb, 0, 0);
#pragma unroll
            for (int step = 0; step < NSTEP; ++step) {
                if (step + D < NSTEP) load_a(wc + (long)(step + D) * 2 * 64, (step + D) % R);
                else load_a(wn + (long)(step + D - NSTEP) * 2 * 64, (step + D) % R);
                if (step + 1 < NSTEP) load_b(xb, step + 1, (step + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
                const int pos = step & 3;
                const int set = step & 1;
                const f16x8 ah = aH[step % R], al = aL[step % R];
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) {
                    acc[pos][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bH[set][nt], acc[pos][nt], 0, 0, 0);
                    acc[pos][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bL[set][nt], acc[pos][nt], 0, 0, 0);
                    acc[pos][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bH[set][nt], acc[pos][nt], 0, 0, 0);
                }
            }
        }

        {
            const unsigned long long ta = WINO_T();
            tm_comp += ta - tm_mark;
            tm_mark = ta;
        }
        // ---- epilogue of item i (the staging waves are already one chunk into the next item)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float m0 = acc[0][nt][r], m1 = acc[1][nt][r], m2 = acc[2][nt][r], m3 = acc[3][nt][r];
                acc[0][nt][r] = (m0 + m1) + m2;
                acc[1][nt][r] = (m1 - m2) - m3;
            }
        float ssum[16], ssq[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ssum[r] = 0.f;
            ssq[r] = 0.f;
            const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            // branch-free (a clamped index and a select; sixteen `if (co < Cout)` loads were sixteen exec-mask branches per item)
            const float bv = p.bias ? p.bias[co < p.Cout ? co : p.Cout - 1] : 0.f;
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                acc[0][nt][r] = p.alpha * acc[0][nt][r] + bv;
                acc[1][nt][r] = p.alpha * acc[1][nt][r] + bv;
            }
        }
        wino_activate(acc, p.act);
        const unsigned long long te1 = WINO_T();
        constexpr unsigned OOB_CH = 0x40000000u;
        const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(
            p.out + ((long)b * p.out_ctotal + p.out_coff) * (long)HW, 0, (int)((long)(p.out_ctotal - p.out_coff) * HW * 4), 0x00020000);
        unsigned o_off[NTW];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            const int oy = y0 + nt * g.RT + l31 / g.UW, ox = x0 + 2 * (l31 % g.UW);
            o_off[nt] = (unsigned)(oy * p.W + ox) * 4u;
        }
        // Stores: a lane holds two adjacent columns of unit u for both unit tiles (nt = 0, 1).  Adjacent lanes (units u, u + 1 of one row: UW is
        // even) swap one pair through a DPP quad permute, after which the even lane owns four adjacent columns of tile 0 and the odd lane four of
        // tile 1: 16 sixteen-byte stores per lane instead of 32 eight-byte ones (the store path moves ~14 B per clock and CU with dwordx4, half
        // that with dwordx2, and the item's stores were its epilogue: profiles/r04_wino_phases.txt).
        const bool odd = (lane & 1) != 0;
        const unsigned st_off = odd ? o_off[1] - 8u : o_off[0];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const bool co_ok = co < p.Cout;
            const unsigned ochan = co_ok ? (unsigned)co * HW4 : OOB_CH;
            float v[NTW][2];
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                float v0 = acc[0][nt][r], v1 = acc[1][nt][r];
                if (p.res) {
                    if (co_ok) {
                        const float* rp = p.res + ((long)b * p.Cout + co) * HW + (o_off[nt] >> 2);
                        v0 += rp[0];
                        v1 += rp[1];
                    }
                }
                v[nt][0] = v0;
                v[nt][1] = v1;
                const float m0 = co_ok ? v0 : 0.f, m1 = co_ok ? v1 : 0.f;
                ssum[r] += m0 + m1;
                ssq[r] += m0 * m0 + m1 * m1;
            }
            const float k0 = odd ? v[1][0] : v[0][0], k1 = odd ? v[1][1] : v[0][1];      // kept: the own tile's pair
            const int s0 = __builtin_bit_cast(int, odd ? v[0][0] : v[1][0]), s1 = __builtin_bit_cast(int, odd ? v[0][1] : v[1][1]);
            const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(s0, s0, 0xB1, 0xf, 0xf, false));   // quad_perm [1, 0, 3, 2]
            const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(s1, s1, 0xB1, 0xf, 0xf, false));
            u32x4 pk;
            pk[0] = __builtin_bit_cast(unsigned, odd ? r0 : k0);
            pk[1] = __builtin_bit_cast(unsigned, odd ? r1 : k1);
            pk[2] = __builtin_bit_cast(unsigned, odd ? k0 : r0);
            pk[3] = __builtin_bit_cast(unsigned, odd ? k1 : r1);
            __builtin_amdgcn_raw_buffer_store_b128(pk, rs_out, st_off + ochan, 0, 0);
        }
        const unsigned long long te2 = WINO_T();
        tm_e1 += te1 - tm_mark;
        tm_e2 += te2 - te1;
        if (p.gn_ws) {
            // per-channel totals by the transpose-reduce of conv_f16s.hip: afterwards the lane with bits (b5 b4 b3 b2 b1 x) holds channel
            // cl = b1 + 2 b2 + 4 b5 + 8 b3 + 16 b4 of this wave's 32; a group of cpg = 2^k consecutive channels is then summed by k more
            // xor-shuffles over the lane bits of cl's low k bits, and one lane per group adds the pair to the fp64 workspace.
            xreduce16(ssum, lane);      // common.h: DPP + v_permlane16_swap, no LDS traffic
            xreduce16(ssq, lane);
            double s1 = ssum[0], s2 = ssq[0];                                // fp64 from the wave's per-channel totals on (conv_f16s.hip)
            const int cpg = p.Cout / p.gn_groups;
            const int cl = ((lane >> 1) & 1) + 2 * ((lane >> 2) & 1) + 4 * half + 8 * ((lane >> 3) & 1) + 16 * ((lane >> 4) & 1);
            int k = 0;
            const bool pow2 = (cpg & (cpg - 1)) == 0;
            // lane masks of cl's bits 0..4: 2, 4, 32, 8, 16 (wave-uniform conditions; the mask-4 level needs the mask-2 level before it: common.h)
            if (pow2 && cpg > 1) { s1 = xor_sum<2>(s1); s2 = xor_sum<2>(s2); k = 1; }
            if (pow2 && cpg > 2) { s1 = xor_sum<4>(s1); s2 = xor_sum<4>(s2); k = 2; }
            if (pow2 && cpg > 4) { s1 = xor_sum<32>(s1); s2 = xor_sum<32>(s2); k = 3; }
            if (pow2 && cpg > 8) { s1 = xor_sum<8>(s1); s2 = xor_sum<8>(s2); k = 4; }
            if (pow2 && cpg > 16) { s1 = xor_sum<16>(s1); s2 = xor_sum<16>(s2); k = 5; }
            const int span = pow2 ? (1 << k) : 1;                            // channels whose total this lane now holds
            const int co = mt * 32 + cl;
            if ((lane & 1) == 0 && (cl & (span - 1)) == 0 && co < p.Cout) {
                double* w = p.gn_ws + 2L * ((long)b * p.gn_groups + co / cpg);
                atomicAdd(w, s1);
                atomicAdd(w + 1, s2);
            }
        }
        tm_e3 += WINO_T() - te2;
    }
    tm_epi += WINO_T() - tm_mark;
    WINO_ADD(0, tm_wait); WINO_ADD(1, tm_comp); WINO_ADD(2, tm_epi); WINO_ADD(6, 1); WINO_ADD(7, N);
    WINO_ADD(8, tm_e1); WINO_ADD(9, tm_e2); WINO_ADD(10, tm_e3);
    CF_CLOCK_END(g_clock_wino);
    }
}

// route level: 0 = off (every layer stays on the direct kernels), 1 = automatic (the persistent wave-specialised kernel where a layer has at
// least two items per CU, else the one-tile-per-workgroup kernel with 2 unit tiles per wave), 2 / 4 = force the one-tile kernel with
// NTW = 2 / 4 (NTW 4 runs only when forced), 8 = force the persistent kernel -- each where the geometry allows.  Initial value from CF_CONV_WINO (0 | 1 | 2 | 4 | 8);
// cf_conv_wino_enable changes it at run time (tests, A/B runs).  16 = level 1's routing with the persistent kernel forced as at level 8 AND its
// 16x16x32 MFMA form forced wherever that form applies (wino_plan); the other levels never change meaning.  wino_plan is its one reader.
int g_wino_level = -1;
int wino_level() {
    if (g_wino_level < 0) {
        const char* e = getenv("CF_CONV_WINO");
        int v = e ? atoi(e) : 1;
        if (!(v == 0 || v == 1 || v == 2 || v == 4 || v == 8 || v == 16)) v = 1;
        g_wino_level = v;
    }
    return g_wino_level;
}

bool wino_geometry(const ConvParams& p, int ntw, WinoGeom& g) {
    g.TW = p.W >= 32 ? 32 : 16;
    g.UW = g.TW / 2;
    g.RT = 32 / g.UW;
    g.TH = ntw * g.RT;
    g.PH = g.TH + 2;
    g.QW = g.TW / 4;
    g.LINE = g.UW * W_REC;
    g.ROWP = 4 * g.LINE + (g.UW == 8 ? 128 : 0);
    if (p.W % g.TW != 0 || p.H % g.TH != 0) return false;
    g.tiles_x = p.W / g.TW;
    g.tiles_y = p.H / g.TH;
    g.c1_pad = p.C2 > 0 ? ((p.C1 + W_CK - 1) / W_CK) * W_CK : (1 << 30);
    g.nchunk = p.C2 > 0 ? g.c1_pad / W_CK + (p.C2 + W_CK - 1) / W_CK : (p.C1 + W_CK - 1) / W_CK;
    g.ntask = g.PH * g.QW * 4;
    return g.ntask <= 256 * (ntw == 4 ? 2 : 1);
}

// MFMA shape of the persistent kernel's matrix waves at level 1: true = v_mfma_f32_16x16x32_f16, per class of launch -- {plain,
// LeakyReLU-deferred, GELU-deferred} x {TW 32, TW 16} -- and only where the layer table measured it faster (profiles/wino_mfma16_bench.md,
// tools/wino_ab.py on the bench's 13 layers, level 8 against level 16 in interleaved rounds): plain +5.4 ... +9.8 % (TW 32) and +7.3 % (TW 16),
// LeakyReLU-deferred +4.8 ... +5.5 % and +4.6 %, GELU-deferred +1.4 ... +3.5 % at TW 32 (the staging waves pace those layers); the bench has
// no GELU-deferred layer at TW 16, so that class is unmeasured and stays on the 32x32x16 form.
constexpr bool WINO_M16_CLASS[3][2] = {
    // TW 32, TW 16
    {true, true},     // plain
    {true, true},     // deferred norm + LeakyReLU
    {true, false},    // deferred norm + GELU
};

// What one launch will be: a pure function of the ConvParams (pointers are read for their alignment, never dereferenced), of this thread's
// product mode and of the route level.  The probes read it, launch_plan executes it: what a probe accepts, the launch runs.
struct WinoPlan {
    int form = 0;                // 0 = declined, 2 / 4 = one tile per workgroup with that many unit tiles per wave, 8 = persistent
    bool m16 = false;            // form 8: the matrix waves run the 16x16x32 MFMA form
    WinoGeom g = {};             // the kernel's geometry argument, complete
    size_t lds_bytes = 0;        // dynamic LDS of the launch
    dim3 grid, block;
    const char* why = nullptr;   // form 0: the message for set_error
};
WinoPlan wino_declined(const char* why) { WinoPlan pl; pl.why = why; return pl; }

WinoPlan wino_plan(const ConvParams& p) {
    const int lvl = wino_level();
    // ---- the argument gate
    if (lvl == 0) return wino_declined("conv_wino: switched off (route level 0)");
    if (conv_terms() != 3) return wino_declined("conv_wino: the one-term product mode is built in conv_f16s only");
    if (p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad_h != 1 || p.pad_w != 1 || p.w_bstride || p.scatter2x2)
        return wino_declined("conv_wino: not a plain 3x3 / stride 1 / pad 1 convolution");
    // Cout: whole 128-channel blocks, or a last block at least three quarters full (the U-Net's 480), as conv_f16s' 128-channel shapes
    if (!(p.Cout % 128 == 0 || (p.Cout > 128 && p.Cout % 128 >= 96))) return wino_declined("conv_wino: Cout is neither whole 128-channel blocks nor ends in a block of >= 96");
    if (p.W < 16 || (p.W & 15) != 0) return wino_declined("conv_wino: W is not a multiple of 16");
    if (((reinterpret_cast<uintptr_t>(p.x1) | reinterpret_cast<uintptr_t>(p.x2)) & 15) != 0) return wino_declined("conv_wino: inputs are not 16-byte aligned");
    const long HW = (long)p.H * p.W;
    if ((long)p.C1 * HW * 4 >= (1L << 31) || (long)p.C2 * HW * 4 >= (1L << 31)) return wino_declined("conv_wino: one sample of an input reaches 2 GiB");
    if ((long)p.out_ctotal * HW * 4 >= (1L << 30))          // 32-bit store offsets, two parking values (kernel epilogue)
        return wino_declined("conv_wino: one sample of the output tensor reaches 1 GiB");
    if (p.in_norm && (p.C2 != 0 || (reinterpret_cast<uintptr_t>(p.in_norm) & 3) != 0))
        return wino_declined("conv_wino: a deferred normalisation needs a single input and an aligned coefficient table");
    if (p.gn_ws && (p.gn_groups <= 0 || p.Cout % p.gn_groups != 0)) return wino_declined("conv_wino: bad GroupNorm statistics request");

    WinoPlan pl;
    const long cblocks = (p.Cout + 127) / 128;
    // ---- the persistent form: levels 8 and 16 force it, level 1 takes it where the layer has at least two items per CU
    // (PH * QW main + 2 PH edge lanes per staging wave: 60 of 64 in both geometries)
    if ((lvl == 1 || lvl == 8 || lvl == 16) && wino_geometry(p, 2, pl.g) && pl.g.PH * (pl.g.QW + 2) <= 64 &&
        (size_t)PS_NBUF * pl.g.PH * pl.g.ROWP <= LDS_LIMIT &&
        (!p.in_norm || ((p.C1 & 3) == 0 && (reinterpret_cast<uintptr_t>(p.in_norm) & 15) == 0))) {
        const long nitems = (long)pl.g.tiles_x * pl.g.tiles_y * p.B * cblocks;
        const long ncu = device_cu_count();
        if (lvl != 1 || nitems >= 2 * ncu) {
            pl.form = 8;
            // the 16x16x32 form needs an even number of 16-channel chunks per item (its K = 32 is a pair of chunks; an odd count would span
            // two items); level 16 forces it where it applies, level 1 takes it per class of launch, level 8 never
            const int cls = !p.in_norm ? 0 : (p.in_slope < 0.f ? 2 : 1);
            pl.m16 = (pl.g.nchunk & 1) == 0 && (lvl == 16 || (lvl == 1 && WINO_M16_CLASS[cls][pl.g.TW == 32 ? 0 : 1]));
            pl.lds_bytes = (size_t)PS_NBUF * pl.g.PH * pl.g.ROWP;
            const long nwg = ncu < ((nitems + 7) & ~7L) ? ncu : ((nitems + 7) & ~7L);      // one workgroup per CU, a multiple of the 8 XCDs
            pl.grid = dim3((unsigned)nwg);
            pl.block = dim3(512);
            return pl;
        }
    }
    if (lvl == 8) return wino_declined("conv_wino: the forced persistent form does not take this geometry");
    // ---- the one-tile form: NTW 2 (two workgroups per CU) unless level 4 forces NTW 4 -- level 1 never picks NTW 4
    const int ntw = lvl == 4 ? 4 : 2;
    if (!wino_geometry(p, ntw, pl.g)) return wino_declined("conv_wino: H or W is not a multiple of the tile");
    // two V buffers and, behind them, the deferred norm's {mean, scale, shift} table of one sample
    pl.lds_bytes = (size_t)2 * pl.g.PH * pl.g.ROWP + (p.in_norm ? (size_t)3 * pl.g.nchunk * W_CK * sizeof(float) : 0);
    if (pl.lds_bytes > LDS_LIMIT) return wino_declined("conv_wino: the deferred norm's coefficient table does not fit the LDS beside the tile");
    pl.form = ntw;
    pl.grid = dim3((unsigned)(pl.g.tiles_x * pl.g.tiles_y * p.B), (unsigned)cblocks);
    pl.block = dim3(256);
    return pl;
}

template <auto KERNEL>
int wino_run(const char* family, const ConvParams& p, const WinoPlan& pl, const _Float16* wpk, hipStream_t s) {
    const double flops = 2.0 * (double)p.B * p.H * p.W * p.Cout * (p.C1 + p.C2) * 9.0;     // algorithmic (direct-form) flops
    return launch_lds<KERNEL>(family, PK_CONV_WINO, flops, pl.grid, pl.block, pl.lds_bytes, s, p, pl.g, wpk);
}

int launch_plan(const ConvParams& p, const WinoPlan& pl, const _Float16* wpk, hipStream_t s) {
    if (!pl.form) { set_error(pl.why); return CF_ERR_ARG; }
    const bool pre = p.in_norm != nullptr;
    return launch_with_stats("conv_wino", p.gn_ws, p.gn_groups, p.gn_prezeroed, true, p.out, p.B, p.Cout, p.Ho * p.Wo, s, [&](double*) {      // every form fuses
        if (pl.form == 8) {
            const char* ps = "conv_wino (persistent)";
            if (pl.m16) return pre ? wino_run<conv_wino_ps_kernel<1, 1>>(ps, p, pl, wpk, s) : wino_run<conv_wino_ps_kernel<0, 1>>(ps, p, pl, wpk, s);
            return pre ? wino_run<conv_wino_ps_kernel<1, 0>>(ps, p, pl, wpk, s) : wino_run<conv_wino_ps_kernel<0, 0>>(ps, p, pl, wpk, s);
        }
        if (pl.form == 4) return pre ? wino_run<conv_wino_kernel<4, 1>>("conv_wino", p, pl, wpk, s) : wino_run<conv_wino_kernel<4, 0>>("conv_wino", p, pl, wpk, s);
        return pre ? wino_run<conv_wino_kernel<2, 1>>("conv_wino", p, pl, wpk, s) : wino_run<conv_wino_kernel<2, 0>>("conv_wino", p, pl, wpk, s);
    });
}

}  // namespace

bool conv_wino_applicable(const ConvParams& p) { return wino_plan(p).form != 0; }

int launch_conv_wino(const ConvParams& p, const _Float16* wpk, hipStream_t s) { return launch_plan(p, wino_plan(p), wpk, s); }

}  // namespace cf

using namespace cf;

static void wino_params(ConvParams& p, const float* x1, int C1, const float* x2, int C2, const float* bias, const float* res, float* out,
                        int out_ctotal, int out_coff, int B, int H, int W, int Cout, int act, float alpha, double* gn_ws, int gn_groups) {
    p.x1 = x1; p.x2 = C2 ? x2 : nullptr; p.wt = nullptr; p.bias = bias; p.res = res; p.out = out; p.w_bstride = 0;
    p.C1 = C1; p.C2 = C2; p.B = B; p.H = H; p.W = W; p.Cout = Cout; p.KH = 3; p.KW = 3; p.stride = 1;
    p.pad_h = 1; p.pad_w = 1; p.Ho = H; p.Wo = W; p.out_ctotal = out_ctotal; p.out_coff = out_coff; p.act = act; p.alpha = alpha; p.scatter2x2 = 0;
    set_stats_request(p, gn_ws, gn_groups);
}

// the plan of a shape query (no tensors: an aligned dummy address, never dereferenced).  prenorm: 0 = none, 1 = deferred norm + LeakyReLU,
// 2 = deferred norm + GELU
static WinoPlan wino_query(int B, int C1, int C2, int H, int W, int Cout, int prenorm) {
    if (B <= 0 || C1 <= 0 || C2 < 0 || H <= 0 || W <= 0 || Cout <= 0) return WinoPlan();
    ConvParams p;
    float* dummy = reinterpret_cast<float*>(uintptr_t(256));
    wino_params(p, dummy, C1, C2 ? dummy : nullptr, C2, nullptr, nullptr, dummy, Cout, 0, B, H, W, Cout, CF_ACT_NONE, 1.f, nullptr, 0);
    if (prenorm) { p.in_norm = dummy; p.in_slope = prenorm == 2 ? -1.f : 0.01f; }
    return wino_plan(p);
}

CF_CLOCK_READER(cf_debug_clock_wino, cf::g_clock_wino)
#ifdef CF_CLOCK_STAMPS
extern "C" int cf_debug_wino_phases(unsigned long long* out12) {
    const unsigned long long z[12] = {};
    if (hipDeviceSynchronize() != hipSuccess) return CF_ERR_LAUNCH;
    if (hipMemcpyFromSymbol(out12, HIP_SYMBOL(cf::g_wino_phase), sizeof(z)) != hipSuccess) return CF_ERR_LAUNCH;
    if (hipMemcpyToSymbol(HIP_SYMBOL(cf::g_wino_phase), z, sizeof(z)) != hipSuccess) return CF_ERR_LAUNCH;
    return CF_OK;
}
#endif

extern "C" int cf_conv_wino_enable(int level) {
    const int prev = wino_level();
    if (level == 0 || level == 1 || level == 2 || level == 4 || level == 8 || level == 16) g_wino_level = level;
    return prev;
}

// the kernel form the dispatch picks for the layer: 0 = not a Winograd layer, 2 / 4 = one tile per workgroup, 8 = persistent
extern "C" int cf_conv2d_wino_form(int B, int C1, int C2, int H, int W, int Cout, int prenorm) { return wino_query(B, C1, C2, H, W, Cout, prenorm).form; }

// MFMA shape the dispatch picks for the layer: 16 = the persistent kernel's 16x16x32 form, 32 = any other Winograd form, 0 = not a Winograd layer.
extern "C" int cf_conv2d_wino_mfma(int B, int C1, int C2, int H, int W, int Cout, int prenorm) {
    const WinoPlan pl = wino_query(B, C1, C2, H, W, Cout, prenorm);
    return !pl.form ? 0 : (pl.m16 ? 16 : 32);
}

extern "C" int cf_conv2d_wino_ok(int B, int C1, int C2, int H, int W, int Cout, int prenorm) { return wino_query(B, C1, C2, H, W, Cout, prenorm).form != 0 ? 1 : 0; }

extern "C" int cf_conv2d_wino(const float* x1, int C1, const float* x2, int C2, const void* wpk, const float* bias, const float* res, float* out,
                              int out_ctotal, int out_coff, int B, int H, int W, int Cout, int act, float alpha, double* gn_ws, int gn_groups,
                              void* stream) {
    CF_REQUIRE(x1 && wpk && out, "null pointer");
    CF_REQUIRE(C1 > 0 && C2 >= 0 && (C2 == 0 || x2), "bad channel split C1=%d C2=%d", C1, C2);
    CF_REQUIRE(B > 0 && H > 0 && W > 0 && Cout > 0, "bad shape B=%d H=%d W=%d Cout=%d", B, H, W, Cout);
    CF_REQUIRE(out_coff >= 0 && out_coff + Cout <= out_ctotal, "output channel slice out of range");
    CF_REQUIRE(act >= CF_ACT_NONE && act <= CF_ACT_SIGMOID, "bad activation %d", act);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(wpk) & 15) == 0, "packed weights must be 16-byte aligned");
    ConvParams p;
    wino_params(p, x1, C1, x2, C2, bias, res, out, out_ctotal, out_coff, B, H, W, Cout, act, alpha, gn_ws, gn_groups);
    CF_REQUIRE(!gn_ws || (p.gn_groups > 0 && Cout % p.gn_groups == 0 && out_coff == 0 && out_ctotal == Cout), "bad GroupNorm statistics request");
    const WinoPlan pl = wino_plan(p);
    CF_REQUIRE(pl.form != 0, "layer shape outside the Winograd kernel (3x3 / stride 1 / pad 1, Cout in whole 128-channel blocks or a last block >= 96, "
                             "W %% 16 == 0, H a multiple of the tile rows, 16-byte aligned inputs; cf_conv2d_wino_ok answers per shape): %s", pl.why);
    return launch_plan(p, pl, reinterpret_cast<const _Float16*>(wpk), as_stream(stream));
}

extern "C" int cf_conv2d_wino_prenorm(const float* x, int C, const float* in_norm, float in_slope, const void* wpk, const float* bias, float* out,
                                      int B, int H, int W, int Cout, float alpha, double* gn_ws, int gn_groups, void* stream) {
    CF_REQUIRE(x && wpk && out && in_norm, "null pointer");
    CF_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Cout > 0, "bad shape B=%d C=%d H=%d W=%d Cout=%d", B, C, H, W, Cout);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(wpk) & 15) == 0, "packed weights must be 16-byte aligned");
    ConvParams p;
    wino_params(p, x, C, nullptr, 0, bias, nullptr, out, Cout, 0, B, H, W, Cout, CF_ACT_NONE, alpha, gn_ws, gn_groups);
    p.in_norm = in_norm;
    p.in_slope = in_slope;
    CF_REQUIRE(!gn_ws || (p.gn_groups > 0 && Cout % p.gn_groups == 0), "bad GroupNorm statistics request");
    const WinoPlan pl = wino_plan(p);
    CF_REQUIRE(pl.form != 0, "layer shape outside the Winograd kernel (cf_conv2d_wino_ok answers per shape): %s", pl.why);
    return launch_plan(p, pl, reinterpret_cast<const _Float16*>(wpk), as_stream(stream));
}
