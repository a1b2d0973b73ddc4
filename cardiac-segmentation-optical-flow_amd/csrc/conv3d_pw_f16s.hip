// Strided (1,1,1) nn.Conv3d forward -- the skip projection of a residual block (conv_blocks.py:126-129) -- as a gathered-B GEMM on the f16
// MFMA (v_mfma_f32_32x32x16_f16) with the 3-term hi/lo operand split of conv3d_f16s.hip (same numerics, same split-exact contract).
//
//     D[co][b, zo, yo, xo] = alpha * sum_ci W[co][ci] * X[b, ci, zo*sd, yo*s, xo*s] + bias[co]
//
// No padding, stride (sd, s, s) with sd, s in {1, 2} independently, K = Cin.
//   * Layout: x and out are dense NCDHW, read and written in place.  Only the (zo*sd, yo*s) rows that the output needs are ever addressed:
//     the planes and rows between them are never read, and neither is anything past the last sampled plane / row / column.
//   * Gather: a staging task is (output voxel, 8-channel group); the lanes of a wave hold consecutive output voxels, so one load instruction
//     walks a row of x at a 4 * s byte pitch.  At s = 2 that touches exactly the 32-byte sectors a full-width read of the row touches and
//     drops the odd columns in the address instead of in a register: same HBM traffic, half the load instructions.
//   * Schedule: one tile of 128 output voxels per workgroup, 64 (32 for Cout <= 32) output channels per blockIdx.y; a step stages 32 input
//     channels -- two 16-channel k-steps -- through LDS as [hi c0..16) | lo c0..16) | 16 B pad] records at the conflict-free 80-byte pitch of
//     conv3d_f16s.hip, double-buffered with one barrier per step, and runs 3 MFMAs per (k-step, pixel tile) on it.
//   * Small maps: when two or more whole samples fit a tile, a workgroup holds up to 128 / (Do*Ho*Wo) of them; the statistics then come
//     from the statistics pass of norm.hip after the kernel.  Otherwise a workgroup stays inside one sample and the fused statistics are
//     summed in a fixed order (conv3d.h).
//   * Weights: cineflow.ops.pack_conv_weight_f16s' 1x1 order [m-tile][chunk of 32][k-step][hi/lo][lane][8], 1 KiB per fragment, one
//     coalesced dwordx4 per lane from L1/L2, the next step's four fragments prefetched while the current step multiplies.
// Only the 3-term product is built: under cf_conv_terms(1) cf_conv3d_pw_f16s_ok answers 0 and the caller keeps its 2-D composition.
// Host half (below the kernel): one plan per launch and one per call, read by the probe and the launcher alike; the epilogue's statistics
// combine is conv3d.h's, shared with conv3d_f16s.hip.
#include <hip/hip_fp16.h>
#include <algorithm>

#include "conv3d.h"

namespace cf {
namespace {

struct PwParams {
    const float* x;       // [B,Cin,D,H,W]
    const float* bias;    // [Cout] or nullptr
    float* out;           // [B,Cout,Do,Ho,Wo]
    double* gn_ws;        // optional fused statistics of the output, [B][groups][2]
    int Cin, B, D, H, W, Cout, sd, stride, Do, Ho, Wo;
    float alpha;
    int gn_groups, gn_prezeroed;
    int nimg, tiles;      // samples per workgroup tile (>= 2: whole samples), tiles per sample (nimg == 1)
};

constexpr int NPX = 128;  // output voxels per workgroup

// tile voxel -> (sample, voxel of the sample); false: the slot is past the tile's samples, the batch or the sample
__device__ __forceinline__ bool decode(const PwParams& p, int b0, int q0, int P, int pidx, int& b, int& q) {
    const int img = p.nimg > 1 ? pidx / P : 0;
    b = b0 + img;
    q = q0 + pidx - img * P;
    return img < p.nimg && b < p.B && q < P;
}

template <int WM, int NTW, int NW>
__global__ void __launch_bounds__(64 * NW, 2) conv3d_pw_f16s_kernel(const PwParams p, const _Float16* __restrict__ wpk) {
    constexpr int CK = 16, KS = 2, REC = CK * 4 + 16, NSTAGE = 64 * NW, NGRP8 = KS * CK / 8;
    constexpr int MAXT = NPX * NGRP8 / NSTAGE;
    constexpr int BUF = KS * NPX * REC;
    static_assert(NPX * NGRP8 % NSTAGE == 0 && (NW / WM) * NTW * 32 == NPX, "tile shape");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int mt = blockIdx.y * WM + (wave % WM);     // 32-channel m-tile of this wave
    const int ngrp = wave / WM;                       // n-tile group of this wave

    const int HW = p.H * p.W, HoWo = p.Ho * p.Wo, P = p.Do * HoWo;
    const unsigned DHW = (unsigned)p.D * (unsigned)HW;
    const int bid = blockIdx.x;
    int b0, q0;
    if (p.nimg > 1) { b0 = bid * p.nimg; q0 = 0; }
    else { b0 = bid / p.tiles; q0 = (bid - b0 * p.tiles) * NPX; }
    const int nstep = (p.Cin + KS * CK - 1) / (KS * CK);

    // ---- staging tasks: (output voxel, 8-channel group of the step) -> 8 raw buffer loads, one hi and one lo 16-byte LDS slot.  Offsets are
    // 32-bit; slots past the tile and the zero-weight channel tail are parked at 2 GiB, where the descriptor's range check returns 0
    // (host: x and out of a launch < 2 GiB).
    constexpr unsigned OOB = 0x80000000u;
    unsigned t_off[MAXT], t_c[MAXT];
    int t_lds[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int task = tid + t * NSTAGE;
        const int grp = task / NPX, pidx = task - grp * NPX;
        t_c[t] = grp * 8;
        t_lds[t] = ((grp >> 1) * NPX + pidx) * REC + (grp & 1) * 16;
        t_off[t] = OOB;
        int b, q;
        if (decode(p, b0, q0, P, pidx, b, q)) {
            const int zo = q / HoWo, r = q - zo * HoWo;
            const int yo = r / p.Wo, xo = r - yo * p.Wo;
            t_off[t] = ((unsigned)b * p.Cin * DHW + (unsigned)(zo * p.sd) * HW + (unsigned)(yo * p.stride * p.W + xo * p.stride)) * 4u;
        }
    }
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)((long)p.B * p.Cin * DHW * 4), 0x00020000);
    const unsigned DHW4 = DHW * 4u;

    auto issue_loads = [&](int step, bool live, float (&stg)[MAXT][8]) {      // !live: every lane parked, no memory traffic
        const unsigned c0 = (unsigned)step * (KS * CK);
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const unsigned c = c0 + t_c[t];
            const unsigned v0 = t_off[t] + c * DHW4;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned off = (live && t_off[t] != OOB && c + (unsigned)j < (unsigned)p.Cin) ? v0 + (unsigned)j * DHW4 : OOB;
                stg[t][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
            }
        }
    };
    auto write_stage = [&](int buf, const float (&stg)[MAXT][8]) {
        unsigned char* base = lds + buf * BUF;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            f16x8 hi, lo;
            split8_f16(stg[t], hi, lo);
            *reinterpret_cast<f16x8*>(base + t_lds[t]) = hi;
            *reinterpret_cast<f16x8*>(base + t_lds[t] + CK * 2) = lo;
        }
    };

    float stg[MAXT][8];
    issue_loads(0, true, stg);

    f32x16 acc[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    // packed weights: fragment (mt, step, k-step, part) = 64 lanes x 8 halves
    const f16x8* wfrag = reinterpret_cast<const f16x8*>(wpk) + (long)mt * nstep * (KS * 2 * 64) + lane;
    f16x8 aH[KS], aL[KS], nH[KS] = {}, nL[KS] = {};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) { aH[ks] = wfrag[ks * 128]; aL[ks] = wfrag[ks * 128 + 64]; }
    write_stage(0, stg);
    __syncthreads();

    const int b_rec = (ngrp * NTW * 32 + l31) * REC + half * 16;
    for (int step = 0; step < nstep; ++step) {
        const bool more = step + 1 < nstep;
        if (more) {                                   // the last step prefetches nothing (uniform branch; the x loads are parked)
            const f16x8* wn = wfrag + (long)(step + 1) * (KS * 2 * 64);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) { nH[ks] = wn[ks * 128]; nL[ks] = wn[ks * 128 + 64]; }
        }
        issue_loads(step + 1, more, stg);
        const unsigned char* xb = lds + (step & 1) * BUF + b_rec;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const unsigned char* rp = xb + (ks * NPX + nt * 32) * REC;
                const f16x8 bh = *reinterpret_cast<const f16x8*>(rp);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(rp + CK * 2);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aL[ks], bh, acc[nt], 0, 0, 0);      // small terms first
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aH[ks], bl, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aH[ks], bh, acc[nt], 0, 0, 0);
            }
        }
        if (more) write_stage((step + 1) & 1, stg);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { aH[ks] = nH[ks]; aL[ks] = nL[ks]; }
    }

    // ---- epilogue: alpha * acc + bias, one store per element through a buffer resource over the output of this launch (< 2 GiB, host check)
    const bool do_stats = p.gn_ws != nullptr;
    float ssum[16], ssq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { ssum[r] = 0.f; ssq[r] = 0.f; }
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)((long)p.B * p.Cout * P * 4), 0x00020000);
    bool o_ok[NTW];
    unsigned o_off[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        int b, q;
        o_ok[nt] = decode(p, b0, q0, P, (ngrp * NTW + nt) * 32 + l31, b, q);
        o_off[nt] = o_ok[nt] ? ((unsigned)b * p.Cout * (unsigned)P + (unsigned)q) * 4u : 0u;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool co_ok = co < p.Cout;
        const float bv = (p.bias && co_ok) ? p.bias[co] : 0.f;
        const unsigned ochan = (unsigned)co * (unsigned)P * 4u;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            const bool ok = o_ok[nt] && co_ok;
            const float v = p.alpha * acc[nt][r] + bv;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs_out, ok ? o_off[nt] + ochan : OOB, 0, 0);
            const float m = ok ? v : 0.f;
            ssum[r] += m;
            ssq[r] += m * m;
        }
    }
    // the main loop ended on a barrier: the patch buffers are free for the combine; host: one sample per workgroup when gn_ws is set
    if (do_stats)
        conv3d_stats_combine<WM, NW>(ssum, ssq, reinterpret_cast<float*>(lds), tid, p.Cout, p.gn_groups, p.gn_ws + 2L * (long)b0 * p.gn_groups);
}

bool shape_ok(const PwParams& p) {
    return (p.sd == 1 || p.sd == 2) && (p.stride == 1 || p.stride == 2) && p.B > 0 && p.Cin > 0 && p.D > 0 && p.H > 0 && p.W > 0 && p.Cout > 0;
}

void fill(PwParams& p, int B, int Cin, int D, int H, int W, int Cout, int sd, int st) {
    p.x = p.bias = nullptr; p.out = nullptr; p.gn_ws = nullptr;
    p.B = B; p.Cin = Cin; p.D = D; p.H = H; p.W = W; p.Cout = Cout; p.sd = sd; p.stride = st;
    p.alpha = 1.f; p.gn_groups = 0; p.gn_prezeroed = 0; p.Do = p.Ho = p.Wo = 0; p.nimg = 1; p.tiles = 1;
    if (!shape_ok(p)) return;
    p.Do = (D - 1) / sd + 1;
    p.Ho = (H - 1) / st + 1;
    p.Wo = (W - 1) / st + 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Host half: the plan of one launch (pw_plan: pure host arithmetic naming the kernel variant, samples per workgroup, tiles per sample,
// grid and statistics route) and the plan of a call (pw_call: the sub-batch cut and the plans of its two part sizes, or why the call is
// declined).  cf_conv3d_pw_f16s_ok and cf_conv3d_pw_f16s both read pw_call; nothing else decides.
constexpr int PW_NW = 4;

// What one launch on a (sub-)batch will be: a pure function of the PwParams (no pointer is read); only a whole call is ever declined.
struct PwPlan {
    int wm;                      // the built variants: <WM, NTW> = <1, 1> for Cout <= 32, else <2, 2>
    int nimg, tiles;             // the kernel arguments of the same names
    unsigned grid_x, grid_y;
    bool fusable;                // the epilogue can accumulate the statistics: one sample per workgroup
};

PwPlan pw_plan(const PwParams& p) {
    PwPlan pl;
    const long P = (long)p.Do * p.Ho * p.Wo;
    pl.wm = p.Cout <= 32 ? 1 : 2;
    pl.nimg = 1; pl.tiles = (int)((P + NPX - 1) / NPX);
    if (2 * P <= NPX && p.B > 1) { pl.nimg = (int)std::min((long)p.B, NPX / P); pl.tiles = 1; }
    pl.grid_x = (unsigned)(pl.nimg > 1 ? (p.B + pl.nimg - 1) / pl.nimg : (long)p.B * pl.tiles);
    pl.grid_y = (unsigned)((p.Cout + 32 * pl.wm - 1) / (32 * pl.wm));
    pl.fusable = pl.nimg == 1;
    return pl;
}

// The plan of a call.  Samples per launch: x and the output of a launch each stay below 2 GiB (32-bit buffer offsets).
// A shape class on which the caller's composition measures faster would be declined here by a size threshold, as cf_conv3d_f16s_ok does.
// None is: on every trainer-width projection (32 -> 64 at 128^3 down to 320 -> 320 at 8^3, strides (2,2,2) and (1,2,2)) the kernel's
// median is 1.18x to 2.40x below the composition's (tools/resenc_bench.py, profiles/resenc_pw3d.txt).
CallPlan<PwPlan> pw_call(PwParams p) {
    CallPlan<PwPlan> c;
    if (!shape_ok(p)) { c.why = "strides 1|2 only"; return c; }
    if (conv_terms() != 3) { c.why = "only the three-term product is built"; return c; }
    const double per = 4.0 * std::max((double)p.Cin * p.D * p.H * p.W, (double)p.Cout * p.Do * p.Ho * p.Wo);
    c.parts = equal_parts(p.B, per >= 2147483648.0 ? 0 : (long)(2147483647.0 / per));
    if (c.parts.n < 1) { c.why = "one sample of x or out exceeds 2 GiB"; return c; }
    p.B = (int)c.parts.n;
    c.first = c.last = pw_plan(p);
    if (c.parts.last != c.parts.n) { p.B = (int)c.parts.last; c.last = pw_plan(p); }
    return c;
}

template <int WM, int NTW>
int launch_pw_shape(const PwParams& p, const PwPlan& pl, const void* wpk, hipStream_t s) {
    hipLaunchKernelGGL((conv3d_pw_f16s_kernel<WM, NTW, PW_NW>), dim3(pl.grid_x, pl.grid_y), dim3(64 * PW_NW), 0, s, p, reinterpret_cast<const _Float16*>(wpk));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string("conv3d_pw_f16s launch failed: ") + hipGetErrorString(e)); return CF_ERR_LAUNCH; }
    return CF_OK;
}

}  // namespace
}  // namespace cf

using namespace cf;

extern "C" int cf_conv3d_pw_f16s_ok(int B, int Cin, int D, int H, int W, int Cout, int stride_d, int stride_hw) {
    PwParams p;
    fill(p, B, Cin, D, H, W, Cout, stride_d, stride_hw);
    return pw_call(p).why ? 0 : 1;
}

extern "C" int cf_conv3d_pw_f16s(const float* x, const void* wpk, const float* bias, float* out, int B, int Cin, int D, int H, int W, int Cout,
                                 int stride_d, int stride_hw, float alpha, double* gn_ws, int gn_groups, void* stream) {
    CF_REQUIRE(x && wpk && out, "null pointer");
    CF_REQUIRE((reinterpret_cast<uintptr_t>(wpk) & 15) == 0, "packed weights must be 16-byte aligned");
    PwParams p;
    fill(p, B, Cin, D, H, W, Cout, stride_d, stride_hw);
    const CallPlan<PwPlan> call = pw_call(p);
    CF_REQUIRE(!call.why, "unsupported configuration B=%d Cin=%d D=%d H=%d W=%d Cout=%d stride (%d,%d,%d): %s (cf_conv3d_pw_f16s_ok)", B, Cin, D, H, W, Cout,
               stride_d, stride_hw, stride_hw, call.why);
    p.x = x; p.bias = bias; p.out = out; p.alpha = alpha;
    set_stats_request(p, gn_ws, gn_groups);
    CF_REQUIRE(!gn_ws || (p.gn_groups > 0 && Cout % p.gn_groups == 0), "bad GroupNorm statistics request");
    const long DHW = (long)D * H * W, DHWo = (long)p.Do * p.Ho * p.Wo;
    const hipStream_t s = as_stream(stream);
    // every part executes its plan; the statistics come from the fused epilogue where the plan can fuse them, else from norm.hip's pass
    return for_each_part(B, call, [&](long b0, int nb, const PwPlan& pl) {
        PwParams q = p;
        q.B = nb; q.nimg = pl.nimg; q.tiles = pl.tiles;
        q.x = x + b0 * Cin * DHW;
        q.out = out + b0 * Cout * DHWo;
        if (gn_ws) q.gn_ws = gn_ws + 2 * b0 * p.gn_groups;
        return launch_with_stats("conv3d_pw_f16s", q.gn_ws, q.gn_groups, q.gn_prezeroed, pl.fusable, q.out, nb, Cout, (int)DHWo, s, [&](double* ws) {
            q.gn_ws = ws;
            return pl.wm == 1 ? launch_pw_shape<1, 1>(q, pl, wpk, s) : launch_pw_shape<2, 2>(q, pl, wpk, s);
        });
    });
}
