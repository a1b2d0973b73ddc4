// nn.Conv3d forward as ONE implicit GEMM on the f16 MFMA (v_mfma_f32_32x32x16_f16), with the 3-term hi/lo operand split of conv_f16s.hip
// (same numerics, same split-exact contract: x = hi + lo, a*b ~= al*bh + ah*bl + ah*bh, weights scaled by an exact 2^s at pack time).
//
//     D[co][b, zo, oy, ox] = sum_{ci, dz, ky, kx} W[co][ci][dz][ky][kx] * X[b, ci, zo*sd + dz - kd/2, oy*s + ky - 1, ox*s + kx - 1]
//
// Kernel (kd, 3, 3) with kd in {1, 3}, padding (kd/2, 1, 1), stride (sd, s, s) with sd, s in {1, 2} independently: every convolution of
// Generic_UNet3D but its (1,1,1) heads.
//   * Layout: x1 / x2 / out are read and written in place as NCDHW (channel stride D*H*W): no plane re-layout, no concatenation of the
//     decoder's cat(up, skip) -- chunks below c1_pad read x1, the others x2 (split-aware packing, as in 2-D).
//   * k order = (channel chunk of 16, depth tap, in-plane tap, channel in chunk); K = chunks x kd x 9 x 16 in ONE accumulation: the output
//     is written exactly once, with alpha * acc + bias and the fused InstanceNorm / GroupNorm statistics.
//   * Schedule: one output-plane tile per workgroup, outer loop over (chunk, depth tap) "steps".  A step stages the 16-channel patch of the
//     input plane zo*sd + dz - kd/2 through LDS -- per-pixel [hi c0..16) | lo c0..16) | 16 B pad] records at the conflict-free 80-byte
//     pitch, stride 2 de-interleaved by column parity -- double-buffered with one barrier per step, and runs the 9 in-plane taps on it.
//     A depth tap whose input plane lies outside [0, D) for every output plane of the workgroup is not a step at all (workgroup-, hence
//     wave-uniform): with one plane per workgroup -- every map larger than a tile -- no zero plane is ever staged or multiplied.
//   * Small maps: a workgroup tile holds up to 8 whole (sample, output plane) pairs (the NIMG of conv_f16s.hip), so the bottleneck stages
//     still fill their n-tiles; a pair whose depth tap is out of range while a neighbour's is not reads zeros for it.  The fused
//     statistics (summed in a fixed order: run-to-run identical) need every pair of a workgroup in one sample; otherwise the statistics pass of norm.hip runs after the kernel.
//   * Weights: host-packed fragment order [m-tile][chunk][dz][ky*3+kx][hi/lo][lane][8], 1 KiB per fragment, one coalesced dwordx4 per lane
//     from L1/L2 through a 3-slot register ring prefetched two taps ahead (conv_f16s.hip's register-fragment path).
// Only the 3-term product is built: under cf_conv_terms(1) cf_conv3d_f16s_ok answers 0 and the caller keeps its 2-D composition.
// Host half (below the kernel): one plan per launch and one per call, read by the probe and the launcher alike; the epilogue's statistics
// combine is conv3d.h's, shared with conv3d_pw_f16s.hip.
#include <hip/hip_fp16.h>
#include <algorithm>

#include "conv3d.h"
#include "profile.h"

namespace cf {
namespace {

struct C3Params {
    const float* x1;      // [B,C1,D,H,W]
    const float* x2;      // [B,C2,D,H,W] or nullptr
    const float* bias;    // [Cout] or nullptr
    float* out;           // [B,Cout,Do,Ho,Wo]
    double* gn_ws;        // optional fused statistics of the output, [B][groups][2]
    int C1, C2, B, D, H, W, Cout, KD, sd, stride, Do, Ho, Wo;
    float alpha;
    int gn_groups, gn_prezeroed;
};

struct C3Geom {
    int TW, TH, NIMG;        // output tile of a workgroup: NIMG (sample, plane) pairs x TH rows x TW cols
    int PH, PW, PWR, pwh;    // staged patch rows / cols per pair, LDS row pitch in records, stride 2: records of the odd columns start at pwh
    int tiles_x, tiles_y, bgroups, nchunk, c1_pad;
    unsigned m_tx, m_ty, m_nrec, m_phpw, m_pw, m_thtw, m_tw, m_do;      // floor(2^32 / d) + 1 multipliers of the index decodes
};

template <int WM, int NTW, int MAXT, int NW>
__global__ void __launch_bounds__(64 * NW, (NTW <= 2 && MAXT <= 3) ? 4 : 2)
conv3d_f16s_kernel(const C3Params p, const C3Geom g, const _Float16* __restrict__ wpk) {
    constexpr int CK = 16, REC = CK * 4 + 16, NG = CK / 8, NSTAGE = 64 * NW, NTAP = 9;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int mt = blockIdx.y * WM + (wave % WM);     // 32-channel m-tile of this wave
    const int ngrp = wave / WM;                       // n-tile group of this wave

    const int bid = blockIdx.x;
    const int t2 = fdiv(bid, g.tiles_x, g.m_tx);
    const int tx = bid - t2 * g.tiles_x;
    const int bg = fdiv(t2, g.tiles_y, g.m_ty);
    const int ty = t2 - bg * g.tiles_y;
    const int x0 = tx * g.TW, y0 = ty * g.TH, bz0 = bg * g.NIMG;      // bz = b * Do + zo
    const int NBZ = p.B * p.Do;
    const int HW = p.H * p.W, HoWo = p.Ho * p.Wo;
    const int pd = p.KD >> 1;
    const int iy_org = y0 * p.stride - 1, ix_org = x0 * p.stride - 1;
    const int nrec = g.NIMG * g.PH * g.PW;
    const int buf_bytes = g.NIMG * g.PH * g.PWR * REC;

    // ---- depth taps that reach an input plane for at least one pair of this workgroup (uniform): the others are never staged or multiplied
    int nv = 0, dzpack = 0;                           // dzpack: the valid taps, two bits each, in ascending order
    for (int dz = 0; dz < p.KD; ++dz) {
        bool any = false;
        for (int img = 0; img < g.NIMG; ++img) {
            const int bz = bz0 + img;
            if (bz >= NBZ) break;
            const int zo = bz - fdiv(bz, p.Do, g.m_do) * p.Do;
            any = any || (unsigned)(zo * p.sd + dz - pd) < (unsigned)p.D;
        }
        if (any) { dzpack |= dz << (2 * nv); ++nv; }
    }
    const int nsteps = g.nchunk * nv;                 // nv >= 1: the centre tap always lands inside

    // ---- staging tasks: (pair, patch pixel, 8-channel group) -> 8 raw buffer loads, one hi and one lo 16-byte LDS slot.  Offsets are 32-bit;
    // padding pixels, pairs past the batch, planes outside [0, D) and the zero-weight channel tail are parked at 2 GiB, where the
    // descriptor's range check returns 0 (host: every tensor of a launch < 2 GiB).
    constexpr unsigned OOB = 0x80000000u;
    unsigned t_o1[MAXT], t_o2[MAXT], t_g8[MAXT];
    int t_lds[MAXT], t_z[MAXT];
    const unsigned DHW = (unsigned)p.D * (unsigned)HW;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        t_o1[t] = OOB; t_o2[t] = OOB; t_g8[t] = 0; t_lds[t] = -1; t_z[t] = 0;
        const int task = tid + t * NSTAGE;
        const int grp = fdiv(task, nrec, g.m_nrec);
        const int pr = task - grp * nrec;
        if (grp < NG) {
            const int img = fdiv(pr, g.PH * g.PW, g.m_phpw);
            const int q = pr - img * (g.PH * g.PW);
            const int py = fdiv(q, g.PW, g.m_pw), px = q - py * g.PW;
            const int iy = iy_org + py, ix = ix_org + px;
            const int bz = bz0 + img;
            const int pxs = g.pwh ? (px >> 1) + (px & 1) * g.pwh : px;
            t_lds[t] = ((img * g.PH + py) * g.PWR + pxs) * REC + grp * 16;
            t_g8[t] = grp * 8;
            if (bz < NBZ && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                const int b = fdiv(bz, p.Do, g.m_do), zo = bz - b * p.Do;
                const unsigned sp = (unsigned)(iy * p.W + ix);
                t_o1[t] = ((unsigned)b * p.C1 * DHW + sp) * 4u;
                t_o2[t] = ((unsigned)b * p.C2 * DHW + sp) * 4u;
                t_z[t] = zo * p.sd - pd;
            }
        }
    }
    const __amdgpu_buffer_rsrc_t rsrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x1), 0, (int)((long)p.B * p.C1 * DHW * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc2 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x2 ? p.x2 : p.x1), 0, p.x2 ? (int)((long)p.B * p.C2 * DHW * 4) : 0, 0x00020000);
    const unsigned HW4 = (unsigned)HW * 4u, DHW4 = DHW * 4u;

    auto issue_loads = [&](int chunk, int dz, float (&stg)[MAXT][8]) {
        const int c0 = chunk * CK;
        const bool in1 = c0 < g.c1_pad;
        const unsigned cb = (unsigned)(in1 ? c0 : c0 - g.c1_pad);
        const unsigned clim = (unsigned)(in1 ? p.C1 : p.C2);
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const int zi = t_z[t] + dz;
            const bool zok = (unsigned)zi < (unsigned)p.D;
            const unsigned v0 = (in1 ? t_o1[t] : t_o2[t]) + (cb + t_g8[t]) * DHW4 + (unsigned)zi * HW4;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned off = (zok && cb + t_g8[t] + (unsigned)j < clim) ? v0 + (unsigned)j * DHW4 : OOB;
                const unsigned raw = in1 ? __builtin_amdgcn_raw_buffer_load_b32(rsrc1, off, 0, 0) : __builtin_amdgcn_raw_buffer_load_b32(rsrc2, off, 0, 0);
                stg[t][j] = __builtin_bit_cast(float, raw);
            }
        }
    };
    auto write_stage = [&](int buf, const float (&stg)[MAXT][8]) {
        unsigned char* base = lds + buf * buf_bytes;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t_lds[t] < 0) continue;
            f16x8 hi, lo;
            split8_f16(stg[t], hi, lo);
            *reinterpret_cast<f16x8*>(base + t_lds[t]) = hi;
            *reinterpret_cast<f16x8*>(base + t_lds[t] + CK * 2) = lo;
        }
    };

    float stg[MAXT][8];
    issue_loads(0, dzpack & 3, stg);

    int b_rec[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int pidx = (ngrp * NTW + nt) * 32 + l31;
        int img = fdiv(pidx, g.TH * g.TW, g.m_thtw);
        const int q = pidx - img * (g.TH * g.TW);
        int tyy = fdiv(q, g.TW, g.m_tw), txx = q - tyy * g.TW;
        if (img >= g.NIMG) { img = 0; tyy = 0; txx = 0; }
        b_rec[nt] = ((img * g.PH + tyy * p.stride) * g.PWR + txx * (g.pwh ? 1 : p.stride)) * REC + half * 16;
    }

    f32x16 acc[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    // packed weights: fragment (mt, chunk, dz, tap, part) = 64 lanes x 8 halves
    const f16x8* wfrag = reinterpret_cast<const f16x8*>(wpk) + (long)mt * g.nchunk * p.KD * (NTAP * 2 * 64) + lane;
    auto wstep = [&](int chunk, int j) { return wfrag + (long)(chunk * p.KD + ((dzpack >> (2 * j)) & 3)) * (NTAP * 2 * 64); };
    constexpr int R = 3, DPF = R - 1;                 // fragment ring, prefetched DPF taps ahead (NTAP % R == 0 keeps the slots static)
    f16x8 aH[R] = {}, aL[R] = {};
    const f16x8* wc = wstep(0, 0);
#pragma unroll
    for (int s = 0; s < DPF; ++s) { aH[s] = wc[s * 128]; aL[s] = wc[s * 128 + 64]; }
    write_stage(0, stg);
    __syncthreads();

    int c_cur = 0, j_cur = 0;
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        int c_n = c_cur, j_n = j_cur;                 // the next step (the last one prefetches itself again: L1/L2 hits, unconditional loads)
        if (more) { if (++j_n == nv) { j_n = 0; ++c_n; } }
        const f16x8* wn = wstep(c_n, j_n);
        const unsigned char* xb = lds + (step & 1) * buf_bytes;
#pragma unroll
        for (int tap = 0; tap < NTAP; ++tap) {
            {
                const f16x8* wp = tap + DPF < NTAP ? wc + (tap + DPF) * 128 : wn + (tap + DPF - NTAP) * 128;
                aH[(tap + DPF) % R] = wp[0];
                aL[(tap + DPF) % R] = wp[64];
            }
            if (tap == 0) issue_loads(c_n, (dzpack >> (2 * j_n)) & 3, stg);
            __builtin_amdgcn_sched_barrier(0);
            const int ky = tap / 3, kx = tap % 3;
            const int toff = (ky * g.PWR + (g.pwh ? (kx >> 1) + (kx & 1) * g.pwh : kx)) * REC;
            const f16x8 ah = aH[tap % R], al = aL[tap % R];
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const unsigned char* rp = xb + b_rec[nt] + toff;
                const f16x8 bh = *reinterpret_cast<const f16x8*>(rp);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(rp + CK * 2);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[nt], 0, 0, 0);      // small terms first
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[nt], 0, 0, 0);
            }
        }
        if (more) write_stage((step + 1) & 1, stg);
        __syncthreads();
        wc = wn; c_cur = c_n; j_cur = j_n;
    }

    // ---- epilogue: alpha * acc + bias, one store per element through a buffer resource over the output of this launch (< 2 GiB, host check)
    const bool do_stats = p.gn_ws != nullptr;
    float ssum[16], ssq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { ssum[r] = 0.f; ssq[r] = 0.f; }
    const unsigned DoHoWo = (unsigned)p.Do * (unsigned)HoWo;
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)((long)p.B * p.Cout * DoHoWo * 4), 0x00020000);
    bool o_ok[NTW];
    unsigned o_off[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        int pidx = (ngrp * NTW + nt) * 32 + l31;
        asm volatile("" : "+v"(pidx));                // keep the address math below the main loop
        int img = fdiv(pidx, g.TH * g.TW, g.m_thtw);
        const int q = pidx - img * (g.TH * g.TW);
        int tyy = fdiv(q, g.TW, g.m_tw), txx = q - tyy * g.TW;
        const bool in_tile = img < g.NIMG;
        if (!in_tile) { img = 0; tyy = 0; txx = 0; }
        const int bz = bz0 + img, oy = y0 + tyy, ox = x0 + txx;
        o_ok[nt] = in_tile && bz < NBZ && oy < p.Ho && ox < p.Wo;
        const int b = fdiv(bz, p.Do, g.m_do), zo = bz - b * p.Do;
        o_off[nt] = (((unsigned)b * p.Cout * p.Do + (unsigned)zo) * (unsigned)HoWo + (unsigned)(oy * p.Wo + ox)) * 4u;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool co_ok = co < p.Cout;
        const float bv = (p.bias && co_ok) ? p.bias[co] : 0.f;
        const unsigned ochan = (unsigned)co * DoHoWo * 4u;
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
        conv3d_stats_combine<WM, NW>(ssum, ssq, reinterpret_cast<float*>(lds), tid, p.Cout, p.gn_groups,
                                     p.gn_ws + 2L * (long)fdiv(bz0, p.Do, g.m_do) * p.gn_groups);
}

// ---------------------------------------------------------------------------------------------------------------------
// Host half: the table of built instantiations (CF_C3_SHAPES), the plan of one launch (c3_plan: pure host arithmetic naming table row,
// geometry, grid, LDS size and statistics route, or why the shape is declined) and the plan of a call (c3_call: the sub-batch cut and the
// plans of its two part sizes).  cf_conv3d_f16s_ok and cf_conv3d_f16s both read c3_call; nothing else decides.
// Every <WM, NTW, MAXT> that is built (WM m-tiles x NTW pixel tiles per wave, staging tasks per thread; four waves each), in the order
// row = 2 * (in-plane stride 2) + (Cout <= 32): 64 channels x 128 pixels at in-plane stride 1, 64 x 64 at stride 2 (its patch is four times
// the tile), 32-channel x 128-pixel forms of both for Cout <= 32.  The launch functions are instantiated from this table and from nothing else.
#define CF_C3_SHAPES(X) X(2, 2, 2) X(1, 1, 2) X(2, 1, 3) X(1, 1, 5)
constexpr int C3_NW = 4;
struct C3Shape { int WM, NTW, MAXT; };
#define CF_C3_ROW(...) {__VA_ARGS__},
constexpr C3Shape k_c3_shapes[] = {CF_C3_SHAPES(CF_C3_ROW)};
#undef CF_C3_ROW

// What one launch on a (sub-)batch will be: a pure function of the C3Params (no pointer is read).
struct C3Plan {
    int shape = -1;              // row of k_c3_shapes
    C3Geom g = {};               // the kernel's geometry argument, complete
    unsigned grid_x = 0, grid_y = 0;
    size_t lds_bytes = 0;        // dynamic LDS of the launch
    bool fusable = false;        // the epilogue can accumulate the statistics: every workgroup stays inside one sample
    const char* why = nullptr;   // declined: the reason
};
C3Plan c3_declined(const char* why) { C3Plan pl; pl.why = why; return pl; }

bool shape_ok(const C3Params& p) {
    return (p.KD == 1 || p.KD == 3) && (p.sd == 1 || p.sd == 2) && (p.stride == 1 || p.stride == 2) && p.B > 0 && p.C1 > 0 && p.C2 >= 0 &&
           p.D > 0 && p.H > 0 && p.W > 0 && p.Cout > 0;
}

C3Plan c3_plan(const C3Params& p) {
    C3Plan pl;
    const bool s2 = p.stride == 2;
    pl.shape = 2 * s2 + (p.Cout <= 32);
    const C3Shape t = k_c3_shapes[pl.shape];
    const int npx = (C3_NW / t.WM) * t.NTW * 32, nstage = 64 * C3_NW;      // output pixels and staging threads of a workgroup
    const int NBZ = p.B * p.Do;
    C3Geom& g = pl.g;
    g.TW = std::min(p.Wo, 32);
    g.TH = std::min(npx / g.TW, p.Ho);
    g.NIMG = (g.TH == p.Ho && g.TW == p.Wo) ? std::max(1, std::min(npx / (g.TH * g.TW), std::min(8, NBZ))) : 1;
    g.PH = (g.TH - 1) * p.stride + 3; g.PW = (g.TW - 1) * p.stride + 3;
    while (g.NIMG > 1 && (g.NIMG * g.PH * g.PW * 2 + nstage - 1) / nstage > t.MAXT) --g.NIMG;
    if ((g.NIMG * g.PH * g.PW * 2 + nstage - 1) / nstage > t.MAXT) return c3_declined("a tall one-column tile: the staging budget does not hold its patch");
    g.PWR = g.PW; g.pwh = 0;
    if (s2) { g.pwh = (g.PW + 1) / 2; g.PWR = 2 * g.pwh; }
    g.tiles_x = (p.Wo + g.TW - 1) / g.TW; g.tiles_y = (p.Ho + g.TH - 1) / g.TH;
    g.bgroups = (NBZ + g.NIMG - 1) / g.NIMG;
    g.c1_pad = p.C2 > 0 ? ((p.C1 + 15) / 16) * 16 : (1 << 30);
    g.nchunk = p.C2 > 0 ? g.c1_pad / 16 + (p.C2 + 15) / 16 : (p.C1 + 15) / 16;
    const long nwg = (long)g.tiles_x * g.tiles_y * g.bgroups;
    if (nwg >= (1L << 31) / std::max(g.tiles_x, g.tiles_y) || (long)NBZ >= (1L << 31) / p.Do) return c3_declined("grid too large for the index decode");
    g.m_tx = magic(g.tiles_x); g.m_ty = magic(g.tiles_y); g.m_nrec = magic(g.NIMG * g.PH * g.PW); g.m_phpw = magic(g.PH * g.PW);
    g.m_pw = magic(g.PW); g.m_thtw = magic(g.TH * g.TW); g.m_tw = magic(g.TW); g.m_do = magic(p.Do);
    const size_t tile_bytes = (size_t)2 * g.NIMG * g.PH * g.PWR * 80;
    if (tile_bytes > LDS_LIMIT) return c3_declined("LDS tile too large");
    pl.lds_bytes = std::max(tile_bytes, (size_t)C3_NW * 64 * sizeof(float));      // at least the statistics combine's slots
    pl.grid_x = (unsigned)nwg, pl.grid_y = (unsigned)((p.Cout + 32 * t.WM - 1) / (32 * t.WM));
    pl.fusable = g.NIMG == 1 || p.Do % g.NIMG == 0;
    return pl;
}

// Shapes the kernel can run but which the caller's composition of 2-D convolutions was measured to run faster (tools/conv3d_ab.py on the
// 3d_fullres cardiac plan, B = 1: profiles/conv3d_ab_parent.txt / conv3d_ab_this.txt): the probe declines them.
//   (a) no depth taps on a large map: the composition is then ONE launch of the tuned 2-D kernels (weights through LDS / the persistent
//       kernel), whose MFMA rate this register-fragment schedule does not reach (32 -> 32 at 20x256x224: 0.32 vs 0.50 ms);
//   (b) in-plane stride 2 at depth stride 1 on a large map: the composition needs no copies of strided plane slices there, and the
//       one-pixel-tile-per-wave stride-2 shape re-reads every weight fragment per 3 MFMAs (64 -> 128 at 20x128x112: 0.25 vs 0.29 ms);
//   (c) fewer than two workgroups per compute unit with a long K loop: every (chunk, depth tap) step exposes a global-load latency that
//       nothing else on the CU hides (320 -> 320 at 5x8x7, 60 steps: 0.18 vs 0.23 ms; 512 -> 256 at 10x32x28, 96 steps: 0.35 vs 0.39 ms).
bool composition_is_faster(const C3Params& p, const C3Plan& pl) {
    const long out_px = (long)p.Do * p.Ho * p.Wo;
    if (p.KD == 1 && out_px >= 65536) return true;
    if (p.stride == 2 && p.sd == 1 && out_px >= 65536) return true;
    return (long)pl.grid_x * pl.grid_y < 512 && pl.g.nchunk * p.KD > 24;
}

// The plan of a call.  Samples per launch: x1, x2 and the output of a launch each stay below 2 GiB (32-bit buffer offsets).
CallPlan<C3Plan> c3_call(C3Params p) {
    CallPlan<C3Plan> c;
    if (!shape_ok(p)) { c.why = "kernel (1|3,3,3) and strides 1|2 only"; return c; }
    if (conv_terms() != 3) { c.why = "only the three-term product is built"; return c; }
    const double dhw = (double)p.D * p.H * p.W, per = 4.0 * std::max({p.C1 * dhw, p.C2 * dhw, (double)p.Cout * p.Do * p.Ho * p.Wo});
    c.parts = equal_parts(p.B, per >= 2147483648.0 ? 0 : (long)(2147483647.0 / per));
    if (c.parts.n < 1) { c.why = "one sample of a tensor exceeds 2 GiB"; return c; }
    p.B = (int)c.parts.n;
    c.first = c.last = c3_plan(p);
    if (c.parts.last != c.parts.n) { p.B = (int)c.parts.last; c.last = c3_plan(p); }
    c.why = c.first.why ? c.first.why : c.last.why;
    return c;
}

// the probe's answer: null when the call has a plan and the composition is not the faster route for its first part, else the reason
const char* declined(const C3Params& p, const CallPlan<C3Plan>& c) {
    if (c.why) return c.why;
    return composition_is_faster(p, c.first) ? "the composition of 2-D convolutions is the faster route" : nullptr;
}

template <int WM, int NTW, int MAXT>
int launch_c3_shape(const C3Params& p, const C3Plan& pl, const _Float16* wpk, hipStream_t s) {      // not among the timed kernels
    return launch_lds<conv3d_f16s_kernel<WM, NTW, MAXT, C3_NW>>("conv3d_f16s", -1, 0.0, dim3(pl.grid_x, pl.grid_y), dim3(64 * C3_NW), pl.lds_bytes, s, p, pl.g, wpk);
}
#define CF_C3_ROW(...) launch_c3_shape<__VA_ARGS__>,
int (*const k_c3_launch[])(const C3Params&, const C3Plan&, const _Float16*, hipStream_t) = {CF_C3_SHAPES(CF_C3_ROW)};
#undef CF_C3_ROW

void fill(C3Params& p, int B, int C1, int C2, int D, int H, int W, int Cout, int KD, int sd, int st) {
    p.x1 = p.x2 = p.bias = nullptr; p.out = nullptr; p.gn_ws = nullptr;
    p.B = B; p.C1 = C1; p.C2 = C2; p.D = D; p.H = H; p.W = W; p.Cout = Cout; p.KD = KD; p.sd = sd; p.stride = st;
    p.alpha = 1.f; p.gn_groups = 0; p.gn_prezeroed = 0; p.Do = p.Ho = p.Wo = 0;
    if (!shape_ok(p)) return;
    p.Do = (D + 2 * (KD / 2) - KD) / sd + 1;
    p.Ho = (H - 1) / st + 1;
    p.Wo = (W - 1) / st + 1;
}

}  // namespace
}  // namespace cf

using namespace cf;

extern "C" int cf_conv3d_f16s_ok(int B, int C1, int C2, int D, int H, int W, int Cout, int KD, int KH, int stride_d, int stride_hw) {
    if (KH != 3) return 0;
    C3Params p;
    fill(p, B, C1, C2, D, H, W, Cout, KD, stride_d, stride_hw);
    return declined(p, c3_call(p)) ? 0 : 1;
}

extern "C" int cf_conv3d_f16s(const float* x1, int C1, const float* x2, int C2, const void* wpk, const float* bias, float* out, int B, int D, int H,
                              int W, int Cout, int KD, int KH, int KW, int stride_d, int stride_hw, float alpha, double* gn_ws, int gn_groups,
                              void* stream) {
    CF_REQUIRE(x1 && wpk && out, "null pointer");
    CF_REQUIRE(C1 > 0 && C2 >= 0 && (C2 == 0 || x2), "bad channel split C1=%d C2=%d", C1, C2);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(wpk) & 15) == 0, "packed weights must be 16-byte aligned");
    CF_REQUIRE(KH == 3 && KW == 3, "in-plane kernel %dx%d: only 3x3 is built", KH, KW);
    C3Params p;
    fill(p, B, C1, C2, D, H, W, Cout, KD, stride_d, stride_hw);
    const CallPlan<C3Plan> call = c3_call(p);
    const char* why = declined(p, call);
    CF_REQUIRE(!why, "unsupported configuration B=%d C=%d+%d D=%d H=%d W=%d Cout=%d kernel (%d,3,3) stride (%d,%d,%d): %s (cf_conv3d_f16s_ok)", B, C1, C2, D,
               H, W, Cout, KD, stride_d, stride_hw, stride_hw, why);
    p.x1 = x1; p.x2 = C2 ? x2 : nullptr; p.bias = bias; p.out = out; p.alpha = alpha;
    set_stats_request(p, gn_ws, gn_groups);
    CF_REQUIRE(!gn_ws || (p.gn_groups > 0 && Cout % p.gn_groups == 0), "bad GroupNorm statistics request");
    const long DHW = (long)D * H * W, DHWo = (long)p.Do * p.Ho * p.Wo;
    const hipStream_t s = as_stream(stream);
    // every part executes its plan; the statistics come from the fused epilogue where the plan can fuse them, else from norm.hip's pass
    return for_each_part(B, call, [&](long b0, int nb, const C3Plan& pl) {
        C3Params q = p;
        q.B = nb; q.x1 = x1 + b0 * C1 * DHW;
        if (q.x2) q.x2 = x2 + b0 * C2 * DHW;
        q.out = out + b0 * Cout * DHWo;
        if (gn_ws) q.gn_ws = gn_ws + 2 * b0 * p.gn_groups;
        return launch_with_stats("conv3d_f16s", q.gn_ws, q.gn_groups, q.gn_prezeroed, pl.fusable, q.out, nb, Cout, (int)DHWo, s, [&](double* ws) {
            q.gn_ws = ws;
            return k_c3_launch[pl.shape](q, pl, reinterpret_cast<const _Float16*>(wpk), s);
        });
    });
}
