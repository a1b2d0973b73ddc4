// Implicit-GEMM convolution on the f16 MFMA (v_mfma_f32_32x32x16_f16) with a 3-term "hi/lo" operand split:
//
//     x = hi + lo,   hi = fp16(x),   lo = fp16(x - hi)                             (22 significant bits per operand)
//     a*b ~= ah*bh + ah*bl + al*bh                                                 (al*bl ~ 2^-22 |a*b| dropped)
//
// Products of fp16 values are exact in the fp32 accumulator, so the result carries ~2^-22 relative operand error --
// two bits short of fp32 -- at 3 MFMAs per 16-deep k-step, i.e. up to 16/3 = 5.3x the rate of the exact fp32 MFMA
// (v_mfma_f32_32x32x2_f32, conv.hip).  fp16's narrow exponent is handled where it matters: the weights are scaled by
// an exact power of two at pack time (max|w| -> ~2^10, undone through alpha), so their lo halves stay normal; the
// activations this path sees are GroupNorm/LayerNorm/GELU outputs of O(1), whose lo halves lose at most 2^-25
// absolute (fp16 subnormal spacing) -- below the fp32 rounding of the sum.  Measured operand-level error on
// conv-shaped data: 7e-8 relative to max|y| vs 3e-7 for an fp32 conv; the recurrent flow network keeps
// its 1e-4 px EPE bar with a wide margin (tests/test_gpu_models.py), which bf16 splits (8-bit pieces) would not.
//
// GEMM view:  D[co][pixel] = sum_{tap, ci} W[co][ci][tap] * X[b, ci, oy*s + kh - p, ox*s + kw - p]
//   * k order = (channel chunk, tap, channel in chunk): one MFMA k-step = 16 consecutive channels at one tap, so a
//     lane's B fragment is 8 consecutive channels of ONE input pixel.
//   * the input patch of a workgroup is staged through LDS transposed on the fly: NCHW fp32 rows are read coalesced
//     along x (8 channels per thread), split into hi/lo halves and written as one 80-byte (CK=16) / 144-byte (CK=32)
//     record per pixel ([hi c0..CK) | lo c0..CK) | 16 B pad]); the odd multiple of 16 B makes every ds_read_b128 /
//     ds_write_b128 lane group hit 16 distinct 16-byte slots (conflict free).  The 3x3 halo is staged once per
//     workgroup, so HBM sees each input element ~1.3x per 64-channel output block.
//   * weights are packed on the host in exact fragment order (hi and lo planes), 1 KiB per (m-tile, chunk, tap, kstep,
//     part): an A fragment is one coalesced global_load_dwordx4 per lane from L1/L2 (all workgroups share them).
//   * double-buffered LDS, one barrier per chunk; global loads of chunk c+1 are issued before the MFMAs of chunk c and
//     converted/written after them (issue-early / write-late).
//   * wave tile: one 32-channel m-tile x NTW n-tiles of 32 pixels, one fp32 accumulator per tile.
#include <hip/hip_fp16.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

#include "conv.h"
#include "profile.h"

namespace cf {

CF_CLOCK_DECL(g_clock_f16s)

struct F16sGeom {
    int TW, TH, NIMG;        // output tile of a workgroup: NIMG images x TH rows x TW cols (NIMG*TH*TW <= NT_WG*32)
    int PH, PW;              // staged patch rows / cols per image
    int pstep;               // input step between patch pixels (1, or the stride for 1x1 convs)
    int ostep;               // patch step between output pixels (stride, or 1 for 1x1 convs)
    int tiles_x, tiles_y, bgroups;
    int nchunk;
    int ablate;              // ablation build only (CF_F16S_ABLATE): 1 = every chunk reads chunk 0's weight fragments (L1-resident), 2 = no fragment loads, 3 = no output stores
    int c1_pad;              // C1 rounded up to a multiple of CK: chunks below it read x1, the others x2 (the packed weights follow the same split)
    int NQ;                  // vector staging: 16-byte column quads per patch row (0: scalar staging)
    // magic multipliers floor(2^32/d)+1 for the index decodes (exact for n < 2^32/d; d == 1 handled apart): the kernel's setup was
    // ~8k ticks of integer division sequences, a tenth of a 4-chunk workgroup's life
    int PWR, pwh, kx1, kx2;  // LDS row pitch in records and the record offsets of taps kx = 1, 2 (stride 2: columns de-interleaved by parity)
    unsigned m_tx, m_ty, m_percg, m_phnq, m_nq, m_nrec, m_phpw, m_pw, m_thtw, m_tw;
};

// No range clamp: an activation beyond fp16's range (|x| >= 65520) becomes hi = inf, lo = NaN and poisons the output loudly, NaN and
// Inf inputs propagate as they do through an fp32 convolution (a clamp here saturated them silently and cost one VALU per element).
// Supported activation range: |x| < 65504, stated in include/cineflow.h.
// Every wave both stages the input patch and runs MFMAs.  vmcnt retires in issue order, so every wait for a weight fragment also waits
// for the staging loads issued before it (ablating those loads made the kernel 19-33 % faster); a design with dedicated loader waves
// removed that coupling and won 10-24 % on stride-2 layers and small maps, but lost 15-25 % on the large 3x3 layers that dominate the
// step, where the kernel is limited by bytes in flight; it was removed.
// WL = 1: the weight fragments go through LDS instead of straight from L1/L2 into registers.  Ablations (profiles/r02_conv_weight_path.md)
// showed that the per-wave fragment loads -- 2 KiB per k-step and wave, L1-resident or not -- cost 30-40 % of the kernel on every shape:
// the vector-memory return path (64 B/clk/CU) is what the MFMAs wait for.  With WL the workgroup fetches each fragment ONCE by LDS-DMA
// (global_load_lds_dwordx4, no VGPRs) into a two-slot ring of tap groups (3x3: one kernel row = 3 taps per slot) and every wave reads
// its A operands with ds_read_b128 (256 B/clk/CU); one barrier per group, the DMA of group q + 1 is in flight while group q is consumed.
#ifdef CF_F16S_ABLATION_BUILD
// per-phase clock sums over all waves (lane 0 of each): prologue, MFMA steps, write_stage, barrier wait, epilogue, waves
__device__ unsigned long long g_f16s_phase[9];   // [6..8]: epilogue split: scale + activation, coordinates + stores, statistics
#define F16S_CLK() __builtin_readcyclecounter()
#endif
// TERMS = 3: the hi/lo split (al*bh + ah*bl + ah*bh); TERMS = 1: ah*bh only -- operands rounded to fp16, fp32 accumulation: what the reference's
// fp16 autocast computes on the segmentation path (mixed_precision=True, nnunet/network_architecture/neural_network.py:140-146), selected per
// thread by cf_conv_terms(1).  Same staging, same packed weights (the lo planes are simply not multiplied).
template <int KH, int KW, int CK, int WM, int NTW, int MAXT, int NW, int VEC, int PRE, int WL, int TERMS>
__global__ void __launch_bounds__(64 * NW, NW == 8 ? 4 : ((NTW <= 2 && MAXT <= 3) ? 4 : 2))
conv_f16s_kernel(const ConvParams p, const F16sGeom g, const _Float16* __restrict__ wpk) {
    constexpr int KHW = KH * KW;           // taps: 3x3, 1x1, and the separable 1x5 / 5x1 of RAFT's SepConvGRU
    constexpr int KS = CK / 16;            // MFMA k-steps per tap per chunk
    constexpr int REC = CK * 4 + 16;       // bytes per pixel record
    constexpr int NT_WG = NTW * (NW / WM);  // n-tiles per workgroup (NW MFMA waves = WM m-tiles x NW/WM n-tile groups)
    constexpr int NG = CK / 8;             // 8-channel groups per record
    constexpr int NSTAGE = 64 * NW;        // threads that stage
    (void)NT_WG;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    CF_CLOCK_BEGIN();

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // wave-uniform by construction: keep it in an SGPR
#ifdef CF_F16S_ABLATION_BUILD
    const unsigned long long ph_t0 = F16S_CLK();
    unsigned long long ph_t1 = 0, ph_stage = 0, ph_bar = 0, ph_t2 = 0;
#endif
    const int half = lane >> 5, l31 = lane & 31;
    const int cw = wave % NW;                       // wave inside the workgroup
    const int mt = blockIdx.y * WM + (cw % WM);     // 32-channel m-tile of this wave
    const int ngrp = cw / WM;                       // n-tile group of this wave

    // ---- workgroup tile decode (XCD-banded so that vertically adjacent tiles share one L2)
    int bid = blockIdx.x;
    {
        const int nb = gridDim.x;
        int xcd = bid & 7, qn = nb >> 3, rn = nb & 7;
        bid = ((xcd < rn) ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (bid >> 3);
    }
    int t2 = fdiv(bid, g.tiles_x, g.m_tx);
    const int tx = bid - t2 * g.tiles_x;
    const int bg = fdiv(t2, g.tiles_y, g.m_ty);
    const int ty = t2 - bg * g.tiles_y;
    const int x0 = tx * g.TW, y0 = ty * g.TH, b0 = bg * g.NIMG;
    const int HW = p.H * p.W;
    const int HoWo = p.Ho * p.Wo;
    const int iy_org = y0 * p.stride - p.pad_h, ix_org = x0 * p.stride - p.pad_w;
    const int nrec = g.NIMG * g.PH * g.PW;
    const int buf_bytes = g.NIMG * g.PH * g.PWR * REC;
    const bool do_stats = p.gn_ws != nullptr;

    // =================================================================================================================
    // staging
    // =================================================================================================================
    // Inputs are read with raw buffer loads: the per-lane 32-bit byte offset of (sample, channel 0, iy, ix) is computed
    // once per task, the channel term is added per load, and the descriptor's range check returns 0 for (a) pixels
    // outside the image / batch, whose offset is parked at 2 GiB, and (b) channel reads past the end of the tensor.
    // (c) the padded channel tail of each input -- channels [C1, c1_pad) of x1 and [C2, ...) of x2, whose packed weights are exactly
    // zero: their loads are parked out of range too (issue_loads*), so a NaN / Inf in the NEXT sample's first channels cannot reach this
    // sample as NaN * 0.  Host checks: one sample of each tensor < 2 GiB (split-aware packing handles any C1 when x2 is present).
    constexpr unsigned OOB = 0x80000000u;
    unsigned t_o1[MAXT], t_o2[MAXT];  // byte offsets into x1 / x2 (OOB when invalid)
    int t_lds[MAXT];                  // byte offset of the 16-byte hi slot inside a buffer, -1: no task
    unsigned t_g8[MAXT];              // (8-channel group inside the chunk) * 8
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        t_o1[t] = OOB;
        t_o2[t] = OOB;
        t_lds[t] = -1;
        t_g8[t] = 0;
        int task = tid + t * NSTAGE;
        int grp = fdiv(task, nrec, g.m_nrec);
        int pr = task - grp * nrec;
        if (grp < NG) {
            int img = fdiv(pr, g.PH * g.PW, g.m_phpw);
            int q = pr - img * (g.PH * g.PW);
            int py = fdiv(q, g.PW, g.m_pw), px = q - py * g.PW;
            int iy = iy_org + py * g.pstep, ix = ix_org + px * g.pstep;
            int b = b0 + img;
            const int pxs = g.pwh ? (px >> 1) + (px & 1) * g.pwh : px;    // stride 2: even columns first, then the odd ones
            t_lds[t] = (((img * g.PH + py) * g.PWR) + pxs) * REC + grp * 16;
            t_g8[t] = grp * 8;
            if (b < p.B && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                const unsigned sp = (unsigned)(iy * p.W + ix);
                t_o1[t] = ((unsigned)b * p.C1 * HW + sp) * 4u;
                t_o2[t] = ((unsigned)b * p.C2 * HW + sp) * 4u;
            }
        }
    }
    const __amdgpu_buffer_rsrc_t rsrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x1), 0, (int)((long)p.B * p.C1 * HW * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc2 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x2 ? p.x2 : p.x1), 0, p.x2 ? (int)((long)p.B * p.C2 * HW * 4) : 0, 0x00020000);
    const unsigned HW4 = (unsigned)HW * 4u;

    // The loaded values stay RAW in registers until the LDS write (nothing consumes a load result early).
    auto issue_loads = [&](int chunk, float (&stg)[MAXT][8]) {
        const int c0 = chunk * CK;
        const bool in1 = c0 < g.c1_pad;                   // workgroup-uniform; c1_pad = C1 rounded up to whole chunks (split-aware packing)
        const unsigned cb = (unsigned)(in1 ? c0 : c0 - g.c1_pad);
        const unsigned clim = (unsigned)(in1 ? p.C1 : p.C2);   // channels at or past it are the zero-weight tail: never fetched (a select, not a branch)
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const unsigned v0 = (in1 ? t_o1[t] : t_o2[t]) + (cb + t_g8[t]) * HW4;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned off = (cb + t_g8[t] + (unsigned)j < clim) ? v0 + (unsigned)j * HW4 : OOB;
                const unsigned raw = in1 ? __builtin_amdgcn_raw_buffer_load_b32(rsrc1, off, 0, 0) : __builtin_amdgcn_raw_buffer_load_b32(rsrc2, off, 0, 0);
                stg[t][j] = __builtin_bit_cast(float, raw);
            }
        }
    };
    auto write_stage = [&](int chunk, const float (&stg)[MAXT][8]) {
        unsigned char* base = lds + (chunk & 1) * buf_bytes;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t_lds[t] < 0) continue;
            f16x8 hi, lo;
            split8_f16(stg[t], hi, lo);
            *reinterpret_cast<f16x8*>(base + t_lds[t]) = hi;
            *reinterpret_cast<f16x8*>(base + t_lds[t] + CK * 2) = lo;
        }
    };


    // ---- vector staging (VEC): task = 4 image columns aligned to 16 bytes x 4 channels -> 4 buffer_load_dwordx4 instead of 16
    // buffer_load_dword for the same 16 elements.  Time stamps in the correlation kernel showed ~150-240 cycles per vector-memory
    // instruction once the CU's address path back-pressures; the scalar staging issues 64 such instructions per workgroup and
    // chunk, this path 15.  Aligned quads never straddle the image border when W % 4 == 0, so a quad is either wholly inside
    // (one range-checked load) or wholly padding (offset parked at 2 GiB -> zeros); columns of a quad that lie outside the
    // patch are simply not written.  Host checks: stride 1, W % 4 == 0, 16-byte aligned tensors, one task per thread.
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    constexpr int VT = VEC ? VEC : 1;                                     // vector tasks per staging thread
    unsigned v_o1[VT], v_o2[VT], v_c4[VT], v_mask[VT];
    int v_lds[VT];
#pragma unroll
    for (int t = 0; t < VT; ++t) { v_o1[t] = OOB; v_o2[t] = OOB; v_c4[t] = 0; v_mask[t] = 0; v_lds[t] = 0; }
    if (VEC) {
        constexpr int NCG = CK / 4;
        const int xq0 = ix_org & ~3;
        const int per_cg = g.NIMG * g.PH * g.NQ;
#pragma unroll
        for (int t = 0; t < VT; ++t) {
            const int task = tid + t * NSTAGE;
            const int cg = fdiv(task, per_cg, g.m_percg);
            int r = task - cg * per_cg;
            if (cg < NCG) {
                const int img = fdiv(r, g.PH * g.NQ, g.m_phnq);
                r -= img * (g.PH * g.NQ);
                const int py = fdiv(r, g.NQ, g.m_nq), q = r - py * g.NQ;
                const int iy = iy_org + py, xq = xq0 + 4 * q, b = b0 + img;
                const int pxp = xq - ix_org;                              // patch column of the quad's first pixel (may be < 0)
#pragma unroll
                for (int k = 0; k < 4; ++k) v_mask[t] |= ((unsigned)(pxp + k) < (unsigned)g.PW) ? (1u << k) : 0u;
                v_lds[t] = ((img * g.PH + py) * g.PWR + pxp) * REC + cg * 8;
                v_c4[t] = cg * 4;
                if (b < p.B && (unsigned)iy < (unsigned)p.H && (unsigned)xq < (unsigned)p.W) {
                    const unsigned sp = (unsigned)(iy * p.W + xq);
                    v_o1[t] = ((unsigned)b * p.C1 * HW + sp) * 4u;
                    v_o2[t] = ((unsigned)b * p.C2 * HW + sp) * 4u;
                }
            }
        }
    }
    auto issue_loads_v = [&](int chunk, f32x4v (&stg)[VT][4]) {
        const int c0 = chunk * CK;
        const bool in1 = c0 < g.c1_pad;
        const unsigned cb = (unsigned)(in1 ? c0 : c0 - g.c1_pad);
        const unsigned clim = (unsigned)(in1 ? p.C1 : p.C2);
#pragma unroll
        for (int t = 0; t < VT; ++t) {
            const unsigned v0 = (in1 ? v_o1[t] : v_o2[t]) + (cb + v_c4[t]) * HW4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned off = (cb + v_c4[t] + (unsigned)j < clim) ? v0 + (unsigned)j * HW4 : OOB;
                stg[t][j] = in1 ? __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc1, off, 0, 0))
                                : __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc2, off, 0, 0));
            }
        }
    };
    // PRE: the input is a raw convolution output; its InstanceNorm / GroupNorm + LeakyReLU is applied here, between the load and the
    // hi/lo split: v = lrelu((v - mean) * scale + shift) with the per-channel triples of this sample staged once in LDS behind the two
    // patch buffers ([3][nchunk * CK] floats; channels past C1 hold zeros).  Padding quads (offset parked out of range) stay zero.
    const float* ctab = reinterpret_cast<const float*>(lds + 2 * buf_bytes);
    const int ctab_n = g.nchunk * CK;
    auto write_stage_v = [&](int chunk, const f32x4v (&stg)[VT][4]) {
#pragma unroll
        for (int t = 0; t < VT; ++t) {
            unsigned char* base = lds + (chunk & 1) * buf_bytes + v_lds[t];
            f32x4v cm = {0.f, 0.f, 0.f, 0.f}, ca = cm, cs = cm;
            const bool valid = v_o1[t] != OOB;
            if (PRE) {
                const int c0 = chunk * CK + (int)v_c4[t];
                cm = *reinterpret_cast<const f32x4v*>(ctab + c0);
                ca = *reinterpret_cast<const f32x4v*>(ctab + ctab_n + c0);
                cs = *reinterpret_cast<const f32x4v*>(ctab + 2 * ctab_n + c0);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!((v_mask[t] >> k) & 1u)) continue;
                f16x4 hi, lo;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = stg[t][j][k];
                    if (PRE) {
                        v[j] = (v[j] - cm[j]) * ca[j] + cs[j];
                        v[j] = p.in_slope < 0.f ? gelu_as(v[j]) : (v[j] > 0.f ? v[j] : v[j] * p.in_slope);
                        v[j] = valid ? v[j] : 0.f;
                    }
                }
                split4_f16(v[0], v[1], v[2], v[3], hi, lo);
                *reinterpret_cast<f16x4*>(base + k * REC) = hi;
                *reinterpret_cast<f16x4*>(base + k * REC + CK * 2) = lo;
            }
        }
    };

    // =================================================================================================================
    // MFMAs
    // =================================================================================================================
    // the first chunk's loads leave before the (division-heavy) output-coordinate setup below, which then overlaps their latency
    float stg0[MAXT][8];   // dead (eliminated) in the VEC instantiations
    f32x4v stgv[VT][4];
    if (VEC) issue_loads_v(0, stgv);
    else issue_loads(0, stg0);
    // ---- per-lane B-fragment record offsets and output coordinates of this wave's n-tiles
    int b_rec[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        int pidx = (ngrp * NTW + nt) * 32 + l31;
        int img = fdiv(pidx, g.TH * g.TW, g.m_thtw);
        int q = pidx - img * (g.TH * g.TW);
        int tyy = fdiv(q, g.TW, g.m_tw), txx = q - tyy * g.TW;
        if (img >= g.NIMG) { img = 0; tyy = 0; txx = 0; }
        b_rec[nt] = ((img * g.PH + tyy * g.ostep) * g.PWR + txx * (g.pwh ? 1 : g.ostep)) * REC + half * 16;
    }

    f32x16 acc1[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[nt][r] = 0.f;

    constexpr int NSTEP = KHW * KS;
    if constexpr (WL) {
        // ---- weights through LDS: ring of two slots, one slot = the fragments of G consecutive k-steps for the WM m-tiles of the workgroup
        constexpr int G = (KHW == 9) ? 3 : ((KHW == 1) ? NSTEP : 5);      // k-steps per group (3x3: one kernel row)
        constexpr int NGRP = NSTEP / G;
        static_assert(NGRP * G == NSTEP, "weight groups must tile the chunk");
        constexpr int WSLOT = WM * G * 2 * 1024;                          // bytes per slot
        unsigned char* wl = lds + 2 * buf_bytes + (PRE ? 3 * ctab_n * 4 : 0);
        const f16x8* wbase = reinterpret_cast<const f16x8*>(wpk) + lane;
        const int nq = g.nchunk * NGRP;
        // The DMA is issued from inline asm on purpose: hipcc tracks a __builtin_amdgcn_global_load_lds as a pending LDS write and puts
        // s_waitcnt vmcnt(0) in front of the next ds_read that may alias it -- i.e. it waited for group q + 1 before reading group q
        // (measured: 20 % of the kernel).  Hidden from the compiler, the DMAs only make ITS counted vmcnt waits stricter (vmcnt counts
        // every outstanding operation and retires in order), never weaker; their own completion is waited for explicitly below.
        auto issue_w = [&](int q) {       // group q = (chunk q / NGRP, steps (q % NGRP) * G ...): packed contiguously per m-tile
            const unsigned dst0 = (unsigned)(size_t)((__attribute__((address_space(3))) unsigned char*)(wl + (q & 1) * WSLOT));
            for (int f = wave; f < WM * G * 2; f += NW) {                 // wave-uniform
                const int m = f / (G * 2), j = f - m * (G * 2);
                const f16x8* src = wbase + (((long)(blockIdx.y * WM + m) * g.nchunk * NSTEP + (long)q * G) * 2 + j) * 64;
                const unsigned dst = __builtin_amdgcn_readfirstlane(dst0 + (unsigned)f * 1024u);
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
            }
        };
        issue_w(0);
        if (PRE) {
            float* ct = reinterpret_cast<float*>(lds + 2 * buf_bytes);
            for (int k = tid; k < 3 * ctab_n; k += 64 * NW) {
                const int which = k / ctab_n, c = k - which * ctab_n;
                ct[k] = c < p.C1 ? p.in_norm[((long)b0 * 3 + which) * p.C1 + c] : 0.f;
            }
            __syncthreads();
        }
        if (VEC) write_stage_v(0, stgv);
        else write_stage(0, stg0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // group 0's fragments have landed
        __syncthreads();
        const unsigned char* wa = wl + ((cw % WM) * G * 2) * 1024 + lane * 16;
        for (int c = 0; c < g.nchunk; ++c) {
            const bool more = c + 1 < g.nchunk;
            const unsigned char* xb = lds + (c & 1) * buf_bytes;
#pragma unroll
            for (int grp = 0; grp < NGRP; ++grp) {
                const int q = c * NGRP + grp;
                if (q + 1 < nq) issue_w(q + 1);
                if (grp == 0) {                   // unconditional (the last chunk re-reads itself), younger than the DMAs: the counted wait at the
                    const int cn = more ? c + 1 : c;      // end of this group leaves them in flight
                    if (VEC) issue_loads_v(cn, stgv);
                    else issue_loads(cn, stg0);
                }
                __builtin_amdgcn_sched_barrier(0);
                const unsigned char* ws = wa + (q & 1) * WSLOT;
#pragma unroll
                for (int sg = 0; sg < G; ++sg) {
                    const int step = grp * G + sg;
                    const int tap = step / KS, ks = step % KS;
                    const int ky = tap / KW, kx = tap % KW;
                    const int toff = (ky * g.PWR + (g.pwh ? (kx >> 1) + (kx & 1) * g.pwh : kx)) * REC;
                    const f16x8 ah = *reinterpret_cast<const f16x8*>(ws + (sg * 2) * 1024);
                    const f16x8 al = *reinterpret_cast<const f16x8*>(ws + (sg * 2 + 1) * 1024);
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) {
                        const unsigned char* rp = xb + b_rec[nt] + toff + ks * 32;
                        const f16x8 bh = *reinterpret_cast<const f16x8*>(rp);
                        const f16x8 bl = *reinterpret_cast<const f16x8*>(rp + CK * 2);
                        if constexpr (TERMS == 3) {
                            acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc1[nt], 0, 0, 0);
                            acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc1[nt], 0, 0, 0);
                        }
                        acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc1[nt], 0, 0, 0);
                    }
                }
                if (grp == NGRP - 1 && more) {
                    if (VEC) write_stage_v(c + 1, stgv);
                    else write_stage(c + 1, stg0);
                }
                // group q + 1's fragments must have landed before anyone reads them: vmcnt retires in order, so at the end of group 0 the
                // patch loads issued after the DMAs (VEC: 4 per task) may stay in flight
                if (VEC && grp == 0 && NGRP > 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(VEC * 4) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
        }
    } else {
    // packed weights: fragment (mt, chunk, tap, ks, part) = 64 lanes x 8 halves
    // A 1x5 / 5x1 layer of <= 32 output channels runs the two-m-tile shape (f16s_plan has no one-tile 1x5 shape) on weights that
    // pack_conv_weight_f16s packs as ONE m-tile: the second tile's waves, whose every store the epilogue drops (co >= Cout), take the first
    // tile's fragments -- their own would lie behind the end of the buffer (a read of nchunk * 20 KiB of whatever follows it, or of nothing).
    const int mtw = (KHW == 5 && p.Cout <= 32) ? 0 : mt;
    const f16x8* wfrag = reinterpret_cast<const f16x8*>(wpk) + (long)mtw * g.nchunk * (KHW * KS * 2) * 64 + lane;

    // A-fragment register ring, prefetched D steps ahead (NSTEP % R == 0 keeps the slots static).
    constexpr int R = (NSTEP % 3 == 0) ? 3 : 2;
    constexpr int D = R - 1;
    f16x8 aH[R] = {}, aL[R] = {};
    auto load_a = [&](int chunk, int step, int slot) {
#ifdef CF_F16S_ABLATION_BUILD          // timing experiments of profiles/r02_conv_weight_path.md: the run-time knob made every fragment load conditional
        if (g.ablate == 2) return;
        const f16x8* wc = wfrag + ((long)(g.ablate == 1 ? 0 : chunk) * NSTEP + step) * 2 * 64;
#else
        const f16x8* wc = wfrag + ((long)chunk * NSTEP + step) * 2 * 64;
#endif
        aH[slot] = wc[0];
        aL[slot] = wc[64];
    };

#pragma unroll
    for (int sidx = 0; sidx < D; ++sidx) load_a(0, sidx, sidx % R);
    if (PRE) {
        float* ct = reinterpret_cast<float*>(lds + 2 * buf_bytes);
        for (int k = tid; k < 3 * ctab_n; k += 64 * NW) {
            const int which = k / ctab_n, c = k - which * ctab_n;
            ct[k] = c < p.C1 ? p.in_norm[((long)b0 * 3 + which) * p.C1 + c] : 0.f;
        }
        __syncthreads();
    }
    if (VEC) write_stage_v(0, stgv);
    else write_stage(0, stg0);
    __syncthreads();
#ifdef CF_F16S_ABLATION_BUILD
    ph_t1 = F16S_CLK();
#endif

    for (int c = 0; c < g.nchunk; ++c) {
        const bool more = c + 1 < g.nchunk;
        const unsigned char* xb = lds + (c & 1) * buf_bytes;
#pragma unroll
        for (int step = 0; step < NSTEP; ++step) {
            const int tap = step / KS, ks = step % KS;
            // Prefetch the fragments of step + D (possibly the next chunk's first steps) and, at step 0, the next chunk's patch.  Every
            // load is UNCONDITIONAL (the last chunk re-reads itself: L1/L2 hits) and pinned here by a scheduling barrier.  Reading the
            // ISA of round 1's loop showed why the fragment loads cost 35-60 % (profiles/r02_conv_weight_path.md): with the loads
            // conditional (`if (more)`) hipcc's waitcnt pass merged the paths and waited vmcnt(0) -- for the patch loads it had just
            // issued -- and, unpinned, its scheduler sank each fragment load to one MFMA before its use; either way the two-step
            // prefetch did not exist.  Unconditional + pinned, the waits come out counted (vmcnt(N) leaves the younger loads in flight).
            const int cn = more ? c + 1 : c;
            if (step + D < NSTEP) load_a(c, step + D, (step + D) % R);
            else load_a(cn, step + D - NSTEP, (step + D) % R);
            if (step == 0) {
                if (VEC) issue_loads_v(cn, stgv);
                else issue_loads(cn, stg0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // record offset of tap (ky, kx); stride 2 stores the patch columns de-interleaved (even columns, then odd), so column
            // 2 * txx + kx sits at txx + (kx >> 1) + (kx & 1) * pwh
            const int ky = tap / KW, kx = tap % KW;      // compile-time after unrolling
            const int toff = (ky * g.PWR + (g.pwh ? (kx >> 1) + (kx & 1) * g.pwh : kx)) * REC;
            const f16x8 ah = aH[step % R], al = aL[step % R];
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const unsigned char* rp = xb + b_rec[nt] + toff + ks * 32;
                const f16x8 bh = *reinterpret_cast<const f16x8*>(rp);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(rp + CK * 2);
                // small terms first, then the main term, into one accumulator
                if constexpr (TERMS == 3) {
                    acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc1[nt], 0, 0, 0);
                    acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc1[nt], 0, 0, 0);
                }
                acc1[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc1[nt], 0, 0, 0);
            }
        }
#ifdef CF_F16S_ABLATION_BUILD
        const unsigned long long ph_a = F16S_CLK();
#endif
        if (more) {
            if (VEC) write_stage_v(c + 1, stgv);
            else write_stage(c + 1, stg0);
        }
#ifdef CF_F16S_ABLATION_BUILD
        const unsigned long long ph_b = F16S_CLK();
#endif
        __syncthreads();
#ifdef CF_F16S_ABLATION_BUILD
        ph_stage += ph_b - ph_a;
        ph_bar += F16S_CLK() - ph_b;
#endif
    }
#ifdef CF_F16S_ABLATION_BUILD
    ph_t2 = F16S_CLK();
#endif

    }

    // ---- epilogue (same fusion as conv.hip): value = act(alpha*acc + bias) + res  (alpha carries the weight scale 2^-s)
    // Optional fused GroupNorm / InstanceNorm statistics of the stored values (sum, sum of squares per (sample, group)):
    // per lane the NTW tiles are added per register (= channel), then a transpose-reduce over the 32 pixel lanes of the
    // half-wave (16 -> 8 -> 4 -> 2 -> 1 registers, 16 shuffles per quantity instead of 80) leaves each channel's total in
    // one lane pair, which adds it to the fp64 workspace.  Host guarantees one sample per workgroup (NIMG == 1).
    float ssum[16], ssq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { ssum[r] = 0.f; ssq[r] = 0.f; }
    // The epilogue is written as separate compact phases (scale+bias, ONE uniform switch over the activation, residual+store):
    // with the activation switch inside the per-element code the unrolled epilogue was ~40 KB of instructions, of which each
    // workgroup executes a sparse path once -- time stamps showed 28-34k ticks (a third of a 64-channel workgroup's life) spent
    // there, on instruction fetch.
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        float bv = 0.f;
        if (p.bias && co < p.Cout) bv = p.bias[p.scatter2x2 ? (co >> 2) : co];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc1[nt][r] = p.alpha * acc1[nt][r] + bv;
    }
    switch (p.act) {   // workgroup-uniform
        case CF_ACT_GELU:
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    acc1[nt][r] = act_apply(acc1[nt][r], CF_ACT_GELU);
                    __builtin_amdgcn_sched_barrier(0);   // one element at a time: these cold paths must not set the kernel's register count
                }
            break;
        case CF_ACT_RELU:
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    acc1[nt][r] = act_apply(acc1[nt][r], CF_ACT_RELU);
                    __builtin_amdgcn_sched_barrier(0);   // one element at a time: these cold paths must not set the kernel's register count
                }
            break;
        case CF_ACT_LRELU:
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    acc1[nt][r] = act_apply(acc1[nt][r], CF_ACT_LRELU);
                    __builtin_amdgcn_sched_barrier(0);   // one element at a time: these cold paths must not set the kernel's register count
                }
            break;
        case CF_ACT_TANH:
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    acc1[nt][r] = act_apply(acc1[nt][r], CF_ACT_TANH);
                    __builtin_amdgcn_sched_barrier(0);   // one element at a time: these cold paths must not set the kernel's register count
                }
            break;
        case CF_ACT_SIGMOID:
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    acc1[nt][r] = act_apply(acc1[nt][r], CF_ACT_SIGMOID);
                    __builtin_amdgcn_sched_barrier(0);   // one element at a time: these cold paths must not set the kernel's register count
                }
            break;
        default: break;
    }
    // output coordinates are derived here rather than ahead of the main loop: 4*NTW fewer registers live across it.
    // Stores go through a buffer resource over the NIMG output samples of this workgroup: one 32-bit add per store, and a pixel outside the
    // tile / a channel beyond Cout is an out-of-range offset (the store is dropped by the range check) instead of a branch around the store
    // and a 64-bit address per element.  Two parking values so that "both invalid" cannot wrap back into range; the host keeps
    // NIMG x (output sample bytes) below 1 GiB (f16s_finish).
    constexpr unsigned OOB_PX = 0x80000000u, OOB_CH = 0x40000000u;
    const unsigned up4 = p.scatter2x2 ? 4u : 1u;
    const unsigned osample = (unsigned)p.out_ctotal * (unsigned)HoWo * up4;                    // elements per output sample
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(
        p.out + ((long)b0 * p.out_ctotal + p.out_coff) * (long)HoWo * up4, 0,
        (int)(((unsigned)(b0 + g.NIMG <= p.B ? g.NIMG : p.B - b0) * osample - (unsigned)p.out_coff * (unsigned)HoWo * up4) * 4u), 0x00020000);
    bool o_ok[NTW];
    unsigned o_off[NTW];
    long r_off[NTW];
    auto out_coords = [&]() {
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            int pidx = (ngrp * NTW + nt) * 32 + l31;
            asm volatile("" : "+v"(pidx));                   // keep the address math below the main loop
            int img = fdiv(pidx, g.TH * g.TW, g.m_thtw);
            int q = pidx - img * (g.TH * g.TW);
            int tyy = fdiv(q, g.TW, g.m_tw), txx = q - tyy * g.TW;
            bool in_tile = img < g.NIMG;
            if (!in_tile) { img = 0; tyy = 0; txx = 0; }
            int b = b0 + img, oy = y0 + tyy, ox = x0 + txx;
            o_ok[nt] = in_tile && b < p.B && oy < p.Ho && ox < p.Wo;
            const unsigned px = p.scatter2x2 ? (unsigned)(2 * oy) * (unsigned)(2 * p.Wo) + 2u * ox : (unsigned)oy * p.Wo + ox;
            o_off[nt] = o_ok[nt] ? ((unsigned)img * osample + px) * 4u : OOB_PX;
            r_off[nt] = (long)b * p.Cout * HoWo + (long)oy * p.Wo + ox;
        }
    };
#ifdef CF_F16S_ABLATION_BUILD
    const unsigned long long ph_e1 = F16S_CLK();
#endif
    {
    out_coords();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool co_ok = co < p.Cout;
        unsigned ochan;
        if (p.scatter2x2) {
            const unsigned cr = (unsigned)co >> 2, dy = ((unsigned)co >> 1) & 1u, dx = (unsigned)co & 1u;
            ochan = (cr * (4u * HoWo) + dy * (2u * p.Wo) + dx) * 4u;
        } else {
            ochan = (unsigned)co * (unsigned)HoWo * 4u;
        }
        if (!co_ok) ochan = OOB_CH;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            const bool ok = o_ok[nt] && co_ok;
            float v = acc1[nt][r];
            if (p.res) { if (ok) v += p.res[r_off[nt] + (long)co * HoWo]; }   // rare (SingleConv / Linear residuals)
#ifdef CF_F16S_ABLATION_BUILD
            if (g.ablate != 3 || v == 12345.678f)      // CF_F16S_ABLATE=3: no output stores (upper bound of what hiding them could give)
#endif
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs_out, o_off[nt] + ochan, 0, 0);
            const float m = ok ? v : 0.f;
            ssum[r] += m;
            ssq[r] += m * m;
        }
    }
    }
#ifdef CF_F16S_ABLATION_BUILD
    const unsigned long long ph_e2 = F16S_CLK();
#endif
    if (do_stats) {
        xreduce16(ssum, lane);      // common.h: DPP + v_permlane16_swap, no LDS traffic
        xreduce16(ssq, lane);
        // workgroup-level combine in LDS (the staging buffers are free now), then ONE fp64 atomic pair per (group, workgroup):
        // thousands of workgroups adding to the same 8 groups of a sample would otherwise serialise at the memory side.
        // fp32 ends with the wave's per-channel totals: from here on the sums are fp64.  A map with |mean| / std of 6 .. 9 (a large bias)
        // loses two digits in E[x^2] - E[x]^2, and a workgroup total rounded to fp32 (2^-24 of the sum of squares) then shows as
        // 1e-5 .. 4e-5 on the normalised map (tests/test_gpu_deferred_norm_blocks.py, the offset rows).
        double* red = reinterpret_cast<double*>(lds);  // [WM*32 channels][2]
        __syncthreads();                              // every wave is done reading the last LDS buffer
        if (tid < WM * 64) red[tid] = 0.0;
        __syncthreads();
        if ((lane & 1) == 0) {
            const int r = ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
            const int cl = (cw % WM) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;  // channel inside the workgroup's block
            atomicAdd(&red[2 * cl], (double)ssum[0]);
            atomicAdd(&red[2 * cl + 1], (double)ssq[0]);
        }
        __syncthreads();
        if (tid < WM * 32 && b0 < p.B) {
            const int cb = blockIdx.y * WM * 32;
            const int co = cb + tid;
            const int cpg = p.Cout / p.gn_groups;
            if (co < p.Cout && (tid == 0 || co % cpg == 0)) {
                int n = cpg - co % cpg;               // channels of this group from co on
                if (n > WM * 32 - tid) n = WM * 32 - tid;
                if (n > p.Cout - co) n = p.Cout - co;
                double s1 = 0.0, s2 = 0.0;
                for (int j = 0; j < n; ++j) { s1 += red[2 * (tid + j)]; s2 += red[2 * (tid + j) + 1]; }
                double* w = p.gn_ws + 2L * ((long)b0 * p.gn_groups + co / cpg);
                atomicAdd(w, s1);
                atomicAdd(w + 1, s2);
            }
        }
    }
    CF_CLOCK_END(g_clock_f16s);
#ifdef CF_F16S_ABLATION_BUILD
    if (lane == 0 && ph_t1 && (blockIdx.x & 63) == 5) {   // a sample of the workgroups: same-address atomics from every wave would dominate the run
        const unsigned long long t3 = F16S_CLK();
        atomicAdd(&g_f16s_phase[0], ph_t1 - ph_t0);
        atomicAdd(&g_f16s_phase[1], (ph_t2 - ph_t1) - ph_stage - ph_bar);
        atomicAdd(&g_f16s_phase[2], ph_stage);
        atomicAdd(&g_f16s_phase[3], ph_bar);
        atomicAdd(&g_f16s_phase[4], t3 - ph_t2);
        atomicAdd(&g_f16s_phase[5], 1ULL);
        atomicAdd(&g_f16s_phase[6], ph_e1 - ph_t2);
        atomicAdd(&g_f16s_phase[7], ph_e2 - ph_e1);
        atomicAdd(&g_f16s_phase[8], t3 - ph_e2);
    }
#endif
}

// ---------------------------------------------------------------------------------------------------------------------
// Host half: the table of built instantiations (CF_F16S_SHAPES), the plan (f16s_plan: pure host arithmetic naming route, table row, geometry,
// grid and LDS size of one launch, or why it is declined) and the launcher that executes a plan (launch_conv_f16s_part).  The queries
// cf_conv2d_f16s_prenorm_ok and cf_conv2d_f16s_route ask the plan; nothing else decides.

// cf_conv_terms: per-thread product mode of the f16-split convolutions launched from this thread (3 = hi/lo split, 1 = hi x hi only)
static thread_local int t_conv_terms = 3;
int conv_terms() { return t_conv_terms; }

// Every <KH, KW, CK, WM, NTW, MAXT, NW, VEC, PRE, WL> that is built, each with TERMS = 3 and 1: the plan can only name a row of this table,
// and the launch functions are instantiated from it and from nothing else.
//   VEC: 1 for the 3x3 shapes (one 4x4 task per staging thread); the 1x5 / 5x1 shapes (CK = 32, wider patches) take 2.  1x1 layers measured
//        6-17 % slower with it -- their scalar loads are already whole rows -- so spatial kernels only; the stride-2 3x3 shapes, MAXT 3 and
//        5, never qualify at run time (two tasks per thread for their (2 TH + 1) x (2 TW + 1) patches: equal or 2 % slower, not built).
//   PRE: the stride-1 3x3 four-wave shapes are also built with the deferred input normalisation; not the 8-wave shape of the small maps
//        (< 1024 workgroups): its short workgroups lose more to the table fill + barrier than the apply pass costs (256 channels at 32x32,
//        B = 32: 192 us vs 120 + 15 us, tools/prenorm_ab.py).
#define CF_F16S_SHAPES(X)                                                                                                                \
    /* 3x3 stride 1: weights through LDS (8 waves, 256 pixels); register fragments, 4 waves x 32 / 64 / 128 channels; 128 channels, 8 waves */ \
    X(3, 3, 16, 1, 1, 2, 8, 1, 0, 1) X(3, 3, 16, 1, 1, 2, 8, 1, 1, 1) X(3, 3, 16, 2, 2, 2, 8, 1, 0, 1) X(3, 3, 16, 2, 2, 2, 8, 1, 1, 1)  \
    X(3, 3, 16, 1, 1, 2, 4, 0, 0, 0) X(3, 3, 16, 1, 1, 2, 4, 1, 0, 0) X(3, 3, 16, 1, 1, 2, 4, 1, 1, 0) X(3, 3, 16, 2, 2, 2, 4, 0, 0, 0)  \
    X(3, 3, 16, 2, 2, 2, 4, 1, 0, 0) X(3, 3, 16, 2, 2, 2, 4, 1, 1, 0) X(3, 3, 16, 4, 4, 2, 4, 0, 0, 0) X(3, 3, 16, 4, 4, 2, 4, 1, 0, 0)  \
    X(3, 3, 16, 4, 4, 2, 4, 1, 1, 0) X(3, 3, 16, 4, 2, 2, 8, 0, 0, 0) X(3, 3, 16, 4, 2, 2, 8, 1, 0, 0)                                   \
    /* 3x3 stride 2; 1x1 (also the transposed 2x2 convolution's GEMM); 1x5 / 5x1 of the SepConvGRU */                                    \
    X(3, 3, 16, 1, 1, 5, 4, 0, 0, 0) X(3, 3, 16, 2, 1, 3, 4, 0, 0, 0) X(3, 3, 16, 4, 2, 3, 4, 0, 0, 0)                                   \
    X(1, 1, 32, 1, 1, 2, 4, 0, 0, 0) X(1, 1, 32, 2, 2, 2, 4, 0, 0, 0) X(1, 1, 32, 4, 4, 2, 4, 0, 0, 0) X(1, 1, 32, 4, 2, 2, 8, 0, 0, 0)  \
    X(1, 5, 32, 2, 2, 4, 4, 0, 0, 0) X(1, 5, 32, 2, 2, 4, 4, 2, 0, 0) X(1, 5, 32, 4, 2, 4, 8, 0, 0, 0) X(1, 5, 32, 4, 2, 4, 8, 2, 0, 0)  \
    X(5, 1, 32, 2, 2, 4, 4, 0, 0, 0) X(5, 1, 32, 2, 2, 4, 4, 2, 0, 0) X(5, 1, 32, 4, 2, 4, 8, 0, 0, 0) X(5, 1, 32, 4, 2, 4, 8, 2, 0, 0)

struct F16sShape { int KH, KW, CK, WM, NTW, MAXT, NW, VEC, PRE, WL; };
#define CF_F16S_ROW(...) {__VA_ARGS__},
static constexpr F16sShape k_f16s_shapes[] = {CF_F16S_SHAPES(CF_F16S_ROW)};
#undef CF_F16S_ROW

enum { F16S_DECLINED = 0, F16S_KERNEL = 1, F16S_STREAM = 2 };

// What one launch on a (sub-)batch will be: a pure function of the ConvParams (pointers are read for their alignment, never dereferenced;
// p.terms is this thread's product mode) and of the cf_conv_stream_enable level.
struct F16sPlan {
    int route = F16S_DECLINED;
    int shape = -1;              // F16S_KERNEL: row of k_f16s_shapes
    F16sGeom g = {};             // F16S_KERNEL: the kernel's geometry argument, complete
    unsigned grid_x = 0, grid_y = 0;
    size_t lds_bytes = 0;        // dynamic LDS of the launch
    bool fusable = false;        // the epilogue can accumulate the GroupNorm statistics: one sample per workgroup, or the stream route
    const char* why = nullptr;   // F16S_DECLINED: the message for set_error
};
static F16sPlan f16s_declined(const char* why) { F16sPlan pl; pl.why = why; return pl; }

// kernel shapes of the f16-split kernel: 3x3 pad 1 and 1x1 pad 0 at stride 1 / 2, and the separable 1x5 (pad 0,2) / 5x1 (pad 2,0)
// convolutions of RAFT's SepConvGRU at stride 1
static int f16s_kind(const ConvParams& p) {
    if (p.KH == 3 && p.KW == 3 && p.pad_h == 1 && p.pad_w == 1 && (p.stride == 1 || p.stride == 2)) return 33;
    if (p.KH == 1 && p.KW == 1 && p.pad_h == 0 && p.pad_w == 0 && (p.stride == 1 || p.stride == 2)) return 11;
    if (p.KH == 1 && p.KW == 5 && p.pad_h == 0 && p.pad_w == 2 && p.stride == 1) return 15;
    if (p.KH == 5 && p.KW == 1 && p.pad_h == 2 && p.pad_w == 0 && p.stride == 1) return 51;
    return 0;
}

// The argument-level gate.  One sample of each input must stay below 2 GiB (32-bit buffer offsets); larger batches are split by f16s_parts.
bool conv_f16s_supported(const ConvParams& p) {
    if (p.w_bstride) return false;
    if (!f16s_kind(p)) return false;
    const long HW = (long)p.H * p.W;
    if ((long)p.C1 * HW * 4 >= (1L << 31) || (long)p.C2 * HW * 4 >= (1L << 31)) return false;
    // the epilogue's buffer-resource stores address the output samples of one workgroup with 32-bit offsets below 1 GiB (f16s_finish
    // checks the same with the plan's own images per workgroup: a backstop, no exported call gets past this gate with more):
    // up to 8 whole images per workgroup when an image fits one tile (<= 256 pixels), else one
    const double osample = (double)p.out_ctotal * p.Ho * p.Wo * (p.scatter2x2 ? 4.0 : 1.0) * 4.0;
    if (osample * ((long)p.Ho * p.Wo <= 256 ? 8.0 : 1.0) >= 1073741824.0) return false;
    return true;
}

// Cout % 128 == 0 takes the 128-channel workgroup shapes (the input patch is staged once per 128 output channels instead of once per 64),
// and so does a Cout whose last 128-channel block is at least three quarters full (the U-Net's 480 = 3 x 128 + 96): the packed weights
// are padded to whole 128-channel blocks anyway (pack_conv_weight_f16s: an even number of 64-channel pairs), the rows past Cout are zero
// weights whose stores the epilogue drops.
static bool f16s_cout_wide(int cout) { return cout % 128 == 0 || (cout > 128 && cout % 128 >= 96); }

// a deferred input normalisation beside the conditions of vector staging: a single input and a 4-byte aligned table
static bool f16s_pre_ok(const ConvParams& p) { return p.C2 == 0 && (reinterpret_cast<uintptr_t>(p.in_norm) & 3) == 0; }

// 16-byte column quads per patch row when the layer qualifies for vector staging (stride 1, W % 4 == 0, tile columns in whole quads,
// 16-byte aligned inputs), else 0
static int f16s_quads(const ConvParams& p, const F16sGeom& g) {
    if (p.stride != 1 || (p.W & 3) || (g.TW & 3) || ((reinterpret_cast<uintptr_t>(p.x1) | reinterpret_cast<uintptr_t>(p.x2)) & 15)) return 0;
    const int a = (-p.pad_w) & 3;                       // ix_org mod 4 (tile origins are multiples of 4)
    return ((a + g.PW - 1) >> 2) + 1;
}

// The staging form of a register-fragment shape: vector staging (t.VEC, g.NQ) when the layer qualifies and its 4x4 tasks fit VEC per staging
// thread, else scalar; the deferred input normalisation (t.PRE) where it is built.  Returns the reason when p.in_norm cannot be served.
static const char* f16s_staging(const ConvParams& p, F16sShape& t, F16sGeom& g) {
    const int KHW = t.KH * t.KW;
    const int nq = (KHW > 1 && !(KHW == 9 && t.MAXT > 2)) ? f16s_quads(p, g) : 0;       // CF_F16S_SHAPES: which shapes have a vector form
    const int tasks = (t.CK / 4) * g.NIMG * g.PH * nq;
    if (nq && KHW == 9 && tasks <= 64 * t.NW) {
        g.NQ = nq; t.VEC = 1; t.PRE = p.in_norm ? 1 : 0;
        const bool pre_built = t.MAXT == 2 && t.NW == 4 && g.NIMG == 1 && f16s_pre_ok(p);
        return p.in_norm && !pre_built ? "conv_f16s: deferred input normalisation is not built for this layer shape" : nullptr;
    }
    if (p.in_norm) return "conv_f16s: deferred input normalisation needs the vector staging path (3x3, stride 1, W % 4 == 0)";
    if (nq && KHW != 9 && tasks <= 2 * 64 * t.NW) { g.NQ = nq; t.VEC = 2; }
    return nullptr;
}

// Completes the plan of a chosen shape: the table row, the index-decode multipliers, every limit of the kernel, LDS size and grid.
static F16sPlan f16s_finish(const ConvParams& p, const F16sShape& t, F16sGeom g) {
    F16sPlan pl;
    for (int i = 0; i < (int)(sizeof(k_f16s_shapes) / sizeof(F16sShape)) && pl.shape < 0; ++i)
        if (memcmp(&k_f16s_shapes[i], &t, sizeof(F16sShape)) == 0) pl.shape = i;
    if (pl.shape < 0) return f16s_declined("conv_f16s: the dispatch named a kernel shape that is not built");
    const int REC = t.CK * 4 + 16;
    const int WGRP = (t.KH * t.KW == 9) ? 3 : ((t.KH * t.KW == 1) ? t.CK / 16 : 5);      // k-steps per LDS weight slot (kernel: G)
    const int NSTAGE = 64 * t.NW;
    const int nrec = g.NIMG * g.PH * g.PW;
    g.m_tx = magic(g.tiles_x);
    g.m_ty = magic(g.tiles_y);
    g.m_percg = magic(g.NIMG * g.PH * g.NQ);
    g.m_phnq = magic(g.PH * g.NQ);
    g.m_nq = magic(g.NQ);
    g.m_nrec = magic(nrec);
    g.m_phpw = magic(g.PH * g.PW);
    g.m_pw = magic(g.PW);
    g.m_thtw = magic(g.TH * g.TW);
    g.m_tw = magic(g.TW);
    if ((long)g.tiles_x * g.tiles_y * g.bgroups >= (1L << 31) / (g.tiles_x > g.tiles_y ? g.tiles_x : g.tiles_y))
        return f16s_declined("conv_f16s: grid too large for the index decode");
    if (!t.VEC && (nrec * (t.CK / 8) + NSTAGE - 1) / NSTAGE > t.MAXT) return f16s_declined("conv_f16s: staging tasks exceed MAXT");
    pl.fusable = g.NIMG == 1;
    pl.lds_bytes = (size_t)2 * g.NIMG * g.PH * g.PWR * REC + (t.PRE ? (size_t)3 * g.nchunk * t.CK * sizeof(float) : 0) +
                   (t.WL ? (size_t)2 * t.WM * WGRP * 2 * 1024 : 0);
    const size_t stats_lds = (size_t)t.WM * 64 * sizeof(double);      // the statistics epilogue's fp64 totals
    if (p.gn_ws && pl.fusable && pl.lds_bytes < stats_lds) pl.lds_bytes = stats_lds;
    if ((double)g.NIMG * p.out_ctotal * p.Ho * p.Wo * (p.scatter2x2 ? 4.0 : 1.0) * 4.0 >= 1073741824.0)
        return f16s_declined("conv_f16s: one workgroup's output samples must stay below 1 GiB (32-bit store offsets)");
    if (pl.lds_bytes > 160 * 1024) return f16s_declined("conv_f16s: LDS tile too large");
    pl.route = F16S_KERNEL;
    pl.g = g;
    pl.grid_x = (unsigned)(g.tiles_x * g.tiles_y * g.bgroups), pl.grid_y = (unsigned)((p.Cout + 32 * t.WM - 1) / (32 * t.WM));
    return pl;
}

// The plan of one launch on a batch whose inputs fit 32-bit buffer offsets (conv_f16s_supported(p) holds; f16s_parts cuts larger batches).
static F16sPlan f16s_plan(const ConvParams& p) {
    // short-K layers on large maps (<= 64 output channels, 3x3, stride 1, >= 1024 tiles): the persistent pipelined kernel of conv_stream.hip,
    // same arithmetic and packed weights (CF_CONV_STREAM=0 keeps this file's shapes: A/B knob)
    if (conv_stream_applicable(p)) { F16sPlan pl; pl.route = F16S_STREAM; pl.fusable = true; return pl; }
    const int kind = f16s_kind(p);
    const bool k3 = kind == 33, sep = kind == 15 || kind == 51, spatial = k3 || sep;      // sep: 1x5 / 5x1
    const int CK = k3 ? 16 : 32;
    const bool narrow = p.Cout <= 32, s2 = k3 && p.stride == 2;
    // Cout = 3 x 128 + 96 and the like ride on the 128-channel shapes with a partly empty last m-tile -- where the four-wave shape runs
    // (>= 1024 workgroups); a small launch keeps the 64-channel shapes (and with them the deferred input normalisation)
    bool cout_wide = f16s_cout_wide(p.Cout);
    if (cout_wide && p.Cout % 128 != 0 && !s2) {
        const int tw = std::min(p.Wo, 32), th = std::min(128 / tw, p.Ho);
        const long nwg = (long)((p.Wo + tw - 1) / tw) * ((p.Ho + th - 1) / th) * p.B * ((p.Cout + 127) / 128);
        if (nwg < 1024) cout_wide = false;
    }
    const bool wide = !s2 && cout_wide;
    // n-tiles (of 32 output pixels) per workgroup: 128-pixel tiles (64 for the stride-2 shapes of more than 32 channels) keep 4 waves
    // per SIMD to hide the staging latency; 256-pixel tiles at 2 waves/SIMD were 15-60 % slower and were removed
    const int NT_WG = (s2 && !narrow) ? 2 : 4;
    F16sGeom g = {};
    auto geometry = [&](int npx) {
    g.TW = std::min(p.Wo, 32);
    g.TH = std::min(npx / g.TW, p.Ho);
    g.NIMG = 1;      // several whole images per workgroup when one fits the tile: up to 8, and no more than the batch has
    if (g.TH == p.Ho && g.TW == p.Wo) g.NIMG = std::max(1, std::min(npx / (g.TH * g.TW), std::min(8, p.B)));
    g.pstep = spatial ? 1 : p.stride;      // a 1x1 layer takes its stride while staging: its patch is its tile
    g.ostep = spatial ? p.stride : 1;
    g.PH = spatial ? (g.TH - 1) * p.stride + p.KH : g.TH;
    g.PW = spatial ? (g.TW - 1) * p.stride + p.KW : g.TW;
    // keep the staging work within the per-thread task budget of the variant (MAXT x 256 eight-channel tasks)
    const int maxt = sep ? 4 : (s2 ? (narrow ? 5 : 3) : 2);
    const int nstage = (wide && !sep) ? 512 : 256;
    while (g.NIMG > 1 && (g.NIMG * g.PH * g.PW * (CK / 8) + nstage - 1) / nstage > maxt) --g.NIMG;
    // Stride 2: output-pixel lanes read every second input column; with plain row-major records (80 B apart) their 160-byte lane
    // stride lands 16 lanes on 8 of the 16 LDS slots (2-way conflicts on every B-fragment read).  The patch rows are therefore stored
    // de-interleaved -- even columns, then odd columns -- so a tap's 32 lanes read consecutive records again.
    g.PWR = g.PW; g.pwh = 0; g.kx1 = 1; g.kx2 = 2;
    if (s2) { g.pwh = (g.PW + 1) / 2; g.PWR = 2 * g.pwh; g.kx1 = g.pwh; g.kx2 = 1; }
    g.tiles_x = (p.Wo + g.TW - 1) / g.TW;
    g.tiles_y = (p.Ho + g.TH - 1) / g.TH;
    g.bgroups = (p.B + g.NIMG - 1) / g.NIMG;
    // split-aware chunking: x1's channels are padded to whole chunks (the packed weights carry zeros there), then x2's follow
    g.c1_pad = p.C2 > 0 ? ((p.C1 + CK - 1) / CK) * CK : (1 << 30);
    g.nchunk = p.C2 > 0 ? g.c1_pad / CK + (p.C2 + CK - 1) / CK : (p.C1 + CK - 1) / CK;
    };
    // The weights-through-LDS shapes come first (3x3, stride 1, not a 128-channel layer): 8 waves, 256 output pixels x 64 (or 32)
    // channels; they need one sample per workgroup and the vector staging path within one task per thread, else the register-fragment
    // shapes below take the layer -- as they do when the layer exceeds a limit of the kernel in this shape (their LDS footprint lacks
    // the 12 / 24 KiB weight ring, which decides for a deferred normalisation of ~13000 channels).
    // Measured (profiles/r02_conv_weight_path.md, B = 16): 64 -> 64 at 256x256 234 -> 263 TF, 32 -> 32 195 -> 205, 81 -> 64 208 -> 222; the
    // 128-channel form of it (4 m-tiles x 2 pixel tiles per wave, 8 waves) lost to the four-wave shape whose fragments feed 12 MFMAs
    // (128 -> 128 at 128x128: 294 vs 343 TF) and was removed.
    if (k3 && p.stride == 1 && !cout_wide) {
        geometry(256);
        g.NQ = g.NIMG == 1 ? f16s_quads(p, g) : 0;
        if (g.NQ && (16 / 4) * g.PH * g.NQ <= 64 * 8 && (!p.in_norm || f16s_pre_ok(p))) {
            const int wm = narrow ? 1 : 2;
            const F16sPlan pl = f16s_finish(p, F16sShape{3, 3, 16, wm, wm, 2, 8, 1, p.in_norm ? 1 : 0, 1}, g);
            if (pl.route != F16S_DECLINED) return pl;
        }
    }
    geometry(NT_WG * 32);
    g.NQ = 0;
    F16sShape t = {p.KH, p.KW, CK, 2, 2, 2, 4, 0, 0, 0};      // 64-channel workgroups: four waves, 2 m-tiles x 2 pixel groups
    if (sep) {
        // RAFT's SepConvGRU (384 -> 128 / 256 at 1/8 resolution): CK = 32 (10 k-steps per chunk keep the 2-slot fragment ring static);
        // 128-pixel tiles; 128-channel workgroups when Cout allows (8 waves: 4 m-tiles x 2 pixel groups), else 64-channel ones
        t.MAXT = 4;
        if (p.Cout % 128 == 0) { t.WM = 4; t.NW = 8; }
    } else if (wide) {
        // Two 128-channel shapes.  Four waves, each ONE m-tile x FOUR pixel tiles: a weight fragment feeds 12 MFMAs instead of 6, which
        // halves the per-wave weight re-reads from L1/L2 -- the resource the time stamps and the persistent-kernel experiment pointed at
        // (+9-15 % on the 128- and 256-channel layers at 64x64 and above); 148 VGPRs (no scratch under a 2-workgroup launch bound; a bound of 3 made the allocator spill 168 B/lane for the same speed), 3 waves/SIMD.  With few workgroups (32x32 maps)
        // the 8-wave shape (4 m-tiles x 2 pixel groups, 4 waves/SIMD) keeps more of the chip busy.  1x1 layers make the same choice.
        const long nwg = (long)g.tiles_x * g.tiles_y * g.bgroups * ((p.Cout + 127) / 128);
        const bool four = nwg >= 1024 && g.NIMG == 1 && (g.NIMG * g.PH * g.PW * (CK / 8) + 255) / 256 <= 2;
        t.WM = 4;
        if (four) t.NTW = 4; else t.NW = 8;
    } else if (narrow) {
        t.WM = t.NTW = 1;
        if (s2) t.MAXT = 5;      // stride-2 3x3 to <= 32 channels
    } else if (s2) {
        // stride 2 with Cout % 128 == 0: four m-tiles x two pixel tiles per wave -- every weight fragment is loaded once per workgroup and
        // feeds 6 MFMAs (the 64-channel shape: loaded twice, 3 MFMAs each)
        t.MAXT = 3;
        if (f16s_cout_wide(p.Cout)) t.WM = 4; else t.NTW = 1;
    }
    // An output map one or two columns wide (up to three for 1x5) gets a tile of up to 128 rows, whose patch -- (TH - 1) * stride + KH rows
    // of TW + 2 (1x5: TW + 4) columns -- is past the scalar staging budget of every shape (f16s_finish would decline it): such a tile
    // takes fewer rows until its patch fits.  The lanes past TH * TW idle, as they do on any map smaller than the tile.  Wider tiles
    // never get here, so no plan that was taken before changes.
    if (spatial && g.NIMG == 1) {
        const int nstage = 64 * t.NW, th0 = g.TH;
        while (g.TH > 1 && (g.PH * g.PW * (CK / 8) + nstage - 1) / nstage > t.MAXT) {
            --g.TH;
            g.PH = (g.TH - 1) * p.stride + p.KH;
        }
        if (g.TH != th0) g.tiles_y = (p.Ho + g.TH - 1) / g.TH;
    }
    if (const char* why = f16s_staging(p, t, g)) return f16s_declined(why);
    return f16s_finish(p, t, g);
}

// Executes the kernel route of a plan; what belongs to the launch stays here: the 160 KiB opt-in, the profile events, the ablation-build hooks.
template <int KH, int KW, int CK, int WM, int NTW, int MAXT, int NW, int VEC, int PRE, int WL>
static int launch_f16s_shape(const ConvParams& p, const F16sPlan& pl, const _Float16* wpk, hipStream_t s) {
    F16sGeom g = pl.g;
    size_t lds_bytes = pl.lds_bytes;
#ifdef CF_F16S_ABLATION_BUILD
    { static int ab = -1; if (ab < 0) { const char* e = getenv("CF_F16S_ABLATE"); ab = e ? atoi(e) : 0; } g.ablate = ab; }
    { static long pad = -1; if (pad < 0) { const char* e = getenv("CF_F16S_LDSPAD"); pad = e ? atol(e) : 0; }   // timing builds: fewer resident workgroups
      if (pad > (long)lds_bytes) lds_bytes = (size_t)pad; }
    if (lds_bytes > 160 * 1024) { set_error("conv_f16s: LDS tile too large"); return CF_ERR_ARG; }
#endif
    const dim3 grid(pl.grid_x, pl.grid_y), block(64 * NW);
    const double flops = 2.0 * (double)p.B * p.Ho * p.Wo * p.Cout * (p.C1 + p.C2) * p.KH * p.KW;
    if (p.terms == 1)
        return launch_lds<conv_f16s_kernel<KH, KW, CK, WM, NTW, MAXT, NW, VEC, PRE, WL, 1>>("conv_f16s", PK_CONV_F16S, flops, grid, block, lds_bytes, s, p, g, wpk);
    return launch_lds<conv_f16s_kernel<KH, KW, CK, WM, NTW, MAXT, NW, VEC, PRE, WL, 3>>("conv_f16s", PK_CONV_F16S, flops, grid, block, lds_bytes, s, p, g, wpk);
}

#define CF_F16S_ROW(...) launch_f16s_shape<__VA_ARGS__>,
static int (*const k_f16s_launch[])(const ConvParams&, const F16sPlan&, const _Float16*, hipStream_t) = {CF_F16S_SHAPES(CF_F16S_ROW)};
#undef CF_F16S_ROW

// Runs the convolution on a batch whose inputs fit 32-bit buffer offsets; when p.gn_ws is set the workspace ends up holding the
// GroupNorm statistics of the output -- from the fused epilogue when every workgroup covers a single sample, otherwise from the
// separate statistics pass.  (The transposed convolution's scatter fuses too: its GEMM rows are co * 4 + dy * 2 + dx, so a group of
// Cout / groups output channels is a run of 4 * Cout / groups consecutive rows -- the same `co / cpg` with cpg = p.Cout / groups.)
static int launch_conv_f16s_part(const ConvParams& p, const _Float16* wpk, hipStream_t s) {
    const F16sPlan pl = f16s_plan(p);
    if (pl.route == F16S_DECLINED) { set_error(pl.why); return CF_ERR_ARG; }
    const int up = p.scatter2x2 ? 2 : 1;
    const int cout = p.scatter2x2 ? p.Cout / 4 : p.Cout;
    return launch_with_stats(pl.route == F16S_STREAM ? "conv_stream" : "conv_f16s", p.gn_ws, p.gn_groups, p.gn_prezeroed, pl.fusable, p.out, p.B, cout,
                             p.Ho * up * p.Wo * up, s, [&](double* ws) -> int {
        if (pl.route == F16S_STREAM) return launch_conv_stream(p, wpk, s);
        ConvParams q = p; q.gn_ws = ws;
        const int rc = k_f16s_launch[pl.shape](q, pl, wpk, s);
        if (rc != CF_OK || !p.gn_ws || ws) return rc;
        if (p.out_coff != 0 || p.out_ctotal != cout) { set_error("conv_f16s: GroupNorm statistics need a dense output tensor"); return CF_ERR_ARG; }
        return CF_OK;
    });
}

// The kernel addresses its inputs with 32-bit buffer offsets (< 2 GiB per descriptor).  A batch whose input tensors are larger is
// cut into sub-batches HERE (same kernel, same numbers, a few more launches) instead of being handed to another kernel: the batch
// axis is the outermost one of every operand, so a sub-batch is a pointer offset.
// Plans are made per part of equal_parts' cut (conv.h): n samples, `last` in the remainder; n == 0: one sample of an input exceeds 2 GiB.
static Parts f16s_parts(const ConvParams& p) {
    if (conv_stream_applicable(p)) return {p.B, p.B};      // per-sample buffer resources: no 2 GiB limit on the batch
    const long HW = (long)p.H * p.W;
    const long per1 = (long)p.C1 * HW * 4, per2 = (long)p.C2 * HW * 4;
    return equal_parts(p.B, ((1L << 31) - 1) / (per1 > per2 ? per1 : per2));
}

int launch_conv_f16s(const ConvParams& p, const _Float16* wpk, hipStream_t s) {
    const long nb = f16s_parts(p).n;
    if (nb < 1) { set_error("conv_f16s: one sample of the input exceeds 2 GiB"); return CF_ERR_ARG; }
    const long HW = (long)p.H * p.W, HoWo = (long)p.Ho * p.Wo;
    const int up = p.scatter2x2 ? 2 : 1;
    for (long b0 = 0; b0 < p.B; b0 += nb) {      // one turn unless the inputs exceed 2 GiB
        ConvParams q = p;
        q.B = (int)(p.B - b0 < nb ? p.B - b0 : nb);
        q.x1 = p.x1 + b0 * p.C1 * HW;
        if (p.x2) q.x2 = p.x2 + b0 * p.C2 * HW;
        if (p.res) q.res = p.res + b0 * p.Cout * HoWo;
        q.out = p.out + b0 * p.out_ctotal * HoWo * up * up;
        if (p.gn_ws) q.gn_ws = p.gn_ws + 2 * b0 * p.gn_groups;
        if (p.in_norm) q.in_norm = p.in_norm + b0 * 3 * p.C1;
        if (const int rc = launch_conv_f16s_part(q, wpk, s)) return rc;
    }
    return CF_OK;
}

// The ConvParams of a plain call on a layer of this shape, in this thread's product mode: no tensors yet, dense output of Cout channels, no
// activation, no statistics.  The exports assign what they have by name.
static ConvParams f16s_layer(int B, int C1, int C2, int H, int W, int Cout, int KH, int KW, int stride, int pad_h, int pad_w) {
    ConvParams p;
    p.x1 = p.x2 = p.wt = p.bias = p.res = nullptr; p.out = nullptr; p.w_bstride = 0;
    p.C1 = C1; p.C2 = C2; p.B = B; p.H = H; p.W = W; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride;
    p.pad_h = pad_h; p.pad_w = pad_w; p.Ho = (H + 2 * pad_h - KH) / stride + 1; p.Wo = (W + 2 * pad_w - KW) / stride + 1;
    p.out_ctotal = Cout; p.out_coff = 0; p.act = CF_ACT_NONE; p.alpha = 1.f; p.scatter2x2 = 0;
    p.gn_ws = nullptr; p.gn_groups = 0; p.gn_prezeroed = 0;
    p.terms = conv_terms();
    return p;
}
// the transposed 2x2 / stride 2 convolution as the kernel sees it: a 1x1 GEMM to 4 * Cout rows (co, dy, dx), scattered by the epilogue
static ConvParams f16s_layer_transposed(int B, int Cin, int H, int W, int Cout) {
    ConvParams p = f16s_layer(B, Cin, 0, H, W, 4 * Cout, 1, 1, 1, 0, 0);
    p.scatter2x2 = 1; p.out_ctotal = Cout;
    return p;
}
static const char* const k_f16s_unsupported =
    "unsupported configuration for the f16-split kernel (3x3 pad 1 or 1x1 pad 0 at stride 1/2, 1x5 pad (0,2) or 5x1 pad (2,0) at stride 1; one sample < 2 GiB)";

// An address with the given low four bits for the queries, which have no tensors: the plan reads alignment only.
static const float* f16s_address(int low4) {
    alignas(16) static const unsigned char anchor[32] = {};
    return reinterpret_cast<const float*>(anchor + (low4 & 15));
}

}  // namespace cf

using namespace cf;

CF_CLOCK_READER(cf_debug_clock_f16s, cf::g_clock_f16s)

extern "C" int cf_conv_terms(int terms) {
    const int prev = t_conv_terms;
    if (terms == 1 || terms == 3) t_conv_terms = terms;
    return prev;
}

extern "C" int cf_conv2d_f16s(const float* x1, int C1, const float* x2, int C2, const void* wpk, const float* bias, const float* res,
                              float* out, int out_ctotal, int out_coff, int B, int H, int W, int Cout, int KH, int KW, int stride,
                              int pad_h, int pad_w, int act, float alpha, double* gn_ws, int gn_groups, void* stream) {
    CF_REQUIRE(x1 && wpk && out, "null pointer");
    CF_REQUIRE(C1 > 0 && C2 >= 0 && (C2 == 0 || x2), "bad channel split C1=%d C2=%d", C1, C2);
    CF_REQUIRE(B > 0 && H > 0 && W > 0 && Cout > 0, "bad shape B=%d H=%d W=%d Cout=%d", B, H, W, Cout);
    CF_REQUIRE(out_coff >= 0 && out_coff + Cout <= out_ctotal, "output channel slice out of range");
    CF_REQUIRE(act >= CF_ACT_NONE && act <= CF_ACT_SIGMOID, "bad activation %d", act);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(wpk) & 15) == 0, "packed weights must be 16-byte aligned");
    ConvParams p = f16s_layer(B, C1, C2, H, W, Cout, KH, KW, stride, pad_h, pad_w);
    p.x1 = x1; p.x2 = C2 ? x2 : nullptr; p.bias = bias; p.res = res; p.out = out;
    p.out_ctotal = out_ctotal; p.out_coff = out_coff; p.act = act; p.alpha = alpha;
    set_stats_request(p, gn_ws, gn_groups);
    CF_REQUIRE(!gn_ws || (p.gn_groups > 0 && Cout % p.gn_groups == 0 && out_coff == 0 && out_ctotal == Cout), "bad GroupNorm statistics request");
    CF_REQUIRE(p.Ho > 0 && p.Wo > 0, "empty output");
    CF_REQUIRE(conv_f16s_supported(p), "%s", k_f16s_unsupported);
    return launch_conv_f16s(p, reinterpret_cast<const _Float16*>(wpk), as_stream(stream));
}

// cf_conv2d_f16s whose input x is a RAW convolution output with its InstanceNorm / GroupNorm + LeakyReLU deferred to this consumer
// (the second convolution of a Generic_UNet stage): in_norm = float [B][3][C] {mean, scale, shift} from cf_group_norm_coef, applied
// as lrelu((x - mean) * scale + shift, in_slope) while the tile is staged -- the producer's apply pass (8 B per element) disappears.
// Built for 3x3 / stride 1 / pad 1 layers on the vector staging path (W % 4 == 0, one sample per workgroup, single input);
// cf_conv2d_f16s_prenorm_ok answers whether a shape qualifies (1) or not (0): every sub-batch's plan is a PRE shape or the stream route.
extern "C" int cf_conv2d_f16s_prenorm_ok(int B, int C, int H, int W, int Cout) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
    ConvParams p = f16s_layer(B, C, 0, H, W, Cout, 3, 3, 1, 1, 1);
    p.x1 = p.in_norm = f16s_address(0);
    if (!conv_f16s_supported(p)) return 0;
    const Parts parts = f16s_parts(p);
    if (parts.n < 1) return 0;
    for (const long b : {parts.n, parts.last}) {
        p.B = (int)b;
        const F16sPlan pl = f16s_plan(p);
        if (!(pl.route == F16S_STREAM || (pl.route == F16S_KERNEL && k_f16s_shapes[pl.shape].PRE))) return 0;
    }
    return 1;
}

extern "C" int cf_conv2d_f16s_prenorm(const float* x, int C, const float* in_norm, float in_slope, const void* wpk, const float* bias, float* out,
                                      int B, int H, int W, int Cout, float alpha, double* gn_ws, int gn_groups, void* stream) {
    CF_REQUIRE(x && wpk && out && in_norm, "null pointer");
    CF_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Cout > 0, "bad shape B=%d C=%d H=%d W=%d Cout=%d", B, C, H, W, Cout);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(wpk) & 15) == 0, "packed weights must be 16-byte aligned");
    ConvParams p = f16s_layer(B, C, 0, H, W, Cout, 3, 3, 1, 1, 1);
    p.x1 = x; p.bias = bias; p.out = out; p.alpha = alpha; p.in_norm = in_norm; p.in_slope = in_slope;
    set_stats_request(p, gn_ws, gn_groups);
    CF_REQUIRE(!gn_ws || (p.gn_groups > 0 && Cout % p.gn_groups == 0), "bad GroupNorm statistics request");
    CF_REQUIRE(conv_f16s_supported(p), "unsupported configuration for the f16-split kernel");
    return launch_conv_f16s(p, reinterpret_cast<const _Float16*>(wpk), as_stream(stream));
}

extern "C" int cf_conv_transpose2d_k2s2_f16s(const float* x, const void* wpk, const float* bias, float* out, int out_ctotal,
                                             int out_coff, int B, int Cin, int H, int W, int Cout, float alpha, double* gn_ws, int gn_groups,
                                             void* stream) {
    CF_REQUIRE(x && wpk && out, "null pointer");
    CF_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0, "bad shape");
    CF_REQUIRE(out_coff >= 0 && out_coff + Cout <= out_ctotal, "output channel slice out of range");
    CF_REQUIRE((reinterpret_cast<uintptr_t>(wpk) & 15) == 0, "packed weights must be 16-byte aligned");
    ConvParams p = f16s_layer_transposed(B, Cin, H, W, Cout);
    p.x1 = x; p.bias = bias; p.out = out; p.out_ctotal = out_ctotal; p.out_coff = out_coff; p.alpha = alpha;
    set_stats_request(p, gn_ws, gn_groups);
    CF_REQUIRE(!gn_ws || (p.gn_groups > 0 && Cout % p.gn_groups == 0 && out_coff == 0 && out_ctotal == Cout), "bad GroupNorm statistics request");
    CF_REQUIRE(conv_f16s_supported(p), "unsupported configuration for the f16-split kernel (one sample of the input must stay below 2 GiB)");
    return launch_conv_f16s(p, reinterpret_cast<const _Float16*>(wpk), as_stream(stream));
}

// The plan of the first sub-batch of a plain call (dense output, no activation, no residual), exported: include/cineflow.h.
extern "C" int cf_conv2d_f16s_route(int B, int C1, int C2, int H, int W, int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int x1_low4,
                                    int x2_low4, int prenorm, int transposed, int stats_groups, int* plan15) {
    if (plan15) memset(plan15, 0, 15 * sizeof(int));
    CF_REQUIRE(C1 > 0 && C2 >= 0 && B > 0 && H > 0 && W > 0 && Cout > 0 && stride > 0, "bad shape B=%d C=%d+%d H=%d W=%d Cout=%d", B, C1, C2, H, W, Cout);
    CF_REQUIRE(stats_groups >= 0 && (stats_groups == 0 || Cout % stats_groups == 0), "bad GroupNorm statistics request");
    ConvParams p = transposed ? f16s_layer_transposed(B, C1, H, W, Cout) : f16s_layer(B, C1, C2, H, W, Cout, KH, KW, stride, pad_h, pad_w);
    p.x1 = f16s_address(x1_low4);
    if (p.C2) p.x2 = f16s_address(x2_low4);
    if (prenorm && !transposed) { p.in_norm = f16s_address(0); p.in_slope = 0.01f; }
    static double stats;      // stands for a workspace: the plan asks only whether there is one
    if (stats_groups) set_stats_request(p, &stats, stats_groups);
    CF_REQUIRE(p.Ho > 0 && p.Wo > 0, "empty output");
    F16sPlan pl;
    Parts parts = {0, 0};
    if (!conv_f16s_supported(p)) {
        pl = f16s_declined(k_f16s_unsupported);
    } else {
        parts = f16s_parts(p);
        p.B = (int)parts.n;
        pl = parts.n < 1 ? f16s_declined("conv_f16s: one sample of the input exceeds 2 GiB") : f16s_plan(p);
    }
    if (pl.route == F16S_DECLINED) { set_error(pl.why); return F16S_DECLINED; }
    if (plan15) {
        const F16sShape t = pl.route == F16S_KERNEL ? k_f16s_shapes[pl.shape] : F16sShape{};
        const int nimg = pl.route == F16S_KERNEL ? pl.g.NIMG : 1;
        const int v[15] = {pl.route, t.KH, t.KW, t.CK, t.WM, t.NTW, t.MAXT, t.NW, t.VEC, t.PRE, t.WL, p.terms, nimg, pl.fusable, (int)parts.n};
        memcpy(plan15, v, sizeof(v));
    }
    return pl.route;
}

#ifdef CF_F16S_ABLATION_BUILD
// timing builds only: read and reset the per-phase clock sums
extern "C" int cf_debug_f16s_phases(unsigned long long* out9) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out9, HIP_SYMBOL(cf::g_f16s_phase), 9 * sizeof(unsigned long long));
    unsigned long long z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    hipMemcpyToSymbol(HIP_SYMBOL(cf::g_f16s_phase), z, sizeof(z));
    return 0;
}
#endif

// Test hook (tests/test_gpu_split.py; not in the header): common.h's split against the plain form it replaced, both on the same n values in
// one launch.  The plain form is kept HERE, as the statement of what the split has to equal bit for bit.
namespace cf {
namespace {
__global__ void __launch_bounds__(256) debug_split_kernel(const float* __restrict__ x, unsigned short* __restrict__ hi_old, unsigned short* __restrict__ lo_old,
                                                          unsigned short* __restrict__ hi_new, unsigned short* __restrict__ lo_new, long n) {
    const long npair = n >> 1;      // host: n even
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < npair; i += (long)gridDim.x * blockDim.x) {
        const float x0 = x[2 * i], x1 = x[2 * i + 1];
        const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1;
        const _Float16 l0 = (_Float16)(x0 - (float)h0), l1 = (_Float16)(x1 - (float)h1);
        hi_old[2 * i] = __builtin_bit_cast(unsigned short, h0);
        hi_old[2 * i + 1] = __builtin_bit_cast(unsigned short, h1);
        lo_old[2 * i] = __builtin_bit_cast(unsigned short, l0);
        lo_old[2 * i + 1] = __builtin_bit_cast(unsigned short, l1);
        f16x2 hn, ln;
        split2_f16(x0, x1, hn, ln);
        reinterpret_cast<unsigned*>(hi_new)[i] = __builtin_bit_cast(unsigned, hn);
        reinterpret_cast<unsigned*>(lo_new)[i] = __builtin_bit_cast(unsigned, ln);
    }
}
}  // namespace
}  // namespace cf

extern "C" int cf_debug_split_f16(const float* x, void* hi_old, void* lo_old, void* hi_new, void* lo_new, long n, void* stream) {
    CF_REQUIRE(x && hi_old && lo_old && hi_new && lo_new, "null pointer");
    CF_REQUIRE(n > 0 && n % 2 == 0, "n must be positive and even");
    CF_REQUIRE(((reinterpret_cast<uintptr_t>(hi_new) | reinterpret_cast<uintptr_t>(lo_new)) & 3) == 0, "outputs must be 4-byte aligned");
    hipLaunchKernelGGL(cf::debug_split_kernel, dim3(cf::flat_grid(n / 2, 256)), dim3(256), 0, cf::as_stream(stream), x,
                       static_cast<unsigned short*>(hi_old), static_cast<unsigned short*>(lo_old), static_cast<unsigned short*>(hi_new),
                       static_cast<unsigned short*>(lo_new), n);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
