// Internal interface of the implicit-GEMM convolution (conv.hip), shared with corr.hip (all-pairs GEMM).
#pragma once
#include "common.h"

namespace cf {

struct ConvParams {
    const float* x1;      // [B,C1,H,W]
    const float* x2;      // [B,C2,H,W] or nullptr
    const float* wt;      // [K][Cout] (+ b * w_bstride)
    const float* bias;    // [Cout] or nullptr
    const float* res;     // [B,Cout,Ho,Wo] or nullptr
    float* out;           // [B,out_ctotal,Ho*up,Wo*up]
    long w_bstride;
    int C1, C2, B, H, W, Cout, KH, KW, stride, pad_h, pad_w;
    int Ho, Wo;
    int out_ctotal, out_coff;
    int act;
    float alpha;
    int scatter2x2;       // 1: ConvTranspose k2s2 epilogue (GEMM row m = co*4 + dy*2 + dx)
    double* gn_ws;        // optional: accumulate GroupNorm statistics of the OUTPUT (sum, sum of squares per (sample, group))
    int gn_groups;
    int gn_prezeroed = 0;   // gn_ws is already zero (caller-managed pool)
    // optional: x1 is a raw convolution output whose normalisation + LeakyReLU has been deferred to this consumer (conv_f16s.hip,
    // vector staging only): per (sample, channel) {mean, scale, shift}, float [B][3][C1]; value = lrelu((x - mean) * scale + shift)
    const float* in_norm = nullptr;
    float in_slope = 1.0f;   // LeakyReLU slope; in_slope < 0 selects GELU (erf form) instead
    int terms = 3;          // f16-split kernels: 3 = hi/lo split, three MFMAs per k-step (f32-class, the default); 1 = hi x hi only ("mixed precision":
                            // operands rounded to fp16, fp32 accumulation -- the segmentation path under mixed_precision=True, cf_conv_terms)
    int profile_kid = -1;   // >= 0: time this launch under that profile id with `profile_work` instead of the conv's own id / flops
    double profile_work = 0.0;
};

// validates nothing; callers validate.  Returns CF_OK / CF_ERR_LAUNCH.
int launch_conv(const ConvParams& p, hipStream_t s);

// f16 hi/lo-split kernel (conv_f16s.hip)
int conv_terms();           // this thread's cf_conv_terms setting (1 | 3)
bool conv_f16s_supported(const ConvParams& p);
int launch_conv_f16s(const ConvParams& p, const _Float16* wpk, hipStream_t s);

// persistent software-pipelined variant of the f16-split kernel for short-K layers on large maps (conv_stream.hip); the caller zeroes p.gn_ws
bool conv_stream_applicable(const ConvParams& p);
int launch_conv_stream(const ConvParams& p, const _Float16* wpk, hipStream_t s);

// row Winograd F(2,3) form of the f16-split kernel for 3x3 / stride 1 layers with >= 128 output channels (conv_wino.hip); `wpk` is packed
// by cineflow.ops.pack_conv_weight_wino (NOT the direct kernels' packing)
bool conv_wino_applicable(const ConvParams& p);
int launch_conv_wino(const ConvParams& p, const _Float16* wpk, hipStream_t s);

// CorrVolume (radius 4, dilation 1 / 2 / 4) on the f16 MFMA in 2-D banded form (corr_mfma.hip); corr.hip keeps every other shape
bool corr_mfma_applicable(int C, int H, int W, int stride, const float* cur, const float* prev);
int launch_corr_volume_mfma(const float* cur, const float* prev, float* out, int B, int C, int H, int W, int stride, hipStream_t s);

// RAFT all-pairs volume + pyramid in one kernel (allpairs.hip); returns 1 when the shape is not one it is built for
int allpairs_pyramid_fused(const float* f1, const float* f2, float* pyr, int B, int C, int H, int W, int levels, hipStream_t stream);

// GroupNorm statistics pass (norm.hip): ws[2*(b*groups+g)] = sum, +1 = sum of squares, fp64
int launch_gn_stats(const float* x, double* ws, int B, int C, int HW, int groups, hipStream_t s);

// ---- host parts that the f16-split launchers share (conv_f16s.hip, conv_wino.hip, conv3d_f16s.hip, conv3d_pw_f16s.hip)

// The statistics request of an exported call: gn_groups < 0 declares gn_ws already zeroed.  P: any of the kernels' parameter structs.
template <class P>
inline void set_stats_request(P& p, double* gn_ws, int gn_groups) {
    p.gn_ws = gn_ws; p.gn_groups = gn_groups < 0 ? -gn_groups : gn_groups; p.gn_prezeroed = gn_groups < 0;
}

// A batch of which at most `max_per_launch` samples fit one launch (32-bit buffer offsets) is cut into the FEWEST parts that fit and the
// parts are made equal: n samples each, `last` (at most parts - 1 fewer) in the final one -- a greedy cut could leave a remainder of one
// sample, for which a plan picks another kernel shape than for the large parts.  n == 0: one sample is already too large.
struct Parts { long n, last; };
inline Parts equal_parts(long B, long max_per_launch) {
    if (max_per_launch < 1) return {0, 0};
    if (B <= max_per_launch) return {B, B};
    const long parts = (B + max_per_launch - 1) / max_per_launch;
    const long n = (B + parts - 1) / parts;
    return {n, B - (B - 1) / n * n};
}

// The plan of a whole call (3-D files): the cut and the plans of its two part sizes, or why the call is declined.  for_each_part runs
// part(first sample, samples, plan) on every part in turn.
template <class Plan>
struct CallPlan { Parts parts = {0, 0}; Plan first = {}, last = {}; const char* why = nullptr; };
template <class Plan, class F>
inline int for_each_part(long B, const CallPlan<Plan>& c, F part) {
    for (long b0 = 0; b0 < B; b0 += c.parts.n) {
        const bool tail = B - b0 < c.parts.n;
        if (const int rc = part(b0, (int)(tail ? c.parts.last : c.parts.n), tail ? c.last : c.first)) return rc;
    }
    return CF_OK;
}

// The statistics half of a launch.  `launch(ws)` runs the kernel with ws as the workspace of its epilogue: gn_ws when the plan can fuse the
// statistics -- they accumulate with atomics, so the workspace is zeroed first unless the caller handed out a slice of a pool it zeroed
// itself -- else null, and norm.hip's pass over the dense output [B, C, HW] follows the kernel.
template <class Launch>
inline int launch_with_stats(const char* family, double* gn_ws, int gn_groups, bool prezeroed, bool fusable, const float* out, int B, int C,
                             int HW, hipStream_t s, Launch launch) {
    const bool fused = gn_ws && fusable;
    if (fused && !prezeroed && hipMemsetAsync(gn_ws, 0, sizeof(double) * 2 * (size_t)B * gn_groups, s) != hipSuccess) {
        set_error(std::string(family) + ": memset failed");
        return CF_ERR_LAUNCH;
    }
    const int rc = launch(fused ? gn_ws : nullptr);
    if (rc != CF_OK || !gn_ws || fused) return rc;
    return launch_gn_stats(out, gn_ws, B, C, HW, gn_groups, s);
}

}  // namespace cf
