// The epilogue part that the two native 3-D kernels share (conv3d_f16s.hip, conv3d_pw_f16s.hip): a wave holds NTW 32x32 MFMA accumulators
// over (32 output channels) x (32 output voxels), and wave = ngrp * WM + (m-tile within the workgroup).
#pragma once
#include "conv.h"

namespace cf {

// The fused-statistics combine of the epilogue.  ssum / ssq: the 16 per-register sums of this lane over its voxels; `red` is LDS that no wave still reads
// ([NW / WM][WM * 32 channels][2] floats), `ws` the statistics of the workgroup's sample (host: one sample per workgroup).
// Every wave owns a slot per channel and the slots are summed in a fixed order: the fp32 part of the sum does not depend on which wave
// arrives first (LDS atomics would make a repeated run differ in the last bit of a mean); the fp64 atomics that follow add fp32-valued
// terms, whose sum is exact in fp64 in any order while they span fewer than 29 binary orders of magnitude.
template <int WM, int NW>
__device__ __forceinline__ void conv3d_stats_combine(float (&ssum)[16], float (&ssq)[16], float* red, int tid, int cout, int gn_groups, double* ws) {
    constexpr int NGRP = NW / WM;
    const int lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int ngrp = wave / WM;
    xreduce16(ssum, lane);      // transpose-reduce as conv_f16s.hip: lane 2k holds channel register r(k)
    xreduce16(ssq, lane);
    if ((lane & 1) == 0) {
        const int r = ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
        const int cl = (wave % WM) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        red[2 * (ngrp * WM * 32 + cl)] = ssum[0];
        red[2 * (ngrp * WM * 32 + cl) + 1] = ssq[0];
    }
    __syncthreads();
    if (tid < WM * 32) {
        const int co = blockIdx.y * WM * 32 + tid;
        const int cpg = cout / gn_groups;
        if (co < cout && (tid == 0 || co % cpg == 0)) {      // one thread per (group, workgroup): the first channel of the group in this block
            int n = cpg - co % cpg;
            if (n > WM * 32 - tid) n = WM * 32 - tid;
            if (n > cout - co) n = cout - co;
            float s1 = 0.f, s2 = 0.f;
            for (int j = 0; j < n; ++j)
                for (int q = 0; q < NGRP; ++q) { s1 += red[2 * (q * WM * 32 + tid + j)]; s2 += red[2 * (q * WM * 32 + tid + j) + 1]; }
            double* w = ws + 2L * (co / cpg);
            atomicAdd(w, (double)s1);
            atomicAdd(w + 1, (double)s2);
        }
    }
}

}  // namespace cf
