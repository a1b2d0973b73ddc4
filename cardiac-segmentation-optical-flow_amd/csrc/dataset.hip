// Voxels by C-order rank among the voxels that match a predicate: the device work behind the training-side preprocessing drivers
// (nnunet/preprocessing/preprocessing.py:387-470 class locations `np.argwhere(seg == c)[idx]`, nnunet/experiment_planning/
// DatasetAnalyzer.py:160-170 foreground samples `modality[seg > 0][::10]`).
//   * count: the volume is cut into scan blocks of SCAN voxels (C order); one pass writes, per value of a short list (or for `> 0`), how
//     many voxels of every block match, a one-workgroup scan per row turns the counts into exclusive prefixes and leaves the row's total;
//   * select: one wave per requested rank.  The block is found by binary search in the prefix row, the voxel inside it by wave-wide
//     ballots: a ballot is 64 bits, its population count says whether the rank lies in these 64 voxels, and the lane whose own bit is set
//     with exactly `rank` set bits below it owns the voxel.  No atomics, no order dependence: the same bits on every run.
// A wave's reads of a block are 256 contiguous bytes (coalesced); the count pass reads every voxel once and is memory-bound.
#include "common.h"

namespace cf {

constexpr int SCAN = 256;              // voxels per scan block = threads per workgroup (four waves of 64)
constexpr int MAXV = 16;               // values per count pass

struct SelectValues { float v[MAXV]; };

__device__ __forceinline__ bool select_match(float k, int mode, float value) { return mode ? (k > 0.f) : (k == value); }

// counts[r * nb + b] = number of voxels of scan block b that match row r (row r: == vals.v[r], or the one row `> 0` of mode 1)
__global__ void __launch_bounds__(SCAN) select_count_kernel(const float* __restrict__ key, long n, int nb, SelectValues vals, int rows, int mode,
                                                            int* __restrict__ counts) {
    __shared__ int wc[SCAN / 64][MAXV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = blockIdx.x; b < nb; b += gridDim.x) {
        const long i = (long)b * SCAN + threadIdx.x;
        const bool in = i < n;
        const float k = in ? key[i] : 0.f;
        for (int r = 0; r < rows; ++r) {
            const int c = __popcll(__ballot(in && select_match(k, mode, vals.v[r])));
            if (lane == 0) wc[wave][r] = c;
        }
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < SCAN / 64; ++w) s += wc[w][threadIdx.x];
            counts[(long)threadIdx.x * nb + b] = s;
        }
        __syncthreads();
    }
}

// one workgroup per row: counts -> exclusive prefixes in place, totals[row] = the row's sum (below 2^31, as n is)
__global__ void __launch_bounds__(SCAN) select_scan_kernel(int* __restrict__ counts, int nb, long long* __restrict__ totals) {
    __shared__ int ws[SCAN / 64];
    int* row = counts + (long)blockIdx.x * nb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nb; base += SCAN) {
        const int i = base + threadIdx.x;
        const int c = i < nb ? row[i] : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) ws[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SCAN / 64; ++w) {
            if (w < wave) before += ws[w];
            all += ws[w];
        }
        if (i < nb) row[i] = carry + before + incl - c;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// one wave per rank.  prefix: the exclusive prefixes of the predicate's row.  A rank at or past the total (the caller's contract forbids
// it) finds no voxel and yields coordinates -1 / the value 0: every write goes to slot k of the outputs, never past them.
__global__ void __launch_bounds__(SCAN) select_rank_kernel(const float* __restrict__ key, long n, int nb, int mode, float value,
                                                           const int* __restrict__ prefix, const long long* __restrict__ ranks, int K,
                                                           const float* __restrict__ src, float* __restrict__ vals, long long* __restrict__ coords,
                                                           int D1, int D2) {
    const int lane = threadIdx.x & 63;
    const long k = (long)blockIdx.x * (SCAN / 64) + (threadIdx.x >> 6);
    if (k >= K) return;                                  // whole waves leave together: the ballots below see full waves
    const long long want = ranks[k];
    // last block whose prefix is <= want (prefix[0] = 0; blocks without a match share their successor's prefix and are skipped)
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if ((long long)prefix[mid] <= want) lo = mid; else hi = mid - 1;
    }
    long long r = want - prefix[lo];
    long found = -1;
    if (want >= 0) {
        for (int s = 0; s < SCAN / 64; ++s) {
            const long i = (long)lo * SCAN + s * 64 + lane;
            const bool m = i < n && select_match(key[i < n ? i : 0], mode, value);
            const unsigned long long bal = __ballot(m);
            const int c = __popcll(bal);
            if (r < c) {
                const bool mine = m && __popcll(bal & ((1ull << lane) - 1ull)) == (int)r;
                const unsigned long long who = __ballot(mine);              // exactly one bit
                found = (long)lo * SCAN + s * 64 + (__ffsll((long long)who) - 1);
                break;
            }
            r -= c;
        }
    }
    if (lane != 0) return;
    if (src) {
        vals[k] = found >= 0 ? src[found] : 0.f;
    } else {
        const long plane = (long)D1 * D2;
        const long x = found >= 0 ? found / plane : -1, q = found >= 0 ? found - x * plane : 0;
        coords[3 * k] = x;
        coords[3 * k + 1] = found >= 0 ? q / D2 : -1;
        coords[3 * k + 2] = found >= 0 ? q % D2 : -1;
    }
}

}  // namespace cf

using namespace cf;

extern "C" int cf_select_blocks(long n) { return n <= 0 ? 0 : (int)((n + SCAN - 1) / SCAN); }

extern "C" int cf_select_count(const float* key, long n, const float* values, int n_values, int mode, int* prefix, long long* totals, void* stream) {
    CF_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (== value) or 1 (> 0), got %d", mode);
    CF_REQUIRE(n >= 0 && n < (1L << 31), "n = %ld voxels: the scan counts in int32 and takes 0 <= n < 2^31", n);
    const int rows = mode ? 1 : n_values;
    CF_REQUIRE(mode || (n_values >= 1 && n_values <= MAXV), "the value list holds 1..%d values, got %d", MAXV, n_values);
    CF_REQUIRE(key && prefix && totals && (mode || values), "null pointer");
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(totals, 0, sizeof(long long) * rows, st) != hipSuccess) { set_error(std::string(__func__) + ": memset failed"); return CF_ERR_LAUNCH; }
        return CF_OK;
    }
    SelectValues vals = {};
    for (int r = 0; r < rows && !mode; ++r) vals.v[r] = values[r];
    const int nb = cf_select_blocks(n);
    const int grid = nb < 256 * 8 ? nb : 256 * 8;
    hipLaunchKernelGGL(select_count_kernel, dim3(grid), dim3(SCAN), 0, st, key, n, nb, vals, rows, mode, prefix);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_scan_kernel, dim3(rows), dim3(SCAN), 0, st, prefix, nb, totals);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_select_rank(const float* key, long n, int mode, float value, const int* prefix, const long long* ranks, int K, const float* src,
                              float* vals, long long* coords, int D0, int D1, int D2, void* stream) {
    CF_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (== value) or 1 (> 0), got %d", mode);
    CF_REQUIRE(n >= 0 && n < (1L << 31), "n = %ld voxels: the scan counts in int32 and takes 0 <= n < 2^31", n);
    CF_REQUIRE(K >= 0, "K = %d ranks: must not be negative", K);
    CF_REQUIRE(key && prefix && (ranks || K == 0), "null pointer");
    CF_REQUIRE((src != nullptr) != (coords != nullptr), "give either src + vals (gather values) or coords (voxel coordinates)");
    CF_REQUIRE(!src || vals, "null pointer");
    CF_REQUIRE(src || (D0 >= 1 && D1 >= 1 && D2 >= 1 && (long)D0 * D1 * D2 == n), "coords: the shape %d x %d x %d does not hold n = %ld voxels", D0, D1, D2, n);
    if (K == 0 || n == 0) return CF_OK;                  // nothing matches in an empty volume: no rank can have been asked for
    const int nb = cf_select_blocks(n);
    hipLaunchKernelGGL(select_rank_kernel, dim3(cdiv(K, SCAN / 64)), dim3(SCAN), 0, as_stream(stream), key, n, nb, mode, value, prefix, ranks, K, src, vals,
                       coords, D1, D2);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
