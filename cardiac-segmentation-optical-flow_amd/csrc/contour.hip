// Contour tracking and strain of a whole patient (nnunet/compute_contour_metrics.py, nnunet/get_strain.py), DESIGN.md 5.3:
//   * cf_contour_track_table: the ground-truth contour points of every slice moved by the predicted flow in one of the script's four
//     modes, and the per-structure mean point error of every (slice, frame).  One thread owns one chain -- (slice, start frame, point),
//     or (slice, point) in the mode whose chain emits an error at every step -- and walks it alone: a step is sample_points_kernel's
//     arithmetic (elementwise.hip) on both flow components followed by one rounded add, so the positions are the bits a chain of
//     cf_sample_points_2d calls gives.  The chain is a run of dependent gathers: latency bound, a few thousand threads, nothing staged.
//     A second launch turns positions into errors in fp64 and sums them per structure: per thread in point order, over the wave by a
//     fixed butterfly, over the four waves in order -- no atomics, the same bits on every run.
//   * cf_contour_strain_table: get_strain.py:531-599 for all slices -- radial and circumferential Green-Lagrange strain of the tracked
//     endo- / epicardial points against the ED frame, averaged over the points, in fp64, by the same reduction.
// The file is built with -ffp-contract=off (Makefile): the chain's adds, the fp64 squares and the strain quotients round one by one.
#include "common.h"

namespace cf {

constexpr int CT_FROM_ED = 0, CT_FROM_ED_ACC = 1, CT_TO_ED_ACC = 2, CT_TO_ED = 3;

struct Vec2 {
    float x, y;
};

// the flow of one (slice, frame), [2][A][B], sampled at the point (x along B, y along A): sample_points_kernel for C = 2
__device__ __forceinline__ Vec2 sample_flow(const float* __restrict__ frame, Vec2 p, int A, int B) {
    const float gx = __fmul_rn(2.0f, __fsub_rn(__fdiv_rn(p.x, (float)(B - 1)), 0.5f));
    const float gy = __fmul_rn(2.0f, __fsub_rn(__fdiv_rn(p.y, (float)(A - 1)), 0.5f));
    const float xs = __fmul_rn(__fdiv_rn(__fadd_rn(gx, 1.0f), 2.0f), (float)(B - 1));
    const float ys = __fmul_rn(__fdiv_rn(__fadd_rn(gy, 1.0f), 2.0f), (float)(A - 1));
    const Taps t = make_taps(ys, xs, A, B);
    Vec2 d;
    d.x = sample_taps(frame, t, B);
    d.y = sample_taps(frame + (long)A * B, t, B);
    return d;
}

__device__ __forceinline__ Vec2 step(const float* __restrict__ frame, Vec2 cur, int A, int B) {
    const Vec2 d = sample_flow(frame, cur, A, B);
    Vec2 r;
    r.x = __fadd_rn(cur.x, d.x);
    r.y = __fadd_rn(cur.y, d.y);
    return r;
}

// live points of slice d: the three counts summed, never more than the padded row (the host checked the same numbers)
__device__ __forceinline__ int live_points(const int* __restrict__ counts, int d, int Pmax) {
    const int n = max(counts[3 * d], 0) + max(counts[3 * d + 1], 0) + max(counts[3 * d + 2], 0);
    return min(max(n, 0), Pmax);
}

// flow [D][T][2][A][B], pts [D][T][Pmax][2], pos [D][T-1][Pmax][2].  S = chains per (slice, point): 1 in CT_FROM_ED_ACC, T - 1 otherwise.
// Frame 0 of the flow is never read.  Padding points get 0.
__global__ void __launch_bounds__(256) contour_track_kernel(const float* __restrict__ flow, const float* __restrict__ pts, const int* __restrict__ counts,
                                                           int D, int T, int A, int B, int Pmax, int mode, float* __restrict__ pos) {
    const int S = mode == CT_FROM_ED_ACC ? 1 : T - 1;
    const long total = (long)D * S * Pmax;
    const long fsz = 2L * A * B;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int p = (int)(idx % Pmax);
        const long r = idx / Pmax;
        const int s = (int)(r % S) + 1, d = (int)(r / S);                  // s: the start frame (the frame of the one flow in the single-flow modes)
        const float* fl = flow + (long)d * T * fsz;
        const float2* pt = reinterpret_cast<const float2*>(pts) + (long)d * T * Pmax;
        float2* out = reinterpret_cast<float2*>(pos) + (long)d * (T - 1) * Pmax;
        const bool live = p < live_points(counts, d, Pmax);
        if (mode == CT_FROM_ED_ACC) {
            Vec2 cur = {0.f, 0.f};
            if (live) { const float2 v = pt[p]; cur.x = v.x; cur.y = v.y; }
            for (int t = 1; t < T; ++t) {
                if (live) cur = step(fl + t * fsz, cur, A, B);
                out[(long)(t - 1) * Pmax + p] = make_float2(cur.x, cur.y);
            }
            continue;
        }
        Vec2 res = {0.f, 0.f};
        if (live) {
            if (mode == CT_FROM_ED) {
                const float2 v = pt[p];
                res = step(fl + s * fsz, Vec2{v.x, v.y}, A, B);
            } else {
                const float2 v = pt[(long)s * Pmax + p];
                const Vec2 init = {v.x, v.y};
                if (mode == CT_TO_ED) {
                    res = sample_flow(fl + s * fsz, init, A, B);
                } else {
                    Vec2 cur = init;
                    for (int t = s; t >= 1; --t) cur = step(fl + t * fsz, cur, A, B);
                    res.x = __fsub_rn(cur.x, init.x);
                    res.y = __fsub_rn(cur.y, init.y);
                }
            }
        }
        out[(long)(s - 1) * Pmax + p] = make_float2(res.x, res.y);
    }
}

// three per-thread fp64 sums -> the workgroup's totals in red[0][0..2]: butterfly inside the wave, the four waves added in order
__device__ __forceinline__ void block_sum3(double (&v)[3], double (*red)[3]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double w = wave_sum_d(v[k]);
        if (lane == 0) red[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < 3) red[0][threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    __syncthreads();
}

// grid (T - 1, D): table[d][r][k] = mean over the points of structure k of || gt - pos ||, fp64 from the fp32 values.  gt is the point of
// frame r + 1 where pos is a position, and (point of frame 0) - (point of frame r + 1) where it is a delta.  No points: 0 / 0 = NaN.
__global__ void __launch_bounds__(256) contour_error_kernel(const float* __restrict__ pts, const float* __restrict__ pos, const int* __restrict__ counts,
                                                           int T, int Pmax, int mode, double* __restrict__ table) {
    __shared__ double red[4][3];
    const int r = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
    const int n = live_points(counts, d, Pmax);
    const int c0 = min(max(counts[3 * d], 0), n), c1 = min(c0 + max(counts[3 * d + 1], 0), n);
    const float2* pt = reinterpret_cast<const float2*>(pts) + (long)d * T * Pmax;
    const float2* ps = reinterpret_cast<const float2*>(pos) + ((long)d * (T - 1) + r) * Pmax;
    const bool delta = mode == CT_TO_ED_ACC || mode == CT_TO_ED;
    double s[3] = {0.0, 0.0, 0.0};
    for (int p = tid; p < n; p += 256) {
        const float2 g = pt[(long)(r + 1) * Pmax + p], q = ps[p];
        double gx = (double)g.x, gy = (double)g.y;
        if (delta) {
            const float2 e = pt[p];
            gx = (double)e.x - gx;
            gy = (double)e.y - gy;
        }
        const double dx = gx - (double)q.x, dy = gy - (double)q.y;
        const double err = sqrt(dx * dx + dy * dy);
        const int k = p < c0 ? 0 : (p < c1 ? 1 : 2);
#pragma unroll
        for (int j = 0; j < 3; ++j) s[j] += j == k ? err : 0.0;
    }
    block_sum3(s, red);
    if (tid < 3) {
        const int cnt = tid == 0 ? c0 : (tid == 1 ? c1 - c0 : n - c1);
        table[((long)d * (T - 1) + r) * 3 + tid] = red[0][tid] / (double)cnt;
    }
}

// grid (T, D): table[d][t] = {radial, circumferential} strain of frame t (0: the ED points themselves) against ED, averaged over the n
// points of each of the two contours (endo at [0, n), epi at [n, 2n)).  mm = (double)pixel * zoom.  Radial: L = || epi - endo || per
// point; circumferential: L = the mean over the two contours of || point p + 1 - point p ||, closed; strain 0.5 (L^2 - L0^2) / L0^2.
__global__ void __launch_bounds__(256) contour_strain_kernel(const float* __restrict__ pos, const float* __restrict__ ed_pts, long ed_stride,
                                                            const int* __restrict__ counts, int T, int Pmax, double zx, double zy,
                                                            double* __restrict__ table) {
    __shared__ double red[4][3];
    const int t = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
    const int n = min(max(counts[3 * d], 0), Pmax / 2);
    const float2* e0 = reinterpret_cast<const float2*>(ed_pts + (long)d * ed_stride);
    const float2* et = t == 0 ? e0 : reinterpret_cast<const float2*>(pos) + ((long)d * (T - 1) + (t - 1)) * Pmax;
    auto dist = [&](const float2* f, int a, int b) {
        const float2 u = f[a], v = f[b];
        const double dx = (double)v.x * zx - (double)u.x * zx, dy = (double)v.y * zy - (double)u.y * zy;
        return sqrt(dx * dx + dy * dy);
    };
    auto strain = [](double l, double l0) { return 0.5 * ((l * l - l0 * l0) / (l0 * l0)); };
    double s[3] = {0.0, 0.0, 0.0};
    for (int p = tid; p < n; p += 256) {
        const int q = p + 1 < n ? p + 1 : 0;
        s[0] += strain(dist(et, p, n + p), dist(e0, p, n + p));
        s[1] += strain((dist(et, p, q) + dist(et, n + p, n + q)) / 2.0, (dist(e0, p, q) + dist(e0, n + p, n + q)) / 2.0);
    }
    block_sum3(s, red);
    if (tid < 2) table[((long)d * T + t) * 2 + tid] = red[0][tid] / (double)n;
}

}  // namespace cf

using namespace cf;

// counts: HOST int [D][3]; every check the kernels rely on is made here
static int contour_counts_ok(const int* counts, int D, int Pmax, bool strain) {
    for (int d = 0; d < D; ++d) {
        const int a = counts[3 * d], b = counts[3 * d + 1], c = counts[3 * d + 2];
        CF_REQUIRE(a >= 0 && b >= 0 && c >= 0, "slice %d: negative count (%d, %d, %d)", d, a, b, c);
        CF_REQUIRE((long)a + b + c <= Pmax, "slice %d: %d + %d + %d points exceed the padded row Pmax=%d", d, a, b, c, Pmax);
        if (strain) CF_REQUIRE(a == b, "slice %d: %d endo and %d epi points: strain needs equal counts", d, a, b);
    }
    return CF_OK;
}

extern "C" int cf_contour_track_table(const float* flow, const float* pts, const int* counts, const int* counts_dev, int D, int T, int A, int B,
                                      int Pmax, int mode, float* pos, double* table, void* stream) {
    CF_REQUIRE(flow && pts && counts && counts_dev && pos && table, "null pointer");
    CF_REQUIRE(D > 0 && T >= 2 && A >= 2 && B >= 2 && Pmax > 0, "bad shape D=%d T=%d A=%d B=%d Pmax=%d (T >= 2 frames, a map of 2 x 2 or more)", D, T, A, B, Pmax);
    CF_REQUIRE(D <= 65535 && (long)A * B < (1L << 30) && (long)D * T * Pmax < (1L << 30), "too large: D=%d T=%d A=%d B=%d Pmax=%d", D, T, A, B, Pmax);
    CF_REQUIRE(mode >= CT_FROM_ED && mode <= CT_TO_ED, "mode must be 0 (from_ed), 1 (from_ed_accumulation), 2 (to_ed_accumulation) or 3 (to_ed), got %d", mode);
    if (int rc = contour_counts_ok(counts, D, Pmax, false)) return rc;
    hipStream_t s = as_stream(stream);
    const long chains = (long)D * (mode == CT_FROM_ED_ACC ? 1 : T - 1) * Pmax;
    hipLaunchKernelGGL(contour_track_kernel, dim3(flat_grid(chains, 256)), dim3(256), 0, s, flow, pts, counts_dev, D, T, A, B, Pmax, mode, pos);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(contour_error_kernel, dim3((unsigned)(T - 1), (unsigned)D), dim3(256), 0, s, pts, (const float*)pos, counts_dev, T, Pmax, mode, table);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_contour_strain_table(const float* pos, const float* ed_pts, long ed_stride, const int* counts, const int* counts_dev, int D, int T,
                                       int Pmax, double zoom_x, double zoom_y, double* table, void* stream) {
    CF_REQUIRE(pos && ed_pts && counts && counts_dev && table, "null pointer");
    CF_REQUIRE(D > 0 && T >= 2 && Pmax > 0, "bad shape D=%d T=%d Pmax=%d (T >= 2 frames)", D, T, Pmax);
    CF_REQUIRE(D <= 65535 && (long)D * T * Pmax < (1L << 30), "too large: D=%d T=%d Pmax=%d", D, T, Pmax);
    CF_REQUIRE(ed_stride >= 2L * Pmax && !(ed_stride & 1), "ed_stride=%ld floats between slices: even and at least one row of Pmax=%d points", ed_stride, Pmax);
    if (int rc = contour_counts_ok(counts, D, Pmax, true)) return rc;
    hipLaunchKernelGGL(contour_strain_kernel, dim3((unsigned)T, (unsigned)D), dim3(256), 0, as_stream(stream), pos, ed_pts, ed_stride, counts_dev, T, Pmax,
                       zoom_x, zoom_y, table);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
