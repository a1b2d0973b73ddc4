// The cine tables of nnunet/compute_metrics.py and nnunet/compute_jacobian.py, one device visit per patient:
//   * cf_label_surface_count / cf_label_surface_table: for every frame n and class c >= 1 of two label stacks, TP / FP / FN of
//     `test == c` vs `reference == c`, the border sets of both masks (medpy's mask ^ binary_erosion(mask, face structure), the
//     rule of surface_border_kernel in metrics.hip applied to `label == c` inside the frame's own volume), and the directed
//     nearest-border distances with their maxima and sums.  One classification pass counts, a one-block scan turns the 2 N K
//     counts into segment offsets, a fill pass compacts the coordinates, and ONE distance launch serves every segment.
//   * cf_flow_regularity_table: compute_jacobian.py:141-198 for a whole cine -- per (frame, slice) the sums of |d/dt| and of
//     |d/dy| + |d/dx| of both flow components (kornia's replicate-padded 0.5 * (x[+1] - x[-1])) and sum / count / negatives of the
//     2-D Jacobian determinant per label and for the whole slice (the arithmetic of jacobian_det_2d_kernel in warp.hip).  No
//     determinant image and no gradient tensor is stored.
//   * cf_cine_ssim_table: nnunet/compute_SSIM.py / compute_SSIM_crop_per_structure.py for a whole cine -- per (frame, slice) the sum of
//     skimage's SSIM map (the arithmetic of ssim_map_kernel in metrics.hip) over the interior and over each label of the ED
//     segmentation, the windows summed separably from an LDS-staged halo.  No SSIM map is stored.
// The file is built with -ffp-contract=off (Makefile): the fp64 products and sums round one by one, as in scipy / numpy.
#include "common.h"

namespace cf {

typedef unsigned long long u64;

constexpr int ST_COLS = 9;        // tp fp fn | border test, border ref | max t->r, max r->t | sum t->r, sum r->t
constexpr int ST_CNT = 5;         // the integer columns, counted as u32 before the scan writes them as fp64

__device__ __forceinline__ bool border_of(const uint8_t* __restrict__ f, long i, int c, int z, int y, int x, int D, int H, int W, long HW, int ndim) {
    bool b = x == 0 || x == W - 1 || y == 0 || y == H - 1 || f[i - 1] != c || f[i + 1] != c || f[i - W] != c || f[i + W] != c;
    if (ndim == 3) b = b || z == 0 || z == D - 1 || f[i - HW] != c || f[i + HW] != c;
    return b;
}

// blockIdx.y = frame.  FILL = false: cnt[n][c][0..4] += tp, fp, fn, border voxels of test == c, of ref == c (c >= 1), *bad += voxels with
// a label >= K.  FILL = true: the border voxels' (z, y, x) go to coords at the segment cursors (segment (n K + c) 2 + side).
template <bool FILL>
__global__ void __launch_bounds__(256) label_border_kernel(const uint8_t* __restrict__ test, const uint8_t* __restrict__ ref, int D, int H, int W,
                                                           int ndim, int K, unsigned* __restrict__ cnt, unsigned* __restrict__ bad,
                                                           const int* __restrict__ offs, int* __restrict__ cursor, int* __restrict__ coords, int total) {
    __shared__ unsigned h[16 * ST_CNT + 1];
    __shared__ unsigned lc[32];
    __shared__ int base[32];
    const int n = blockIdx.y, tid = threadIdx.x;
    const long HW = (long)H * W, V = (long)D * HW;
    const uint8_t* tf = test + (long)n * V;
    const uint8_t* rf = ref + (long)n * V;
    if (!FILL) {
        for (int k = tid; k <= 16 * ST_CNT; k += 256) h[k] = 0;
        __syncthreads();
    }
    const long step = (long)gridDim.x * 256;
    const long trips = (V + step - 1) / step;
    for (long trip = 0; trip < trips; ++trip) {
        const long i = trip * step + (long)blockIdx.x * 256 + tid;
        int t = 0, r = 0;
        bool bt = false, br = false;
        int z = 0, y = 0, x = 0;
        if (i < V) {
            t = tf[i];
            r = rf[i];
            if (!FILL && (t >= K || r >= K)) atomicAdd(&h[16 * ST_CNT], 1u);
            if (t >= K) t = 0;
            if (r >= K) r = 0;
            if (t | r) {
                z = (int)(i / HW);
                const int q = (int)(i - (long)z * HW);
                y = q / W;
                x = q - y * W;
                bt = t && border_of(tf, i, t, z, y, x, D, H, W, HW, ndim);
                br = r && border_of(rf, i, r, z, y, x, D, H, W, HW, ndim);
            }
        }
        if (!FILL) {
            if (t && t == r) atomicAdd(&h[t * ST_CNT], 1u);
            else {
                if (t) atomicAdd(&h[t * ST_CNT + 1], 1u);
                if (r) atomicAdd(&h[r * ST_CNT + 2], 1u);
            }
            if (bt) atomicAdd(&h[t * ST_CNT + 3], 1u);
            if (br) atomicAdd(&h[r * ST_CNT + 4], 1u);
        } else {
            if (tid < 32) lc[tid] = 0;
            __syncthreads();
            unsigned st = 0, sr = 0;
            if (bt) st = atomicAdd(&lc[2 * t], 1u);
            if (br) sr = atomicAdd(&lc[2 * r + 1], 1u);
            __syncthreads();
            if (tid < 2 * K) base[tid] = lc[tid] ? atomicAdd(&cursor[(long)n * 2 * K + tid], (int)lc[tid]) : 0;
            __syncthreads();
            if (bt) {
                const int seg = n * 2 * K + 2 * t;
                const int slot = base[2 * t] + (int)st;
                if (slot < offs[seg + 1] && slot < total) { coords[3L * slot] = z; coords[3L * slot + 1] = y; coords[3L * slot + 2] = x; }
            }
            if (br) {
                const int seg = n * 2 * K + 2 * r + 1;
                const int slot = base[2 * r + 1] + (int)sr;
                if (slot < offs[seg + 1] && slot < total) { coords[3L * slot] = z; coords[3L * slot + 1] = y; coords[3L * slot + 2] = x; }
            }
            __syncthreads();
        }
    }
    if (!FILL) {
        __syncthreads();
        for (int k = tid; k < K * ST_CNT; k += 256)
            if (h[k]) atomicAdd(&cnt[(long)n * K * ST_CNT + k], h[k]);
        if (tid == 0 && h[16 * ST_CNT]) atomicAdd(bad, h[16 * ST_CNT]);
    }
}

// one block: exclusive scans over the S = 2 N K segments of (border points) -> offs[S + 1] and of (distance workgroups: 256 points of a
// segment each, none where either side of the pair is empty) -> blk[S + 1]; cursor = offs; the table's count columns as fp64, the
// maxima and sums zeroed, table[N K ST_COLS] = voxels with a label >= K.
__global__ void __launch_bounds__(256) label_segment_scan_kernel(const unsigned* __restrict__ cnt, const unsigned* __restrict__ bad, int S, int* __restrict__ offs,
                                                                 int* __restrict__ blk, int* __restrict__ cursor, double* __restrict__ table) {
    __shared__ int pa[256], pb[256];
    const int tid = threadIdx.x;
    const int per = (S + 255) / 256;
    const int s0 = min(S, tid * per), s1 = min(S, s0 + per);
    auto points = [&](int s) { return (int)cnt[(long)(s >> 1) * ST_CNT + 3 + (s & 1)]; };
    auto blocks = [&](int s) { const int a = points(s), b = points(s ^ 1); return (a > 0 && b > 0) ? (a + 255) / 256 : 0; };
    int a = 0, b = 0;
    for (int s = s0; s < s1; ++s) { a += points(s); b += blocks(s); }
    pa[tid] = a;
    pb[tid] = b;
    __syncthreads();
    if (tid == 0) {
        int ra = 0, rb = 0;
        for (int k = 0; k < 256; ++k) {
            const int ta = pa[k], tb = pb[k];
            pa[k] = ra;
            pb[k] = rb;
            ra += ta;
            rb += tb;
        }
        offs[S] = ra;
        blk[S] = rb;
        table[(long)(S >> 1) * ST_COLS] = (double)bad[0];
    }
    __syncthreads();
    a = pa[tid];
    b = pb[tid];
    for (int s = s0; s < s1; ++s) {
        offs[s] = a;
        cursor[s] = a;
        blk[s] = b;
        a += points(s);
        b += blocks(s);
        if (!(s & 1)) {
            const long row = s >> 1;
            for (int k = 0; k < ST_COLS; ++k) table[row * ST_COLS + k] = k < ST_CNT ? (double)cnt[row * ST_CNT + k] : 0.0;
        }
    }
}

// one workgroup = 256 A-points of one segment against all B-points of its partner (the other side of the same frame and class),
// streamed through LDS: dist[a] = min_b || spacing * (a - b) || as surface_min_dist_kernel, then the maximum (atomicMax on the bit
// pattern of a non-negative double) and the sum (fp64 atomicAdd) of the workgroup's distances into the table
__global__ void __launch_bounds__(256) label_surface_dist_kernel(const int* __restrict__ coords, const int* __restrict__ offs, const int* __restrict__ blk,
                                                                 int S, int total, double sz, double sy, double sx, double* __restrict__ dist,
                                                                 double* __restrict__ table) {
    __shared__ int tile[256 * 3];
    __shared__ double rm[4], rs[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= blk[S]) return;
    int lo = 0, hi = S;                                           // blk[lo] <= b < blk[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk[mid] <= b) lo = mid; else hi = mid;
    }
    const int s = lo, p = s ^ 1;
    const int a0 = offs[s], a1 = offs[s + 1], b0 = offs[p], b1 = offs[p + 1];
    if (a0 < 0 || b0 < 0 || a1 > total || b1 > total || a1 < a0 || b1 < b0) return;
    const int nA = a1 - a0, nB = b1 - b0;
    const int i = (b - blk[s]) * 256 + tid;
    const bool live = i < nA;
    int az = 0, ay = 0, ax = 0;
    if (live) { az = coords[3L * (a0 + i)]; ay = coords[3L * (a0 + i) + 1]; ax = coords[3L * (a0 + i) + 2]; }
    double best = INFINITY;
    for (int j0 = 0; j0 < nB; j0 += 256) {
        const int c = min(256, nB - j0);
        __syncthreads();
        for (int k = tid; k < c * 3; k += 256) tile[k] = coords[3L * (b0 + j0) + k];
        __syncthreads();
        if (live) {
            for (int j = 0; j < c; ++j) {
                const double dz = sz * (double)(az - tile[3 * j]), dy = sy * (double)(ay - tile[3 * j + 1]), dx = sx * (double)(ax - tile[3 * j + 2]);
                best = fmin(best, __dadd_rn(__dadd_rn(__dmul_rn(dz, dz), __dmul_rn(dy, dy)), __dmul_rn(dx, dx)));
            }
        }
    }
    double mx = 0.0, sm = 0.0;
    if (live && nB > 0) {
        mx = sm = sqrt(best);
        dist[a0 + i] = mx;
    }
    for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_xor(mx, o, 64)); sm += __shfl_xor(sm, o, 64); }
    if ((tid & 63) == 0) { rm[tid >> 6] = mx; rs[tid >> 6] = sm; }
    __syncthreads();
    if (tid == 0) {
        mx = fmax(fmax(rm[0], rm[1]), fmax(rm[2], rm[3]));
        sm = rs[0] + rs[1] + rs[2] + rs[3];
        double* row = table + (long)(s >> 1) * ST_COLS;
        atomicMax(reinterpret_cast<u64*>(&row[5 + (s & 1)]), (u64)__double_as_longlong(mx));
        atomicAdd(&row[7 + (s & 1)], sm);
    }
}

// ------------------------------------------------------------------------------------------------ flow regularity
constexpr int FR_TW = 64, FR_TH = 32, FR_MAXCOLS = 2 + 3 * 17;

// grid (tiles, T * D); a workgroup owns a 32 x 64 tile of one slice of one frame, a thread 8 pixels of one column.  Every per-thread
// accumulator is summed over the wave by a fixed butterfly and over the four waves in order; part[slice][tile][col] gets the tile's
// totals, which flow_regularity_reduce_kernel adds in tile order: the table is the same bit pattern on every run.
__global__ void __launch_bounds__(256) flow_regularity_tile_kernel(const float* __restrict__ flow, const uint8_t* __restrict__ lab, int T, int D, int H, int W,
                                                                   int K, int tiles_x, double* __restrict__ part) {
    __shared__ double red[4][FR_MAXCOLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slice = blockIdx.y, t = slice / D, d = slice - t * D;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const long HW = (long)H * W;
    const float* f0 = flow + (long)slice * 2 * HW;
    const float* f1 = f0 + HW;
    const int tm = t > 0 ? t - 1 : t, tp = t < T - 1 ? t + 1 : t;
    const float* m0 = flow + ((long)tm * D + d) * 2 * HW;
    const float* p0 = flow + ((long)tp * D + d) * 2 * HW;
    const uint8_t* ls = lab + (long)slice * HW;
    double gt = 0.0, gs = 0.0, sw = 0.0, sj[16];
    unsigned cw = 0, cn[16];                                     // count in the low half, negatives in the high half (8 pixels per thread)
#pragma unroll
    for (int k = 0; k < 16; ++k) { sj[k] = 0.0; cn[k] = 0; }
    const int j = tx * FR_TW + lane;
    if (j < W) {
        const int jl = j > 0 ? j - 1 : j, jr = j < W - 1 ? j + 1 : j;
        const double rhj = jr - jl == 2 ? 0.5 : 1.0;
        for (int r = 0; r < FR_TH / 4; ++r) {
            const int i = ty * FR_TH + wave + 4 * r;
            if (i >= H) break;
            const int iu = i > 0 ? i - 1 : i, id = i < H - 1 ? i + 1 : i;
            const double rhi = id - iu == 2 ? 0.5 : 1.0;
            const long c = (long)i * W + j;
            const float u0 = f0[(long)iu * W + j], n0 = f0[(long)id * W + j], l0 = f0[(long)i * W + jl], r0 = f0[(long)i * W + jr];
            const float u1 = f1[(long)iu * W + j], n1 = f1[(long)id * W + j], l1 = f1[(long)i * W + jl], r1 = f1[(long)i * W + jr];
            gt += (double)fabsf(0.5f * (p0[c] - m0[c])) + (double)fabsf(0.5f * (p0[HW + c] - m0[HW + c]));
            gs += (double)fabsf(0.5f * (r0 - l0)) + (double)fabsf(0.5f * (n0 - u0)) + (double)fabsf(0.5f * (r1 - l1)) + (double)fabsf(0.5f * (n1 - u1));
            // np.gradient of displacement + identity grid, fp64: jacobian_det_2d_kernel's expressions (1 / spacing as an exact factor)
            const double p0_a0 = (((double)n0 + id) - ((double)u0 + iu)) * rhi;
            const double p1_a0 = (((double)n1 + j) - ((double)u1 + j)) * rhi;
            const double p0_a1 = (((double)r0 + i) - ((double)l0 + i)) * rhj;
            const double p1_a1 = (((double)r1 + jr) - ((double)l1 + jl)) * rhj;
            const double det = p0_a0 * p1_a1 - p0_a1 * p1_a0;
            const unsigned one = 1u | (det < 0.0 ? 0x10000u : 0u);
            sw += det;
            cw += one;
            const int k = ls[c];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                sj[q] += q == k ? det : 0.0;
                cn[q] += q == k ? one : 0u;
            }
        }
    }
    auto put = [&](int col, double v) {
        v = wave_sum_d(v);
        if (lane == 0) red[wave][col] = v;
    };
    put(0, gt);
    put(1, gs);
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < K) { put(2 + 3 * k, sj[k]); put(3 + 3 * k, (double)(cn[k] & 0xffffu)); put(4 + 3 * k, (double)(cn[k] >> 16)); }
    put(2 + 3 * K, sw);
    put(3 + 3 * K, (double)(cw & 0xffffu));
    put(4 + 3 * K, (double)(cw >> 16));
    __syncthreads();
    const int cols = 5 + 3 * K;
    if (tid < cols) part[((long)slice * gridDim.x + blockIdx.x) * cols + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ void __launch_bounds__(64) flow_regularity_reduce_kernel(const double* __restrict__ part, int ntiles, int cols, double* __restrict__ table) {
    const int slice = blockIdx.x, c = threadIdx.x;
    if (c >= cols) return;
    double s = 0.0;
    for (int k = 0; k < ntiles; ++k) s += part[((long)slice * ntiles + k) * cols + c];
    table[(long)slice * cols + c] = s;
}

// ------------------------------------------------------------------------------------------------ cine SSIM
constexpr int CS_TW = 64, CS_TH = 32, CS_ROWS = CS_TH / 4, CS_MAXWIN = 15, CS_MAXCOLS = 2 + 2 * 16;

// scipy's 'reflect' (d c b a | a b c d | d c b a), as ssim_map_kernel resolves it; the clamp keeps the halo of a partial tile's dead pixels in bounds
__device__ __forceinline__ int reflect_index(int i, int n) {
    i = i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
    return min(max(i, 0), n - 1);
}

// one workgroup of 1024 per slice: range[slice] = {min, max} of the registered slice, NaN when a value is (numpy's min / max)
__global__ void __launch_bounds__(1024) cine_ssim_range_kernel(const float* __restrict__ reg, long HW, float* __restrict__ range) {
    __shared__ float rmin[16], rmax[16];
    __shared__ int rbad[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* p = reg + (long)blockIdx.x * HW;
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    for (long i = tid; i < HW; i += 1024) {
        const float v = p[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
        bad |= v != v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    if (lane == 0) { rmin[wave] = mn; rmax[wave] = mx; rbad[wave] = bad; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 16; ++k) { mn = fminf(mn, rmin[k]); mx = fmaxf(mx, rmax[k]); bad |= rbad[k]; }
        range[2L * blockIdx.x] = bad ? NAN : mn;
        range[2L * blockIdx.x + 1] = bad ? NAN : mx;
    }
}

// grid (tiles, T * D); a workgroup owns a 32 x 64 tile of one slice of one frame, a wave 8 rows of it, a thread those 8 rows of one column.
// The (32 + win - 1) x (64 + win - 1) halo of both images is staged once (fixed fp64, registered fp32), reflection resolved on the way in.
// Window sums are separable: for each of the 8 + win - 1 halo rows of its strip a thread forms the five row sums over win columns from LDS
// (lane = column: every wave read is one contiguous run, free of bank conflicts at 4 and at 8 bytes) and adds them to those of its 8 pixels
// whose window holds the row -- the column sums stay in registers: five fp64 row-sum planes of a strip do not fit beside the halo.  That is
// 2 win (8 + win - 1) / 8 LDS reads per pixel for all five quantities where ssim_map_kernel reads 2 win^2 values from global memory.  The
// window is a template argument (one instantiation per odd win 3..15): the halo arrays have their exact size (31.9 KB at win 7, 43.1 KB at
// win 15), both loops unroll, a row's LDS reads are issued together and which pixel takes which row sum is known at compile time.
// S is ssim_map_kernel's expression; the sums go over the wave by a fixed butterfly and over the four waves in order.
template <int WIN>
__global__ void __launch_bounds__(256) cine_ssim_tile_kernel(const double* __restrict__ fixed, const float* __restrict__ reg, const uint8_t* __restrict__ lab,
                                                             int D, int H, int W, int K, double K1, double K2, double cov_norm, int tiles_x,
                                                             const float* __restrict__ range, double* __restrict__ part) {
    constexpr int win = WIN, pad = WIN / 2, hh = CS_TH + WIN - 1, hw = CS_TW + WIN - 1;
    __shared__ double A[hh * hw];
    __shared__ float B[hh * hw];
    __shared__ double red[4][CS_MAXCOLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slice = blockIdx.y, d = slice % D;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const long HW = (long)H * W;
    const double* fs = fixed + (long)d * HW;
    const float* rs = reg + (long)slice * HW;
    const int y0 = ty * CS_TH - pad, x0 = tx * CS_TW - pad;
    for (int i = tid; i < hh * hw; i += 256) {
        const int r = i / hw, c = i - r * hw;
        const long g = (long)reflect_index(y0 + r, H) * W + reflect_index(x0 + c, W);
        A[i] = fs[g];
        B[i] = rs[g];
    }
    __syncthreads();

    const int row0 = wave * CS_ROWS;                             // the strip's first row inside the tile, and its first halo row
    double ax[CS_ROWS], ay[CS_ROWS], axx[CS_ROWS], ayy[CS_ROWS], axy[CS_ROWS];
#pragma unroll
    for (int o = 0; o < CS_ROWS; ++o) ax[o] = ay[o] = axx[o] = ayy[o] = axy[o] = 0.0;
    const bool strip_live = ty * CS_TH + row0 < H;               // wave-uniform
    if (strip_live) {
#pragma unroll
        for (int hr = 0; hr < CS_ROWS + win - 1; ++hr) {
            const double* ar = A + (row0 + hr) * hw + lane;
            const float* br = B + (row0 + hr) * hw + lane;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int dx = 0; dx < win; ++dx) {
                const double u = ar[dx], v = (double)br[dx];
                sx += u; sy += v; sxx += u * u; syy += v * v; sxy += u * v;
            }
#pragma unroll
            for (int o = 0; o < CS_ROWS; ++o)
                if (hr >= o && hr < o + win) {                            // halo row hr lies in the window of the strip's pixel row o: known at compile time
                    ax[o] += sx; ay[o] += sy; axx[o] += sxx; ayy[o] += syy; axy[o] += sxy;
                }
        }
    }

    // C1 = (K1 R)^2, C2 = (K2 R)^2 with R = max - min subtracted in fp32, as on a float32 array
    const double R = (double)(range[2L * slice + 1] - range[2L * slice]);
    const double C1 = (K1 * R) * (K1 * R), C2 = (K2 * R) * (K2 * R);
    const double inv = 1.0 / ((double)win * win);
    const uint8_t* ls = lab ? lab + (long)d * HW : nullptr;
    double sw = 0.0, sk[16];
    unsigned cw = 0, ck[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { sk[k] = 0.0; ck[k] = 0; }
    const int x = tx * CS_TW + lane;
    if (strip_live && x < W) {
#pragma unroll
        for (int o = 0; o < CS_ROWS; ++o) {
            const int y = ty * CS_TH + row0 + o;
            if (y < H) {
                const double ux = ax[o] * inv, uy = ay[o] * inv;
                const double vx = cov_norm * (axx[o] * inv - ux * ux), vy = cov_norm * (ayy[o] * inv - uy * uy), vxy = cov_norm * (axy[o] * inv - ux * uy);
                const double S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
                if (y >= pad && y < H - pad && x >= pad && x < W - pad) { sw += S; cw += 1; }
                const int k = ls ? ls[(long)y * W + x] : 255;
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (q < K) {                                      // uniform: labels >= K count nowhere
                        sk[q] += q == k ? S : 0.0;
                        ck[q] += q == k ? 1u : 0u;
                    }
            }
        }
    }
    auto put = [&](int col, double v) {
        v = wave_sum_d(v);
        if (lane == 0) red[wave][col] = v;
    };
    put(0, sw);
    put(1, (double)cw);
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < K) { put(2 + 2 * k, sk[k]); put(3 + 2 * k, (double)ck[k]); }
    __syncthreads();
    const int cols = 2 + 2 * K;
    if (tid < cols) part[((long)slice * gridDim.x + blockIdx.x) * cols + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

}  // namespace cf

using namespace cf;

#define CHECK_HIP(expr, what)                                              \
    do {                                                                   \
        if ((expr) != hipSuccess) { set_error(what); return CF_ERR_LAUNCH; } \
    } while (0)

static int surface_args_ok(int N, int D, int H, int W, int ndim, int K) {
    CF_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && N <= 65535, "bad shape N=%d D=%d H=%d W=%d (N <= 65535)", N, D, H, W);
    CF_REQUIRE((long)N * D * H * W < (1L << 30), "stack of %ld voxels: the segment offsets are 32-bit (N D H W < 2^30)", (long)N * D * H * W);
    CF_REQUIRE(ndim == 3 || (ndim == 2 && D == 1), "ndim must be 3, or 2 with D == 1");
    CF_REQUIRE(K >= 2 && K <= 16, "K must be 2..16, got %d", K);
    return CF_OK;
}

// ws layout (int32): cnt [N K 5] | bad [1] | offs [2 N K + 1] | blk [2 N K + 1] | cursor [2 N K]
struct SurfaceWs {
    unsigned *cnt, *bad;
    int *offs, *blk, *cursor;
    SurfaceWs(int* ws, int N, int K) {
        const long nk = (long)N * K;
        cnt = reinterpret_cast<unsigned*>(ws);
        bad = cnt + nk * ST_CNT;
        offs = ws + nk * ST_CNT + 1;
        blk = offs + 2 * nk + 1;
        cursor = blk + 2 * nk + 1;
    }
};

static dim3 border_grid(int N, int D, int H, int W) {
    long gx = ((long)D * H * W + 255) / 256;
    if (gx > 1024) gx = 1024;
    return dim3((unsigned)gx, (unsigned)N);
}

extern "C" int cf_label_surface_count(const uint8_t* test, const uint8_t* reference, int N, int D, int H, int W, int ndim, int K, int* ws, double* table,
                                      void* stream) {
    CF_REQUIRE(test && reference && ws && table, "null pointer");
    if (int rc = surface_args_ok(N, D, H, W, ndim, K)) return rc;
    hipStream_t s = as_stream(stream);
    SurfaceWs w(ws, N, K);
    CHECK_HIP(hipMemsetAsync(ws, 0, ((size_t)N * K * ST_CNT + 1) * sizeof(int), s), "cf_label_surface_count: memset failed");
    hipLaunchKernelGGL(label_border_kernel<false>, border_grid(N, D, H, W), dim3(256), 0, s, test, reference, D, H, W, ndim, K, w.cnt, w.bad,
                       (const int*)nullptr, (int*)nullptr, (int*)nullptr, 0);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(label_segment_scan_kernel, dim3(1), dim3(256), 0, s, w.cnt, w.bad, 2 * N * K, w.offs, w.blk, w.cursor, table);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_label_surface_table(const uint8_t* test, const uint8_t* reference, int N, int D, int H, int W, int ndim, int K, double sz, double sy,
                                      double sx, int* ws, int total, int nblocks, int* coords, double* dist, double* table, void* stream) {
    CF_REQUIRE(test && reference && ws && table, "null pointer");
    if (int rc = surface_args_ok(N, D, H, W, ndim, K)) return rc;
    CF_REQUIRE(total >= 0 && nblocks >= 0 && nblocks <= total, "bad sizes total=%d nblocks=%d (offs[2NK] and blk[2NK] of cf_label_surface_count)", total, nblocks);
    CF_REQUIRE(total == 0 || (coords && dist), "null pointer");
    if (total == 0) return CF_OK;
    hipStream_t s = as_stream(stream);
    SurfaceWs w(ws, N, K);
    hipLaunchKernelGGL(label_border_kernel<true>, border_grid(N, D, H, W), dim3(256), 0, s, test, reference, D, H, W, ndim, K, w.cnt, w.bad,
                       (const int*)w.offs, w.cursor, coords, total);
    CF_CHECK_LAUNCH();
    if (nblocks > 0) {
        hipLaunchKernelGGL(label_surface_dist_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, (const int*)coords, (const int*)w.offs, (const int*)w.blk,
                           2 * N * K, total, sz, sy, sx, dist, table);
        CF_CHECK_LAUNCH();
    }
    return CF_OK;
}

extern "C" int cf_flow_regularity_table(const float* flow, const uint8_t* labels, int T, int D, int H, int W, int K, double* part, double* table,
                                        void* stream) {
    CF_REQUIRE(flow && labels && part && table, "null pointer");
    CF_REQUIRE(T > 0 && D > 0 && H >= 2 && W >= 2, "bad shape T=%d D=%d H=%d W=%d (np.gradient needs two points per axis)", T, D, H, W);
    CF_REQUIRE((long)T * D <= 65535, "T * D = %ld slices exceed one grid dimension (65535)", (long)T * D);
    CF_REQUIRE(K >= 1 && K <= 16, "K must be 1..16, got %d", K);
    const int tiles_x = cdiv(W, FR_TW), tiles_y = cdiv(H, FR_TH);
    const long ntiles = (long)tiles_x * tiles_y;
    CF_REQUIRE(ntiles < (1L << 24), "map too large");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(flow_regularity_tile_kernel, dim3((unsigned)ntiles, (unsigned)(T * D)), dim3(256), 0, s, flow, labels, T, D, H, W, K, tiles_x, part);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(flow_regularity_reduce_kernel, dim3((unsigned)(T * D)), dim3(64), 0, s, (const double*)part, (int)ntiles, 5 + 3 * K, table);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_cine_ssim_table(const double* fixed, const float* registered, const uint8_t* labels, int T, int D, int H, int W, int K, int win,
                                  double K1, double K2, double cov_norm, float* range, double* part, double* table, void* stream) {
    CF_REQUIRE(fixed && registered && range && part && table, "null pointer");
    CF_REQUIRE(K >= 0 && K <= 16, "K must be 0..16, got %d", K);
    CF_REQUIRE(labels || K == 0, "labels may be null only with K = 0, got K=%d", K);
    CF_REQUIRE(T > 0 && D > 0 && H > 0 && W > 0, "bad shape T=%d D=%d H=%d W=%d", T, D, H, W);
    CF_REQUIRE((long)T * D <= 65535, "T * D = %ld slices exceed one grid dimension (65535)", (long)T * D);
    CF_REQUIRE((win & 1) && win >= 3 && win <= CS_MAXWIN, "win must be odd and 3..%d, got %d", CS_MAXWIN, win);
    CF_REQUIRE(win <= H && win <= W, "win=%d exceeds the image (H=%d W=%d)", win, H, W);
    const int tiles_x = cdiv(W, CS_TW), tiles_y = cdiv(H, CS_TH);
    const long ntiles = (long)tiles_x * tiles_y;
    CF_REQUIRE(ntiles < (1L << 24), "map too large");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(cine_ssim_range_kernel, dim3((unsigned)(T * D)), dim3(1024), 0, s, registered, (long)H * W, range);
    CF_CHECK_LAUNCH();
    const dim3 grid((unsigned)ntiles, (unsigned)(T * D));
#define CS_TILE(WIN)                                                                                                                              \
    case WIN:                                                                                                                                     \
        hipLaunchKernelGGL(cine_ssim_tile_kernel<WIN>, grid, dim3(256), 0, s, fixed, registered, labels, D, H, W, K, K1, K2, cov_norm, tiles_x, \
                           (const float*)range, part);                                                                                            \
        break;
    switch (win) { CS_TILE(3) CS_TILE(5) CS_TILE(7) CS_TILE(9) CS_TILE(11) CS_TILE(13) CS_TILE(15) }
#undef CS_TILE
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(flow_regularity_reduce_kernel, dim3((unsigned)(T * D)), dim3(64), 0, s, (const double*)part, (int)ntiles, 2 + 2 * K, table);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
