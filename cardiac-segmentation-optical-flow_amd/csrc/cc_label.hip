// Connected components for determine_postprocessing (nnunet/postprocessing/connected_components.py:123-447) in one visit per case:
//   * cf_cc_label     union-find labelling of EVERY region of a label map in one call, no host round trip;
//   * cf_cc_sizes     component sizes and the largest size per region id (optionally only among `alive` components);
//   * cf_pp_confusion TP / FP / FN per class of the raw prediction and of the three filtered variants the decision compares, without
//                     writing a filtered image;
//   * cf_cc_apply     the filtered image for "foreground step yes/no + this set of single classes".
// scipy.ndimage.label's default structure (face neighbours).  Labels use cf_cc_init's convention: 0 outside, else 1 + a voxel index of
// the component; after cf_cc_label that index is the smallest one, which is what converged cf_cc_sweep passes give as well.
//
// Ordering between the phases comes from kernel boundaries only; no kernel waits for another workgroup.
#include "common.h"

namespace cf {

#define GRID_STRIDE(i, n) for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

typedef unsigned long long u64;

struct RegionTable {
    uint8_t r[256];      // label value -> region id (0 = outside)
};

constexpr int TX = 32, TY = 8, TZ = 4, TILE = TX * TY * TZ, PER_THREAD = TILE / 256;

__global__ void __launch_bounds__(256) ccl_init_kernel(const uint8_t* __restrict__ image, int* __restrict__ labels, long n, RegionTable tab) {
    __shared__ uint8_t rt[256];
    rt[threadIdx.x] = tab.r[threadIdx.x];
    __syncthreads();
    GRID_STRIDE(i, n) labels[i] = rt[image[i]] ? (int)(i + 1) : 0;
}

// ---- union-find on "label = index + 1" arrays.  Invariant, in LDS and in global memory alike: L[x-1] <= x at all times (the init value is x
// and the only later write is an atomicMin), and L[x-1] always names a voxel of x's own component.  A stale read only returns an older
// such value, which keeps both properties, so the loops below are correct with plain (possibly L1-cached) loads.
//
// find: every step moves to a strictly smaller label (L[x-1] < x unless x is a root), so it ends after fewer than x steps.
template <typename T>
__device__ __forceinline__ int uf_find(const T* L, int x) {
    int p = L[x - 1];
    while (p != x) {
        x = p;
        p = L[x - 1];
    }
    return x;
}

// union: an iteration either returns (a == b, or the atomicMin found a still a root and hung it under b < a) or the atomicMin returned
// old != a.  Since L[a-1] <= a that means old < a, and the loop goes on with (old, b): a + b strictly decreases with every iteration that
// does not return and is bounded below by 2, so the loop terminates by construction.  When the atomicMin replaces a link a -> old by
// a -> b (old > b) the dropped link is restored by that next iteration, which unites old and b.
template <typename T>
__device__ __forceinline__ void uf_union(T* L, int a, int b) {
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin((int*)&L[a - 1], b);
        if (old == a) return;
        a = old;
    }
}

// One tile of TZ x TY x TX voxels per workgroup iteration: (1) union inside the tile in LDS, (2) hang every voxel under its tile-local root in
// the global array, (3) unite across the tile's low x / y / z faces.  Steps 2 and 3 go through uf_union only, which is safe whatever other
// workgroups are doing to the same entries at the same time.  The local index order (z, y, x) is the global order, so a tile-local root is
// the smallest global index of its piece.
__global__ void __launch_bounds__(256) ccl_merge_kernel(const uint8_t* __restrict__ image, int* labels, int D, int H, int W, int ntx, int nty,
                                                        long ntiles, RegionTable tab) {
    __shared__ uint8_t rt[256];
    __shared__ uint8_t rid[TILE];
    __shared__ int lp[TILE];
    rt[threadIdx.x] = tab.r[threadIdx.x];
    const long HW = (long)H * W;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = (int)(tile % ntx), ty = (int)((tile / ntx) % nty), tz = (int)(tile / ((long)ntx * nty));
        const int x0 = tx * TX, y0 = ty * TY, z0 = tz * TZ;
        __syncthreads();                                            // rt is written; the previous tile's LDS is no longer read
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const int t = threadIdx.x + 256 * k;
            const int x = x0 + (t % TX), y = y0 + (t / TX) % TY, z = z0 + t / (TX * TY);
            const bool in = x < W && y < H && z < D;
            rid[t] = in ? rt[image[(long)z * HW + (long)y * W + x]] : 0;
            lp[t] = t + 1;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const int t = threadIdx.x + 256 * k;
            const int r = rid[t];
            if (!r) continue;
            volatile int* vlp = lp;
            if ((t % TX) > 0 && rid[t - 1] == r) uf_union(vlp, t + 1, t);
            if ((t / TX) % TY > 0 && rid[t - TX] == r) uf_union(vlp, t + 1, t - TX + 1);
            if (t >= TX * TY && rid[t - TX * TY] == r) uf_union(vlp, t + 1, t - TX * TY + 1);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const int t = threadIdx.x + 256 * k;
            const int r = rid[t];
            if (!r) continue;
            const int lx = t % TX, ly = (t / TX) % TY, lz = t / (TX * TY);
            const long g = (long)(z0 + lz) * HW + (long)(y0 + ly) * W + (x0 + lx);
            const int root = uf_find(lp, t + 1) - 1;
            if (root != t) {
                const long gr = (long)(z0 + root / (TX * TY)) * HW + (long)(y0 + (root / TX) % TY) * W + (x0 + root % TX);
                uf_union(labels, (int)(g + 1), (int)(gr + 1));
            }
            if (lx == 0 && x0 > 0 && rt[image[g - 1]] == r) uf_union(labels, (int)(g + 1), (int)g);
            if (ly == 0 && y0 > 0 && rt[image[g - W]] == r) uf_union(labels, (int)(g + 1), (int)(g - W + 1));
            if (lz == 0 && z0 > 0 && rt[image[g - HW]] == r) uf_union(labels, (int)(g + 1), (int)(g - HW + 1));
        }
    }
}

// Path compression, after the merge kernel has ended: every entry becomes its root.  In place: a racing reader sees the old ancestor or the
// root, both of its own component, and roots are never rewritten.
__global__ void __launch_bounds__(256) ccl_compress_kernel(int* labels, long n) {
    GRID_STRIDE(i, n) {
        const int l = labels[i];
        if (l) labels[i] = uf_find(labels, l);
    }
}

// ---- sizes.  A workgroup counts a run of SZ_CHUNK voxels into an LDS hash table keyed by label and then adds every used slot to the global
// counter once: one global atomic per (workgroup pass, component).  At most SZ_CHUNK distinct keys meet 2 * SZ_CHUNK slots, so the linear
// probe always finds the key or an empty slot.
constexpr int SZ_CHUNK = 1024, SZ_SLOTS = 2 * SZ_CHUNK;

__global__ void __launch_bounds__(256) ccs_count_kernel(const int* __restrict__ labels, int* __restrict__ counts, long n) {
    __shared__ int keys[SZ_SLOTS];
    __shared__ int cnt[SZ_SLOTS];
    for (long base = (long)blockIdx.x * SZ_CHUNK; base < n; base += (long)gridDim.x * SZ_CHUNK) {
        for (int s = threadIdx.x; s < SZ_SLOTS; s += 256) { keys[s] = 0; cnt[s] = 0; }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SZ_CHUNK / 256; ++k) {
            const long i = base + threadIdx.x + 256 * k;
            const int l = i < n ? labels[i] : 0;
            if (!l) continue;
            unsigned h = ((unsigned)l * 2654435761u) >> 21;         // 11 bits
            for (;;) {
                const int prev = atomicCAS(&keys[h], 0, l);
                if (prev == 0 || prev == l) break;
                h = (h + 1) & (SZ_SLOTS - 1);
            }
            atomicAdd(&cnt[h], 1);
        }
        __syncthreads();
        for (int s = threadIdx.x; s < SZ_SLOTS; s += 256)
            if (keys[s]) atomicAdd(&counts[keys[s] - 1], cnt[s]);
        __syncthreads();
    }
}

// largest component per region id, read at the components' root voxels once the counts are complete.  A component is alive or dead as a whole
// (see cf_pp_confusion), so its root voxel answers for it.
__global__ void __launch_bounds__(256) ccs_max_kernel(const int* __restrict__ labels, const int* __restrict__ counts, const uint8_t* __restrict__ image,
                                                      const uint8_t* __restrict__ alive, long n, int* __restrict__ region_max,
                                                      int* __restrict__ region_max_alive, RegionTable tab) {
    __shared__ uint8_t rt[256];
    __shared__ int m[256], ma[256];
    rt[threadIdx.x] = tab.r[threadIdx.x];
    m[threadIdx.x] = 0;
    ma[threadIdx.x] = 0;
    __syncthreads();
    GRID_STRIDE(i, n) {
        if (labels[i] != (int)(i + 1)) continue;
        const int r = rt[image[i]], c = counts[i];
        atomicMax(&m[r], c);
        if (alive && alive[i]) atomicMax(&ma[r], c);
    }
    __syncthreads();
    if (m[threadIdx.x]) atomicMax(&region_max[threadIdx.x], m[threadIdx.x]);
    if (alive && ma[threadIdx.x]) atomicMax(&region_max_alive[threadIdx.x], ma[threadIdx.x]);
}

// connected_components.py:90-101 (cc_remove_kernel's rule): an object goes when its size differs from the region's largest and it is smaller
// than min_valid (min_valid < 0: always).  Ties with the largest stay.
__device__ __forceinline__ bool cc_goes(int count, int max_count, double vpv, double min_valid) {
    return count != max_count && (min_valid < 0.0 || (double)count * vpv < min_valid);
}

constexpr int PP_KMAX = 16;

struct PPArgs {
    const uint8_t *pred, *gt;
    const int *lf, *cf, *lc, *cc;              // foreground-joint labels / counts, per-class labels / counts
    const int *fmax, *cmax_raw, *cmax_alive;   // region_max tables [256]
    long n, HW;
    int K;
    double vpv;
    double mv[PP_KMAX + 1];                    // [0] the foreground region, [c] class c
    int zskip[PP_KMAX];
};

// out[v][c] = {TP, FP, FN} of class c for v = raw, foreground-filtered, per-class-filtered raw, per-class-filtered after the foreground filter.
// The fourth variant: a class component is face-connected and all foreground, so it lies inside exactly one foreground component; removing
// whole foreground components removes whole class components and never splits one.  The survivors keep their sizes; only the per-class
// maximum changes, and cmax_alive is that maximum among the survivors.
__global__ void __launch_bounds__(256) pp_confusion_kernel(PPArgs a, u64* __restrict__ out) {
    __shared__ unsigned h[4 * PP_KMAX * 3];
    __shared__ int cmr[PP_KMAX], cma[PP_KMAX], zs[PP_KMAX];
    __shared__ double mv[PP_KMAX + 1];
    for (int k = threadIdx.x; k < 4 * PP_KMAX * 3; k += 256) h[k] = 0;
    if (threadIdx.x < a.K) { cmr[threadIdx.x] = a.cmax_raw[threadIdx.x]; cma[threadIdx.x] = a.cmax_alive[threadIdx.x]; }
    if (threadIdx.x < PP_KMAX) zs[threadIdx.x] = a.zskip[threadIdx.x];
    if (threadIdx.x <= PP_KMAX) mv[threadIdx.x] = a.mv[threadIdx.x];
    const int fmax = a.fmax[1];
    const int K = a.K;
    __syncthreads();
    unsigned bb = 0;                                               // background in both volumes: TP of class 0 in every variant
    GRID_STRIDE(i, a.n) {
        const int p = a.pred[i], g = a.gt[i];
        const int z = (int)(i / a.HW);
        if (p == 0 && g == 0) {
            bb += z >= zs[0];
            continue;
        }
        bool fr = false, cr = false, ca = false;
        if (p) {
            const int l = a.lf[i];
            fr = l && cc_goes(a.cf[l - 1], fmax, a.vpv, mv[0]);
            const int l2 = p < K ? a.lc[i] : 0;
            if (l2) {
                const int c = a.cc[l2 - 1];
                cr = cc_goes(c, cmr[p], a.vpv, mv[p]);
                ca = cc_goes(c, cma[p], a.vpv, mv[p]);
            }
        }
        const int pv[4] = {p, fr ? 0 : p, cr ? 0 : p, (fr || ca) ? 0 : p};
        const bool gin = g < K && z >= zs[g < K ? g : 0];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int q = pv[v];
            const bool qin = q < K && z >= zs[q < K ? q : 0];
            if (q == g) {
                if (qin) atomicAdd(&h[(v * PP_KMAX + q) * 3], 1u);
            } else {
                if (qin) atomicAdd(&h[(v * PP_KMAX + q) * 3 + 1], 1u);
                if (gin) atomicAdd(&h[(v * PP_KMAX + g) * 3 + 2], 1u);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) bb += __shfl_xor(bb, o, 64);
    if ((threadIdx.x & 63) == 0 && bb)
        for (int v = 0; v < 4; ++v) atomicAdd(&h[v * PP_KMAX * 3], bb);
    __syncthreads();
    for (int k = threadIdx.x; k < 4 * PP_KMAX * 3; k += 256) {
        const int v = k / (PP_KMAX * 3), c = (k / 3) % PP_KMAX, j = k % 3;
        if (h[k] && c < K) atomicAdd(&out[((long)v * K + c) * 3 + j], (u64)h[k]);
    }
}

struct ApplyArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int *lf, *cf, *lc, *cc, *fmax, *cmax;
    long n;
    int K, do_fg;
    unsigned class_bits;
    double vpv;
    double mv[PP_KMAX + 1];
};

__global__ void __launch_bounds__(256) cc_apply_kernel(ApplyArgs a) {
    __shared__ double mv[PP_KMAX + 1];
    if (threadIdx.x <= PP_KMAX) mv[threadIdx.x] = a.mv[threadIdx.x];
    __syncthreads();
    const int fmax = a.do_fg ? a.fmax[1] : 0;
    GRID_STRIDE(i, a.n) {
        const int p = a.src[i];
        int q = p;
        if (p) {
            if (a.do_fg) {
                const int l = a.lf[i];
                if (l && cc_goes(a.cf[l - 1], fmax, a.vpv, mv[0])) q = 0;
            }
            if (q && p < a.K && ((a.class_bits >> p) & 1u)) {
                const int l = a.lc[i];
                if (l && cc_goes(a.cc[l - 1], a.cmax[p], a.vpv, mv[p])) q = 0;
            }
        }
        a.dst[i] = (uint8_t)q;
    }
}

}  // namespace cf

using namespace cf;

#define CHECK_HIP(call, msg)                  \
    do {                                      \
        if ((call) != hipSuccess) {           \
            cf::set_error(msg);               \
            return CF_ERR_LAUNCH;             \
        }                                     \
    } while (0)

static RegionTable make_table(const uint8_t* region_of) {
    RegionTable t;
    for (int k = 0; k < 256; ++k) t.r[k] = region_of[k];
    return t;
}

extern "C" int cf_cc_label(const uint8_t* image, int* labels, int D, int H, int W, const uint8_t* region_of, void* stream) {
    CF_REQUIRE(image && labels && region_of, "null pointer");
    CF_REQUIRE(D > 0 && H > 0 && W > 0 && (long)D * H * W < (1L << 31) - 1, "bad shape");
    CF_REQUIRE(region_of[0] == 0, "label 0 is the background: region_of[0] must be 0");
    const long n = (long)D * H * W;
    const RegionTable tab = make_table(region_of);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ccl_init_kernel, dim3(flat_grid(n, 256, 4)), dim3(256), 0, s, image, labels, n, tab);
    CF_CHECK_LAUNCH();
    const int ntx = cdiv(W, TX), nty = cdiv(H, TY), ntz = cdiv(D, TZ);
    const long ntiles = (long)ntx * nty * ntz;
    hipLaunchKernelGGL(ccl_merge_kernel, dim3((unsigned)(ntiles < 65536 ? ntiles : 65536)), dim3(256), 0, s, image, labels, D, H, W, ntx, nty,
                       ntiles, tab);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_compress_kernel, dim3(flat_grid(n, 256, 4)), dim3(256), 0, s, labels, n);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_cc_sizes(const int* labels, const uint8_t* image, const uint8_t* region_of, const uint8_t* alive, long n, int* counts,
                           int* region_max, int* region_max_alive, void* stream) {
    CF_REQUIRE(labels && image && region_of && counts && region_max, "null pointer");
    CF_REQUIRE(n > 0 && n < (1L << 31) - 1, "bad size");
    CF_REQUIRE((alive != nullptr) == (region_max_alive != nullptr), "alive and region_max_alive go together");
    hipStream_t s = as_stream(stream);
    CHECK_HIP(hipMemsetAsync(counts, 0, n * sizeof(int), s), "cf_cc_sizes: memset failed");
    CHECK_HIP(hipMemsetAsync(region_max, 0, 256 * sizeof(int), s), "cf_cc_sizes: memset failed");
    if (region_max_alive) CHECK_HIP(hipMemsetAsync(region_max_alive, 0, 256 * sizeof(int), s), "cf_cc_sizes: memset failed");
    hipLaunchKernelGGL(ccs_count_kernel, dim3(flat_grid(n, SZ_CHUNK)), dim3(256), 0, s, labels, counts, n);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccs_max_kernel, dim3(flat_grid(n, 256, 4)), dim3(256), 0, s, labels, (const int*)counts, image, alive, n, region_max,
                       region_max_alive, make_table(region_of));
    CF_CHECK_LAUNCH();
    return CF_OK;
}

static bool fill_min_valid(double* mv, const double* min_valid, int K) {
    for (int k = 0; k <= PP_KMAX; ++k) mv[k] = -1.0;
    if (min_valid)
        for (int k = 0; k < K; ++k) mv[k] = min_valid[k];
    return true;
}

extern "C" int cf_pp_confusion(const uint8_t* pred, const uint8_t* gt, int D, int H, int W, int K, const int* labels_fg, const int* counts_fg,
                               const int* max_fg, const int* labels_cls, const int* counts_cls, const int* max_cls, const int* max_cls_alive,
                               double volume_per_voxel, const double* min_valid, const int* z_skip, unsigned long long* out, void* stream) {
    CF_REQUIRE(pred && gt && labels_fg && counts_fg && max_fg && labels_cls && counts_cls && max_cls && max_cls_alive && out, "null pointer");
    CF_REQUIRE(D > 0 && H > 0 && W > 0 && (long)D * H * W < (1L << 31) - 1, "bad shape");
    CF_REQUIRE(K >= 1 && K <= PP_KMAX, "K must be 1..16, got %d", K);
    PPArgs a;
    a.pred = pred; a.gt = gt; a.lf = labels_fg; a.cf = counts_fg; a.lc = labels_cls; a.cc = counts_cls;
    a.fmax = max_fg; a.cmax_raw = max_cls; a.cmax_alive = max_cls_alive;
    a.n = (long)D * H * W; a.HW = (long)H * W; a.K = K; a.vpv = volume_per_voxel;
    fill_min_valid(a.mv, min_valid, K);
    for (int k = 0; k < PP_KMAX; ++k) a.zskip[k] = (z_skip && k < K) ? z_skip[k] : 0;
    hipStream_t s = as_stream(stream);
    CHECK_HIP(hipMemsetAsync(out, 0, (size_t)4 * K * 3 * sizeof(u64), s), "cf_pp_confusion: memset failed");
    hipLaunchKernelGGL(pp_confusion_kernel, dim3(flat_grid(a.n, 256, 16)), dim3(256), 0, s, a, out);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_cc_apply(const uint8_t* src, uint8_t* dst, long n, int K, int do_fg, int class_bits, const int* labels_fg,
                           const int* counts_fg, const int* max_fg, const int* labels_cls, const int* counts_cls, const int* max_cls,
                           double volume_per_voxel, const double* min_valid, void* stream) {
    CF_REQUIRE(src && dst && n > 0, "bad arguments");
    CF_REQUIRE(K >= 1 && K <= PP_KMAX, "K must be 1..16, got %d", K);
    CF_REQUIRE(class_bits >= 0 && (class_bits & 1) == 0 && (class_bits >> K) == 0, "class_bits names a class outside 1..K-1");
    CF_REQUIRE(!do_fg || (labels_fg && counts_fg && max_fg), "the foreground step needs its labels, counts and maximum");
    CF_REQUIRE(!class_bits || (labels_cls && counts_cls && max_cls), "the per-class step needs its labels, counts and maxima");
    ApplyArgs a;
    a.src = src; a.dst = dst; a.lf = labels_fg; a.cf = counts_fg; a.lc = labels_cls; a.cc = counts_cls; a.fmax = max_fg; a.cmax = max_cls;
    a.n = n; a.K = K; a.do_fg = do_fg; a.class_bits = (unsigned)class_bits; a.vpv = volume_per_voxel;
    fill_min_valid(a.mv, min_valid, K);
    hipLaunchKernelGGL(cc_apply_kernel, dim3(flat_grid(n, 256, 4)), dim3(256), 0, as_stream(stream), a);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
