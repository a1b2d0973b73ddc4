// Exact Euclidean distance transform and the evaluator's surface visit built on it.
//   * scipy.ndimage.distance_transform_edt(input, sampling): every voxel's distance to the nearest voxel whose value is 0, defined as the
//     minimum over those voxels of sqrt(fl(fl(fl((sz dz)^2) + fl((sy dy)^2)) + fl((sx dx)^2))) -- surface_min_dist_kernel's expression in
//     surface_min_dist_kernel's order, which is what scipy evaluates on the integer offsets of its feature transform;
//   * medpy's __surface_distances behind hd / hd95 / asd / assd for every listed label of two label volumes: the border voxels of
//     `test == c` and `reference == c` (surface_border_kernel's rule) and, for each of them, the distance to the nearest border voxel of
//     the other volume, read from the transform instead of searched over pairs.
// Three separable passes that carry the nearest zero's integer offsets (|dx|, then |dx| and |dy|) and evaluate the expression only at the
// end, so the bits are those of the definition whenever the products are exact, and within the roundings of the expression otherwise:
//   x  one wave per row: the nearest zero to the left by a ballot scan, then to the right, 64 voxels per step;
//   y  one thread per voxel, lanes along x: the column is walked outwards from the voxel, both ways at once, until (sy k)^2 alone is
//      no smaller than the best candidate -- at most H steps, in practice about the distance itself; every step reads 64 contiguous values;
//   z  the same walk over the (|dx|, |dy|) pairs with the full expression as the cost.
// Work is O(N max(D, H, W)) at the worst and never a search over pairs.  The file is built with -ffp-contract=off.
#include "common.h"

namespace cf {

typedef unsigned long long u64;

constexpr unsigned NONE16 = 0xFFFFu;          // no zero in this row
constexpr unsigned NONE32 = 0xFFFFFFFFu;      // no zero in this plane
constexpr int EDT_MAX_EXTENT = 65534;         // offsets travel as uint16
constexpr int EDT_MAX_LABELS = 16;

// ---- workspace: header | scan u64 [nb + 1] | flags u8 [N] | ox u16 [N] | pack u32 [N]      (nb = ceil(N / 256))
struct LabelState {                            // one per listed label, 128 bytes
    int lo[3], hi[3];                          // joint bounding box of the two border sets (z, y, x), hi < lo when there is nothing to do
    int valid, pad;
    u64 other[2];                              // nonzero when test / reference holds a voxel that is NOT the label (the label does not fill it)
    u64 seg[2];                                // first slot of the test->ref / ref->test distances
    u64 cnt[2];                                // border voxels of test / reference
    u64 spare[6];
};
struct Header {
    int box_lo[3], box_hi[3];                  // cf_edt's box: the whole volume
    int status, pad;                           // cf_edt: 1 when some voxel found no zero
    u64 cursor;                                // next free slot of the distance buffer
    u64 spare[3];
    LabelState lab[EDT_MAX_LABELS];
};
constexpr long EDT_HEADER_BYTES = 4096;
static_assert(sizeof(LabelState) == 128 && sizeof(Header) <= EDT_HEADER_BYTES, "workspace header layout");

static inline long align256(long v) { return (v + 255) / 256 * 256; }
struct Layout {
    long nb, scan, flags, ox, pack, total;
};
static inline Layout edt_layout(long D, long H, long W) {
    Layout l;
    const long n = D * H * W;
    l.nb = (n + 255) / 256;
    l.scan = EDT_HEADER_BYTES;
    l.flags = l.scan + align256((l.nb + 1) * 8);
    l.ox = l.flags + align256(n);
    l.pack = l.ox + align256(2 * n);
    l.total = l.pack + align256(4 * n);
    return l;
}

__device__ __forceinline__ double sq_rn(double s, unsigned k) {
    const double d = __dmul_rn(s, (double)k);
    return __dmul_rn(d, d);
}

__global__ void edt_init_kernel(Header* __restrict__ h, int D, int H, int W) {
    const int t = threadIdx.x;
    if (t == 0) {
        h->box_lo[0] = h->box_lo[1] = h->box_lo[2] = 0;
        h->box_hi[0] = D - 1; h->box_hi[1] = H - 1; h->box_hi[2] = W - 1;
        h->status = 0;
        h->cursor = 0;
    }
    if (t < EDT_MAX_LABELS) {
        LabelState& s = h->lab[t];
        s.lo[0] = s.lo[1] = s.lo[2] = 0x7FFFFFFF;
        s.hi[0] = s.hi[1] = s.hi[2] = -1;
        s.valid = 0;
        s.other[0] = s.other[1] = s.seg[0] = s.seg[1] = s.cnt[0] = s.cnt[1] = 0;
    }
}

// x pass.  A voxel is a zero of the transform when ((src[i] & bit) != 0) != invert: invert = 1, bit = 0xFF reads a mask (zero where the mask
// is 0), invert = 0 reads one bit of the border flags.  One wave per row of the box; ox = |x - nearest zero of the row|, NONE16 without one.
__global__ void __launch_bounds__(256) edt_x_kernel(const uint8_t* __restrict__ src, int bit, int invert, const int* __restrict__ box, int H, int W,
                                                    uint16_t* __restrict__ ox) {
    const int z0 = box[0], y0 = box[1], x0 = box[2], z1 = box[3], y1 = box[4], x1 = box[5];
    if (z1 < z0 || y1 < y0 || x1 < x0) return;
    const long bh = y1 - y0 + 1, rows = (long)(z1 - z0 + 1) * bh;
    const int lane = threadIdx.x & 63;
    const long wave = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = (long)gridDim.x * (blockDim.x >> 6);
    const int last_chunk = x0 + (x1 - x0) / 64 * 64;
    for (long r = wave; r < rows; r += nwaves) {
        const long base = ((long)(z0 + r / bh) * H + (y0 + r % bh)) * W;
        int seen = -1;
        for (int xc = x0; xc <= x1; xc += 64) {                         // nearest zero at or to the left
            const int x = xc + lane;
            const bool in = x <= x1;
            const bool zero = in && (((src[base + x] & bit) != 0) != (invert != 0));
            const u64 b = __ballot(zero);
            const u64 low = b & ((2ull << lane) - 1ull);
            const int l = low ? xc + 63 - __clzll((long long)low) : seen;
            if (in) ox[base + x] = (uint16_t)(l < 0 ? NONE16 : (unsigned)(x - l));
            if (b) seen = xc + 63 - __clzll((long long)b);
        }
        seen = -1;
        for (int xc = last_chunk; xc >= x0; xc -= 64) {                  // nearest zero at or to the right, the smaller of the two kept
            const int x = xc + lane;
            const bool in = x <= x1;
            const unsigned left = in ? ox[base + x] : NONE16;
            const u64 b = __ballot(in && left == 0);
            const u64 high = b & ~((1ull << lane) - 1ull);
            const int rr = high ? xc + __ffsll((long long)high) - 1 : seen;
            if (in && rr >= 0) {
                const unsigned right = (unsigned)(rr - x);
                if (right < left) ox[base + x] = (uint16_t)right;
            }
            if (b) seen = xc + __ffsll((long long)b) - 1;
        }
    }
}

// y pass: pack = |dx| | |dy| << 16 of the zero of plane z that is nearest in (y, x), NONE32 when the plane has none in the box
__global__ void __launch_bounds__(256) edt_y_kernel(const uint16_t* __restrict__ ox, const int* __restrict__ box, int H, int W, double sy, double sx,
                                                    unsigned* __restrict__ pack) {
    const int z0 = box[0], y0 = box[1], x0 = box[2], z1 = box[3], y1 = box[4], x1 = box[5];
    if (z1 < z0 || y1 < y0 || x1 < x0) return;
    const long bw = x1 - x0 + 1, bh = y1 - y0 + 1, total = (long)(z1 - z0 + 1) * bh * bw;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long t = i / bw;
        const int x = x0 + (int)(i - t * bw), y = y0 + (int)(t % bh), z = z0 + (int)(t / bh);
        const long idx = ((long)z * H + y) * W + x;
        double best = INFINITY;
        unsigned win = NONE32;
        unsigned o = ox[idx];
        if (o != NONE16) { best = sq_rn(sx, o); win = o; }
        for (int k = 1; best > 0.0; ++k) {
            const double ty = sq_rn(sy, (unsigned)k);
            const bool up = y - k >= y0, dn = y + k <= y1;
            if (ty >= best || !(up || dn)) break;
            if (up) {
                o = ox[idx - (long)k * W];
                if (o != NONE16) {
                    const double c = __dadd_rn(ty, sq_rn(sx, o));
                    if (c < best) { best = c; win = o | ((unsigned)k << 16); }
                }
            }
            if (dn) {
                o = ox[idx + (long)k * W];
                if (o != NONE16) {
                    const double c = __dadd_rn(ty, sq_rn(sx, o));
                    if (c < best) { best = c; win = o | ((unsigned)k << 16); }
                }
            }
        }
        pack[idx] = win;
    }
}

// z walk of one voxel: min over the planes z' in [z0, z1] of fl(fl(fl((sz dz)^2) + fl((sy dy)^2)) + fl((sx dx)^2)); INFINITY without a zero
__device__ __forceinline__ double edt_z_walk(const unsigned* __restrict__ pack, long idx, int z, int z0, int z1, long HW, double sz, double sy, double sx) {
    double best = INFINITY;
    unsigned p = pack[idx];
    if (p != NONE32) best = __dadd_rn(sq_rn(sy, p >> 16), sq_rn(sx, p & 0xFFFFu));
    for (int k = 1; best > 0.0; ++k) {
        const double tz = sq_rn(sz, (unsigned)k);
        const bool up = z - k >= z0, dn = z + k <= z1;
        if (tz >= best || !(up || dn)) break;
        if (up) {
            p = pack[idx - (long)k * HW];
            if (p != NONE32) best = fmin(best, __dadd_rn(__dadd_rn(tz, sq_rn(sy, p >> 16)), sq_rn(sx, p & 0xFFFFu)));
        }
        if (dn) {
            p = pack[idx + (long)k * HW];
            if (p != NONE32) best = fmin(best, __dadd_rn(__dadd_rn(tz, sq_rn(sy, p >> 16)), sq_rn(sx, p & 0xFFFFu)));
        }
    }
    return best;
}

// z pass of cf_edt: every voxel of the volume
__global__ void __launch_bounds__(256) edt_z_kernel(const unsigned* __restrict__ pack, int D, long HW, double sz, double sy, double sx,
                                                    double* __restrict__ out, int* __restrict__ status) {
    const long n = (long)D * HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double d2 = edt_z_walk(pack, i, (int)(i / HW), 0, D - 1, HW, sz, sy, sx);
        if (d2 == INFINITY) *status = 1;
        out[i] = sqrt(d2);
    }
}

// ---- the evaluator's visit, label by label -------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_border(const uint8_t* __restrict__ v, int c, long i, int z, int y, int x, int D, int H, int W, long HW, int ndim) {
    if (v[i] != c) return false;
    bool b = x == 0 || x == W - 1 || y == 0 || y == H - 1 || v[i - 1] != c || v[i + 1] != c || v[i - W] != c || v[i + W] != c;
    if (ndim == 3) b = b || z == 0 || z == D - 1 || v[i - HW] != c || v[i + HW] != c;
    return b;
}

// flags[i] = (border of test == c) | (border of reference == c) << 1; block b's two counts go to scan[b] (test low, reference high word),
// whether either volume holds anything but the label, and the joint bounding box, to its state.  Block b owns the voxels 256 b .. 256 b + 255.
__global__ void __launch_bounds__(256) edt_flag_kernel(const uint8_t* __restrict__ test, const uint8_t* __restrict__ ref, int c, int D, int H, int W, int ndim,
                                                       uint8_t* __restrict__ flags, u64* __restrict__ scan, LabelState* __restrict__ st) {
    const long HW = (long)H * W, n = (long)D * HW;
    const long i = blockIdx.x * 256L + threadIdx.x;
    bool bt = false, br = false, vt = false, vr = false;
    int z = 0, y = 0, x = 0;
    if (i < n) {
        z = (int)(i / HW);
        const int q = (int)(i - (long)z * HW);
        y = q / W;
        x = q - y * W;
        vt = test[i] == c;
        vr = ref[i] == c;
        bt = vt && is_border(test, c, i, z, y, x, D, H, W, HW, ndim);
        br = vr && is_border(ref, c, i, z, y, x, D, H, W, HW, ndim);
        flags[i] = (uint8_t)((bt ? 1 : 0) | (br ? 2 : 0));
    }
    __shared__ unsigned cnt[4][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 mt = __ballot(bt), mr = __ballot(br);
    const bool ot = __any(i < n && !vt), orf = __any(i < n && !vr);
    if (mt | mr) {                                                       // wave-uniform
        const bool any = bt || br;
        int lo0 = any ? z : 0x7FFFFFFF, lo1 = any ? y : 0x7FFFFFFF, lo2 = any ? x : 0x7FFFFFFF;
        int hi0 = any ? z : -1, hi1 = any ? y : -1, hi2 = any ? x : -1;
        for (int o = 32; o > 0; o >>= 1) {
            lo0 = min(lo0, __shfl_xor(lo0, o, 64)); lo1 = min(lo1, __shfl_xor(lo1, o, 64)); lo2 = min(lo2, __shfl_xor(lo2, o, 64));
            hi0 = max(hi0, __shfl_xor(hi0, o, 64)); hi1 = max(hi1, __shfl_xor(hi1, o, 64)); hi2 = max(hi2, __shfl_xor(hi2, o, 64));
        }
        // an atomic only where it can still move the box: the value read may be stale, but the box only grows, so a stale value errs towards
        // one atomic too many, never one too few (tens of thousands of same-address atomics per label otherwise: they serialise)
        if (lane == 0) {
            const int l0 = lo0, l1 = lo1, l2 = lo2, h0 = hi0, h1 = hi1, h2 = hi2;
            if (l0 < __hip_atomic_load(&st->lo[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&st->lo[0], l0);
            if (l1 < __hip_atomic_load(&st->lo[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&st->lo[1], l1);
            if (l2 < __hip_atomic_load(&st->lo[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&st->lo[2], l2);
            if (h0 > __hip_atomic_load(&st->hi[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&st->hi[0], h0);
            if (h1 > __hip_atomic_load(&st->hi[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&st->hi[1], h1);
            if (h2 > __hip_atomic_load(&st->hi[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&st->hi[2], h2);
        }
    }
    if (lane == 0) {
        cnt[w][0] = __popcll(mt); cnt[w][1] = __popcll(mr);
        // "the label does not fill this volume": every writer stores the same value, and only until somebody's store has become visible
        if (ot && !__hip_atomic_load(&st->other[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) st->other[0] = 1;
        if (orf && !__hip_atomic_load(&st->other[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) st->other[1] = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 t = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0], r = cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1];
        scan[blockIdx.x] = t | (r << 32);
    }
}

// exclusive scan of scan[0 .. nb) in place (both 32-bit halves at once: neither half reaches 2^31), the totals into scan[nb].  Then the
// label's decision, by thread 0: a label that is empty or -- unless score_full -- full in either volume, or whose distances would not fit
// the buffer, gets two empty segments and an empty box, so that every later launch of the label finds nothing to do.
__global__ void __launch_bounds__(1024) edt_scan_kernel(u64* __restrict__ scan, long nb, long capacity, int score_full, int slot, int K,
                                                        Header* __restrict__ h, double* __restrict__ head) {
    __shared__ u64 wsum[16];
    __shared__ u64 carry_s;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (long b0 = 0; b0 < nb; b0 += 4096) {                             // four consecutive entries per thread
        const long b = b0 + 4L * threadIdx.x;
        u64 v[4], own = 0;
        for (int j = 0; j < 4; ++j) { v[j] = b + j < nb ? scan[b + j] : 0; own += v[j]; }
        u64 inc = own;
        for (int o = 1; o < 64; o <<= 1) {
            const u64 up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        u64 before = carry_s;
        for (int j = 0; j < w; ++j) before += wsum[j];
        u64 run = before + inc - own;
        for (int j = 0; j < 4; ++j) {
            if (b + j < nb) scan[b + j] = run;
            run += v[j];
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const u64 tot = carry_s;
        scan[nb] = tot;
        LabelState& s = h->lab[slot];
        u64 ct = tot & 0xFFFFFFFFull, cr = tot >> 32;
        s.cnt[0] = ct; s.cnt[1] = cr;
        bool ok = ct > 0 && cr > 0 && (score_full || (s.other[0] && s.other[1]));
        if (ok && h->cursor + ct + cr > (u64)capacity) { ok = false; head[2 * K + 1 + 8 * K] = 1.0; }
        if (!ok) {
            s.lo[0] = s.lo[1] = s.lo[2] = 0; s.hi[0] = s.hi[1] = s.hi[2] = -1;
            ct = cr = 0;
        }
        s.valid = ok ? 1 : 0;
        s.seg[0] = h->cursor; s.seg[1] = h->cursor + ct;
        h->cursor += ct + cr;
        head[2 * slot + 1] = (double)s.seg[1];
        head[2 * slot + 2] = (double)h->cursor;
        double* row = head + 2 * K + 1 + 8 * slot;
        row[0] = (double)ct; row[1] = (double)cr;
        row[2] = row[3] = row[4] = row[5] = 0.0;
        row[6] = (double)s.cnt[0]; row[7] = (double)s.cnt[1];
    }
}

// z pass of the visit, only where it is read: the border voxels of side `dir` (0 test, 1 reference), in raster order.  A voxel's slot is
// the segment's start + the scanned count of the blocks before its own + its rank inside the block: no atomics, the same order every run.
__global__ void __launch_bounds__(256) edt_gather_kernel(const uint8_t* __restrict__ flags, const unsigned* __restrict__ pack, const u64* __restrict__ scan,
                                                         const LabelState* __restrict__ st, int dir, int D, int H, int W, double sz, double sy, double sx,
                                                         double* __restrict__ dist) {
    if (!st->valid) return;
    const int sh = dir ? 32 : 0;
    const u64 before = (scan[blockIdx.x] >> sh) & 0xFFFFFFFFull, after = (scan[blockIdx.x + 1] >> sh) & 0xFFFFFFFFull;
    if (after == before) return;
    const long HW = (long)H * W, n = (long)D * HW;
    const long i = blockIdx.x * 256L + threadIdx.x;
    const bool has = i < n && ((flags[i] >> dir) & 1);
    __shared__ unsigned wcnt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 m = __ballot(has);
    if (lane == 0) wcnt[w] = __popcll(m);
    __syncthreads();
    if (!has) return;
    unsigned rank = __popcll(m & ((1ull << lane) - 1ull));
    for (int j = 0; j < w; ++j) rank += wcnt[j];
    const int z = (int)(i / HW);
    const double d2 = edt_z_walk(pack, i, z, st->lo[0], st->hi[0], HW, sz, sy, sx);
    dist[st->seg[dir] + before + rank] = sqrt(d2);
}

// max and sum of the label's two segments, one workgroup each, in a fixed order: thread t takes the elements t, t + 1024, ... one after
// another, then a fixed tree over the threads
__global__ void __launch_bounds__(1024) edt_reduce_kernel(const double* __restrict__ dist, const LabelState* __restrict__ st, int slot, int K,
                                                          double* __restrict__ head) {
    const int dir = blockIdx.x;
    const u64 cnt = st->valid ? st->cnt[dir] : 0;
    const double* d = dist + st->seg[dir];
    double mx = 0.0, sm = 0.0;
    for (u64 e = threadIdx.x; e < cnt; e += 1024) { mx = fmax(mx, d[e]); sm += d[e]; }
    for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_xor(mx, o, 64)); sm += __shfl_xor(sm, o, 64); }
    __shared__ double rm[16], rs[16];
    if ((threadIdx.x & 63) == 0) { rm[threadIdx.x >> 6] = mx; rs[threadIdx.x >> 6] = sm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = rm[0]; sm = rs[0];
        for (int j = 1; j < 16; ++j) { mx = fmax(mx, rm[j]); sm += rs[j]; }
        double* row = head + 2 * K + 1 + 8 * slot;
        row[2 + dir] = mx;
        row[4 + dir] = sm;
    }
}

}  // namespace cf

using namespace cf;

static bool edt_shape_ok(int D, int H, int W, int ndim) {
    return D > 0 && H > 0 && W > 0 && D <= EDT_MAX_EXTENT && H <= EDT_MAX_EXTENT && W <= EDT_MAX_EXTENT && (ndim == 3 || (ndim == 2 && D == 1));
}

extern "C" long cf_edt_workspace_bytes(int D, int H, int W) {
    if (!edt_shape_ok(D, H, W, 3)) { set_error("cf_edt_workspace_bytes: bad shape"); return CF_ERR_ARG; }
    return edt_layout(D, H, W).total;
}

static inline int row_grid(long rows) {                  // 4 rows (waves) per block
    long b = (rows + 3) / 4;
    if (b < 1) b = 1;
    if (b > 256L * 32) b = 256L * 32;
    return (int)b;
}

extern "C" int cf_edt(const uint8_t* mask, int D, int H, int W, int ndim, double sz, double sy, double sx, void* ws, double* out, void* stream) {
    CF_REQUIRE(mask && ws && out, "null pointer");
    CF_REQUIRE(edt_shape_ok(D, H, W, ndim), "bad shape D=%d H=%d W=%d ndim=%d (extents 1..%d; ndim 3, or 2 with D == 1)", D, H, W, ndim, EDT_MAX_EXTENT);
    CF_REQUIRE(sz > 0.0 && sy > 0.0 && sx > 0.0, "spacing must be positive");
    CF_REQUIRE(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    const Layout l = edt_layout(D, H, W);
    char* base = reinterpret_cast<char*>(ws);
    Header* h = reinterpret_cast<Header*>(base);
    uint16_t* ox = reinterpret_cast<uint16_t*>(base + l.ox);
    unsigned* pack = reinterpret_cast<unsigned*>(base + l.pack);
    const long HW = (long)H * W, n = (long)D * HW;
    hipLaunchKernelGGL(edt_init_kernel, dim3(1), dim3(64), 0, s, h, D, H, W);
    hipLaunchKernelGGL(edt_x_kernel, dim3(row_grid((long)D * H)), dim3(256), 0, s, mask, 0xFF, 1, h->box_lo, H, W, ox);
    hipLaunchKernelGGL(edt_y_kernel, dim3(flat_grid(n, 256, 4)), dim3(256), 0, s, ox, h->box_lo, H, W, sy, sx, pack);
    hipLaunchKernelGGL(edt_z_kernel, dim3(flat_grid(n, 256, 4)), dim3(256), 0, s, pack, D, HW, sz, sy, sx, out, &h->status);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_label_surface_edt(const uint8_t* test, const uint8_t* reference, int D, int H, int W, int ndim, const int* labels, int K, double sz,
                                    double sy, double sx, int score_full, void* ws, double* dist, long capacity, double* head, void* stream) {
    CF_REQUIRE(test && reference && labels && ws && dist && head, "null pointer");
    CF_REQUIRE(edt_shape_ok(D, H, W, ndim), "bad shape D=%d H=%d W=%d ndim=%d (extents 1..%d; ndim 3, or 2 with D == 1)", D, H, W, ndim, EDT_MAX_EXTENT);
    CF_REQUIRE((long)D * H * W < (1L << 31), "volumes of 2^31 voxels or more are not built (the border counts travel as 32-bit halves)");
    CF_REQUIRE(K >= 1 && K <= EDT_MAX_LABELS, "K must be 1..%d, got %d", EDT_MAX_LABELS, K);
    for (int k = 0; k < K; ++k) CF_REQUIRE(labels[k] >= 0 && labels[k] <= 255, "label %d is no uint8 value", labels[k]);
    CF_REQUIRE(sz > 0.0 && sy > 0.0 && sx > 0.0, "spacing must be positive");
    CF_REQUIRE(capacity > 0, "capacity must be positive");
    CF_REQUIRE(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    const Layout l = edt_layout(D, H, W);
    char* base = reinterpret_cast<char*>(ws);
    Header* h = reinterpret_cast<Header*>(base);
    u64* scan = reinterpret_cast<u64*>(base + l.scan);
    uint8_t* flags = reinterpret_cast<uint8_t*>(base + l.flags);
    uint16_t* ox = reinterpret_cast<uint16_t*>(base + l.ox);
    unsigned* pack = reinterpret_cast<unsigned*>(base + l.pack);
    const long n = (long)D * H * W;
    const int nb = (int)l.nb;
    if (hipMemsetAsync(head, 0, (size_t)(2 * K + 1 + 8 * K + 1) * sizeof(double), s) != hipSuccess) {
        set_error("cf_label_surface_edt: memset failed");
        return CF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(edt_init_kernel, dim3(1), dim3(64), 0, s, h, D, H, W);
    for (int k = 0; k < K; ++k) {
        LabelState* st = &h->lab[k];
        hipLaunchKernelGGL(edt_flag_kernel, dim3(nb), dim3(256), 0, s, test, reference, labels[k], D, H, W, ndim, flags, scan, st);
        hipLaunchKernelGGL(edt_scan_kernel, dim3(1), dim3(1024), 0, s, scan, (long)nb, capacity, score_full, k, K, h, head);
        for (int dir = 0; dir < 2; ++dir) {                              // the zeros are the OTHER side's border voxels
            hipLaunchKernelGGL(edt_x_kernel, dim3(row_grid((long)D * H)), dim3(256), 0, s, flags, dir ? 1 : 2, 0, st->lo, H, W, ox);
            hipLaunchKernelGGL(edt_y_kernel, dim3(flat_grid(n, 256, 4)), dim3(256), 0, s, ox, st->lo, H, W, sy, sx, pack);
            hipLaunchKernelGGL(edt_gather_kernel, dim3(nb), dim3(256), 0, s, flags, pack, scan, st, dir, D, H, W, sz, sy, sx, dist);
        }
        hipLaunchKernelGGL(edt_reduce_kernel, dim3(2), dim3(1024), 0, s, dist, st, k, K, head);
    }
    CF_CHECK_LAUNCH();
    return CF_OK;
}
