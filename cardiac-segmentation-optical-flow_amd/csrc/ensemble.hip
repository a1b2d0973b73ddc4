// Ensemble of saved softmax volumes: the arithmetic of nnunet/inference/ensemble_predictions.py merge_files plus the label step and the
// bounding-box placement of segmentation_export.py, one launch per case.
//
// cf_ensemble_merge reads N member volumes [K][Z][Y][X] (all __half or all float) and writes
//   * the uint8 label volume at the size before cropping [Zf][Yf][Xf]: the crop placed at (z0, y0, x0), 0 everywhere else -- the grid covers
//     the whole output, so the caller needs no memset;
//   * the mean volume [K][Z][Y][X] in the members' dtype when the caller wants it (--npz).
// The numbers are numpy's np.mean(np.vstack([a[None] for a in members]), 0), step by step:
//   * s = the fp32 sum of the members in the order given, one add per member (the reduction axis is the outermost one: numpy adds
//     member by member, nothing pairwise);
//   * m = s / float(N): a true, correctly rounded fp32 division -- NOT a multiply by 1.0f / N, which rounds differently (N = 7: 7 of 4420
//     elements of a seeded softmax) -- and for __half members m is then rounded to fp16, nearest even;
//   * label = the first index of the maximum of m over K (numpy's argmax: a NaN counts as the maximum), taken on the ROUNDED fp16 values for
//     __half members, not on s (N = 3: the two differ in 2 of 1105 voxels of the seeded case);
//   * with a regions_class_order: label = 0, then for i = 0..K-1 label = order[i] where m[i] > 0.5, a later region overwriting an earlier one.
// There is no multiply next to an add anywhere, so nothing contracts into an fma; the division is hipcc's IEEE expansion (its default
// -fhip-fp32-correctly-rounded-divide-sqrt), and fp32 / fp16 denormals are kept (hipcc's default for gfx9).
//
// Streaming shape: a thread owns 8 consecutive x voxels of one crop row.  Where the chunk is whole and its address is 16-byte aligned, one
// 16-byte load per (member, class) for __half and two for float, scalar loads otherwise; the mean is stored the same way; the 8 labels
// leave as one 8-byte store where the destination is 8-byte aligned, byte stores otherwise (the row tail when X % 8 != 0, and every row
// of a volume whose X, Xf or x0 puts rows off the boundary).  An output row is cut into chunks of the left margin [0, x0), of the crop and of
// the right margin [x0 + X, Xf), each counted from its own start, so that the crop's chunks line up with the members' rows; rows above and
// below the crop have the same chunks and write zeros.  Every offset into a member, the mean or the labels is 64-bit.
//
// cf_ensemble_pairs is the same visit for model selection (nnunet/evaluation/model_selection/ensemble.py: every two-member ensemble of M
// models, scored against the ground truth): M members and a list of P (i, j) pairs in, P label volumes and P 16 x 16 label confusions
// (cf_label_confusion's layout, overflow bin included) out.  The numbers of pair p are those of cf_ensemble_merge on the two members --
// the kernels share chunk_of, mean8, takes_over and store_labels8 below -- and of cf_label_confusion on that volume.  A thread loads the 8
// values of each member once per class and forms from them every one of the M (M - 1) / 2 two-member means (M is a template argument, so
// the members' values and each combination's running maximum stay in registers); fp32 addition commutes, so (i, j) and (j, i) are one
// combination, and a table in the kernel arguments names the listed pairs that each combination serves.  Labels are kept as packed
// bytes, two registers per combination.  Counting: a block keeps P histograms of 257 32-bit bins in LDS; a thread whose 8 voxels fall into
// one bin joins a wave-wide ballot with the lanes that hold the same bin and one lane adds the total (the background of a label volume
// is nearly all of it), other threads add one LDS atomic per run of equal bins; at the end each block adds its non-zero bins to the
// 64-bit counters with vector-memory atomics.
#include <hip/hip_fp16.h>

#include "common.h"

namespace cf {

constexpr int ENSEMBLE_MAX_MEMBERS = 16;
constexpr int ENSEMBLE_MAX_CLASSES = 255;
struct EnsembleMembers {
    const void* p[ENSEMBLE_MAX_MEMBERS];        // kernel argument: member n's base is a scalar load
};
struct EnsembleOrder {
    uint8_t v[ENSEMBLE_MAX_CLASSES + 1];        // regions_class_order, kernel argument like PrevStageClasses
};

// 8 consecutive values as fp32 (exact for __half); entries past nx are never stored and hold 0
__device__ __forceinline__ void load8(const __half* p, int nx, float (&v)[8]) {
    if (nx == 8 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const __half2* h = reinterpret_cast<const __half2*>(&q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float2 f = __half22float2(h[e]);
            v[2 * e] = f.x;
            v[2 * e + 1] = f.y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = e < nx ? __half2float(p[e]) : 0.f;
    }
}
__device__ __forceinline__ void load8(const float* p, int nx, float (&v)[8]) {
    if (nx == 8 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = e < nx ? p[e] : 0.f;
    }
}

// the mean in the members' dtype: rounds m IN PLACE to what is stored (the arg-max reads the rounded values) and stores it when p != nullptr
__device__ __forceinline__ void round_store8(__half* p, int nx, float (&m)[8]) {
    __half h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        h[e] = __float2half_rn(m[e]);
        m[e] = __half2float(h[e]);
    }
    if (!p) return;
    if (nx == 8 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(h);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < nx) p[e] = h[e];
    }
}
__device__ __forceinline__ void round_store8(float* p, int nx, float (&m)[8]) {
    if (!p) return;
    if (nx == 8 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        reinterpret_cast<float4*>(p)[0] = make_float4(m[0], m[1], m[2], m[3]);
        reinterpret_cast<float4*>(p)[1] = make_float4(m[4], m[5], m[6], m[7]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < nx) p[e] = m[e];
    }
}

// One 8-voxel chunk of the output: its row (zf * Yf + yf), output x, length, and for a chunk inside the crop the x inside the crop row and the
// offset of its first voxel inside a class plane of a member (xc = -1: margin, or a row above / below the crop)
struct Chunk {
    unsigned row;
    int xs, nx, xc;
    long off;
};
struct ChunkPlan {
    unsigned CL, XC, CR, per_row, units;
};
__device__ __forceinline__ ChunkPlan plan_chunks(int X, int Zf, int Yf, int Xf, int x0) {
    ChunkPlan p;
    p.CL = (unsigned)(x0 + 7) >> 3, p.XC = (unsigned)(X + 7) >> 3, p.CR = (unsigned)(Xf - x0 - X + 7) >> 3;   // chunks: left margin, crop, right margin
    p.per_row = p.CL + p.XC + p.CR;
    p.units = (unsigned)Zf * (unsigned)Yf * p.per_row;               // < 2^31, checked by the launcher
    return p;
}
__device__ __forceinline__ Chunk chunk_of(unsigned u, const ChunkPlan& p, int Z, int Y, int X, int Yf, int Xf, int z0, int y0, int x0) {
    Chunk ch;
    ch.row = u / p.per_row;
    const unsigned c = u - ch.row * p.per_row;
    const int zf = (int)(ch.row / (unsigned)Yf), yf = (int)(ch.row - (unsigned)zf * (unsigned)Yf);
    const int z = zf - z0, y = yf - y0;
    ch.xc = -1;
    if (c < p.CL) {
        ch.xs = (int)c * 8;
        ch.nx = min(8, x0 - ch.xs);
    } else if (c < p.CL + p.XC) {
        const int xi = (int)(c - p.CL) * 8;
        ch.xs = x0 + xi;
        ch.nx = min(8, X - xi);
        if ((unsigned)z < (unsigned)Z && (unsigned)y < (unsigned)Y) ch.xc = xi;
    } else {
        ch.xs = x0 + X + (int)(c - p.CL - p.XC) * 8;
        ch.nx = min(8, Xf - ch.xs);
    }
    ch.off = ((long)z * Y + y) * X + ch.xc;
    return ch;
}

// the fp32 sum of the members -> the mean as the members' dtype holds it: a true division by fn, rounded to fp16 for __half members (m is
// what the label step reads); stored at p when p != nullptr
template <typename T>
__device__ __forceinline__ void mean8(float (&m)[8], float fn, T* p, int nx) {
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = __fdiv_rn(m[e], fn);
    round_store8(p, nx, m);
}
// numpy's argmax step: strictly greater, so the first maximum stays; a NaN counts as the maximum, and the first NaN stays
__device__ __forceinline__ bool takes_over(float m, float best) { return m > best || (m != m && best == best); }
// the region rule's step (segmentation_export.py:148-150)
__device__ __forceinline__ bool region_hit(float m) { return m > 0.5f; }

// 8 labels as packed bytes (lo: voxels 0-3, hi: 4-7) -> d: one 8-byte store where d is 8-byte aligned and the chunk whole, byte stores otherwise
__device__ __forceinline__ void store_labels8(uint8_t* d, int nx, unsigned lo, unsigned hi) {
    if (nx == 8 && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
        *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < nx) d[e] = (uint8_t)((e < 4 ? lo : hi) >> (8 * (e & 3)));
    }
}

template <typename T, bool REGIONS>
__global__ void __launch_bounds__(256) ensemble_merge_kernel(EnsembleMembers members, int N, int K, int Z, int Y, int X, uint8_t* __restrict__ seg,
                                                             int Zf, int Yf, int Xf, int z0, int y0, int x0, T* __restrict__ mean,
                                                             EnsembleOrder order) {
    const ChunkPlan plan = plan_chunks(X, Zf, Yf, Xf, x0);
    const long plane = (long)Z * Y * X;
    const float fn = (float)N;
    for (unsigned u = blockIdx.x * blockDim.x + threadIdx.x; u < plan.units; u += gridDim.x * blockDim.x) {
        const Chunk ch = chunk_of(u, plan, Z, Y, X, Yf, Xf, z0, y0, x0);
        const int nx = ch.nx;
        int label[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ch.xc >= 0) {
            float best[8];
            for (int k = 0; k < K; ++k) {
                const long o = (long)k * plane + ch.off;
                float m[8];
                load8(static_cast<const T*>(members.p[0]) + o, nx, m);
#pragma unroll 4
                for (int n = 1; n < N; ++n) {
                    float a[8];
                    load8(static_cast<const T*>(members.p[n]) + o, nx, a);
#pragma unroll
                    for (int e = 0; e < 8; ++e) m[e] = __fadd_rn(m[e], a[e]);
                }
                mean8(m, fn, mean ? mean + o : nullptr, nx);
                if (REGIONS) {
                    const int c_k = order.v[k];
#pragma unroll
                    for (int e = 0; e < 8; ++e) label[e] = region_hit(m[e]) ? c_k : label[e];
                } else if (k == 0) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) best[e] = m[e];
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const bool up = takes_over(m[e], best[e]);
                        best[e] = up ? m[e] : best[e];
                        label[e] = up ? k : label[e];
                    }
                }
            }
        }
        const unsigned lo = (unsigned)label[0] | (unsigned)label[1] << 8 | (unsigned)label[2] << 16 | (unsigned)label[3] << 24;
        const unsigned hi = (unsigned)label[4] | (unsigned)label[5] << 8 | (unsigned)label[6] << 16 | (unsigned)label[7] << 24;
        store_labels8(seg + ((long)ch.row * Xf + ch.xs), nx, lo, hi);
    }
}

// ---- every two-member ensemble of M members against one ground truth
constexpr int PAIRS_MAX_MEMBERS = 8;
constexpr int PAIRS_MAX = PAIRS_MAX_MEMBERS * (PAIRS_MAX_MEMBERS - 1) / 2;     // 28
constexpr int PAIRS_HIST_K = 16;
constexpr int PAIRS_BINS = PAIRS_HIST_K * PAIRS_HIST_K + 1;                     // cf_label_confusion's layout at K = 16: the last bin is the overflow
struct EnsemblePairUsers {
    unsigned v[PAIRS_MAX];      // v[c]: bit p is set when pair p of the caller's list is combination c (the (i < j) in lexicographic order)
};

// byte e of a packed label word <- v where up
__device__ __forceinline__ unsigned set_label(unsigned w, int e, bool up, unsigned v) {
    const int s = 8 * (e & 3);
    return up ? (w & ~(0xffu << s)) | (v << s) : w;
}
// 8 ground-truth labels as packed bytes; bytes past nx are never read back
__device__ __forceinline__ uint2 load_labels8(const uint8_t* p, int nx) {
    if (nx == 8 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) return *reinterpret_cast<const uint2*>(p);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (e < nx) (e < 4 ? lo : hi) |= (unsigned)p[e] << (8 * (e & 3));
    return make_uint2(lo, hi);
}

template <typename T, int M, bool REGIONS>
__global__ void __launch_bounds__(256) ensemble_pairs_kernel(EnsembleMembers members, EnsemblePairUsers users, int P, int K, int Z, int Y, int X,
                                                             const uint8_t* __restrict__ gt, uint8_t* __restrict__ seg, int Zf, int Yf, int Xf, int z0,
                                                             int y0, int x0, EnsembleOrder order, unsigned long long* __restrict__ hist) {
    constexpr int C = M * (M - 1) / 2;
    extern __shared__ unsigned h[];                                   // [P][PAIRS_BINS]
    const int bins = P * PAIRS_BINS;
    for (int b = threadIdx.x; b < bins; b += blockDim.x) h[b] = 0;
    __syncthreads();
    const ChunkPlan plan = plan_chunks(X, Zf, Yf, Xf, x0);
    const long plane = (long)Z * Y * X, full = (long)Zf * Yf * Xf;
    const int lane = threadIdx.x & 63;
    for (unsigned u = blockIdx.x * blockDim.x + threadIdx.x; u < plan.units; u += gridDim.x * blockDim.x) {
        const Chunk ch = chunk_of(u, plan, Z, Y, X, Yf, Xf, z0, y0, x0);
        const int nx = ch.nx;
        const long at = (long)ch.row * Xf + ch.xs;
        const uint2 g = load_labels8(gt + at, nx);
        unsigned lo[C], hi[C];
#pragma unroll
        for (int c = 0; c < C; ++c) lo[c] = hi[c] = 0;
        if (ch.xc >= 0) {
            float best[C][8];
            for (int k = 0; k < K; ++k) {
                const long o = (long)k * plane + ch.off;
                float a[M][8];
#pragma unroll
                for (int n = 0; n < M; ++n) load8(static_cast<const T*>(members.p[n]) + o, nx, a[n]);
                const unsigned c_k = REGIONS ? order.v[k] : (unsigned)k;
                int c = 0;
#pragma unroll
                for (int i = 0; i < M; ++i) {
#pragma unroll
                    for (int j = i + 1; j < M; ++j, ++c) {
                        float m[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) m[e] = __fadd_rn(a[i][e], a[j][e]);
                        mean8(m, 2.0f, static_cast<T*>(nullptr), nx);
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            bool up;
                            if (REGIONS) {
                                up = region_hit(m[e]);
                            } else {
                                up = k > 0 && takes_over(m[e], best[c][e]);
                                best[c][e] = (k == 0 || up) ? m[e] : best[c][e];
                            }
                            if (e < 4) lo[c] = set_label(lo[c], e, up, c_k);
                            else hi[c] = set_label(hi[c], e, up, c_k);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            int bin[8];
            bool one = nx == 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned t = ((e < 4 ? lo[c] : hi[c]) >> (8 * (e & 3))) & 0xffu, r = ((e < 4 ? g.x : g.y) >> (8 * (e & 3))) & 0xffu;
                bin[e] = (t < PAIRS_HIST_K && r < PAIRS_HIST_K) ? (int)(t * PAIRS_HIST_K + r) : PAIRS_HIST_K * PAIRS_HIST_K;
                one = one && bin[e] == bin[0];
            }
            const int lead = __builtin_amdgcn_readfirstlane(bin[0]);  // the first active lane's bin: the one the ballot gathers
            const bool agree = one && bin[0] == lead;
            const unsigned long long who = __ballot(agree);
            const bool adds = agree && lane == __ffsll((long long)who) - 1;
            const unsigned together = 8u * (unsigned)__popcll(who);
            for (unsigned todo = users.v[c]; todo; todo &= todo - 1) {    // uniform: the listed pairs this combination serves (one, as a rule)
                const int p = __builtin_ctz(todo);
                store_labels8(seg + ((long)p * full + at), nx, lo[c], hi[c]);
                unsigned* hp = h + p * PAIRS_BINS;
                if (adds) atomicAdd(&hp[lead], together);
                if (!agree) {
                    unsigned run = 0;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if (e < nx) {
                            ++run;
                            if (e + 1 == nx || bin[e + 1 < 8 ? e + 1 : e] != bin[e]) {
                                atomicAdd(&hp[bin[e]], run);
                                run = 0;
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += blockDim.x)
        if (h[b]) atomicAdd(&hist[b], (unsigned long long)h[b]);
}

template <typename T>
static void launch_ensemble(unsigned blocks, hipStream_t s, const EnsembleMembers& mem, int N, int K, int Z, int Y, int X, uint8_t* seg, int Zf, int Yf,
                            int Xf, int z0, int y0, int x0, void* mean, const EnsembleOrder& ord, bool regions) {
    if (regions)
        hipLaunchKernelGGL((ensemble_merge_kernel<T, true>), dim3(blocks), dim3(256), 0, s, mem, N, K, Z, Y, X, seg, Zf, Yf, Xf, z0, y0, x0,
                           static_cast<T*>(mean), ord);
    else
        hipLaunchKernelGGL((ensemble_merge_kernel<T, false>), dim3(blocks), dim3(256), 0, s, mem, N, K, Z, Y, X, seg, Zf, Yf, Xf, z0, y0, x0,
                           static_cast<T*>(mean), ord);
}

// The label step above on its own, for probabilities that are already on the device (the sliding window's merged sigmoid maps):
// probs [B,K,HW] fp32 -> seg [B,HW]: label = 0, then for i = 0..K-1 label = order[i] where probs[i] > 0.5f (neural_network.py:749-751,
// segmentation_export.py:148-150).  V = 4: four voxels per thread, one 16-byte load per region and one 4-byte store (HW % 4 == 0, probs
// 16-byte and seg 4-byte aligned); V = 1: one voxel.
template <int V>
__global__ void __launch_bounds__(256) region_labels_kernel(const float* __restrict__ probs, uint8_t* __restrict__ seg, int K, long HW, long total,
                                                            EnsembleOrder order) {
    const long HWv = HW / V;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {   // i over (b, p / V)
        const long b = i / HWv, p = (i - b * HWv) * V;
        const float* q = probs + b * K * HW + p;
        int label[V];
#pragma unroll
        for (int v = 0; v < V; ++v) label[v] = 0;
        for (int k = 0; k < K; ++k) {
            const int c_k = order.v[k];
            if constexpr (V == 4) {
                const float4 m = *reinterpret_cast<const float4*>(q + k * HW);
                label[0] = m.x > 0.5f ? c_k : label[0];
                label[1] = m.y > 0.5f ? c_k : label[1];
                label[2] = m.z > 0.5f ? c_k : label[2];
                label[3] = m.w > 0.5f ? c_k : label[3];
            } else {
                label[0] = q[k * HW] > 0.5f ? c_k : label[0];
            }
        }
        uint8_t* d = seg + b * HW + p;
        if constexpr (V == 4) *reinterpret_cast<uchar4*>(d) = make_uchar4((uint8_t)label[0], (uint8_t)label[1], (uint8_t)label[2], (uint8_t)label[3]);
        else d[0] = (uint8_t)label[0];
    }
}

}  // namespace cf

using namespace cf;

static EnsembleOrder order_of(const uint8_t* order, int K) {        // HOST array of the regions' label values; all 0 without one
    EnsembleOrder ord = {};
    if (order)
        for (int k = 0; k < K; ++k) ord.v[k] = order[k];
    return ord;
}

// What cf_ensemble_merge and cf_ensemble_pairs share ahead of their launch, under the entry's name `who` (the prefix of cf_last_error()).
// Two steps, with the entry's own checks in between, so that the first check to fail is the one it always was.
struct EnsembleCall {
    EnsembleMembers mem;
    EnsembleOrder ord;
    long units;                                                     // 8-voxel chunks of the output

    int check(const char* who, const void* const* members, int n_members, int dtype, int K, int Z, int Y, int X, int Zf, int Yf, int Xf, int z0,
              int y0, int x0, const uint8_t* order) {
        CF_REQUIRE_AS(who, dtype == 0 || dtype == 1, "dtype = %d is neither 0 (fp16) nor 1 (fp32)", dtype);
        CF_REQUIRE_AS(who, K >= 1 && K <= ENSEMBLE_MAX_CLASSES, "K = %d is outside 1..%d", K, ENSEMBLE_MAX_CLASSES);
        CF_REQUIRE_AS(who, Z > 0 && Y > 0 && X > 0 && Zf > 0 && Yf > 0 && Xf > 0, "bad shape (%d, %d, %d) in (%d, %d, %d)", Z, Y, X, Zf, Yf, Xf);
        CF_REQUIRE_AS(who, z0 >= 0 && y0 >= 0 && x0 >= 0 && (long)z0 + Z <= Zf && (long)y0 + Y <= Yf && (long)x0 + X <= Xf,
                      "the crop (%d, %d, %d) at (%d, %d, %d) overhangs the volume (%d, %d, %d)", Z, Y, X, z0, y0, x0, Zf, Yf, Xf);
        const uintptr_t emask = dtype == 0 ? 1 : 3;
        mem = {};
        for (int n = 0; n < n_members; ++n) {                       // HOST array of device pointers
            CF_REQUIRE_AS(who, members[n], "member %d is a null pointer", n);
            CF_REQUIRE_AS(who, (reinterpret_cast<uintptr_t>(members[n]) & emask) == 0, "member %d is not aligned to its element size", n);
            mem.p[n] = members[n];
        }
        ord = order_of(order, K);
        units = (long)Zf * Yf * ((x0 + 7) / 8 + (X + 7) / 8 + (Xf - x0 - X + 7) / 8);
        return CF_OK;
    }
    int grid(const char* who, unsigned* blocks) const {
        CF_REQUIRE_AS(who, units < (1L << 31) - 1, "output of %ld 8-voxel chunks is too large", units);
        const long cap = (long)device_cu_count() * 8;               // grid-stride: 8 blocks of 4 waves per compute unit
        *blocks = (unsigned)std::min((units + 255) / 256, cap);
        return CF_OK;
    }
};

extern "C" int cf_region_labels(const float* probs, uint8_t* seg, int B, int K, long HW, const uint8_t* order, void* stream) {
    CF_REQUIRE(probs && seg && order, "null pointer");
    CF_REQUIRE(K >= 1 && K <= ENSEMBLE_MAX_CLASSES, "K = %d is outside 1..%d", K, ENSEMBLE_MAX_CLASSES);
    CF_REQUIRE(B > 0 && HW > 0, "bad shape B=%d HW=%ld", B, HW);
    const EnsembleOrder ord = order_of(order, K);
    const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(probs) & 15) == 0 && (reinterpret_cast<uintptr_t>(seg) & 3) == 0;
    const long total = vec ? (long)B * (HW / 4) : (long)B * HW;
    if (vec)
        hipLaunchKernelGGL(region_labels_kernel<4>, dim3(flat_grid(total, 256)), dim3(256), 0, as_stream(stream), probs, seg, K, HW, total, ord);
    else
        hipLaunchKernelGGL(region_labels_kernel<1>, dim3(flat_grid(total, 256)), dim3(256), 0, as_stream(stream), probs, seg, K, HW, total, ord);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_ensemble_merge(const void* const* members, int n_members, int dtype, int K, int Z, int Y, int X, uint8_t* seg, int Zf, int Yf,
                                 int Xf, int z0, int y0, int x0, void* mean, const uint8_t* order, void* stream) {
    CF_REQUIRE(n_members >= 1 && n_members <= ENSEMBLE_MAX_MEMBERS, "n_members = %d is outside 1..%d", n_members, ENSEMBLE_MAX_MEMBERS);
    CF_REQUIRE(members && seg, "null pointer");
    EnsembleCall c;
    unsigned blocks;
    if (int e = c.check(__func__, members, n_members, dtype, K, Z, Y, X, Zf, Yf, Xf, z0, y0, x0, order)) return e;
    CF_REQUIRE((reinterpret_cast<uintptr_t>(mean) & (dtype == 0 ? 1 : 3)) == 0, "mean is not aligned to its element size");
    if (int e = c.grid(__func__, &blocks)) return e;
    if (dtype == 0)
        launch_ensemble<__half>(blocks, as_stream(stream), c.mem, n_members, K, Z, Y, X, seg, Zf, Yf, Xf, z0, y0, x0, mean, c.ord, order != nullptr);
    else
        launch_ensemble<float>(blocks, as_stream(stream), c.mem, n_members, K, Z, Y, X, seg, Zf, Yf, Xf, z0, y0, x0, mean, c.ord, order != nullptr);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

template <typename T, int M>
static void launch_pairs(unsigned blocks, hipStream_t s, const EnsembleMembers& mem, const EnsemblePairUsers& users, int P, int K, int Z, int Y, int X,
                         const uint8_t* gt, uint8_t* seg, int Zf, int Yf, int Xf, int z0, int y0, int x0, const EnsembleOrder& ord, bool regions,
                         unsigned long long* hist) {
    const size_t lds = (size_t)P * PAIRS_BINS * sizeof(unsigned);
    if (regions)
        hipLaunchKernelGGL((ensemble_pairs_kernel<T, M, true>), dim3(blocks), dim3(256), lds, s, mem, users, P, K, Z, Y, X, gt, seg, Zf, Yf, Xf, z0, y0,
                           x0, ord, hist);
    else
        hipLaunchKernelGGL((ensemble_pairs_kernel<T, M, false>), dim3(blocks), dim3(256), lds, s, mem, users, P, K, Z, Y, X, gt, seg, Zf, Yf, Xf, z0, y0,
                           x0, ord, hist);
}

extern "C" int cf_ensemble_pairs(const void* const* members, int n_members, int dtype, int K, int Z, int Y, int X, const int* pairs, int n_pairs,
                                 const uint8_t* gt, uint8_t* seg, int Zf, int Yf, int Xf, int z0, int y0, int x0, const uint8_t* order,
                                 unsigned long long* hist, void* stream) {
    CF_REQUIRE(n_members >= 2 && n_members <= PAIRS_MAX_MEMBERS, "n_members = %d is outside 2..%d", n_members, PAIRS_MAX_MEMBERS);
    CF_REQUIRE(n_pairs >= 1 && n_pairs <= PAIRS_MAX, "n_pairs = %d is outside 1..%d", n_pairs, PAIRS_MAX);
    CF_REQUIRE(members && pairs && gt && seg && hist, "null pointer");
    EnsembleCall c;
    unsigned blocks;
    if (int e = c.check(__func__, members, n_members, dtype, K, Z, Y, X, Zf, Yf, Xf, z0, y0, x0, order)) return e;
    EnsemblePairUsers users = {};
    for (int p = 0; p < n_pairs; ++p) {                             // HOST array of n_pairs (i, j)
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        CF_REQUIRE(i >= 0 && i < n_members && j >= 0 && j < n_members, "pair %d = (%d, %d) names a member outside 0..%d", p, i, j, n_members - 1);
        CF_REQUIRE(i != j, "pair %d = (%d, %d) names one member twice", p, i, j);
        const int a = i < j ? i : j, b = i < j ? j : i;
        users.v[a * n_members - a * (a + 1) / 2 + (b - a - 1)] |= 1u << p;     // (a, b)'s place among the (i < j) in lexicographic order
    }
    if (int e = c.grid(__func__, &blocks)) return e;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(hist, 0, (size_t)n_pairs * PAIRS_BINS * sizeof(unsigned long long), s) != hipSuccess) {
        set_error("cf_ensemble_pairs: memset failed");
        return CF_ERR_LAUNCH;
    }
    const EnsembleMembers& mem = c.mem;                             // (the names the switch below reads)
    const EnsembleOrder& ord = c.ord;
    const bool regions = order != nullptr;
#define CF_PAIRS_CASE(M_)                                                                                                                      \
    case M_:                                                                                                                                   \
        if (dtype == 0) launch_pairs<__half, M_>((unsigned)blocks, s, mem, users, n_pairs, K, Z, Y, X, gt, seg, Zf, Yf, Xf, z0, y0, x0, ord, regions, hist); \
        else launch_pairs<float, M_>((unsigned)blocks, s, mem, users, n_pairs, K, Z, Y, X, gt, seg, Zf, Yf, Xf, z0, y0, x0, ord, regions, hist);            \
        break;
    switch (n_members) {
        CF_PAIRS_CASE(2) CF_PAIRS_CASE(3) CF_PAIRS_CASE(4) CF_PAIRS_CASE(5) CF_PAIRS_CASE(6) CF_PAIRS_CASE(7) CF_PAIRS_CASE(8)
    }
#undef CF_PAIRS_CASE
    CF_CHECK_LAUNCH();
    return CF_OK;
}
