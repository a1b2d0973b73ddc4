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

template <typename T, bool REGIONS>
__global__ void __launch_bounds__(256) ensemble_merge_kernel(EnsembleMembers members, int N, int K, int Z, int Y, int X, uint8_t* __restrict__ seg,
                                                             int Zf, int Yf, int Xf, int z0, int y0, int x0, T* __restrict__ mean,
                                                             EnsembleOrder order) {
    const unsigned CL = (unsigned)(x0 + 7) >> 3, XC = (unsigned)(X + 7) >> 3, CR = (unsigned)(Xf - x0 - X + 7) >> 3;   // chunks: left margin, crop, right margin
    const unsigned per_row = CL + XC + CR;
    const unsigned units = (unsigned)Zf * (unsigned)Yf * per_row;     // < 2^31, checked by the launcher
    const long plane = (long)Z * Y * X;
    const float fn = (float)N;
    for (unsigned u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const unsigned row = u / per_row, c = u - row * per_row;
        const int zf = (int)(row / (unsigned)Yf), yf = (int)(row - (unsigned)zf * (unsigned)Yf);
        const int z = zf - z0, y = yf - y0;
        int xs, nx, xc = -1;                                          // output x of the chunk, its length, and its x inside the crop row (-1: margin)
        if (c < CL) {
            xs = (int)c * 8;
            nx = min(8, x0 - xs);
        } else if (c < CL + XC) {
            const int xi = (int)(c - CL) * 8;
            xs = x0 + xi;
            nx = min(8, X - xi);
            if ((unsigned)z < (unsigned)Z && (unsigned)y < (unsigned)Y) xc = xi;
        } else {
            xs = x0 + X + (int)(c - CL - XC) * 8;
            nx = min(8, Xf - xs);
        }
        int label[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (xc >= 0) {
            const long off = ((long)z * Y + y) * X + xc;
            float best[8];
            for (int k = 0; k < K; ++k) {
                const long o = (long)k * plane + off;
                float m[8];
                load8(static_cast<const T*>(members.p[0]) + o, nx, m);
#pragma unroll 4
                for (int n = 1; n < N; ++n) {
                    float a[8];
                    load8(static_cast<const T*>(members.p[n]) + o, nx, a);
#pragma unroll
                    for (int e = 0; e < 8; ++e) m[e] = __fadd_rn(m[e], a[e]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = __fdiv_rn(m[e], fn);
                round_store8(mean ? mean + o : nullptr, nx, m);
                if (REGIONS) {
                    const int c_k = order.v[k];
#pragma unroll
                    for (int e = 0; e < 8; ++e) label[e] = m[e] > 0.5f ? c_k : label[e];
                } else if (k == 0) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) best[e] = m[e];
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const bool up = m[e] > best[e] || (m[e] != m[e] && best[e] == best[e]);    // strictly greater: the first maximum stays
                        best[e] = up ? m[e] : best[e];
                        label[e] = up ? k : label[e];
                    }
                }
            }
        }
        uint8_t* d = seg + ((long)row * Xf + xs);
        if (nx == 8 && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
            const unsigned lo = (unsigned)label[0] | (unsigned)label[1] << 8 | (unsigned)label[2] << 16 | (unsigned)label[3] << 24;
            const unsigned hi = (unsigned)label[4] | (unsigned)label[5] << 8 | (unsigned)label[6] << 16 | (unsigned)label[7] << 24;
            *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e < nx) d[e] = (uint8_t)label[e];
        }
    }
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

extern "C" int cf_region_labels(const float* probs, uint8_t* seg, int B, int K, long HW, const uint8_t* order, void* stream) {
    CF_REQUIRE(probs && seg && order, "null pointer");
    CF_REQUIRE(K >= 1 && K <= ENSEMBLE_MAX_CLASSES, "K = %d is outside 1..%d", K, ENSEMBLE_MAX_CLASSES);
    CF_REQUIRE(B > 0 && HW > 0, "bad shape B=%d HW=%ld", B, HW);
    EnsembleOrder ord = {};
    for (int k = 0; k < K; ++k) ord.v[k] = order[k];                // HOST array of the regions' label values
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
    CF_REQUIRE(dtype == 0 || dtype == 1, "dtype = %d is neither 0 (fp16) nor 1 (fp32)", dtype);
    CF_REQUIRE(K >= 1 && K <= ENSEMBLE_MAX_CLASSES, "K = %d is outside 1..%d", K, ENSEMBLE_MAX_CLASSES);
    CF_REQUIRE(Z > 0 && Y > 0 && X > 0 && Zf > 0 && Yf > 0 && Xf > 0, "bad shape (%d, %d, %d) in (%d, %d, %d)", Z, Y, X, Zf, Yf, Xf);
    CF_REQUIRE(z0 >= 0 && y0 >= 0 && x0 >= 0 && (long)z0 + Z <= Zf && (long)y0 + Y <= Yf && (long)x0 + X <= Xf,
               "the crop (%d, %d, %d) at (%d, %d, %d) overhangs the volume (%d, %d, %d)", Z, Y, X, z0, y0, x0, Zf, Yf, Xf);
    const uintptr_t emask = dtype == 0 ? 1 : 3;
    EnsembleMembers mem = {};
    for (int n = 0; n < n_members; ++n) {                           // HOST array of device pointers
        CF_REQUIRE(members[n], "member %d is a null pointer", n);
        CF_REQUIRE((reinterpret_cast<uintptr_t>(members[n]) & emask) == 0, "member %d is not aligned to its element size", n);
        mem.p[n] = members[n];
    }
    CF_REQUIRE((reinterpret_cast<uintptr_t>(mean) & emask) == 0, "mean is not aligned to its element size");
    EnsembleOrder ord = {};
    if (order)
        for (int k = 0; k < K; ++k) ord.v[k] = order[k];            // HOST array of the regions' label values
    const long per_row = (x0 + 7) / 8 + (X + 7) / 8 + (Xf - x0 - X + 7) / 8;
    const long units = (long)Zf * Yf * per_row;
    CF_REQUIRE(units < (1L << 31) - 1, "output of %ld 8-voxel chunks is too large", units);
    long blocks = (units + 255) / 256;
    const long cap = (long)device_cu_count() * 8;                   // grid-stride: 8 blocks of 4 waves per compute unit
    if (blocks > cap) blocks = cap;
    if (dtype == 0)
        launch_ensemble<__half>((unsigned)blocks, as_stream(stream), mem, n_members, K, Z, Y, X, seg, Zf, Yf, Xf, z0, y0, x0, mean, ord, order != nullptr);
    else
        launch_ensemble<float>((unsigned)blocks, as_stream(stream), mem, n_members, K, Z, Y, X, seg, Zf, Yf, Xf, z0, y0, x0, mean, ord, order != nullptr);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
