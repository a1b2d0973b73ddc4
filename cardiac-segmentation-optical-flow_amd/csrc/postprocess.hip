// Largest-connected-component filter of the export step (nnunet/postprocessing/connected_components.py:31-107) on the device:
// scipy.ndimage.label's default structure (face neighbours: 4 in 2-D, 6 in 3-D) by min-label propagation with pointer jumping,
// component sizes by one atomic histogram, removal in one pass.  Labels are "index of a voxel of the component + 1".
#include "common.h"
#include <hip/hip_fp16.h>
#include <algorithm>

namespace cf {

#define GRID_STRIDE(i, n) for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// labels[i] = i+1 where image[i] is one of the (up to 8) class values of the region, else 0
__global__ void __launch_bounds__(256) cc_init_kernel(const uint8_t* __restrict__ image, int* __restrict__ labels, long n,
                                                      unsigned long long classes, int nclasses) {
    GRID_STRIDE(i, n) {
        const unsigned v = image[i];
        bool in = false;
        for (int k = 0; k < nclasses; ++k) in |= (v == ((classes >> (8 * k)) & 0xffu));
        labels[i] = in ? (int)(i + 1) : 0;
    }
}

// one sweep: take the smallest label among the face neighbours, then jump to that label's own label (path halving).
// Labels only ever decrease, so racing reads of neighbours are harmless; *changed is raised when anything moved.
__global__ void __launch_bounds__(256) cc_sweep_kernel(int* __restrict__ labels, int D, int H, int W, int* __restrict__ changed) {
    const long HW = (long)H * W, n = (long)D * HW;
    GRID_STRIDE(i, n) {
        int l = labels[i];
        if (l == 0) continue;
        const int z = (int)(i / HW), q = (int)(i - (long)z * HW), y = q / W, x = q - y * W;
        int m = l;
        int t;
        if (x > 0 && (t = labels[i - 1]) != 0) m = min(m, t);
        if (x < W - 1 && (t = labels[i + 1]) != 0) m = min(m, t);
        if (y > 0 && (t = labels[i - W]) != 0) m = min(m, t);
        if (y < H - 1 && (t = labels[i + W]) != 0) m = min(m, t);
        if (z > 0 && (t = labels[i - HW]) != 0) m = min(m, t);
        if (z < D - 1 && (t = labels[i + HW]) != 0) m = min(m, t);
        t = labels[m - 1];          // voxel m-1 belongs to the same component: its label is a smaller-or-equal representative
        if (t != 0 && t < m) m = t;
        if (m < l) {
            labels[i] = m;
            *changed = 1;
        }
    }
}

__global__ void __launch_bounds__(256) cc_count_kernel(const int* __restrict__ labels, int* __restrict__ counts, long n) {
    GRID_STRIDE(i, n) {
        const int l = labels[i];
        if (l) atomicAdd(&counts[l - 1], 1);
    }
}

// connected_components.py:90-101: every object whose size differs from the largest one is removed when it is smaller than
// min_valid (min_valid < 0: always)
__global__ void __launch_bounds__(256) cc_remove_kernel(uint8_t* __restrict__ image, const int* __restrict__ labels,
                                                        const int* __restrict__ counts, long n, int max_count, double volume_per_voxel,
                                                        double min_valid) {
    GRID_STRIDE(i, n) {
        const int l = labels[i];
        if (!l) continue;
        const int c = counts[l - 1];
        if (c != max_count && (min_valid < 0.0 || (double)c * volume_per_voxel < min_valid)) image[i] = 0;
    }
}

// Export resampling (resample_data_or_seg, nnunet/preprocessing/preprocessing.py:111-200): skimage.transform.resize(mode='edge',
// anti_aliasing=False) / map_coordinates(mode='nearest') sample at src = scale * (dst + 0.5) - 0.5 with edge clamping; per axis
// either linear (order 1) or nearest (order 0, floor(src + 0.5)).  Coordinates in double like the reference.
struct ResizeAxis {
    int i0, i1;
    float w1;
};
__device__ __forceinline__ ResizeAxis resize_axis(int o, int n_src, int n_dst, int linear) {
    const double s = ((double)n_src / (double)n_dst) * ((double)o + 0.5) - 0.5;
    ResizeAxis a;
    if (linear) {
        const double f = floor(s);
        int i = (int)f;
        a.w1 = (float)(s - f);
        a.i0 = min(max(i, 0), n_src - 1);
        a.i1 = min(max(i + 1, 0), n_src - 1);
    } else {
        a.i0 = a.i1 = min(max((int)floor(s + 0.5), 0), n_src - 1);
        a.w1 = 0.f;
    }
    return a;
}

// one output value: the 8-tap lerp of channel `s` [.,Y,Z] at the three axis records, z first, then y, then x.  The one fp32 chain of
// resize3d_kernel and resample_argmax_kernel (their outputs are equal bit for bit because both are this function)
__device__ __forceinline__ float resize_sample(const float* __restrict__ s, int Y, int Z, const ResizeAxis& ax, const ResizeAxis& ay,
                                               const ResizeAxis& az) {
    auto at = [&](int a, int b, int c) { return s[((long)a * Y + b) * Z + c]; };
    auto lerp = [](float u, float v, float w) { return u + (v - u) * w; };
    const float c00 = lerp(at(ax.i0, ay.i0, az.i0), at(ax.i0, ay.i0, az.i1), az.w1);
    const float c01 = lerp(at(ax.i0, ay.i1, az.i0), at(ax.i0, ay.i1, az.i1), az.w1);
    const float c10 = lerp(at(ax.i1, ay.i0, az.i0), at(ax.i1, ay.i0, az.i1), az.w1);
    const float c11 = lerp(at(ax.i1, ay.i1, az.i0), at(ax.i1, ay.i1, az.i1), az.w1);
    return lerp(lerp(c00, c01, ay.w1), lerp(c10, c11, ay.w1), ax.w1);
}

__global__ void __launch_bounds__(256) resize3d_kernel(const float* __restrict__ src, float* __restrict__ dst, int X, int Y, int Z, int X2,
                                                       int Y2, int Z2, int lx, int ly, int lz, long total) {
    const long V2 = (long)X2 * Y2 * Z2, V = (long)X * Y * Z;
    GRID_STRIDE(i, total) {
        const long n = i / V2, p = i - n * V2;
        const int z = (int)(p % Z2);
        const long r = p / Z2;
        const int y = (int)(r % Y2), x = (int)(r / Y2);
        const ResizeAxis ax = resize_axis(x, X, X2, lx), ay = resize_axis(y, Y, Y2, ly), az = resize_axis(z, Z, Z2, lz);
        dst[i] = resize_sample(src + n * V, Y, Z, ax, ay, az);
    }
}

// ---- Validation export in one visit (nnUNetTrainer.validate's save_segmentation_nifti_from_softmax + the evaluator's confusion counts, and
// predict_next_stage's resample + arg-max): src [K,X,Y,Z] -> labels at (X2,Y2,Z2) placed at (x0,y0,z0) inside seg [Xf,Yf,Zf].  One thread per
// voxel of the FULL volume, consecutive threads along Z (the fastest axis: byte stores of seg, 2-byte stores of probs and the z taps of src
// coalesce).  The three axis records (fp64 coordinates) are formed once per voxel, ahead of the channel loop; each channel is one
// resize_sample.  Label: the first maximum over the channels with numpy's NaN rule, or with REGIONS 0 overwritten by order[k] where
// p_k > 0.5, in channel order.  probs (may be NULL): the resampled value as fp16, round-to-nearest-even; with REGIONS a value > 0.5 that
// rounds to <= 0.5 is stored as the next fp16 above 0.5 (export.probabilities_as_stored).  gt (may be NULL): hist[t * 16 + r] over the full
// volume, the last bin for a label >= 16 in either volume (cf_label_confusion's layout) -- a per-block LDS histogram, to which the lanes of a
// wave that hold one bin add once, then one 64-bit atomic per non-empty bin.
constexpr int RESAMPLE_MAX_CLASSES = 255;
constexpr int RESAMPLE_HIST_K = 16;
constexpr int RESAMPLE_BINS = RESAMPLE_HIST_K * RESAMPLE_HIST_K + 1;
struct ResampleOrder {
    uint8_t v[RESAMPLE_MAX_CLASSES + 1];
};

template <bool REGIONS>
__global__ void __launch_bounds__(256) resample_argmax_kernel(const float* __restrict__ src, int K, int X, int Y, int Z, int X2, int Y2, int Z2, int lx,
                                                              int ly, int lz, uint8_t* __restrict__ seg, int Xf, int Yf, int Zf, int x0, int y0, int z0,
                                                              ResampleOrder order, __half* __restrict__ probs, const uint8_t* __restrict__ gt,
                                                              unsigned long long* __restrict__ hist) {
    __shared__ unsigned h[RESAMPLE_BINS];
    for (int b = threadIdx.x; b < RESAMPLE_BINS; b += blockDim.x) h[b] = 0;
    __syncthreads();
    const long V = (long)X * Y * Z, V2 = (long)X2 * Y2 * Z2, full = (long)Xf * Yf * Zf;
    const int lane = threadIdx.x & 63;
    // the trip count is the block's, not the thread's: every lane of a wave reaches the ballots below
    for (long base = blockIdx.x * (long)blockDim.x; base < full; base += (long)gridDim.x * blockDim.x) {
        const long i = base + threadIdx.x;
        const bool valid = i < full;
        int label = 0;
        if (valid) {
            const int zf = (int)(i % Zf);
            const long r = i / Zf;
            const int z = zf - z0, y = (int)(r % Yf) - y0, x = (int)(r / Yf) - x0;
            if (x >= 0 && x < X2 && y >= 0 && y < Y2 && z >= 0 && z < Z2) {
                const ResizeAxis ax = resize_axis(x, X, X2, lx), ay = resize_axis(y, Y, Y2, ly), az = resize_axis(z, Z, Z2, lz);
                const long p = ((long)x * Y2 + y) * Z2 + z;
                float best = 0.f;
                for (int k = 0; k < K; ++k) {
                    const float m = resize_sample(src + k * V, Y, Z, ax, ay, az);
                    if (probs) {
                        __half q = __float2half_rn(m);
                        if (REGIONS && m > 0.5f && !(__half2float(q) > 0.5f)) q = __ushort_as_half((unsigned short)0x3801);   // 0.5 + 2^-11
                        probs[k * V2 + p] = q;
                    }
                    if (REGIONS) {
                        label = m > 0.5f ? (int)order.v[k] : label;
                    } else {
                        const bool up = k > 0 && (m > best || (m != m && best == best));     // numpy's argmax: first maximum, first NaN
                        best = (k == 0 || up) ? m : best;
                        label = up ? k : label;
                    }
                }
            }
            seg[i] = (uint8_t)label;
        }
        if (gt) {
            int bin = RESAMPLE_BINS - 1;
            if (valid) {
                const int r = gt[i];
                if (label < RESAMPLE_HIST_K && r < RESAMPLE_HIST_K) bin = label * RESAMPLE_HIST_K + r;
            }
            bool todo = valid;
            while (__ballot(todo)) {                                  // one trip per distinct bin of the wave: one or two as a rule
                if (todo) {
                    const int lead = __builtin_amdgcn_readfirstlane(bin);
                    if (bin == lead) {
                        const unsigned long long who = __ballot(1);
                        if (lane == __ffsll((long long)who) - 1) atomicAdd(&h[lead], (unsigned)__popcll(who));
                        todo = false;
                    }
                }
            }
        }
    }
    if (gt) {
        __syncthreads();
        for (int b = threadIdx.x; b < RESAMPLE_BINS; b += blockDim.x)
            if (h[b]) atomicAdd(&hist[b], (unsigned long long)h[b]);
    }
}

}  // namespace cf

using namespace cf;

#define LAUNCH_FLAT(kernel, n, ...)                                                                              \
    do {                                                                                                         \
        hipLaunchKernelGGL(kernel, dim3(flat_grid((n), 256)), dim3(256), 0, as_stream(stream), __VA_ARGS__);      \
        CF_CHECK_LAUNCH();                                                                                       \
        return CF_OK;                                                                                            \
    } while (0)

extern "C" int cf_cc_init(const uint8_t* image, int* labels, long n, const uint8_t* classes, int nclasses, void* stream) {
    CF_REQUIRE(image && labels && classes, "null pointer");
    CF_REQUIRE(n > 0 && n < (1L << 31) - 1 && nclasses >= 1 && nclasses <= 8, "bad size");
    unsigned long long packed = 0;
    for (int k = 0; k < nclasses; ++k) packed |= (unsigned long long)classes[k] << (8 * k);   // host array of class values
    LAUNCH_FLAT(cc_init_kernel, n, image, labels, n, packed, nclasses);
}

extern "C" int cf_cc_sweep(int* labels, int D, int H, int W, int* changed, void* stream) {
    CF_REQUIRE(labels && changed, "null pointer");
    CF_REQUIRE(D > 0 && H > 0 && W > 0 && (long)D * H * W < (1L << 31) - 1, "bad shape");
    const long n = (long)D * H * W;
    LAUNCH_FLAT(cc_sweep_kernel, n, labels, D, H, W, changed);
}

extern "C" int cf_cc_count(const int* labels, int* counts, long n, void* stream) {
    CF_REQUIRE(labels && counts && n > 0, "bad arguments");
    LAUNCH_FLAT(cc_count_kernel, n, labels, counts, n);
}

extern "C" int cf_cc_remove(uint8_t* image, const int* labels, const int* counts, long n, int max_count, double volume_per_voxel,
                            double min_valid, void* stream) {
    CF_REQUIRE(image && labels && counts && n > 0, "bad arguments");
    LAUNCH_FLAT(cc_remove_kernel, n, image, labels, counts, n, max_count, volume_per_voxel, min_valid);
}

extern "C" int cf_resize3d(const float* src, float* dst, int N, int X, int Y, int Z, int X2, int Y2, int Z2, int linear_x, int linear_y,
                           int linear_z, void* stream) {
    CF_REQUIRE(src && dst && src != dst, "null or aliased pointer");
    CF_REQUIRE(N > 0 && X > 0 && Y > 0 && Z > 0 && X2 > 0 && Y2 > 0 && Z2 > 0, "bad shape");
    const long total = (long)N * X2 * Y2 * Z2;
    LAUNCH_FLAT(resize3d_kernel, total, src, dst, X, Y, Z, X2, Y2, Z2, linear_x, linear_y, linear_z, total);
}

extern "C" int cf_resample_argmax(const float* src, int K, int X, int Y, int Z, int X2, int Y2, int Z2, int linear_x, int linear_y, int linear_z,
                                  uint8_t* seg, int Xf, int Yf, int Zf, int x0, int y0, int z0, const uint8_t* order, void* probs_out,
                                  const uint8_t* gt, unsigned long long* hist, void* stream) {
    CF_REQUIRE(src && seg, "null pointer");
    CF_REQUIRE(K >= 1 && K <= RESAMPLE_MAX_CLASSES, "K = %d is outside 1..%d", K, RESAMPLE_MAX_CLASSES);
    CF_REQUIRE(X > 0 && Y > 0 && Z > 0 && X2 > 0 && Y2 > 0 && Z2 > 0 && Xf > 0 && Yf > 0 && Zf > 0, "bad shape (%d, %d, %d) -> (%d, %d, %d) in (%d, %d, %d)",
               X, Y, Z, X2, Y2, Z2, Xf, Yf, Zf);
    CF_REQUIRE(x0 >= 0 && y0 >= 0 && z0 >= 0 && (long)x0 + X2 <= Xf && (long)y0 + Y2 <= Yf && (long)z0 + Z2 <= Zf,
               "the crop (%d, %d, %d) at (%d, %d, %d) overhangs the volume (%d, %d, %d)", X2, Y2, Z2, x0, y0, z0, Xf, Yf, Zf);
    CF_REQUIRE((gt == nullptr) == (hist == nullptr), "gt and hist go together");
    CF_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3) == 0 && (reinterpret_cast<uintptr_t>(probs_out) & 1) == 0 &&
                   (reinterpret_cast<uintptr_t>(hist) & 7) == 0, "a pointer is not aligned to its element size");
    const long full = (long)Xf * Yf * Zf;
    CF_REQUIRE(full < (1L << 40) && (long)K * X * Y * Z < (1L << 40), "volume too large");
    ResampleOrder ord = {};
    if (order)
        for (int k = 0; k < K; ++k) ord.v[k] = order[k];            // HOST array of the regions' label values
    hipStream_t s = as_stream(stream);
    if (hist && hipMemsetAsync(hist, 0, RESAMPLE_BINS * sizeof(unsigned long long), s) != hipSuccess) {
        set_error("cf_resample_argmax: memset failed");
        return CF_ERR_LAUNCH;
    }
    const unsigned blocks = (unsigned)std::min((full + 255) / 256, (long)device_cu_count() * 8);    // grid-stride: 8 blocks of 4 waves per compute unit
    if (order)
        hipLaunchKernelGGL(resample_argmax_kernel<true>, dim3(blocks), dim3(256), 0, s, src, K, X, Y, Z, X2, Y2, Z2, linear_x, linear_y, linear_z, seg,
                           Xf, Yf, Zf, x0, y0, z0, ord, static_cast<__half*>(probs_out), gt, hist);
    else
        hipLaunchKernelGGL(resample_argmax_kernel<false>, dim3(blocks), dim3(256), 0, s, src, K, X, Y, Z, X2, Y2, Z2, linear_x, linear_y, linear_z, seg,
                           Xf, Yf, Zf, x0, y0, z0, ord, static_cast<__half*>(probs_out), gt, hist);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
