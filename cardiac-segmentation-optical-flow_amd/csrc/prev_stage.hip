// Previous-stage labels as network input: the device step of a `3d_cascade_fullres` model (nnunet/inference/predict.py:61-85).
//
// cf_prev_stage_onehot fuses batchgenerators' resize_segmentation(seg, new_shape, order=1) with nnU-Net's to_one_hot(., classes)
// (nnunet/utilities/one_hot_encoding.py) and writes the planes straight into the network-input tensor:
//   * sampling is cf_resize3d's: per axis s = (n / n2) (i + 0.5) - 0.5 in double, neighbours clamped to [0, n - 1], linear.  n2 == n gives
//     s = i, so an unchanged axis keeps its samples and an unchanged shape yields the input's own one-hot;
//   * the resized indicator of a label is the weight sum of the (up to 8) trilinear neighbours that carry it;
//   * the output label is the LARGEST label whose indicator is >= 0.5 (the reference assigns labels in ascending order, a later
//     one overwriting an earlier one) and 0 where none reaches 0.5 -- such voxels exist wherever three or more labels meet;
//   * plane j is 1.0f where that label equals classes[j], else 0.0f.  A label absent from `classes` still takes part in the
//     overwrite and gets no plane.
// Only a neighbour's own label can reach 0.5, so the kernel needs neither the list of labels present nor a host round trip, and
// there is no intermediate label volume: one pass reads the small uint8 map (through the cache) and streams the fp32 planes.
//
// The decision is the reference's own, ties included.  The reference resizes fp64 indicators with scipy.ndimage.zoom(order=1,
// mode='nearest', grid_mode=True), and that is one fixed fp64 chain (tests/_kernel_refs.py linear_chain_f64 reproduces it bit for bit):
//   per axis   s = (n / n2) (o + 0.5) - 0.5,  y = s - floor(s),  weights (1 - y, y) on the two edge-clamped neighbours;
//   per output t += ((v w_x) w_y) w_z over the eight neighbours, z fastest, every product and every sum rounded on its own.
// On a non-dyadic shape ratio the exact indicator of a straight label edge is exactly 1/2 at regular columns (56 -> 50 samples: every
// 25th), where the fp64 coordinate is k + 0.5 -+ 2e-15 and the reference lands on one definite side.  Both kernels below run that
// chain in double, so they land on the same side: the file is built with -ffp-contract=off (Makefile) -- an FMA of a product into
// the sum, or of the ratio into the coordinate, would round differently.  cf_resize_labels is the same decision without the one-hot
// step, for resample_data_or_seg(is_seg=True, order=1): fp32 label maps (label -1 included), and per axis linear or nearest.
//
// Streaming shape: a thread owns 4 consecutive z voxels of one (x, y) row -- the x / y index and weight setup is done once for the
// four -- and writes one 16-byte store per plane where the row chunk is whole and 16-byte aligned, one 4-byte store per voxel otherwise (the
// tail of a row with Z2 % 4 != 0, and rows of such a volume that start off a 16-byte boundary).  Offsets into dst are 64-bit: a
// full-resolution volume times n_classes passes 2^31 bytes.
#include "common.h"

// every product and sum below rounds on its own, as in scipy (the Makefile passes -ffp-contract=off too)
#pragma clang fp contract(off)

namespace cf {

constexpr int PREV_STAGE_MAX_CLASSES = 255;
struct PrevStageClasses {
    uint8_t v[PREV_STAGE_MAX_CLASSES + 1];      // kernel argument: plane j's label is a scalar load
};

struct LabelAxis {
    int i0, i1;
    double w0, w1;
};
// one axis of the reference's chain; a nearest axis (order 0 along the separate axis: floor(s + 0.5), as cf_resize3d's) is its one
// sample with weight 1 -- the second tap's weight 0 adds exact zeros
__device__ __forceinline__ LabelAxis label_axis(int o, int n_src, int n_dst, int linear = 1) {
    const double s = ((double)n_src / (double)n_dst) * ((double)o + 0.5) - 0.5;
    LabelAxis a;
    if (linear) {
        const double f = floor(s);
        const int i = (int)f;
        a.w1 = s - f;
        a.w0 = 1.0 - a.w1;
        a.i0 = min(max(i, 0), n_src - 1);
        a.i1 = min(max(i + 1, 0), n_src - 1);
    } else {
        a.i0 = a.i1 = min(max((int)floor(s + 0.5), 0), n_src - 1);
        a.w0 = 1.0;
        a.w1 = 0.0;
    }
    return a;
}

// the largest of the eight neighbours' labels whose indicator reaches 0.5, else 0.  l and w are in the chain's order (x slowest, z
// fastest), w[j] = (w_x w_y) w_z; a neighbour with another label contributes the exact zero that v = 0 gives the reference's product
template <typename T>
__device__ __forceinline__ T label_at_half(const T (&l)[8], const double (&wxy)[4], double wz0, double wz1) {
    double w[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[2 * k] = wxy[k] * wz0;
        w[2 * k + 1] = wxy[k] * wz1;
    }
    T best = 0;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double ind = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) ind += l[j] == l[k] ? w[j] : 0.0;
        if (ind >= 0.5) {
            best = any ? max(best, l[k]) : l[k];
            any = true;
        }
    }
    return best;
}

__global__ void __launch_bounds__(256) prev_stage_onehot_kernel(const uint8_t* __restrict__ seg, int X, int Y, int Z, float* __restrict__ dst,
                                                                int X2, int Y2, int Z2, PrevStageClasses classes, int n_classes) {
    const unsigned ZC = (unsigned)(Z2 + 3) >> 2;                  // 4-voxel chunks per row
    const unsigned units = (unsigned)X2 * (unsigned)Y2 * ZC;      // < 2^31, checked by the launcher
    const long V2 = (long)X2 * Y2 * Z2;
    for (unsigned u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const unsigned row = u / ZC, zc = u - row * ZC;
        const int x = (int)(row / (unsigned)Y2), y = (int)(row - (unsigned)x * (unsigned)Y2);
        const LabelAxis ax = label_axis(x, X, X2), ay = label_axis(y, Y, Y2);
        const uint8_t* r00 = seg + ((long)ax.i0 * Y + ay.i0) * Z;
        const uint8_t* r01 = seg + ((long)ax.i0 * Y + ay.i1) * Z;
        const uint8_t* r10 = seg + ((long)ax.i1 * Y + ay.i0) * Z;
        const uint8_t* r11 = seg + ((long)ax.i1 * Y + ay.i1) * Z;
        const double wxy[4] = {ax.w0 * ay.w0, ax.w0 * ay.w1, ax.w1 * ay.w0, ax.w1 * ay.w1};
        const int z0 = (int)zc * 4, nz = min(4, Z2 - z0);
        int label[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const LabelAxis az = label_axis(min(z0 + e, Z2 - 1), Z, Z2);   // (past the row's end: computed, never stored)
            const int l[8] = {r00[az.i0], r00[az.i1], r01[az.i0], r01[az.i1], r10[az.i0], r10[az.i1], r11[az.i0], r11[az.i1]};
            label[e] = label_at_half(l, wxy, az.w0, az.w1);
        }
        float* p = dst + ((long)row * Z2 + z0);
        const bool whole = nz == 4;
        for (int j = 0; j < n_classes; ++j, p += V2) {
            const int c = classes.v[j];
            const float4 v = make_float4(label[0] == c ? 1.f : 0.f, label[1] == c ? 1.f : 0.f, label[2] == c ? 1.f : 0.f, label[3] == c ? 1.f : 0.f);
            if (whole && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                *reinterpret_cast<float4*>(p) = v;
            } else {
                const float s[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nz) p[e] = s[e];
            }
        }
    }
}

// resample_data_or_seg(is_seg=True, order=1) / resize_segmentation(order=1) of N fp32 label maps: one thread per output voxel
__global__ void __launch_bounds__(256) resize_labels_kernel(const float* __restrict__ src, float* __restrict__ dst, int X, int Y, int Z, int X2,
                                                            int Y2, int Z2, int lx, int ly, int lz, long total) {
    const long V2 = (long)X2 * Y2 * Z2, V = (long)X * Y * Z;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / V2, p = i - n * V2;
        const int z = (int)(p % Z2);
        const long r = p / Z2;
        const int y = (int)(r % Y2), x = (int)(r / Y2);
        const LabelAxis ax = label_axis(x, X, X2, lx), ay = label_axis(y, Y, Y2, ly), az = label_axis(z, Z, Z2, lz);
        const float* s = src + n * V;
        auto at = [&](int a, int b, int c) { return s[((long)a * Y + b) * Z + c]; };
        const float l[8] = {at(ax.i0, ay.i0, az.i0), at(ax.i0, ay.i0, az.i1), at(ax.i0, ay.i1, az.i0), at(ax.i0, ay.i1, az.i1),
                            at(ax.i1, ay.i0, az.i0), at(ax.i1, ay.i0, az.i1), at(ax.i1, ay.i1, az.i0), at(ax.i1, ay.i1, az.i1)};
        const double wxy[4] = {ax.w0 * ay.w0, ax.w0 * ay.w1, ax.w1 * ay.w0, ax.w1 * ay.w1};
        dst[i] = label_at_half(l, wxy, az.w0, az.w1);
    }
}

}  // namespace cf

using namespace cf;

extern "C" int cf_prev_stage_onehot(const uint8_t* seg, int X, int Y, int Z, float* dst, int X2, int Y2, int Z2, const uint8_t* classes,
                                    int n_classes, void* stream) {
    CF_REQUIRE(seg && dst && classes, "null pointer");
    CF_REQUIRE(X > 0 && Y > 0 && Z > 0 && X2 > 0 && Y2 > 0 && Z2 > 0, "bad shape (%d, %d, %d) -> (%d, %d, %d)", X, Y, Z, X2, Y2, Z2);
    CF_REQUIRE(n_classes >= 1 && n_classes <= PREV_STAGE_MAX_CLASSES, "n_classes = %d is outside 1..%d", n_classes, PREV_STAGE_MAX_CLASSES);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 3) == 0, "dst is not aligned to a float");
    const long units = (long)X2 * Y2 * ((Z2 + 3) / 4);
    CF_REQUIRE(units < (1L << 31) - 1, "output of %ld 4-voxel chunks is too large", units);
    PrevStageClasses cls = {};
    for (int j = 0; j < n_classes; ++j) cls.v[j] = classes[j];     // HOST array of the planes' label values
    long blocks = (units + 255) / 256;
    const long cap = (long)device_cu_count() * 8;                   // grid-stride: 8 blocks of 4 waves per compute unit
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(prev_stage_onehot_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), seg, X, Y, Z, dst, X2, Y2, Z2, cls,
                       n_classes);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_resize_labels(const float* src, float* dst, int N, int X, int Y, int Z, int X2, int Y2, int Z2, int linear_x, int linear_y,
                                int linear_z, void* stream) {
    CF_REQUIRE(src && dst && src != dst, "null or aliased pointer");
    CF_REQUIRE(N > 0 && X > 0 && Y > 0 && Z > 0 && X2 > 0 && Y2 > 0 && Z2 > 0, "bad shape (%d; %d, %d, %d) -> (%d, %d, %d)", N, X, Y, Z, X2, Y2, Z2);
    const long total = (long)N * X2 * Y2 * Z2;
    hipLaunchKernelGGL(resize_labels_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, as_stream(stream), src, dst, X, Y, Z, X2, Y2, Z2,
                       linear_x, linear_y, linear_z, total);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
