// Small HBM-bound kernels around the convolutions: GRU gating, channel-slice copies (cat/split), TTA and
// sliding-window accumulation, crop / pad.  One pass each, coalesced along the innermost (x) axis.
#include "common.h"

namespace cf {

static thread_local std::string g_last_error;
void set_error(const std::string& s) { g_last_error = s; }

#define GRID_STRIDE(i, n) for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

__global__ void __launch_bounds__(256) gru_reset_mul_kernel(const float* __restrict__ gates, const float* __restrict__ h,
                                                           float* __restrict__ rh, int C, long CHW, long total) {
    GRID_STRIDE(i, total) {
        long b = i / CHW, r = i - b * CHW;
        rh[i] = gates[b * 2 * CHW + r] * h[i];
    }
}

__global__ void __launch_bounds__(256) gru_blend_kernel(const float* __restrict__ gates, const float* __restrict__ h,
                                                       const float* __restrict__ cand, float* __restrict__ out, long CHW,
                                                       long total) {
    GRID_STRIDE(i, total) {
        long b = i / CHW, r = i - b * CHW;
        float u = gates[b * 2 * CHW + CHW + r];
        out[i] = (1.0f - u) * h[i] + u * cand[i];
    }
}

__global__ void __launch_bounds__(256) binary_kernel(int op, const float* __restrict__ a, const float* __restrict__ b,
                                                    float* __restrict__ out, long n, long period) {
    GRID_STRIDE(i, n) {
        float x = a[i], y = b[period == n ? i : i % period];
        out[i] = op == CF_OP_ADD ? x + y : (op == CF_OP_SUB ? x - y : x * y);
    }
}

// debug aid of the f16-split convolutions (CF_F16S_RANGE_CHECK=1): elements that the hi/lo split cannot represent -- non-finite, or
// |x| >= limit (65504 = fp16 max) -- are counted into one device counter; one ballot + one atomic per wave that saw any
__global__ void __launch_bounds__(256) count_out_of_range_kernel(const float* __restrict__ x, long n, float limit, unsigned long long* __restrict__ counter) {
    GRID_STRIDE(i, n) {
        const float v = x[i];
        const bool bad = !(fabsf(v) < limit);            // NaN compares false: counted
        const unsigned long long m = __ballot(bad);
        if (m && (threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1u) atomicAdd(counter, (unsigned long long)__popcll(m));
    }
}

__global__ void __launch_bounds__(256) copy_channels_kernel(const float* __restrict__ src, int sct, int sco, float* __restrict__ dst,
                                                           int dct, int dco, int C, int HW, int act, long total) {
    GRID_STRIDE(i, total) {
        int p = (int)(i % HW);
        long r = i / HW;
        int c = (int)(r % C);
        long b = r / C;
        dst[(b * dct + dco + c) * HW + p] = act_apply(src[(b * sct + sco + c) * HW + p], act);
    }
}

__global__ void __launch_bounds__(256) coords_grid_kernel(float* __restrict__ out, int H, int W, long total) {
    const int HW = H * W;
    GRID_STRIDE(i, total) {
        int p = (int)(i % HW);
        int ch = (int)((i / HW) & 1);
        out[i] = ch == 0 ? (float)(p % W) : (float)(p / W);
    }
}

__global__ void __launch_bounds__(256) crop2d_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int y0,
                                                    int x0, int h, int w, long total) {
    GRID_STRIDE(i, total) {
        int x = (int)(i % w);
        long r = i / w;
        int y = (int)(r % h);
        long n = r / h;
        dst[i] = src[(n * H + y0 + y) * W + x0 + x];
    }
}

__global__ void __launch_bounds__(256) pad2d_kernel(const float* __restrict__ src, float* __restrict__ dst, int h, int w, int y0,
                                                   int x0, int H, int W, long total) {
    GRID_STRIDE(i, total) {
        int x = (int)(i % W);
        long r = i / W;
        int y = (int)(r % H);
        long n = r / H;
        int ys = y - y0, xs = x - x0;
        dst[i] = ((unsigned)ys < (unsigned)h && (unsigned)xs < (unsigned)w) ? src[(n * h + ys) * w + xs] : 0.f;
    }
}

// acc[b,k,y,x] += weight * softmax_k(logits[b,:,yf,xf])  with (yf,xf) the mirrored position
__global__ void __launch_bounds__(256) tta_accumulate_kernel(const float* __restrict__ logits, float* __restrict__ acc, int K, int H,
                                                            int W, int fh, int fw, float weight, long total) {
    const long HW = (long)H * W;
    GRID_STRIDE(i, total) {  // i over (b, y, x)
        int p = (int)(i % HW);
        long b = i / HW;
        int y = p / W, x = p - y * W;
        int ys = fh ? H - 1 - y : y, xs = fw ? W - 1 - x : x;
        const float* lp = logits + b * K * HW + (long)ys * W + xs;
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, lp[k * HW]);
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += expf(lp[k * HW] - mx);
        float* ap = acc + b * K * HW + p;
        for (int k = 0; k < K; ++k) ap[k * HW] += weight * (expf(lp[k * HW] - mx) / sum);
    }
}

// tta_accumulate_kernel with a per-sample placement: logits [B,K,c,c] of the crops, acc [B,K,H,W]; sample b's window starts at column
// windows[b][0], row windows[b][2] (the crop_indices of cf_crop_windows).  The same softmax expression and the same `+= weight * p` as
// tta_accumulate_kernel: inside the window acc carries the bits of that kernel on a crop-sized buffer followed by pad2d_kernel; outside it
// nothing is read or written.  A window that leaves the map (the table is device data the host never sees) is skipped.
__global__ void __launch_bounds__(256) tta_accumulate_window_kernel(const float* __restrict__ logits, const int* __restrict__ windows,
                                                                   float* __restrict__ acc, int K, int c, int H, int W, int fh, int fw,
                                                                   float weight, long total) {
    const long cc = (long)c * c, HW = (long)H * W;
    GRID_STRIDE(i, total) {  // i over (b, y, x) of the crop
        int p = (int)(i % cc);
        long b = i / cc;
        int y = p / c, x = p - y * c;
        const int x0 = windows[b * 4], y0 = windows[b * 4 + 2];
        if (x0 < 0 || y0 < 0 || x0 > W - c || y0 > H - c) continue;
        int ys = fh ? c - 1 - y : y, xs = fw ? c - 1 - x : x;
        const float* lp = logits + b * K * cc + (long)ys * c + xs;
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, lp[k * cc]);
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += expf(lp[k * cc] - mx);
        float* ap = acc + b * K * HW + (long)(y0 + y) * W + x0 + x;
        for (int k = 0; k < K; ++k) ap[k * HW] += weight * (expf(lp[k * cc] - mx) / sum);
    }
}

__global__ void __launch_bounds__(256) flip2d_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int fh,
                                                    int fw, long total) {
    const long HW = (long)H * W;
    GRID_STRIDE(i, total) {
        int p = (int)(i % HW);
        long n = i / HW;
        int y = p / W, x = p - y * W;
        dst[i] = src[n * HW + (long)(fh ? H - 1 - y : y) * W + (fw ? W - 1 - x : x)];
    }
}

__global__ void __launch_bounds__(256) tile_accumulate_kernel(const float* __restrict__ pred, const float* __restrict__ gauss,
                                                             float* __restrict__ agg, float* __restrict__ cnt, int X, int Y, int lx,
                                                             int ly, int ph, int pw, long total) {
    GRID_STRIDE(i, total) {  // i over (k, py, px)
        int px = (int)(i % pw);
        long r = i / pw;
        int py = (int)(r % ph);
        long k = r / ph;
        float g = gauss ? gauss[py * pw + px] : 1.f;
        long o = (k * X + lx + py) * Y + ly + px;
        agg[o] += pred[i];  // pred already carries the Gaussian weight (mult in _internal_maybe_mirror_and_pred_2D)
        cnt[o] += g;
    }
}


// ---- 3-D twins for _internal_maybe_mirror_and_pred_3D / _internal_predict_3D_3Dconv_tiled (neural_network.py:506-571, :292-430)
__global__ void __launch_bounds__(256) tta_accumulate_3d_kernel(const float* __restrict__ logits, float* __restrict__ acc, int K, int D,
                                                               int H, int W, int fd, int fh, int fw, float weight, long total) {
    const long HW = (long)H * W, V = (long)D * HW;
    GRID_STRIDE(i, total) {  // i over (b, z, y, x)
        long p = i % V, b = i / V;
        int z = (int)(p / HW), q = (int)(p - (long)z * HW);
        int y = q / W, x = q - y * W;
        int zs = fd ? D - 1 - z : z, ys = fh ? H - 1 - y : y, xs = fw ? W - 1 - x : x;
        const float* lp = logits + b * K * V + (long)zs * HW + (long)ys * W + xs;
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, lp[k * V]);
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += expf(lp[k * V] - mx);
        float* ap = acc + b * K * V + p;
        for (int k = 0; k < K; ++k) ap[k * V] += weight * (expf(lp[k * V] - mx) / sum);
    }
}

// The sigmoid form of the two accumulate kernels above (region-based heads, inference_apply_nonlin = nn.Sigmoid()): every channel on its
// own, acc[n,z,y,x] += weight * sigmoid(logits[n, zf, yf, xf]) with n = b * K + k.  No max / sum pass: one read of the logits, one
// read-modify-write of acc.  V = 4: one thread owns 4 consecutive x of a row (W % 4 == 0, no flip along x, both pointers 16-byte aligned:
// every row then starts on a 16-byte boundary); V = 1: one value.  A 2-D map is D = 1.  exp overflows to +inf for logits below about -88.7 and
// 1 / (1 + inf) is 0; it underflows to 0 above, and 1 / (1 + 0) is 1: saturated logits give exactly 0 and 1, never NaN.
__device__ __forceinline__ float sigmoid_f32(float v) { return 1.f / (1.f + expf(-v)); }

template <int V>
__global__ void __launch_bounds__(256) tta_accumulate_sigmoid_kernel(const float* __restrict__ logits, float* __restrict__ acc, int D, int H,
                                                                    int W, int fd, int fh, int fw, float weight, long total) {
    const int Wv = W / V;
    GRID_STRIDE(i, total) {  // i over (n, z, y, x / V)
        const int x = (int)(i % Wv) * V;
        long r = i / Wv;
        const int y = (int)(r % H);
        r /= H;
        const int z = (int)(r % D);
        const long n = r / D;
        const int zs = fd ? D - 1 - z : z, ys = fh ? H - 1 - y : y;
        const float* lp = logits + ((n * D + zs) * H + ys) * (long)W;
        float* ap = acc + ((n * D + z) * H + y) * (long)W + x;
        if constexpr (V == 4) {
            const float4 l = *reinterpret_cast<const float4*>(lp + x);
            float4 a = *reinterpret_cast<const float4*>(ap);
            a.x += weight * sigmoid_f32(l.x);
            a.y += weight * sigmoid_f32(l.y);
            a.z += weight * sigmoid_f32(l.z);
            a.w += weight * sigmoid_f32(l.w);
            *reinterpret_cast<float4*>(ap) = a;
        } else {
            ap[0] += weight * sigmoid_f32(lp[fw ? W - 1 - x : x]);
        }
    }
}

__global__ void __launch_bounds__(256) flip3d_kernel(const float* __restrict__ src, float* __restrict__ dst, int D, int H, int W, int fd,
                                                    int fh, int fw, long total) {
    const long HW = (long)H * W, V = (long)D * HW;
    GRID_STRIDE(i, total) {
        long p = i % V, n = i / V;
        int z = (int)(p / HW), q = (int)(p - (long)z * HW);
        int y = q / W, x = q - y * W;
        dst[i] = src[n * V + (long)(fd ? D - 1 - z : z) * HW + (long)(fh ? H - 1 - y : y) * W + (fw ? W - 1 - x : x)];
    }
}

__global__ void __launch_bounds__(256) tile_accumulate_3d_kernel(const float* __restrict__ pred, const float* __restrict__ gauss,
                                                                float* __restrict__ agg, float* __restrict__ cnt, int X, int Y, int Z,
                                                                int lx, int ly, int lz, int px, int py, int pz, long total) {
    const long pv = (long)px * py * pz;
    GRID_STRIDE(i, total) {  // i over (k, tx, ty, tz)
        long t = i % pv, k = i / pv;
        int tz = (int)(t % pz);
        long r = t / pz;
        int ty = (int)(r % py), tx = (int)(r / py);
        float g = gauss ? gauss[t] : 1.f;
        long o = ((k * X + lx + tx) * Y + ly + ty) * Z + lz + tz;
        agg[o] += pred[i];  // pred already carries the Gaussian weight (mult in _internal_maybe_mirror_and_pred_3D)
        cnt[o] += g;
    }
}

__global__ void __launch_bounds__(256) tile_finalize_kernel(const float* __restrict__ agg, const float* __restrict__ cnt,
                                                           float* __restrict__ probs, uint8_t* __restrict__ seg, int K, long XY) {
    GRID_STRIDE(i, XY) {
        float best = -INFINITY;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            float v = agg[k * XY + i] / cnt[k * XY + i];
            probs[k * XY + i] = v;
            if (v > best) { best = v; arg = k; }
        }
        seg[i] = (uint8_t)arg;
    }
}

// ---- the cine-batched sliding window (neural_network.py:623-769 for many slices at once): cf_tile_gather / cf_tile_merge
// dst[j] = src[n_j][:, lx_j:lx_j+ph, ly_j:ly_j+pw].  V = 4: one thread moves 4 floats of a row (pw % 4 == 0, Y % 4 == 0, both pointers 16-byte
// aligned; the load is one 16-byte access when ly_j % 4 == 0, four 4-byte ones otherwise), V = 1: one float.  A job whose window leaves
// the source (the table is device data the host never sees) reads nothing and gives zeros.
template <int V>
__global__ void __launch_bounds__(256) tile_gather_kernel(const float* __restrict__ src, const int* __restrict__ jobs, float* __restrict__ dst,
                                                         int N, int C, int X, int Y, int ph, int pw, long total) {
    const int pwv = pw / V;
    GRID_STRIDE(i, total) {  // i over (j, c, px, py / V)
        int py = (int)(i % pwv) * V;
        long r = i / pwv;
        int px = (int)(r % ph);
        r /= ph;
        int c = (int)(r % C);
        long j = r / C;
        const int n = jobs[j * 3], lx = jobs[j * 3 + 1], ly = jobs[j * 3 + 2];
        const bool ok = (unsigned)n < (unsigned)N && lx >= 0 && ly >= 0 && lx <= X - ph && ly <= Y - pw;
        const float* s = src + (((long)n * C + c) * X + lx + px) * Y + ly + py;
        float* d = dst + ((j * C + c) * ph + px) * pw + py;
        if constexpr (V == 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                if ((ly & 3) == 0) v = *reinterpret_cast<const float4*>(s);
                else v = make_float4(s[0], s[1], s[2], s[3]);
            }
            *reinterpret_cast<float4*>(d) = v;
        } else {
            d[0] = ok ? s[0] : 0.f;
        }
    }
}

struct TileSteps {   // the step lists of compute_steps_for_sliding_window, by value in the kernel arguments
    int lx[16], ly[16];
    int nx, ny;
};

// One thread per output pixel (V = 1) or per 4 pixels of a row (V = 4: Y % 4 == 0, pw % 4 == 0 and every ly % 4 == 0, so the 4 pixels are
// covered by the same tiles and every access is 16-byte aligned).  Per pixel and class the covering tiles are added IN TILE ORDER (lx outer,
// ly inner) to a zero start -- the fp32 sequence of the serial tile_accumulate launches -- then divided as tile_finalize divides.
template <int V>
__global__ void __launch_bounds__(256) tile_merge_kernel(const float* __restrict__ pred, const float* __restrict__ gauss, float* __restrict__ probs,
                                                        uint8_t* __restrict__ seg, int K, int X, int Y, int ph, int pw, TileSteps st, long total) {
    const int Yv = Y / V, ntile = st.nx * st.ny;
    const long pp = (long)ph * pw, XY = (long)X * Y;
    GRID_STRIDE(i, total) {  // i over (n, x, y / V)
        const int y = (int)(i % Yv) * V;
        long r = i / Yv;
        const int x = (int)(r % X);
        const long n = r / X;
        float cnt[V];
#pragma unroll
        for (int v = 0; v < V; ++v) cnt[v] = 0.f;
        for (int ix = 0; ix < st.nx; ++ix) {
            const int tx = x - st.lx[ix];
            if ((unsigned)tx >= (unsigned)ph) continue;
            for (int iy = 0; iy < st.ny; ++iy) {
                const int ty = y - st.ly[iy];
                if ((unsigned)ty >= (unsigned)pw) continue;
                if constexpr (V == 4) {
                    float4 g = gauss ? *reinterpret_cast<const float4*>(gauss + (long)tx * pw + ty) : make_float4(1.f, 1.f, 1.f, 1.f);
                    cnt[0] += g.x; cnt[1] += g.y; cnt[2] += g.z; cnt[3] += g.w;
                } else {
                    cnt[0] += gauss ? gauss[(long)tx * pw + ty] : 1.f;
                }
            }
        }
        float best[V];
        int arg[V];
#pragma unroll
        for (int v = 0; v < V; ++v) { best[v] = -INFINITY; arg[v] = 0; }
        for (int k = 0; k < K; ++k) {
            float agg[V];
#pragma unroll
            for (int v = 0; v < V; ++v) agg[v] = 0.f;
            for (int ix = 0; ix < st.nx; ++ix) {
                const int tx = x - st.lx[ix];
                if ((unsigned)tx >= (unsigned)ph) continue;
                for (int iy = 0; iy < st.ny; ++iy) {
                    const int ty = y - st.ly[iy];
                    if ((unsigned)ty >= (unsigned)pw) continue;
                    const float* p = pred + ((n * ntile + ix * st.ny + iy) * K + k) * pp + (long)tx * pw + ty;
                    if constexpr (V == 4) {
                        const float4 q = *reinterpret_cast<const float4*>(p);
                        agg[0] += q.x; agg[1] += q.y; agg[2] += q.z; agg[3] += q.w;
                    } else {
                        agg[0] += p[0];
                    }
                }
            }
            float out[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                out[v] = agg[v] / cnt[v];
                if (out[v] > best[v]) { best[v] = out[v]; arg[v] = k; }
            }
            float* o = probs + (n * K + k) * XY + (long)x * Y + y;
            if constexpr (V == 4) *reinterpret_cast<float4*>(o) = make_float4(out[0], out[1], out[2], out[3]);
            else o[0] = out[0];
        }
        uint8_t* so = seg + n * XY + (long)x * Y + y;
        if constexpr (V == 4) *reinterpret_cast<uchar4*>(so) = make_uchar4((uint8_t)arg[0], (uint8_t)arg[1], (uint8_t)arg[2], (uint8_t)arg[3]);
        else so[0] = (uint8_t)arg[0];
    }
}

__global__ void __launch_bounds__(256) argmax_channels_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int K, long HW,
                                                             long total) {
    GRID_STRIDE(i, total) {
        long b = i / HW, p = i - b * HW;
        float best = -INFINITY;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            float v = x[(b * K + k) * HW + p];
            if (v > best) { best = v; arg = k; }
        }
        out[i] = (uint8_t)arg;
    }
}

}  // namespace cf

using namespace cf;

#define LAUNCH_FLAT(kernel, n, ...)                                                                              \
    hipLaunchKernelGGL(kernel, dim3(flat_grid((n), 256)), dim3(256), 0, as_stream(stream), __VA_ARGS__);         \
    CF_CHECK_LAUNCH();                                                                                           \
    return CF_OK

extern "C" const char* cf_last_error(void) { return g_last_error.c_str(); }
extern "C" int cf_version(void) { return 100; }

extern "C" int cf_gru_reset_mul(const float* gates, const float* h, float* rh, int B, int C, int HW, void* stream) {
    CF_REQUIRE(gates && h && rh, "null pointer");
    CF_REQUIRE(B > 0 && C > 0 && HW > 0, "bad shape");
    long chw = (long)C * HW, total = (long)B * chw;
    LAUNCH_FLAT(gru_reset_mul_kernel, total, gates, h, rh, C, chw, total);
}

extern "C" int cf_gru_blend(const float* gates, const float* h, const float* cand, float* out, int B, int C, int HW, void* stream) {
    CF_REQUIRE(gates && h && cand && out, "null pointer");
    CF_REQUIRE(B > 0 && C > 0 && HW > 0, "bad shape");
    long chw = (long)C * HW, total = (long)B * chw;
    LAUNCH_FLAT(gru_blend_kernel, total, gates, h, cand, out, chw, total);
}

extern "C" int cf_binary(int op, const float* a, const float* b, float* out, long n, long b_period, void* stream) {
    CF_REQUIRE(a && b && out, "null pointer");
    CF_REQUIRE(n > 0 && b_period > 0 && b_period <= n && op >= CF_OP_ADD && op <= CF_OP_MUL, "bad arguments");
    LAUNCH_FLAT(binary_kernel, n, op, a, b, out, n, b_period);
}

extern "C" int cf_count_out_of_range(const float* x, long n, float limit, unsigned long long* counter, void* stream) {
    CF_REQUIRE(x && counter && n > 0 && limit > 0.f, "bad arguments");
    LAUNCH_FLAT(count_out_of_range_kernel, n, x, n, limit, counter);
}

extern "C" int cf_copy_channels(const float* src, int src_ctotal, int src_coff, float* dst, int dst_ctotal, int dst_coff, int B,
                                int C, int HW, int act, void* stream) {
    CF_REQUIRE(src && dst, "null pointer");
    CF_REQUIRE(B > 0 && C > 0 && HW > 0 && src_coff >= 0 && dst_coff >= 0 && src_coff + C <= src_ctotal && dst_coff + C <= dst_ctotal,
               "channel slice out of range");
    CF_REQUIRE(act >= CF_ACT_NONE && act <= CF_ACT_SIGMOID, "bad activation");
    long total = (long)B * C * HW;
    LAUNCH_FLAT(copy_channels_kernel, total, src, src_ctotal, src_coff, dst, dst_ctotal, dst_coff, C, HW, act, total);
}

extern "C" int cf_coords_grid(float* out, int B, int H, int W, void* stream) {
    CF_REQUIRE(out && B > 0 && H > 0 && W > 0, "bad arguments");
    long total = (long)B * 2 * H * W;
    LAUNCH_FLAT(coords_grid_kernel, total, out, H, W, total);
}

extern "C" int cf_crop2d(const float* src, float* dst, int N, int H, int W, int y0, int x0, int h, int w, void* stream) {
    CF_REQUIRE(src && dst, "null pointer");
    CF_REQUIRE(N > 0 && h > 0 && w > 0 && y0 >= 0 && x0 >= 0 && y0 + h <= H && x0 + w <= W, "crop window out of range");
    long total = (long)N * h * w;
    LAUNCH_FLAT(crop2d_kernel, total, src, dst, H, W, y0, x0, h, w, total);
}

extern "C" int cf_pad2d(const float* src, float* dst, int N, int h, int w, int y0, int x0, int H, int W, void* stream) {
    CF_REQUIRE(src && dst, "null pointer");
    CF_REQUIRE(N > 0 && h > 0 && w > 0 && y0 >= 0 && x0 >= 0 && y0 + h <= H && x0 + w <= W, "pad window out of range");
    long total = (long)N * H * W;
    LAUNCH_FLAT(pad2d_kernel, total, src, dst, h, w, y0, x0, H, W, total);
}

extern "C" int cf_tta_accumulate(const float* logits, float* acc, int B, int K, int H, int W, int flip_h, int flip_w, float weight,
                                 void* stream) {
    CF_REQUIRE(logits && acc, "null pointer");
    CF_REQUIRE(B > 0 && K > 0 && K <= 64 && H > 0 && W > 0, "bad shape");
    long total = (long)B * H * W;
    LAUNCH_FLAT(tta_accumulate_kernel, total, logits, acc, K, H, W, flip_h, flip_w, weight, total);
}

extern "C" int cf_tta_accumulate_window(const float* logits, const int* windows, float* acc, int B, int K, int crop, int H, int W, int flip_h,
                                        int flip_w, float weight, void* stream) {
    CF_REQUIRE(logits && windows && acc, "null pointer");
    CF_REQUIRE(B > 0 && K > 0 && K <= 64 && crop > 0 && crop <= H && crop <= W, "bad shape B=%d K=%d crop=%d H=%d W=%d", B, K, crop, H, W);
    long total = (long)B * crop * crop;
    LAUNCH_FLAT(tta_accumulate_window_kernel, total, logits, windows, acc, K, crop, H, W, flip_h, flip_w, weight, total);
}

extern "C" int cf_flip2d(const float* src, float* dst, int N, int H, int W, int flip_h, int flip_w, void* stream) {
    CF_REQUIRE(src && dst && src != dst, "null or aliased pointer");
    CF_REQUIRE(N > 0 && H > 0 && W > 0, "bad shape");
    long total = (long)N * H * W;
    LAUNCH_FLAT(flip2d_kernel, total, src, dst, H, W, flip_h, flip_w, total);
}

extern "C" int cf_tile_accumulate(const float* pred, const float* gauss, float* agg, float* cnt, int K, int X, int Y, int lx, int ly,
                                  int ph, int pw, void* stream) {
    CF_REQUIRE(pred && agg && cnt, "null pointer");
    CF_REQUIRE(K > 0 && lx >= 0 && ly >= 0 && lx + ph <= X && ly + pw <= Y && ph > 0 && pw > 0, "tile out of range");
    long total = (long)K * ph * pw;
    LAUNCH_FLAT(tile_accumulate_kernel, total, pred, gauss, agg, cnt, X, Y, lx, ly, ph, pw, total);
}

extern "C" int cf_tile_finalize(const float* agg, const float* cnt, float* probs, uint8_t* seg, int K, int X, int Y, void* stream) {
    CF_REQUIRE(agg && cnt && probs && seg, "null pointer");
    CF_REQUIRE(K > 0 && K <= 255 && X > 0 && Y > 0, "bad shape");
    long xy = (long)X * Y;
    LAUNCH_FLAT(tile_finalize_kernel, xy, agg, cnt, probs, seg, K, xy);
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int cf_tile_gather(const float* src, const int* jobs, float* dst, int J, int N, int C, int X, int Y, int ph, int pw, void* stream) {
    CF_REQUIRE(src && jobs && dst, "null pointer");
    CF_REQUIRE(J > 0 && N > 0 && C > 0 && ph > 0 && pw > 0 && ph <= X && pw <= Y, "bad shape J=%d N=%d C=%d X=%d Y=%d patch %dx%d", J, N, C, X, Y, ph, pw);
    if (pw % 4 == 0 && Y % 4 == 0 && aligned16(src) && aligned16(dst)) {
        long total = (long)J * C * ph * (pw / 4);
        LAUNCH_FLAT(tile_gather_kernel<4>, total, src, jobs, dst, N, C, X, Y, ph, pw, total);
    }
    long total = (long)J * C * ph * pw;
    LAUNCH_FLAT(tile_gather_kernel<1>, total, src, jobs, dst, N, C, X, Y, ph, pw, total);
}

// a step list of compute_steps_for_sliding_window: ascending from 0, the last window ends at the image's end, no gap between windows
static bool steps_cover(const int* l, int n, int p, int size) {
    if (l[0] != 0 || l[n - 1] + p != size) return false;
    for (int i = 1; i < n; ++i)
        if (l[i] <= l[i - 1] || l[i] - l[i - 1] > p) return false;
    return true;
}

extern "C" int cf_tile_merge(const float* pred, const float* gauss, float* probs, uint8_t* seg, int N, int K, int X, int Y, int ph, int pw,
                             const int* lx, int nx, const int* ly, int ny, void* stream) {
    CF_REQUIRE(pred && probs && seg && lx && ly, "null pointer");
    CF_REQUIRE(N > 0 && K > 0 && K <= 255 && ph > 0 && pw > 0 && ph <= X && pw <= Y, "bad shape N=%d K=%d X=%d Y=%d patch %dx%d", N, K, X, Y, ph, pw);
    CF_REQUIRE(nx > 0 && nx <= 16 && ny > 0 && ny <= 16, "1..16 steps per axis, got %d x %d", nx, ny);
    CF_REQUIRE(steps_cover(lx, nx, ph, X) && steps_cover(ly, ny, pw, Y), "the step lists must rise from 0, leave no gap and end at X - ph / Y - pw");
    TileSteps st;
    bool vec = pw % 4 == 0 && Y % 4 == 0 && aligned16(pred) && aligned16(probs) && aligned16(gauss) && (reinterpret_cast<uintptr_t>(seg) & 3) == 0;
    for (int i = 0; i < 16; ++i) {
        st.lx[i] = i < nx ? lx[i] : 0;
        st.ly[i] = i < ny ? ly[i] : 0;
        vec = vec && st.ly[i] % 4 == 0;
    }
    st.nx = nx;
    st.ny = ny;
    if (vec) {
        long total = (long)N * X * (Y / 4);
        LAUNCH_FLAT(tile_merge_kernel<4>, total, pred, gauss, probs, seg, K, X, Y, ph, pw, st, total);
    }
    long total = (long)N * X * Y;
    LAUNCH_FLAT(tile_merge_kernel<1>, total, pred, gauss, probs, seg, K, X, Y, ph, pw, st, total);
}

extern "C" int cf_argmax_channels(const float* x, uint8_t* out, int B, int K, int HW, void* stream) {
    CF_REQUIRE(x && out, "null pointer");
    CF_REQUIRE(B > 0 && K > 0 && K <= 255 && HW > 0, "bad shape");
    long total = (long)B * HW;
    LAUNCH_FLAT(argmax_channels_kernel, total, x, out, K, (long)HW, total);
}

extern "C" int cf_tta_accumulate_3d(const float* logits, float* acc, int B, int K, int D, int H, int W, int flip_d, int flip_h, int flip_w,
                                    float weight, void* stream) {
    CF_REQUIRE(logits && acc, "null pointer");
    CF_REQUIRE(B > 0 && K > 0 && D > 0 && H > 0 && W > 0, "bad shape");
    long total = (long)B * D * H * W;
    LAUNCH_FLAT(tta_accumulate_3d_kernel, total, logits, acc, K, D, H, W, flip_d, flip_h, flip_w, weight, total);
}

// the sigmoid accumulate of [N = B * K] maps of (D, H, W); a 2-D call is D = 1
static int launch_tta_sigmoid(const char* who, const float* logits, float* acc, long N, int D, int H, int W, int fd, int fh, int fw, float weight,
                              void* stream) {
    const long n = N * D * H * W;
    if (W % 4 == 0 && !fw && aligned16(logits) && aligned16(acc)) {
        const long total = n / 4;
        hipLaunchKernelGGL(tta_accumulate_sigmoid_kernel<4>, dim3(flat_grid(total, 256)), dim3(256), 0, as_stream(stream), logits, acc, D, H, W, fd,
                           fh, fw, weight, total);
    } else {
        hipLaunchKernelGGL(tta_accumulate_sigmoid_kernel<1>, dim3(flat_grid(n, 256)), dim3(256), 0, as_stream(stream), logits, acc, D, H, W, fd, fh,
                           fw, weight, n);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string(who) + ": launch failed: " + hipGetErrorString(e));
        return CF_ERR_LAUNCH;
    }
    return CF_OK;
}

extern "C" int cf_tta_accumulate_nonlin(const float* logits, float* acc, int B, int K, int H, int W, int flip_h, int flip_w, float weight,
                                        int nonlin, void* stream) {
    CF_REQUIRE(nonlin == CF_NONLIN_SOFTMAX || nonlin == CF_NONLIN_SIGMOID, "nonlin = %d is neither CF_NONLIN_SOFTMAX nor CF_NONLIN_SIGMOID", nonlin);
    if (nonlin == CF_NONLIN_SOFTMAX) return cf_tta_accumulate(logits, acc, B, K, H, W, flip_h, flip_w, weight, stream);   // the same kernel
    CF_REQUIRE(logits && acc, "null pointer");
    CF_REQUIRE(B > 0 && K > 0 && K <= 64 && H > 0 && W > 0, "bad shape");
    return launch_tta_sigmoid(__func__, logits, acc, (long)B * K, 1, H, W, 0, flip_h, flip_w, weight, stream);
}

extern "C" int cf_tta_accumulate_3d_nonlin(const float* logits, float* acc, int B, int K, int D, int H, int W, int flip_d, int flip_h, int flip_w,
                                           float weight, int nonlin, void* stream) {
    CF_REQUIRE(nonlin == CF_NONLIN_SOFTMAX || nonlin == CF_NONLIN_SIGMOID, "nonlin = %d is neither CF_NONLIN_SOFTMAX nor CF_NONLIN_SIGMOID", nonlin);
    if (nonlin == CF_NONLIN_SOFTMAX) return cf_tta_accumulate_3d(logits, acc, B, K, D, H, W, flip_d, flip_h, flip_w, weight, stream);
    CF_REQUIRE(logits && acc, "null pointer");
    CF_REQUIRE(B > 0 && K > 0 && D > 0 && H > 0 && W > 0, "bad shape");
    return launch_tta_sigmoid(__func__, logits, acc, (long)B * K, D, H, W, flip_d, flip_h, flip_w, weight, stream);
}

extern "C" int cf_flip3d(const float* src, float* dst, int N, int D, int H, int W, int flip_d, int flip_h, int flip_w, void* stream) {
    CF_REQUIRE(src && dst && src != dst, "null or aliased pointer");
    CF_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "bad shape");
    long total = (long)N * D * H * W;
    LAUNCH_FLAT(flip3d_kernel, total, src, dst, D, H, W, flip_d, flip_h, flip_w, total);
}

extern "C" int cf_tile_accumulate_3d(const float* pred, const float* gauss, float* agg, float* cnt, int K, int X, int Y, int Z, int lx,
                                     int ly, int lz, int px, int py, int pz, void* stream) {
    CF_REQUIRE(pred && agg && cnt, "null pointer");
    CF_REQUIRE(K > 0 && lx >= 0 && ly >= 0 && lz >= 0 && lx + px <= X && ly + py <= Y && lz + pz <= Z && px > 0 && py > 0 && pz > 0,
               "tile out of range");
    long total = (long)K * px * py * pz;
    LAUNCH_FLAT(tile_accumulate_3d_kernel, total, pred, gauss, agg, cnt, X, Y, Z, lx, ly, lz, px, py, pz, total);
}


// ---------------------------------------------------------------------------------------------------------------------
// Per-frame bounding boxes of the non-zero pixels (torchvision.ops.masks_to_boxes as Processor.get_mean_centroid uses it,
// processor.py:140-160) and bilinear sampling of a field at a list of points (SpatialTransformerContour, integration.py:5-34).
namespace cf {

template <typename T>
__global__ void __launch_bounds__(256) frame_boxes_kernel(const T* __restrict__ x, int* __restrict__ boxes, int H, int W) {
    __shared__ int red[4];   // x1, y1 (min), x2, y2 (max)
    if (threadIdx.x < 4) red[threadIdx.x] = threadIdx.x < 2 ? INT_MAX : -1;
    __syncthreads();
    const T* f = x + (long)blockIdx.x * H * W;
    int x1 = INT_MAX, y1 = INT_MAX, x2 = -1, y2 = -1;
    for (int i = threadIdx.x; i < H * W; i += blockDim.x) {
        if (f[i] != (T)0) {
            const int yy = i / W, xx = i - yy * W;
            x1 = min(x1, xx); y1 = min(y1, yy); x2 = max(x2, xx); y2 = max(y2, yy);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        x1 = min(x1, __shfl_xor(x1, o, 64)); y1 = min(y1, __shfl_xor(y1, o, 64));
        x2 = max(x2, __shfl_xor(x2, o, 64)); y2 = max(y2, __shfl_xor(y2, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { atomicMin(&red[0], x1); atomicMin(&red[1], y1); atomicMax(&red[2], x2); atomicMax(&red[3], y2); }
    __syncthreads();
    if (threadIdx.x < 4) boxes[blockIdx.x * 4 + threadIdx.x] = red[2] < 0 ? -1 : red[threadIdx.x];
}

// Processor.get_mean_centroid for ONE frame followed by Processor.adjust_cropping_window (processor.py:140-160, :109-132), per sample and
// in integers: the box of the non-zero labels as frame_boxes_kernel finds it, centre x1 + (x2 - x1) / 2 (the reference's fp32 value has a
// fraction of 0 or .5 and .int() truncates it: the integer division), an empty map takes (H / 2, W / 2) in that order, then the clamps.
// One block per sample, a grid-stride loop over the samples.  WORDS: the map is read four labels per load (W % 4 == 0, 4-byte aligned base).
// windows[n] = {x_low, x_high, y_low, y_high} (crop_indices);  jobs[n] = {n, y_low, x_low}: a cf_tile_gather job (rows first).
template <bool WORDS>
__global__ void __launch_bounds__(256) crop_windows_kernel(const uint8_t* __restrict__ lab, int* __restrict__ windows, int* __restrict__ jobs,
                                                          int N, int H, int W, int crop, int image) {
    __shared__ int red[4];   // x1, y1 (min), x2, y2 (max)
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        if (threadIdx.x < 4) red[threadIdx.x] = threadIdx.x < 2 ? INT_MAX : -1;
        __syncthreads();
        const uint8_t* f = lab + (long)n * H * W;
        int x1 = INT_MAX, y1 = INT_MAX, x2 = -1, y2 = -1;
        if constexpr (WORDS) {
            const uint32_t* f4 = reinterpret_cast<const uint32_t*>(f);
            for (int i = threadIdx.x; i < H * W / 4; i += blockDim.x) {
                const uint32_t v = f4[i];
                if (v) {
                    const int yy = (i * 4) / W, xx = i * 4 - yy * W;      // W % 4 == 0: the four labels lie in one row
                    x1 = min(x1, xx + ((__ffs((int)v) - 1) >> 3)); x2 = max(x2, xx + ((31 - __clz((int)v)) >> 3));
                    y1 = min(y1, yy); y2 = max(y2, yy);
                }
            }
        } else {
            for (int i = threadIdx.x; i < H * W; i += blockDim.x) {
                if (f[i]) {
                    const int yy = i / W, xx = i - yy * W;
                    x1 = min(x1, xx); y1 = min(y1, yy); x2 = max(x2, xx); y2 = max(y2, yy);
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            x1 = min(x1, __shfl_xor(x1, o, 64)); y1 = min(y1, __shfl_xor(y1, o, 64));
            x2 = max(x2, __shfl_xor(x2, o, 64)); y2 = max(y2, __shfl_xor(y2, o, 64));
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&red[0], x1); atomicMin(&red[1], y1); atomicMax(&red[2], x2); atomicMax(&red[3], y2); }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cx = red[2] < 0 ? H / 2 : red[0] + (red[2] - red[0]) / 2;
            const int cy = red[2] < 0 ? W / 2 : red[1] + (red[3] - red[1]) / 2;
            const int half = crop / 2;
            int x_low = max(0, cx - half), x_high = min(image, cx + half), y_low = max(0, cy - half), y_high = min(image, cy + half);
            if (x_low == 0) x_high = crop;
            if (x_high == image) x_low = image - crop;
            if (y_low == 0) y_high = crop;
            if (y_high == image) y_low = image - crop;
            windows[n * 4 + 0] = x_low; windows[n * 4 + 1] = x_high; windows[n * 4 + 2] = y_low; windows[n * 4 + 3] = y_high;
            jobs[n * 3 + 0] = n; jobs[n * 3 + 1] = y_low; jobs[n * 3 + 2] = x_low;
        }
        __syncthreads();     // red is reset by the next trip
    }
}

// out[b, c, p] = bilinear sample of field[b, c] at the point whose grid_sample coordinates are (gx, gy) = the normalised
// (pts[b,0,p], pts[b,1,p]): 2 * (v / (size - 1) - 0.5) with size = W for channel 0 and H for channel 1 (the reference's shape[~i]),
// align_corners = True, zeros outside -- every intermediate rounded as PyTorch rounds it.
__global__ void __launch_bounds__(256) sample_points_kernel(const float* __restrict__ field, const float* __restrict__ pts, float* __restrict__ out,
                                                           int B, int C, int H, int W, int P) {
    const long total = (long)B * C * P;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int p = (int)(idx % P);
        const long r = idx / P;
        const int c = (int)(r % C), b = (int)(r / C);
        const float px = pts[((long)b * 2 + 0) * P + p], py = pts[((long)b * 2 + 1) * P + p];
        const float gx = __fmul_rn(2.0f, __fsub_rn(__fdiv_rn(px, (float)(W - 1)), 0.5f));
        const float gy = __fmul_rn(2.0f, __fsub_rn(__fdiv_rn(py, (float)(H - 1)), 0.5f));
        const float xs = __fmul_rn(__fdiv_rn(__fadd_rn(gx, 1.0f), 2.0f), (float)(W - 1));
        const float ys = __fmul_rn(__fdiv_rn(__fadd_rn(gy, 1.0f), 2.0f), (float)(H - 1));
        Taps t = make_taps(ys, xs, H, W);
        out[idx] = sample_taps(field + ((long)b * C + c) * H * W, t, W);
    }
}

}  // namespace cf

extern "C" int cf_frame_boxes(const void* x, int is_float, int* boxes, int N, int H, int W, void* stream) {
    CF_REQUIRE(x && boxes, "null pointer");
    CF_REQUIRE(N > 0 && H > 0 && W > 0 && (long)H * W < (1L << 31), "bad shape N=%d H=%d W=%d", N, H, W);
    if (is_float) hipLaunchKernelGGL(cf::frame_boxes_kernel<float>, dim3((unsigned)N), dim3(256), 0, cf::as_stream(stream), (const float*)x, boxes, H, W);
    else hipLaunchKernelGGL(cf::frame_boxes_kernel<uint8_t>, dim3((unsigned)N), dim3(256), 0, cf::as_stream(stream), (const uint8_t*)x, boxes, H, W);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_crop_windows(const uint8_t* labels, int* windows, int* jobs, int N, int H, int W, int crop, int image, void* stream) {
    CF_REQUIRE(labels && windows && jobs, "null pointer");
    CF_REQUIRE(N > 0 && H > 0 && W > 0 && (long)H * W < (1L << 31) && N <= (1 << 28), "bad shape N=%d H=%d W=%d", N, H, W);
    CF_REQUIRE(crop > 0 && crop % 2 == 0 && crop <= image && image <= H && image <= W,
               "bad window crop=%d image=%d on a %dx%d map: crop must be even (Processor.crop_and_pad cuts 2 * (crop / 2) pixels) and crop <= image <= H, W",
               crop, image, H, W);
    const unsigned grid = (unsigned)(N < 4096 ? N : 4096);
    if (W % 4 == 0 && (reinterpret_cast<uintptr_t>(labels) & 3) == 0)
        hipLaunchKernelGGL(cf::crop_windows_kernel<true>, dim3(grid), dim3(256), 0, cf::as_stream(stream), labels, windows, jobs, N, H, W, crop, image);
    else
        hipLaunchKernelGGL(cf::crop_windows_kernel<false>, dim3(grid), dim3(256), 0, cf::as_stream(stream), labels, windows, jobs, N, H, W, crop, image);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_sample_points_2d(const float* field, const float* pts, float* out, int B, int C, int H, int W, int P, void* stream) {
    CF_REQUIRE(field && pts && out, "null pointer");
    CF_REQUIRE(B > 0 && C > 0 && H > 1 && W > 1 && P > 0, "bad shape");
    const long total = (long)B * C * P;
    hipLaunchKernelGGL(cf::sample_points_kernel, dim3(cf::flat_grid(total, 256)), dim3(256), 0, cf::as_stream(stream), field, pts, out, B, C, H, W, P);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
