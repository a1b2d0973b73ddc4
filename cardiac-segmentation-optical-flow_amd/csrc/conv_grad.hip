// Backward of the exact-fp32 convolution (conv.hip) on the same MFMA, v_mfma_f32_32x32x2_f32: every product exact, every sum a k-ordered
// fmaf chain, so both gradients are the same bits on every run.  No atomics, no workgroup waits on another.
//
//   wgrad   dW[n = (ci,kh,kw)][m = co] = sum over pixels (b,oy,ox) of  dY[b,co,oy,ox] * X[b,ci,oy*s+kh-ph,ox*s+kw-pw]
//           A GEMM with a small M x N and a long K (the pixels).  K is cut into `splits` chunks of whole pixel pairs; one wave owns one
//           32 x 32 tile of one chunk and writes it to part[split][n][m].  A second launch adds the chunks in split order (fp64) and
//           writes dW in the [(Cin*kh*kw), Cout] layout the forward reads.  db rides along: the waves of the first n-tile also sum their
//           dY operand (fp64), one partial per split.
//   dgrad   dX[b,ci,iy,ix] = sum over k = (co,kh,kw) of W[(ci,kh,kw)][co] * dY[b,co,(iy+ph-kh)/s,(ix+pw-kw)/s]   (taps that divide only)
//           conv.hip's implicit GEMM with the roles of the channel axes exchanged and the gather inverted: no zero-stuffed map for
//           stride 2.  The result goes to a channel range of a wider tensor, overwriting or adding (one read, one add, one write: the
//           second gradient of a skip map lands on the first in call order).
#include "common.h"

namespace cf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GradParams {
    const float* x1;
    const float* x2;
    const float* dy;
    const float* wt;
    float* part;
    double* bpart;
    float* dx;
    int C1, C2, B, H, W, Cout, KH, KW, stride, pad_h, pad_w, Ho, Wo;
    int Ktot;      // (C1 + C2) * KH * KW
    long P;        // B * Ho * Wo
    long chunk;    // pixels per split (even)
    int ntn;       // n-tiles
    int want_bias;
    int ci_off, Cn, dx_ctotal, dx_coff, accumulate;
};

// one wave = one 32 (co) x 32 (k index) tile of one pixel chunk
__global__ void __launch_bounds__(64) conv_wgrad_kernel(const GradParams p) {
    constexpr int PF = 4;
    const int lane = threadIdx.x, half = lane >> 5, l31 = lane & 31;
    const int nt = blockIdx.x % p.ntn, mt = blockIdx.x / p.ntn;
    const int split = blockIdx.y;
    const int HoWo = p.Ho * p.Wo, HW = p.H * p.W, KHW = p.KH * p.KW;
    const int co = mt * 32 + l31;
    const int n = nt * 32 + l31;
    const bool mv = co < p.Cout, nv = n < p.Ktot;
    const int nn = nv ? n : 0;
    const int ci = nn / KHW, kr = nn - ci * KHW, kh = kr / p.KW, kw = kr - kh * p.KW;
    const float* xc = ci < p.C1 ? p.x1 + (long)ci * HW : p.x2 + (long)(ci - p.C1) * HW;
    const int Cx = ci < p.C1 ? p.C1 : p.C2;     // channels of the tensor this lane's input plane lives in
    const long p0 = (long)split * p.chunk;
    long pend = p0 + p.chunk;
    if (pend > p.P) pend = p.P;

    // pixel cursor of this half-wave: pix, pix + 2, ...
    long pix = p0 + half;
    int b = (int)(pix / HoWo);
    int r = (int)(pix - (long)b * HoWo);
    int oy = r / p.Wo, ox = r - oy * p.Wo;

    float a[PF], bq[PF];
    double bs = 0.0;
    const bool do_bias = p.want_bias && nt == 0;
    auto load_step = [&](int slot) {
        const bool pv = pix < pend;
        float av = 0.f, bv = 0.f;
        if (pv) {
            if (mv) av = p.dy[((long)b * p.Cout + co) * HoWo + (long)oy * p.Wo + ox];
            const int iy = oy * p.stride + kh - p.pad_h, ix = ox * p.stride + kw - p.pad_w;
            if (nv && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) bv = xc[(long)b * Cx * HW + (long)iy * p.W + ix];
        }
        a[slot] = av;
        bq[slot] = bv;
        pix += 2;
        ox += 2;
        while (ox >= p.Wo) { ox -= p.Wo; ++oy; }
        while (oy >= p.Ho) { oy -= p.Ho; ++b; }
    };

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int s = 0; s < PF; ++s) load_step(s);
    for (long k0 = p0; k0 < pend; k0 += 2 * PF) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bq[s], acc, 0, 0, 0);
            if (do_bias) bs += (double)a[s];
            load_step(s);   // zeros past the chunk
        }
    }

    // C/D layout: col = lane & 31 (n), row = (i & 3) + 8 * (i >> 2) + 4 * half (co)
    if (nv) {
        float* dst = p.part + ((long)split * p.Ktot + n) * p.Cout;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
            if (c < p.Cout) dst[c] = acc[i];
        }
    }
    if (do_bias) {
        const double other = __shfl_xor(bs, 32);
        if (half == 0 && mv) p.bpart[(long)split * p.Cout + co] = bs + other;   // even pixels + odd pixels, the same order every run
    }
}

__global__ void __launch_bounds__(256) conv_wgrad_reduce_kernel(const float* __restrict__ part, const double* __restrict__ bpart,
                                                                float* __restrict__ dw, float* __restrict__ db, long MN, int Cout,
                                                                int splits) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < MN) {
        double s = 0.0;
        for (int sp = 0; sp < splits; ++sp) s += (double)part[(long)sp * MN + i];
        dw[i] = (float)s;
    }
    if (db && i < Cout) {
        double s = 0.0;
        for (int sp = 0; sp < splits; ++sp) s += bpart[(long)sp * Cout + i];
        db[i] = (float)s;
    }
}

// four waves on four consecutive tiles of 64 input pixels, 32 input channels each
__global__ void __launch_bounds__(256) conv_dgrad_kernel(const GradParams p) {
    constexpr int PF = 4, NT = 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int HW = p.H * p.W, HoWo = p.Ho * p.Wo, KHW = p.KH * p.KW;
    const long Ntot = (long)p.B * HW;
    const long n0 = ((long)blockIdx.x * 4 + wave) * (32 * NT);
    if (n0 >= Ntot) return;   // wave-uniform
    const int m0 = blockIdx.y * 32;
    const int K = p.Cout * KHW;
    const int sh = p.stride == 2 ? 1 : 0, smask = p.stride - 1;

    bool pv[NT];
    int ty0[NT], tx0[NT];
    const float* dyb[NT];
    long obase[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const long n = n0 + t * 32 + l31;
        pv[t] = n < Ntot;
        const long nn = pv[t] ? n : 0;
        const int b = (int)(nn / HW);
        const int r = (int)(nn - (long)b * HW);
        const int iy = r / p.W, ix = r - iy * p.W;
        ty0[t] = iy + p.pad_h;
        tx0[t] = ix + p.pad_w;
        dyb[t] = p.dy + (long)b * p.Cout * HoWo;
        obase[t] = ((long)b * p.dx_ctotal + p.dx_coff) * HW + r;
    }
    const int mci = m0 + l31;
    const bool mv = mci < p.Cn;
    const long wrow = (long)(p.ci_off + (mv ? mci : 0)) * KHW * p.Cout;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    int lk = half, co = 0, kh = 0, kw = half;
    while (kw >= p.KW) { kw -= p.KW; ++kh; }
    while (kh >= p.KH) { kh -= p.KH; ++co; }

    float a[PF], bq[PF][NT];
    auto load_step = [&](int slot) {
        const bool kv = lk < K;
        a[slot] = (kv && mv) ? p.wt[wrow + (long)(kh * p.KW + kw) * p.Cout + co] : 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int ty = ty0[t] - kh, tx = tx0[t] - kw;
            const int oy = ty >> sh, ox = tx >> sh;
            const bool ok = kv && pv[t] && ty >= 0 && tx >= 0 && !(ty & smask) && !(tx & smask) && oy < p.Ho && ox < p.Wo;
            bq[slot][t] = ok ? dyb[t][(long)co * HoWo + (long)oy * p.Wo + ox] : 0.f;
        }
        lk += 2;
        kw += 2;
        while (kw >= p.KW) { kw -= p.KW; ++kh; }
        while (kh >= p.KH) { kh -= p.KH; ++co; }
    };
#pragma unroll
    for (int s = 0; s < PF; ++s) load_step(s);
    for (int k0 = 0; k0 < K; k0 += 2 * PF) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bq[s][t], acc[t], 0, 0, 0);
            load_step(s);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = m0 + (i & 3) + 8 * (i >> 2) + 4 * half;
        if (c >= p.Cn) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (!pv[t]) continue;
            float* d = p.dx + obase[t] + (long)c * HW;
            *d = p.accumulate ? *d + acc[t][i] : acc[t][i];
        }
    }
}

// the K split of one wgrad: a function of the shape alone, so the partition (and with it every bit of dW) is the same on every call
static int wgrad_splits(int Cout, int Ktot, long P) {
    const long tiles = (long)cdiv(Cout, 32) * cdiv(Ktot, 32);
    long want = (2048 + tiles - 1) / tiles;          // about 2048 waves in flight
    const long most = (P + 255) / 256;               // at least 256 pixels per split
    if (want > most) want = most;
    if (want > 256) want = 256;
    if (want < 1) want = 1;
    long chunk = (P + want - 1) / want;
    chunk += chunk & 1;
    return (int)((P + chunk - 1) / chunk);
}

static int conv_shape_ok(const char* who, int C1, int C2, int B, int H, int W, int Cout, int KH, int KW, int stride, int* Ho, int* Wo) {
    CF_REQUIRE_AS(who, C1 > 0 && C2 >= 0, "bad channel split C1=%d C2=%d", C1, C2);
    CF_REQUIRE_AS(who, B > 0 && H > 0 && W > 0 && Cout > 0, "bad shape B=%d H=%d W=%d Cout=%d", B, H, W, Cout);
    CF_REQUIRE_AS(who, (KH == 3 && KW == 3) || (KH == 1 && KW == 1), "kernel %dx%d: 3x3 (pad 1) or 1x1 (pad 0) only", KH, KW);
    CF_REQUIRE_AS(who, stride == 1 || stride == 2, "stride %d: 1 or 2", stride);
    const int pad = KH / 2;
    *Ho = (H + 2 * pad - KH) / stride + 1;
    *Wo = (W + 2 * pad - KW) / stride + 1;
    CF_REQUIRE_AS(who, *Ho > 0 && *Wo > 0, "empty output");
    CF_REQUIRE_AS(who, (long)B * (C1 + C2) * H * W < (1L << 40) && (long)(C1 + C2) * KH * KW * Cout < (1L << 31), "tensor too large");
    return CF_OK;
}

}  // namespace cf

using namespace cf;

extern "C" int cf_conv2d_wgrad_splits(int Cin, int Cout, int KH, int KW, int B, int Ho, int Wo) {
    CF_REQUIRE(Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && B > 0 && Ho > 0 && Wo > 0, "bad shape");
    return wgrad_splits(Cout, Cin * KH * KW, (long)B * Ho * Wo);
}

extern "C" int cf_conv2d_wgrad(const float* x1, int C1, const float* x2, int C2, const float* dy, float* dw, float* db, void* ws,
                               long ws_bytes, int B, int H, int W, int Cout, int KH, int KW, int stride, void* stream) {
    CF_REQUIRE(x1 && dy && dw && ws, "null pointer");
    CF_REQUIRE(C2 == 0 || x2, "x2 missing");
    int Ho, Wo;
    if (int rc = conv_shape_ok(__func__, C1, C2, B, H, W, Cout, KH, KW, stride, &Ho, &Wo)) return rc;
    GradParams p = {};
    p.Ktot = (C1 + C2) * KH * KW;
    p.P = (long)B * Ho * Wo;
    const int splits = wgrad_splits(Cout, p.Ktot, p.P);
    const long MN = (long)p.Ktot * Cout;
    const long part_bytes = ((long)splits * MN * 4 + 7) & ~7L;
    CF_REQUIRE(ws_bytes >= part_bytes + (long)splits * Cout * 8, "workspace: %ld bytes, need %ld", ws_bytes, part_bytes + (long)splits * Cout * 8);
    CF_REQUIRE(((uintptr_t)ws & 7) == 0, "workspace must be 8-byte aligned");
    p.x1 = x1; p.x2 = C2 ? x2 : nullptr; p.dy = dy;
    p.part = (float*)ws;
    p.bpart = (double*)((char*)ws + part_bytes);
    p.C1 = C1; p.C2 = C2; p.B = B; p.H = H; p.W = W; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride;
    p.pad_h = p.pad_w = KH / 2; p.Ho = Ho; p.Wo = Wo;
    p.chunk = (p.P + splits - 1) / splits;
    p.chunk += p.chunk & 1;
    p.ntn = cdiv(p.Ktot, 32);
    p.want_bias = db != nullptr;
    const long tiles = (long)p.ntn * cdiv(Cout, 32);
    CF_REQUIRE(tiles < (1L << 31), "grid too large");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(64), 0, s, p);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)cdiv(MN > Cout ? MN : Cout, 256)), dim3(256), 0, s, p.part, p.bpart, dw, db, MN,
                       Cout, splits);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_conv2d_dgrad(const float* dy, const float* wt, float* dx, int dx_ctotal, int dx_coff, int ci_off, int Cn, int Cin, int B,
                               int H, int W, int Cout, int KH, int KW, int stride, int accumulate, void* stream) {
    CF_REQUIRE(dy && wt && dx, "null pointer");
    int Ho, Wo;
    if (int rc = conv_shape_ok(__func__, Cin, 0, B, H, W, Cout, KH, KW, stride, &Ho, &Wo)) return rc;
    CF_REQUIRE(ci_off >= 0 && Cn > 0 && ci_off + Cn <= Cin, "input channel range [%d, %d) outside %d", ci_off, ci_off + Cn, Cin);
    CF_REQUIRE(dx_coff >= 0 && dx_coff + Cn <= dx_ctotal, "destination channel slice out of range");
    GradParams p = {};
    p.dy = dy; p.wt = wt; p.dx = dx;
    p.B = B; p.H = H; p.W = W; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad_h = p.pad_w = KH / 2; p.Ho = Ho; p.Wo = Wo;
    p.ci_off = ci_off; p.Cn = Cn; p.dx_ctotal = dx_ctotal; p.dx_coff = dx_coff; p.accumulate = accumulate ? 1 : 0;
    const long ntiles = ((long)B * H * W + 255) / 256;
    CF_REQUIRE(ntiles < (1L << 31), "grid too large");
    hipLaunchKernelGGL(conv_dgrad_kernel, dim3((unsigned)ntiles, (unsigned)cdiv(Cn, 32)), dim3(256), 0, as_stream(stream), p);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
