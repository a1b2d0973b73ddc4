/*
 * cineflow.h -- C ABI of libcineflow_hip.so (MI355X / gfx950 only).
 *
 * The reference (nicolas1805961/Cardiac-Segmentation-Optical-flow) has no FFI layer: its operator
 * boundary is the `forward` of a handful of PyTorch modules.  Each entry point
 * below replaces the device work of one such `forward` (or a fused group of them) and cites it as
 * file:line relative to the reference root.  INTEGRATION.md shows the ctypes stub a reference maintainer
 * would add to route those modules here.
 *
 * Conventions
 *   - all tensors are caller-owned device pointers, contiguous, fp32 unless stated, NCHW ("channel-first");
 *   - no allocation, no ownership transfer, no host synchronisation inside the library; workspaces are
 *     passed in; every launch goes on the caller's `stream` (a hipStream_t passed as void*), so every
 *     entry point is safe to capture in a hipGraph and to call concurrently on different streams;
 *   - return value 0 = success, <0 = error (CF_ERR_*); cf_last_error() gives the text for the calling
 *     thread.  Shapes are validated on the host before any launch.
 */
#ifndef CINEFLOW_H
#define CINEFLOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_OK 0
#define CF_ERR_ARG (-1)     /* bad shape / null pointer / unsupported size */
#define CF_ERR_LAUNCH (-2)  /* hipGetLastError() after a launch            */

/* activation codes used by the fused epilogues */
#define CF_ACT_NONE 0
#define CF_ACT_GELU 1    /* exact erf GELU (torch.nn.GELU default)       */
#define CF_ACT_RELU 2
#define CF_ACT_LRELU 3   /* LeakyReLU(0.01), generic_UNet.py:38          */
#define CF_ACT_TANH 4
#define CF_ACT_SIGMOID 5
#define CF_ACT_MISH 6    /* x tanh(softplus(x)); cf_coef_apply only       */

/* residual placement for cf_group_norm */
#define CF_RES_NONE 0
#define CF_RES_BEFORE_ACT 1  /* SingleConv, lib/utils.py:1258-1261  */
#define CF_RES_AFTER_ACT 2   /* DoubleConv, lib/utils.py:1207-1212  */

const char* cf_last_error(void);
int cf_version(void);

/* ---------------------------------------------------------------- VoxelMorph warp family
 * SpatialTransformer.forward, nnunet/network_architecture/integration.py:61-79 (2-D branch):
 * out[b,c,i,j] = bilinear(src[b,c], i + flow[b,0,i,j], j + flow[b,1,i,j]), align_corners=True, zero padding,
 * with the reference's normalise/un-normalise fp32 rounding path reproduced.
 * No entry point of this family requires more than the natural alignment of its element type: the four-pixel kernels (W % 4 == 0) run
 * only when every tensor they access 16 bytes at a time (4 for the label output) lies on such a boundary, the one-pixel kernels
 * otherwise, with bit-identical results. */
int cf_warp_bilinear_2d(const float* flow, const float* src, float* out, int B, int C, int H, int W, void* stream);

/* VecInt.forward, integration.py:95-99: v = v/2^nsteps; nsteps x { v = v + warp(v, v) }.
 * `tmp` is a caller workspace of B*2*H*W floats; result in `out` (may not alias `vec`). */
int cf_vecint_2d(const float* vec, float* out, float* tmp, int B, int H, int W, int nsteps, void* stream);

/* warp_linear, nnunet/network_architecture/SegFlowGaussian.py:3571-3580, fused:
 * one_hot(labels, K) -> warp with flow[t] -> argmax over K (first maximum wins).
 * flow [T,B,2,H,W]; labels uint8 [B,H,W] (ED label map, values < K <= 8); out uint8 [T,B,H,W]. */
int cf_warp_labels_2d(const float* flow, const uint8_t* labels, uint8_t* out, int T, int B, int K, int H, int W,
                      void* stream);

/* The 6-channel memory-encoder input of SegFlowGaussian.py:1427-1433 / :1898-1904, fused:
 * reg = warp(cum, xt); out = cat[x0, xt, cum(2), x0 - reg, reg].  x0, xt [B,1,H,W]; cum [B,2,H,W]; out [B,6,H,W]. */
int cf_memory_input(const float* x0, const float* xt, const float* cum, float* out, int B, int H, int W, void* stream);

/* jacobian_determinant, nnunet/compute_jacobian.py:16-59 (2-D branch), np.gradient semantics, float64 math.
 * disp [B,2,H,W] channel-first (channel 0 along axis H); det float64 [B,H,W].  H,W >= 2. */
int cf_jacobian_det_2d(const float* disp, double* det, int B, int H, int W, void* stream);

/* 3-D branches of the same two functions: SpatialTransformer.forward for a volume (integration.py:75-77; trilinear,
 * align_corners=True, zeros outside; flow [B,3,D,H,W] with channel i displacing along axis i of (D,H,W), src/out
 * [B,C,D,H,W], out must not alias src) and jacobian_determinant's 3-D case (compute_jacobian.py:42-52;
 * disp [B,3,D,H,W] -> det float64 [B,D,H,W]).  All sizes >= 2. */
int cf_warp_trilinear_3d(const float* flow, const float* src, float* out, int B, int C, int D, int H, int W, void* stream);
int cf_jacobian_det_3d(const float* disp, double* det, int B, int D, int H, int W, void* stream);

/* ---------------------------------------------------------------- correlation
 * CorrVolume(radius, stride)(cur, prev) -- source absent from the reference; call sites
 * SegFlowGaussian.py:256-261, :1376-1377; spec in DESIGN.md ("parity unpinned"):
 * out[b,(dy+r)(2r+1)+(dx+r),y,x] = mean_c cur[b,c,y,x] * prev[b,c,y+dy*stride,x+dx*stride], zero outside. */
int cf_corr_volume(const float* cur, const float* prev, float* out, int B, int C, int H, int W, int radius, int stride,
                   void* stream);
/* The kernel cf_corr_volume launches for these arguments (host code, launches nothing; cf_corr_volume dispatches on this very value):
 * 0 = the one-thread-per-output kernel (any radius <= 8, any stride, any alignment), 1 = the persistent fp32 kernel (radius 4, stride 1 / 2 / 4,
 * W % 4 == 0, both inputs 16-byte aligned), 2 = the f16-MFMA kernel (see cf_corr_mfma_enable).
 * Non-finite inputs.  The zero padding is a factor like any other: on every route a NaN in cur makes all (2r+1)^2 outputs of its pixel NaN
 * (cur * 0 at the displacements that leave the map), and a NaN in prev reaches exactly the outputs that read it, as in the oracle.  An Inf in
 * cur makes all outputs of its pixel non-finite: NaN where the displacement leaves the map (Inf * 0), +-Inf or NaN elsewhere (Inf * prev) on
 * routes 0 and 1, NaN on route 2.  Routes 0 and 1 are fp32 throughout.  Route 2 splits both operands into f16 halves: a finite |value| above
 * the f16 range (65504, after rounding: >= 65520) has hi = Inf, lo = -Inf there, and every output that reads it is NaN; nothing else is
 * affected and no range scan is made.  Features of that size belong on route 1 (cf_corr_mfma_enable(0)). */
int cf_corr_volume_route(const float* cur, const float* prev, int C, int H, int W, int radius, int stride);
/* A/B knob without a reference counterpart: CorrVolume calls with radius 4, dilation 1 / 2 / 4, C % 16 == 0, W % 64 == 0 and H % (8 x dilation) == 0
 * run on the f16-MFMA kernel (csrc/corr_mfma.hip: 2-D banded products of hi/lo-split operands, fp32 accumulation, within 1e-5 of the fp32 kernel);
 * 0 keeps them on the fp32 vector kernel (also CF_CORR_MFMA=0).  Returns the previous setting.  The 1e-5 is for O(1) features: the split keeps
 * 22 bits relative to O(1) only (measured |out - true| up to 1.7e-5 x the sum of |cur||prev| / C with cur x 300, prev x 1e-3) and has the f16
 * range; see the comment of cf_corr_volume_route above and the header of csrc/corr_mfma.hip. */
int cf_corr_mfma_enable(int on);

/* CorrBlock (published RAFT; call site SegFlowGaussian.py:929): all-pairs volume
 * corr[b, n1, n2] = sum_c f1[b,c,n1] f2[b,c,n2] / sqrt(C) into pyr level 0, then `levels`-1 2x2 average pools.
 * pyr: one buffer, level l at element offset sum_{j<l} B*N*(H>>j)*(W>>j), N = H*W.  H*W % 64 == 0. */
int cf_corr_pyramid(const float* f1, const float* f2, float* pyr, int B, int C, int H, int W, int levels, void* stream);

/* CorrBlock.__call__(coords), call site SegFlowGaussian.py:935: radius-r bilinear lookup on every level.
 * coords [B,2,H,W] (x,y); out [B, levels*(2r+1)^2, H, W]. */
int cf_corr_lookup(const float* pyr, const float* coords, float* out, int B, int H, int W, int levels, int radius,
                   void* stream);

/* SegFlowGaussian.upsample_flow, SegFlowGaussian.py:846-857: convex 8x upsampling.
 * flow [B,C,h,w], mask [B,576,h,w] -> out [B,C,8h,8w] (C = 2 for flow, 4 for upsample_seg :860-871). */
int cf_convex_upsample(const float* flow, const float* mask, float* out, int B, int C, int h, int w, void* stream);

/* ---------------------------------------------------------------- convolution (implicit GEMM on fp32 MFMA)
 * nn.Conv2d forward as used by DoubleConv (lib/utils.py:1182-1215), ConvDropoutNormNonlin
 * (generic_UNet.py:64-68), ConvGRUCell (convGRU.py:57-66), the nn.Linear / MultiheadAttention projections of
 * TransformerFlowLayer (lib/vit_transformer.py:1253-1267, as 1x1 convs on channel-first tokens) and the RAFT
 * update block.  The input is the channel concatenation cat[x1 (C1 ch), x2 (C2 ch)] (x2 may be NULL/0): the
 * reference's torch.cat((skip, x), 1) never materialises.
 *   wt    : weights pre-transposed to [K = (C1+C2)*KH*KW][Cout]  (K index = ci*KH*KW + kh*KW + kw);
 *           w_bstride != 0 selects per-sample weights (element stride) -- used for the all-pairs GEMM
 *   out   : written into channels [out_coff, out_coff+Cout) of a [B,out_ctotal,Ho,Wo] tensor
 *   value : act(alpha * conv + bias[co]) + res[b,co,oy,ox]      (bias, res nullable; res is [B,Cout,Ho,Wo]) */
int cf_conv2d(const float* x1, int C1, const float* x2, int C2, const float* wt, long w_bstride, const float* bias,
              const float* res, float* out, int out_ctotal, int out_coff, int B, int H, int W, int Cout, int KH,
              int KW, int stride, int pad_h, int pad_w, int act, float alpha, void* stream);

/* Same operator on the f16 MFMA with a 3-term hi/lo operand split (conv_f16s.hip): ~2^-22 relative operand error
 * (fp32-class accuracy, measured in DESIGN.md) at up to 5.3x the fp32-MFMA rate.  Supported: 3x3 pad 1 or 1x1 pad 0 at
 * stride 1 or 2, and the separable 1x5 pad (0,2) / 5x1 pad (2,0) convolutions of RAFT's SepConvGRU at stride 1; anything
 * else returns CF_ERR_ARG (the caller decides: cf_conv2d is the exact fp32 operator).  `wpk` = weights packed by the host
 * in MFMA fragment order as fp16 hi/lo planes and pre-scaled by 2^s (cineflow/ops.py pack_conv_weight_f16s);
 * pass alpha * 2^-s as `alpha`.  With a second input (C2 > 0) whose split C1 is not a multiple of the chunk size (16
 * channels for 3x3, 32 otherwise) the weights must be packed split-aware (pack_conv_weight_f16s(w, c1=C1): x1's channels
 * padded to whole chunks) -- the kernel switches input pointers at a chunk boundary.
 * Sizes: the kernel addresses its inputs with 32-bit offsets; ONE SAMPLE of x1 / x2 must stay below 2 GiB, a batch of any
 * size is cut into sub-batches inside the library (same kernel, same numbers).
 * Activation range: |x| < 65504 (fp16's range for the hi half).  Larger magnitudes, Inf and NaN are not clamped: they come
 * out as NaN, as loudly as in an fp32 convolution fed with NaN, and stay inside their own sample (the zero-weight channel tail of a chunk
 * is never fetched, so nothing of sample b + 1 reaches sample b).  cf_count_out_of_range is the debug check.  Below 2^-14 |x| the lo half goes subnormal (absolute error
 * 2^-25), which is under the fp32 rounding of the sum for the normalised activations this path is built for.
 * gn_ws (nullable, 2*B*gn_groups doubles): on return it holds the GroupNorm / InstanceNorm statistics (sum, sum of squares
 * per (sample, group)) of the OUTPUT, accumulated in the conv epilogue (or by a statistics pass when a workgroup spans
 * several samples); feed it to cf_group_norm_apply.  Requires a dense output (out_coff 0, out_ctotal == Cout).
 * A NEGATIVE gn_groups (= -groups) declares that gn_ws already holds zeros (slices of a pool the caller cleared with one
 * memset): the per-launch memset is skipped. */
int cf_conv2d_f16s(const float* x1, int C1, const float* x2, int C2, const void* wpk, const float* bias, const float* res,
                   float* out, int out_ctotal, int out_coff, int B, int H, int W, int Cout, int KH, int KW, int stride,
                   int pad_h, int pad_w, int act, float alpha, double* gn_ws, int gn_groups, void* stream);
/* Product mode of the f16-MFMA convolutions launched FROM THE CALLING THREAD afterwards (thread-local; returns the previous mode):
 * 3 (default) = hi/lo operand split, three MFMAs per k-step, f32-class results; 1 = hi x hi only, i.e. operands rounded to fp16 with fp32
 * accumulation -- what the reference's fp16 autocast gives the segmentation path under mixed_precision=True
 * (nnunet/network_architecture/neural_network.py:140-146; the flow path forces it off, SegFlowGaussian.py:2905-2909).  In mode 1 every
 * cf_conv2d_f16s* / cf_conv_transpose2d_k2s2_f16s call takes the one-tile kernel's hi x hi instantiation (a third of the MFMAs) and
 * cf_conv2d_wino_ok answers 0. */
int cf_conv_terms(int terms);
/* nn.Conv3d forward on the same f16 MFMA with the same 3-term split (csrc/conv3d_f16s.hip; generic_UNet.py with conv_op = nn.Conv3d): kernel
 * (KD, 3, 3) with KD in {1, 3}, padding (KD/2, 1, 1), stride (stride_d, stride_hw, stride_hw) with each in {1, 2}.  x1 [B,C1,D,H,W], the optional
 * x2 [B,C2,D,H,W] (cat[x1, x2] never materialised) and out [B,Cout,Do,Ho,Wo] are dense NCDHW, read and written in place; all KD * 9 taps of a
 * channel chunk accumulate in one kernel and the output is written once with alpha * acc + bias.  wpk from
 * cineflow.ops.pack_conv3d_weight_f16s (fragment order [m-tile][chunk of 16][dz][ky*3+kx][hi/lo][lane][8], scaled by 2^s: pass alpha * 2^-s;
 * split-aware when C2 > 0 and C1 % 16 != 0).  gn_ws / gn_groups as in cf_conv2d_f16s: fp64 {sum, sum of squares} per (sample, group) of the
 * output over (Do, Ho, Wo), from the epilogue or -- where a workgroup holds planes of several samples -- from a statistics pass; a negative
 * gn_groups declares gn_ws already zeroed.
 * Sizes: 32-bit offsets -- ONE SAMPLE of x1, x2 and out must each stay below 2 GiB; larger batches are cut into sub-batches inside the
 * library.  Activation range as cf_conv2d_f16s.  Only the three-term product is built.
 * cf_conv3d_f16s_ok (host code, no launch) returns 1 when the kernel takes the shape and 0 otherwise: a kernel other than (1|3, 3, 3), a
 * stride outside {1, 2}, a sample of some tensor at or above 2 GiB, a one-column map taller than the staging budget, cf_conv_terms(1), or
 * a shape class on which the caller's composition of 2-D convolutions was measured faster (no depth taps or in-plane-only stride 2 at
 * >= 65536 output voxels per sample; fewer than 512 workgroups with more than 24 (chunk, depth tap) steps: csrc/conv3d_f16s.hip);
 * cf_conv3d_f16s then fails with CF_ERR_ARG and the caller keeps its own route. */
int cf_conv3d_f16s(const float* x1, int C1, const float* x2, int C2, const void* wpk, const float* bias, float* out, int B, int D, int H,
                   int W, int Cout, int KD, int KH, int KW, int stride_d, int stride_hw, float alpha, double* gn_ws, int gn_groups,
                   void* stream);
int cf_conv3d_f16s_ok(int B, int C1, int C2, int D, int H, int W, int Cout, int KD, int KH, int stride_d, int stride_hw);
/* Strided (1, 1, 1) nn.Conv3d forward -- the skip projection of a residual block (conv_blocks.py:126-129) -- on the same f16 MFMA with the
 * same 3-term split (csrc/conv3d_pw_f16s.hip): out[b, co, zo, yo, xo] = alpha * sum_ci W[co][ci] * x[b, ci, zo*stride_d, yo*stride_hw,
 * xo*stride_hw] + bias[co], no padding, each stride in {1, 2}, Do = (D - 1) / stride_d + 1 and likewise Ho, Wo.  x [B,Cin,D,H,W] and out
 * [B,Cout,Do,Ho,Wo] are dense NCDHW, read and written in place: only the planes, rows and columns the strides select are addressed.  wpk
 * from cineflow.ops.pack_conv3d_pw_weight_f16s (the 1x1 fragment order of cf_conv2d_f16s: [m-tile][chunk of 32][k-step][hi/lo][lane][8],
 * scaled by 2^s: pass alpha * 2^-s); bias nullable.  gn_ws / gn_groups as in cf_conv3d_f16s: fp64 {sum, sum of squares} per (sample, group)
 * of the output, from the epilogue or -- where a workgroup holds several whole samples -- from a statistics pass; a negative gn_groups
 * declares gn_ws already zeroed.
 * Sizes: 32-bit offsets -- ONE SAMPLE of x and out must each stay below 2 GiB; larger batches are cut into sub-batches inside the library.
 * Activation range as cf_conv2d_f16s.  Only the three-term product is built.
 * cf_conv3d_pw_f16s_ok (host code, no launch) returns 1 when the kernel takes the shape and 0 otherwise: a stride outside {1, 2}, a sample of
 * x or out at or above 2 GiB, or cf_conv_terms(1); cf_conv3d_pw_f16s then fails with CF_ERR_ARG and the caller keeps its own route.  No
 * shape class is declined on measured time: the trainer-width projections (32 -> 64 at 128^3 down to 320 -> 320 at 8^3, strides (2,2,2)
 * and (1,2,2)) all measure faster than the caller's composition (profiles/resenc_pw3d.txt). */
int cf_conv3d_pw_f16s(const float* x, const void* wpk, const float* bias, float* out, int B, int Cin, int D, int H, int W, int Cout,
                      int stride_d, int stride_hw, float alpha, double* gn_ws, int gn_groups, void* stream);
int cf_conv3d_pw_f16s_ok(int B, int Cin, int D, int H, int W, int Cout, int stride_d, int stride_hw);
int cf_conv_transpose2d_k2s2_f16s(const float* x, const void* wpk, const float* bias, float* out, int out_ctotal,
                                  int out_coff, int B, int Cin, int H, int W, int Cout, float alpha, double* gn_ws, int gn_groups,
                                  void* stream);

/* nn.ConvTranspose2d(k=2, s=2) of PatchExpand2DGroup (lib/utils.py:1982-1994) and Generic_UNet.tu
 * (generic_UNet.py:343-345).  w is the torch layout [Cin][Cout][2][2] (no transposition needed); bias nullable.
 * out is written into channels [out_coff, out_coff+Cout) of a [B,out_ctotal,2H,2W] tensor. */
int cf_conv_transpose2d_k2s2(const float* x, const float* w, const float* bias, float* out, int out_ctotal,
                             int out_coff, int B, int Cin, int H, int W, int Cout, void* stream);

/* ---------------------------------------------------------------- normalisation
 * nn.GroupNorm(groups, C) / nn.InstanceNorm2d(C, affine) (groups == C) + activation + residual, two launches
 * (fp64 statistics, then apply).  ws: caller workspace of 2*B*groups doubles.  gamma/beta nullable (1 / 0).
 * out = act(gn(x) [+ res]) [+ res]  per res_mode.  In-place (out == x) allowed. */
int cf_group_norm(const float* x, const float* gamma, const float* beta, const float* res, float* out, int B, int C,
                  int HW, int groups, float eps, int act, int res_mode, double* ws, void* stream);

/* The apply pass of cf_group_norm alone; `ws` holds the statistics (from cf_conv2d_f16s' fused epilogue). */
int cf_group_norm_apply(const float* x, const float* gamma, const float* beta, const float* res, float* out, int B, int C,
                        int HW, int groups, float eps, int act, int res_mode, const double* ws, void* stream);
/* The statistics pass of cf_group_norm alone: ws[2 * (b * groups + g)] = {sum, sum of squares} of the slab, in fp64. */
int cf_group_norm_stats(const float* x, double* ws, int B, int C, int HW, int groups, void* stream);
/* The launch plan of the three calls above and of cf_group_norm_apply_res_norm, exported (host code, launches nothing, needs no GPU): the
 * launchers execute exactly this plan.  x, out, res: the pointers of the call (only their 16-byte alignment matters; out / res may be
 * NULL).  plan8 (nullable) receives {statistics kernel: 0 gn_stats_wave_kernel, 1 gn_stats_block_kernel; blocks per slab of the block
 * kernel, or 0; statistics grid; apply kernel: 0 gn_apply_small_kernel, 1 gn_apply_kernel; VEC; planes per block (small) or blocks per
 * plane (large); apply grid; planes of the last small block, or 0}.  Returns CF_OK, or CF_ERR_ARG for a shape the calls refuse. */
int cf_group_norm_route(const float* x, const float* out, const float* res, int B, int C, int HW, int groups, int* plan8);
/* The same apply pass when the residual is a raw convolution output that still awaits ITS OWN GroupNorm (the 1x1 conv + GroupNorm
 * `downsample` branch of DoubleConv, nnunet/lib/utils.py:1192-1195, :1208-1213): res is normalised on the fly with res_ws (its
 * {sum, sum of squares} pairs, same groups and eps) and res_gamma / res_beta, saving that branch's own apply pass. */
int cf_group_norm_apply_res_norm(const float* x, const float* gamma, const float* beta, const float* res, float* out, int B, int C,
                                 int HW, int groups, float eps, int act, int res_mode, const double* ws, const double* res_ws,
                                 const float* res_gamma, const float* res_beta, void* stream);
/* Deferred normalisation: instead of running the apply pass on a convolution output, hand its per-(sample, channel) coefficients to
 * the consuming convolution.  cf_group_norm_coef: ws ({sum, sum of squares} pairs) -> coef float [B][3][C] = {mean, rstd * gamma,
 * beta}.  cf_conv2d_f16s_prenorm: 3x3 / stride 1 / pad 1 convolution of lrelu((x - mean) * scale + shift, in_slope) (in_slope < 0:
 * GELU, for the second convolution of a DoubleConv, nnunet/lib/utils.py:1182-1215) -- the second
 * convolution of a Generic_UNet stage, nnunet/network_architecture/generic_UNet.py:79-144, consuming the first one's raw output --
 * dense output, optional fused statistics as in cf_conv2d_f16s.  Built for the vector-staging layer shapes only;
 * cf_conv2d_f16s_prenorm_ok(B, C, H, W, Cout) returns 1 when a shape qualifies (no launch), and the call fails otherwise. */
int cf_group_norm_coef(const double* ws, const float* gamma, const float* beta, int B, int C, int HW, int groups, float eps, float* coef,
                       void* stream);
/* Deferred normalisation into a 1x1 head: out[b][k][p] = bias[k] + sum_c w[k][c] * lrelu((x[b][c][p] - mean) * scale + shift, slope) with
 * coef from cf_group_norm_coef -- Generic_UNet's seg_outputs[-1] (a bias-free 1x1 convolution, generic_UNet.py:405-408) behind the last
 * decoder convolution's InstanceNorm + LeakyReLU, in one pass over that convolution's raw output.  K in {2, 4, 8}, HW % 4 == 0, fp32 FMAs
 * in channel order; w is the [K][C] weight, bias may be NULL. */
int cf_norm_head_1x1(const float* x, const float* coef, float slope, const float* w, const float* bias, float* out, int B, int C, int HW,
                     int K, void* stream);
/* Normalisations whose table is not made of statistics of the map, and the apply pass that takes a table (csrc/norm_coef.hip): what
 * nnU-Net's trainer variants need beside InstanceNorm + LeakyReLU(0.01).
 * cf_batch_norm_coef: BatchNorm in eval mode -> coef float [B][3][C] = {running_mean, gamma / sqrt(running_var + eps), beta}, the same
 * rows for every sample: layout and meaning of cf_group_norm_coef's output, so every consumer of that table takes this one.  gamma / beta
 * may be NULL (1 / 0).
 * cf_coef_apply: out = act((x - mean) * scale + shift) on x [B][C][HW] with mean / scale / shift from coef [B][3][C]; coef == NULL applies
 * the activation alone.  act is a CF_ACT_* code (CF_ACT_MISH included); CF_ACT_LRELU uses `slope` (>= 0) instead of the fixed 0.01 of the
 * fused epilogues, every other code ignores it.  out may be x.  x and out need 4-byte alignment only: rows are read and written in 16-byte
 * pieces between a scalar head and tail wherever x and out agree modulo 16, one value at a time otherwise; HW is arbitrary.  An NCDHW
 * tensor is passed as its [B][C][D*H*W] rows.  cf_coef_apply_ok (host code, no launch) returns 1 when the index arithmetic holds the
 * shape (HW <= 2^30, B * C * HW <= 2^40), and the call fails with CF_ERR_ARG otherwise. */
int cf_batch_norm_coef(const float* running_mean, const float* running_var, const float* gamma, const float* beta, float eps, int B, int C,
                       float* coef, void* stream);
int cf_coef_apply_ok(int B, int C, long HW);
int cf_coef_apply(const float* x, const float* coef, int act, float slope, float* out, int B, int C, int HW, void* stream);
/* Tuning / A-B knob without a reference counterpart: the short-K layers on large maps (3x3, stride 1, 32 or 64 output channels, >= 1024 tiles of
 * 16 / 8 rows x 32 pixels) run on a persistent software-pipelined kernel (csrc/conv_stream.hip) that sums the taps of a chunk in (kx, ky)
 * instead of (ky, kx) order: outputs equal the one-tile-per-workgroup kernel's to fp32 summation-order noise (<= 4e-6 of the output scale).
 * level 0 routes everything back to conv_f16s (also CF_CONV_STREAM=0), 1 (default) takes the shapes measured faster there (all but the
 * 64-channel layers with deferred input normalisation), 2 every shape the kernel can run.  Returns the previous level. */
int cf_conv_stream_enable(int on);
int cf_conv2d_f16s_prenorm_ok(int B, int C, int H, int W, int Cout);
int cf_conv2d_f16s_prenorm(const float* x, int C, const float* in_norm, float in_slope, const void* wpk, const float* bias, float* out,
                           int B, int H, int W, int Cout, float alpha, double* gn_ws, int gn_groups, void* stream);
/* The launch plan of the f16-split convolution, exported (host code, launches nothing, needs no GPU): what cf_conv2d_f16s (prenorm 0,
 * transposed 0), cf_conv2d_f16s_prenorm (prenorm 1; KH = KW = 3, stride 1, pad 1, C2 = 0) or cf_conv_transpose2d_k2s2_f16s (transposed 1:
 * C1 = Cin, Cout as passed there; KH, KW, stride >= 1 and the pads are ignored) does with a plain call -- dense output, no activation, no
 * residual -- of this shape in the calling thread's cf_conv_terms mode and at the current cf_conv_stream_enable level.  x1_low4 / x2_low4
 * are the low four bits of the input addresses (the vector staging forms need 16-byte alignment), stats_groups the gn_groups of the
 * call (0: no statistics).  prenorm 1 with another kernel, stride or C2 > 0 is planned as given -- no call can issue it, the plan declines it.
 * Returns the route: 0 = declined (cf_last_error holds the reason the call would fail with), 1 = conv_f16s_kernel,
 * 2 = conv_stream_kernel; CF_ERR_ARG for arguments no call accepts.  plan15 (nullable, 15 ints) receives
 *   [0] the route, [1..10] the instantiation <KH, KW, CK, WM, NTW, MAXT, NW, VEC, PRE, WL> (route 1, else zeros), [11] TERMS,
 *   [12] images per workgroup, [13] 1 when the epilogue accumulates the GroupNorm statistics (one sample per workgroup, or route 2;
 *   otherwise a statistics pass follows the convolution), [14] samples per launch: B, or ceil(B / parts) with the fewest parts whose
 *   inputs stay below 2 GiB -- the plan is that of such a part; ask with B = the last part's size for the route of the remainder. */
int cf_conv2d_f16s_route(int B, int C1, int C2, int H, int W, int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int x1_low4,
                         int x2_low4, int prenorm, int transposed, int stats_groups, int* plan15);

/* The same operator (nn.Conv2d 3x3 / stride 1 / padding 1 of DoubleConv, nnunet/lib/utils.py:1182-1215; ConvDropoutNormNonlin,
 * generic_UNet.py:26-69; ConvGRUCell's gate convolutions, convGRU.py:57-66) as a ROW Winograd F(2,3) on the f16 MFMA with the 3-term hi/lo
 * split (csrc/conv_wino.hip): the input transform (d0 - d2, d1 + d2, d2 - d1, d1 - d3) runs in fp32 before the split, the kernel transform
 * (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2) on the host in fp64 (cineflow/ops.py pack_conv_weight_wino -- `wpk` is NOT the
 * direct kernels' packing), 12 instead of 18 MFMA k-steps per pair of output columns; results equal cf_conv2d_f16s' to fp32 summation
 * noise (3-5e-7 of max|y| against fp64 at 128 / 256 channels).  Built for Cout in whole 128-channel blocks (or a last block >= 96: the
 * U-Net's 480), W % 16 == 0, H a multiple of the tile rows (4 / 8 at W >= 32, 8 / 16 at W = 16), 16-byte aligned inputs, one sample of
 * each tensor < 2 GiB; arguments as cf_conv2d_f16s (cat[x1, x2] packed split-aware when C1 % 16 != 0; alpha carries 2^-s; fused GroupNorm
 * statistics with gn_ws), the _prenorm form as cf_conv2d_f16s_prenorm.  cf_conv2d_wino_ok(B, C1, C2, H, W, Cout, prenorm) returns 1 when
 * a shape qualifies (no launch); the calls fail with CF_ERR_ARG otherwise (the caller stays on cf_conv2d_f16s).  CF_CONV_WINO=0 in the
 * environment makes cf_conv2d_wino_ok answer 0 for every shape (A/B knob). */
int cf_conv2d_wino_ok(int B, int C1, int C2, int H, int W, int Cout, int prenorm);
/* which kernel form the current route level sends the shape to (no launch): 0 = none, 2 / 4 = one tile per workgroup with 2 / 4 unit tiles
 * per wave, 8 = the persistent kernel.  Level 1 chooses between 8 and 2; the NTW 4 form runs only under the forced level 4. */
int cf_conv2d_wino_form(int B, int C1, int C2, int H, int W, int Cout, int prenorm);
/* MFMA shape of the kernel the current route level sends the shape to (no launch): 16 = the persistent kernel's v_mfma_f32_16x16x32_f16 form
 * (an even number of 16-channel chunks per item; level 16 forces it, level 1 takes it per class of launch where it was measured faster),
 * 32 = any other Winograd form, 0 = not a Winograd layer.  prenorm: 0 = none, 1 = deferred norm + LeakyReLU, 2 = deferred norm + GELU.
 * cf_conv2d_wino_form answers 8 for the persistent kernel under either shape. */
int cf_conv2d_wino_mfma(int B, int C1, int C2, int H, int W, int Cout, int prenorm);
/* route level (tests, A/B runs): 0 = off, 1 = automatic (default: the persistent wave-specialised kernel where a layer has at least two items per
 * CU, else one tile per workgroup with 2 unit tiles per wave), 2 / 4 = force the one-tile kernel with 2 / 4 unit tiles per wave, 8 = force the persistent kernel (32x32x16 MFMAs),
 * 16 = force the persistent kernel and its 16x16x32 MFMA form where that applies, level 1's routing otherwise -- each
 * where the geometry allows (initial value from CF_CONV_WINO).  Returns the previous level. */
int cf_conv_wino_enable(int level);
int cf_conv2d_wino(const float* x1, int C1, const float* x2, int C2, const void* wpk, const float* bias, const float* res, float* out,
                   int out_ctotal, int out_coff, int B, int H, int W, int Cout, int act, float alpha, double* gn_ws, int gn_groups,
                   void* stream);
int cf_conv2d_wino_prenorm(const float* x, int C, const float* in_norm, float in_slope, const void* wpk, const float* bias, float* out,
                           int B, int H, int W, int Cout, float alpha, double* gn_ws, int gn_groups, void* stream);

/* nn.LayerNorm(C) over the channel axis of channel-first tokens x [B,C,N] (lib/vit_transformer.py:1257,1261,1265);
 * the residual add is done by the preceding conv epilogue. */
int cf_layer_norm_cf(const float* x, const float* gamma, const float* beta, float* out, int B, int C, int N, float eps,
                     void* stream);

/* ---------------------------------------------------------------- attention
 * nn.MultiheadAttention core (need_weights path: q scaled by 1/sqrt(d) first), channel-first:
 * q [B,heads*d,Nq], k,v [B,heads*d,Nk] with element batch strides q_bs,k_bs,v_bs (so they may be channel slices
 * of a fused projection buffer); out [B,heads*d,Nq] contiguous.  d in {8,16,32,64}; Nq,Nk multiples of 32. */
int cf_attention_cf(const float* q, long q_bs, const float* k, long k_bs, const float* v, long v_bs, float* out, int B,
                    int heads, int d, int Nq, int Nk, void* stream);
/* cf_attention_cf for sequences whose length is not a multiple of 32: the caller zero-pads q / k / v to Nq, Nk (multiples of 32); only
 * the first nk_valid keys take part in the softmax (nk_valid in the last 32-key block); padded query rows of `out` are garbage.
 * The padded keys need only be finite, not zero: their weight is exactly 0, and the result is bit-identical whatever finite values they hold.
 * Range: the f16-split kernel (route 1 below) clamps q / sqrt(d), k and v to +-60000 before its f16 hi/lo split, so a finite value above the
 * f16 range saturates there instead of becoming Inf; the fp32 kernel (route 0) has the fp32 range. */
int cf_attention_cf_masked(const float* q, long q_bs, const float* k, long k_bs, const float* v, long v_bs, float* out, int B,
                           int heads, int d, int Nq, int Nk, int nk_valid, void* stream);
/* The kernel cf_attention_cf / cf_attention_cf_masked launch for this V pointer, batch stride, head dimension and key count (host code,
 * launches nothing, needs no GPU; the launcher dispatches on this very value): 0 = attention_cf_kernel<d>, fp32 MFMA (d == 8, or a V whose
 * 8-key groups are not 16-byte aligned: pointer, v_bs * 4 or Nk % 8), 1 = attention_cf_f16s_kernel<d>, f16 hi/lo split (d in {16, 32, 64},
 * aligned V), -1 with cf_last_error set for any other d. */
int cf_attention_cf_route(const float* v, long v_bs, int d, int Nk);

/* ---------------------------------------------------------------- ConvGRU gating (convGRU.py:60-68)
 * gates [B,2C,HW] = sigmoid(conv_gates(...)) with channels [0,C) = reset, [C,2C) = update. */
int cf_gru_reset_mul(const float* gates, const float* h, float* rh, int B, int C, int HW, void* stream);
int cf_gru_blend(const float* gates, const float* h, const float* cand, float* out, int B, int C, int HW, void* stream);

/* ---------------------------------------------------------------- small tensor plumbing kernels */
#define CF_OP_ADD 0
#define CF_OP_SUB 1
#define CF_OP_MUL 2
/* out[i] = a[i] op b[i % b_period]  (b_period = n for no broadcast) */
int cf_binary(int op, const float* a, const float* b, float* out, long n, long b_period, void* stream);
/* Debug aid for the f16-split convolutions (no reference counterpart: the reference's autocast has no range check either): *counter +=
 * number of elements of x[0..n) that are NaN / Inf or have |x| >= limit.  cineflow.ops runs it on every cf_conv2d_f16s* input when
 * CF_F16S_RANGE_CHECK=1 (limit 65504, the largest fp16 value) and reports through ops.f16s_range_violations(); inputs outside the range come
 * out of those kernels as NaN (see cf_conv2d_f16s).  The exact fp32 route for such data is cf_conv2d (cineflow.ops.set_conv_mode("f32")). */
int cf_count_out_of_range(const float* x, long n, float limit, unsigned long long* counter, void* stream);
/* dst[b, dst_coff + c, :] = act(src[b, src_coff + c, :])  for c < C : cat / split / activation of channel slices */
int cf_copy_channels(const float* src, int src_ctotal, int src_coff, float* dst, int dst_ctotal, int dst_coff, int B,
                     int C, int HW, int act, void* stream);
/* coords_grid (published RAFT; call site SegFlowGaussian.py:838-839): out [B,2,H,W], channel 0 = x, 1 = y */
int cf_coords_grid(float* out, int B, int H, int W, void* stream);
/* dst [N,h,w] = src [N,H,W][y0:y0+h, x0:x0+w]   (Processor.crop_data, processor.py:134-138) */
int cf_crop2d(const float* src, float* dst, int N, int H, int W, int y0, int x0, int h, int w, void* stream);
/* dst [N,H,W] = zero-pad of src [N,h,w] placed at (y0,x0)  (Processor.uncrop_no_registration, processor.py:178-186) */
int cf_pad2d(const float* src, float* dst, int N, int h, int w, int y0, int x0, int H, int W, void* stream);

/* ---------------------------------------------------------------- sliding-window / TTA (neural_network.py)
 * _internal_maybe_mirror_and_pred_2D :596-615, one term: acc += weight * flip(softmax_K(flip-input logits)).
 * logits [B,K,H,W] are the network output on the (possibly flipped) input; flips undo the mirroring. */
int cf_tta_accumulate(const float* logits, float* acc, int B, int K, int H, int W, int flip_h, int flip_w, float weight,
                      void* stream);
/* cf_tta_accumulate with a per-sample placement (MTL_model.py:905-936: flip-averaged softmax of the crops, then uncrop_no_registration's
 * F.pad): logits [B,K,crop,crop] of one flip variant, acc [B,K,H,W]; windows: DEVICE int32 [B,4] = cf_crop_windows' crop_indices, sample b
 * lands at rows windows[b][2].., columns windows[b][0]...  acc[b][:, window] += weight * flip(softmax_K(logits[b])); nothing outside the
 * window is read or written, so a zero-filled acc stays zero there (the pad).  Inside the window the value carries the bits of
 * cf_tta_accumulate into a [B,K,crop,crop] buffer followed by cf_pad2d (same softmax, same order of additions over successive calls).
 * A window that leaves the map is skipped. */
int cf_tta_accumulate_window(const float* logits, const int* windows, float* acc, int B, int K, int crop, int H, int W, int flip_h,
                             int flip_w, float weight, void* stream);
int cf_flip2d(const float* src, float* dst, int N, int H, int W, int flip_h, int flip_w, void* stream);
/* :711-731: agg[:, lx:lx+ph, ly:ly+pw] += pred * g ; cnt[...] += g   (g nullable = ones). pred [K,ph,pw]. */
int cf_tile_accumulate(const float* pred, const float* gauss, float* agg, float* cnt, int K, int X, int Y, int lx,
                       int ly, int ph, int pw, void* stream);
/* :741-744: probs = agg/cnt ; seg = argmax_K probs (first maximum).  seg uint8 [X,Y]. */
int cf_tile_finalize(const float* agg, const float* cnt, float* probs, uint8_t* seg, int K, int X, int Y, void* stream);
/* The cine-batched sliding window: _internal_predict_2D_2Dconv_tiled (neural_network.py:623-769) for every slice of every frame at once.
 * cf_tile_gather cuts the tiles (:705-710): dst[j] = src[n_j][:, lx_j:lx_j+ph, ly_j:ly_j+pw];  jobs: DEVICE int32 [J,3] = (n, lx, ly);
 * src [N,C,X,Y] -> dst [J,C,ph,pw].  A job whose window leaves the source reads nothing and gives zeros.  16-byte stores when pw % 4 == 0,
 * Y % 4 == 0 and both pointers are 16-byte aligned (16-byte loads for the jobs with ly % 4 == 0), a scalar path otherwise. */
int cf_tile_gather(const float* src, const int* jobs, float* dst, int J, int N, int C, int X, int Y, int ph, int pw, void* stream);
/* The aggregation of :711-744 for N slices at once, in gather form.
 * pred [N*nx*ny, K, ph, pw]: tile predictions that already carry the Gaussian weight, slice-major, then tile order (lx outer, ly inner);
 * lx[nx], ly[ny]: HOST arrays (the step lists of :267-290: rising from 0, no gap, last window ending at X / Y; nx, ny <= 16), passed to the
 * kernel by value;  gauss [ph,pw] nullable (= ones);
 * per output pixel, over the covering tiles IN TILE ORDER: agg = 0 + pred_1 + pred_2 + ..., cnt = 0 + g_1 + g_2 + ...;
 * probs [N,K,X,Y] = agg / cnt;  seg uint8 [N,X,Y] = first maximum over K.  No agg / cnt buffers, no atomics: for the same pred the result is
 * bit-identical to cf_tile_accumulate per tile + cf_tile_finalize per slice.  16-byte accesses when pw % 4 == 0, Y % 4 == 0, every
 * ly % 4 == 0 and the pointers are aligned, a scalar path otherwise. */
int cf_tile_merge(const float* pred, const float* gauss, float* probs, uint8_t* seg, int N, int K, int X, int Y, int ph, int pw,
                  const int* lx, int nx, const int* ly, int ny, void* stream);
/* 3-D twins: _internal_maybe_mirror_and_pred_3D (neural_network.py:506-571; logits/acc [B,K,D,H,W], the three flags undo
 * the mirroring of axes 2,3,4) and the tile aggregation of _internal_predict_3D_3Dconv_tiled (:381-398; pred [K,px,py,pz],
 * gauss [px,py,pz] nullable, agg/cnt [K,X,Y,Z]).  cf_tile_finalize serves 3-D volumes as (K, X, Y*Z). */
int cf_tta_accumulate_3d(const float* logits, float* acc, int B, int K, int D, int H, int W, int flip_d, int flip_h, int flip_w,
                         float weight, void* stream);
int cf_flip3d(const float* src, float* dst, int N, int D, int H, int W, int flip_d, int flip_h, int flip_w, void* stream);
int cf_tile_accumulate_3d(const float* pred, const float* gauss, float* agg, float* cnt, int K, int X, int Y, int Z, int lx, int ly,
                          int lz, int px, int py, int pz, void* stream);
/* argmax over K of [B,K,HW] -> uint8 [B,HW] */
int cf_argmax_channels(const float* x, uint8_t* out, int B, int K, int HW, void* stream);
/* Region-based heads (nnUNetTrainerV2BraTSRegions*: inference_apply_nonlin = nn.Sigmoid(), one channel per region).
 * cf_tta_accumulate[_3d] with the nonlinearity as an argument.  CF_NONLIN_SOFTMAX launches the kernel of cf_tta_accumulate[_3d] itself (the
 * same bits); CF_NONLIN_SIGMOID: acc[b,k,p] += weight * (1 / (1 + exp(-logits[b,k,flip(p)]))), every channel on its own, one thread per value
 * (per 4 values of a row with 16-byte accesses when W % 4 == 0, flip_w == 0 and both pointers are 16-byte aligned).  Logits of +-100 give
 * exactly 1 and 0.  Any other nonlin is CF_ERR_ARG. */
#define CF_NONLIN_SOFTMAX 0
#define CF_NONLIN_SIGMOID 1
int cf_tta_accumulate_nonlin(const float* logits, float* acc, int B, int K, int H, int W, int flip_h, int flip_w, float weight, int nonlin,
                             void* stream);
int cf_tta_accumulate_3d_nonlin(const float* logits, float* acc, int B, int K, int D, int H, int W, int flip_d, int flip_h, int flip_w,
                                float weight, int nonlin, void* stream);
/* The region label rule (neural_network.py:749-751, segmentation_export.py:148-150; cf_ensemble_merge applies the same): probs [B,K,HW]
 * fp32 -> seg uint8 [B,HW], label = 0, then for i = 0..K-1: label = order[i] where probs[b,i,p] > 0.5f, a later region overwriting an earlier
 * one.  order: HOST array of K label values (regions_class_order), passed to the kernel by value; 1 <= K <= 255. */
int cf_region_labels(const float* probs, uint8_t* seg, int B, int K, long HW, const uint8_t* order, void* stream);

/* ---------------------------------------------------------------- export post-processing
 * remove_all_but_the_largest_connected_component, nnunet/postprocessing/connected_components.py:51-107, on the device.
 * scipy.ndimage.label's default structure (face neighbours).  labels int32 [n]: 0 = outside the region, else 1 + the
 * smallest voxel index of the component once cf_cc_sweep has converged (*changed stays 0 after a sweep; the caller
 * zeroes it before each sweep and reads it back).  `classes`: HOST array of the 1..8 label values forming the region. */
int cf_cc_init(const uint8_t* image, int* labels, long n, const uint8_t* classes, int nclasses, void* stream);
int cf_cc_sweep(int* labels, int D, int H, int W, int* changed, void* stream);
/* counts int32 [n], zero-initialised by the caller: counts[l-1] += 1 for every voxel with label l */
int cf_cc_count(const int* labels, int* counts, long n, void* stream);
/* image[i] = 0 where the voxel's component size differs from max_count and (min_valid < 0 or size*volume_per_voxel < min_valid) */
int cf_cc_remove(uint8_t* image, const int* labels, const int* counts, long n, int max_count, double volume_per_voxel,
                 double min_valid, void* stream);

/* ---------------------------------------------------------------- determine_postprocessing (connected_components.py:123-447) on the device
 * Union-find labelling of EVERY region of a label map in one call, without a host round trip.  region_of: HOST table [256], label value ->
 * region id (0 = outside; region_of[0] must be 0).  Two face neighbours are connected iff their region ids are equal and non-zero:
 * region_of[c] = 1 for every class labels "all foreground as one object", region_of[c] = c labels every class on its own.
 * labels int32 [D*H*W]: 0 outside, else 1 + the smallest voxel index of the component (what converged cf_cc_sweep passes give). */
int cf_cc_label(const uint8_t* image, int* labels, int D, int H, int W, const uint8_t* region_of, void* stream);
/* counts int32 [n] (zeroed here): counts[l-1] = size of the component labelled l.  region_max int32 [256] (device): the largest size per
 * region id.  alive (device uint8 [n], optional, together with region_max_alive int32 [256]): the largest size among the components whose
 * voxels are alive (non-zero in `alive`); a component must be alive or dead as a whole. */
int cf_cc_sizes(const int* labels, const uint8_t* image, const uint8_t* region_of, const uint8_t* alive, long n, int* counts,
                int* region_max, int* region_max_alive, void* stream);
/* The what-if pass: out (device u64 [4][K][3]) = {TP, FP, FN} of every class c < K (labels >= K are scored nowhere; K <= 16) for the raw
 * prediction, the foreground-filtered one, the per-class-filtered raw one and the per-class-filtered one after the foreground filter;
 * no filtered image is written.  labels_fg / counts_fg / max_fg: cf_cc_label with region id 1 for every class + cf_cc_sizes;
 * labels_cls / counts_cls / max_cls / max_cls_alive: the same with region_of[c] = c (max_cls_alive restricted to what the foreground filter
 * keeps).  min_valid: HOST double [K] or NULL, [0] for the foreground region and [c] for class c, in cf_cc_remove's convention (< 0:
 * always remove; NULL: all -1).  z_skip: HOST int [K] or NULL: class c is scored on slices z >= z_skip[c] only. */
int cf_pp_confusion(const uint8_t* pred, const uint8_t* gt, int D, int H, int W, int K, const int* labels_fg, const int* counts_fg,
                    const int* max_fg, const int* labels_cls, const int* counts_cls, const int* max_cls, const int* max_cls_alive,
                    double volume_per_voxel, const double* min_valid, const int* z_skip, unsigned long long* out, void* stream);
/* dst = src with the foreground step applied (do_fg) and then the largest-component filter of every class whose bit is set in class_bits
 * (bit c for class c, 1 <= c < K), from the same label maps; max_cls is the per-class maximum of the image the class step sees (the alive
 * one after a foreground step).  src == dst is allowed. */
int cf_cc_apply(const uint8_t* src, uint8_t* dst, long n, int K, int do_fg, int class_bits, const int* labels_fg, const int* counts_fg,
                const int* max_fg, const int* labels_cls, const int* counts_cls, const int* max_cls, double volume_per_voxel,
                const double* min_valid, void* stream);

/* resample_data_or_seg, nnunet/preprocessing/preprocessing.py:111-200 (export path, orders 0 and 1): src [N,X,Y,Z] ->
 * dst [N,X2,Y2,Z2], sampling at src = (n/n2)*(dst+0.5)-0.5 with edge clamping (skimage resize mode='edge',
 * map_coordinates mode='nearest'); per axis linear (1) or nearest (0). */
int cf_resize3d(const float* src, float* dst, int N, int X, int Y, int Z, int X2, int Y2, int Z2, int linear_x, int linear_y,
                int linear_z, void* stream);
/* The export of one validated case in one launch (nnUNetTrainer.validate, nnunet/training/network_training/nnUNetTrainer.py:801-868, and
 * predict_next_stage, nnunet/training/cascade_stuff/predict_next_stage.py:31-87): src, device fp32 [K][X][Y][Z] (K in 1..255), is resampled
 * to (X2, Y2, Z2) exactly as cf_resize3d resamples each channel (the two kernels share the sampling function; equal sizes copy), and
 * seg, device uint8 [Xf][Yf][Zf], is written everywhere: the label of the crop at (x0, y0, z0), 0 outside (a crop that overhangs is
 * refused).  Label: the first maximum over the K resampled channels (numpy's argmax, NaN rule included), or with `order` (HOST array of K
 * label values, regions_class_order; may be NULL) 0 overwritten by order[k] where channel k > 0.5, in channel order.  probs_out (may be
 * NULL): device __half [K][X2][Y2][Z2], the resampled values rounded to nearest even; with `order`, a value > 0.5 that rounds to <= 0.5
 * is stored as the next fp16 above 0.5, so that stored > 0.5 exactly where the value is.  gt with hist (both or neither): gt device uint8
 * [Xf][Yf][Zf], hist device u64 [16 * 16 + 1] = what cf_label_confusion(seg, gt, ., 16, .) gives, overflow bin included; this call zeroes
 * hist on `stream` before the launch. */
int cf_resample_argmax(const float* src, int K, int X, int Y, int Z, int X2, int Y2, int Z2, int linear_x, int linear_y, int linear_z,
                       uint8_t* seg, int Xf, int Yf, int Zf, int x0, int y0, int z0, const uint8_t* order, void* probs_out, const uint8_t* gt,
                       unsigned long long* hist, void* stream);

/* Stem convolutions (nn.Conv2d with 1, 2 or 6 input channels, 3x3 pad 1 or 1x1, stride 1, e.g. Generic_UNet's first conv,
 * nnunet/network_architecture/generic_UNet.py:70-86, and the encoders' first DoubleConv, nnunet/lib/utils.py:1175-1210) as a direct
 * fp32 kernel: weight fp32 [Cout][Cin][K][K] (the checkpoint layout), out dense [B][Cout][H][W].  gn_ws (may be NULL): device fp64
 * [B][gn_groups][2] = {sum, sum of squares} of the output per (sample, group), zeroed here; gn_groups <= 64 divides Cout.  With a NULL
 * gn_ws no statistics are formed and gn_groups is not read.  Each output is one fmaf chain: the bias (or +0), then ci, ky, kx. */
int cf_conv2d_small_cin(const float* x, const float* weight, const float* bias, float* out, int B, int Cin, int H, int W, int Cout, int K,
                        double* gn_ws, int gn_groups, void* stream);
/* Head convolutions (nn.Conv2d, 3x3 pad 1 stride 1, 1..4 OUTPUT channels: the flow head `final_conv` of Decoder2D,
 * nnunet/lib/decoder_alt.py:890-892, and FlowHead.conv2 of the published RAFT update block) as a direct, exact fp32 kernel:
 * out = conv(x) + bias (+ res): weight fp32 [Cout][Cin][3][3] (checkpoint layout), x [B][Cin][H][W], res / out dense [B][Cout][H][W];
 * bias and res may be NULL. */
int cf_conv2d_small_cout(const float* x, const float* weight, const float* bias, const float* res, float* out, int B, int Cin, int H, int W,
                         int Cout, void* stream);
/* The same head directly behind a DoubleConv (nnunet/lib/utils.py:1182-1215) whose last apply pass is left out: the head's input
 * GELU((y2 - m2) * s2 + b2) + ((r - mr) * sr + br) is formed from the block's two raw maps while the tile is staged -- y2 = conv2's output
 * with coef2, r = the 1x1 downsample branch's output with coefr, both coefficient tables float [B][3][Cin] from cf_group_norm_coef.
 * out = conv(that) + bias, same summation order as cf_conv2d_small_cout.  cf_conv2d_small_cout_norm2_ok (host code, no launch) returns 1
 * when the kernel takes the shape (1..4 output channels, one input sample below 2 GiB); the call fails with CF_ERR_ARG otherwise. */
int cf_conv2d_small_cout_norm2_ok(int B, int Cin, int H, int W, int Cout);
int cf_conv2d_small_cout_norm2(const float* y2, const float* coef2, const float* r, const float* coefr, const float* weight, const float* bias,
                               float* out, int B, int Cin, int H, int W, int Cout, void* stream);
/* The stem DoubleConv of the flow encoders (nnunet/lib/utils.py:1182-1215 with a 1x1 downsample; Cin 1 or 6) in ONE launch over the
 * input: y = conv3x3(x; w3, b3) (pad 1) and r = conv1x1(x; w1, b1), both raw, dense [B][Cout][H][W], exact fp32 with the summation order
 * of cf_conv2d_small_cin, and the GroupNorm statistics of each ({sum, sum of squares} per (sample, group), fp64 [B][gn_groups][2]) in
 * ws_y / ws_r.  gn_groups <= 64 divides Cout; negative gn_groups declares both workspaces already zeroed, otherwise they are zeroed
 * here.  b3 / b1 may be NULL.  cf_stem_block_ok (host code, no launch) returns 1 when the kernel takes the shape, and the call fails
 * with CF_ERR_ARG otherwise. */
int cf_stem_block_ok(int B, int Cin, int H, int W, int Cout, int gn_groups);
int cf_stem_block(const float* x, const float* w3, const float* b3, const float* w1, const float* b1, float* y, float* r, int B, int Cin,
                  int H, int W, int Cout, double* ws_y, double* ws_r, int gn_groups, void* stream);
/* cf_stem_block without the store of r, for a block whose output is applied by cf_group_norm_apply_res_stem: the same kernel writes y
 * and ws_y and accumulates r's statistics into ws_r, but r itself is never written (its one consumer recomputes it from x).  y is bit
 * equal to cf_stem_block's; same shapes (cf_stem_block_ok), same zeroing rule for gn_groups. */
int cf_stem_block_y(const float* x, const float* w3, const float* b3, const float* w1, const float* b1, float* y, int B, int Cin, int H, int W,
                    int Cout, double* ws_y, double* ws_r, int gn_groups, void* stream);
/* The final apply pass of that block: out = act(GN(y2) [+ r']) [+ r'] as cf_group_norm_apply_res_norm forms it, with the raw residual
 * r = conv1x1(x; w1, b1) rebuilt per element from the block's input x [B][Cin][H][W] (w1 fp32 [C][Cin], b1 may be NULL) in cf_stem_block's
 * summation order, so that out is bit equal to cf_group_norm_apply_res_norm fed with the r cf_stem_block stores and the same workspaces.
 * ws / res_ws: the statistics of y2 / of r (fp64 [B][groups][2]); out may be y2.  cf_group_norm_apply_res_stem_ok (host code, no
 * launch) returns 1 when the kernel takes the shape: Cin 1 or 6, C <= 128, H * W >= 2048 and a multiple of 4; the call fails with
 * CF_ERR_ARG otherwise, and the caller keeps the stored-r pass. */
int cf_group_norm_apply_res_stem_ok(int B, int Cin, int C, int H, int W, int groups);
int cf_group_norm_apply_res_stem(const float* y2, const float* gamma, const float* beta, const double* ws, const float* x, const float* w1,
                                 const float* b1, const double* res_ws, const float* res_gamma, const float* res_beta, float* out, int B, int Cin,
                                 int C, int H, int W, int groups, float eps, int act, int res_mode, void* stream);

/* ---------------------------------------------------------------- test-time preprocessing (the step before the path)
 * create_nonzero_mask, nnunet/preprocessing/cropping.py:25-32: mask[v] = any_c data[c][v] != 0 (uint8 [V]). */
int cf_nonzero_mask(const float* data, int C, long V, uint8_t* mask, void* stream);
/* scipy.ndimage.binary_fill_holes of cropping.py:31 -- `labels` are the converged cf_cc_init/cf_cc_sweep labels of the BACKGROUND
 * (class value 0) of `mask`; background components without a voxel on the array border become 1.  touch: int32 [D*H*W] scratch.
 * ndim 3: all six faces are border; ndim 2 (D == 1): the four edges. */
int cf_fill_holes(uint8_t* mask, const int* labels, int* touch, int D, int H, int W, int ndim, void* stream);
/* get_bbox_from_mask, cropping.py:47-55: bbox (device int32 [6]) = {min z, max z, min y, max y, min x, max x} over mask != 0
 * (inclusive maxima; {INT_MAX, -1, ...} for an empty mask).  Synchronises the stream once for its initialisation copy. */
int cf_mask_bbox(const uint8_t* mask, int D, int H, int W, int* bbox, void* stream);
/* One axis of skimage.transform.resize(order=3, mode='edge', anti_aliasing=False) (= scipy.ndimage.zoom(order=3, mode='nearest',
 * grid_mode=True)) as used by resample_data_or_seg, preprocessing.py:111-200: src fp64 [outer][n][inner] -> dst [outer][m][inner]. */
int cf_spline3_resample_axis(const double* src, double* dst, long outer, int n, long inner, int m, void* stream);
/* resize's clip=True: range of every slab (c, s) of x fp64 [C][A][S][B] -> minmax fp64 [C*S][2]; then y (same layout, resampled
 * A and B) clipped to its slab's range (minmax may be NULL: no clipping) and rounded to fp32. */
int cf_slab_minmax_chunks(int C, int A, int S, long B);   /* k: `partial` of cf_slab_minmax is fp64 [C*S][k][2] scratch */
int cf_slab_minmax(const double* x, int C, int A, int S, long B, double* minmax, double* partial, void* stream);
int cf_slab_clip_to_f32(const double* y, float* out, int C, int A, int S, long B, const double* minmax, void* stream);
/* Intensity normalisation, preprocessing.py:274-320.  cf_masked_moments: out3 (device fp64) = {sum, sum of squares, count} over the
 * voxels with seg >= 0 (seg may be NULL: all) and, when use_range, lo < x < hi.  cf_normalize, in place:
 * x = ((clip ? clamp(x, lo, hi) : x) - sub) / div, then 0 where zero_outside and seg < 0. */
int cf_masked_moments(const float* x, const float* seg, long n, int use_range, float lo, float hi, double* out3, void* stream);
int cf_normalize(float* x, const float* seg, long n, int clip, float lo, float hi, float sub, float div, int zero_outside, void* stream);
/* preprocessing.py:251 `data[np.isnan(data)] = 0`, in place */
int cf_nan_to_zero(float* x, long n, void* stream);
/* dst[i] = value where src[i] >= thr (the per-label step of batchgenerators' resize_segmentation; the package's own label route is
 * cf_resize_labels, which decides on the reference's fp64 indicator instead of a resized fp32 one) */
int cf_assign_where_ge(float* dst, const float* src, long n, float thr, float value, void* stream);
/* cropping.py:128-135: seg [C][V] gets `label` where seg == 0 and mask [V] == 0 (a zero-filled seg yields the created one) */
int cf_seg_outside_mask(float* seg, const uint8_t* mask, int C, long V, float label, void* stream);
/* Previous-stage labels of a `3d_cascade_fullres` model as network input (nnunet/inference/predict.py:82-85): batchgenerators'
 * resize_segmentation(seg, (X2, Y2, Z2), order=1) and to_one_hot(., classes) in one pass.  seg: device uint8 [X][Y][Z], the previous
 * stage's label map, already transposed.  dst: device fp32, n_classes planes of X2*Y2*Z2 -- a pointer INTO the network-input tensor
 * [num_modalities + n_classes][X2][Y2][Z2] at channel num_modalities.  classes: HOST array, the label value of plane j
 * (n_classes <= 255).  Sampling as cf_resize3d (linear on every axis); a voxel gets the largest label whose resized indicator is
 * >= 0.5, else 0; plane j is 1.0f where that label is classes[j], else 0.0f.  Labels outside `classes` compete and get no plane.
 * The indicator is the reference's fp64 chain (scipy.ndimage.zoom, order 1), product by product and sum by sum, so an indicator
 * of exactly 0.5 falls on the reference's side (csrc/prev_stage.hip). */
int cf_prev_stage_onehot(const uint8_t* seg, int X, int Y, int Z, float* dst, int X2, int Y2, int Z2, const uint8_t* classes,
                         int n_classes, void* stream);
/* batchgenerators resize_segmentation(order=1) of N label maps, src [N][X][Y][Z] -> dst [N][X2][Y2][Z2] (device fp32, label values
 * of either sign): a voxel gets the largest label whose resized indicator is >= 0.5, else 0.  Per axis linear, or nearest
 * (linear_* = 0: the separate axis of resample_data_or_seg, order_z 0) as cf_resize3d; the same fp64 chain as cf_prev_stage_onehot. */
int cf_resize_labels(const float* src, float* dst, int N, int X, int Y, int Z, int X2, int Y2, int Z2, int linear_x, int linear_y,
                     int linear_z, void* stream);
/* Ensemble of saved softmax volumes (nnunet/inference/ensemble_predictions.py merge_files + the label step and bounding-box placement of
 * segmentation_export.py) in one launch.  members: HOST array of n_members (1..16) device pointers, each [K][Z][Y][X] of __half (dtype 0)
 * or float (dtype 1).  seg: device uint8 [Zf][Yf][Xf], written everywhere: the labels of the crop at (z0, y0, x0), 0 outside (a crop that
 * overhangs the volume is refused).  mean: device [K][Z][Y][X] in the members' dtype, or NULL.  order: HOST array of K label values
 * (regions_class_order), or NULL.  Bit for bit numpy's np.mean(np.vstack(...), 0): fp32 sum in member order, one true fp32 division by
 * n_members, rounded to fp16 for __half members; label = first maximum over K of the rounded mean, or with `order` the last i with
 * mean[i] > 0.5 mapped through order[i], else 0 (csrc/ensemble.hip). */
int cf_ensemble_merge(const void* const* members, int n_members, int dtype, int K, int Z, int Y, int X, uint8_t* seg, int Zf, int Yf, int Xf,
                      int z0, int y0, int x0, void* mean, const uint8_t* order, void* stream);
/* Every two-member ensemble of n_members (2..8) saved softmax volumes against one ground truth, in one launch (model selection:
 * nnunet/evaluation/model_selection/ensemble.py merge + aggregate_scores' confusion counts).  members, dtype, K, the crop and `order` as in
 * cf_ensemble_merge.  pairs: HOST array of n_pairs (1..28) index pairs (i, j), i != j, both below n_members.  gt: device uint8
 * [Zf][Yf][Xf].  seg: device uint8 [n_pairs][Zf][Yf][Xf], written everywhere: seg[p] is what cf_ensemble_merge writes for the members
 * (i, j) of pair p.  hist: device u64 [n_pairs][16 * 16 + 1]: hist[p] is what cf_label_confusion(seg[p], gt, ., 16, .) gives, the
 * overflow bin for voxels with a label >= 16 included.  This call zeroes hist (on `stream`, before the launch); the caller need not.
 * Each member value is loaded once per class and serves every pair that holds it (csrc/ensemble.hip). */
int cf_ensemble_pairs(const void* const* members, int n_members, int dtype, int K, int Z, int Y, int X, const int* pairs, int n_pairs,
                      const uint8_t* gt, uint8_t* seg, int Zf, int Yf, int Xf, int z0, int y0, int x0, const uint8_t* order,
                      unsigned long long* hist, void* stream);

/* ---------------------------------------------------------------- downstream metrics (consumers of the output layout)
 * ConfusionMatrix.compute, nnunet/evaluation/metrics.py:65-82: counts3 (device u64 [3]) = {TP, FP, FN} of test != 0 vs
 * reference != 0 over n voxels (TN = n - TP - FP - FN). */
int cf_confusion_counts(const uint8_t* test, const uint8_t* reference, long n, unsigned long long* counts3, void* stream);
/* all classes of nnunet/compute_metrics.py:96-106 in one pass: hist (device u64 [K*K + 1]), hist[t*K + r] = #voxels with test label t
 * and reference label r; hist[K*K] counts voxels with a label >= K.  K <= 16. */
int cf_label_confusion(const uint8_t* test, const uint8_t* reference, long n, int K, unsigned long long* hist, void* stream);
/* medpy.metric.binary.__surface_distances (behind metrics.py:323-392): border voxels of mask [D,H,W] (mask ^ binary_erosion(mask,
 * generate_binary_structure(ndim, 1))) compacted as int32 (z, y, x) triples into coords (capacity 3*D*H*W); *count (device int32)
 * receives their number.  Then dist[i] = min_j ||spacing * (a[i] - b[j])|| in fp64 (= distance_transform_edt(~border_b, sampling)
 * read at border_a), and {max, sum} of a non-negative fp64 array -> out2. */
int cf_surface_border(const uint8_t* mask, int D, int H, int W, int ndim, int* coords, int* count, void* stream);
int cf_surface_min_dist(const int* a, int na, const int* b, int nb, double sz, double sy, double sx, double* dist, void* stream);
int cf_max_sum_nonneg(const double* x, long n, double* out2, void* stream);
/* nnunet/compute_jacobian.py:160-186: per label k < K (<= 16) of `labels`, stats (device fp64 [3*K]) = {sum x, count, #(x < 0)} */
int cf_region_stats(const double* x, const uint8_t* labels, long n, int K, double* stats, void* stream);
/* kornia.filters.spatial_gradient3d(mode='diff', order=1) of compute_jacobian.py:146: x [N][D][H][W] -> out [N][3][D][H][W]
 * (component 0 along W, 1 along H, 2 along D), replicate-padded central differences times 0.5; and the sums of |x| per slab
 * (c, s) of x [C][A][S][B] -> sums fp64 [C*S] behind the per-frame means of :147-159. */
int cf_spatial_gradient3d(const float* x, float* out, long N, int D, int H, int W, void* stream);
int cf_slab_abs_sum(const float* x, int C, int A, int S, long B, double* sums, void* stream);
/* skimage.metrics.structural_similarity as nnunet/compute_SSIM.py:91 calls it (2-D, uniform win x win window, sample covariance):
 * S (fp64 [H][W]) = SSIM of every pixel from the five local means with scipy's 'reflect' boundary; C1 = (K1 R)^2, C2 = (K2 R)^2,
 * cov_norm = NP / (NP - 1).  The mean over the interior (cf_region_stats on the cropped map) is the score. */
int cf_ssim_map(const double* im1, const double* im2, int H, int W, int win, double C1, double C2, double cov_norm, double* S, void* stream);

/* ---------------------------------------------------------------- cine tables: one device visit per patient (csrc/score.hip)
 * nnunet/compute_metrics.py:96-106 for all frames and classes of a patient.  test / reference: uint8 label stacks [N][D][H][W]
 * (N <= 65535 frames, N D H W < 2^30), K in 2..16 labels, ndim 3, or 2 with D == 1 (no z-face rule, as cf_surface_border).  For every
 * frame n and class 1 <= c < K the masks are `label == c`; a border voxel has a face neighbour that is not c or lies outside the frame's
 * own volume (frames never see each other).  Everything is caller-owned:
 *   ws      int32 [11 N K + 3]:  counts [N K 5] | bad [1] | offs [2 N K + 1] | blk [2 N K + 1] | cursors [2 N K]
 *   table   fp64  [N K 9 + 1]:   per (n, c) {TP, FP, FN, border voxels of test, of reference, max test->ref, max ref->test,
 *                                sum test->ref, sum ref->test}; the last element counts the voxels whose label is >= K
 * cf_label_surface_count classifies every voxel once, scans the 2 N K border counts on the device and fills the table's count columns.
 * Segment s = (n K + c) 2 + side (0: test border, 1: reference border) owns the points offs[s] .. offs[s + 1]; blk is the same scan over
 * the distance workgroups (256 points of a segment each; none where either side of the pair is empty).  The caller reads offs / blk once,
 * allocates coords int32 [3 total] and dist fp64 [total] for total = offs[2 N K], and calls cf_label_surface_table with nblocks =
 * blk[2 N K]: a fill pass compacts the border coordinates (z, y, x), one distance launch writes dist[p] = min_q || spacing (p - q) ||
 * over the partner segment (fp64, squares summed z, y, x as cf_surface_min_dist) and reduces maxima and sums into the table.  The order
 * of the points inside a segment follows the compaction; the distance search is brute force (cine-sized objects). */
int cf_label_surface_count(const uint8_t* test, const uint8_t* reference, int N, int D, int H, int W, int ndim, int K, int* ws, double* table,
                           void* stream);
int cf_label_surface_table(const uint8_t* test, const uint8_t* reference, int N, int D, int H, int W, int ndim, int K, double sz, double sy, double sx,
                           int* ws, int total, int nblocks, int* coords, double* dist, double* table, void* stream);
/* nnunet/compute_jacobian.py:141-198 for a whole cine.  flow fp32 [T][D][2][H][W] (component 0 along H), labels uint8 [T][D][H][W],
 * K <= 16, H, W >= 2, T D <= 65535.  table fp64 [T][D][5 + 3 K]: {sum |d/dt|, sum (|d/dy| + |d/dx|)} over both components with
 * kornia's replicate-padded 0.5 (x[+1] - x[-1]) in fp32, then {sum J, count, #(J < 0)} per label k < K and for the whole slice, J the
 * determinant of cf_jacobian_det_2d.  part: fp64 workspace [T D ceil(H / 32) ceil(W / 64) (5 + 3 K)] of per-tile totals, added in tile
 * order by a second launch, so the table has the same bits on every run.  Labels >= K count for the whole slice only. */
int cf_flow_regularity_table(const float* flow, const uint8_t* labels, int T, int D, int H, int W, int K, double* part, double* table, void* stream);
/* nnunet/compute_SSIM.py and compute_SSIM_crop_per_structure.py for a whole cine: cf_ssim_map's S of every frame against the ED frame,
 * summed, without storing a map.  fixed fp64 [D][H][W] (the ED image), registered fp32 [T][D][H][W] (every other frame warped onto ED),
 * labels uint8 [D][H][W] (the ED segmentation; NULL with K = 0).  win odd, 3 <= win <= 15, win <= min(H, W); K <= 16; T D <= 65535.
 * table fp64 [T][D][2 + 2 K]: {sum S, count} over the interior [pad, H - pad) x [pad, W - pad), pad = (win - 1) / 2, then {sum S, count}
 * over ALL pixels of the slice with labels == k for each k < K (S with scipy's 'reflect' boundary there, as cf_ssim_map; labels >= K count
 * nowhere).  Per slice data_range R = (double)(max - min) of the registered slice, subtracted in fp32; C1 = (K1 R)^2, C2 = (K2 R)^2 in
 * fp64.  range: fp32 workspace [T][D][2] (min, max); part: fp64 workspace [T D ceil(H / 32) ceil(W / 64) (2 + 2 K)] of per-tile totals,
 * added in tile order, so the table has the same bits on every run.  Three launches, no allocation, no synchronisation.  NaN propagates:
 * a slice where both images are constant zero has R = 0, S = 0 / 0 and NaN sums, as numpy's. */
int cf_cine_ssim_table(const double* fixed, const float* registered, const uint8_t* labels, int T, int D, int H, int W, int K, int win,
                       double K1, double K2, double cov_norm, float* range, double* part, double* table, void* stream);
/* nnunet/compute_contour_metrics.py for a whole patient (csrc/contour.hip).  flow fp32 [D][T][2][A][B]: the flows of every slice in
 * ED-first frame order (cineflow.strain.prepare_flow; frame 0 is the ED placeholder and is never read), component 0 along B.  pts fp32
 * [D][T][Pmax][2]: the 0-based ground-truth points (x along B, y along A) in the same frame order, each slice's endo, epi and RV points
 * one after the other, padded to Pmax.  counts int [D][3] = the numbers of endo, epi and RV points per slice, TWICE: `counts` in HOST
 * memory, which the argument checks read (non-negative, sum <= Pmax), and `counts_dev` the same numbers in device memory for the kernels
 * (they clamp what they read to Pmax).  mode:
 *   0 from_ed               pos[d][t-1][p] = pts[d][0][p] + flow[d][t](pts[d][0][p]);  error against pts[d][t][p]
 *   1 from_ed_accumulation  one chain per point from pts[d][0][p] through flows 1 .. t, pos[d][t-1] the position after flow t;  error
 *                           against pts[d][t][p]
 *   2 to_ed_accumulation    one chain per (frame t, point) from pts[d][t][p] through flows t, t-1 .. 1, pos[d][t-1][p] = end - start;
 *                           error against pts[d][0][p] - pts[d][t][p]
 *   3 to_ed                 pos[d][t-1][p] = flow[d][t](pts[d][t][p]);  error against pts[d][0][p] - pts[d][t][p]
 * A sample is cf_sample_points_2d's on both components (zeros outside the map), a chain step one rounded fp32 add: pos fp32
 * [D][T-1][Pmax][2] holds the bits of chained cf_sample_points_2d calls (padding points: 0).  table fp64 [D][T-1][3]: the mean over the
 * endo, epi and RV points of the Euclidean norm of (ground truth - pos), fp64 from the fp32 values; NaN for a structure without points.
 * T >= 2, A, B >= 2, D <= 65535.  Two launches, no allocation, no atomics: the same bits on every run. */
int cf_contour_track_table(const float* flow, const float* pts, const int* counts, const int* counts_dev, int D, int T, int A, int B, int Pmax,
                           int mode, float* pos, double* table, void* stream);
/* nnunet/get_strain.py:531-599 for all slices.  pos: the mode-0 positions of cf_contour_track_table, [D][T-1][Pmax][2]; ed_pts: the ED
 * points, slice d at ed_pts + d * ed_stride floats (the pts array itself with ed_stride = 2 T Pmax); counts / counts_dev as above, with
 * counts[d][0] == counts[d][1] (endo point p pairs with epi point p) or the call is refused.  table fp64 [D][T][2], row 0 the ED frame:
 * {radial, circumferential} Green-Lagrange strain 0.5 (L^2 - L0^2) / L0^2 in fp64 on (double)pixel * zoom (zoom_x for component 0),
 * averaged over the points -- L the endo-epi distance of a point, and the distance from a point to the next one along its closed
 * contour averaged over the two contours.  Rows are in the ED-first frame order; L0 = 0 gives NaN as in the script. */
int cf_contour_strain_table(const float* pos, const float* ed_pts, long ed_stride, const int* counts, const int* counts_dev, int D, int T, int Pmax,
                            double zoom_x, double zoom_y, double* table, void* stream);

/* ---------------------------------------------------------------- exact distance transform and the evaluator's visit (csrc/edt.hip)
 * scipy.ndimage.distance_transform_edt(mask, sampling = (sz, sy, sx)): out fp64 [D][H][W], every voxel's distance to the nearest voxel
 * whose mask value is 0, defined as the minimum over those voxels of sqrt(fl(fl(fl((sz dz)^2) + fl((sy dy)^2)) + fl((sx dx)^2))) --
 * cf_surface_min_dist's expression and order.  ndim 3, or 2 with D == 1; every extent <= 65534; 64-bit voxel indices.  Three separable
 * passes that carry the nearest zero's integer offsets: O(N max(D, H, W)) at the worst, never a search over pairs.
 * ws: cf_edt_workspace_bytes(D, H, W) bytes, 16-byte aligned, caller-owned (about 7 bytes per voxel: border flags 1, x offsets 2,
 * (x, y) offsets 4, plus 8 bytes per 256 voxels and a 4 KiB header; cf_edt itself uses the last two arrays).  The query is host code and
 * returns CF_ERR_ARG for a shape the calls refuse.
 * Nothing synchronises, so a mask WITHOUT any zero voxel is reported on the device: the int at byte 24 of ws is 1 afterwards (0
 * otherwise) and such voxels hold +inf; the caller that wants the error reads that word (cineflow.metrics.distance_transform_edt does). */
long cf_edt_workspace_bytes(int D, int H, int W);
int cf_edt(const uint8_t* mask, int D, int H, int W, int ndim, double sz, double sy, double sx, void* ws, double* out, void* stream);
/* medpy's surface distances of `test == c` vs `reference == c` for K <= 16 listed label values c (host array `labels`), one label after
 * another in one workspace (D H W < 2^31).  Border voxels by cf_surface_border's rule; for each border voxel the distance to the
 * nearest border voxel of the OTHER volume, read from the transform of that border set -- confined to the joint bounding box of the
 * label's two border sets, outside of which nothing is computed -- and only at the voxels where it is read.
 *   dist  fp64 [capacity]: per label the test->ref distances, then the ref->test ones, each in raster (z, y, x) order of the voxels they
 *         belong to.  Compaction is a prefix scan over 256-voxel blocks: no atomics, the same order and the same sums on every run.
 *         The total never exceeds 2 D H W (a voxel carries one label per volume).
 *   head  fp64 [2 K + 1 + 8 K + 1]: offsets [2 K + 1] (segment 2 k = test->ref of label k, 2 k + 1 = ref->test; segment s is
 *         dist[offsets[s] .. offsets[s + 1])), then per label {count test->ref, count ref->test, max test->ref, max ref->test,
 *         sum test->ref, sum ref->test, border voxels of test, border voxels of reference}, then 1.0 if some label did not fit capacity.
 * A label without border voxels in either volume, or -- unless score_full -- filling either volume, or not fitting, gets two empty
 * segments (counts 0); no launch touches memory for it beyond the flag pass. */
int cf_label_surface_edt(const uint8_t* test, const uint8_t* reference, int D, int H, int W, int ndim, const int* labels, int K, double sz, double sy,
                         double sx, int score_full, void* ws, double* dist, long capacity, double* head, void* stream);

/* SwinCrossAttention (nnunet/lib/swin_cross_attention.py:13-112) after the projections: qk [B][2C][H][W] = the q and k maps of the
 * "rescaler" input, v [B][C][H][W] the value map of the "rescaled" input, bias_table [(2w-1)^2][heads] the learned relative position
 * bias; out [B][C][H][W] = softmax(q k^T / sqrt(C/heads) + bias + shift mask) v per window of w x w tokens (w <= 8 dividing H and W),
 * windows taken on the map cyclically shifted by `shift` and written back un-shifted. */
int cf_window_attention(const float* qk, const float* v, const float* bias_table, float* out, int B, int C, int H, int W, int heads,
                        int window, int shift, void* stream);

/* Processor.get_mean_centroid's masks_to_boxes (training/network_training/processor.py:140-160): per frame n of x [N][H][W]
 * (uint8, or float32 when is_float) boxes[n] = {x1, y1, x2, y2} of the non-zero pixels, or {-1,-1,-1,-1} for an all-zero frame. */
int cf_frame_boxes(const void* x, int is_float, int* boxes, int N, int H, int W, void* stream);
/* Processor.get_mean_centroid for one frame + Processor.adjust_cropping_window (processor.py:140-160, :109-132) per sample, integer for
 * integer, nothing read back: labels uint8 [N][H][W]; the centre of the non-zero labels' box is (x1 + (x2 - x1) / 2, y1 + (y2 - y1) / 2)
 * truncated, an all-zero map takes (H / 2, W / 2) in that order; the window of `crop` (even) pixels around it is clamped into
 * [0, image), crop <= image <= H, W.  Two DEVICE outputs: windows int32 [N][4] = {x_low, x_high, y_low, y_high} (crop_indices; x is the
 * column) and jobs int32 [N][3] = {n, y_low, x_low}, the job table cf_tile_gather takes (rows first), so the gather cuts the crops. */
int cf_crop_windows(const uint8_t* labels, int* windows, int* jobs, int N, int H, int W, int crop, int image, void* stream);
/* SpatialTransformerContour.forward(new_locs, original) (network_architecture/integration.py:5-34) as get_strain.py calls it:
 * out[b,c,p] = bilinear sample (align_corners, zeros outside) of field [B][C][H][W] at the contour point (pts[b,0,p], pts[b,1,p]) --
 * channel 0 is normalised by W - 1 and used as grid x, channel 1 by H - 1 as grid y (the reference's shape[~i]). */
int cf_sample_points_2d(const float* field, const float* pts, float* out, int B, int C, int H, int W, int P, void* stream);

/* ---------------------------------------------------------------- voxels by rank among the matching voxels (csrc/dataset.hip)
 * The training-side preprocessing drivers pick voxels by their C-order rank among the voxels that match a predicate:
 * np.argwhere(seg == c)[idx] (class locations, nnunet/preprocessing/preprocessing.py:387-470) and modality[seg > 0][::10] (foreground
 * samples, nnunet/experiment_planning/DatasetAnalyzer.py).  key: device fp32 [n] in C order, 0 <= n < 2^31, cut into scan blocks of 256
 * voxels; cf_select_blocks(n) = their number nb (host arithmetic).
 * cf_select_count, mode 0: `values` is a HOST array of n_values (1..16) floats; row r counts the voxels with key == values[r].  mode 1:
 * one row, the voxels with key > 0 (values and n_values are not read).  prefix: device int32 [rows][nb], on return the EXCLUSIVE prefix
 * over the blocks of every row's per-block counts; totals: device int64 [rows], the rows' sums -- the only numbers a caller reads back
 * (its random generator needs them).  Two launches (count, one-workgroup scan per row), no atomics.
 * cf_select_rank: `prefix` is ONE row of cf_select_count's result for the same key and predicate (mode, and `value` in mode 0).  ranks:
 * device int64 [K], any order, duplicates allowed, each 0 <= rank < that row's total.  One wave per rank: binary search for the block, then
 * 64-bit ballots and population counts inside it.  Either src (device fp32 [n]) + vals (device fp32 [K]): vals[k] = src at the voxel --
 * src[key > 0][ranks] -- or coords (device int64 [K][3]) with the key's shape D0 x D1 x D2 (D0 D1 D2 == n): the voxel's index triple --
 * np.argwhere(key == value)[ranks].  Exactly one of src / coords is non-NULL.  K == 0 launches nothing.  A rank outside the contract
 * writes -1s / 0 to its own slot and touches nothing else. */
int cf_select_blocks(long n);
int cf_select_count(const float* key, long n, const float* values, int n_values, int mode, int* prefix, long long* totals, void* stream);
int cf_select_rank(const float* key, long n, int mode, float value, const int* prefix, const long long* ranks, int K, const float* src,
                   float* vals, long long* coords, int D0, int D1, int D2, void* stream);

/* ---------------------------------------------------------------- DEFLATE and CRC-32 of a device buffer (csrc/deflate.hip)
 * cf_deflate writes the RFC 1951 blocks of src[0..n) (device bytes of any dtype) to out: the input is cut into chunks of
 * cf_deflate_chunk_bytes() = 32768 bytes, every chunk is compressed on its own (matches of 4..258 bytes at distances inside the chunk,
 * dynamic Huffman codes; a stored block when that is not smaller) and ends on a byte boundary as NON-final blocks, the chunks' streams
 * stand back to back.  There is no final block: the caller appends the two bytes 03 00 (an empty final fixed-Huffman block) and has a
 * complete raw-deflate stream that zlib, zipfile and gzip readers inflate.  *out_bytes_dev (device int64) = the stream's length, at most
 * cf_deflate_bound(n) = n + 5 ceil(n / chunk) -- out_cap must be at least that, and nothing past it is written.  n == 0 writes nothing
 * and sets the length to 0.  ws: cf_deflate_workspace_bytes(n) bytes, 16-byte aligned, caller-owned (per-chunk output slots, 128 KiB of
 * match state for each of at most 512 workgroups, the slot sizes and offsets).  Three launches on the caller's stream, no allocation,
 * no synchronisation.  The same input gives the same bytes on every run, whatever ws and out held before.
 * cf_crc32: *crc_dev (device uint32) = zlib's crc32 of src[0..n) (0 for n == 0).  ws: cf_crc32_workspace_bytes(n) bytes (4 per 256 KiB of
 * input plus 256), 4-byte aligned.  Two launches.
 * The three size queries are host arithmetic and return CF_ERR_ARG for a negative n.  Null pointers, a negative n, a short out_cap or
 * workspace and a misaligned workspace are refused on the host before any launch. */
int cf_deflate_chunk_bytes(void);
long cf_deflate_bound(long n);
long cf_deflate_workspace_bytes(long n);
int cf_deflate(const void* src, long n, void* out, long out_cap, void* ws, long ws_bytes, long long* out_bytes_dev, void* stream);
/* cf_huffman_code_lengths -- a TEST HOOK, not part of what callers need: the code lengths cf_deflate gives a histogram -- freq device uint32 [n], 2 <= n <= 286, lens device uint8 [n]:
 * Huffman lengths when none exceeds max_bits (1..15, 2^max_bits >= n), else folded to max_bits and repaired to a complete code with the
 * heaviest symbols on the shortest codes; weight 0 gives length 0, and fewer than two used symbols are made two.  One small launch. */
int cf_huffman_code_lengths(const unsigned* freq, int n, int max_bits, unsigned char* lens, void* stream);
long cf_crc32_workspace_bytes(long n);
int cf_crc32(const void* src, long n, void* ws, long ws_bytes, unsigned* crc_dev, void* stream);

/* ---------------------------------------------------------------- training: nnUNetTrainerV2_noDataAugmentation on the 2-D Generic_UNet
 * The backward of cf_conv2d, of InstanceNorm + LeakyReLU, the deep-supervision DC + CE loss (loss_functions/dice_loss.py:201-237,436-497,
 * deep_supervision.py), clip_grad_norm_ and torch.optim.SGD(nesterov) (nnUNetTrainerV2.py:231-279).  No floating-point atomics and no
 * workgroup that waits on another: every cross-workgroup sum is a second launch adding partials in a fixed order, so the same inputs give
 * the same bits on every call.
 *
 * cf_conv2d_wgrad: dw[(C1+C2)*KH*KW][Cout] (the layout cf_conv2d reads) and, when db is not null, db[Cout], from the layer input cat[x1, x2]
 * [B,C1|C2,H,W] and dy [B,Cout,Ho,Wo].  Kernels 3x3 pad 1 and 1x1 pad 0, stride 1 or 2.  Exact fp32 products on v_mfma_f32_32x32x2_f32; the
 * pixel axis is cut into cf_conv2d_wgrad_splits(...) chunks (a function of the shape alone; > 0, or CF_ERR_ARG), one partial tile each in
 * ws, added in split order in fp64.  ws: 8-byte aligned, at least round8(splits * Cin*KH*KW * Cout * 4) + splits * Cout * 8 bytes.
 * cf_conv2d_dgrad: the adjoint of the same convolution in gather form (no zero-stuffed map at stride 2), for the input channels
 * [ci_off, ci_off + Cn) of the layer's Cin, written to channels [dx_coff, dx_coff + Cn) of dx [B,dx_ctotal,H,W]; accumulate != 0 adds to
 * what dx holds (a skip map's second gradient). */
int cf_conv2d_wgrad_splits(int Cin, int Cout, int KH, int KW, int B, int Ho, int Wo);
int cf_conv2d_wgrad(const float* x1, int C1, const float* x2, int C2, const float* dy, float* dw, float* db, void* ws, long ws_bytes, int B,
                    int H, int W, int Cout, int KH, int KW, int stride, void* stream);
int cf_conv2d_dgrad(const float* dy, const float* wt, float* dx, int dx_ctotal, int dx_coff, int ci_off, int Cn, int Cin, int B, int H, int W,
                    int Cout, int KH, int KW, int stride, int accumulate, void* stream);
/* cf_norm_act_bwd: y = leaky(gamma * xhat + beta, slope) per (b, c) plane of the raw map x [B,C,HW], ws = cf_group_norm_stats' {sum, sum of
 * squares} with groups == C.  dy = dL/dy -> dx = dL/dx, dgamma[C], dbeta[C].  The LeakyReLU derivative is taken on the recomputed z
 * (z > 0 ? 1 : slope).  bws: B*C*2 doubles (the planes' {sum dz, sum dz * xhat}, statistics launch); the apply launch adds them over the
 * batch in batch order. */
int cf_norm_act_bwd(const float* x, const float* dy, const double* ws, const float* gamma, const float* beta, float* dx, float* dgamma,
                    float* dbeta, double* bws, int B, int C, int HW, float eps, float slope, void* stream);
/* cf_dc_ce_loss: l = CE(mean over pixels) + 1 - mean over classes 1..K-1 of (2tp + smooth) / (2tp + fp + fn + smooth + 1e-8), tp/fp/fn summed
 * over batch and space (batch_dice, do_bg = False) of softmax(logits [B,K,HW]); target int32 [B,HW].  *loss += weight * l (a device scalar
 * that collects a step's outputs in call order), *loss_out = l when not null, dlogits = weight * dl/dlogits when not null.  coef: 2*K
 * floats, part: cf_dc_ce_loss_blocks(B*HW) * (1 + 3K) doubles.  2 <= K <= 16.  Three launches, no host read. */
int cf_dc_ce_loss_blocks(long N);
int cf_dc_ce_loss(const float* logits, const int* target, float* dlogits, float* loss, float* loss_out, float* coef, double* part, int B, int K,
                  int HW, float smooth, float weight, void* stream);
/* The optimizer works on flat fp32 arenas; table (device int64 [T][3]) = {offset, size, has_grad} per tensor.
 * cf_grad_norm: out[0] = torch's total_norm over the tensors with a gradient (the 2-norm of the per-tensor 2-norms), out[1] =
 * min(1, max_norm / (out[0] + 1e-6)); tnorm: T floats.
 * cf_sgd_nesterov, per element of every tensor with has_grad: g = grad * clip[1]; g += wd * p; buf = first ? g : mu * buf + g; g += mu * buf;
 * p -= lr * g.  Tensors without a gradient keep parameter and buffer bit for bit (no weight decay either).  max_size: the largest tensor. */
int cf_grad_norm(const float* grad, const long* table, int T, float max_norm, float* tnorm, float* out, void* stream);
int cf_sgd_nesterov(float* param, const float* grad, float* mom, const long* table, int T, long max_size, const float* clip, float lr,
                    float wd, float mu, int first, void* stream);

/* ---------------------------------------------------------------- measurement hooks (bench.py only; no reference analogue)
 * cf_profile_enable(n): pre-create n event pairs and time every conv / CorrVolume launch with a (start, stop) pair that
 * brackets exactly that kernel on its own stream (hipExtLaunchKernelGGL); 0 disables.  Kernel ids:
 * 0,1,2 = conv_igemm MT 1,2,4 (work = flops); 3,4,5 = corr_volume_p7 stride 1,2,4 (work = algorithmic bytes);
 * 6 = conv_f16s (work = flops); 7 = RAFT all-pairs volume + pyramid pooling, 8 = RAFT correlation lookup, 9 = convex
 * upsampling, 10 = GroupNorm apply passes, 11 = 2-D bilinear warp, 12 = 2-D label warp, 13 = 2-D Jacobian determinant (work =
 * algorithmic bytes), 14 = direct 3x3 convolution to <= 4 channels (bytes), 15 = conv_stream, 16 = conv_wino (work = direct-form flops).
 * cf_profile_read sums kernel durations [ms], work and launches since the last cf_profile_reset (it synchronises: call it
 * outside the timed region). */
int cf_profile_enable(int max_launches);
int cf_profile_reset(void);
int cf_profile_read(int kernel_id, double* total_ms, double* total_work, long* launches);

#ifdef __cplusplus
}
#endif
#endif /* CINEFLOW_H */
