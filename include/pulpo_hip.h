/* pulpo_hip.h — C ABI of libpulpo_hip.so: PULPo's registration hot path as hand-written HIP kernels for
 * AMD Instinct MI355X (gfx950, CDNA4).
 *
 * The reference (leonardsiegert/PULPo) has no native/FFI layer: its hot path is a sequence of ATen operators issued
 * from Python.  Each entry point below replaces one of those operator call sites; the citation names
 * the reference line that issues it.  The Python host (pulpo_amd/ops.py) binds these with ctypes inside
 * torch.autograd.Function wrappers; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer to fp32 unless stated; the library never allocates, frees or synchronises:
 *    outputs, scratch and saved-for-backward buffers are owned by the caller.  Work is only enqueued on `stream`
 *    (a hipStream_t passed as void*; NULL = the default stream).  No global mutable state: safe to call from the
 *    main thread and the autograd thread concurrently, and from one process per GPU.
 *  - Return value: 0 on success, otherwise a non-zero code (hipError_t value, or -1 for an argument error);
 *    pulpo_last_error() then returns a thread-local message.  Nothing throws.
 *  - "channels-last" activations: element (b, voxel v, channel c) lives at  base + b*bs + v*ps + c*cs  (strides in
 *    floats).  A contiguous (B,D,H,W,C) tensor has ps = C, cs = 1, bs = D*H*W*C; a channel slice of a wider
 *    concatenation buffer keeps the buffer's ps.  Where only `ps` is passed, cs == 1 and bs == D*H*W*ps are implied.
 *  - "planar": contiguous (B, C, D, H, W), the reference's own layout, used for 1- and 3-channel images and fields.
 *  - voxel order is (D,H,W) = ('ij' indexing of dims 0,1,2), channel i of a displacement field moves along dim i
 *    (src/network_blocks.py:94-98).
 */
#ifndef PULPO_HIP_H
#define PULPO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------- runtime
 * PULPO_ABI_VERSION is bumped whenever a prototype below changes its argument list or a buffer contract, or an entry point is removed
 * (history: INTEGRATION.md "ABI history").  pulpo_abi_version() returns the value the library was built with: a client compares it with
 * the header it was compiled against before the first call (pulpo_amd/_lib.py does). */
#define PULPO_ABI_VERSION 8
int pulpo_abi_version(void);
const char* pulpo_last_error(void);

/* ------------------------------------------------------------------------- ConvUnit: Conv3d(k=3, pad=1, bias)
 * replaces nn.Conv3d inside ConvUnit (src/network_blocks.py:23) = aten::convolution / convolution_backward.
 * Implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32).  K = reduction channels, N = output channels.
 *   forward : K = Cin,  N = Cout, weights packed with dgrad = 0
 *   dgrad   : K = Cout, N = Cin,  weights packed with dgrad = 1 (transposed + tap-flipped), bias = NULL
 * `stats` (nullable): [pulpo_conv3d_k3_stat_tiles()][2][N] per-tile (sum, sum of squares) of the outputs, the
 * BatchNorm batch statistics partials (src/network_blocks.py:24). */
size_t pulpo_conv3d_k3_packed_floats(int K, int N);
int pulpo_conv3d_k3_pack_weight(const float* w /*[Cout][Cin][3][3][3]*/, float* wp, int Cin, int Cout, int dgrad, void* stream);
int pulpo_conv3d_k3_stat_tiles(int B, int D, int H, int W);
int pulpo_conv3d_k3_tile_config(int K, int N); /* CH*1000 + NT of the kernel instantiation used (for profiling) */
size_t pulpo_conv3d_k3_fwd_scratch_floats(int B, int D, int H, int W, int K, int N); /* > 0 for small volumes (deterministic split-K) */
int pulpo_conv3d_k3_fwd(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, const float* bias, float* out,
                        int64_t out_bs, int64_t out_ps, int64_t out_cs, float* stats, float* scratch /*nullable if the query is 0*/, int B,
                        int D, int H, int W, int K, int N, void* stream);
/* eval-mode ConvUnit in ONE kernel (inference: predict / predict_deterministic / evaluate.py): out = LeakyReLU_slope(conv * scale + shift)
 * with coef from pulpo_bn_eval_coef (running statistics folded) - the store of the convolution applies what pulpo_bn_lrelu_apply would */
int pulpo_conv3d_k3_fwd_bn_lrelu(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, const float* bias,
                                 const float* coef, float slope, float* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, float* scratch, int B,
                                 int D, int H, int W, int K, int N, void* stream);
/* Winograd F(2x2,3x3) in (y, x) of the same convolution for volumes tiled 4x8x8 (2.25x fewer matrix instructions, all fp32; results differ
 * from the direct kernel by fp32 rounding only).  pulpo_conv3d_k3_algo() says which kernel family to use for a shape (0 direct, 2 this one);
 * each has its own weight packing; coef (nullable) selects the fused eval-mode BatchNorm + LeakyReLU store, stats (nullable) the BatchNorm
 * partials (same tiles).  (Family 1, F(2,3) along x only, was retired in round 3: measured slower on every shape.) */
int pulpo_conv3d_k3_algo(int B, int D, int H, int W, int K, int N);
size_t pulpo_conv3d_k3_packed_wino2_floats(int K, int N);
int pulpo_conv3d_k3_pack_weight_wino2(const float* w /*[Cout][Cin][3][3][3]*/, float* wp, int Cin, int Cout, int dgrad, void* stream);
/* scratch: pulpo_conv3d_k3_fwd_wino2_scratch_floats() floats, > 0 for volumes with fewer (voxel tile, channel tile) pairs than resident
 * workgroups (the 20^3 level): the reduction channels are split over several work items (partial slabs + ordered reduce, deterministic) */
size_t pulpo_conv3d_k3_fwd_wino2_scratch_floats(int B, int D, int H, int W, int K, int N);
int pulpo_conv3d_k3_fwd_wino2(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, const float* bias, const float* coef,
                              float slope, float* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, float* stats,
                              float* scratch /*nullable if the query is 0*/, int B, int D, int H, int W, int K, int N, void* stream);
/* 1 when the _wino2 entry points run the pipelined kernel (conv3d_wino2p.hip: double-buffered halo images, weights global -> registers) for a
 * channels-last 16-byte-aligned operand: K % 8 == 0 and D*H*W*in_ps*4 < 2^31.  Otherwise the round-2 kernel runs.
 * Same results either way (network_blocks.py:23). */
int pulpo_conv3d_k3_wino2_pipelined(int D, int H, int W, int K, int64_t in_ps);
/* The data-gradient convolution of a ConvUnit (in = dy of that unit, wp packed with dgrad = 1, N = the unit's input channels) with the
 * FIRST pass of the BatchNorm/LeakyReLU backward of the ConvUnit in front of it fused into the store (the reference runs these as
 * separate autograd nodes: ConvolutionBackward of src/network_blocks.py:23, then LeakyReluBackward / NativeBatchNormBackward of :24-25):
 * part[tile][2][N], tile < pulpo_conv3d_k3_stat_tiles(), receives sum(dbn) and sum(dbn * (bn_y - fp32 batch mean)) per voxel tile, where
 * dbn = out * lrelu'(bn_y * scale + shift); the layout pulpo_bn_bwd_finalize takes.  bn_y / bn_coef: pre-norm tensor (channels-last,
 * N channels) and coefficient block (pulpo_bn_fwd_finalize) of the unit in front.  _ok() = 1 when the shape is accepted. */
int pulpo_conv3d_k3_dgrad_wino2_bnred_ok(int B, int D, int H, int W, int K, int N);
int pulpo_conv3d_k3_dgrad_wino2_bnred(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, float* out, int64_t out_bs,
                                      int64_t out_ps, const float* bn_y, int64_t bn_y_bs, int64_t bn_y_ps, const float* bn_coef, float slope,
                                      float* part, int B, int D, int H, int W, int K, int N, void* stream);
/* Re-packing of many weights in one launch (after an optimizer step wrote the parameters through raw pointers): jobs is a DEVICE array,
 * wp buffers as sized by pulpo_conv3d_k3_packed_floats (kind 0, the layout of pulpo_conv3d_k3_pack_weight) or
 * pulpo_conv3d_k3_packed_wino2_floats (kind 2, the layout of pulpo_conv3d_k3_pack_weight_wino2) or pulpo_conv3d_k3_packed_bf16_elems
 * bf16 elements (kind 3, the layout of pulpo_conv3d_k3_pack_weight_bf16; wp then points to uint16_t). */
typedef struct PulpoPackJob {
    const float* w;   /* [Cout][Cin][3][3][3] */
    float* wp;
    int Cin, Cout, dgrad, kind;
} PulpoPackJob;
int pulpo_conv3d_k3_pack_weights_multi(const PulpoPackJob* jobs, int njobs, void* stream);
/* weight gradient: dw[Cout][Cin][27] = sum_voxels in[v + tap - 1][ci] * dy[v][co]; scratch is overwritten */
size_t pulpo_conv3d_k3_wgrad_scratch_floats(int Cin, int Cout);
/* which weight-gradient kernel pulpo_conv3d_k3_wgrad runs for a shape: 3 = Winograd F(2x2x2,3x3x3) (even depths), 2 = Winograd F(2x2,3x3) in
 * (y, x), 0 = direct.  (1, F(2,3) along x only, was retired.)  vec != 0: both operands channels-last, 16-byte aligned, channel counts multiples of 4 (diagnostics / roofline accounting) */
int pulpo_conv3d_k3_wgrad_algo(int B, int D, int H, int W, int Cin, int Cout, int vec);
/* accumulate: 0 dw = result, 1 dw += result, 2 DEFERRED - `scratch` must arrive all zero, keeps the packed sums [27][Cin][NPad] and dw (may
 * be NULL) is not touched: the caller finishes every deferred gradient of a backward pass with one pulpo_grad_finish_multi launch (which
 * adds into dw and returns the scratch to all zero).  The same holds for the bf16-operand variant below. */
int pulpo_conv3d_k3_wgrad(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* dy, int64_t dy_bs, int64_t dy_ps,
                          int64_t dy_cs, float* dw, int accumulate, float* scratch, int B, int D, int H, int W, int Cin,
                          int Cout, void* stream);
/* One launch for the parameter-gradient epilogues of a whole backward pass (the reference has no counterpart: autograd's per-parameter
 * AccumulateGrad adds, torch.optim's view of .grad).  jobs: DEVICE array of njobs entries.
 *   kind 0  dst[co][ci][27] += src[tap][ci][co of NPad] and src := 0     a = Cin, b = Cout, c = NPad   (deferred pulpo_conv3d_k3_wgrad)
 *   kind 1  dst[col] += sum_r src[r][col]                                a = rows, b = columns         (conv-bias gradient from the
 *           pulpo_bn_lrelu_bwd_apply partials) */
typedef struct PulpoGradJob {
    const float* src;
    float* dst;
    int kind, a, b, c;
} PulpoGradJob;
int pulpo_grad_finish_multi(const PulpoGradJob* jobs, int njobs, void* stream);

/* bf16-operand variant (BASELINE configs 4-5; no counterpart in the reference, whose arithmetic is fp32 throughout - SURVEY.md 8(d)):
 * the same convolution with both operands rounded to bf16 (round-to-nearest-even) as they are staged, products and sums in
 * fp32 on v_mfma_f32_32x32x16_bf16.  Activations, gradients, bias, outputs and `stats` stay fp32; `stats` has
 * pulpo_conv3d_k3_fwd_bf16_stat_tiles() rows.  wp holds bf16 bit patterns. */
size_t pulpo_conv3d_k3_packed_bf16_elems(int K, int N);
int pulpo_conv3d_k3_pack_weight_bf16(const float* w /*[Cout][Cin][3][3][3]*/, uint16_t* wp, int Cin, int Cout, int dgrad, void* stream);
size_t pulpo_conv3d_k3_fwd_bf16_scratch_floats(int B, int D, int H, int W, int K, int N);
int pulpo_conv3d_k3_fwd_bf16_stat_tiles(int B, int D, int H, int W); /* rows of `stats` this kernel writes (its own tiling policy) */
int pulpo_conv3d_k3_fwd_bf16(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const uint16_t* wp, const float* bias, float* out,
                             int64_t out_bs, int64_t out_ps, int64_t out_cs, float* stats, float* scratch, int B, int D, int H, int W, int K,
                             int N, void* stream);
int pulpo_conv3d_k3_fwd_bn_lrelu_bf16(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const uint16_t* wp, const float* bias,
                                      const float* coef, float slope, float* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, float* scratch,
                                      int B, int D, int H, int W, int K, int N, void* stream);
int pulpo_conv3d_k3_wgrad_bf16(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* dy, int64_t dy_bs, int64_t dy_ps,
                               int64_t dy_cs, float* dw, int accumulate, float* scratch /*pulpo_conv3d_k3_wgrad_scratch_floats*/, int B, int D,
                               int H, int W, int Cin, int Cout, void* stream);

/* ------------------------------------------------------------- ConvUnit: BatchNorm3d + LeakyReLU(0.2, inplace)
 * replaces nn.BatchNorm3d / nn.LeakyReLU (src/network_blocks.py:24-25) = aten::native_batch_norm(+_backward),
 * aten::leaky_relu_(+_backward).  coef = 8*C floats: [4][C] floats (mean, rstd, scale = gamma*rstd, shift = beta - mean*scale)
 * followed by [2][C] doubles (mean, rstd): the backward carries the per-channel means in double, as ATen's CPU kernels do. */
int pulpo_colsum(const float* partials, int nrow, int ncol, float* out, float scale, int accumulate, void* stream);
size_t pulpo_bn_fwd_finalize_scratch_doubles(int ntile, int C);
int pulpo_bn_fwd_finalize(const float* stats, int ntile, int C, double count, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, int64_t* num_batches_tracked /*nullable, += 1*/, float momentum, float eps, float* coef,
                          double* scratch, void* stream);
int pulpo_bn_eval_coef(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, int C,
                       float* coef, void* stream);
int pulpo_bn_lrelu_apply(const float* y, int64_t yps, float* z, int64_t zps, const float* coef, int64_t npix, int C, float slope, void* stream);
/* the same pass for the last ConvUnit of an encoder level, whose output is pooled for the next level (components/pulpo.py:58): writes z AND
 * pooled = AvgPool3d(2, 2, ceil_mode=True)(z) while y is read once; _ok() = 1 when the float4 path applies (else: the two separate passes) */
int pulpo_bn_lrelu_apply_pool2_ok(int C, int64_t yps, int64_t zps, int64_t pps);
int pulpo_bn_lrelu_apply_pool2(const float* y, int64_t yps, float* z, int64_t zps, float* pooled, int64_t pps, const float* coef, int B, int D, int H,
                               int W, int C, float slope, void* stream);
int pulpo_bn_bwd_blocks(int64_t npix, int C);
/* gin = (add +) avgpool2_bwd(gout) AND the partial rows of pulpo_bn_lrelu_bwd_reduce for the ConvUnit whose output was pooled, in one pass
 * (the last unit of every encoder level: pooling backward, autograd's accumulation add and the BatchNorm-backward reduction read its
 * gradient three times otherwise); partial: pulpo_bn_bwd_blocks(B*D*H*W, C) rows of 2C floats; add nullable */
int pulpo_avgpool2_bwd_bnred(const float* gout, int64_t gops, const float* add, int64_t aps, float* gin, int64_t gips, const float* y, int64_t yps,
                             const float* coef, float slope, float* partial, int B, int D, int H, int W, int C, void* stream);
int pulpo_bn_lrelu_bwd_reduce(const float* dz, int64_t dzps, const float* y, int64_t yps, const float* coef, int64_t npix, int C, float slope,
                              float* partial /*[blocks][2C]*/, void* stream);
/* rows [nrow][2][C] = (sum dbn, sum dbn * (y - fp32 batch mean)): the block partials of pulpo_bn_lrelu_bwd_reduce (nrow = pulpo_bn_bwd_blocks)
 * or the per-voxel-tile rows of pulpo_conv3d_k3_dgrad_wino2_bnred (nrow = pulpo_conv3d_k3_stat_tiles).  coef: the unit's coefficient block.
 * scratch: pulpo_bn_bwd_finalize_scratch_doubles(nrow, C) doubles (NULL when that is 0). */
size_t pulpo_bn_bwd_finalize_scratch_doubles(int nrow, int C);
int pulpo_bn_bwd_finalize(const float* rows, int nrow, int C, const float* coef, double count, int use_means, float* dbeta, float* dgamma,
                          int accumulate, double* totd /*[2C]: mean(dbn) | mean(dbn*xhat)*/, double* scratch, void* stream);
int pulpo_bn_lrelu_bwd_apply(const float* dz, int64_t dzps, const float* y, int64_t yps, const float* coef, const double* totd, float* dy,
                             int64_t dyps, int64_t npix, int C, float slope, float* partial2 /*[blocks][C]*/, void* stream);

/* ---------------------------------------------------------------------------- 1x1x1 heads (channel mixing C -> 3)
 * nout = 6: MuSigmaBlock + gauss_sampler (src/network_blocks.py:54-60, :7-8; eps = injected N(0,1) noise, NULL -> z = mu)
 * nout = 3: VelocityField's last conv (src/network_blocks.py:81).   Wt = [nout][C], bias = [nout]; outputs planar (B,3,V). */
int pulpo_heads_fwd(const float* h, int64_t ps, const float* Wt, const float* bias, const float* eps, float* o0, float* o1, float* o2, int nout,
                    int B, int64_t V, int C, void* stream);
int pulpo_heads_bwd_blocks(int B, int64_t V, int C);
int pulpo_heads_bwd(const float* h, int64_t ps, const float* Wt, const float* g0, const float* g1, const float* g2, const float* eps,
                    const float* sigma, float* dh, int64_t dps, float* partial /*[blocks][nout*C+nout]*/, int nout, int B, int64_t V, int C,
                    void* stream);

/* ------------------------------------------------------------------------------------------------- resampling
 * avgpool2: nn.AvgPool3d(2,2,ceil_mode=True) (src/components/pulpo.py:33,59,174-177), channels-last, any C (C = 1: images)
 * resize_trilinear: F.interpolate(trilinear, align_corners=False) on planar tensors (pulpo.py:202; network_blocks.py:141-147
 *   with `mult` = ResizeTransform's factor and `add` = DFAdder's second operand, network_blocks.py:156-157; losses.py:313)
 * feedback_up2: the x2 up-sampling + torch.cat of the feedback tensors (pulpo.py:195-206), planar sources -> channels-last out */
int pulpo_avgpool2_fwd(const float* in, int64_t ips, float* out, int64_t ops, int B, int D, int H, int W, int C, void* stream);
int pulpo_avgpool2_bwd(const float* gout, int64_t gops, float* gin, int64_t gips, int B, int D, int H, int W, int C, void* stream);
/* gin = add + avgpool2_bwd(gout): the gradient of a tensor that is pooled AND used as a skip connection (components/pulpo.py:58, 77), both
 * contributions in one pass instead of a pooling backward and autograd's accumulation add; add: channels-last with voxel stride aps */
int pulpo_avgpool2_bwd_add(const float* gout, int64_t gops, const float* add, int64_t aps, float* gin, int64_t gips, int B, int D, int H, int W,
                           int C, void* stream);
int pulpo_resize_trilinear_fwd(const float* in, const float* add, float* out, int64_t nplanes, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                               float mult, void* stream);
int pulpo_resize_trilinear_bwd(const float* gout, float* gin, int64_t nplanes, int Di, int Hi, int Wi, int Do, int Ho, int Wo, float mult,
                               void* stream);
/* the same with explicit source-coordinate steps per output voxel (scale_* <= 0: in / out, as above).  F.interpolate(scale_factor = f) - what
 * ResizeTransform calls, src/network_blocks.py:141-147 - maps coordinates with 1 / f whatever floor(in * f) is, so for sizes where in * f is
 * not an integer (a factor < 1 on odd sizes, non-integer factors) it differs from the size-ratio mapping of F.interpolate(size = ...)
 * (components/pulpo.py:202, losses.py:313).  Since ABI 3. */
int pulpo_resize_trilinear_scaled_fwd(const float* in, const float* add, float* out, int64_t nplanes, int Di, int Hi, int Wi, int Do, int Ho,
                                      int Wo, float scale_d, float scale_h, float scale_w, float mult, void* stream);
int pulpo_resize_trilinear_scaled_bwd(const float* gout, float* gin, int64_t nplanes, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                      float scale_d, float scale_h, float scale_w, float mult, void* stream);
int pulpo_feedback_up2_fwd(const float* const* srcs /*host array of device ptrs*/, const int* chans /*host*/, int nsrc, float* out, int64_t ops,
                           int B, int Di, int Hi, int Wi, void* stream);
int pulpo_feedback_up2_bwd(const float* gout, int64_t gops, float* const* gsrcs /*host array, entries may be NULL*/, const int* chans, int nsrc,
                           int B, int Di, int Hi, int Wi, void* stream);

/* ------------------------------------------------------------------------------ warp and scaling-and-squaring
 * warp3d: SpatialTransformer.forward (src/network_blocks.py:101-121) = grid_sample(bilinear, border, align_corners=False)
 *   on coordinates normalised by (S-1); image size may differ from the grid size (src/models.py:330).
 * vecint: VecInt.forward (src/network_blocks.py:173-177).  work = (nsteps+1) field buffers, result = the last one. */
int pulpo_warp3d_fwd(const float* df, const float* img, float* out, int B, int C, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, void* stream);
/* pulpo_warp3d_fwd for a single-channel weight volume (cost-function masks): the same sample positions and corners, the
 * interpolation as nested differences a + f (b - a), which returns a constant volume exactly (the eight fp32 corner weights of
 * pulpo_warp3d_fwd do not sum to exactly 1).  mask (B,1,Di,Hi,Wi) -> out (B,1,Dg,Hg,Wg); forward only. */
int pulpo_warp_mask_fwd(const float* df, const float* mask, float* out, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, void* stream);
int pulpo_warp3d_bwd(const float* df, const float* img, const float* gout, float* gdf, float* gimg, int B, int C, int Dg, int Hg, int Wg, int Di,
                     int Hi, int Wi, void* stream);
int pulpo_vecint_fwd(const float* v, float* work, int B, int D, int H, int W, int nsteps, void* stream);
/* tmp: pulpo_vecint_bwd_tmp_floats() floats (one zero-filled buffer per step for fields of 16^3 and up, two otherwise) */
size_t pulpo_vecint_bwd_tmp_floats(int B, int D, int H, int W, int nsteps);
int pulpo_vecint_bwd(const float* work, const float* gout, float* gin, float* tmp /*nullable if the query is 0*/, int B, int D, int H, int W,
                     int nsteps, void* stream);

/* ------------------------------------------------------------------------------------------------------ losses
 * ncc:   NCC_loss (src/losses.py:85-135); I = y_true, J = y_pred, planar (B,1,D,H,W); N = B*D*H*W.
 * kl:    KL_two_gauss_with_diag_cov (src/losses.py:47-76); mu1/sigma1 NULL = the N(0,1) prior (src/components/pulpo.py:330-341)
 * l2reg: L2_reg (src/losses.py:208-222).
 * Forward kernels write pulpo_loss_blocks(n) partial sums; pulpo_colsum(partial, blocks, 1, out, scale) finishes the
 * scalar.  Backward kernels take the upstream scalar gradient as a device pointer `gscale` (nullable = 1). */
int pulpo_loss_blocks(int64_t n);
int pulpo_ncc_fwd(const float* I, const float* J, float* S /*5N, saved*/, float* T /*10N scratch*/, float* partial, int B, int D, int H, int W,
                  int win, void* stream);
int pulpo_ncc_bwd(const float* I, const float* J, const float* S, float* T /*6N scratch*/, const float* gscale, float coef, float* gJ, int B, int D,
                  int H, int W, int win, void* stream);
/* Cost-function masking (no counterpart in the reference, whose loaders raise "Mask not implemented").  wa and wb
 * (wb nullable = 1) are weight volumes (B,1,D,H,W) in [0,1], m = wa * wb is formed inside the kernels.  The window sums run over all
 * voxels; m weights the per-voxel cost.  The forward kernels write TWO columns per block, partial[2 * blk] = sum of m * cost and
 * partial[2 * blk + 1] = sum of m (2 * pulpo_loss_blocks / pulpo_metric_blocks floats); pulpo_masked_finish reduces them in double on the
 * device:  q = scale * sum0 / M (0 when M == 0),
 *   out[0] = root ? sqrt(q) : q                          the loss
 *   out[1] = d out[0] / d sum0  (0 when M == 0, or when root and q == 0): the backward entry points take  upstream * out[1]  as gscale
 *   out[2] = M / count,  out[3] = M
 * ncc_masked:    scale = -gamma * V                   -> -gamma * V * sum(m cc) / M;     bwd: gJ = coef * gscale * (box(m a) + 2 J box(m b) + I box(m c))
 *                the launch sequences of pulpo_ncc_fwd / pulpo_ncc_bwd with the MASKED instantiation of the one kernel m enters: the last (D) pass
 *                (box_march_kernel<5, PAD, 1, true> / ncc_final_kernel<true>) forward, ncc_abc_kernel<true> backward
 * sqdiff_masked: a, b planar (B,C,V), m broadcast over the C channels, sum of m counted once per voxel;
 *                scale = V / C -> L2_masked, scale = 1 / C with root -> RMSE_masked;  bwd: ga = coef * gscale * 2 m (a - b) */
int pulpo_ncc_masked_fwd(const float* I, const float* J, const float* wa, const float* wb /*nullable*/, float* S /*5N, saved*/,
                         float* T /*10N scratch*/, float* partial /*2 * pulpo_loss_blocks(N)*/, int B, int D, int H, int W, int win, void* stream);
int pulpo_ncc_masked_bwd(const float* I, const float* J, const float* S, const float* wa, const float* wb /*nullable*/, float* T /*6N scratch*/,
                         const float* gscale, float coef, float* gJ, int B, int D, int H, int W, int win, void* stream);
int pulpo_masked_finish(const float* partial, int nblk, double scale, int root, double count, float* out /*4*/, void* stream);
/* MIND-SSC similarity term (no counterpart in the reference): the 12-channel self-similarity descriptor
 *   f_k = exp(-(D_k - min_j D_j) / (mean_k (D_k - min_j D_j) + eps)),  D_k = clamped 3^3 box mean of the squared difference of the image at the
 *   two offsets of channel k (offsets -z +z -y +y -x +x times the dilation d, replicate padding), and cost = 1/12 sum_k (f_k[pred] - f_k[true])^2.
 * Images planar (B,1,D,H,W) fp32, every extent >= 2, d >= 1 (as far as the staged tile fits 64 KiB of LDS: d <= 7), eps > 0; N = B*D*H*W.
 * mind_descriptor: out = (B,12,D,H,W) stored as 12 planes of N floats, out[k N + e].
 * mind_fwd: partial = pulpo_mind_blocks(B,D,H,W,d) rows of one column (wa NULL: sum of cost; finish with pulpo_colsum(scale = 1/B)) or of two
 *   columns (masks wa, wb nullable: sum of m cost, sum of m; finish with pulpo_masked_finish(scale = V)).
 * mind_bwd: gpred = coef * gscale[0] * d(sum m cost)/d pred (gscale nullable = 1); scratch: 12 N floats.  No atomics: bit-identical run to run. */
int pulpo_mind_blocks(int B, int D, int H, int W, int d);
int pulpo_mind_descriptor(const float* I, float* out /*12N*/, int B, int D, int H, int W, int d, float eps, void* stream);
int pulpo_mind_fwd(const float* y_true, const float* y_pred, const float* wa /*nullable*/, const float* wb /*nullable*/, float* partial, int B, int D,
                   int H, int W, int d, float eps, void* stream);
int pulpo_mind_bwd(const float* y_true, const float* y_pred, const float* wa /*nullable*/, const float* wb /*nullable*/, float* scratch /*12N*/,
                   const float* gscale, float coef, float* gpred, int B, int D, int H, int W, int d, float eps, void* stream);
/* Mutual-information similarity term (Mattes; no counterpart in the reference): a cubic-B-spline Parzen joint histogram
 *   P[a,c] = sum_v m_v beta3(u(pred_v) - a) beta3(u(true_v) - c),  u(v) = clamp(v,0,1) (K - 3) + 1,  K bins in [4, 64],  m = wa * wb (1 without),
 *   p = P / sum P,  MI_b = sum p (log(p + 1e-12) - log(pa pb + 1e-12)),  loss = -gamma V mean_b MI_b  (MI_b = 0 where sum P = 0).
 * Images planar fp32, B batch elements of V voxels each (volumes and slices alike: the term is pointwise), expected in [0,1].
 * mi_fwd: scratch = pulpo_mi_scratch_floats(B,V,K) floats, one slab row per workgroup of the histogram kernel (pulpo_mi_blocks(B,V) rows
 *   over the batch), uninitialised on entry; writes p (B K K), mi (B), G = d MI_b / d P (B K K) and the loss scalar.  No host read.
 * mi_bwd: gpred = coef * gscale[0] * d(sum_b sum_ac G P)/d pred (gscale nullable = 1); the caller's coef is -gamma V / B.
 * No atomics: bit-identical run to run, and a time that does not depend on the image content. */
int pulpo_mi_blocks(int B, int64_t V);
int64_t pulpo_mi_scratch_floats(int B, int64_t V, int K);
int pulpo_mi_fwd(const float* y_true, const float* y_pred, const float* wa /*nullable*/, const float* wb /*nullable*/, float* scratch, double* p,
                 double* mi, float* G, float* loss, int B, int64_t V, int K, double gamma, void* stream);
int pulpo_mi_bwd(const float* y_true, const float* y_pred, const float* wa /*nullable*/, const float* wb /*nullable*/, const float* G,
                 const float* gscale, float coef, float* gpred, int B, int64_t V, int K, void* stream);
int pulpo_kl_fwd(const float* mu, const float* sigma, const float* mu1 /*nullable: 0*/, const float* sigma1 /*nullable: 1*/, int64_t n,
                 float* partial, void* stream);
int pulpo_kl_bwd(const float* mu, const float* sigma, const float* mu1, const float* sigma1, const float* gscale, float coef, float* gmu,
                 float* gsigma, int64_t n, void* stream);
int pulpo_l2reg_fwd(const float* df, int64_t nplanes, int D, int H, int W, float* partial, void* stream);
int pulpo_l2reg_bwd(const float* df, const float* gscale, float coef, float* gdf, int64_t nplanes, int D, int H, int W, void* stream);
/* Bending-energy regulariser (no counterpart in the reference; added without a version bump).  df = nplanes planar
 * volumes (D,H,W) of fp32 voxels, nplanes = B * C.  With central differences at INTERIOR voxels only (1 .. extent - 2; no padding, no one-sided
 * stencil),  u_xx = u[x+1] - 2u + u[x-1],  u_xy = (u[x+1,y+1] - u[x+1,y-1] - u[x-1,y+1] + u[x-1,y-1]) / 4  and
 *   e = u_xx^2 + u_yy^2 + u_zz^2 + 2 u_xy^2 + 2 u_xz^2 + 2 u_yz^2;    D == 1 is the 2-D form (no z term).
 * bending_fwd: partial[blk] = the workgroup's sum of e over its interior voxels, pulpo_bending_blocks(nplanes, D, H, W) floats; finish with
 *   pulpo_colsum(scale = lamb * D*H*W / (nplanes * n_interior)).
 * bending_bwd: gdf = 2 * coef * gscale[0] * sum_k w_k A_k^T (M . A_k u) (gscale nullable = 1), M the interior mask, w = (1,1,1,2,2,2).
 * One launch each, no atomics, no scratch: bit-identical run to run.  Needs H >= 3, W >= 3 and D == 1 or D >= 3; pulpo_bending_blocks
 * returns 0 for any other shape. */
int pulpo_bending_blocks(int64_t nplanes, int D, int H, int W);
int pulpo_bending_fwd(const float* df, int64_t nplanes, int D, int H, int W, float* partial, void* stream);
int pulpo_bending_bwd(const float* df, const float* gscale, float coef, float* gdf, int64_t nplanes, int D, int H, int W, void* stream);
/* sum_l w_l * term_l of the Hierarchical* losses (src/losses.py:262-276, 305-325, 343-355) and models.py:161-162's `kl * beta` in one launch:
 * levels[i] = w[i] * terms[i] (* scale if scaled), total[0] = (sum_i w[i] * terms[i]) (* scale if scaled), summed in index order like the
 * reference's `loss = loss + all_levels[l]`.  Device arrays of n floats (total: 1); n <= 64.  Backward: gterms[i] = (gtotal[0] + glevels[i]) *
 * scale * w[i]; gtotal / glevels nullable (= 0). */
int pulpo_weighted_sum_fwd(const float* terms, const float* weights, int n, float scale, int scaled, float* levels, float* total, void* stream);
int pulpo_weighted_sum_bwd(const float* gtotal, const float* glevels, const float* weights, int n, float scale, float* gterms, void* stream);

/* ------------------------------------------------------------------- alternative losses / evaluation metrics
 *   sqdiff: L2_loss (src/losses.py:79-83); dice: Soft_dice_loss (:137-145);
 * jacdet: jacobian_det (:172-199, 3-D); jdetstd: JDetStd (:202-204).  Scalars finish on the device. */
int pulpo_metric_blocks(int64_t n);
int pulpo_sqdiff_fwd(const float* a, const float* b, int64_t n, float* partial, void* stream);
int pulpo_sqdiff_bwd(const float* a, const float* b, const float* gscale, float coef, float* ga, int64_t n, void* stream);
int pulpo_sqdiff_masked_fwd(const float* a, const float* b, const float* wa, const float* wb /*nullable*/,
                            float* partial /*2 * pulpo_metric_blocks(B*C*V)*/, int B, int C, int64_t V, void* stream);
int pulpo_sqdiff_masked_bwd(const float* a, const float* b, const float* wa, const float* wb /*nullable*/, const float* gscale, float coef, float* ga,
                            int B, int C, int64_t V, void* stream);
int pulpo_dice_blocks(int64_t V);
int pulpo_dice_fwd(const float* inp, const float* tgt, int nplanes, int64_t V, float dice_factor, float* partial, double* numden, float* loss,
                   void* stream);
int pulpo_dice_bwd(const float* inp, const float* tgt, const double* numden, const float* gscale, int nplanes, int64_t V, float dice_factor,
                   float* ginp, void* stream);
/* jacdet partial (since ABI 8): 2 * pulpo_metric_blocks(B*D*H*W) DOUBLES, each block's sums of J - 1 and (J - 1)^2 (centred: J sits near 1) */
int pulpo_jacdet_fwd(const float* df, float* out, double* partial /*nullable*/, int B, int D, int H, int W, int normalize, void* stream);
int pulpo_jdetstd_finalize(const double* partial, int64_t n, float lamb, double* stat, float* loss, void* stream);
/* KL_nondiagonal.loss (src/losses.py:8-44, 3-D): mu, sigma planar (B,3,D,H,W), nplanes = B*3 */
int pulpo_kl_nondiag_fwd(const float* mu, const float* sigma, int64_t nplanes, int D, int H, int W, float prior_lambda, float* partial, float* loss,
                         void* stream);
int pulpo_kl_nondiag_bwd(const float* mu, const float* sigma, const float* gscale, int64_t nplanes, int D, int H, int W, float prior_lambda,
                         float* gmu, float* gsigma, void* stream);
int pulpo_jdetstd_bwd(const float* df, const float* jdet, const double* stat, const float* gscale, float lamb, float* gdf, int B, int D, int H, int W,
                      int normalize, void* stream);

/* Evaluation scalars of the reference's harness, finished on the device:
 *   pulpo_rmse           Evaluate.rmse, evaluate.py:315-319   sqrt(MSELoss(input, target))
 *   pulpo_dsc            Evaluate.dsc, evaluate.py:321-327    mean over (B, C) of (2 mean(t i) + 1e-6) / (mean(t^2) + mean(i^2) + 1e-6)
 *   pulpo_percent_leq0   evaluate.py:1441-1446 ("JDetLeq0")   100 * count(jacobian_det <= 0) / numel
 *   pulpo_warp_landmarks Evaluate.warp_landmarks, evaluate.py:410-423 = src/components/utils.py:15-25
 *                        out[s][k][:] = long(lm[k]) - df[s, :, lm[k][0], lm[k][1], lm[k][2]]; *flag = 1 if an index is out of range */
int pulpo_rmse(const float* a, const float* b, int64_t n, float* partial /* pulpo_metric_blocks(n) */, float* out, void* stream);
int pulpo_dsc(const float* inp, const float* tgt, int nplanes, int64_t V, float* partial /* nplanes*pulpo_dice_blocks(V)*3 */, float* out,
              void* stream);
int pulpo_percent_leq0(const float* x, int64_t n, float* partial /* pulpo_metric_blocks(n) */, float* out, void* stream);
int pulpo_warp_landmarks(const float* lm /*(nlm,nd)*/, const float* df /*(nsamp,nd,D,H,W)*/, float* out /*(nsamp,nlm,nd)*/, int nlm, int nsamp,
                         int nd, int D, int H, int W, int* flag, void* stream);
/* pulpo_field_quality: the two field-quality rows of Evaluate.performance (evaluate.py:1440-1449: HierarchicalRegularization(JDetStd) with
 * lamb = 1, and JDetLeq0) in one pass that reads df (B,3,D,H,W; D == 1: (B,2,1,H,W)) once and writes no determinant map:
 *   out[0] = mean, out[1] = unbiased std, out[2] = 100 * count(J <= 0) / n of jacobian_det(df) over all n = B*D*H*W voxels,
 *   J bit for bit the value pulpo_jacdet_fwd stores.  Block partials of sum(J - 1), sum((J - 1)^2) in double and an integer count, added in
 *   a fixed order: two calls give the same bits.  ws: pulpo_field_quality_ws_bytes(B, D, H, W) bytes. */
int pulpo_field_quality_blocks(int B, int D, int H, int W);
size_t pulpo_field_quality_ws_bytes(int B, int D, int H, int W);
int pulpo_field_quality(const float* df, float* out /* 3 floats */, void* ws, int B, int D, int H, int W, int normalize, void* stream);

/* ------------------------------------------------------------------------------------------ inverse fields (since ABI 6)
 * Inference only: no backward forms (training: "paired VecInt for training" below).  The level fields are stationary velocity fields, so the inverse of the flow VecInt(v) is VecInt(-v).
 * pulpo_vecint_pair_fwd: VecInt.forward (src/network_blocks.py:160-177) on v and on -v in one call: fwd = VecInt(v), the result of
 *   pulpo_vecint_fwd (the same coordinate arithmetic and gather), inv = VecInt(-v).  v, fwd, inv planar (B,3,D,H,W); D == 1 is the 2-D form
 *   (channel 0 zero).  No intermediate field is kept: fields of up to 2048 voxels per batch element run every step in one launch out of
 *   LDS, larger ones one launch per squaring step for both directions, ping-ponging between (fwd, inv) and two scratch fields.
 *   nsteps == 0: fwd = v, inv = -v.  scratch: pulpo_vecint_pair_scratch_floats() floats (2 fields, or 0 for the one-launch form).
 * The two operators below sample GEOMETRICALLY: position p + d in voxel units clamped to [0, S - 1], trilinear with upper corner
 *   min(i0 + 1, S - 1), so that a zero field is the identity.  This is deliberately NOT SpatialTransformer's (S-1)-normalised,
 *   align_corners=False sampling (src/network_blocks.py:101-121), whose zero field is not the identity; it reads a
 *   field the way the reference's landmark rule does (evaluate.py:410-423: displacements in voxels at voxel centres).
 * pulpo_inverse_consistency: a, b planar (B,3,D,H,W), or (B,2,1,H,W) for D == 1.  r(p) = b(p) + a(p + b(p)) per voxel, in double;
 *   out[0] = mean of ||r||_2 over the B*D*H*W voxels, out[1] = its maximum - how far a o b is from the identity, the sanity number of a
 *   diffeomorphic model next to "JDetLeq0" (evaluate.py:1441-1446).  One pass, no composed field; block partials in double added in a fixed
 *   order: two calls give the same bits.  ws: pulpo_inverse_consistency_ws_bytes(B, D, H, W) bytes.
 * pulpo_transport_points: out[s][k][:] = pts[k] + field[s](pts[k]), the field sampled at the point's own fractional position.  With the
 *   inverse field this carries landmarks from the moving to the fixed image exactly where Evaluate.warp_landmarks (evaluate.py:410-423,
 *   long(lm) - df[long(lm)]) is the first-order approximation at a truncated position.  Layout as pulpo_warp_landmarks: pts (npts,nd),
 *   field (nsamp,nd,D,H,W), nd 3, or 2 with D == 1; *flag (zeroed here) = 1 if a point lies outside [0, S - 1]. */
size_t pulpo_vecint_pair_scratch_floats(int B, int D, int H, int W, int nsteps);
int pulpo_vecint_pair_fwd(const float* v, float* fwd, float* inv, float* scratch /*nullable if the query is 0*/, int B, int D, int H, int W, int nsteps,
                          void* stream);
size_t pulpo_inverse_consistency_ws_bytes(int B, int D, int H, int W);
int pulpo_inverse_consistency(const float* a, const float* b, float* out /* 2 floats */, void* ws, int B, int D, int H, int W, void* stream);
int pulpo_transport_points(const float* pts /*(npts,nd)*/, const float* field /*(nsamp,nd,D,H,W)*/, float* out /*(nsamp,npts,nd)*/, int npts,
                           int nsamp, int nd, int D, int H, int W, int* flag, void* stream);

/* ------------------------------------------------------------------------- paired VecInt for training (added within ABI 8: nothing else changed)
 * Both directions of a stationary velocity field integrated with the fields a backward pass needs, and their joint gradient (DESIGN.md
 * section 3u).  work: (nsteps+1, 2, B, 3, D, H, W) floats; work[k][0] is the field after k squarings of v / 2^nsteps, work[k][1] that of
 * -v / 2^nsteps, each with the bits pulpo_vecint_fwd stores for v and for -v.  Fields of up to 2048 voxels per batch element: one launch
 * of 2 B workgroups out of LDS; larger ones: one launch that writes both signs of v / 2^nsteps, then one launch per squaring step.
 * pulpo_vecint_pair_bwd: gin = d loss / d v given gfwd = d loss / d work[nsteps][0] and ginv = d loss / d work[nsteps][1].  One of the two
 *   may be NULL (= zero): that direction's chain is skipped, its fields in work and its share of tmp are not read.  With both, the last
 *   squaring step (whose input gradients are two tensors) runs once per direction and every other step once for both; the last launch
 *   writes gin = (g+ - g-) / 2^nsteps.  Kernels per step as pulpo_vecint_bwd chooses them.  tmp: pulpo_vecint_pair_bwd_tmp_floats() floats.
 * pulpo_vecint_pair_bwd_det: ordered sums, the same bits on every call; each direction runs pulpo_vecint_bwd_det's chain with fixed-point
 *   scales of its own, so with one gradient NULL the result has pulpo_vecint_bwd_det's bits for the other (negated for the inverse
 *   direction).  ws: pulpo_vecint_pair_bwd_det_ws_bytes() bytes. */
int pulpo_vecint_pair_fwd_work(const float* v, float* work, int B, int D, int H, int W, int nsteps, void* stream);
size_t pulpo_vecint_pair_bwd_tmp_floats(int B, int D, int H, int W, int nsteps);
int pulpo_vecint_pair_bwd(const float* work, const float* gfwd /*nullable*/, const float* ginv /*nullable*/, float* gin,
                          float* tmp /*nullable if the query is 0*/, int B, int D, int H, int W, int nsteps, void* stream);
size_t pulpo_vecint_pair_bwd_det_ws_bytes(int B, int D, int H, int W, int nsteps);
int pulpo_vecint_pair_bwd_det(const float* work, const float* gfwd /*nullable*/, const float* ginv /*nullable*/, float* gin,
                              void* ws /*nullable if the query is 0*/, int B, int D, int H, int W, int nsteps, void* stream);

/* ------------------------------------------------------------------------- affine pre-alignment (added within ABI 8: nothing else changed)
 * No counterpart in the reference, whose pairs arrive affinely aligned; DESIGN.md section 3m holds the conventions.
 * theta: (B,3,4) fp32 row-major [M | t] in voxel units of a stated grid (D,H,W), about that grid's centre c = ((D-1)/2, (H-1)/2, (W-1)/2):
 *   voxel v is sent to p = c + M (v - c) + t, and the displacement the affine stands for is d(v) = p - v under SpatialTransformer's convention
 *   (pulpo_warp3d_fwd(d, img) samples img at the coordinate of v + d(v)).  One fp32 expression with a fixed operation order (csrc/affine_core.h)
 *   serves every kernel below: they agree bit for bit, and [I | 0] gives d = 0 exactly.  A depth-1 grid is the 2-D form: theta's depth row and
 *   column are the identity's (the depth displacement is written as 0 whatever they hold).  Arguments are checked before any launch: non-null
 *   pointers, 1 <= B <= 65535, C >= 1, extents >= 1, fewer than 2^31 voxels.
 * pulpo_affine_field: out (B,3,D,H,W) planar = d.
 * pulpo_affine_warp_fwd: out (B,C,Dg,Hg,Wg) = pulpo_warp3d_fwd(pulpo_affine_field(theta on (Dg,Hg,Wg)), img (B,C,Di,Hi,Wi)) bit for bit, without the
 *   field: 8 bytes per voxel and channel instead of 32.  A depth-1 grid needs a depth-1 image.
 * pulpo_affine_warp_bwd: gtheta (B,3,4) = the gradient with respect to theta given gout (B,C,Dg,Hg,Wg); the image is data.  Per voxel
 *   gpos_a = dscale_a sum_c gout_c d interp / d coord_a (pulpo_warp3d_bwd's displacement gradient, dscale_a = 0 where the coordinate was clamped);
 *   gtheta[a][b] = sum_v gpos_a (v_b - c_b), gtheta[a][3] = sum_v gpos_a.  Sums in double: per thread, wave shuffles, LDS, one row of 12
 *   doubles per block in ws, a second launch adds the rows in a fixed order (lane t of a wave rows t, t + 64, ..., then a butterfly).
 *   No float atomics: two calls give the same bits.
 *   ws: pulpo_affine_warp_bwd_ws_bytes(B, Dg, Hg, Wg) bytes, required.
 * pulpo_affine_compose: "affine first, deformable second" as one field out (B,3,Dg,Hg,Wg) on df's grid; theta is in the frame of the image grid
 *   (Di,Hi,Wi).  Per axis q = the clamped coordinate at which pulpo_warp3d_fwd(df, .) samples an image of that size, p = A(q), and
 *   out = p (Sg-1)/(Si-1) - v, the displacement whose sample index is p Si/(Si-1) - 0.5: warp3d(out, img) = warp3d(df, warp3d(affine_field(theta), img))
 *   up to the second interpolation of the two-step route.  H, W > 1 on both grids; depth 1 on both or on neither. */
int pulpo_affine_field(const float* theta, float* out, int B, int D, int H, int W, void* stream);
int pulpo_affine_warp_fwd(const float* theta, const float* img, float* out, int B, int C, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, void* stream);
size_t pulpo_affine_warp_bwd_ws_bytes(int B, int Dg, int Hg, int Wg);
int pulpo_affine_warp_bwd(const float* theta, const float* img, const float* gout, float* gtheta /*(B,3,4)*/, void* ws, int B, int C, int Dg, int Hg,
                          int Wg, int Di, int Hi, int Wi, void* stream);
int pulpo_affine_compose(const float* theta, const float* df, float* out, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, void* stream);

/* ------------------------------------------------------------------------------- Monte-Carlo uncertainty statistics
 * evaluate.py:222-251 stacks N sampled volumes / fields per level and takes torch.std(axis=0) (unbiased) then torch.mean over the
 * channel axis.  Streaming form: fold sample k (1-based count) into running (mean, M2) images of the sample's shape, then
 * out[b][v] = mean_c sqrt(M2[b][c][v] / (k - 1)) (* |scale[b][v]| when scale != NULL: the warped mask of evaluate.py:249). */
int pulpo_mc_moments_update(const float* sample, float* mean, float* m2, int64_t n, int k, void* stream);
int pulpo_mc_moments_std(const float* m2, const float* scale /*nullable (B,V)*/, float* out /*(B,V)*/, int B, int C, int64_t V, int k, void* stream);

/* ------------------------------------------------------------------------------- label maps (Monte-Carlo segmentation uncertainty)
 * pulpo_warp_labels = warp3d(df, one_hot(labels, C)) without the one-hot map: SpatialTransformer (src/network_blocks.py:101-121) applied
 * to a segmentation, as evaluate.py:252-274 does per sample in 2-D (the 3-D branch gives segmentations up, evaluate.py:208).
 *   df (B,3,Dg,Hg,Wg); labels (B,1,Di,Hi,Wi) of dtype ldt (0 = uint8, 1 = int32), 1 <= C <= 256; grid and map may differ in size, depth 1 =
 *   the 2-D form, as in pulpo_warp3d_fwd.  Every output is optional (NULL = not computed):
 *     onehot (B,C,Dg,Hg,Wg)  the warped one-hot map; equal to pulpo_warp3d_fwd on one_hot(labels) bit for bit
 *     amax   (B,1,Dg,Hg,Wg)  arg-max label (dtype ldt), the lowest class on ties
 *     dice   (B,C)           with target (B,1,Dg,Hg,Wg, dtype ldt): per-class Evaluate.dsc (evaluate.py:321-327) of the warped one-hot map
 *                            against one_hot(target); deterministic (64-bit fixed-point sums); ws: pulpo_warp_labels_ws_bytes(B, C) bytes
 *     mean, m2 (B,C,Dg,Hg,Wg) fold the warped one-hot map in as sample k: the arithmetic of pulpo_mc_moments_update
 *   *flag = 1 when a gathered or target label lies outside [0, C) (zeroed here).
 * pulpo_labels_check: *flag = 1 when any of the n labels lies outside [0, C) (zeroed here).
 * pulpo_labels_from_onehot: (B,C,V) fp32 -> (B,V) labels of dtype ldt, arg-max over C with the lowest class on ties (the reference's
 *   one-hot loader output, src/data/OASIS/oasis.py:17,78, converted once).
 * pulpo_map_ncc: Evaluate.ncc (evaluate.py:334-353, zero-normed, population std, eps 1e-15) of two maps of n floats, in double;
 *   partial: 5 * pulpo_map_ncc_blocks(n) doubles; out: 1 double. */
size_t pulpo_warp_labels_ws_bytes(int B, int C);
int pulpo_warp_labels(const float* df, const void* labels, int ldt, int C, const void* target /*nullable*/, float* onehot /*nullable*/,
                      void* amax /*nullable*/, float* dice /*nullable iff target is*/, float* mean /*nullable*/, float* m2 /*nullable iff mean is*/,
                      int k, void* ws, int* flag, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, void* stream);
int pulpo_labels_check(const void* labels, int ldt, int64_t n, int C, int* flag, void* stream);
/* pulpo_warp_labels_soft_dice: the level Dice of Evaluate.performance (evaluate.py:1427, 1454-1455) without a one-hot tensor:
 * Soft_dice_loss (src/losses.py:137-145) of SpatialTransformer(df, one_hot(labels)) against F.interpolate(one_hot(target), size = grid,
 * trilinear, align_corners=False), as HierarchicalReconstructionLoss(["dice"]) resizes it (src/losses.py:279-325).
 *   df (B,3,Dg,Hg,Wg); labels (B,1,Di,Hi,Wi) and target (B,1,Dt,Ht,Wt) of dtype ldt; depth 1 = the 2-D form.
 *   dice (B,C): (2 sum(p t) + 1e-6) / (sum(t^2) + sum(p^2) + 1e-6), sums over the grid's voxels; mean: 1 float, their mean over (b, c)
 *   = 1 - level_dice / num_pixels.  Deterministic (per-voxel products rounded to 64-bit fixed point, integer adds).
 *   ws: pulpo_warp_labels_ws_bytes(B, C) bytes; *flag = 1 when a gathered label lies outside [0, C) (zeroed here). */
int pulpo_warp_labels_soft_dice(const float* df, const void* labels, const void* target, int ldt, int C, float* dice, float* mean, void* ws,
                                int* flag, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, int Dt, int Ht, int Wt, void* stream);
int pulpo_labels_from_onehot(const float* seg, void* labels, int ldt, int B, int C, int64_t V, void* stream);
int pulpo_map_ncc_blocks(int64_t n);
int pulpo_map_ncc(const float* a, const float* b, int64_t n, double* partial, double* out, void* stream);
/* The Dice term of the training step from label maps (added within ABI 8: nothing else changed).
 * pulpo_label_dice_fwd: loss (1 float) = mean_(b,c)(1 - dice_bc) * Vg / dice_factor, Vg = Dg*Hg*Wg: Soft_dice_loss (src/losses.py:137-145) of
 *   SpatialTransformer(df, one_hot(labels)) against F.interpolate(one_hot(target), size = grid) from the fixed-point sums of
 *   pulpo_warp_labels_soft_dice (the same kernel; same arguments, ws and flag).  dice (B,C): that entry point's values bit for bit.
 *   coef (B,C,2) = (a, b) with dL/dp_c(v) = a t_c(v) + b p_c(v): a = -2 S / den, b = 2 S num / den^2, num = 2 sum(p t) + 1e-6,
 *   den = sum(t^2) + sum(p^2) + 1e-6, S = Vg / (dice_factor B C); formed in double.
 * pulpo_label_dice_bwd: ddf (B,3,Dg,Hg,Wg) planar = gup[0] * dL/d df (gup: one float on the device), one thread per grid voxel:
 *   ddf_axis = gup dscale_axis sum_i G_i dw_i/dcoord_axis over the 8 corners, G_i = a[c_i] t_{c_i} + b[c_i] p_{c_i}; dscale is 0 where the
 *   coordinate was clamped and on the depth axis of a depth-1 grid.  No atomics: two calls give the same bits.  A label outside [0, C)
 *   counts for no class.
 * pulpo_labels_pool2: out (B,C,ceil(D/2),ceil(H/2),ceil(W/2)) planar = avg_pool3d(one_hot(labels), 2, 2, ceil_mode=True), edge windows divided
 *   by their in-bounds count (exact: counts over powers of two).
 * pulpo_labels_resize: out (B,C,Do,Ho,Wo) planar = F.interpolate(one_hot(labels (B,1,Dt,Ht,Wt)), size, trilinear, align_corners=False): the tap
 *   weights of pulpo_warp_labels_soft_dice's target summed per class.  Depth 1 is the 2-D form in both. */
int pulpo_label_dice_fwd(const float* df, const void* labels, const void* target, int ldt, int C, float dice_factor, float* loss, float* dice,
                         float* coef, void* ws, int* flag, int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, int Dt, int Ht, int Wt,
                         void* stream);
int pulpo_label_dice_bwd(const float* df, const void* labels, const void* target, int ldt, int C, const float* coef, const float* gup, float* ddf,
                         int B, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, int Dt, int Ht, int Wt, void* stream);
int pulpo_labels_pool2(const void* labels, int ldt, int C, float* out, int B, int D, int H, int W, void* stream);
int pulpo_labels_resize(const void* labels, int ldt, int C, float* out, int B, int Dt, int Ht, int Wt, int Do, int Ho, int Wo, void* stream);

/* ------------------------------------------------------------------------- boundary metrics: distance transform, HD / HD95 / ASSD (added within ABI 8: nothing else changed)
 * No counterpart in the reference; DESIGN.md section 3l holds the definitions.  All distances are in voxels.  Integer arithmetic up to the
 * final square roots: exact, and bit-identical from run to run.
 * pulpo_edt_sq: out[p] = min over the non-zero voxels q of mask of |p - q|^2, exact, for mask (B,1,D,H,W) uint8 and out int32 of the same
 *   shape; an item without a non-zero voxel gets PULPO_EDT_INF everywhere.  Extents 1 ... 1024 per axis; depth 1 is the 2-D form.  Needs no
 *   workspace: the passes along H and D run in place on out.
 * pulpo_surface_distances: for label maps lab_a, lab_b (B,1,D,H,W) (ldt 0 uint8, 1 int32) on one grid and every class c in [0, C), with
 *   S_c(L) = the voxels of class c that have a face neighbour (6 for nd = 3, 4 for nd = 2, which needs D = 1) outside the class or the volume:
 *   hist (B, C, 2, bins) int32, bins = pulpo_surface_distances_bins(D, H, W) = (D-1)^2 + (H-1)^2 + (W-1)^2 + 1: [b][c][0][k] = the number of
 *   voxels of S_c(a) whose squared distance to S_c(b) is k, [b][c][1][k] the mirror (nullable: then it lives in ws);
 *   out (B, C, 5) fp32 = HD, HDq (q in [0, 100], linear interpolation between order statistics, in double), ASSD, |S_c(a)|, |S_c(b)|;
 *   HD, HDq, ASSD are NaN where either surface is empty (the counts in out are fp32: exact up to 2^24).  ws:
 *   pulpo_surface_distances_ws_bytes(B, C, D, H, W) bytes, in this order - the counts (B, C, 2) int32 = |S_c(a)|, |S_c(b)|, exact, left there for
 *   the caller; the distance planes of one chunk of classes (a size fixed by B and the volume, not by C); the histograms, which a caller
 *   that passes hist may leave off (ws shorter by 8 B C bins bytes).
 *   *flag = 1 when a label lies outside [0, C) (zeroed here). */
#define PULPO_EDT_INF (1 << 29)
int pulpo_edt_sq(const void* mask, int* out, int B, int D, int H, int W, void* stream);
int64_t pulpo_surface_distances_bins(int D, int H, int W);
size_t pulpo_surface_distances_ws_bytes(int B, int C, int D, int H, int W);
int pulpo_surface_distances(const void* lab_a, const void* lab_b, int ldt, int C, double q, float* out, int* hist /*nullable*/, void* ws, int* flag,
                            int B, int D, int H, int W, int nd, void* stream);

/* ------------------------------------------------------------------------- training augmentation (added within ABI 8: nothing else changed)
 * No counterpart in the reference, whose datasets hand out raw pairs; DESIGN.md section 3p holds the definitions.
 * Spatial map of an output voxel v of the grid (D,H,W): q = v + e(v), p = c + M (q - c) + t with theta (B,3,4) = [M | t] as for the affine
 *   operators (NULL: the identity); e = the cubic B-spline free-form deformation of the control lattice phi (B,3,Gz,Gy,Gx), voxel displacements,
 *   integer spacing s >= 2 voxels, G = ceil((S - 1) / s) + 3 per axis (NULL: e = 0).  A depth-1 grid is the 2-D form: Gz = 1, no depth coordinate.
 * Sampler, in voxel units: images and masks trilinear at p with corners outside the volume contributing `fill`
 *   (grid_sample(align_corners=True, padding_mode="zeros") for fill = 0); label maps at floor(p + 0.5) per axis, fill_label outside.
 * pulpo_augment_apply: one launch for up to three sources of a sample on the grid (D,H,W), each with an output of its own shape - img (B,C,..)
 *   fp32, mask (B,Cm,..) fp32, labels (B,1,..) (ldt 0 uint8, 1 int32); any may be NULL, not all.  The image alone goes through the intensity
 *   transform, in this order, each piece present when its bit of iflags is set: 1 r = clamp(r,0,1)^gamma; (bias non-NULL) r *= exp(beta(v)),
 *   beta = the trilinear interpolation of the lattice bias (B,Lz,Ly,Lx) whose end nodes sit on the volume's end voxels (at most 4096 nodes);
 *   2 r = gain r + offset; 4 r += sigma n(i); 8 r = clamp(r,0,1).  iparams (B,4) = gamma, gain, offset, sigma per sample.  n(i): a standard
 *   normal that is a pure function of the seed (one int64 ON THE DEVICE) and the element's linear index i in the planar output - Philox4x32-10
 *   with counter (i >> 2, 0) and key = the seed's halves, Box-Muller on the word pair of lane i & 3.  No atomics: the same bits on every call.
 * pulpo_bspline_field: out (B,3,D,H,W) planar = e, or p - v when theta is given; the fused kernel's coordinates bit for bit.
 * pulpo_philox4x32: out (n,4) = Philox4x32-10 of counters (n,4) under key (2 words), all int32 bit patterns on the device. */
int pulpo_augment_apply(const float* theta, const float* phi, int spacing, int Gz, int Gy, int Gx, const float* img, float* img_out, int C,
                        const float* mask, float* mask_out, int Cm, const void* labels, void* labels_out, int ldt, const float* iparams, int iflags,
                        const float* bias, int Lz, int Ly, int Lx, const void* seed, float fill, int fill_label, int B, int D, int H, int W,
                        void* stream);
int pulpo_bspline_field(const float* phi, const float* theta, float* out, int spacing, int Gz, int Gy, int Gx, int B, int D, int H, int W, void* stream);
int pulpo_philox4x32(const void* counters, const void* key, void* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------- cubic B-spline interpolation (added within ABI 8: nothing else changed)
 * No counterpart in the reference, whose SpatialTransformer stores `mode` and resamples trilinearly; DESIGN.md section 3t holds the definition:
 * scipy.ndimage's order-3 spline, mode="mirror", at the deformable warp's clamped sample coordinate (csrc/sampling.h).  fp32, planar.
 * pulpo_bspline_prefilter: coef = the interpolating coefficients of `planes` volumes img (D,H,W), out of place: per axis of N >= 2 samples the
 *   solution of s[k] = (coef[m(k-1)] + 4 coef[k] + coef[m(k+1)]) / 6 with the whole-sample mirror m (period 2 (N - 1)), by the recursive filter
 *   of pole sqrt(3) - 2 and gain 6; an axis of one sample is left alone (= scipy.ndimage.spline_filter(order=3, mode="mirror")).
 * pulpo_warp3d_cubic_fwd: out (B,C,Dg,Hg,Wg) = per voxel and axis, with pulpo_warp3d_fwd's coordinate c (clamped to [0, Si - 1]), i = floor(c),
 *   f = c - i: the tensor-product sum over the taps m(i - 1 + l), l = 0..3, of B_l(fz) B_l(fy) B_l(fx) coef (B,C,Di,Hi,Wi); a depth-1 grid is
 *   the 2-D form (16 taps).  coef is pulpo_bspline_prefilter of the image; the result may leave the image's range (overshoot).
 * pulpo_warp3d_cubic_bwd: gdf (B,3,Dg,Hg,Wg) = the gradient with respect to df given gout (B,C,Dg,Hg,Wg): the same gather with B'_l along
 *   the axis, times d c / d df (0 where the coordinate was clamped).  Every element written, no atomics: the same bits on every call.  The
 *   coefficients are data (no gradient with respect to the image). */
int pulpo_bspline_prefilter(const float* img, float* coef, int planes, int D, int H, int W, void* stream);
int pulpo_warp3d_cubic_fwd(const float* df, const float* coef, float* out, int B, int C, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, void* stream);
int pulpo_warp3d_cubic_bwd(const float* df, const float* coef, const float* gout, float* gdf, int B, int C, int Dg, int Hg, int Wg, int Di, int Hi,
                           int Wi, void* stream);

/* --------------------------------------------------------------------------------------------------- optimizer
 * torch.optim.Adam(lr) defaults (src/models.py:398-400) over a flat fp32 arena; gscale pre-multiplies the gradient.  beta1, beta2 are doubles
 * (since ABI 8): 1 - beta and 1 - beta^step are formed in double. */
int pulpo_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2, float eps, int step, float gscale,
                    void* stream);
/* Adam over a flat arena of velocity fields with a Gaussian anchor (instance-specific refinement; added without a
 * version bump).  With a = prec ? prec[e] : 1 and d = p[e] - mean[e], the gradient used is g[e] + a d and the blocks' partials receive
 * 0.5 a d^2 (the anchor's value before the update); then pulpo_adam_step's update.  mean NULL: plain Adam, bit-identical to pulpo_adam_step
 * with gscale = 1; prec needs mean.  Every non-null array 16-byte aligned.  partial (nullable): pulpo_loss_blocks(n) floats, all written when
 * mean is given; finish with pulpo_colsum.  One launch, no float atomics. */
int pulpo_anchored_adam_step(float* p, const float* g, float* m, float* v, const float* mean, const float* prec, int64_t n, float lr, double beta1,
                             double beta2, float eps, int step, float* partial, void* stream);

/* ------------------------------------------------------------------------- Winograd F(2x2x2,3x3x3): the deep layers (since ABI 3)
 * The same convolution (src/network_blocks.py:23, forward and data gradient) with minimal filtering along z, y AND x: 64 products per 2x2x2
 * output block instead of 216 (1.5x fewer matrix instructions than the (y, x) form above), all fp32, coefficients +-1 and 1/2 (results differ
 * from the direct kernel by fp32 rounding only).  pulpo_conv3d_k3_algo() answers 3 for the shapes it takes: whole 4x8x8 tiles (D % 4 == 0,
 * H % 8 == 0, W % 8 == 0) of a volume of at least 20^3 voxels (where pulpo_conv3d_k3_stat_tiles() counts 4-deep tiles too), K % 8 == 0 and
 * K >= 16 (two 8-channel chunks: the entry point refuses fewer), N % 4 == 0 and N >= 16 (cout tiles of 32, the last one may be partly empty), at
 * least 256 (tile, cout tile) work items; operands channels-last and 16-byte aligned (the caller guarantees that; the entry point refuses
 * anything else).  stats / part: pulpo_conv3d_k3_stat_tiles(B, D, H, W) rows of 2 * N floats, one row per 4x8x8 tile.  Own weight packing
 * (kind 4 of PulpoPackJob); stats / coef / bias and the _bnred form as for the (y, x) kernel. */
size_t pulpo_conv3d_k3_packed_wino3_floats(int K, int N);
int pulpo_conv3d_k3_pack_weight_wino3(const float* w /*[Cout][Cin][3][3][3]*/, float* wp, int Cin, int Cout, int dgrad, void* stream);
int pulpo_conv3d_k3_fwd_wino3(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, const float* bias, const float* coef,
                              float slope, float* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, float* stats, int B, int D, int H, int W, int K,
                              int N, void* stream);
int pulpo_conv3d_k3_dgrad_wino3_bnred(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, float* out, int64_t out_bs,
                                      int64_t out_ps, const float* bn_y, int64_t bn_y_bs, int64_t bn_y_ps, const float* bn_coef, float slope, float* part,
                                      int B, int D, int H, int W, int K, int N, void* stream);
/* Which form of a kernel a channel pair runs (read-only, added without a version bump; the launchers decide through it).  kind 0: the forward /
 * data-gradient F(2x2x2,3x3x3) entries above with K reduction and N output channels - 1: the 16-column form on v_mfma_f32_16x16x4_f32 (N == 16:
 * the feedback layers' data gradient), 0: 32-wide cout tiles.  kind 1: the F(2x2x2,3x3x3) weight gradient (pulpo_conv3d_k3_wgrad_algo() == 3) with
 * K = Cin, N = Cout - 1: the workgroups of the last ci tile run the 16-input-channel form (Cin % 32 == 16), 0: 32-channel tiles only.  Same packs,
 * same operands, same results to fp32 rounding.  Other kinds: 0. */
int pulpo_conv3d_k3_narrow16(int kind, int K, int N);
/* The same F(2x2x2,3x3x3) convolution as 64 batched GEMMs in the transformed domain (added without a version bump), for the coarse pyramid
 * levels whose extents are not whole 4x8x8 tiles (20^3, 10^3): an input transform writes V[64][rows][K] (one row per 2x2x2 output block, rows
 * padded to 128), a batched MFMA GEMM forms M[p] = V[p] U[p] with U = the pack of pulpo_conv3d_k3_pack_weight_wino3 read as it is, an output
 * transform stores the result through its strides with the bias and either the BatchNorm partials (stats: pulpo_conv3d_k3_stat_tiles() rows of
 * 2 * N floats, every row written) or the eval-mode store (coef).  No atomics.  Takes even D, H, W, K % 8 == 0, N % 4 == 0 and any operand /
 * result strides; scratch: pulpo_conv3d_k3_fwd_wino3g_scratch_floats() floats, 16-byte aligned, any content.  pulpo_conv3d_k3_wino3g_ok() = 1
 * for the shapes the host routes here by default - fp32, pulpo_conv3d_k3_algo() == 2, N % 32 == 0, 125 .. 1000 output blocks,
 * min(K, N) >= 128; pulpo_conv3d_k3_algo() keeps answering 2 for them (pulpo_conv3d_k3_fwd_wino2 still takes them). */
int pulpo_conv3d_k3_wino3g_ok(int B, int D, int H, int W, int K, int N);
size_t pulpo_conv3d_k3_fwd_wino3g_scratch_floats(int B, int D, int H, int W, int K, int N);
int pulpo_conv3d_k3_fwd_wino3g(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* wp, const float* bias, const float* coef,
                               float slope, float* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, float* stats, float* scratch, int B, int D,
                               int H, int W, int K, int N, void* stream);

/* ------------------------------------------------------------------------- bf16 ACTIVATION STORAGE (BASELINE configs 4-5; since ABI 3)
 * No counterpart in the reference (fp32 throughout).  On top of the bf16-operand convolutions the multi-channel activation
 * tensors of a ConvUnit - the pre-norm output y (src/network_blocks.py:23), the output z (:25), pooled / concatenated / up-sampled feature
 * maps (components/pulpo.py:58, 195-206, 250) - and their gradients may live in HBM as bf16: every kernel below computes in fp32 and
 * rounds to nearest even on the store; BatchNorm statistics describe the tensor AS STORED, and so do the conv-bias gradient rows (partial2) of
 * the second BatchNorm-backward pass: the column sums of the dy it stores.  These are the typed forms of the entry points
 * above: activation operands are `void*` with a dtype code (0 = fp32, 1 = bf16), strides in ELEMENTS, everything else (coefficients,
 * partial sums, planar fields, parameters) stays fp32; with code 0 they are the fp32 entry points.  The convolution and weight-gradient
 * kernels take operand and result in ONE storage type (dt). */
int pulpo_conv3d_k3_fwd_bf16_t(const void* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const uint16_t* wp, const float* bias, void* out,
                               int64_t out_bs, int64_t out_ps, int64_t out_cs, int dt, float* stats, float* scratch, int B, int D, int H, int W,
                               int K, int N, void* stream);
int pulpo_conv3d_k3_fwd_bn_lrelu_bf16_t(const void* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const uint16_t* wp, const float* bias,
                                        const float* coef, float slope, void* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, int dt,
                                        float* scratch, int B, int D, int H, int W, int K, int N, void* stream);
int pulpo_conv3d_k3_wgrad_bf16_t(const void* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const void* dy, int64_t dy_bs, int64_t dy_ps,
                                 int64_t dy_cs, int dt, float* dw, int accumulate, float* scratch, int B, int D, int H, int W, int Cin, int Cout,
                                 void* stream);
/* Which kernel the two launchers above pick (read-only queries, added without a version bump), for 16-byte-aligned channels-last operands
 * (channel stride 1, batch stride = D*H*W * voxel stride) with the given voxel strides in elements:
 *  - forward (also the fused eval-mode store and the data gradient, which are the same entry with another pack): 0 the staged kernel on
 *    2x8x8 tiles, 1 the staged kernel on 4x8x8 tiles (D % 4 == 0 and at least 40^3 voxels), 2 the persistent pw<1,9> (32-cout tiles),
 *    3 the persistent pw<2,3> (64-cout tiles); + 16 with split-K (pulpo_conv3d_k3_fwd_bf16_scratch_floats() > 0).  The persistent kernel
 *    takes dt = 1, whole 4x8x8 tiles, K % 32 == 0, whole cout tiles, voxel strides in 16-byte pieces and tensors below 2 GB per batch element.
 *  - weight gradient: ntw (1, 2, 4 or 7 row tiles per wave) + 16 tr (transposing LDS reads, Cin % 16 == 0) + 32 pf (register-prefetched
 *    staging: tr, dt = 1, channels and voxel strides in 16-byte pieces, H % 8 == 0, W % 8 == 0, tensors below 2 GB per batch element).
 * -1 for a bad argument. */
int pulpo_conv3d_k3_fwd_bf16_kernel(int B, int D, int H, int W, int K, int N, int dt, int64_t in_ps, int64_t out_ps);
int pulpo_conv3d_k3_wgrad_bf16_kernel(int B, int D, int H, int W, int Cin, int Cout, int dt, int64_t in_ps, int64_t dy_ps);
int pulpo_bn_lrelu_apply_t(const void* y, int y_dt, int64_t yps, void* z, int z_dt, int64_t zps, const float* coef, int64_t npix, int C, float slope,
                           void* stream);
int pulpo_bn_lrelu_apply_pool2_t(const void* y, int y_dt, int64_t yps, void* z /* nullable since ABI 4: only the pooled tensor is written */, int z_dt, int64_t zps,
                                 void* pooled /* z_dt */, int64_t pps,
                                 const float* coef, int B, int D, int H, int W, int C, float slope, void* stream);
int pulpo_bn_lrelu_bwd_reduce_t(const void* dz, int dz_dt, int64_t dzps, const void* y, int y_dt, int64_t yps, const float* coef, int64_t npix, int C,
                                float slope, float* partial, void* stream);
int pulpo_bn_lrelu_bwd_apply_t(const void* dz, int dz_dt, int64_t dzps, const void* y, int y_dt, int64_t yps, const float* coef, const double* totd,
                               void* dy /* y's dtype */, int64_t dyps, int64_t npix, int C, float slope, float* partial2, void* stream);
int pulpo_avgpool2_bwd_bnred_t(const void* gout, int64_t gops, const void* add, int64_t aps, void* gin, int64_t gips, int g_dt /* gout, add, gin */,
                               const void* y, int y_dt, int64_t yps, const float* coef, float slope, float* partial, int B, int D, int H, int W,
                               int C, void* stream);
int pulpo_heads_fwd_t(const void* h, int h_dt, int64_t ps, const float* Wt, const float* bias, const float* eps, float* o0, float* o1, float* o2,
                      int nout, int B, int64_t V, int C, void* stream);
int pulpo_heads_bwd_t(const void* h, int h_dt, int64_t ps, const float* Wt, const float* g0, const float* g1, const float* g2, const float* eps,
                      const float* sigma, void* dh /* h's dtype */, int64_t dps, float* partial, int nout, int B, int64_t V, int C, void* stream);
int pulpo_avgpool2_fwd_t(const void* in, int64_t ips, void* out, int64_t ops, int dt, int B, int D, int H, int W, int C, void* stream);
int pulpo_avgpool2_bwd_t(const void* gout, int64_t gops, const void* add /* nullable */, int64_t aps, void* gin, int64_t gips, int dt, int B, int D,
                         int H, int W, int C, void* stream);
int pulpo_feedback_up2_fwd_t(const float* const* srcs /*host array of device ptrs, planar fp32*/, const int* chans /*host*/, int nsrc, void* out,
                             int dt, int64_t ops, int B, int Di, int Hi, int Wi, void* stream);
int pulpo_feedback_up2_bwd_t(const void* gout, int dt, int64_t gops, float* const* gsrcs /*host array, entries may be NULL*/, const int* chans,
                             int nsrc, int B, int Di, int Hi, int Wi, void* stream);

/* ------------------------------------------------------------------------- input-layer weight gradient with the unit's BatchNorm backward fused (since ABI 4)
 * The ConvUnit of the image pair (src/network_blocks.py:22-26 as down_blocks[0]._op[0], components/pulpo.py:26): nobody needs its data gradient, so
 * the gradient dy of its pre-norm tensor has ONE reader - this weight gradient.  The kernel forms dy = batch_norm_backward(leaky_relu_backward(dz))
 * per element while it stages its tiles (pulpo_bn_lrelu_bwd_apply's arithmetic from the same coefficient block and totals), so the pass that
 * writes dy is not run.  part2: pulpo_conv3d_k3_wgrad_bn_rows() rows of Cout floats - the column sums of dy (conv-bias gradient partials).
 * Cin <= 4, Cout % 4 == 0; dz fp32 or bf16 (dz_dt), y fp32, channels-last.  scratch / dw / accumulate as pulpo_conv3d_k3_wgrad. */
int pulpo_conv3d_k3_wgrad_bn_rows(int B, int D, int H, int W, int Cout);
int pulpo_conv3d_k3_wgrad_bn(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const void* dz, int dz_dt, int64_t dz_bs, int64_t dz_ps,
                             const float* y, int64_t y_bs, int64_t y_ps, const float* coef, const double* totd, float slope, float* dw,
                             int accumulate, float* scratch, float* part2, int B, int D, int H, int W, int Cin, int Cout, void* stream);

/* ------------------------------------------------------------------------- BatchNorm backward of a POOLED ConvUnit output without its gradient tensor (since ABI 4)
 * DownPath pools the output z of every level's last ConvUnit (components/pulpo.py:58: avg_pool3d, ceil mode) and may also use it as a skip
 * connection.  dz = (skip gradient +) avg_pool3d_backward(gradient of the pooled tensor) is formed per element inside BOTH passes of the unit's
 * batch_norm_backward + leaky_relu_backward: pulpo_avgpool2_bwd_bnred_t with gin == NULL (first pass) and this entry point (second pass). */
int pulpo_bn_lrelu_bwd_apply_pooled_t(const void* gout, int64_t gops, const void* add /*nullable*/, int64_t aps, int g_dt, const void* y, int y_dt,
                                      int64_t yps, const float* coef, const double* totd, void* dy /* y's dtype */, int64_t dyps, float slope,
                                      float* partial2, int B, int D, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------- CHANNEL-BLOCKED gradient of the pre-norm tensor (since ABI 5)
 * Replaces nothing in the reference: inside aten::native_batch_norm_backward -> aten::convolution_backward (src/network_blocks.py:23-25) the gradient
 * dy of a ConvUnit's pre-norm tensor has exactly two readers, the unit's data- and weight-gradient convolution, so its layout is this library's own
 * business.  Channels-last, a staging item of the F(2x2x2,3x3x3) data-gradient kernel gathers 32 useful bytes from each of four 128-byte voxel
 * lines per 8-channel chunk; blocked - element (b, voxel v, channel c) at  p + b * bs + (c / 8) * kb + v * ps + c % 8  floats with ps = 8,
 * bs = D*H*W * 8, kb = B * D*H*W * 8, i.e. [C / 8][B][D][H][W][8] - the four taps are 128 consecutive bytes (32 -> 32 at 160^3: 0.94 -> 0.80 ms,
 * profiles/r5_blocked_probe.txt).  kb = 8 with ps = the row pitch addresses an ordinary channels-last tensor through the same entry points.
 *  - pulpo_bn_lrelu_bwd_apply_kb_t / _pooled_kb_t: the second BatchNorm-backward pass (pulpo_bn_lrelu_bwd_apply_t / _pooled_t) writing dy blocked;
 *    fp32 y / dy, C % 8 == 0.
 *  The same holds for the activation z BETWEEN two ConvUnits of a ConvSequence (src/network_blocks.py:40-46: read by the next unit's convolution,
 *  forward and weight gradient, and by nothing else) and for its gradient dz:
 *  - pulpo_bn_lrelu_apply_kb: the BatchNorm + LeakyReLU pass writing z blocked; the *_kb convolution entries take it (in_kb) and write the gradient dz
 *    blocked (out_kb); pulpo_bn_lrelu_bwd_apply_kb_t (dzkb) and, for the input layer, pulpo_conv3d_k3_wgrad_bn_kb (dz_kb) read it.
 *  - pulpo_conv3d_k3_fwd_wino3_kb / pulpo_conv3d_k3_dgrad_wino3_bnred_kb: pulpo_conv3d_k3_fwd_wino3 / _dgrad_wino3_bnred on a blocked operand
 *    (result channels-last); same shape contract (pulpo_conv3d_k3_algo == 3).
 *  - pulpo_conv3d_k3_wgrad_kb: pulpo_conv3d_k3_wgrad (slabs == NULL) / pulpo_conv3d_k3_wgrad_det on a blocked dy; shapes with
 *    pulpo_conv3d_k3_wgrad_algo(...) == 3 only (the entry point refuses others). */
int pulpo_bn_lrelu_apply_kb(const float* y, int64_t yps, float* z, int64_t zps, int64_t zkb, const float* coef, int64_t npix, int C, float slope, void* stream);
int pulpo_bn_lrelu_bwd_apply_kb_t(const void* dz, int dz_dt, int64_t dzps, int64_t dzkb, const float* y, int64_t yps, const float* coef, const double* totd,
                                  float* dy, int64_t dyps, int64_t dykb, int64_t npix, int C, float slope, float* partial2, void* stream);
int pulpo_conv3d_k3_wgrad_bn_kb(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* dz, int64_t dz_bs, int64_t dz_ps, int64_t dz_kb,
                                const float* y, int64_t y_bs, int64_t y_ps, const float* coef, const double* totd, float slope, float* dw, int accumulate,
                                float* scratch, float* part2, int B, int D, int H, int W, int Cin, int Cout, void* stream);
int pulpo_bn_lrelu_bwd_apply_pooled_kb_t(const void* gout, int64_t gops, const void* add /*nullable*/, int64_t aps, int g_dt, const float* y, int64_t yps,
                                         const float* coef, const double* totd, float* dy, int64_t dyps, int64_t dykb, float slope, float* partial2,
                                         int B, int D, int H, int W, int C, void* stream);
int pulpo_conv3d_k3_fwd_wino3_kb(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_kb, const float* wp, const float* bias, const float* coef,
                                 float slope, float* out, int64_t out_bs, int64_t out_ps, int64_t out_kb, float* stats, int B, int D, int H, int W, int K,
                                 int N, void* stream);
int pulpo_conv3d_k3_dgrad_wino3_bnred_kb(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_kb, const float* wp, float* out, int64_t out_bs,
                                         int64_t out_ps, int64_t out_kb, const float* bn_y, int64_t bn_y_bs, int64_t bn_y_ps, const float* bn_coef, float slope,
                                         float* part, int B, int D, int H, int W, int K, int N, void* stream);
int pulpo_conv3d_k3_wgrad_kb(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_kb, const float* dy, int64_t dy_bs, int64_t dy_ps, int64_t dy_kb,
                             float* dw, int accumulate, float* scratch, float* slabs /*nullable*/, int nslab, int B, int D, int H, int W, int Cin, int Cout,
                             void* stream);

/* ------------------------------------------------------------------------- DETERMINISTIC forms of the backward kernels that add with float atomics (since ABI 4)
 * The reference's CPU backward is run-to-run deterministic; the plain entry points above add the weight-gradient partial sums
 * of concurrent workgroups (aten::convolution_backward, src/network_blocks.py:23) and the image-gradient scatter of grid_sampler_3d_backward
 * (src/network_blocks.py:120, :175) with float atomics, i.e. in arrival order: gradients differ in their last bits from run to run.  These forms
 * give bit-identical results on every run of the same build (pulpo_amd.ops.set_deterministic / PULPO_DETERMINISTIC=1 routes the operators here):
 *  - weight gradient: the same kernels, but workgroups that share a (ci tile, co tile) accumulate into separate zeroed copies ("slabs") of the
 *    packed scratch, which an ordered pass adds up.  slabs: nslab * pulpo_conv3d_k3_wgrad_scratch_floats(Cin, Cout) floats, 16-byte aligned, any
 *    content; nslab = pulpo_conv3d_k3_wgrad_det_slabs(Cin, Cout) (a smaller count is accepted and caps the spatial splits of the grid).
 *  - warp / VecInt backward: every scattered contribution enters a 64-bit fixed-point accumulator (integer adds commute) scaled by the largest
 *    |upstream gradient| of the pass (2^46 units per that maximum), a second pass converts back.  ws: caller-owned workspace of the queried
 *    size, any content.
 *  - F.interpolate backward at ratios other than the exact x2 (src/network_blocks.py:146-150 with other factors, losses.py:313): a gather in fixed
 *    order instead of the scatter. */
int pulpo_conv3d_k3_wgrad_det_slabs(int Cin, int Cout);
int pulpo_conv3d_k3_wgrad_det(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* dy, int64_t dy_bs, int64_t dy_ps,
                              int64_t dy_cs, float* dw, int accumulate, float* scratch, float* slabs, int nslab, int B, int D, int H, int W,
                              int Cin, int Cout, void* stream);
int pulpo_conv3d_k3_wgrad_bf16_det_t(const void* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const void* dy, int64_t dy_bs, int64_t dy_ps,
                                     int64_t dy_cs, int dt, float* dw, int accumulate, float* scratch, float* slabs, int nslab, int B, int D,
                                     int H, int W, int Cin, int Cout, void* stream);
int pulpo_resize_trilinear_scaled_bwd_det(const float* gout, float* gin, int64_t nplanes, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                          float scale_d, float scale_h, float scale_w, float mult, void* stream);
size_t pulpo_warp3d_bwd_det_ws_bytes(int B, int C, int Di, int Hi, int Wi);
int pulpo_warp3d_bwd_det(const float* df, const float* img, const float* gout, float* gdf /*nullable*/, float* gimg /*nullable*/,
                         void* ws /*nullable when gimg is*/, int B, int C, int Dg, int Hg, int Wg, int Di, int Hi, int Wi, void* stream);
size_t pulpo_vecint_bwd_det_ws_bytes(int B, int D, int H, int W, int nsteps);
int pulpo_vecint_bwd_det(const float* work, const float* gout, float* gin, void* ws /*nullable if the query is 0*/, int B, int D, int H, int W,
                         int nsteps, void* stream);

/* ------------------------------------------------------------------------- weight gradient under a WORKGROUP BUDGET (added within ABI 5: nothing else changed)
 * pulpo_conv3d_k3_wgrad / _det / _kb with one more argument.  The Winograd weight-gradient kernels (pulpo_conv3d_k3_wgrad_algo >= 2) run one
 * workgroup per CU and hold it whole; max_workgroups > 0 launches at most that many - never fewer than one per (32-channel ci tile, co tile) pair,
 * and a multiple of 8 where the pair count allows, so that the grid lies evenly on the eight XCDs - which leaves the other CUs to the kernels of
 * another stream (the coarse pyramid levels of the backward pass).  max_workgroups = 0 is the entry point without the suffix;
 * the direct and the input-layer kernels ignore the budget.  Deterministic form: the slab count follows the split count, so results are
 * bit-identical run to run for ONE budget, not across budgets.  pulpo_conv3d_k3_wgrad_grid: the workgroups such a launch takes for vectorisable
 * operands (0: the shape runs no Winograd kernel). */
int pulpo_conv3d_k3_wgrad_grid(int B, int D, int H, int W, int Cin, int Cout, int max_workgroups);
int pulpo_conv3d_k3_wgrad_wg(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* dy, int64_t dy_bs, int64_t dy_ps,
                             int64_t dy_cs, float* dw, int accumulate, float* scratch, int B, int D, int H, int W, int Cin, int Cout, void* stream,
                             int max_workgroups);
int pulpo_conv3d_k3_wgrad_det_wg(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_cs, const float* dy, int64_t dy_bs, int64_t dy_ps,
                                 int64_t dy_cs, float* dw, int accumulate, float* scratch, float* slabs, int nslab, int B, int D, int H, int W,
                                 int Cin, int Cout, void* stream, int max_workgroups);
int pulpo_conv3d_k3_wgrad_kb_wg(const float* in, int64_t in_bs, int64_t in_ps, int64_t in_kb, const float* dy, int64_t dy_bs, int64_t dy_ps, int64_t dy_kb,
                                float* dw, int accumulate, float* scratch, float* slabs /*nullable*/, int nslab, int B, int D, int H, int W, int Cin, int Cout,
                                void* stream, int max_workgroups);

/* ------------------------------------------------------------------------- 1x1x1 heads on the PRE-NORM tensor of the ConvUnit in front of them (added within ABI 5: nothing else changed)
 * The last ConvUnit before a head (src/components/pulpo.py:254 sample_merge_block -> mu_sigma; src/network_blocks.py:77-81 VelocityField's last unit -> its
 * 1x1x1 convolution) produces an activation z = leaky_relu(scale * y + shift) that only the head reads, and the gradient dz the head returns is read only by
 * that unit's batch_norm_backward.  These entry points form both per element, so neither tensor exists:
 *  - pulpo_heads_fwd_bn_t: pulpo_heads_fwd on (y, coef, slope) - coef is the block pulpo_bn_fwd_finalize wrote; fp32 results bit-identical to
 *    pulpo_bn_lrelu_apply followed by pulpo_heads_fwd (one shared expression, csrc/head_bn.h).
 *  - pulpo_heads_bwd_bn_t: pulpo_heads_bwd (partial: the same rows, pulpo_heads_bwd_blocks of them) AND pulpo_bn_lrelu_bwd_reduce in one pass: bnpart =
 *    [pulpo_heads_bwd_blocks][2][C] rows for pulpo_bn_bwd_finalize.  Nothing of C channels is written.
 *  - pulpo_bn_lrelu_bwd_apply_heads_t / _kb_t: pulpo_bn_lrelu_bwd_apply_t / _kb_t with dz formed from the head's planar operands (g0 for nout 3; g0, g1, g2,
 *    eps, sigma for nout 6, as pulpo_heads_bwd takes them); partial2: pulpo_bn_bwd_blocks(B * V, C) rows of C floats.
 * fp32 activations only (bf16 activation storage keeps the separate passes).  Groups of four channels where C % 4 == 0 and the operands are 16-byte
 * aligned, single channels otherwise (C <= 256: e.g. a channel slice at an odd offset of a wider buffer).  Run-to-run deterministic. */
int pulpo_heads_fwd_bn_t(const float* y, int64_t ps, const float* coef, float slope, const float* Wt, const float* bias, const float* eps /*nullable*/,
                         float* o0, float* o1, float* o2, int nout, int B, int64_t V, int C, void* stream);
int pulpo_heads_bwd_bn_t(const float* y, int64_t ps, const float* coef, float slope, const float* Wt, const float* g0, const float* g1, const float* g2,
                         const float* eps, const float* sigma, float* partial /*[blocks][nout*C+nout]*/, float* bnpart /*[blocks][2][C]*/, int nout, int B,
                         int64_t V, int C, void* stream);
int pulpo_bn_lrelu_bwd_apply_heads_t(const float* y, int64_t yps, const float* coef, const double* totd, float slope, const float* Wt, const float* g0,
                                     const float* g1, const float* g2, const float* eps, const float* sigma, float* dy, int64_t dyps, float* partial2,
                                     int nout, int B, int64_t V, int C, void* stream);
int pulpo_bn_lrelu_bwd_apply_heads_kb_t(const float* y, int64_t yps, const float* coef, const double* totd, float slope, const float* Wt, const float* g0,
                                        const float* g1, const float* g2, const float* eps, const float* sigma, float* dy, int64_t dyps, int64_t dykb,
                                        float* partial2, int nout, int B, int64_t V, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PULPO_HIP_H */
