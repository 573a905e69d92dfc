/*
 * libcwt test and measurement hooks -- NOT part of the drop-in boundary (include/cwt.h).
 *
 * These entry points exist for the parity tests (tests/test_gpu_conv*.py run single convs
 * with forced plans), the timing studies (tools/persist_stamps.py, tools/adapt_stamps.py)
 * and the CU-partition probe.  A reference-side binding never needs them; they are exported
 * by the same libcwt.so so the tests exercise the shipped kernels.
 */
#ifndef CWT_DEBUG_H_
#define CWT_DEBUG_H_
#include "cwt.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Test hook: one exact-fp32 implicit-GEMM conv (CWT_CONV=f32, the training-mode-BN pass) +
 * folded BN (+residual) (+ReLU), NHWC, with the tile (bm x bn in {128x128, 128x64, 64x64}; 0 =
 * automatic) and split-K count (0 = automatic) forced, so every plan can be checked against a
 * reference conv.  precision must be 0 (the bf16x3 plans: cwt_debug_conv_s).  w_packed: device
 * [Co][k][k][Ci]; scale/shift: device [Co]; res: NHWC (pixel stride res_ld) or NULL.
 */
int cwt_debug_conv(cwt_ctx* ctx, const float* x, int N, int Hi, int Wi, int Ci, int x_ld,
                   const float* w_packed, const float* scale, const float* shift, int Co, int k,
                   int stride, int pad, int dil, const float* res, int res_ld, int relu, float* y,
                   int y_ld, int y_off, int bm, int bn, int nsplit, int precision, void* stream);

/*
 * Test hooks of the split-activation conv (conv_x3s.hip).  S-layout = [rows][C/32][64 bf16]:
 * per 32-channel block 32 x hi = bf16_rne(v) then 32 x lo = bf16_rne(v - hi).
 * cwt_debug_split_act: fp32 [P][C] (pixel stride ld) -> S-layout; cwt_debug_unsplit_act the
 * inverse (hi + lo).  cwt_debug_pack_wsplit: weights [Co][k][k][Ci] fp32 -> S-layout rows of
 * K = k*k*Ci in the library's K order.  cwt_debug_conv_s: one conv on S-layout input and
 * weights, folded BN, optional fp32 (res) or S-layout (res_s) residual, ReLU; writes fp32 NHWC
 * y (pixel stride y_ld, channel offset y_off) and/or S-layout ys; bm/bn/nsplit force the plan
 * (0 = automatic); bm = 1000 * variant + rows also forces the kernel form on the tile (the form
 * table of csrc/conv_forms.h: cwt_debug_conv_form says which exist; a pair it does not hold is
 * CWT_EARG; the timing-study forms carry their own tile, which replaces the one named).
 */
int cwt_debug_split_act(cwt_ctx* ctx, const float* x, int64_t P, int C, int ld, void* out, void* stream);
int cwt_debug_unsplit_act(cwt_ctx* ctx, const void* s, int64_t P, int C, float* out, int ld, void* stream);
int cwt_debug_pack_wsplit(cwt_ctx* ctx, const float* w, int Co, int k, int Ci, void* out, void* stream);
int cwt_debug_conv_s(cwt_ctx* ctx, const void* xs, int N, int Hi, int Wi, int Ci, const void* ws,
                     const float* scale, const float* shift, int Co, int k, int stride, int pad,
                     int dil, const float* res, int res_ld, const void* res_s, int relu, float* y,
                     int y_ld, int y_off, void* ys, int bm, int bn, int nsplit, void* stream);
/* The same conv on plain bf16 operands (the CWT_CONV_BF16 kernel): xs bf16 NHWC [N*Hi*Wi][Ci]
 * (Ci % 64 == 0), ws bf16 [Co][K] with K ordered (64-channel block, tap, channel in block),
 * res_s / ys bf16 NHWC [M][Co]. */
int cwt_debug_conv_b16(cwt_ctx* ctx, const void* xs, int N, int Hi, int Wi, int Ci, const void* ws,
                       const float* scale, const float* shift, int Co, int k, int stride, int pad,
                       int dil, const float* res, int res_ld, const void* res_s, int relu, float* y,
                       int y_ld, int y_off, void* ys, int bm, int bn, int nsplit, void* stream);

/* The exact-fp32 conv on the LDS-DMA body (conv_igemm_f32d, the eval-mode exact path of
 * cwt_ctx_set_conv_arith(CWT_CONV_ARITH_F32)): x fp32 NHWC [N][Hi][Wi][Ci] (Ci % 32 == 0,
 * pixel stride Ci), w_packed fp32 [Co][K] in the packed_k order (32-channel block, tap, channel),
 * res fp32 [M][res_ld] or NULL, y fp32 [M][y_ld] at channel offset y_off.  bm / bn / nsplit as
 * cwt_debug_conv_s (bm = 1000 * variant + rows; 0 = the library's plan). */
int cwt_debug_conv_f32d(cwt_ctx* ctx, const float* x, int N, int Hi, int Wi, int Ci, const float* w_packed,
                        const float* scale, const float* shift, int Co, int k, int stride, int pad, int dil,
                        const float* res, int res_ld, int relu, float* y, int y_ld, int y_off, int bm, int bn,
                        int nsplit, void* stream);

/* The same conv at fp32 width on the bf16 matrix cores (conv_igemm_x6, the conv of
 * cwt_ctx_set_conv_arith(CWT_CONV_ARITH_BF16X6)): arguments and layouts as cwt_debug_conv_f32d. */
int cwt_debug_conv_x6(cwt_ctx* ctx, const float* x, int N, int Hi, int Wi, int Ci, const float* w_packed,
                      const float* scale, const float* shift, int Co, int k, int stride, int pad, int dil,
                      const float* res, int res_ld, int relu, float* y, int y_ld, int y_off, int bm, int bn,
                      int nsplit, void* stream);

/* The form table and the plan lookup behind these convs, on the host alone (no context, no device
 * call).  prec: 0 conv_igemm_f32d, 1 _b16, 3 _x3s, 6 _x6.  cwt_debug_conv_form: the kernel form of
 * variant var on tile bm x bn -> out4 = WAVES_M, WAVES_N, NSTG, PF (csrc/conv_forms.h), or
 * CWT_EARG where the table holds no such form.  cwt_debug_conv_plan: the library's plan of the GEMM
 * shape [M][K] x [K][Co] (batch: 0 a direct conv, else the Winograd form's GEMM count with M its
 * tiles) -> out5 = bm, bn, var, nsplit, kt_per_split; CWT_EARG if that plan names no form. */
int cwt_debug_conv_form(int prec, int bm, int bn, int var, int* out4);
int cwt_debug_conv_plan(int prec, int M, int Co, int K, int batch, int* out5);

/* The inner loop's launch plan (csrc/adapt_plan.h), on the host alone (no context, no device call;
 * the CWT_ADAPT_* knobs are read from the environment as cwt_inner_adapt reads them).  For E
 * episodes of n shots of h x w features, iters steps, the context's units per workgroup upw
 * (cwt_ctx_set_adapt_units; 0 none) on a device of cu_count CUs -> out8 = persist (1 one persistent
 * launch, 0 the per-step launches: then form is -1 and the rest 0), form (the kernel's NRES, 0..6),
 * G workgroups, units, ncb column blocks per row pair, uc columns per unit, k units per workgroup
 * at most, span episodes a workgroup's units touch at most.
 * cwt_debug_adapt_form: the traits of persistent form 0..6 -> out6 = units in lockstep, episodes a
 * workgroup may span, lock, breg, stream, res1 (PaFormTraits); CWT_EARG for any other form. */
int cwt_debug_adapt_plan(int E, int n, int h, int w, int iters, int upw, int cu_count, int* out8);
int cwt_debug_adapt_form(int form, int* out6);

/* The extractor's plan of one pass (csrc/extract_plan.h), on the host alone: no context, no device
 * call, no loaded backbone (the architecture is csrc/backbone_arch.h's, the operand forms those the
 * loader would build); the CWT_CONV_F32D / CWT_WINO / CWT_FUSE_DOWN / CWT_FUSE_SPLITK_WINO /
 * CWT_PPM_SPLITK knobs are read from the environment as cwt_extract_features reads them.  For a
 * ResNet-`layers` backbone of `precision` (CWT_CONV_FP32 / CWT_CONV_BF16) under a context of
 * `conv_arith` (CWT_CONV_ARITH_*), train_bn != 0 the pass of cwt_extract_features_train_bn, want_mid
 * != 0 that of cwt_extract_features_mid with all three layers: buf (cap bytes, NUL-terminated;
 * CWT_EARG if too small) receives the pass's profile records in the order a pass at profile level 3
 * takes them, one line "level\tname\tflops\tbytes" each (numbers as %.17g; a pass at level L takes the
 * lines of level <= L), then the workspace sizes in floats as lines "ws\tname\tcount", then
 * "form\tppm_gemm\tfew_rows|splitk" (the form of the two PPM GEMMs, which no record names).
 * cwt_debug_extract_mode: the traits of conv family 0..4 (ExtractMode: f32, f32d, x6, x3s, b16) ->
 * out5 = activation layout (0 fp32 NHWC, 1 S-layout, 2 bf16 NHWC), prec, on the LDS-DMA body, every
 * conv writes fp32, bytes per element of the accounting; CWT_EARG for any other mode.
 * cwt_debug_backbone_arch: the architecture's conv + BatchNorm pairs in order, one line
 * "weight name\tBN prefix\tCi\tCo\tk\tstride\tpad\tdil" each. */
int cwt_debug_extract_plan(int layers, int N, int S, int precision, int conv_arith, int train_bn, int want_mid,
                           char* buf, int64_t cap);
int cwt_debug_extract_mode(int mode, int* out5);
int cwt_debug_backbone_arch(int layers, char* buf, int64_t cap);

/* The same conv in the Winograd F(2x2, 3x3) form on the x6 arithmetic (wino.hip; the form the
 * x6 stack takes for stride-1 3x3 layers with Ci >= 256): k == 3, stride 1, pad == dil; the weights
 * are transformed and split on the device each call; bm / bn pick the 16 batched GEMMs' tile
 * (nsplit ignored: the batch fills the chip). */
int cwt_debug_conv_x6w(cwt_ctx* ctx, const float* x, int N, int Hi, int Wi, int Ci, const float* w_packed,
                       const float* scale, const float* shift, int Co, int k, int stride, int pad, int dil,
                       const float* res, int res_ld, int relu, float* y, int y_ld, int y_off, int bm, int bn,
                       int nsplit, void* stream);

/* The x6 extractor's fused conv3 + downsample conv of a bottleneck block, one launch:
 * y [N*Ho*Wo][Co] = [relu]( t . (s3 W3)^T + x(stride2) . (sd Wd)^T + b3 + bd ), the rows folded on the
 * device as cwt_backbone_load does (each product rounded once), then ONE 1x1 GEMM over K1 + K2 whose
 * K-tiles past K1 / 32 read the second source.  t fp32 NHWC [N][Ho][Wo][K1]; x fp32 NHWC
 * [N][Hi2][Wi2][K2], read at (oh, ow) * stride2; w3 [Co][K1], wd [Co][K2]; s3 b3 sd bd [Co].  bm / bn /
 * nsplit as cwt_debug_conv_s: bm = 1000 * variant + rows names the loop (a base variant: 4 or 5), the
 * launch takes its two-source form; a tile without one is CWT_EARG. */
int cwt_debug_conv_x6_dual(cwt_ctx* ctx, const float* t, int N, int Ho, int Wo, int K1, const float* x, int Hi2,
                           int Wi2, int K2, int stride2, const float* w3, const float* s3, const float* b3,
                           const float* wd, const float* sd, const float* bd, int Co, int relu, float* y, int bm,
                           int bn, int nsplit, void* stream);

/* The Winograd input transform alone (wino.hip): V [(m+2)^2][T][C] of the fp32 NHWC map x [N][H][W][C]
 * at dilation d, output tile m (2 or 4).  nsplit > 0: x holds the split-K partial planes
 * [nsplit][N*H*W][C] of the map's producer instead, and the transform reads relu?(fmaf(sum of the
 * planes, scale, shift)) -- the fused form the x6 extractor takes after a split-K conv1.
 * cwt_debug_splitk_epilogue: the fp32 convs' split-K reduction kernel alone, y [M][Co] from part
 * [nsplit][M][Co] (Co % 8 == 0). */
int cwt_debug_wino_in(cwt_ctx* ctx, const float* x, int nsplit, const float* scale, const float* shift, int relu,
                      int N, int H, int W, int C, int d, int m, float* V, void* stream);
int cwt_debug_splitk_epilogue(cwt_ctx* ctx, const float* part, int nsplit, int M, int Co, const float* scale,
                              const float* shift, int relu, float* y, void* stream);

/* One CenterPivotConv4d layer + ReLU (src/model/conv4d.py:40-62) on the channels-last 4-D
 * tensor x [B][hA*wA][hB*wB][cin] -> y [B][hA*wA][hB*wB][cout]: Wa / Wb [cout][cin][3][3] the
 * a-plane / b-plane filters, ba / bb their biases.  variant 0: the library's kernel choice, 1:
 * never the rolling-window kernel (cp4d_roll_kernel), 2: only it (CWT_EARG where it has no form),
 * 3: the channel-chunked kernel of the wide first layer (cp4d_nc_fwd_kernel; cin 1..32, cout 10). */
int cwt_debug_cp4d_layer(cwt_ctx* ctx, const float* x, int B, int hA, int wA, int hB, int wB, int cin, int cout,
                         const float* Wa, const float* ba, const float* Wb, const float* bb, float* y, int variant,
                         void* stream);
/* The layer's input gradient: dx [B][hA*wA][hB*wB][gout] = (accum ? dx : 0) + the transposed, flipped
 * convolutions of g [B][hA*wA][hB*wB][gin] (gin the layer's output channels, gout its input channels;
 * Wa / Wb [gin][gout][3][3] as the forward applied them; no bias, no ReLU).  variant as above:
 * 0 the library's choice, 1 never the rolling window (the tile kernel cp4d_mfma_kernel<gin, 1> where
 * gout = 10), 2 only it, 3 the channel-chunked kernel (cp4d_nc_dgrad_kernel; gin 10, gout 1..32). */
int cwt_debug_cp4d_dgrad(cwt_ctx* ctx, const float* g, int B, int hA, int wA, int hB, int wB, int gin, int gout,
                         const float* Wa, const float* Wb, float* dx, int accum, int variant, void* stream);
/* The layer's weight and bias gradients as cwt_match_corr_backward launches them: x [B][hA*wA][hB*wB][cin]
 * the layer's input, gm [B][hA*wA][hB*wB][cout] its ReLU-masked output gradient; dWa / dWb [cout][cin][3][3]
 * and db1 / db2 [cout] (conv1's and conv2's bias gradients, the same sum) are added into.  The form is the one
 * cwt_debug_cp4d_plan(dir 2) names under the environment at the call (CWT_WGRAD_SCALAR is read per launch);
 * the partial sums live in the context's workspace of cwt_debug_cp4d_wgrad_part_floats() floats. */
int cwt_debug_cp4d_wgrad(cwt_ctx* ctx, const float* x, const float* gm, int B, int hA, int wA, int hB, int wB, int cin,
                         int cout, float* dWa, float* dWb, float* db1, float* db2, void* stream);

/* MutualMatching's backward alone (src/model/match.py:34-53 under autograd): x, dy device [B][NA][NB][C]
 * (channels last, as cwt_mutual_matching) -> dx of that shape.  A row's / column's maximum sends its
 * gradient to the first maximal index, as torch.max(dim) does.  C <= 64. */
int cwt_debug_mutual_matching_bwd(cwt_ctx* ctx, const float* x, const float* dy, int B, int NA, int NB, int C,
                                  float* dx, void* stream);

/* The consensus layer's launch plan (csrc/cp4d_plan.h), on the host alone (no context, no device
 * call; the CWT_CP4D_*, CWT_DGRAD_SCALAR and CWT_WGRAD_SCALAR knobs are read from the environment as
 * every launch reads them).  dir 0 the forward, 1 the input gradient (cin = gin, cout = gout), 2 the
 * weight gradient; variant as cwt_debug_cp4d_layer; cu, occ the device's CUs and the persistent
 * kernel's workgroups per CU (the persistent forms' grid alone depends on them) -> out16 = rc, form
 * (Cp4dForm), the kernel's template arguments cin, cout, mode, pf, the grid x, y, z in workgroups, wc,
 * nsa (rolling window), ntiles, order, dbg (persistent forms), G, n (weight gradient: partials and
 * floats per partial).  Returns rc: 0, or CWT_EARG with the launcher's message for a refused shape.
 * cwt_debug_cp4d_form: form 0..11 -> buf = "name\tkernel\ttemplate arguments" (the plan fields the
 * kernel is instantiated on, comma-separated, in order); CWT_EARG for any other form.
 * cwt_debug_cp4d_wgrad_part_floats: the floats of the weight gradient's partial workspace. */
int cwt_debug_cp4d_plan(int dir, int B, int hA, int wA, int hB, int wB, int cin, int cout, int variant, int cu,
                        int occ, int* out16);
int cwt_debug_cp4d_form(int form, char* buf, int64_t cap);
int cwt_debug_cp4d_wgrad_part_floats(void);

/* The match pass's plan (csrc/match_plan.h), on the host alone (no context, no device call; the
 * CWT_MM_FUSE and CWT_MATCH_BRANCH_STREAMS knobs are read from the environment as every call reads
 * them).  dir 0: the MatchPlan of cwt_match_corr_forward (cv4: of _forward_cv4; train: of
 * _forward_train) with or without the readout (weighted_v); dir 1: the MatchBwdPlan of
 * cwt_match_corr_backward producing d_corr / d_v (want_d_corr, want_d_v) with or without
 * d_weighted_v (readout); cv4 and train are ignored there.  buf (cap bytes, NUL-terminated;
 * CWT_EARG if too small) receives tab-separated lines:
 *   "plan\tfwd\tmm1=direct|planar2|clast\tlayers=cp4d|cv4d\tbranches=N\tfork=0|1\tmm2=plain|add|sum\t
 *    readout=0|1\ttrain=0|1", or "plan\tbwd\tbranches=N\td_corr=0|1\td_v=0|1\treadout=0|1\tclast=0|1";
 *   "param\tlayer\tname\toffset\tfloats" per entry of the packed parameter vector in its order (name
 *    conv1.weight, conv1.bias, conv2.weight, conv2.bias, or weight, bias for cv4), then
 *    "param\ttotal\tfloats"; for the 'red' layers "role\tbranch\tlayer\tWa\tba\tWb\tbb": the offsets of
 *    the filters and biases that branch applies over the a and the b positions;
 *   "buf\ttensor\twhere\toffset\tfloats\tper": where is a workspace's name (offset 0) or "saved" (the
 *    float offset into the caller's buffer), per is "Cv" where floats counts one value channel, else
 *    "1"; a tensor the pass does not have is left out; then, training forward and backward,
 *    "saved\ttotal\tfloats" (= cwt_match_corr_saved_floats).
 * Returns the plan's rc: 0, or CWT_EARG with the entry point's message for a refused call. */
int cwt_debug_match_plan(int dir, int B, int L, int h, int w, int symmetric, int cv4, int train, int readout,
                         int want_d_corr, int want_d_v, char* buf, int64_t cap);

/* Timing-study hook of cwt_episode_tail: with CWT_TAIL_STAMPS=1 in the environment the tail runs a
 * separately compiled instantiation whose workgroups record s_memtime at each phase edge
 * ([G][16]: 0 entry, 2k-1 / 2k before / after grid barrier k, 11 the partials written, 14 / 15
 * s_memrealtime at entry / before the ticket; tools/tail_stamps.py).  Copies up to max_count of
 * the last stamped launch's values to host_out; *count = G * 16 (0 if none). */
int cwt_debug_tail_stamps(cwt_ctx* ctx, unsigned long long* host_out, int64_t max_count, int64_t* count);

/* Timing-study hook: hold nwg CUs for about `us` microseconds (nwg workgroups of 1024 threads, each
 * taking a whole CU's LDS, spinning on the realtime clock with s_sleep, bounded), so a kernel timed
 * on another stream meanwhile sees the CUs the pipeline's resident inner loop leaves it.  nwg <= 256,
 * us <= 100000. */
int cwt_debug_occupy(cwt_ctx* ctx, int nwg, int us, void* stream);

/* Timing-study hook of the inner loop: with CWT_ADAPT_DBG=32 in the environment, the inner
 * loop runs a separately compiled instantiation that records clock stamps per step and
 * workgroup (persistent loop: tools/persist_stamps.py; per-step launches with
 * CWT_ADAPT_PERSIST=0: tools/adapt_stamps.py).  Copies up to max_count of them to host_out
 * (may be NULL) and stores the number available in *count. */
int cwt_debug_adapt_stamps(cwt_ctx* ctx, unsigned long long* host_out, int64_t max_count, int64_t* count);

/* Test hook: the persistent inner loop's per-barrier spin bound on this context (polls before
 * the grid gives up and raises CWT_STATUS_ADAPT_BARRIER); 0 restores the default (~4 s).  A
 * bound of 1 makes nearly every barrier time out, to exercise the error path. */
int cwt_debug_adapt_spin_limit(cwt_ctx* ctx, int64_t limit);

/* Test hooks of the pretraining step's teacher-forced per-block parity test
 * (tests/test_gpu_pretrain_chain.py).  capture != 0: the next cwt_pretrain_step keeps copies of
 * its transient backward gradients ("dlogits" [M][nc], "dcat" [M][2048] = the gradient at
 * layer4's output, "dx:l<layer>.<block>" = a ResNet block's input gradient [M][Ci]).
 * cwt_debug_pretrain_tensor copies one of those, or a forward tensor of the last step
 * ("in:l<layer>.<block>" = a block's input [M][Ci], "a:l<layer>.<block>.c<1|2|3>" = a conv's
 * BN (+ residual) + ReLU output, "a:stem<i>", "a:ppm<i>", "fpre" = the bottleneck's output before
 * Dropout2d, "cat" = layer4's output, "mp" = the stem's max-pool output, "logits" [M][nc]), to
 * host_out (numel floats, NHWC rows). */
int cwt_debug_pretrain_capture(cwt_pretrain* pt, int on);
int cwt_debug_pretrain_tensor(cwt_pretrain* pt, const char* name, float* host_out, int64_t numel);

/* Test hook: per workgroup of a 64-thread grid, the raw HW_REG_HW_ID and HW_REG_XCC_ID of the
 * CU it ran on (out[2*b], out[2*b+1]); with a CU-masked stream this maps mask bits to CUs. */
int cwt_debug_census(cwt_ctx* ctx, int nblocks, unsigned* out, void* stream);

/*
 * CU-partitioned streams (probe of episode pipelining, tools/cu_partition_probe.py): a HIP
 * stream whose kernels (including replays of graphs launched on it) only run on the CUs whose
 * bits are set in mask (mask_words 32-bit words, bit i = CU i of the device).
 * cwt_cu_count returns the device's CU count.
 */
int cwt_cu_count(cwt_ctx* ctx, int* count);
int cwt_stream_create_masked(cwt_ctx* ctx, const uint32_t* mask, int mask_words, void** stream);
int cwt_stream_destroy(void* stream);

/* Single steps of the pretraining iteration on caller buffers (tests/test_gpu_pretrain_ops.py):
 * op 0 conv weight gradient, 1 conv input gradient (b = dy, x | w, out; ia = N Hi Ci Co k stride
 * pad dil; NHWC fp32, weights packed [Co][K] as conv.hip), 2 label-smoothed CE (b = logits
 * [N][h][h][nc], int64 target, dlogits, loss; ia = N S h nc; fa = on off), 3 training BN + ReLU
 * forward and backward (b = y gamma beta out dout dy dgamma dbeta; ia = M C; fa = eps), 4 max
 * pool 3x3 s2 p1 forward and adjoint (b = in out dout din; ia = N H C), 5 the folded PPM field of
 * the bottleneck conv and its adjoint (b = P dF F dP W dW; ia = N h; P [cells][512] bin-major,
 * W / dW packed [512][4096 * 9], only dW's PPM columns written). */
int cwt_debug_pretrain_op(cwt_ctx* ctx, int op, void* const* bufs, const int64_t* iargs, const float* fargs,
                          void* stream);

/* Single kernels of the feature extractor's glue between the convs, on caller buffers
 * (tests/test_gpu_backbone_ops.py).  layout: 0 fp32 NHWC, 1 the S-layout, 2 bf16 NHWC.
 * op 0 the stem's first conv 3 -> 64, 3x3 s2 p1 (b = img [N][3][S][S] fp32, w [27][64], scale, shift,
 * out [N*Ho*Ho][64] in layout; ia = N S layout relu), 1 max pool 3x3 s2 p1 (b = in out, NHWC in layout;
 * ia = N H W C layout), 2 the PPM's adaptive average pooling to bins 1 2 3 6 (b = x in layout,
 * pooled fp32 [50 * N][2048] bin-major; ia = N h w ld layout; ld is the fp32 pixel stride), 3 the
 * PPM's grouped small-M GEMM out_g = A_g * Bt_g^T, * scale_g + shift_g and ReLU where scale_g is not
 * NULL (b = A, Bt0..3, scale0..3, shift0..3, out; ia = M0..3, N, K, kchunk, form; A fp32 [sum M_g][K]
 * and out [sum M_g][N] hold the groups' rows one after another, Bt_g [K][N], scale / shift all four
 * or all NULL; form 0 the MFMA kernel, 1 the split-K kernel with K chunk kchunk (32 or 64), < 0 the
 * extractor's own choice by sum M_g), 4 training-mode BN, in place (b = y in layout, res in the same
 * layout or NULL, bn [4][C] = gamma beta running_mean running_var, scale [C], shift [C], the last
 * three rewritten; ia = M C layout ld res_ld relu rows_per_image seed; fa = eps momentum drop_p;
 * ld / res_ld the fp32 row strides), 5 bf16 -> fp32 widening (b = in out; ia = count). */
int cwt_debug_backbone_op(cwt_ctx* ctx, int op, void* const* bufs, const int64_t* iargs, const float* fargs,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CWT_DEBUG_H_ */
