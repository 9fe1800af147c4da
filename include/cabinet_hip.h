/*
 * cabinet_hip.h -- C ABI of libcabinet_hip.so (gfx950 / MI355X only).
 *
 * Drop-in boundary for the CABiNet hot path.  The reference (dronefreak/CABiNet)
 * is pure Python/PyTorch and has no native interface; each entry point below
 * replaces a span of ATen calls inside a reference nn.Module.forward (cited
 * per function, paths relative to the reference repo) plus the autograd
 * backward of that span.  INTEGRATION.md shows the ctypes binding a reference
 * maintainer would add at those lines.
 *
 * Conventions
 *  - All tensors are dense fp32, NCHW-contiguous, resident on the current HIP
 *    device.  Pointers are borrowed; nothing is retained after the call returns.
 *  - Tensor pointers must be 16-byte aligned: the kernels move rows with 128-bit
 *    loads and stores.  (Any allocator's base pointer is; a view that starts 4 or
 *    8 bytes into an allocation is not -- copy it first.)  The attention, OHEM, FFM,
 *    q/k/v producer, 1x1 / 3x3 convolution and BatchNorm entry points check the
 *    activation and weight pointers they move that way and return
 *    CABINET_ERR_INVALID_ARG for a misaligned one.
 *  - Every call is asynchronous on `stream` (a hipStream_t; NULL = the default
 *    stream).  No call synchronises, allocates device memory or uses a private
 *    stream, so calls are hipGraph-capturable and re-entrant.
 *  - Scratch memory is caller-provided: query the size with the matching
 *    *_workspace_bytes() and pass a buffer at least that large (256-byte
 *    aligned).  A too-small buffer is an error, never an overflow.
 *  - Return value: CABINET_OK (0) or a negative CABINET_ERR_* code; the
 *    message for the calling thread is available from cabinet_last_error().
 *    Mirrors how the ATen ops they replace raise RuntimeError on bad
 *    shape/dtype/device.
 */
#ifndef CABINET_HIP_H_
#define CABINET_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CABINET_ABI_VERSION 8

#define CABINET_OK 0
#define CABINET_ERR_INVALID_ARG (-1) /* null pointer, non-positive dim            */
#define CABINET_ERR_UNSUPPORTED (-2) /* shape outside what the kernels implement  */
#define CABINET_ERR_WORKSPACE (-3)   /* workspace missing or too small            */
#define CABINET_ERR_HIP (-4)         /* a HIP runtime call failed                 */

typedef void* cabinet_stream_t; /* hipStream_t */

int cabinet_abi_version(void);
const char* cabinet_last_error(void);

/* ------------------------------------------------------------------------- *
 * CAB attention core: affinity matmul -> softmax over keys -> aggregation.
 * Replaces src/models/cab.py:149-154
 *     attn = torch.bmm(query, key); attn = attn * (key.shape[1] ** -0.5)
 *     attn = F.softmax(attn, dim=-1); context = torch.bmm(attn, value)
 *     context = context.transpose(1, 2).view(B, -1, Hd, Wd)
 * with q,k: (B,Kc,n) and v: (B,Vc,n) being the NCHW-flattened outputs of
 * to_query / psp_key / psp_value (cab.py:137-146) -- no transposes needed.
 *   ctx[b,c,i] = sum_j softmax_j(scale * sum_c' q[b,c',i] k[b,c',j]) v[b,c,j]
 *   lse[b,i]   = log sum_j exp(scale * S[b,i,j])       (saved for backward)
 * The n x n affinity matrix is never written to memory.
 * Instantiated for (Kc,Vc) in {(128,128), (256,128), (64,64)}; n >= 1 arbitrary.  cabinet_cab_attn_supported()
 * answers 1 / 0 for a channel pair; callers route other pairs to their composite path (the fwd / bwd entry points
 * return CABINET_ERR_UNSUPPORTED for them).
 *
 * `precision` selects the matrix arithmetic of the two contractions (same kernel structure, same operand layout trick):
 *   CABINET_PREC_FP32   (0)  v_mfma_f32_32x32x2_f32: exact fp32 products and sums (bit-wise an fma chain).  Default.
 *   CABINET_PREC_BF16X3 (1)  every fp32 operand split into 2 bf16 pieces, 3 bf16 MFMA products per fp32 product
 *                            (~2^-17 relative per product, ~1e-5 per tensor): 5.3x the fp32 matrix rate.  Measured variant.
 *   CABINET_PREC_BF16X6 (2)  3 pieces (fp32's 24-bit significand exactly), 6 products: fp32-level accuracy at 2.7x the rate.
 * The split forms exist for (Kc,Vc) in {(128,128), (64,64)} (cabinet_cab_attn_precision_supported); their workspace
 * also holds the operands re-laid out as bf16 pieces in MFMA operand order (one pack pass per call).
 * ------------------------------------------------------------------------- */
#define CABINET_PREC_FP32 0
#define CABINET_PREC_BF16X3 1
#define CABINET_PREC_BF16X6 2
int cabinet_cab_attn_supported(int Kc, int Vc);
int cabinet_cab_attn_precision_supported(int Kc, int Vc, int precision);
size_t cabinet_cab_attn_fwd_workspace_bytes(int B, int Kc, int Vc, int n, int precision);
int cabinet_cab_attn_fwd(const float* q, const float* k, const float* v, float scale,
                         int B, int Kc, int Vc, int n, int precision,
                         float* ctx /* (B,Vc,n) */, float* lse /* (B,n) */,
                         void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* K1 with the CAB's output projection in its epilogue (round 5).  Replaces src/models/cab.py:149-155, i.e. the span above
 * plus   context = self.project_out(context)   (a bias-free 1x1 convolution, w_out: (Co,Vc) row-major):
 *   glob[b,o,i] = sum_c w_out[o,c] ctx[b,c,i]
 * applied to each 32-query context tile while the kernel still holds it in LDS: one launch instead of two, and ctx only
 * reaches memory when the caller asks for it (ctx != NULL: training saves it for cabinet_cab_attn_bwd and the projection's
 * weight gradient; pass NULL for inference).  fp32 MFMA only.  cabinet_cab_attn_proj_supported() answers 1 for the shapes
 * the fused form takes -- (Kc,Vc) in {(128,128), (64,64)}, n % 4 == 0, Co % 32 == 0, and a (B, n) the forward runs
 * without a key split (every BASELINE configuration with B * n/32 >= ~200 query tiles) -- callers use
 * cabinet_cab_attn_fwd + cabinet_conv1x1_fwd otherwise.  Backward: cabinet_conv1x1_bwd (dctx = w_out^T dglob,
 * dw_out = dglob ctx^T) followed by cabinet_cab_attn_bwd; no new entry point. */
int cabinet_cab_attn_proj_supported(int B, int Kc, int Vc, int Co, int n);
int cabinet_cab_attn_proj_fwd(const float* q, const float* k, const float* v, const float* w_out /* (Co,Vc) */,
                              float scale, int B, int Kc, int Vc, int Co, int n,
                              float* ctx /* (B,Vc,n) or NULL */, float* glob /* (B,Co,n) */, float* lse /* (B,n) */,
                              cabinet_stream_t stream);

/* Backward of the span above (what autograd derives for cab.py:149-154).
 * Recomputes the affinity tiles from q, k and lse; dctx is dL/dctx (B,Vc,n). */
size_t cabinet_cab_attn_bwd_workspace_bytes(int B, int Kc, int Vc, int n);
int cabinet_cab_attn_bwd(const float* dctx, const float* q, const float* k, const float* v,
                         const float* ctx, const float* lse, float scale,
                         int B, int Kc, int Vc, int n,
                         float* dq /* (B,Kc,n) */, float* dk /* (B,Kc,n) */, float* dv /* (B,Vc,n) */,
                         void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Feature Fusion Module.
 * Replaces src/models/cabinet.py:142-153 (FeatureFusionModule.forward) incl.
 * its ConvBNReLU (cabinet.py:42-44):
 *     fcat = cat([fsp, fcp], 1); feat = relu(bn(conv1x1(fcat)))
 *     atten = sigmoid(conv2(relu(conv1(avg_pool(feat))))); return feat*atten + feat
 * fsp: (B,Cs,H,W)  fcp: (B,Cc,H,W)  w_blk: (Co,Cs+Cc)  w1: (Cm,Co)  w2: (Co,Cm)
 * The concat is never materialised.  training != 0: BatchNorm uses batch
 * statistics and updates running_mean / running_var in place (momentum, unbiased
 * variance) exactly like nn.BatchNorm2d; training == 0: running statistics.
 * Saved for backward: z = pre-BN conv output (B,Co,H,W), save_mean / save_invstd
 * (Co), pooled (B,Co) = spatial mean of feat, gate (B,Co) = sigmoid output.
 * Requires Cs, Cc, Co multiples of 32, Cm <= 256.
 * ------------------------------------------------------------------------- */
size_t cabinet_ffm_fwd_workspace_bytes(int B, int Cs, int Cc, int Co, int Cm, int H, int W);
int cabinet_ffm_fwd(const float* fsp, const float* fcp, const float* w_blk,
                    const float* bn_weight, const float* bn_bias,
                    float* running_mean, float* running_var,
                    const float* w1, const float* w2,
                    int B, int Cs, int Cc, int Co, int Cm, int H, int W,
                    int training, float momentum, float eps,
                    float* out, float* z, float* save_mean, float* save_invstd,
                    float* pooled, float* gate,
                    void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

size_t cabinet_ffm_bwd_workspace_bytes(int B, int Cs, int Cc, int Co, int Cm, int H, int W);
int cabinet_ffm_bwd(const float* dout, const float* fsp, const float* fcp, const float* w_blk,
                    const float* bn_weight, const float* bn_bias,
                    const float* w1, const float* w2,
                    const float* z, const float* save_mean, const float* save_invstd,
                    const float* pooled, const float* gate,
                    int B, int Cs, int Cc, int Co, int Cm, int H, int W, int training,
                    float* dfsp, float* dfcp, float* dw_blk, float* dbn_weight, float* dbn_bias,
                    float* dw1, float* dw2,
                    void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Feature Fusion Module with the bilinear upsample of its context input fused in.
 * Replaces src/models/cabinet.py:228-230 + :236 inside CABiNet.forward
 *     low_res_logit_up = F.interpolate(low_res_logit, size=feat_sb.shape[2:], mode="bilinear",
 *                                      align_corners=False)
 *     feat_fuse = self.ffm(feat_sb, low_res_logit_up)
 * fsp: (B,Cs,H,W)   low: (B,Cc,Hl,Wl)  ->  out (B,Co,H,W); the (B,Cc,H,W) upsampled tensor is never
 * materialised.  The 1x1 conv and the resize commute (both linear, different indices), so the Cc part of
 * the conv runs at (Hl,Wl) and is added bilinearly in the GEMM epilogue; backward likewise returns dlow at
 * (Hl,Wl).  Everything else (BN, gate, saved tensors, argument meaning) is as cabinet_ffm_fwd/bwd.
 * `precision` (CABINET_PREC_*, see the attention section) selects the matrix arithmetic of the big product z = W_s . fsp +
 * U(W_c . low): the split-bf16 forms exist for Co % 256 == 0, Cs == 128, (H*W) % 128 == 0, W == 128, Wl == 32 (the model's
 * grid at 1024 x 1024); any other shape runs the exact fp32 MFMA product whatever is asked.
 * ------------------------------------------------------------------------- */
size_t cabinet_ffm_up_fwd_workspace_bytes(int B, int Cs, int Cc, int Co, int Cm, int H, int W, int Hl, int Wl);
int cabinet_ffm_up_fwd(const float* fsp, const float* low, const float* w_blk,
                       const float* bn_weight, const float* bn_bias,
                       float* running_mean, float* running_var,
                       const float* w1, const float* w2,
                       int B, int Cs, int Cc, int Co, int Cm, int H, int W, int Hl, int Wl,
                       int training, float momentum, float eps, int precision,
                       float* out, float* z, float* save_mean, float* save_invstd,
                       float* pooled, float* gate,
                       void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

size_t cabinet_ffm_up_bwd_workspace_bytes(int B, int Cs, int Cc, int Co, int Cm, int H, int W, int Hl, int Wl);
int cabinet_ffm_up_bwd(const float* dout, const float* fsp, const float* low, const float* w_blk,
                       const float* bn_weight, const float* bn_bias,
                       const float* w1, const float* w2,
                       const float* z, const float* save_mean, const float* save_invstd,
                       const float* pooled, const float* gate,
                       int B, int Cs, int Cc, int Co, int Cm, int H, int W, int Hl, int Wl, int training,
                       float* dfsp, float* dlow /* (B,Cc,Hl,Wl) */, float* dw_blk, float* dbn_weight,
                       float* dbn_bias, float* dw1, float* dw2,
                       void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * OHEM cross-entropy fused with the final bilinear upsample (one call per head).
 * Replaces src/models/cabinet.py:240-245 (F.interpolate of the (B,C,Hl,Wl) logits to (H,W), bilinear,
 * align_corners=False) + src/utils/loss.py:51-80 (per-pixel CE with ignore_index, OHEM selection, mean)
 * for the selection branch "at least n_min pixels have loss > thresh" (loss.py:74-75).  The other branch
 * (top-n_min) needs an order statistic: cabinet_ohem_select + the `_bwd_sel` entry points further down, or the unfused path.
 *   fwd : loss_px (B,H,W) per-pixel CE (0 at ignored pixels); per-workgroup partials
 *         blk_cnt[2*i] = #valid, blk_cnt[2*i+1] = #(loss > thresh), blk_sum[i] = sum of those losses,
 *         i < cabinet_ohem_up_blocks(B,H,W); the caller reduces them (and decides the branch)
 *   bwd : dlogits_low (B,C,Hl,Wl) = coef * U^T[ sel * (softmax - onehot) ],  sel = valid & (loss_px > thresh),
 *         coef = upstream_grad / #selected.  Deterministic (no atomics).   C <= 32.
 * labels are int64 (torch.long), (B,H,W), each either ignore_lb or in [0, C).  A label outside that set is the
 * caller's error (F.cross_entropy asserts on it); the forward kernel reports it by writing blk_cnt[2*i] = -2^30 for
 * every workgroup that met one, so the reduced #valid is negative (valid as long as B*H*W < 2^30, W < 2^20).
 * ------------------------------------------------------------------------- */
int cabinet_ohem_up_blocks(int B, int H, int W);
int cabinet_ohem_up_fwd(const float* logits_low, const long long* labels,
                        int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb,
                        float* loss_px, float* blk_sum, int* blk_cnt, cabinet_stream_t stream);
size_t cabinet_ohem_up_bwd_workspace_bytes(int B, int C, int Hl, int Wl, int H, int W);
/* The forward's partials reduced on the device (ABI v4): stats (nheads,3) double = per head [#valid, #(loss > thresh), sum of
 * those losses] from blk_sum (nheads,nblk) and blk_cnt (nheads,nblk,2), nblk = cabinet_ohem_up_blocks(B,H,W).  One launch in
 * place of the caller's own reductions (loss.py:66-75 takes these three numbers to pick its branch and form the mean); a
 * negative #valid reports an out-of-range label (see above).  Fixed summation order: bit-reproducible.                      */
int cabinet_ohem_stats(const float* blk_sum, const int* blk_cnt, int nheads, int nblk, double* stats, cabinet_stream_t stream);
int cabinet_ohem_up_bwd(const float* logits_low, const long long* labels, const float* loss_px,
                        int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb, float coef,
                        float* dlogits_low, void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
/* BOTH loss heads of the step in one launch each way -- src/scripts/train.py:435 `criteria_p(out, lb) + criteria_16(out16, lb)`
 * on the two outputs of cabinet.py:240-245: same labels, same (B,C,Hl,Wl) logits shape, same thresh / ignore_lb.
 *   fwd : loss_px (2,B,H,W), blk_sum (2,nblk), blk_cnt (2,nblk,2): head 0 = logits_low_a, head 1 = logits_low_b; the label tile
 *         is read once and every thread runs the two heads' exp / log chains side by side
 *   bwd : dlogits_low (2,B,C,Hl,Wl); workspace = 2 x the single-head workspace                                              */
int cabinet_ohem_up_pair_fwd(const float* logits_low_a, const float* logits_low_b, const long long* labels,
                             int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb,
                             float* loss_px, float* blk_sum, int* blk_cnt, cabinet_stream_t stream);
size_t cabinet_ohem_up_pair_bwd_workspace_bytes(int B, int C, int Hl, int Wl, int H, int W);
int cabinet_ohem_up_pair_bwd(const float* logits_low_a, const float* logits_low_b, const long long* labels,
                             const float* loss_px, int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb,
                             float coef, float* dlogits_low, void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
/* The same four with per-class weights -- reference loss.py:38-80 with `weight=w`, what src/scripts/train.py:332-349 builds
 * from configs/train.yaml `cls_pw` by default.  class_weight[_a|_b]: (C,) fp32 on the device, non-negative and finite, one
 * table per head (the two criteria own separate buffers); NULL = that head is unweighted, and with every table NULL these
 * ARE the entry points above, bit for bit.  Argument lists = the unweighted ones plus the tables in front of the stream;
 * workspaces are those of cabinet_ohem_up[_pair]_bwd_workspace_bytes.  (Added under ABI v8.)
 *   per-pixel loss  l = w[label] * (lse - x[label])          (F.cross_entropy(weight=w, reduction="none"))
 *   #valid          does not depend on w (a class of weight 0 is still valid)
 *   selection       valid & (l > thresh); #above and the sum are over l; the caller forms sum / #above (a plain mean)
 *   bwd             dlogits_low = coef * U^T[ sel * w[label] * (softmax - onehot) ]; no gradient w.r.t. the weights
 * loss_px between the two passes holds the UNWEIGHTED lse - x[label] (the backward rebuilds lse from it and re-evaluates the
 * selection as w[label] * loss_px > thresh with the forward's own product): hand the backward the forward's tables.        */
int cabinet_ohem_up_w_fwd(const float* logits_low, const long long* labels,
                          int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb,
                          float* loss_px, float* blk_sum, int* blk_cnt, const float* class_weight, cabinet_stream_t stream);
int cabinet_ohem_up_w_bwd(const float* logits_low, const long long* labels, const float* loss_px,
                          int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb, float coef,
                          float* dlogits_low, void* workspace, size_t workspace_bytes, const float* class_weight,
                          cabinet_stream_t stream);
int cabinet_ohem_up_pair_w_fwd(const float* logits_low_a, const float* logits_low_b, const long long* labels,
                               int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb,
                               float* loss_px, float* blk_sum, int* blk_cnt,
                               const float* class_weight_a, const float* class_weight_b, cabinet_stream_t stream);
int cabinet_ohem_up_pair_w_bwd(const float* logits_low_a, const float* logits_low_b, const long long* labels,
                               const float* loss_px, int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb,
                               float coef, float* dlogits_low, void* workspace, size_t workspace_bytes,
                               const float* class_weight_a, const float* class_weight_b, cabinet_stream_t stream);
/* BOTH branches of the criterion with the branch decided ON THE DEVICE -- reference src/utils/loss.py:67-80: `if
 * sorted_loss[n_min] > thresh: keep loss > thresh, else: keep the n_min hardest`, then the mean.  (Added under ABI v8.)
 * Per head, over the valid pixels (label != ignore_lb), l = w[label] * loss_px (the forward's product), k = min(n_min, #valid):
 *   #above >= k : t = thresh,            tie = 0,                      denom = #above, value = sum_above / #above
 *   else        : t = k-th largest l,    tie = (k - #(l > t)) / #(l == t), denom = k,  value = (sum_{l > t} l + (k - #(l > t)) t) / k
 * cabinet_ohem_select: loss_px (nheads,B,H,W) and stats (nheads,3) as the forward and cabinet_ohem_stats left them ->
 *   sel (nheads,4) double = [t, tie, denom, value]; nheads = 1 | 2 (n_min_b, class_weight_b unused for 1).  value is loss.py's
 *   mean of the kept losses.  An MSD radix select over order-preserving keys of l (-0.0 == +0.0); integer histograms and
 *   ordered double sums: bit-reproducible.  k is formed on the device (#valid is data); no host read.  B*H*W < 2^31.
 * cabinet_ohem_up[_pair]_w_bwd_sel: the `_w_bwd` argument lists with `const double* sel` (device) in place of `float thresh`:
 *   dlogits_low = coef * U^T[ f * w[label] * (softmax - onehot) ],  f = 1 (l > t) | tie (l == t) | 0; the caller folds
 *   upstream_grad / denom in.  With a unique k-th value this is loss.py's gradient; where the k-th value is tied the
 *   reference keeps whichever of the tied pixels its sort put first, here the same total weight is spread evenly over them. */
size_t cabinet_ohem_select_workspace_bytes(int nheads, int B, int H, int W);
int cabinet_ohem_select(const float* loss_px, const long long* labels, const double* stats, int nheads,
                        int B, int C, int H, int W, float thresh, int n_min_a, int n_min_b, int ignore_lb,
                        const float* class_weight_a, const float* class_weight_b, double* sel,
                        void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
int cabinet_ohem_up_w_bwd_sel(const float* logits_low, const long long* labels, const float* loss_px,
                              int B, int C, int Hl, int Wl, int H, int W, const double* sel, int ignore_lb, float coef,
                              float* dlogits_low, void* workspace, size_t workspace_bytes, const float* class_weight,
                              cabinet_stream_t stream);
int cabinet_ohem_up_pair_w_bwd_sel(const float* logits_low_a, const float* logits_low_b, const long long* labels,
                                   const float* loss_px, int B, int C, int Hl, int Wl, int H, int W, const double* sel,
                                   int ignore_lb, float coef, float* dlogits_low, void* workspace, size_t workspace_bytes,
                                   const float* class_weight_a, const float* class_weight_b, cabinet_stream_t stream);

/* Softmax focal loss behind the same fused upsample -- reference src/utils/loss.py:86-127 (SoftmaxFocalLoss) on the output of
 * cabinet.py:240-245; the focal mode of the OHEM kernels above.  (Added under ABI v8.)  Every entry point takes one or two heads
 * over the same labels: logits_low_b == NULL means one (gamma_b, class_weight_b are then unused); with two, loss_px is
 * (2,B,H,W), blk_sum (2,nblk,2), blk_cnt (2,nblk), dlogits_low (2,B,C,Hl,Wl), nblk = cabinet_ohem_up_blocks(B,H,W).
 * Per valid pixel (label != ignore_lb), with z the low logits, U the bilinear upsample (align_corners=False), t the label:
 *   l = lse(Uz) - (Uz)_t,  p = exp(-l),  q = 1 - p
 * and per head, w the class weights (NULL = ones; non-negative, finite):
 *   D = sum w_t,  S = sum w_t q^gamma l,  loss = S / D,
 *   a = q^gamma + gamma p q^(gamma-1) l  ( = q^(gamma-1) (q + gamma p l) >= 0 ),
 *   dloss/dz = (g / D) U^T[ w_t a (softmax - onehot) ].
 * Pinned values: q is formed as -expm1(-l), never as 1 - exp(-l); q^0 = 1 also at q = 0 (torch's 0 ** 0); for gamma > 0 and
 * q = 0 the pixel's term and a are 0 -- also for 0 < gamma < 1, where the reference's fp32 autograd returns NaN gradients
 * (0^(gamma-1) * 0); q^(gamma-1) is never formed on its own.  gamma is a run-time value per head: finite and >= 0.
 * cabinet_focal_up_supported: 1, or 0 with the reason in cabinet_last_error() (the limits of the OHEM head: C <= 32, the LDS
 *   row buffers; and gamma).
 * cabinet_focal_up_fwd: loss_px = the UNWEIGHTED l (0 at ignored pixels), and per workgroup, ordered:
 *   blk_sum[blk] = {sum w_t, sum w_t q^gamma l}, blk_cnt[blk] = #valid, or -2^30 when the block met a label outside [0,C)
 *   that is not ignore_lb (such a label is clamped before it indexes anything).
 * cabinet_focal_stats: partials -> stats (nheads,3) double = [n_valid, D, S], fixed summation order; n_valid < 0 = bad label.
 * cabinet_focal_up_bwd: dlogits_low = coef * U^T[ w_t a(loss_px) (softmax - onehot) ] from the forward's loss_px and the same
 *   gamma / weights; a pixel whose factor is 0 is switched off.  The caller folds upstream_grad / D in.  No atomics, ordered
 *   sums: bit-reproducible.  Workspace: cabinet_focal_up_bwd_workspace_bytes(nheads, ...). */
int cabinet_focal_up_supported(int C, int Hl, int Wl, int H, int W, float gamma);
int cabinet_focal_up_fwd(const float* logits_low_a, const float* logits_low_b, const long long* labels,
                         int B, int C, int Hl, int Wl, int H, int W, float gamma_a, float gamma_b, int ignore_lb,
                         float* loss_px, float* blk_sum, int* blk_cnt,
                         const float* class_weight_a, const float* class_weight_b, cabinet_stream_t stream);
int cabinet_focal_stats(const float* blk_sum, const int* blk_cnt, int nheads, int nblk, double* stats, cabinet_stream_t stream);
size_t cabinet_focal_up_bwd_workspace_bytes(int nheads, int B, int C, int Hl, int Wl, int H, int W);
int cabinet_focal_up_bwd(const float* logits_low_a, const float* logits_low_b, const long long* labels,
                         const float* loss_px, int B, int C, int Hl, int Wl, int H, int W, float gamma_a, float gamma_b,
                         int ignore_lb, float coef, float* dlogits_low, void* workspace, size_t workspace_bytes,
                         const float* class_weight_a, const float* class_weight_b, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * CAB local branch + block output.
 * Replaces src/models/cab.py:175-184 (LocalAttention.forward: three DWConv = depthwise 3x3 conv (cab.py:36-45)
 * + BatchNorm2d + ReLU, sigmoid gate, x + x*mask) and, when `glob` is given, cab.py:213-216
 * (ContextAggregationBlock.forward: gamma * global + local).
 *   x, glob, out, dout, dx, dglob : (B,C,H,W).  Two forms behind the same entry points:
 *     B*H*W <= 8192  : one kernel each way, one channel lives in the LDS of one CU, no workspace (..._workspace_bytes = 0)
 *     anything larger: (e.g. B = 16 at 1024^2, or the un-tiled 4096x2160 validation frame of src/scripts/train.py:444-456,
 *                      n = 8704) tiled form, B * ceil(H / rows) workgroups per channel, BatchNorm batch statistics as
 *                      two-phase ordered reductions: 4 launches forward, 8 backward, workspace from ..._workspace_bytes
 *   dw_w[s] (C,9) depthwise weights (C,1,3,3), bn_weight[s] / bn_bias[s] / running_mean[s] / running_var[s] (C),
 *   s = 0..2: HOST arrays of three DEVICE pointers (the three DWConv stages own separate parameter tensors)
 *   gamma : device scalar (cab.py:208); glob == NULL  ->  out = x * (1 + sigmoid(mask)) only (gamma, dglob and
 *           dgamma_part are then ignored and may be NULL)
 *   training != 0 : batch statistics per channel (biased variance for normalisation, unbiased into running_var,
 *           running = (1-momentum)*running + momentum*stat), save_mean / save_invstd (3,C) hold them;
 *           training == 0 : running statistics are used (and copied into save_*).
 *   bwd : recomputes the chain from x (nothing else is saved); writes dx, dglob = gamma*dout,
 *         dgamma_part (C) = per-channel <dout, glob> (caller sums it: d gamma), ddw_w[s] (C,9),
 *         dbn_weight[s], dbn_bias[s] (C).  Deterministic (no atomics).
 * ------------------------------------------------------------------------- */
int cabinet_cab_local_supported(int B, int C, int H, int W);   /* 1 if one of the two forms serves the shape, else 0 */
size_t cabinet_cab_local_fwd_workspace_bytes(int B, int C, int H, int W);   /* 0 for the channel-resident form */
size_t cabinet_cab_local_bwd_workspace_bytes(int B, int C, int H, int W);
int cabinet_cab_local_fwd(const float* x, const float* glob, const float* gamma,
                          const float* const* dw_w, const float* const* bn_weight, const float* const* bn_bias,
                          float* const* running_mean, float* const* running_var,
                          int B, int C, int H, int W, int training, float momentum, float eps,
                          float* out, float* save_mean, float* save_invstd,
                          void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
int cabinet_cab_local_bwd(const float* dout, const float* x, const float* glob, const float* gamma,
                          const float* const* dw_w, const float* const* bn_weight, const float* const* bn_bias,
                          const float* save_mean, const float* save_invstd,
                          int B, int C, int H, int W, int training,
                          float* dx, float* dglob, float* dgamma_part,
                          float* const* ddw_w, float* const* dbn_weight, float* const* dbn_bias,
                          void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * q/k/v producers of the CAB global branch (1x1 projections + BatchNorm + ReLU + pyramid pooling).
 * Replaces src/models/cab.py:137,141,145 with the modules of cab.py:107-123 and PSPModule.forward cab.py:65-76:
 *   q = relu(bn_q(W_q x));  k = PSP_k(relu(bn_k(W_k x)));  v = PSP_v(W_v x)
 *   PSP(u) = W_p . cat[u, U(A_s u) for s in sizes]   (A_s = AdaptiveAvgPool2d((s,s)), U = bilinear resize to
 *   (H,W), align_corners=False); evaluated as W_p[:, :Kc] u + sum_s U(W_p[:, block s] A_s u), no concat.
 *   x (B,C,H,W); wq, wk (Kc,C); wv (Vc,C)  [Conv2d 1x1 weights, no bias]; bn*_ (Kc);
 *   wpk (Kc,(n_sizes+1)*Kc), wpv (Vc,(n_sizes+1)*Vc)  [PSP project weights, identity block first]
 *   sizes: HOST array of n_sizes (1..4) pyramid sizes (each 1..16); C, Kc, Vc multiples of 16; H*W <= ~8192
 *   outputs q, k (B,Kc,H*W), v (B,Vc,H*W) -- the NCHW-flattened operands cabinet_cab_attn_fwd takes
 *   saved for backward (caller-allocated): zqk (B,2Kc,H*W), vv (B,Vc,H*W), kk (B,Kc,H*W),
 *   pooled_k (B,n_sizes*Kc,NBp), pooled_v (B,n_sizes*Vc,NBp) with NBp = cabinet_cab_qkv_padded_bins(),
 *   save_mean / save_invstd (2Kc) = [bn_q | bn_k]
 *   BatchNorm semantics and running-stat updates as in cabinet_ffm_fwd (training flag, momentum, eps).
 *   bwd: dq, dk (B,Kc,H*W), dv (B,Vc,H*W) -> dx, dwqk (2Kc,C) = [dW_q; dW_k], dwv, dbn*, dwpk, dwpv.
 *   Deterministic (no atomics).
 * ------------------------------------------------------------------------- */
int cabinet_cab_qkv_supported(int B, int C, int Kc, int Vc, int H, int W, int n_sizes, const int* sizes);
int cabinet_cab_qkv_padded_bins(int n_sizes, const int* sizes);
size_t cabinet_cab_qkv_fwd_workspace_bytes(int B, int C, int Kc, int Vc, int H, int W, int n_sizes, const int* sizes);
int cabinet_cab_qkv_fwd(const float* x, const float* wq, const float* wk, const float* wv,
                        const float* bnq_weight, const float* bnq_bias, float* bnq_running_mean, float* bnq_running_var,
                        const float* bnk_weight, const float* bnk_bias, float* bnk_running_mean, float* bnk_running_var,
                        const float* wpk, const float* wpv,
                        int B, int C, int Kc, int Vc, int H, int W, int n_sizes, const int* sizes,
                        int training, float momentum, float eps,
                        float* q, float* k, float* v,
                        float* zqk, float* vv, float* kk, float* pooled_k, float* pooled_v,
                        float* save_mean, float* save_invstd,
                        void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
size_t cabinet_cab_qkv_bwd_workspace_bytes(int B, int C, int Kc, int Vc, int H, int W, int n_sizes, const int* sizes);
int cabinet_cab_qkv_bwd(const float* dq, const float* dk, const float* dv, const float* x,
                        const float* wq, const float* wk, const float* wv,
                        const float* bnq_weight, const float* bnq_bias, const float* bnk_weight, const float* bnk_bias,
                        const float* wpk, const float* wpv,
                        const float* zqk, const float* vv, const float* kk, const float* pooled_k,
                        const float* pooled_v, const float* save_mean, const float* save_invstd,
                        int B, int C, int Kc, int Vc, int H, int W, int n_sizes, const int* sizes, int training,
                        float* dx, float* dwqk, float* dwv,
                        float* dbnq_weight, float* dbnq_bias, float* dbnk_weight, float* dbnk_bias,
                        float* dwpk, float* dwpv,
                        void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Bias-free 1x1 convolution, y (B,Co,P) = W (Co,Ci) . x (B,Ci,P), on the exact-fp32 MFMA GEMMs.
 * Replaces src/models/cab.py:155 (project_out of the attention context).  Ci, Co multiples of 4.
 * bwd: dx = W^T dy (skipped if dx == NULL), dw = sum_{b,p} dy (x) x (skipped if dw == NULL).
 * ------------------------------------------------------------------------- */
size_t cabinet_conv1x1_fwd_workspace_bytes(int Ci, int Co);
int cabinet_conv1x1_fwd(const float* x, const float* w, int B, int Ci, int Co, int P, float* y,
                        void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
/* The same with an output bias (`AttentionBranch.convb`, src/models/cabinet.py:65-66, 86: a 1x1 convolution WITH bias on the CAB's
 * output) on the small-grid path (cabinet_conv1x1_bias_supported: the CAB's resolution; larger planes use the stock operator).
 * Backward: cabinet_conv1x1_bwd for dx / dw, cabinet_channel_sum(dy, B, Co, P, dbias) for the bias gradient
 * (dbias[c] = sum over images and positions, one workgroup per channel, fixed order). */
int cabinet_conv1x1_bias_supported(int B, int Ci, int Co, int P);
int cabinet_conv1x1_bias_fwd(const float* x, const float* w, const float* bias /* (Co) */, int B, int Ci, int Co, int P, float* y,
                             void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
int cabinet_channel_sum(const float* d /* (B,C,P) */, int B, int C, int P, float* out /* (C) */, cabinet_stream_t stream);
size_t cabinet_conv1x1_bwd_workspace_bytes(int B, int Ci, int Co, int P);
int cabinet_conv1x1_bwd(const float* dy, const float* x, const float* w, int B, int Ci, int Co, int P,
                        float* dx, float* dw, void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * BatchNorm2d fused with the activation that follows it (NCHW fp32, P = H*W).
 * Replaces the bn -> relu tail of ConvBNReLU.forward, src/models/cabinet.py:42-44, and the same
 * BatchNorm2d -> ReLU / HardSwish pairs at cabinet.py:59-63,67-68 and src/models/mobilenetv3.py:86-99,118-152
 * (HardSwish: x * relu6(x + 3) / 6, mobilenetv3.py:48-50,63-65).
 *   act: 0 = none, 1 = ReLU, 2 = HardSwish.   y = act(weight * xhat + bias) [+ residual], xhat = (x - mean) * invstd
 *   (residual: the identity shortcut `x + self.conv(x)` of an MBConv block, mobilenetv3.py:158, added in the same
 *   pass; its gradient is dy itself, so backward is unchanged)
 *   training != 0: batch statistics (biased variance; unbiased into running_var; running buffers updated with
 *   `momentum`), save_mean / save_invstd (C) receive them; training == 0: running statistics.
 *   bwd needs only x, save_mean, save_invstd (the pre-activation is recomputed):
 *     du = dy * act'(u);  dweight = sum du * xhat;  dbias = sum du;
 *     dx = weight * invstd * (du - mean(du) - xhat * mean(du * xhat))   (training)   or  weight * invstd * du  (eval)
 *   Deterministic (no atomics).  One workspace size serves both directions.
 * ------------------------------------------------------------------------- */
size_t cabinet_bn_act_workspace_bytes(int B, int C, int P);
int cabinet_bn_act_fwd(const float* x, const float* weight, const float* bias,
                       float* running_mean, float* running_var, const float* residual /* nullable, (B,C,P) */,
                       int B, int C, int P, int act, int training, float momentum, float eps,
                       float* y, float* save_mean, float* save_invstd,
                       void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
/* The same forward when x (B,C,H,W) was just produced by cabinet_conv3x3_fwd with `bn_part`: the batch statistics come from
 * those per-block (mean, M2) pairs (Chan-merged in double, as above) and the statistics pass over x is skipped.
 * conv_part: [2][C][cabinet_conv3x3_tile_blocks(B,H,W)] floats; ignored when training == 0. */
int cabinet_bn_act_fwd_part(const float* x, const float* conv_part, const float* weight, const float* bias,
                            float* running_mean, float* running_var, const float* residual /* nullable */,
                            int B, int C, int H, int W, int act, int training, float momentum, float eps,
                            float* y, float* save_mean, float* save_invstd, cabinet_stream_t stream);
int cabinet_bn_act_bwd(const float* dy, const float* x, const float* weight, const float* bias,
                       const float* save_mean, const float* save_invstd,
                       int B, int C, int P, int act, int training,
                       float* dx, float* dweight, float* dbias,
                       void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * BatchNorm2d -> ReLU -> 1x1 classifier convolution as ONE streaming operator (round 5, K12).
 * Replaces the tail of src/models/cabinet.py:156-172 (CABiNetOutput.forward: `self.conv_out(relu(bn(conv(x))))`, behind
 * cabinet_conv3x3_fwd) and of the fusion head, cabinet.py:90-92 (`self.b4(self.b3(self.b2(.)))`):
 *     y[b,k,p] = bias[k] + sum_c w_cls[k,c] * relu(bn_weight[c] * (z[b,c,p] - mean[c]) * invstd[c] + bn_bias[c])
 * z (B,C,H,W): the convolution output in front of the BatchNorm;  w_cls (K,C): the 1x1 classifier;  bias (K) or NULL.
 * The (B,C,H,W) activation and, in backward, its gradient are never written: forward reads z once and writes the K
 * logits; backward reads z and dy twice and writes dz.  training != 0: batch statistics -- from conv_part when given (the
 * (mean, M2) pairs cabinet_conv3x3_fwd left: [2][C][cabinet_conv3x3_tile_blocks(B,H,W)], no statistics pass), else from a
 * pass over z -- and running_mean / running_var updated like nn.BatchNorm2d; training == 0: running statistics.
 * `table` (cabinet_bn_cls_table_floats(C,K) floats) is written by fwd and read by bwd: per channel the classifier column
 * and [mean, invstd, bn_weight, bn_bias, bn_weight * invstd].  Covered: C % 64 == 0, K <= 32, (H*W) % 4 == 0
 * (cabinet_bn_cls_supported).  Deterministic (ordered partial sums, no atomics).
 *   bwd: du = (pre > 0) * sum_k w_cls[k,c] dy[k];  dbn_weight = sum du * xhat;  dbn_bias = sum du;
 *        dz = bn_weight * invstd * (du - mean(du) - xhat * mean(du * xhat))  (training; eval: bn_weight * invstd * du);
 *        dw_cls[k,c] = sum dy[k] * relu(pre);  dbias[k] = sum dy[k]  (dbias may be NULL).
 * ------------------------------------------------------------------------- */
int cabinet_bn_cls_supported(int C, int K, int P);
int cabinet_bn_cls_table_floats(int C, int K);
size_t cabinet_bn_cls_fwd_workspace_bytes(int B, int C, int P);
int cabinet_bn_cls_fwd(const float* z, const float* conv_part /* nullable */, const float* bn_weight, const float* bn_bias,
                       float* running_mean, float* running_var, const float* w_cls /* (K,C) */, const float* bias /* nullable */,
                       int B, int C, int K, int H, int W, int training, float momentum, float eps,
                       float* y /* (B,K,H,W) */, float* table,
                       void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
size_t cabinet_bn_cls_bwd_workspace_bytes(int B, int C, int K, int P);
int cabinet_bn_cls_bwd(const float* dy /* (B,K,H,W) */, const float* z, const float* table,
                       int B, int C, int K, int H, int W, int training,
                       float* dz, float* dbn_weight, float* dbn_bias, float* dw_cls, float* dbias /* nullable */,
                       void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Depthwise KxK convolution (groups == channels, no bias, dilation 1, padding K/2), NCHW fp32.
 * Replaces the depthwise nn.Conv2d of the MBConv blocks, src/models/mobilenetv3.py:118-126,135-143
 * (K in {3,5}, stride in {1,2}); weight is the Conv2d weight (C,1,K,K).
 *   fwd : y (B,C,Ho,Wo), Ho = (H + 2*(K/2) - K)/stride + 1
 *   bwd : dx (B,C,H,W) and dw (C,1,K,K) from dy, x, weight in one pass over dy; deterministic (no atomics)
 * ------------------------------------------------------------------------- */
int cabinet_dwconv_supported(int K, int stride);
int cabinet_dwconv_fwd(const float* x, const float* weight, int B, int C, int H, int W, int K, int stride,
                       float* y, cabinet_stream_t stream);
size_t cabinet_dwconv_bwd_workspace_bytes(int B, int C, int H, int W, int K, int stride);
int cabinet_dwconv_bwd(const float* dy, const float* x, const float* weight, int B, int C, int H, int W, int K,
                       int stride, float* dx, float* dw, void* workspace, size_t workspace_bytes,
                       cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Channel gate + activation: y = act(x * gate[b,c]) for x (B,C,P), gate (B,C); act as in cabinet_bn_act.
 * Replaces the `x * y.view(n, c, 1, 1)` of SELayer.forward, src/models/mobilenetv3.py:79-83, fused with the
 * ReLU / HardSwish that follows it in the MBConv block (mobilenetv3.py:121,141).
 *   bwd: dx = dy * act'(x*gate) * gate,  dgate[b,c] = sum_p dy * act'(x*gate) * x   (x is the only saved tensor)
 * ------------------------------------------------------------------------- */
int cabinet_gate_act_fwd(const float* x, const float* gate, int B, int C, int P, int act, float* y,
                         cabinet_stream_t stream);
size_t cabinet_gate_act_bwd_workspace_bytes(int B, int C, int P);
int cabinet_gate_act_bwd(const float* dy, const float* x, const float* gate, int B, int C, int P, int act,
                         float* dx, float* dgate, void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Backward of the squeeze-excite tail y = act(gate * x), x = bn(z), gate = hsig(W2 relu(W1 avgpool(x) + b1) + b2), of the
 * MBConv blocks `dw -> BatchNorm -> SELayer -> act` (src/models/mobilenetv3.py:146-149, SELayer :68-83) in two passes over
 * (dy, z) instead of the gate, pool, add and BatchNorm backward passes; the forward is cabinet_bn_act_fwd (act 0), the
 * caller's pool and MLP on (B,C), and cabinet_gate_act_fwd.  z (B,C,H,W), P = H*W; mean / invstd as cabinet_bn_act_fwd
 * saved them; gate (B,C).  Deterministic.
 *   reduce : sums [3][B][C] = (sum_p du, sum_p du * xhat, sum_p xhat), xhat = (z - mean) * invstd,
 *            du = dy * act'(gate * (bn_weight * xhat + bn_bias)); and da2 (B,C), the gradient at the hard sigmoid's input
 *            a2 (B,C): (bn_weight * X + bn_bias * A) / 6 where 0 < a2 + 3 < 6, else 0.
 *   coef   : from sums, gate and ds (B,C), the gradient of the pooled input (the caller's MLP backward of da2):
 *            ds_over_p = ds / P, dbn_bias = sum_b (gate A + ds), dbn_weight = sum_b (gate X + ds_over_p S) and
 *            coef [2][C] = (dbn_bias, dbn_weight) / (B*P) (zeros when training == 0).
 *   dx     : dz = bn_weight * invstd * (gate * du + ds_over_p - coef[0][c] - xhat * coef[1][c]).
 *   mlp    : the MLP's backward and coef in two launches, between reduce and dx.  h1 (B,Cs) the hidden layer after its ReLU,
 *            pooled (B,C), w1 (Cs,C), w2 (C,Cs); from reduce's sums and da2:
 *              dw2[c][j] = sum_b da2[b][c] h1[b][j],  db2[c] = sum_b da2[b][c],
 *              da1[b][j] = sum_c da2[b][c] w2[c][j] where h1[b][j] > 0, else 0   (workspace),
 *              dw1[j][c] = sum_b da1[b][j] pooled[b][c],  db1[j] = sum_b da1[b][j],  ds[b][c] = sum_j da1[b][j] w1[j][c],
 *            then coef's outputs from that ds, bit for bit what cabinet_se_act_bwd_coef gives for it.  C and Cs up to 1024
 *            (cabinet_se_act_bwd_mlp_supported; CABINET_ERR_UNSUPPORTED beyond: the caller forms ds itself and calls coef), any B.
 * ------------------------------------------------------------------------- */
size_t cabinet_se_act_bwd_workspace_bytes(int B, int C, int P);
int cabinet_se_act_bwd_reduce(const float* dy, const float* z, const float* mean, const float* invstd, const float* bn_weight,
                              const float* bn_bias, const float* gate, const float* a2, int B, int C, int P, int act,
                              float* sums, float* da2, void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
int cabinet_se_act_bwd_coef(const float* sums, const float* gate, const float* ds, int B, int C, int P, int training,
                            float* dbn_weight, float* dbn_bias, float* coef, float* ds_over_p, cabinet_stream_t stream);
int cabinet_se_act_bwd_mlp_supported(int C, int Cs); /* 1 / 0 */
size_t cabinet_se_act_bwd_mlp_workspace_bytes(int B, int C, int Cs);
int cabinet_se_act_bwd_mlp(const float* sums, const float* da2, const float* gate, const float* h1, const float* pooled,
                           const float* w1, const float* w2, int B, int C, int Cs, int P, int training, float* dw1, float* db1,
                           float* dw2, float* db2, float* ds, float* dbn_weight, float* dbn_bias, float* coef, float* ds_over_p,
                           void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
int cabinet_se_act_bwd_dx(const float* dy, const float* z, const float* mean, const float* invstd, const float* bn_weight,
                          const float* bn_bias, const float* gate, const float* ds_over_p, const float* coef,
                          int B, int C, int P, int act, float* dz, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * BatchNorm2d (+activation) followed by a depthwise convolution, as one operator.
 * Replaces `nn.BatchNorm2d(hidden), act, depthwise nn.Conv2d` of the MBConv block, src/models/mobilenetv3.py:135-143:
 * the normalised, activated (B,C,H,W) tensor is neither written nor re-read -- the convolution normalises while it
 * stages its input tile, and its backward emits the BatchNorm-backward partial sums.
 *   z: the BatchNorm input (B,C,H,W); bn_* / running_* / save_* / act / training / momentum / eps as cabinet_bn_act;
 *   conv_weight (C,1,K,K), K, stride as cabinet_dwconv.   y (B,C,Ho,Wo).
 *   bwd: dy (B,C,Ho,Wo) -> dz (B,C,H,W), dbn_weight, dbn_bias (C), dconv_weight (C,1,K,K).  Deterministic.
 * ------------------------------------------------------------------------- */
size_t cabinet_bn_dwconv_fwd_workspace_bytes(int B, int C, int H, int W);
int cabinet_bn_dwconv_fwd(const float* z, const float* bn_weight, const float* bn_bias,
                          float* running_mean, float* running_var, const float* conv_weight,
                          int B, int C, int H, int W, int K, int stride, int act, int training,
                          float momentum, float eps, float* y, float* save_mean, float* save_invstd,
                          void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
size_t cabinet_bn_dwconv_bwd_workspace_bytes(int B, int C, int H, int W, int K, int stride);
int cabinet_bn_dwconv_bwd(const float* dy, const float* z, const float* bn_weight, const float* bn_bias,
                          const float* save_mean, const float* save_invstd, const float* conv_weight,
                          int B, int C, int H, int W, int K, int stride, int act, int training,
                          float* dz, float* dbn_weight, float* dbn_bias, float* dconv_weight,
                          void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * The 7x7 stride-2 padding-3 stem convolution of the spatial branch: x (B,3,H,W) -> y (B,64,Ho,Wo), no bias.
 * Replaces the nn.Conv2d inside ConvBNReLU(3, 64, kernel_size=7, stride=2, padding=3), src/models/cabinet.py:111
 * (forward cabinet.py:42).  weight (64,3,7,7).  The input is the image: only the weight gradient exists.
 *   wrw : dw (64,3,7,7) = sum over images and pixels of dy (x) patches; ordered slab sum, deterministic.
 * ------------------------------------------------------------------------- */
int cabinet_stem_conv_fwd(const float* x, const float* weight, int B, int H, int W, float* y, cabinet_stream_t stream);
size_t cabinet_stem_conv_wrw_workspace_bytes(int B, int H, int W);
int cabinet_stem_conv_wrw(const float* dy, const float* x, int B, int H, int W, float* dw,
                          void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Backward of relu(bn(stem_conv(image))) as one operator: the stem's ConvBNReLU, src/models/cabinet.py:111 with the
 * bn -> relu tail of ConvBNReLU.forward, cabinet.py:42-44.  g (B,64,Ho,Wo) is the gradient at the ReLU's output, z
 * (B,64,Ho,Wo) the convolution's output, x (B,3,H,W) the image; save_mean / save_invstd (64) as cabinet_bn_act_fwd
 * returned them.  BatchNorm's reduce + finalize give dbn_weight / dbn_bias (64); the weight-gradient kernel then forms the
 * BatchNorm input gradient per element while it stages its tile, so that (B,64,Ho,Wo) tensor is never written.
 * dw (64,3,7,7) and the BatchNorm gradients are bit for bit those of cabinet_bn_act_bwd followed by
 * cabinet_stem_conv_wrw.  training = 0: eval-mode BatchNorm (save_mean / save_invstd from the running buffers).
 * g, z 16-byte aligned.  Deterministic.
 * ------------------------------------------------------------------------- */
size_t cabinet_stem_conv_bn_bwd_workspace_bytes(int B, int H, int W);
int cabinet_stem_conv_bn_bwd(const float* g, const float* z, const float* x, const float* bn_weight, const float* bn_bias,
                             const float* save_mean, const float* save_invstd, int B, int H, int W, int training,
                             float* dw, float* dbn_weight, float* dbn_bias,
                             void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Thin pointwise (1x1, bias-free, stride 1) convolution on large planes, streaming form:
 * y (B,Co,P) = W (Co,Ci) . x (B,Ci,P).  Replaces the nn.Conv2d(kernel_size=1) of the first MBConv blocks,
 * src/models/mobilenetv3.py:128-131,144-151, where the product is HBM-bound (Ci, Co <= 128).
 * Supported: Ci, Co multiples of 8, <= 128, ceil(Ci/32)*ceil(Co/32) <= 8, P <= 2^21, max(Ci, Co) * P <= 2^28 (the kernels
 *   address one image's operand with 32-bit byte offsets) (cabinet_pwconv_supported).
 *   bwd: dx = W^T dy (skipped if NULL), dw = sum_{b,p} dy (x) x (skipped if NULL); ordered slab sum, deterministic.
 * ------------------------------------------------------------------------- */
int cabinet_pwconv_supported(int Ci, int Co, int P);
/* The launch plan of the stream kernel for one M x K product (forward: M = Co, K = Ci; input gradient: M = Ci, K = Co) on B
 * planes of P pixels -- the decision cabinet_pwconv_fwd / _bwd take, read from the same function; host-only, no HIP call.
 * x_align_bytes / y_align_bytes: the operand's and the output's address modulo 16 (or, what decides the same, its alignment
 * 16, 8 or 4).  out = {form (0 plain walk, 1 pipelined), pixels per lane and access V (4, 2, 1), pixels per block, blocks}.
 * The grid is min(blocks, 256 x the workgroups the runtime reports resident on a CU, 8 at the most). */
int cabinet_pwconv_stream_plan(int B, int M, int K, int P, int x_align_bytes, int y_align_bytes, int out[4]);
int cabinet_pwconv_fwd(const float* x, const float* w, int B, int Ci, int Co, int P, float* y, cabinet_stream_t stream);
size_t cabinet_pwconv_bwd_workspace_bytes(int B, int Ci, int Co, int P);
int cabinet_pwconv_bwd(const float* dy, const float* x, const float* w, int B, int Ci, int Co, int P,
                       float* dx, float* dw, void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Backward of a thin pointwise convolution z = W x (as cabinet_pwconv_fwd) TOGETHER with the BatchNorm (+activation) that
 * consumes z, src/models/mobilenetv3.py:128-152: the BatchNorm's input gradient dz is formed while the weight-gradient kernel
 * stages its operands, feeds dw = sum dz (x) x and dx = W^T dz from the LDS, and is never written.  One tile: Ci, Co
 * multiples of 8, <= 96, P as cabinet_pwconv_wide_supported (cabinet_pw_bn_bwd_supported).  dx and / or dw may be NULL (that
 * product is skipped).  Ordered sums, no atomics, deterministic.
 *   cabinet_pw_bn_act_bwd     : z -> act(bn(z)) (cabinet_bn_act_fwd; a shortcut's gradient is g itself).  g (B,Co,P) is the
 *       gradient at the activation's output.  dbn_weight / dbn_bias are bit for bit cabinet_bn_act_bwd's, dw is
 *       cabinet_pwconv_bwd's applied to that call's dx.  g, z 16-byte aligned where P % 4 == 0.
 *   cabinet_pw_bn_dwconv_bwd  : z -> depthwise conv(act(bn(z))) (cabinet_bn_dwconv_fwd).  dy (B,C,Ho,Wo); dconv_weight,
 *       dbn_weight, dbn_bias are bit for bit cabinet_bn_dwconv_bwd's.  x (B,Ci,H,W), pw_weight (C,Ci).
 * ------------------------------------------------------------------------- */
int cabinet_pw_bn_bwd_supported(int Ci, int Co, int P);
/* The launch plan of the BN form, as the two entry points below take it (host-only, no HIP call).  dx_align_bytes: the address
 * of dx modulo 16 (0 for a NULL dx).  out = {row blocks of Co (BM), row blocks of Ci (BN), splits = workgroups, 16-byte dx
 * stores (1) or dwords (0), dynamic LDS bytes}. */
int cabinet_pw_bn_bwd_plan(int B, int Ci, int Co, int P, int dx_align_bytes, int out[5]);
size_t cabinet_pw_bn_act_bwd_workspace_bytes(int B, int Ci, int Co, int P);
int cabinet_pw_bn_act_bwd(const float* g, const float* z, const float* x, const float* pw_weight, const float* bn_weight,
                          const float* bn_bias, const float* save_mean, const float* save_invstd, int B, int Ci, int Co, int P,
                          int act, int training, float* dx, float* dpw_weight, float* dbn_weight, float* dbn_bias,
                          void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
size_t cabinet_pw_bn_dwconv_bwd_workspace_bytes(int B, int Ci, int C, int H, int W, int K, int stride);
int cabinet_pw_bn_dwconv_bwd(const float* dy, const float* z, const float* x, const float* pw_weight, const float* bn_weight,
                             const float* bn_bias, const float* save_mean, const float* save_invstd, const float* conv_weight,
                             int B, int Ci, int C, int H, int W, int K, int stride, int act, int training, float* dx,
                             float* dpw_weight, float* dbn_weight, float* dbn_bias, float* dconv_weight,
                             void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Weight gradient of the WIDE pointwise (1x1, bias-free, stride 1) convolutions, the ones cabinet_pwconv_supported leaves
 * to the stock operator (src/models/mobilenetv3.py:128-131,144-151,193, cabinet.py:114): NCHW in, no layout copy,
 *   dw (Co,Ci) = sum_{b,p} dy (B,Co,P) (x) x (B,Ci,P)
 * exact-fp32 MFMA with fp32 accumulation, split over (image, 64-pixel chunk), ordered slab sum: no atomics, bit-reproducible,
 * capturable (the workspace comes from the caller).  The forward and the input gradient stay with the stock operator.
 * Supported: Ci, Co multiples of 8, <= 4096, P <= 2^21, max(Ci, Co) * P <= 2^28 (cabinet_pwconv_wide_supported).
 * workspace: cabinet_pwconv_wide_wgrad_workspace_bytes (one (Co,Ci) slab per split of the pixels; at most 512).
 * ------------------------------------------------------------------------- */
int cabinet_pwconv_wide_supported(int Ci, int Co, int P);
/* The launch plan of cabinet_pwconv_wide_wgrad (host-only, no HIP call): out = {BM, BN (32-row blocks of Co / Ci per tile),
 * tiles along Co, tiles along Ci, splits of the pixel chunks}; the grid is tiles x splits, the workspace one slab per split. */
int cabinet_pwconv_wide_plan(int B, int Ci, int Co, int P, int out[5]);
size_t cabinet_pwconv_wide_wgrad_workspace_bytes(int B, int Ci, int Co, int P);
int cabinet_pwconv_wide_wgrad(const float* dy, const float* x, int B, int Ci, int Co, int P, float* dw,
                              void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Dense 3x3 convolution, stride 1, padding 1, no bias (nn.Conv2d(Ci, Co, 3, padding=1, bias=False)) as Winograd
 * F(2x2,3x3) on the exact-fp32 MFMA; input transform, the 16 products and the output transform in ONE launch.
 * Replaces src/models/cabinet.py:59 (`conva[0]`), :68 + :88-89 (`b1(torch.cat([x, feat], dim=1))`: the two inputs are read
 * through two pointers, the concat is never materialised) and :160 (`conv_out.conv.conv`), plus their autograd backward.
 *   x0 (B,C0,H,W), x1 (B,C1,H,W) (C1 = 0, x1 = NULL: a plain convolution);  w (Co, C0+C1, 3, 3);  y (B,Co,H,W)
 *   bn_part (fwd, nullable): [2][Co][cabinet_conv3x3_tile_blocks(B,H,W)] floats -- per output channel and tile block
 *     (4 x 32 output pixels) the mean and the sum of squared deviations of the block's valid outputs, for the training-mode
 *     BatchNorm2d that follows (cabinet.py:60, :90): cabinet_bn_act_fwd_stats consumes them instead of a pass over y.
 *   bwd: dx0 (B,C0,H,W) and dx1 (B,C1,H,W) = data gradient (either pair skipped when dx0 == NULL), dw (Co,C0+C1,3,3) =
 *     weight gradient (skipped when NULL); both Winograd too (the weight gradient contracts over tiles: F(3x3,2x2));
 *     ordered slab sums, no atomics: deterministic.
 * Supported (cabinet_conv3x3_supported): C0, C1 multiples of 16, Co and C0+C1 multiples of 64, C0 a multiple of 64 when C1 > 0;
 * any B, H, W (odd sizes masked) with one image's tensors below 1 GiB (zero padding rides on the buffer range check).
 * ------------------------------------------------------------------------- */
int cabinet_conv3x3_supported(int C0, int C1, int Co);
int cabinet_conv3x3_tile_blocks(int B, int H, int W);
size_t cabinet_conv3x3_fwd_workspace_bytes(int B, int C0, int C1, int Co, int H, int W);
int cabinet_conv3x3_fwd(const float* x0, const float* x1, const float* w, int B, int C0, int C1, int Co, int H, int W,
                        float* y, float* bn_part, void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
size_t cabinet_conv3x3_bwd_workspace_bytes(int B, int C0, int C1, int Co, int H, int W);
int cabinet_conv3x3_bwd(const float* dy, const float* x0, const float* x1, const float* w, int B, int C0, int C1, int Co,
                        int H, int W, float* dx0, float* dx1, float* dw,
                        void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Evaluation tail (ABI v8): everything the multi-scale evaluator does after the model, on the device.
 * Replaces src/scripts/evaluate.py:75-87 (eval_chip: softmax, flip, softmax, +=, *= 0.5) together with the final x8
 * upsample of cabinet.py:240-245, :133-134 (window +=, count +=), :137 (prob / count), :156-158 (resize back) with :217
 * (probs +=), and :218-224 with :161-191 (argmax, copy to the host, numpy.bincount per image).
 *
 * cabinet_eval_chip_accum -- one launch per chip.
 *   a (N,C,hl,wl): logits of the chip at the model's resolution; b: same shape, logits of the horizontally flipped chip,
 *   or NULL (no flip).  For every pixel (y,x) of the ch x cw chip: the C logits sampled bilinearly from `a`
 *   (align_corners=False, ratios hl/ch and wl/cw, PyTorch's source-index rule; exact at ratio 1), softmax over classes;
 *   with b the same at column cw-1-x of b's upsample and the two averaged; the result times rcp_y[y0+y] * rcp_x[x0+x]
 *   is ADDED to dst (N,C,FH,FW) at (y0+y, x0+x).  rcp_y (FH) and rcp_x (FW) hold 1 / (number of windows covering the row /
 *   the column): the reference's count map is their outer product and never exists; NULL = all ones.
 *   Launches that write overlapping windows must be ordered on one stream (plain read-modify-write, no atomics).
 *   C <= 32 (8 and 19 are compiled forms); supported when the staged source rows fit the LDS (any ratio <= 1 does).
 * cabinet_eval_scale_merge -- total (N,C,H,W) += resize(prob (N,C,FH,FW)[:, :, hst:hed, wst:wed] -> (H,W)), bilinear,
 *   align_corners=False; prob is already normalised by the reciprocals above.
 * cabinet_eval_argmax_hist -- pred = argmax over C of total (N,C,H,W), lowest index on ties; labels (N,H,W) int64;
 *   a pixel whose label == ignore_lb is dropped, any other label is clipped into [0, C-1];
 *   hist (C,C) int64, hist[pred][label] += 1 (integer atomics: exactly reproducible; the caller zeroes it once);
 *   pred (N,H,W) uint8 receives the predictions when not NULL.  C <= 32.
 * ------------------------------------------------------------------------- */
int cabinet_eval_chip_accum_supported(int C, int hl, int wl, int ch, int cw, int flip);
int cabinet_eval_chip_accum(const float* a, const float* b, int N, int C, int hl, int wl, int ch, int cw, float* dst, int FH, int FW,
                            int y0, int x0, const float* rcp_y, const float* rcp_x, cabinet_stream_t stream);
int cabinet_eval_scale_merge(const float* prob, int N, int C, int FH, int FW, int hst, int hed, int wst, int wed, float* total, int H,
                             int W, cabinet_stream_t stream);
int cabinet_eval_argmax_hist(const float* total, const long long* labels, int N, int C, int H, int W, int ignore_lb, long long* hist,
                             unsigned char* pred, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Inference tail (K17; ADDITIVE to ABI version 8: no existing entry point, constant or layout changes).
 * Replaces, for one image or a batch, what src/scripts/visualize.py does after the model: :114-139 (softmax, flip, resize,
 * +=, /=, argmax, the copy of int64 labels to the host) together with the model's final x8 upsample (cabinet.py:240-245),
 * :50-61 (colorize_mask) and :165-177 (de-normalise, clip, * 255, astype(uint8), Image.blend).
 * Every output is a byte array; neither its start nor its row starts need be dword-aligned, and no byte outside it is written.
 *
 * cabinet_predict_up_argmax -- visualize.py:113-114 + :139 for scales = [1.0], flip = False, with cabinet.py:240-245:
 *   labels (N,H,W) uint8 [n,y,x] = argmax over c of the bilinear resize of logits_low (N,C,hl,wl) to (H,W)
 *   (align_corners=False, ratios hl/H and wl/W, PyTorch's source-index rule; at ratio 1 the logits themselves are compared).
 *   softmax is monotonic per pixel, so this is the argmax of the reference's probabilities; the full-resolution class tensor
 *   never exists.  Strict `>`: the lowest index wins among equal values (torch.argmax); a NaN logit is never chosen.
 *   C <= 32 (8 and 19 are compiled forms); supported when the staged source rows of one row segment fit the LDS
 *   (every ratio wl/W <= 1 does; a strongly shrinking resize of many classes is refused).
 * cabinet_predict_argmax -- visualize.py:139 for the multi-scale / flip path: labels (N,H,W) uint8 = argmax over c of
 *   total (N,C,H,W) fp32 (16-byte aligned), lowest index on ties; bit-exact against torch.argmax on NaN-free input.  C <= 32.
 * cabinet_predict_render -- visualize.py:50-61 and :165-177, byte for byte; all arrays but mean / std in device memory:
 *   pred_rgb (N,H,W,3)    = palette (n_colors,3) [min(label, n_colors - 1)]                     1 <= n_colors <= 256
 *   input_rgb (N,H,W,3)   = (uint8) (clip(image (N,3,H,W) * std[c] + mean[c], 0, 1) * 255)      or NULL: not written
 *   overlay_rgb (N,H,W,3) = (uint8) ((float) in + alpha * (float) (colour - in))                or NULL: not written
 *   in fp32, every product and sum rounded on its own (no fused multiply-add), truncated toward zero: numpy's float32
 *   arithmetic and Pillow's Image.blend for 0 <= alpha <= 1.  image may be NULL when both optional outputs are;
 *   mean and std point to three HOST floats each, read during the call.
 * ------------------------------------------------------------------------- */
int cabinet_predict_up_argmax_supported(int C, int hl, int wl, int H, int W);
int cabinet_predict_up_argmax(const float* logits_low, int N, int C, int hl, int wl, int H, int W, unsigned char* labels,
                              cabinet_stream_t stream);
int cabinet_predict_argmax(const float* total, int N, int C, int H, int W, unsigned char* labels, cabinet_stream_t stream);
int cabinet_predict_render(const unsigned char* labels, const float* image, const unsigned char* palette, int n_colors,
                           const float* mean, const float* std, float alpha, int N, int H, int W, unsigned char* pred_rgb,
                           unsigned char* input_rgb, unsigned char* overlay_rgb, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Weight and input gradient of the 3x3 stride-2 padding-1 bias-free convolutions (added under ABI v8): NCHW, no layout copy,
 *   dw (Co,Ci,3,3) = sum_{b,oy,ox} dy (B,Co,Ho,Wo)[.,oy,ox] (x) x (B,Ci,H,W)[., 2 oy - 1 + ky, 2 ox - 1 + kx]
 * with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.  Replaces the weight-gradient half of the autograd backward of
 * ConvBNReLU(64, 64, kernel_size=3, stride=2, padding=1), src/models/cabinet.py:112-113 (SpatialBranch.conv2 / conv3,
 * forward cabinet.py:42), and of conv_3x3_bn(3, input_channel, 2), src/models/mobilenetv3.py:173 (:86-91), the backbone's
 * first layer.  Exact-fp32 MFMA with fp32 accumulation, one slab per workgroup, ordered slab sum: no atomics,
 * bit-reproducible, capturable (the workspace comes from the caller).
 * Supported (cabinet_conv3x3s2_supported): (Ci, Co) = (64, 64) or (3, 16); any B, H, W >= 1.
 *   dgrad (64 -> 64 only; the 3 -> 16 layer reads the image): w (Co,Ci,3,3),
 *     dx (B,Ci,H,W)[., iy, ix] = sum_{co,ky,kx} w[co,.,ky,kx] * dy[., co, (iy + 1 - ky) / 2, (ix + 1 - kx) / 2]
 *   over the taps with integer, in-range quotients, by the four parity classes of (iy, ix): no product with a structural
 *   zero.  Every element of dx is written; no workspace, fixed summation order.
 *   fwd (cabinet_conv3x3s2_fwd_supported: (Ci, Co) = (64, 64) only; the 3 -> 16 layer keeps the stock forward):
 *     y (B,Co,Ho,Wo)[., oy, ox] = sum_{ci,ky,kx} w[.,ci,ky,kx] * x (B,Ci,H,W)[., ci, 2 oy - 1 + ky, 2 ox - 1 + kx]
 *   with zero padding, i.e. conv2d(x, w, stride 2, padding 1) of ConvBNReLU(64, 64, 3, 2, 1), cabinet.py:112-113, straight
 *   on NCHW.  Any B, H, W >= 1, tensors at 4-byte alignment; every element of y is written; no workspace, no atomics, a
 *   fixed summation order that does not depend on the launch plan.
 * ------------------------------------------------------------------------- */
int cabinet_conv3x3s2_supported(int Ci, int Co);
size_t cabinet_conv3x3s2_wgrad_workspace_bytes(int B, int Ci, int Co, int H, int W);
int cabinet_conv3x3s2_wgrad(const float* dy, const float* x, int B, int Ci, int Co, int H, int W, float* dw,
                            void* workspace, size_t workspace_bytes, cabinet_stream_t stream);
int cabinet_conv3x3s2_dgrad(const float* dy, const float* w, int B, int Ci, int Co, int H, int W, float* dx,
                            cabinet_stream_t stream);
int cabinet_conv3x3s2_fwd_supported(int Ci, int Co);
int cabinet_conv3x3s2_fwd(const float* x, const float* w, int B, int Ci, int Co, int H, int W, float* y,
                          cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Optimizer tail (K16): gradient clipping, warm-up / poly SGD with momentum and
 * per-group weight decay, and the weight EMA, as three launches on `stream`.
 * Replaces src/scripts/train.py:411-427 per step:
 *     clip_grad_norm_(net.parameters(), max_grad_norm)
 *     optim.step()        (src/utils/optimizer.py:124-156: host-side schedule + torch SGD)
 *     ema.update(net)     (src/utils/ema.py:51-62: two launches per state_dict entry)
 * ADDITIVE to ABI version 8: no existing entry point, constant or layout changes, so a
 * caller built against the earlier v8 header is unaffected and the version stays 8.
 *
 * The step counter `it`, the EMA counter `updates` and the schedule live in DEVICE
 * memory (the state block), so a hipGraph replay of the call advances them.
 *
 * Tables (device memory, built by the caller once; NOT kernel arguments, any count):
 *   entries[n_entries]  one per floating-point tensor.  param/grad/buf/ema are dense
 *                       fp32 arrays of `numel` elements in the SAME element order.
 *                       flags & CABINET_SGD_TAIL_EMA_ONLY (or grad == NULL): only
 *                       ema = d*ema + (1-d)*param runs (BatchNorm running statistics,
 *                       frozen parameters, parameters without a gradient this step).
 *                       buf may be NULL when momentum == 0, ema NULL without an EMA.
 *                       group: index 0..3 into the config's per-group arrays.
 *   chunks[n_chunks]    (tensor, start, length): length <= CABINET_SGD_TAIL_CHUNK and
 *                       start a multiple of it, so that a chunk is as aligned as its
 *                       tensor; every element of every entry in exactly one chunk.
 *                       A chunk that leaves its tensor or names no entry is ignored.
 * Pointers need 4-byte alignment only: chunks whose pointers are 16-byte aligned move
 * as float4, the others (and each chunk's last numel % 4 elements) as scalars.
 *
 * State block, cabinet_sgd_tail_state_bytes(n_entries) bytes of device memory, zeroed by
 * the caller before the first step (byte offsets; all fields may be read or preset by
 * the caller between steps, e.g. to resume):
 *     0 int64 it        8 int64 updates      16 int64 skipped
 *    24 int32 nonfinite (last step)          28 int32 apply (last step ran)
 *    32 float last_grad_norm   36 float clip coefficient   40 float lr[4]
 *    56 float d (EMA factor)   60 float 1-d
 *   128 int32 valid[n_entries]  momentum buffer of entry i holds a value (0: the next
 *       step sets buf = g, torch's first-step rule); then int32 first[n_entries] (scratch)
 * Workspace: cabinet_sgd_tail_workspace_bytes(n_chunks), one fp32 partial per chunk.
 *
 * Per step:  norm = sqrt(sum over owned entries of g^2) -- per-chunk fp32 partials in a
 * fixed order, summed in double, no atomics: bit-reproducible;
 *   coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1;
 *   lr_g = float(lr_scale[g] * (it < warmup ? start + it/warmup * (lr0 - start)
 *                                           : lr0 * (1 - k)^power)),
 *          k = clamp((it - warmup) / (max_iter - warmup), 0, 1), in double
 *          (past max_iter the reference's formula leaves the reals; here lr = 0);
 *   updates += 1; d = decay * (1 - exp(-updates / tau)); it += 1;
 *   per element: g = g*coef; if wd_g != 0: g += wd_g*p; buf = valid ? momentum*buf + g : g;
 *                p -= lr_g*buf; ema = d*ema + (1-d)*p.
 * With skip_nonfinite != 0 and a norm that is inf or nan NOTHING is written but
 * last_grad_norm / nonfinite / apply, the counters do not advance and `skipped` goes up
 * by one (what scaler.step and the `optim.it != prev_it` gate do in train.py:419-427).
 * max_grid: 0 = the default cap of 2048 workgroups; smaller values force the
 * grid-stride loop (tests).
 * ------------------------------------------------------------------------- */
#define CABINET_SGD_TAIL_CHUNK 4096
#define CABINET_SGD_TAIL_EMA_ONLY 1

typedef struct cabinet_sgd_tail_entry {
    float* param;
    const float* grad;
    float* buf;
    float* ema;
    long long numel;
    int group;
    int flags;
} cabinet_sgd_tail_entry; /* 48 bytes */

typedef struct cabinet_sgd_tail_chunk {
    long long start;
    int tensor;
    int length;
} cabinet_sgd_tail_chunk; /* 16 bytes */

typedef struct cabinet_sgd_tail_config { /* host memory, read during the call */
    double lr0, warmup_start_lr, max_iter, power;
    double lr_scale[4], weight_decay[4];
    double momentum, max_norm, ema_decay, ema_tau;
    long long warmup_steps;
    int skip_nonfinite;
    int reserved;
} cabinet_sgd_tail_config;

size_t cabinet_sgd_tail_workspace_bytes(int n_chunks);
size_t cabinet_sgd_tail_state_bytes(int n_entries);
int cabinet_sgd_tail_step(const cabinet_sgd_tail_entry* entries, int n_entries, const cabinet_sgd_tail_chunk* chunks, int n_chunks,
                          const cabinet_sgd_tail_config* config, void* state, size_t state_bytes, int max_grid,
                          void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Gradient accumulation across hipGraph replays (K21; ADDITIVE to ABI version 8: no
 * existing entry point, constant or layout changes).  Replaces what autograd's own
 * accumulation into .grad does over a window of src/scripts/train.py:435-439 when the
 * backward is a captured graph, which OVERWRITES its static gradient tensors on every
 * replay.  Two launches on `stream`; nothing is allocated, synchronised or read on the
 * host, so ONE recorded call serves every micro-step of every window.
 *
 * Tables (device memory, built by the caller once), K16's conventions:
 *   entries[n_entries]  (acc, grad, numel): dense fp32 arrays of `numel` elements in the
 *                       SAME element order; acc and grad must not overlap.
 *   chunks[n_chunks]    cabinet_sgd_tail_chunk: length <= CABINET_SGD_TAIL_CHUNK, start a
 *                       multiple of it, every element of every entry in exactly one chunk.
 *                       A chunk that leaves its tensor or names no entry is ignored.
 * Pointers need 4-byte alignment only: a chunk whose two pointers are 16-byte aligned
 * moves as float4, the others (and each chunk's last numel % 4 elements) as scalars.
 *
 * State block, cabinet_grad_accum_state_bytes() (= 64) bytes of device memory, 8-byte
 * aligned, zeroed by the caller before the first call (byte offsets; the caller may read
 * or preset the field between calls):
 *     0 int32 micro     micro-steps folded into acc in the current window
 *     4 .. 63           reserved, left alone
 *
 * cabinet_grad_accum, per element i of every entry:
 *     micro == 0:  acc[i] = grad[i]           a copy; acc is NOT read, so a stale NaN or
 *                                             inf does not survive and -0.0 stays -0.0
 *     otherwise:   acc[i] = acc[i] + grad[i]  ONE fp32 add: no scale factor (1/accum_steps
 *                                             lives in the loss), no FMA -- the bits of
 *                                             autograd's accumulation in the same order
 *   then, in a one-lane launch BEHIND the pass, micro += 1 (a plain store): every
 *   workgroup of the pass reads the same micro.  No atomics, no scratch, no reduction:
 *   the result does not depend on the grid and is bit-reproducible.  Nothing outside
 *   [acc, acc + numel) is written.
 * cabinet_grad_accum_reset: micro = 0 (one-lane launch): the next call starts a window.
 * max_grid: 0 = the default cap of 2048 workgroups; smaller values force the
 * grid-stride loop (tests).
 * Errors: -1 for a null table or state block, a non-positive count, a negative max_grid
 * or a misaligned table; -3 for state_bytes < cabinet_grad_accum_state_bytes().
 * ------------------------------------------------------------------------- */
typedef struct cabinet_grad_accum_entry {
    float* acc;
    const float* grad;
    long long numel;
} cabinet_grad_accum_entry; /* 24 bytes */

size_t cabinet_grad_accum_state_bytes(void);
int cabinet_grad_accum(const cabinet_grad_accum_entry* entries, int n_entries, const cabinet_sgd_tail_chunk* chunks, int n_chunks,
                       void* state, size_t state_bytes, int max_grid, cabinet_stream_t stream);
int cabinet_grad_accum_reset(void* state, size_t state_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Training augmentation (K18; ADDITIVE to ABI version 8: no existing entry point, constant or layout changes).
 * Replaces, for a batch, what src/datasets/cityscapes.py does to a decoded train sample: :114-136 (RandomHorizontalFlip,
 * RandomScale, RandomCrop with reflect padding, RandomColorJitter, RandomGrayscale, RandomGamma, RandomNoise, RandomCutout of
 * src/datasets/transform.py), :102-109 (ToTensor, Normalize) and :156-158 (convert_labels, int64) -- byte for byte, but for the
 * VALUES of the noise when the library draws them itself.  Two launches on `stream`; nothing is allocated, nothing synchronises.
 *
 * samples: DEVICE memory, one block the caller builds per batch and copies once: N entries of cabinet_augment_sample, then the
 * tables they name by BYTE OFFSET from `samples` (4-byte aligned).  Per sample:
 *   image (H,W,3) uint8 interleaved and label (H,W) uint8, device pointers; samples of one batch may differ in H and W.
 *   col_taps[tw], row_taps[th] of cabinet_augment_tap: output column x of the crop is, per channel,
 *       clip8((2^21 + sum_{k<n} coef[k] * in[first + step*k]) >> 22)
 *     (Pillow's resize(BILINEAR): horizontal pass first into a uint8 intermediate, then the vertical pass over it; coef are
 *     Pillow's 22-bit integer coefficients).  The caller folds in the horizontal flip (step = -1 from the mirrored index), the
 *     crop offset (only the window's entries are passed) and the reflect padding (a column past the resized width w takes the
 *     entry of resized column 2 (w - 1) - c).  n <= 5; an unchanged axis is the single coefficient 2^22.
 *   lab_col[tw], lab_row[th] int32: the label's source index (Pillow's resize(NEAREST), flip and crop folded in), or -1 for a
 *     padded position, which becomes ignore_label.  Otherwise the label is label_lut[source byte] (id -> trainId).
 *   brightness, contrast, saturation: the three ImageEnhance factors r of Image.blend(degenerate, image, r), 1 = identity.  fp32,
 *     t = deg + r * (src - deg) with every operation rounded on its own; (uint8) t for 0 <= r <= 1, else 0 for t <= 0, 255 for
 *     t >= 255, (uint8) t between.  Degenerates: 0; m = (int)(mean L of the brightened crop + 0.5); the pixel's own L, with
 *     L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
 *   flags: CABINET_AUGMENT_GRAY (all channels = L), _GAMMA (byte -> gamma_lut[byte]; the caller builds the table with the
 *     reference's numpy expression), _NOISE ((uint8) clip((double) byte + (double) noise, 0, 255)), _CUTOUT (zero bytes on the
 *     square rows cut_y .. cut_y + cut_size - 1, columns cut_x .. cut_x + cut_size - 1), applied in this order after the blends.
 * noise: NULL, or device fp32 (N,th,tw,3) of values ALREADY scaled by sigma * 255, used as given.  NULL: the library draws
 *   standard normals -- Philox4x32-10 keyed by `seed`, counter (pixel index y tw + x, sample index), Box-Muller on the two
 *   pairs of the block, the first three values for R, G, B -- and multiplies them by noise_scale.  Stateless, no atomics: the
 *   same (seed, sample, pixel) gives the same bytes.
 * mean, std: three HOST floats each, read during the call.  out_image (N,3,th,tw) fp32 = ((float) byte / 255 - mean[c]) / std[c],
 *   two correctly rounded operations (4-byte aligned; 16-byte stores are used where an address allows them); out_label
 *   (N,th,tw) int64; out_u8 (N,th,tw,3) uint8, the final bytes, or NULL.  No byte outside a source array is read -- every table
 *   index is clamped into its array -- and no byte outside an output is written.
 * workspace: cabinet_augment_workspace_bytes(N, th, tw), 16-byte aligned: the uint8 crop after the brightness blend and one
 *   64-bit partial sum of L per workgroup tile.  Every call writes all of it before reading: the caller zeroes nothing.
 * Coverage (cabinet_augment_supported: 1 / 0, with the reason in cabinet_last_error()): 1 <= th, tw <= 32768; max_taps <= 5;
 *   reflect padding of an axis <= the smallest resized size - 1 (numpy's multiple reflection is out).  The limit behind the
 *   tap count is the resize ratio in/out <= 2.5 per axis (scale >= 0.4): Pillow's tables then have at most five taps, and the
 *   row taps of 16 consecutive output rows span fewer than 17 * 2.5 + 1 source rows, inside the 48 the geometry kernel stages
 *   per tile.  That span (largest minus smallest source row of row_taps[16 j .. 16 j + 15], plus one, <= 48) is part of the
 *   contract for tables built any other way: five taps alone do not imply it (a tiny output clamps its taps at the borders at
 *   any ratio), and rows past it are read as row 47 of the tile.  The tables live in device memory, so cabinet_augment_batch
 *   itself checks what it can see: -1 for a null pointer, a non-positive count, a misaligned pointer or a short workspace; -2
 *   for a shape outside coverage.  The caller states the rest -- the batch's largest tap count and pads, its smallest resized
 *   size -- to cabinet_augment_supported.
 * ------------------------------------------------------------------------- */
#define CABINET_AUGMENT_GRAY 1
#define CABINET_AUGMENT_GAMMA 2
#define CABINET_AUGMENT_NOISE 4
#define CABINET_AUGMENT_CUTOUT 8

typedef struct cabinet_augment_tap {
    int first, step, n;
    int coef[5];
} cabinet_augment_tap; /* 32 bytes */

typedef struct cabinet_augment_sample {
    const unsigned char* image;
    const unsigned char* label;
    int H, W;
    unsigned long long col_taps, row_taps, lab_col, lab_row; /* byte offsets from `samples` */
    float brightness, contrast, saturation;
    int flags;
    float noise_scale; /* sigma * 255 */
    int cut_y, cut_x, cut_size;
    int ignore_label;
    int reserved;
    unsigned char gamma_lut[256];
    long long label_lut[256];
} cabinet_augment_sample; /* 2400 bytes */

int cabinet_augment_supported(int th, int tw, int max_taps, int max_pad_y, int max_pad_x, int min_h, int min_w);
size_t cabinet_augment_workspace_bytes(int N, int th, int tw);
int cabinet_augment_batch(const void* samples, int N, int th, int tw, const float* noise, unsigned long long seed,
                          const float* mean, const float* std, float* out_image, long long* out_label, unsigned char* out_u8,
                          void* workspace, size_t workspace_bytes, cabinet_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Aerial-dataset augmentation (K20; ADDITIVE to ABI version 8).  What the train pipeline shared by src/datasets/uavid.py
 * (:192-230), vdd.py and aeroscapes.py does ahead of RandomScale -- ResizeIfLarger, RandomHorizontalFlip, RandomVerticalFlip,
 * RandomTranslate, RandomRotate(expand=True) of src/datasets/transform.py -- as batched passes from uint8 to uint8 (Pillow
 * truncates to bytes between the steps), and RandomHSV inside cabinet_augment_batch.  One launch per call on `stream`; nothing
 * is allocated, nothing synchronises.
 *
 * RandomHSV: flag CABINET_AUGMENT_HSV in cabinet_augment_sample.flags; `reserved` is then the BYTE OFFSET from `samples` of 768
 * bytes: the H, S and V byte tables (the caller builds them with the reference's numpy expressions).  Each pixel of the crop,
 * after the resample and ahead of the brightness blend (so the contrast blend's mean luma is that of the converted crop), goes
 * RGB -> HSV bytes (Pillow's rgb2hsv), through the tables, and HSV -> RGB bytes (Pillow's hsv2rgb).  Flag clear: `reserved` is
 * not read, and 0 as before.
 *
 * descs: DEVICE memory, 8-byte aligned: N entries of cabinet_augment_warp_desc, then the tables they name by BYTE OFFSET from
 * `descs` (4-byte aligned).  Image arrays are (rows, cols, 3) uint8 interleaved, label arrays (rows, cols) uint8, any alignment;
 * a pass writes EVERY byte of dst_image (out_h, out_w, 3) and dst_label (out_h, out_w), fill included, and no other byte; every
 * source index is clamped into [0, H) x [0, W) where it is used.  Samples of a batch may differ in every size: the grid is sized
 * by max_out_h x max_out_w, which must be >= every entry's out_h x out_w.
 *
 * cabinet_augment_warp_batch -- Pillow's Image.transform(size, AFFINE, a, BILINEAR) for the image and (..., NEAREST,
 * fillcolor=fill) for the label.  The source is read through `flip` (bit 0: columns mirrored, bit 1: rows mirrored), i.e. the
 * pass transforms the flipped source.  Image, output pixel (x, y), in double with every operation rounded on its own:
 *     xin = a[0] (x + 0.5) + a[1] (y + 0.5) + a[2],  yin = a[3] (x + 0.5) + a[4] (y + 0.5) + a[5]   (left to right)
 *   outside 0 <= xin < W, 0 <= yin < H the pixel is 0; otherwise with xs = xin - 0.5, xf = floor(xs), dx = xs - xf (y likewise),
 *   columns clamp(xf), clamp(xf + 1), row clamp(yf): v1 = p00 + (p01 - p00) dx; v2 the same from row yf + 1 if it is inside,
 *   else v1; byte = (uint8)(v1 + (v2 - v1) dy), truncated.
 *   Label, label_mode CABINET_WARP_LABEL_TABLES (a[1] == a[3] == 0; Pillow builds per-axis tables by a running sum): lab_col
 *   [out_w] and lab_row [out_h] int32 at byte offsets, the source index or -1; both >= 0: the source byte, else `fill`.
 *   label_mode CABINET_WARP_LABEL_FIXED (Pillow's 16.16 fixed point): column (fix[2] + y fix[1] + x fix[0]) >> 16, row
 *   (fix[5] + y fix[4] + x fix[3]) >> 16, arithmetic shifts of 64-bit integers; both inside the source: its byte, else `fill`.
 *   The caller computes fix[] as FIX(v) = floor(v 65536 + 0.5) of a[0], a[1], a[2] + a[0]/2 + a[1]/2, a[3], a[4], a[5] + a[3]/2 + a[4]/2.
 *
 * cabinet_augment_resize_batch -- Pillow's resize: BILINEAR for the image through col_taps[out_w], row_taps[out_h] of
 * cabinet_augment_tap (horizontal pass into a uint8 intermediate, then vertical; the arithmetic and the tile contract of
 * cabinet_augment_batch: <= 5 taps, <= 48 source rows under 16 consecutive output rows, i.e. ratio in/out <= 2.5), NEAREST for
 * the label through lab_col, lab_row (clamped into the source; no fill).  a, fix, flip, label_mode and fill are not read.
 *
 * Return codes: -1 for null descs, N <= 0, a non-positive max size or descs not 8-byte aligned; -2 for a max size above 32768 or
 * N above 65535 -- all before any HIP call.  cabinet_augment_warp_supported answers 1 / 0 (reason in cabinet_last_error()) for
 * one sample's figures: sizes in [1, 32768]; angle_deg (rotation, 0 for none) exactly 0 or 0 < |angle| <= 45 after reduction to
 * (-180, 180]; resize_ratio (ResizeIfLarger's in/out, 0 for none) <= 2.5.
 * ------------------------------------------------------------------------- */
#define CABINET_AUGMENT_HSV 16

#define CABINET_WARP_LABEL_TABLES 0
#define CABINET_WARP_LABEL_FIXED 1
#define CABINET_WARP_FLIP_X 1
#define CABINET_WARP_FLIP_Y 2

typedef struct cabinet_augment_warp_desc {
    const unsigned char* src_image;
    const unsigned char* src_label;
    unsigned char* dst_image;
    unsigned char* dst_label;
    int H, W;                                                /* source */
    int out_h, out_w;
    double a[6];
    long long fix[6];
    unsigned long long lab_col, lab_row, col_taps, row_taps; /* byte offsets from `descs` */
    int flip, label_mode, fill, reserved;
} cabinet_augment_warp_desc; /* 192 bytes */

int cabinet_augment_warp_supported(int H, int W, int out_h, int out_w, double angle_deg, double resize_ratio);
int cabinet_augment_warp_batch(const void* descs, int N, int max_out_h, int max_out_w, cabinet_stream_t stream);
int cabinet_augment_resize_batch(const void* descs, int N, int max_out_h, int max_out_w, cabinet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CABINET_HIP_H_ */
