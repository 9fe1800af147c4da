// C ABI of libcabinet_hip.so: argument checking, workspace carving, dispatch.
// Declarations and the reference lines each entry point replaces: include/cabinet_hip.h
#include "../../include/cabinet_hip.h"

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "blocks.hpp"
#include "cab_local.hpp"
#include "cab_qkv.hpp"
#include "common.hpp"

namespace cabinet {
// cab_attn_fwd.hip
int attn_fwd_kvsplit(int B, int n);
bool attn_shape_supported(int Kc, int Vc);
hipError_t attn_fwd_dispatch(const float* q, const float* k, const float* v, float scale, int B, int Kc,
                             int Vc, int n, float* ctx, float* lse, float* part_ctx, float* part_lse,
                             int kvsplit, hipStream_t stream);
bool attn_fwd_proj_supported(int B, int Kc, int Vc, int Co, int n);
hipError_t attn_fwd_proj_dispatch(const float* q, const float* k, const float* v, const float* w_out, float scale, int B, int Kc,
                                  int Vc, int Co, int n, float* ctx, float* glob, float* lse, hipStream_t stream);
// cab_attn_bf16.hip
bool attn_bf16_supported(int Kc, int Vc);
size_t attn_bf16_pack_bytes(int B, int Kc, int Vc, int n, int precision);
hipError_t attn_fwd_bf16_dispatch(const float* q, const float* k, const float* v, float scale, int B, int Kc, int Vc, int n,
                                  float* ctx, float* lse, float* part_ctx, float* part_lse, int kvsplit, void* pack, int precision,
                                  hipStream_t stream);
// cab_attn_bwd.hip
size_t attn_bwd_workspace(int B, int Kc, int Vc, int n);
hipError_t attn_bwd_dispatch(const float* dctx, const float* q, const float* k, const float* v,
                             const float* ctx, const float* lse, float scale, int B, int Kc, int Vc, int n,
                             float* dq, float* dk, float* dv, void* ws, hipStream_t stream);
// ffm.hip
struct FfmShape {
    int B, Cs, Cc, Co, Cm, H, W;
};
size_t ffm_fwd_workspace(const FfmShape& s);
size_t ffm_bwd_workspace(const FfmShape& s);
hipError_t ffm_fwd_run(const FfmShape& s, const float* fsp, const float* fcp, const float* w_blk,
                       const float* bn_w, const float* bn_b, float* run_mean, float* run_var,
                       const float* w1, const float* w2, int training, float momentum, float eps, float* out,
                       float* z, float* save_mean, float* save_invstd, float* pooled, float* gate, void* ws,
                       hipStream_t stream);
size_t ffm_up_fwd_workspace(const FfmShape& s, int Hl, int Wl);
size_t ffm_up_bwd_workspace(const FfmShape& s, int Hl, int Wl);
size_t ffm_up_bwd_adjoint_lds(const FfmShape& s, int Hl, int Wl, size_t* limit, int* band_rows);
hipError_t ffm_up_fwd_run(const FfmShape& s, int Hl, int Wl, const float* fsp, const float* low,
                          const float* w_blk, const float* bn_w, const float* bn_b, float* run_mean,
                          float* run_var, const float* w1, const float* w2, int training, float momentum,
                          float eps, float* out, float* z, float* save_mean, float* save_invstd, float* pooled,
                          float* gate, void* ws, int precision, hipStream_t stream);
hipError_t ffm_up_bwd_run(const FfmShape& s, int Hl, int Wl, const float* dout, const float* fsp,
                          const float* low, const float* w_blk, const float* bn_w, const float* bn_b,
                          const float* w1, const float* w2, const float* z, const float* save_mean,
                          const float* save_invstd, const float* pooled, const float* gate, int training,
                          float* dfsp, float* dlow, float* dw_blk, float* dbn_w, float* dbn_b, float* dw1,
                          float* dw2, void* ws, hipStream_t stream);
hipError_t ffm_bwd_run(const FfmShape& s, const float* dout, const float* fsp, const float* fcp,
                       const float* w_blk, const float* bn_w, const float* bn_b, const float* w1,
                       const float* w2, const float* z, const float* save_mean, const float* save_invstd,
                       const float* pooled, const float* gate, int training, float* dfsp, float* dfcp,
                       float* dw_blk, float* dbn_w, float* dbn_b, float* dw1, float* dw2, void* ws,
                       hipStream_t stream);
// bn_act.hip
size_t bn_act_workspace(int B, int C, int P);
hipError_t bn_act_fwd_run(const float* x, const float* weight, const float* bias, float* running_mean,
                          float* running_var, const float* residual, int B, int C, int P, int act, int training,
                          float momentum, float eps, float* y, float* save_mean, float* save_invstd, void* ws,
                          hipStream_t stream);
hipError_t bn_act_bwd_run(const float* dy, const float* x, const float* weight, const float* bias,
                          const float* save_mean, const float* save_invstd, int B, int C, int P, int act, int training,
                          float* dx, float* dweight, float* dbias, void* ws, hipStream_t stream);
hipError_t bn_act_fwd_part_run(const float* x, const float* conv_part, int H, int W, const float* weight, const float* bias,
                               float* running_mean, float* running_var, const float* residual, int B, int C, int act, int training,
                               float momentum, float eps, float* y, float* save_mean, float* save_invstd, hipStream_t stream);
size_t se_act_bwd_workspace(int B, int C, int P);
hipError_t se_act_bwd_reduce_run(const float* dy, const float* z, const float* mean, const float* invstd, const float* weight,
                                 const float* bias, const float* gate, const float* a2, int B, int C, int P, int act, float* sums,
                                 float* da2, void* ws, hipStream_t stream);
hipError_t se_act_bwd_coef_run(const float* sums, const float* gate, const float* ds, int B, int C, int P, int training,
                               float* dweight, float* dbias, float* coef, float* ds_p, hipStream_t stream);
hipError_t se_act_bwd_dx_run(const float* dy, const float* z, const float* mean, const float* invstd, const float* weight,
                             const float* bias, const float* gate, const float* ds_p, const float* coef, int B, int C, int P,
                             int act, float* dz, hipStream_t stream);
// se_mlp.hip
bool se_act_bwd_mlp_supported(int C, int Cs);
size_t se_act_bwd_mlp_workspace(int B, int Cs);
hipError_t se_act_bwd_mlp_run(const float* sums, const float* da2, const float* gate, const float* h1, const float* pooled,
                              const float* w1, const float* w2, int B, int C, int Cs, int P, int training, float* dw1, float* db1,
                              float* dw2, float* db2, float* ds, float* dweight, float* dbias, float* coef, float* ds_p, void* ws,
                              hipStream_t stream);
// bn_act.hip
size_t gate_act_workspace(int rows, int P);
hipError_t gate_act_fwd_run(const float* x, const float* gate, int rows, int P, int act, float* y, hipStream_t stream);
hipError_t gate_act_bwd_run(const float* dy, const float* x, const float* gate, int rows, int P, int act, float* dx,
                            float* dgate, void* ws, hipStream_t stream);
// bn_cls.hip
bool bn_cls_supported(int C, int K, int P);
int bn_cls_table_floats(int C, int K);
size_t bn_cls_fwd_workspace(int B, int C, int P);
size_t bn_cls_bwd_workspace(int B, int C, int K, int P);
hipError_t bn_cls_fwd_run(const float* z, const float* conv_part, const float* bn_w, const float* bn_b, float* run_mean, float* run_var,
                          const float* w_cls, const float* bias, int B, int C, int K, int H, int W, int training, float momentum,
                          float eps, float* y, float* tab, void* ws, hipStream_t stream);
hipError_t bn_cls_bwd_run(const float* dy, const float* z, const float* tab, int B, int C, int K, int H, int W, int training, float* dz,
                          float* dbn_w, float* dbn_b, float* dw_cls, float* dbias, void* ws, hipStream_t stream);
// dwconv.hip
bool dwconv_supported(int K, int S);
size_t dwconv_bwd_workspace(int B, int C, int H, int W, int K);
hipError_t dwconv_fwd_run(const float* x, const float* w, int B, int C, int H, int W, int K, int S, float* y,
                          hipStream_t stream);
hipError_t dwconv_bwd_run(const float* dy, const float* x, const float* w, int B, int C, int H, int W, int K, int S,
                          float* dx, float* dw, void* ws, hipStream_t stream);
size_t bn_dwconv_fwd_workspace(int B, int C, int H, int W);
size_t bn_dwconv_bwd_workspace(int B, int C, int H, int W, int K);
hipError_t bn_dwconv_fwd_run(const float* z, const float* bn_w, const float* bn_b, float* run_mean, float* run_var,
                             const float* w, int B, int C, int H, int W, int K, int S, int act, int training,
                             float momentum, float eps, float* y, float* save_mean, float* save_invstd, void* ws,
                             hipStream_t stream);
hipError_t bn_dwconv_bwd_run(const float* dy, const float* z, const float* bn_w, const float* bn_b,
                             const float* save_mean, const float* save_invstd, const float* w, int B, int C, int H,
                             int W, int K, int S, int act, int training, float* dz, float* dbn_w, float* dbn_b,
                             float* dw, void* ws, hipStream_t stream);
// stem_conv.hip
size_t stem_conv_wrw_workspace(int B, int H, int W);
hipError_t stem_conv_fwd_run(const float* x, const float* w, int B, int H, int W, float* y, hipStream_t stream);
size_t stem_conv_bn_bwd_workspace(int B, int H, int W);
hipError_t stem_conv_bn_bwd_run(const float* g, const float* z, const float* x, const float* bn_weight, const float* bn_bias,
                                const float* save_mean, const float* save_invstd, int B, int H, int W, int training, float* dw,
                                float* dbn_weight, float* dbn_bias, void* ws, hipStream_t stream);
hipError_t stem_conv_wrw_run(const float* dy, const float* x, int B, int H, int W, float* dw, void* ws,
                             hipStream_t stream);
// pwconv_wide.hip / dwconv.hip: the BN form (thin convolution + BatchNorm backward in one walk)
bool pw_bn_bwd_supported(int Ci, int Co, int P);
void pw_bn_bwd_plan_query(int B, int Ci, int Co, int P, unsigned dx_align, int out[5]);
size_t pw_bn_act_bwd_workspace(int B, int Ci, int Co, int P);
hipError_t pw_bn_act_bwd_run(const float* g, const float* z, const float* x, const float* w, const float* bn_w, const float* bn_b,
                             const float* save_mean, const float* save_invstd, int B, int Ci, int Co, int P, int act, int training,
                             float* dx, float* dw, float* dbn_w, float* dbn_b, void* ws, hipStream_t stream);
size_t pw_bn_dwconv_bwd_workspace(int B, int Ci, int C, int H, int W, int K);
hipError_t pw_bn_dwconv_bwd_run(const float* dy, const float* z, const float* x, const float* pw_w, const float* bn_w,
                                const float* bn_b, const float* save_mean, const float* save_invstd, const float* w, int B, int Ci,
                                int C, int H, int W, int K, int S, int act, int training, float* dx, float* dpw_w, float* dbn_w,
                                float* dbn_b, float* dw, void* ws, hipStream_t stream);
// pwconv_wide.hip
bool pwconv_wide_supported(int Ci, int Co, int P);
void pwconv_wide_plan_query(int B, int Ci, int Co, int P, int out[5]);
size_t pwconv_wide_wgrad_workspace(int B, int Ci, int Co, int P);
hipError_t pwconv_wide_wgrad_run(const float* dy, const float* x, int B, int Ci, int Co, int P, float* dw, void* ws,
                                 hipStream_t stream);
// conv3x3_s2.hip
bool conv3x3s2_supported(int Ci, int Co);
long long conv3x3s2_wgrad_slabs(int B, int Ci, int H, int W);
size_t conv3x3s2_wgrad_workspace(int B, int Ci, int H, int W);
hipError_t conv3x3s2_wgrad_run(const float* dy, const float* x, int B, int Ci, int H, int W, float* dw, void* ws,
                               hipStream_t stream);
long long conv3x3s2_dgrad_workgroups(int B, int H, int W);
hipError_t conv3x3s2_dgrad_run(const float* dy, const float* w, int B, int H, int W, float* dx, hipStream_t stream);
bool conv3x3s2_fwd_supported(int Ci, int Co);
long long conv3x3s2_fwd_workgroups(int B, int H, int W);
hipError_t conv3x3s2_fwd_run(const float* x, const float* w, int B, int H, int W, float* y, hipStream_t stream);
// pwconv.hip
bool pwconv_supported(int Ci, int Co, int P);
void pwconv_stream_plan_query(int B, int M, int K, int P, unsigned x_align, unsigned y_align, int out[4]);
size_t pwconv_bwd_workspace(int B, int Ci, int Co, int P);
hipError_t pwconv_fwd_run(const float* x, const float* w, int B, int Ci, int Co, int P, float* y, hipStream_t stream);
hipError_t pwconv_bwd_run(const float* dy, const float* x, const float* w, int B, int Ci, int Co, int P, float* dx,
                          float* dw, void* ws, hipStream_t stream);
// ohem.hip
int ohem_blocks(int B, int H, int W);
hipError_t ohem_up_fwd_run(int nh, const float* const* low, const long long* labels, int B, int C, int Hl, int Wl, int H, int W,
                           float thresh, int ignore_lb, float* const* loss_px, float* const* blk_sum, int* const* blk_cnt,
                           const float* const* class_weight, hipStream_t stream, const float* focal_gamma = nullptr);
hipError_t focal_stats_run(const float* blk_sum, const int* blk_cnt, int nheads, int nblk, double* stats, hipStream_t stream);
hipError_t ohem_stats_run(const float* blk_sum, const int* blk_cnt, int nheads, int nblk, double* stats, hipStream_t stream);
size_t ohem_up_bwd_workspace(int B, int C, int H, int Wl);
bool ohem_up_supported(int C, int Wl, int W);
hipError_t ohem_up_bwd_run(int nh, const float* const* low, const long long* labels, const float* const* loss_px, int B, int C,
                           int Hl, int Wl, int H, int W, float thresh, int ignore_lb, float coef, float* dlow, void* ws,
                           const float* const* cw, const double* dsel, hipStream_t stream, const float* focal_gamma = nullptr);
size_t ohem_select_workspace(int nheads);
hipError_t ohem_select_run(int nheads, const float* const* loss_px, const long long* labels, const double* stats, long long P, int C,
                           float thresh, const int* n_min, int ignore_lb, const float* const* cw, double* sel, void* ws,
                           hipStream_t stream);
// conv3x3_wino.hip
struct WinoShape {
    int B, C0, C1, K, H, W;
};
bool conv3x3_supported(int C0, int C1, int K);
bool conv3x3_shape_ok(const WinoShape& s);
int conv3x3_tile_blocks(int B, int H, int W);
size_t conv3x3_fwd_workspace(const WinoShape& s);
size_t conv3x3_bwd_workspace(const WinoShape& s);
hipError_t conv3x3_fwd_run(const WinoShape& s, const float* x0, const float* x1, const float* w, float* y, float* stat_part, void* ws,
                           hipStream_t stream);
hipError_t conv3x3_bwd_run(const WinoShape& s, const float* dy, const float* x0, const float* x1, const float* w, float* dx0,
                           float* dx1, float* dw, void* ws, hipStream_t stream);
// eval_tail.hip
int eval_chip_threads(int C, int wl, int cw, int nsrc);
hipError_t eval_chip_accum_run(const float* a, const float* b, int N, int C, int hl, int wl, int ch, int cw, float* dst, int FH,
                               int FW, int y0, int x0, const float* rcp_y, const float* rcp_x, hipStream_t stream);
hipError_t eval_scale_merge_run(const float* prob, int N, int C, int FH, int FW, int hst, int hed, int wst, int wed, float* total,
                                int H, int W, hipStream_t stream);
hipError_t eval_argmax_hist_run(const float* total, const long long* labels, int N, int C, int H, int W, int ignore_lb, long long* hist,
                                unsigned char* pred, hipStream_t stream);
// predict_tail.hip
int predict_up_threads(int C, int wl, int W);
hipError_t predict_up_argmax_run(const float* a, int N, int C, int hl, int wl, int H, int W, unsigned char* labels, hipStream_t stream);
hipError_t predict_argmax_run(const float* total, int N, int C, int H, int W, unsigned char* labels, hipStream_t stream);
hipError_t predict_render_run(const unsigned char* labels, const float* image, const unsigned char* palette, int n_colors,
                              const float* mean, const float* std, float alpha, int N, int H, int W, unsigned char* pred,
                              unsigned char* inp, unsigned char* ovl, hipStream_t stream);
// augment_warp.hip
hipError_t augment_warp_run(const void* descs, int N, int max_oh, int max_ow, hipStream_t stream);
hipError_t augment_resize_run(const void* descs, int N, int max_oh, int max_ow, hipStream_t stream);
// augment.hip
size_t augment_workspace(int N, int th, int tw);
hipError_t augment_run(const void* samples, int N, int th, int tw, const float* noise, unsigned long long seed, const float* mean,
                       const float* std, float* out_image, long long* out_label, unsigned char* out_u8, void* workspace,
                       hipStream_t stream);
// opt_tail.hip
size_t sgd_tail_workspace(int n_chunks);
size_t sgd_tail_state(int n_entries);
hipError_t sgd_tail_run(const cabinet_sgd_tail_entry* entries, int n_entries, const cabinet_sgd_tail_chunk* chunks, int n_chunks,
                        const cabinet_sgd_tail_config& cfg, void* state, void* ws, int max_grid, hipStream_t stream);
// grad_accum.hip
size_t grad_accum_state();
hipError_t grad_accum_run(const cabinet_grad_accum_entry* entries, int n_entries, const cabinet_sgd_tail_chunk* chunks, int n_chunks,
                          void* state, int max_grid, hipStream_t stream);
hipError_t grad_accum_reset_run(void* state, hipStream_t stream);
}  // namespace cabinet

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// 128-bit loads / stores on activation rows: every tensor pointer named must be 16-byte aligned (include/cabinet_hip.h)
template <typename... P>
static bool aligned16(P... p) {
    return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}
#define CABINET_REQUIRE_ALIGNED(what, ...)                                                                            \
    if (!aligned16(__VA_ARGS__))                                                                                      \
    return fail(CABINET_ERR_INVALID_ARG, what ": tensor pointers must be 16-byte aligned (128-bit loads / stores)")

static int hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return CABINET_OK;
    return fail(CABINET_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

extern "C" {

int cabinet_abi_version(void) { return CABINET_ABI_VERSION; }
const char* cabinet_last_error(void) { return g_err; }

// ------------------------------------------------------------------ attention
static int check_attn_shape(int B, int Kc, int Vc, int n) {
    if (B <= 0 || Kc <= 0 || Vc <= 0 || n <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "cab_attn: non-positive dimension B=%d Kc=%d Vc=%d n=%d", B, Kc,
                    Vc, n);
    if (!cabinet::attn_shape_supported(Kc, Vc))
        return fail(CABINET_ERR_UNSUPPORTED,
                    "cab_attn: (Kc=%d, Vc=%d) has no gfx950 instantiation; built: (128,128) (256,128) (64,64)",
                    Kc, Vc);
    if (B > 65535) return fail(CABINET_ERR_UNSUPPORTED, "cab_attn: B=%d exceeds grid.z", B);
    return CABINET_OK;
}

int cabinet_cab_attn_supported(int Kc, int Vc) { return cabinet::attn_shape_supported(Kc, Vc) ? 1 : 0; }

int cabinet_cab_attn_precision_supported(int Kc, int Vc, int precision) {
    if (precision == CABINET_PREC_FP32) return cabinet_cab_attn_supported(Kc, Vc);
    if (precision == CABINET_PREC_BF16X3 || precision == CABINET_PREC_BF16X6) return cabinet::attn_bf16_supported(Kc, Vc) ? 1 : 0;
    return 0;
}

static size_t attn_fwd_split_bytes(int B, int Vc, int n, int split) {
    if (split == 1) return 0;
    return align_up((size_t)split * B * Vc * n * sizeof(float), 256) + align_up((size_t)split * B * n * sizeof(float), 256);
}

size_t cabinet_cab_attn_fwd_workspace_bytes(int B, int Kc, int Vc, int n, int precision) {
    if (B <= 0 || Kc <= 0 || Vc <= 0 || n <= 0 || !cabinet_cab_attn_precision_supported(Kc, Vc, precision)) return 0;
    const size_t pack = precision == CABINET_PREC_FP32 ? 0 : cabinet::attn_bf16_pack_bytes(B, Kc, Vc, n, precision);
    return attn_fwd_split_bytes(B, Vc, n, cabinet::attn_fwd_kvsplit(B, n)) + pack;
}

int cabinet_cab_attn_fwd(const float* q, const float* k, const float* v, float scale, int B, int Kc, int Vc,
                         int n, int precision, float* ctx, float* lse, void* workspace, size_t workspace_bytes,
                         cabinet_stream_t stream) {
    if (int rc = check_attn_shape(B, Kc, Vc, n)) return rc;
    if (!cabinet_cab_attn_precision_supported(Kc, Vc, precision))
        return fail(CABINET_ERR_UNSUPPORTED, "cab_attn_fwd: precision %d is not built for (Kc=%d, Vc=%d)", precision, Kc, Vc);
    if (!q || !k || !v || !ctx || !lse) return fail(CABINET_ERR_INVALID_ARG, "cab_attn_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("cab_attn_fwd", q, k, v, ctx, lse);
    const size_t need = cabinet_cab_attn_fwd_workspace_bytes(B, Kc, Vc, n, precision);
    if (need && (!workspace || workspace_bytes < need))
        return fail(CABINET_ERR_WORKSPACE, "cab_attn_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    const int split = cabinet::attn_fwd_kvsplit(B, n);
    float* part_ctx = static_cast<float*>(workspace);
    float* part_lse = split > 1 ? reinterpret_cast<float*>(static_cast<char*>(workspace) +
                                                           align_up((size_t)split * B * Vc * n * sizeof(float), 256))
                                : nullptr;
    if (precision != CABINET_PREC_FP32) {
        void* pack = static_cast<char*>(workspace) + attn_fwd_split_bytes(B, Vc, n, split);
        return hip_status(cabinet::attn_fwd_bf16_dispatch(q, k, v, scale, B, Kc, Vc, n, ctx, lse, part_ctx, part_lse, split, pack,
                                                          precision, static_cast<hipStream_t>(stream)),
                          "cab_attn_fwd (split bf16) launch");
    }
    return hip_status(cabinet::attn_fwd_dispatch(q, k, v, scale, B, Kc, Vc, n, ctx, lse, part_ctx, part_lse,
                                                 split, static_cast<hipStream_t>(stream)),
                      "cab_attn_fwd launch");
}

int cabinet_cab_attn_proj_supported(int B, int Kc, int Vc, int Co, int n) {
    return cabinet::attn_fwd_proj_supported(B, Kc, Vc, Co, n) ? 1 : 0;
}

int cabinet_cab_attn_proj_fwd(const float* q, const float* k, const float* v, const float* w_out, float scale, int B, int Kc,
                              int Vc, int Co, int n, float* ctx, float* glob, float* lse, cabinet_stream_t stream) {
    if (int rc = check_attn_shape(B, Kc, Vc, n)) return rc;
    if (Co <= 0) return fail(CABINET_ERR_INVALID_ARG, "cab_attn_proj_fwd: non-positive Co=%d", Co);
    if (!cabinet::attn_fwd_proj_supported(B, Kc, Vc, Co, n))
        return fail(CABINET_ERR_UNSUPPORTED,
                    "cab_attn_proj_fwd: (B=%d, Kc=%d, Vc=%d, Co=%d, n=%d) is outside the fused form (see "
                    "cabinet_cab_attn_proj_supported); use cabinet_cab_attn_fwd + cabinet_conv1x1_fwd",
                    B, Kc, Vc, Co, n);
    if (!q || !k || !v || !w_out || !glob || !lse) return fail(CABINET_ERR_INVALID_ARG, "cab_attn_proj_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("cab_attn_proj_fwd", q, k, v, w_out, ctx, glob, lse);
    return hip_status(cabinet::attn_fwd_proj_dispatch(q, k, v, w_out, scale, B, Kc, Vc, Co, n, ctx, glob, lse,
                                                      static_cast<hipStream_t>(stream)),
                      "cab_attn_proj_fwd launch");
}

size_t cabinet_cab_attn_bwd_workspace_bytes(int B, int Kc, int Vc, int n) {
    if (B <= 0 || Kc <= 0 || Vc <= 0 || n <= 0) return 0;
    return cabinet::attn_bwd_workspace(B, Kc, Vc, n);
}

int cabinet_cab_attn_bwd(const float* dctx, const float* q, const float* k, const float* v, const float* ctx,
                         const float* lse, float scale, int B, int Kc, int Vc, int n, float* dq, float* dk,
                         float* dv, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_attn_shape(B, Kc, Vc, n)) return rc;
    if (!dctx || !q || !k || !v || !ctx || !lse || !dq || !dk || !dv)
        return fail(CABINET_ERR_INVALID_ARG, "cab_attn_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("cab_attn_bwd", dctx, q, k, v, ctx, lse, dq, dk, dv);
    const size_t need = cabinet_cab_attn_bwd_workspace_bytes(B, Kc, Vc, n);
    if (need && (!workspace || workspace_bytes < need))
        return fail(CABINET_ERR_WORKSPACE, "cab_attn_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::attn_bwd_dispatch(dctx, q, k, v, ctx, lse, scale, B, Kc, Vc, n, dq, dk, dv,
                                                 workspace, static_cast<hipStream_t>(stream)),
                      "cab_attn_bwd launch");
}

// ------------------------------------------------------------------------ FFM
static int check_ffm_shape(int B, int Cs, int Cc, int Co, int Cm, int H, int W) {
    if (B <= 0 || Cs <= 0 || Cc <= 0 || Co <= 0 || Cm <= 0 || H <= 0 || W <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "ffm: non-positive dimension");
    if (Cs % 32 || Cc % 32 || Co % 32)
        return fail(CABINET_ERR_UNSUPPORTED, "ffm: Cs=%d Cc=%d Co=%d must be multiples of 32", Cs, Cc, Co);
    if (Cm > 256 || Co > 1024)
        return fail(CABINET_ERR_UNSUPPORTED, "ffm: Cm=%d (max 256) / Co=%d (max 1024) too large", Cm, Co);
    if (B > 65535) return fail(CABINET_ERR_UNSUPPORTED, "ffm: B=%d exceeds grid limits", B);
    return CABINET_OK;
}

size_t cabinet_ffm_fwd_workspace_bytes(int B, int Cs, int Cc, int Co, int Cm, int H, int W) {
    if (B <= 0 || Cs <= 0 || Cc <= 0 || Co <= 0 || Cm <= 0 || H <= 0 || W <= 0) return 0;
    return cabinet::ffm_fwd_workspace({B, Cs, Cc, Co, Cm, H, W});
}

int cabinet_ffm_fwd(const float* fsp, const float* fcp, const float* w_blk, const float* bn_weight,
                    const float* bn_bias, float* running_mean, float* running_var, const float* w1,
                    const float* w2, int B, int Cs, int Cc, int Co, int Cm, int H, int W, int training,
                    float momentum, float eps, float* out, float* z, float* save_mean, float* save_invstd,
                    float* pooled, float* gate, void* workspace, size_t workspace_bytes,
                    cabinet_stream_t stream) {
    if (int rc = check_ffm_shape(B, Cs, Cc, Co, Cm, H, W)) return rc;
    if (!fsp || !fcp || !w_blk || !bn_weight || !bn_bias || !running_mean || !running_var || !w1 || !w2 ||
        !out || !z || !save_mean || !save_invstd || !pooled || !gate)
        return fail(CABINET_ERR_INVALID_ARG, "ffm_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ffm_fwd", fsp, fcp, w_blk, out, z);
    const size_t need = cabinet_ffm_fwd_workspace_bytes(B, Cs, Cc, Co, Cm, H, W);
    if (need && (!workspace || workspace_bytes < need))
        return fail(CABINET_ERR_WORKSPACE, "ffm_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::ffm_fwd_run({B, Cs, Cc, Co, Cm, H, W}, fsp, fcp, w_blk, bn_weight, bn_bias,
                                           running_mean, running_var, w1, w2, training, momentum, eps, out, z,
                                           save_mean, save_invstd, pooled, gate, workspace,
                                           static_cast<hipStream_t>(stream)),
                      "ffm_fwd launch");
}

size_t cabinet_ffm_bwd_workspace_bytes(int B, int Cs, int Cc, int Co, int Cm, int H, int W) {
    if (B <= 0 || Cs <= 0 || Cc <= 0 || Co <= 0 || Cm <= 0 || H <= 0 || W <= 0) return 0;
    return cabinet::ffm_bwd_workspace({B, Cs, Cc, Co, Cm, H, W});
}

int cabinet_ffm_bwd(const float* dout, const float* fsp, const float* fcp, const float* w_blk,
                    const float* bn_weight, const float* bn_bias, const float* w1, const float* w2,
                    const float* z, const float* save_mean, const float* save_invstd, const float* pooled,
                    const float* gate, int B, int Cs, int Cc, int Co, int Cm, int H, int W, int training,
                    float* dfsp, float* dfcp, float* dw_blk, float* dbn_weight, float* dbn_bias, float* dw1,
                    float* dw2, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_ffm_shape(B, Cs, Cc, Co, Cm, H, W)) return rc;
    if (!dout || !fsp || !fcp || !w_blk || !bn_weight || !bn_bias || !w1 || !w2 || !z || !save_mean ||
        !save_invstd || !pooled || !gate || !dfsp || !dfcp || !dw_blk || !dbn_weight || !dbn_bias || !dw1 ||
        !dw2)
        return fail(CABINET_ERR_INVALID_ARG, "ffm_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ffm_bwd", dout, fsp, fcp, w_blk, z, dfsp, dfcp, dw_blk);
    const size_t need = cabinet_ffm_bwd_workspace_bytes(B, Cs, Cc, Co, Cm, H, W);
    if (need && (!workspace || workspace_bytes < need))
        return fail(CABINET_ERR_WORKSPACE, "ffm_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::ffm_bwd_run({B, Cs, Cc, Co, Cm, H, W}, dout, fsp, fcp, w_blk, bn_weight, bn_bias,
                                           w1, w2, z, save_mean, save_invstd, pooled, gate, training, dfsp,
                                           dfcp, dw_blk, dbn_weight, dbn_bias, dw1, dw2, workspace,
                                           static_cast<hipStream_t>(stream)),
                      "ffm_bwd launch");
}

// ------------------------------------------------------------- FFM + fused upsample
static int check_low(int Hl, int Wl) {
    if (Hl <= 0 || Wl <= 0) return fail(CABINET_ERR_INVALID_ARG, "ffm_up: non-positive low-resolution size");
    return CABINET_OK;
}

size_t cabinet_ffm_up_fwd_workspace_bytes(int B, int Cs, int Cc, int Co, int Cm, int H, int W, int Hl, int Wl) {
    if (B <= 0 || Cs <= 0 || Cc <= 0 || Co <= 0 || Cm <= 0 || H <= 0 || W <= 0 || Hl <= 0 || Wl <= 0) return 0;
    return cabinet::ffm_up_fwd_workspace({B, Cs, Cc, Co, Cm, H, W}, Hl, Wl);
}

int cabinet_ffm_up_fwd(const float* fsp, const float* low, const float* w_blk, const float* bn_weight,
                       const float* bn_bias, float* running_mean, float* running_var, const float* w1,
                       const float* w2, int B, int Cs, int Cc, int Co, int Cm, int H, int W, int Hl, int Wl,
                       int training, float momentum, float eps, int precision, float* out, float* z, float* save_mean,
                       float* save_invstd, float* pooled, float* gate, void* workspace, size_t workspace_bytes,
                       cabinet_stream_t stream) {
    if (int rc = check_ffm_shape(B, Cs, Cc, Co, Cm, H, W)) return rc;
    if (int rc = check_low(Hl, Wl)) return rc;
    if (precision < CABINET_PREC_FP32 || precision > CABINET_PREC_BF16X6)
        return fail(CABINET_ERR_INVALID_ARG, "ffm_up_fwd: unknown precision %d", precision);
    if (!fsp || !low || !w_blk || !bn_weight || !bn_bias || !running_mean || !running_var || !w1 || !w2 || !out ||
        !z || !save_mean || !save_invstd || !pooled || !gate)
        return fail(CABINET_ERR_INVALID_ARG, "ffm_up_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ffm_up_fwd", fsp, low, w_blk, out, z);
    const size_t need = cabinet_ffm_up_fwd_workspace_bytes(B, Cs, Cc, Co, Cm, H, W, Hl, Wl);
    if (need && (!workspace || workspace_bytes < need))
        return fail(CABINET_ERR_WORKSPACE, "ffm_up_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::ffm_up_fwd_run({B, Cs, Cc, Co, Cm, H, W}, Hl, Wl, fsp, low, w_blk, bn_weight, bn_bias,
                                              running_mean, running_var, w1, w2, training, momentum, eps, out, z,
                                              save_mean, save_invstd, pooled, gate, workspace, precision,
                                              static_cast<hipStream_t>(stream)),
                      "ffm_up_fwd launch");
}

size_t cabinet_ffm_up_bwd_workspace_bytes(int B, int Cs, int Cc, int Co, int Cm, int H, int W, int Hl, int Wl) {
    if (B <= 0 || Cs <= 0 || Cc <= 0 || Co <= 0 || Cm <= 0 || H <= 0 || W <= 0 || Hl <= 0 || Wl <= 0) return 0;
    return cabinet::ffm_up_bwd_workspace({B, Cs, Cc, Co, Cm, H, W}, Hl, Wl);
}

int cabinet_ffm_up_bwd(const float* dout, const float* fsp, const float* low, const float* w_blk,
                       const float* bn_weight, const float* bn_bias, const float* w1, const float* w2,
                       const float* z, const float* save_mean, const float* save_invstd, const float* pooled,
                       const float* gate, int B, int Cs, int Cc, int Co, int Cm, int H, int W, int Hl, int Wl,
                       int training, float* dfsp, float* dlow, float* dw_blk, float* dbn_weight, float* dbn_bias,
                       float* dw1, float* dw2, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_ffm_shape(B, Cs, Cc, Co, Cm, H, W)) return rc;
    if (int rc = check_low(Hl, Wl)) return rc;
    if (!dout || !fsp || !low || !w_blk || !bn_weight || !bn_bias || !w1 || !w2 || !z || !save_mean ||
        !save_invstd || !pooled || !gate || !dfsp || !dlow || !dw_blk || !dbn_weight || !dbn_bias || !dw1 || !dw2)
        return fail(CABINET_ERR_INVALID_ARG, "ffm_up_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ffm_up_bwd", dout, fsp, low, w_blk, z, dfsp, dlow, dw_blk);
    size_t lds_limit = 0;
    int band_rows = 0;
    if (const size_t lds = cabinet::ffm_up_bwd_adjoint_lds({B, Cs, Cc, Co, Cm, H, W}, Hl, Wl, &lds_limit, &band_rows); lds > lds_limit)
        return fail(CABINET_ERR_UNSUPPORTED,
                    "ffm_up_bwd: the resize %dx%d -> %dx%d is refused: one band of %d low-resolution rows of the resize adjoint would "
                    "stage %zu bytes of LDS (limit %zu); the staged band grows with H/Hl x W",
                    Hl, Wl, H, W, band_rows, lds, lds_limit);
    const size_t need = cabinet_ffm_up_bwd_workspace_bytes(B, Cs, Cc, Co, Cm, H, W, Hl, Wl);
    if (need && (!workspace || workspace_bytes < need))
        return fail(CABINET_ERR_WORKSPACE, "ffm_up_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::ffm_up_bwd_run({B, Cs, Cc, Co, Cm, H, W}, Hl, Wl, dout, fsp, low, w_blk, bn_weight,
                                              bn_bias, w1, w2, z, save_mean, save_invstd, pooled, gate, training,
                                              dfsp, dlow, dw_blk, dbn_weight, dbn_bias, dw1, dw2, workspace,
                                              static_cast<hipStream_t>(stream)),
                      "ffm_up_bwd launch");
}

// ------------------------------------------------------ OHEM-CE + fused upsample
static int check_ohem(int B, int C, int Hl, int Wl, int H, int W) {
    if (B <= 0 || C <= 0 || Hl <= 0 || Wl <= 0 || H <= 0 || W <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "ohem_up: non-positive dimension");
    if (C > 32) return fail(CABINET_ERR_UNSUPPORTED, "ohem_up: C=%d classes (max 32)", C);
    if (B > 65535 || H > 65535) return fail(CABINET_ERR_UNSUPPORTED, "ohem_up: B or H exceeds grid limits");
    if (!cabinet::ohem_up_supported(C, Wl, W))
        return fail(CABINET_ERR_UNSUPPORTED, "ohem_up: C=%d x Wl=%d (or the resize ratio %d/%d) exceeds the LDS row buffers",
                    C, Wl, W, Wl);
    return CABINET_OK;
}

int cabinet_ohem_up_blocks(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return cabinet::ohem_blocks(B, H, W);
}

// The class-weighted forms (`_w_`) carry the whole implementation; a null weight table selects the unweighted kernel
// instantiations, which is all the original entry points below them do.
int cabinet_ohem_up_w_fwd(const float* logits_low, const long long* labels, int B, int C, int Hl, int Wl, int H, int W,
                          float thresh, int ignore_lb, float* loss_px, float* blk_sum, int* blk_cnt,
                          const float* class_weight, cabinet_stream_t stream) {
    if (int rc = check_ohem(B, C, Hl, Wl, H, W)) return rc;
    if (!logits_low || !labels || !loss_px || !blk_sum || !blk_cnt)
        return fail(CABINET_ERR_INVALID_ARG, "ohem_up_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ohem_up_fwd", logits_low, labels, loss_px);
    return hip_status(cabinet::ohem_up_fwd_run(1, &logits_low, labels, B, C, Hl, Wl, H, W, thresh, ignore_lb, &loss_px, &blk_sum,
                                               &blk_cnt, &class_weight, static_cast<hipStream_t>(stream)),
                      "ohem_up_fwd launch");
}

int cabinet_ohem_up_fwd(const float* logits_low, const long long* labels, int B, int C, int Hl, int Wl, int H, int W,
                        float thresh, int ignore_lb, float* loss_px, float* blk_sum, int* blk_cnt,
                        cabinet_stream_t stream) {
    return cabinet_ohem_up_w_fwd(logits_low, labels, B, C, Hl, Wl, H, W, thresh, ignore_lb, loss_px, blk_sum, blk_cnt, nullptr,
                                 stream);
}

int cabinet_ohem_stats(const float* blk_sum, const int* blk_cnt, int nheads, int nblk, double* stats, cabinet_stream_t stream) {
    if (nheads <= 0 || nheads > 65535 || nblk <= 0) return fail(CABINET_ERR_INVALID_ARG, "ohem_stats: nheads=%d nblk=%d", nheads, nblk);
    if (!blk_sum || !blk_cnt || !stats) return fail(CABINET_ERR_INVALID_ARG, "ohem_stats: null tensor pointer");
    return hip_status(cabinet::ohem_stats_run(blk_sum, blk_cnt, nheads, nblk, stats, static_cast<hipStream_t>(stream)),
                      "ohem_stats launch");
}

size_t cabinet_ohem_up_bwd_workspace_bytes(int B, int C, int Hl, int Wl, int H, int W) {
    if (B <= 0 || C <= 0 || Hl <= 0 || Wl <= 0 || H <= 0 || W <= 0) return 0;
    return cabinet::ohem_up_bwd_workspace(B, C, H, Wl);
}

int cabinet_ohem_up_w_bwd(const float* logits_low, const long long* labels, const float* loss_px, int B, int C, int Hl,
                          int Wl, int H, int W, float thresh, int ignore_lb, float coef, float* dlogits_low,
                          void* workspace, size_t workspace_bytes, const float* class_weight, cabinet_stream_t stream) {
    if (int rc = check_ohem(B, C, Hl, Wl, H, W)) return rc;
    if (!logits_low || !labels || !loss_px || !dlogits_low)
        return fail(CABINET_ERR_INVALID_ARG, "ohem_up_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ohem_up_bwd", logits_low, labels, loss_px, dlogits_low);
    const size_t need = cabinet_ohem_up_bwd_workspace_bytes(B, C, Hl, Wl, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "ohem_up_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::ohem_up_bwd_run(1, &logits_low, labels, &loss_px, B, C, Hl, Wl, H, W, thresh, ignore_lb, coef,
                                               dlogits_low, workspace, &class_weight, nullptr, static_cast<hipStream_t>(stream)),
                      "ohem_up_bwd launch");
}

int cabinet_ohem_up_bwd(const float* logits_low, const long long* labels, const float* loss_px, int B, int C, int Hl,
                        int Wl, int H, int W, float thresh, int ignore_lb, float coef, float* dlogits_low,
                        void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    return cabinet_ohem_up_w_bwd(logits_low, labels, loss_px, B, C, Hl, Wl, H, W, thresh, ignore_lb, coef, dlogits_low, workspace,
                                 workspace_bytes, nullptr, stream);
}

// both loss heads of the step (same labels, same shapes) per launch
int cabinet_ohem_up_pair_w_fwd(const float* logits_low_a, const float* logits_low_b, const long long* labels, int B, int C,
                               int Hl, int Wl, int H, int W, float thresh, int ignore_lb, float* loss_px, float* blk_sum,
                               int* blk_cnt, const float* class_weight_a, const float* class_weight_b,
                               cabinet_stream_t stream) {
    if (int rc = check_ohem(B, C, Hl, Wl, H, W)) return rc;
    if (!logits_low_a || !logits_low_b || !labels || !loss_px || !blk_sum || !blk_cnt)
        return fail(CABINET_ERR_INVALID_ARG, "ohem_up_pair_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ohem_up_pair_fwd", logits_low_a, logits_low_b, labels, loss_px);
    const int nblk = cabinet::ohem_blocks(B, H, W);
    const float* low[2] = {logits_low_a, logits_low_b};
    float* lp[2] = {loss_px, loss_px + (size_t)B * H * W};
    float* bs[2] = {blk_sum, blk_sum + nblk};
    int* bc[2] = {blk_cnt, blk_cnt + 2 * nblk};
    const float* cw[2] = {class_weight_a, class_weight_b};
    return hip_status(cabinet::ohem_up_fwd_run(2, low, labels, B, C, Hl, Wl, H, W, thresh, ignore_lb, lp, bs, bc, cw,
                                               static_cast<hipStream_t>(stream)),
                      "ohem_up_pair_fwd launch");
}

int cabinet_ohem_up_pair_fwd(const float* logits_low_a, const float* logits_low_b, const long long* labels, int B, int C, int Hl,
                             int Wl, int H, int W, float thresh, int ignore_lb, float* loss_px, float* blk_sum, int* blk_cnt,
                             cabinet_stream_t stream) {
    return cabinet_ohem_up_pair_w_fwd(logits_low_a, logits_low_b, labels, B, C, Hl, Wl, H, W, thresh, ignore_lb, loss_px, blk_sum,
                                      blk_cnt, nullptr, nullptr, stream);
}

size_t cabinet_ohem_up_pair_bwd_workspace_bytes(int B, int C, int Hl, int Wl, int H, int W) {
    return 2 * cabinet_ohem_up_bwd_workspace_bytes(B, C, Hl, Wl, H, W);
}

int cabinet_ohem_up_pair_w_bwd(const float* logits_low_a, const float* logits_low_b, const long long* labels,
                               const float* loss_px, int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb,
                               float coef, float* dlogits_low, void* workspace, size_t workspace_bytes,
                               const float* class_weight_a, const float* class_weight_b, cabinet_stream_t stream) {
    if (int rc = check_ohem(B, C, Hl, Wl, H, W)) return rc;
    if (!logits_low_a || !logits_low_b || !labels || !loss_px || !dlogits_low)
        return fail(CABINET_ERR_INVALID_ARG, "ohem_up_pair_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ohem_up_pair_bwd", logits_low_a, logits_low_b, labels, loss_px, dlogits_low);
    const size_t need = cabinet_ohem_up_pair_bwd_workspace_bytes(B, C, Hl, Wl, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "ohem_up_pair_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    const float* low[2] = {logits_low_a, logits_low_b};
    const float* lp[2] = {loss_px, loss_px + (size_t)B * H * W};
    const float* cw[2] = {class_weight_a, class_weight_b};
    return hip_status(cabinet::ohem_up_bwd_run(2, low, labels, lp, B, C, Hl, Wl, H, W, thresh, ignore_lb, coef, dlogits_low,
                                               workspace, cw, nullptr, static_cast<hipStream_t>(stream)),
                      "ohem_up_pair_bwd launch");
}

int cabinet_ohem_up_pair_bwd(const float* logits_low_a, const float* logits_low_b, const long long* labels, const float* loss_px,
                             int B, int C, int Hl, int Wl, int H, int W, float thresh, int ignore_lb, float coef,
                             float* dlogits_low, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    return cabinet_ohem_up_pair_w_bwd(logits_low_a, logits_low_b, labels, loss_px, B, C, Hl, Wl, H, W, thresh, ignore_lb, coef,
                                      dlogits_low, workspace, workspace_bytes, nullptr, nullptr, stream);
}

// The top-n_min branch on the device: selection into sel (nheads,4), then the backward kernels read [t, tie] from it.
size_t cabinet_ohem_select_workspace_bytes(int nheads, int B, int H, int W) {
    if (nheads < 1 || nheads > 2 || B <= 0 || H <= 0 || W <= 0) return 0;
    return cabinet::ohem_select_workspace(nheads);
}

int cabinet_ohem_select(const float* loss_px, const long long* labels, const double* stats, int nheads, int B, int C, int H, int W,
                        float thresh, int n_min_a, int n_min_b, int ignore_lb, const float* class_weight_a,
                        const float* class_weight_b, double* sel, void* workspace, size_t workspace_bytes,
                        cabinet_stream_t stream) {
    if (nheads < 1 || nheads > 2) return fail(CABINET_ERR_INVALID_ARG, "ohem_select: nheads=%d (1 or 2)", nheads);
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(CABINET_ERR_INVALID_ARG, "ohem_select: non-positive dimension");
    if (C > 32) return fail(CABINET_ERR_UNSUPPORTED, "ohem_select: C=%d classes (max 32)", C);
    if ((long long)B * H * W >= (1ll << 31)) return fail(CABINET_ERR_UNSUPPORTED, "ohem_select: B*H*W exceeds 2^31 - 1 pixels");
    if (n_min_a < 0 || n_min_b < 0) return fail(CABINET_ERR_INVALID_ARG, "ohem_select: negative n_min");
    if (!loss_px || !labels || !stats || !sel) return fail(CABINET_ERR_INVALID_ARG, "ohem_select: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ohem_select", loss_px, labels, stats, sel, workspace);
    const size_t need = cabinet_ohem_select_workspace_bytes(nheads, B, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "ohem_select: workspace %zu < %zu bytes", workspace_bytes, need);
    const long long P = (long long)B * H * W;
    const float* lp[2] = {loss_px, loss_px + (nheads == 2 ? P : 0)};
    const float* cw[2] = {class_weight_a, class_weight_b};
    const int n_min[2] = {n_min_a, n_min_b};
    return hip_status(cabinet::ohem_select_run(nheads, lp, labels, stats, P, C, thresh, n_min, ignore_lb, cw, sel, workspace,
                                               static_cast<hipStream_t>(stream)),
                      "ohem_select launch");
}

int cabinet_ohem_up_w_bwd_sel(const float* logits_low, const long long* labels, const float* loss_px, int B, int C, int Hl,
                              int Wl, int H, int W, const double* sel, int ignore_lb, float coef, float* dlogits_low,
                              void* workspace, size_t workspace_bytes, const float* class_weight, cabinet_stream_t stream) {
    if (int rc = check_ohem(B, C, Hl, Wl, H, W)) return rc;
    if (!logits_low || !labels || !loss_px || !dlogits_low || !sel)
        return fail(CABINET_ERR_INVALID_ARG, "ohem_up_bwd_sel: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ohem_up_bwd_sel", logits_low, labels, loss_px, dlogits_low, sel);
    const size_t need = cabinet_ohem_up_bwd_workspace_bytes(B, C, Hl, Wl, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "ohem_up_bwd_sel: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::ohem_up_bwd_run(1, &logits_low, labels, &loss_px, B, C, Hl, Wl, H, W, 0.f, ignore_lb, coef,
                                               dlogits_low, workspace, &class_weight, sel, static_cast<hipStream_t>(stream)),
                      "ohem_up_bwd_sel launch");
}

int cabinet_ohem_up_pair_w_bwd_sel(const float* logits_low_a, const float* logits_low_b, const long long* labels,
                                   const float* loss_px, int B, int C, int Hl, int Wl, int H, int W, const double* sel,
                                   int ignore_lb, float coef, float* dlogits_low, void* workspace, size_t workspace_bytes,
                                   const float* class_weight_a, const float* class_weight_b, cabinet_stream_t stream) {
    if (int rc = check_ohem(B, C, Hl, Wl, H, W)) return rc;
    if (!logits_low_a || !logits_low_b || !labels || !loss_px || !dlogits_low || !sel)
        return fail(CABINET_ERR_INVALID_ARG, "ohem_up_pair_bwd_sel: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("ohem_up_pair_bwd_sel", logits_low_a, logits_low_b, labels, loss_px, dlogits_low, sel);
    const size_t need = cabinet_ohem_up_pair_bwd_workspace_bytes(B, C, Hl, Wl, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "ohem_up_pair_bwd_sel: workspace %zu < %zu bytes", workspace_bytes, need);
    const float* low[2] = {logits_low_a, logits_low_b};
    const float* lp[2] = {loss_px, loss_px + (size_t)B * H * W};
    const float* cw[2] = {class_weight_a, class_weight_b};
    return hip_status(cabinet::ohem_up_bwd_run(2, low, labels, lp, B, C, Hl, Wl, H, W, 0.f, ignore_lb, coef, dlogits_low,
                                               workspace, cw, sel, static_cast<hipStream_t>(stream)),
                      "ohem_up_pair_bwd_sel launch");
}

// ------------------------------------------------------ softmax focal loss + fused upsample (the OHEM kernels' focal mode)
static bool focal_gamma_ok(float gamma) { return gamma >= 0.f && gamma <= 3.0e38f; }  // false for NaN and +inf as well

int cabinet_focal_up_supported(int C, int Hl, int Wl, int H, int W, float gamma) {
    if (!focal_gamma_ok(gamma)) {
        fail(CABINET_ERR_UNSUPPORTED, "focal_up: gamma=%g (needs a finite gamma >= 0)", (double)gamma);
        return 0;
    }
    return check_ohem(1, C, Hl, Wl, H, W) == CABINET_OK ? 1 : 0;  // check_ohem leaves its reason in cabinet_last_error()
}

int cabinet_focal_up_fwd(const float* logits_low_a, const float* logits_low_b, const long long* labels, int B, int C, int Hl,
                         int Wl, int H, int W, float gamma_a, float gamma_b, int ignore_lb, float* loss_px, float* blk_sum,
                         int* blk_cnt, const float* class_weight_a, const float* class_weight_b, cabinet_stream_t stream) {
    if (int rc = check_ohem(B, C, Hl, Wl, H, W)) return rc;
    const int nh = logits_low_b ? 2 : 1;
    if (!focal_gamma_ok(gamma_a) || (nh == 2 && !focal_gamma_ok(gamma_b)))
        return fail(CABINET_ERR_UNSUPPORTED, "focal_up_fwd: gamma=%g / %g (needs a finite gamma >= 0)", (double)gamma_a,
                    (double)gamma_b);
    if (!logits_low_a || !labels || !loss_px || !blk_sum || !blk_cnt)
        return fail(CABINET_ERR_INVALID_ARG, "focal_up_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("focal_up_fwd", logits_low_a, logits_low_b, labels, loss_px, blk_sum);
    const int nblk = cabinet::ohem_blocks(B, H, W);
    const float* low[2] = {logits_low_a, logits_low_b};
    float* lp[2] = {loss_px, loss_px + (size_t)B * H * W};
    float* bs[2] = {blk_sum, blk_sum + 2 * (size_t)nblk};
    int* bc[2] = {blk_cnt, blk_cnt + nblk};
    const float* cw[2] = {class_weight_a, class_weight_b};
    const float gm[2] = {gamma_a, gamma_b};
    return hip_status(cabinet::ohem_up_fwd_run(nh, low, labels, B, C, Hl, Wl, H, W, 0.f, ignore_lb, lp, bs, bc, cw,
                                               static_cast<hipStream_t>(stream), gm),
                      "focal_up_fwd launch");
}

int cabinet_focal_stats(const float* blk_sum, const int* blk_cnt, int nheads, int nblk, double* stats, cabinet_stream_t stream) {
    if (nheads <= 0 || nheads > 65535 || nblk <= 0) return fail(CABINET_ERR_INVALID_ARG, "focal_stats: nheads=%d nblk=%d", nheads, nblk);
    if (!blk_sum || !blk_cnt || !stats) return fail(CABINET_ERR_INVALID_ARG, "focal_stats: null tensor pointer");
    if ((reinterpret_cast<uintptr_t>(blk_sum) & 7) != 0) return fail(CABINET_ERR_INVALID_ARG, "focal_stats: blk_sum is not 8-byte aligned");
    return hip_status(cabinet::focal_stats_run(blk_sum, blk_cnt, nheads, nblk, stats, static_cast<hipStream_t>(stream)),
                      "focal_stats launch");
}

size_t cabinet_focal_up_bwd_workspace_bytes(int nheads, int B, int C, int Hl, int Wl, int H, int W) {
    if (nheads < 1 || nheads > 2) return 0;
    return (size_t)nheads * cabinet_ohem_up_bwd_workspace_bytes(B, C, Hl, Wl, H, W);
}

int cabinet_focal_up_bwd(const float* logits_low_a, const float* logits_low_b, const long long* labels, const float* loss_px,
                         int B, int C, int Hl, int Wl, int H, int W, float gamma_a, float gamma_b, int ignore_lb, float coef,
                         float* dlogits_low, void* workspace, size_t workspace_bytes, const float* class_weight_a,
                         const float* class_weight_b, cabinet_stream_t stream) {
    if (int rc = check_ohem(B, C, Hl, Wl, H, W)) return rc;
    const int nh = logits_low_b ? 2 : 1;
    if (!focal_gamma_ok(gamma_a) || (nh == 2 && !focal_gamma_ok(gamma_b)))
        return fail(CABINET_ERR_UNSUPPORTED, "focal_up_bwd: gamma=%g / %g (needs a finite gamma >= 0)", (double)gamma_a,
                    (double)gamma_b);
    if (!logits_low_a || !labels || !loss_px || !dlogits_low)
        return fail(CABINET_ERR_INVALID_ARG, "focal_up_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("focal_up_bwd", logits_low_a, logits_low_b, labels, loss_px, dlogits_low);
    const size_t need = cabinet_focal_up_bwd_workspace_bytes(nh, B, C, Hl, Wl, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "focal_up_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    const float* low[2] = {logits_low_a, logits_low_b};
    const float* lp[2] = {loss_px, loss_px + (size_t)B * H * W};
    const float* cw[2] = {class_weight_a, class_weight_b};
    const float gm[2] = {gamma_a, gamma_b};
    return hip_status(cabinet::ohem_up_bwd_run(nh, low, labels, lp, B, C, Hl, Wl, H, W, 0.f, ignore_lb, coef, dlogits_low,
                                               workspace, cw, nullptr, static_cast<hipStream_t>(stream), gm),
                      "focal_up_bwd launch");
}

// ------------------------------------------------------ CAB local branch + block output
// two forms behind one entry point: the channel-resident kernel (B*H*W <= 8192, no workspace) and the tiled
// multi-workgroup-per-channel form for everything larger (cab_local_tiled.hip)
static int check_local(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(CABINET_ERR_INVALID_ARG, "cab_local: non-positive dimension");
    if (C > 65535) return fail(CABINET_ERR_UNSUPPORTED, "cab_local: C = %d exceeds the grid's 65535 channels", C);
    if (!cabinet::local_shape_supported(B, H, W) && !cabinet::local_tiled_supported(B, H, W))
        return fail(CABINET_ERR_UNSUPPORTED, "cab_local: %d x %d x %d planes fit neither the resident nor the tiled form", B, H, W);
    return CABINET_OK;
}

int cabinet_cab_local_supported(int B, int C, int H, int W) {
    return B > 0 && C > 0 && C <= 65535 && H > 0 && W > 0 &&
                   (cabinet::local_shape_supported(B, H, W) || cabinet::local_tiled_supported(B, H, W))
               ? 1
               : 0;
}

size_t cabinet_cab_local_fwd_workspace_bytes(int B, int C, int H, int W) {
    if (!cabinet_cab_local_supported(B, C, H, W) || cabinet::local_shape_supported(B, H, W)) return 0;
    return cabinet::local_tiled_fwd_workspace(B, C, H, W);
}

size_t cabinet_cab_local_bwd_workspace_bytes(int B, int C, int H, int W) {
    if (!cabinet_cab_local_supported(B, C, H, W) || cabinet::local_shape_supported(B, H, W)) return 0;
    return cabinet::local_tiled_bwd_workspace(B, C, H, W);
}

int cabinet_cab_local_fwd(const float* x, const float* glob, const float* gamma, const float* const* dw_w,
                          const float* const* bn_weight, const float* const* bn_bias, float* const* running_mean,
                          float* const* running_var, int B, int C, int H, int W, int training, float momentum,
                          float eps, float* out, float* save_mean, float* save_invstd, void* workspace,
                          size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_local(B, C, H, W)) return rc;
    if (!x || !out || !save_mean || !save_invstd || !dw_w || !bn_weight || !bn_bias || !running_mean || !running_var)
        return fail(CABINET_ERR_INVALID_ARG, "cab_local_fwd: null tensor pointer");
    if (glob && !gamma) return fail(CABINET_ERR_INVALID_ARG, "cab_local_fwd: glob given without gamma");
    const size_t need = cabinet_cab_local_fwd_workspace_bytes(B, C, H, W);
    if (need && (!workspace || workspace_bytes < need))
        return fail(CABINET_ERR_WORKSPACE, "cab_local_fwd: workspace %zu < %zu", workspace_bytes, need);
    cabinet::LocalArgs a{};
    a.x = x, a.glob = glob, a.gamma = gamma;
    for (int s = 0; s < 3; ++s) {
        if (!dw_w[s] || !bn_weight[s] || !bn_bias[s] || !running_mean[s] || !running_var[s])
            return fail(CABINET_ERR_INVALID_ARG, "cab_local_fwd: null parameter pointer (stage %d)", s);
        a.st[s].w = dw_w[s], a.st[s].bn_w = bn_weight[s], a.st[s].bn_b = bn_bias[s];
        a.st[s].run_mean = running_mean[s], a.st[s].run_var = running_var[s];
    }
    a.B = B, a.C = C, a.H = H, a.W = W, a.training = training, a.momentum = momentum, a.eps = eps;
    a.out = out, a.save_mean = save_mean, a.save_invstd = save_invstd;
    if (need) return hip_status(cabinet::cab_local_tiled_fwd_run(a, workspace, static_cast<hipStream_t>(stream)), "cab_local_fwd launch");
    return hip_status(cabinet::cab_local_fwd_run(a, static_cast<hipStream_t>(stream)), "cab_local_fwd launch");
}

int cabinet_cab_local_bwd(const float* dout, const float* x, const float* glob, const float* gamma,
                          const float* const* dw_w, const float* const* bn_weight, const float* const* bn_bias,
                          const float* save_mean, const float* save_invstd, int B, int C, int H, int W, int training,
                          float* dx, float* dglob, float* dgamma_part, float* const* ddw_w, float* const* dbn_weight,
                          float* const* dbn_bias, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_local(B, C, H, W)) return rc;
    if (!dout || !x || !dx || !save_mean || !save_invstd || !dw_w || !bn_weight || !bn_bias || !ddw_w || !dbn_weight ||
        !dbn_bias)
        return fail(CABINET_ERR_INVALID_ARG, "cab_local_bwd: null tensor pointer");
    if (glob && (!gamma || !dglob || !dgamma_part))
        return fail(CABINET_ERR_INVALID_ARG, "cab_local_bwd: glob given without gamma / dglob / dgamma_part");
    const size_t need = cabinet_cab_local_bwd_workspace_bytes(B, C, H, W);
    if (need && (!workspace || workspace_bytes < need))
        return fail(CABINET_ERR_WORKSPACE, "cab_local_bwd: workspace %zu < %zu", workspace_bytes, need);
    cabinet::LocalArgs a{};
    a.x = x, a.glob = glob, a.gamma = gamma, a.dout = dout;
    for (int s = 0; s < 3; ++s) {
        if (!dw_w[s] || !bn_weight[s] || !bn_bias[s] || !ddw_w[s] || !dbn_weight[s] || !dbn_bias[s])
            return fail(CABINET_ERR_INVALID_ARG, "cab_local_bwd: null parameter pointer (stage %d)", s);
        a.st[s].w = dw_w[s], a.st[s].bn_w = bn_weight[s], a.st[s].bn_b = bn_bias[s];
        a.st[s].dw = ddw_w[s], a.st[s].dbn_w = dbn_weight[s], a.st[s].dbn_b = dbn_bias[s];
    }
    a.B = B, a.C = C, a.H = H, a.W = W, a.training = training;
    a.save_mean = const_cast<float*>(save_mean), a.save_invstd = const_cast<float*>(save_invstd);
    a.dx = dx, a.dglob = dglob, a.dgamma_part = dgamma_part;
    if (need) return hip_status(cabinet::cab_local_tiled_bwd_run(a, workspace, static_cast<hipStream_t>(stream)), "cab_local_bwd launch");
    return hip_status(cabinet::cab_local_bwd_run(a, static_cast<hipStream_t>(stream)), "cab_local_bwd launch");
}

// ------------------------------------------------------ q/k/v producers
static int qkv_shape(int B, int C, int Kc, int Vc, int H, int W, int ns, const int* sizes, cabinet::QkvShape& s,
                     const char* who) {
    if (B <= 0 || C <= 0 || Kc <= 0 || Vc <= 0 || H <= 0 || W <= 0 || !sizes)
        return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension or null sizes", who);
    if (ns < 1 || ns > 4) return fail(CABINET_ERR_UNSUPPORTED, "%s: n_sizes=%d (1..4)", who, ns);
    s = cabinet::QkvShape{B, C, Kc, Vc, H, W, ns, {0, 0, 0, 0}};
    for (int i = 0; i < ns; ++i) s.sizes[i] = sizes[i];
    if (const char* need = cabinet::qkv_unsupported(s)) return fail(CABINET_ERR_UNSUPPORTED, "%s: needs %s", who, need);
    if ((long long)B * (2 * Kc + Vc) > 2147483647LL / 2) return fail(CABINET_ERR_UNSUPPORTED, "%s: grid too large", who);
    return CABINET_OK;
}

int cabinet_cab_qkv_supported(int B, int C, int Kc, int Vc, int H, int W, int n_sizes, const int* sizes) {
    cabinet::QkvShape s;
    return qkv_shape(B, C, Kc, Vc, H, W, n_sizes, sizes, s, "cab_qkv") == CABINET_OK ? 1 : 0;
}

int cabinet_cab_qkv_padded_bins(int n_sizes, const int* sizes) {
    if (n_sizes < 1 || n_sizes > 4 || !sizes) return 0;
    cabinet::QkvShape s{1, 16, 16, 16, 1, 1, n_sizes, {0, 0, 0, 0}};
    for (int i = 0; i < n_sizes; ++i) s.sizes[i] = sizes[i];
    return cabinet::qkv_padded_bins(s);
}

size_t cabinet_cab_qkv_fwd_workspace_bytes(int B, int C, int Kc, int Vc, int H, int W, int n_sizes, const int* sizes) {
    cabinet::QkvShape s;
    if (qkv_shape(B, C, Kc, Vc, H, W, n_sizes, sizes, s, "cab_qkv_fwd")) return 0;
    return cabinet::qkv_fwd_workspace(s);
}

int cabinet_cab_qkv_fwd(const float* x, const float* wq, const float* wk, const float* wv, const float* bnq_weight,
                        const float* bnq_bias, float* bnq_running_mean, float* bnq_running_var,
                        const float* bnk_weight, const float* bnk_bias, float* bnk_running_mean,
                        float* bnk_running_var, const float* wpk, const float* wpv, int B, int C, int Kc, int Vc, int H,
                        int W, int n_sizes, const int* sizes, int training, float momentum, float eps, float* q,
                        float* k, float* v, float* zqk, float* vv, float* kk, float* pooled_k, float* pooled_v,
                        float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                        cabinet_stream_t stream) {
    cabinet::QkvShape s;
    if (int rc = qkv_shape(B, C, Kc, Vc, H, W, n_sizes, sizes, s, "cab_qkv_fwd")) return rc;
    if (!x || !wq || !wk || !wv || !bnq_weight || !bnq_bias || !bnq_running_mean || !bnq_running_var || !bnk_weight ||
        !bnk_bias || !bnk_running_mean || !bnk_running_var || !wpk || !wpv || !q || !k || !v || !zqk || !vv || !kk ||
        !pooled_k || !pooled_v || !save_mean || !save_invstd)
        return fail(CABINET_ERR_INVALID_ARG, "cab_qkv_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("cab_qkv_fwd", x, q, k, v, zqk, vv, kk);
    const size_t need = cabinet::qkv_fwd_workspace(s);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "cab_qkv_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    const cabinet::QkvParams w{wq, wk, wv, bnq_weight, bnq_bias, bnk_weight, bnk_bias, bnq_running_mean,
                               bnq_running_var, bnk_running_mean, bnk_running_var, wpk, wpv};
    const cabinet::QkvSaved sv{zqk, vv, kk, pooled_k, pooled_v, save_mean, save_invstd};
    return hip_status(cabinet::qkv_fwd_run(s, w, x, training, momentum, eps, sv, q, k, v, workspace,
                                           static_cast<hipStream_t>(stream)),
                      "cab_qkv_fwd launch");
}

size_t cabinet_cab_qkv_bwd_workspace_bytes(int B, int C, int Kc, int Vc, int H, int W, int n_sizes, const int* sizes) {
    cabinet::QkvShape s;
    if (qkv_shape(B, C, Kc, Vc, H, W, n_sizes, sizes, s, "cab_qkv_bwd")) return 0;
    return cabinet::qkv_bwd_workspace(s);
}

int cabinet_cab_qkv_bwd(const float* dq, const float* dk, const float* dv, const float* x, const float* wq,
                        const float* wk, const float* wv, const float* bnq_weight, const float* bnq_bias,
                        const float* bnk_weight, const float* bnk_bias, const float* wpk, const float* wpv,
                        const float* zqk, const float* vv, const float* kk, const float* pooled_k,
                        const float* pooled_v, const float* save_mean, const float* save_invstd, int B, int C, int Kc,
                        int Vc, int H, int W, int n_sizes, const int* sizes, int training, float* dx, float* dwqk,
                        float* dwv, float* dbnq_weight, float* dbnq_bias, float* dbnk_weight, float* dbnk_bias,
                        float* dwpk, float* dwpv, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    cabinet::QkvShape s;
    if (int rc = qkv_shape(B, C, Kc, Vc, H, W, n_sizes, sizes, s, "cab_qkv_bwd")) return rc;
    if (!dq || !dk || !dv || !x || !wq || !wk || !wv || !bnq_weight || !bnq_bias || !bnk_weight || !bnk_bias || !wpk ||
        !wpv || !zqk || !vv || !kk || !pooled_k || !pooled_v || !save_mean || !save_invstd || !dx || !dwqk || !dwv ||
        !dbnq_weight || !dbnq_bias || !dbnk_weight || !dbnk_bias || !dwpk || !dwpv)
        return fail(CABINET_ERR_INVALID_ARG, "cab_qkv_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("cab_qkv_bwd", dq, dk, dv, x, zqk, vv, kk, dx);
    const size_t need = cabinet::qkv_bwd_workspace(s);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "cab_qkv_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    const cabinet::QkvParams w{wq, wk, wv, bnq_weight, bnq_bias, bnk_weight, bnk_bias, nullptr, nullptr, nullptr,
                               nullptr, wpk, wpv};
    const cabinet::QkvSaved sv{const_cast<float*>(zqk), const_cast<float*>(vv), const_cast<float*>(kk),
                               const_cast<float*>(pooled_k), const_cast<float*>(pooled_v),
                               const_cast<float*>(save_mean), const_cast<float*>(save_invstd)};
    const cabinet::QkvGrads gr{dx, dwqk, dwv, dbnq_weight, dbnq_bias, dbnk_weight, dbnk_bias, dwpk, dwpv};
    return hip_status(cabinet::qkv_bwd_run(s, w, dq, dk, dv, x, training, sv, gr, workspace,
                                           static_cast<hipStream_t>(stream)),
                      "cab_qkv_bwd launch");
}

// ------------------------------------------------------ bias-free 1x1 convolution
static int check_conv1x1(int B, int Ci, int Co, int P, const char* who) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || P <= 0) return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension", who);
    if ((Ci % 4) || (Co % 4))
        return fail(CABINET_ERR_UNSUPPORTED, "%s: Ci=%d, Co=%d must be multiples of 4", who, Ci, Co);
    if (B > 65535) return fail(CABINET_ERR_UNSUPPORTED, "%s: B exceeds grid limits", who);
    return CABINET_OK;
}

size_t cabinet_conv1x1_fwd_workspace_bytes(int Ci, int Co) {
    return Ci > 0 && Co > 0 ? cabinet::conv1x1_fwd_workspace(Ci, Co) : 0;
}

int cabinet_conv1x1_fwd(const float* x, const float* w, int B, int Ci, int Co, int P, float* y, void* workspace,
                        size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_conv1x1(B, Ci, Co, P, "conv1x1_fwd")) return rc;
    if (!x || !w || !y) return fail(CABINET_ERR_INVALID_ARG, "conv1x1_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("conv1x1_fwd", x, w, y);
    const size_t need = cabinet::conv1x1_fwd_workspace(Ci, Co);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "conv1x1_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::conv1x1_fwd_run(x, w, B, Ci, Co, P, y, workspace, static_cast<hipStream_t>(stream)),
                      "conv1x1_fwd launch");
}

int cabinet_conv1x1_bias_supported(int B, int Ci, int Co, int P) {
    return (B > 0 && Ci > 0 && Co > 0 && P > 0 && cabinet::conv1x1_bias_supported(B, Ci, Co, P)) ? 1 : 0;
}

int cabinet_conv1x1_bias_fwd(const float* x, const float* w, const float* bias, int B, int Ci, int Co, int P, float* y, void* workspace,
                             size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_conv1x1(B, Ci, Co, P, "conv1x1_bias_fwd")) return rc;
    if (!x || !w || !bias || !y) return fail(CABINET_ERR_INVALID_ARG, "conv1x1_bias_fwd: null tensor pointer");
    if (!cabinet::conv1x1_bias_supported(B, Ci, Co, P))
        return fail(CABINET_ERR_UNSUPPORTED, "conv1x1_bias_fwd: (B=%d, Ci=%d, Co=%d, P=%d) is outside the small-grid path "
                    "(cabinet_conv1x1_bias_supported)", B, Ci, Co, P);
    CABINET_REQUIRE_ALIGNED("conv1x1_bias_fwd", x, w, y);
    const size_t need = cabinet::conv1x1_fwd_workspace(Ci, Co);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "conv1x1_bias_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::conv1x1_fwd_run(x, w, B, Ci, Co, P, y, workspace, static_cast<hipStream_t>(stream), bias),
                      "conv1x1_bias_fwd launch");
}

int cabinet_channel_sum(const float* d, int B, int C, int P, float* out, cabinet_stream_t stream) {
    if (B <= 0 || C <= 0 || P <= 0) return fail(CABINET_ERR_INVALID_ARG, "channel_sum: non-positive dimension");
    if (!d || !out) return fail(CABINET_ERR_INVALID_ARG, "channel_sum: null tensor pointer");
    return hip_status(cabinet::channel_sum_run(d, B, C, P, out, static_cast<hipStream_t>(stream)), "channel_sum launch");
}

size_t cabinet_conv1x1_bwd_workspace_bytes(int B, int Ci, int Co, int P) {
    return B > 0 && Ci > 0 && Co > 0 && P > 0 ? cabinet::conv1x1_bwd_workspace(B, Ci, Co, P) : 0;
}

int cabinet_conv1x1_bwd(const float* dy, const float* x, const float* w, int B, int Ci, int Co, int P, float* dx,
                        float* dw, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_conv1x1(B, Ci, Co, P, "conv1x1_bwd")) return rc;
    if (!dy || !x || !w) return fail(CABINET_ERR_INVALID_ARG, "conv1x1_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("conv1x1_bwd", dy, x, w, dx, dw);
    const size_t need = cabinet::conv1x1_bwd_workspace(B, Ci, Co, P);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "conv1x1_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::conv1x1_bwd_run(dy, x, w, B, Ci, Co, P, dx, dw, workspace, static_cast<hipStream_t>(stream)),
                      "conv1x1_bwd launch");
}

// ------------------------------------------------------ BatchNorm2d + activation
static int check_bn_act(int B, int C, int P, int act, const char* who) {
    if (B <= 0 || C <= 0 || P <= 0) return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension", who);
    if (act < 0 || act > 2) return fail(CABINET_ERR_INVALID_ARG, "%s: act=%d (0 none, 1 relu, 2 hardswish)", who, act);
    if ((long long)B * C * ((P + 8191) / 8192) > 2147483647LL)
        return fail(CABINET_ERR_UNSUPPORTED, "%s: grid too large", who);
    return CABINET_OK;
}

size_t cabinet_bn_act_workspace_bytes(int B, int C, int P) {
    return B > 0 && C > 0 && P > 0 ? cabinet::bn_act_workspace(B, C, P) : 0;
}

int cabinet_bn_act_fwd(const float* x, const float* weight, const float* bias, float* running_mean, float* running_var,
                       const float* residual, int B, int C, int P, int act, int training, float momentum, float eps, float* y,
                       float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                       cabinet_stream_t stream) {
    if (int rc = check_bn_act(B, C, P, act, "bn_act_fwd")) return rc;
    if (!x || !weight || !bias || !running_mean || !running_var || !y || !save_mean || !save_invstd)
        return fail(CABINET_ERR_INVALID_ARG, "bn_act_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("bn_act_fwd", x, residual, y);
    const size_t need = cabinet::bn_act_workspace(B, C, P);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "bn_act_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::bn_act_fwd_run(x, weight, bias, running_mean, running_var, residual, B, C, P, act, training,
                                              momentum, eps, y, save_mean, save_invstd, workspace,
                                              static_cast<hipStream_t>(stream)),
                      "bn_act_fwd launch");
}

int cabinet_bn_act_fwd_part(const float* x, const float* conv_part, const float* weight, const float* bias, float* running_mean,
                            float* running_var, const float* residual, int B, int C, int H, int W, int act, int training,
                            float momentum, float eps, float* y, float* save_mean, float* save_invstd, cabinet_stream_t stream) {
    if (H <= 0 || W <= 0) return fail(CABINET_ERR_INVALID_ARG, "bn_act_fwd_part: non-positive dimension");
    if (int rc = check_bn_act(B, C, H * W, act, "bn_act_fwd_part")) return rc;
    if (!x || !weight || !bias || !running_mean || !running_var || !y || !save_mean || !save_invstd || (training && !conv_part))
        return fail(CABINET_ERR_INVALID_ARG, "bn_act_fwd_part: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("bn_act_fwd_part", x, residual, y);
    return hip_status(cabinet::bn_act_fwd_part_run(x, conv_part, H, W, weight, bias, running_mean, running_var, residual, B, C, act,
                                                   training, momentum, eps, y, save_mean, save_invstd,
                                                   static_cast<hipStream_t>(stream)),
                      "bn_act_fwd_part launch");
}

int cabinet_bn_act_bwd(const float* dy, const float* x, const float* weight, const float* bias, const float* save_mean,
                       const float* save_invstd, int B, int C, int P, int act, int training, float* dx, float* dweight,
                       float* dbias, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_bn_act(B, C, P, act, "bn_act_bwd")) return rc;
    if (!dy || !x || !weight || !bias || !save_mean || !save_invstd || !dx || !dweight || !dbias)
        return fail(CABINET_ERR_INVALID_ARG, "bn_act_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("bn_act_bwd", dy, x, dx);
    const size_t need = cabinet::bn_act_workspace(B, C, P);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "bn_act_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::bn_act_bwd_run(dy, x, weight, bias, save_mean, save_invstd, B, C, P, act, training, dx,
                                              dweight, dbias, workspace, static_cast<hipStream_t>(stream)),
                      "bn_act_bwd launch");
}

// ------------------------------------------------------ BatchNorm + ReLU + 1x1 classifier (K12)
int cabinet_bn_cls_supported(int C, int K, int P) { return cabinet::bn_cls_supported(C, K, P) ? 1 : 0; }
int cabinet_bn_cls_table_floats(int C, int K) { return (C > 0 && K > 0 && K <= 32) ? cabinet::bn_cls_table_floats(C, K) : 0; }

static int check_bn_cls(int B, int C, int K, int H, int W, const char* who) {
    if (B <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0) return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension", who);
    if (!cabinet::bn_cls_supported(C, K, H * W))
        return fail(CABINET_ERR_UNSUPPORTED, "%s: (C=%d, K=%d, H*W=%d) outside C %% 64 == 0, K <= 32, (H*W) %% 4 == 0", who, C, K, H * W);
    if ((long long)B * ((H * W + 63) / 64) > 2147483647LL || (long long)B * C * H * W >= (1LL << 40))
        return fail(CABINET_ERR_UNSUPPORTED, "%s: grid too large", who);
    return CABINET_OK;
}

size_t cabinet_bn_cls_fwd_workspace_bytes(int B, int C, int P) {
    return (B > 0 && C > 0 && P > 0) ? cabinet::bn_cls_fwd_workspace(B, C, P) : 0;
}

int cabinet_bn_cls_fwd(const float* z, const float* conv_part, const float* bn_weight, const float* bn_bias, float* running_mean,
                       float* running_var, const float* w_cls, const float* bias, int B, int C, int K, int H, int W, int training,
                       float momentum, float eps, float* y, float* table, void* workspace, size_t workspace_bytes,
                       cabinet_stream_t stream) {
    if (int rc = check_bn_cls(B, C, K, H, W, "bn_cls_fwd")) return rc;
    if (!z || !bn_weight || !bn_bias || !running_mean || !running_var || !w_cls || !y || !table)
        return fail(CABINET_ERR_INVALID_ARG, "bn_cls_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("bn_cls_fwd", z, y, table);
    const size_t need = cabinet::bn_cls_fwd_workspace(B, C, H * W);
    if (!workspace || workspace_bytes < need) return fail(CABINET_ERR_WORKSPACE, "bn_cls_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::bn_cls_fwd_run(z, conv_part, bn_weight, bn_bias, running_mean, running_var, w_cls, bias, B, C, K, H, W,
                                              training, momentum, eps, y, table, workspace, static_cast<hipStream_t>(stream)),
                      "bn_cls_fwd launch");
}

size_t cabinet_bn_cls_bwd_workspace_bytes(int B, int C, int K, int P) {
    return (B > 0 && C > 0 && K > 0 && K <= 32 && P > 0) ? cabinet::bn_cls_bwd_workspace(B, C, K, P) : 0;
}

int cabinet_bn_cls_bwd(const float* dy, const float* z, const float* table, int B, int C, int K, int H, int W, int training, float* dz,
                       float* dbn_weight, float* dbn_bias, float* dw_cls, float* dbias, void* workspace, size_t workspace_bytes,
                       cabinet_stream_t stream) {
    if (int rc = check_bn_cls(B, C, K, H, W, "bn_cls_bwd")) return rc;
    if (!dy || !z || !table || !dz || !dbn_weight || !dbn_bias || !dw_cls) return fail(CABINET_ERR_INVALID_ARG, "bn_cls_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("bn_cls_bwd", dy, z, table, dz);
    const size_t need = cabinet::bn_cls_bwd_workspace(B, C, K, H * W);
    if (!workspace || workspace_bytes < need) return fail(CABINET_ERR_WORKSPACE, "bn_cls_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::bn_cls_bwd_run(dy, z, table, B, C, K, H, W, training, dz, dbn_weight, dbn_bias, dw_cls, dbias, workspace,
                                              static_cast<hipStream_t>(stream)),
                      "bn_cls_bwd launch");
}

// ------------------------------------------------------ depthwise convolution
static int check_dwconv(int B, int C, int H, int W, int K, int S, const char* who) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension", who);
    if (!cabinet::dwconv_supported(K, S))
        return fail(CABINET_ERR_UNSUPPORTED, "%s: kernel %d stride %d (kernel 3|5, stride 1|2)", who, K, S);
    if ((long long)B * C * ((H + 15) / 16) * ((W + 7) / 8) > 2147483647LL)
        return fail(CABINET_ERR_UNSUPPORTED, "%s: grid too large", who);
    return CABINET_OK;
}

int cabinet_dwconv_supported(int K, int stride) { return cabinet::dwconv_supported(K, stride) ? 1 : 0; }

int cabinet_dwconv_fwd(const float* x, const float* weight, int B, int C, int H, int W, int K, int stride, float* y,
                       cabinet_stream_t stream) {
    if (int rc = check_dwconv(B, C, H, W, K, stride, "dwconv_fwd")) return rc;
    if (!x || !weight || !y) return fail(CABINET_ERR_INVALID_ARG, "dwconv_fwd: null tensor pointer");
    return hip_status(cabinet::dwconv_fwd_run(x, weight, B, C, H, W, K, stride, y, static_cast<hipStream_t>(stream)),
                      "dwconv_fwd launch");
}

size_t cabinet_dwconv_bwd_workspace_bytes(int B, int C, int H, int W, int K, int stride) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !cabinet::dwconv_supported(K, stride)) return 0;
    return cabinet::dwconv_bwd_workspace(B, C, H, W, K);
}

int cabinet_dwconv_bwd(const float* dy, const float* x, const float* weight, int B, int C, int H, int W, int K,
                       int stride, float* dx, float* dw, void* workspace, size_t workspace_bytes,
                       cabinet_stream_t stream) {
    if (int rc = check_dwconv(B, C, H, W, K, stride, "dwconv_bwd")) return rc;
    if (!dy || !x || !weight || !dx || !dw) return fail(CABINET_ERR_INVALID_ARG, "dwconv_bwd: null tensor pointer");
    const size_t need = cabinet::dwconv_bwd_workspace(B, C, H, W, K);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "dwconv_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::dwconv_bwd_run(dy, x, weight, B, C, H, W, K, stride, dx, dw, workspace,
                                              static_cast<hipStream_t>(stream)),
                      "dwconv_bwd launch");
}

// ------------------------------------------------------ channel gate + activation
int cabinet_gate_act_fwd(const float* x, const float* gate, int B, int C, int P, int act, float* y,
                         cabinet_stream_t stream) {
    if (int rc = check_bn_act(B, C, P, act, "gate_act_fwd")) return rc;
    if (!x || !gate || !y) return fail(CABINET_ERR_INVALID_ARG, "gate_act_fwd: null tensor pointer");
    return hip_status(cabinet::gate_act_fwd_run(x, gate, B * C, P, act, y, static_cast<hipStream_t>(stream)),
                      "gate_act_fwd launch");
}

size_t cabinet_gate_act_bwd_workspace_bytes(int B, int C, int P) {
    return B > 0 && C > 0 && P > 0 ? cabinet::gate_act_workspace(B * C, P) : 0;
}

int cabinet_gate_act_bwd(const float* dy, const float* x, const float* gate, int B, int C, int P, int act, float* dx,
                         float* dgate, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_bn_act(B, C, P, act, "gate_act_bwd")) return rc;
    if (!dy || !x || !gate || !dx || !dgate) return fail(CABINET_ERR_INVALID_ARG, "gate_act_bwd: null tensor pointer");
    const size_t need = cabinet::gate_act_workspace(B * C, P);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "gate_act_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::gate_act_bwd_run(dy, x, gate, B * C, P, act, dx, dgate, workspace,
                                                static_cast<hipStream_t>(stream)),
                      "gate_act_bwd launch");
}

// ------------------------------------------------------ squeeze-excite tail backward: act(SE(bn(z)))
size_t cabinet_se_act_bwd_workspace_bytes(int B, int C, int P) {
    return B > 0 && C > 0 && P > 0 ? cabinet::se_act_bwd_workspace(B, C, P) : 0;
}

int cabinet_se_act_bwd_reduce(const float* dy, const float* z, const float* mean, const float* invstd, const float* bn_weight,
                              const float* bn_bias, const float* gate, const float* a2, int B, int C, int P, int act, float* sums,
                              float* da2, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_bn_act(B, C, P, act, "se_act_bwd_reduce")) return rc;
    if (!dy || !z || !mean || !invstd || !bn_weight || !bn_bias || !gate || !a2 || !sums || !da2)
        return fail(CABINET_ERR_INVALID_ARG, "se_act_bwd_reduce: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("se_act_bwd_reduce", dy, z);
    const size_t need = cabinet::se_act_bwd_workspace(B, C, P);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "se_act_bwd_reduce: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::se_act_bwd_reduce_run(dy, z, mean, invstd, bn_weight, bn_bias, gate, a2, B, C, P, act, sums, da2,
                                                     workspace, static_cast<hipStream_t>(stream)),
                      "se_act_bwd_reduce launch");
}

int cabinet_se_act_bwd_coef(const float* sums, const float* gate, const float* ds, int B, int C, int P, int training,
                            float* dbn_weight, float* dbn_bias, float* coef, float* ds_over_p, cabinet_stream_t stream) {
    if (B <= 0 || C <= 0 || P <= 0) return fail(CABINET_ERR_INVALID_ARG, "se_act_bwd_coef: non-positive dimension");
    if (!sums || !gate || !ds || !dbn_weight || !dbn_bias || !coef || !ds_over_p)
        return fail(CABINET_ERR_INVALID_ARG, "se_act_bwd_coef: null tensor pointer");
    return hip_status(cabinet::se_act_bwd_coef_run(sums, gate, ds, B, C, P, training, dbn_weight, dbn_bias, coef, ds_over_p,
                                                   static_cast<hipStream_t>(stream)),
                      "se_act_bwd_coef launch");
}

int cabinet_se_act_bwd_mlp_supported(int C, int Cs) { return C > 0 && Cs > 0 && cabinet::se_act_bwd_mlp_supported(C, Cs) ? 1 : 0; }

size_t cabinet_se_act_bwd_mlp_workspace_bytes(int B, int C, int Cs) {
    return B > 0 && C > 0 && Cs > 0 ? cabinet::se_act_bwd_mlp_workspace(B, Cs) : 0;
}

int cabinet_se_act_bwd_mlp(const float* sums, const float* da2, const float* gate, const float* h1, const float* pooled,
                           const float* w1, const float* w2, int B, int C, int Cs, int P, int training, float* dw1, float* db1,
                           float* dw2, float* db2, float* ds, float* dbn_weight, float* dbn_bias, float* coef, float* ds_over_p,
                           void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (B <= 0 || C <= 0 || Cs <= 0 || P <= 0) return fail(CABINET_ERR_INVALID_ARG, "se_act_bwd_mlp: non-positive dimension");
    if (!sums || !da2 || !gate || !h1 || !pooled || !w1 || !w2 || !dw1 || !db1 || !dw2 || !db2 || !ds || !dbn_weight || !dbn_bias ||
        !coef || !ds_over_p)
        return fail(CABINET_ERR_INVALID_ARG, "se_act_bwd_mlp: null tensor pointer");
    if (!cabinet::se_act_bwd_mlp_supported(C, Cs))
        return fail(CABINET_ERR_UNSUPPORTED, "se_act_bwd_mlp: C=%d / Cs=%d beyond the staged operand (max 1024)", C, Cs);
    const size_t need = cabinet::se_act_bwd_mlp_workspace(B, Cs);
    if (workspace_bytes < need || !workspace)
        return fail(CABINET_ERR_WORKSPACE, "se_act_bwd_mlp: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::se_act_bwd_mlp_run(sums, da2, gate, h1, pooled, w1, w2, B, C, Cs, P, training, dw1, db1, dw2, db2, ds,
                                                  dbn_weight, dbn_bias, coef, ds_over_p, workspace, static_cast<hipStream_t>(stream)),
                      "se_act_bwd_mlp launch");
}

int cabinet_se_act_bwd_dx(const float* dy, const float* z, const float* mean, const float* invstd, const float* bn_weight,
                          const float* bn_bias, const float* gate, const float* ds_over_p, const float* coef, int B, int C, int P,
                          int act, float* dz, cabinet_stream_t stream) {
    if (int rc = check_bn_act(B, C, P, act, "se_act_bwd_dx")) return rc;
    if (!dy || !z || !mean || !invstd || !bn_weight || !bn_bias || !gate || !ds_over_p || !coef || !dz)
        return fail(CABINET_ERR_INVALID_ARG, "se_act_bwd_dx: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("se_act_bwd_dx", dy, z, dz);
    return hip_status(cabinet::se_act_bwd_dx_run(dy, z, mean, invstd, bn_weight, bn_bias, gate, ds_over_p, coef, B, C, P, act, dz,
                                                 static_cast<hipStream_t>(stream)),
                      "se_act_bwd_dx launch");
}

// ------------------------------------------------------ BatchNorm (+act) -> depthwise convolution
size_t cabinet_bn_dwconv_fwd_workspace_bytes(int B, int C, int H, int W) {
    return B > 0 && C > 0 && H > 0 && W > 0 ? cabinet::bn_dwconv_fwd_workspace(B, C, H, W) : 0;
}

int cabinet_bn_dwconv_fwd(const float* z, const float* bn_weight, const float* bn_bias, float* running_mean,
                          float* running_var, const float* conv_weight, int B, int C, int H, int W, int K, int stride,
                          int act, int training, float momentum, float eps, float* y, float* save_mean,
                          float* save_invstd, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_dwconv(B, C, H, W, K, stride, "bn_dwconv_fwd")) return rc;
    if (int rc = check_bn_act(B, C, H * W, act, "bn_dwconv_fwd")) return rc;
    if (!z || !bn_weight || !bn_bias || !running_mean || !running_var || !conv_weight || !y || !save_mean || !save_invstd)
        return fail(CABINET_ERR_INVALID_ARG, "bn_dwconv_fwd: null tensor pointer");
    const size_t need = cabinet::bn_dwconv_fwd_workspace(B, C, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "bn_dwconv_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::bn_dwconv_fwd_run(z, bn_weight, bn_bias, running_mean, running_var, conv_weight, B, C, H, W,
                                                 K, stride, act, training, momentum, eps, y, save_mean, save_invstd,
                                                 workspace, static_cast<hipStream_t>(stream)),
                      "bn_dwconv_fwd launch");
}

size_t cabinet_bn_dwconv_bwd_workspace_bytes(int B, int C, int H, int W, int K, int stride) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !cabinet::dwconv_supported(K, stride)) return 0;
    return cabinet::bn_dwconv_bwd_workspace(B, C, H, W, K);
}

int cabinet_bn_dwconv_bwd(const float* dy, const float* z, const float* bn_weight, const float* bn_bias,
                          const float* save_mean, const float* save_invstd, const float* conv_weight, int B, int C,
                          int H, int W, int K, int stride, int act, int training, float* dz, float* dbn_weight,
                          float* dbn_bias, float* dconv_weight, void* workspace, size_t workspace_bytes,
                          cabinet_stream_t stream) {
    if (int rc = check_dwconv(B, C, H, W, K, stride, "bn_dwconv_bwd")) return rc;
    if (int rc = check_bn_act(B, C, H * W, act, "bn_dwconv_bwd")) return rc;
    if (!dy || !z || !bn_weight || !bn_bias || !save_mean || !save_invstd || !conv_weight || !dz || !dbn_weight ||
        !dbn_bias || !dconv_weight)
        return fail(CABINET_ERR_INVALID_ARG, "bn_dwconv_bwd: null tensor pointer");
    const size_t need = cabinet::bn_dwconv_bwd_workspace(B, C, H, W, K);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "bn_dwconv_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::bn_dwconv_bwd_run(dy, z, bn_weight, bn_bias, save_mean, save_invstd, conv_weight, B, C, H,
                                                 W, K, stride, act, training, dz, dbn_weight, dbn_bias, dconv_weight,
                                                 workspace, static_cast<hipStream_t>(stream)),
                      "bn_dwconv_bwd launch");
}

// ------------------------------------------------------ 7x7 stride-2 stem convolution
static int check_stem(int B, int H, int W, const char* who) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension", who);
    if ((long long)B * ((H + 1) / 2) > 2147483647LL / 4) return fail(CABINET_ERR_UNSUPPORTED, "%s: grid too large", who);
    return CABINET_OK;
}

int cabinet_stem_conv_fwd(const float* x, const float* weight, int B, int H, int W, float* y, cabinet_stream_t stream) {
    if (int rc = check_stem(B, H, W, "stem_conv_fwd")) return rc;
    if (!x || !weight || !y) return fail(CABINET_ERR_INVALID_ARG, "stem_conv_fwd: null tensor pointer");
    return hip_status(cabinet::stem_conv_fwd_run(x, weight, B, H, W, y, static_cast<hipStream_t>(stream)),
                      "stem_conv_fwd launch");
}

// the weight-gradient kernel addresses one image's operands with 32-bit byte offsets: 64 Ho Wo floats (and 3 H W) below 4 GiB
static int check_stem_wrw(int B, int H, int W, const char* who) {
    if (int rc = check_stem(B, H, W, who)) return rc;
    if ((long long)((H + 1) / 2) * ((W + 1) / 2) > (1LL << 24)) return fail(CABINET_ERR_UNSUPPORTED, "%s: plane too large", who);
    return CABINET_OK;
}

size_t cabinet_stem_conv_wrw_workspace_bytes(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 ? cabinet::stem_conv_wrw_workspace(B, H, W) : 0;
}

int cabinet_stem_conv_wrw(const float* dy, const float* x, int B, int H, int W, float* dw, void* workspace,
                          size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_stem_wrw(B, H, W, "stem_conv_wrw")) return rc;
    if (!dy || !x || !dw) return fail(CABINET_ERR_INVALID_ARG, "stem_conv_wrw: null tensor pointer");
    const size_t need = cabinet::stem_conv_wrw_workspace(B, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "stem_conv_wrw: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::stem_conv_wrw_run(dy, x, B, H, W, dw, workspace, static_cast<hipStream_t>(stream)),
                      "stem_conv_wrw launch");
}

size_t cabinet_stem_conv_bn_bwd_workspace_bytes(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 ? cabinet::stem_conv_bn_bwd_workspace(B, H, W) : 0;
}

int cabinet_stem_conv_bn_bwd(const float* g, const float* z, const float* x, const float* bn_weight, const float* bn_bias,
                             const float* save_mean, const float* save_invstd, int B, int H, int W, int training, float* dw,
                             float* dbn_weight, float* dbn_bias, void* workspace, size_t workspace_bytes,
                             cabinet_stream_t stream) {
    if (int rc = check_stem_wrw(B, H, W, "stem_conv_bn_bwd")) return rc;
    if (!g || !z || !x || !bn_weight || !bn_bias || !save_mean || !save_invstd || !dw || !dbn_weight || !dbn_bias)
        return fail(CABINET_ERR_INVALID_ARG, "stem_conv_bn_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("stem_conv_bn_bwd", g, z);
    const size_t need = cabinet::stem_conv_bn_bwd_workspace(B, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "stem_conv_bn_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::stem_conv_bn_bwd_run(g, z, x, bn_weight, bn_bias, save_mean, save_invstd, B, H, W, training, dw,
                                                    dbn_weight, dbn_bias, workspace, static_cast<hipStream_t>(stream)),
                      "stem_conv_bn_bwd launch");
}

// ------------------------------------------------------ thin pointwise convolution
static int check_pwconv(int B, int Ci, int Co, int P, const char* who) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || P <= 0) return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension", who);
    if (!cabinet::pwconv_supported(Ci, Co, P))
        return fail(CABINET_ERR_UNSUPPORTED, "%s: Ci=%d, Co=%d, P=%d (multiples of 8, <= 128, block product <= 8, P <= 2^21, max(Ci, Co) * P <= 2^28)", who, Ci, Co, P);
    return CABINET_OK;
}

int cabinet_pwconv_supported(int Ci, int Co, int P) {
    return Ci > 0 && Co > 0 && P > 0 && cabinet::pwconv_supported(Ci, Co, P) ? 1 : 0;
}

int cabinet_pwconv_stream_plan(int B, int M, int K, int P, int x_align_bytes, int y_align_bytes, int out[4]) {
    if (int rc = check_pwconv(B, K, M, P, "pwconv_stream_plan")) return rc;
    if (!out || x_align_bytes < 0 || y_align_bytes < 0) return fail(CABINET_ERR_INVALID_ARG, "pwconv_stream_plan: null out / negative alignment");
    cabinet::pwconv_stream_plan_query(B, M, K, P, (unsigned)x_align_bytes, (unsigned)y_align_bytes, out);
    return CABINET_OK;
}

int cabinet_pwconv_fwd(const float* x, const float* w, int B, int Ci, int Co, int P, float* y, cabinet_stream_t stream) {
    if (int rc = check_pwconv(B, Ci, Co, P, "pwconv_fwd")) return rc;
    if (!x || !w || !y) return fail(CABINET_ERR_INVALID_ARG, "pwconv_fwd: null tensor pointer");
    return hip_status(cabinet::pwconv_fwd_run(x, w, B, Ci, Co, P, y, static_cast<hipStream_t>(stream)),
                      "pwconv_fwd launch");
}

size_t cabinet_pwconv_bwd_workspace_bytes(int B, int Ci, int Co, int P) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || P <= 0 || !cabinet::pwconv_supported(Ci, Co, P)) return 0;
    return cabinet::pwconv_bwd_workspace(B, Ci, Co, P);
}

int cabinet_pwconv_bwd(const float* dy, const float* x, const float* w, int B, int Ci, int Co, int P, float* dx,
                       float* dw, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_pwconv(B, Ci, Co, P, "pwconv_bwd")) return rc;
    if (!dy || !x || !w) return fail(CABINET_ERR_INVALID_ARG, "pwconv_bwd: null tensor pointer");
    const size_t need = cabinet::pwconv_bwd_workspace(B, Ci, Co, P);
    if (dw && (!workspace || workspace_bytes < need))
        return fail(CABINET_ERR_WORKSPACE, "pwconv_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::pwconv_bwd_run(dy, x, w, B, Ci, Co, P, dx, dw, workspace, static_cast<hipStream_t>(stream)),
                      "pwconv_bwd launch");
}

// ------------------------------------------------------ thin pointwise convolution + BatchNorm, backward in one walk
static int check_pw_bn(int B, int Ci, int Co, int P, int act, const char* who) {
    if (int rc = check_bn_act(B, Co, P, act, who)) return rc;
    if (Ci <= 0) return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension", who);
    if (!cabinet::pw_bn_bwd_supported(Ci, Co, P))
        return fail(CABINET_ERR_UNSUPPORTED, "%s: Ci=%d, Co=%d, P=%d (multiples of 8, <= 96, P <= 2^21)", who, Ci, Co, P);
    return CABINET_OK;
}

int cabinet_pw_bn_bwd_supported(int Ci, int Co, int P) {
    return Ci > 0 && Co > 0 && P > 0 && cabinet::pw_bn_bwd_supported(Ci, Co, P) ? 1 : 0;
}

int cabinet_pw_bn_bwd_plan(int B, int Ci, int Co, int P, int dx_align_bytes, int out[5]) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || P <= 0 || dx_align_bytes < 0 || !out)
        return fail(CABINET_ERR_INVALID_ARG, "pw_bn_bwd_plan: non-positive dimension, negative alignment or null out");
    if (!cabinet::pw_bn_bwd_supported(Ci, Co, P))
        return fail(CABINET_ERR_UNSUPPORTED, "pw_bn_bwd_plan: Ci=%d, Co=%d, P=%d (multiples of 8, <= 96, P <= 2^21)", Ci, Co, P);
    cabinet::pw_bn_bwd_plan_query(B, Ci, Co, P, (unsigned)dx_align_bytes, out);
    return CABINET_OK;
}

size_t cabinet_pw_bn_act_bwd_workspace_bytes(int B, int Ci, int Co, int P) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || P <= 0 || !cabinet::pw_bn_bwd_supported(Ci, Co, P)) return 0;
    return cabinet::pw_bn_act_bwd_workspace(B, Ci, Co, P);
}

int cabinet_pw_bn_act_bwd(const float* g, const float* z, const float* x, const float* pw_weight, const float* bn_weight,
                          const float* bn_bias, const float* save_mean, const float* save_invstd, int B, int Ci, int Co, int P,
                          int act, int training, float* dx, float* dpw_weight, float* dbn_weight, float* dbn_bias,
                          void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_pw_bn(B, Ci, Co, P, act, "pw_bn_act_bwd")) return rc;
    if (!g || !z || !pw_weight || !bn_weight || !bn_bias || !save_mean || !save_invstd || !dbn_weight || !dbn_bias ||
        (dpw_weight && !x))
        return fail(CABINET_ERR_INVALID_ARG, "pw_bn_act_bwd: null tensor pointer");
    if (P % 4 == 0) {  // the BatchNorm reduce reads g and z 16 bytes at a time there; x, dx and the weights may start anywhere
        CABINET_REQUIRE_ALIGNED("pw_bn_act_bwd", g, z);
    }
    const size_t need = cabinet::pw_bn_act_bwd_workspace(B, Ci, Co, P);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "pw_bn_act_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::pw_bn_act_bwd_run(g, z, x, pw_weight, bn_weight, bn_bias, save_mean, save_invstd, B, Ci, Co, P, act,
                                                 training, dx, dpw_weight, dbn_weight, dbn_bias, workspace,
                                                 static_cast<hipStream_t>(stream)),
                      "pw_bn_act_bwd launch");
}

size_t cabinet_pw_bn_dwconv_bwd_workspace_bytes(int B, int Ci, int C, int H, int W, int K, int stride) {
    if (B <= 0 || Ci <= 0 || C <= 0 || H <= 0 || W <= 0 || !cabinet::dwconv_supported(K, stride) ||
        !cabinet::pw_bn_bwd_supported(Ci, C, H * W))
        return 0;
    return cabinet::pw_bn_dwconv_bwd_workspace(B, Ci, C, H, W, K);
}

int cabinet_pw_bn_dwconv_bwd(const float* dy, const float* z, const float* x, const float* pw_weight, const float* bn_weight,
                             const float* bn_bias, const float* save_mean, const float* save_invstd, const float* conv_weight,
                             int B, int Ci, int C, int H, int W, int K, int stride, int act, int training, float* dx,
                             float* dpw_weight, float* dbn_weight, float* dbn_bias, float* dconv_weight, void* workspace,
                             size_t workspace_bytes, cabinet_stream_t stream) {
    if (int rc = check_dwconv(B, C, H, W, K, stride, "pw_bn_dwconv_bwd")) return rc;
    if (int rc = check_pw_bn(B, Ci, C, H * W, act, "pw_bn_dwconv_bwd")) return rc;
    if (!dy || !z || !pw_weight || !bn_weight || !bn_bias || !save_mean || !save_invstd || !conv_weight || !dbn_weight ||
        !dbn_bias || !dconv_weight || (dpw_weight && !x))
        return fail(CABINET_ERR_INVALID_ARG, "pw_bn_dwconv_bwd: null tensor pointer");
    const size_t need = cabinet::pw_bn_dwconv_bwd_workspace(B, Ci, C, H, W, K);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "pw_bn_dwconv_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::pw_bn_dwconv_bwd_run(dy, z, x, pw_weight, bn_weight, bn_bias, save_mean, save_invstd, conv_weight, B,
                                                    Ci, C, H, W, K, stride, act, training, dx, dpw_weight, dbn_weight, dbn_bias,
                                                    dconv_weight, workspace, static_cast<hipStream_t>(stream)),
                      "pw_bn_dwconv_bwd launch");
}

// ------------------------------------------------------ wide pointwise convolution: weight gradient
int cabinet_pwconv_wide_supported(int Ci, int Co, int P) {
    return Ci > 0 && Co > 0 && P > 0 && cabinet::pwconv_wide_supported(Ci, Co, P) ? 1 : 0;
}

int cabinet_pwconv_wide_plan(int B, int Ci, int Co, int P, int out[5]) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || P <= 0 || !out)
        return fail(CABINET_ERR_INVALID_ARG, "pwconv_wide_plan: non-positive dimension or null out");
    if (!cabinet::pwconv_wide_supported(Ci, Co, P))
        return fail(CABINET_ERR_UNSUPPORTED, "pwconv_wide_plan: Ci=%d, Co=%d, P=%d (multiples of 8, <= 4096, P <= 2^21, max(Ci, Co) * P <= 2^28)",
                    Ci, Co, P);
    cabinet::pwconv_wide_plan_query(B, Ci, Co, P, out);
    return CABINET_OK;
}

size_t cabinet_pwconv_wide_wgrad_workspace_bytes(int B, int Ci, int Co, int P) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || P <= 0 || !cabinet::pwconv_wide_supported(Ci, Co, P)) return 0;
    if ((long long)B * ((P + 63) / 64) > (1ll << 30)) return 0;
    return cabinet::pwconv_wide_wgrad_workspace(B, Ci, Co, P);
}

int cabinet_pwconv_wide_wgrad(const float* dy, const float* x, int B, int Ci, int Co, int P, float* dw, void* workspace,
                              size_t workspace_bytes, cabinet_stream_t stream) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || P <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "pwconv_wide_wgrad: non-positive dimension");
    if ((long long)B * ((P + 63) / 64) > (1ll << 30))
        return fail(CABINET_ERR_UNSUPPORTED, "pwconv_wide_wgrad: B=%d, P=%d: more than 2^30 pixel chunks", B, P);
    if (!cabinet::pwconv_wide_supported(Ci, Co, P))
        return fail(CABINET_ERR_UNSUPPORTED, "pwconv_wide_wgrad: Ci=%d, Co=%d, P=%d (multiples of 8, <= 4096, P <= 2^21, max(Ci, Co) * P <= 2^28)",
                    Ci, Co, P);
    if (!dy || !x || !dw) return fail(CABINET_ERR_INVALID_ARG, "pwconv_wide_wgrad: null tensor pointer");
    const size_t need = cabinet::pwconv_wide_wgrad_workspace(B, Ci, Co, P);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "pwconv_wide_wgrad: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::pwconv_wide_wgrad_run(dy, x, B, Ci, Co, P, dw, workspace, static_cast<hipStream_t>(stream)),
                      "pwconv_wide_wgrad launch");
}

// ------------------------------------------------------ 3x3 stride-2 convolution: weight and input gradient, 64 -> 64 forward
static bool conv3x3s2_size_ok(int B, int Ci, int H, int W) {  // the kernels index with 64 bits; the grid is one workgroup per slab
    return cabinet::conv3x3s2_wgrad_slabs(B, Ci, H, W) <= (1ll << 30);
}

int cabinet_conv3x3s2_supported(int Ci, int Co) { return cabinet::conv3x3s2_supported(Ci, Co) ? 1 : 0; }

size_t cabinet_conv3x3s2_wgrad_workspace_bytes(int B, int Ci, int Co, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || !cabinet::conv3x3s2_supported(Ci, Co) || !conv3x3s2_size_ok(B, Ci, H, W)) return 0;
    return cabinet::conv3x3s2_wgrad_workspace(B, Ci, H, W);
}

int cabinet_conv3x3s2_wgrad(const float* dy, const float* x, int B, int Ci, int Co, int H, int W, float* dw, void* workspace,
                            size_t workspace_bytes, cabinet_stream_t stream) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "conv3x3s2_wgrad: non-positive dimension");
    if (!cabinet::conv3x3s2_supported(Ci, Co))
        return fail(CABINET_ERR_UNSUPPORTED, "conv3x3s2_wgrad: Ci=%d, Co=%d ((64, 64) and (3, 16) are compiled)", Ci, Co);
    if (!conv3x3s2_size_ok(B, Ci, H, W))
        return fail(CABINET_ERR_UNSUPPORTED, "conv3x3s2_wgrad: B=%d, H=%d, W=%d: grid too large", B, H, W);
    if (!dy || !x || !dw) return fail(CABINET_ERR_INVALID_ARG, "conv3x3s2_wgrad: null tensor pointer");
    const size_t need = cabinet::conv3x3s2_wgrad_workspace(B, Ci, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "conv3x3s2_wgrad: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::conv3x3s2_wgrad_run(dy, x, B, Ci, H, W, dw, workspace, static_cast<hipStream_t>(stream)),
                      "conv3x3s2_wgrad launch");
}

int cabinet_conv3x3s2_dgrad(const float* dy, const float* w, int B, int Ci, int Co, int H, int W, float* dx,
                            cabinet_stream_t stream) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "conv3x3s2_dgrad: non-positive dimension");
    if (Ci != 64 || Co != 64)
        return fail(CABINET_ERR_UNSUPPORTED, "conv3x3s2_dgrad: Ci=%d, Co=%d ((64, 64) is compiled)", Ci, Co);
    if (cabinet::conv3x3s2_dgrad_workgroups(B, H, W) > (1ll << 30))
        return fail(CABINET_ERR_UNSUPPORTED, "conv3x3s2_dgrad: B=%d, H=%d, W=%d: grid too large", B, H, W);
    if (!dy || !w || !dx) return fail(CABINET_ERR_INVALID_ARG, "conv3x3s2_dgrad: null tensor pointer");
    if ((reinterpret_cast<size_t>(dx) & 7) != 0)
        return fail(CABINET_ERR_INVALID_ARG, "conv3x3s2_dgrad: dx must be 8-byte aligned");
    return hip_status(cabinet::conv3x3s2_dgrad_run(dy, w, B, H, W, dx, static_cast<hipStream_t>(stream)), "conv3x3s2_dgrad launch");
}

int cabinet_conv3x3s2_fwd_supported(int Ci, int Co) { return cabinet::conv3x3s2_fwd_supported(Ci, Co) ? 1 : 0; }

int cabinet_conv3x3s2_fwd(const float* x, const float* w, int B, int Ci, int Co, int H, int W, float* y, cabinet_stream_t stream) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "conv3x3s2_fwd: non-positive dimension");
    if (!cabinet::conv3x3s2_fwd_supported(Ci, Co))
        return fail(CABINET_ERR_UNSUPPORTED, "conv3x3s2_fwd: Ci=%d, Co=%d ((64, 64) is compiled)", Ci, Co);
    if (cabinet::conv3x3s2_fwd_workgroups(B, H, W) > (1ll << 30))
        return fail(CABINET_ERR_UNSUPPORTED, "conv3x3s2_fwd: B=%d, H=%d, W=%d: grid too large", B, H, W);
    if (!x || !w || !y) return fail(CABINET_ERR_INVALID_ARG, "conv3x3s2_fwd: null tensor pointer");
    return hip_status(cabinet::conv3x3s2_fwd_run(x, w, B, H, W, y, static_cast<hipStream_t>(stream)), "conv3x3s2_fwd launch");
}

// ------------------------------------------------------ dense 3x3 convolution (Winograd F(2x2,3x3), fp32 MFMA)
static int check_conv3x3(const cabinet::WinoShape& s, const char* who) {
    if (s.B <= 0 || s.C0 <= 0 || s.C1 < 0 || s.K <= 0 || s.H <= 0 || s.W <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension", who);
    if (!cabinet::conv3x3_shape_ok(s))
        return fail(CABINET_ERR_UNSUPPORTED,
                    "%s: C0=%d C1=%d Co=%d H=%d W=%d (C0, C1 multiples of 16; Co, C0+C1 multiples of 64; C0 %% 64 == 0 when C1 > 0; "
                    "one image's tensors < 1 GiB)", who, s.C0, s.C1, s.K, s.H, s.W);
    return CABINET_OK;
}

int cabinet_conv3x3_supported(int C0, int C1, int Co) { return cabinet::conv3x3_supported(C0, C1, Co) ? 1 : 0; }

int cabinet_conv3x3_tile_blocks(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 ? cabinet::conv3x3_tile_blocks(B, H, W) : 0;
}

size_t cabinet_conv3x3_fwd_workspace_bytes(int B, int C0, int C1, int Co, int H, int W) {
    const cabinet::WinoShape s{B, C0, C1, Co, H, W};
    return B > 0 && H > 0 && W > 0 && cabinet::conv3x3_shape_ok(s) ? cabinet::conv3x3_fwd_workspace(s) : 0;
}

int cabinet_conv3x3_fwd(const float* x0, const float* x1, const float* w, int B, int C0, int C1, int Co, int H, int W, float* y,
                        float* bn_part, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    const cabinet::WinoShape s{B, C0, C1, Co, H, W};
    if (int rc = check_conv3x3(s, "conv3x3_fwd")) return rc;
    if (!x0 || !w || !y || (C1 > 0 && !x1)) return fail(CABINET_ERR_INVALID_ARG, "conv3x3_fwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("conv3x3_fwd", x0, x1, w, y, bn_part);
    const size_t need = cabinet::conv3x3_fwd_workspace(s);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "conv3x3_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::conv3x3_fwd_run(s, x0, C1 > 0 ? x1 : nullptr, w, y, bn_part, workspace, static_cast<hipStream_t>(stream)),
                      "conv3x3_fwd launch");
}

size_t cabinet_conv3x3_bwd_workspace_bytes(int B, int C0, int C1, int Co, int H, int W) {
    const cabinet::WinoShape s{B, C0, C1, Co, H, W};
    return B > 0 && H > 0 && W > 0 && cabinet::conv3x3_shape_ok(s) ? cabinet::conv3x3_bwd_workspace(s) : 0;
}

int cabinet_conv3x3_bwd(const float* dy, const float* x0, const float* x1, const float* w, int B, int C0, int C1, int Co, int H,
                        int W, float* dx0, float* dx1, float* dw, void* workspace, size_t workspace_bytes, cabinet_stream_t stream) {
    const cabinet::WinoShape s{B, C0, C1, Co, H, W};
    if (int rc = check_conv3x3(s, "conv3x3_bwd")) return rc;
    if (!dy || !w || (dw && (!x0 || (C1 > 0 && !x1))) || (dx0 && C1 > 0 && !dx1))
        return fail(CABINET_ERR_INVALID_ARG, "conv3x3_bwd: null tensor pointer");
    CABINET_REQUIRE_ALIGNED("conv3x3_bwd", dy, x0, x1, w, dx0, dx1, dw);
    const size_t need = cabinet::conv3x3_bwd_workspace(s);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "conv3x3_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::conv3x3_bwd_run(s, dy, x0, C1 > 0 ? x1 : nullptr, w, dx0, C1 > 0 ? dx1 : nullptr, dw, workspace,
                                               static_cast<hipStream_t>(stream)),
                      "conv3x3_bwd launch");
}

// ------------------------------------------------------------------ evaluation tail (K13)
int cabinet_eval_chip_accum_supported(int C, int hl, int wl, int ch, int cw, int flip) {
    if (C < 1 || C > 32 || hl < 1 || wl < 1 || ch < 1 || cw < 1 || ch > 65535) return 0;
    return cabinet::eval_chip_threads(C, wl, cw, flip ? 2 : 1) > 0 ? 1 : 0;
}

int cabinet_eval_chip_accum(const float* a, const float* b, int N, int C, int hl, int wl, int ch, int cw, float* dst, int FH, int FW,
                            int y0, int x0, const float* rcp_y, const float* rcp_x, cabinet_stream_t stream) {
    if (N <= 0 || C <= 0 || hl <= 0 || wl <= 0 || ch <= 0 || cw <= 0 || FH <= 0 || FW <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "eval_chip_accum: non-positive dimension");
    if (!a || !dst) return fail(CABINET_ERR_INVALID_ARG, "eval_chip_accum: null tensor pointer");
    if (y0 < 0 || x0 < 0 || y0 > FH - ch || x0 > FW - cw)
        return fail(CABINET_ERR_INVALID_ARG, "eval_chip_accum: window (%d,%d)+(%d,%d) leaves the %dx%d destination", y0, x0, ch, cw, FH, FW);
    if (C > 32) return fail(CABINET_ERR_UNSUPPORTED, "eval_chip_accum: C=%d classes (max 32)", C);
    if (N > 65535 || ch > 65535) return fail(CABINET_ERR_UNSUPPORTED, "eval_chip_accum: N or chip height exceeds grid limits");
    if (!cabinet_eval_chip_accum_supported(C, hl, wl, ch, cw, b != nullptr))
        return fail(CABINET_ERR_UNSUPPORTED, "eval_chip_accum: C=%d x resize ratio %d/%d exceeds the LDS row buffers", C, wl, cw);
    return hip_status(cabinet::eval_chip_accum_run(a, b, N, C, hl, wl, ch, cw, dst, FH, FW, y0, x0, rcp_y, rcp_x,
                                                   static_cast<hipStream_t>(stream)),
                      "eval_chip_accum launch");
}

int cabinet_eval_scale_merge(const float* prob, int N, int C, int FH, int FW, int hst, int hed, int wst, int wed, float* total, int H,
                             int W, cabinet_stream_t stream) {
    if (N <= 0 || C <= 0 || FH <= 0 || FW <= 0 || H <= 0 || W <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "eval_scale_merge: non-positive dimension");
    if (!prob || !total) return fail(CABINET_ERR_INVALID_ARG, "eval_scale_merge: null tensor pointer");
    if (hst < 0 || wst < 0 || hed <= hst || wed <= wst || hed > FH || wed > FW)
        return fail(CABINET_ERR_INVALID_ARG, "eval_scale_merge: crop [%d:%d, %d:%d] leaves the %dx%d source", hst, hed, wst, wed, FH, FW);
    if ((long long)N * C > 65535 || H > 65535) return fail(CABINET_ERR_UNSUPPORTED, "eval_scale_merge: N*C or H exceeds grid limits");
    CABINET_REQUIRE_ALIGNED("eval_scale_merge", total);
    return hip_status(cabinet::eval_scale_merge_run(prob, N, C, FH, FW, hst, hed, wst, wed, total, H, W, static_cast<hipStream_t>(stream)),
                      "eval_scale_merge launch");
}

int cabinet_eval_argmax_hist(const float* total, const long long* labels, int N, int C, int H, int W, int ignore_lb, long long* hist,
                             unsigned char* pred, cabinet_stream_t stream) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(CABINET_ERR_INVALID_ARG, "eval_argmax_hist: non-positive dimension");
    if (!total || !labels || !hist) return fail(CABINET_ERR_INVALID_ARG, "eval_argmax_hist: null tensor pointer");
    if (C > 32) return fail(CABINET_ERR_UNSUPPORTED, "eval_argmax_hist: C=%d classes (max 32)", C);
    CABINET_REQUIRE_ALIGNED("eval_argmax_hist", total, labels);
    if (reinterpret_cast<uintptr_t>(pred) & 3) return fail(CABINET_ERR_INVALID_ARG, "eval_argmax_hist: pred must be 4-byte aligned");
    return hip_status(cabinet::eval_argmax_hist_run(total, labels, N, C, H, W, ignore_lb, hist, pred, static_cast<hipStream_t>(stream)),
                      "eval_argmax_hist launch");
}

// ------------------------------------------------------------------ inference tail (K17)
int cabinet_predict_up_argmax_supported(int C, int hl, int wl, int H, int W) {
    if (C < 1 || C > 32 || hl < 1 || wl < 1 || H < 1 || W < 1 || H > 65535) return 0;
    return cabinet::predict_up_threads(C, wl, W) > 0 ? 1 : 0;
}

int cabinet_predict_up_argmax(const float* logits_low, int N, int C, int hl, int wl, int H, int W, unsigned char* labels,
                              cabinet_stream_t stream) {
    if (N <= 0 || C <= 0 || hl <= 0 || wl <= 0 || H <= 0 || W <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "predict_up_argmax: non-positive dimension");
    if (!logits_low || !labels) return fail(CABINET_ERR_INVALID_ARG, "predict_up_argmax: null tensor pointer");
    if (reinterpret_cast<uintptr_t>(logits_low) & 3) return fail(CABINET_ERR_INVALID_ARG, "predict_up_argmax: logits must be 4-byte aligned");
    if (C > 32) return fail(CABINET_ERR_UNSUPPORTED, "predict_up_argmax: C=%d classes (max 32)", C);
    if (N > 65535 || H > 65535) return fail(CABINET_ERR_UNSUPPORTED, "predict_up_argmax: N or H exceeds grid limits");
    if (!cabinet_predict_up_argmax_supported(C, hl, wl, H, W))
        return fail(CABINET_ERR_UNSUPPORTED, "predict_up_argmax: C=%d x resize ratio %d/%d exceeds the LDS row buffer", C, wl, W);
    return hip_status(cabinet::predict_up_argmax_run(logits_low, N, C, hl, wl, H, W, labels, static_cast<hipStream_t>(stream)),
                      "predict_up_argmax launch");
}

int cabinet_predict_argmax(const float* total, int N, int C, int H, int W, unsigned char* labels, cabinet_stream_t stream) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(CABINET_ERR_INVALID_ARG, "predict_argmax: non-positive dimension");
    if (!total || !labels) return fail(CABINET_ERR_INVALID_ARG, "predict_argmax: null tensor pointer");
    if (C > 32) return fail(CABINET_ERR_UNSUPPORTED, "predict_argmax: C=%d classes (max 32)", C);
    if (N > 65535) return fail(CABINET_ERR_UNSUPPORTED, "predict_argmax: N exceeds grid limits");
    CABINET_REQUIRE_ALIGNED("predict_argmax", total);
    return hip_status(cabinet::predict_argmax_run(total, N, C, H, W, labels, static_cast<hipStream_t>(stream)), "predict_argmax launch");
}

int cabinet_predict_render(const unsigned char* labels, const float* image, const unsigned char* palette, int n_colors,
                           const float* mean, const float* std, float alpha, int N, int H, int W, unsigned char* pred_rgb,
                           unsigned char* input_rgb, unsigned char* overlay_rgb, cabinet_stream_t stream) {
    if (N <= 0 || H <= 0 || W <= 0) return fail(CABINET_ERR_INVALID_ARG, "predict_render: non-positive dimension");
    if (!labels || !palette || !pred_rgb) return fail(CABINET_ERR_INVALID_ARG, "predict_render: null labels, palette or pred_rgb");
    if (n_colors < 1 || n_colors > 256) return fail(CABINET_ERR_INVALID_ARG, "predict_render: n_colors=%d outside [1, 256]", n_colors);
    if ((input_rgb || overlay_rgb) && !(image && mean && std))
        return fail(CABINET_ERR_INVALID_ARG, "predict_render: input_rgb / overlay_rgb need the image with its mean and std");
    if (!(alpha >= 0.f && alpha <= 1.f)) return fail(CABINET_ERR_INVALID_ARG, "predict_render: alpha=%g outside [0, 1]", (double)alpha);
    if (reinterpret_cast<uintptr_t>(image) & 3) return fail(CABINET_ERR_INVALID_ARG, "predict_render: image must be 4-byte aligned");
    if ((size_t)N * H * W > ((size_t)1 << 33)) return fail(CABINET_ERR_UNSUPPORTED, "predict_render: more than 2^33 pixels");
    return hip_status(cabinet::predict_render_run(labels, image, palette, n_colors, mean, std, alpha, N, H, W, pred_rgb, input_rgb,
                                                  overlay_rgb, static_cast<hipStream_t>(stream)),
                      "predict_render launch");
}

// ------------------------------------------------------ optimizer tail (K16): clip + warm-up / poly SGD + EMA
size_t cabinet_sgd_tail_workspace_bytes(int n_chunks) { return n_chunks > 0 ? cabinet::sgd_tail_workspace(n_chunks) : 0; }

size_t cabinet_sgd_tail_state_bytes(int n_entries) { return n_entries > 0 ? cabinet::sgd_tail_state(n_entries) : 0; }

int cabinet_sgd_tail_step(const cabinet_sgd_tail_entry* entries, int n_entries, const cabinet_sgd_tail_chunk* chunks, int n_chunks,
                          const cabinet_sgd_tail_config* config, void* state, size_t state_bytes, int max_grid, void* workspace,
                          size_t workspace_bytes, cabinet_stream_t stream) {
    if (n_entries <= 0 || n_chunks <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "sgd_tail_step: non-positive count n_entries=%d n_chunks=%d", n_entries, n_chunks);
    if (!entries || !chunks) return fail(CABINET_ERR_INVALID_ARG, "sgd_tail_step: null table");
    if (!config || !state) return fail(CABINET_ERR_INVALID_ARG, "sgd_tail_step: null config or state block");
    if (max_grid < 0) return fail(CABINET_ERR_INVALID_ARG, "sgd_tail_step: negative max_grid=%d", max_grid);
    if (!(config->max_iter > (double)config->warmup_steps) || config->warmup_steps < 0 || !(config->ema_tau > 0.0))
        return fail(CABINET_ERR_INVALID_ARG, "sgd_tail_step: needs max_iter > warmup_steps >= 0 and ema_tau > 0");
    if ((reinterpret_cast<uintptr_t>(entries) | reinterpret_cast<uintptr_t>(chunks) | reinterpret_cast<uintptr_t>(state)) & 7)
        return fail(CABINET_ERR_INVALID_ARG, "sgd_tail_step: tables and state block must be 8-byte aligned");
    if (state_bytes < cabinet_sgd_tail_state_bytes(n_entries))
        return fail(CABINET_ERR_WORKSPACE, "sgd_tail_step: state block %zu < %zu bytes", state_bytes, cabinet_sgd_tail_state_bytes(n_entries));
    const size_t need = cabinet_sgd_tail_workspace_bytes(n_chunks);
    if (!workspace || workspace_bytes < need)
        return fail(CABINET_ERR_WORKSPACE, "sgd_tail_step: workspace %zu < %zu bytes", workspace_bytes, need);
    return hip_status(cabinet::sgd_tail_run(entries, n_entries, chunks, n_chunks, *config, state, workspace, max_grid,
                                            static_cast<hipStream_t>(stream)),
                      "sgd_tail_step launch");
}

// ------------------------------------------------------ gradient accumulation across graph replays (K21)
size_t cabinet_grad_accum_state_bytes(void) { return cabinet::grad_accum_state(); }

int cabinet_grad_accum(const cabinet_grad_accum_entry* entries, int n_entries, const cabinet_sgd_tail_chunk* chunks, int n_chunks,
                       void* state, size_t state_bytes, int max_grid, cabinet_stream_t stream) {
    if (n_entries <= 0 || n_chunks <= 0)
        return fail(CABINET_ERR_INVALID_ARG, "grad_accum: non-positive count n_entries=%d n_chunks=%d", n_entries, n_chunks);
    if (!entries || !chunks) return fail(CABINET_ERR_INVALID_ARG, "grad_accum: null table");
    if (!state) return fail(CABINET_ERR_INVALID_ARG, "grad_accum: null state block");
    if (max_grid < 0) return fail(CABINET_ERR_INVALID_ARG, "grad_accum: negative max_grid=%d", max_grid);
    if ((reinterpret_cast<uintptr_t>(entries) | reinterpret_cast<uintptr_t>(chunks) | reinterpret_cast<uintptr_t>(state)) & 7)
        return fail(CABINET_ERR_INVALID_ARG, "grad_accum: tables and state block must be 8-byte aligned");
    if (state_bytes < cabinet_grad_accum_state_bytes())
        return fail(CABINET_ERR_WORKSPACE, "grad_accum: state block %zu < %zu bytes", state_bytes, cabinet_grad_accum_state_bytes());
    return hip_status(cabinet::grad_accum_run(entries, n_entries, chunks, n_chunks, state, max_grid, static_cast<hipStream_t>(stream)),
                      "grad_accum launch");
}

int cabinet_grad_accum_reset(void* state, size_t state_bytes, cabinet_stream_t stream) {
    if (!state) return fail(CABINET_ERR_INVALID_ARG, "grad_accum_reset: null state block");
    if (reinterpret_cast<uintptr_t>(state) & 7) return fail(CABINET_ERR_INVALID_ARG, "grad_accum_reset: state block must be 8-byte aligned");
    if (state_bytes < cabinet_grad_accum_state_bytes())
        return fail(CABINET_ERR_WORKSPACE, "grad_accum_reset: state block %zu < %zu bytes", state_bytes, cabinet_grad_accum_state_bytes());
    return hip_status(cabinet::grad_accum_reset_run(state, static_cast<hipStream_t>(stream)), "grad_accum_reset launch");
}

// ------------------------------------------------------ training augmentation (K18): the reference's Cityscapes transform
int cabinet_augment_supported(int th, int tw, int max_taps, int max_pad_y, int max_pad_x, int min_h, int min_w) {
    if (th < 1 || tw < 1 || th > 32768 || tw > 32768) return fail(0, "augment: crop %d x %d outside [1, 32768]", th, tw);
    if (max_taps < 1 || max_taps > 5) return fail(0, "augment: %d taps per output pixel (1 to 5: resize ratio in/out <= 2.5)", max_taps);
    if (min_h < 1 || min_w < 1) return fail(0, "augment: empty resized image %d x %d", min_h, min_w);
    if (max_pad_y < 0 || max_pad_x < 0 || max_pad_y > min_h - 1 || max_pad_x > min_w - 1)
        return fail(0, "augment: reflect padding (%d, %d) exceeds the resized size (%d, %d) - 1", max_pad_y, max_pad_x, min_h, min_w);
    return 1;
}

size_t cabinet_augment_workspace_bytes(int N, int th, int tw) {
    return (N > 0 && th > 0 && tw > 0) ? cabinet::augment_workspace(N, th, tw) : 0;
}

int cabinet_augment_batch(const void* samples, int N, int th, int tw, const float* noise, unsigned long long seed, const float* mean,
                          const float* std, float* out_image, long long* out_label, unsigned char* out_u8, void* workspace,
                          size_t workspace_bytes, cabinet_stream_t stream) {
    if (N <= 0 || th <= 0 || tw <= 0) return fail(CABINET_ERR_INVALID_ARG, "augment_batch: non-positive dimension");
    if (!samples || !mean || !std || !out_image || !out_label)
        return fail(CABINET_ERR_INVALID_ARG, "augment_batch: null samples, mean, std, out_image or out_label");
    if (!cabinet_augment_supported(th, tw, 1, 0, 0, 1, 1)) return CABINET_ERR_UNSUPPORTED;  // the message is already set
    if (N > 65535) return fail(CABINET_ERR_UNSUPPORTED, "augment_batch: N=%d exceeds grid limits", N);
    if ((reinterpret_cast<uintptr_t>(samples) | reinterpret_cast<uintptr_t>(out_label)) & 7)
        return fail(CABINET_ERR_INVALID_ARG, "augment_batch: samples and out_label must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(out_image) | reinterpret_cast<uintptr_t>(noise)) & 3)
        return fail(CABINET_ERR_INVALID_ARG, "augment_batch: out_image and noise must be 4-byte aligned");
    const size_t need = cabinet_augment_workspace_bytes(N, th, tw);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return fail(CABINET_ERR_INVALID_ARG, "augment_batch: workspace of %zu bytes (16-byte aligned) needed, got %zu", need, workspace_bytes);
    return hip_status(cabinet::augment_run(samples, N, th, tw, noise, seed, mean, std, out_image, out_label, out_u8, workspace,
                                           static_cast<hipStream_t>(stream)),
                      "augment_batch launch");
}

// ------------------------------------------------------ aerial augmentation (K20): resize, flips + translate, rotate as uint8 passes
int cabinet_augment_warp_supported(int H, int W, int out_h, int out_w, double angle_deg, double resize_ratio) {
    if (H < 1 || W < 1 || out_h < 1 || out_w < 1 || H > 32768 || W > 32768 || out_h > 32768 || out_w > 32768)
        return fail(0, "augment_warp: source %d x %d or output %d x %d outside [1, 32768]", H, W, out_h, out_w);
    double a = fmod(angle_deg, 360.0);  // NaN stays NaN and fails the comparison below
    if (a > 180.0) a -= 360.0;
    if (a <= -180.0) a += 360.0;
    if (!(fabs(a) <= 45.0)) return fail(0, "augment_warp: RandomRotate by %g degrees (the rotation pass covers |angle| <= 45)", angle_deg);
    if (!(resize_ratio >= 0.0 && resize_ratio <= 2.5))
        return fail(0, "augment_warp: ResizeIfLarger ratio in/out %g (at most 2.5: five taps, 48 staged rows per tile)", resize_ratio);
    return 1;
}

static int warp_args(const char* who, const void* descs, int N, int max_out_h, int max_out_w) {
    if (!descs) return fail(CABINET_ERR_INVALID_ARG, "%s: null descs", who);
    if (N <= 0 || max_out_h <= 0 || max_out_w <= 0) return fail(CABINET_ERR_INVALID_ARG, "%s: non-positive dimension", who);
    if (reinterpret_cast<uintptr_t>(descs) & 7) return fail(CABINET_ERR_INVALID_ARG, "%s: descs must be 8-byte aligned", who);
    if (max_out_h > 32768 || max_out_w > 32768) return fail(CABINET_ERR_UNSUPPORTED, "%s: output %d x %d above 32768", who, max_out_h, max_out_w);
    if (N > 65535) return fail(CABINET_ERR_UNSUPPORTED, "%s: N=%d exceeds grid limits", who, N);
    return CABINET_OK;
}

int cabinet_augment_warp_batch(const void* descs, int N, int max_out_h, int max_out_w, cabinet_stream_t stream) {
    const int rc = warp_args("augment_warp_batch", descs, N, max_out_h, max_out_w);
    if (rc != CABINET_OK) return rc;
    return hip_status(cabinet::augment_warp_run(descs, N, max_out_h, max_out_w, static_cast<hipStream_t>(stream)), "augment_warp_batch launch");
}

int cabinet_augment_resize_batch(const void* descs, int N, int max_out_h, int max_out_w, cabinet_stream_t stream) {
    const int rc = warp_args("augment_resize_batch", descs, N, max_out_h, max_out_w);
    if (rc != CABINET_OK) return rc;
    return hip_status(cabinet::augment_resize_run(descs, N, max_out_h, max_out_w, static_cast<hipStream_t>(stream)), "augment_resize_batch launch");
}

}  // extern "C"
