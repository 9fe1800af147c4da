// K9 -- the 7x7 stride-2 stem convolution of the spatial branch (3 -> 64 channels, no bias), forward and weight
// gradient, NCHW fp32.
//
// Replaces the nn.Conv2d of `ConvBNReLU(3, 64, kernel_size=7, stride=2, padding=3)`, reference
// src/models/cabinet.py:111 (SpatialBranch.conv1; ConvBNReLU is SURVEY.md section 8 row a6's operator).  Its input is
// the image, so no input gradient exists.  MIOpen serves it with NHWC implicit-GEMM kernels plus layout transposes
// of the image, of the 537 MB output and of its gradient: ~3.2 ms of the config-3 step.
//
// As a GEMM: M = 64 output channels, N = pixels, K = 3*7*7 = 147 (padded to 148).  With only 3 input channels the
// im2col matrix is never worth building: a workgroup stages the input patch of its output tile in LDS (17 KB) and
// every lane gathers its B operand from it with a precomputed (ci,ky,kx) offset -- the "pixel on the lane" layout of
// v_mfma_f32_32x32x2_f32, so outputs leave as 128-byte rows of the NCHW tensor.  Weights live in LDS for the whole
// workgroup, which walks a strip of tiles (persistent over 16 tiles: one staging of the 38 KB weight image).
//   fwd : y[co][px]  = sum_k W[co][k] * patch[k][px]            A = W (LDS, stride 149), B = patch gather
//   wrw : dW[co][k]  = sum_px dy[co][px] * patch[k][px]         A = dy tile (LDS, stride 129), B = patch gather,
//         contraction over pixels; each wave accumulates the full 64 x 160 tile over its pixels, one ordered slab per
//         workgroup, final ordered slab sum (slab_sum.hpp; no atomics).
//
// The forward is software-pipelined over the tiles of its strip like the weight gradient below: the patch of tile t+1 is requested
// (unconditional row-segment loads, clamped, 0 selected on the way into LDS: 16 rows per wave + 2 elements of columns 64..68 per
// thread) before tile t's 296 MFMAs and written behind them.  135 VGPRs: store addresses and patch offsets are formed where they
// are used, not hoisted over the tile loop (the staging this replaces -- 17 loads per thread and tile, each behind a division and
// a bounds test -- ran at 0.50 of the fp32 MFMA rate with 0.34-0.40 of the wave cycles parked; this one at 0.72 with 0.12-0.14).
//
// The weight gradient is one software-pipelined kernel with two operand forms.  Plain: A is dy.  BN (cabinet_stem_conv_bn_bwd, the
// backward of relu(bn(conv(image)))): A is the BatchNorm + ReLU input gradient, formed per element from (g, z) and the six
// per-channel scalars on the way into LDS with the expressions of bn_act_bwd_dx_kernel -- the same bits, so dW is the bits of
// the pair bn_act_bwd + stem_conv_wrw, and the 537 MB dz of the config-3 step (one writer, one reader) is never written.
// Staging: every load is unconditional (addresses clamped into the tensor, what lies outside replaced by 0 on the way into LDS
// -- in the BN form the 0 is staged, not the dz of clamped operands), patch rows load as row segments at wave-uniform scalar
// offsets with lane = column, and the operands of tile t+1 are requested before tile t is multiplied.  The staging this replaces
// had each of its ~19 loads per thread and tile behind a bounds branch, hence one exposed memory latency each: the kernel
// waited (SQ_WAIT_ANY 0.49 of wave cycles) at 0.42 of the fp32 MFMA rate.
// Register budget at 2 workgroups per CU (256 VGPRs per wave, accumulators included): 160 accumulators; prefetch of the plain
// form 32 (dy) + 11 (patch) = 240 VGPRs in all; the BN form prefetches half of the tile's channel groups (16 g + 16 z + 11) and
// requests the other half, in two batches, once the first is in LDS: 255 VGPRs.  No scratch in any instantiation (the full
// 64-register prefetch of the BN form spills; one workgroup per CU would hold it but leaves the MFMA pipe to a single wave).
#include "act.hpp"
#include "common.hpp"
#include "slab_sum.hpp"

namespace cabinet {

constexpr int ST_K = 7, ST_S = 2, ST_PAD = 3, ST_CI = 3, ST_CO = 64;
constexpr int ST_KK = ST_CI * ST_K * ST_K;  // 147
constexpr int ST_KP = 148;                  // padded to a multiple of the MFMA k-step (2)
constexpr int ST_WLD = 149;                 // LDS row stride of the weight image (odd: conflict-free column reads)

// patch offset of contraction index k = (ci, ky, kx) in a [3][IH][IW] LDS patch (k >= 147: the zero-weight pad)
__host__ __device__ constexpr int stem_koff(int k, int IH, int IW) {
    return k < ST_KK ? ((k / (ST_K * ST_K)) * IH + (k % (ST_K * ST_K)) / ST_K) * IW + (k % ST_K) : 0;
}

struct StemShape {
    int B, H, W, Ho, Wo;
};

// load at a wave-uniform base + a 32-bit per-lane byte offset (one address register per lane, whatever the number of bases)
template <typename T>
__device__ __forceinline__ T sw_ld(const float* base, unsigned byte_off) {
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}

// ------------------------------------------------------------------------------------------------ forward
constexpr int SF_TH = 8, SF_TW = 32;                         // output tile of a workgroup step
constexpr int SF_IH = (SF_TH - 1) * ST_S + ST_K;             // 21
constexpr int SF_IW = (SF_TW - 1) * ST_S + ST_K;             // 69
constexpr int SF_PATCH = ST_CI * SF_IH * SF_IW;              // 4347 floats
constexpr int SF_ROWS = ST_CI * SF_IH;                       // 63 patch rows of 69 columns: lane = column, 64..68 apart
constexpr int SF_PR = (SF_ROWS + 3) / 4;                     // 16 patch rows per wave
constexpr int SF_XW = SF_IW - 64;                            // the 5-column tail of a row
constexpr int SF_EXTRA = SF_ROWS * SF_XW;                    // 315 tail elements: two per thread
constexpr int SF_XT = (SF_EXTRA + 255) / 256;                // 2
constexpr int SF_KG = 2, SF_NG = ST_KP / (2 * SF_KG);        // 37 groups of two k-steps (8 MFMAs) in the operand pipeline
static_assert(SF_NG * 2 * SF_KG == ST_KP, "k-groups tile the contraction");

// Software pipeline over the tiles of a strip: the patch of tile t+1 is requested (unconditional loads: addresses clamped into
// the image, what lies outside replaced by 0 on the way into LDS) before tile t is multiplied, and written into the one patch
// buffer behind the MFMAs and a barrier.
__global__ __launch_bounds__(256, 2) void stem_conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wgt,
                                                                StemShape s, int tiles_x, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wl = smem;                          // [64][149]
    float* xs = wl + ST_CO * ST_WLD;           // [3][21][69]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;
    const int strips_y = (s.Ho + SF_TH - 1) / SF_TH;
    const int b = blockIdx.x / strips_y, oy0 = (blockIdx.x - b * strips_y) * SF_TH;
    const float* xb = x + (size_t)b * ST_CI * s.H * s.W;
    const int iy0 = oy0 * ST_S - ST_PAD;
    // patch: row SF_PR * wave + jj of the 63 (wave-uniform image row ci * H + iy, -1 above / below the image), column = lane ...
    int prow[SF_PR];
#pragma unroll
    for (int jj = 0; jj < SF_PR; ++jj) {
        const int rr = min(SF_PR * wave + jj, SF_ROWS - 1), ci = rr / SF_IH, iy = iy0 + rr - ci * SF_IH;
        prow[jj] = __builtin_amdgcn_readfirstlane((iy >= 0 && iy < s.H) ? ci * s.H + iy : -1);  // a scalar register each
    }
    // ... and elements tid, tid + 256 of the 315 in columns 64..68
    int xlds[SF_XT], xcol[SF_XT], xrow[SF_XT];  // index in the patch, patch column, image row (-1 outside)
#pragma unroll
    for (int e = 0; e < SF_XT; ++e) {
        const int i = min(tid + 256 * e, SF_EXTRA - 1), er = i / SF_XW, ci = er / SF_IH, iy = iy0 + er - ci * SF_IH;
        xcol[e] = 64 + i - er * SF_XW;
        xlds[e] = er * SF_IW + xcol[e];
        xrow[e] = (iy >= 0 && iy < s.H) ? ci * s.H + iy : -1;
    }
    float pp[SF_PR + SF_XT];
    auto request = [&](int t) {
        const int ix0 = t * SF_TW * ST_S - ST_PAD;
        const unsigned ixc = min(max(ix0 + lane, 0), s.W - 1) * 4u;
#pragma unroll
        for (int jj = 0; jj < SF_PR; ++jj) pp[jj] = sw_ld<float>(xb + (size_t)max(prow[jj], 0) * s.W, ixc);
#pragma unroll
        for (int e = 0; e < SF_XT; ++e)
            pp[SF_PR + e] = xb[(size_t)max(xrow[e], 0) * s.W + min(max(ix0 + xcol[e], 0), s.W - 1)];
    };
    auto commit = [&](int t) {
        const int ix0 = t * SF_TW * ST_S - ST_PAD;
        const bool okx = ix0 + lane >= 0 && ix0 + lane < s.W;
#pragma unroll
        for (int jj = 0; jj < SF_PR; ++jj)  // wave 3's sixteenth row is its fifteenth again: the same value to the same place
            xs[min(SF_PR * wave + jj, SF_ROWS - 1) * SF_IW + lane] = (prow[jj] >= 0 && okx) ? pp[jj] : 0.f;
#pragma unroll
        for (int e = 0; e < SF_XT; ++e)
            if (tid + 256 * e < SF_EXTRA)
                xs[xlds[e]] = (xrow[e] >= 0 && ix0 + xcol[e] >= 0 && ix0 + xcol[e] < s.W) ? pp[SF_PR + e] : 0.f;
    };

    request(0);
    for (int i = tid; i < ST_CO * ST_KP; i += 256) {
        const int co = i / ST_KP, k = i - co * ST_KP;
        wl[co * ST_WLD + k] = k < ST_KK ? wgt[co * ST_KK + k] : 0.f;
    }
    commit(0);
    __syncthreads();
    // the two output rows of this wave, pixel li of each: patch offsets of their top-left taps
    const int poff0 = (ST_S * (2 * wave)) * SF_IW + ST_S * li;  // the second row's are ST_S * SF_IW further
    const size_t ylane = (((size_t)b * ST_CO + 4 * h) * s.Ho + oy0 + 2 * wave) * s.Wo + li;  // channel 4 h, row 2 wave, pixel li
    for (int t = 0; t < tiles_x; ++t) {
        const int ox0 = t * SF_TW;
        if (t + 1 < tiles_x) request(t + 1);  // in flight underneath this tile's MFMAs
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        const float* wrow = wl + li * ST_WLD + h;
        const float* xp0 = xs + poff0;
        // Fully unrolled: the (ci,ky,kx) patch offsets of both lane halves are compile-time constants.  The operands of k-group
        // g + 1 are read while group g is multiplied, and no further ahead (the scheduling barrier): with the next patch in
        // flight the registers hold two groups' operands, not the tens the scheduler would hoist.
        float av[2][SF_KG][2], bv[2][SF_KG][2];
        auto read_group = [&](int g, float(*a)[2], float(*bq)[2]) {
#pragma unroll
            for (int i = 0; i < SF_KG; ++i) {
                const int k0 = 2 * (SF_KG * g + i);
                // offset of the upper lane half = that of the lower + d, and d takes four values over the 74 steps: a base per
                // value and an immediate, not 74 per-lane offsets carried through the tile loop
                const int kl = stem_koff(k0, SF_IH, SF_IW), d = stem_koff(k0 + 1, SF_IH, SF_IW) - kl;
                const float* q = xp0 + (h ? d : 0);
                a[i][0] = wrow[k0], a[i][1] = wrow[32 * ST_WLD + k0];
                bq[i][0] = q[kl], bq[i][1] = q[kl + ST_S * SF_IW];
            }
        };
        read_group(0, av[0], bv[0]);
#pragma unroll
        for (int g = 0; g < SF_NG; ++g) {
            if (g + 1 < SF_NG) read_group(g + 1, av[(g + 1) & 1], bv[(g + 1) & 1]);
#pragma unroll
            for (int i = 0; i < SF_KG; ++i) {  // k-order 0..147
                const float a0 = av[g & 1][i][0], a1 = av[g & 1][i][1], b0 = bv[g & 1][i][0], b1 = bv[g & 1][i][1];
                acc[0][0] = mfma32(a0, b0, acc[0][0]);
                acc[0][1] = mfma32(a0, b1, acc[0][1]);
                acc[1][0] = mfma32(a1, b0, acc[1][0]);
                acc[1][1] = mfma32(a1, b1, acc[1][1]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (t + 1 < tiles_x) {
            __syncthreads();  // this tile's readers are done with the patch
            commit(t + 1);
        }
        const int ox = ox0 + li;
        // the 64 store addresses are formed here from one per-lane offset, not carried (128 registers) through the tile loop
        size_t yo = ylane + ox0;
        asm volatile("" : "+v"(yo));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int oy = oy0 + 2 * wave + j;
            if (oy < s.Ho && ox < s.Wo) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        y[yo + ((size_t)(32 * i + acc_row(r)) * s.Ho + j) * s.Wo] = acc[i][j][r];
            }
        }
        __syncthreads();  // tile t+1 is in LDS
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int SW_TH = 4, SW_TW = 32;                         // 128 pixels per step, 32 per wave
constexpr int SW_IH = (SW_TH - 1) * ST_S + ST_K;             // 13
constexpr int SW_IW = (SW_TW - 1) * ST_S + ST_K;             // 69
constexpr int SW_PATCH = ST_CI * SW_IH * SW_IW;              // 2691 floats
constexpr int SW_DLD = SW_TH * SW_TW + 1;                    // 129: row stride of the dy tile
constexpr int SW_KB = 5;                                     // 5 x 32 = 160 >= 147 columns
constexpr int SW_G = ST_CO * SW_TH * (SW_TW / 4) / 256;      // 8: 4-pixel groups of the dy tile per thread (channels gco + 8 j)
constexpr int SW_ROWS = ST_CI * SW_IH;                       // 39 patch rows of 69 columns: lane = column, 64..68 apart
constexpr int SW_PR = (SW_ROWS + 3) / 4;                     // 10 patch rows per wave
constexpr int SW_EXTRA = SW_ROWS * (SW_IW - 64);             // 195 elements in columns 64..68: one per thread
constexpr int SW_BNP = 8;                                    // per-channel scalars of the BN form in LDS (7 used)

// BN form of the "dy" operand: the BatchNorm + ReLU that follows the convolution, differentiated while the tile is staged
//   dy = (gam * inv) * (du - m1 - xh * m2),  xh = (z - mu) * inv,  du = g * relu'(fmaf(xh, gam, bet))
// (the expressions of bn_act_bwd_dx_kernel, bn_act.hip; coef = [m1 | m2] from bn_act_bwd_finalize_kernel)
struct StemBn {
    const float *z, *mean, *invstd, *weight, *bias, *coef;
};

// One kernel, two operand forms: BN = false reads dy; BN = true reads (g, z) and forms dy per element on the way into LDS, so
// the 537 MB dz of sb.conv1's BatchNorm is never written.  VEC (Wo % 4 == 0, 16-byte aligned operands): 128-bit row loads.
// Software pipeline: the operands of tile t+1 (PJ of the SW_G channel groups of g [and z], the image patch) are requested
// before tile t is multiplied and written to LDS behind it; groups PJ..SW_G-1 are requested, in two batches, when the first
// ones have been written (each batch waits one memory latency, which the other workgroup of the CU covers with its MFMAs).  No
// load sits behind a branch: addresses are clamped into the tensor and what lies outside is replaced by 0 on the way into LDS.
template <bool BN, bool VEC, int PJ>
__global__ __launch_bounds__(256, 2) void stem_conv_wrw_kernel(const float* __restrict__ dy, const float* __restrict__ x, StemBn bn,
                                                                StemShape s, int tiles_x, float* __restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* dys = smem;                          // [64][129]
    float* xs = dys + ST_CO * SW_DLD;           // [3][13][69]
    float* bnp = xs + SW_PATCH;                 // [64][SW_BNP] (BN only)
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;
    const int strips_y = (s.Ho + SW_TH - 1) / SW_TH;
    const int b = blockIdx.x / strips_y, oy0 = (blockIdx.x - b * strips_y) * SW_TH;
    int ko[SW_KB];  // patch offset of this lane's column k = 32*kb + li (columns >= 147 read offset 0 and are dropped)
#pragma unroll
    for (int kb = 0; kb < SW_KB; ++kb) {
        const int k = 32 * kb + li, kk = k < ST_KK ? k : 0;
        const int ci = kk / (ST_K * ST_K), r = kk - ci * ST_K * ST_K, ky = r / ST_K, kx = r - ky * ST_K;
        ko[kb] = (ci * SW_IH + ky) * SW_IW + kx;
    }
    f32x16 acc[2][SW_KB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < SW_KB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const float* xb = x + (size_t)b * ST_CI * s.H * s.W;
    const float* dyb = dy + (size_t)b * ST_CO * s.Ho * s.Wo;
    const float* zb = BN ? bn.z + (size_t)b * ST_CO * s.Ho * s.Wo : nullptr;
    const int iy0 = oy0 * ST_S - ST_PAD;
    if (BN && tid < ST_CO) {  // visible after the first barrier of the tile loop
        const float mu = bn.mean[tid], inv = bn.invstd[tid], gam = bn.weight[tid];
        float* q = bnp + tid * SW_BNP;
        q[0] = mu, q[1] = inv, q[2] = gam, q[3] = bn.bias[tid], q[4] = bn.coef[tid], q[5] = bn.coef[ST_CO + tid], q[6] = gam * inv;
    }
    // dy tile: this thread's 4 pixels (row gr, columns gc..gc+3) of channels gco + 8 j
    const int gco = tid >> 5, gr = (tid >> 3) & 3, gc = (tid & 7) * 4;
    const bool grow_ok = oy0 + gr < s.Ho;
    const size_t gcs = (size_t)8 * s.Ho * s.Wo;
    const unsigned grow = ((unsigned)gco * s.Ho + min(oy0 + gr, s.Ho - 1)) * s.Wo;  // byte offsets fit 32 bits: the host's check
    float* gdst = dys + gco * SW_DLD + gr * SW_TW + gc;
    // patch: row SW_PR * wave + jj of the 39 (wave-uniform image offset, -1 above / below the image), column = lane ...
    int prow[SW_PR];
#pragma unroll
    for (int jj = 0; jj < SW_PR; ++jj) {
        const int rr = min(SW_PR * wave + jj, SW_ROWS - 1), ci = rr / SW_IH, iy = iy0 + rr - ci * SW_IH;
        prow[jj] = __builtin_amdgcn_readfirstlane((iy >= 0 && iy < s.H) ? (ci * s.H + iy) * s.W : -1);  // a scalar register each
    }
    // ... and element `tid` of the 195 in columns 64..68.  Its indices are derived again from the thread id where they are used:
    // carried through the tile loop they cost three registers of a budget that has none to spare.
    struct Extra {
        int lds, col, row;  // index in xs, patch column, image offset of the row (-1 outside)
    };
    auto extra = [&]() {
        int te = tid;
        asm volatile("" : "+v"(te));
        const int i = min(te, SW_EXTRA - 1), er = i / (SW_IW - 64), ec = 64 + i - er * (SW_IW - 64);
        const int eci = er / SW_IH, eiy = iy0 + er - eci * SW_IH;
        return Extra{er * SW_IW + ec, ec, (eiy >= 0 && eiy < s.H) ? (eci * s.H + eiy) * s.W : -1};
    };

    f32x4 pg[SW_G], pz[SW_G];
    float pp[SW_PR + 1];
    auto request_dy = [&](int t, int j0, int j1) {
        const int ox = t * SW_TW + gc;
        if (VEC) {
            const unsigned o = (grow + min(ox, s.Wo - 4)) * 4u;  // per lane; the channel group's base is wave-uniform
#pragma unroll
            for (int j = j0; j < j1; ++j) {
                pg[j] = sw_ld<f32x4>(dyb + j * gcs, o);
                if (BN) pz[j] = sw_ld<f32x4>(zb + j * gcs, o);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned o = (grow + min(ox + e, s.Wo - 1)) * 4u;
#pragma unroll
                for (int j = j0; j < j1; ++j) {
                    pg[j][e] = sw_ld<float>(dyb + j * gcs, o);
                    if (BN) pz[j][e] = sw_ld<float>(zb + j * gcs, o);
                }
            }
        }
    };
    auto commit_dy = [&](int t, int j0, int j1) {
        const int ox = t * SW_TW + gc;
#pragma unroll
        for (int j = j0; j < j1; ++j) {
            f32x4 v = pg[j];
            if (BN) {
                const float* q = bnp + (gco + 8 * j) * SW_BNP;
                const float mu = q[0], inv = q[1], gam = q[2], bet = q[3], m1 = q[4], m2 = q[5], gi = q[6];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (pz[j][e] - mu) * inv;
                    const float du = v[e] * act_grad(fmaf(xh, gam, bet), ACT_RELU);
                    v[e] = gi * (du - m1 - xh * m2);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)  // past Ho / Wo: 0, not the dz of a clamped load
                gdst[j * 8 * SW_DLD + e] = (grow_ok && ox + e < s.Wo) ? v[e] : 0.f;
            if (BN) __builtin_amdgcn_sched_barrier(0);  // one channel's 7 scalars in registers at a time, not all SW_G x 7
        }
    };
    auto request_patch = [&](int t) {
        const int ix0 = t * SW_TW * ST_S - ST_PAD;
        const unsigned ixc = min(max(ix0 + lane, 0), s.W - 1) * 4u;
#pragma unroll
        for (int jj = 0; jj < SW_PR; ++jj) pp[jj] = sw_ld<float>(xb + max(prow[jj], 0), ixc);
        const Extra x5 = extra();
        pp[SW_PR] = sw_ld<float>(xb, (max(x5.row, 0) + min(max(ix0 + x5.col, 0), s.W - 1)) * 4u);
    };
    auto commit_patch = [&](int t) {
        const int ix0 = t * SW_TW * ST_S - ST_PAD;
        const bool okx = ix0 + lane >= 0 && ix0 + lane < s.W;
#pragma unroll
        for (int jj = 0; jj < SW_PR; ++jj)  // wave 3's tenth row is its ninth again: the same value to the same place
            xs[min(SW_PR * wave + jj, SW_ROWS - 1) * SW_IW + lane] = (prow[jj] >= 0 && okx) ? pp[jj] : 0.f;
        const Extra x5 = extra();
        if (tid < SW_EXTRA) xs[x5.lds] = (x5.row >= 0 && ix0 + x5.col >= 0 && ix0 + x5.col < s.W) ? pp[SW_PR] : 0.f;
    };

    request_dy(0, 0, PJ);
    request_patch(0);
    for (int t = 0; t < tiles_x; ++t) {
        __syncthreads();  // the previous tile's readers are done with dys / xs
        commit_patch(t);
        commit_dy(t, 0, PJ);
        if (PJ < SW_G) {
            __builtin_amdgcn_sched_barrier(0);  // the late groups' registers are the prefetched groups' registers: not both at once
            request_dy(t, PJ, PJ + 2);
            commit_dy(t, PJ, PJ + 2);
            __builtin_amdgcn_sched_barrier(0);
            request_dy(t, PJ + 2, SW_G);
            commit_dy(t, PJ + 2, SW_G);
        }
        __syncthreads();
        if (t + 1 < tiles_x) {  // in flight underneath this tile's MFMAs
            request_dy(t + 1, 0, PJ);
            request_patch(t + 1);
        }
        // this wave contracts over pixels p = 32*wave .. +31 (output row `wave` of the tile), two per MFMA
        const float* drow = dys + li * SW_DLD + 32 * wave + h;
        const int prow0 = (ST_S * wave) * SW_IW;
#pragma unroll 2
        for (int c0 = 0; c0 < 32; c0 += 2) {
            const float a0 = drow[c0], a1 = drow[32 * SW_DLD + c0];
            const int poff = prow0 + ST_S * (c0 + h);
#pragma unroll
            for (int kb = 0; kb < SW_KB; ++kb) {
                const float bv = xs[ko[kb] + poff];
                acc[0][kb] = mfma32(a0, bv, acc[0][kb]);
                acc[1][kb] = mfma32(a1, bv, acc[1][kb]);
            }
        }
    }
    // ordered cross-wave sum through LDS, then this workgroup's slab [64][147]
    __syncthreads();
    float* red = smem;  // [64][161] reused (fits: 64*161 <= 64*129 + 2691)
    constexpr int RLD = 161;
    int tid_e = tid;
    asm volatile("" : "+v"(tid_e));  // the addresses below are formed here, not carried in registers through the tile loop
    const int li_e = tid_e & 31, h_e = (tid_e >> 5) & 1;
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int kb = 0; kb < SW_KB; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int co = 32 * i + acc_row(r) + 4 * h_e, k = 32 * kb + li_e;
                        float* p = red + co * RLD + k;
                        *p = (w == 0) ? acc[i][kb][r] : *p + acc[i][kb][r];
                    }
        }
        __syncthreads();
    }
    float* slab = slabs + (size_t)blockIdx.x * ST_CO * ST_KK;
    for (int i = tid_e; i < ST_CO * ST_KK; i += 256) {
        const int co = i / ST_KK, k = i - co * ST_KK;
        slab[i] = red[co * RLD + k];
    }
}

static StemShape stem_shape(int B, int H, int W) {
    return StemShape{B, H, W, (H + 2 * ST_PAD - ST_K) / ST_S + 1, (W + 2 * ST_PAD - ST_K) / ST_S + 1};
}

size_t stem_conv_wrw_workspace(int B, int H, int W) {
    const StemShape s = stem_shape(B, H, W);
    return align_up((size_t)B * ceil_div(s.Ho, SW_TH) * ST_CO * ST_KK * sizeof(float), 256);
}

hipError_t stem_conv_fwd_run(const float* x, const float* w, int B, int H, int W, float* y, hipStream_t stream) {
    const StemShape s = stem_shape(B, H, W);
    const size_t lds = ((size_t)ST_CO * ST_WLD + SF_PATCH) * sizeof(float);
    static bool attr = false;
    if (!attr) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(stem_conv_fwd_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr = true;
    }
    hipLaunchKernelGGL(stem_conv_fwd_kernel, dim3(B * ceil_div(s.Ho, SF_TH)), dim3(256), lds, stream, x, w, s,
                       ceil_div(s.Wo, SF_TW), y);
    return hipGetLastError();
}

// prefetch depth of the two forms (of SW_G channel groups): see the register budget in the header comment
constexpr int SW_PJ_PLAIN = 8, SW_PJ_BN = 4, SW_PJ_BN_RAGGED = 2;

template <bool BN>
static hipError_t stem_wrw_launch(const float* dy, const float* x, const StemBn& bn, int B, int H, int W, float* dw, float* slabs,
                                  hipStream_t stream) {
    const StemShape s = stem_shape(B, H, W);
    const int nslab = B * ceil_div(s.Ho, SW_TH), tiles_x = ceil_div(s.Wo, SW_TW);
    const size_t lds = ((size_t)ST_CO * SW_DLD + SW_PATCH + (BN ? ST_CO * SW_BNP : 0)) * sizeof(float);
    constexpr int PJ = BN ? SW_PJ_BN : SW_PJ_PLAIN, PJR = BN ? SW_PJ_BN_RAGGED : SW_PJ_PLAIN;
    const bool vec = (s.Wo & 3) == 0 && ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(bn.z)) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL((stem_conv_wrw_kernel<BN, true, PJ>), dim3(nslab), dim3(256), lds, stream, dy, x, bn, s, tiles_x, slabs);
    else
        hipLaunchKernelGGL((stem_conv_wrw_kernel<BN, false, PJR>), dim3(nslab), dim3(256), lds, stream, dy, x, bn, s, tiles_x, slabs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the slabs (1024 x 38 KB at 8 x 1024^2) summed on the whole chip: 32 slab lanes per 128-byte segment, then in order
    slab_sum_launch(slabs, nslab, ST_CO * ST_KK, dw, stream);
    return hipGetLastError();
}

hipError_t stem_conv_wrw_run(const float* dy, const float* x, int B, int H, int W, float* dw, void* ws,
                             hipStream_t stream) {
    return stem_wrw_launch<false>(dy, x, StemBn{}, B, H, W, dw, static_cast<float*>(ws), stream);
}

// workspace: the BatchNorm partials + coef (bn_act_workspace), then the slabs
size_t stem_conv_bn_bwd_workspace(int B, int H, int W) {
    const StemShape s = stem_shape(B, H, W);
    return bn_act_workspace(B, ST_CO, s.Ho * s.Wo) + stem_conv_wrw_workspace(B, H, W);
}

// backward of relu(bn(stem_conv(image))) as one operator: g = dL/dy, z = the convolution's output.  BatchNorm's reduce and
// finalize (dweight, dbias, coef), then the weight gradient with dz formed in its loader.
hipError_t stem_conv_bn_bwd_run(const float* g, const float* z, const float* x, const float* bn_weight, const float* bn_bias,
                                const float* save_mean, const float* save_invstd, int B, int H, int W, int training, float* dw,
                                float* dbn_weight, float* dbn_bias, void* ws, hipStream_t stream) {
    const StemShape s = stem_shape(B, H, W);
    const float* coef = nullptr;
    hipError_t e = bn_act_bwd_stats_run(g, z, bn_weight, bn_bias, save_mean, save_invstd, B, ST_CO, s.Ho * s.Wo, ACT_RELU, training,
                                        dbn_weight, dbn_bias, ws, &coef, stream);
    if (e != hipSuccess) return e;
    float* slabs = reinterpret_cast<float*>(static_cast<char*>(ws) + bn_act_workspace(B, ST_CO, s.Ho * s.Wo));
    return stem_wrw_launch<true>(g, x, StemBn{z, save_mean, save_invstd, bn_weight, bn_bias, coef}, B, H, W, dw, slabs, stream);
}

}  // namespace cabinet
