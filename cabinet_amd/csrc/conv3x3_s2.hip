// K15 -- weight gradient (and, 64 -> 64, input gradient and forward) of the 3x3 stride-2 padding-1 bias-free convolutions, NCHW
// fp32, no layout copy.
//
// Serves the spatial branch's conv2 / conv3 (64 -> 64, reference src/models/cabinet.py:112-113, SpatialBranch) and the
// backbone's first layer (3 -> 16, reference src/models/mobilenetv3.py:86-91,173, conv_3x3_bn(3, 16, 2)).  MIOpen computes these
// weight gradients with NHWC implicit-GEMM kernels and first copies x and dy to NHWC and dw back; the product
//     dW[co][ci][ky][kx] = sum_{b,oy,ox} dY[b][co][oy][ox] * X[b][ci][2 oy - 1 + ky][2 ox - 1 + kx]
// contracts over pixels, the contiguous axis of BOTH operands in NCHW.  The 3 -> 16 forward stays the stock operator's (NCHW
// there, no copies); the 64 -> 64 forward is the last section below.
//
//   64 -> 64 : a workgroup (4 waves) walks output rows oy of one 32-pixel column tile.  Per row it multiplies the 64 x 32 dy
//              segment ([co][33]) and the 64 x 3 x 65 input patch ([ci][3 slots][65]: channel pitch 195, odd, so the 32
//              channels on 32 lanes fall on 32 banks) out of LDS.  dW is 2 x 2 x 9 blocks of 32 x 32 (co half, ci half, tap);
//              wave (i, j) owns the nine taps of its (co half, ci half): 144 accumulator registers, one A read and nine B
//              reads ("pixel pair on h, channel on li") per nine exact-fp32 MFMA 32x32x2.  All four waves walk the same pixels
//              and own disjoint blocks, so no cross-wave sum exists: each wave stores its blocks of the workgroup's slab.
//              Staging: the three patch rows are a ring -- input row 2 oy + 1 of step oy is row 2 (oy + 1) - 1 of the next step
//              and stays in its slot; the two new rows and the dy segment of step oy + 1 are requested before the MFMAs of
//              step oy (41 registers per thread: whole-wave row segments at wave-uniform (channel, row) bases, lane = column,
//              unconditional clamped loads) and written behind them, 0 selected on the way into LDS for iy = -1, iy >= H,
//              ix = -1, ix >= W and ox >= Wo.  Every input row is fetched once per workgroup.  Two barriers per step: a
//              one-barrier ring needs five row slots (100 KB); with three, 58 KB of LDS and 246 VGPRs keep two workgroups
//              per CU.  The staging this replaces (57 scalar loads per thread and step, each behind a division and a bounds
//              test, all written to LDS before the step's first MFMA, the shared row read again) ran at 0.21 / 0.18 of the
//              fp32 MFMA rate (sb.conv2 / sb.conv3, config 3); this one at 0.63 / 0.48, with the same bits.
//   3 -> 16  : K9's weight-gradient form at (Ci 3, k 3, Co 16): a 4 x 32 output tile, the dy tile ([32][129], rows 16..31
//              zero) and the 3 x 9 x 65 patch in LDS, one 32 x 32 block per wave (27 of 32 columns live), wave = tile row,
//              ordered cross-wave sum.  234 MB of operands for 1.8 GFLOP: a streaming kernel.
//   output   : one slab per workgroup, ordered slab sum (slab_sum.hpp): no atomics, bit-reproducible, capturable.
//
// Input gradient, 64 -> 64:
//     dX[b][ci][iy][ix] = sum_{co,ky,kx} W[co][ci][ky][kx] * dY[b][co][(iy + 1 - ky) / 2][(ix + 1 - kx) / 2]
// over the taps where both quotients are integers and in range: by the four parity classes of (iy, ix), which take 1, 2, 2 and
// 4 taps, so no product with a structural zero is executed.  M = ci, N = the pixels of a class, K = co x taps, on the exact-fp32
// MFMA 16x16x4: a wave owns 16 input channels and keeps their 64 x 9 weights in 144 registers for the whole kernel (the A
// operand never touches the LDS); the workgroup keeps a ring of three dy rows ([co][3][80]) in LDS -- rows m and m + 1 of the
// step, row m + 2 requested before the step's MFMAs and written behind them, every row fetched once -- and every wave reads its B
// operand from them, tap by tap.  Staging loads are unconditional row segments (clamped addresses, 0 selected on the way into
// LDS).  The even- and odd-column classes of one lane are neighbours in dX: a lane
// stores them as one pair, 16 lanes as one 128-byte run.  Every element of dX is written (rows and columns past the last tap
// included: their sums are over zero-staged dy).
// Register budget at 2 workgroups per CU (256 VGPRs): 144 weights, 16 accumulators, 8 tap partials, 17 prefetch, two half-taps of
// B operands (16); no scratch.  The staging this replaces (both rows of a pair between two barriers, ~33 loads per thread each
// behind two divisions and a bounds select, row m + 1 fetched twice) ran at 0.41 of the fp32 MFMA rate with 0.46 of the wave
// cycles parked; this one at 0.73 with 0.11.
//
// Forward, 64 -> 64 (conv3x3s2_fwd64_kernel):
//     Y[b][co][oy][ox] = sum_{ci,ky,kx} W[co][ci][ky][kx] * X[b][ci][2 oy - 1 + ky][2 ox - 1 + kx]
// the gather form of the input gradient's scatter (the stock operator runs it as an NHWC implicit GEMM between a copy of x to
// NHWC and a copy of y back).  M = co, N = output pixels, K = ci x 9 taps = 576 on the exact-fp32 MFMA 16x16x4: a wave owns 16
// output channels and keeps their 64 x 9 weights in 144 registers for the whole kernel (the A operand never touches the LDS).
// A workgroup (4 waves) walks the output rows oy of one strip (cv_plan: 512 workgroups aimed at) of one T = 32 column tile of one
// image.  The input lives in LDS as a ring of three rows (2 oy - 1, 2 oy, 2 oy + 1) of all 64 channels; row 2 oy + 1 stays in its
// slot for the next step, the two new rows are requested before the step's MFMAs (33 registers per thread: whole-wave row
// segments at wave-uniform (ci, row) bases, lane = column, unconditional clamped loads) and written behind them, 0 selected on
// the way into LDS for iy = -1, iy >= H, ix = -1, ix >= W: nothing is masked by multiplication.  Every input row is fetched once
// per workgroup (the first step's three rows are the only unpipelined fetch).  Two barriers per step, as in the weight gradient.
//   B operand : tap kx of 16 neighbouring output pixels reads input columns 2 ox - 1 + kx, a stride of 2; so a row is staged split
//               by column parity -- [patch columns 0, 2, .., 2 T | 1, 3, .., 2 T - 1] -- and every B read is a unit-stride run
//               of 16 (kx = 0: even run at n, kx = 1: odd run at n, kx = 2: even run at n + 1).  Row pitch 66, channel pitch 208
//               = 16 mod 32: the two k-groups (channels 4 ks + lk) of a 32-lane ds_read_b32 group fall on disjoint banks.
//   order     : tap by tap, the 64 input channels of a tap as two interleaved chains of 32 terms, folded into the pixel's sum
//               in tap order (the fold is pinned where it is written: sunk to the guarded store it kept nine taps' partials
//               live and spilled 26 registers).  The order does not depend on the strip, the tile or the launch; no atomics.
//   stores    : register r of a lane is output channel co0 + 4 lk + r of its pixel: 16 lanes store a 64-byte run of a row of y.
//   resources : 214 VGPRs (144 weights, 4 accumulators, 8 tap partials, two half-taps of B operands, 33 prefetch), no scratch,
//               53,248 B of LDS: two workgroups per CU.  The group loop is not unrolled and the half-taps are fenced as in the
//               input gradient.  In the step the 33 staging loads issue before the first MFMA; the waits ahead of them only
//               retire the previous step's stores of y, the loads are first waited for behind the last MFMA.
//   measured  : operator alone, hipGraph replay against the whole stock call (profiles/conv3x3s2_fwd64_summary.md), share of the
//               157.3 TFLOP/s fp32 MFMA rate: sb.conv2 / sb.conv3 at config 3 0.66 / 0.59 (373 and 104 us against 626 and 153),
//               at config 5 0.64 / 0.50, of one 1024 x 2048 image 0.56 / 0.40; the shorter the strip, the larger the share of
//               the unpipelined first step.  The T = 64 variant (-DCABINET_CV_TW=64: 102,400 B of LDS, one workgroup per CU,
//               246 VGPRs, the same bits) ran at 0.50 / 0.45 / 0.47 / 0.41 / 0.45 / 0.36 of the rate: with one wave per SIMD
//               nothing covers the barriers and the LDS writes of the hand-over.  T = 32 is what is built.
#include "common.hpp"
#include "slab_sum.hpp"

namespace cabinet {

struct C3Shape {
    int B, H, W, Ho, Wo;
};

static C3Shape c3_shape(int B, int H, int W) { return C3Shape{B, H, W, (H - 1) / 2 + 1, (W - 1) / 2 + 1}; }

// ------------------------------------------------------------------------------------------------ 64 -> 64
constexpr int CW_C = 64;                  // channels, both sides
constexpr int CW_TW = 32;                 // output pixels of a step: one row segment
constexpr int CW_IW = 2 * CW_TW + 1;      // 65 input columns
constexpr int CW_XP = 3 * CW_IW;          // 195: channel pitch of the patch (odd)
constexpr int CW_DLD = CW_TW + 1;         // 33: row stride of the dy segment
constexpr int CW_SLAB = CW_C * CW_C * 9;  // 36864 floats
constexpr int CW_TARGET_WG = 512;         // two resident workgroups on each of the 256 CUs
constexpr int CW_MIN_ROWS = 4;            // a workgroup walks at least this many rows per 147 KB slab it writes

struct C3Plan {
    int tiles_x, strips, rows_per;
};

static C3Plan cw_plan(const C3Shape& s) {
    C3Plan p;
    p.tiles_x = ceil_div(s.Wo, CW_TW);
    const long per = (long)s.B * p.tiles_x;
    long strips = CW_TARGET_WG / per;
    const int cap = ceil_div(s.Ho, CW_MIN_ROWS);
    if (strips > cap) strips = cap;
    if (strips < 1) strips = 1;
    p.rows_per = ceil_div(s.Ho, (int)strips);
    p.strips = ceil_div(s.Ho, p.rows_per);
    return p;
}

// load at a wave-uniform base + a 32-bit per-lane byte offset
__device__ __forceinline__ float cd_ld(const float* base, unsigned byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}

constexpr int CW_PR = CW_C / 4;  // 16 channels' row segments per wave and input row

__global__ __launch_bounds__(256, 2) void conv3x3s2_wgrad64_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 C3Shape s, int tiles_x, int strips, int rows_per,
                                                                 float* __restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;                 // [64][3 slots][65]: a ring of input rows; column 0 is ix0 = 2 ox0 - 1
    float* dys = xs + CW_C * CW_XP;   // [64][33]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;
    int bi = blockIdx.x;
    const int tx = bi % tiles_x;
    bi /= tiles_x;
    const int strip = bi % strips, b = bi / strips;
    const int oy_begin = strip * rows_per, oy_end = min(s.Ho, oy_begin + rows_per);
    const int ox0 = tx * CW_TW, ix0 = 2 * ox0 - 1;
    const int ch = wave & 1, cj = wave >> 1;  // this wave's co half and ci half

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const float* xb = x + (size_t)b * CW_C * s.H * s.W;
    const float* dyb = dy + (size_t)b * CW_C * s.Ho * s.Wo;
    const float* arow = dys + (32 * ch + li) * CW_DLD + h;
    const float* brow = xs + (32 * cj + li) * CW_XP + 2 * h;
    // Staging.  An input row is 64 channels x 65 columns: this wave's 16 channels as row segments (wave-uniform (ci, row) base,
    // lane = column 2 ox0 + lane, patch column 1 + lane) and the left halo column ix0 as one element per thread (thread = (row of
    // the request, channel)).  The dy segment is 64 channels x 32 columns: a wave load takes two channels (co = 16 wave + 2 j + h,
    // column ox0 + li).  Every load is unconditional: row and column are clamped into the tensor, and what lies outside it
    // (iy = -1, iy >= H, ix = -1, ix >= W, ox >= Wo) is replaced by 0 on the way into LDS.
    const unsigned colo = (unsigned)min(2 * ox0 + lane, s.W - 1) * 4u;
    const bool col_ok = 2 * ox0 + lane < s.W, halo_ok = ix0 >= 0, dcol_ok = ox0 + li < s.Wo;
    const int hrow = tid >> 6, hch = tid & 63;
    const float* dyl = dyb + (size_t)h * s.Ho * s.Wo + min(ox0 + li, s.Wo - 1);
    float xr[2 * CW_PR], xh, dr[CW_PR / 2];
    // rows iya (and, nr = 2, iyb) of x; with_dy: the dy segment of output row oy
    auto request = [&](int nr, int iya, int iyb, bool with_dy, int oy) {
        const int ya = min(max(iya, 0), s.H - 1), yb = min(max(iyb, 0), s.H - 1);
#pragma unroll
        for (int j = 0; j < CW_PR; ++j) xr[j] = cd_ld(xb + ((size_t)(CW_PR * wave + j) * s.H + ya) * s.W, colo);
        if (nr == 2) {
#pragma unroll
            for (int j = 0; j < CW_PR; ++j) xr[CW_PR + j] = cd_ld(xb + ((size_t)(CW_PR * wave + j) * s.H + yb) * s.W, colo);
        }
        xh = xb[((size_t)hch * s.H + (hrow == 0 ? ya : yb)) * s.W + max(ix0, 0)];
        if (with_dy) {
#pragma unroll
            for (int j = 0; j < CW_PR / 2; ++j) dr[j] = dyl[((size_t)(CW_PR * wave + 2 * j) * s.Ho + oy) * s.Wo];
        }
    };
    auto commit = [&](int nr, int iya, int iyb, int sa, int sb, bool with_dy) {
        const bool oka = iya >= 0 && iya < s.H, okb = iyb >= 0 && iyb < s.H;
        float* d = xs + CW_PR * wave * CW_XP + 1 + lane;
#pragma unroll
        for (int j = 0; j < CW_PR; ++j) d[j * CW_XP + sa * CW_IW] = (oka && col_ok) ? xr[j] : 0.f;
        if (nr == 2) {
#pragma unroll
            for (int j = 0; j < CW_PR; ++j) d[j * CW_XP + sb * CW_IW] = (okb && col_ok) ? xr[CW_PR + j] : 0.f;
        }
        if (hrow < nr) xs[hch * CW_XP + (hrow == 0 ? sa : sb) * CW_IW] = ((hrow == 0 ? oka : okb) && halo_ok) ? xh : 0.f;
        if (with_dy) {
#pragma unroll
            for (int j = 0; j < CW_PR / 2; ++j) dys[(CW_PR * wave + 2 * j + h) * CW_DLD + li] = dcol_ok ? dr[j] : 0.f;
        }
    };
    // Input row iy of the strip lives in slot (iy - iy_begin) % 3.  Step oy multiplies rows 2 oy - 1 .. 2 oy + 1 (slots s0, s0 + 1,
    // s0 + 2) while the two new rows of step oy + 1 and its dy segment are in flight in registers; behind the MFMAs they are
    // written over rows 2 oy - 1 and 2 oy, and row 2 oy + 1 stays where it is: every input row is fetched once per workgroup.
    // Five slots (three in use, two being written) would take one barrier per step and 100 KB; three take two and 58 KB, and
    // two workgroups share a CU.
    const int iy_begin = 2 * oy_begin - 1;
    request(2, iy_begin, iy_begin + 1, true, oy_begin);
    commit(2, iy_begin, iy_begin + 1, 0, 1, true);
    request(1, iy_begin + 2, iy_begin + 2, false, 0);
    commit(1, iy_begin + 2, iy_begin + 2, 2, 2, false);
    __syncthreads();
    int s0 = 0;  // slot of row 2 oy - 1
    for (int oy = oy_begin; oy < oy_end; ++oy) {
        const int s1 = s0 == 2 ? 0 : s0 + 1, s2 = s1 == 2 ? 0 : s1 + 1;
        const bool more = oy + 1 < oy_end;
        if (more) request(2, 2 * oy + 2, 2 * oy + 3, true, oy + 1);  // in flight underneath this step's MFMAs
        const float* b0 = brow + s0 * CW_IW;
        const float* b1 = brow + s1 * CW_IW;
        const float* b2 = brow + s2 * CW_IW;
#pragma unroll
        for (int c0 = 0; c0 < CW_TW; c0 += 2) {  // pixels c0 + h: two per MFMA
            const float a = arow[c0];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[kx] = mfma32(a, b0[2 * c0 + kx], acc[kx]);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[3 + kx] = mfma32(a, b1[2 * c0 + kx], acc[3 + kx]);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[6 + kx] = mfma32(a, b2[2 * c0 + kx], acc[6 + kx]);
        }
        if (more) {
            __syncthreads();  // every wave has read this step's operands
            commit(2, 2 * oy + 2, 2 * oy + 3, s0, s1, true);
            __syncthreads();
        }
        s0 = s2;
    }
    // this wave's 32 x 32 x 9 part of the slab, in dW's own layout [co][ci][tap]
    float* slab = slabs + (size_t)blockIdx.x * CW_SLAB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = 32 * ch + acc_row(r) + 4 * h, ci = 32 * cj + li;
        float* p = slab + (co * CW_C + ci) * 9;
#pragma unroll
        for (int t = 0; t < 9; ++t) p[t] = acc[t][r];
    }
}

// ------------------------------------------------------------------------------------------------ 3 -> 16
constexpr int CF_CI = 3, CF_CO = 16, CF_KK = CF_CI * 9;  // 27 columns
constexpr int CF_TH = 4, CF_TW = 32;                     // 128 pixels per step, 32 per wave
constexpr int CF_IH = 2 * CF_TH + 1, CF_IW = 2 * CF_TW + 1;  // 9 x 65
constexpr int CF_PATCH = CF_CI * CF_IH * CF_IW;          // 1755 floats
constexpr int CF_DLD = CF_TH * CF_TW + 1;                // 129: row stride of the dy tile
constexpr int CF_SLAB = CF_CO * CF_KK;                   // 432 floats

__global__ __launch_bounds__(256) void conv3x3s2_wgrad_3_16_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                  C3Shape s, int tiles_x, float* __restrict__ slabs) {
    __shared__ __attribute__((aligned(16))) float dys[32 * CF_DLD];  // rows 16..31 stay zero: the A operand's upper half
    __shared__ float xs[CF_PATCH];                                    // [3][9][65]
    __shared__ float red[4][CF_CO][32];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
    const int strips_y = (s.Ho + CF_TH - 1) / CF_TH;
    const int b = blockIdx.x / strips_y, oy0 = (blockIdx.x - b * strips_y) * CF_TH;
    // patch offset of this lane's column k = li = (ci, ky, kx); columns >= 27 read offset 0 and are dropped
    const int kk = li < CF_KK ? li : 0;
    const int ko = ((kk / 9) * CF_IH + (kk % 9) / 3) * CF_IW + kk % 3;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int i = tid; i < 16 * CF_DLD; i += 256) dys[16 * CF_DLD + i] = 0.f;
    const float* xb = x + (size_t)b * CF_CI * s.H * s.W;
    const float* dyb = dy + (size_t)b * CF_CO * s.Ho * s.Wo;
    const int iy0 = 2 * oy0 - 1;
    for (int t = 0; t < tiles_x; ++t) {
        const int ox0 = t * CF_TW, ix0 = 2 * ox0 - 1;
        __syncthreads();
        for (int i = tid; i < CF_PATCH; i += 256) {
            const int ci = i / (CF_IH * CF_IW), r = i - ci * CF_IH * CF_IW, yy = r / CF_IW, xx = r - yy * CF_IW;
            const int iy = iy0 + yy, ix = ix0 + xx;
            xs[i] = (iy >= 0 && iy < s.H && ix >= 0 && ix < s.W) ? xb[((size_t)ci * s.H + iy) * s.W + ix] : 0.f;
        }
        for (int i = tid; i < CF_CO * CF_TH * CF_TW; i += 256) {
            const int co = i / (CF_TH * CF_TW), p = i - co * (CF_TH * CF_TW), r = p / CF_TW, c = p - r * CF_TW;
            const int oy = oy0 + r, ox = ox0 + c;
            dys[co * CF_DLD + p] = (oy < s.Ho && ox < s.Wo) ? dyb[((size_t)co * s.Ho + oy) * s.Wo + ox] : 0.f;
        }
        __syncthreads();
        // this wave contracts over output row `wave` of the tile, two pixels per MFMA
        const float* drow = dys + li * CF_DLD + 32 * wave + h;
        const float* prow = xs + ko + 2 * wave * CF_IW + 2 * h;
#pragma unroll
        for (int c0 = 0; c0 < 32; c0 += 2) acc = mfma32(drow[c0], prow[2 * c0], acc);
    }
    // rows 0..15 of the block are registers 0..7 (acc_row(r) + 4 h < 16); the four waves' copies are added in wave order
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = acc_row(r) + 4 * h;
        if (co < CF_CO) red[wave][co][li] = acc[r];
    }
    __syncthreads();
    float* slab = slabs + (size_t)blockIdx.x * CF_SLAB;
    for (int i = tid; i < CF_SLAB; i += 256) {
        const int co = i / CF_KK, k = i - co * CF_KK;
        slab[i] = ((red[0][co][k] + red[1][co][k]) + red[2][co][k]) + red[3][co][k];
    }
}

// ------------------------------------------------------------------------------------------------ input gradient, 64 -> 64
typedef float f32x4v __attribute__((ext_vector_type(4)));
// v_mfma_f32_16x16x4_f32: lane l supplies A[row = l&15][k = l>>4] and B[k = l>>4][col = l&15]; register r of lane l is
// D[row = 4*(l>>4) + r][col = l&15]
__device__ __forceinline__ f32x4v mfma16(float a, float b, f32x4v c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int CD_NT = 64;             // columns n of dy per step: 128 columns of dX
constexpr int CD_RP = 80;             // row pitch of the dy ring (65 columns live)
constexpr int CD_SLOTS = 3;           // rows m, m + 1 of the step and row m + 2 on its way in
constexpr int CD_CP = CD_SLOTS * CD_RP;  // 240: channel pitch, = 16 mod 32 (the two channels of a 32-lane read group: disjoint banks)
constexpr int CD_PR = CW_C / 4;       // 16 channels' row segments per wave and dy row

// the tap of dY that input parity 0 (even) / 1 (odd) takes with kernel index k: even rows take k = 1 from row m; odd rows
// take k = 0 from row m + 1 and k = 2 from row m
__host__ __device__ constexpr int cd_par(int k) { return k == 1 ? 0 : 1; }
__host__ __device__ constexpr int cd_shift(int k) { return k == 0 ? 1 : 0; }

__global__ __launch_bounds__(256, 2) void conv3x3s2_dgrad64_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                 C3Shape s, int tiles_n, int strips, int rows_per,
                                                                 float* __restrict__ dx) {
    __shared__ __attribute__((aligned(16))) float dys[CW_C * CD_CP];  // [co][3 slots][80]: a ring of dy rows
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lc = lane & 15, lk = lane >> 4;
    int bi = blockIdx.x;
    const int tn = bi % tiles_n;
    bi /= tiles_n;
    const int strip = bi % strips, b = bi / strips;
    const int m_begin = strip * rows_per, m_end = min(s.Ho, m_begin + rows_per);
    const int n0 = tn * CD_NT;
    const int ci0 = 16 * wave;  // this wave's 16 input channels: their 64 x 9 weights stay in registers

    float wr[9][16];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) wr[t][ks] = w[((4 * ks + lk) * CW_C + ci0 + lc) * 9 + t];

    const float* dyb = dy + (size_t)b * CW_C * s.Ho * s.Wo;
    float* dxb = dx + ((size_t)b * CW_C + ci0 + 4 * lk) * s.H * s.W;
    const float* brow = dys + lk * CD_CP + lc;
    const bool pair_ok = (s.W & 1) == 0;  // rows of dX start 8-byte aligned
    // Staging of one dy row (64 channels x 65 columns): this wave's 16 channels as row segments (wave-uniform (co, row) base,
    // lane = column n0 + lane) and, one per thread of wave 0, the halo column n0 + 64 of channel tid.  Every load is
    // unconditional: row and column are clamped into the tensor and what lies outside is replaced by 0 on the way into LDS.
    const unsigned colo = (unsigned)min(n0 + lane, s.Wo - 1) * 4u;
    const bool col_ok = n0 + lane < s.Wo, halo_ok = n0 + CD_NT < s.Wo;
    float pp[CD_PR + 1];
    auto request = [&](int r) {
        const int oy = min(r, s.Ho - 1);
#pragma unroll
        for (int j = 0; j < CD_PR; ++j) pp[j] = cd_ld(dyb + ((size_t)(CD_PR * wave + j) * s.Ho + oy) * s.Wo, colo);
        int te = tid;  // the halo element's address is formed here, not carried (two registers) through the MFMAs
        asm volatile("" : "+v"(te));
        pp[CD_PR] = dyb[((size_t)min(te, CW_C - 1) * s.Ho + oy) * s.Wo + min(n0 + CD_NT, s.Wo - 1)];
    };
    auto commit = [&](int r, int slot) {
        const bool row_ok = r < s.Ho;
        float* d = dys + slot * CD_RP;
#pragma unroll
        for (int j = 0; j < CD_PR; ++j) d[(CD_PR * wave + j) * CD_CP + lane] = (row_ok && col_ok) ? pp[j] : 0.f;
        if (tid < CW_C) d[tid * CD_CP + CD_NT] = (row_ok && halo_ok) ? pp[CD_PR] : 0.f;
    };
    // Row r of the strip lives in slot (r - m_begin) % 3.  Step m multiplies rows (m, m + 1) while row m + 2 is in flight; it is
    // written at the top of step m + 1 over row m - 1, whose last readers (step m - 1) are behind the barrier of step m: one
    // barrier per step, every dy row fetched once per workgroup.
    request(m_begin);
    commit(m_begin, 0);
    request(m_begin + 1);
    int s0 = 0;  // slot of row m
    for (int m = m_begin; m < m_end; ++m) {
        const int s1 = s0 == CD_SLOTS - 1 ? 0 : s0 + 1;
        commit(m + 1, s1);
        __syncthreads();
        if (m + 1 < m_end) request(m + 2);  // in flight underneath this step's MFMAs
        const float* bp0 = brow + s0 * CD_RP;  // row m
        const float* bp1 = brow + s1 * CD_RP;  // row m + 1
        s0 = s1;
#pragma unroll 1  // 144 MFMAs per group already: unrolling the groups only spills the weights
        for (int ng = 0; ng < CD_NT / 16 && n0 + 16 * ng < s.Wo; ++ng) {
            f32x4v acc[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};
            // tap by tap, the 64 output channels of a tap as two interleaved chains of 32 (k-steps of 4 channels, even and odd:
            // no MFMA waits on the one before it), folded into the class sum in a fixed order: the longest fp32 chain is 32
            // terms, which keeps the result as close to fp64 as the stock kernel's
            // The B operands of half-tap g + 1 (8 k-steps) are read while half-tap g is multiplied, and no further ahead (the
            // scheduling barrier): with the 144 weights and the row in flight there are registers for two half-taps' operands,
            // not for the taps the scheduler would hoist.
            float bv[2][8];
            auto read_half = [&](int g, float* v) {
                const int t = g / 2;
                const float* bt = (cd_shift(t / 3) ? bp1 : bp0) + 16 * ng + cd_shift(t % 3);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = bt[4 * (8 * (g % 2) + i) * CD_CP];
            };
            read_half(0, bv[0]);
            f32x4v p0, p1;
#pragma unroll
            for (int g = 0; g < 18; ++g) {
                const int t = g / 2, k8 = 8 * (g % 2);
                if (g + 1 < 18) read_half(g + 1, bv[(g + 1) & 1]);
                if (g % 2 == 0) p0 = p1 = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 8; i += 2) {
                    p0 = mfma16(wr[t][k8 + i], bv[g & 1][i], p0);
                    p1 = mfma16(wr[t][k8 + i + 1], bv[g & 1][i + 1], p1);
                }
                if (g % 2 == 1) acc[cd_par(t / 3)][cd_par(t % 3)] += p0 + p1;
                __builtin_amdgcn_sched_barrier(0);
            }
            // column pair (2 n, 2 n + 1) of one lane: 16 lanes store 128 contiguous bytes of a dX row
            const int ix = 2 * (n0 + 16 * ng + lc);
#pragma unroll
            for (int rp = 0; rp < 2; ++rp) {
                const int iy = 2 * m + rp;
                if (iy < s.H && ix < s.W) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* p = dxb + ((size_t)r * s.H + iy) * s.W + ix;
                        if (pair_ok) {
                            *reinterpret_cast<f32x2*>(p) = f32x2{acc[rp][0][r], acc[rp][1][r]};
                        } else {
                            p[0] = acc[rp][0][r];
                            if (ix + 1 < s.W) p[1] = acc[rp][1][r];
                        }
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward, 64 -> 64
#ifndef CABINET_CV_TW
#define CABINET_CV_TW 32  // 64 is the one-workgroup-per-CU variant the header's table was measured with
#endif
constexpr int CV_TW = CABINET_CV_TW;   // output columns of a tile: 2 T + 1 input columns
constexpr int CV_NSEG = CV_TW / 32;    // 64-column wave segments of an input row
constexpr int CV_EV = 0;               // run of the patch columns j = 2 n (ix = 2 (ox0 + n) - 1), n = 0 .. T: taps kx = 0 (n) and 2 (n + 1)
constexpr int CV_OD = CV_TW + 1;       // run of the patch columns j = 2 n + 1 (ix = 2 (ox0 + n)), n = 0 .. T - 1: tap kx = 1
constexpr int CV_RP = 2 * CV_TW + 2;   // row pitch (2 T + 1 live)
constexpr int CV_CP = (3 * CV_RP - 16 + 31) / 32 * 32 + 16;  // channel pitch >= 3 rows, = 16 mod 32: 208 (T 32), 400 (T 64)
constexpr int CV_PR = CW_C / 4;        // 16 channels' row segments per wave and input row
constexpr int CV_WG_PER_CU = CV_TW == 32 ? 2 : 1;
constexpr int CV_TARGET_WG = 256 * CV_WG_PER_CU;
constexpr size_t CV_LDS = (size_t)CW_C * CV_CP * sizeof(float);  // 53,248 B (T 32), 102,400 B (T 64)
static_assert(CV_TW == 32 || CV_TW == 64, "the staging covers a row with one or two 64-lane segments");
static_assert(CV_CP % 32 == 16 && CV_CP >= 3 * CV_RP, "k-groups lk and lk + 1 of a 32-lane read group on disjoint banks");

__host__ __device__ constexpr int cv_koff(int kx) { return kx == 0 ? CV_EV : kx == 1 ? CV_OD : CV_EV + 1; }

__global__ __launch_bounds__(256, CV_WG_PER_CU) void conv3x3s2_fwd64_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                          C3Shape s, int tiles_x, int strips, int rows_per,
                                                                          float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;  // [ci][3 slots][even run | odd run]: a ring of input rows, each split by column parity
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lc = lane & 15, lk = lane >> 4;
    int bi = blockIdx.x;
    const int tx = bi % tiles_x;
    bi /= tiles_x;
    const int strip = bi % strips, b = bi / strips;
    const int oy_begin = strip * rows_per, oy_end = min(s.Ho, oy_begin + rows_per);
    const int ox0 = tx * CV_TW, ix0 = 2 * ox0 - 1;
    const int co0 = 16 * wave;  // this wave's 16 output channels: their 64 x 9 weights stay in registers

    float wr[9][16];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) wr[t][ks] = w[((co0 + lc) * CW_C + 4 * ks + lk) * 9 + t];

    const float* xb = x + (size_t)b * CW_C * s.H * s.W;
    float* yb = y + ((size_t)b * CW_C + co0 + 4 * lk) * s.Ho * s.Wo;
    const float* brow = xs + lk * CV_CP + lc;
    // Staging.  An input row is 64 channels x (2 T + 1) columns: this wave's 16 channels as row segments (wave-uniform (ci, row)
    // base, lane = column ix = 2 ox0 + c, c = 64 sg + lane: patch column j = c + 1, so even c goes to the odd run and odd c to
    // the even run) and the left halo column ix0 (j = 0) as one element per thread (thread = (row of the request, channel)).
    // Every load is unconditional: row and column are clamped into the tensor, and what lies outside it (iy = -1, iy >= H,
    // ix = -1, ix >= W) is replaced by 0 on the way into LDS.
    unsigned colo[CV_NSEG];
    int dcol[CV_NSEG];
    bool col_ok[CV_NSEG];
#pragma unroll
    for (int sg = 0; sg < CV_NSEG; ++sg) {
        const int c = 64 * sg + lane;
        colo[sg] = (unsigned)min(2 * ox0 + c, s.W - 1) * 4u;
        col_ok[sg] = 2 * ox0 + c < s.W;
        dcol[sg] = (c & 1) ? CV_EV + (c + 1) / 2 : CV_OD + c / 2;
    }
    const bool halo_ok = ix0 >= 0;
    const int hrow = tid >> 6, hch = tid & 63;
    float xr[2 * CV_PR * CV_NSEG], xh;
    auto request = [&](int nr, int iya, int iyb) {  // rows iya (and, nr = 2, iyb) of x
        const int ya = min(max(iya, 0), s.H - 1), yb_ = min(max(iyb, 0), s.H - 1);
#pragma unroll
        for (int j = 0; j < CV_PR; ++j)
#pragma unroll
            for (int sg = 0; sg < CV_NSEG; ++sg)
                xr[j * CV_NSEG + sg] = cd_ld(xb + ((size_t)(CV_PR * wave + j) * s.H + ya) * s.W, colo[sg]);
        if (nr == 2) {
#pragma unroll
            for (int j = 0; j < CV_PR; ++j)
#pragma unroll
                for (int sg = 0; sg < CV_NSEG; ++sg)
                    xr[(CV_PR + j) * CV_NSEG + sg] = cd_ld(xb + ((size_t)(CV_PR * wave + j) * s.H + yb_) * s.W, colo[sg]);
        }
        xh = xb[((size_t)hch * s.H + (hrow == 0 ? ya : yb_)) * s.W + max(ix0, 0)];
    };
    auto commit = [&](int nr, int iya, int iyb, int sa, int sb) {
        const bool oka = iya >= 0 && iya < s.H, okb = iyb >= 0 && iyb < s.H;
        float* d = xs + CV_PR * wave * CV_CP;
#pragma unroll
        for (int j = 0; j < CV_PR; ++j)
#pragma unroll
            for (int sg = 0; sg < CV_NSEG; ++sg)
                d[j * CV_CP + sa * CV_RP + dcol[sg]] = (oka && col_ok[sg]) ? xr[j * CV_NSEG + sg] : 0.f;
        if (nr == 2) {
#pragma unroll
            for (int j = 0; j < CV_PR; ++j)
#pragma unroll
                for (int sg = 0; sg < CV_NSEG; ++sg)
                    d[j * CV_CP + sb * CV_RP + dcol[sg]] = (okb && col_ok[sg]) ? xr[(CV_PR + j) * CV_NSEG + sg] : 0.f;
        }
        if (hrow < nr) xs[hch * CV_CP + (hrow == 0 ? sa : sb) * CV_RP + CV_EV] = ((hrow == 0 ? oka : okb) && halo_ok) ? xh : 0.f;
    };
    // Input row iy of the strip lives in slot (iy - iy_begin) % 3.  Step oy multiplies rows 2 oy - 1 .. 2 oy + 1 (slots s0, s1, s2)
    // while the two new rows of step oy + 1 are in flight in registers; behind the MFMAs they are written over rows 2 oy - 1
    // and 2 oy, and row 2 oy + 1 stays where it is: every input row is fetched once per workgroup.
    const int iy_begin = 2 * oy_begin - 1;
    request(2, iy_begin, iy_begin + 1);
    commit(2, iy_begin, iy_begin + 1, 0, 1);
    request(1, iy_begin + 2, iy_begin + 2);
    commit(1, iy_begin + 2, iy_begin + 2, 2, 2);
    __syncthreads();
    int s0 = 0;  // slot of row 2 oy - 1
    for (int oy = oy_begin; oy < oy_end; ++oy) {
        const int s1 = s0 == 2 ? 0 : s0 + 1, s2 = s1 == 2 ? 0 : s1 + 1;
        const bool more = oy + 1 < oy_end;
        if (more) request(2, 2 * oy + 2, 2 * oy + 3);  // in flight underneath this step's MFMAs
        const float* bp0 = brow + s0 * CV_RP;  // row 2 oy - 1
        const float* bp1 = brow + s1 * CV_RP;  // row 2 oy
        const float* bp2 = brow + s2 * CV_RP;  // row 2 oy + 1
#pragma unroll 1  // 144 MFMAs per group already: unrolling the groups only spills the weights
        for (int ng = 0; ng < CV_TW / 16 && ox0 + 16 * ng < s.Wo; ++ng) {
            f32x4v acc = f32x4v{0.f, 0.f, 0.f, 0.f};
            // tap by tap, the 64 input channels of a tap as two interleaved chains of 32 (k-steps of 4 channels, even and odd: no
            // MFMA waits on the one before it), folded into the pixel's sum in tap order: the longest fp32 chain is 32 terms, and
            // the order does not depend on where the pixel sits.  The B operands of half-tap g + 1 (8 k-steps) are read while
            // half-tap g is multiplied, and no further ahead (the scheduling barrier), as in the input gradient.
            float bv[2][8];
            auto read_half = [&](int g, float* v) {
                const int t = g / 2, ky = t / 3;
                const float* bt = (ky == 0 ? bp0 : ky == 1 ? bp1 : bp2) + 16 * ng + cv_koff(t % 3);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = bt[4 * (8 * (g % 2) + i) * CV_CP];
            };
            read_half(0, bv[0]);
            f32x4v p0, p1;
#pragma unroll
            for (int g = 0; g < 18; ++g) {
                const int t = g / 2, k8 = 8 * (g % 2);
                if (g + 1 < 18) read_half(g + 1, bv[(g + 1) & 1]);
                if (g % 2 == 0) p0 = p1 = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 8; i += 2) {
                    p0 = mfma16(wr[t][k8 + i], bv[g & 1][i], p0);
                    p1 = mfma16(wr[t][k8 + i + 1], bv[g & 1][i + 1], p1);
                }
                if (g % 2 == 1) {
                    acc += p0 + p1;
                    asm volatile("" : "+v"(acc));  // folded here: sunk to the guarded store, nine taps' partials would stay live
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // register r is output channel co0 + 4 lk + r of pixel ox: 16 lanes store 64 contiguous bytes of a row of y
            const int ox = ox0 + 16 * ng + lc;
            if (ox < s.Wo) {
#pragma unroll
                for (int r = 0; r < 4; ++r) yb[((size_t)r * s.Ho + oy) * s.Wo + ox] = acc[r];
            }
        }
        if (more) {
            __syncthreads();  // every wave has read this step's operands
            commit(2, 2 * oy + 2, 2 * oy + 3, s0, s1);
            __syncthreads();
        }
        s0 = s2;
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool conv3x3s2_supported(int Ci, int Co) { return (Ci == CW_C && Co == CW_C) || (Ci == CF_CI && Co == CF_CO); }
bool conv3x3s2_fwd_supported(int Ci, int Co) { return Ci == CW_C && Co == CW_C; }

static C3Plan cv_plan(const C3Shape& s) {  // strips of output rows per (image, column tile), as cd_plan
    C3Plan p;
    p.tiles_x = ceil_div(s.Wo, CV_TW);
    const long per = (long)s.B * p.tiles_x;
    long strips = CV_TARGET_WG / per;
    if (strips > s.Ho) strips = s.Ho;
    if (strips < 1) strips = 1;
    p.rows_per = ceil_div(s.Ho, (int)strips);
    p.strips = ceil_div(s.Ho, p.rows_per);
    return p;
}

long long conv3x3s2_fwd_workgroups(int B, int H, int W) {
    const C3Shape s = c3_shape(B, H, W);
    const long long per = (long long)B * ceil_div(s.Wo, CV_TW);
    if (per > (1ll << 30)) return per;
    const C3Plan p = cv_plan(s);
    return per * p.strips;
}

hipError_t conv3x3s2_fwd_run(const float* x, const float* w, int B, int H, int W, float* y, hipStream_t stream) {
    const C3Shape s = c3_shape(B, H, W);
    const C3Plan p = cv_plan(s);
    static lds_attr_mask mask{0};
    if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(conv3x3s2_fwd64_kernel), CV_LDS, mask); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(conv3x3s2_fwd64_kernel, dim3(B * p.tiles_x * p.strips), dim3(256), CV_LDS, stream, x, w, s, p.tiles_x,
                       p.strips, p.rows_per, y);
    return hipGetLastError();
}

static C3Plan cd_plan(const C3Shape& s) {  // strips of row pairs m per (image, 64-column tile), as cw_plan
    C3Plan p;
    p.tiles_x = ceil_div(s.Wo, CD_NT);
    const long per = (long)s.B * p.tiles_x;
    long strips = CW_TARGET_WG / per;
    if (strips > s.Ho) strips = s.Ho;
    if (strips < 1) strips = 1;
    p.rows_per = ceil_div(s.Ho, (int)strips);
    p.strips = ceil_div(s.Ho, p.rows_per);
    return p;
}

long long conv3x3s2_dgrad_workgroups(int B, int H, int W) {
    const C3Shape s = c3_shape(B, H, W);
    const long long per = (long long)B * ceil_div(s.Wo, CD_NT);
    if (per > (1ll << 30)) return per;
    const C3Plan p = cd_plan(s);
    return per * p.strips;
}

hipError_t conv3x3s2_dgrad_run(const float* dy, const float* w, int B, int H, int W, float* dx, hipStream_t stream) {
    const C3Shape s = c3_shape(B, H, W);
    const C3Plan p = cd_plan(s);
    hipLaunchKernelGGL(conv3x3s2_dgrad64_kernel, dim3(B * p.tiles_x * p.strips), dim3(256), 0, stream, dy, w, s, p.tiles_x,
                       p.strips, p.rows_per, dx);
    return hipGetLastError();
}

// number of slabs (= workgroups) of the weight gradient, as a 64-bit count: the caller checks it against the grid limit
long long conv3x3s2_wgrad_slabs(int B, int Ci, int H, int W) {
    const C3Shape s = c3_shape(B, H, W);
    if (Ci == CF_CI) return (long long)B * ceil_div(s.Ho, CF_TH);
    const long long tiles_x = ceil_div(s.Wo, CW_TW);
    if ((long long)B * tiles_x > (1ll << 30)) return (long long)B * tiles_x;
    const C3Plan p = cw_plan(s);
    return (long long)B * p.tiles_x * p.strips;
}

size_t conv3x3s2_wgrad_workspace(int B, int Ci, int H, int W) {
    return align_up((size_t)conv3x3s2_wgrad_slabs(B, Ci, H, W) * (Ci == CF_CI ? CF_SLAB : CW_SLAB) * sizeof(float), 256);
}

hipError_t conv3x3s2_wgrad_run(const float* dy, const float* x, int B, int Ci, int H, int W, float* dw, void* ws,
                               hipStream_t stream) {
    const C3Shape s = c3_shape(B, H, W);
    float* slabs = static_cast<float*>(ws);
    const int nslab = (int)conv3x3s2_wgrad_slabs(B, Ci, H, W);
    if (Ci == CF_CI) {
        hipLaunchKernelGGL(conv3x3s2_wgrad_3_16_kernel, dim3(nslab), dim3(256), 0, stream, dy, x, s, ceil_div(s.Wo, CF_TW),
                           slabs);
    } else {
        const C3Plan p = cw_plan(s);
        const size_t lds = (size_t)(CW_C * CW_XP + CW_C * CW_DLD) * sizeof(float);
        static lds_attr_mask mask{0};
        if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(conv3x3s2_wgrad64_kernel), lds, mask); e != hipSuccess)
            return e;
        hipLaunchKernelGGL(conv3x3s2_wgrad64_kernel, dim3(nslab), dim3(256), lds, stream, dy, x, s, p.tiles_x, p.strips,
                           p.rows_per, slabs);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    slab_sum_launch(slabs, nslab, Ci == CF_CI ? CF_SLAB : CW_SLAB, dw, stream);
    return hipGetLastError();
}

}  // namespace cabinet
