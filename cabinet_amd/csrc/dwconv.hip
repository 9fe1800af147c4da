// K8 -- depthwise KxK convolution (groups == channels, no bias), forward and backward, NCHW fp32.
//
// Replaces the depthwise nn.Conv2d of the reference's MBConv blocks (src/models/mobilenetv3.py:118-126,135-143:
// kernel 3 or 5, stride 1 or 2, padding k//2) for which MIOpen on gfx950 falls back to its `naive_conv_*` solvers
// (fp32, groups == channels): 12 % of the config-3 step, plus an im2col + 16x16-tile GEMM weight gradient.
//
// A depthwise convolution never mixes channels: every (b,c) plane is an independent KxK stencil with its own
// filter -- a few FLOP per byte, so these kernels only move memory (read x, write y) and what they wait for is HBM
// latency, not arithmetic: ~100 instructions per pixel are ~20 us of issue on a 33 M pixel tensor, and the counters
// (profiles/dwconv_strips_summary.md) have the waves parked on memory for 0.5-0.77 of their cycles, issuing in 0.14-0.30.
//   fwd : y[oy][ox] = sum w[ky][kx] * x[oy*S - p + ky][ox*S - p + kx]
//   bwd : ONE kernel per input-space tile, sharing the staged dy tile between both gradients:
//           dx[y][x]   = sum w[ky][kx] * dy[(y+p-ky)/S][(x+p-kx)/S]      (taps where the division is exact)
//           dw[ky][kx] = sum_{b,y,x} x[y][x] * dy[(y+p-ky)/S][(x+p-kx)/S]  -> per-workgroup partials, ordered final sum
//         stride 1 is the forward stencil with the flipped filter; stride 2 works on 2x2 input quads so that every
//         tap is used exactly once per quad with compile-time offsets.
//
// Strip walking (the stride-1 forward, the 3x3 stride-1 backward and the stride-2 backward): the unit of work is still the
// 1024-pixel tile TH x TW (TW in {64,32,16,8}), but a workgroup owns a RUN of vertically adjacent tiles ("blocks") of one
// column strip and walks it: the loads of block i+1 (the staged operand and, backward, x) are issued into registers
// before block i is computed, go to the other half of a double LDS buffer afterwards, and the K-1 halo rows two
// consecutive blocks share are copied LDS to LDS instead of being read again.  Rows are moved 16 bytes per lane where
// W % 4 == 0 (8 bytes per lane for the quads of stride 2), element by element otherwise.  The weight-gradient taps
// stay in registers over the whole run: one reduction and one partial per workgroup.  The two BatchNorm sums of the folded
// backward keep one partial per block, summed in the one-tile kernels' order (dw_bn_block_partial below).
// Every output element keeps its own fmaf chain (taps in ascending order from 0.f), so y, dx, da and with them dbn_weight,
// dbn_bias and dz are bit for bit what the one-tile kernels gave; only the grouping of the dw partial sums differs.
// No atomics anywhere: bitwise reproducible (MIOpen's naive backward is, too; its wrw GEMM path is not).
#include "act.hpp"
#include "common.hpp"

#include <stdint.h>

namespace cabinet {

constexpr int DW_T = 256;          // threads
constexpr int DW_OUT = 1024;       // outputs (fwd) / input pixels (bwd) per tile: TH x TW with TW in {64,32,16,8}
constexpr int DW_MIN_WG = 4096;    // a run grows only while the launch keeps this many workgroups (16 per CU: two rounds at 8 resident) ...
constexpr int DW_MIN_BLOCKS = 4;   // ... but is 4 blocks long wherever the plane has them: below that the prologue is not amortised

struct DwShape {
    int B, C, H, W, Ho, Wo;
};

static int dw_tile_w(int w) { return w > 32 ? 64 : w > 16 ? 32 : w > 8 ? 16 : 8; }

// the one-tile forward: stride 2 only (its strip form was not built; the stride-1 forward is dwconv_s1_strip_kernel)
template <int K, int S>
__global__ __launch_bounds__(DW_T) void dwconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wgt,
                                                           DwShape s, int TW, int tiles_x, int tiles_y, BnFold f,
                                                           float* __restrict__ y) {
    constexpr int PAD = K / 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int TH = DW_OUT / TW;
    const int tile = blockIdx.x % (tiles_x * tiles_y), plane = blockIdx.x / (tiles_x * tiles_y);
    const int c = plane % s.C;
    const int oy0 = (tile / tiles_x) * TH, ox0 = (tile % tiles_x) * TW;
    const int in_h = (TH - 1) * S + K, in_w = (TW - 1) * S + K;
    const int iy0 = oy0 * S - PAD, ix0 = ox0 * S - PAD;
    const float* xp = x + (size_t)plane * s.H * s.W;
    if (f.mean) {  // the input is act(bn(z)): evaluated while staging; the zero padding is that of the activated map
        const float mu = f.mean[c], inv = f.invstd[c], gam = f.weight[c], bet = f.bias[c];
        for (int i = threadIdx.x; i < in_h * in_w; i += DW_T) {
            const int r = i / in_w, q = i - r * in_w, iy = iy0 + r, ix = ix0 + q;
            smem[i] = (iy >= 0 && iy < s.H && ix >= 0 && ix < s.W)
                          ? act_fwd(fmaf((xp[(size_t)iy * s.W + ix] - mu) * inv, gam, bet), f.act)
                          : 0.f;
        }
    } else {
        for (int i = threadIdx.x; i < in_h * in_w; i += DW_T) {
            const int r = i / in_w, q = i - r * in_w, iy = iy0 + r, ix = ix0 + q;
            smem[i] = (iy >= 0 && iy < s.H && ix >= 0 && ix < s.W) ? xp[(size_t)iy * s.W + ix] : 0.f;
        }
    }
    float w[K][K];
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) w[ky][kx] = wgt[(c * K + ky) * K + kx];
    __syncthreads();
    const int tx = threadIdx.x & (TW - 1), tq = threadIdx.x / TW;  // 4 outputs: rows tq*4 .. tq*4+3, column tx
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* base = smem + (tq * 4 * S) * in_w + tx * S;
#pragma unroll
    for (int r = 0; r < 3 * S + K; ++r) {
        float v[K];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) v[kx] = base[r * in_w + kx];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ky = r - j * S;  // compile-time after unrolling
            if (ky >= 0 && ky < K) {
#pragma unroll
                for (int kx = 0; kx < K; ++kx) acc[j] = fmaf(w[ky][kx], v[kx], acc[j]);
            }
        }
    }
    float* yp = y + (size_t)plane * s.Ho * s.Wo;
    const int ox = ox0 + tx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = oy0 + tq * 4 + j;
        if (oy < s.Ho && ox < s.Wo) yp[(size_t)oy * s.Wo + ox] = acc[j];
    }
}

// ---- the one-tile stride-1 backward, kept for K = 5 (its strip form needs 156 VGPRs, 3 waves per SIMD, and lost on the 32 x 32 and
// 128 x 128 planes that are all its workload): dx and per-tile partials part[c][b*tiles + tile][K*K], one input-space tile ----
// workgroup reduction of the K*K per-thread partial sums (fixed order); red is [KK][DW_T + 8] (row of 32 padded to 33)
template <int KK>
__device__ __forceinline__ void dw_reduce_partials(const float (&pw)[KK], float* red, float* __restrict__ out) {
    constexpr int LD = DW_T + 8;
    const int slot = threadIdx.x + (threadIdx.x >> 5);
#pragma unroll
    for (int t = 0; t < KK; ++t) red[t * LD + slot] = pw[t];
    __syncthreads();
    if (threadIdx.x < KK * 8) {
        const int tap = threadIdx.x >> 3, seg = threadIdx.x & 7;
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) t += red[tap * LD + seg * 33 + i];
        t += __shfl_xor(t, 1, 64);
        t += __shfl_xor(t, 2, 64);
        t += __shfl_xor(t, 4, 64);
        if (seg == 0) out[tap] = t;
    }
}

// stride 1: with the flipped filter wf[a][b] = w[K-1-a][K-1-b] the input gradient is the SAME stencil as forward,
// applied to dy (pad K/2), and dw[K-1-a][K-1-b] = sum x[y][x] * dy[y-p+a][x-p+b]: one staged dy tile (+halo),
// a thread owns 4 vertically adjacent pixels, every LDS row it loads feeds up to K of them -- no masks.
template <int K>
__global__ __launch_bounds__(DW_T) void dwconv_bwd_s1_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              const float* __restrict__ wgt, DwShape s, int TW, int tiles_x,
                                                              int tiles_y, BnFold f, float* __restrict__ dx,
                                                              float* __restrict__ part, float* __restrict__ bnpart) {
    constexpr int PAD = K / 2, KK = K * K;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red4[4];
    const int TH = DW_OUT / TW;
    const int ntile = tiles_x * tiles_y;
    const int tile = blockIdx.x % ntile, plane = blockIdx.x / ntile;
    const int b = plane / s.C, c = plane - b * s.C;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int in_h = TH + K - 1, in_w = TW + K - 1;
    float* tile_dy = smem;               // [in_h][in_w]
    float* red = smem + in_h * in_w;     // [KK][DW_T + 8]
    const float* dyp = dy + (size_t)plane * s.H * s.W;  // stride 1: dy has the input's size
    for (int i = threadIdx.x; i < in_h * in_w; i += DW_T) {
        const int r = i / in_w, q = i - r * in_w, oy = y0 - PAD + r, ox = x0 - PAD + q;
        tile_dy[i] = (oy >= 0 && oy < s.H && ox >= 0 && ox < s.W) ? dyp[(size_t)oy * s.W + ox] : 0.f;
    }
    float wf[K][K];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int bb = 0; bb < K; ++bb) wf[a][bb] = wgt[(c * K + (K - 1 - a)) * K + (K - 1 - bb)];
    __syncthreads();
    const int tx = threadIdx.x & (TW - 1), tq = threadIdx.x / TW;
    const int xx = x0 + tx;
    const float* xp = x + (size_t)plane * s.H * s.W;
    float xv[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
    float xh[4], dact[4];  // folded BatchNorm: xhat and act'(u) of the thread's pixels
    float mu = 0.f, inv = 1.f, gam = 1.f, bet = 0.f;
    if (f.mean) mu = f.mean[c], inv = f.invstd[c], gam = f.weight[c], bet = f.bias[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = y0 + tq * 4 + j;
        const bool live = yy < s.H && xx < s.W;
        xv[j] = live ? xp[(size_t)yy * s.W + xx] : 0.f;
        xh[j] = 0.f, dact[j] = 0.f;
        if (f.mean) {
            xh[j] = (xv[j] - mu) * inv;
            const float u = fmaf(xh[j], gam, bet);
            xv[j] = live ? act_fwd(u, f.act) : 0.f;
            dact[j] = live ? act_grad(u, f.act) : 0.f;
        }
    }
    float pw[KK];
#pragma unroll
    for (int t = 0; t < KK; ++t) pw[t] = 0.f;
    const float* base = tile_dy + (tq * 4) * in_w + tx;
#pragma unroll
    for (int r = 0; r < 3 + K; ++r) {
        float v[K];
#pragma unroll
        for (int bb = 0; bb < K; ++bb) v[bb] = base[r * in_w + bb];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = r - j;  // compile-time after unrolling
            if (a >= 0 && a < K) {
#pragma unroll
                for (int bb = 0; bb < K; ++bb) {
                    acc[j] = fmaf(wf[a][bb], v[bb], acc[j]);
                    pw[(K - 1 - a) * K + (K - 1 - bb)] = fmaf(xv[j], v[bb], pw[(K - 1 - a) * K + (K - 1 - bb)]);
                }
            }
        }
    }
    float* dxp = dx + (size_t)plane * s.H * s.W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = y0 + tq * 4 + j;
        if (yy < s.H && xx < s.W) dxp[(size_t)yy * s.W + xx] = acc[j];
    }
    if (f.mean) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float du = acc[j] * dact[j];
            s1 += du, s2 = fmaf(du, xh[j], s2);
        }
        s1 = block_sum_256(s1, red4);
        s2 = block_sum_256(s2, red4);
        if (threadIdx.x == 0) {
            const int nt = s.B * ntile;
            bnpart[(size_t)c * nt + b * ntile + tile] = s1;
            bnpart[((size_t)s.C + c) * nt + b * ntile + tile] = s2;
        }
    }
    dw_reduce_partials<KK>(pw, red, part + ((size_t)c * (s.B * ntile) + (size_t)b * ntile + tile) * KK);
}

// ---- strip walking ----------------------------------------------------------------------------------------------------------
// Launch plan of a (hp, wp) plane (the input plane for the backward kernels, the output plane for the forward): `strips` column
// strips of `blocks` tiles each, cut into `runs` runs of `nb` blocks (the last run may be shorter); one workgroup per run.
struct DwPlan {
    int TW, TH, lgG, strips, blocks, nb, runs;  // lgG = log2(TW / 4): a thread owns 4 adjacent columns (stride 1)
};
static DwPlan dw_plan(int planes, int hp, int wp) {
    DwPlan p;
    p.TW = dw_tile_w(wp), p.TH = DW_OUT / p.TW;
    p.lgG = p.TW == 64 ? 4 : p.TW == 32 ? 3 : p.TW == 16 ? 2 : 1;
    p.strips = ceil_div(wp, p.TW), p.blocks = ceil_div(hp, p.TH);
    const long long tiles = (long long)planes * p.strips * p.blocks, want = tiles / DW_MIN_WG;
    p.nb = (int)(want > p.blocks ? p.blocks : want < DW_MIN_BLOCKS ? (p.blocks < DW_MIN_BLOCKS ? p.blocks : DW_MIN_BLOCKS) : want);
    p.runs = ceil_div(p.blocks, p.nb);
    p.nb = ceil_div(p.blocks, p.runs);  // even runs
    p.runs = ceil_div(p.blocks, p.nb);
    return p;
}

// the KK per-thread weight-gradient sums of a workgroup -> one partial each, fixed order: wave butterflies, then the four waves
// pairwise.  part: [C][nparts][KK]
template <int KK>
__device__ __forceinline__ void dw_strip_reduce(const float (&pw)[KK], float* red, int c, int nparts, int pi,
                                                float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < KK; ++t) {
        const float v = wave_sum(pw[t]);
        if (lane == 0) red[t * 4 + wv] = v;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < KK) part[((size_t)c * nparts + pi) * KK + t] = (red[t * 4] + red[t * 4 + 1]) + (red[t * 4 + 2] + red[t * 4 + 3]);
}

// The two BatchNorm sums of a folded backward keep the one-tile kernels' grouping, bit for bit: one partial per 1024-pixel block
// (bnpart: [2][C][B * strips * blocks], block (by, strip) of image b at b * ntile + by * strips + strip), per thread the chain over
// its four pixels, wave butterflies, the four waves pairwise -- dbn_weight and dbn_bias are C numbers that sit within one fp32
// rounding of fp64, where another grouping of the same terms is as often twice as far as half as far.  bred: 8 floats of LDS;
// the caller's barrier of the next block separates thread 0's reads from the next writes.
__device__ __forceinline__ void dw_bn_block_partial(float t1, float t2, float* bred, int c, int C, int nt, int idx,
                                                    float* __restrict__ bnpart) {
    t1 = wave_sum(t1), t2 = wave_sum(t2);
    if ((threadIdx.x & 63) == 0) bred[threadIdx.x >> 6] = t1, bred[4 + (threadIdx.x >> 6)] = t2;
    __syncthreads();
    if (threadIdx.x == 0) {
        bnpart[(size_t)c * nt + idx] = (bred[0] + bred[1]) + (bred[2] + bred[3]);
        bnpart[((size_t)C + c) * nt + idx] = (bred[4] + bred[5]) + (bred[6] + bred[7]);
    }
}

// With a folded BatchNorm (BnFold, act.hpp) the backward kernels also (i) rebuild their x operand a = act(bn(z)) from z
// and (ii) turn the input gradient da they produce into the BatchNorm-backward partial sums of their run,
// sum du and sum du * xhat with du = da * act'(u): the BatchNorm's own reduce pass over (da, z) disappears.

// stride 1, forward (BWD = false: src = x, dst = y, the BatchNorm folded into the staging) and backward (BWD = true: src = dy,
// dst = dx, xop = x or z).  With the flipped filter wf[a][b] = w[K-1-a][K-1-b] the input gradient is the SAME stencil as
// forward, applied to dy, and dw[K-1-a][K-1-b] = sum x[y][x] * dy[y-p+a][x-p+b].
// LDS: two buffers of (TH + K-1) rows x (TW + 8) floats; the strip's columns start at float 4 of a row (16-byte aligned), the
// left halo sits in floats 4-PAD..3, the right one behind the strip.  Buffer row 0 is row y0 - PAD of the staged plane.
// A thread owns pixels (y0 + r, x0 + 4 gc .. + 3): one 16-byte load of its staged row r + PAD and of x, one 16-byte store.
template <int K, bool BWD, bool VEC>
__global__ __launch_bounds__(DW_T) void dwconv_s1_strip_kernel(const float* __restrict__ src, const float* __restrict__ xop,
                                                                const float* __restrict__ wgt, DwShape s, DwPlan p, BnFold f,
                                                                float* __restrict__ dst, float* __restrict__ part,
                                                                float* __restrict__ bnpart) {
    constexpr int PAD = K / 2, KK = K * K, HR = K - 1, HC = 2 * PAD;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[KK * 4];
    __shared__ float bred[8];
    const int tid = threadIdx.x;
    const int TW = p.TW, TH = p.TH, LD = TW + 8, BUF = (TH + HR) * LD;
    const int wgpp = p.strips * p.runs;
    const int plane = blockIdx.x / wgpp, rem = blockIdx.x - plane * wgpp;
    const int run = rem / p.strips, strip = rem - run * p.strips;
    const int b = plane / s.C, c = plane - b * s.C;
    const int x0 = strip * TW, yb = run * p.nb * TH, nblk = min(p.nb, p.blocks - run * p.nb);
    const int H = s.H, W = s.W;  // stride 1: the output plane has the input's size
    const int gc = tid & ((TW >> 2) - 1), r = tid >> p.lgG, col = x0 + 4 * gc;
    const bool fold = f.mean != nullptr, sfold = !BWD && fold;
    float mu = 0.f, inv = 1.f, gam = 1.f, bet = 0.f;
    if (fold) mu = f.mean[c], inv = f.invstd[c], gam = f.weight[c], bet = f.bias[c];
    const float* sp = src + (size_t)plane * H * W;
    const float* xp = BWD ? xop + (size_t)plane * H * W : nullptr;
    float* dp = dst + (size_t)plane * H * W;

    // raw loads (0 outside the plane); the forward's fold is applied when a value goes to LDS, so that a prefetch does not wait
    auto raw1 = [&](int gy, int gx) -> float {
        return (gy >= 0 && gy < H && gx >= 0 && gx < W) ? sp[(size_t)gy * W + gx] : 0.f;
    };
    auto raw4 = [&](const float* __restrict__ base, int gy) -> f32x4 {  // gy >= 0
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            if (gy < H && col < W) v = *reinterpret_cast<const f32x4*>(base + (size_t)gy * W + col);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (gy < H && col + e < W) v[e] = base[(size_t)gy * W + col + e];
        }
        return v;
    };
    // staged value of the activated map: zero padding is that of act(bn(z))
    auto staged = [&](float v, bool live) -> float {
        return sfold ? (live ? act_fwd(fmaf((v - mu) * inv, gam, bet), f.act) : 0.f) : v;
    };
    // halo columns of the TH new rows of a block: TH * HC elements, at most two per thread
    int hrow[2], hl[2];
    bool hon[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int h = tid + k * DW_T;
        hon[k] = h < TH * HC;
        hrow[k] = h / HC;
        const int hc = h - hrow[k] * HC;
        hl[k] = hc < PAD ? 4 - PAD + hc : 4 + TW + hc - PAD;
    }

    // the K-1 rows in front of the first block, straight into buffer 0
    if (tid < TW + HC) {
#pragma unroll
        for (int j = 0; j < HR; ++j) {
            const int gy = yb - PAD + j, gx = x0 - PAD + tid;
            smem[j * LD + 4 - PAD + tid] = staged(raw1(gy, gx), gy >= 0 && gy < H && gx >= 0 && gx < W);
        }
    }
    f32x4 nv = raw4(sp, yb + r + PAD), nx = {0.f, 0.f, 0.f, 0.f};
    float nh[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) nh[k] = hon[k] ? raw1(yb + hrow[k] + PAD, x0 + hl[k] - 4) : 0.f;
    if (BWD) nx = raw4(xp, yb + r);

    float wf[K][K];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int bb = 0; bb < K; ++bb) wf[a][bb] = BWD ? wgt[(c * K + (K - 1 - a)) * K + (K - 1 - bb)] : wgt[(c * K + a) * K + bb];
    float pw[KK];
#pragma unroll
    for (int t = 0; t < KK; ++t) pw[t] = 0.f;

    for (int i = 0; i < nblk; ++i) {
        float* cur = smem + (i & 1) * BUF;
        float* nxt = smem + ((i & 1) ^ 1) * BUF;
        const int y0 = yb + i * TH;
        {   // block i's new rows: registers -> LDS
            const int gy = y0 + r + PAD;
            f32x4 v = nv;
            if (sfold) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = staged(v[e], gy < H && col + e < W);
            }
            *reinterpret_cast<f32x4*>(cur + (r + HR) * LD + 4 + 4 * gc) = v;
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (hon[k]) {
                    const int hy = y0 + hrow[k] + PAD, hx = x0 + hl[k] - 4;
                    cur[(hrow[k] + HR) * LD + hl[k]] = staged(nh[k], hy < H && hx >= 0 && hx < W);
                }
        }
        const f32x4 xc = nx;
        if (i + 1 < nblk) {  // block i+1's loads fly while block i is computed
            const int y1 = y0 + TH;
            nv = raw4(sp, y1 + r + PAD);
#pragma unroll
            for (int k = 0; k < 2; ++k) nh[k] = hon[k] ? raw1(y1 + hrow[k] + PAD, x0 + hl[k] - 4) : 0.f;
            if (BWD) nx = raw4(xp, y1 + r);
        }
        __syncthreads();
        const int yy = y0 + r;
        float xv[4], xh[4], dact[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xv[e] = xc[e], xh[e] = 0.f, dact[e] = 0.f;
            if (BWD && fold) {
                const bool live = yy < H && col + e < W;
                xh[e] = (xv[e] - mu) * inv;
                const float u = fmaf(xh[e], gam, bet);
                xv[e] = live ? act_fwd(u, f.act) : 0.f;
                dact[e] = live ? act_grad(u, f.act) : 0.f;
            }
        }
        const float* rowp = cur + r * LD + 4 * gc;
#pragma unroll
        for (int a = 0; a < K; ++a) {
            const f32x4 q0 = *reinterpret_cast<const f32x4*>(rowp + a * LD);
            const f32x4 q1 = *reinterpret_cast<const f32x4*>(rowp + a * LD + 4);
            const f32x4 q2 = *reinterpret_cast<const f32x4*>(rowp + a * LD + 8);
            const float v[12] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3], q2[0], q2[1], q2[2], q2[3]};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int bb = 0; bb < K; ++bb) {
                    const float d = v[4 - PAD + e + bb];
                    acc[e] = fmaf(wf[a][bb], d, acc[e]);
                    if (BWD) pw[(K - 1 - a) * K + (K - 1 - bb)] = fmaf(xv[e], d, pw[(K - 1 - a) * K + (K - 1 - bb)]);
                }
        }
        if (VEC) {
            if (yy < H && col < W) {
                const f32x4 o = {acc[0], acc[1], acc[2], acc[3]};
                *reinterpret_cast<f32x4*>(dp + (size_t)yy * W + col) = o;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (yy < H && col + e < W) dp[(size_t)yy * W + col + e] = acc[e];
        }
        if (BWD && fold) {  // the block's BatchNorm partial in the one-tile kernels' order: thread (tq, tx) sums rows 4 tq .. 4 tq + 3 of column tx
            float* D = smem + 2 * BUF;   // [TH][TW] du, then [TH][TW] xhat
            float* X = D + DW_OUT;
            const f32x4 dv = {acc[0] * dact[0], acc[1] * dact[1], acc[2] * dact[2], acc[3] * dact[3]};
            const f32x4 xq = {xh[0], xh[1], xh[2], xh[3]};
            *reinterpret_cast<f32x4*>(D + r * TW + 4 * gc) = dv;
            *reinterpret_cast<f32x4*>(X + r * TW + 4 * gc) = xq;
            __syncthreads();
            const int tx = tid & (TW - 1), tq = tid >> (p.lgG + 2);
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float du = D[(tq * 4 + j) * TW + tx];
                t1 += du, t2 = fmaf(du, X[(tq * 4 + j) * TW + tx], t2);
            }
            const int ntile = p.strips * p.blocks;
            dw_bn_block_partial(t1, t2, bred, c, s.C, s.B * ntile, b * ntile + (run * p.nb + i) * p.strips + strip, bnpart);
        }
        // the K-1 rows the next block shares with this one (its buffer was last read before this iteration's barrier)
        if (i + 1 < nblk && tid < TW + HC) {
#pragma unroll
            for (int j = 0; j < HR; ++j) nxt[j * LD + 4 - PAD + tid] = cur[(TH + j) * LD + 4 - PAD + tid];
        }
    }
    if (BWD) dw_strip_reduce<KK>(pw, red, c, s.B * wgpp, b * wgpp + rem, part);
}

// stride 2: a thread owns the 2x2 input quad (2n+py, 2m+px).  A tap (ky,kx) reaches pixel parity
// (py,px) = ((ky+p)&1, (kx+p)&1) only, from dy[n + (py+p-ky)/2][m + (px+p-kx)/2]: every tap is used exactly once per
// quad, all offsets are compile-time, and the <= 3x3 dy neighbourhood is read from LDS once.  x and dx move as one 8-byte
// pair per lane and row.  LDS: two buffers of (TH/2 + NO-1) x (TW/2 + NO-1) dy values, origin (n0 + OLO, m0 + OLO).
template <int K, bool VEC>
__global__ __launch_bounds__(DW_T) void dwconv_bwd_s2_strip_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                    const float* __restrict__ wgt, DwShape s, DwPlan p, BnFold f,
                                                                    float* __restrict__ dx, float* __restrict__ part,
                                                                    float* __restrict__ bnpart) {
    constexpr int PAD = K / 2, KK = K * K;
    // smallest / largest dy offset (py + PAD - ky) / 2 over the exact divisions: K=3 -> 0..1, K=5 -> -1..1
    constexpr int OLO = (K == 3) ? 0 : -1, OHI = 1, NO = OHI - OLO + 1, HR = NO - 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[KK * 4];
    __shared__ float bred[8];
    const int tid = threadIdx.x;
    const int TW = p.TW, TH = p.TH, TWm = TW >> 1, THn = TH >> 1, tw = TWm + HR, BUF = (THn + HR) * tw;
    const int wgpp = p.strips * p.runs;
    const int plane = blockIdx.x / wgpp, rem = blockIdx.x - plane * wgpp;
    const int run = rem / p.strips, strip = rem - run * p.strips;
    const int b = plane / s.C, c = plane - b * s.C;
    const int x0 = strip * TW, yb = run * p.nb * TH, nblk = min(p.nb, p.blocks - run * p.nb);  // even
    const int m0 = x0 >> 1, nb0 = yb >> 1;
    const int H = s.H, W = s.W, Ho = s.Ho, Wo = s.Wo;
    const int tm = tid & (TWm - 1), tn = tid >> (p.lgG + 1);
    const bool fold = f.mean != nullptr;
    float mu = 0.f, inv = 1.f, gam = 1.f, bet = 0.f;
    if (fold) mu = f.mean[c], inv = f.invstd[c], gam = f.weight[c], bet = f.bias[c];
    const float* dyp = dy + (size_t)plane * Ho * Wo;
    const float* xp = x + (size_t)plane * H * W;
    float* dxp = dx + (size_t)plane * H * W;
    auto ld = [&](int oy, int ox) -> float {
        return (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) ? dyp[(size_t)oy * Wo + ox] : 0.f;
    };
    auto ldx = [&](int yy) -> f32x2 {  // the quad's row yy: pixels x0 + 2 tm, + 1
        const int xx = x0 + 2 * tm;
        f32x2 v = {0.f, 0.f};
        if (VEC) {
            if (yy < H && xx < W) v = *reinterpret_cast<const f32x2*>(xp + (size_t)yy * W + xx);
        } else {
            if (yy < H && xx < W) v[0] = xp[(size_t)yy * W + xx];
            if (yy < H && xx + 1 < W) v[1] = xp[(size_t)yy * W + xx + 1];
        }
        return v;
    };
    // the NO-1 halo columns of the THn new rows of a block
    const bool hon = tid < THn * HR;
    const int hrow = tid / HR, hq = TWm + (tid - hrow * HR);

    if (tid < tw) {  // the NO-1 rows in front of the first block
#pragma unroll
        for (int j = 0; j < HR; ++j) smem[j * tw + tid] = ld(nb0 + OLO + j, m0 + OLO + tid);
    }
    float nv = ld(nb0 + OHI + tn, m0 + OLO + tm), nh = hon ? ld(nb0 + OHI + hrow, m0 + OLO + hq) : 0.f;
    f32x2 nx[2];
#pragma unroll
    for (int py = 0; py < 2; ++py) nx[py] = ldx(yb + 2 * tn + py);

    float w[K][K];
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) w[ky][kx] = wgt[(c * K + ky) * K + kx];
    float pw[KK];
#pragma unroll
    for (int t = 0; t < KK; ++t) pw[t] = 0.f;

    for (int i = 0; i < nblk; ++i) {
        float* cur = smem + (i & 1) * BUF;
        float* nxt = smem + ((i & 1) ^ 1) * BUF;
        const int y0 = yb + i * TH;
        cur[(tn + HR) * tw + tm] = nv;
        if (hon) cur[(hrow + HR) * tw + hq] = nh;
        const f32x2 xc[2] = {nx[0], nx[1]};
        if (i + 1 < nblk) {  // block i+1's loads fly while block i is computed
            const int n1 = nb0 + (i + 1) * THn;
            nv = ld(n1 + OHI + tn, m0 + OLO + tm);
            nh = hon ? ld(n1 + OHI + hrow, m0 + OLO + hq) : 0.f;
#pragma unroll
            for (int py = 0; py < 2; ++py) nx[py] = ldx(y0 + TH + 2 * tn + py);
        }
        __syncthreads();
        float g[NO][NO], t1 = 0.f, t2 = 0.f;  // t1, t2: the block's BatchNorm sums of this thread, the one-tile kernel's chain
#pragma unroll
        for (int a = 0; a < NO; ++a)
#pragma unroll
            for (int bb = 0; bb < NO; ++bb) g[a][bb] = cur[(tn + a) * tw + tm + bb];
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            const int yy = y0 + 2 * tn + py;
            float xv[2], xh[2] = {0.f, 0.f}, dact[2] = {0.f, 0.f}, acc[2] = {0.f, 0.f};
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                const int xx = x0 + 2 * tm + px;
                const bool live = yy < H && xx < W;
                xv[px] = xc[py][px];
                if (fold) {
                    xh[px] = (xv[px] - mu) * inv;
                    const float u = fmaf(xh[px], gam, bet);
                    xv[px] = live ? act_fwd(u, f.act) : 0.f;
                    dact[px] = live ? act_grad(u, f.act) : 0.f;
                }
            }
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                if (((py + PAD - ky) & 1) != 0) continue;           // compile-time
                const int a = (py + PAD - ky) / 2 - OLO;            // row of g
#pragma unroll
                for (int px = 0; px < 2; ++px)
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        if (((px + PAD - kx) & 1) != 0) continue;
                        const int bb = (px + PAD - kx) / 2 - OLO;
                        acc[px] = fmaf(w[ky][kx], g[a][bb], acc[px]);
                        pw[ky * K + kx] = fmaf(xv[px], g[a][bb], pw[ky * K + kx]);
                    }
            }
            const int xx = x0 + 2 * tm;
            if (VEC) {
                if (yy < H && xx < W) {
                    const f32x2 o = {acc[0], acc[1]};
                    *reinterpret_cast<f32x2*>(dxp + (size_t)yy * W + xx) = o;
                }
            } else {
                if (yy < H && xx < W) dxp[(size_t)yy * W + xx] = acc[0];
                if (yy < H && xx + 1 < W) dxp[(size_t)yy * W + xx + 1] = acc[1];
            }
#pragma unroll
            for (int px = 0; px < 2 && fold; ++px) {
                const float du = acc[px] * dact[px];
                t1 += du, t2 = fmaf(du, xh[px], t2);
            }
        }
        if (fold) {
            const int ntile = p.strips * p.blocks;
            dw_bn_block_partial(t1, t2, bred, c, s.C, s.B * ntile, b * ntile + (run * p.nb + i) * p.strips + strip, bnpart);
        }
        if (i + 1 < nblk && tid < tw) {  // the NO-1 rows the next block shares with this one
#pragma unroll
            for (int j = 0; j < HR; ++j) nxt[j * tw + tid] = cur[(THn + j) * tw + tid];
        }
    }
    dw_strip_reduce<KK>(pw, red, c, s.B * wgpp, b * wgpp + rem, part);
}

// dw[c][tap] = sum over the nparts partials (double accumulation, fixed order)
__global__ __launch_bounds__(256) void dwconv_dw_finalize_kernel(const float* __restrict__ part, int nparts, int KK,
                                                                  float* __restrict__ dw) {
    __shared__ double dred[4];
    const int c = blockIdx.x / KK, tap = blockIdx.x - c * KK;
    double t = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) t += (double)part[((size_t)c * nparts + i) * KK + tap];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) dw[blockIdx.x] = (float)((dred[0] + dred[1]) + (dred[2] + dred[3]));
}

bool dwconv_supported(int K, int S) { return (K == 3 || K == 5) && (S == 1 || S == 2); }

static void out_size(int H, int W, int K, int S, int& Ho, int& Wo) {
    Ho = (H + 2 * (K / 2) - K) / S + 1;
    Wo = (W + 2 * (K / 2) - K) / S + 1;
}

// The workspace areas are sized for one partial per 1024-pixel tile; the strip kernels write a prefix of them.
size_t dwconv_bwd_workspace(int B, int C, int H, int W, int K) {
    const int TW = dw_tile_w(W), TH = DW_OUT / TW;
    return align_up((size_t)C * B * ceil_div(W, TW) * ceil_div(H, TH) * K * K * sizeof(float), 256);
}

static int bwd_tiles(int H, int W) {
    const int TW = dw_tile_w(W), TH = DW_OUT / TW;
    return ceil_div(W, TW) * ceil_div(H, TH);
}

static bool dw_aligned(const void* a, const void* b, const void* c, uintptr_t mask) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & mask) == 0;
}

template <int K, int S>
static hipError_t fwd_launch(const float* x, const float* w, const DwShape& s, const BnFold& f, float* y,
                             hipStream_t stream) {
    if constexpr (S == 1) {
        const DwPlan p = dw_plan(s.B * s.C, s.Ho, s.Wo);
        const size_t lds = (size_t)2 * (p.TH + K - 1) * (p.TW + 8) * sizeof(float);
        const dim3 grid((unsigned)((size_t)s.B * s.C * p.strips * p.runs));
        if ((s.W & 3) == 0 && dw_aligned(x, y, nullptr, 15))
            hipLaunchKernelGGL((dwconv_s1_strip_kernel<K, false, true>), grid, dim3(DW_T), lds, stream, x, nullptr, w, s, p, f, y,
                               nullptr, nullptr);
        else
            hipLaunchKernelGGL((dwconv_s1_strip_kernel<K, false, false>), grid, dim3(DW_T), lds, stream, x, nullptr, w, s, p, f, y,
                               nullptr, nullptr);
    } else {
        const int TW = dw_tile_w(s.Wo), TH = DW_OUT / TW;
        const int tiles_x = ceil_div(s.Wo, TW), tiles_y = ceil_div(s.Ho, TH);
        const size_t lds = (size_t)((TH - 1) * S + K) * ((TW - 1) * S + K) * sizeof(float);
        hipLaunchKernelGGL((dwconv_fwd_kernel<K, S>), dim3((unsigned)((size_t)s.B * s.C * tiles_x * tiles_y)), dim3(DW_T), lds,
                           stream, x, w, s, TW, tiles_x, tiles_y, f, y);
    }
    return hipGetLastError();
}

// part holds one weight-gradient partial per workgroup (never more than B * bwd_tiles(H, W): a prefix of its area), bnpart one
// BatchNorm partial per 1024-pixel tile, B * bwd_tiles(H, W) of them, for every kernel
template <int K, int S>
static hipError_t bwd_launch(const float* dy, const float* x, const float* w, const DwShape& s, const BnFold& f,
                             float* dx, float* dw, float* part, float* bnpart, hipStream_t stream) {
    int nparts;
    if constexpr (K == 5 && S == 1) {  // one tile per workgroup, one partial per tile
        const int TW = dw_tile_w(s.W), TH = DW_OUT / TW;
        const int tiles_x = ceil_div(s.W, TW), tiles_y = ceil_div(s.H, TH);
        const size_t lds = ((size_t)(TH + K - 1) * (TW + K - 1) + (size_t)K * K * (DW_T + 8)) * sizeof(float);
        hipLaunchKernelGGL((dwconv_bwd_s1_kernel<K>), dim3((unsigned)((size_t)s.B * s.C * tiles_x * tiles_y)), dim3(DW_T), lds,
                           stream, dy, x, w, s, TW, tiles_x, tiles_y, f, dx, part, bnpart);
        nparts = s.B * tiles_x * tiles_y;
    } else {
        const DwPlan p = dw_plan(s.B * s.C, s.H, s.W);
        const int wgpp = p.strips * p.runs;
        if (p.nb < 1 || wgpp > bwd_tiles(s.H, s.W)) return hipErrorInvalidValue;  // a run covers at least one tile: a prefix of the areas
        const dim3 grid((unsigned)((size_t)s.B * s.C * wgpp));
        if constexpr (S == 1) {
            const size_t lds = ((size_t)2 * (p.TH + K - 1) * (p.TW + 8) + 2 * DW_OUT) * sizeof(float);  // + du, xhat of a block
            if ((s.W & 3) == 0 && dw_aligned(dy, x, dx, 15))
                hipLaunchKernelGGL((dwconv_s1_strip_kernel<K, true, true>), grid, dim3(DW_T), lds, stream, dy, x, w, s, p, f, dx,
                                   part, bnpart);
            else
                hipLaunchKernelGGL((dwconv_s1_strip_kernel<K, true, false>), grid, dim3(DW_T), lds, stream, dy, x, w, s, p, f, dx,
                                   part, bnpart);
        } else {
            const size_t lds = (size_t)2 * (p.TH / 2 + 2) * (p.TW / 2 + 2) * sizeof(float);
            if ((s.W & 1) == 0 && dw_aligned(x, dx, nullptr, 7))
                hipLaunchKernelGGL((dwconv_bwd_s2_strip_kernel<K, true>), grid, dim3(DW_T), lds, stream, dy, x, w, s, p, f, dx, part,
                                   bnpart);
            else
                hipLaunchKernelGGL((dwconv_bwd_s2_strip_kernel<K, false>), grid, dim3(DW_T), lds, stream, dy, x, w, s, p, f, dx,
                                   part, bnpart);
        }
        nparts = s.B * wgpp;
    }
    hipLaunchKernelGGL(dwconv_dw_finalize_kernel, dim3(s.C * K * K), dim3(256), 0, stream, part, nparts, K * K, dw);
    return hipGetLastError();
}

static hipError_t fwd_dispatch(const float* x, const float* w, const DwShape& s, int K, int S, const BnFold& f, float* y,
                               hipStream_t stream) {
    if (K == 3 && S == 1) return fwd_launch<3, 1>(x, w, s, f, y, stream);
    if (K == 3 && S == 2) return fwd_launch<3, 2>(x, w, s, f, y, stream);
    if (K == 5 && S == 1) return fwd_launch<5, 1>(x, w, s, f, y, stream);
    return fwd_launch<5, 2>(x, w, s, f, y, stream);
}

static hipError_t bwd_dispatch(const float* dy, const float* x, const float* w, const DwShape& s, int K, int S,
                               const BnFold& f, float* dx, float* dw, float* part, float* bnpart, hipStream_t stream) {
    if (K == 3 && S == 1) return bwd_launch<3, 1>(dy, x, w, s, f, dx, dw, part, bnpart, stream);
    if (K == 3 && S == 2) return bwd_launch<3, 2>(dy, x, w, s, f, dx, dw, part, bnpart, stream);
    if (K == 5 && S == 1) return bwd_launch<5, 1>(dy, x, w, s, f, dx, dw, part, bnpart, stream);
    return bwd_launch<5, 2>(dy, x, w, s, f, dx, dw, part, bnpart, stream);
}

hipError_t dwconv_fwd_run(const float* x, const float* w, int B, int C, int H, int W, int K, int S, float* y,
                          hipStream_t stream) {
    DwShape s{B, C, H, W, 0, 0};
    out_size(H, W, K, S, s.Ho, s.Wo);
    return fwd_dispatch(x, w, s, K, S, BnFold{nullptr, nullptr, nullptr, nullptr, 0}, y, stream);
}

hipError_t dwconv_bwd_run(const float* dy, const float* x, const float* w, int B, int C, int H, int W, int K, int S,
                          float* dx, float* dw, void* ws, hipStream_t stream) {
    DwShape s{B, C, H, W, 0, 0};
    out_size(H, W, K, S, s.Ho, s.Wo);
    return bwd_dispatch(dy, x, w, s, K, S, BnFold{nullptr, nullptr, nullptr, nullptr, 0}, dx, dw, static_cast<float*>(ws),
                        nullptr, stream);
}

// ---- BatchNorm2d (+activation) -> depthwise convolution as one operator (reference mobilenetv3.py:135-143:
// `BatchNorm2d(hidden), act, depthwise Conv2d`): the normalised, activated tensor is never written or re-read.
//   fwd : BN statistics of z (one read), then the convolution reads z again and normalises while staging
//   bwd : the convolution's backward rebuilds a = act(bn(z)) from z, writes da and the BN-backward partial sums;
//         the BN-backward dx pass (da, z -> dz) finishes.  6 passes over the (B,C,H,W) tensor instead of 10.
struct BnDwWs {
    size_t bn, part, bnpart, coef, da, total;
};
static BnDwWs bn_dw_layout(int B, int C, int H, int W, int K) {
    BnDwWs w{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += align_up(bytes, 256);
        return o;
    };
    const int nt = B * bwd_tiles(H, W);
    w.bn = take(bn_act_workspace(B, C, H * W));
    w.part = take((size_t)C * nt * K * K * sizeof(float));
    w.bnpart = take((size_t)2 * C * nt * sizeof(float));
    w.coef = take((size_t)2 * C * sizeof(float));
    w.da = take((size_t)B * C * H * W * sizeof(float));
    w.total = off;
    return w;
}
size_t bn_dwconv_fwd_workspace(int B, int C, int H, int W) { return bn_act_workspace(B, C, H * W); }
size_t bn_dwconv_bwd_workspace(int B, int C, int H, int W, int K) { return bn_dw_layout(B, C, H, W, K).total; }

hipError_t bn_dwconv_fwd_run(const float* z, const float* bn_w, const float* bn_b, float* run_mean, float* run_var,
                             const float* w, int B, int C, int H, int W, int K, int S, int act, int training,
                             float momentum, float eps, float* y, float* save_mean, float* save_invstd, void* ws,
                             hipStream_t stream) {
    hipError_t e = bn_stats_run(z, run_mean, run_var, B, C, H * W, training, momentum, eps, save_mean, save_invstd, ws,
                                stream);
    if (e != hipSuccess) return e;
    DwShape s{B, C, H, W, 0, 0};
    out_size(H, W, K, S, s.Ho, s.Wo);
    return fwd_dispatch(z, w, s, K, S, BnFold{save_mean, save_invstd, bn_w, bn_b, act}, y, stream);
}

hipError_t bn_dwconv_bwd_run(const float* dy, const float* z, const float* bn_w, const float* bn_b,
                             const float* save_mean, const float* save_invstd, const float* w, int B, int C, int H,
                             int W, int K, int S, int act, int training, float* dz, float* dbn_w, float* dbn_b,
                             float* dw, void* ws, hipStream_t stream) {
    const BnDwWs L = bn_dw_layout(B, C, H, W, K);
    char* base = static_cast<char*>(ws);
    auto at = [&](size_t o) { return reinterpret_cast<float*>(base + o); };
    DwShape s{B, C, H, W, 0, 0};
    out_size(H, W, K, S, s.Ho, s.Wo);
    hipError_t e = bwd_dispatch(dy, z, w, s, K, S, BnFold{save_mean, save_invstd, bn_w, bn_b, act}, at(L.da), dw,
                                at(L.part), at(L.bnpart), stream);
    if (e != hipSuccess) return e;
    return bn_bwd_tail_run(at(L.bnpart), B * bwd_tiles(H, W), at(L.da), z, bn_w, bn_b, save_mean, save_invstd, B, C, H * W, act,
                           training, dz, dbn_w, dbn_b, at(L.coef), stream);
}

// ---- thin 1x1 convolution -> BatchNorm (+activation) -> depthwise convolution, backward: what bn_dwconv_bwd_run runs up to the
// BatchNorm partials, the stand-alone finalize on them, then K10's BN-form kernel with g = da -- the BatchNorm's dz (its dx pass)
// and the 1x1 convolution's two backward kernels that read it are one walk (pwconv_wide.hip).
size_t pw_bn_dwconv_bwd_workspace(int B, int Ci, int C, int H, int W, int K) {
    return bn_dw_layout(B, C, H, W, K).total + pw_bn_bwd_slab_bytes(B, Ci, C, H * W);
}

hipError_t pw_bn_dwconv_bwd_run(const float* dy, const float* z, const float* x, const float* pw_w, const float* bn_w,
                                const float* bn_b, const float* save_mean, const float* save_invstd, const float* w, int B, int Ci,
                                int C, int H, int W, int K, int S, int act, int training, float* dx, float* dpw_w, float* dbn_w,
                                float* dbn_b, float* dw, void* ws, hipStream_t stream) {
    const BnDwWs L = bn_dw_layout(B, C, H, W, K);
    char* base = static_cast<char*>(ws);
    auto at = [&](size_t o) { return reinterpret_cast<float*>(base + o); };
    DwShape s{B, C, H, W, 0, 0};
    out_size(H, W, K, S, s.Ho, s.Wo);
    hipError_t e = bwd_dispatch(dy, z, w, s, K, S, BnFold{save_mean, save_invstd, bn_w, bn_b, act}, at(L.da), dw, at(L.part),
                                at(L.bnpart), stream);
    if (e != hipSuccess) return e;
    e = bn_bwd_finalize_run(at(L.bnpart), B * bwd_tiles(H, W), C, (double)B * (double)(H * W), training, dbn_w, dbn_b, at(L.coef),
                            stream);
    if (e != hipSuccess) return e;
    return pw_bn_bwd_run(at(L.da), z, x, pw_w, save_mean, save_invstd, bn_w, bn_b, at(L.coef), B, Ci, C, H * W, act, dx, dpw_w,
                         base + L.total, stream);
}

}  // namespace cabinet
