// BatchNorm finalize shared by K7 (bn_act.hip) and K12 (bn_cls.hip): one 256-thread workgroup per channel merges per-chunk (mean, M2)
// partials with Chan's formula in double, in a fixed order, and updates the running buffers exactly like nn.BatchNorm2d.
#pragma once
#include "common.hpp"

namespace cabinet {

constexpr int BA_T = 256;
constexpr int BA_V = 8;                     // float4 per thread and chunk
constexpr int BA_CHUNK = BA_T * 4 * BA_V;   // 8192 elements

// part[0][c][tile] = chunk mean, part[1][c][tile] = chunk M2 (sum of squared deviations), tile = b * chunks + chunk
// conv_h > 0: the partials come from the epilogue of the 3x3 convolution that produced x (conv3x3_wino.hip: one (mean, M2) pair per
// channel and tile block of 4 x 32 output pixels, blocks ordered image, block row, block column) instead of bn_act_stats_kernel.
// Call from all BA_T threads of the block: every thread gets the channel's (mean, invstd) (eval mode: from the running buffers).
// A block merges for itself alone -- the result depends on `part` and the fixed order only, so the stand-alone finalize kernel
// and the prologue of a consumer kernel (any number of blocks per channel) arrive at the same bits.  Thread 0 of a `writer`
// block stores save_mean[c] / save_invstd[c] and updates the running buffers, which nobody else reads or writes in that launch:
// exactly one block per channel may be the writer.
struct BnStat {
    float mean, invstd;
};
// number of partials per channel (nt) for the two producers above
__host__ __device__ __forceinline__ int bn_fwd_nt(int B, int chunks, int conv_h, int conv_w) {
    return B * (conv_h > 0 ? ((conv_h + 3) / 4) * ((conv_w + 31) / 32) : chunks);
}
// The first trip of a merge's loops over [2][C][nt] partials: the pair thread t owns.  A consumer kernel requests it in FRONT of
// its activation loads: vector loads retire in order, so a partial requested behind them is waited for behind them, and the merge
// would start only when the whole chunk has landed instead of running underneath it.  nt == 0: nothing to load.
struct BnPart {
    float a, b;
};
__device__ __forceinline__ BnPart bn_part_first(const float* __restrict__ part, int c, int C, int nt) {
    BnPart p{0.f, 0.f};
    if ((int)threadIdx.x < nt) p.a = part[(size_t)c * nt + threadIdx.x], p.b = part[((size_t)C + c) * nt + threadIdx.x];
    return p;
}
// Placed behind the caller's activation loads: the first use of the pair (and with it the wait for its two loads) stays
// behind them instead of being hoisted in front, where it would hold the activation loads back by one L2 round trip.
__device__ __forceinline__ void bn_part_pin(BnPart& p) { asm volatile("" : "+v"(p.a), "+v"(p.b)); }
__device__ __forceinline__ BnStat bn_finalize_channel(const float* __restrict__ part, int c, int B, int C, int P, int chunks, int conv_h,
                                                      int conv_w, int training, float momentum, float eps,
                                                      float* __restrict__ running_mean, float* __restrict__ running_var,
                                                      float* __restrict__ save_mean, float* __restrict__ save_invstd, BnPart first,
                                                      bool writer) {
    __shared__ double dred[4];
    if (!training) {
        const BnStat r{running_mean[c], 1.0f / sqrtf(running_var[c] + eps)};
        if (writer && threadIdx.x == 0) {
            save_mean[c] = r.mean;
            save_invstd[c] = r.invstd;
        }
        return r;
    }
    const int nbx = conv_h > 0 ? (conv_w + 31) / 32 : 1, nbi = conv_h > 0 ? ((conv_h + 3) / 4) * nbx : chunks;
    const int nt = B * nbi, t0 = threadIdx.x;   // `first` = bn_part_first(part, c, C, nt)
    const float* pm = part + (size_t)c * nt;
    const float* p2 = part + ((size_t)C + c) * nt;
    auto block_sum_d = [&](double v) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = v;
        __syncthreads();
        const double t = (dred[0] + dred[1]) + (dred[2] + dred[3]);
        __syncthreads();
        return t;
    };
    auto count_of = [&](int t) {
        const int r = t % nbi;
        if (conv_h > 0) return (double)(min(4, conv_h - 4 * (r / nbx)) * min(32, conv_w - 32 * (r % nbx)));
        return (double)(min((r + 1) * BA_CHUNK, P) - r * BA_CHUNK);
    };
    const double N = (double)B * (double)P;
    double s = 0.0;
    if (t0 < nt) {
        s += count_of(t0) * (double)first.a;
        for (int t = t0 + BA_T; t < nt; t += BA_T) s += count_of(t) * (double)pm[t];
    }
    const double mean = block_sum_d(s) / N;
    double m2 = 0.0;
    if (t0 < nt) {
        const double d0 = (double)first.a - mean;
        m2 += (double)first.b + count_of(t0) * d0 * d0;
        for (int t = t0 + BA_T; t < nt; t += BA_T) {
            const double d = (double)pm[t] - mean;
            m2 += (double)p2[t] + count_of(t) * d * d;
        }
    }
    m2 = block_sum_d(m2);
    const double var = m2 / N;
    const BnStat r{(float)mean, (float)(1.0 / sqrt(var + (double)eps))};
    if (writer && threadIdx.x == 0) {
        save_mean[c] = r.mean;
        save_invstd[c] = r.invstd;
        const double unbiased = N > 1.0 ? m2 / (N - 1.0) : var;
        running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * mean);
        running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unbiased);
    }
    return r;
}

// The finalize as the prologue of the kernel that needs its result: every workgroup of the consumer merges its channel's
// partials itself (bn_finalize_channel: same code, same order, same bits as the stand-alone finalize kernel), and the launch of
// C small workgroups between the statistics pass and the consumer disappears.  Nothing one workgroup writes is read by another
// one of the same launch: ONE workgroup per channel (the consumer's first of image 0) is the writer of save_mean /
// save_invstd / the running buffers, and only it reads the running buffers (training mode).
struct BnFwdMerge {
    int on;             // 0: save_mean / save_invstd are finished values (the stand-alone finalize ran in front)
    const float* part;  // [2][C][nt] (mean, M2) partials, as bn_finalize_channel takes them
    int B, conv_h, conv_w, training;
    float momentum, eps;
    float *running_mean, *running_var, *save_mean, *save_invstd;
};
__device__ __forceinline__ BnPart bn_part_first(const BnFwdMerge& m, int c, int C, int chunks) {
    return bn_part_first(m.part, c, C, m.on && m.training ? bn_fwd_nt(m.B, chunks, m.conv_h, m.conv_w) : 0);
}
// the consumer's (mean, invstd) of channel c; `first` = bn_part_first(m, c, C, chunks).  Call from all BA_T threads.
__device__ __forceinline__ BnStat bn_consumer_stat(const BnFwdMerge& m, int c, int C, int P, int chunks, BnPart first, bool writer) {
    if (!m.on) return BnStat{m.save_mean[c], m.save_invstd[c]};
    return bn_finalize_channel(m.part, c, m.B, C, P, chunks, m.conv_h, m.conv_w, m.training, m.momentum, m.eps, m.running_mean,
                               m.running_var, m.save_mean, m.save_invstd, first, writer);
}

}  // namespace cabinet
