// K7 -- BatchNorm2d fused with the activation that follows it, forward and backward (NCHW fp32).
//
// Replaces the `bn -> relu` tail of reference ConvBNReLU.forward (src/models/cabinet.py:42-44; SURVEY.md section 8
// row a6 lists ConvBNReLU with the FFM) and the same BatchNorm2d -> ReLU / HardSwish pairs elsewhere in the model
// (cabinet.py:59-63,67-68; mobilenetv3.py:86-99,118-152 with HardSwish of mobilenetv3.py:53-65).  On stock
// PyTorch-ROCm each pair is a MIOpen batch-norm launch plus one (ReLU) to four (HardSwish = add, clamp, div, mul)
// elementwise launches, each a full HBM round trip, and the mirror image in backward; at config 3 the model
// normalises 4.0 GB of activations per step and these launches are ~30 % of the step.
//
// This is HBM-bound streaming work; the plan is the minimum number of passes a training-mode BatchNorm allows:
//   fwd  : stats  (read x)            per-chunk (mean, M2), merged per channel with Chan's formula in double
//          apply  (read x, write y)   y = act(gamma * xhat + beta)
//   bwd  : reduce (read dy, x)        sum du, sum du*xhat with du = dy * act'(u), u recomputed from x
//          dx     (read dy, x, write) dx = gamma*invstd*(du - mean(du) - xhat*mean(du*xhat))
// Nothing but x, mean and invstd is kept for backward (no pre-activation or mask tensor).  One workgroup streams
// one 8192-element chunk of one (b,c) plane with 128-bit loads; partial results are combined in a fixed order
// (no atomics): bitwise reproducible.
#include "act.hpp"
#include "bn_finalize.hpp"
#include "common.hpp"

namespace cabinet {


// chunk of a plane -> registers (zeros past the end); returns the number of valid elements of the chunk
__device__ __forceinline__ int ba_load(const float* __restrict__ row, int P, int lo, f32x4 (&v)[BA_V]) {
    const int hi = min(lo + BA_CHUNK, P);
    if ((P & 3) == 0) {
#pragma unroll
        for (int i = 0; i < BA_V; ++i) {
            const int p = lo + (i * BA_T + threadIdx.x) * 4;
            v[i] = p < hi ? *reinterpret_cast<const f32x4*>(row + p) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    } else {
#pragma unroll
        for (int i = 0; i < BA_V; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = lo + (i * BA_T + threadIdx.x) * 4 + e;
                v[i][e] = p < hi ? row[p] : 0.f;
            }
    }
    return hi - lo;
}
__device__ __forceinline__ bool ba_valid(int P, int lo, int i, int e) {
    return lo + (i * BA_T + (int)threadIdx.x) * 4 + e < min(lo + BA_CHUNK, P);
}
// The chunk load of the element-wise kernels that merge statistics in their prologue (apply, dx).  AL (P % 4 == 0): no branch
// around a load -- one past the end of the chunk reads the plane's last four elements instead, and what is computed from them is
// never stored (ba_store).  Behind a branch per load the compiler waits for everything requested earlier (the prologue's
// partials) before the first load and drains each block of loads before the next, and the merge could not run underneath them.
template <bool AL>
__device__ __forceinline__ void ba_request(const float* __restrict__ row, int P, int lo, f32x4 (&v)[BA_V]) {
    if (AL) {
#pragma unroll
        for (int i = 0; i < BA_V; ++i)
            v[i] = *reinterpret_cast<const f32x4*>(row + min(lo + (i * BA_T + (int)threadIdx.x) * 4, P - 4));
    } else {
        ba_load(row, P, lo, v);
    }
}
__device__ __forceinline__ void ba_store(float* __restrict__ row, int P, int lo, const f32x4 (&v)[BA_V]) {
    const int hi = min(lo + BA_CHUNK, P);
    if ((P & 3) == 0) {
#pragma unroll
        for (int i = 0; i < BA_V; ++i) {
            const int p = lo + (i * BA_T + threadIdx.x) * 4;
            if (p < hi) *reinterpret_cast<f32x4*>(row + p) = v[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < BA_V; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = lo + (i * BA_T + threadIdx.x) * 4 + e;
                if (p < hi) row[p] = v[i][e];
            }
    }
}

// part[0][c][tile] = chunk mean, part[1][c][tile] = chunk M2 (sum of squared deviations), tile = b*chunks + chunk
__global__ __launch_bounds__(BA_T) void bn_act_stats_kernel(const float* __restrict__ x, float* __restrict__ part, int B,
                                                             int C, int P, int chunks) {
    __shared__ float red[4];
    const int row = blockIdx.x / chunks, ch = blockIdx.x - row * chunks, b = row / C, c = row - b * C;
    f32x4 v[BA_V];
    const int cnt = ba_load(x + (size_t)row * P, P, ch * BA_CHUNK, v);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < BA_V; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    const float mean = block_sum_256(s, red) / (float)cnt;
    float m2 = 0.f;
#pragma unroll
    for (int i = 0; i < BA_V; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (ba_valid(P, ch * BA_CHUNK, i, e)) m2 += (v[i][e] - mean) * (v[i][e] - mean);
    m2 = block_sum_256(m2, red);
    if (threadIdx.x == 0) {
        const int nt = B * chunks, tile = b * chunks + ch;
        part[(size_t)c * nt + tile] = mean;
        part[((size_t)C + c) * nt + tile] = m2;
    }
}

// one workgroup per channel: merge the chunk statistics (Chan et al.), update the running buffers (bn_finalize.hpp: shared with K12)
__global__ __launch_bounds__(BA_T) void bn_act_finalize_kernel(const float* __restrict__ part, int B, int C, int P,
                                                                int chunks, int conv_h, int conv_w, int training, float momentum, float eps,
                                                                float* __restrict__ running_mean,
                                                                float* __restrict__ running_var,
                                                                float* __restrict__ save_mean,
                                                                float* __restrict__ save_invstd) {
    const BnPart first = bn_part_first(part, blockIdx.x, C, training ? bn_fwd_nt(B, chunks, conv_h, conv_w) : 0);
    bn_finalize_channel(part, blockIdx.x, B, C, P, chunks, conv_h, conv_w, training, momentum, eps, running_mean, running_var, save_mean,
                        save_invstd, first, true);
}

// m.on: the finalize runs here (BnFwdMerge, bn_finalize.hpp), underneath the workgroup's own activation loads; the writer is the
// workgroup of image 0, chunk 0 of the channel
template <bool AL>   // AL: P % 4 == 0, the host's choice
__global__ __launch_bounds__(BA_T) void bn_act_apply_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ weight,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ residual, int C, int P,
                                                             int chunks, int act, float* __restrict__ y, BnFwdMerge m) {
    const int row = blockIdx.x / chunks, ch = blockIdx.x - row * chunks, c = row % C;
    const float gam = weight[c], bet = bias[c];
    BnPart first = bn_part_first(m, c, C, chunks);
    f32x4 v[BA_V], r[BA_V];
    ba_request<AL>(x + (size_t)row * P, P, ch * BA_CHUNK, v);
    if (residual) ba_request<AL>(residual + (size_t)row * P, P, ch * BA_CHUNK, r);
    bn_part_pin(first);
    const BnStat st = bn_consumer_stat(m, c, C, P, chunks, first, row < C && ch == 0);
    const float mu = st.mean, inv = st.invstd;
#pragma unroll
    for (int i = 0; i < BA_V; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] = act_fwd(fmaf((v[i][e] - mu) * inv, gam, bet), act);
    if (residual) {  // the identity shortcut of an MBConv block (mobilenetv3.py:158), added in the same pass
#pragma unroll
        for (int i = 0; i < BA_V; ++i) v[i] += r[i];
    }
    ba_store(y + (size_t)row * P, P, ch * BA_CHUNK, v);
}

// part[0][c][tile] = sum du, part[1][c][tile] = sum du * xhat
__global__ __launch_bounds__(BA_T) void bn_act_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd,
                                                                  const float* __restrict__ weight,
                                                                  const float* __restrict__ bias, int B, int C, int P,
                                                                  int chunks, int act, float* __restrict__ part) {
    __shared__ float red[4];
    const int row = blockIdx.x / chunks, ch = blockIdx.x - row * chunks, b = row / C, c = row - b * C;
    const float mu = mean[c], inv = invstd[c], gam = weight[c], bet = bias[c];
    f32x4 vx[BA_V], vg[BA_V];
    ba_load(x + (size_t)row * P, P, ch * BA_CHUNK, vx);
    ba_load(dy + (size_t)row * P, P, ch * BA_CHUNK, vg);  // zeros past the end: no contribution
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < BA_V; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (vx[i][e] - mu) * inv;
            const float du = vg[i][e] * act_grad(fmaf(xh, gam, bet), act);
            s1 += du, s2 += du * xh;
        }
    s1 = block_sum_256(s1, red);
    s2 = block_sum_256(s2, red);
    if (threadIdx.x == 0) {
        const int nt = B * chunks, tile = b * chunks + ch;
        part[(size_t)c * nt + tile] = s1;
        part[((size_t)C + c) * nt + tile] = s2;
    }
}

// per channel: dbias = sum du, dweight = sum du*xhat, coef = (mean(du), mean(du*xhat)) (zeros in eval mode)
// (call from all BA_T threads of the block; every thread gets the coefficients, thread 0 of a `writer` block stores dweight /
// dbias -- like bn_finalize_channel, one block's result depends on `part` and the fixed order only)
struct BnCoef {
    float m1, m2;
};
__device__ __forceinline__ BnCoef bn_bwd_finalize_channel(const float* __restrict__ part, int nt, int c, int C, double count,
                                                          int training, float* __restrict__ dweight, float* __restrict__ dbias,
                                                          BnPart first, bool writer) {
    __shared__ double dred[2][4];
    double s1 = 0.0, s2 = 0.0;
    if ((int)threadIdx.x < nt) {   // `first` = bn_part_first(part, c, C, nt)
        s1 += (double)first.a;
        s2 += (double)first.b;
        for (int t = threadIdx.x + BA_T; t < nt; t += BA_T) {
            s1 += (double)part[(size_t)c * nt + t];
            s2 += (double)part[((size_t)C + c) * nt + t];
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) dred[0][threadIdx.x >> 6] = s1, dred[1][threadIdx.x >> 6] = s2;
    __syncthreads();
    s1 = (dred[0][0] + dred[0][1]) + (dred[0][2] + dred[0][3]);
    s2 = (dred[1][0] + dred[1][1]) + (dred[1][2] + dred[1][3]);
    if (writer && threadIdx.x == 0) {
        dbias[c] = (float)s1;
        dweight[c] = (float)s2;
    }
    return BnCoef{training ? (float)(s1 / count) : 0.f, training ? (float)(s2 / count) : 0.f};
}

__global__ __launch_bounds__(BA_T) void bn_act_bwd_finalize_kernel(const float* __restrict__ part, int nt, int C,
                                                                    double count, int training,
                                                                    float* __restrict__ dweight,
                                                                    float* __restrict__ dbias, float* __restrict__ coef) {
    const int c = blockIdx.x;
    const BnCoef k = bn_bwd_finalize_channel(part, nt, c, C, count, training, dweight, dbias, bn_part_first(part, c, C, nt), true);
    if (threadIdx.x == 0) coef[c] = k.m1, coef[C + c] = k.m2;
}

// the backward finalize as the dx pass's prologue (see BnFwdMerge, bn_finalize.hpp): the writer of dweight / dbias is the workgroup of image 0,
// chunk 0 of the channel; `coef` is not used
struct BnBwdMerge {
    int on;             // 0: coef holds finished values (the stand-alone finalize ran in front)
    const float* part;  // [2][C][nt] (sum du, sum du * xhat) partials
    int nt, training;
    double count;
    float *dweight, *dbias;
};

template <bool AL>   // AL: P % 4 == 0, the host's choice
__global__ __launch_bounds__(BA_T) void bn_act_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd,
                                                              const float* __restrict__ weight,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ coef, int C, int P, int chunks,
                                                              int act, float* __restrict__ dx, BnBwdMerge m) {
    const int row = blockIdx.x / chunks, ch = blockIdx.x - row * chunks, c = row % C;
    const float mu = mean[c], inv = invstd[c], gam = weight[c], bet = bias[c], gi = gam * inv;
    BnPart first = bn_part_first(m.part, c, C, m.on ? m.nt : 0);
    f32x4 vx[BA_V], vg[BA_V];
    ba_request<AL>(x + (size_t)row * P, P, ch * BA_CHUNK, vx);
    ba_request<AL>(dy + (size_t)row * P, P, ch * BA_CHUNK, vg);
    bn_part_pin(first);
    float m1, m2;
    if (m.on) {
        const BnCoef k = bn_bwd_finalize_channel(m.part, m.nt, c, C, m.count, m.training, m.dweight, m.dbias, first,
                                                 row < C && ch == 0);
        m1 = k.m1, m2 = k.m2;
    } else {
        m1 = coef[c], m2 = coef[C + c];
    }
#pragma unroll
    for (int i = 0; i < BA_V; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (vx[i][e] - mu) * inv;
            const float du = vg[i][e] * act_grad(fmaf(xh, gam, bet), act);
            vg[i][e] = gi * (du - m1 - xh * m2);
        }
    ba_store(dx + (size_t)row * P, P, ch * BA_CHUNK, vg);
}


// ---- channel gate + activation (squeeze-excite tail, reference mobilenetv3.py:79-83 followed by :121/:141) ----
// y = act(x * gate[b,c]);  backward: du = dy * act'(x*gate), dx = du * gate, dgate[b,c] = sum_p du * x
__global__ __launch_bounds__(BA_T) void gate_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gate,
                                                             int P, int chunks, int act, float* __restrict__ y) {
    const int row = blockIdx.x / chunks, ch = blockIdx.x - row * chunks;
    const float gt = gate[row];
    f32x4 v[BA_V];
    ba_load(x + (size_t)row * P, P, ch * BA_CHUNK, v);
#pragma unroll
    for (int i = 0; i < BA_V; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] = act_fwd(v[i][e] * gt, act);
    ba_store(y + (size_t)row * P, P, ch * BA_CHUNK, v);
}

__global__ __launch_bounds__(BA_T) void gate_act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                             const float* __restrict__ gate, int P, int chunks, int act,
                                                             float* __restrict__ dx, float* __restrict__ part) {
    __shared__ float red[4];
    const int row = blockIdx.x / chunks, ch = blockIdx.x - row * chunks;
    const float gt = gate[row];
    f32x4 vx[BA_V], vg[BA_V];
    ba_load(x + (size_t)row * P, P, ch * BA_CHUNK, vx);
    ba_load(dy + (size_t)row * P, P, ch * BA_CHUNK, vg);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < BA_V; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float du = vg[i][e] * act_grad(vx[i][e] * gt, act);
            s = fmaf(du, vx[i][e], s);
            vg[i][e] = du * gt;
        }
    ba_store(dx + (size_t)row * P, P, ch * BA_CHUNK, vg);
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) part[(size_t)row * chunks + ch] = s;
}

__global__ void gate_act_dgate_kernel(const float* __restrict__ part, int rows, int chunks, float* __restrict__ dgate) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)row * chunks + c];
    dgate[row] = s;
}

// ---- backward of the squeeze-excite tail as one operator: y = act(g[b,c] * x), x = gamma * xhat + beta = bn(z),
// g = SE-MLP(avgpool(x)) (reference mobilenetv3.py:146-149 with SELayer :68-83; the forward is K7 + the pool + the MLP +
// gate_act_fwd, unchanged).  Composed from the separate backward operators this is gate_act_bwd (read dy, x; write dx),
// the pool's broadcast gradient (write), autograd's add of the two (read 2, write 1), then BatchNorm's reduce (read 2) and
// dx (read 2, write 1).  Here: 2 reads of (dy, z) + 1 write, and x is never kept for backward:
//   reduce : A[b,c] = sum_p du, X[b,c] = sum_p du * xhat, S[b,c] = sum_p xhat, du = dy * act'(u), u = g * x
//            -> dgate = gamma X + beta A; the MLP backward (torch, on (B, C)) gives ds, the pooled input's gradient
//   dx     : dz = gamma invstd (g du + ds/P - sum(dx)/N - xhat sum(dx xhat)/N)   (eval mode: without the two means),
//            sum(dx) = sum_b (g A + ds), sum(dx xhat) = sum_b (g X + ds S / P) per channel

// part[k][row][chunk], k = 0: sum du, 1: sum du * xhat, 2: sum xhat
__global__ __launch_bounds__(BA_T) void se_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ weight, const float* __restrict__ bias,
                                                             const float* __restrict__ gate, int rows, int C, int P, int chunks,
                                                             int act, float* __restrict__ part) {
    __shared__ float red[4];
    const int row = blockIdx.x / chunks, ch = blockIdx.x - row * chunks, c = row % C;
    const float mu = mean[c], inv = invstd[c], gam = weight[c], bet = bias[c], gt = gate[row];
    f32x4 vz[BA_V], vg[BA_V];
    ba_load(z + (size_t)row * P, P, ch * BA_CHUNK, vz);
    ba_load(dy + (size_t)row * P, P, ch * BA_CHUNK, vg);  // zeros past the end: no contribution
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int i = 0; i < BA_V; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (vz[i][e] - mu) * inv;
            const float du = vg[i][e] * act_grad(fmaf(xh, gam, bet) * gt, act);
            s1 += du, s2 = fmaf(du, xh, s2);
            if (ba_valid(P, ch * BA_CHUNK, i, e)) s3 += xh;
        }
    s1 = block_sum_256(s1, red);
    s2 = block_sum_256(s2, red);
    s3 = block_sum_256(s3, red);
    if (threadIdx.x == 0) {
        part[(size_t)row * chunks + ch] = s1;
        part[((size_t)rows + row) * chunks + ch] = s2;
        part[((size_t)2 * rows + row) * chunks + ch] = s3;
    }
}

// per row (b,c): sums[k][row] = A, X, S (the chunks of the row in order) and the gradient at the hard sigmoid's input,
// da2 = dgate / 6 where 0 < a2 + 3 < 6 (autograd's ReLU6 convention), dgate = gamma X + beta A
__global__ void se_bwd_gate_kernel(const float* __restrict__ part, int rows, int C, int chunks, const float* __restrict__ weight,
                                   const float* __restrict__ bias, const float* __restrict__ a2, float* __restrict__ sums,
                                   float* __restrict__ da2) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    float s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float t = 0.f;
        for (int j = 0; j < chunks; ++j) t += part[((size_t)k * rows + row) * chunks + j];
        sums[(size_t)k * rows + row] = s[k] = t;
    }
    const int c = row % C;
    const float dgate = weight[c] * s[1] + bias[c] * s[0], u = a2[row] + 3.f;
    da2[row] = (u > 0.f && u < 6.f) ? dgate / 6.f : 0.f;
}

// per channel, images in order: ds_p = ds / P, dbias = sum_b (g A + ds), dweight = sum_b (g X + ds_p S) -- the sums over the
// BatchNorm output's gradient dx = g du + ds_p -- and the dx pass's coefficients coef = (dbias, dweight) / (B P) (eval: 0)
__global__ void se_bwd_coef_kernel(const float* __restrict__ sums, const float* __restrict__ gate, const float* __restrict__ ds,
                                   int B, int C, int P, int training, float* __restrict__ dweight, float* __restrict__ dbias,
                                   float* __restrict__ coef, float* __restrict__ ds_p) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int rows = B * C;
    float db = 0.f, dw = 0.f;
    for (int b = 0; b < B; ++b) {
        const int row = b * C + c;
        const float g = gate[row], d = ds[row], dp = d / (float)P;
        ds_p[row] = dp;
        db += g * sums[row] + d;
        dw += g * sums[rows + row] + dp * sums[2 * rows + row];
    }
    dbias[c] = db;
    dweight[c] = dw;
    const float n = (float)B * (float)P;
    coef[c] = training ? db / n : 0.f;
    coef[C + c] = training ? dw / n : 0.f;
}

__global__ __launch_bounds__(BA_T) void se_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                         const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         const float* __restrict__ weight, const float* __restrict__ bias,
                                                         const float* __restrict__ gate, const float* __restrict__ ds_p,
                                                         const float* __restrict__ coef, int C, int P, int chunks, int act,
                                                         float* __restrict__ dz) {
    const int row = blockIdx.x / chunks, ch = blockIdx.x - row * chunks, c = row % C;
    const float mu = mean[c], inv = invstd[c], gam = weight[c], bet = bias[c], gt = gate[row], dp = ds_p[row];
    const float m1 = coef[c], m2 = coef[C + c], gi = gam * inv;
    f32x4 vz[BA_V], vg[BA_V];
    ba_load(z + (size_t)row * P, P, ch * BA_CHUNK, vz);
    ba_load(dy + (size_t)row * P, P, ch * BA_CHUNK, vg);
#pragma unroll
    for (int i = 0; i < BA_V; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (vz[i][e] - mu) * inv;
            const float du = vg[i][e] * act_grad(fmaf(xh, gam, bet) * gt, act);
            vg[i][e] = gi * (fmaf(gt, du, dp) - m1 - xh * m2);
        }
    ba_store(dz + (size_t)row * P, P, ch * BA_CHUNK, vg);
}

static int ba_chunks(int P) { return ceil_div(P, BA_CHUNK); }

// Launch plan of the two finalizes: merged in the consumer's prologue when a channel has at most BA_PROLOGUE_MAX_NT partials
// (every consumer workgroup reads 2 nt floats of them: <= 8 KB against the 64-96 KB it streams), in the stand-alone kernel above
// that (eval mode has no partials: nt = 0).  CABINET_BN_PROLOGUE=0 restores the stand-alone launch everywhere (read per call:
// the tests flip it in-process).
constexpr int BA_PROLOGUE_MAX_NT = 1024;
static bool bn_prologue_plan(int nt) {
    const char* e = getenv("CABINET_BN_PROLOGUE");
    return !(e && e[0] == '0') && nt <= BA_PROLOGUE_MAX_NT;
}
static void apply_launch(int grid, hipStream_t stream, const float* x, const float* weight, const float* bias,
                         const float* residual, int C, int P, int chunks, int act, float* y, const BnFwdMerge& m) {
    if ((P & 3) == 0)
        hipLaunchKernelGGL(bn_act_apply_kernel<true>, dim3(grid), dim3(BA_T), 0, stream, x, weight, bias, residual, C, P, chunks,
                           act, y, m);
    else
        hipLaunchKernelGGL(bn_act_apply_kernel<false>, dim3(grid), dim3(BA_T), 0, stream, x, weight, bias, residual, C, P, chunks,
                           act, y, m);
}

size_t se_act_bwd_workspace(int B, int C, int P) { return align_up((size_t)3 * B * C * ba_chunks(P) * sizeof(float), 256); }

hipError_t se_act_bwd_reduce_run(const float* dy, const float* z, const float* mean, const float* invstd, const float* weight,
                                 const float* bias, const float* gate, const float* a2, int B, int C, int P, int act, float* sums,
                                 float* da2, void* ws, hipStream_t stream) {
    const int chunks = ba_chunks(P), rows = B * C;
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL(se_bwd_reduce_kernel, dim3(rows * chunks), dim3(BA_T), 0, stream, dy, z, mean, invstd, weight, bias, gate,
                       rows, C, P, chunks, act, part);
    hipLaunchKernelGGL(se_bwd_gate_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, stream, part, rows, C, chunks, weight, bias, a2,
                       sums, da2);
    return hipGetLastError();
}

hipError_t se_act_bwd_coef_run(const float* sums, const float* gate, const float* ds, int B, int C, int P, int training,
                               float* dweight, float* dbias, float* coef, float* ds_p, hipStream_t stream) {
    hipLaunchKernelGGL(se_bwd_coef_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, stream, sums, gate, ds, B, C, P, training, dweight,
                       dbias, coef, ds_p);
    return hipGetLastError();
}

hipError_t se_act_bwd_dx_run(const float* dy, const float* z, const float* mean, const float* invstd, const float* weight,
                             const float* bias, const float* gate, const float* ds_p, const float* coef, int B, int C, int P,
                             int act, float* dz, hipStream_t stream) {
    const int chunks = ba_chunks(P);
    hipLaunchKernelGGL(se_bwd_dx_kernel, dim3(B * C * chunks), dim3(BA_T), 0, stream, dy, z, mean, invstd, weight, bias, gate,
                       ds_p, coef, C, P, chunks, act, dz);
    return hipGetLastError();
}

size_t bn_act_workspace(int B, int C, int P) {
    return align_up((size_t)2 * C * B * ba_chunks(P) * sizeof(float), 256) + align_up((size_t)2 * C * sizeof(float), 256);
}

// The statistics of x for the apply pass: with the finalize in its prologue (the returned m.on: the plan above) only the statistics
// pass runs here, otherwise bn_stats_run.
static BnFwdMerge bn_stats_merge_run(const float* x, float* running_mean, float* running_var, int B, int C, int P, int training,
                              float momentum, float eps, float* save_mean, float* save_invstd, void* ws, hipStream_t stream) {
    const int chunks = ba_chunks(P);
    BnFwdMerge m{0, static_cast<const float*>(ws), B, 0, 0, training, momentum, eps, running_mean, running_var, save_mean, save_invstd};
    if (bn_prologue_plan(training ? B * chunks : 0)) {
        m.on = 1;
        if (training)
            hipLaunchKernelGGL(bn_act_stats_kernel, dim3(B * C * chunks), dim3(BA_T), 0, stream, x, static_cast<float*>(ws), B, C, P,
                               chunks);
    } else {
        (void)bn_stats_run(x, running_mean, running_var, B, C, P, training, momentum, eps, save_mean, save_invstd, ws, stream);
    }
    return m;
}

hipError_t bn_stats_run(const float* x, float* running_mean, float* running_var, int B, int C, int P, int training,
                        float momentum, float eps, float* save_mean, float* save_invstd, void* ws, hipStream_t stream) {
    const int chunks = ba_chunks(P), grid = B * C * chunks;
    float* part = static_cast<float*>(ws);
    if (training)
        hipLaunchKernelGGL(bn_act_stats_kernel, dim3(grid), dim3(BA_T), 0, stream, x, part, B, C, P, chunks);
    hipLaunchKernelGGL(bn_act_finalize_kernel, dim3(C), dim3(BA_T), 0, stream, part, B, C, P, chunks, 0, 0, training, momentum,
                       eps, running_mean, running_var, save_mean, save_invstd);
    return hipGetLastError();
}

// the same forward with the statistics pass replaced by partials a producer already holds (K11's epilogue): finalize + apply only
hipError_t bn_act_fwd_part_run(const float* x, const float* conv_part, int H, int W, const float* weight, const float* bias,
                               float* running_mean, float* running_var, const float* residual, int B, int C, int act, int training,
                               float momentum, float eps, float* y, float* save_mean, float* save_invstd, hipStream_t stream) {
    const int P = H * W, chunks = ba_chunks(P), grid = B * C * chunks;
    const int nt = B * ceil_div(H, 4) * ceil_div(W, 32);   // the producer's tile blocks (bn_finalize.hpp)
    BnFwdMerge m{0, conv_part, B, H, W, training, momentum, eps, running_mean, running_var, save_mean, save_invstd};
    if (bn_prologue_plan(training ? nt : 0))
        m.on = 1;
    else
        hipLaunchKernelGGL(bn_act_finalize_kernel, dim3(C), dim3(BA_T), 0, stream, conv_part, B, C, P, chunks, H, W, training,
                           momentum, eps, running_mean, running_var, save_mean, save_invstd);
    apply_launch(grid, stream, x, weight, bias, residual, C, P, chunks, act, y, m);
    return hipGetLastError();
}

hipError_t bn_act_fwd_run(const float* x, const float* weight, const float* bias, float* running_mean,
                          float* running_var, const float* residual, int B, int C, int P, int act, int training,
                          float momentum, float eps, float* y, float* save_mean, float* save_invstd, void* ws,
                          hipStream_t stream) {
    const int chunks = ba_chunks(P), grid = B * C * chunks;
    const BnFwdMerge m = bn_stats_merge_run(x, running_mean, running_var, B, C, P, training, momentum, eps, save_mean, save_invstd,
                                            ws, stream);
    apply_launch(grid, stream, x, weight, bias, residual, C, P, chunks, act, y, m);
    return hipGetLastError();
}

hipError_t bn_bwd_tail_run(const float* part, int nt, const float* dy, const float* x, const float* weight,
                           const float* bias, const float* save_mean, const float* save_invstd, int B, int C, int P,
                           int act, int training, float* dx, float* dweight, float* dbias, float* coef,
                           hipStream_t stream) {
    const int chunks = ba_chunks(P), grid = B * C * chunks;
    BnBwdMerge m{0, part, nt, training, (double)B * (double)P, dweight, dbias};
    if (bn_prologue_plan(nt))
        m.on = 1;
    else
        hipLaunchKernelGGL(bn_act_bwd_finalize_kernel, dim3(C), dim3(BA_T), 0, stream, part, nt, C, m.count, training, dweight,
                           dbias, coef);
    if ((P & 3) == 0)
        hipLaunchKernelGGL(bn_act_bwd_dx_kernel<true>, dim3(grid), dim3(BA_T), 0, stream, dy, x, save_mean, save_invstd, weight,
                           bias, coef, C, P, chunks, act, dx, m);
    else
        hipLaunchKernelGGL(bn_act_bwd_dx_kernel<false>, dim3(grid), dim3(BA_T), 0, stream, dy, x, save_mean, save_invstd, weight,
                           bias, coef, C, P, chunks, act, dx, m);
    return hipGetLastError();
}

hipError_t bn_act_bwd_run(const float* dy, const float* x, const float* weight, const float* bias,
                          const float* save_mean, const float* save_invstd, int B, int C, int P, int act, int training,
                          float* dx, float* dweight, float* dbias, void* ws, hipStream_t stream) {
    const int chunks = ba_chunks(P), grid = B * C * chunks, nt = B * chunks;
    float* part = static_cast<float*>(ws);
    float* coef = reinterpret_cast<float*>(static_cast<char*>(ws) + align_up((size_t)2 * C * nt * sizeof(float), 256));
    hipLaunchKernelGGL(bn_act_bwd_reduce_kernel, dim3(grid), dim3(BA_T), 0, stream, dy, x, save_mean, save_invstd, weight,
                       bias, B, C, P, chunks, act, part);
    return bn_bwd_tail_run(part, nt, dy, x, weight, bias, save_mean, save_invstd, B, C, P, act, training, dx, dweight,
                           dbias, coef, stream);
}

// The backward without its dx pass, for a consumer that forms dx itself while it stages its operand (K9's weight gradient, the
// only reader of sb.conv1's dz): reduce + the stand-alone finalize, which writes dweight, dbias and -- at *coef, inside `ws`
// (bn_act_workspace) -- (mean(du), mean(du * xhat)) per channel, the bits bn_bwd_tail_run's prologue plan gives its dx pass.
hipError_t bn_act_bwd_stats_run(const float* dy, const float* x, const float* weight, const float* bias,
                                const float* save_mean, const float* save_invstd, int B, int C, int P, int act, int training,
                                float* dweight, float* dbias, void* ws, const float** coef, hipStream_t stream) {
    const int chunks = ba_chunks(P), grid = B * C * chunks, nt = B * chunks;
    float* part = static_cast<float*>(ws);
    float* cf = reinterpret_cast<float*>(static_cast<char*>(ws) + align_up((size_t)2 * C * nt * sizeof(float), 256));
    hipLaunchKernelGGL(bn_act_bwd_reduce_kernel, dim3(grid), dim3(BA_T), 0, stream, dy, x, save_mean, save_invstd, weight,
                       bias, B, C, P, chunks, act, part);
    hipLaunchKernelGGL(bn_act_bwd_finalize_kernel, dim3(C), dim3(BA_T), 0, stream, part, nt, C, (double)B * (double)P, training,
                       dweight, dbias, cf);
    *coef = cf;
    return hipGetLastError();
}

// the stand-alone finalize alone, on partials a producer kernel wrote (K8's backward): dweight, dbias and coef [2][C]
hipError_t bn_bwd_finalize_run(const float* part, int nt, int C, double count, int training, float* dweight, float* dbias,
                               float* coef, hipStream_t stream) {
    hipLaunchKernelGGL(bn_act_bwd_finalize_kernel, dim3(C), dim3(BA_T), 0, stream, part, nt, C, count, training, dweight, dbias,
                       coef);
    return hipGetLastError();
}

size_t gate_act_workspace(int rows, int P) { return align_up((size_t)rows * ba_chunks(P) * sizeof(float), 256); }

hipError_t gate_act_fwd_run(const float* x, const float* gate, int rows, int P, int act, float* y, hipStream_t stream) {
    const int chunks = ba_chunks(P);
    hipLaunchKernelGGL(gate_act_fwd_kernel, dim3(rows * chunks), dim3(BA_T), 0, stream, x, gate, P, chunks, act, y);
    return hipGetLastError();
}

hipError_t gate_act_bwd_run(const float* dy, const float* x, const float* gate, int rows, int P, int act, float* dx,
                            float* dgate, void* ws, hipStream_t stream) {
    const int chunks = ba_chunks(P);
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL(gate_act_bwd_kernel, dim3(rows * chunks), dim3(BA_T), 0, stream, dy, x, gate, P, chunks, act, dx,
                       part);
    hipLaunchKernelGGL(gate_act_dgate_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, stream, part, rows, chunks, dgate);
    return hipGetLastError();
}

}  // namespace cabinet
