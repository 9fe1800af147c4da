// Backward of the squeeze-excite MLP between the two streaming passes of the SE tail (bn_act.hip: se_bwd_reduce / se_bwd_dx),
// gate = hsig(a2), a2 = W2 h1 + b2, h1 = relu(W1 pooled + b1), on (B, C) and (B, Cs) tensors (reference mobilenetv3.py:68-83):
//   dw2[c][j] = sum_b da2[b][c] h1[b][j]      db2[c] = sum_b da2[b][c]
//   da1[b][j] = sum_c da2[b][c] w2[c][j]  where h1[b][j] > 0, else 0  (autograd's ReLU convention: the OUTPUT is > 0)
//   dw1[j][c] = sum_b da1[b][j] pooled[b][c]  db1[j] = sum_b da1[b][j]
//   ds[b][c]  = sum_j da1[b][j] w1[j][c]      then the tail of se_bwd_coef_kernel (ds_p, dbias, dweight, coef)
// Two launches, because da1 needs all of da2 and ds needs all of da1; no workgroup of a launch reads what another one of the
// same launch writes.  The work is a few MFLOP on L2-resident data: what counts is the number of dependent launches (the
// torch form took ten) and that each launch spreads over enough CUs to keep its own dependent-load chain short.
//   launch A : [contraction over C  -> da1 (workspace)]  [outer products -> dw2, db2]
//   launch B : [contraction over Cs -> ds, coefficient tail]  [outer products -> dw1, db1]
// Every sum has a fixed order (per thread a strided walk, the SM_KS walks merged in order, images in order): bit-reproducible.
// The sums are kept in fp64 and rounded once when stored: at this size the fp64 FMAs cost nothing that can be measured, and
// each gradient is then the fp32 number next to the exact sum whatever the grouping (the coefficient tail stays fp32, as it is
// in se_bwd_coef_kernel).
#include "common.hpp"

namespace cabinet {

constexpr int SM_T = 256;    // threads per workgroup
constexpr int SM_NB = 8;     // images per pass of a contraction (B beyond it: further passes)
constexpr int SM_CT = 8;     // output columns per contraction workgroup: one 32-byte segment of each weight row
constexpr int SM_KS = SM_T / SM_CT;  // ways the contracted dimension is split across threads
constexpr int SM_RT = 8;     // rows per outer-product workgroup
// largest contracted dimension.  LDS of a workgroup: the staged operand, SM_NB x SM_MAX_K floats (32 KB), and the SM_KS partial
// sums per (image, column) as doubles (16 KB): 48 KB, plus 256 B in launch B -- under the 64 KB a workgroup may declare.  The
// outer-product workgroups of the same kernels declare it without using it (3 per CU: no matter at these grids).
constexpr int SM_MAX_K = 1024;

// One pass of out[b][q] = sum_k a[b][k] w[k][q] for the images b0 .. b0 + SM_NB - 1 and the SM_CT columns from q0 on:
// thread (ql, ks) walks k = ks, ks + SM_KS, ... with the pass's rows of a in LDS, the walks are merged in the order of ks.
// Returns, in the threads t < SM_NB * SM_CT, the sum for (image b0 + t / SM_CT, column q0 + t % SM_CT); 0 outside (B, Q).
__device__ __forceinline__ float contract_pass(const float* __restrict__ a, const float* __restrict__ w, int B, int K, int Q, int b0,
                                               int q0, float* as, double* red) {
    const int t = threadIdx.x, ql = t % SM_CT, ks = t / SM_CT, q = q0 + ql;
    __syncthreads();  // the previous pass has read as and red
    for (int bl = 0; bl < SM_NB; ++bl)
        for (int k = t; k < K; k += SM_T) as[bl * K + k] = b0 + bl < B ? a[(size_t)(b0 + bl) * K + k] : 0.f;
    __syncthreads();
    double acc[SM_NB];
#pragma unroll
    for (int bl = 0; bl < SM_NB; ++bl) acc[bl] = 0.;
    if (q < Q)
        for (int k = ks; k < K; k += SM_KS) {
            const double wv = w[(size_t)k * Q + q];
#pragma unroll
            for (int bl = 0; bl < SM_NB; ++bl) acc[bl] = fma((double)as[bl * K + k], wv, acc[bl]);
        }
#pragma unroll
    for (int bl = 0; bl < SM_NB; ++bl) red[(ks * SM_NB + bl) * SM_CT + ql] = acc[bl];
    __syncthreads();
    double s = 0.;
    if (t < SM_NB * SM_CT)
        for (int k = 0; k < SM_KS; ++k) s += red[k * SM_NB * SM_CT + t];
    return (float)s;
}

// out[r][q] = sum_b a[b][r] v[b][q] for the SM_RT rows from r0 on and column q = q0 + thread, rsum[r] = sum_b a[b][r] (by the
// workgroups of the first column tile); images in order.  a is read at wave-uniform addresses.
__device__ __forceinline__ void outer_tile(const float* __restrict__ a, const float* __restrict__ v, int B, int R, int Q, int r0,
                                           int q0, float* __restrict__ out, float* __restrict__ rsum) {
    const int t = threadIdx.x, q = q0 + t, nr = min(SM_RT, R - r0);
    if (q < Q) {
        double acc[SM_RT];
#pragma unroll
        for (int r = 0; r < SM_RT; ++r) acc[r] = 0.;
        for (int b = 0; b < B; ++b) {
            const double x = v[(size_t)b * Q + q];
#pragma unroll
            for (int r = 0; r < SM_RT; ++r)
                if (r < nr) acc[r] = fma((double)a[(size_t)b * R + r0 + r], x, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < SM_RT; ++r)
            if (r < nr) out[(size_t)(r0 + r) * Q + q] = (float)acc[r];
    }
    if (q0 == 0 && t < nr) {
        double s = 0.;
        for (int b = 0; b < B; ++b) s += (double)a[(size_t)b * R + r0 + t];
        rsum[r0 + t] = (float)s;
    }
}

// workgroups [0, nslab): da1 for SM_CT columns of Cs; the rest: dw2 / db2 tiles, (row slab of C) x (column tile of Cs)
__global__ __launch_bounds__(SM_T) void se_mlp_bwd_a_kernel(const float* __restrict__ da2, const float* __restrict__ h1,
                                                            const float* __restrict__ w2, int B, int C, int Cs, int nslab, int qtiles,
                                                            float* __restrict__ da1, float* __restrict__ dw2, float* __restrict__ db2) {
    __shared__ float as[SM_NB * SM_MAX_K];
    __shared__ double red[SM_KS * SM_NB * SM_CT];
    const int blk = blockIdx.x;
    if (blk < nslab) {
        const int t = threadIdx.x, j = blk * SM_CT + t % SM_CT;
        for (int b0 = 0; b0 < B; b0 += SM_NB) {
            const float s = contract_pass(da2, w2, B, C, Cs, b0, blk * SM_CT, as, red);
            const int b = b0 + t / SM_CT;
            if (t < SM_NB * SM_CT && b < B && j < Cs) da1[(size_t)b * Cs + j] = h1[(size_t)b * Cs + j] > 0.f ? s : 0.f;
        }
    } else {
        const int tile = blk - nslab;
        outer_tile(da2, h1, B, C, Cs, (tile / qtiles) * SM_RT, (tile % qtiles) * SM_T, dw2, db2);
    }
}

// workgroups [0, nslab): ds for SM_CT channels and, those channels being this workgroup's for every image, the tail of
// se_bwd_coef_kernel (bn_act.hip) with its expressions and its image order; the rest: dw1 / db1 tiles
__global__ __launch_bounds__(SM_T) void se_mlp_bwd_b_kernel(const float* __restrict__ da1, const float* __restrict__ pooled,
                                                            const float* __restrict__ w1, const float* __restrict__ sums,
                                                            const float* __restrict__ gate, int B, int C, int Cs, int P, int training,
                                                            int nslab, int qtiles, float* __restrict__ ds, float* __restrict__ dw1,
                                                            float* __restrict__ db1, float* __restrict__ dweight,
                                                            float* __restrict__ dbias, float* __restrict__ coef,
                                                            float* __restrict__ ds_p) {
    __shared__ float as[SM_NB * SM_MAX_K];
    __shared__ double red[SM_KS * SM_NB * SM_CT];
    __shared__ float dsl[SM_NB * SM_CT];
    const int blk = blockIdx.x;
    if (blk < nslab) {
        const int t = threadIdx.x, c = blk * SM_CT + t, rows = B * C;
        float db = 0.f, dw = 0.f;
        for (int b0 = 0; b0 < B; b0 += SM_NB) {
            const float s = contract_pass(da1, w1, B, Cs, C, b0, blk * SM_CT, as, red);
            if (t < SM_NB * SM_CT) {
                const int b = b0 + t / SM_CT, cc = blk * SM_CT + t % SM_CT;
                dsl[t] = s;
                if (b < B && cc < C) ds[(size_t)b * C + cc] = s;
            }
            __syncthreads();  // the next write of dsl comes after the next pass's barriers
            if (t < SM_CT && c < C)
                for (int b = b0; b < min(b0 + SM_NB, B); ++b) {
                    const int row = b * C + c;
                    const float g = gate[row], d = dsl[(b - b0) * SM_CT + t], dp = d / (float)P;
                    ds_p[row] = dp;
                    db += g * sums[row] + d;
                    dw += g * sums[rows + row] + dp * sums[2 * rows + row];
                }
        }
        if (t < SM_CT && c < C) {
            dbias[c] = db;
            dweight[c] = dw;
            const float n = (float)B * (float)P;
            coef[c] = training ? db / n : 0.f;
            coef[C + c] = training ? dw / n : 0.f;
        }
    } else {
        const int tile = blk - nslab;
        outer_tile(da1, pooled, B, Cs, C, (tile / qtiles) * SM_RT, (tile % qtiles) * SM_T, dw1, db1);
    }
}

bool se_act_bwd_mlp_supported(int C, int Cs) { return C <= SM_MAX_K && Cs <= SM_MAX_K; }

size_t se_act_bwd_mlp_workspace(int B, int Cs) { return align_up((size_t)B * Cs * sizeof(float), 256); }  // da1

hipError_t se_act_bwd_mlp_run(const float* sums, const float* da2, const float* gate, const float* h1, const float* pooled,
                              const float* w1, const float* w2, int B, int C, int Cs, int P, int training, float* dw1, float* db1,
                              float* dw2, float* db2, float* ds, float* dweight, float* dbias, float* coef, float* ds_p, void* ws,
                              hipStream_t stream) {
    float* da1 = static_cast<float*>(ws);
    const int slab_a = ceil_div(Cs, SM_CT), qt_a = ceil_div(Cs, SM_T), slab_b = ceil_div(C, SM_CT), qt_b = ceil_div(C, SM_T);
    hipLaunchKernelGGL(se_mlp_bwd_a_kernel, dim3(slab_a + ceil_div(C, SM_RT) * qt_a), dim3(SM_T), 0, stream, da2, h1, w2, B, C, Cs,
                       slab_a, qt_a, da1, dw2, db2);
    hipLaunchKernelGGL(se_mlp_bwd_b_kernel, dim3(slab_b + ceil_div(Cs, SM_RT) * qt_b), dim3(SM_T), 0, stream, da1, pooled, w1, sums,
                       gate, B, C, Cs, P, training, slab_b, qt_b, ds, dw1, db1, dweight, dbias, coef, ds_p);
    return hipGetLastError();
}

}  // namespace cabinet
