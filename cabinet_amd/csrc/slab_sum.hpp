// Ordered sum of the per-workgroup slabs a split weight gradient leaves behind (K9, K14, K15): no atomics, a fixed order.
#pragma once
#include "common.hpp"

namespace cabinet {

// dw[i] = sum over the slabs in a fixed order: 32 elements x Q slab lanes per workgroup (128-byte row segments; a lane adds
// slabs q, q + Q, ... in four independent chains), then the Q partial sums in order.  Q = 32 where one tile was split
// hundreds of ways (the thin layers: 512 slabs of 19 KB), Q = 8 for the few large slabs of the wide ones.
template <int Q>
__global__ __launch_bounds__(32 * Q) void slab_sum_kernel(const float* __restrict__ slabs, int nslab, int count,
                                                          float* __restrict__ dw) {
    __shared__ float red[Q][32];
    const int e = threadIdx.x & 31, q = threadIdx.x >> 5, i = blockIdx.x * 32 + e;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (i < count) {
        const float* p = slabs + i;
        int k = q;
        for (; k + 3 * Q < nslab; k += 4 * Q) {
            s0 += p[(size_t)k * count];
            s1 += p[(size_t)(k + Q) * count];
            s2 += p[(size_t)(k + 2 * Q) * count];
            s3 += p[(size_t)(k + 3 * Q) * count];
        }
        for (; k < nslab; k += Q) s0 += p[(size_t)k * count];
    }
    red[q][e] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (q == 0 && i < count) {
        float t = red[0][e];
#pragma unroll
        for (int k = 1; k < Q; ++k) t += red[k][e];
        dw[i] = t;
    }
}

// Q = 32 from 128 slabs on (every slab lane then still adds four or more), else Q = 8
static inline void slab_sum_launch(const float* slabs, int nslab, int count, float* dw, hipStream_t stream) {
    if (nslab >= 128)
        hipLaunchKernelGGL(slab_sum_kernel<32>, dim3(ceil_div(count, 32)), dim3(1024), 0, stream, slabs, nslab, count, dw);
    else
        hipLaunchKernelGGL(slab_sum_kernel<8>, dim3(ceil_div(count, 32)), dim3(256), 0, stream, slabs, nslab, count, dw);
}

}  // namespace cabinet
