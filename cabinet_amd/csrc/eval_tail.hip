// K13 -- the probability tail of multi-scale evaluation (reference src/scripts/evaluate.py:69-159 and :193-226).
//
// The model ends at a low resolution (CABiNet.forward_lowres: H/8 x W/8); the reference's evaluator then walks the
// (N, C, H, W) tensor again and again: upsample, softmax, flip, softmax, +=, *= 0.5, window +=, count +=, divide, resize
// back, probs +=, argmax, copy to the host, numpy.bincount.  Here that is three kernels:
//   eval_chip_accum   one launch per chip: sample the C low-resolution logits of a pixel (bilinear, align_corners=False),
//                     softmax over classes in registers, the same for the logits of the flipped chip at the mirrored column,
//                     average, scale by 1 / (number of windows covering the pixel) and add into the window of the destination.
//                     Only the destination is read or written at full resolution.
//   eval_scale_merge  total += resize(prob[:, :, hst:hed, wst:wed] -> (H, W)): one pass over `total`.
//   eval_argmax_hist  argmax over classes (lowest index on ties), ignore / clip rule of compute_hist, C x C histogram in LDS,
//                     one global 64-bit integer atomic per non-zero bin per workgroup: exactly reproducible.
// The reference's count map is the outer product of two 1-D vectors (windows form a grid), so it never exists as a tensor:
// the caller passes the two reciprocal vectors and the scaling happens at accumulation time.
#include <stdint.h>

#include "common.hpp"

namespace cabinet {

// source columns a segment of `T` chip pixels can touch (both taps): the source index grows by rw per pixel
static inline int eval_span(int T, int wl, int cw) {
    const float rw = (float)wl / (float)cw;
    const int s = (int)ceilf((float)T * rw) + 3;
    return s < wl ? s : wl;
}
static const size_t EVAL_LDS_MAX = 64 * 1024;

// threads per workgroup (= chip pixels of one row segment) for which the staged source rows fit the LDS; 0: none does
int eval_chip_threads(int C, int wl, int cw, int nsrc) {
    for (int T = 256; T >= 64; T >>= 1)
        if ((size_t)nsrc * C * eval_span(T, wl, cw) * sizeof(float) <= EVAL_LDS_MAX) return T;
    return 0;
}

// softmax over the CMAX classes of one pixel from vertically lerped source rows in LDS; p[c] (+)= w * softmax(x)[c]
template <int CMAX, bool ADD>
__device__ __forceinline__ void eval_pixel_softmax(const float* __restrict__ rows, int span, int i0, int i1, float lx, float w,
                                                   float (&p)[CMAX]) {
    float x[CMAX], mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        x[c] = (1.f - lx) * rows[c * span + i0] + lx * rows[c * span + i1];
        mx = fmaxf(mx, x[c]);
    }
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        x[c] = fast_exp2((x[c] - mx) * LOG2E_F);
        sum += x[c];
    }
    const float s = w / sum;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) p[c] = ADD ? p[c] + x[c] * s : x[c] * s;
}

// One workgroup per (row segment of blockDim.x chip pixels, chip row, image).  The two source rows of every class are lerped
// vertically into LDS once (for the columns this segment touches), so a pixel's logit costs two LDS reads.
// CMAX = 8, 19: C == CMAX, the per-class loops fully unrolled with the probabilities in registers (the project's two class
// counts); CMAX = 0: any C, run-time loops.
template <int CMAX>
__global__ __launch_bounds__(256) void eval_chip_accum_kernel(const float* __restrict__ a, const float* __restrict__ b, int C, int hl,
                                                               int wl, int ch, int cw, float rh, float rw, int span,
                                                               float* __restrict__ dst, int FH, int FW, int y0, int x0,
                                                               const float* __restrict__ rcp_y, const float* __restrict__ rcp_x) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [a | b][C][span]
    const int T = blockDim.x, n = blockIdx.z, oy = blockIdx.y;
    const int ox_lo = blockIdx.x * T, ox_hi = min(ox_lo + T, cw) - 1, ox = ox_lo + threadIdx.x;
    const size_t plane = (size_t)hl * wl;
    int ys0, ys1, t0, t1;
    float ly, tl;
    bilinear_taps(oy, rh, hl, ys0, ys1, ly);
    // first source column of the segment for a, and for b (which is read at the mirrored column cw - 1 - ox)
    int a_lo, a_hi, b_lo = 0, b_hi = 0;
    bilinear_taps(ox_lo, rw, wl, a_lo, t1, tl);
    bilinear_taps(ox_hi, rw, wl, t0, a_hi, tl);
    if (b) {
        bilinear_taps(cw - 1 - ox_hi, rw, wl, b_lo, t1, tl);
        bilinear_taps(cw - 1 - ox_lo, rw, wl, t0, b_hi, tl);
    }
    const int na = min(a_hi - a_lo + 1, span), nb = b ? min(b_hi - b_lo + 1, span) : 0;
    const float* a_n = a + (size_t)n * C * plane;
    for (int i = threadIdx.x; i < C * na; i += T) {
        const int c = i / na, xs = i - c * na;
        const float* p = a_n + (size_t)c * plane + a_lo + xs;
        lds[c * span + xs] = (1.f - ly) * p[ys0 * wl] + ly * p[ys1 * wl];
    }
    if (b) {
        const float* b_n = b + (size_t)n * C * plane;
        float* lb = lds + C * span;
        for (int i = threadIdx.x; i < C * nb; i += T) {
            const int c = i / nb, xs = i - c * nb;
            const float* p = b_n + (size_t)c * plane + b_lo + xs;
            lb[c * span + xs] = (1.f - ly) * p[ys0 * wl] + ly * p[ys1 * wl];
        }
    }
    __syncthreads();
    if (ox >= cw) return;
    const int gy = y0 + oy, gx = x0 + ox;
    float w = b ? 0.5f : 1.f;
    if (rcp_y) w *= rcp_y[gy];
    if (rcp_x) w *= rcp_x[gx];
    float* d = dst + ((size_t)n * C * FH + gy) * FW + gx;
    const size_t dplane = (size_t)FH * FW;
    int i0, i1, j0 = 0, j1 = 0;
    float lx, mx = 0.f;
    bilinear_taps(ox, rw, wl, i0, i1, lx);
    i0 = max(min(i0 - a_lo, na - 1), 0), i1 = max(min(i1 - a_lo, na - 1), 0);
    if (b) {
        bilinear_taps(cw - 1 - ox, rw, wl, j0, j1, mx);
        j0 = max(min(j0 - b_lo, nb - 1), 0), j1 = max(min(j1 - b_lo, nb - 1), 0);
    }
    const float* lb = lds + C * span;
    if constexpr (CMAX == 0) {
        // any C <= 32: run-time loops, the logits re-read from LDS in each of the three passes (no per-class registers)
        float ma = -INFINITY, mb = -INFINITY, sa = 0.f, sb = 0.f;
        for (int c = 0; c < C; ++c) {
            ma = fmaxf(ma, (1.f - lx) * lds[c * span + i0] + lx * lds[c * span + i1]);
            if (b) mb = fmaxf(mb, (1.f - mx) * lb[c * span + j0] + mx * lb[c * span + j1]);
        }
        for (int c = 0; c < C; ++c) {
            sa += fast_exp2((((1.f - lx) * lds[c * span + i0] + lx * lds[c * span + i1]) - ma) * LOG2E_F);
            if (b) sb += fast_exp2((((1.f - mx) * lb[c * span + j0] + mx * lb[c * span + j1]) - mb) * LOG2E_F);
        }
        sa = w / sa, sb = w / sb;
        for (int c = 0; c < C; ++c) {
            float p = fast_exp2((((1.f - lx) * lds[c * span + i0] + lx * lds[c * span + i1]) - ma) * LOG2E_F) * sa;
            if (b) p += fast_exp2((((1.f - mx) * lb[c * span + j0] + mx * lb[c * span + j1]) - mb) * LOG2E_F) * sb;
            d[c * dplane] += p;
        }
    } else {
        float p[CMAX];
        eval_pixel_softmax<CMAX, false>(lds, span, i0, i1, lx, w, p);
        if (b) eval_pixel_softmax<CMAX, true>(lb, span, j0, j1, mx, w, p);
#pragma unroll
        for (int c = 0; c < CMAX; ++c) d[c * dplane] += p[c];
    }
}

hipError_t eval_chip_accum_run(const float* a, const float* b, int N, int C, int hl, int wl, int ch, int cw, float* dst, int FH,
                               int FW, int y0, int x0, const float* rcp_y, const float* rcp_x, hipStream_t stream) {
    const int nsrc = b ? 2 : 1, T = eval_chip_threads(C, wl, cw, nsrc);
    if (T == 0) return hipErrorInvalidValue;
    const int span = eval_span(T, wl, cw);
    const size_t lds = (size_t)nsrc * C * span * sizeof(float);
    const dim3 grid(ceil_div(cw, T), ch, N);
    const float rh = (float)hl / (float)ch, rw = (float)wl / (float)cw;
#define EVAL_CHIP(CM)                                                                                                            \
    hipLaunchKernelGGL((eval_chip_accum_kernel<CM>), grid, dim3(T), lds, stream, a, b, C, hl, wl, ch, cw, rh, rw, span, dst, FH, \
                       FW, y0, x0, rcp_y, rcp_x)
    if (C == 8)
        EVAL_CHIP(8);
    else if (C == 19)
        EVAL_CHIP(19);
    else
        EVAL_CHIP(0);
#undef EVAL_CHIP
    return hipGetLastError();
}

// total (N,C,H,W) += resize(prob (N,C,FH,FW)[:, :, hst:hst+sh, wst:wst+sw] -> (H,W)); VEC output pixels of one row per thread
template <int VEC>
__global__ __launch_bounds__(256) void eval_scale_merge_kernel(const float* __restrict__ prob, int FH, int FW, int hst, int wst, int sh,
                                                                int sw, float rh, float rw, float* __restrict__ total, int H, int W) {
    const int xv = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, nc = blockIdx.z;
    const int x = xv * VEC;
    if (x >= W) return;
    int ya, yb;
    float ly;
    bilinear_taps(y, rh, sh, ya, yb, ly);
    const float* r0 = prob + ((size_t)nc * FH + hst + ya) * FW + wst;
    const float* r1 = prob + ((size_t)nc * FH + hst + yb) * FW + wst;
    float* t = total + ((size_t)nc * H + y) * W + x;
    float v[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        int xa, xb;
        float lx;
        bilinear_taps(x + j, rw, sw, xa, xb, lx);  // VEC > 1 only when W % VEC == 0: x + j < W
        v[j] = (1.f - ly) * ((1.f - lx) * r0[xa] + lx * r0[xb]) + ly * ((1.f - lx) * r1[xa] + lx * r1[xb]);
    }
    if (VEC == 4) {
        f32x4 o = *reinterpret_cast<const f32x4*>(t);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += v[j];
        *reinterpret_cast<f32x4*>(t) = o;
    } else {
        t[0] += v[0];
    }
}

hipError_t eval_scale_merge_run(const float* prob, int N, int C, int FH, int FW, int hst, int hed, int wst, int wed, float* total,
                                int H, int W, hipStream_t stream) {
    const int sh = hed - hst, sw = wed - wst;
    const float rh = (float)sh / (float)H, rw = (float)sw / (float)W;
    if (W % 4 == 0) {
        const dim3 grid(ceil_div(W / 4, 256), H, N * C);
        hipLaunchKernelGGL((eval_scale_merge_kernel<4>), grid, dim3(256), 0, stream, prob, FH, FW, hst, wst, sh, sw, rh, rw, total, H, W);
    } else {
        const dim3 grid(ceil_div(W, 256), H, N * C);
        hipLaunchKernelGGL((eval_scale_merge_kernel<1>), grid, dim3(256), 0, stream, prob, FH, FW, hst, wst, sh, sw, rh, rw, total, H, W);
    }
    return hipGetLastError();
}

// argmax over classes + confusion matrix.  P = H * W pixels per image, VEC consecutive pixels per thread (P % VEC == 0).
// hist[pred * C + label]: int32 bins in LDS (a workgroup sees far fewer than 2^31 pixels), flushed with one 64-bit atomic per
// non-zero bin.  Strict `>` keeps the lowest index among equal values (torch.argmax).
// EVAL_HIST_COPIES copies of the bins, chosen by lane: neighbouring pixels of a real image share (prediction, label), and LDS
// atomics on one address serialise.  CFIX = 8, 19: C == CFIX, the class loop fully unrolled so that a thread's C loads are in
// flight together; CFIX = 0: any C, unrolled by four.
// 512 workgroups: every workgroup ends with up to C * C atomics on the SAME C * C addresses, which serialise in the L2 (2048
// workgroups measured 85 us at config 5's shape, most of it that flush); 8 waves per CU with C 16-byte loads each in flight
// still keep the memory pipe full.
#define EVAL_HIST_BLOCKS 512
#define EVAL_HIST_COPIES 8
template <int VEC, int CFIX>
__global__ __launch_bounds__(256) void eval_argmax_hist_kernel(const float* __restrict__ total, const long long* __restrict__ labels,
                                                                int N, int Crt, size_t P, int ignore_lb,
                                                                unsigned long long* __restrict__ hist, unsigned char* __restrict__ pred) {
    constexpr int CC = CFIX ? CFIX * CFIX : 32 * 32;
    __shared__ int bins[EVAL_HIST_COPIES * CC];
    const int C = CFIX ? CFIX : Crt;
    for (int i = threadIdx.x; i < EVAL_HIST_COPIES * CC; i += 256) bins[i] = 0;
    __syncthreads();
    int* my_bins = bins + (threadIdx.x & (EVAL_HIST_COPIES - 1)) * CC;
    const size_t groups = (size_t)N * (P / VEC);
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        const size_t n = g / (P / VEC), q = (g - n * (P / VEC)) * VEC;
        const float* t = total + n * C * P + q;
        float best[VEC];
        int arg[VEC];
        if (VEC == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(t);
#pragma unroll
            for (int j = 0; j < 4; ++j) best[j] = v[j], arg[j] = 0;
            if constexpr (CFIX > 0) {
                f32x4 u[CFIX];
#pragma unroll
                for (int c = 1; c < CFIX; ++c) u[c] = *reinterpret_cast<const f32x4*>(t + c * P);
#pragma unroll
                for (int c = 1; c < CFIX; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (u[c][j] > best[j]) best[j] = u[c][j], arg[j] = c;
            } else {
#pragma unroll 4
                for (int c = 1; c < C; ++c) {
                    const f32x4 u = *reinterpret_cast<const f32x4*>(t + c * P);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (u[j] > best[j]) best[j] = u[j], arg[j] = c;
                }
            }
        } else {
            best[0] = t[0], arg[0] = 0;
#pragma unroll 4
            for (int c = 1; c < C; ++c) {
                const float u = t[c * P];
                if (u > best[0]) best[0] = u, arg[0] = c;
            }
        }
        const long long* lb = labels + n * P + q;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const long long l = lb[j];
            if (l != (long long)ignore_lb) {
                const int lc = (int)(l < 0 ? 0 : (l > (long long)(C - 1) ? (long long)(C - 1) : l));
                atomicAdd(&my_bins[arg[j] * C + lc], 1);
            }
        }
        if (pred) {
            if (VEC == 4) {
                *reinterpret_cast<unsigned*>(pred + n * P + q) =
                    (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
            } else {
                pred[n * P + q] = (unsigned char)arg[0];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < EVAL_HIST_COPIES; ++k) v += bins[k * CC + i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

hipError_t eval_argmax_hist_run(const float* total, const long long* labels, int N, int C, int H, int W, int ignore_lb, long long* hist,
                                unsigned char* pred, hipStream_t stream) {
    const size_t P = (size_t)H * W;
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    const int vec = P % 4 == 0 ? 4 : 1;
    const size_t blocks = ((size_t)N * (P / vec) + 255) / 256;
    const dim3 grid((unsigned)(blocks < EVAL_HIST_BLOCKS ? blocks : EVAL_HIST_BLOCKS));
#define EVAL_HIST(V, CF) \
    hipLaunchKernelGGL((eval_argmax_hist_kernel<V, CF>), grid, dim3(256), 0, stream, total, labels, N, C, P, ignore_lb, h, pred)
    if (vec == 4) {
        if (C == 8)
            EVAL_HIST(4, 8);
        else if (C == 19)
            EVAL_HIST(4, 19);
        else
            EVAL_HIST(4, 0);
    } else {
        EVAL_HIST(1, 0);
    }
#undef EVAL_HIST
    return hipGetLastError();
}

}  // namespace cabinet
