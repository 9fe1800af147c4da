// K17 -- the tail of single-image inference (reference src/scripts/visualize.py:50-61, :64-140 and :165-177).
//
// The deployment setting (scales = [1.0], no flip) never needs the full-resolution class tensor: softmax is monotonic per
// pixel, so argmax_c softmax(up(x)) = argmax_c up(x), and the label map follows from the H/8 x W/8 logits the model ends at
// (CABiNet.forward_lowres).  Three kernels:
//   predict_up_argmax  labels = argmax over classes of the bilinear resize (align_corners=False) of the low-resolution logits;
//                      the staging of eval_chip_accum_kernel with a running (best, arg) in place of the softmax.
//   predict_argmax     labels = argmax over classes of a full-resolution (N, C, H, W) map (the multi-scale / flip path): the
//                      arg-max half of eval_argmax_hist_kernel, without labels, histogram or atomics.
//   predict_render     label -> palette colour, normalised image -> RGB bytes, and the alpha blend of the two, as the reference's
//                      numpy / Pillow lines compute them, byte for byte.
// Every output is a byte array whose start and row starts need not be dword-aligned: dword stores are used only where the
// launcher has checked the alignment, everything else is written byte by byte, and no byte outside the tensor is touched.
#include <stdint.h>

#include "common.hpp"

namespace cabinet {

static const size_t PREDICT_LDS_MAX = 64 * 1024;
#define PREDICT_PX 4  // consecutive pixels of one row per lane

// source columns a segment of `px` output pixels can touch (both taps): the source index grows by rw per pixel
static inline int predict_span(int px, int wl, int W) {
    const float rw = (float)wl / (float)W;
    const int s = (int)ceilf((float)px * rw) + 3;
    return s < wl ? s : wl;
}

// threads per workgroup (a row segment of PREDICT_PX * T pixels) for which the staged source rows fit the LDS; 0: none does
// (a strongly shrinking resize of many classes).  The smallest workgroup that still covers a whole row is preferred.
int predict_up_threads(int C, int wl, int W) {
    int best = 0;
    for (int T = 256; T >= 64; T >>= 1)
        if ((size_t)C * predict_span(PREDICT_PX * T, wl, W) * sizeof(float) <= PREDICT_LDS_MAX && (best == 0 || PREDICT_PX * T >= W))
            best = T;
    return best;
}

// One workgroup per (row segment, output row, image).  The two source rows of every class are lerped vertically into LDS once
// (for the columns this segment touches); each lane then owns PREDICT_PX consecutive pixels and keeps a running (best, arg)
// per pixel.  Strict `>` keeps the lowest index among equal values (torch.argmax).  At ratio 1 both lerp weights are 0 or 1,
// so the logits themselves are compared.  CMAX = 8, 19: C == CMAX with the class loop unrolled; CMAX = 0: any C.
// packed: W % 4 == 0 and `labels` dword-aligned, so the four labels of a lane leave in one dword.
template <int CMAX>
__global__ __launch_bounds__(256) void predict_up_argmax_kernel(const float* __restrict__ a, int Crt, int hl, int wl, int H, int W,
                                                                 float rh, float rw, int span, unsigned char* __restrict__ labels,
                                                                 int packed) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [C][span]
    const int C = CMAX ? CMAX : Crt;
    const int T = blockDim.x, n = blockIdx.z, oy = blockIdx.y;
    const int ox_lo = blockIdx.x * T * PREDICT_PX, ox_hi = min(ox_lo + T * PREDICT_PX, W) - 1;
    const size_t plane = (size_t)hl * wl;
    int ys0, ys1, t0, t1, a_lo, a_hi;
    float ly, tl;
    bilinear_taps(oy, rh, hl, ys0, ys1, ly);
    bilinear_taps(ox_lo, rw, wl, a_lo, t1, tl);
    bilinear_taps(ox_hi, rw, wl, t0, a_hi, tl);
    const int na = min(a_hi - a_lo + 1, span);
    const float* a_n = a + (size_t)n * C * plane;
    for (int i = threadIdx.x; i < C * na; i += T) {
        const int c = i / na, xs = i - c * na;
        const float* p = a_n + (size_t)c * plane + a_lo + xs;
        lds[c * span + xs] = (1.f - ly) * p[ys0 * wl] + ly * p[ys1 * wl];
    }
    __syncthreads();
    const int x = ox_lo + threadIdx.x * PREDICT_PX;
    if (x >= W) return;
    int i0[PREDICT_PX], i1[PREDICT_PX], arg[PREDICT_PX];
    float lx[PREDICT_PX], best[PREDICT_PX];
#pragma unroll
    for (int j = 0; j < PREDICT_PX; ++j) {
        bilinear_taps(min(x + j, W - 1), rw, wl, i0[j], i1[j], lx[j]);
        i0[j] = max(min(i0[j] - a_lo, na - 1), 0), i1[j] = max(min(i1[j] - a_lo, na - 1), 0);
        best[j] = (1.f - lx[j]) * lds[i0[j]] + lx[j] * lds[i1[j]];
        arg[j] = 0;
    }
    if constexpr (CMAX > 0) {
#pragma unroll
        for (int c = 1; c < CMAX; ++c)
#pragma unroll
            for (int j = 0; j < PREDICT_PX; ++j) {
                const float v = (1.f - lx[j]) * lds[c * span + i0[j]] + lx[j] * lds[c * span + i1[j]];
                if (v > best[j]) best[j] = v, arg[j] = c;
            }
    } else {
#pragma unroll 2
        for (int c = 1; c < C; ++c)
#pragma unroll
            for (int j = 0; j < PREDICT_PX; ++j) {
                const float v = (1.f - lx[j]) * lds[c * span + i0[j]] + lx[j] * lds[c * span + i1[j]];
                if (v > best[j]) best[j] = v, arg[j] = c;
            }
    }
    unsigned char* out = labels + ((size_t)n * H + oy) * W + x;
    if (packed) {  // W % 4 == 0: x + 3 < W
        *reinterpret_cast<unsigned*>(out) = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < PREDICT_PX; ++j)
            if (x + j < W) out[j] = (unsigned char)arg[j];
    }
}

hipError_t predict_up_argmax_run(const float* a, int N, int C, int hl, int wl, int H, int W, unsigned char* labels, hipStream_t stream) {
    const int T = predict_up_threads(C, wl, W);
    if (T == 0) return hipErrorInvalidValue;
    const int span = predict_span(PREDICT_PX * T, wl, W);
    const size_t lds = (size_t)C * span * sizeof(float);
    const dim3 grid(ceil_div(W, PREDICT_PX * T), H, N);
    const float rh = (float)hl / (float)H, rw = (float)wl / (float)W;
    const int packed = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(labels) & 3) == 0) ? 1 : 0;
#define PREDICT_UP(CM) \
    hipLaunchKernelGGL((predict_up_argmax_kernel<CM>), grid, dim3(T), lds, stream, a, C, hl, wl, H, W, rh, rw, span, labels, packed)
    if (C == 8)
        PREDICT_UP(8);
    else if (C == 19)
        PREDICT_UP(19);
    else
        PREDICT_UP(0);
#undef PREDICT_UP
    return hipGetLastError();
}

// labels = argmax over classes of total (N, C, P): PREDICT_PX consecutive pixels of one image per lane, grid (groups, N).
// VEC: P % 4 == 0 with `total` 16-byte and `labels` 4-byte aligned -- one 16-byte load per class and one dword store; otherwise
// dword loads and byte stores, the last group of an image cut at P.  CFIX = 8, 19: the class loop unrolled so that a lane's C
// loads are in flight together; CFIX = 0: any C, unrolled by four.
template <bool VEC, int CFIX>
__global__ __launch_bounds__(256) void predict_argmax_kernel(const float* __restrict__ total, int Crt, size_t P,
                                                              unsigned char* __restrict__ labels) {
    const int C = CFIX ? CFIX : Crt;
    const size_t q = ((size_t)blockIdx.x * 256 + threadIdx.x) * PREDICT_PX, n = blockIdx.y;
    if (q >= P) return;
    const float* t = total + n * C * P + q;
    unsigned char* out = labels + n * P + q;
    float best[PREDICT_PX];
    int arg[PREDICT_PX];
    if constexpr (VEC) {
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
        *reinterpret_cast<unsigned*>(out) = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
    } else {
        const int m = (int)(P - q < (size_t)PREDICT_PX ? P - q : (size_t)PREDICT_PX);  // pixels of this group inside the image
        int off[PREDICT_PX];
#pragma unroll
        for (int j = 0; j < PREDICT_PX; ++j) off[j] = min(j, m - 1), best[j] = t[off[j]], arg[j] = 0;
#pragma unroll 4
        for (int c = 1; c < C; ++c)
#pragma unroll
            for (int j = 0; j < PREDICT_PX; ++j) {
                const float u = t[c * P + off[j]];
                if (u > best[j]) best[j] = u, arg[j] = c;
            }
#pragma unroll
        for (int j = 0; j < PREDICT_PX; ++j)
            if (j < m) out[j] = (unsigned char)arg[j];
    }
}

hipError_t predict_argmax_run(const float* total, int N, int C, int H, int W, unsigned char* labels, hipStream_t stream) {
    const size_t P = (size_t)H * W, groups = (P + PREDICT_PX - 1) / PREDICT_PX;
    const dim3 grid((unsigned)((groups + 255) / 256), N);
    const bool vec = P % 4 == 0 && ((reinterpret_cast<uintptr_t>(total) & 15) | (reinterpret_cast<uintptr_t>(labels) & 3)) == 0;
#define PREDICT_ARGMAX(V, CF) hipLaunchKernelGGL((predict_argmax_kernel<V, CF>), grid, dim3(256), 0, stream, total, C, P, labels)
    if (vec) {
        if (C == 8)
            PREDICT_ARGMAX(true, 8);
        else if (C == 19)
            PREDICT_ARGMAX(true, 19);
        else
            PREDICT_ARGMAX(true, 0);
    } else {
        PREDICT_ARGMAX(false, 0);
    }
#undef PREDICT_ARGMAX
    return hipGetLastError();
}

struct RenderConst {
    float mean[3], std[3], alpha;
};

__device__ __forceinline__ unsigned pack4(const unsigned* b) { return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); }

// 12 RGB bytes of four consecutive pixels: three dwords when the array is dword-aligned and the group is whole, else bytes
__device__ __forceinline__ void store_rgb4(unsigned char* __restrict__ base, size_t p0, const unsigned (&b)[12], int m, bool packed) {
    unsigned char* o = base + 3 * p0;
    if (packed && m == 4) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);  // p0 % 4 == 0: 3 * p0 is a multiple of 4
        o4[0] = pack4(b), o4[1] = pack4(b + 4), o4[2] = pack4(b + 8);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < m) o[3 * j] = (unsigned char)b[3 * j], o[3 * j + 1] = (unsigned char)b[3 * j + 1], o[3 * j + 2] = (unsigned char)b[3 * j + 2];
    }
}

// Four consecutive pixels of the flat (N * H * W) pixel array per lane; the palette sits in LDS.
//   pred    = palette[min(label, n_colors - 1)]
//   input   = (uint8) (clip(x * std + mean, 0, 1) * 255): fp32, every product and sum rounded on its own (a fused multiply-add
//             moves values across the truncation), truncated toward zero -- numpy's float32 arithmetic and astype(uint8)
//   overlay = (uint8) ((float) in + alpha * (float) (colour - in)): Pillow's Image.blend for 0 <= alpha <= 1
// lab_packed: labels dword-aligned; out_packed: every output array dword-aligned; img_vec: H * W % 4 == 0 and the image 16-byte
// aligned, so the four pixels are one 16-byte load per channel and never straddle two images.
__global__ __launch_bounds__(256) void predict_render_kernel(const unsigned char* __restrict__ labels, const float* __restrict__ image,
                                                              const unsigned char* __restrict__ palette, int n_colors, RenderConst rc,
                                                              size_t NP, size_t HW, unsigned char* __restrict__ pred,
                                                              unsigned char* __restrict__ inp, unsigned char* __restrict__ ovl,
                                                              int lab_packed, int out_packed, int img_vec) {
    __shared__ unsigned char pal[256 * 3];
    for (int i = threadIdx.x; i < n_colors * 3; i += 256) pal[i] = palette[i];
    __syncthreads();
    const size_t p0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= NP) return;
    const int m = (int)(NP - p0 < (size_t)4 ? NP - p0 : (size_t)4);
    unsigned lab[4];
    if (lab_packed && m == 4) {
        const unsigned u = *reinterpret_cast<const unsigned*>(labels + p0);
#pragma unroll
        for (int j = 0; j < 4; ++j) lab[j] = (u >> (8 * j)) & 255u;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) lab[j] = labels[p0 + min(j, m - 1)];
    }
    unsigned col[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned idx = min(lab[j], (unsigned)(n_colors - 1)) * 3;
        col[3 * j] = pal[idx], col[3 * j + 1] = pal[idx + 1], col[3 * j + 2] = pal[idx + 2];
    }
    store_rgb4(pred, p0, col, m, out_packed);
    if (!image) return;
    unsigned in[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float x[4];
        if (img_vec) {  // NP % 4 == 0 as well: m == 4
            const size_t n = p0 / HW, r = p0 - n * HW;
            const f32x4 v = *reinterpret_cast<const f32x4*>(image + (n * 3 + k) * HW + r);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = v[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t p = p0 + min(j, m - 1), n = p / HW, r = p - n * HW;
                x[j] = image[(n * 3 + k) * HW + r];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = __fadd_rn(__fmul_rn(x[j], rc.std[k]), rc.mean[k]);
            v = fminf(fmaxf(v, 0.f), 1.f);
            in[3 * j + k] = (unsigned)(int)__fmul_rn(v, 255.f);
        }
    }
    if (inp) store_rgb4(inp, p0, in, m, out_packed);
    if (!ovl) return;
    unsigned ov[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const float d = (float)((int)col[i] - (int)in[i]);
        ov[i] = (unsigned)(int)__fadd_rn((float)in[i], __fmul_rn(rc.alpha, d));
    }
    store_rgb4(ovl, p0, ov, m, out_packed);
}

hipError_t predict_render_run(const unsigned char* labels, const float* image, const unsigned char* palette, int n_colors,
                              const float* mean, const float* std, float alpha, int N, int H, int W, unsigned char* pred,
                              unsigned char* inp, unsigned char* ovl, hipStream_t stream) {
    RenderConst rc;
    for (int k = 0; k < 3; ++k) rc.mean[k] = mean ? mean[k] : 0.f, rc.std[k] = std ? std[k] : 1.f;
    rc.alpha = alpha;
    const size_t HW = (size_t)H * W, NP = HW * N, groups = (NP + 3) / 4;
    const uintptr_t outs = reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(inp) | reinterpret_cast<uintptr_t>(ovl);
    const int lab_packed = (reinterpret_cast<uintptr_t>(labels) & 3) == 0, out_packed = (outs & 3) == 0;
    const int img_vec = image && HW % 4 == 0 && (reinterpret_cast<uintptr_t>(image) & 15) == 0;
    hipLaunchKernelGGL(predict_render_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, stream, labels, image, palette,
                       n_colors, rc, NP, HW, pred, inp, ovl, lab_packed, out_packed, img_vec);
    return hipGetLastError();
}

}  // namespace cabinet
