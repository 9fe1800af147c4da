// K18 -- the training augmentation of the reference's Cityscapes dataset (src/datasets/cityscapes.py:114-136 and :102-109 with
// src/datasets/transform.py: RandomHorizontalFlip, RandomScale, RandomCrop, RandomColorJitter, RandomGrayscale, RandomGamma,
// RandomNoise, RandomCutout; ToTensor / Normalize; convert_labels), for a batch, byte for byte.
//
// Everything geometric arrives in per-sample tables the host builds (include/cabinet_hip.h, cabinet_augment_sample): per output
// column and row the source taps of Pillow's antialiased bilinear resample with 22-bit integer coefficients -- flip, crop
// window and reflect padding already folded in -- and the label's source index.  Two kernels, because the contrast blend needs
// the mean luma of the WHOLE brightened crop:
//   augment_geom   one workgroup per 16 x 64 tile of the crop: the horizontal pass of the source rows the tile needs, once, into
//                  LDS (uint8, as Pillow's intermediate image); the vertical pass from there; the brightness blend; the uint8
//                  crop to the workspace; the label through index tables and the id -> trainId table as int64; the tile's sum
//                  of luma as one 64-bit partial (every partial is written by every call: nothing to zero, no atomics).
//   augment_photo  prologue: m = (int)(sum of the sample's partials / (th tw) + 0.5) in double.  Per pixel: contrast blend
//                  against m, colour blend against the pixel's own luma, gray, gamma table, noise, cutout, normalise; fp32 NCHW,
//                  four consecutive pixels of a plane per lane (one 16-byte store per plane where the address allows it), and
//                  the final bytes to an optional uint8 NHWC array.
// No byte outside a source array is read (every table index is clamped into its array) and no byte outside an output written.
#include <stdint.h>

#include "../../include/cabinet_hip.h"
#include "common.hpp"
#include "augment_taps.hpp"

namespace cabinet {

typedef cabinet_augment_sample AugSample;

static_assert(sizeof(AugSample) == 2400, "table layout (include/cabinet_hip.h, cabinet_amd/augment.py)");

int augment_tiles(int th, int tw) { return ceil_div(th, AUG_TY) * ceil_div(tw, AUG_TX); }
static size_t augment_crop_stride(int th, int tw) { return align_up((size_t)th * tw * 3, 16); }
size_t augment_workspace(int N, int th, int tw) {
    return align_up((size_t)N * augment_crop_stride(th, tw), 256) + (size_t)N * augment_tiles(th, tw) * sizeof(unsigned long long);
}

// Pillow's L of an RGB pixel
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Pillow's Image.blend(deg, src, r): fp32, every operation rounded on its own, truncated; outside 0 <= r <= 1 clipped first
__device__ __forceinline__ int blend8(int deg, int src, float r, bool inside) {
    const float t = __fadd_rn((float)deg, __fmul_rn(r, (float)(src - deg)));
    if (inside) return (int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// RandomHSV on one pixel (K20): Pillow's RGB -> HSV bytes, the three byte tables (H at 0, S at 256, V at 512), Pillow's HSV -> RGB.
// fp32 where Pillow's C uses float, double where its expressions promote; every operation rounded on its own.
__device__ __forceinline__ void hsv_pixel(const unsigned char* __restrict__ lut, int (&px)[3]) {
    const int r = px[0], g = px[1], b = px[2];
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int h8 = 0, s8 = 0;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float s = __fdiv_rn(cr, (float)maxc);
        const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr), bc = __fdiv_rn((float)(maxc - b), cr);
        float h;
        if (r == maxc) h = __fsub_rn(bc, gc);
        else if (g == maxc) h = (float)__dsub_rn(__dadd_rn(2.0, (double)rc), (double)bc);
        else h = (float)__dsub_rn(__dadd_rn(4.0, (double)gc), (double)rc);
        const double u = __dadd_rn(__ddiv_rn((double)h, 6.0), 1.0);  // in (0.8, 2): fmod(u, 1) = u - floor(u), exact
        h = (float)__dsub_rn(u, floor(u));
        h8 = clip8((int)__dmul_rn((double)h, 255.0));
        s8 = clip8((int)__dmul_rn((double)s, 255.0));
    }
    const int H = lut[h8], S = lut[256 + s8], V = lut[512 + maxc];
    if (S == 0) {
        px[0] = px[1] = px[2] = V;
        return;
    }
    const double hh = __ddiv_rn(__dmul_rn((double)H, 6.0), 255.0);
    const double fl = floor(hh);
    const float f = (float)__dsub_rn(hh, fl);
    const float fs = (float)__ddiv_rn((double)S, 255.0);
    const double v = (double)V;
    const int p = clip8((int)round(__dmul_rn(v, __dsub_rn(1.0, (double)fs))));
    const int q = clip8((int)round(__dmul_rn(v, __dsub_rn(1.0, __dmul_rn((double)fs, (double)f)))));
    const int tt = clip8((int)round(__dmul_rn(v, __dsub_rn(1.0, __dmul_rn((double)fs, __dsub_rn(1.0, (double)f))))));
    switch ((int)fl % 6) {
        case 0: px[0] = V, px[1] = tt, px[2] = p; break;
        case 1: px[0] = q, px[1] = V, px[2] = p; break;
        case 2: px[0] = p, px[1] = V, px[2] = tt; break;
        case 3: px[0] = p, px[1] = q, px[2] = V; break;
        case 4: px[0] = tt, px[1] = p, px[2] = V; break;
        default: px[0] = V, px[1] = p, px[2] = q; break;
    }
}

__global__ __launch_bounds__(256) void augment_geom_kernel(const unsigned char* __restrict__ table, int th, int tw,
                                                            unsigned char* __restrict__ crop, size_t crop_stride,
                                                            long long* __restrict__ out_label, unsigned long long* __restrict__ partials) {
    __shared__ unsigned char hrow[AUG_RS][AUG_TX * 3];
    __shared__ AugTap rtap[AUG_TY];
    __shared__ unsigned red[4];
    __shared__ unsigned char hsvt[768];  // RandomHSV's H, S and V byte tables (CABINET_AUGMENT_HSV)
    const int t = threadIdx.x, n = blockIdx.z;
    const int x0 = blockIdx.x * AUG_TX, y0 = blockIdx.y * AUG_TY;
    const AugSample* S = reinterpret_cast<const AugSample*>(table) + n;
    const int H = S->H, W = S->W;
    const unsigned char* __restrict__ img = S->image;
    const AugTap* row_taps = reinterpret_cast<const AugTap*>(table + S->row_taps);
    const AugTap* col_taps = reinterpret_cast<const AugTap*>(table + S->col_taps);
    const int rows = min(AUG_TY, th - y0);
    if (t < rows) rtap[t] = load_tap(row_taps + y0 + t, H);
    const bool hsv = (S->flags & CABINET_AUGMENT_HSV) != 0;  // uniform per sample: a scalar branch
    if (hsv) {
        const unsigned char* g = table + (size_t)max(S->reserved, 0);
        for (int i = t; i < 768; i += 256) hsvt[i] = g[i];
    }
    __syncthreads();
    int lo, span;  // source rows this tile reads; coverage (in/out <= 2.5) keeps the span <= 43
    tap_rows_span(rtap, rows, H, lo, span);

    const int col = t & (AUG_TX - 1), x = x0 + col;
    const bool live = x < tw;
    if (live) {  // horizontal pass: source rows lo .. lo + span - 1 at this thread's column
        const AugTap c = load_tap(col_taps + x, W);
        for (int r = t >> 6; r < span; r += 4) {
            tap_horizontal(img + (size_t)(lo + r) * W * 3, c, W, &hrow[r][col * 3]);
        }
    }
    __syncthreads();

    unsigned sum = 0;  // at most 4 pixels x 255 per thread
    if (live) {
        const float rb = S->brightness;
        const bool inside = rb >= 0.f && rb <= 1.f;
        const int lc = reinterpret_cast<const int*>(table + S->lab_col)[x];
        const int* lab_row = reinterpret_cast<const int*>(table + S->lab_row);
        const unsigned char* __restrict__ lab = S->label;
        for (int j = t >> 6; j < rows; j += 4) {
            const int y = y0 + j;
            const AugTap v = rtap[j];
            int px[3];
            tap_vertical(hrow, col * 3, v, lo, span, px);
            if (hsv) hsv_pixel(hsvt, px);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) px[ch] = blend8(0, px[ch], rb, inside);
            sum += (unsigned)luma(px[0], px[1], px[2]);
            unsigned char* o = crop + (size_t)n * crop_stride + ((size_t)y * tw + x) * 3;
            o[0] = (unsigned char)px[0], o[1] = (unsigned char)px[1], o[2] = (unsigned char)px[2];
            const int lr = lab_row[y];
            long long id = S->ignore_label;
            if (lr >= 0 && lc >= 0) id = S->label_lut[lab[(size_t)min(lr, H - 1) * W + min(lc, W - 1)]];
            out_label[((size_t)n * th + y) * tw + x] = id;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((t & 63) == 0) red[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[(size_t)n * gridDim.x * gridDim.y + tile] = (unsigned long long)red[0] + red[1] + red[2] + red[3];
    }
}

struct AugNorm {
    float mean[3], std[3];
};

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1)
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (unsigned)p1, c[3] = (unsigned)p0, c[0] = n0, c[2] = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// three standard normals of pixel p of sample n: one Philox block keyed by the seed, counter (p, n), Box-Muller on its two pairs
__device__ __forceinline__ void normal3(unsigned long long seed, unsigned n, unsigned long long p, float (&z)[3]) {
    unsigned c[4] = {(unsigned)p, (unsigned)(p >> 32), n, 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    const float u0 = ((float)(c[0] >> 8) + 0.5f) * 5.9604644775390625e-8f, u1 = ((float)(c[1] >> 8) + 0.5f) * 5.9604644775390625e-8f;  // (0, 1)
    const float u2 = ((float)(c[2] >> 8) + 0.5f) * 5.9604644775390625e-8f, u3 = ((float)(c[3] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float r0 = sqrtf(-2.f * logf(u0)), r1 = sqrtf(-2.f * logf(u2));
    z[0] = r0 * cosf(6.283185307179586f * u1), z[1] = r0 * sinf(6.283185307179586f * u1), z[2] = r1 * cosf(6.283185307179586f * u3);
}

__global__ __launch_bounds__(256) void augment_photo_kernel(const unsigned char* __restrict__ table, int th, int tw,
                                                             const unsigned char* __restrict__ crop, size_t crop_stride,
                                                             const unsigned long long* __restrict__ partials, int tiles,
                                                             const float* __restrict__ noise, unsigned long long seed, AugNorm nc,
                                                             float* __restrict__ out_image, unsigned char* __restrict__ out_u8) {
    __shared__ unsigned long long red[4];
    __shared__ unsigned char glut[256];
    const int t = threadIdx.x, n = blockIdx.y;
    const AugSample* S = reinterpret_cast<const AugSample*>(table) + n;
    unsigned long long s = 0;
    for (int i = t; i < tiles; i += 256) s += partials[(size_t)n * tiles + i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((t & 63) == 0) red[t >> 6] = s;
    glut[t] = S->gamma_lut[t];
    __syncthreads();
    const size_t P = (size_t)th * tw;
    const int m = (int)((double)(red[0] + red[1] + red[2] + red[3]) / (double)P + 0.5);

    const size_t p0 = ((size_t)blockIdx.x * 256 + t) * 4;
    if (p0 >= P) return;
    const int cnt = (int)(P - p0 < (size_t)4 ? P - p0 : (size_t)4);
    const float rc = S->contrast, rs = S->saturation;
    const bool c_in = rc >= 0.f && rc <= 1.f, s_in = rs >= 0.f && rs <= 1.f;
    const int flags = S->flags;
    const int cy = S->cut_y, cx = S->cut_x, cs = S->cut_size;
    const float nscale = S->noise_scale;

    unsigned b[12];
    const unsigned char* src = crop + (size_t)n * crop_stride + p0 * 3;  // crop_stride % 16 == 0 and p0 % 4 == 0: dword-aligned
    if (cnt == 4) {
        const unsigned* s4 = reinterpret_cast<const unsigned*>(src);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const unsigned u = s4[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[4 * i + j] = (u >> (8 * j)) & 255u;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) b[i] = src[min(i, cnt * 3 - 1)];
    }
    float o[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const size_t p = p0 + j;
        int v[3] = {(int)b[3 * j], (int)b[3 * j + 1], (int)b[3 * j + 2]};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = blend8(m, v[ch], rc, c_in);
        const int L = luma(v[0], v[1], v[2]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = blend8(L, v[ch], rs, s_in);
        if (flags & CABINET_AUGMENT_GRAY) v[0] = v[1] = v[2] = luma(v[0], v[1], v[2]);
        if (flags & CABINET_AUGMENT_GAMMA) v[0] = glut[v[0]], v[1] = glut[v[1]], v[2] = glut[v[2]];
        if ((flags & CABINET_AUGMENT_NOISE) && j < cnt) {
            float z[3];
            if (noise) {
                const float* q = noise + ((size_t)n * P + p) * 3;
                z[0] = q[0], z[1] = q[1], z[2] = q[2];
            } else {
                normal3(seed, (unsigned)n, p, z);
                z[0] = __fmul_rn(z[0], nscale), z[1] = __fmul_rn(z[1], nscale), z[2] = __fmul_rn(z[2], nscale);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = (int)fmin(fmax((double)v[ch] + (double)z[ch], 0.0), 255.0);
        }
        if (flags & CABINET_AUGMENT_CUTOUT) {
            const int y = (int)(p / (size_t)tw), x = (int)(p - (size_t)y * tw);
            if (y >= cy && y < cy + cs && x >= cx && x < cx + cs) v[0] = v[1] = v[2] = 0;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            b[3 * j + ch] = (unsigned)v[ch];
            o[ch][j] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)v[ch], 255.f), nc.mean[ch]), nc.std[ch]);
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float* dst = out_image + ((size_t)n * 3 + ch) * P + p0;
        if (cnt == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            *reinterpret_cast<f32x4*>(dst) = f32x4{o[ch][0], o[ch][1], o[ch][2], o[ch][3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) dst[j] = o[ch][j];
        }
    }
    if (out_u8) {
        unsigned char* d = out_u8 + ((size_t)n * P + p0) * 3;
        if (cnt == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
            unsigned* d4 = reinterpret_cast<unsigned*>(d);
#pragma unroll
            for (int i = 0; i < 3; ++i) d4[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i)
                if (i < cnt * 3) d[i] = (unsigned char)b[i];
        }
    }
}

hipError_t augment_run(const void* samples, int N, int th, int tw, const float* noise, unsigned long long seed, const float* mean,
                       const float* std, float* out_image, long long* out_label, unsigned char* out_u8, void* workspace,
                       hipStream_t stream) {
    const unsigned char* table = static_cast<const unsigned char*>(samples);
    unsigned char* crop = static_cast<unsigned char*>(workspace);
    const size_t crop_stride = augment_crop_stride(th, tw);
    unsigned long long* partials = reinterpret_cast<unsigned long long*>(crop + align_up((size_t)N * crop_stride, 256));
    const int tiles = augment_tiles(th, tw);
    const dim3 ggrid(ceil_div(tw, AUG_TX), ceil_div(th, AUG_TY), N);
    hipLaunchKernelGGL(augment_geom_kernel, ggrid, dim3(256), 0, stream, table, th, tw, crop, crop_stride, out_label, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    AugNorm nc;
    for (int k = 0; k < 3; ++k) nc.mean[k] = mean[k], nc.std[k] = std[k];
    const size_t groups = ((size_t)th * tw + 3) / 4;
    hipLaunchKernelGGL(augment_photo_kernel, dim3((unsigned)((groups + 255) / 256), N), dim3(256), 0, stream, table, th, tw, crop,
                       crop_stride, partials, tiles, noise, seed, nc, out_image, out_u8);
    return hipGetLastError();
}

}  // namespace cabinet
