// The tap arithmetic of Pillow's antialiased resample, shared by augment.hip (K18: scale + crop) and augment_warp.hip (K20:
// ResizeIfLarger): a workgroup tile of AUG_TY x AUG_TX output pixels stages the horizontal pass of at most AUG_RS source rows in
// LDS as uint8 -- Pillow's intermediate image -- and takes the vertical pass from there.
#pragma once
#include "../../include/cabinet_hip.h"

namespace cabinet {

#define AUG_TX 64   // tile columns
#define AUG_TY 16   // tile rows
#define AUG_RS 48   // source rows a tile can need: fewer than (AUG_TY + 1) * 2.5 + 1 = 43.5 at the widest resize ratio, 2.5; rounded up
#define AUG_TAPS 5

typedef cabinet_augment_tap AugTap;
static_assert(sizeof(AugTap) == 32, "table layout (include/cabinet_hip.h, cabinet_amd/augment.py)");

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// a tap as the kernels use it: at most AUG_TAPS of them, all inside [0, size)
__device__ __forceinline__ AugTap load_tap(const AugTap* p, int size) {
    AugTap t = *p;
    t.n = min(max(t.n, 0), AUG_TAPS);
    t.first = min(max(t.first, 0), size - 1);
    t.step = t.step < 0 ? -1 : 1;
    return t;
}

// the source rows [lo, lo + span) that the row taps rtap[0 .. rows) read, span clamped to AUG_RS for memory safety alone
__device__ __forceinline__ void tap_rows_span(const AugTap* rtap, int rows, int H, int& lo, int& span) {
    int hi = 0;
    lo = H - 1;
    for (int j = 0; j < rows; ++j) {
        const int a = rtap[j].first, b = min(max(a + rtap[j].step * (max(rtap[j].n, 1) - 1), 0), H - 1);
        lo = min(lo, min(a, b)), hi = max(hi, max(a, b));
    }
    span = min(hi - lo + 1, AUG_RS);
}

// horizontal pass: one output pixel of the interleaved RGB source row `src` (W pixels): clip8((2^21 + sum coef * in) >> 22)
__device__ __forceinline__ void tap_horizontal(const unsigned char* __restrict__ src, const AugTap& c, int W, unsigned char* out3) {
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
    for (int k = 0; k < AUG_TAPS; ++k)
        if (k < c.n) {
            const unsigned char* p = src + (size_t)min(max(c.first + c.step * k, 0), W - 1) * 3;
            acc[0] += c.coef[k] * (int)p[0], acc[1] += c.coef[k] * (int)p[1], acc[2] += c.coef[k] * (int)p[2];
        }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out3[ch] = (unsigned char)clip8(acc[ch] >> 22);
}

// vertical pass over the staged rows (row r of `hrow` is source row lo + r) at byte column col3
__device__ __forceinline__ void tap_vertical(const unsigned char (*hrow)[AUG_TX * 3], int col3, const AugTap& v, int lo, int span,
                                             int (&px)[3]) {
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
    for (int k = 0; k < AUG_TAPS; ++k)
        if (k < v.n) {
            const unsigned char* p = &hrow[min(max(v.first + v.step * k - lo, 0), span - 1)][col3];
            acc[0] += v.coef[k] * (int)p[0], acc[1] += v.coef[k] * (int)p[1], acc[2] += v.coef[k] * (int)p[2];
        }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) px[ch] = clip8(acc[ch] >> 22);
}

}  // namespace cabinet
