// K20 -- the geometric steps the reference's aerial datasets (src/datasets/uavid.py:192-230, vdd.py, aeroscapes.py) run ahead of
// RandomScale, as batched passes from uint8 to uint8, byte for byte with Pillow (include/cabinet_hip.h, cabinet_augment_warp_desc):
//   augment_warp_kernel    Image.transform(size, AFFINE, a, BILINEAR) for the image, NEAREST with a fill for the label, the source
//                          read through optional flips.  RandomTranslate (with both flips folded in) and RandomRotate(expand=True)
//                          are one launch each.  One output pixel per thread, 32 x 8 pixels per workgroup: a tile close to square
//                          keeps the bilinear gather of a rotated tile (|angle| <= 45 degrees) inside a few cache lines per row,
//                          and a wavefront writes two runs of 96 consecutive bytes.  No LDS.
//   augment_resize_kernel  ResizeIfLarger: Pillow's two-pass antialiased resize, the tile scheme and tap arithmetic of
//                          augment_geom_kernel (augment_taps.hpp), the label through nearest-index tables.
// Grid z is the sample and x, y cover the batch's largest output: a workgroup outside its own sample's extent exits at once.
// Every output byte of a sample's extent is written, fill included; every source index is clamped where it is used.
#include <stdint.h>

#include "../../include/cabinet_hip.h"
#include "common.hpp"
#include "augment_taps.hpp"

namespace cabinet {

typedef cabinet_augment_warp_desc WarpDesc;
static_assert(sizeof(WarpDesc) == 192, "descriptor layout (include/cabinet_hip.h, cabinet_amd/augment.py)");

#define WARP_TX 32
#define WARP_TY 8

// Pillow's BILINEAR(v, a, b, d): double, each operation rounded on its own
__device__ __forceinline__ double lerp_rn(double a, double b, double d) { return __dadd_rn(a, __dmul_rn(__dsub_rn(b, a), d)); }

__global__ __launch_bounds__(256) void augment_warp_kernel(const unsigned char* __restrict__ descs) {
    const WarpDesc* D = reinterpret_cast<const WarpDesc*>(descs) + blockIdx.z;
    const int ow = D->out_w, oh = D->out_h;
    if ((int)(blockIdx.x * WARP_TX) >= ow || (int)(blockIdx.y * WARP_TY) >= oh) return;
    const int x = blockIdx.x * WARP_TX + (threadIdx.x & (WARP_TX - 1)), y = blockIdx.y * WARP_TY + (threadIdx.x >> 5);
    if (x >= ow || y >= oh) return;
    const int H = D->H, W = D->W;
    const bool fx = (D->flip & CABINET_WARP_FLIP_X) != 0, fy = (D->flip & CABINET_WARP_FLIP_Y) != 0;
    const unsigned char* __restrict__ img = D->src_image;
    const unsigned char* __restrict__ lab = D->src_label;

    // image
    const double xh = __dadd_rn((double)x, 0.5), yh = __dadd_rn((double)y, 0.5);
    const double xin = __dadd_rn(__dadd_rn(__dmul_rn(D->a[0], xh), __dmul_rn(D->a[1], yh)), D->a[2]);
    const double yin = __dadd_rn(__dadd_rn(__dmul_rn(D->a[3], xh), __dmul_rn(D->a[4], yh)), D->a[5]);
    int px[3] = {0, 0, 0};
    if (!(xin < 0.0) && xin < (double)W && !(yin < 0.0) && yin < (double)H) {  // a NaN from a wrong matrix fails these and stays fill
        const double xs = __dsub_rn(xin, 0.5), ys = __dsub_rn(yin, 0.5);
        const double xfl = floor(xs), yfl = floor(ys);
        const double dx = __dsub_rn(xs, xfl), dy = __dsub_rn(ys, yfl);
        const int xf = (int)xfl, yf = (int)yfl;
        int c0 = min(max(xf, 0), W - 1), c1 = min(max(xf + 1, 0), W - 1);
        int r0 = min(max(yf, 0), H - 1);
        const bool below = yf + 1 >= 0 && yf + 1 < H;
        int r1 = min(max(yf + 1, 0), H - 1);
        if (fx) c0 = W - 1 - c0, c1 = W - 1 - c1;
        if (fy) r0 = H - 1 - r0, r1 = H - 1 - r1;
        const unsigned char* p00 = img + ((size_t)r0 * W + c0) * 3;
        const unsigned char* p01 = img + ((size_t)r0 * W + c1) * 3;
        const unsigned char* p10 = img + ((size_t)r1 * W + c0) * 3;
        const unsigned char* p11 = img + ((size_t)r1 * W + c1) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double v1 = lerp_rn((double)p00[ch], (double)p01[ch], dx);
            const double v2 = below ? lerp_rn((double)p10[ch], (double)p11[ch], dx) : v1;
            px[ch] = (int)lerp_rn(v1, v2, dy) & 255;  // (UINT8) of a value in [0, 255]
        }
    }
    unsigned char* o = D->dst_image + ((size_t)y * ow + x) * 3;
    o[0] = (unsigned char)px[0], o[1] = (unsigned char)px[1], o[2] = (unsigned char)px[2];

    // label
    long long lc, lr;
    if (D->label_mode == CABINET_WARP_LABEL_FIXED) {
        lc = (D->fix[2] + (long long)y * D->fix[1] + (long long)x * D->fix[0]) >> 16;
        lr = (D->fix[5] + (long long)y * D->fix[4] + (long long)x * D->fix[3]) >> 16;
    } else {
        lc = reinterpret_cast<const int*>(descs + D->lab_col)[x];
        lr = reinterpret_cast<const int*>(descs + D->lab_row)[y];
    }
    int id = D->fill;
    if (lc >= 0 && lc < W && lr >= 0 && lr < H) {
        const int c = fx ? W - 1 - (int)lc : (int)lc, r = fy ? H - 1 - (int)lr : (int)lr;
        id = lab[(size_t)r * W + c];
    }
    D->dst_label[(size_t)y * ow + x] = (unsigned char)id;
}

__global__ __launch_bounds__(256) void augment_resize_kernel(const unsigned char* __restrict__ descs) {
    __shared__ unsigned char hrow[AUG_RS][AUG_TX * 3];
    __shared__ AugTap rtap[AUG_TY];
    const WarpDesc* D = reinterpret_cast<const WarpDesc*>(descs) + blockIdx.z;
    const int ow = D->out_w, oh = D->out_h;
    const int t = threadIdx.x, x0 = blockIdx.x * AUG_TX, y0 = blockIdx.y * AUG_TY;
    if (x0 >= ow || y0 >= oh) return;  // uniform per workgroup
    const int H = D->H, W = D->W;
    const unsigned char* __restrict__ img = D->src_image;
    const AugTap* row_taps = reinterpret_cast<const AugTap*>(descs + D->row_taps);
    const AugTap* col_taps = reinterpret_cast<const AugTap*>(descs + D->col_taps);
    const int rows = min(AUG_TY, oh - y0);
    if (t < rows) rtap[t] = load_tap(row_taps + y0 + t, H);
    __syncthreads();
    int lo, span;
    tap_rows_span(rtap, rows, H, lo, span);

    const int col = t & (AUG_TX - 1), x = x0 + col;
    const bool live = x < ow;
    if (live) {
        const AugTap c = load_tap(col_taps + x, W);
        for (int r = t >> 6; r < span; r += 4) tap_horizontal(img + (size_t)(lo + r) * W * 3, c, W, &hrow[r][col * 3]);
    }
    __syncthreads();
    if (live) {
        const int lc = min(max(reinterpret_cast<const int*>(descs + D->lab_col)[x], 0), W - 1);
        const int* lab_row = reinterpret_cast<const int*>(descs + D->lab_row);
        const unsigned char* __restrict__ lab = D->src_label;
        for (int j = t >> 6; j < rows; j += 4) {
            const int y = y0 + j;
            int px[3];
            tap_vertical(hrow, col * 3, rtap[j], lo, span, px);
            unsigned char* o = D->dst_image + ((size_t)y * ow + x) * 3;
            o[0] = (unsigned char)px[0], o[1] = (unsigned char)px[1], o[2] = (unsigned char)px[2];
            const int lr = min(max(lab_row[y], 0), H - 1);
            D->dst_label[(size_t)y * ow + x] = lab[(size_t)lr * W + lc];
        }
    }
}

hipError_t augment_warp_run(const void* descs, int N, int max_oh, int max_ow, hipStream_t stream) {
    const dim3 grid(ceil_div(max_ow, WARP_TX), ceil_div(max_oh, WARP_TY), N);
    hipLaunchKernelGGL(augment_warp_kernel, grid, dim3(256), 0, stream, static_cast<const unsigned char*>(descs));
    return hipGetLastError();
}

hipError_t augment_resize_run(const void* descs, int N, int max_oh, int max_ow, hipStream_t stream) {
    const dim3 grid(ceil_div(max_ow, AUG_TX), ceil_div(max_oh, AUG_TY), N);
    hipLaunchKernelGGL(augment_resize_kernel, grid, dim3(256), 0, stream, static_cast<const unsigned char*>(descs));
    return hipGetLastError();
}

}  // namespace cabinet
