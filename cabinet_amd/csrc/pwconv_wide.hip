// K14 -- weight gradient of the WIDE pointwise (1x1, bias-free, stride 1) convolutions, NCHW fp32, no layout copy.
//
// Serves the 1x1 convolutions K10 (pwconv.hip) leaves to the stock operator: the projection of features.4, every 1x1 of
// features.5 .. features.15, the closing backbone.conv and the spatial branch's conv_out (reference src/models/
// mobilenetv3.py:128-131,144-151,193 and cabinet.py:114).  MIOpen computes these weight gradients with an NHWC implicit-GEMM
// kernel and first copies x and dy from NCHW to NHWC; the product itself
//     dW[co][ci] = sum_{b,p} dY[b][co][p] * X[b][ci][p]
// contracts over pixels, the contiguous axis of BOTH operands in NCHW, so nothing has to be transposed.
//
//   tile    : a workgroup (4 waves) owns a (32 BM) x (32 BN) block of dW and a contiguous run of 64-pixel chunks (split-K over
//             (image, pixel chunk)).  Every wave holds the WHOLE tile in its accumulators (BM x BN blocks of 32 x 32, exact-fp32
//             MFMA 32x32x2) and multiplies its own quarter of each chunk's pixels: the four waves are balanced whatever the
//             channel counts are.  Rows past Co / Ci are staged as zeros (skipping their MFMAs under a wave-uniform branch
//             cost 60 vector registers and with them the second resident workgroup); the host picks the tile shape.
//   staging : the 32 (BM + BN) rows of the chunk go global -> registers -> LDS as whole 256-byte row segments, [row][68]
//             floats; the registers of chunk k+1 are loaded before chunk k is multiplied.  A lane reads its MFMA operands as
//             one ds_read_b128 (4 consecutive pixels of its row): stride 68 puts the 16 lanes of every b128 lane group on 64
//             distinct banks, and the dword stores of a row walk consecutive banks.
//   output  : the four partial tiles are added in wave order through the LDS (all threads), one slab per split; an ordered slab sum
//             (no atomics) gives dW.  Bit-reproducible; no allocation, no host synchronisation.
#include "common.hpp"
#include "slab_sum.hpp"

namespace cabinet {

constexpr int PWW_KC = 64;           // pixels per staged chunk
constexpr int PWW_LD = 68;           // LDS row stride (floats)
constexpr int PWW_TARGET_WG = 512;   // two resident workgroups on each of the 256 CUs
constexpr int PWW_MAX_C = 4096;
constexpr int PWW_MAX_P = 1 << 21;    // 48 row offsets of 16 P bytes stay below 2^31
constexpr int PWW_OOB = 0x40000000;  // byte offset beyond every buffer resource (one image's operand is at most 1 GB)

template <int BM, int BN>
__device__ __forceinline__ void pww_multiply(const float* __restrict__ tl, int kb, int li,
                                             f32x16 (&acc)[BM][BN]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        f32x4 a[BM], b[BN];
#pragma unroll
        for (int i = 0; i < BM; ++i) a[i] = *reinterpret_cast<const f32x4*>(tl + (32 * i + li) * PWW_LD + kb + 8 * s);
#pragma unroll
        for (int j = 0; j < BN; ++j)
            b[j] = *reinterpret_cast<const f32x4*>(tl + (32 * (BM + j) + li) * PWW_LD + kb + 8 * s);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < BM; ++i)
#pragma unroll
                for (int j = 0; j < BN; ++j)
                    acc[i][j] = mfma32(a[i][q], b[j][q], acc[i][j]);
    }
}

template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void pww_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, int Co,
                                                        int Ci, int P, int nchunks, int chunks_per_img, int tiles_n,
                                                        int ntiles, int nsplit, float* __restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) float tl[];  // [32 (BM + BN)][68]; reused for the wave reduction
    constexpr int RPT = 8 * (BM + BN);                          // rows staged per thread: row = wave + 4 j
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
    const int lin = xcd_chunked_tile(blockIdx.x, gridDim.x);  // the tiles of one split share an XCD's L2
    const int split = lin / ntiles, tile = lin - split * ntiles;
    const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
    const int co0 = 32 * BM * tm, ci0 = 32 * BN * tn;
    const int c_begin = (int)((long long)split * nchunks / nsplit), c_end = (int)((long long)(split + 1) * nchunks / nsplit);

    f32x16 acc[BM][BN];
#pragma unroll
    for (int i = 0; i < BM; ++i)
#pragma unroll
        for (int j = 0; j < BN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // wave-uniform row bases + one lane offset: a buffer load per row with a SCALAR row offset (48 rows in flight would
    // otherwise hold 48 64-bit addresses in vector registers)
    const int wrow = __builtin_amdgcn_readfirstlane(wave);
    float v[RPT];
    auto load = [&](int c) {
        const int b = c / chunks_per_img, p0 = (c - b * chunks_per_img) * PWW_KC;
        // no predicates: a lane past the plane gets an offset beyond every resource, rows past Co / Ci lie beyond this
        // resource's records -- the range check (it covers lane + scalar offset) loads both as 0
        const int voff = p0 + lane < P ? lane * 4 : PWW_OOB;
        const int rows_y = Co - co0 - wrow, rows_x = Ci - ci0 - wrow;  // rows left from this wave's first one
        const buf_rsrc ry = make_rsrc(dy + ((size_t)b * Co + co0 + wrow) * P + p0,
                                      rows_y > 0 ? (unsigned)(((size_t)(rows_y - 1) * P + (P - p0)) * sizeof(float)) : 0u);
        const buf_rsrc rx = make_rsrc(x + ((size_t)b * Ci + ci0 + wrow) * P + p0,
                                      rows_x > 0 ? (unsigned)(((size_t)(rows_x - 1) * P + (P - p0)) * sizeof(float)) : 0u);
        const int row_bytes = 4 * P * (int)sizeof(float);
#pragma unroll
        for (int j = 0; j < 8 * BM; ++j) v[j] = bload(ry, voff, j * row_bytes);
#pragma unroll
        for (int j = 0; j < 8 * BN; ++j) v[8 * BM + j] = bload(rx, voff, j * row_bytes);
    };

    const int kb = 16 * wave + 4 * h;  // this lane's first pixel column of the chunk (then + 8 s, + q)
    if (c_begin < c_end) load(c_begin);
    for (int c = c_begin; c < c_end; ++c) {
        __syncthreads();  // the previous chunk's operand reads are done
#pragma unroll
        for (int j = 0; j < RPT; ++j) tl[(wave + 4 * j) * PWW_LD + lane] = v[j];
        __syncthreads();
        if (c + 1 < c_end) load(c + 1);  // in flight while this chunk is multiplied
        pww_multiply<BM, BN>(tl, kb, li, acc);
    }

    // The four partial tiles, one 32 x 32 block at a time through the LDS: every wave parks its copy [wave][register][lane],
    // then all 256 threads add the four copies in wave order -- four neighbouring columns each, one ds_read_b128 per copy --
    // and store 16 bytes of the split's slab (128-byte row segments).  Everybody works: a wave-by-wave chain through the
    // LDS with wave 0 storing the whole tile took 10 us of a 40 us kernel.
    float* slab = slabs + (size_t)split * Co * Ci;
    const int rr = tid >> 4, c4 = 4 * (tid & 15);  // this thread's accumulator register (row) and first lane (column)
    const int row_in = (rr & 3) + 8 * (rr >> 2) + 4 * (c4 >> 5), col_in = c4 & 31;
#pragma unroll
    for (int i = 0; i < BM; ++i)
#pragma unroll
        for (int j = 0; j < BN; ++j) {
            __syncthreads();  // the operand reads / the previous block's sums are done
#pragma unroll
            for (int r = 0; r < 16; ++r) tl[(wave * 16 + r) * 64 + lane] = acc[i][j][r];
            __syncthreads();
            f32x4 t = *reinterpret_cast<const f32x4*>(tl + rr * 64 + c4);
#pragma unroll
            for (int w = 1; w < 4; ++w) t += *reinterpret_cast<const f32x4*>(tl + (w * 16 + rr) * 64 + c4);
            const int co = co0 + 32 * i + row_in, ci = ci0 + 32 * j + col_in;  // Ci % 8 == 0: four columns live or none
            if (co < Co && ci < Ci) *reinterpret_cast<f32x4*>(slab + (size_t)co * Ci + ci) = t;
        }
}

// ------------------------------------------------------------------------------------------------ host side
struct PwwPlan {
    int bm, bn, tiles_m, tiles_n, nsplit, nchunks, cpi;
};

// Tile shape: per tile and chunk the MFMAs take 512 BM BN cycles of the CU and the staged rows 8 KB (BM + BN), which is
// 768 (BM + BN) cycles at the ~10 B/clk/CU an L2-fed CU sustains: the cheapest (BM, BN) over all tiles, then the fewest tiles.
static PwwPlan pww_plan(int B, int Ci, int Co, int P) {
    static const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {1, 3}, {3, 1}, {2, 3}, {3, 2}, {1, 4}, {4, 1},
                                    {2, 4}, {4, 2}, {3, 3}};
    const int cob = ceil_div(Co, 32), cib = ceil_div(Ci, 32);
    PwwPlan best{};
    long best_cost = -1, best_tiles = 0;
    for (const auto& s : shapes) {
        const int tm = ceil_div(cob, s[0]), tn = ceil_div(cib, s[1]);
        const int mfma = 2 * s[0] * s[1], rows = 3 * (s[0] + s[1]);
        const long tiles = (long)tm * tn, cost = tiles * (mfma > rows ? mfma : rows);
        if (best_cost < 0 || cost < best_cost || (cost == best_cost && tiles < best_tiles)) {
            best_cost = cost, best_tiles = tiles;
            best.bm = s[0], best.bn = s[1], best.tiles_m = tm, best.tiles_n = tn;
        }
    }
    best.cpi = ceil_div(P, PWW_KC);
    best.nchunks = B * best.cpi;
    const int ntiles = best.tiles_m * best.tiles_n;
    int ns = PWW_TARGET_WG / ntiles, cap = best.nchunks / 2;
    if (ns > cap) ns = cap;
    best.nsplit = ns < 1 ? 1 : ns;
    return best;
}

bool pwconv_wide_supported(int Ci, int Co, int P) {
    // one image's operand stays under 1 GB: the row offsets of the buffer loads are 32-bit byte counts
    return Ci % 8 == 0 && Co % 8 == 0 && Ci <= PWW_MAX_C && Co <= PWW_MAX_C && P > 0 && P <= PWW_MAX_P &&
           (size_t)(Ci > Co ? Ci : Co) * P <= ((size_t)1 << 28);
}

size_t pwconv_wide_wgrad_workspace(int B, int Ci, int Co, int P) {
    return align_up((size_t)pww_plan(B, Ci, Co, P).nsplit * Co * Ci * sizeof(float), 256);
}

hipError_t pwconv_wide_wgrad_run(const float* dy, const float* x, int B, int Ci, int Co, int P, float* dw, void* ws,
                                 hipStream_t stream) {
    const PwwPlan pl = pww_plan(B, Ci, Co, P);
    const int ntiles = pl.tiles_m * pl.tiles_n, grid = ntiles * pl.nsplit;
    const size_t lds = (size_t)32 * (pl.bm + pl.bn) * PWW_LD * sizeof(float);
    float* slabs = static_cast<float*>(ws);
#define PWW(BMV, BNV)                                                                                                   \
    hipLaunchKernelGGL((pww_wgrad_kernel<BMV, BNV>), dim3(grid), dim3(256), lds, stream, dy, x, Co, Ci, P, pl.nchunks,   \
                       pl.cpi, pl.tiles_n, ntiles, pl.nsplit, slabs)
    switch (pl.bm * 8 + pl.bn) {
        case 1 * 8 + 1: PWW(1, 1); break;
        case 1 * 8 + 2: PWW(1, 2); break;
        case 2 * 8 + 1: PWW(2, 1); break;
        case 2 * 8 + 2: PWW(2, 2); break;
        case 1 * 8 + 3: PWW(1, 3); break;
        case 3 * 8 + 1: PWW(3, 1); break;
        case 2 * 8 + 3: PWW(2, 3); break;
        case 3 * 8 + 2: PWW(3, 2); break;
        case 1 * 8 + 4: PWW(1, 4); break;
        case 4 * 8 + 1: PWW(4, 1); break;
        case 2 * 8 + 4: PWW(2, 4); break;
        case 4 * 8 + 2: PWW(4, 2); break;
        default: PWW(3, 3); break;
    }
#undef PWW
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    slab_sum_launch(slabs, pl.nsplit, Co * Ci, dw, stream);
    return hipGetLastError();
}

}  // namespace cabinet
