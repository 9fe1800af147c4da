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
#include "act.hpp"
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

void pwconv_wide_plan_query(int B, int Ci, int Co, int P, int out[5]) {
    const PwwPlan pl = pww_plan(B, Ci, Co, P);
    out[0] = pl.bm, out[1] = pl.bn, out[2] = pl.tiles_m, out[3] = pl.tiles_n, out[4] = pl.nsplit;
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

// ------------------------------------------------------------------------------------------------ BN form (thin convolutions)
// Backward of  z = W x  (one tile: Co, Ci <= 96)  followed by BatchNorm + activation, in one walk over g, z and x:
//   staging : the kernel above with g and z rows loaded in place of dy; dz = (gamma invstd) (du - m1 - xhat m2),
//             du = g act'(fma(xhat, gamma, beta)) -- the expressions of bn_act_bwd_dx_kernel, same build flags, same bits -- is
//             formed on the way into the LDS and never stored to memory.  Pixels past P and rows past Co stage 0.
//   dW      : as above (same chunk ranges, same slabs, same ordered slab sum).
//   dX      : dx_chunk = W^T dz of the staged chunk: wave w owns pixels 16 w .. + 15 of it (the quarter it multiplies for dW), the
//             exact-fp32 MFMA 16x16x4 with pixel = row, ci = column, W in the LDS ([co][32 BN + 4]: the four co rows a k-step
//             reads, co, co + 4, co + 8, co + 12, fall on disjoint banks, as do the dz rows at stride 68).  A lane ends up with
//             four consecutive pixels of one ci row: one 16-byte buffer store (dwords where P % 4 != 0 or dx is unaligned).
// The seven per-channel scalars sit in the LDS ([co][8]); a thread reads the two quads of its row per staged element row.
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int BM, int BN>
__global__ __launch_bounds__(256, (BM * BN > 4 ? 1 : 2)) void pw_bn_bwd_kernel(
    const float* __restrict__ g, const float* __restrict__ z, const float* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ coef, int Co, int Ci, int P, int act, int nchunks,
    int chunks_per_img, int nsplit, int vec, float* __restrict__ dx, float* __restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) float tl[];  // [32 (BM + BN)][68] | W [32 BM][32 BN + 4] | scalars [32 BM][8]
    constexpr int LDW = 32 * BN + 4;
    float* wl = tl + 32 * (BM + BN) * PWW_LD;
    float* sc = wl + 32 * BM * LDW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
    const int split = xcd_chunked_tile(blockIdx.x, gridDim.x);  // neighbouring chunk ranges share an XCD's L2
    const int c_begin = (int)((long long)split * nchunks / nsplit), c_end = (int)((long long)(split + 1) * nchunks / nsplit);
    const bool want_dw = slabs != nullptr, want_dx = dx != nullptr;

    for (int i = tid; i < 32 * BM * LDW; i += 256) {
        const int co = i / LDW, ci = i - co * LDW;
        wl[i] = (co < Co && ci < Ci) ? w[co * Ci + ci] : 0.f;
    }
    for (int co = tid; co < 32 * BM; co += 256) {
        const bool live = co < Co;
        const float mu = live ? mean[co] : 0.f, inv = live ? invstd[co] : 0.f, gam = live ? gamma[co] : 0.f;
        float* s = sc + 8 * co;
        s[0] = mu, s[1] = inv, s[2] = gam, s[3] = live ? beta[co] : 0.f;
        s[4] = live ? coef[co] : 0.f, s[5] = live ? coef[Co + co] : 0.f, s[6] = gam * inv, s[7] = 0.f;
    }

    f32x16 acc[BM][BN];
#pragma unroll
    for (int i = 0; i < BM; ++i)
#pragma unroll
        for (int j = 0; j < BN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int wrow = __builtin_amdgcn_readfirstlane(wave);
    float vg[8 * BM], vz[8 * BM], vx[8 * BN];
    auto load = [&](int c) {
        const int b = c / chunks_per_img, p0 = (c - b * chunks_per_img) * PWW_KC;
        // as in pww_wgrad_kernel: no predicates, lanes past the plane and rows past Co / Ci are out of the resource and load 0
        const int voff = p0 + lane < P ? lane * 4 : PWW_OOB;
        const int rows_y = Co - wrow, rows_x = Ci - wrow;
        const unsigned by = rows_y > 0 ? (unsigned)(((size_t)(rows_y - 1) * P + (P - p0)) * sizeof(float)) : 0u;
        const buf_rsrc rg = make_rsrc(g + ((size_t)b * Co + wrow) * P + p0, by);
        const buf_rsrc rz = make_rsrc(z + ((size_t)b * Co + wrow) * P + p0, by);
        const int row_bytes = 4 * P * (int)sizeof(float);
#pragma unroll
        for (int j = 0; j < 8 * BM; ++j) vg[j] = bload(rg, voff, j * row_bytes);
#pragma unroll
        for (int j = 0; j < 8 * BM; ++j) vz[j] = bload(rz, voff, j * row_bytes);
        if (want_dw) {
            const buf_rsrc rx = make_rsrc(x + ((size_t)b * Ci + wrow) * P + p0,
                                          rows_x > 0 ? (unsigned)(((size_t)(rows_x - 1) * P + (P - p0)) * sizeof(float)) : 0u);
#pragma unroll
            for (int j = 0; j < 8 * BN; ++j) vx[j] = bload(rx, voff, j * row_bytes);
        }
    };

    const int kb = 16 * wave + 4 * h;         // dW: this lane's first pixel column of the chunk
    const int l16 = lane & 15, gq = lane >> 4;  // dX: pixel / ci within 16, k-group
    if (c_begin < c_end) load(c_begin);
    for (int c = c_begin; c < c_end; ++c) {
        const int b = c / chunks_per_img, p0 = (c - b * chunks_per_img) * PWW_KC;
        __syncthreads();  // the previous chunk's operand reads are done (first pass: W and the scalars are staged)
        const bool px_live = p0 + lane < P;
#pragma unroll
        for (int j = 0; j < 8 * BM; ++j) {
            const int row = wave + 4 * j;
            const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc + 8 * row), s1 = *reinterpret_cast<const f32x4*>(sc + 8 * row + 4);
            const float xh = (vz[j] - s0[0]) * s0[1];
            const float du = vg[j] * act_grad(fmaf(xh, s0[2], s0[3]), act);
            const float d = s1[2] * (du - s1[0] - xh * s1[1]);
            tl[row * PWW_LD + lane] = (px_live && row < Co) ? d : 0.f;  // not the dz of zero-filled operands
        }
        if (want_dw) {
#pragma unroll
            for (int j = 0; j < 8 * BN; ++j) tl[(32 * BM + wave + 4 * j) * PWW_LD + lane] = vx[j];
        }
        __syncthreads();
        if (c + 1 < c_end) load(c + 1);  // in flight while this chunk is multiplied
        if (want_dw) pww_multiply<BM, BN>(tl, kb, li, acc);
        if (want_dx) {
            f32x4 d[2 * BN];
#pragma unroll
            for (int t = 0; t < 2 * BN; ++t) d[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 8 * BM; ++k) {
                const int co = 16 * (k >> 2) + (k & 3) + 4 * gq;  // k-step k contracts co, co + 4, co + 8, co + 12
                const float a = tl[co * PWW_LD + 16 * wave + l16];
#pragma unroll
                for (int t = 0; t < 2 * BN; ++t) d[t] = mfma16(a, wl[co * LDW + 16 * t + l16], d[t]);
            }
            // straight-line buffer stores: a pixel past P or a row past Ci gets an offset beyond the resource and is dropped.
            // The data pass through vector registers first (stores fed from accumulator registers).
            const buf_rsrc rd = make_rsrc(dx + (size_t)b * Ci * P, (unsigned)((size_t)Ci * P * sizeof(float)));
            const int px = p0 + 16 * wave + 4 * gq;
#pragma unroll
            for (int t = 0; t < 2 * BN; ++t) {
                const int ci = 16 * t + l16;
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    o[r] = d[t][r];
                    asm volatile("" : "+v"(o[r]));
                }
                const int off = (ci * P + px) * (int)sizeof(float);
                if (vec) {
                    const f32x4 q = {o[0], o[1], o[2], o[3]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, q), rd, (ci < Ci && px < P) ? off : PWW_OOB, 0, 0);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o[r]), rd,
                                                              (ci < Ci && px + r < P) ? off + 4 * r : PWW_OOB, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);  // one tile's data read out at a time
            }
        }
    }

    if (!want_dw) return;
    // the four partial tiles in wave order, as in pww_wgrad_kernel
    float* slab = slabs + (size_t)split * Co * Ci;
    const int rr = tid >> 4, c4 = 4 * (tid & 15);
    const int row_in = (rr & 3) + 8 * (rr >> 2) + 4 * (c4 >> 5), col_in = c4 & 31;
#pragma unroll
    for (int i = 0; i < BM; ++i)
#pragma unroll
        for (int j = 0; j < BN; ++j) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) tl[(wave * 16 + r) * 64 + lane] = acc[i][j][r];
            __syncthreads();
            f32x4 t = *reinterpret_cast<const f32x4*>(tl + rr * 64 + c4);
#pragma unroll
            for (int q = 1; q < 4; ++q) t += *reinterpret_cast<const f32x4*>(tl + (q * 16 + rr) * 64 + c4);
            const int co = 32 * i + row_in, ci = 32 * j + col_in;
            if (co < Co && ci < Ci) *reinterpret_cast<f32x4*>(slab + (size_t)co * Ci + ci) = t;
        }
}

// one tile: the block counts are the tile shape; the split is K14's (at most 512 workgroups, two chunks or more each)
static PwwPlan pw_bn_plan(int B, int Ci, int Co, int P) {
    PwwPlan pl{};
    pl.bm = ceil_div(Co, 32), pl.bn = ceil_div(Ci, 32), pl.tiles_m = pl.tiles_n = 1;
    pl.cpi = ceil_div(P, PWW_KC);
    pl.nchunks = B * pl.cpi;
    int ns = PWW_TARGET_WG, cap = pl.nchunks / 2;
    if (ns > cap) ns = cap;
    pl.nsplit = ns < 1 ? 1 : ns;
    return pl;
}

// the launch: the plan above, the store form of dx (16 bytes where the plane and the pointer allow; a null dx counts as aligned)
// and the LDS of the instantiation -- read by pw_bn_bwd_run and by the plan query of the C ABI
struct PwBnLaunch {
    PwwPlan pl;
    int vec;
    size_t lds;
};
static PwBnLaunch pw_bn_launch(int B, int Ci, int Co, int P, uintptr_t dx_at) {
    PwBnLaunch l{};
    l.pl = pw_bn_plan(B, Ci, Co, P);
    l.vec = (P % 4 == 0 && dx_at % 16 == 0) ? 1 : 0;
    l.lds = ((size_t)32 * (l.pl.bm + l.pl.bn) * PWW_LD + (size_t)32 * l.pl.bm * (32 * l.pl.bn + 4) + (size_t)32 * l.pl.bm * 8) *
            sizeof(float);
    return l;
}

void pw_bn_bwd_plan_query(int B, int Ci, int Co, int P, unsigned dx_align, int out[5]) {
    const PwBnLaunch l = pw_bn_launch(B, Ci, Co, P, dx_align);
    out[0] = l.pl.bm, out[1] = l.pl.bn, out[2] = l.pl.nsplit, out[3] = l.vec, out[4] = (int)l.lds;
}

bool pw_bn_bwd_supported(int Ci, int Co, int P) {
    return Ci <= 96 && Co <= 96 && pwconv_wide_supported(Ci, Co, P);
}

size_t pw_bn_bwd_slab_bytes(int B, int Ci, int Co, int P) {
    return align_up((size_t)pw_bn_plan(B, Ci, Co, P).nsplit * Co * Ci * sizeof(float), 256);
}

// coef: [2][Co] (mean(du), mean(du xhat)), zeros in eval mode; dx and / or dw may be null (dw null: `slabs` is not touched)
hipError_t pw_bn_bwd_run(const float* g, const float* z, const float* x, const float* w, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, const float* coef, int B, int Ci, int Co, int P, int act,
                         float* dx, float* dw, void* slab_ws, hipStream_t stream) {
    if (!dx && !dw) return hipSuccess;
    const PwBnLaunch launch = pw_bn_launch(B, Ci, Co, P, reinterpret_cast<uintptr_t>(dx));
    const PwwPlan& pl = launch.pl;
    const size_t lds = launch.lds;
    float* slabs = dw ? static_cast<float*>(slab_ws) : nullptr;
    const int vec = launch.vec;
    hipError_t e = hipSuccess;
#define PWB(BMV, BNV)                                                                                                    \
    {                                                                                                                    \
        static lds_attr_mask mask{0};                                                                                    \
        if (lds > 64 * 1024) e = ensure_dynamic_lds(reinterpret_cast<const void*>(&pw_bn_bwd_kernel<BMV, BNV>), lds, mask); \
        if (e == hipSuccess)                                                                                             \
            hipLaunchKernelGGL((pw_bn_bwd_kernel<BMV, BNV>), dim3(pl.nsplit), dim3(256), lds, stream, g, z, x, w, mean,   \
                               invstd, gamma, beta, coef, Co, Ci, P, act, pl.nchunks, pl.cpi, pl.nsplit, vec, dx, slabs); \
    }
    switch (pl.bm * 8 + pl.bn) {
        case 1 * 8 + 1: PWB(1, 1) break;
        case 1 * 8 + 2: PWB(1, 2) break;
        case 2 * 8 + 1: PWB(2, 1) break;
        case 2 * 8 + 2: PWB(2, 2) break;
        case 1 * 8 + 3: PWB(1, 3) break;
        case 3 * 8 + 1: PWB(3, 1) break;
        case 2 * 8 + 3: PWB(2, 3) break;
        case 3 * 8 + 2: PWB(3, 2) break;
        default: PWB(3, 3) break;
    }
#undef PWB
    if (e != hipSuccess) return e;
    e = hipGetLastError();
    if (e != hipSuccess || !dw) return e;
    slab_sum_launch(slabs, pl.nsplit, Co * Ci, dw, stream);
    return hipGetLastError();
}

// ---- thin 1x1 convolution -> BatchNorm + activation (the closing BatchNorm of an MBConv block), backward: K7's reduce and
// stand-alone finalize (dweight, dbias, coefficients: the bits of bn_act_bwd_run), then the BN-form kernel.
size_t pw_bn_act_bwd_workspace(int B, int Ci, int Co, int P) {
    return bn_act_workspace(B, Co, P) + pw_bn_bwd_slab_bytes(B, Ci, Co, P);
}

hipError_t pw_bn_act_bwd_run(const float* g, const float* z, const float* x, const float* w, const float* bn_w, const float* bn_b,
                             const float* save_mean, const float* save_invstd, int B, int Ci, int Co, int P, int act, int training,
                             float* dx, float* dw, float* dbn_w, float* dbn_b, void* ws, hipStream_t stream) {
    const float* coef = nullptr;
    hipError_t e = bn_act_bwd_stats_run(g, z, bn_w, bn_b, save_mean, save_invstd, B, Co, P, act, training, dbn_w, dbn_b, ws, &coef,
                                        stream);
    if (e != hipSuccess) return e;
    return pw_bn_bwd_run(g, z, x, w, save_mean, save_invstd, bn_w, bn_b, coef, B, Ci, Co, P, act, dx, dw,
                         static_cast<char*>(ws) + bn_act_workspace(B, Co, P), stream);
}

}  // namespace cabinet
