// K10 -- thin pointwise (1x1, bias-free) convolutions on large planes: streaming MFMA kernels, NCHW fp32.
//
// Replaces the nn.Conv2d(kernel_size=1) of the first MBConv blocks (reference src/models/mobilenetv3.py:128-131,
// 133-134,144-151: channel counts 16..120 on 128^2..512^2 planes).  There the product is HBM-bound (a few FLOP per
// byte) and MIOpen's NHWC implicit-GEMM path pays three layout transposes per call; the square-tile GEMM of ffm.hip
// is no better (its 128 x 128 tiles are mostly padding).
//   stream : Y[b][m][p] = sum_k A[m][k] X[b][k][p]     forward (A = W) and input gradient (A = W^T)
//            One wave per workgroup, no barriers in the walk.  A (<= 32 KB) is staged once in LDS; a wave walks blocks of
//            64 or 128 pixels, loading its MFMA B operand straight from global memory in the "pixel on the lane" layout
//            and storing accumulator rows as whole 128-byte lines -- no transposition anywhere.  The operand rows of the
//            wave's next block are requested while the current block is multiplied and stored (see the kernel).
//            Occupancy: the vector width is chosen so that every product of the backbone leaves two or three waves on a
//            SIMD (stream_vec); the grid is 256 CUs x the workgroups the runtime reports resident on one (8 at the most),
//            so all launched workgroups run in one round.
//   wgrad  : dW[co][ci] = sum_{b,p} dY[b][co][p] X[b][ci][p]
//            is K14's kernel (pwconv_wide.hip), which takes every shape of this operator: measured at the six layers of
//            the backbone it ran 1.3 .. 2.9 times as fast as the one-wave staging kernel this file had.
//            Its slabs (<= 512) use a prefix of the workspace, whose size stays what it was.
#include "common.hpp"

namespace cabinet {

constexpr int PW_MAXB = 4;  // row blocks of 32

// ------------------------------------------------------------------------------------------------ stream
// A[m][k] = a[m * sm + k * sk]  (forward: W (M=Co, K=Ci): sm = Ci, sk = 1;  input gradient: W^T: sm = 1, sk = Ci)
//
// A wave walks blocks of 32 NC pixels (NC column sets of 32 MFMA columns).  Lane (li, h) holds, for every row pair
// (2t, 2t + 1) of x, row 2t + h at its NC pixels: K / 2 "slots" of NC registers.  The slots ROLL: as soon as the MFMAs of
// slot t of this block are issued, the same registers are loaded with slot t of the wave's NEXT block, so a whole block of
// operand rows (K values per lane) is in flight under the MFMAs and the stores of the current one and nothing is held twice.
//   V = 4 : a lane loads 4 consecutive pixels (one 16-byte load per slot); column li of set j is pixel 4 li + j; 16-byte stores
//   V = 2 : 2 consecutive pixels, 8-byte loads and stores (the form of wide products: NC = 2 halves the registers)
//   V = 1 : column li of set j is pixel 32 j + li, dword loads and stores: ragged planes (P % 2 != 0), misaligned pointers
// Loads are unconditional buffer loads: wave-uniform image base, 32-bit lane offset (clamped into the plane; the columns past
// P are masked at the store), scalar row offset.  Slots are instantiated in groups of 8 (KQ = ceil(K / 16)); the 4 slots past
// K of a K % 16 == 8 product lie beyond the resource (no memory access) and their MFMAs are skipped.  After a wave's last
// block every lane's offset lies beyond the resource.  Offsets are 32-bit: max(Ci, Co) * P <= 2^28 (pwconv_supported).
// The arithmetic of an output element is the same chain whatever V: accumulator from 0, k ascending in pairs (k, k + 1).
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
constexpr int PW_OOB = 0x40000000;  // byte offset beyond every buffer resource (an image's operand is at most 1 GB)

template <int V>
__device__ __forceinline__ void pw_load_slot(buf_rsrc r, const int (&vo)[2], int soff, float (&d)[V == 1 ? 2 : V]) {
    if constexpr (V == 1) {
        d[0] = bload(r, vo[0], soff);
        d[1] = bload(r, vo[1], soff);
    } else if constexpr (V == 2) {
        const f32x2 t = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, vo[0], soff, 0));
        d[0] = t[0], d[1] = t[1];
    } else {
        const f32x4 t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, vo[0], soff, 0));
        d[0] = t[0], d[1] = t[1], d[2] = t[2], d[3] = t[3];
    }
}

template <int MB, int KQ, int V>
__global__ __launch_bounds__(64) void pw_stream_kernel(const float* __restrict__ a, int sm, int sk, int M, int K,
                                                        const float* __restrict__ x, int P, int nblocks,
                                                        int blocks_per_img, float* __restrict__ y) {
    constexpr int NC = V == 1 ? 2 : V, PX = 32 * NC, NS = 8 * KQ;  // column sets, pixels per block, slots
    extern __shared__ __attribute__((aligned(16))) float al[];     // [32*MB][K + 1], zero rows past M
    const int lane = threadIdx.x, li = lane & 31, h = lane >> 5, ld = K + 1;
    // batches of 8 loads in flight (written as a plain loop the compiler waits for every load before its LDS store)
    for (int i0 = 0; i0 < 32 * MB * K; i0 += 64 * 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + j * 64 + lane, m = i / K, k = i - m * K;
            v[j] = (i < 32 * MB * K && m < M) ? a[(size_t)m * sm + (size_t)k * sk] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + j * 64 + lane, m = i / K, k = i - m * K;
            if (i < 32 * MB * K) al[m * ld + k] = v[j];
        }
    }
    __syncthreads();

    const int pair_bytes = 2 * P * (int)sizeof(float);           // from one row pair to the next
    const unsigned img_bytes = (unsigned)((size_t)K * P * sizeof(float));
    // this lane's first pixel of a block at p0, as an offset into the block (sets of V == 1: + 32 j)
    const int lp = V == 1 ? li : V * li;
    float nx[NS][NC];
    buf_rsrc rs;
    int vo[2];
    auto aim = [&](int blk) {  // resource and lane offsets of a block; beyond the resource when there is no such block
        const bool any = blk < nblocks;
        const int bb = any ? blk : 0;
        const int b = bb / blocks_per_img, p0 = (bb - b * blocks_per_img) * PX;
        rs = make_rsrc(x + (size_t)b * K * P, img_bytes);
        vo[0] = any ? (h * P + min(p0 + lp, P - (V == 1 ? 1 : V))) * (int)sizeof(float) : PW_OOB;
        vo[1] = any ? (h * P + min(p0 + lp + 32, P - 1)) * (int)sizeof(float) : PW_OOB;
    };
    aim(blockIdx.x);
#pragma unroll
    for (int t = 0; t < NS; ++t) pw_load_slot<V>(rs, vo, t * pair_bytes, nx[t]);
#pragma unroll
    for (int t = 0; t < NS; ++t)  // waited for here as in the loop (below), or the loop's first MFMA inherits the wait
#pragma unroll
        for (int j = 0; j < NC; ++j) asm volatile("" : "+v"(nx[t][j])::"memory");

    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int b = blk / blocks_per_img, p0 = (blk - b * blocks_per_img) * PX;
        aim(blk + gridDim.x);
        f32x16 acc[MB][NC];
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < NC; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
        for (int q = 0; q < 2 * KQ; ++q) {  // steps of 8 values of k (K % 8 == 0): 4 slots
            if (q < 2 * KQ - 1 || 8 * q < K) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int i = 0; i < MB; ++i) {
                        const float av = al[(32 * i + li) * ld + 8 * q + 2 * s + h];
#pragma unroll
                        for (int j = 0; j < NC; ++j) acc[i][j] = mfma32(av, nx[4 * q + s][j], acc[i][j]);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) pw_load_slot<V>(rs, vo, (4 * q + s) * pair_bytes, nx[4 * q + s]);
            __builtin_amdgcn_sched_barrier(0);  // or the scheduler gathers the loads behind the last MFMAs of the block
        }
        // Loads and stores retire on one counter and out of order with each other, so a wait for a load drains every store
        // issued before it.  Touch the next block's rows HERE (an empty asm that "uses" them: the compiler waits for the
        // loads now, with no younger store pending, and under the MFMAs above the previous block's stores have drained);
        // then the stores below drain under the next block's MFMAs, which wait for nothing.
#pragma unroll
        for (int t = 0; t < NS; ++t)
#pragma unroll
            for (int j = 0; j < NC; ++j) asm volatile("" : "+v"(nx[t][j])::"memory");
        // Straight-line buffer stores, no branch: a lane past P stores at an offset beyond the resource and a row past M
        // lies beyond its records (M P floats) -- the range check drops both.  With branches around the stores the compiler
        // loses count of them and drains every store (vmcnt(0)) before the next block's first MFMA.
        const buf_rsrc ry = make_rsrc(y + (size_t)b * M * P, (unsigned)((size_t)M * P * sizeof(float)));
        const int row_bytes = P * (int)sizeof(float), so = (4 * h * P + p0 + lp) * (int)sizeof(float);
        // The data go through vector registers (the empty asm): taken straight from the accumulator tuples, hipcc (ROCm 7)
        // gathers them in spare accumulator registers and overwrites those right behind the store that still has to read
        // them -- rows of some blocks then carried their neighbour's values, depending on timing (and the dword form stored
        // element 0 of the tuple for every r).
        const int so0 = p0 + lp < P ? so : PW_OOB;  // V > 1: P % V == 0, the V pixels of a lane are live or not together
        const int so1 = p0 + lp + 32 < P ? so + 32 * (int)sizeof(float) : PW_OOB;  // V == 1: the second column set
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rb = (32 * i + acc_row(r)) * row_bytes;
                float o[NC];
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    o[j] = acc[i][j][r];
                    asm volatile("" : "+v"(o[j]));
                }
                if constexpr (V == 1) {
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o[0]), ry, so0, rb, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o[1]), ry, so1, rb, 0);
                } else if constexpr (V == 2) {
                    const f32x2 t = {o[0], o[1]};
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, t), ry, so0, rb, 0);
                } else {
                    const f32x4 t = {o[0], o[1], o[2], o[3]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, t), ry, so0, rb, 0);
                }
                __builtin_amdgcn_sched_barrier(0);  // or every row is read out before the first store: 16 MB NC more registers
            }
    }
}

// ------------------------------------------------------------------------------------------------ stream, plain form
// The walk without prefetch: per step of 8 values of k, 8 dword loads, wait, 8 MB MFMAs; 64-pixel blocks.  Kept for the
// products where the pipelined form measured no faster (stream_plain below); the same chain per output element.
template <int MB>
__global__ __launch_bounds__(64) void pw_stream_plain_kernel(const float* __restrict__ a, int sm, int sk, int M, int K,
                                                              const float* __restrict__ x, int P, int nblocks,
                                                              int blocks_per_img, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float al[];  // [32*MB][K + 1], zero rows past M
    const int lane = threadIdx.x, li = lane & 31, h = lane >> 5, ld = K + 1;
    for (int i0 = 0; i0 < 32 * MB * K; i0 += 64 * 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + j * 64 + lane, m = i / K, k = i - m * K;
            v[j] = (i < 32 * MB * K && m < M) ? a[(size_t)m * sm + (size_t)k * sk] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + j * 64 + lane, m = i / K, k = i - m * K;
            if (i < 32 * MB * K) al[m * ld + k] = v[j];
        }
    }
    __syncthreads();
    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int b = blk / blocks_per_img, p0 = (blk - b * blocks_per_img) * 64;
        const float* xb = x + (size_t)b * K * P;
        const int pa = min(p0 + li, P - 1), pb = min(p0 + 32 + li, P - 1);  // clamped: masked at the store
        f32x16 acc[MB][2];
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        for (int k0 = 0; k0 < K; k0 += 8) {  // K % 8 == 0
            float b0[4], b1[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float* row = xb + (size_t)(k0 + 2 * s + h) * P;
                b0[s] = row[pa];
                b1[s] = row[pb];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int i = 0; i < MB; ++i) {
                    const float av = al[(32 * i + li) * ld + k0 + 2 * s + h];
                    acc[i][0] = mfma32(av, b0[s], acc[i][0]);
                    acc[i][1] = mfma32(av, b1[s], acc[i][1]);
                }
            }
        }
        float* yb = y + (size_t)b * M * P;
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = 32 * i + acc_row(r) + 4 * h;
                if (m < M) {
                    if (p0 + li < P) yb[(size_t)m * P + p0 + li] = acc[i][0][r];
                    if (p0 + 32 + li < P) yb[(size_t)m * P + p0 + 32 + li] = acc[i][1][r];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// K14 (pwconv_wide.hip): 4-wave workgroups, at most 512, two resident on every CU; the rows of chunk k + 1 are in registers
// while chunk k is multiplied; one slab per workgroup.
hipError_t pwconv_wide_wgrad_run(const float* dy, const float* x, int B, int Ci, int Co, int P, float* dw, void* ws,
                                 hipStream_t stream);
size_t pwconv_wide_wgrad_workspace(int B, int Ci, int Co, int P);
bool pwconv_wide_supported(int Ci, int Co, int P);

// ------------------------------------------------------------------------------------------------ host side
static int blocks_of(int n) { return ceil_div(n, 32); }
constexpr int PW_GRID = 256 * 8;  // 8 one-wave workgroups on a CU; also the slabs the workspace is sized for (callers allocate it)

bool pwconv_supported(int Ci, int Co, int P) {
    // 32-bit byte offsets into one image's operand: max(Ci, Co) * P <= 2^28 (1 GB); the weight gradient is K14's: P <= 2^21
    return Ci % 8 == 0 && Co % 8 == 0 && Ci <= 32 * PW_MAXB && Co <= 32 * PW_MAXB &&
           blocks_of(Ci) * blocks_of(Co) <= 8 && 32 * PW_MAXB * (Ci > Co ? Ci + 1 : Co + 1) * 4 <= 64 * 1024 && P > 0 &&
           (size_t)(Ci > Co ? Ci : Co) * P <= ((size_t)1 << 28) && pwconv_wide_supported(Ci, Co, P);
}

static int wgrad_slabs(int B, int P) {
    const int nchunks = B * ceil_div(P, 64);
    return nchunks < PW_GRID ? nchunks : PW_GRID;
}
size_t pwconv_bwd_workspace(int B, int Ci, int Co, int P) {
    return align_up((size_t)wgrad_slabs(B, P) * Co * Ci * sizeof(float), 256);
}

// Pixels per lane and load.  A lane holds 16 MB NC accumulator registers, as many again while they are read out for the
// stores, and 8 KQ NC operand registers; the 16-byte form (NC = 4) is taken where these stay within 224, which leaves two
// waves on every SIMD (one-wave workgroups, 8 on a CU); the 8-byte form has no such limit among the supported shapes.
static constexpr bool stream_vec4_fits(int mb, int kq) { return 4 * (32 * mb + 8 * kq) <= 224; }
static int stream_vec(int mb, int kq, uintptr_t x_at, uintptr_t y_at, int P) {  // the addresses, or their residues modulo 16
    const uintptr_t at = x_at | y_at;
    if (P % 4 == 0 && at % 16 == 0 && stream_vec4_fits(mb, kq)) return 4;
    if (P % 2 == 0 && at % 8 == 0) return 2;
    return 1;
}

// Where the pipelined form measured no faster than the plain one at a routed shape (tools/time_pwconv.py):
//   64 x 24 (dx of 64 -> 24)              48.4 - 48.9 us against 47.9 - 49.5 at 8 x 256^2
//   24 x 72 (dx of 24 -> 72, 72 -> 24)    34.1 - 35.2 us against 33.4 - 34.4 at 2 x 512 x 256, where a wave walks 2 blocks
//                                         (at 8 x 256^2, 4 blocks: 48.7 - 50.9 against 54.5 - 55.7)
// Only these two walk lengths, 2 and 4 blocks per wave, were measured: the threshold between them (plain up to 2 blocks) is
// where config 5 sits, the crossover at other plane sizes is unmeasured.
static bool stream_plain(int mb, int kq, int nblocks64) {
    if (mb == 2 && kq == 2) return true;
    if (mb == 1 && kq == 5) return nblocks64 <= 2 * PW_GRID;
    return false;
}

// What stream_launch does with an M x K product on B planes of P pixels: the one place where it is decided (the launch below
// and the plan query of the C ABI both read it).  The grid is min(nblocks, 256 x resident workgroups): that figure is the
// runtime's and not part of the plan.
struct StreamPlan {
    int pipelined, v, px, bpi, nblocks;  // plain form: v = 1 (dword accesses), 64-pixel blocks
};
static StreamPlan stream_plan(int B, int M, int K, int P, uintptr_t x_at, uintptr_t y_at) {
    const int mb = blocks_of(M), kq = ceil_div(K, 16);
    StreamPlan pl{};
    pl.pipelined = stream_plain(mb, kq, B * ceil_div(P, 64)) ? 0 : 1;
    pl.v = pl.pipelined ? stream_vec(mb, kq, x_at, y_at, P) : 1;
    pl.px = pl.v == 4 ? 128 : 64;
    pl.bpi = ceil_div(P, pl.px);
    pl.nblocks = B * pl.bpi;
    return pl;
}

void pwconv_stream_plan_query(int B, int M, int K, int P, unsigned x_align, unsigned y_align, int out[4]) {
    const StreamPlan pl = stream_plan(B, M, K, P, x_align, y_align);
    out[0] = pl.pipelined, out[1] = pl.v, out[2] = pl.px, out[3] = pl.nblocks;
}

template <int MB, int KQ, int V>
static hipError_t stream_launch_v(const StreamPlan& pl, const float* a, int sm, int sk, int M, int K, const float* x, int P,
                                  float* y, hipStream_t stream) {
    if constexpr ((V != 4 || stream_vec4_fits(MB, KQ)) && MB * ((KQ + 1) / 2) <= 8) {
        if (pl.px != 32 * (V == 1 ? 2 : V)) return hipErrorInvalidValue;  // the kernel's block is the plan's
        const int bpi = pl.bpi, nblocks = pl.nblocks;
        const size_t lds = (size_t)32 * MB * (K + 1) * sizeof(float);
        // every launched workgroup is resident: as many one-wave workgroups on a CU as the instantiation's registers and
        // its largest A tile (K = 16 KQ) admit, 8 at the most (two waves on a SIMD).  Asked of the runtime once per device
        // ordinal (the query is no stream operation, so a first call inside a capture is fine); a failure is returned.
        static std::atomic<int> resident[64];
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const bool tracked = dev >= 0 && dev < 64;
        int per_cu = tracked ? resident[dev].load(std::memory_order_relaxed) : 0;
        if (per_cu == 0) {
            int n = 0;
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pw_stream_kernel<MB, KQ, V>, 64,
                                                             (size_t)32 * MB * (16 * KQ + 1) * sizeof(float));
            if (e != hipSuccess) return e;
            per_cu = n < 1 ? 1 : (n < 8 ? n : 8);  // 16 where the registers allow measured no faster
            if (tracked) resident[dev].store(per_cu, std::memory_order_relaxed);
        }
        const int grid = nblocks < 256 * per_cu ? nblocks : 256 * per_cu;
        hipLaunchKernelGGL((pw_stream_kernel<MB, KQ, V>), dim3(grid), dim3(64), lds, stream, a, sm, sk, M, K, x, P, nblocks,
                           bpi, y);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;  // no such instantiation: pwconv_supported and stream_vec never ask for it
    }
}

template <int MB, int KQ>
static hipError_t stream_launch_kq(const StreamPlan& pl, const float* a, int sm, int sk, int M, int K, const float* x, int P,
                                   float* y, hipStream_t stream) {
    if (pl.v == 4) return stream_launch_v<MB, KQ, 4>(pl, a, sm, sk, M, K, x, P, y, stream);
    if (pl.v == 2) return stream_launch_v<MB, KQ, 2>(pl, a, sm, sk, M, K, x, P, y, stream);
    return stream_launch_v<MB, KQ, 1>(pl, a, sm, sk, M, K, x, P, y, stream);
}

template <int MB>
static hipError_t stream_launch_mb(int kq, const StreamPlan& pl, const float* a, int sm, int sk, int M, int K, const float* x,
                                   int P, float* y, hipStream_t stream) {
#define PW_STREAM(KQV) \
    case KQV: return stream_launch_kq<MB, KQV>(pl, a, sm, sk, M, K, x, P, y, stream)
    switch (kq) {
        PW_STREAM(1);
        PW_STREAM(2);
        PW_STREAM(3);
        PW_STREAM(4);
        PW_STREAM(5);
        PW_STREAM(6);
        PW_STREAM(7);
        default: PW_STREAM(8);
    }
#undef PW_STREAM
}

static hipError_t stream_launch(const float* a, int sm, int sk, int M, int K, const float* x, int B, int P, float* y,
                                hipStream_t stream) {
    const int mb = blocks_of(M), kq = ceil_div(K, 16);
    const StreamPlan pl = stream_plan(B, M, K, P, reinterpret_cast<uintptr_t>(x), reinterpret_cast<uintptr_t>(y));
    if (!pl.pipelined) {
        const int grid = pl.nblocks < PW_GRID ? pl.nblocks : PW_GRID;
        const size_t lds = (size_t)32 * mb * (K + 1) * sizeof(float);
        if (mb == 1)
            hipLaunchKernelGGL(pw_stream_plain_kernel<1>, dim3(grid), dim3(64), lds, stream, a, sm, sk, M, K, x, P, pl.nblocks, pl.bpi, y);
        else
            hipLaunchKernelGGL(pw_stream_plain_kernel<2>, dim3(grid), dim3(64), lds, stream, a, sm, sk, M, K, x, P, pl.nblocks, pl.bpi, y);
        return hipGetLastError();
    }
    if (mb == 1) return stream_launch_mb<1>(kq, pl, a, sm, sk, M, K, x, P, y, stream);
    if (mb == 2) return stream_launch_mb<2>(kq, pl, a, sm, sk, M, K, x, P, y, stream);
    if (mb == 3) return stream_launch_mb<3>(kq, pl, a, sm, sk, M, K, x, P, y, stream);
    return stream_launch_mb<4>(kq, pl, a, sm, sk, M, K, x, P, y, stream);
}

hipError_t pwconv_fwd_run(const float* x, const float* w, int B, int Ci, int Co, int P, float* y, hipStream_t stream) {
    return stream_launch(w, Ci, 1, Co, Ci, x, B, P, y, stream);
}

hipError_t pwconv_bwd_run(const float* dy, const float* x, const float* w, int B, int Ci, int Co, int P, float* dx,
                          float* dw, void* ws, hipStream_t stream) {
    if (dx) {
        hipError_t e = stream_launch(w, 1, Ci, Ci, Co, dy, B, P, dx, stream);  // dx = W^T dy
        if (e != hipSuccess) return e;
    }
    if (dw) {
        // the slabs of K14's plan (at most 512, never more than the pixel chunks) are a prefix of this operator's workspace
        if (pwconv_wide_wgrad_workspace(B, Ci, Co, P) > pwconv_bwd_workspace(B, Ci, Co, P)) return hipErrorInvalidValue;
        return pwconv_wide_wgrad_run(dy, x, B, Ci, Co, P, dw, ws, stream);
    }
    return hipGetLastError();
}

}  // namespace cabinet
