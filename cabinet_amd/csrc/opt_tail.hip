// K16: the optimizer tail of the step as three launches on one stream -- gradient norm, step scalars, fused apply.
// Replaces, per step (reference src/scripts/train.py:411-427): clip_grad_norm_ over all parameters, Optimizer.step()
// (src/utils/optimizer.py:124-156: warm-up / poly learning rate computed on the HOST from its own step counter, then SGD with
// momentum and per-group weight decay) and ModelEMA.update() (src/utils/ema.py:51-62: two launches per floating-point state_dict
// entry).  Here the step counter, the EMA counter and the schedule live on the DEVICE, so a captured step does not freeze them.
//
//   sgd_tail_norm     one fp32 partial of sum(g^2) per chunk; in-lane accumulators -> wave -> LDS, fixed order, no atomics
//   sgd_tail_scalars  ONE workgroup: partials summed in double in a fixed order, clip coefficient, non-finite flag, the learning rate
//                     per group and the EMA factor from the device counters, the counters advanced, the per-tensor "first step" flags
//   sgd_tail_apply    per element: g*coef (+ wd*p) -> momentum buffer -> p -> EMA; EMA-only entries fold the live tensor
//
// Why the scalars are a launch of their own and not the apply pass's prologue: every one of up to 2048 workgroups would re-sum
// ~2,600 partials in double (42 MB of L2 reads against the pass's 290 MB of HBM), and the counters would have to be
// double-buffered; one extra node in a graph costs less than either.
//
// Chunks are <= 4096 elements (256 threads x 16 B x 4) and start at a multiple of 4096 inside their tensor, so a chunk is as aligned
// as its tensor's base pointers.  A tensor of <= 4096 elements is ONE chunk of its own (the 144 tiny tensors of CABiNet-Large are
// 144 of ~2,700 chunks: packing several per workgroup would save ~5 % of the workgroups' iterations and cost a second index level).
// Where the pointers a pass touches are 16-byte aligned the body of the chunk moves as float4 and the last numel % 4 elements as
// scalars; otherwise the whole chunk moves as scalars -- in the norm pass element for element in the float4 form's order, so that
// neither the norm nor anything derived from it depends on where a gradient starts.  Nothing here allocates, synchronises or reads
// on the host.
#include "../../include/cabinet_hip.h"
#include "common.hpp"

#include <stdint.h>

namespace cabinet {

constexpr int TAIL_THREADS = 256;
constexpr int TAIL_CHUNK = CABINET_SGD_TAIL_CHUNK;  // 4096
constexpr int TAIL_GRID_CAP = 2048;
constexpr int TAIL_HEADER_BYTES = 128;  // sizeof(TailState) rounded up; the flag arrays follow it

// device state block (the header's layout comment is the contract; Python reads these fields through views)
struct TailState {
    long long it;        //  0
    long long updates;   //  8
    long long skipped;   // 16
    int nonfinite;       // 24  last step's norm was inf / nan
    int apply;           // 28  the apply pass of this step runs (0: skipped step)
    float grad_norm;     // 32
    float coef;          // 36
    float lr[4];         // 40
    float ema_d;         // 56
    float ema_omd;       // 60  float(1 - d), rounded from the double as Tensor.add_(alpha=1 - d) does
};
static_assert(sizeof(TailState) <= TAIL_HEADER_BYTES, "state header");

__device__ __forceinline__ bool ptr_aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

// ---------------------------------------------------------------------------------------------------------------- norm
__global__ __launch_bounds__(TAIL_THREADS) void sgd_tail_norm(const cabinet_sgd_tail_entry* __restrict__ entries, int n_entries,
                                                               const cabinet_sgd_tail_chunk* __restrict__ chunks, int n_chunks,
                                                               float* __restrict__ partials) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const cabinet_sgd_tail_chunk ck = chunks[c];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        bool live = ck.tensor >= 0 && ck.tensor < n_entries && ck.length > 0 && ck.length <= TAIL_CHUNK && ck.start >= 0;
        const cabinet_sgd_tail_entry e = live ? entries[ck.tensor] : cabinet_sgd_tail_entry{};
        live = live && ck.start + ck.length <= e.numel;  // a chunk never leaves its tensor, whatever the table says
        if (live && !(e.flags & CABINET_SGD_TAIL_EMA_ONLY) && e.grad) {
            const float* g = e.grad + ck.start;
            const int len = ck.length;
            // the same elements in the same order whether or not the gradient is 16-byte aligned (then four dword loads stand
            // for the float4): the norm, and with it the clip coefficient, has the same bits for any address of the gradient
            const bool vec = ptr_aligned16(g, nullptr, nullptr, nullptr);
            const int nvec = len >> 2;
            const float4* g4 = reinterpret_cast<const float4*>(g);
            // 4 independent accumulators: vector v of the chunk goes to accumulator (v / 256) & 3
            float4 x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = j * TAIL_THREADS + t;
                x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (v < nvec) x[j] = vec ? g4[v] : make_float4(g[4 * v], g[4 * v + 1], g[4 * v + 2], g[4 * v + 3]);
            }
            a0 = (x[0].x * x[0].x + x[0].y * x[0].y) + (x[0].z * x[0].z + x[0].w * x[0].w);
            a1 = (x[1].x * x[1].x + x[1].y * x[1].y) + (x[1].z * x[1].z + x[1].w * x[1].w);
            a2 = (x[2].x * x[2].x + x[2].y * x[2].y) + (x[2].z * x[2].z + x[2].w * x[2].w);
            a3 = (x[3].x * x[3].x + x[3].y * x[3].y) + (x[3].z * x[3].z + x[3].w * x[3].w);
            // the last length % 4 elements
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            int j = 0;
            for (int i = nvec * 4 + t; i < len; i += TAIL_THREADS, ++j) {
                const float v = g[i];
                s[j & 3] += v * v;
            }
            a0 += s[0];
            a1 += s[1];
            a2 += s[2];
            a3 += s[3];
        }
        const float total = block_sum_256((a0 + a1) + (a2 + a3), red);
        if (t == 0) partials[c] = total;
    }
}

// ------------------------------------------------------------------------------------------------------------- scalars
__global__ __launch_bounds__(TAIL_THREADS) void sgd_tail_scalars(const cabinet_sgd_tail_entry* __restrict__ entries, int n_entries,
                                                                  const float* __restrict__ partials, int n_chunks,
                                                                  cabinet_sgd_tail_config cfg, TailState* __restrict__ st,
                                                                  int* __restrict__ valid, int* __restrict__ first) {
    __shared__ double red[TAIL_THREADS];
    __shared__ int s_apply;
    const int t = threadIdx.x;
    // fixed order: thread t sums partials t, t + 256, ... in double; then a binary tree over the 256 slots
    double acc = 0.0;
    for (int i = t; i < n_chunks; i += TAIL_THREADS) acc += (double)partials[i];
    red[t] = acc;
    __syncthreads();
    for (int w = TAIL_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const double sumsq = red[0];
        const double norm = sqrt(sumsq);
        const bool nonfinite = !(norm <= 1.7976931348623157e308);  // inf or nan
        const bool skip = nonfinite && cfg.skip_nonfinite;
        st->grad_norm = (float)norm;
        st->nonfinite = nonfinite ? 1 : 0;
        st->apply = skip ? 0 : 1;
        s_apply = skip ? 0 : 1;
        if (skip) {
            st->skipped = st->skipped + 1;
        } else {
            // torch.nn.utils.clip_grad_norm_: coef = clamp(max_norm / (norm + 1e-6), max = 1)
            double coef = 1.0;
            if (cfg.max_norm > 0.0) coef = fmin(1.0, cfg.max_norm / (norm + 1e-6));
            st->coef = (float)coef;
            // optimizer.py:124-138, in double as the interpreter computes it, rounded to float per group
            const long long it = st->it;
            double lr;
            if (it < cfg.warmup_steps) {
                const double alpha = (double)it / (double)cfg.warmup_steps;
                lr = cfg.warmup_start_lr + alpha * (cfg.lr0 - cfg.warmup_start_lr);
            } else {
                double k = ((double)it - (double)cfg.warmup_steps) / (cfg.max_iter - (double)cfg.warmup_steps);
                k = fmin(fmax(k, 0.0), 1.0);  // past max_iter the reference's (1 - k) ** power leaves the reals: lr = 0 here
                lr = cfg.lr0 * pow(1.0 - k, cfg.power);
            }
            for (int gi = 0; gi < 4; ++gi) st->lr[gi] = (float)(lr * cfg.lr_scale[gi]);
            // ema.py:51-58: the counter advances first
            const long long up = st->updates + 1;
            const double d = cfg.ema_decay * (1.0 - exp(-(double)up / cfg.ema_tau));
            st->ema_d = (float)d;
            st->ema_omd = (float)(1.0 - d);
            st->updates = up;
            st->it = it + 1;
        }
    }
    __syncthreads();
    if (!s_apply) return;
    // a tensor's momentum buffer holds a value once it has been stepped: `first` is what THIS step's apply pass reads
    for (int i = t; i < n_entries; i += TAIL_THREADS) {
        const bool owned = !(entries[i].flags & CABINET_SGD_TAIL_EMA_ONLY) && entries[i].grad != nullptr;
        first[i] = (owned && !valid[i]) ? 1 : 0;
        if (owned) valid[i] = 1;
    }
}

// --------------------------------------------------------------------------------------------------------------- apply
struct TailCoef {
    float coef, wd, momentum, lr, d, omd;
    bool first, has_buf, has_ema;
};

__device__ __forceinline__ void tail_elem(const TailCoef& k, float g, float& p, float& buf, float& ema) {
    g = g * k.coef;
    if (k.wd != 0.f) g = g + k.wd * p;
    if (k.has_buf) {
        buf = k.first ? g : k.momentum * buf + g;
        g = buf;
    }
    p = p - k.lr * g;
    ema = k.d * ema + k.omd * p;
}

__global__ __launch_bounds__(TAIL_THREADS) void sgd_tail_apply(const cabinet_sgd_tail_entry* __restrict__ entries, int n_entries,
                                                                const cabinet_sgd_tail_chunk* __restrict__ chunks, int n_chunks,
                                                                float momentum, float wd0, float wd1, float wd2, float wd3,
                                                                const TailState* __restrict__ st, const int* __restrict__ first) {
    if (!st->apply) return;  // skipped step: nothing is written
    const int t = threadIdx.x;
    const float d = st->ema_d, omd = st->ema_omd, coef = st->coef;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const cabinet_sgd_tail_chunk ck = chunks[c];
        if (ck.tensor < 0 || ck.tensor >= n_entries || ck.length <= 0 || ck.length > TAIL_CHUNK || ck.start < 0) continue;
        const cabinet_sgd_tail_entry e = entries[ck.tensor];
        const int len = ck.length;
        if (ck.start + len > e.numel) continue;  // a chunk never leaves its tensor, whatever the table says
        if ((e.flags & CABINET_SGD_TAIL_EMA_ONLY) || !e.grad) {
            if (!e.ema || !e.param) continue;
            const float* p = e.param + ck.start;
            float* m = e.ema + ck.start;
            const int nvec = ptr_aligned16(p, m, nullptr, nullptr) ? (len >> 2) : 0;
            for (int v = t; v < nvec; v += TAIL_THREADS) {
                const float4 pv = reinterpret_cast<const float4*>(p)[v];
                float4 mv = reinterpret_cast<float4*>(m)[v];
                mv.x = d * mv.x + omd * pv.x;
                mv.y = d * mv.y + omd * pv.y;
                mv.z = d * mv.z + omd * pv.z;
                mv.w = d * mv.w + omd * pv.w;
                reinterpret_cast<float4*>(m)[v] = mv;
            }
            for (int i = nvec * 4 + t; i < len; i += TAIL_THREADS) m[i] = d * m[i] + omd * p[i];
            continue;
        }
        const int gi = e.group & 3;
        TailCoef k;
        k.coef = coef;
        k.wd = gi == 0 ? wd0 : gi == 1 ? wd1 : gi == 2 ? wd2 : wd3;
        k.momentum = momentum;
        k.lr = st->lr[gi];
        k.d = d;
        k.omd = omd;
        k.first = first[ck.tensor] != 0;
        k.has_buf = e.buf != nullptr && momentum != 0.f;
        k.has_ema = e.ema != nullptr;
        float* p = e.param + ck.start;
        const float* g = e.grad + ck.start;
        float* b = k.has_buf ? e.buf + ck.start : nullptr;
        float* m = k.has_ema ? e.ema + ck.start : nullptr;
        const int nvec = ptr_aligned16(p, g, b, m) ? (len >> 2) : 0;
        // all loads of the chunk's float4 body first (4 per array and thread), then the arithmetic, then the stores
        float4 pv[4], gv[4], bv[4], mv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = j * TAIL_THREADS + t;
            pv[j] = gv[j] = bv[j] = mv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (v < nvec) {
                pv[j] = reinterpret_cast<const float4*>(p)[v];
                gv[j] = reinterpret_cast<const float4*>(g)[v];
                if (k.has_buf && !k.first) bv[j] = reinterpret_cast<const float4*>(b)[v];
                if (k.has_ema) mv[j] = reinterpret_cast<const float4*>(m)[v];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = j * TAIL_THREADS + t;
            if (v >= nvec) continue;
            tail_elem(k, gv[j].x, pv[j].x, bv[j].x, mv[j].x);
            tail_elem(k, gv[j].y, pv[j].y, bv[j].y, mv[j].y);
            tail_elem(k, gv[j].z, pv[j].z, bv[j].z, mv[j].z);
            tail_elem(k, gv[j].w, pv[j].w, bv[j].w, mv[j].w);
            reinterpret_cast<float4*>(p)[v] = pv[j];
            if (k.has_buf) reinterpret_cast<float4*>(b)[v] = bv[j];
            if (k.has_ema) reinterpret_cast<float4*>(m)[v] = mv[j];
        }
        for (int i = nvec * 4 + t; i < len; i += TAIL_THREADS) {
            float ps = p[i], bs = (k.has_buf && !k.first) ? b[i] : 0.f, ms = k.has_ema ? m[i] : 0.f;
            tail_elem(k, g[i], ps, bs, ms);
            p[i] = ps;
            if (k.has_buf) b[i] = bs;
            if (k.has_ema) m[i] = ms;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
size_t sgd_tail_workspace(int n_chunks) { return align_up((size_t)n_chunks * sizeof(float), 256); }

size_t sgd_tail_state(int n_entries) { return TAIL_HEADER_BYTES + align_up((size_t)n_entries * 2 * sizeof(int), 256); }

hipError_t sgd_tail_run(const cabinet_sgd_tail_entry* entries, int n_entries, const cabinet_sgd_tail_chunk* chunks, int n_chunks,
                        const cabinet_sgd_tail_config& cfg, void* state, void* ws, int max_grid, hipStream_t stream) {
    const int cap = max_grid > 0 ? (max_grid < TAIL_GRID_CAP ? max_grid : TAIL_GRID_CAP) : TAIL_GRID_CAP;
    const int grid = n_chunks < cap ? n_chunks : cap;
    TailState* st = static_cast<TailState*>(state);
    int* valid = reinterpret_cast<int*>(static_cast<char*>(state) + TAIL_HEADER_BYTES);
    int* first = valid + n_entries;
    float* partials = static_cast<float*>(ws);
    sgd_tail_norm<<<grid, TAIL_THREADS, 0, stream>>>(entries, n_entries, chunks, n_chunks, partials);
    sgd_tail_scalars<<<1, TAIL_THREADS, 0, stream>>>(entries, n_entries, partials, n_chunks, cfg, st, valid, first);
    sgd_tail_apply<<<grid, TAIL_THREADS, 0, stream>>>(entries, n_entries, chunks, n_chunks, (float)cfg.momentum,
                                                       (float)cfg.weight_decay[0], (float)cfg.weight_decay[1],
                                                       (float)cfg.weight_decay[2], (float)cfg.weight_decay[3], st, first);
    return hipGetLastError();
}

}  // namespace cabinet
