// K21: gradient accumulation across hipGraph replays -- one recorded launch pair that serves every micro-step of a window.
// Inside a captured backward autograd writes each gradient into a static tensor of its own and overwrites it on every replay
// (train.py: _capture_both_branches relies on it), so the reference's accumulation contract (src/scripts/train.py:435-439:
// loss / accum_steps per micro-batch, the optimizer on every accum_steps-th) needs a device-side pass over all gradient tensors:
//
//   grad_accum       per element: acc = grad on a window's first micro-step (acc is NOT read: a stale NaN does not survive and
//                    -0.0 stays -0.0), acc = acc + grad on every later one (one fp32 add: no scale factor, no FMA -- the same
//                    bits as autograd's own accumulation in the same order)
//   grad_accum_bump  ONE lane: micro += 1, a plain store, in a launch of its own BEHIND the pass on the stream
//
// Which of the two forms runs is read from the device state (int32 `micro`), so the same graph node serves first and later
// micro-steps and nothing is read on the host.  Every workgroup of the pass must see the same `micro`: advancing it inside the
// pass (an atomic, or "the last workgroup stores") would let a workgroup that starts late read the advanced value; a one-lane
// launch that follows on the stream cannot.  No scratch, no atomics, no reduction: the result does not depend on the grid.
//
// Tables follow K16 (opt_tail.hip): entries and chunks in device memory, chunks of <= 4096 elements that start at a multiple of
// 4096 inside their tensor; where both pointers of a chunk are 16-byte aligned its body moves as float4 (4 per array and thread,
// all loads issued before the adds) and the last length % 4 elements as scalars, otherwise the whole chunk moves as scalars.
#include "../../include/cabinet_hip.h"
#include "common.hpp"

#include <stdint.h>

namespace cabinet {

constexpr int ACCUM_THREADS = 256;
constexpr int ACCUM_CHUNK = CABINET_SGD_TAIL_CHUNK;  // 4096
constexpr int ACCUM_GRID_CAP = 2048;
constexpr int ACCUM_STATE_BYTES = 64;

// The table hands out generic pointers; every array is device memory, so the accesses are stated as global ones (global_load /
// global_store: one counter to wait on and no aperture check, where a generic pointer compiles to flat_load / flat_store).
typedef float vec4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) vec4* gvec4_p;
typedef const __attribute__((address_space(1))) vec4* gvec4_cp;
typedef __attribute__((address_space(1))) float* gfloat_p;
typedef const __attribute__((address_space(1))) float* gfloat_cp;

// device state block (the header's layout comment is the contract; Python reads `micro` through a view)
struct AccumState {
    int micro;  //  0  micro-steps folded into acc in the current window
};
static_assert(sizeof(AccumState) <= ACCUM_STATE_BYTES, "state block");

__global__ __launch_bounds__(ACCUM_THREADS) void grad_accum(const cabinet_grad_accum_entry* __restrict__ entries, int n_entries,
                                                             const cabinet_sgd_tail_chunk* __restrict__ chunks, int n_chunks,
                                                             const AccumState* __restrict__ st) {
    const int t = threadIdx.x;
    const bool first = st->micro == 0;  // the same value in every workgroup: it is advanced by the launch behind this one
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const cabinet_sgd_tail_chunk ck = chunks[c];
        if (ck.tensor < 0 || ck.tensor >= n_entries || ck.length <= 0 || ck.length > ACCUM_CHUNK || ck.start < 0) continue;
        const cabinet_grad_accum_entry e = entries[ck.tensor];
        const int len = ck.length;
        if (ck.start + len > e.numel || !e.acc || !e.grad) continue;  // a chunk never leaves its tensor, whatever the table says
        const gfloat_p a = (gfloat_p)(e.acc + ck.start);
        const gfloat_cp g = (gfloat_cp)(e.grad + ck.start);
        const bool vec = ((reinterpret_cast<uintptr_t>(e.acc + ck.start) | reinterpret_cast<uintptr_t>(e.grad + ck.start)) & 15) == 0;
        const int nvec = vec ? (len >> 2) : 0;
        const gvec4_p a4 = (gvec4_p)a;
        const gvec4_cp g4 = (gvec4_cp)g;
        if (first) {
            vec4 gv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = j * ACCUM_THREADS + t;
                gv[j] = vec4{0.f, 0.f, 0.f, 0.f};
                if (v < nvec) gv[j] = g4[v];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = j * ACCUM_THREADS + t;
                if (v < nvec) a4[v] = gv[j];
            }
            for (int i = nvec * 4 + t; i < len; i += ACCUM_THREADS) a[i] = g[i];
            continue;
        }
        // all loads of the chunk's float4 body first (4 per array and thread), then the adds, then the stores
        vec4 av[4], gv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = j * ACCUM_THREADS + t;
            av[j] = gv[j] = vec4{0.f, 0.f, 0.f, 0.f};
            if (v < nvec) {
                av[j] = a4[v];
                gv[j] = g4[v];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = j * ACCUM_THREADS + t;
            if (v < nvec) a4[v] = av[j] + gv[j];  // four fp32 adds, element for element (the build has -ffp-contract=off)
        }
        for (int i = nvec * 4 + t; i < len; i += ACCUM_THREADS) a[i] = a[i] + g[i];
    }
}

__global__ void grad_accum_bump(AccumState* __restrict__ st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int m = st->micro;
        st->micro = m < 0x7fffffff ? m + 1 : m;
    }
}

__global__ void grad_accum_zero(AccumState* __restrict__ st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) st->micro = 0;
}

// ---------------------------------------------------------------------------------------------------------------- host
size_t grad_accum_state() { return ACCUM_STATE_BYTES; }

hipError_t grad_accum_run(const cabinet_grad_accum_entry* entries, int n_entries, const cabinet_sgd_tail_chunk* chunks, int n_chunks,
                          void* state, int max_grid, hipStream_t stream) {
    const int cap = max_grid > 0 ? (max_grid < ACCUM_GRID_CAP ? max_grid : ACCUM_GRID_CAP) : ACCUM_GRID_CAP;
    const int grid = n_chunks < cap ? n_chunks : cap;
    AccumState* st = static_cast<AccumState*>(state);
    grad_accum<<<grid, ACCUM_THREADS, 0, stream>>>(entries, n_entries, chunks, n_chunks, st);
    grad_accum_bump<<<1, 64, 0, stream>>>(st);
    return hipGetLastError();
}

hipError_t grad_accum_reset_run(void* state, hipStream_t stream) {
    grad_accum_zero<<<1, 64, 0, stream>>>(static_cast<AccumState*>(state));
    return hipGetLastError();
}

}  // namespace cabinet
