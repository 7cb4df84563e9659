// Per-token log-probabilities of a decode step, on the device: pc_token_logprobs.
//
// No reference counterpart (the reference returns text only).  One workgroup of 1024 threads per row of fp32 logits computes
// the log-softmax of the RAW row -- the model's own distribution, in front of temperature, repetition penalty, top-p and top-k --
// at the row's token and at the top_n most likely tokens, ordered by (value descending, index ascending): the project's "lowest
// index among equal maxima" rule, extended to the whole order.
//
// Two passes over the row and one workgroup reduction per further rank:
//   pass 0   the maximum m and its lowest index (rank 1)
//   pass 1   s = sum exp(x - m), and every thread's own candidate: the first of ITS elements behind rank 1 in the order
//   rank r   the first of the 1024 candidates; only the elements of the thread that held it are walked again, for its next
//            candidate behind the winner (by that thread out of its registers; for a row that is re-read, by the whole
//            workgroup, one group per thread) -- everybody else's candidate still stands
// Every thread reads the result of a reduction, so "behind rank r" is a register compare and no element is ever marked.  A row of
// at most 32 768 tokens (8 groups of 4 per thread) is loaded ONCE and every pass walks registers; a longer row is re-read from L2
// once per pass (513 KB at V = 128 256: it stays on-die).  Both walks visit a thread's tokens in the same order, so they give the
// same bits.  The kernel keeps no state and writes nothing but its two output rows, with ordinary vector stores from thread 0.
#include <math.h>

#include "pc_common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kNone = 0x7fffffff;

// values of tokens 4g .. 4g+3 (tokens past V: never visited by the callers' index test); NaN counts as -inf
__device__ __forceinline__ void load_group(const float* __restrict__ row, int V, bool al16, int g, float x[4]) {
    const int i = 4 * g;
    if (al16 && i + 3 < V) {
        const f4 t = *(const f4*)(row + i);
        x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = (i + e < V) ? row[i + e] : -INFINITY;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (x[e] != x[e]) x[e] = -INFINITY;
}

// f(index, value) for every token of this thread's groups, the loads of 4 groups in flight at a time (sample_row's walk)
template <typename F>
__device__ __forceinline__ void for_each_token(const float* __restrict__ row, int V, bool al16, F&& f) {
    const int G = (V + 3) >> 2;
    int g = threadIdx.x;
    for (; g + 3 * kThreads < G; g += 4 * kThreads) {
        float x[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) load_group(row, V, al16, g + u * kThreads, x[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * (g + u * kThreads) + e < V) f(4 * (g + u * kThreads) + e, x[u][e]);
    }
    for (; g < G; g += kThreads) {
        float x[4];
        load_group(row, V, al16, g, x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * g + e < V) f(4 * g + e, x[e]);
    }
}

// The row of a thread: kept in registers (REG: at most kRegGroups groups per thread, loaded once) or re-read on every walk.
constexpr int kRegGroups = 8;

template <bool REG>
struct RowWalk {
    const float* __restrict__ row;
    int V;
    bool al16;
    float x[REG ? kRegGroups : 1][4];

    __device__ __forceinline__ void load() {
        if (!REG) return;
        const int G = (V + 3) >> 2;
#pragma unroll
        for (int u = 0; u < kRegGroups; ++u) {
            const int g = threadIdx.x + u * kThreads;
            if (g < G) {
                load_group(row, V, al16, g, x[u]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[u][e] = -INFINITY;
            }
        }
    }

    template <typename F>
    __device__ __forceinline__ void each(F&& f) const {
        if (REG) {
#pragma unroll
            for (int u = 0; u < kRegGroups; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * ((int)threadIdx.x + u * kThreads) + e;
                    if (i < V) f(i, x[u][e]);
                }
        } else {
            for_each_token(row, V, al16, f);
        }
    }
};

// (v, i) is in front of (bv, bi) in the order: value descending, index ascending.  (-inf, kNone) is behind everything.
__device__ __forceinline__ bool in_front(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// The first element of the order over the whole workgroup, in every thread.  Two barriers: s_v / s_i may be reused at once.
__device__ __forceinline__ void block_first(float& v, int& i, float* s_v, int* s_i) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (in_front(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if (lane == 0) { s_v[wave] = v; s_i[wave] = i; }
    __syncthreads();
    v = lane < kWaves ? s_v[lane] : -INFINITY;
    i = lane < kWaves ? s_i[lane] : kNone;
#pragma unroll
    for (int o = kWaves / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (in_front(ov, oi, v, i)) { v = ov; i = oi; }
    }
    v = __shfl(v, 0);
    i = __shfl(i, 0);
    __syncthreads();
}

// The sum over the workgroup, in every thread: a tree over the 64 lanes, then over the 16 waves.
__device__ __forceinline__ float block_sum(float s, float* s_v) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) s_v[wave] = s;
    __syncthreads();
    s = lane < kWaves ? s_v[lane] : 0.0f;
#pragma unroll
    for (int o = kWaves / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    s = __shfl(s, 0);
    __syncthreads();
    return s;
}

template <bool REG>
__device__ __forceinline__ void logprobs_row(const float* __restrict__ row, int V, int64_t t, int top_n, int32_t* __restrict__ ids,
                                             float* __restrict__ lp, float* s_v, int* s_i) {
    const int tid = threadIdx.x;
    RowWalk<REG> w;
    w.row = row;
    w.V = V;
    w.al16 = ((uintptr_t)row & 15) == 0;
    w.load();

    // ---- pass 0: the maximum and its lowest index ----------------------------------------------------------------------------
    float m = -INFINITY;
    int i1 = kNone;
    w.each([&](int i, float x) {
        if (in_front(x, i, m, i1)) { m = x; i1 = i; }
    });
    block_first(m, i1, s_v, s_i);
    if (!(m > -INFINITY && m < INFINITY)) {                // nothing finite (or a +inf entry): no distribution (uniform exit)
        if (tid == 0)
            for (int j = 0; j <= top_n; ++j) { ids[j] = -1; lp[j] = NAN; }
        return;
    }

    // ---- pass 1: the softmax denominator, and this thread's candidate behind rank 1 ---------------------------------------
    float s = 0.0f, cv = -INFINITY;
    int ci = kNone;
    const bool second = top_n >= 2;
    w.each([&](int i, float x) {
        s += __expf(x - m);
        if (second && in_front(m, i1, x, i) && in_front(x, i, cv, ci)) { cv = x; ci = i; }
    });
    s = block_sum(s, s_v);
    const float logs = logf(s);
    if (tid == 0) {
        if (t >= 0 && t < V) {
            float x = row[t];
            if (x != x) x = -INFINITY;
            ids[0] = (int32_t)t;
            lp[0] = (x - m) - logs;
        } else {
            ids[0] = -1;
            lp[0] = NAN;
        }
        if (top_n >= 1) { ids[1] = i1; lp[1] = (m - m) - logs; }
    }

    // ---- ranks 2 ..: the first of the candidates; its owner alone looks for its next one ----------------------------------
    for (int rank = 2; rank <= top_n; ++rank) {
        float gv = cv;
        int gi = ci;
        block_first(gv, gi, s_v, s_i);
        if (tid == 0) { ids[rank] = gi; lp[rank] = (gv - m) - logs; }
        if (rank == top_n || gi == kNone) continue;        // (uniform; top_n < V leaves every rank a winner)
        if (REG) {
            if (ci == gi) {                                // one thread, out of its registers
                cv = -INFINITY;
                ci = kNone;
                w.each([&](int i, float x) {
                    if (in_front(gv, gi, x, i) && in_front(x, i, cv, ci)) { cv = x; ci = i; }
                });
            }
        } else {
            // the owner's groups are owner, owner + 1024, ...: one thread alone would wait for them load after load, so the
            // workgroup reads them together, one group per thread and round, and hands the owner the first of what it found
            const int owner = (gi >> 2) & (kThreads - 1), G = (V + 3) >> 2;
            float nv = -INFINITY;
            int ni = kNone;
            for (int64_t g = owner + (int64_t)tid * kThreads; g < G; g += (int64_t)kThreads * kThreads) {
                float x[4];
                load_group(row, V, w.al16, (int)g, x);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * (int)g + e;
                    if (i < V && in_front(gv, gi, x[e], i) && in_front(x[e], i, nv, ni)) { nv = x[e]; ni = i; }
                }
            }
            block_first(nv, ni, s_v, s_i);
            if (tid == owner) { cv = nv; ci = ni; }
        }
    }
}

__global__ __launch_bounds__(kThreads) void token_logprobs_kernel(const float* __restrict__ logits, int64_t ldl, int V,
                                                                  const int64_t* __restrict__ tok64, const int32_t* __restrict__ tok32,
                                                                  int64_t tok_stride, int top_n, int32_t* __restrict__ out_ids,
                                                                  float* __restrict__ out_lp) {
    __shared__ float s_v[kWaves];
    __shared__ int s_i[kWaves];
    const int r = blockIdx.x;
    const float* __restrict__ row = logits + (int64_t)r * ldl;
    const int64_t t = tok64 ? tok64[(int64_t)r * tok_stride] : (int64_t)tok32[(int64_t)r * tok_stride];
    int32_t* ids = out_ids + (int64_t)r * (1 + top_n);
    float* lp = out_lp + (int64_t)r * (1 + top_n);
    if (((V + 3) >> 2) <= kRegGroups * kThreads)           // (uniform over the launch)
        logprobs_row<true>(row, V, t, top_n, ids, lp, s_v, s_i);
    else
        logprobs_row<false>(row, V, t, top_n, ids, lp, s_v, s_i);
}

}  // namespace

PC_EXPORT int pc_token_logprobs(const float* logits, int64_t ldl, int32_t vocab, int32_t rows, const int64_t* tok64, const int32_t* tok32,
                                int64_t tok_stride, int32_t top_n, int32_t* out_ids, float* out_lp, void* stream) {
    PC_REQUIRE(logits && out_ids && out_lp, PC_ERR_ARG, "pc_token_logprobs: null pointer");
    PC_REQUIRE((tok64 != nullptr) != (tok32 != nullptr), PC_ERR_ARG, "pc_token_logprobs: exactly one of tok64 and tok32");
    PC_REQUIRE(rows >= 1 && rows <= 64 && top_n >= 0 && top_n <= PC_LOGPROBS_MAX_TOP && tok_stride >= 1, PC_ERR_ARG,
               "pc_token_logprobs: need 1 <= rows <= 64, 0 <= top_n <= %d, tok_stride >= 1", PC_LOGPROBS_MAX_TOP);
    PC_REQUIRE(vocab > top_n && vocab < (1 << 24) && ldl >= vocab, PC_ERR_ARG,
               "pc_token_logprobs: need top_n < vocab < 2^24 and a row stride of at least vocab");
    PC_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)tok64 & 7) == 0 && ((uintptr_t)tok32 & 3) == 0 &&
                   ((uintptr_t)out_ids & 3) == 0 && ((uintptr_t)out_lp & 3) == 0, PC_ERR_ARG,
               "pc_token_logprobs: logits, tok32 and the outputs must be 4-byte, tok64 8-byte aligned");
    hipLaunchKernelGGL(token_logprobs_kernel, dim3(rows), dim3(kThreads), 0, (hipStream_t)stream, logits, ldl, vocab, tok64, tok32,
                       tok_stride, top_n, out_ids, out_lp);
    return pc_check_launch("token_logprobs_kernel");
}
