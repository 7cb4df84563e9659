// Token controls of a decode step, on the device: pc_logit_adjust.
//
// No reference counterpart (the reference has a fixed processor chain: temperature, penalty, top-p, top-k).  The kernel makes the
// ADJUSTED copy of fp32 logits rows that the samplers then read in place of the raw rows: logit_bias (a ban is a bias of -inf), an
// allow-list (one bit per token) and min_new_tokens (the stop ids are -inf while the row's token number is below the minimum).  It
// writes out of place, so whoever wants the model's own distribution (pc_token_logprobs) keeps reading the raw rows.
//
// The row is a streaming copy; the sparse passes touch at most 64 + 8 elements.  A workgroup of 256 threads owns kChunk = 2048
// columns of one row (grid: column chunks x rows) and applies only the table entries that fall into its columns, so no element is
// ever written by two workgroups.  Inside the workgroup the writes to one element are ordered across workgroup barriers:
//   pass 0   every column of the chunk: out[j] = allowed(j) ? x[j] : -inf                  (16-byte loads and stores)
//   barrier
//   pass 1   thread t < n_bias, bias_id[t] in the chunk: out[id] = allowed(id) ? x[id] + bias[t] : -inf   (ids are distinct)
//   barrier
//   pass 2   thread 0, while the row's token number is below the minimum: out[stop] = -inf for the stop ids in the chunk
// which is the rule "bias, then allow-list, then stop ids" on every element: x + bias is one fp32 add (x + (-inf) = -inf, NaN stays
// NaN), a disallowed token is -inf whatever its bias, and a suppressed stop id is -inf whatever else.  No state, no counter, no
// atomic; nothing but `out` is written, with ordinary vector stores.
#include <math.h>

#include "pc_common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kChunk = 2048;             // columns per workgroup: two 16-byte groups per thread, both loads in flight

__device__ __forceinline__ bool allowed_at(const uint32_t* __restrict__ bits, int j) {
    return bits == nullptr || ((bits[j >> 5] >> (j & 31)) & 1u) != 0;
}

__global__ __launch_bounds__(kThreads) void logit_adjust_kernel(const float* __restrict__ logits, int64_t ldl, int V, int rows_per_slot,
                                                                const pc_logit_ctl* __restrict__ ctl,
                                                                const uint32_t* __restrict__ allowed_bits,
                                                                const int32_t* __restrict__ len, float* __restrict__ out, int64_t ldo) {
    const int r = blockIdx.y, b = r / rows_per_slot, i = r - b * rows_per_slot;
    const int c0 = blockIdx.x * kChunk, c1 = min(c0 + kChunk, V);
    const pc_logit_ctl* __restrict__ c = ctl + b;
    const float* __restrict__ x = logits + (int64_t)r * ldl;
    float* __restrict__ y = out + (int64_t)r * ldo;
    const int words = (V + 31) >> 5;
    // (uniform over the workgroup) the slot's allowed row, or null: every token is allowed
    const uint32_t* __restrict__ bits = (allowed_bits != nullptr && c->use_allowed != 0) ? allowed_bits + (int64_t)b * words : nullptr;
    const bool al16 = ((uintptr_t)x & 15) == 0;          // c0 is a multiple of 4, so the row base decides for every group

    // ---- pass 0: the streaming copy under the allow-list ------------------------------------------------------------------------
    float v[2][4];
    uint32_t m[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int j = c0 + 4 * ((int)threadIdx.x + u * kThreads);
        m[u] = 0xfu;
        if (j < c1) {
            if (al16 && j + 3 < V) {
                const f4 t = *(const f4*)(x + j);
                v[u][0] = t[0]; v[u][1] = t[1]; v[u][2] = t[2]; v[u][3] = t[3];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[u][e] = (j + e < V) ? x[j + e] : 0.0f;
            }
            if (bits != nullptr) m[u] = bits[j >> 5] >> (j & 31);      // (j % 4 == 0: the group's four bits lie in one word)
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int j = c0 + 4 * ((int)threadIdx.x + u * kThreads);
        if (j >= c1) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (!((m[u] >> e) & 1u)) v[u][e] = -INFINITY;
        if (j + 3 < V) {
            f4 t;
            t[0] = v[u][0]; t[1] = v[u][1]; t[2] = v[u][2]; t[3] = v[u][3];
            *(f4*)(y + j) = t;                            // (out is 16-byte aligned and ldo % 4 == 0)
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < V) y[j + e] = v[u][e];
        }
    }
    __syncthreads();

    // ---- pass 1: the bias table, one entry per thread (distinct ids: no two threads meet) ----------------------------------------
    const int nb = min(max(c->n_bias, 0), PC_LOGIT_BIAS_MAX);
    if ((int)threadIdx.x < nb) {
        const int id = c->bias_id[threadIdx.x];
        if (id >= c0 && id < c1)                          // (c1 <= V: ids outside [0, vocab) fall into no chunk)
            y[id] = allowed_at(bits, id) ? x[id] + c->bias[threadIdx.x] : -INFINITY;
    }
    __syncthreads();

    // ---- pass 2: the stop ids, while this row's token number is below the minimum -------------------------------------------------
    if (threadIdx.x == 0 && (len != nullptr ? len[b] : 0) + i < c->stop_free_len) {
#pragma unroll
        for (int s = 0; s < PC_LOGIT_STOP_MAX; ++s) {
            const int id = c->stop_ids[s];
            if (id >= c0 && id < c1) y[id] = -INFINITY;
        }
    }
}

}  // namespace

PC_EXPORT int pc_logit_adjust(const float* logits, int64_t ldl, int32_t vocab, int32_t S, int32_t rows_per_slot, const pc_logit_ctl* ctl,
                              const uint32_t* allowed_bits, const int32_t* len, float* out, int64_t ldo, void* stream) {
    PC_REQUIRE(logits && ctl && out, PC_ERR_ARG, "pc_logit_adjust: null pointer");
    PC_REQUIRE(S >= 1 && rows_per_slot >= 1 && rows_per_slot <= 16 && (int64_t)S * rows_per_slot <= 64, PC_ERR_ARG,
               "pc_logit_adjust: need S >= 1, 1 <= rows_per_slot <= 16 and S * rows_per_slot <= 64");
    PC_REQUIRE(vocab >= 1 && vocab < (1 << 24) && ldl >= vocab && ldo >= vocab && (ldo & 3) == 0, PC_ERR_ARG,
               "pc_logit_adjust: need 1 <= vocab < 2^24, row strides of at least vocab and ldo %% 4 == 0");
    PC_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)ctl & 3) == 0 &&
                   ((uintptr_t)allowed_bits & 3) == 0 && ((uintptr_t)len & 3) == 0, PC_ERR_ARG,
               "pc_logit_adjust: logits, ctl, allowed_bits and len must be 4-byte, out 16-byte aligned");
    PC_REQUIRE((const void*)logits != (const void*)out, PC_ERR_ARG, "pc_logit_adjust: out must not be the logits (it writes out of place)");
    const dim3 grid(pc_ceil_div(vocab, kChunk), S * rows_per_slot);
    hipLaunchKernelGGL(logit_adjust_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, logits, ldl, vocab, rows_per_slot, ctl,
                       allowed_bits, len, out, ldo);
    return pc_check_launch("logit_adjust_kernel");
}
