// Prompt-lookup speculative decoding, the two ends of a device-side step (model/llama_hip.py LookupLoop):
//   pc_lookup_draft   first node: copy the tokens that followed the most recent earlier occurrence of the history's suffix
//   pc_lookup_verify  last node:  per-row argmax of the k+1-row forward, longest agreeing prefix + one bonus token, state advance
// (and, between two replays of the step over slots, pc_lookup_slot_arm: admission of one sequence into a running loop)
// Between them runs the ordinary <= 16-row forward over the ids / positions / past length these kernels keep in device words,
// so a replay of the captured step needs nothing from the host.  The result is greedy decoding (the accepted tokens ARE the
// model's argmax at their positions); only the number of tokens per weight stream varies.
#include "pc_common.h"
#include "pc_lookup_common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kDraftThreads = 1024;
constexpr int kMaxRows = 16;          // k + 1 <= 16: the row tile of the weight-streaming projections
constexpr int kMaxNgram = 8;
constexpr int kMaxSlotRows = 64;     // S * (k + 1): the most rows the weight-streaming projections take

// One workgroup.  With h = hist[0..L) and h[L-1] the token the step feeds (ids[0]): a follower index e in [1, L-1] has match
// length ml(e) = the largest t <= nmax with h[e-t..e) == h[L-t..L) (t <= e).  The candidates of suffix length n are the
// j = e - n with ml(e) >= n, so "the longest n that has a candidate, and of those the largest j" is the maximum of
// (ml(e), e) in lexicographic order: ONE max-reduction of ml << 24 | e over e (hist_cap < 2^24).
__device__ __forceinline__ void lookup_draft_rule(const int32_t* __restrict__ hist, const int32_t* __restrict__ hist_len, int hist_cap,
                                                  int64_t* ids, int32_t* pos, int32_t* ndraft, int k, int nmax, int* s_best,
                                                  int& s_key) {
    const int tid = threadIdx.x;
    int L = hist_len[0];
    L = L < 0 ? 0 : (L > hist_cap ? hist_cap : L);
    int suf[kMaxNgram];                                   // suf[t-1] = h[L-t]
#pragma unroll
    for (int t = 1; t <= kMaxNgram; ++t) suf[t - 1] = (t <= nmax && L - t >= 0) ? hist[L - t] : -1;
    int best = 0;
    for (int e = 1 + tid; e < L; e += kDraftThreads) {
        int ml = 0;
#pragma unroll
        for (int t = 1; t <= kMaxNgram; ++t) {
            // (unrolled with the suffix in registers; a failed position ends the run)
            if (ml == t - 1 && t <= nmax && e - t >= 0 && hist[e - t] == suf[t - 1]) ml = t;
        }
        const int key = ml > 0 ? ((ml << 24) | e) : 0;
        best = key > best ? key : best;                   // (e grows along the loop: the later follower wins within a lane too)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_xor(best, o);
        best = ob > best ? ob : best;
    }
    if ((tid & 63) == 0) s_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kDraftThreads / 64; ++w) best = s_best[w] > best ? s_best[w] : best;
        s_key = best;
    }
    __syncthreads();
    const int key = s_key;
    const int e0 = key & 0xffffff;                        // index of the first follower (0: no candidate)
    int m = key ? L - e0 : 0;
    m = m < k ? m : k;
    const int64_t id0 = ids[0];
    const int p0 = pos[0];
    if (tid < k) ids[1 + tid] = tid < m ? (int64_t)hist[e0 + tid] : id0;      // pad rows: a valid embedding row
    if (tid >= 1 && tid <= k) pos[tid] = p0 + tid;
    if (tid == 0) ndraft[0] = m;
}

__global__ __launch_bounds__(kDraftThreads) void lookup_draft_kernel(const int32_t* __restrict__ hist, const int32_t* __restrict__ hist_len,
                                                                      int hist_cap, int64_t* ids, int32_t* pos, int32_t* ndraft,
                                                                      int k, int nmax) {
    __shared__ int s_best[kDraftThreads / 64];
    __shared__ int s_key;
    lookup_draft_rule(hist, hist_len, hist_cap, ids, pos, ndraft, k, nmax, s_best, s_key);
}

// One workgroup per slot: the rule above on the slot's own history and words.  `forced` (null: pc_lookup_draft_slots): a slot
// with forced rows feeds its question instead (lookup_draft_forced_rule; uniform over the workgroup).
__global__ __launch_bounds__(kDraftThreads) void lookup_draft_slots_kernel(const int32_t* __restrict__ hist,
                                                                            const int32_t* __restrict__ hist_len, int hist_cap,
                                                                            int64_t* ids, int32_t* pos, int32_t* ndraft,
                                                                            const int32_t* __restrict__ cap, const int32_t* __restrict__ len,
                                                                            const int32_t* __restrict__ live, int k, int nmax,
                                                                            const int32_t* __restrict__ forced) {
    __shared__ int s_best[kDraftThreads / 64];
    __shared__ int s_key;
    const int b = blockIdx.x;
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
    if (const int R = lookup_forced_rows(forced, b)) {
        lookup_draft_forced_rule(hist + (int64_t)b * hist_cap, hist_len[b], hist_cap, ids + (int64_t)b * (k + 1), pos + (int64_t)b * (k + 1),
                                 ndraft + b, k, R);
        return;
    }
    lookup_draft_rule(hist + (int64_t)b * hist_cap, hist_len + b, hist_cap, ids + (int64_t)b * (k + 1), pos + (int64_t)b * (k + 1),
                      ndraft + b, k, nmax, s_best, s_key);
}

// a[row] = argmax(logits[row][0..V)), the lowest index among equal maxima (greedy_advance_kernel's rule, all -inf / NaN -> 0).
// One workgroup per row.  The row need only be 4-byte aligned: a scalar head up to the first 16-byte boundary, float4 body,
// scalar tail; a lane meets its indices in increasing order, so "strictly greater" keeps the lowest index.
__global__ __launch_bounds__(1024) void lookup_argmax_kernel(const float* __restrict__ logits, int64_t ld, int V, int32_t* __restrict__ amax) {
    __shared__ float sv[16];
    __shared__ int si[16];
    const int tid = threadIdx.x;
    const float* row = logits + (int64_t)blockIdx.x * ld;
    int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    head = head < V ? head : V;
    const int nvec = (V - head) >> 2;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if (tid < head) {
        const float x = row[tid];
        if (x > best) { best = x; bi = tid; }
    }
    const f4* body = (const f4*)(row + head);
    for (int v = tid; v < nvec; v += 1024) {
        const f4 x = body[v];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x[e] > best) { best = x[e]; bi = head + 4 * v + e; }
    }
    const int t0 = head + 4 * nvec;
    if (t0 + tid < V) {                                   // (< 4 elements)
        const float x = row[t0 + tid];
        if (x > best) { best = x; bi = t0 + tid; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
        if (bi == 0x7fffffff) bi = 0;
        amax[blockIdx.x] = bi;
    }
}

// One wave: lookup_accept_rule (pc_lookup_common.h) on the per-row argmax.
__global__ __launch_bounds__(64) void lookup_accept_kernel(const int32_t* __restrict__ amax, int rows, int32_t* hist, int32_t* hist_len,
                                                           int hist_cap, int64_t* ids, int32_t* pos, int32_t* past, const int32_t* ndraft,
                                                           int32_t* budget, int32_t* ring, int32_t* ctr, int ring_cap) {
    const int a = (int)threadIdx.x < rows ? amax[threadIdx.x] : 0;
    lookup_accept_rule(a, rows, hist, hist_len, hist_cap, ids, pos, past, ndraft, budget, ring, ctr, ring_cap);
}

// One wave per slot: lookup_accept_slots_rule (pc_lookup_common.h) on the per-row argmax.
__global__ __launch_bounds__(64) void lookup_accept_slots_kernel(const int32_t* __restrict__ amax, int rows, int32_t* hist, int32_t* hist_len,
                                                                 int hist_cap, int64_t* ids, int32_t* pos, int32_t* len,
                                                                 const int32_t* __restrict__ cap, int32_t* live, const int32_t* ndraft,
                                                                 int32_t* budget, const int32_t* __restrict__ stop_ids, int32_t* ring,
                                                                 int32_t* ctr, int ring_cap) {
    int a;
    lookup_accept_slots_rule(amax + blockIdx.x * rows, rows, blockIdx.x, hist, hist_len, hist_cap, ids, pos, len, cap, live, ndraft, budget,
                             stop_ids, ring, ctr, ring_cap, a);
}

// ---- pc_lookup_slot_arm: every word of ONE slot of the lookup step from a pinned host block, one launch -----------------------
// pc_slot_arm (pc_slots.hip) for the words of pc_lookup_verify_slots_each's step: the launch sits on the stream between two
// replays, the block is host memory read with system-scope loads, live[slot] = 1 is the last store.  One workgroup: the header
// goes through LDS, the bitmap row and the history ids are copied by all threads, two 32-bit words per load.
// `forced` (null: pc_lookup_slot_arm): pc_lookup_slot_arm_prompt -- the last n_forced ids of the block are a question still to be
// fed: they are copied behind hist_len like the rest, and the slot starts with hist_len - n_forced, forced = n_forced, draws = 0.
constexpr int kLookupArmWords = (int)(sizeof(pc_lookup_slot_arm_block) / 8);

__global__ __launch_bounds__(kDraftThreads) void lookup_slot_arm_kernel(const unsigned long long* __restrict__ src, pc_lookup_slot_state st,
                                                                        int S, int k, int hw, int hist_cap, int32_t* forced,
                                                                        int n_forced) {
    typedef __attribute__((address_space(1))) unsigned long long g64;
    __shared__ __attribute__((aligned(8))) unsigned long long h[kLookupArmWords];
    const int tid = threadIdx.x;
    if (tid < kLookupArmWords) h[tid] = __hip_atomic_load((g64*)(src + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    const pc_lookup_slot_arm_block& b = *(const pc_lookup_slot_arm_block*)h;
    const int s = b.slot, hl = b.hist_len;
    if (s < 0 || s >= S || b.hist_words != hw || hl < 1 || hl > hist_cap || n_forced >= hl) return;      // (the block changed under the launch: touch nothing)
    const unsigned long long* bits = src + kLookupArmWords;
    const unsigned long long* hids = bits + (hw + 1) / 2;
    uint32_t* row = st.history_bits + (int64_t)s * hw;
    for (int i = tid; 2 * i < hw; i += kDraftThreads) {
        const unsigned long long w = __hip_atomic_load((g64*)(bits + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        row[2 * i] = (uint32_t)w;
        if (2 * i + 1 < hw) row[2 * i + 1] = (uint32_t)(w >> 32);
    }
    int32_t* hrow = st.hist + (int64_t)s * hist_cap;
    for (int i = tid; 2 * i < hl; i += kDraftThreads) {
        const unsigned long long w = __hip_atomic_load((g64*)(hids + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        hrow[2 * i] = (int32_t)(uint32_t)w;
        if (2 * i + 1 < hl) hrow[2 * i + 1] = (int32_t)(uint32_t)(w >> 32);
    }
    if (tid == 0) {
        st.kv_base[s] = b.kv_base;
        st.cap[s] = b.cap;
        st.len[s] = b.len;
        st.leader[s] = b.leader;
        st.trunk[s] = b.trunk;
        st.budget[s] = b.budget;
        st.counters[s] = b.counter;
        st.draws[s] = forced ? 0 : 1;
        st.seeds[s] = b.seed;
        st.params[s] = b.params;
        st.ids[(int64_t)s * (k + 1)] = b.id;
        st.pos[(int64_t)s * (k + 1)] = b.pos;
        st.ndraft[s] = 0;
        st.hist_len[s] = hl - n_forced;
        if (forced) forced[s] = n_forced;
    } else if (tid >= 64 && tid < 72) {
        st.stop_ids[s * 8 + tid - 64] = b.stop_ids[tid - 64];
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) st.live[s] = 1;
}

}  // namespace

PC_EXPORT int pc_lookup_draft(const int32_t* hist, const int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos,
                              int32_t* ndraft, int32_t k, int32_t nmax, void* stream) {
    PC_REQUIRE(hist && hist_len && ids && pos && ndraft, PC_ERR_ARG, "pc_lookup_draft: null pointer");
    PC_REQUIRE(k >= 1 && k < kMaxRows && nmax >= 1 && nmax <= kMaxNgram && hist_cap >= 1 && hist_cap < (1 << 24), PC_ERR_ARG,
               "pc_lookup_draft: need 1 <= k <= %d, 1 <= nmax <= %d, 1 <= hist_cap < 2^24", kMaxRows - 1, kMaxNgram);
    hipLaunchKernelGGL(lookup_draft_kernel, dim3(1), dim3(kDraftThreads), 0, (hipStream_t)stream, hist, hist_len, hist_cap, ids, pos,
                       ndraft, k, nmax);
    return pc_check_launch("lookup_draft_kernel");
}

PC_EXPORT int pc_lookup_verify(const float* logits, int64_t ldl, int32_t vocab, int32_t rows, int32_t* row_argmax, int32_t* hist,
                               int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* past_len,
                               const int32_t* ndraft, int32_t* budget, int32_t* ring, int32_t* counter, int32_t ring_cap,
                               void* stream) {
    PC_REQUIRE(logits && row_argmax && hist && hist_len && ids && pos && past_len && ndraft && budget && ring && counter, PC_ERR_ARG,
               "pc_lookup_verify: null pointer");
    PC_REQUIRE(rows >= 1 && rows <= kMaxRows && vocab > 0 && ldl >= vocab && ring_cap > 0 && hist_cap >= 1, PC_ERR_ARG,
               "pc_lookup_verify: need 1 <= rows <= %d, vocab > 0, ldl >= vocab, ring_cap > 0", kMaxRows);
    PC_REQUIRE(((uintptr_t)logits & 3) == 0, PC_ERR_ARG, "pc_lookup_verify: logits must be 4-byte aligned");
    hipLaunchKernelGGL(lookup_argmax_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)stream, logits, ldl, vocab, row_argmax);
    int rc = pc_check_launch("lookup_argmax_kernel");
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(lookup_accept_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, row_argmax, rows, hist, hist_len, hist_cap, ids,
                       pos, past_len, ndraft, budget, ring, counter, ring_cap);
    return pc_check_launch("lookup_accept_kernel");
}

namespace {

// pc_lookup_draft_slots (forced null) and pc_lookup_draft_slots_prompt
int draft_slots(const char* name, const int32_t* hist, const int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos,
                int32_t* ndraft, const int32_t* cap, const int32_t* len, const int32_t* live, const int32_t* forced, int32_t S, int32_t k,
                int32_t nmax, void* stream) {
    PC_REQUIRE(hist && hist_len && ids && pos && ndraft && cap && len && live, PC_ERR_ARG, "%s: null pointer", name);
    PC_REQUIRE(S >= 1 && S <= 16 && k >= 1 && k < kMaxRows && S * (k + 1) <= kMaxSlotRows && nmax >= 1 && nmax <= kMaxNgram &&
                   hist_cap >= 1 && hist_cap < (1 << 24), PC_ERR_ARG,
               "%s: need 1 <= S <= 16, 1 <= k <= %d, S * (k + 1) <= %d, 1 <= nmax <= %d, 1 <= hist_cap < 2^24", name,
               kMaxRows - 1, kMaxSlotRows, kMaxNgram);
    hipLaunchKernelGGL(lookup_draft_slots_kernel, dim3(S), dim3(kDraftThreads), 0, (hipStream_t)stream, hist, hist_len, hist_cap, ids, pos,
                       ndraft, cap, len, live, k, nmax, forced);
    return pc_check_launch("lookup_draft_slots_kernel");
}

}  // namespace

PC_EXPORT int pc_lookup_draft_slots(const int32_t* hist, const int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos,
                                    int32_t* ndraft, const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t k,
                                    int32_t nmax, void* stream) {
    return draft_slots("pc_lookup_draft_slots", hist, hist_len, hist_cap, ids, pos, ndraft, cap, len, live, nullptr, S, k, nmax, stream);
}

PC_EXPORT int pc_lookup_draft_slots_prompt(const int32_t* hist, const int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos,
                                           int32_t* ndraft, const int32_t* cap, const int32_t* len, const int32_t* live,
                                           const int32_t* forced, int32_t S, int32_t k, int32_t nmax, void* stream) {
    PC_REQUIRE(forced, PC_ERR_ARG, "pc_lookup_draft_slots_prompt: null pointer");
    return draft_slots("pc_lookup_draft_slots_prompt", hist, hist_len, hist_cap, ids, pos, ndraft, cap, len, live, forced, S, k, nmax,
                       stream);
}

PC_EXPORT int pc_lookup_verify_slots(const float* logits, int64_t ldl, int32_t vocab, int32_t S, int32_t k, int32_t* row_argmax,
                                     int32_t* hist, int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* len,
                                     const int32_t* cap, int32_t* live, const int32_t* ndraft, int32_t* budget, const int32_t* stop_ids,
                                     int32_t* ring, int32_t* counters, int32_t ring_cap, void* stream) {
    PC_REQUIRE(logits && row_argmax && hist && hist_len && ids && pos && len && cap && live && ndraft && budget && stop_ids && ring &&
                   counters, PC_ERR_ARG, "pc_lookup_verify_slots: null pointer");
    PC_REQUIRE(S >= 1 && S <= 16 && k >= 1 && k < kMaxRows && S * (k + 1) <= kMaxSlotRows && vocab > 0 && ldl >= vocab && ring_cap > 0 &&
                   hist_cap >= 1, PC_ERR_ARG,
               "pc_lookup_verify_slots: need 1 <= S <= 16, 1 <= k <= %d, S * (k + 1) <= %d, vocab > 0, ldl >= vocab, ring_cap > 0",
               kMaxRows - 1, kMaxSlotRows);
    PC_REQUIRE(((uintptr_t)logits & 3) == 0, PC_ERR_ARG, "pc_lookup_verify_slots: logits must be 4-byte aligned");
    hipLaunchKernelGGL(lookup_argmax_kernel, dim3(S * (k + 1)), dim3(1024), 0, (hipStream_t)stream, logits, ldl, vocab, row_argmax);
    int rc = pc_check_launch("lookup_argmax_kernel");
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(lookup_accept_slots_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, row_argmax, k + 1, hist, hist_len, hist_cap,
                       ids, pos, len, cap, live, ndraft, budget, stop_ids, ring, counters, ring_cap);
    return pc_check_launch("lookup_accept_slots_kernel");
}

namespace {

// pc_lookup_slot_arm (forced null, n_forced 0) and pc_lookup_slot_arm_prompt
int slot_arm(const char* name, const pc_lookup_slot_arm_block* host_block, int32_t nbytes, const pc_lookup_slot_state* state,
             int32_t* forced, int32_t n_forced, int32_t S, int32_t k, int32_t hist_cap, void* stream) {
    PC_REQUIRE(host_block && state, PC_ERR_ARG, "%s: null pointer", name);
    PC_REQUIRE(state->kv_base && state->cap && state->len && state->live && state->leader && state->trunk && state->ids && state->pos &&
                   state->ndraft && state->budget && state->hist_len && state->counters && state->draws && state->seeds && state->params &&
                   state->stop_ids && state->history_bits && state->hist, PC_ERR_ARG, "%s: null pointer in the slot state", name);
    PC_REQUIRE(S >= 1 && S <= 16 && k >= 1 && k < kMaxRows && S * (k + 1) <= kMaxSlotRows && hist_cap >= 1 && hist_cap < (1 << 24), PC_ERR_ARG,
               "%s: need 1 <= S <= 16, 1 <= k <= %d, S * (k + 1) <= %d, 1 <= hist_cap < 2^24", name, kMaxRows - 1, kMaxSlotRows);
    PC_REQUIRE(((uintptr_t)host_block & 7) == 0 && ((uintptr_t)state->params & 7) == 0 && ((uintptr_t)state->seeds & 7) == 0 &&
                   ((uintptr_t)state->kv_base & 7) == 0 && ((uintptr_t)state->ids & 7) == 0, PC_ERR_ARG,
               "%s: the block and the 64-bit state arrays must be 8-byte aligned", name);
    const int32_t slot = host_block->slot, hw = host_block->hist_words, hl = host_block->hist_len;   // (pinned HOST memory: readable here)
    PC_REQUIRE(slot >= 0 && slot < S, PC_ERR_ARG, "%s: slot outside [0, S)", name);
    PC_REQUIRE(hw >= 1 && hw <= (1 << 19) && hl >= 1 && hl <= hist_cap, PC_ERR_ARG,
               "%s: need 1 <= hist_words <= 2^19 and 1 <= hist_len <= hist_cap", name);
    PC_REQUIRE(n_forced >= 0 && n_forced < hl, PC_ERR_ARG, "%s: n_forced must be in [0, hist_len)", name);
    PC_REQUIRE((int64_t)nbytes == (int64_t)sizeof(pc_lookup_slot_arm_block) + (((int64_t)hw * 4 + 7) & ~(int64_t)7) +
                                      (((int64_t)hl * 4 + 7) & ~(int64_t)7), PC_ERR_ARG,
               "%s: nbytes must be sizeof(pc_lookup_slot_arm_block) + 4 * hist_words + 4 * hist_len, each rounded up to 8", name);
    hipLaunchKernelGGL(lookup_slot_arm_kernel, dim3(1), dim3(kDraftThreads), 0, (hipStream_t)stream, (const unsigned long long*)host_block,
                       *state, S, k, hw, hist_cap, forced, n_forced);
    return pc_check_launch("lookup_slot_arm_kernel");
}

}  // namespace

PC_EXPORT int pc_lookup_slot_arm(const pc_lookup_slot_arm_block* host_block, int32_t nbytes, const pc_lookup_slot_state* state, int32_t S,
                                 int32_t k, int32_t hist_cap, void* stream) {
    return slot_arm("pc_lookup_slot_arm", host_block, nbytes, state, nullptr, 0, S, k, hist_cap, stream);
}

PC_EXPORT int pc_lookup_slot_arm_prompt(const pc_lookup_slot_arm_block* host_block, int32_t nbytes, const pc_lookup_slot_state* state,
                                        int32_t* forced, int32_t n_forced, int32_t S, int32_t k, int32_t hist_cap, void* stream) {
    PC_REQUIRE(forced, PC_ERR_ARG, "pc_lookup_slot_arm_prompt: null pointer");
    return slot_arm("pc_lookup_slot_arm_prompt", host_block, nbytes, state, forced, n_forced, S, k, hist_cap, stream);
}
