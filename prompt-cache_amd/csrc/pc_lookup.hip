// Prompt-lookup speculative decoding, the two ends of a device-side step (model/llama_hip.py LookupLoop):
//   pc_lookup_draft   first node: copy the tokens that followed the most recent earlier occurrence of the history's suffix
//   pc_lookup_verify  last node:  per-row argmax of the k+1-row forward, longest agreeing prefix + one bonus token, state advance
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

// One workgroup per slot: the rule above on the slot's own history and words.
__global__ __launch_bounds__(kDraftThreads) void lookup_draft_slots_kernel(const int32_t* __restrict__ hist,
                                                                            const int32_t* __restrict__ hist_len, int hist_cap,
                                                                            int64_t* ids, int32_t* pos, int32_t* ndraft,
                                                                            const int32_t* __restrict__ cap, const int32_t* __restrict__ len,
                                                                            const int32_t* __restrict__ live, int k, int nmax) {
    __shared__ int s_best[kDraftThreads / 64];
    __shared__ int s_key;
    const int b = blockIdx.x;
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
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

// One wave per slot: lookup_accept_kernel's rule on the slot's words, cut behind the first emitted stop id, with the slot's
// length where the B = 1 form has `past`.  A slot that did not run (idle, or no room for a step's rows) leaves an EMPTY record
// and nothing else -- its counter keeps pace with the replays, so that record c of every slot belongs to replay c -- and a
// live slot without room is switched off.
__global__ __launch_bounds__(64) void lookup_accept_slots_kernel(const int32_t* __restrict__ amax, int rows, int32_t* hist, int32_t* hist_len,
                                                                 int hist_cap, int64_t* ids, int32_t* pos, int32_t* len,
                                                                 const int32_t* __restrict__ cap, int32_t* live, const int32_t* ndraft,
                                                                 int32_t* budget, const int32_t* __restrict__ stop_ids, int32_t* ring,
                                                                 int32_t* ctr, int ring_cap) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int k = rows - 1;
    const int c = ctr[b];
    int32_t* rec = ring + ((int64_t)b * ring_cap + (int64_t)(((unsigned)c) % (unsigned)ring_cap)) * (rows + 1);
    if (!lookup_slot_runs(cap, len, live, b, k)) {
        if (lane == 0) {
            rec[0] = 0;
            ctr[b] = c + 1;
            if (live[b] != 0) live[b] = 0;
        }
        return;
    }
    hist += (int64_t)b * hist_cap;
    ids += (int64_t)b * rows;
    pos += (int64_t)b * rows;
    int nd = ndraft[b];
    nd = nd < 0 ? 0 : (nd > k ? k : nd);
    const int a = lane < rows ? amax[b * rows + lane] : 0;
    const bool miss = lane < nd && (int64_t)a != ids[1 + lane];
    const unsigned long long mm = __ballot(miss);
    const int acc = mm ? (int)__builtin_ctzll(mm) : nd;
    const int bud = budget[b];
    const int L = hist_len[b];
    const int p0 = pos[0], pl = len[b], cp = cap[b];
    int emit = acc + 1 < bud ? acc + 1 : bud;
    int room = L < 0 ? 0 : hist_cap - L;
    room = room < 0 ? 0 : room;
    emit = emit < room ? emit : room;
    emit = emit < 0 ? 0 : emit;
    bool stop = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) stop = stop || a == stop_ids[b * 8 + j];
    const unsigned long long sm = __ballot(stop && lane < emit);
    if (sm) emit = (int)__builtin_ctzll(sm) + 1;              // the stop id itself is emitted
    const int last = __shfl(a, emit > 0 ? emit - 1 : 0);
    if (lane == 0) rec[0] = emit;
    if (lane < emit) {
        rec[1 + lane] = a;
        hist[L + lane] = a;
    }
    if (lane == 0) {
        ctr[b] = c + 1;
        if (emit > 0) {
            hist_len[b] = L + emit;
            ids[0] = last;
            pos[0] = p0 + emit;
            len[b] = pl + emit;
            budget[b] = bud - emit;
        }
        if (sm != 0 || bud - emit <= 0 || pl + emit + k + 1 > cp) live[b] = 0;
    }
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

PC_EXPORT int pc_lookup_draft_slots(const int32_t* hist, const int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos,
                                    int32_t* ndraft, const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t k,
                                    int32_t nmax, void* stream) {
    PC_REQUIRE(hist && hist_len && ids && pos && ndraft && cap && len && live, PC_ERR_ARG, "pc_lookup_draft_slots: null pointer");
    PC_REQUIRE(S >= 1 && S <= 16 && k >= 1 && k < kMaxRows && S * (k + 1) <= kMaxSlotRows && nmax >= 1 && nmax <= kMaxNgram &&
                   hist_cap >= 1 && hist_cap < (1 << 24), PC_ERR_ARG,
               "pc_lookup_draft_slots: need 1 <= S <= 16, 1 <= k <= %d, S * (k + 1) <= %d, 1 <= nmax <= %d, 1 <= hist_cap < 2^24",
               kMaxRows - 1, kMaxSlotRows, kMaxNgram);
    hipLaunchKernelGGL(lookup_draft_slots_kernel, dim3(S), dim3(kDraftThreads), 0, (hipStream_t)stream, hist, hist_len, hist_cap, ids, pos,
                       ndraft, cap, len, live, k, nmax);
    return pc_check_launch("lookup_draft_slots_kernel");
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
