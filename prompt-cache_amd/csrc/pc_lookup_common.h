// Shared by the slot launches (pc_slots.hip, pc_lookup.hip, pc_lookup_slots.hip) and the two verify tails (pc_lookup.hip,
// pc_sample.hip).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

// A slot of the batched lookup step takes part when it is live and its arena has room for the k + 1 rows of a step
// (pc_slots.hip's "len >= cap" at k = 0).  Every launch of the step -- draft, rope + append, attention, merge, accept -- asks
// this one question, so a slot is either in all of them or in none.
__device__ __forceinline__ bool lookup_slot_runs(const int32_t* __restrict__ cap, const int32_t* __restrict__ len,
                                                 const int32_t* __restrict__ live, int b, int k) {
    const int past = len[b];
    return live[b] != 0 && past >= 0 && past + k + 1 <= cap[b];
}

// Shared rows of slot b (pc_attn_decode_slots_trunk, pc_attn_verify_slots_trunk): trunk[b] where the host contract holds for b --
// a leader g inside the S slots that leads itself, a trunk that fits the leader's arena and the slot's own length and is the
// leader's -- and 0 otherwise: the slot is then on its own.  The trunk launch, the own launch and the merge all ask here, so a
// violated contract gives the slot's plain attention over its own arena, never a read of records nobody wrote.
__device__ __forceinline__ int slot_trunk_rows(int b, int S, const uint64_t* __restrict__ kv_base, const int32_t* __restrict__ cap,
                                               const int32_t* __restrict__ len, const int32_t* __restrict__ leader,
                                               const int32_t* __restrict__ trunk) {
    const int g = leader[b];
    if (g < 0 || g >= S) return 0;
    const int T = trunk[g];
    return (leader[g] == g && T > 0 && T <= cap[g] && kv_base[g] != 0 && trunk[b] == T && T <= len[b]) ? T : 0;
}

// Shared rows of slot b over int8 IMAGES (pc_attn_decode_slots_trunk_q8): slot_trunk_rows with the leader's image in the place of
// its arena -- the trunk fits the images' qcap rows per plane and the leader has an image; neither the leader's arena nor its cap
// word is looked at, since no trunk key is read from an arena.  The trunk launch, the own launch and the merge of that entry all
// ask here and nowhere else.
__device__ __forceinline__ int slot_trunk_rows_q8(int b, int S, const uint64_t* __restrict__ kvq_base, int qcap,
                                                  const int32_t* __restrict__ len, const int32_t* __restrict__ leader,
                                                  const int32_t* __restrict__ trunk) {
    const int g = leader[b];
    if (g < 0 || g >= S) return 0;
    const int T = trunk[g];
    return (leader[g] == g && T > 0 && T <= qcap && kvq_base[g] != 0 && trunk[b] == T && T <= len[b]) ? T : 0;
}

// The accept rule of a prompt-lookup step (pc_lookup_verify, pc_lookup_verify_sample), by one wave.  Lane i holds a = the
// model's token for row i; the accepted count is the first draft row the model disagrees with (rows at / behind ndraft are
// pads: never accepted, whatever they hold).  Everything is read before anything is written; the ring record goes first.
// -> emit, the number of tokens the step yields (the same in every lane).
__device__ __forceinline__ int lookup_accept_rule(int a, int rows, int32_t* hist, int32_t* hist_len, int hist_cap, int64_t* ids,
                                                  int32_t* pos, int32_t* past, const int32_t* ndraft, int32_t* budget, int32_t* ring,
                                                  int32_t* ctr, int ring_cap) {
    const int lane = threadIdx.x;
    const int k = rows - 1;
    int nd = ndraft[0];
    nd = nd < 0 ? 0 : (nd > k ? k : nd);
    const bool miss = lane < nd && (int64_t)a != ids[1 + lane];
    const unsigned long long mm = __ballot(miss);
    const int acc = mm ? (int)__builtin_ctzll(mm) : nd;
    const int bud = budget[0];
    const int L = hist_len[0];
    const int c = ctr[0];
    const int p0 = pos[0], pl = past[0];
    int emit = acc + 1 < bud ? acc + 1 : bud;
    int room = L < 0 ? 0 : hist_cap - L;                  // (never binding on a history sized for the budget)
    room = room < 0 ? 0 : room;
    emit = emit < room ? emit : room;
    emit = emit < 0 ? 0 : emit;
    const int last = __shfl(a, emit > 0 ? emit - 1 : 0);
    int32_t* rec = ring + (int64_t)(((unsigned)c) % (unsigned)ring_cap) * (rows + 1);
    if (lane == 0) rec[0] = emit;
    if (lane < emit) {
        rec[1 + lane] = a;
        hist[L + lane] = a;
    }
    if (lane == 0) {
        ctr[0] = c + 1;
        if (emit > 0) {
            hist_len[0] = L + emit;
            ids[0] = last;
            pos[0] = p0 + emit;
            past[0] = pl + emit;
            budget[0] = bud - emit;
        }
    }
    return emit;
}

// The accept rule of a prompt-lookup step over SLOTS (pc_lookup_verify_slots, pc_lookup_verify_slots_each), by one wave for
// slot b: lookup_accept_rule on the slot's words, cut behind the first emitted stop id, with the slot's length where the B = 1
// form has `past`.  tok[i] = the model's token for draft row i of the slot (rows behind ndraft are pads: not read).  A slot that
// did not run (idle, or no room for a step's rows) leaves an EMPTY record and nothing else -- its counter keeps pace with the
// replays, so that record c of every slot belongs to replay c -- and a live slot without room is switched off.
// -> emit, the number of tokens the step yields (the same in every lane; -1: the slot did not run); a = this lane's token.
__device__ __forceinline__ int lookup_accept_slots_rule(const int32_t* __restrict__ tok, int rows, int b, int32_t* hist, int32_t* hist_len,
                                                        int hist_cap, int64_t* ids, int32_t* pos, int32_t* len,
                                                        const int32_t* __restrict__ cap, int32_t* live, const int32_t* ndraft,
                                                        int32_t* budget, const int32_t* __restrict__ stop_ids, int32_t* ring,
                                                        int32_t* ctr, int ring_cap, int& a) {
    const int lane = threadIdx.x;
    const int k = rows - 1;
    const int c = ctr[b];
    int32_t* rec = ring + ((int64_t)b * ring_cap + (int64_t)(((unsigned)c) % (unsigned)ring_cap)) * (rows + 1);
    a = 0;
    if (!lookup_slot_runs(cap, len, live, b, k)) {
        if (lane == 0) {
            rec[0] = 0;
            ctr[b] = c + 1;
            if (live[b] != 0) live[b] = 0;
        }
        return -1;
    }
    hist += (int64_t)b * hist_cap;
    ids += (int64_t)b * rows;
    pos += (int64_t)b * rows;
    int nd = ndraft[b];
    nd = nd < 0 ? 0 : (nd > k ? k : nd);
    a = lane <= nd ? tok[lane] : 0;
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
    return emit;
}

// ---- forced rows: a question fed through the draft rows of the step over slots (pc_lookup_*_slots_prompt) ----------------------
// forced[b] = R > 0: R prompt tokens are still to be fed behind ids[b][0].  They stand in hist[L .. L + R) (L = hist_len[b],
// hist[L - 1] = ids[b][0]); the host armed the slot so (pc_lookup_slot_arm_prompt) and L + R + budget <= hist_cap.  A null
// `forced` and forced[b] <= 0 are today's slot.
__device__ __forceinline__ int lookup_forced_rows(const int32_t* __restrict__ forced, int b) {
    const int R = forced ? forced[b] : 0;
    return R > 0 ? R : 0;
}

// (an index into the slot's history, kept inside the buffer whatever the words hold)
__device__ __forceinline__ int lookup_hist_at(int i, int hist_cap) { return i < 0 ? 0 : (i >= hist_cap ? hist_cap - 1 : i); }

// The draft of a RUNNING slot with R forced rows, by one workgroup: rows 1..m feed the next m = min(k, R) prompt tokens, pad rows
// and positions are lookup_draft_rule's, no n-gram search runs.
__device__ __forceinline__ void lookup_draft_forced_rule(const int32_t* __restrict__ hist, int L, int hist_cap, int64_t* ids, int32_t* pos,
                                                         int32_t* ndraft, int k, int R) {
    const int tid = threadIdx.x;
    const int m = R < k ? R : k;
    const int64_t id0 = ids[0];
    const int p0 = pos[0];
    if (tid < k) ids[1 + tid] = tid < m ? (int64_t)hist[lookup_hist_at(L + tid, hist_cap)] : id0;
    if (tid >= 1 && tid <= k) pos[tid] = p0 + tid;
    if (tid == 0) ndraft[0] = m;
}

// The accept rule of a RUNNING slot b with R forced rows, by one wave (pc_lookup_verify_slots_prompt).  R > k: the question goes
// on -- an EMPTY record, the k + 1 rows are kept, row 0 of the next step is the prompt token behind them.  R <= k: the question
// ends in row m = R, whose draw g (tok[m], the only row drawn) is the sequence's first token: from here on the words are what
// pc_lookup_slot_arm writes behind a prefill that drew g, the counter apart.  The stop-id, spent-budget and no-room rules apply
// to g as to any emitted token.
__device__ __forceinline__ void lookup_accept_forced_rule(const int32_t* __restrict__ tok, int rows, int V, int b, int R, int32_t* forced,
                                                          uint32_t* hist_bits, int32_t* draws, int32_t* hist, int32_t* hist_len,
                                                          int hist_cap, int64_t* ids, int32_t* pos, int32_t* len,
                                                          const int32_t* __restrict__ cap, int32_t* live, int32_t* budget,
                                                          const int32_t* __restrict__ stop_ids, int32_t* ring, int32_t* ctr,
                                                          int ring_cap) {
    if (threadIdx.x != 0) return;
    const int k = rows - 1;
    const int c = ctr[b];
    int32_t* rec = ring + ((int64_t)b * ring_cap + (int64_t)(((unsigned)c) % (unsigned)ring_cap)) * (rows + 1);
    hist += (int64_t)b * hist_cap;
    ids += (int64_t)b * rows;
    pos += (int64_t)b * rows;
    const int L = hist_len[b], p0 = pos[0], pl = len[b];
    ctr[b] = c + 1;
    if (R > k) {
        rec[0] = 0;
        hist_len[b] = L + k + 1;
        ids[0] = hist[lookup_hist_at(L + k, hist_cap)];
        pos[0] = p0 + k + 1;
        len[b] = pl + k + 1;
        forced[b] = R - k - 1;
        return;
    }
    const int m = R, g = tok[m], bud = budget[b];
    rec[0] = 1;
    rec[1] = g;
    if (L >= 0 && L + m < hist_cap) hist[L + m] = g;
    hist_len[b] = L + m + 1;
    ids[0] = g;
    pos[0] = p0 + m + 1;
    len[b] = pl + m + 1;
    forced[b] = 0;
    budget[b] = bud - 1;
    draws[b] = 1;
    if (g >= 0 && g < V) hist_bits[(int64_t)b * ((V + 31) >> 5) + (g >> 5)] |= 1u << (g & 31);
    bool stop = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) stop = stop || g == stop_ids[b * 8 + j];
    if (stop || bud - 1 <= 0 || pl + m + 1 + k + 1 > cap[b]) live[b] = 0;
}
