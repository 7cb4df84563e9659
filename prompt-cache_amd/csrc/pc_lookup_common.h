// Shared by the slot launches (pc_slots.hip, pc_lookup.hip, pc_lookup_slots.hip).
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
