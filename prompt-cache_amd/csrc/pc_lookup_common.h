// Shared by the prompt-lookup slot launches (pc_lookup.hip, pc_lookup_slots.hip).
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
