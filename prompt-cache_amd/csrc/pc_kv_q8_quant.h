// The pinned quantisation of one K / V row of the int8 KV format (pc_kv_q8.hip has the format and the arithmetic in words), once
// for the units that produce image rows: the segment quantiser (pc_kv_q8.hip) and the slot attention that stages the row it has
// just been given (pc_slots_q8.hip).  tests/kv_q8_ref.py restates it in numpy, bit for bit.
#pragma once
#include "pc_common.h"

namespace pcq {

// A row's D / 16 = 1 << lg lanes are consecutive lanes of one wave and ALL call, each with its 16 values; every lane of the wave
// executes the cross-lane swaps.  -> this lane's 16 codes (four dwords, byte b of dword q = value 4q + b) and the row's scale
// (the same in all of the row's lanes).  Every step in fp32, round to nearest even, nothing contracted.
__device__ __forceinline__ void quant_row16(const float (&x)[16], int lg, uint32_t (&w)[4], float& scale) {
    float s = 0.0f;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float ax = __builtin_fabsf(x[i]);
        bad |= !(ax <= 65504.0f);                           // NaN or infinity (every finite fp16 is <= 65504)
        s = (ax > s) ? ax : s;
    }
    for (int m = 1; m < (1 << lg); m <<= 1) {
        const float o = __shfl_xor(s, m);
        const int ob = __shfl_xor((int)bad, m);
        s = (o > s) ? o : s;
        bad |= ob != 0;
    }
    const float inv = (s > 0.0f && !bad) ? __fdiv_rn(127.0f, s) : 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t acc = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float t = bad ? 0.0f : __builtin_rintf(__fmul_rn(x[q * 4 + b], inv));
            acc |= ((uint32_t)(int)t & 0xffu) << (8 * b);
        }
        w[q] = acc;
    }
    scale = bad ? __builtin_nanf("") : __fdiv_rn(s, 127.0f);
}

}  // namespace pcq
