// Sampled decode step tail, on the device: the sampled counterpart of greedy_advance_kernel (pc_misc.hip).
//
// Replaces  GenerationParameters.get_logits_processor()   promptcache/generation_engine.py:32-42
//           processors(...) + softmax + multinomial      promptcache/generation_engine.py:149-168
//
// One workgroup of 1024 threads turns one row of fp32 logits into the next token and advances the loop state the next
// replay of the captured decode graph reads.  The chain is the reference's, in its order: temperature (a true divide),
// repetition penalty over a history bitmap (CTRL rule), top-p (rank order: value descending, the higher index first among
// equal values -- what the stable ascending argsort implies; the top token is always kept), then top-k (ties at the kth
// value kept).  The draw is Gumbel-max over the kept tokens (an exact sample of softmax over the kept set) with a
// hand-written Philox4x32-10 stream keyed by the seed and counted by (token / 4, step); greedy mode is the argmax of the
// processed row, the lowest index among equal maxima.
//
// The top-p and top-k thresholds are radix selects over order-preserving uint32 keys: 4 passes of 8 bits, each with LDS
// histograms of counts and of exp(x - max) mass per bucket (after a max pass that only top-p needs); the row is re-read from L2 on every pass (a 65 024-token row
// does not fit in LDS).  Ties at the top-p boundary value are resolved in index order by a second, count-only select over
// the index bits (run only when the boundary value is shared and the mass cuts through it).
#include <math.h>

#include "pc_common.h"
#include "pc_lookup_common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ uint32_t order_key(float x) {
    if (x == 0.0f) x = 0.0f;                      // -0 and +0 compare equal: one key
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Philox4x32-10 (Salmon et al., SC'11): counter c, key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// -log(-log u) for u = ((w >> 8) + 0.5) * 2^-24 without cancellation on either side of 1/2.  Below 1/2, u is exact in fp32
// (an odd multiple of 2^-25 below 2^24 of them) and E = -log u >= log 2 takes the hardware log at its relative accuracy.  Above,
// v = 1 - u is the exact one and E = -log(1 - v) = 2 atanh(v / (2 - v)), a series in t^2 <= 1/9 (8 terms: < 3e-9 relative), so
// the smallest E -- the winners of the race -- keep their relative precision.  The last log needs absolute accuracy only.
__device__ __forceinline__ float gumbel(uint32_t w) {
    const uint32_t a = w >> 8;
    float e;
    if (a < (1u << 23)) {
        e = -__logf((float)(2u * a + 1u) * 0x1p-25f);
    } else {
        const float v = (float)((1u << 25) - 2u * a - 1u) * 0x1p-25f;
        const float t = v / (2.0f - v), t2 = t * t;
        float s = 1.0f / 15.0f;
        s = fmaf(s, t2, 1.0f / 13.0f);
        s = fmaf(s, t2, 1.0f / 11.0f);
        s = fmaf(s, t2, 1.0f / 9.0f);
        s = fmaf(s, t2, 1.0f / 7.0f);
        s = fmaf(s, t2, 1.0f / 5.0f);
        s = fmaf(s, t2, 1.0f / 3.0f);
        s = fmaf(s, t2, 1.0f);
        e = 2.0f * t * s;
    }
    return -__logf(e);
}

struct Row {
    const float* __restrict__ logits;
    const uint32_t* __restrict__ hist;
    int V;
    bool al16, tdiv, pen;
    float T, rp;

    // processed values of tokens 4g .. 4g+3 (tokens past V: -inf); NaN counts as -inf
    __device__ __forceinline__ void load(int g, float x[4]) const {
        const int i = 4 * g;
        if (al16 && i + 3 < V) {
            const f4 t = *(const f4*)(logits + i);
            x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = (i + e < V) ? logits[i + e] : -INFINITY;
        }
        const uint32_t bits = pen ? hist[i >> 5] >> (i & 31) : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = x[e];
            if (v != v) v = -INFINITY;
            if (tdiv) v = v / T;
            if ((bits >> e) & 1u) v = v < 0.0f ? v * rp : v / rp;
            x[e] = (i + e < V) ? v : -INFINITY;
        }
    }
};

// Wave-level descending select over a 256-bucket histogram: the largest digit d with base + sum_{d' >= d} w[d'] >= target,
// and above = base + sum_{d' > d} w[d'].  None (a mass target past the rounded total): the smallest non-empty digit.
template <typename W>
__device__ __forceinline__ void select_desc(const W* w, const uint32_t* cnt, W base, W target, int lane, int& dsel, W& above) {
    W v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = w[255 - 4 * lane - j]; s += v[j]; }
    W incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const W t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    W run = __shfl_up(incl, 1);
    if (lane == 0) run = 0;
    run += base;
    int found = -1;
    W ab = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (found < 0 && run + v[j] >= target) { found = j; ab = run; }
        run += v[j];
    }
    const unsigned long long hit = __ballot(found >= 0);
    if (hit) {
        const int src = __ffsll((long long)hit) - 1;
        dsel = __shfl(255 - 4 * lane - found, src);
        above = __shfl(ab, src);
        return;
    }
    // fallback: the lowest non-empty digit, everything above it
    int lo = 256;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (cnt[255 - 4 * lane - j] != 0) lo = 255 - 4 * lane - j;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o));
    if (lo == 256) lo = 0;
    dsel = lo;
    const W total = __shfl(incl, 63);
    above = base + total - w[lo];
}

// f(g, x) for every group g of 4 tokens of this thread, the loads of 4 groups in flight at a time (each pass is a re-read of
// the row from L2: latency, not bandwidth, is what one workgroup pays for it)
template <typename F>
__device__ __forceinline__ void for_each_group(const Row& row, int G, F&& f) {
    int g = threadIdx.x;
    for (; g + 3 * kThreads < G; g += 4 * kThreads) {
        float x[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) row.load(g + u * kThreads, x[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) f(g + u * kThreads, x[u]);
    }
    for (; g < G; g += kThreads) {
        float x[4];
        row.load(g, x);
        f(g, x);
    }
}

// Radix histograms live in LDS as kCols lane-private columns per digit (column = lane & 31: the 32 lanes of a half-wave hit 32
// distinct banks, so an update never serialises on one address however the digits cluster -- logits crowd into a few exponent
// buckets); a reduction over the columns feeds the selects.
constexpr int kCols = 32;

__device__ __forceinline__ void reduce_columns(const uint32_t* __restrict__ c, uint32_t* out, int b) {
    uint32_t s = 0;
#pragma unroll 8
    for (int j = 0; j < kCols; ++j) s += c[b * kCols + ((j + b) & (kCols - 1))];
    out[b] = s;
}

__device__ __forceinline__ void reduce_columns(const float* __restrict__ c, float* out, int b) {
    float s = 0.0f;
#pragma unroll 8
    for (int j = 0; j < kCols; ++j) s += c[b * kCols + ((j + b) & (kCols - 1))];
    out[b] = s;
}

// The chain and the draw for ONE row, by one workgroup of kThreads threads: the token, valid in thread 0 (every thread of the
// workgroup must call it).  `hist` is read only.
__device__ __forceinline__ int sample_row(const float* __restrict__ logits, int V, const pc_sample_params* __restrict__ prm,
                                          const uint32_t* hist, uint64_t seed, uint32_t step, float* processed_out) {
    __shared__ uint32_t cp[256 * kCols];  // top-p select: counts per digit and column
    __shared__ float mp[256 * kCols];     //               exp(x - max) mass per digit and column
    __shared__ uint32_t ck[256 * kCols];  // top-k select, then the boundary-tie index select: counts per digit and column
    __shared__ uint32_t rcp[256], rck[256];
    __shared__ float rmp[256];
    __shared__ float s_red[kWaves];
    __shared__ int s_idx[kWaves];
    __shared__ float s_max, s_base_p, s_target_p;
    __shared__ uint32_t s_pref_p, s_pref_k, s_base_k, s_pref_i, s_keep_ties;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = tid & (kCols - 1);
    const float T = prm->temperature, rp = prm->repetition_penalty, top_p = prm->top_p;
    const int top_k = prm->top_k;
    const bool greedy = T < 1e-5f || top_p < 1e-8f;
    const Row row{logits, hist, V, ((uintptr_t)logits & 15) == 0, T >= 1e-5f && T != 1.0f, rp > 1.0f, T, rp};
    const int G = (V + 3) >> 2;
    const bool want_p = top_p >= 1e-8f && top_p < 1.0f;
    const bool want_k = top_k > 0 && top_k < V;

    // ---- pass 0 (top-p only): the row maximum --------------------------------------------------------------------------
    float m = 0.0f;
    if (want_p || want_k) {
        for (int i = tid; i < 256 * kCols; i += kThreads) {
            if (want_p) { cp[i] = 0u; mp[i] = 0.0f; }
            if (want_k) ck[i] = 0u;
        }
        if (tid == 0) { s_pref_p = 0u; s_pref_k = 0u; s_base_p = 0.0f; s_base_k = 0u; s_pref_i = 0u; s_keep_ties = 0x7fffffffu; }
        if (want_p) {
            m = -INFINITY;
            for_each_group(row, G, [&](int, const float* x) {
#pragma unroll
                for (int e = 0; e < 4; ++e) m = fmaxf(m, x[e]);
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if (lane == 0) s_red[wave] = m;
        }
        __syncthreads();
        if (want_p && tid == 0) {
            float mm = s_red[0];
            for (int w = 1; w < kWaves; ++w) mm = fmaxf(mm, s_red[w]);
            s_max = mm;
        }
        __syncthreads();
        if (want_p) m = s_max;
    }

    // filters only on a finite row (an all -inf row draws token 0 below, as greedy_advance_kernel does)
    const bool topp_on = want_p && m > -INFINITY && m < INFINITY;
    const bool topk_on = want_k;
    uint32_t b_key = 0u, k_key = 0u;       // keep: key > b_key (or == b_key at index >= tie_index); key >= k_key
    int tie_index = 0;

    if (topp_on || topk_on) {
        // ---- passes 1..4: radix selects, 8 bits at a time from the top ----------------------------------------------
        for (int p = 0; p < 4; ++p) {
            const int shift = 24 - 8 * p;
            const uint32_t hi = p == 0 ? 0u : (0xffffffffu << (shift + 8));
            const uint32_t pp = s_pref_p & hi, pk = s_pref_k & hi;
            for_each_group(row, G, [&](int g, const float* x) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (4 * g + e >= V) break;
                    const uint32_t k = order_key(x[e]);
                    const int a = (int)((k >> shift) & 255u) * kCols + col;
                    if (topp_on && (k & hi) == pp) {
                        atomicAdd(&cp[a], 1u);
                        atomicAdd(&mp[a], __expf(x[e] - m));
                    }
                    if (topk_on && (k & hi) == pk) atomicAdd(&ck[a], 1u);
                }
            });
            __syncthreads();
            if (tid < 256) {
                if (topp_on) { reduce_columns(cp, rcp, tid); reduce_columns(mp, rmp, tid); }
            } else if (tid < 512) {
                if (topk_on) reduce_columns(ck, rck, tid - 256);
            }
            __syncthreads();
            if (wave == 0 && topp_on) {
                float target = s_target_p;
                if (p == 0) {            // the softmax denominator is the first pass's total mass
                    float z = 0.0f;
                    for (int j = lane; j < 256; j += 64) z += rmp[j];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
                    target = top_p * z;
                }
                int d;
                float above;
                select_desc<float>(rmp, rcp, s_base_p, target, lane, d, above);
                if (lane == 0) {
                    s_pref_p |= (uint32_t)d << shift;
                    s_base_p = above;
                    s_target_p = target;
                    if (p == 3) {
                        // the boundary value's tie group: its n highest indices are kept, n = #{j : above + j p_b < target}
                        const uint32_t cnt = rcp[d];
                        const float pb = __expf(key_value(s_pref_p) - m);
                        uint32_t n = cnt;
                        if (pb > 0.0f) {
                            const float q = ceilf((target - above) / pb);
                            n = q < 1.0f ? 1u : (q < (float)cnt ? (uint32_t)q : cnt);
                        }
                        s_keep_ties = n < cnt ? n : 0x7fffffffu;
                    }
                }
            } else if (wave == 1 && topk_on) {
                int d;
                uint32_t above;
                select_desc<uint32_t>(rck, rck, s_base_k, (uint32_t)top_k, lane, d, above);
                if (lane == 0) { s_pref_k |= (uint32_t)d << shift; s_base_k = above; }
            } else if (wave >= 2) {
                for (int i = tid - 128; i < 256 * kCols; i += kThreads - 128) {
                    if (topp_on) { cp[i] = 0u; mp[i] = 0.0f; }
                    if (topk_on) ck[i] = 0u;
                }
            }
            __syncthreads();
        }
        b_key = topp_on ? s_pref_p : 0u;
        k_key = topk_on ? s_pref_k : 0u;

        // ---- the top-p boundary value is shared and the mass cuts through it: the kept ties are its highest indices -----
        const uint32_t keep_ties = s_keep_ties;
        if (topp_on && keep_ties != 0x7fffffffu) {
            if (!topk_on)
                for (int i = tid; i < 256 * kCols; i += kThreads) ck[i] = 0u;
            if (tid == 0) s_base_k = 0u;
            __syncthreads();
            for (int p = 0; p < 3; ++p) {
                const int shift = 16 - 8 * p;
                const uint32_t hi = p == 0 ? 0xff000000u : (0xffffffffu << (shift + 8));
                const uint32_t pi = s_pref_i & hi;
                for_each_group(row, G, [&](int g, const float* x) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t i = (uint32_t)(4 * g + e);
                        if ((int)i < V && order_key(x[e]) == b_key && (i & hi) == pi)
                            atomicAdd(&ck[((i >> shift) & 255u) * kCols + col], 1u);
                    }
                });
                __syncthreads();
                if (tid < 256) reduce_columns(ck, rck, tid);
                __syncthreads();
                if (wave == 0) {
                    int d;
                    uint32_t above;
                    select_desc<uint32_t>(rck, rck, s_base_k, keep_ties, lane, d, above);
                    if (lane == 0) { s_pref_i |= (uint32_t)d << shift; s_base_k = above; }
                } else if (wave >= 2) {
                    for (int i = tid - 128; i < 256 * kCols; i += kThreads - 128) ck[i] = 0u;
                }
                __syncthreads();
            }
            tie_index = (int)s_pref_i;
        }
    }

    // ---- final pass: filter, processed row, draw --------------------------------------------------------------------------
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for_each_group(row, G, [&](int g, const float* x) {
        bool keep[4];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t k = order_key(x[e]);
            bool kp = true;
            if (topp_on) kp = k > b_key || (k == b_key && 4 * g + e >= tie_index);
            if (topk_on) kp = kp && k >= k_key;
            keep[e] = kp && x[e] > -INFINITY;
            any |= keep[e];
        }
        if (processed_out) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * g + e < V) processed_out[4 * g + e] = keep[e] ? x[e] : -INFINITY;
        }
        if (!any) return;
        uint32_t c[4] = {(uint32_t)g, step, 0u, 0u};
        if (!greedy) philox4x32_10(c, k0, k1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!keep[e]) continue;
            const float sc = greedy ? x[e] : x[e] + gumbel(c[e]);
            if (sc > best) { best = sc; bi = 4 * g + e; }
        }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { s_red[wave] = best; s_idx[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kWaves; ++w)
            if (s_red[w] > best || (s_red[w] == best && s_idx[w] < bi)) { best = s_red[w]; bi = s_idx[w]; }
        if (bi == 0x7fffffff) bi = 0;                 // all -inf / NaN: token 0, as greedy_advance_kernel
    }
    return bi;
}

__global__ __launch_bounds__(kThreads) void sample_advance_kernel(const float* __restrict__ logits, int V,
                                                                  const pc_sample_params* __restrict__ prm, uint32_t* hist,
                                                                  int64_t* ids, int32_t* pos, int32_t* past, int32_t* ring,
                                                                  int32_t* ctr, int ring_cap, float* processed_out) {
    const uint32_t step = (uint32_t)ctr[0];
    const int bi = sample_row(logits, V, prm, hist, prm->seed, step, processed_out);
    if (threadIdx.x == 0) {
        ids[0] = bi;
        pos[0] += 1;
        past[0] += 1;
        ring[step % (uint32_t)ring_cap] = bi;
        ctr[0] = (int32_t)(step + 1u);
        hist[bi >> 5] |= 1u << (bi & 31);
    }
}

// One workgroup per slot (pc_sample_advance_slots): the row, random stream, history bitmap and state words of slot b.  An idle
// slot changes nothing; a live slot whose arena is full (len >= cap: nothing was appended for it) only goes idle.
__global__ __launch_bounds__(kThreads) void sample_advance_slots_kernel(
    const float* __restrict__ logits, int64_t ldl, int V, const pc_sample_params* __restrict__ prm,
    const uint64_t* __restrict__ seeds, uint32_t* hist, int64_t* ids, int32_t* pos, int32_t* len, const int32_t* __restrict__ cap,
    int32_t* live, int32_t* budget, const int32_t* __restrict__ stop_ids, int32_t* ring, int32_t* ctr, int ring_cap,
    float* processed_out) {
    const int b = blockIdx.x;
    if (live[b] == 0) return;                          // (uniform over the workgroup)
    if (len[b] < 0 || len[b] >= cap[b]) {
        if (threadIdx.x == 0) live[b] = 0;
        return;
    }
    const int hw = (V + 31) >> 5;
    uint32_t* hb = hist + (int64_t)b * hw;
    const uint32_t step = (uint32_t)ctr[b];
    const int bi = sample_row(logits + (int64_t)b * ldl, V, prm, hb, seeds[b], step, processed_out ? processed_out + (int64_t)b * V : nullptr);
    if (threadIdx.x == 0) {
        ids[b] = bi;
        pos[b] += 1;
        const int n = len[b] + 1;
        len[b] = n;
        ring[(int64_t)b * ring_cap + step % (uint32_t)ring_cap] = bi;
        ctr[b] = (int32_t)(step + 1u);
        hb[bi >> 5] |= 1u << (bi & 31);
        const int left = budget[b] - 1;
        budget[b] = left;
        bool stop = left <= 0 || n + 1 >= cap[b];
#pragma unroll
        for (int j = 0; j < 8; ++j) stop |= stop_ids[j] == bi;
        if (stop) live[b] = 0;
    }
}

// pc_sample_advance_slots_each: sample_advance_slots_kernel with the sampling state per slot -- parameter block b, stop row b and
// the Philox step draws[b] of slot b's own random stream; ctr[b] only places the token in the ring.  A sequence admitted into a
// running loop keeps the stream it would have had alone while its ring rows line up with the other slots'.
__global__ __launch_bounds__(kThreads) void sample_advance_slots_each_kernel(
    const float* __restrict__ logits, int64_t ldl, int V, const pc_sample_params* __restrict__ prm,
    const uint64_t* __restrict__ seeds, uint32_t* hist, int64_t* ids, int32_t* pos, int32_t* len, const int32_t* __restrict__ cap,
    int32_t* live, int32_t* budget, const int32_t* __restrict__ stop_ids, int32_t* ring, int32_t* ctr, int32_t* draws, int ring_cap,
    float* processed_out) {
    const int b = blockIdx.x;
    if (live[b] == 0) return;                          // (uniform over the workgroup)
    if (len[b] < 0 || len[b] >= cap[b]) {
        if (threadIdx.x == 0) live[b] = 0;
        return;
    }
    const int hw = (V + 31) >> 5;
    uint32_t* hb = hist + (int64_t)b * hw;
    const uint32_t step = (uint32_t)draws[b];
    const int bi = sample_row(logits + (int64_t)b * ldl, V, prm + b, hb, seeds[b], step, processed_out ? processed_out + (int64_t)b * V : nullptr);
    if (threadIdx.x == 0) {
        ids[b] = bi;
        pos[b] += 1;
        const int n = len[b] + 1;
        len[b] = n;
        const uint32_t c = (uint32_t)ctr[b];
        ring[(int64_t)b * ring_cap + c % (uint32_t)ring_cap] = bi;
        ctr[b] = (int32_t)(c + 1u);
        draws[b] = (int32_t)(step + 1u);
        hb[bi >> 5] |= 1u << (bi & 31);
        const int left = budget[b] - 1;
        budget[b] = left;
        bool stop = left <= 0 || n + 1 >= cap[b];
#pragma unroll
        for (int j = 0; j < 8; ++j) stop |= stop_ids[b * 8 + j] == bi;
        if (stop) live[b] = 0;
    }
}

// pc_lookup_verify_sample, first launch: one workgroup per row of the k + 1-row verify forward.  Row i <= ndraft is drawn as the
// one-token loop would draw it had drafts 1..i been emitted: Philox step draws + i, and a history of its own -- row_bits[i] =
// history_bits with the bits of ids[1..i] set, built here -- so that sample_row and the shared bitmap stay read-only.  Pad rows
// (i > ndraft) leave at once (uniform over the workgroup).
__global__ __launch_bounds__(kThreads) void lookup_sample_rows_kernel(const float* __restrict__ logits, int64_t ldl, int V, int rows,
                                                                      const pc_sample_params* __restrict__ prm,
                                                                      const uint32_t* __restrict__ hist, uint32_t* row_bits,
                                                                      const int32_t* __restrict__ draws, const int64_t* __restrict__ ids,
                                                                      const int32_t* __restrict__ ndraft, int32_t* row_token,
                                                                      float* processed_out) {
    const int i = blockIdx.x;
    int nd = ndraft[0];
    nd = nd < 0 ? 0 : (nd > rows - 1 ? rows - 1 : nd);
    if (i > nd) return;
    const int hw = (V + 31) >> 5;
    uint32_t* rb = row_bits + (int64_t)i * hw;
    for (int w = threadIdx.x; w < hw; w += kThreads) rb[w] = hist[w];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j <= i; ++j) {
            const int64_t t = ids[j];
            if (t >= 0 && t < V) rb[t >> 5] |= 1u << (t & 31);
        }
    }
    __syncthreads();
    const uint32_t step = (uint32_t)draws[0] + (uint32_t)i;
    const int bi = sample_row(logits + (int64_t)i * ldl, V, prm, rb, prm->seed, step, processed_out ? processed_out + (int64_t)i * V : nullptr);
    if (threadIdx.x == 0) row_token[i] = bi;
}

// ... second launch, one wave: lookup_accept_rule on the rows' draws, then the sampled loop's own words -- the emitted tokens'
// bits into the shared bitmap and the random stream advanced by what was emitted (the draws of rejected rows are not consumed:
// the next replay draws step draws + emit again, for the token that then stands there).
__global__ __launch_bounds__(64) void lookup_sample_accept_kernel(const int32_t* __restrict__ row_token, int rows, int V, uint32_t* hist_bits,
                                                                  int32_t* draws, int32_t* hist, int32_t* hist_len, int hist_cap,
                                                                  int64_t* ids, int32_t* pos, int32_t* past, const int32_t* ndraft,
                                                                  int32_t* budget, int32_t* ring, int32_t* ctr, int ring_cap) {
    const int lane = threadIdx.x;
    int nd = ndraft[0];
    nd = nd < 0 ? 0 : (nd > rows - 1 ? rows - 1 : nd);
    const int a = lane <= nd ? row_token[lane] : 0;        // (pad rows were not drawn)
    const int d = draws[0];
    const int emit = lookup_accept_rule(a, rows, hist, hist_len, hist_cap, ids, pos, past, ndraft, budget, ring, ctr, ring_cap);
    for (int j = 0; j < emit; ++j) {
        const int t = __shfl(a, j);
        if (lane == 0 && t >= 0 && t < V) hist_bits[t >> 5] |= 1u << (t & 31);
    }
    if (lane == 0 && emit > 0) draws[0] = d + emit;
}

// pc_lookup_verify_slots_each, first launch: lookup_sample_rows_kernel per slot -- one workgroup per row r = b * (k + 1) + i of
// the S * (k + 1)-row verify forward, with parameter block b, seed b, draws[b] and bitmap row b.  A greedy block takes the argmax
// of its processed row, so greedy and sampled requests share the step.  Rows of a slot that does not run and pad rows
// (i > ndraft[b]) leave at once (uniform over the workgroup).  `forced` (null: pc_lookup_verify_slots_each): of a slot with
// R = forced[b] > 0 rows only the row that ends its question is drawn -- row R where R <= k, none otherwise -- as the first token
// of a sequence is: under the bitmap as armed (the rows in front of it are prompt tokens) at step draws[b].
__global__ __launch_bounds__(kThreads) void lookup_sample_rows_slots_kernel(
    const float* __restrict__ logits, int64_t ldl, int V, int k, const pc_sample_params* __restrict__ prm,
    const uint64_t* __restrict__ seeds, const uint32_t* __restrict__ hist, uint32_t* row_bits, const int32_t* __restrict__ draws,
    const int64_t* __restrict__ ids, const int32_t* __restrict__ ndraft, const int32_t* __restrict__ cap,
    const int32_t* __restrict__ len, const int32_t* __restrict__ live, int32_t* row_token, const int32_t* __restrict__ forced) {
    const int r = blockIdx.x, b = r / (k + 1), i = r - b * (k + 1);
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
    const int R = lookup_forced_rows(forced, b);
    int nd = ndraft[b];
    nd = nd < 0 ? 0 : (nd > k ? k : nd);
    if (R ? i != R : i > nd) return;                   // (R > k: no row has index R)
    const int hw = (V + 31) >> 5;
    const uint32_t* hb = hist + (int64_t)b * hw;
    uint32_t* rb = row_bits + (int64_t)r * hw;
    for (int w = threadIdx.x; w < hw; w += kThreads) rb[w] = hb[w];
    __syncthreads();
    if (threadIdx.x == 0 && !R) {
        for (int j = 1; j <= i; ++j) {
            const int64_t t = ids[(int64_t)b * (k + 1) + j];
            if (t >= 0 && t < V) rb[t >> 5] |= 1u << (t & 31);
        }
    }
    __syncthreads();
    const uint32_t step = (uint32_t)draws[b] + (R ? 0u : (uint32_t)i);
    const int bi = sample_row(logits + (int64_t)r * ldl, V, prm + b, rb, seeds[b], step, nullptr);
    if (threadIdx.x == 0) row_token[r] = bi;
}

// ... second launch, one wave per slot: lookup_accept_slots_rule on the rows' draws, then the sampled loop's own words of the
// slot -- the emitted tokens' bits into bitmap row b and the slot's random stream advanced by what was emitted, counted behind
// the stop cut (the draws of rejected rows are not consumed).  `forced` (null: pc_lookup_verify_slots_each): a running slot with
// forced rows takes lookup_accept_forced_rule instead (uniform over the wave).
__global__ __launch_bounds__(64) void lookup_accept_slots_each_kernel(const int32_t* __restrict__ row_token, int rows, int V,
                                                                      uint32_t* hist_bits, int32_t* draws, int32_t* hist, int32_t* hist_len,
                                                                      int hist_cap, int64_t* ids, int32_t* pos, int32_t* len,
                                                                      const int32_t* __restrict__ cap, int32_t* live, const int32_t* ndraft,
                                                                      int32_t* budget, const int32_t* __restrict__ stop_ids, int32_t* ring,
                                                                      int32_t* ctr, int ring_cap, int32_t* forced) {
    const int lane = threadIdx.x, b = blockIdx.x;
    if (const int R = lookup_forced_rows(forced, b)) {
        if (lookup_slot_runs(cap, len, live, b, rows - 1)) {
            lookup_accept_forced_rule(row_token + b * rows, rows, V, b, R, forced, hist_bits, draws, hist, hist_len, hist_cap, ids, pos, len,
                                      cap, live, budget, stop_ids, ring, ctr, ring_cap);
            return;
        }
    }
    const int d = draws[b];
    int a;
    const int emit = lookup_accept_slots_rule(row_token + b * rows, rows, b, hist, hist_len, hist_cap, ids, pos, len, cap, live, ndraft,
                                              budget, stop_ids, ring, ctr, ring_cap, a);
    uint32_t* hb = hist_bits + (int64_t)b * ((V + 31) >> 5);
    for (int j = 0; j < emit; ++j) {
        const int t = __shfl(a, j);
        if (lane == 0 && t >= 0 && t < V) hb[t >> 5] |= 1u << (t & 31);
    }
    if (lane == 0 && emit > 0) draws[b] = d + emit;
}

}  // namespace

PC_EXPORT int pc_sample_advance(const float* logits, int32_t vocab, const pc_sample_params* params_dev, uint32_t* history_bits,
                                int64_t* ids, int32_t* pos, int32_t* past_len, int32_t* ring, int32_t* counter, int32_t ring_cap,
                                float* processed_out, void* stream) {
    PC_REQUIRE(logits && params_dev && history_bits && ids && pos && past_len && ring && counter && ring_cap > 0, PC_ERR_ARG,
               "pc_sample_advance: null pointer or bad sizes");
    PC_REQUIRE(vocab > 0 && vocab < (1 << 24), PC_ERR_ARG, "pc_sample_advance: vocab must be in [1, 2^24)");
    PC_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)params_dev & 7) == 0, PC_ERR_ARG,
               "pc_sample_advance: logits must be 4-byte and params 8-byte aligned");
    hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, logits, vocab, params_dev,
                       history_bits, ids, pos, past_len, ring, counter, ring_cap, processed_out);
    return pc_check_launch("sample_advance_kernel");
}

PC_EXPORT int pc_sample_advance_slots(const float* logits, int64_t logits_row_stride, int32_t vocab,
                                      const pc_sample_params* params_dev, const uint64_t* seeds, uint32_t* history_bits,
                                      int64_t* ids, int32_t* pos, int32_t* len, const int32_t* cap, int32_t* live, int32_t* budget,
                                      const int32_t* stop_ids, int32_t* ring, int32_t* counters, int32_t ring_cap, int32_t S,
                                      float* processed_out, void* stream) {
    PC_REQUIRE(logits && params_dev && seeds && history_bits && ids && pos && len && cap && live && budget && stop_ids && ring &&
                   counters && ring_cap > 0, PC_ERR_ARG, "pc_sample_advance_slots: null pointer or bad sizes");
    PC_REQUIRE(S >= 1 && S <= 16, PC_ERR_ARG, "pc_sample_advance_slots: 1 <= S <= 16");
    PC_REQUIRE(vocab > 0 && vocab < (1 << 24) && logits_row_stride >= vocab, PC_ERR_ARG,
               "pc_sample_advance_slots: vocab must be in [1, 2^24) and the row stride at least vocab");
    PC_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)params_dev & 7) == 0 && ((uintptr_t)seeds & 7) == 0, PC_ERR_ARG,
               "pc_sample_advance_slots: logits must be 4-byte, params and seeds 8-byte aligned");
    hipLaunchKernelGGL(sample_advance_slots_kernel, dim3(S), dim3(kThreads), 0, (hipStream_t)stream, logits, logits_row_stride,
                       vocab, params_dev, seeds, history_bits, ids, pos, len, cap, live, budget, stop_ids, ring, counters, ring_cap,
                       processed_out);
    return pc_check_launch("sample_advance_slots_kernel");
}

PC_EXPORT int pc_sample_advance_slots_each(const float* logits, int64_t logits_row_stride, int32_t vocab,
                                           const pc_sample_params* params_dev, const uint64_t* seeds, uint32_t* history_bits,
                                           int64_t* ids, int32_t* pos, int32_t* len, const int32_t* cap, int32_t* live,
                                           int32_t* budget, const int32_t* stop_ids, int32_t* ring, int32_t* counters,
                                           int32_t* draws, int32_t ring_cap, int32_t S, float* processed_out, void* stream) {
    PC_REQUIRE(logits && params_dev && seeds && history_bits && ids && pos && len && cap && live && budget && stop_ids && ring &&
                   counters && draws && ring_cap > 0, PC_ERR_ARG, "pc_sample_advance_slots_each: null pointer or bad sizes");
    PC_REQUIRE(S >= 1 && S <= 16, PC_ERR_ARG, "pc_sample_advance_slots_each: 1 <= S <= 16");
    PC_REQUIRE(vocab > 0 && vocab < (1 << 24) && logits_row_stride >= vocab, PC_ERR_ARG,
               "pc_sample_advance_slots_each: vocab must be in [1, 2^24) and the row stride at least vocab");
    PC_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)params_dev & 7) == 0 && ((uintptr_t)seeds & 7) == 0, PC_ERR_ARG,
               "pc_sample_advance_slots_each: logits must be 4-byte, params and seeds 8-byte aligned");
    hipLaunchKernelGGL(sample_advance_slots_each_kernel, dim3(S), dim3(kThreads), 0, (hipStream_t)stream, logits, logits_row_stride,
                       vocab, params_dev, seeds, history_bits, ids, pos, len, cap, live, budget, stop_ids, ring, counters, draws,
                       ring_cap, processed_out);
    return pc_check_launch("sample_advance_slots_each_kernel");
}

PC_EXPORT int pc_lookup_verify_sample(const float* logits, int64_t ldl, int32_t vocab, int32_t rows, const pc_sample_params* params_dev,
                                      uint32_t* history_bits, uint32_t* row_bits, int32_t* draws, int32_t* row_token, int32_t* hist,
                                      int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* past_len,
                                      const int32_t* ndraft, int32_t* budget, int32_t* ring, int32_t* counter, int32_t ring_cap,
                                      float* processed_out, void* stream) {
    PC_REQUIRE(logits && params_dev && history_bits && row_bits && draws && row_token && hist && hist_len && ids && pos && past_len &&
                   ndraft && budget && ring && counter, PC_ERR_ARG, "pc_lookup_verify_sample: null pointer");
    PC_REQUIRE(rows >= 1 && rows <= 16 && ldl >= vocab && ring_cap > 0 && hist_cap >= 1, PC_ERR_ARG,
               "pc_lookup_verify_sample: need 1 <= rows <= 16, ldl >= vocab, ring_cap > 0, hist_cap >= 1");
    PC_REQUIRE(vocab > 0 && vocab < (1 << 24), PC_ERR_ARG, "pc_lookup_verify_sample: vocab must be in [1, 2^24)");
    PC_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)params_dev & 7) == 0, PC_ERR_ARG,
               "pc_lookup_verify_sample: logits must be 4-byte and params 8-byte aligned");
    hipLaunchKernelGGL(lookup_sample_rows_kernel, dim3(rows), dim3(kThreads), 0, (hipStream_t)stream, logits, ldl, vocab, rows,
                       params_dev, history_bits, row_bits, draws, ids, ndraft, row_token, processed_out);
    int rc = pc_check_launch("lookup_sample_rows_kernel");
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(lookup_sample_accept_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, row_token, rows, vocab, history_bits,
                       draws, hist, hist_len, hist_cap, ids, pos, past_len, ndraft, budget, ring, counter, ring_cap);
    return pc_check_launch("lookup_sample_accept_kernel");
}

namespace {

// pc_lookup_verify_slots_each (forced null) and pc_lookup_verify_slots_prompt
int verify_slots_each(const char* name, const float* logits, int64_t ldl, int32_t vocab, int32_t S, int32_t k,
                      const pc_sample_params* params_dev, const uint64_t* seeds, uint32_t* history_bits, uint32_t* row_bits,
                      int32_t* draws, int32_t* row_token, int32_t* hist, int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos,
                      int32_t* len, const int32_t* cap, int32_t* live, const int32_t* ndraft, int32_t* budget, const int32_t* stop_ids,
                      int32_t* ring, int32_t* counters, int32_t* forced, int32_t ring_cap, void* stream) {
    PC_REQUIRE(logits && params_dev && seeds && history_bits && row_bits && draws && row_token && hist && hist_len && ids && pos && len &&
                   cap && live && ndraft && budget && stop_ids && ring && counters, PC_ERR_ARG, "%s: null pointer", name);
    PC_REQUIRE(S >= 1 && S <= 16 && k >= 1 && k <= 15 && S * (k + 1) <= 64 && ldl >= vocab && ring_cap > 0 && hist_cap >= 1, PC_ERR_ARG,
               "%s: need 1 <= S <= 16, 1 <= k <= 15, S * (k + 1) <= 64, ldl >= vocab, ring_cap > 0, hist_cap >= 1", name);
    PC_REQUIRE(vocab > 0 && vocab < (1 << 24), PC_ERR_ARG, "%s: vocab must be in [1, 2^24)", name);
    PC_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)params_dev & 7) == 0 && ((uintptr_t)seeds & 7) == 0, PC_ERR_ARG,
               "%s: logits must be 4-byte, params and seeds 8-byte aligned", name);
    hipLaunchKernelGGL(lookup_sample_rows_slots_kernel, dim3(S * (k + 1)), dim3(kThreads), 0, (hipStream_t)stream, logits, ldl, vocab, k,
                       params_dev, seeds, history_bits, row_bits, draws, ids, ndraft, cap, len, live, row_token, forced);
    int rc = pc_check_launch("lookup_sample_rows_slots_kernel");
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(lookup_accept_slots_each_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, row_token, k + 1, vocab, history_bits,
                       draws, hist, hist_len, hist_cap, ids, pos, len, cap, live, ndraft, budget, stop_ids, ring, counters, ring_cap, forced);
    return pc_check_launch("lookup_accept_slots_each_kernel");
}

}  // namespace

PC_EXPORT int pc_lookup_verify_slots_each(const float* logits, int64_t ldl, int32_t vocab, int32_t S, int32_t k,
                                          const pc_sample_params* params_dev, const uint64_t* seeds, uint32_t* history_bits,
                                          uint32_t* row_bits, int32_t* draws, int32_t* row_token, int32_t* hist, int32_t* hist_len,
                                          int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* len, const int32_t* cap, int32_t* live,
                                          const int32_t* ndraft, int32_t* budget, const int32_t* stop_ids, int32_t* ring,
                                          int32_t* counters, int32_t ring_cap, void* stream) {
    return verify_slots_each("pc_lookup_verify_slots_each", logits, ldl, vocab, S, k, params_dev, seeds, history_bits, row_bits, draws,
                             row_token, hist, hist_len, hist_cap, ids, pos, len, cap, live, ndraft, budget, stop_ids, ring, counters,
                             nullptr, ring_cap, stream);
}

PC_EXPORT int pc_lookup_verify_slots_prompt(const float* logits, int64_t ldl, int32_t vocab, int32_t S, int32_t k,
                                            const pc_sample_params* params_dev, const uint64_t* seeds, uint32_t* history_bits,
                                            uint32_t* row_bits, int32_t* draws, int32_t* row_token, int32_t* hist, int32_t* hist_len,
                                            int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* len, const int32_t* cap,
                                            int32_t* live, const int32_t* ndraft, int32_t* budget, const int32_t* stop_ids,
                                            int32_t* ring, int32_t* counters, int32_t* forced, int32_t ring_cap, void* stream) {
    PC_REQUIRE(forced, PC_ERR_ARG, "pc_lookup_verify_slots_prompt: null pointer");
    return verify_slots_each("pc_lookup_verify_slots_prompt", logits, ldl, vocab, S, k, params_dev, seeds, history_bits, row_bits, draws,
                             row_token, hist, hist_len, hist_cap, ids, pos, len, cap, live, ndraft, budget, stop_ids, ring, counters,
                             forced, ring_cap, stream);
}
