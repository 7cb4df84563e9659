// Batched decode over SLOTS: several running sequences, each in a batch-1 KV arena of its own, advanced by one captured step.
//
// Replaces, for S sequences at once, what the B = 1 decode step does per layer between the q|k|v projection and o_proj:
//           apply_rotary_pos_emb + torch.cat([past, new])        promptcache/model/llama2.py:202-210, :361-364
//           softmax(q k^T / sqrt(d)) v over the sequence's keys  promptcache/model/llama2.py:366-400
//
// A slot is described by device words -- arena base address, capacity, length, live flag -- so that one captured graph serves
// every step: the advance launch (pc_sample_advance_slots, pc_sample.hip) rewrites them.  Nothing a slot computes depends on
// another slot: every workgroup works for exactly one slot, the split of the key axis is a function of that slot's own length
// and of the host-fixed split count, and every reduction runs in a fixed order.  A slot's output is therefore bit-identical
// whatever the other slots hold and whichever index it sits at.
//
// The attention is the memory-bound one-row case: K / V rows go from global memory straight to registers (16 bytes per lane,
// D / 8 lanes per key), scores and P.V are fp32 VALU work on q = hi + lo (at least the precision of the split-precision MFMA
// form of attn_small_kernel), and the query heads of one kv head share every K / V load (GQ heads per workgroup pass).
//
// The step shares the kernels of the k + 1 row step (pc_lookup_slots.hip) at k = 0 -- RoPE + append, the shared-trunk attention
// and the merges -- through the launchers of pc_attn_rows.h; the one-row attention below is this unit's own.
#include <hip/hip_fp16.h>
#include <math.h>

#include "pc_attn_rows.h"

namespace {

using pca::kNegBig;
using pca::kThreads;
using pcr::h8;
using pcr::SlotAttnArgs;

// ---- one-row attention per slot, split over the key axis ---------------------------------------------------------------
// grid (split, kv head x pass, slot).  A pass takes GQ query heads of the kv head's group; D / 8 lanes hold one key row, a wave
// 64 / (D / 8) keys at a time, four keys per lane group in flight.  Every lane group keeps an online softmax of its own
// keys; the groups of a wave are merged through lane exchanges, the four waves through LDS, always in the same order.
// Shared rows of a slot (pc_attn_decode_slots_trunk): slot_trunk_rows, pc_lookup_common.h.
// TRUNK (pc_attn_decode_slots_trunk): a slot with shared rows (slot_trunk_rows) takes keys [trunk[b], len[b]] only -- the keys in front of them
// are the trunk launch's -- and its partials are records rec0 .. rec0 + nsplit - 1 of the nrec records per (slot, head).  With
// none the arithmetic is the plain instantiation's.
template <int D, int GQ, bool TRUNK = false>
__global__ __launch_bounds__(kThreads) void attn_decode_slots_kernel(
    const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo, int64_t q_ts, const uint64_t* __restrict__ kv_base,
    const int32_t* __restrict__ cap, const int32_t* __restrict__ len, const int32_t* __restrict__ live, int layer, int H, int Hkv,
    float scale_log2, int nsplit, float* __restrict__ part_o, float* __restrict__ part_ml,
    const int32_t* __restrict__ leader = nullptr, const int32_t* __restrict__ trunk = nullptr, int nrec = 0, int rec0 = 0,
    int S = 0) {
    constexpr int LPK = D / 8;          // lanes per key row
    constexpr int GPW = 64 / LPK;       // key groups per wave
    constexpr int NG = 4 * GPW;         // key groups per workgroup
    constexpr int U = 4;                // keys in flight per group
    __shared__ float sm[4][GQ][D + 2];

    const int split = blockIdx.x, b = blockIdx.z;
    if (live[b] == 0) return;
    const int past = len[b], c = cap[b];
    if (past < 0 || past >= c) return;
    const int G = H / Hkv, passes = (G + GQ - 1) / GQ;
    const int kvh = blockIdx.y / passes, g0 = (blockIdx.y - kvh * passes) * GQ;
    const int n = past + 1;                       // keys of this slot: its staged and decoded rows and the row just appended
    int t0 = 0;                                   // first key of this launch
    if constexpr (TRUNK) t0 = slot_trunk_rows(b, S, kv_base, cap, len, leader, trunk);
    const int chunk = (max(n - t0, 0) + nsplit - 1) / nsplit;
    const int k0 = t0 + split * chunk, k1 = min(n, k0 + chunk);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % LPK, grp = wave * GPW + lane / LPK;
    const _Float16* kp = (const _Float16*)(uintptr_t)kv_base[b] + ((int64_t)(layer * 2) * Hkv + kvh) * c * D + sub * 8;
    const _Float16* vp = kp + (int64_t)Hkv * c * D;

    float q[GQ][8], acc[GQ][8], m[GQ], l[GQ];
#pragma unroll
    for (int g = 0; g < GQ; ++g) {
        const int h = kvh * G + min(g0 + g, G - 1);
        const int64_t qo = (int64_t)b * q_ts + (int64_t)h * D + sub * 8;
        const h8 a = *(const h8*)(q_hi + qo), r = *(const h8*)(q_lo + qo);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            q[g][e] = ((float)a[e] + (float)r[e]) * scale_log2;
            acc[g][e] = 0.0f;
        }
        m[g] = kNegBig;
        l[g] = 0.0f;
    }

    for (int base = k0; base < k1; base += NG * U) {
        h8 kk[U], vv[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int key = base + u * NG + grp;
            ok[u] = key < k1;
            const int64_t off = (int64_t)min(key, k1 - 1) * D;
            kk[u] = *(const h8*)(kp + off);
            vv[u] = *(const h8*)(vp + off);
        }
#pragma unroll
        for (int g = 0; g < GQ; ++g) {
            float s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float d = 0.0f;
#pragma unroll
                for (int e = 0; e < 8; ++e) d = fmaf(q[g][e], (float)kk[u][e], d);
#pragma unroll
                for (int o = 1; o < LPK; o <<= 1) d += __shfl_xor(d, o);
                s[u] = ok[u] ? d : -INFINITY;
            }
            float mn = m[g];
#pragma unroll
            for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u]);
            const float sc = exp2f(m[g] - mn);
            float ll = l[g] * sc;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[g][e] *= sc;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float p = exp2f(s[u] - mn);
                ll += p;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[g][e] = fmaf(p, (float)vv[u][e], acc[g][e]);
            }
            m[g] = mn;
            l[g] = ll;
        }
    }

    // the key groups of a wave -> its first group
#pragma unroll
    for (int g = 0; g < GQ; ++g) {
#pragma unroll
        for (int o = LPK; o < 64; o <<= 1) {
            const float mo = __shfl_xor(m[g], o), lo = __shfl_xor(l[g], o);
            const float mn = fmaxf(m[g], mo);
            const float wa = exp2f(m[g] - mn), wb = exp2f(mo - mn);
            l[g] = l[g] * wa + lo * wb;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[g][e] = acc[g][e] * wa + __shfl_xor(acc[g][e], o) * wb;
            m[g] = mn;
        }
        if (lane < LPK) {
#pragma unroll
            for (int e = 0; e < 8; ++e) sm[wave][g][sub * 8 + e] = acc[g][e];
            if (sub == 0) { sm[wave][g][D] = m[g]; sm[wave][g][D + 1] = l[g]; }
        }
    }
    __syncthreads();
    // the four waves -> this split's partial (unnormalised sum, maximum, denominator)
    for (int i = tid; i < GQ * D; i += kThreads) {
        const int g = i / D, d = i - g * D;
        if (g0 + g >= G) break;
        float ms = sm[0][g][D];
#pragma unroll
        for (int w = 1; w < 4; ++w) ms = fmaxf(ms, sm[w][g][D]);
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float wt = exp2f(sm[w][g][D] - ms);
            den = fmaf(wt, sm[w][g][D + 1], den);
            num = fmaf(wt, sm[w][g][d], num);
        }
        const int64_t slot = TRUNK ? ((int64_t)b * H + kvh * G + g0 + g) * nrec + rec0 + split
                                   : ((int64_t)b * H + kvh * G + g0 + g) * nsplit + split;
        part_o[slot * D + d] = num;
        if (d == 0) { part_ml[slot * 2] = ms; part_ml[slot * 2 + 1] = den; }
    }
}

// own launch: keys [slot_trunk_rows, len] of every slot as records ns_trunk .. of its heads (TRUNK), or all keys (plain)
template <int D, int GQ, bool TRUNK>
void launch_own(const SlotAttnArgs& a, hipStream_t st) {
    const int passes = (a.H / a.Hkv + GQ - 1) / GQ;
    hipLaunchKernelGGL((attn_decode_slots_kernel<D, GQ, TRUNK>), dim3(a.ns_own, a.Hkv * passes, a.S), dim3(kThreads), 0, st, a.q_hi,
                       a.q_lo, a.q_ts, a.kv_base, a.cap, a.len, a.live, a.layer, a.H, a.Hkv, a.scale_log2, a.ns_own, a.part_o, a.part_ml,
                       a.leader, a.trunk, a.ns_trunk + a.ns_own, a.ns_trunk, a.S);
}

template <int D, bool TRUNK>
void launch_own_d(const SlotAttnArgs& a, hipStream_t st) {
    const int G = a.H / a.Hkv;
    if (G == 1) launch_own<D, 1, TRUNK>(a, st);
    else if (G <= 4) launch_own<D, 4, TRUNK>(a, st);
    else launch_own<D, 8, TRUNK>(a, st);
}

// ---- pc_slot_arm: every state word of ONE slot from a pinned host block, one launch ---------------------------------------
// Admission into a running loop: the launch sits on the stream between two replays of the captured step, so the replays before
// it saw the slot's old words (idle) and the replays behind it see the new sequence.  The block is host memory the host rewrites
// between admissions: system-scope loads (pc_fetch_block's rule), never a device cache.  One workgroup: the header goes through
// LDS, the history bitmap row (ceil(V / 32) words, 1 000 at V = 32 000) is copied by all threads, live[slot] = 1 is the last store.
constexpr int kArmWords = (int)(sizeof(pc_slot_arm_block) / 8);

__global__ __launch_bounds__(kThreads) void slot_arm_kernel(const unsigned long long* __restrict__ src, pc_slot_state st, int S, int hw) {
    typedef __attribute__((address_space(1))) unsigned long long g64;
    __shared__ __attribute__((aligned(8))) unsigned long long h[kArmWords];
    const int tid = threadIdx.x;
    if (tid < kArmWords) h[tid] = __hip_atomic_load((g64*)(src + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    const pc_slot_arm_block& b = *(const pc_slot_arm_block*)h;
    const int s = b.slot;
    if (s < 0 || s >= S || b.hist_words != hw) return;          // (the block changed under the launch: touch nothing)
    uint32_t* row = st.history_bits + (int64_t)s * hw;
    for (int i = tid; 2 * i < hw; i += kThreads) {
        const unsigned long long w = __hip_atomic_load((g64*)(src + kArmWords + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        row[2 * i] = (uint32_t)w;
        if (2 * i + 1 < hw) row[2 * i + 1] = (uint32_t)(w >> 32);
    }
    if (tid == 0) {
        st.kv_base[s] = b.kv_base;
        st.cap[s] = b.cap;
        st.len[s] = b.len;
        st.pos[s] = b.pos;
        st.ids[s] = b.id;
        st.leader[s] = b.leader;
        st.trunk[s] = b.trunk;
        st.budget[s] = b.budget;
        st.counters[s] = b.counter;
        st.draws[s] = b.draws;
        st.seeds[s] = b.seed;
        st.params[s] = b.params;
    } else if (tid >= 64 && tid < 72) {
        st.stop_ids[s * 8 + tid - 64] = b.stop_ids[tid - 64];
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) st.live[s] = 1;
}

}  // namespace

PC_EXPORT int pc_rope_append_slots(const float* qkv, int64_t ld, int32_t in_layout, void* q_hi, void* q_lo, int64_t q_token_stride,
                                   const float* cs, const uint64_t* kv_base, const int32_t* cap, const int32_t* len,
                                   const int32_t* live, int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D, void* stream) {
    PC_REQUIRE(S >= 1 && S <= 16 && layer >= 0 && H > 0 && Hkv > 0, PC_ERR_ARG, "pc_rope_append_slots: bad sizes (1 <= S <= 16)");
    PC_REQUIRE(D > 0 && D % 16 == 0, PC_ERR_ARG, "pc_rope_append_slots: head_dim must be a multiple of 16");
    PC_REQUIRE(qkv && q_hi && q_lo && cs && kv_base && cap && len && live, PC_ERR_ARG, "pc_rope_append_slots: null pointer");
    PC_REQUIRE(in_layout == 0 || in_layout == 1, PC_ERR_ARG, "pc_rope_append_slots: in_layout is 0 (natural) or 1 (rotary-pair tiles)");
    PC_REQUIRE(ld >= (int64_t)(H + 2 * Hkv) * D && ld % 4 == 0 && q_token_stride % 8 == 0 && ((uintptr_t)qkv & 15) == 0 &&
                   ((uintptr_t)q_hi & 15) == 0 && ((uintptr_t)q_lo & 15) == 0,
               PC_ERR_ARG, "pc_rope_append_slots: rows must keep 16-byte alignment");
    pcr::launch_rope_append_slots_rows(qkv, ld, in_layout, (_Float16*)q_hi, (_Float16*)q_lo, q_token_stride, (const float2*)cs, kv_base,
                                       cap, len, live, S, 0, layer, H, Hkv, D, (hipStream_t)stream);
    return pc_check_launch("rope_append_slots_rows_kernel");
}

PC_EXPORT int64_t pc_attn_decode_slots_workspace_bytes(int32_t S, int32_t H, int32_t D, int32_t nsplit) {
    if (S < 1 || H < 1 || D < 1 || nsplit < 1) return 0;
    return (int64_t)S * H * nsplit * (D + 2) * (int64_t)sizeof(float);
}

PC_EXPORT int pc_attn_decode_slots(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                   const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t layer, int32_t H,
                                   int32_t Hkv, int32_t D, float softmax_scale, int32_t nsplit, void* workspace,
                                   int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, void* stream) {
    SlotAttnArgs a = {(const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len, live, nullptr, nullptr,
                      S, 0, layer, H, Hkv, 0.f, nsplit, 0, nullptr, nullptr, (_Float16*)out_frag_hi, (_Float16*)out_frag_lo};
    if (const int rc = pcr::slot_attn_prepare("pc_attn_decode_slots", false, false, 8, a, D, softmax_scale, workspace, workspace_bytes))
        return rc;
    if (D == 128) launch_own_d<128, false>(a, (hipStream_t)stream);
    else launch_own_d<64, false>(a, (hipStream_t)stream);
    pcr::launch_attn_merge_slots(a, D, false, (hipStream_t)stream);
    return pc_check_launch("attn_decode_slots_kernel");
}

PC_EXPORT int64_t pc_attn_decode_slots_trunk_workspace_bytes(int32_t S, int32_t H, int32_t D, int32_t nsplit_own,
                                                             int32_t nsplit_trunk) {
    if (S < 1 || H < 1 || D < 1 || nsplit_own < 1 || nsplit_trunk < 1) return 0;
    return (int64_t)S * H * (nsplit_own + nsplit_trunk) * (D + 2) * (int64_t)sizeof(float);
}

PC_EXPORT int pc_attn_decode_slots_trunk(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                         const int32_t* cap, const int32_t* len, const int32_t* live, const int32_t* leader,
                                         const int32_t* trunk, int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                                         float softmax_scale, int32_t nsplit_own, int32_t nsplit_trunk, void* workspace,
                                         int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, void* stream) {
    SlotAttnArgs a = {(const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len, live, leader, trunk,
                      S, 0, layer, H, Hkv, 0.f, nsplit_own, nsplit_trunk, nullptr, nullptr, (_Float16*)out_frag_hi, (_Float16*)out_frag_lo};
    if (const int rc = pcr::slot_attn_prepare("pc_attn_decode_slots_trunk", false, true, 16, a, D, softmax_scale, workspace, workspace_bytes))
        return rc;
    // trunk launch (two tiles per pass unless a kv head has one query head), own launch, merge
    hipStream_t st = (hipStream_t)stream;
    pcr::launch_attn_trunk_slots(a, D, H == Hkv ? 1 : 2, st);
    if (D == 128) launch_own_d<128, true>(a, st);
    else launch_own_d<64, true>(a, st);
    pcr::launch_attn_merge_slots(a, D, true, st);
    return pc_check_launch("attn_verify_trunk_slots_kernel");
}

PC_EXPORT int pc_slot_arm(const pc_slot_arm_block* host_block, int32_t nbytes, const pc_slot_state* state, int32_t S, void* stream) {
    PC_REQUIRE(host_block && state, PC_ERR_ARG, "pc_slot_arm: null pointer");
    PC_REQUIRE(state->kv_base && state->cap && state->len && state->pos && state->ids && state->live && state->leader && state->trunk &&
                   state->budget && state->counters && state->draws && state->seeds && state->params && state->stop_ids &&
                   state->history_bits, PC_ERR_ARG, "pc_slot_arm: null pointer in the slot state");
    PC_REQUIRE(S >= 1 && S <= 16, PC_ERR_ARG, "pc_slot_arm: 1 <= S <= 16");
    PC_REQUIRE(((uintptr_t)host_block & 7) == 0 && ((uintptr_t)state->params & 7) == 0 && ((uintptr_t)state->seeds & 7) == 0 &&
                   ((uintptr_t)state->kv_base & 7) == 0 && ((uintptr_t)state->ids & 7) == 0, PC_ERR_ARG,
               "pc_slot_arm: the block and the 64-bit state arrays must be 8-byte aligned");
    const int32_t slot = host_block->slot, hw = host_block->hist_words;       // (pinned HOST memory: readable here)
    PC_REQUIRE(slot >= 0 && slot < S, PC_ERR_ARG, "pc_slot_arm: slot outside [0, S)");
    PC_REQUIRE(hw >= 1 && hw <= (1 << 19) && (int64_t)nbytes == (int64_t)sizeof(pc_slot_arm_block) + (((int64_t)hw * 4 + 7) & ~(int64_t)7),
               PC_ERR_ARG, "pc_slot_arm: nbytes must be sizeof(pc_slot_arm_block) + 4 * hist_words rounded up to 8");
    hipLaunchKernelGGL(slot_arm_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned long long*)host_block, *state, S,
                       hw);
    return pc_check_launch("slot_arm_kernel");
}
