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
#include <hip/hip_fp16.h>
#include <math.h>

#include "pc_attn_common.h"
#include "pc_lookup_common.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr float kNegBig = -1.0e30f;   // finite "-inf" of the running maxima
constexpr int kThreads = 256;
constexpr int kMaxSplit = 32;

// position of element (row m, feature k) in a fragment-major plane with KS k-steps (pc_gemm.hip)
__device__ __forceinline__ int64_t frag_off(int m, int k, int KS) {
    return ((((int64_t)(m >> 4) * KS + (k >> 5)) * 64) + ((k & 31) >> 3) * 16 + (m & 15)) * 8 + (k & 7);
}

__device__ __forceinline__ void load8(const float* p, float (&x)[8]) {
    const f4 a = *(const f4*)p, b = *(const f4*)(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[e] = a[e]; x[e + 4] = b[e]; }
}

// ---- RoPE + append, one workgroup per slot -----------------------------------------------------------------------------
// The work items and the arithmetic are rope_append_kernel<float>'s (pc_rope.hip): the rows written are bit-identical to what
// pc_rope_append_ex writes for the same projection row and position.  layout 1: the projection row is in the row order of the
// q|k|v fragment image (_native.qkv_rope_row_perm: inside a head, 16-column tile j = features 8j.. then D/2 + 8j..).
__global__ __launch_bounds__(kThreads) void rope_append_slots_kernel(
    const float* __restrict__ qkv, int64_t ld, int layout, _Float16* __restrict__ q_hi, _Float16* __restrict__ q_lo, int64_t q_ts,
    const float2* __restrict__ cs, const uint64_t* __restrict__ kv_base, const int32_t* __restrict__ cap,
    const int32_t* __restrict__ len, const int32_t* __restrict__ live, int layer, int H, int Hkv, int D) {
    const int b = blockIdx.x;
    if (live[b] == 0) return;
    const int past = len[b], c = cap[b];
    if (past < 0 || past >= c) return;
    const int half = D >> 1;
    const int cph = D >> 4;  // 8-pair chunks per head
    const int nq = H * cph, nk = Hkv * cph, nv = Hkv * (D >> 3);
    const float2* csr = cs + (int64_t)b * half;
    const float* row = qkv + (int64_t)b * ld;
    _Float16* k_plane = (_Float16*)(uintptr_t)kv_base[b] + (int64_t)(layer * 2) * Hkv * c * D;
    _Float16* v_plane = k_plane + (int64_t)Hkv * c * D;
    for (int it = threadIdx.x; it < nq + nk + nv; it += blockDim.x) {
        if (it < nq + nk) {
            const bool is_q = it < nq;
            const int j = is_q ? it : it - nq;
            const int h = j / cph, ch = j - h * cph;
            const float* src = row + (int64_t)(is_q ? h : H + h) * D;
            _Float16* dst = is_q ? q_hi + (int64_t)b * q_ts + (int64_t)h * D : k_plane + ((int64_t)h * c + past) * D;
            float lo[8], hi[8];
            load8(src + (layout ? ch * 16 : ch * 8), lo);
            load8(src + (layout ? ch * 16 + 8 : half + ch * 8), hi);
            h8 olo, ohi, rlo, rhi;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float2 w = csr[ch * 8 + e];
                const float a = lo[e] * w.x - hi[e] * w.y, b2 = hi[e] * w.x + lo[e] * w.y;
                _Float16 t0, t1, t2, t3;
                pc_split(a, t0, t1);
                pc_split(b2, t2, t3);
                olo[e] = t0; rlo[e] = t1;
                ohi[e] = t2; rhi[e] = t3;
            }
            *(h8*)(dst + ch * 8) = olo;
            *(h8*)(dst + half + ch * 8) = ohi;
            if (is_q) {
                _Float16* dl = q_lo + (int64_t)b * q_ts + (int64_t)h * D;
                *(h8*)(dl + ch * 8) = rlo;
                *(h8*)(dl + half + ch * 8) = rhi;
            }
        } else {
            const int j = it - nq - nk;
            const int cpv = D >> 3;
            const int h = j / cpv, ch = j - h * cpv;
            float x[8];
            load8(row + (int64_t)(H + Hkv + h) * D + (layout ? (ch < cph ? ch * 16 : (ch - cph) * 16 + 8) : ch * 8), x);
            h8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)x[e];
            *(h8*)(v_plane + ((int64_t)h * c + past) * D + ch * 8) = o;
        }
    }
}

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

// merge of the split partials, one workgroup per (head, slot), one thread per head dim, splits in index order
template <int D>
__global__ __launch_bounds__(D) void attn_merge_slots_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                             const int32_t* __restrict__ cap, const int32_t* __restrict__ len,
                                                             const int32_t* __restrict__ live, int H, int nsplit,
                                                             _Float16* __restrict__ of_hi, _Float16* __restrict__ of_lo) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    if (live[b] == 0) return;
    const int past = len[b];
    if (past < 0 || past >= cap[b]) return;
    const int64_t base = ((int64_t)b * H + h) * nsplit;
    float ms = kNegBig;
    for (int s = 0; s < nsplit; ++s) ms = fmaxf(ms, part_ml[(base + s) * 2]);
    float num = 0.0f, den = 0.0f;
    for (int s = 0; s < nsplit; ++s) {
        const float wt = exp2f(part_ml[(base + s) * 2] - ms);
        den = fmaf(wt, part_ml[(base + s) * 2 + 1], den);
        num = fmaf(wt, part_o[(base + s) * D + d], num);
    }
    _Float16 hi, lo;
    pc_split(num / den, hi, lo);
    const int64_t off = frag_off(b, h * D + d, H * D / 32);
    of_hi[off] = hi;
    of_lo[off] = lo;
}

template <int D, int GQ>
void launch_decode(int S, int H, int Hkv, int nsplit, hipStream_t st, const _Float16* q_hi, const _Float16* q_lo, int64_t q_ts,
                   const uint64_t* kv_base, const int32_t* cap, const int32_t* len, const int32_t* live, int layer,
                   float scale_log2, float* part_o, float* part_ml) {
    const int passes = (H / Hkv + GQ - 1) / GQ;
    hipLaunchKernelGGL((attn_decode_slots_kernel<D, GQ>), dim3(nsplit, Hkv * passes, S), dim3(kThreads), 0, st, q_hi, q_lo, q_ts,
                       kv_base, cap, len, live, layer, H, Hkv, scale_log2, nsplit, part_o, part_ml);
}

template <int D>
void launch_decode_d(int S, int H, int Hkv, int nsplit, hipStream_t st, const _Float16* q_hi, const _Float16* q_lo, int64_t q_ts,
                     const uint64_t* kv_base, const int32_t* cap, const int32_t* len, const int32_t* live, int layer,
                     float scale_log2, float* part_o, float* part_ml) {
    const int G = H / Hkv;
    if (G == 1)
        launch_decode<D, 1>(S, H, Hkv, nsplit, st, q_hi, q_lo, q_ts, kv_base, cap, len, live, layer, scale_log2, part_o, part_ml);
    else if (G <= 4)
        launch_decode<D, 4>(S, H, Hkv, nsplit, st, q_hi, q_lo, q_ts, kv_base, cap, len, live, layer, scale_log2, part_o, part_ml);
    else
        launch_decode<D, 8>(S, H, Hkv, nsplit, st, q_hi, q_lo, q_ts, kv_base, cap, len, live, layer, scale_log2, part_o, part_ml);
}

// ---- shared trunk: the keys a group of slots has in common, read once for all of them ----------------------------------
// Slots that staged the same leading module rows (leader[b] = g, trunk[b] = T) hold the same bytes in rows [0, T) of their
// arenas.  This launch reads those rows from the leader's arena only and multiplies them with the query rows of ALL members:
// row = (member, query head of the kv head), 16 rows per MFMA tile, RT tiles per workgroup pass.  The formulation is
// attn_small_kernel's (pc_attn.hip): S^T = K . Q^T and O^T += V^T . P^T on mfma_f32_16x16x32_f16, Q and P as hi / lo pairs, fp32
// online softmax; every WAVE owns a contiguous slice of the split's keys, K fragments go from global memory into the A operand,
// V through a wave-private LDS tile and back transposed, no barrier until the four waves' partials are merged.
// grid (trunk split, kv head x pass, candidate leader).  A column of an MFMA tile depends on that column's B operand only, the
// key slices are a function of (T, nsplit_t) and every reduction runs in a fixed order: what a row gets does not depend on how
// many members the group has, on the row's place in the tile or on the slot index.  Pad rows are zero and are never written.
template <int D, int RT>
__global__ __launch_bounds__(kThreads, RT > 1 ? 1 : 2) void attn_trunk_slots_kernel(
    const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo, int64_t q_ts, const uint64_t* __restrict__ kv_base,
    const int32_t* __restrict__ cap, const int32_t* __restrict__ len, const int32_t* __restrict__ live,
    const int32_t* __restrict__ leader, const int32_t* __restrict__ trunk, int S, int layer, int H, int Hkv, float scale_log2,
    int nsplit_t, int nrec, float* __restrict__ part_o, float* __restrict__ part_ml) {
    using pca::kTK;
    constexpr int KS = D / 32, DB = D / 16, CPR = D / 8;
    constexpr int LPW = kTK * CPR / 64;              // 16-byte V chunks per lane per tile
    constexpr int kTileHalfs = kTK * D;
    constexpr int kMergeBytes = RT * (4 * DB * 64 * 4 + 4 * 16 * 2) * 4;
    constexpr int kLdsBytes = 4 * kTileHalfs * 2 > kMergeBytes ? 4 * kTileHalfs * 2 : kMergeBytes;
    __shared__ __attribute__((aligned(16))) char smem[kLdsBytes];

    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x, gl = blockIdx.z;
    const int G = H / Hkv, passes = (G + RT - 1) / RT;
    const int kvh = blockIdx.y / passes, row0 = (blockIdx.y - kvh * passes) * 16 * RT;
    const int T = trunk[gl], cg = cap[gl];
    if (leader[gl] != gl || T <= 0 || T > cg || kv_base[gl] == 0) return;     // (no slot_trunk_rows of this group is non-zero)

    // the member list, in slot order (S state words, workgroup-uniform), and this lane's row of each tile
    int mi[RT], gh[RT], sb[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int r = row0 + rt * 16 + n;
        mi[rt] = r / G;
        gh[rt] = r - mi[rt] * G;
        sb[rt] = -1;
    }
    int nmem = 0;
    for (int b = 0; b < S; ++b) {
        const int past = len[b];
        if (leader[b] != gl || live[b] == 0 || past < 0 || past >= cap[b]) continue;
        if (slot_trunk_rows(b, S, kv_base, cap, len, leader, trunk) == 0) continue;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
            if (mi[rt] == nmem) sb[rt] = b;
        ++nmem;
    }
    if (row0 >= nmem * G) return;                    // workgroup-uniform: no member, or no row left for this pass

    int cpw = (T + nsplit_t * 4 - 1) / (nsplit_t * 4);             // keys per wave
    cpw = (cpw + 15) & ~15;
    const int k0 = (split * 4 + wave) * cpw;
    const int k1 = (k0 + cpw < T) ? k0 + cpw : T;

    h8 qf[RT][KS], qfl[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int b = sb[rt] < 0 ? 0 : sb[rt];
        const int64_t off = (int64_t)b * q_ts + (int64_t)(kvh * G + gh[rt]) * D + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            const h8 a = *(const h8*)(q_hi + off + ks * 32), r = *(const h8*)(q_lo + off + ks * 32);
            qf[rt][ks] = sb[rt] < 0 ? z : a;
            qfl[rt][ks] = sb[rt] < 0 ? z : r;
        }
    }
    f4 o[RT][DB];
    float m_run[RT], l_run[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int db = 0; db < DB; ++db) { f4 z = {0.f, 0.f, 0.f, 0.f}; o[rt][db] = z; }
        m_run[rt] = kNegBig; l_run[rt] = 0.f;
    }
    const _Float16* kbase = (const _Float16*)(uintptr_t)kv_base[gl] + ((int64_t)(layer * 2) * Hkv + kvh) * cg * D;
    const _Float16* vbase = kbase + (int64_t)Hkv * cg * D;
    _Float16* Vw = (_Float16*)smem + wave * kTileHalfs;            // this wave's V tile
    char* Vwb = smem + wave * kTileHalfs * 2;

    for (int key0 = k0; key0 < k1; key0 += kTK) {
        // every load of the tile first, all unconditional (keys past k1 re-read the last valid row and are masked below)
        pca::u32x4 kr[4][KS];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int key = key0 + kb * 16 + n < k1 ? key0 + kb * 16 + n : k1 - 1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kr[kb][ks] = *(const pca::u32x4*)(kbase + (int64_t)key * D + ks * 32 + g * 8);
        }
        // V rows by LDS-DMA, rotated by 32 B per row on the source side (attn_small_kernel)
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            const int c = lane + i * 64, row = c / CPR, pos = c - row * CPR;
            const int col = (pos - 2 * (row & 7)) & (CPR - 1);
            const int rr = key0 + row < k1 ? key0 + row : k1 - 1;
            pca::glds16(vbase + (int64_t)rr * D + col * 8, Vwb + i * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
        h8 pb[RT][2], pbl[RT][2];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float sv[4][4];
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const h8 a = __builtin_bit_cast(h8, kr[kb][ks]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[rt][ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qfl[rt][ks], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + kb * 16 + g * 4 + r;
                    const float s = key < k1 ? acc[r] * scale_log2 : -INFINITY;
                    sv[kb][r] = s;
                    mx = fmaxf(mx, s);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run[rt], mx);
            const float alpha = pca::fast_exp2(m_run[rt] - m_new);
            float rs = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = pca::fast_exp2(sv[kb][r] - m_new);
                    rs += e;
                    const _Float16 eh = (_Float16)e;
                    pb[rt][kb >> 1][(kb & 1) * 4 + r] = eh;
                    pbl[rt][kb >> 1][(kb & 1) * 4 + r] = (_Float16)(e - (float)eh);
                }
            rs += __shfl_xor(rs, 16);
            rs += __shfl_xor(rs, 32);
            l_run[rt] = l_run[rt] * alpha + rs;
#pragma unroll
            for (int db = 0; db < DB; ++db) { o[rt][db][0] *= alpha; o[rt][db][1] *= alpha; o[rt][db][2] *= alpha; o[rt][db][3] *= alpha; }
            m_run[rt] = m_new;
        }
        // the V tile has landed (this wave's own DMA: vmcnt covers it), back transposed
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int vrow = t * 32 + g * 4 + (n >> 2);
                const _Float16* vp = Vw + vrow * D + ((db * 16 + (n & 3) * 4 + 16 * (vrow & 7)) & (D - 1));
                const pca::h4 lo = pca::lds_tr_read(vp);
                const pca::h4 hi = pca::lds_tr_read(vp + 16 * D);
                const h8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    o[rt][db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb[rt][t], o[rt][db], 0, 0, 0);
                    o[rt][db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pbl[rt][t], o[rt][db], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();             // (the next tile's DMA overwrites what these reads took)
    }

    // the four waves' partials through LDS, in wave order: one (O, m, l) record per (slot, head, trunk split)
    __syncthreads();
    float* mo = (float*)smem;                            // [RT][4][DB][64][4]
    float* mml = mo + RT * 4 * DB * 64 * 4;              // [RT][4][16][2]
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int db = 0; db < DB; ++db) *(f4*)(mo + (((rt * 4 + wave) * DB + db) * 64 + lane) * 4) = o[rt][db];
        if (g == 0) { mml[((rt * 4 + wave) * 16 + n) * 2] = m_run[rt]; mml[((rt * 4 + wave) * 16 + n) * 2 + 1] = l_run[rt]; }
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        float mw[4], lw[4], mstar = kNegBig;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            mw[w] = mml[((rt * 4 + w) * 16 + n) * 2]; lw[w] = mml[((rt * 4 + w) * 16 + n) * 2 + 1];
            mstar = fmaxf(mstar, mw[w]);
        }
        float wt[4], lsum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { wt[w] = pca::fast_exp2(mw[w] - mstar); lsum += wt[w] * lw[w]; }
        if (sb[rt] >= 0) {
            const int64_t slot = ((int64_t)sb[rt] * H + kvh * G + gh[rt]) * nrec + split;
            constexpr int DPW = (DB + 3) / 4;                // head-dim blocks merged by one wave
#pragma unroll
            for (int j = 0; j < DPW; ++j) {
                const int db = wave * DPW + j;
                if (db < DB) {
                    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const f4 x = *(const f4*)(mo + (((rt * 4 + w) * DB + db) * 64 + lane) * 4);
                        acc[0] += wt[w] * x[0]; acc[1] += wt[w] * x[1]; acc[2] += wt[w] * x[2]; acc[3] += wt[w] * x[3];
                    }
                    *(f4*)(part_o + slot * D + db * 16 + g * 4) = acc;
                }
            }
            if (wave == 0 && g == 0) { part_ml[slot * 2] = mstar; part_ml[slot * 2 + 1] = lsum; }
        }
    }
}

// merge of the trunk + own records of a (slot, head), in key order; a slot on its own has no trunk records
template <int D>
__global__ __launch_bounds__(D) void attn_merge_slots_trunk_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                   const int32_t* __restrict__ cap, const int32_t* __restrict__ len,
                                                                   const int32_t* __restrict__ live, const int32_t* __restrict__ leader,
                                                                   const int32_t* __restrict__ trunk,
                                                                   const uint64_t* __restrict__ kv_base, int S, int H, int nsplit_t,
                                                                   int nrec, _Float16* __restrict__ of_hi,
                                                                   _Float16* __restrict__ of_lo) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    if (live[b] == 0) return;
    const int past = len[b];
    if (past < 0 || past >= cap[b]) return;
    const int64_t base = ((int64_t)b * H + h) * nrec;
    const int s0 = slot_trunk_rows(b, S, kv_base, cap, len, leader, trunk) > 0 ? 0 : nsplit_t;
    float ms = kNegBig;
    for (int s = s0; s < nrec; ++s) ms = fmaxf(ms, part_ml[(base + s) * 2]);
    float num = 0.0f, den = 0.0f;
    for (int s = s0; s < nrec; ++s) {
        const float wt = exp2f(part_ml[(base + s) * 2] - ms);
        den = fmaf(wt, part_ml[(base + s) * 2 + 1], den);
        num = fmaf(wt, part_o[(base + s) * D + d], num);
    }
    _Float16 hi, lo;
    pc_split(num / den, hi, lo);
    const int64_t off = frag_off(b, h * D + d, H * D / 32);
    of_hi[off] = hi;
    of_lo[off] = lo;
}

struct TrunkArgs {
    const _Float16 *q_hi, *q_lo; int64_t q_ts;
    const uint64_t* kv_base; const int32_t *cap, *len, *live, *leader, *trunk;
    int S, layer, H, Hkv; float scale_log2; int ns_own, ns_trunk; float *part_o, *part_ml; _Float16 *of_hi, *of_lo;
};

template <int D, int GQ>
void launch_own_trunk(const TrunkArgs& a, hipStream_t st) {
    const int passes = (a.H / a.Hkv + GQ - 1) / GQ;
    hipLaunchKernelGGL((attn_decode_slots_kernel<D, GQ, true>), dim3(a.ns_own, a.Hkv * passes, a.S), dim3(kThreads), 0, st, a.q_hi,
                       a.q_lo, a.q_ts, a.kv_base, a.cap, a.len, a.live, a.layer, a.H, a.Hkv, a.scale_log2, a.ns_own, a.part_o, a.part_ml,
                       a.leader, a.trunk, a.ns_trunk + a.ns_own, a.ns_trunk, a.S);
}

template <int D>
void launch_trunk_d(const TrunkArgs& a, hipStream_t st) {
    const int G = a.H / a.Hkv, nrec = a.ns_trunk + a.ns_own;
    if (G == 1)
        hipLaunchKernelGGL((attn_trunk_slots_kernel<D, 1>), dim3(a.ns_trunk, a.Hkv, a.S), dim3(kThreads), 0, st, a.q_hi, a.q_lo, a.q_ts,
                           a.kv_base, a.cap, a.len, a.live, a.leader, a.trunk, a.S, a.layer, a.H, a.Hkv, a.scale_log2, a.ns_trunk, nrec,
                           a.part_o, a.part_ml);
    else
        hipLaunchKernelGGL((attn_trunk_slots_kernel<D, 2>), dim3(a.ns_trunk, a.Hkv * ((G + 1) / 2), a.S), dim3(kThreads), 0, st, a.q_hi,
                           a.q_lo, a.q_ts, a.kv_base, a.cap, a.len, a.live, a.leader, a.trunk, a.S, a.layer, a.H, a.Hkv, a.scale_log2,
                           a.ns_trunk, nrec, a.part_o, a.part_ml);
    if (G == 1) launch_own_trunk<D, 1>(a, st);
    else if (G <= 4) launch_own_trunk<D, 4>(a, st);
    else launch_own_trunk<D, 8>(a, st);
    hipLaunchKernelGGL(attn_merge_slots_trunk_kernel<D>, dim3(a.H, a.S), dim3(D), 0, st, a.part_o, a.part_ml, a.cap, a.len, a.live,
                       a.leader, a.trunk, a.kv_base, a.S, a.H, a.ns_trunk, nrec, a.of_hi, a.of_lo);
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

bool slot_shape_ok(int S, int H, int Hkv, int D) {
    return S >= 1 && S <= 16 && H > 0 && Hkv > 0 && H % Hkv == 0 && (D == 64 || D == 128);
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
    hipLaunchKernelGGL(rope_append_slots_kernel, dim3(S), dim3(kThreads), 0, (hipStream_t)stream, qkv, ld, in_layout,
                       (_Float16*)q_hi, (_Float16*)q_lo, q_token_stride, (const float2*)cs, kv_base, cap, len, live, layer, H, Hkv, D);
    return pc_check_launch("rope_append_slots_kernel");
}

PC_EXPORT int64_t pc_attn_decode_slots_workspace_bytes(int32_t S, int32_t H, int32_t D, int32_t nsplit) {
    if (S < 1 || H < 1 || D < 1 || nsplit < 1) return 0;
    return (int64_t)S * H * nsplit * (D + 2) * (int64_t)sizeof(float);
}

PC_EXPORT int pc_attn_decode_slots(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                   const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t layer, int32_t H,
                                   int32_t Hkv, int32_t D, float softmax_scale, int32_t nsplit, void* workspace,
                                   int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, void* stream) {
    PC_REQUIRE(slot_shape_ok(S, H, Hkv, D) && layer >= 0, PC_ERR_ARG,
               "pc_attn_decode_slots: 1 <= S <= 16, H a multiple of Hkv, head_dim 64 or 128");
    PC_REQUIRE(nsplit >= 1 && nsplit <= kMaxSplit, PC_ERR_ARG, "pc_attn_decode_slots: nsplit must be in [1, 32]");
    PC_REQUIRE(q_hi && q_lo && kv_base && cap && len && live && workspace && out_frag_hi && out_frag_lo, PC_ERR_ARG,
               "pc_attn_decode_slots: null pointer");
    PC_REQUIRE(q_token_stride % 8 == 0 && ((uintptr_t)q_hi & 15) == 0 && ((uintptr_t)q_lo & 15) == 0 && (H * D) % 32 == 0, PC_ERR_ARG,
               "pc_attn_decode_slots: q rows must keep 16-byte alignment and H * head_dim be a multiple of 32");
    PC_REQUIRE(workspace_bytes >= pc_attn_decode_slots_workspace_bytes(S, H, D, nsplit) && ((uintptr_t)workspace & 7) == 0, PC_ERR_ARG,
               "pc_attn_decode_slots: workspace too small (pc_attn_decode_slots_workspace_bytes) or misaligned");
    float* part_o = (float*)workspace;
    float* part_ml = part_o + (int64_t)S * H * nsplit * D;
    const float scale_log2 = softmax_scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    if (D == 128) {
        launch_decode_d<128>(S, H, Hkv, nsplit, st, (const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len,
                             live, layer, scale_log2, part_o, part_ml);
        hipLaunchKernelGGL(attn_merge_slots_kernel<128>, dim3(H, S), dim3(128), 0, st, part_o, part_ml, cap, len, live, H, nsplit,
                           (_Float16*)out_frag_hi, (_Float16*)out_frag_lo);
    } else {
        launch_decode_d<64>(S, H, Hkv, nsplit, st, (const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len,
                            live, layer, scale_log2, part_o, part_ml);
        hipLaunchKernelGGL(attn_merge_slots_kernel<64>, dim3(H, S), dim3(64), 0, st, part_o, part_ml, cap, len, live, H, nsplit,
                           (_Float16*)out_frag_hi, (_Float16*)out_frag_lo);
    }
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
    PC_REQUIRE(slot_shape_ok(S, H, Hkv, D) && layer >= 0, PC_ERR_ARG,
               "pc_attn_decode_slots_trunk: 1 <= S <= 16, H a multiple of Hkv, head_dim 64 or 128");
    PC_REQUIRE(nsplit_own >= 1 && nsplit_own <= kMaxSplit && nsplit_trunk >= 1 && nsplit_trunk <= kMaxSplit, PC_ERR_ARG,
               "pc_attn_decode_slots_trunk: nsplit_own and nsplit_trunk must be in [1, 32]");
    PC_REQUIRE(q_hi && q_lo && kv_base && cap && len && live && leader && trunk && workspace && out_frag_hi && out_frag_lo, PC_ERR_ARG,
               "pc_attn_decode_slots_trunk: null pointer");
    PC_REQUIRE(q_token_stride % 8 == 0 && ((uintptr_t)q_hi & 15) == 0 && ((uintptr_t)q_lo & 15) == 0 && (H * D) % 32 == 0, PC_ERR_ARG,
               "pc_attn_decode_slots_trunk: q rows must keep 16-byte alignment and H * head_dim be a multiple of 32");
    PC_REQUIRE(workspace_bytes >= pc_attn_decode_slots_trunk_workspace_bytes(S, H, D, nsplit_own, nsplit_trunk) &&
                   ((uintptr_t)workspace & 15) == 0,
               PC_ERR_ARG, "pc_attn_decode_slots_trunk: workspace too small (pc_attn_decode_slots_trunk_workspace_bytes) or misaligned");
    TrunkArgs a;
    a.q_hi = (const _Float16*)q_hi; a.q_lo = (const _Float16*)q_lo; a.q_ts = q_token_stride;
    a.kv_base = kv_base; a.cap = cap; a.len = len; a.live = live; a.leader = leader; a.trunk = trunk;
    a.S = S; a.layer = layer; a.H = H; a.Hkv = Hkv; a.scale_log2 = softmax_scale * 1.4426950408889634f;
    a.ns_own = nsplit_own; a.ns_trunk = nsplit_trunk;
    a.part_o = (float*)workspace;
    a.part_ml = a.part_o + (int64_t)S * H * (nsplit_own + nsplit_trunk) * D;
    a.of_hi = (_Float16*)out_frag_hi; a.of_lo = (_Float16*)out_frag_lo;
    if (D == 128) launch_trunk_d<128>(a, (hipStream_t)stream);
    else launch_trunk_d<64>(a, (hipStream_t)stream);
    return pc_check_launch("attn_trunk_slots_kernel");
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
