// Batched decode over slots with int8 K / V images: the one-row slot attention of pc_slots.hip reading, per slot, an image of the
// sequence's rows in the format of pc_kv_q8.hip -- 0.516 of the fp16 bytes -- instead of the fp16 arena.
//
// Replaces, for S sequences at once, with the keys held as int8 codes and one fp32 scale per row and plane:
//           softmax(q k^T / sqrt(d)) v over the sequence's keys  promptcache/model/llama2.py:366-400
//
// Image of one slot, qcap rows per plane, P = n_layers * 2 * n_kv_heads planes in the arena's plane order -- ONE contiguous run,
// the layout of pc_kv_q8.hip at n = qcap:
//   int8  codes [P][qcap][D]
//   fp32  scale [P][qcap]      starts at byte P*qcap*D
//
// A live slot b (live[b] != 0, 0 <= len[b] < cap[b]) attends over len + 1 keys.  Keys [0, len) come from the image, an element's
// value is (float)code * scale in fp32 (no fp16 rounding of the product; the scale is applied to the reduced dot on the K side
// and folded into p on the V side).  Key len is the row pc_rope_append_slots has just written: it is read from the fp16 arena,
// exact.  The key axis is split as pc_attn_decode_slots splits it (chunk = ceil((len + 1) / nsplit), host-fixed nsplit); the
// partial records and the merge are that entry's (pcr::launch_attn_merge_slots).
//
// Staging while reading: the workgroup whose key slice holds key len also quantises that fp16 row -- K and V of its kv head -- with
// the pinned arithmetic (pcq::quant_row16) and stores codes and scale at image row len; of the G = H / Hkv passes over a kv head
// only the first does.  No workgroup of the launch reads image row len (the image keys end at len - 1), so nothing is handed
// from one workgroup to another; no other image row is written.
//
// Order of summation, all a function of the slot's own length and of nsplit: a lane group (8 lanes, 16 head dims each) keeps an
// online softmax over keys k0 + grp, k0 + grp + 32, ..., four at a time; the group that takes the exact row (group 0 of wave 0)
// adds it last; the eight groups of a wave are merged through lane exchanges, the four waves through LDS, in index order.  A
// slot's bits depend on nothing another slot holds, nor on its index.
//
// One instantiation (head_dim 128, one query head per workgroup pass): a kv head with G query heads is read G times.
//
// Int8-only residency (pc_rope_append_slots_q8 / pc_attn_decode_slots_q8_fresh): a slot keeps no fp16 arena.  kv_base[b] is then the
// slot's FRESH-ROW buffer, fp16 [P][D] (plane stride D): the append launch writes the step's K / V row there AND quantises it into
// image row len (rope_append_slots_q8_kernel), and the attention -- the kernel above with `fresh` set -- reads the exact row from
// kv_base[b] + plane * D and stages nothing.  cap[b] is still the bound on len.
//
// Prompt-lookup drafts over images (pc_rope_append_slots_rows_q8 / pc_attn_verify_slots_q8, model/llama_hip.py LookupSlotLoopQ8):
// the step of pc_lookup_slots.hip, k + 1 rows per slot.  The append launch writes every row as fp16 (arena row len + i, or row i
// of a fresh-row buffer that is now [P][k + 1][D]) AND as image row len + i; the attention gives draft row i the image keys
// [0, len + i) and its own key exact -- what the one-row step above computes for the token at that position, whatever the step
// boundaries and however many drafts were accepted.
//
// Shared trunks over images (pc_attn_decode_slots_trunk_q8, model/llama_hip.py SlotLoopQ8 with trunks): slots whose first T rows
// are the same fp16 rows hold the same image rows [0, T) -- pc_kv_quant_q8_rows is row-local -- so a group's trunk is read once
// per step, from the leader's image, for all live members (attn_trunk_slots_q8_kernel); every slot reads image rows [T, len) and
// the exact row of its own and stages that row into its own image (attn_decode_slots_q8_kernel<true>).  One predicate,
// slot_trunk_rows_q8 (pc_lookup_common.h), is asked by both launches and by the merge.  Image rows below len are written by nobody.
#include <hip/hip_fp16.h>
#include <math.h>

#include "pc_attn_rows.h"
#include "pc_kv_q8_quant.h"

namespace {

using pca::kNegBig;
using pca::kThreads;
using pcr::h8;
using pcr::load8;
using pcr::SlotAttnArgs;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kD = 128;
constexpr int kLPK = kD / 16;        // lanes per key row: 16 codes (one 16-byte load) each
constexpr int kGPW = 64 / kLPK;      // key groups per wave: a wave instruction reads 8 consecutive rows, 1 KiB
constexpr int kNG = 4 * kGPW;        // key groups per workgroup
constexpr int kU = 4;                // keys in flight per group

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ---- RoPE + append of k + 1 rows per slot into image and fp16 row, one workgroup per (draft row, slot) ------------------------
// (pc_rope_append_slots_rows_q8; pc_rope_append_slots_q8 is its k = 0, fresh = 1 case.)  A slot runs under lookup_slot_runs and
// with len + k + 1 <= qcap; row r = b (k + 1) + i of the projection is rotated with row r of the table.
// q: the work items and the arithmetic of rope_append_slots_rows_kernel (pcr::rope_pairs8), bit for bit.  K / V: a row of
// a kv head is held by 8 consecutive lanes, lane `sub` with features [8 sub, 8 sub + 8) and [64 + 8 sub, 64 + 8 sub + 8) -- K as
// that kernel's rotary work item has them, V loaded the same way --, rounded to fp16 as that kernel rounds what it stores.  The
// fp16 row of plane (layer * 2) * Hkv + h (K) / + Hkv (V) goes -- `fresh` is uniform over the launch -- to row i of the fresh-row
// buffer kv_base[b] (fp16 [P][k + 1][D]) or to arena row len + i (plane stride cap[b]), and through pcq::quant_row16 -- the row
// maximum is an exchange among the 8 lanes; a code depends on its value and that maximum only -- into image row len + i: this
// lane's first two code dwords are bytes [8 sub, 8 sub + 8) of the row, the other two bytes [64 + 8 sub, ..).
__global__ __launch_bounds__(kThreads) void rope_append_slots_q8_kernel(
    const float* __restrict__ qkv, int64_t ld, int layout, _Float16* __restrict__ q_hi, _Float16* __restrict__ q_lo, int64_t q_ts,
    const float2* __restrict__ cs, const uint64_t* __restrict__ kv_base, const uint64_t* __restrict__ kvq_base,
    const int32_t* __restrict__ cap, const int32_t* __restrict__ len, const int32_t* __restrict__ live, int k, int layer, int n_layers,
    int H, int Hkv, int qcap, int fresh_rows) {
    const int i = blockIdx.x, b = blockIdx.y;
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
    if (len[b] + k + 1 > qcap) return;                          // (nothing of this slot is written anywhere)
    const int past = len[b] + i;                                // (< cap and < qcap)
    const int rr = b * (k + 1) + i;
    constexpr int half = kD / 2;
    const float2* csr = cs + (int64_t)rr * half;
    const float* row = qkv + (int64_t)rr * ld;
    for (int it = threadIdx.x; it < H * kLPK; it += kThreads) {
        const int h = it / kLPK, ch = it - h * kLPK;
        const float* src = row + (int64_t)h * kD;
        float lo[8], hi[8];
        load8(src + (layout ? ch * 16 : ch * 8), lo);
        load8(src + (layout ? ch * 16 + 8 : half + ch * 8), hi);
        h8 olo, ohi, rlo, rhi;
        pcr::rope_pairs8(lo, hi, csr + ch * 8, olo, ohi, rlo, rhi);
        _Float16* dh = q_hi + (int64_t)rr * q_ts + (int64_t)h * kD;
        _Float16* dl = q_lo + (int64_t)rr * q_ts + (int64_t)h * kD;
        *(h8*)(dh + ch * 8) = olo;
        *(h8*)(dh + half + ch * 8) = ohi;
        *(h8*)(dl + ch * 8) = rlo;
        *(h8*)(dl + half + ch * 8) = rhi;
    }
    // rows [0, Hkv): K of kv head r; rows [Hkv, 2 Hkv): V of kv head r - Hkv -- projection head H + r, plane plane0 + r
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane % kLPK, nrow = 2 * Hkv;
    const int64_t plane0 = (int64_t)(layer * 2) * Hkv;
    // where plane p's fp16 row lies: fresh + p * pstride + roff
    _Float16* fresh = (_Float16*)(uintptr_t)kv_base[b];
    const int64_t pstride = fresh_rows ? (int64_t)(k + 1) * kD : (int64_t)cap[b] * kD;
    const int64_t roff = fresh_rows ? (int64_t)i * kD : (int64_t)past * kD;
    char* img = (char*)(uintptr_t)kvq_base[b];
    float* sbase = (float*)(img + (int64_t)n_layers * 2 * Hkv * qcap * kD);
    for (int r0 = wave * kGPW; r0 < nrow; r0 += 4 * kGPW) {     // (wave-uniform trip count: every lane runs the exchanges)
        const int r = r0 + lane / kLPK;
        const bool on = r < nrow;                               // (whole rows: uniform over a row's 8 lanes)
        float lo[8], hi[8];
        if (on) {
            const float* src = row + (int64_t)(H + r) * kD;
            load8(src + (layout ? sub * 16 : sub * 8), lo);
            load8(src + (layout ? sub * 16 + 8 : half + sub * 8), hi);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) lo[e] = hi[e] = 0.0f;
        }
        h8 olo, ohi;
        if (r < Hkv) {
            h8 rlo, rhi;
            pcr::rope_pairs8(lo, hi, csr + sub * 8, olo, ohi, rlo, rhi);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) { olo[e] = (_Float16)lo[e]; ohi[e] = (_Float16)hi[e]; }
        }
        float x[16];
#pragma unroll
        for (int e = 0; e < 8; ++e) { x[e] = (float)olo[e]; x[8 + e] = (float)ohi[e]; }
        uint32_t w[4];
        float qs;
        pcq::quant_row16(x, 3, w, qs);
        if (on) {
            _Float16* fp = fresh + (plane0 + r) * pstride + roff;
            *(h8*)(fp + sub * 8) = olo;
            *(h8*)(fp + half + sub * 8) = ohi;
            char* cp = img + ((plane0 + r) * qcap + past) * kD;
            *(u32x2*)(cp + sub * 8) = u32x2{w[0], w[1]};
            *(u32x2*)(cp + half + sub * 8) = u32x2{w[2], w[3]};
            if (sub == 0) sbase[(plane0 + r) * qcap + past] = qs;
        }
    }
}

__device__ __forceinline__ float code_f32(uint32_t w, int b) { return (float)(int)(int8_t)(w >> (8 * b)); }

// grid (split, query head, slot)
// TRUNK (pc_attn_decode_slots_trunk_q8): a slot with shared rows (slot_trunk_rows_q8) takes keys [t0, len] only -- image rows
// [t0, len) of its OWN image and the exact row; its image rows [0, t0) are never read, the keys in front of t0 are the trunk
// launch's -- and its partials are records rec0 .. rec0 + nsplit - 1 of the nrec records per (slot, head).  t0 <= len: at least the
// exact key is left.  With t0 = 0 the arithmetic is the plain instantiation's.
template <bool TRUNK = false>
__global__ __launch_bounds__(kThreads) void attn_decode_slots_q8_kernel(
    const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo, int64_t q_ts, const uint64_t* __restrict__ kv_base,
    const uint64_t* __restrict__ kvq_base, const int32_t* __restrict__ cap, const int32_t* __restrict__ len,
    const int32_t* __restrict__ live, int layer, int n_layers, int H, int Hkv, int qcap, float scale_log2, int nsplit,
    float* __restrict__ part_o, float* __restrict__ part_ml, int fresh, const int32_t* __restrict__ leader = nullptr,
    const int32_t* __restrict__ trunk = nullptr, int nrec = 0, int rec0 = 0, int S = 0) {
    __shared__ float sm[4][kD + 2];

    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    if (live[b] == 0) return;
    const int past = len[b], c = cap[b];
    if (past < 0 || past >= c) return;
    if (past >= qcap) return;                     // out of contract (the host sizes qcap >= every cap): nothing leaves the image
    const int G = H / Hkv, kvh = h / G;
    const int n = past + 1;                       // keys of this slot: image rows [0, past) and the row just appended
    int t0 = 0;                                   // first key of this launch (<= past)
    if constexpr (TRUNK) t0 = slot_trunk_rows_q8(b, S, kvq_base, qcap, len, leader, trunk);
    const int chunk = (n - t0 + nsplit - 1) / nsplit;
    const int k0 = t0 + split * chunk, k1 = min(n, k0 + chunk);
    const int kq = min(k1, past);                 // image keys of this slice: [k0, kq)
    const bool has_new = k0 <= past && past < k1; // (uniform over the workgroup)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % kLPK, grp = wave * kGPW + lane / kLPK;
    // image planes of this kv head (rows [0, past] of them are all the kernel touches, and past < qcap)
    const int64_t kplane = (int64_t)(layer * 2) * Hkv + kvh, vplane = kplane + Hkv;
    const char* img = (const char*)(uintptr_t)kvq_base[b];
    const float* sbase = (const float*)(img + (int64_t)n_layers * 2 * Hkv * qcap * kD);
    const char* kc = img + kplane * qcap * kD + sub * 16;
    const char* vc = img + vplane * qcap * kD + sub * 16;
    const float* ks = sbase + kplane * qcap;
    const float* vs = sbase + vplane * qcap;

    float q[16], acc[16], m = kNegBig, l = 0.0f;
    {
        const int64_t qo = (int64_t)b * q_ts + (int64_t)h * kD + sub * 16;
        const h8 a0 = *(const h8*)(q_hi + qo), a1 = *(const h8*)(q_hi + qo + 8);
        const h8 r0 = *(const h8*)(q_lo + qo), r1 = *(const h8*)(q_lo + qo + 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            q[e] = ((float)a0[e] + (float)r0[e]) * scale_log2;
            q[8 + e] = ((float)a1[e] + (float)r1[e]) * scale_log2;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    }

    for (int base = k0; base < kq; base += kNG * kU) {
        u32x4 kk[kU], vv[kU];
        float sk[kU], sv[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int key = base + u * kNG + grp;
            ok[u] = key < kq;
            const int row = min(key, kq - 1);     // (a key past the slice re-reads its last row and is masked below)
            kk[u] = *(const u32x4*)(kc + (int64_t)row * kD);
            vv[u] = *(const u32x4*)(vc + (int64_t)row * kD);
            sk[u] = ks[row];
            sv[u] = vs[row];
        }
        float s[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            float d = 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) d = fmaf(q[e], code_f32(kk[u][e >> 2], e & 3), d);
#pragma unroll
            for (int o = 1; o < kLPK; o <<= 1) d += __shfl_xor(d, o);
            s[u] = ok[u] ? d * sk[u] : -INFINITY;
        }
        float mn = m;
#pragma unroll
        for (int u = 0; u < kU; ++u) mn = fmaxf(mn, s[u]);
        const float sc = exp2f(m - mn);
        l *= sc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] *= sc;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const float p = exp2f(s[u] - mn);
            l += p;
            const float pv = ok[u] ? p * sv[u] : 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = fmaf(pv, code_f32(vv[u][e >> 2], e & 3), acc[e]);
        }
        m = mn;
    }

    // the row just appended: exact from the fp16 arena, the last key of group 0 of wave 0; staged into the image on the way.
    // fresh (uniform over the launch): the row lies in the slot's fresh-row buffer, plane stride D, and its image row is written
    if (has_new && wave == 0) {                   // (wave-uniform; every lane group of the wave loads the same row)
        const _Float16* kp = (const _Float16*)(uintptr_t)kv_base[b] + (fresh ? kplane : kplane * c + past) * kD + sub * 16;
        const _Float16* vp = (const _Float16*)(uintptr_t)kv_base[b] + (fresh ? vplane : vplane * c + past) * kD + sub * 16;
        const h8 k0v = *(const h8*)kp, k1v = *(const h8*)(kp + 8), v0v = *(const h8*)vp, v1v = *(const h8*)(vp + 8);
        float kx[16], vx[16];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            kx[e] = (float)k0v[e]; kx[8 + e] = (float)k1v[e];
            vx[e] = (float)v0v[e]; vx[8 + e] = (float)v1v[e];
        }
        float d = 0.0f;
#pragma unroll
        for (int e = 0; e < 16; ++e) d = fmaf(q[e], kx[e], d);
#pragma unroll
        for (int o = 1; o < kLPK; o <<= 1) d += __shfl_xor(d, o);
        if (grp == 0) {
            const float mn = fmaxf(m, d);
            const float sc = exp2f(m - mn), p = exp2f(d - mn);
            l = l * sc + p;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = fmaf(p, vx[e], acc[e] * sc);
            m = mn;
        }
        if (!fresh && h == kvh * G) {             // the first pass over this kv head stages the row (wave-uniform)
            uint32_t wk[4], wv[4];
            float qsk, qsv;
            pcq::quant_row16(kx, 3, wk, qsk);
            pcq::quant_row16(vx, 3, wv, qsv);
            if (grp == 0) {
                char* wimg = (char*)(uintptr_t)kvq_base[b];
                float* wsb = (float*)(wimg + (int64_t)n_layers * 2 * Hkv * qcap * kD);
                *(u32x4*)(wimg + (kplane * qcap + past) * kD + sub * 16) = u32x4{wk[0], wk[1], wk[2], wk[3]};
                *(u32x4*)(wimg + (vplane * qcap + past) * kD + sub * 16) = u32x4{wv[0], wv[1], wv[2], wv[3]};
                if (sub == 0) {
                    wsb[kplane * qcap + past] = qsk;
                    wsb[vplane * qcap + past] = qsv;
                }
            }
        }
    }

    // the key groups of a wave -> its first group
#pragma unroll
    for (int o = kLPK; o < 64; o <<= 1) {
        const float mo = __shfl_xor(m, o), lo = __shfl_xor(l, o);
        const float mn = fmaxf(m, mo);
        const float wa = exp2f(m - mn), wb = exp2f(mo - mn);
        l = l * wa + lo * wb;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = acc[e] * wa + __shfl_xor(acc[e], o) * wb;
        m = mn;
    }
    if (lane < kLPK) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sm[wave][sub * 16 + e] = acc[e];
        if (sub == 0) { sm[wave][kD] = m; sm[wave][kD + 1] = l; }
    }
    __syncthreads();
    // the four waves -> this split's partial (unnormalised sum, maximum, denominator)
    if (tid < kD) {
        const int d = tid;
        float ms = sm[0][kD];
#pragma unroll
        for (int w = 1; w < 4; ++w) ms = fmaxf(ms, sm[w][kD]);
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float wt = exp2f(sm[w][kD] - ms);
            den = fmaf(wt, sm[w][kD + 1], den);
            num = fmaf(wt, sm[w][d], num);
        }
        const int64_t rec = TRUNK ? ((int64_t)b * H + h) * nrec + rec0 + split : ((int64_t)b * H + h) * nsplit + split;
        part_o[rec * kD + d] = num;
        if (d == 0) { part_ml[rec * 2] = ms; part_ml[rec * 2 + 1] = den; }
    }
}

// ---- k + 1 causally ordered query rows per slot over the int8 image (pc_attn_verify_slots_q8) ----------------------------------
// attn_verify_slots_kernel<128, 1> (pc_lookup_slots.hip) with the tile loop reading codes (pcr::attn_rows_tiles_q8): grid (split,
// kv head x pass, slot), a tile column is (draft row i, query head g of the kv head), 16 per pass.  The IMAGE keys of the slot
// are [0, len + k) -- rows len .. len + k - 1 are what pc_rope_append_slots_rows_q8 has just quantised -- and column (i, .) sees
// those below len + i: every key in front of its own, quantised, however the rows were spread over steps.  The wave slices are cut
// from len + k.  Its OWN key, len + i, is exact: the workgroups of split 0 leave it as one more record per (row, head), index
// nsplit behind the nsplit records of the slices: m = q . k * scale_log2 with q = (float)hi + (float)lo, the 128 products summed
// in fp32 as a wave's xor tree over lane pairs (an order D alone fixes), l = 1, O = v.  k / v: arena row len + i, or row i of the
// fresh-row buffer (`fresh_rows`, uniform over the launch).  Every record is written by exactly one workgroup and read by the
// merge launch only; no image byte is written.
__global__ __launch_bounds__(kThreads, 2) void attn_verify_slots_q8_kernel(
    const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo, int64_t q_ts, const uint64_t* __restrict__ kv_base,
    const uint64_t* __restrict__ kvq_base, const int32_t* __restrict__ cap, const int32_t* __restrict__ len,
    const int32_t* __restrict__ live, int k, int layer, int n_layers, int H, int Hkv, int qcap, float scale_log2, int nsplit,
    float* __restrict__ part_o, float* __restrict__ part_ml, int fresh_rows) {
    __shared__ __attribute__((aligned(16))) char smem[pcr::rows_lds_bytes<kD, 1>()];
    const int lane = threadIdx.x & 63, n = lane & 15, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int split = blockIdx.x, b = blockIdx.z;
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
    const int past = len[b], cb = cap[b];
    if (past + k + 1 > qcap) return;                 // out of contract: nothing leaves the image
    const int G = H / Hkv, cols = (k + 1) * G, passes = (cols + 15) / 16;
    const int kvh = blockIdx.y / passes, col0 = (blockIdx.y - kvh * passes) * 16;
    const int nimg = past + k;                       // image keys of the slot (< qcap)
    const int nrec = nsplit + 1;

    int64_t qoff[1], rec[1];
    bool pad[1];
    int lim[1];
    {
        const int c = col0 + n;
        pad[0] = c >= cols;
        const int di = pad[0] ? 0 : c / G, gh = pad[0] ? 0 : c - di * G;
        lim[0] = pad[0] ? 0 : past + di;
        qoff[0] = (int64_t)(b * (k + 1) + di) * q_ts + (int64_t)(kvh * G + gh) * kD;
        rec[0] = ((int64_t)(b * (k + 1) + di) * H + kvh * G + gh) * nrec + split;
    }
    int cpw = (nimg + nsplit * 4 - 1) / (nsplit * 4);              // keys per wave
    cpw = (cpw + 15) & ~15;
    const int k0 = (split * 4 + wave) * cpw;
    const int k1 = (k0 + cpw < nimg) ? k0 + cpw : nimg;

    const int64_t kplane = (int64_t)(layer * 2) * Hkv + kvh, vplane = kplane + Hkv;
    const char* img = (const char*)(uintptr_t)kvq_base[b];
    const float* sbase = (const float*)(img + (int64_t)n_layers * 2 * Hkv * qcap * kD);
    pcr::attn_rows_tiles_q8<1>(q_hi, q_lo, qoff, pad, lim, rec, img + kplane * qcap * kD, img + vplane * qcap * kD,
                               sbase + kplane * qcap, sbase + vplane * qcap, k0, k1, scale_log2, smem, part_o, part_ml);

    if (split != 0) return;
    // the exact key of every column of this pass: one column per wave turn, two features per lane
    const _Float16* ex = (const _Float16*)(uintptr_t)kv_base[b];
    for (int cc = wave; cc < 16; cc += 4) {
        const int c = col0 + cc;
        if (c >= cols) break;                                       // (wave-uniform)
        const int di = c / G, h = kvh * G + (c - di * G), row = b * (k + 1) + di;
        const int64_t ko = (fresh_rows ? kplane * (k + 1) + di : kplane * cb + past + di) * kD + lane * 2;
        const int64_t vo = (fresh_rows ? vplane * (k + 1) + di : vplane * cb + past + di) * kD + lane * 2;
        const int64_t qo = (int64_t)row * q_ts + (int64_t)h * kD + lane * 2;
        const pca::h2 qh = *(const pca::h2*)(q_hi + qo), ql = *(const pca::h2*)(q_lo + qo);
        const pca::h2 kx = *(const pca::h2*)(ex + ko), vx = *(const pca::h2*)(ex + vo);
        float d = ((float)qh[0] + (float)ql[0]) * (float)kx[0];
        d = fmaf((float)qh[1] + (float)ql[1], (float)kx[1], d);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) d += __shfl_xor(d, o);
        const int64_t r = ((int64_t)row * H + h) * nrec + nsplit;
        *(float2*)(part_o + r * kD + lane * 2) = make_float2((float)vx[0], (float)vx[1]);
        if (lane == 0) { part_ml[r * 2] = d * scale_log2; part_ml[r * 2 + 1] = 1.0f; }
    }
}

// ---- shared trunk over images: the keys a group of slots has in common, read once for all members (pc_attn_decode_slots_trunk_q8) -
// attn_verify_trunk_slots_kernel (pc_lookup_slots.hip) at k = 0 with the tile loop reading codes (pcr::attn_rows_tiles_q8): grid
// (trunk split, kv head x pass, candidate leader), S * G columns cut into passes; a tile column is (member m, query head g of the kv
// head), column index m * G + g among nmem * G, 16 per MFMA tile, RT tiles per pass.  The keys [0, T) are rows of the LEADER's image
// -- read whether or not the leader is live: no step writes an image row below len >= T -- and every column's limit is T.  Members
// are the live slots of leader gl with 0 <= len < cap, len < qcap -- the slots the own launch works for -- and slot_trunk_rows_q8 > 0,
// in slot order.  The key slices are a function of (T, nsplit_t), every reduction runs in a fixed order and a column of an MFMA
// tile depends on that column's B operand only: what a member gets does not depend on how many members the group has, on its place
// in the tile or on the slot index.  Records 0 .. nsplit_t - 1 of the nrec per (slot, head); pad columns are zero and are never
// written; no image byte is written.
template <int RT>
__global__ __launch_bounds__(kThreads, RT > 1 ? 1 : 2) void attn_trunk_slots_q8_kernel(
    const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo, int64_t q_ts, const uint64_t* __restrict__ kvq_base,
    const int32_t* __restrict__ cap, const int32_t* __restrict__ len, const int32_t* __restrict__ live,
    const int32_t* __restrict__ leader, const int32_t* __restrict__ trunk, int S, int layer, int n_layers, int H, int Hkv, int qcap,
    float scale_log2, int nsplit_t, int nrec, float* __restrict__ part_o, float* __restrict__ part_ml) {
    __shared__ __attribute__((aligned(16))) char smem[pcr::rows_lds_bytes<kD, RT>()];
    const int n = threadIdx.x & 15, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int split = blockIdx.x, gl = blockIdx.z;
    const int G = H / Hkv, passes = (S * G + 16 * RT - 1) / (16 * RT);
    const int kvh = blockIdx.y / passes, col0 = (blockIdx.y - kvh * passes) * 16 * RT;
    const int T = trunk[gl];
    if (leader[gl] != gl || T <= 0 || T > qcap || kvq_base[gl] == 0) return;  // (no slot_trunk_rows_q8 of this group is non-zero)

    // the member list, in slot order: lane b < S of every wave answers for slot b -- the S slots' words in one round of loads, not
    // one slot after the other -- and the ballot is the list (the same in every wave: workgroup-uniform)
    bool mem = false;
    {
        const int b = threadIdx.x & 63;
        if (b < S) {
            const int past = len[b];
            mem = leader[b] == gl && live[b] != 0 && past >= 0 && past < cap[b] && past < qcap &&
                  slot_trunk_rows_q8(b, S, kvq_base, qcap, len, leader, trunk) > 0;
        }
    }
    const uint32_t members = (uint32_t)__ballot(mem);                         // (S <= 16)
    const int nmem = __popc(members);
    if (col0 >= nmem * G) return;                    // workgroup-uniform: no member, or no column left for this pass

    // this lane's column of each tile: member, query head, slot (negative: a pad column) -- the slot of member m is the m-th set bit
    int gh[RT], qr[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int c = col0 + rt * 16 + n, m = c / G;
        gh[rt] = c - m * G;
        uint32_t rest = members;
        for (int j = 0; j < m && rest != 0; ++j) rest &= rest - 1;
        qr[rt] = (m < nmem && rest != 0) ? __builtin_ctz(rest) : -1;
    }

    int cpw = (T + nsplit_t * 4 - 1) / (nsplit_t * 4);             // keys per wave
    cpw = (cpw + 15) & ~15;
    const int k0 = (split * 4 + wave) * cpw;
    const int k1 = (k0 + cpw < T) ? k0 + cpw : T;

    int64_t qoff[RT], rec[RT];
    bool pad[RT];
    int lim[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        pad[rt] = qr[rt] < 0;
        const int row = pad[rt] ? 0 : qr[rt], head = kvh * G + (pad[rt] ? 0 : gh[rt]);
        lim[rt] = pad[rt] ? 0 : T;
        qoff[rt] = (int64_t)row * q_ts + (int64_t)head * kD;
        rec[rt] = ((int64_t)row * H + head) * nrec + split;
    }
    const int64_t kplane = (int64_t)(layer * 2) * Hkv + kvh, vplane = kplane + Hkv;
    const char* img = (const char*)(uintptr_t)kvq_base[gl];
    const float* sbase = (const float*)(img + (int64_t)n_layers * 2 * Hkv * qcap * kD);
    pcr::attn_rows_tiles_q8<RT>(q_hi, q_lo, qoff, pad, lim, rec, img + kplane * qcap * kD, img + vplane * qcap * kD,
                                sbase + kplane * qcap, sbase + vplane * qcap, k0, k1, scale_log2, smem, part_o, part_ml);
}

}  // namespace

namespace {

// Both attention entries: `fresh` = 0 reads the exact row from the arena and stages it, 1 reads it from the fresh-row buffer.
int attn_slots_q8(const char* name, int fresh, const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                  const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                  float softmax_scale, int32_t nsplit, void* workspace, int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo,
                  const uint64_t* kvq_base, int32_t qcap, int32_t n_layers, void* stream) {
    PC_REQUIRE(D == kD, PC_ERR_ARG, "%s: head_dim must be 128", name);
    PC_REQUIRE(kvq_base != nullptr, PC_ERR_ARG, "%s: null pointer", name);
    PC_REQUIRE(qcap >= 1 && n_layers >= 1 && layer < n_layers, PC_ERR_ARG,
               "%s: qcap >= 1 and 0 <= layer < n_layers (the image's scales start behind all its planes)", name);
    SlotAttnArgs a = {(const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len, live, nullptr, nullptr,
                      S, 0, layer, H, Hkv, 0.f, nsplit, 0, nullptr, nullptr, (_Float16*)out_frag_hi, (_Float16*)out_frag_lo};
    if (const int rc = pcr::slot_attn_prepare(name, false, false, 8, a, D, softmax_scale, workspace, workspace_bytes)) return rc;
    hipLaunchKernelGGL(attn_decode_slots_q8_kernel<false>, dim3(a.ns_own, a.H, a.S), dim3(kThreads), 0, (hipStream_t)stream, a.q_hi,
                       a.q_lo, a.q_ts, a.kv_base, kvq_base, a.cap, a.len, a.live, a.layer, n_layers, a.H, a.Hkv, qcap, a.scale_log2,
                       a.ns_own, a.part_o, a.part_ml, fresh, (const int32_t*)nullptr, (const int32_t*)nullptr, 0, 0, 0);
    pcr::launch_attn_merge_slots(a, D, false, (hipStream_t)stream);
    return pc_check_launch("attn_decode_slots_q8_kernel");
}

// trunk launch of pc_attn_decode_slots_trunk_q8; grid.y follows the kernel's own pass count, ceil(S * G / (16 * RT))
template <int RT>
void launch_trunk_q8(const SlotAttnArgs& a, int n_layers, hipStream_t st) {
    const int passes = pc_ceil_div(a.S * (a.H / a.Hkv), 16 * RT);
    hipLaunchKernelGGL(attn_trunk_slots_q8_kernel<RT>, dim3(a.ns_trunk, a.Hkv * passes, a.S), dim3(kThreads), 0, st, a.q_hi, a.q_lo,
                       a.q_ts, a.kvq_base, a.cap, a.len, a.live, a.leader, a.trunk, a.S, a.layer, n_layers, a.H, a.Hkv, a.qcap,
                       a.scale_log2, a.ns_trunk, a.ns_trunk + a.ns_own, a.part_o, a.part_ml);
}

}  // namespace

// pc_attn_decode_slots_q8 for slots that share their leading rows: three launches asking slot_trunk_rows_q8 -- the shared rows of
// every group from the leader's image (attn_trunk_slots_q8_kernel, RT = 2 where the S slots can fill more than one tile), every
// slot's own image rows and exact row (attn_decode_slots_q8_kernel<true>, which stages the row as the plain entry does), merge.
PC_EXPORT int pc_attn_decode_slots_trunk_q8(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                            const int32_t* cap, const int32_t* len, const int32_t* live, const int32_t* leader,
                                            const int32_t* trunk, int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                                            float softmax_scale, int32_t nsplit_own, int32_t nsplit_trunk, void* workspace,
                                            int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, const uint64_t* kvq_base,
                                            int32_t qcap, int32_t n_layers, void* stream) {
    const char* name = "pc_attn_decode_slots_trunk_q8";
    PC_REQUIRE(D == kD, PC_ERR_ARG, "%s: head_dim must be 128", name);
    PC_REQUIRE(kvq_base != nullptr, PC_ERR_ARG, "%s: null pointer", name);
    PC_REQUIRE(qcap >= 1 && n_layers >= 1 && layer < n_layers, PC_ERR_ARG,
               "%s: qcap >= 1 and 0 <= layer < n_layers (the image's scales start behind all its planes)", name);
    SlotAttnArgs a = {(const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len, live, leader, trunk,
                      S, 0, layer, H, Hkv, 0.f, nsplit_own, nsplit_trunk, nullptr, nullptr, (_Float16*)out_frag_hi, (_Float16*)out_frag_lo,
                      0, kvq_base, qcap};
    if (const int rc = pcr::slot_attn_prepare(name, false, true, 16, a, D, softmax_scale, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a.S * (a.H / a.Hkv) <= 16) launch_trunk_q8<1>(a, n_layers, st);
    else launch_trunk_q8<2>(a, n_layers, st);
    hipLaunchKernelGGL(attn_decode_slots_q8_kernel<true>, dim3(a.ns_own, a.H, a.S), dim3(kThreads), 0, st, a.q_hi, a.q_lo, a.q_ts,
                       a.kv_base, a.kvq_base, a.cap, a.len, a.live, a.layer, n_layers, a.H, a.Hkv, a.qcap, a.scale_log2, a.ns_own, a.part_o,
                       a.part_ml, 0, a.leader, a.trunk, a.ns_trunk + a.ns_own, a.ns_trunk, a.S);
    pcr::launch_attn_merge_slots(a, D, true, st);
    return pc_check_launch("attn_trunk_slots_q8_kernel");
}

PC_EXPORT int pc_attn_decode_slots_q8(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                      const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t layer,
                                      int32_t H, int32_t Hkv, int32_t D, float softmax_scale, int32_t nsplit, void* workspace,
                                      int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, const uint64_t* kvq_base,
                                      int32_t qcap, int32_t n_layers, void* stream) {
    return attn_slots_q8("pc_attn_decode_slots_q8", 0, q_hi, q_lo, q_token_stride, kv_base, cap, len, live, S, layer, H, Hkv, D,
                         softmax_scale, nsplit, workspace, workspace_bytes, out_frag_hi, out_frag_lo, kvq_base, qcap, n_layers, stream);
}

PC_EXPORT int pc_attn_decode_slots_q8_fresh(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                            const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t layer,
                                            int32_t H, int32_t Hkv, int32_t D, float softmax_scale, int32_t nsplit, void* workspace,
                                            int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, const uint64_t* kvq_base,
                                            int32_t qcap, int32_t n_layers, void* stream) {
    return attn_slots_q8("pc_attn_decode_slots_q8_fresh", 1, q_hi, q_lo, q_token_stride, kv_base, cap, len, live, S, layer, H, Hkv, D,
                         softmax_scale, nsplit, workspace, workspace_bytes, out_frag_hi, out_frag_lo, kvq_base, qcap, n_layers, stream);
}

namespace {

// Both append entries: pc_rope_append_slots_q8 is k = 0 with the fresh-row buffer.
int rope_append_q8(const char* name, const float* qkv, int64_t ld, int32_t in_layout, void* q_hi, void* q_lo, int64_t q_token_stride,
                   const float* cs, const uint64_t* kv_base, const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S,
                   int32_t k, int32_t layer, int32_t H, int32_t Hkv, int32_t D, const uint64_t* kvq_base, int32_t qcap,
                   int32_t n_layers, int32_t fresh, void* stream) {
    PC_REQUIRE(S >= 1 && S <= 16 && k >= 0 && k <= 15 && S * (k + 1) <= 64 && layer >= 0 && H > 0 && Hkv > 0, PC_ERR_ARG,
               "%s: bad sizes (1 <= S <= 16, 0 <= k <= 15, S * (k + 1) <= 64)", name);
    PC_REQUIRE(D == kD, PC_ERR_ARG, "%s: head_dim must be 128", name);
    PC_REQUIRE(qkv && q_hi && q_lo && cs && kv_base && cap && len && live && kvq_base, PC_ERR_ARG, "%s: null pointer", name);
    PC_REQUIRE(in_layout == 0 || in_layout == 1, PC_ERR_ARG, "%s: in_layout is 0 (natural) or 1 (rotary-pair tiles)", name);
    PC_REQUIRE(fresh == 0 || fresh == 1, PC_ERR_ARG, "%s: fresh is 0 (arena rows) or 1 (fresh-row buffers)", name);
    PC_REQUIRE(qcap >= 1 && n_layers >= 1 && layer < n_layers, PC_ERR_ARG,
               "%s: qcap >= 1 and 0 <= layer < n_layers (the image's scales start behind all its planes)", name);
    PC_REQUIRE(ld >= (int64_t)(H + 2 * Hkv) * D && ld % 4 == 0 && q_token_stride % 8 == 0 && ((uintptr_t)qkv & 15) == 0 &&
                   ((uintptr_t)q_hi & 15) == 0 && ((uintptr_t)q_lo & 15) == 0,
               PC_ERR_ARG, "%s: rows must keep 16-byte alignment", name);
    hipLaunchKernelGGL(rope_append_slots_q8_kernel, dim3(k + 1, S), dim3(kThreads), 0, (hipStream_t)stream, qkv, ld, in_layout,
                       (_Float16*)q_hi, (_Float16*)q_lo, q_token_stride, (const float2*)cs, kv_base, kvq_base, cap, len, live, k, layer,
                       n_layers, H, Hkv, qcap, fresh);
    return pc_check_launch("rope_append_slots_q8_kernel");
}

}  // namespace

PC_EXPORT int pc_rope_append_slots_q8(const float* qkv, int64_t ld, int32_t in_layout, void* q_hi, void* q_lo, int64_t q_token_stride,
                                      const float* cs, const uint64_t* kv_base, const int32_t* cap, const int32_t* len,
                                      const int32_t* live, int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                                      const uint64_t* kvq_base, int32_t qcap, int32_t n_layers, void* stream) {
    return rope_append_q8("pc_rope_append_slots_q8", qkv, ld, in_layout, q_hi, q_lo, q_token_stride, cs, kv_base, cap, len, live, S, 0,
                          layer, H, Hkv, D, kvq_base, qcap, n_layers, 1, stream);
}

PC_EXPORT int pc_rope_append_slots_rows_q8(const float* qkv, int64_t ld, int32_t in_layout, void* q_hi, void* q_lo,
                                           int64_t q_token_stride, const float* cs, const uint64_t* kv_base, const int32_t* cap,
                                           const int32_t* len, const int32_t* live, int32_t S, int32_t k, int32_t layer, int32_t H,
                                           int32_t Hkv, int32_t D, const uint64_t* kvq_base, int32_t qcap, int32_t n_layers,
                                           int32_t fresh, void* stream) {
    return rope_append_q8("pc_rope_append_slots_rows_q8", qkv, ld, in_layout, q_hi, q_lo, q_token_stride, cs, kv_base, cap, len, live, S,
                          k, layer, H, Hkv, D, kvq_base, qcap, n_layers, fresh, stream);
}

PC_EXPORT int64_t pc_attn_verify_slots_q8_workspace_bytes(int32_t S, int32_t k, int32_t H, int32_t D, int32_t nsplit) {
    if (S < 1 || k < 0 || H < 1 || D < 1 || nsplit < 1) return 0;
    return (int64_t)S * (k + 1) * H * (nsplit + 1) * (D + 2) * (int64_t)sizeof(float);
}

PC_EXPORT int pc_attn_verify_slots_q8(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                      const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t k, int32_t layer,
                                      int32_t H, int32_t Hkv, int32_t D, float softmax_scale, int32_t nsplit, void* workspace,
                                      int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, const uint64_t* kvq_base,
                                      int32_t qcap, int32_t n_layers, int32_t fresh, void* stream) {
    const char* name = "pc_attn_verify_slots_q8";
    PC_REQUIRE(D == kD, PC_ERR_ARG, "%s: head_dim must be 128", name);
    PC_REQUIRE(kvq_base != nullptr, PC_ERR_ARG, "%s: null pointer", name);
    PC_REQUIRE(qcap >= 1 && n_layers >= 1 && layer < n_layers, PC_ERR_ARG,
               "%s: qcap >= 1 and 0 <= layer < n_layers (the image's scales start behind all its planes)", name);
    PC_REQUIRE(fresh == 0 || fresh == 1, PC_ERR_ARG, "%s: fresh is 0 (arena rows) or 1 (fresh-row buffers)", name);
    // one record more per (row, head) than pc_attn_verify_slots: the exact key's
    SlotAttnArgs a = {(const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len, live, nullptr, nullptr,
                      S, k, layer, H, Hkv, 0.f, nsplit, 0, nullptr, nullptr, (_Float16*)out_frag_hi, (_Float16*)out_frag_lo, 1};
    if (const int rc = pcr::slot_attn_prepare(name, true, false, 16, a, D, softmax_scale, workspace, workspace_bytes)) return rc;
    const int passes = pc_ceil_div((a.k + 1) * (a.H / a.Hkv), 16);
    hipLaunchKernelGGL(attn_verify_slots_q8_kernel, dim3(a.ns_own, a.Hkv * passes, a.S), dim3(kThreads), 0, (hipStream_t)stream, a.q_hi,
                       a.q_lo, a.q_ts, a.kv_base, kvq_base, a.cap, a.len, a.live, a.k, a.layer, n_layers, a.H, a.Hkv, qcap, a.scale_log2,
                       a.ns_own, a.part_o, a.part_ml, fresh);
    pcr::launch_attn_merge_slots(a, D, false, (hipStream_t)stream);
    return pc_check_launch("attn_verify_slots_q8_kernel");
}
