// The middle of a prompt-lookup step over SLOTS (model/llama_hip.py LookupSlotLoop): every running sequence feeds k + 1 rows --
// its token and k drafts -- into one captured step, so row r = b * (k + 1) + i of every activation is draft row i of slot b.
//   pc_rope_append_slots_rows   pc_rope_append_slots for k + 1 rows per slot: K / V of row i go to arena row len[b] + i
//   pc_attn_verify_slots        per slot, draft row and head: softmax(q k^T) v over keys [0, len[b] + i] -- the staged rows, the
//                               rows earlier steps appended and draft rows 0..i of this step (a causal mask inside the draft rows)
//   pc_attn_verify_slots_trunk  the same for slots that share their leading rows (pc_attn_decode_slots_trunk's leader / trunk words):
//                               keys [0, T) come from the leader's arena, read once for all draft rows of all members
// The ends of the step (pc_lookup_draft_slots / pc_lookup_verify_slots) live beside their B = 1 forms in pc_lookup.hip.
//
// A slot takes part when it is live and len[b] + k + 1 <= cap[b]; otherwise no launch here reads or writes anything of it.
// Every workgroup works for one slot, the key slices are a function of the slot's own length, k and the host-fixed split count,
// and every reduction runs in a fixed order: a row's result does not depend on the other slots, the slot index or the live count.
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
constexpr int kMaxRows = 64;          // S * (k + 1)

__device__ __forceinline__ void load8(const float* p, float (&x)[8]) {
    const f4 a = *(const f4*)p, b = *(const f4*)(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[e] = a[e]; x[e + 4] = b[e]; }
}

// ---- RoPE + append, one workgroup per (draft row, slot) ----------------------------------------------------------------
// The work items and the arithmetic are rope_append_slots_kernel's (pc_slots.hip), which are rope_append_kernel<float>'s
// (pc_rope.hip): row r of the projection, rotated with row r of the table, q to row r of the pair, K / V to arena row len + i.
__global__ __launch_bounds__(kThreads) void rope_append_slots_rows_kernel(
    const float* __restrict__ qkv, int64_t ld, int layout, _Float16* __restrict__ q_hi, _Float16* __restrict__ q_lo, int64_t q_ts,
    const float2* __restrict__ cs, const uint64_t* __restrict__ kv_base, const int32_t* __restrict__ cap,
    const int32_t* __restrict__ len, const int32_t* __restrict__ live, int k, int layer, int H, int Hkv, int D) {
    const int i = blockIdx.x, b = blockIdx.y;
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
    const int c = cap[b], past = len[b] + i;                  // (< cap: len + k + 1 <= cap)
    const int r = b * (k + 1) + i;
    const int half = D >> 1;
    const int cph = D >> 4;  // 8-pair chunks per head
    const int nq = H * cph, nk = Hkv * cph, nv = Hkv * (D >> 3);
    const float2* csr = cs + (int64_t)r * half;
    const float* row = qkv + (int64_t)r * ld;
    _Float16* k_plane = (_Float16*)(uintptr_t)kv_base[b] + (int64_t)(layer * 2) * Hkv * c * D;
    _Float16* v_plane = k_plane + (int64_t)Hkv * c * D;
    for (int it = threadIdx.x; it < nq + nk + nv; it += blockDim.x) {
        if (it < nq + nk) {
            const bool is_q = it < nq;
            const int j = is_q ? it : it - nq;
            const int h = j / cph, ch = j - h * cph;
            const float* src = row + (int64_t)(is_q ? h : H + h) * D;
            _Float16* dst = is_q ? q_hi + (int64_t)r * q_ts + (int64_t)h * D : k_plane + ((int64_t)h * c + past) * D;
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
                _Float16* dl = q_lo + (int64_t)r * q_ts + (int64_t)h * D;
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

// ---- k + 1 causally ordered query rows per slot, split over the key axis ----------------------------------------------------
// The formulation is attn_trunk_slots_kernel's (pc_slots.hip), which is attn_small_kernel's (pc_attn.hip): S^T = K . Q^T and
// O^T += V^T . P^T on mfma_f32_16x16x32_f16, Q and P as hi / lo pairs, fp32 online softmax; every WAVE owns a contiguous slice of
// the split's keys, K fragments go from global memory into the A operand, V through a wave-private LDS tile and back transposed,
// no barrier until the four waves' partials are merged.
// grid (split, kv head x pass, slot).  A tile column is (draft row i, query head g of the kv head): column index i * G + g inside
// the slot's (k + 1) * G columns, RT tiles of 16 per pass.  The keys of the slot are [0, n), n = len + k + 1; column (i, .) sees
// keys below len + i + 1 only -- the mask of the draft rows -- and a column that sees no key of a slice keeps (m = -1e30, l = 0).
// A column of an MFMA tile depends on that column's B operand only: what a row gets does not depend on the other columns of
// its tile.  Pad columns are zero and are never written.
// TRUNK (pc_attn_verify_slots_trunk): a slot with shared rows (slot_trunk_rows) takes keys [t0, n) only -- the keys in front of
// them are the trunk launch's --, its wave slices are cut from n - t0 and its partials are records rec0 .. rec0 + nsplit - 1 of
// the nrec records per (row, head).  The mask of the draft rows is unchanged; with t0 = 0 the arithmetic is the plain
// instantiation's.
template <int D, int RT, bool TRUNK = false>
__global__ __launch_bounds__(kThreads, RT > 1 ? 1 : 2) void attn_verify_slots_kernel(
    const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo, int64_t q_ts, const uint64_t* __restrict__ kv_base,
    const int32_t* __restrict__ cap, const int32_t* __restrict__ len, const int32_t* __restrict__ live, int k, int layer, int H,
    int Hkv, float scale_log2, int nsplit, float* __restrict__ part_o, float* __restrict__ part_ml,
    const int32_t* __restrict__ leader = nullptr, const int32_t* __restrict__ trunk = nullptr, int nrec = 0, int rec0 = 0,
    int S = 0) {
    using pca::kTK;
    constexpr int KS = D / 32, DB = D / 16, CPR = D / 8;
    constexpr int LPW = kTK * CPR / 64;              // 16-byte V chunks per lane per tile
    constexpr int kTileHalfs = kTK * D;
    constexpr int kMergeBytes = RT * (4 * DB * 64 * 4 + 4 * 16 * 2) * 4;
    constexpr int kLdsBytes = 4 * kTileHalfs * 2 > kMergeBytes ? 4 * kTileHalfs * 2 : kMergeBytes;
    __shared__ __attribute__((aligned(16))) char smem[kLdsBytes];

    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x, b = blockIdx.z;
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
    const int G = H / Hkv, cols = (k + 1) * G, passes = (cols + 16 * RT - 1) / (16 * RT);
    const int kvh = blockIdx.y / passes, col0 = (blockIdx.y - kvh * passes) * 16 * RT;
    const int past = len[b], cb = cap[b];
    const int nkeys = past + k + 1;                  // (<= cap)

    // this lane's column of each tile: draft row, query head, the keys it may see (0: a pad column)
    int di[RT], gh[RT], lim[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int c = col0 + rt * 16 + n;
        di[rt] = c / G;
        gh[rt] = c - di[rt] * G;
        lim[rt] = c < cols ? past + di[rt] + 1 : 0;
        if (c >= cols) { di[rt] = 0; gh[rt] = 0; }
    }

    int t0 = 0;                                      // first key of this launch
    if constexpr (TRUNK) t0 = slot_trunk_rows(b, S, kv_base, cap, len, leader, trunk);
    int cpw = (nkeys - t0 + nsplit * 4 - 1) / (nsplit * 4);        // keys per wave
    cpw = (cpw + 15) & ~15;
    const int k0 = t0 + (split * 4 + wave) * cpw;
    const int k1 = (k0 + cpw < nkeys) ? k0 + cpw : nkeys;

    h8 qf[RT][KS], qfl[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int64_t off = (int64_t)(b * (k + 1) + di[rt]) * q_ts + (int64_t)(kvh * G + gh[rt]) * D + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            const h8 a = *(const h8*)(q_hi + off + ks * 32), r = *(const h8*)(q_lo + off + ks * 32);
            qf[rt][ks] = lim[rt] == 0 ? z : a;
            qfl[rt][ks] = lim[rt] == 0 ? z : r;
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
    const _Float16* kbase = (const _Float16*)(uintptr_t)kv_base[b] + ((int64_t)(layer * 2) * Hkv + kvh) * cb * D;
    const _Float16* vbase = kbase + (int64_t)Hkv * cb * D;
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
            const int vis = lim[rt] < k1 ? lim[rt] : k1;          // keys of this slice the column sees
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
                    const float s = key < vis ? acc[r] * scale_log2 : -INFINITY;
                    sv[kb][r] = s;
                    mx = fmaxf(mx, s);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run[rt], mx);             // (stays -1e30, finite, while the column has seen no key)
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

    // the four waves' partials through LDS, in wave order: one (O, m, l) record per (row, head, split)
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
        if (lim[rt] != 0) {
            const int64_t rec = ((int64_t)(b * (k + 1) + di[rt]) * H + kvh * G + gh[rt]) * (TRUNK ? nrec : nsplit) +
                                (TRUNK ? rec0 : 0) + split;
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
                    *(f4*)(part_o + rec * D + db * 16 + g * 4) = acc;
                }
            }
            if (wave == 0 && g == 0) { part_ml[rec * 2] = mstar; part_ml[rec * 2 + 1] = lsum; }
        }
    }
}

// ---- shared trunk of the draft rows: the keys a group of slots has in common, read once for all rows of all members ------------
// attn_trunk_slots_kernel (pc_slots.hip) with k + 1 rows per member: grid (trunk split, kv head x pass, candidate leader); a tile
// column is (member m, draft row i, query head g of the kv head), column index (m * (k + 1) + i) * G + g among nmem * (k + 1) * G,
// 16 per MFMA tile, RT tiles per pass.  Members are the RUNNING slots (lookup_slot_runs) of leader gl with slot_trunk_rows > 0, in
// slot order.  No mask: every trunk key lies below T <= len[b] and is visible to every draft row.  The tile loop is the one
// above; the key slices are a function of (T, nsplit_t), every reduction runs in a fixed order and a column of an MFMA tile
// depends on that column's B operand only: what a row gets does not depend on how many members the group has, on the row's
// place in the tile or on the slot index.  Pad columns are zero and are never written.
template <int D, int RT>
__global__ __launch_bounds__(kThreads, RT > 1 ? 1 : 2) void attn_verify_trunk_slots_kernel(
    const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo, int64_t q_ts, const uint64_t* __restrict__ kv_base,
    const int32_t* __restrict__ cap, const int32_t* __restrict__ len, const int32_t* __restrict__ live,
    const int32_t* __restrict__ leader, const int32_t* __restrict__ trunk, int S, int k, int layer, int H, int Hkv,
    float scale_log2, int nsplit_t, int nrec, float* __restrict__ part_o, float* __restrict__ part_ml) {
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
    const int G = H / Hkv, mcols = (k + 1) * G, passes = (S * mcols + 16 * RT - 1) / (16 * RT);
    const int kvh = blockIdx.y / passes, col0 = (blockIdx.y - kvh * passes) * 16 * RT;
    const int T = trunk[gl], cg = cap[gl];
    if (leader[gl] != gl || T <= 0 || T > cg || kv_base[gl] == 0) return;     // (no slot_trunk_rows of this group is non-zero)

    // this lane's column of each tile: member, query head, row of the activations (-1: a pad column)
    int mi[RT], gh[RT], qr[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int c = col0 + rt * 16 + n;
        mi[rt] = c / mcols;
        const int rem = c - mi[rt] * mcols, i = rem / G;
        gh[rt] = rem - i * G;
        qr[rt] = -1 - i;                             // (-1 - draft row until the member's slot is known)
    }
    // the member list, in slot order (S state words, workgroup-uniform)
    int nmem = 0;
    for (int b = 0; b < S; ++b) {
        if (leader[b] != gl || !lookup_slot_runs(cap, len, live, b, k)) continue;
        if (slot_trunk_rows(b, S, kv_base, cap, len, leader, trunk) == 0) continue;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
            if (mi[rt] == nmem) qr[rt] = b * (k + 1) + (-1 - qr[rt]);
        ++nmem;
    }
    if (col0 >= nmem * mcols) return;                // workgroup-uniform: no member, or no column left for this pass
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
        if (qr[rt] < 0) { qr[rt] = -1; gh[rt] = 0; }

    int cpw = (T + nsplit_t * 4 - 1) / (nsplit_t * 4);             // keys per wave
    cpw = (cpw + 15) & ~15;
    const int k0 = (split * 4 + wave) * cpw;
    const int k1 = (k0 + cpw < T) ? k0 + cpw : T;

    h8 qf[RT][KS], qfl[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int64_t off = (int64_t)(qr[rt] < 0 ? 0 : qr[rt]) * q_ts + (int64_t)(kvh * G + gh[rt]) * D + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            const h8 a = *(const h8*)(q_hi + off + ks * 32), r = *(const h8*)(q_lo + off + ks * 32);
            qf[rt][ks] = qr[rt] < 0 ? z : a;
            qfl[rt][ks] = qr[rt] < 0 ? z : r;
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

    // the four waves' partials through LDS, in wave order: one (O, m, l) record per (row, head, trunk split)
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
        if (qr[rt] >= 0) {
            const int64_t rec = ((int64_t)qr[rt] * H + kvh * G + gh[rt]) * nrec + split;
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
                    *(f4*)(part_o + rec * D + db * 16 + g * 4) = acc;
                }
            }
            if (wave == 0 && g == 0) { part_ml[rec * 2] = mstar; part_ml[rec * 2 + 1] = lsum; }
        }
    }
}

// merge of the split partials, one workgroup per (head, row), one thread per head dim, splits in index (= key) order
template <int D>
__global__ __launch_bounds__(D) void attn_merge_verify_slots_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                    const int32_t* __restrict__ cap, const int32_t* __restrict__ len,
                                                                    const int32_t* __restrict__ live, int k, int H, int nsplit,
                                                                    _Float16* __restrict__ of_hi, _Float16* __restrict__ of_lo) {
    const int h = blockIdx.x, r = blockIdx.y, d = threadIdx.x;
    if (!lookup_slot_runs(cap, len, live, r / (k + 1), k)) return;
    const int64_t base = ((int64_t)r * H + h) * nsplit;
    float ms = kNegBig;
    for (int s = 0; s < nsplit; ++s) ms = fmaxf(ms, part_ml[(base + s) * 2]);
    float num = 0.0f, den = 0.0f;
    for (int s = 0; s < nsplit; ++s) {
        const float wt = exp2f(part_ml[(base + s) * 2] - ms);
        den = fmaf(wt, part_ml[(base + s) * 2 + 1], den);
        num = fmaf(wt, part_o[(base + s) * D + d], num);
    }
    _Float16 hi, lo;
    pc_split(num / den, hi, lo);                              // (den > 0: every row sees key 0)
    const int64_t off = pca::frag_off(r, h * D + d, H * D / 32);
    of_hi[off] = hi;
    of_lo[off] = lo;
}

// merge of the trunk + own records of a (row, head), in key order; a row of a slot on its own has no trunk records
template <int D>
__global__ __launch_bounds__(D) void attn_merge_verify_slots_trunk_kernel(
    const float* __restrict__ part_o, const float* __restrict__ part_ml, const int32_t* __restrict__ cap,
    const int32_t* __restrict__ len, const int32_t* __restrict__ live, const int32_t* __restrict__ leader,
    const int32_t* __restrict__ trunk, const uint64_t* __restrict__ kv_base, int S, int k, int H, int nsplit_t, int nrec,
    _Float16* __restrict__ of_hi, _Float16* __restrict__ of_lo) {
    const int h = blockIdx.x, r = blockIdx.y, d = threadIdx.x;
    const int b = r / (k + 1);
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
    const int64_t base = ((int64_t)r * H + h) * nrec;
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
    pc_split(num / den, hi, lo);                              // (den > 0: every row sees its own key len + i)
    const int64_t off = pca::frag_off(r, h * D + d, H * D / 32);
    of_hi[off] = hi;
    of_lo[off] = lo;
}

template <int D>
void launch_verify(int S, int k, int H, int Hkv, int nsplit, hipStream_t st, const _Float16* q_hi, const _Float16* q_lo, int64_t q_ts,
                   const uint64_t* kv_base, const int32_t* cap, const int32_t* len, const int32_t* live, int layer, float scale_log2,
                   float* part_o, float* part_ml, _Float16* of_hi, _Float16* of_lo) {
    const int cols = (k + 1) * (H / Hkv);
    if (cols <= 16)
        hipLaunchKernelGGL((attn_verify_slots_kernel<D, 1>), dim3(nsplit, Hkv, S), dim3(kThreads), 0, st, q_hi, q_lo, q_ts, kv_base, cap,
                           len, live, k, layer, H, Hkv, scale_log2, nsplit, part_o, part_ml);
    else
        hipLaunchKernelGGL((attn_verify_slots_kernel<D, 2>), dim3(nsplit, Hkv * ((cols + 31) / 32), S), dim3(kThreads), 0, st, q_hi, q_lo,
                           q_ts, kv_base, cap, len, live, k, layer, H, Hkv, scale_log2, nsplit, part_o, part_ml);
    hipLaunchKernelGGL(attn_merge_verify_slots_kernel<D>, dim3(H, S * (k + 1)), dim3(D), 0, st, part_o, part_ml, cap, len, live, k, H,
                       nsplit, of_hi, of_lo);
}

struct VerifyTrunkArgs {
    const _Float16 *q_hi, *q_lo; int64_t q_ts;
    const uint64_t* kv_base; const int32_t *cap, *len, *live, *leader, *trunk;
    int S, k, layer, H, Hkv; float scale_log2; int ns_own, ns_trunk; float *part_o, *part_ml; _Float16 *of_hi, *of_lo;
};

// trunk launch (RT = 2 where the S slots can fill more than one tile: it halves the passes over the trunk), own launch (RT as
// launch_verify picks it), merge
template <int D>
void launch_verify_trunk(const VerifyTrunkArgs& a, hipStream_t st) {
    const int cols = (a.k + 1) * (a.H / a.Hkv), nrec = a.ns_trunk + a.ns_own;
    if (a.S * cols <= 16)
        hipLaunchKernelGGL((attn_verify_trunk_slots_kernel<D, 1>), dim3(a.ns_trunk, a.Hkv, a.S), dim3(kThreads), 0, st, a.q_hi, a.q_lo,
                           a.q_ts, a.kv_base, a.cap, a.len, a.live, a.leader, a.trunk, a.S, a.k, a.layer, a.H, a.Hkv, a.scale_log2,
                           a.ns_trunk, nrec, a.part_o, a.part_ml);
    else
        hipLaunchKernelGGL((attn_verify_trunk_slots_kernel<D, 2>), dim3(a.ns_trunk, a.Hkv * ((a.S * cols + 31) / 32), a.S),
                           dim3(kThreads), 0, st, a.q_hi, a.q_lo, a.q_ts, a.kv_base, a.cap, a.len, a.live, a.leader, a.trunk, a.S, a.k,
                           a.layer, a.H, a.Hkv, a.scale_log2, a.ns_trunk, nrec, a.part_o, a.part_ml);
    if (cols <= 16)
        hipLaunchKernelGGL((attn_verify_slots_kernel<D, 1, true>), dim3(a.ns_own, a.Hkv, a.S), dim3(kThreads), 0, st, a.q_hi, a.q_lo,
                           a.q_ts, a.kv_base, a.cap, a.len, a.live, a.k, a.layer, a.H, a.Hkv, a.scale_log2, a.ns_own, a.part_o, a.part_ml,
                           a.leader, a.trunk, nrec, a.ns_trunk, a.S);
    else
        hipLaunchKernelGGL((attn_verify_slots_kernel<D, 2, true>), dim3(a.ns_own, a.Hkv * ((cols + 31) / 32), a.S), dim3(kThreads), 0,
                           st, a.q_hi, a.q_lo, a.q_ts, a.kv_base, a.cap, a.len, a.live, a.k, a.layer, a.H, a.Hkv, a.scale_log2, a.ns_own,
                           a.part_o, a.part_ml, a.leader, a.trunk, nrec, a.ns_trunk, a.S);
    hipLaunchKernelGGL(attn_merge_verify_slots_trunk_kernel<D>, dim3(a.H, a.S * (a.k + 1)), dim3(D), 0, st, a.part_o, a.part_ml, a.cap,
                       a.len, a.live, a.leader, a.trunk, a.kv_base, a.S, a.k, a.H, a.ns_trunk, nrec, a.of_hi, a.of_lo);
}

bool rows_shape_ok(int S, int k) { return S >= 1 && S <= 16 && k >= 0 && k <= 15 && S * (k + 1) <= kMaxRows; }

}  // namespace

PC_EXPORT int pc_rope_append_slots_rows(const float* qkv, int64_t ld, int32_t in_layout, void* q_hi, void* q_lo,
                                        int64_t q_token_stride, const float* cs, const uint64_t* kv_base, const int32_t* cap,
                                        const int32_t* len, const int32_t* live, int32_t S, int32_t k, int32_t layer, int32_t H,
                                        int32_t Hkv, int32_t D, void* stream) {
    PC_REQUIRE(rows_shape_ok(S, k) && layer >= 0 && H > 0 && Hkv > 0, PC_ERR_ARG,
               "pc_rope_append_slots_rows: bad sizes (1 <= S <= 16, 0 <= k <= 15, S * (k + 1) <= 64)");
    PC_REQUIRE(D > 0 && D % 16 == 0, PC_ERR_ARG, "pc_rope_append_slots_rows: head_dim must be a multiple of 16");
    PC_REQUIRE(qkv && q_hi && q_lo && cs && kv_base && cap && len && live, PC_ERR_ARG, "pc_rope_append_slots_rows: null pointer");
    PC_REQUIRE(in_layout == 0 || in_layout == 1, PC_ERR_ARG,
               "pc_rope_append_slots_rows: in_layout is 0 (natural) or 1 (rotary-pair tiles)");
    PC_REQUIRE(ld >= (int64_t)(H + 2 * Hkv) * D && ld % 4 == 0 && q_token_stride % 8 == 0 && ((uintptr_t)qkv & 15) == 0 &&
                   ((uintptr_t)q_hi & 15) == 0 && ((uintptr_t)q_lo & 15) == 0,
               PC_ERR_ARG, "pc_rope_append_slots_rows: rows must keep 16-byte alignment");
    hipLaunchKernelGGL(rope_append_slots_rows_kernel, dim3(k + 1, S), dim3(kThreads), 0, (hipStream_t)stream, qkv, ld, in_layout,
                       (_Float16*)q_hi, (_Float16*)q_lo, q_token_stride, (const float2*)cs, kv_base, cap, len, live, k, layer, H, Hkv, D);
    return pc_check_launch("rope_append_slots_rows_kernel");
}

PC_EXPORT int64_t pc_attn_verify_slots_workspace_bytes(int32_t S, int32_t k, int32_t H, int32_t D, int32_t nsplit) {
    if (S < 1 || k < 0 || H < 1 || D < 1 || nsplit < 1) return 0;
    return (int64_t)S * (k + 1) * H * nsplit * (D + 2) * (int64_t)sizeof(float);
}

PC_EXPORT int pc_attn_verify_slots(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                   const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t k, int32_t layer,
                                   int32_t H, int32_t Hkv, int32_t D, float softmax_scale, int32_t nsplit, void* workspace,
                                   int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, void* stream) {
    PC_REQUIRE(rows_shape_ok(S, k) && layer >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && (D == 64 || D == 128), PC_ERR_ARG,
               "pc_attn_verify_slots: 1 <= S <= 16, 0 <= k <= 15, S * (k + 1) <= 64, H a multiple of Hkv, head_dim 64 or 128");
    PC_REQUIRE(nsplit >= 1 && nsplit <= kMaxSplit, PC_ERR_ARG, "pc_attn_verify_slots: nsplit must be in [1, 32]");
    PC_REQUIRE(q_hi && q_lo && kv_base && cap && len && live && workspace && out_frag_hi && out_frag_lo, PC_ERR_ARG,
               "pc_attn_verify_slots: null pointer");
    PC_REQUIRE(q_token_stride % 8 == 0 && q_token_stride >= (int64_t)H * D && ((uintptr_t)q_hi & 15) == 0 && ((uintptr_t)q_lo & 15) == 0 &&
                   (H * D) % 32 == 0, PC_ERR_ARG,
               "pc_attn_verify_slots: q rows must keep 16-byte alignment and H * head_dim be a multiple of 32");
    PC_REQUIRE(workspace_bytes >= pc_attn_verify_slots_workspace_bytes(S, k, H, D, nsplit) && ((uintptr_t)workspace & 15) == 0, PC_ERR_ARG,
               "pc_attn_verify_slots: workspace too small (pc_attn_verify_slots_workspace_bytes) or misaligned");
    float* part_o = (float*)workspace;
    float* part_ml = part_o + (int64_t)S * (k + 1) * H * nsplit * D;
    const float scale_log2 = softmax_scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    if (D == 128)
        launch_verify<128>(S, k, H, Hkv, nsplit, st, (const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len, live,
                           layer, scale_log2, part_o, part_ml, (_Float16*)out_frag_hi, (_Float16*)out_frag_lo);
    else
        launch_verify<64>(S, k, H, Hkv, nsplit, st, (const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len, live,
                          layer, scale_log2, part_o, part_ml, (_Float16*)out_frag_hi, (_Float16*)out_frag_lo);
    return pc_check_launch("attn_verify_slots_kernel");
}

PC_EXPORT int64_t pc_attn_verify_slots_trunk_workspace_bytes(int32_t S, int32_t k, int32_t H, int32_t D, int32_t nsplit_own,
                                                             int32_t nsplit_trunk) {
    if (S < 1 || k < 0 || H < 1 || D < 1 || nsplit_own < 1 || nsplit_trunk < 1) return 0;
    return (int64_t)S * (k + 1) * H * (nsplit_own + nsplit_trunk) * (D + 2) * (int64_t)sizeof(float);
}

PC_EXPORT int pc_attn_verify_slots_trunk(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                         const int32_t* cap, const int32_t* len, const int32_t* live, const int32_t* leader,
                                         const int32_t* trunk, int32_t S, int32_t k, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                                         float softmax_scale, int32_t nsplit_own, int32_t nsplit_trunk, void* workspace,
                                         int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, void* stream) {
    PC_REQUIRE(rows_shape_ok(S, k) && layer >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && (D == 64 || D == 128), PC_ERR_ARG,
               "pc_attn_verify_slots_trunk: 1 <= S <= 16, 0 <= k <= 15, S * (k + 1) <= 64, H a multiple of Hkv, head_dim 64 or 128");
    PC_REQUIRE(nsplit_own >= 1 && nsplit_own <= kMaxSplit && nsplit_trunk >= 1 && nsplit_trunk <= kMaxSplit, PC_ERR_ARG,
               "pc_attn_verify_slots_trunk: nsplit_own and nsplit_trunk must be in [1, 32]");
    PC_REQUIRE(q_hi && q_lo && kv_base && cap && len && live && leader && trunk && workspace && out_frag_hi && out_frag_lo, PC_ERR_ARG,
               "pc_attn_verify_slots_trunk: null pointer");
    PC_REQUIRE(q_token_stride % 8 == 0 && q_token_stride >= (int64_t)H * D && ((uintptr_t)q_hi & 15) == 0 && ((uintptr_t)q_lo & 15) == 0 &&
                   (H * D) % 32 == 0, PC_ERR_ARG,
               "pc_attn_verify_slots_trunk: q rows must keep 16-byte alignment and H * head_dim be a multiple of 32");
    PC_REQUIRE(workspace_bytes >= pc_attn_verify_slots_trunk_workspace_bytes(S, k, H, D, nsplit_own, nsplit_trunk) &&
                   ((uintptr_t)workspace & 15) == 0,
               PC_ERR_ARG, "pc_attn_verify_slots_trunk: workspace too small (pc_attn_verify_slots_trunk_workspace_bytes) or misaligned");
    VerifyTrunkArgs a;
    a.q_hi = (const _Float16*)q_hi; a.q_lo = (const _Float16*)q_lo; a.q_ts = q_token_stride;
    a.kv_base = kv_base; a.cap = cap; a.len = len; a.live = live; a.leader = leader; a.trunk = trunk;
    a.S = S; a.k = k; a.layer = layer; a.H = H; a.Hkv = Hkv; a.scale_log2 = softmax_scale * 1.4426950408889634f;
    a.ns_own = nsplit_own; a.ns_trunk = nsplit_trunk;
    a.part_o = (float*)workspace;
    a.part_ml = a.part_o + (int64_t)S * (k + 1) * H * (nsplit_own + nsplit_trunk) * D;
    a.of_hi = (_Float16*)out_frag_hi; a.of_lo = (_Float16*)out_frag_lo;
    if (D == 128) launch_verify_trunk<128>(a, (hipStream_t)stream);
    else launch_verify_trunk<64>(a, (hipStream_t)stream);
    return pc_check_launch("attn_verify_trunk_slots_kernel");
}
