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
//
// The one-row step over slots (pc_slots.hip) is this step at k = 0: its RoPE + append, its shared-trunk attention and its merges
// are the kernels here, reached through the launchers of pc_attn_rows.h, where the MFMA tile loop of the attention kernels lives.
#include <hip/hip_fp16.h>
#include <math.h>

#include "pc_attn_rows.h"

namespace {

using pca::kMaxSplit;
using pca::kThreads;
using pcr::h8;
using pcr::load8;
using pcr::SlotAttnArgs;

constexpr int kMaxRows = 64;          // S * (k + 1)

// ---- RoPE + append, one workgroup per (draft row, slot) ----------------------------------------------------------------
// The work items and the arithmetic are rope_append_kernel<float>'s (pc_rope.hip): the rows written are bit-identical to what
// pc_rope_append_ex writes for the same projection row and position.  Row r of the projection, rotated with row r of the table,
// q to row r of the pair, K / V to arena row len + i.  layout 1: the projection row is in the row order of the q|k|v fragment
// image (_native.qkv_rope_row_perm: inside a head, 16-column tile j = features 8j.. then D/2 + 8j..).
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
            pcr::rope_pairs8(lo, hi, csr + ch * 8, olo, ohi, rlo, rhi);
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
// The tile loop is pcr::attn_rows_tiles (pc_attn_rows.h); every WAVE owns a contiguous slice of the split's keys.
// grid (split, kv head x pass, slot).  A tile column is (draft row i, query head g of the kv head): column index i * G + g inside
// the slot's (k + 1) * G columns, RT tiles of 16 per pass.  The keys of the slot are [0, n), n = len + k + 1; column (i, .) sees
// keys below len + i + 1 only -- the mask of the draft rows -- and a column that sees no key of a slice keeps (m = -1e30, l = 0).
// leader != nullptr (pc_attn_verify_slots_trunk; uniform over the launch -- an argument, not a template flag: the library's
// instantiation budget, tests/test_kernel_resources.py, is spent on the kernels of pc_attn_decode_slots_trunk_q8): a slot with
// shared rows (slot_trunk_rows) takes keys [t0, n) only -- the keys in front of them are the trunk launch's --, its wave slices
// are cut from n - t0 and its partials are records rec0 .. rec0 + nsplit - 1 of the nrec records per (row, head).  The mask of
// the draft rows is unchanged; with t0 = 0 the arithmetic is the plain launch's (nrec = nsplit, rec0 = 0, null words).
template <int D, int RT>
__global__ __launch_bounds__(kThreads, RT > 1 ? 1 : 2) void attn_verify_slots_kernel(
    const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo, int64_t q_ts, const uint64_t* __restrict__ kv_base,
    const int32_t* __restrict__ cap, const int32_t* __restrict__ len, const int32_t* __restrict__ live, int k, int layer, int H,
    int Hkv, float scale_log2, int nsplit, float* __restrict__ part_o, float* __restrict__ part_ml,
    const int32_t* __restrict__ leader, const int32_t* __restrict__ trunk, int nrec, int rec0, int S) {
    __shared__ __attribute__((aligned(16))) char smem[pcr::rows_lds_bytes<D, RT>()];
    const int n = threadIdx.x & 15, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int split = blockIdx.x, b = blockIdx.z;
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
    const int G = H / Hkv, cols = (k + 1) * G, passes = (cols + 16 * RT - 1) / (16 * RT);
    const int kvh = blockIdx.y / passes, col0 = (blockIdx.y - kvh * passes) * 16 * RT;
    const int past = len[b], cb = cap[b];
    const int nkeys = past + k + 1;                  // (<= cap)

    // this lane's column of each tile: its q row, the keys it may see, its record of this split (a pad column: row 0, head 0)
    int64_t qoff[RT], rec[RT];
    bool pad[RT];
    int lim[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int c = col0 + rt * 16 + n;
        pad[rt] = c >= cols;
        const int di = pad[rt] ? 0 : c / G, gh = pad[rt] ? 0 : c - di * G;
        lim[rt] = pad[rt] ? 0 : past + di + 1;
        qoff[rt] = (int64_t)(b * (k + 1) + di) * q_ts + (int64_t)(kvh * G + gh) * D;
        rec[rt] = ((int64_t)(b * (k + 1) + di) * H + kvh * G + gh) * nrec + rec0 + split;
    }

    int t0 = 0;                                      // first key of this launch
    if (leader != nullptr) t0 = slot_trunk_rows(b, S, kv_base, cap, len, leader, trunk);
    int cpw = (nkeys - t0 + nsplit * 4 - 1) / (nsplit * 4);        // keys per wave
    cpw = (cpw + 15) & ~15;
    const int k0 = t0 + (split * 4 + wave) * cpw;
    const int k1 = (k0 + cpw < nkeys) ? k0 + cpw : nkeys;

    const _Float16* kbase = (const _Float16*)(uintptr_t)kv_base[b] + ((int64_t)(layer * 2) * Hkv + kvh) * cb * D;
    pcr::attn_rows_tiles<D, RT, true>(q_hi, q_lo, qoff, pad, lim, rec, kbase, kbase + (int64_t)Hkv * cb * D, k0, k1, scale_log2, smem,
                                      part_o, part_ml);
}

// ---- shared trunk of the draft rows: the keys a group of slots has in common, read once for all rows of all members ------------
// Slots that staged the same leading module rows (leader[b] = gl, trunk[b] = T) hold the same bytes in rows [0, T) of their
// arenas.  This launch reads those rows from the leader's arena only and multiplies them with the query rows of ALL members.
// It serves pc_attn_decode_slots_trunk at k = 0.  grid (trunk split, kv head x pass, candidate leader), S * (k + 1) * G columns
// cut into passes; a tile column is (member m, draft row i, query head g of the kv head), column index (m * (k + 1) + i) * G + g
// among nmem * (k + 1) * G, 16 per MFMA tile, RT tiles per pass.  Members are the RUNNING slots (lookup_slot_runs) of leader gl
// with slot_trunk_rows > 0, in slot order.  No mask: every trunk key lies below T <= len[b] and is visible to every draft row.
// The tile loop is pcr::attn_rows_tiles; the key slices are a function of (T, nsplit_t), every reduction runs in a fixed order and
// a column of an MFMA tile depends on that column's B operand only: what a row gets does not depend on how many members the group
// has, on the row's place in the tile or on the slot index.  Pad columns are zero and are never written.
template <int D, int RT>
__global__ __launch_bounds__(kThreads, RT > 1 ? 1 : 2) void attn_verify_trunk_slots_kernel(
    const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo, int64_t q_ts, const uint64_t* __restrict__ kv_base,
    const int32_t* __restrict__ cap, const int32_t* __restrict__ len, const int32_t* __restrict__ live,
    const int32_t* __restrict__ leader, const int32_t* __restrict__ trunk, int S, int k, int layer, int H, int Hkv,
    float scale_log2, int nsplit_t, int nrec, float* __restrict__ part_o, float* __restrict__ part_ml) {
    __shared__ __attribute__((aligned(16))) char smem[pcr::rows_lds_bytes<D, RT>()];
    const int n = threadIdx.x & 15, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int split = blockIdx.x, gl = blockIdx.z;
    const int G = H / Hkv, mcols = (k + 1) * G, passes = (S * mcols + 16 * RT - 1) / (16 * RT);
    const int kvh = blockIdx.y / passes, col0 = (blockIdx.y - kvh * passes) * 16 * RT;
    const int T = trunk[gl], cg = cap[gl];
    if (leader[gl] != gl || T <= 0 || T > cg || kv_base[gl] == 0) return;     // (no slot_trunk_rows of this group is non-zero)

    // this lane's column of each tile: member, query head, row of the activations (negative: a pad column)
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

    int cpw = (T + nsplit_t * 4 - 1) / (nsplit_t * 4);             // keys per wave
    cpw = (cpw + 15) & ~15;
    const int k0 = (split * 4 + wave) * cpw;
    const int k1 = (k0 + cpw < T) ? k0 + cpw : T;

    int64_t qoff[RT], rec[RT];
    bool pad[RT];
    int lim[RT];                                     // (no mask)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        pad[rt] = qr[rt] < 0;
        const int row = pad[rt] ? 0 : qr[rt], head = kvh * G + (pad[rt] ? 0 : gh[rt]);
        lim[rt] = 0;
        qoff[rt] = (int64_t)row * q_ts + (int64_t)head * D;
        rec[rt] = ((int64_t)row * H + head) * nrec + split;
    }
    const _Float16* kbase = (const _Float16*)(uintptr_t)kv_base[gl] + ((int64_t)(layer * 2) * Hkv + kvh) * cg * D;
    pcr::attn_rows_tiles<D, RT, false>(q_hi, q_lo, qoff, pad, lim, rec, kbase, kbase + (int64_t)Hkv * cg * D, k0, k1, scale_log2, smem,
                                       part_o, part_ml);
}

// own launch of a slot's rows (RT = 2 where its (k + 1) * G columns fill more than one tile); a plain entry's leader / trunk words
// are null and its ns_trunk 0: nrec = ns_own, rec0 = 0
template <int D>
void launch_verify_own(const SlotAttnArgs& a, hipStream_t st) {
    const int cols = (a.k + 1) * (a.H / a.Hkv), nrec = a.ns_trunk + a.ns_own;
    if (cols <= 16)
        hipLaunchKernelGGL((attn_verify_slots_kernel<D, 1>), dim3(a.ns_own, a.Hkv, a.S), dim3(kThreads), 0, st, a.q_hi, a.q_lo,
                           a.q_ts, a.kv_base, a.cap, a.len, a.live, a.k, a.layer, a.H, a.Hkv, a.scale_log2, a.ns_own, a.part_o, a.part_ml,
                           a.leader, a.trunk, nrec, a.ns_trunk, a.S);
    else
        hipLaunchKernelGGL((attn_verify_slots_kernel<D, 2>), dim3(a.ns_own, a.Hkv * ((cols + 31) / 32), a.S), dim3(kThreads), 0,
                           st, a.q_hi, a.q_lo, a.q_ts, a.kv_base, a.cap, a.len, a.live, a.k, a.layer, a.H, a.Hkv, a.scale_log2, a.ns_own,
                           a.part_o, a.part_ml, a.leader, a.trunk, nrec, a.ns_trunk, a.S);
}

// grid.y follows the kernel's own pass count, ceil(S * (k + 1) * G / (16 * RT))
template <int D, int RT>
void launch_trunk(const SlotAttnArgs& a, hipStream_t st) {
    const int passes = pc_ceil_div(a.S * (a.k + 1) * (a.H / a.Hkv), 16 * RT);
    hipLaunchKernelGGL((attn_verify_trunk_slots_kernel<D, RT>), dim3(a.ns_trunk, a.Hkv * passes, a.S), dim3(kThreads), 0, st, a.q_hi,
                       a.q_lo, a.q_ts, a.kv_base, a.cap, a.len, a.live, a.leader, a.trunk, a.S, a.k, a.layer, a.H, a.Hkv, a.scale_log2,
                       a.ns_trunk, a.ns_trunk + a.ns_own, a.part_o, a.part_ml);
}

// (trunk: whether the merge skips the trunk records of a slot on its own -- said by the leader words, null without)
template <int D>
void launch_merge(const SlotAttnArgs& a, bool trunk, hipStream_t st) {
    hipLaunchKernelGGL((pcr::attn_merge_slots_kernel<D>), dim3(a.H, a.S * (a.k + 1)), dim3(D), 0, st, a.part_o, a.part_ml, a.cap,
                       a.len, a.live, trunk ? a.leader : nullptr, a.trunk, a.kv_base, a.S, a.k, a.H, a.ns_trunk,
                       a.ns_trunk + a.ns_own + a.ns_extra, a.of_hi, a.of_lo, trunk ? a.kvq_base : nullptr, a.qcap);
}

bool rows_shape_ok(int S, int k) { return S >= 1 && S <= 16 && k >= 0 && k <= 15 && S * (k + 1) <= kMaxRows; }

}  // namespace

namespace pcr {

int slot_attn_prepare(const char* name, bool rows, bool trunk, int ws_align, SlotAttnArgs& a, int D, float softmax_scale,
                      void* workspace, int64_t workspace_bytes) {
    PC_REQUIRE(rows_shape_ok(a.S, a.k) && a.layer >= 0 && a.H > 0 && a.Hkv > 0 && a.H % a.Hkv == 0 && (D == 64 || D == 128), PC_ERR_ARG,
               "%s: 1 <= S <= 16%s, H a multiple of Hkv, head_dim 64 or 128", name, rows ? ", 0 <= k <= 15, S * (k + 1) <= 64" : "");
    PC_REQUIRE(a.ns_own >= 1 && a.ns_own <= kMaxSplit && (!trunk || (a.ns_trunk >= 1 && a.ns_trunk <= kMaxSplit)), PC_ERR_ARG,
               "%s: %s must be in [1, 32]", name, trunk ? "nsplit_own and nsplit_trunk" : "nsplit");
    PC_REQUIRE(a.q_hi && a.q_lo && a.kv_base && a.cap && a.len && a.live && (!trunk || (a.leader && a.trunk)) && workspace && a.of_hi &&
                   a.of_lo, PC_ERR_ARG, "%s: null pointer", name);
    PC_REQUIRE(a.q_ts % 8 == 0 && (!rows || a.q_ts >= (int64_t)a.H * D) && ((uintptr_t)a.q_hi & 15) == 0 && ((uintptr_t)a.q_lo & 15) == 0 &&
                   (a.H * D) % 32 == 0, PC_ERR_ARG,
               "%s: q rows must keep 16-byte alignment and H * head_dim be a multiple of 32", name);
    // (what <name>_workspace_bytes counts; ns_extra: pc_attn_verify_slots_q8's exact-key record)
    const int64_t nrec = (int64_t)a.S * (a.k + 1) * a.H * (a.ns_own + a.ns_trunk + a.ns_extra);
    PC_REQUIRE(workspace_bytes >= nrec * (D + 2) * (int64_t)sizeof(float) && ((uintptr_t)workspace & (ws_align - 1)) == 0, PC_ERR_ARG,
               "%s: workspace too small (%s_workspace_bytes) or misaligned", name, name);
    a.scale_log2 = softmax_scale * 1.4426950408889634f;
    a.part_o = (float*)workspace;
    a.part_ml = a.part_o + nrec * D;
    return PC_OK;
}

void launch_attn_trunk_slots(const SlotAttnArgs& a, int D, int RT, hipStream_t st) {
    if (D == 128) RT > 1 ? launch_trunk<128, 2>(a, st) : launch_trunk<128, 1>(a, st);
    else RT > 1 ? launch_trunk<64, 2>(a, st) : launch_trunk<64, 1>(a, st);
}

void launch_attn_merge_slots(const SlotAttnArgs& a, int D, bool trunk, hipStream_t st) {
    if (D == 128) launch_merge<128>(a, trunk, st);
    else launch_merge<64>(a, trunk, st);
}

void launch_rope_append_slots_rows(const float* qkv, int64_t ld, int layout, _Float16* q_hi, _Float16* q_lo, int64_t q_ts,
                                   const float2* cs, const uint64_t* kv_base, const int32_t* cap, const int32_t* len,
                                   const int32_t* live, int S, int k, int layer, int H, int Hkv, int D, hipStream_t st) {
    hipLaunchKernelGGL(rope_append_slots_rows_kernel, dim3(k + 1, S), dim3(kThreads), 0, st, qkv, ld, layout, q_hi, q_lo, q_ts, cs, kv_base,
                       cap, len, live, k, layer, H, Hkv, D);
}

}  // namespace pcr

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
    pcr::launch_rope_append_slots_rows(qkv, ld, in_layout, (_Float16*)q_hi, (_Float16*)q_lo, q_token_stride, (const float2*)cs, kv_base,
                                       cap, len, live, S, k, layer, H, Hkv, D, (hipStream_t)stream);
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
    SlotAttnArgs a = {(const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len, live, nullptr, nullptr,
                      S, k, layer, H, Hkv, 0.f, nsplit, 0, nullptr, nullptr, (_Float16*)out_frag_hi, (_Float16*)out_frag_lo};
    if (const int rc = pcr::slot_attn_prepare("pc_attn_verify_slots", true, false, 16, a, D, softmax_scale, workspace, workspace_bytes))
        return rc;
    if (D == 128) launch_verify_own<128>(a, (hipStream_t)stream);
    else launch_verify_own<64>(a, (hipStream_t)stream);
    pcr::launch_attn_merge_slots(a, D, false, (hipStream_t)stream);
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
    SlotAttnArgs a = {(const _Float16*)q_hi, (const _Float16*)q_lo, q_token_stride, kv_base, cap, len, live, leader, trunk,
                      S, k, layer, H, Hkv, 0.f, nsplit_own, nsplit_trunk, nullptr, nullptr, (_Float16*)out_frag_hi, (_Float16*)out_frag_lo};
    if (const int rc = pcr::slot_attn_prepare("pc_attn_verify_slots_trunk", true, true, 16, a, D, softmax_scale, workspace, workspace_bytes))
        return rc;
    // trunk launch (RT = 2 where the S slots can fill more than one tile: it halves the passes over the trunk), own launch, merge
    hipStream_t st = (hipStream_t)stream;
    pcr::launch_attn_trunk_slots(a, D, S * (k + 1) * (H / Hkv) <= 16 ? 1 : 2, st);
    if (D == 128) launch_verify_own<128>(a, st);
    else launch_verify_own<64>(a, st);
    pcr::launch_attn_merge_slots(a, D, true, st);
    return pc_check_launch("attn_verify_trunk_slots_kernel");
}
