// Shared by the slot attention units (pc_slots.hip, pc_lookup_slots.hip): the MFMA tile loop over a wave's key slice with the
// four-wave merge behind it, the merge of a row's split records, and the host side the four attention entries have in common.
// The kernels built from this header are compiled in pc_lookup_slots.hip alone; pc_slots.hip reaches them through the launchers
// declared here.
#pragma once
#include <hip/hip_fp16.h>
#include <math.h>

#include "pc_attn_common.h"
#include "pc_lookup_common.h"

namespace pcr {

using pca::f4;
using pca::h8;

// ---- host side ---------------------------------------------------------------------------------------------------------------
// One description for pc_attn_decode_slots[_trunk] (k = 0) and pc_attn_verify_slots[_trunk]: row b * (k + 1) + i of the q pair is
// draft row i of slot b, a (row, head) has ns_trunk + ns_own + ns_extra records -- the trunk launch's first -- and the plain
// entries have no leader / trunk words and ns_trunk = 0.
struct SlotAttnArgs {
    const _Float16 *q_hi, *q_lo; int64_t q_ts;
    const uint64_t* kv_base; const int32_t *cap, *len, *live, *leader, *trunk;
    int S, k, layer, H, Hkv; float scale_log2; int ns_own, ns_trunk; float *part_o, *part_ml; _Float16 *of_hi, *of_lo;
    int ns_extra;                    // records behind the own ones that the entry's own kernel writes (pc_attn_verify_slots_q8: 1)
    const uint64_t* kvq_base; int qcap;   // pc_attn_decode_slots_trunk_q8: the images, whose predicate (slot_trunk_rows_q8) the merge asks
};

// The argument checks of the four entries, messages prefixed with the entry's `name`, and the split of the workspace into
// a.part_o / a.part_ml.  rows: an entry with k + 1 rows per slot, which needs q_token_stride >= H * D.
int slot_attn_prepare(const char* name, bool rows, bool trunk, int ws_align, SlotAttnArgs& a, int D, float softmax_scale,
                      void* workspace, int64_t workspace_bytes);
// attn_verify_trunk_slots_kernel<D, RT>: the shared rows of every group, once for all rows of all members
void launch_attn_trunk_slots(const SlotAttnArgs& a, int D, int RT, hipStream_t st);
// attn_merge_slots_kernel<D> (trunk: the launch passes the leader / trunk words, otherwise null)
void launch_attn_merge_slots(const SlotAttnArgs& a, int D, bool trunk, hipStream_t st);
// rope_append_slots_rows_kernel, grid (k + 1, S)
void launch_rope_append_slots_rows(const float* qkv, int64_t ld, int layout, _Float16* q_hi, _Float16* q_lo, int64_t q_ts,
                                   const float2* cs, const uint64_t* kv_base, const int32_t* cap, const int32_t* len,
                                   const int32_t* live, int S, int k, int layer, int H, int Hkv, int D, hipStream_t st);

// ---- device side -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load8(const float* p, float (&x)[8]) {
    const f4 a = *(const f4*)p, b = *(const f4*)(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[e] = a[e]; x[e + 4] = b[e]; }
}

// RoPE on the 8 rotary pairs (lo[e], hi[e]) of one work item of rope_append_kernel<float> (pc_rope.hip) with the table entries
// w8[e] = (cos, sin): the rotated pair as split-precision halves, (olo, rlo) = hi / lo of the first member, (ohi, rhi) of the second.
// Once for the kernels that append a slot's row (rope_append_slots_rows_kernel, rope_append_slots_q8_kernel).
__device__ __forceinline__ void rope_pairs8(const float (&lo)[8], const float (&hi)[8], const float2* __restrict__ w8, h8& olo, h8& ohi,
                                            h8& rlo, h8& rhi) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float2 w = w8[e];
        const float a = lo[e] * w.x - hi[e] * w.y, b2 = hi[e] * w.x + lo[e] * w.y;
        _Float16 t0, t1, t2, t3;
        pc_split(a, t0, t1);
        pc_split(b2, t2, t3);
        olo[e] = t0; rlo[e] = t1;
        ohi[e] = t2; rhi[e] = t3;
    }
}

// LDS of a kernel that calls attn_rows_tiles: four wave-private V tiles, reused for the four waves' partials
template <int D, int RT>
constexpr int rows_lds_bytes() {
    constexpr int tiles = 4 * pca::kTK * D * 2, merge = RT * (4 * (D / 16) * 64 * 4 + 4 * 16 * 2) * 4;
    return tiles > merge ? tiles : merge;
}

// The end of a tile loop (attn_rows_tiles, attn_rows_tiles_q8): the four waves' partials through LDS, in wave order -- one
// (O, m, l) record per column.  Lane (n, g) = `lane` of wave `wave` holds column n of every tile as the MFMA leaves it.
template <int D, int RT>
__device__ __forceinline__ void rows_merge_waves(const f4 (&o)[RT][D / 16], const float (&m_run)[RT], const float (&l_run)[RT],
                                                 const bool (&pad)[RT], const int64_t (&rec)[RT], int lane, int wave, char* smem,
                                                 float* __restrict__ part_o, float* __restrict__ part_ml) {
    constexpr int DB = D / 16;
    const int n = lane & 15, g = lane >> 4;
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
        float mw[4], lw[4], mstar = pca::kNegBig;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            mw[w] = mml[((rt * 4 + w) * 16 + n) * 2]; lw[w] = mml[((rt * 4 + w) * 16 + n) * 2 + 1];
            mstar = fmaxf(mstar, mw[w]);
        }
        float wt[4], lsum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { wt[w] = pca::fast_exp2(mw[w] - mstar); lsum += wt[w] * lw[w]; }
        if (!pad[rt]) {
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
                    *(f4*)(part_o + rec[rt] * D + db * 16 + g * 4) = acc;
                }
            }
            if (wave == 0 && g == 0) { part_ml[rec[rt] * 2] = mstar; part_ml[rec[rt] * 2 + 1] = lsum; }
        }
    }
}

// RT tiles of 16 query columns against the keys [k0, k1) of THIS WAVE, then the four waves' partials merged into one
// (O, m, l) record per column.  The formulation is attn_small_kernel's (pc_attn.hip): S^T = K . Q^T and O^T += V^T . P^T on
// mfma_f32_16x16x32_f16, Q and P as hi / lo pairs, fp32 online softmax; K fragments go from global memory into the A operand, V
// through a wave-private LDS tile and back transposed, no barrier until the merge.
// Lane (n, g) of a wave holds column n of every tile: its q row starts at q + qoff[rt], pad[rt] marks a column past the last one
// (zero operand, nothing written), it sees keys below lim[rt] (MASK only; without MASK every key of the slice) and its record
// is rec[rt].  A column that sees no key of the slice keeps (m = -1e30, l = 0).  A column of an MFMA tile depends on that
// column's B operand only and every reduction runs in a fixed order: what a column gets does not depend on the other columns.
// smem: rows_lds_bytes<D, RT>() bytes, 16-byte aligned.  All 256 threads of the workgroup must call.
template <int D, int RT, bool MASK>
__device__ __forceinline__ void attn_rows_tiles(const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo,
                                                const int64_t (&qoff)[RT], const bool (&pad)[RT], const int (&lim)[RT],
                                                const int64_t (&rec)[RT], const _Float16* kbase, const _Float16* vbase, int k0, int k1,
                                                float scale_log2, char* smem, float* __restrict__ part_o,
                                                float* __restrict__ part_ml) {
    using pca::kTK;
    constexpr int KS = D / 32, DB = D / 16, CPR = D / 8;
    constexpr int LPW = kTK * CPR / 64;              // 16-byte V chunks per lane per tile
    constexpr int kTileHalfs = kTK * D;
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    h8 qf[RT][KS], qfl[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int64_t off = qoff[rt] + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            const h8 a = *(const h8*)(q_hi + off + ks * 32), r = *(const h8*)(q_lo + off + ks * 32);
            qf[rt][ks] = pad[rt] ? z : a;
            qfl[rt][ks] = pad[rt] ? z : r;
        }
    }
    f4 o[RT][DB];
    float m_run[RT], l_run[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int db = 0; db < DB; ++db) { f4 z = {0.f, 0.f, 0.f, 0.f}; o[rt][db] = z; }
        m_run[rt] = pca::kNegBig; l_run[rt] = 0.f;
    }
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
            const int vis = MASK && lim[rt] < k1 ? lim[rt] : k1;  // keys of this slice the column sees
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

    rows_merge_waves<D, RT>(o, m_run, l_run, pad, rec, lane, wave, smem, part_o, part_ml);
}

// Eight int8 codes (two dwords, byte b of dword q = code 4q + b) -> eight fp16 values, exact.  byte ^ 0x80 is code + 128, in
// 0..255; behind the byte 0x64 it is the fp16 number 1024 + (code + 128), whose spacing is 1; one packed subtract takes 1152 off.
// Per dword: one v_xor, two v_perm_b32, two v_pk_add_f16 -- 5 VALU for 4 codes.
__device__ __forceinline__ h8 codes8_h(uint32_t w0, uint32_t w1) {
    const pca::h2 off = {(_Float16)1152.0f, (_Float16)1152.0f};
    const uint32_t x0 = w0 ^ 0x80808080u, x1 = w1 ^ 0x80808080u;
    // v_perm_b32: selector bytes 0..3 take bytes of the second operand, 4..7 of the first -> {x.b0, 0x64, x.b1, 0x64} etc.
    const pca::h2 a = __builtin_bit_cast(pca::h2, __builtin_amdgcn_perm(0x64646464u, x0, 0x04010400u)) - off;
    const pca::h2 b = __builtin_bit_cast(pca::h2, __builtin_amdgcn_perm(0x64646464u, x0, 0x04030402u)) - off;
    const pca::h2 c = __builtin_bit_cast(pca::h2, __builtin_amdgcn_perm(0x64646464u, x1, 0x04010400u)) - off;
    const pca::h2 d = __builtin_bit_cast(pca::h2, __builtin_amdgcn_perm(0x64646464u, x1, 0x04030402u)) - off;
    const h8 r = {a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    return r;
}

// attn_rows_tiles over int8 IMAGE rows (pc_kv_q8.hip's format, head_dim 128): kcodes / vcodes are the planes' codes, [rows][128]
// int8, kscale / vscale their fp32 row scales.  Same tiles, same columns, same mask (lim[rt], always on), same records and the
// same four-wave merge; what differs is how a row reaches the MFMA:
//   K  lane (n, g) loads the 32 codes [32 g, 32 g + 32) of its key row as two 16-byte loads and turns them into four h8 A
//      operands (codes8_h).  The contraction index is permuted accordingly -- k-step ks of lane group g multiplies features
//      32 g + 8 ks .. + 8, and the q operands are loaded from there --, so S^T is the same sum of the same products in another
//      order.  A code is exact in fp16: q . code is the fp32 product of the split q with the integer.
//   scale  the score of a key is acc * (kscale[key] * scale_log2) before mask and softmax; p is multiplied by vscale[key] in fp32
//      BEFORE it is split into its hi / lo halves (the row sum l takes the unscaled p).  Nothing rounds code * scale to fp16.
//   V  every lane loads eight 16-byte code chunks of the tile (64 rows x 128 B), turns each into 16 fp16 values and writes them
//      to the wave's LDS tile in the rotated row layout attn_rows_tiles' DMA leaves; the transposing reads are that function's.
// A masked key contributes exactly nothing whatever its scale holds (select, not multiply): rows behind lim may carry NaN scales.
// smem: rows_lds_bytes<128, RT>() bytes.  All 256 threads of the workgroup must call; k1 <= the rows the planes hold.
template <int RT>
__device__ __forceinline__ void attn_rows_tiles_q8(const _Float16* __restrict__ q_hi, const _Float16* __restrict__ q_lo,
                                                   const int64_t (&qoff)[RT], const bool (&pad)[RT], const int (&lim)[RT],
                                                   const int64_t (&rec)[RT], const char* kcodes, const char* vcodes,
                                                   const float* kscale, const float* vscale, int k0, int k1, float scale_log2,
                                                   char* smem, float* __restrict__ part_o, float* __restrict__ part_ml) {
    using pca::kTK;
    constexpr int D = 128, KS = D / 32, DB = D / 16;
    constexpr int CPR = D / 16;                      // 16-byte code chunks per row
    constexpr int LPW = kTK * CPR / 64;              // code chunks per lane per tile
    constexpr int kTileHalfs = kTK * D;
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    h8 qf[RT][KS], qfl[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int64_t off = qoff[rt] + g * 32;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            const h8 a = *(const h8*)(q_hi + off + ks * 8), r = *(const h8*)(q_lo + off + ks * 8);
            qf[rt][ks] = pad[rt] ? z : a;
            qfl[rt][ks] = pad[rt] ? z : r;
        }
    }
    f4 o[RT][DB];
    float m_run[RT], l_run[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int db = 0; db < DB; ++db) { f4 z = {0.f, 0.f, 0.f, 0.f}; o[rt][db] = z; }
        m_run[rt] = pca::kNegBig; l_run[rt] = 0.f;
    }
    _Float16* Vw = (_Float16*)smem + wave * kTileHalfs;            // this wave's V tile

    for (int key0 = k0; key0 < k1; key0 += kTK) {
        // every load of the tile first, all unconditional (keys past k1 re-read the last valid row and are masked below)
        pca::u32x4 kr[4][2], vr[LPW];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int key = key0 + kb * 16 + n < k1 ? key0 + kb * 16 + n : k1 - 1;
            const char* kp = kcodes + (int64_t)key * D + g * 32;
            kr[kb][0] = *(const pca::u32x4*)kp;
            kr[kb][1] = *(const pca::u32x4*)(kp + 16);
        }
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            const int c = lane + i * 64, row = c / CPR, pos = c - row * CPR;
            const int rr = key0 + row < k1 ? key0 + row : k1 - 1;
            vr[i] = *(const pca::u32x4*)(vcodes + (int64_t)rr * D + pos * 16);
        }
        // the scales of the keys this lane holds scores of: key0 + 16 kb + 4 g + r
        float ksl[4][4], vsc[4][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = key0 + kb * 16 + g * 4 + r;
                const int kc = key < k1 ? key : k1 - 1;
                ksl[kb][r] = kscale[kc] * scale_log2;
                vsc[kb][r] = vscale[kc];
            }
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
                    const h8 a = codes8_h(kr[kb][ks >> 1][(ks & 1) * 2], kr[kb][ks >> 1][(ks & 1) * 2 + 1]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[rt][ks], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qfl[rt][ks], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + kb * 16 + g * 4 + r;
                    const float s = key < vis ? acc[r] * ksl[kb][r] : -INFINITY;
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
                    const int key = key0 + kb * 16 + g * 4 + r;
                    const float e = pca::fast_exp2(sv[kb][r] - m_new);
                    rs += e;
                    const float pv = key < vis ? e * vsc[kb][r] : 0.f;
                    const _Float16 eh = (_Float16)pv;
                    pb[rt][kb >> 1][(kb & 1) * 4 + r] = eh;
                    pbl[rt][kb >> 1][(kb & 1) * 4 + r] = (_Float16)(pv - (float)eh);
                }
            rs += __shfl_xor(rs, 16);
            rs += __shfl_xor(rs, 32);
            l_run[rt] = l_run[rt] * alpha + rs;
#pragma unroll
            for (int db = 0; db < DB; ++db) { o[rt][db][0] *= alpha; o[rt][db][1] *= alpha; o[rt][db][2] *= alpha; o[rt][db][3] *= alpha; }
            m_run[rt] = m_new;
        }
        // the V tile as fp16 into this wave's LDS tile: chunk `pos` of a row is features [16 pos, 16 pos + 16), which the row
        // layout of attn_rows_tiles rotates by 16 (row & 7) halfs
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            const int c = lane + i * 64, row = c / CPR, pos = c - row * CPR;
            _Float16* dst = Vw + row * D + ((pos * 16 + 16 * (row & 7)) & (D - 1));
            *(h8*)dst = codes8_h(vr[i][0], vr[i][1]);
            *(h8*)(dst + 8) = codes8_h(vr[i][2], vr[i][3]);
        }
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
        __builtin_amdgcn_wave_barrier();             // (the next tile's stores overwrite what these reads took)
    }

    rows_merge_waves<D, RT>(o, m_run, l_run, pad, rec, lane, wave, smem, part_o, part_ml);
}

// Merge of the records of a (row, head) in index (= key) order, one workgroup per (head, row), one thread per head dim; k + 1
// rows per slot, nrec records per (row, head).  leader != nullptr (the entries with shared trunks; uniform over the launch): the
// first nsplit_t records are the trunk launch's, and a row of a slot on its own (slot_trunk_rows 0) has none: its merge starts at
// record nsplit_t.  kvq_base != nullptr (pc_attn_decode_slots_trunk_q8): the shared rows are slot_trunk_rows_q8's, the question the
// launches of that entry ask.  den > 0: every row sees its own key.
template <int D>
__global__ __launch_bounds__(D) void attn_merge_slots_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                             const int32_t* __restrict__ cap, const int32_t* __restrict__ len,
                                                             const int32_t* __restrict__ live, const int32_t* __restrict__ leader,
                                                             const int32_t* __restrict__ trunk,
                                                             const uint64_t* __restrict__ kv_base, int S, int k, int H, int nsplit_t,
                                                             int nrec, _Float16* __restrict__ of_hi, _Float16* __restrict__ of_lo,
                                                             const uint64_t* __restrict__ kvq_base, int qcap) {
    const int h = blockIdx.x, r = blockIdx.y, d = threadIdx.x;
    const int b = r / (k + 1);
    if (!lookup_slot_runs(cap, len, live, b, k)) return;
    const int64_t base = ((int64_t)r * H + h) * nrec;
    int s0 = 0;
    if (leader != nullptr) {
        const int T = kvq_base != nullptr ? slot_trunk_rows_q8(b, S, kvq_base, qcap, len, leader, trunk)
                                          : slot_trunk_rows(b, S, kv_base, cap, len, leader, trunk);
        s0 = T > 0 ? 0 : nsplit_t;
    }
    float ms = pca::kNegBig;
    for (int s = s0; s < nrec; ++s) ms = fmaxf(ms, part_ml[(base + s) * 2]);
    float num = 0.0f, den = 0.0f;
    for (int s = s0; s < nrec; ++s) {
        const float wt = exp2f(part_ml[(base + s) * 2] - ms);
        den = fmaf(wt, part_ml[(base + s) * 2 + 1], den);
        num = fmaf(wt, part_o[(base + s) * D + d], num);
    }
    _Float16 hi, lo;
    pc_split(num / den, hi, lo);
    const int64_t off = pca::frag_off(r, h * D + d, H * D / 32);
    of_hi[off] = hi;
    of_lo[off] = lo;
}

}  // namespace pcr
