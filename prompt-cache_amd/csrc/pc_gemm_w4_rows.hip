// pc_gemm_w4_rows -- the 1..64-row weight-streaming projections over the MXFP4 weight images of pc_gemm_w4 (pc_gemm_w4.hip; the
// images are documented in include/promptcache_hip.h).  The same two images, no re-layout: this is the form the 17..64-row flows
// call (the cached step with a 17..64-token question, the slot-lookup verify step of S * (k + 1) rows).
//
// Contract.  For 1 <= M <= 64 rows:  y[m][n] = sum_k (hi + lo)[m][k] * W'[n][k]  with the activations as split-precision
// fragment planes [ceil(M/16)][K/32][64][8] -- pc_gemm_w4's arithmetic, row tile by row tile.  Epilogues: STORE (with K cut
// into kslices workgroup slices, slice s writes slab y + s * M * ldy: the slabs pc_rmsnorm_frag folds) and SILU into planes.
//
// Kernel.  One workgroup = 8 waves that split the K range of its slice eight ways over the same T output tiles (T gate/up
// pairs for SILU) and up to four row tiles.  The unit of the K loop is a QUAD of k-steps: one 16-byte load per lane and weight
// tile.  A weight fragment is converted ONCE per k-step (four v_cvt_scalef32_pk_f16_fp4) and multiplied against the hi and lo
// plane of every LIVE row tile: row tiles at or behind ceil(M/16) are skipped wave-uniformly (no loads, no MFMAs), so one
// instantiation per epilogue serves every M.  The activations of ONE k-step (8 VGPRs per row tile) are double-buffered: the
// next k-step's are fetched (L2) while the current one's 8 * TT * tiles MFMAs run, the next quad's codes (HBM) one quad ahead.
//
// Summation order (fixed; no atomics, no hand-off between workgroups):
//   * slice s owns the quads [s * ceil(KQ / kslices), ...) clipped to KQ; a slice that owns none stores zeros to its slab;
//   * inside a slice, wave w owns ceil(n / 8) consecutive quads of the slice's n, ascending: a function of (K, kslices) alone;
//   * a wave adds k-steps in ascending order, hi plane then lo plane; the LDS reduction adds the waves 0..7 in order.
//   Hence a row's bits depend neither on M, nor on the other rows, nor on its row tile, and at kslices = 1 they are the bits
//   pc_gemm_w4 gives that row (same K split, same order, same epilogue code).
#include "pc_gemm_skinny.h"

namespace pcg {
namespace {

constexpr int kRowsMT = 4;          // row tiles the accumulators are laid out for (M <= 64)

struct W4RowsParams {
    GemmParams g;               // rows, tiles, activation planes, epilogue outputs, kslices / slab_stride
    const unsigned char* codes; // [ntiles][KQ][64][16]
    const uint32_t* scales;     // [ntiles][KQ][16]
    int32_t KQ;                 // K / 128
};

// the eight fp16 weights of one k-step of this lane: dword of codes (low nibble = lower feature), E8M0 byte
__device__ __forceinline__ h8 cvt_w4_rows(uint32_t c, uint32_t e8) {
    const float sc = __uint_as_float(e8 << 23);
    const h2v a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 0);
    const h2v b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 1);
    const h2v d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 2);
    const h2v e = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 3);
    const h8 out = {a[0], a[1], b[0], b[1], d[0], d[1], e[0], e[1]};
    return out;
}

template <int TT>
__device__ __forceinline__ void w4r_load_w(const W4RowsParams& p, const int (&tile)[TT], int lane, int q, u32x4 (&raw)[TT],
                                           uint32_t (&sc)[TT]) {
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        const int64_t unit = (int64_t)tile[t] * p.KQ + q;
        raw[t] = __builtin_nontemporal_load((const u32x4*)(p.codes + (unit * 64 + lane) * 16));   // 1 KiB / wave, streamed once
        sc[t] = p.scales[unit * 16 + (lane & 15)];
    }
}

// the activation fragments of k-step ks for the live row tiles (pad rows cost no traffic: their columns are never stored)
__device__ __forceinline__ void w4r_load_x(const W4RowsParams& p, int lane, int ks, int mtl, const bool (&row_ok)[kRowsMT],
                                           h8 (&xh)[kRowsMT], h8 (&xl)[kRowsMT]) {
#pragma unroll
    for (int a = 0; a < kRowsMT; ++a) {
        const h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        xh[a] = z; xl[a] = z;
        if (a < mtl && row_ok[a]) {
            const int64_t off = (((int64_t)a * p.g.KS + ks) * 64 + lane) * 8;
            xh[a] = ldg_h8(p.g.xf_hi + off);                                                    // L2-resident
            xl[a] = ldg_h8(p.g.xf_lo + off);
        }
    }
}

template <int T, int EPI>
__global__ __launch_bounds__(kThreads) void gemm_w4_rows_kernel(const W4RowsParams p) {
    constexpr int MT = kRowsMT;
    constexpr int TT = (EPI == EPI_SILU) ? 2 * T : T;
    static_assert(2 * T <= kWaves, "one reduction round = two row tiles of T items, one item per wave");
    __shared__ __attribute__((aligned(16))) float red[kWaves][2 * TT][64][4];

    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = blockIdx.x, by = blockIdx.y;
    const int mtl = (p.g.M + 15) >> 4;                           // live row tiles (workgroup-uniform)
    // K range: the slice's quads, then eight ways across the waves
    const int ksq = (p.KQ + p.g.kslices - 1) / p.g.kslices;
    const int kq0 = by * ksq < p.KQ ? by * ksq : p.KQ;
    const int kq1 = kq0 + ksq < p.KQ ? kq0 + ksq : p.KQ;
    const int per = (kq1 - kq0 + kWaves - 1) / kWaves;
    const int q0 = kq0 + wave * per < kq1 ? kq0 + wave * per : kq1;
    const int q1 = q0 + per < kq1 ? q0 + per : kq1;
    int tile[TT];
    wg_tiles<T, EPI>(p.g, bx, tile);

    f4 acc[MT][TT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int t = 0; t < TT; ++t) { f4 z = {0.f, 0.f, 0.f, 0.f}; acc[a][t] = z; }
    bool row_ok[MT];
#pragma unroll
    for (int a = 0; a < MT; ++a) row_ok[a] = a * 16 + m < p.g.M;

    if (q0 < q1) {
        u32x4 rawn[TT];
        uint32_t scn[TT];
        h8 xh[2][MT], xl[2][MT];
        w4r_load_w<TT>(p, tile, lane, q0, rawn, scn);
        w4r_load_x(p, lane, q0 * 4, mtl, row_ok, xh[0], xl[0]);
        for (int q = q0; q < q1; ++q) {
            u32x4 raw[TT];
            uint32_t sc[TT];
#pragma unroll
            for (int t = 0; t < TT; ++t) { raw[t] = rawn[t]; sc[t] = scn[t]; }
            const int qn = q + 1 < q1 ? q + 1 : q;               // (the last quad re-reads itself: in bounds, unused)
            w4r_load_w<TT>(p, tile, lane, qn, rawn, scn);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w4r_load_x(p, lane, j < 3 ? q * 4 + j + 1 : qn * 4, mtl, row_ok, xh[(j + 1) & 1], xl[(j + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);               // the prefetches stay in front of this k-step's MFMAs
                h8 wv[TT];
#pragma unroll
                for (int t = 0; t < TT; ++t) wv[t] = cvt_w4_rows(raw[t][j], (sc[t] >> (8 * j)) & 0xffu);
#pragma unroll
                for (int a = 0; a < MT; ++a) {
                    if (a < mtl) {                               // (wave-uniform)
#pragma unroll
                        for (int t = 0; t < TT; ++t) {
                            acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[t], xh[j & 1][a], acc[a][t], 0, 0, 0);
                            acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[t], xl[j & 1][a], acc[a][t], 0, 0, 0);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // ---- split-K reduction through LDS, fixed wave order; a round = two row tiles, an item = one output tile (a gate/up pair
    // for SILU) of one row tile, one item per wave ----
#pragma unroll
    for (int r = 0; r < MT / 2; ++r) {
        if (2 * r < mtl) {                                       // (workgroup-uniform: every wave meets the same barriers)
            if (r > 0) lds_barrier();                            // the previous round's readers are done with the buffer
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int t = 0; t < TT; ++t) *(f4*)red[wave][i * TT + t][lane] = acc[2 * r + i][t];
            lds_barrier();
            const int i = wave / T, t = wave - i * T;
            if (wave < 2 * T && 2 * r + i < mtl) {
                f4 v = {0.f, 0.f, 0.f, 0.f}, u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int w = 0; w < kWaves; ++w) {
                    const f4 x = *(const f4*)red[w][i * TT + t][lane];
                    v[0] += x[0]; v[1] += x[1]; v[2] += x[2]; v[3] += x[3];
                    if (EPI == EPI_SILU) {
                        const f4 y = *(const f4*)red[w][i * TT + T + t][lane];
                        u[0] += y[0]; u[1] += y[1]; u[2] += y[2]; u[3] += y[3];
                    }
                }
                tile_epilogue<EPI>(p.g, v, u, (2 * r + i) * 16 + m, bx * T + t, g, by);
            }
        }
    }
}

template <int T, int EPI>
int launch_w4_rows(const W4RowsParams& p, int units, hipStream_t s) {
    hipLaunchKernelGGL((gemm_w4_rows_kernel<T, EPI>), dim3(pc_ceil_div(units, T), p.g.kslices), dim3(kThreads), 0, s, p);
    return pc_check_launch("gemm_w4_rows_kernel");
}

}  // namespace
}  // namespace pcg

using namespace pcg;

// Two kernels, one per epilogue: STORE with four output tiles per workgroup, SILU with two gate/up pairs -- sixteen accumulator
// tiles at four row tiles either way.  Every workgroup reads all of the activation planes, so wide workgroups keep that L2
// traffic next to the weights' (pc_gemm_skinny.h, launch_T).
PC_EXPORT int pc_gemm_w4_rows(const pc_gemm_w4_rows_args* a, void* stream) {
    PC_REQUIRE(a && a->struct_bytes == (uint32_t)sizeof(pc_gemm_w4_rows_args), PC_ERR_ARG,
               "pc_gemm_w4_rows: args is NULL or struct_bytes != sizeof(pc_gemm_w4_rows_args) (ABI mismatch)");
    const int epi = a->epilogue, M = a->M, N = a->N, K = a->K, kslices = a->kslices;
    PC_REQUIRE(epi == PC_GEMM_EPI_STORE || epi == PC_GEMM_EPI_SILU, PC_ERR_ARG, "pc_gemm_w4_rows: epilogue %d is not store / SiLU", epi);
    PC_REQUIRE(M > 0 && M <= 64, PC_ERR_ARG, "pc_gemm_w4_rows: M=%d outside 1..64", M);
    PC_REQUIRE(N > 0 && N % 16 == 0 && K > 0 && K % 128 == 0, PC_ERR_ARG, "pc_gemm_w4_rows: need N%%16==0 and K%%128==0 (N=%d, K=%d)", N, K);
    PC_REQUIRE(kslices >= 1 && kslices <= 8 && (kslices == 1 || epi == PC_GEMM_EPI_STORE), PC_ERR_ARG,
               "pc_gemm_w4_rows: kslices=%d outside 1..8, or K slices with an epilogue other than store", kslices);
    PC_REQUIRE(a->codes && a->scales && ((uintptr_t)a->codes & 15) == 0 && ((uintptr_t)a->scales & 3) == 0, PC_ERR_ARG,
               "pc_gemm_w4_rows: null or misaligned weight images");
    PC_REQUIRE(a->xf_hi && a->xf_lo && ((uintptr_t)a->xf_hi & 15) == 0 && ((uintptr_t)a->xf_lo & 15) == 0, PC_ERR_ARG,
               "pc_gemm_w4_rows: null or misaligned activation planes");
    W4RowsParams p;
    memset(&p, 0, sizeof(p));
    p.codes = (const unsigned char*)a->codes; p.scales = (const uint32_t*)a->scales; p.KQ = K / 128;
    GemmParams& gp = p.g;
    gp.xf_hi = (const _Float16*)a->xf_hi; gp.xf_lo = (const _Float16*)a->xf_lo;
    gp.M = M; gp.ntiles = N / 16; gp.KS = K / 32; gp.kslices = kslices;
    hipStream_t s = (hipStream_t)stream;
    if (epi == PC_GEMM_EPI_SILU) {
        PC_REQUIRE(N % 64 == 0 && a->of_hi && a->of_lo, PC_ERR_ARG,
                   "pc_gemm_w4_rows: the SiLU epilogue needs N = 2*inter with inter%%32==0 and output planes");
        gp.of_hi = (_Float16*)a->of_hi; gp.of_lo = (_Float16*)a->of_lo;
        gp.npairs = N / 32; gp.KSo = (N / 2) / 32;
        return launch_w4_rows<2, EPI_SILU>(p, gp.npairs, s);
    }
    PC_REQUIRE(a->y && a->ldy >= N && a->ldy % 4 == 0 && ((uintptr_t)a->y & 15) == 0, PC_ERR_ARG, "pc_gemm_w4_rows: bad output");
    gp.y = a->y; gp.ldy = a->ldy; gp.slab_stride = (int64_t)M * a->ldy;
    return launch_w4_rows<4, EPI_STORE>(p, gp.ntiles, s);
}
