// pc_gemm_w4 -- the <= 16-row weight-streaming projections over MXFP4 weight images (OCP MX: 32-element blocks of FP4 E2M1
// codes under one E8M0 scale; include/promptcache_hip.h documents the two images).  4.25 bits per weight instead of 16.
//
// Contract.  For 1 <= M <= 16 rows:  y[m][n] = sum_k (hi + lo)[m][k] * W'[n][k],  W' = the dequantised weight (exact in fp16),
// accumulated in fp32 on mfma_f32_16x16x32_f16 -- the arithmetic of pc_gemm (pc_gemm_skinny.h) on the fp16 image of W'.  An MX
// block is one k-step of that MFMA for one weight row, so a lane's eight values of a k-step share one scale: the codes are
// converted right before their MFMAs by v_cvt_scalef32_pk_f16_fp4 (one byte of codes and an fp32 scale -> two fp16 values;
// the scale operand is the bit pattern  E8M0 byte << 23,  i.e. 2^(byte - 127)).  Four conversions and two MFMAs (hi, lo) per
// weight tile and k-step.
//
// Kernel.  One workgroup = 8 waves that split K eight ways over the same T output tiles (T gate/up PAIRS for the SiLU
// epilogue), as gemm_skinny_kernel does.  The unit of the K loop is a QUAD of k-steps (128 features): one 16-byte load per lane
// and tile brings the codes of four k-steps, one dword per row their four scales.  A block is UQ quads: every load of the block
// is issued, then the MFMAs.  The partial tiles meet in LDS and are added in wave order; the epilogue is pc_gemm's
// (tile_epilogue: STORE, ADD into the fp32 residual stream, SILU into fragment planes).  Activation source: the split-precision
// fragment planes, or the fp32 residual stream with RMSNorm folded in exactly as k_block_norm folds it (gain through the wave's
// LDS slice, 1/rms applied to the reduced tile).
//
// Properties the loops above rely on:
//   * The summation order is fixed: k-steps in ascending order inside a wave, waves 0..7 in order in the reduction.  The result
//     of a launch does not depend on timing; there is no atomic and no hand-off between workgroups (K is never cut across
//     workgroups here).
//   * A row's result does not depend on M, on the other rows or on its index in the tile: the K split is a function of K alone
//     (ceil(K/128 / 8) quads per wave), the tiles per workgroup a function of (epilogue, source, N) alone, and a column of the
//     MFMA's B operand only reaches the same column of D.  Rows behind M are neither loaded nor stored; rows in [*rows_dev, M) are not
//     loaded: they are computed from zero activations and stored (unspecified values to the caller, as in pc_gemm).
//   * K % 128 == 0, N % 16 == 0 (SILU: N % 64 == 0), M <= 16; the norm source needs K <= 16384.
#include "pc_gemm_skinny.h"

namespace pcg {
namespace {

struct W4Params {
    GemmParams g;               // rows, tiles, activation source, epilogue outputs (wf / wscale unused)
    const unsigned char* codes; // [ntiles][KQ][64][16]
    const uint32_t* scales;     // [ntiles][KQ][16]
    int32_t KQ;                 // K / 128
};

// the eight fp16 weights of one k-step of this lane: dword of codes (low nibble = lower feature), E8M0 byte
__device__ __forceinline__ h8 cvt_w4(uint32_t c, uint32_t e8) {
    const float sc = __uint_as_float(e8 << 23);
    const h2v a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 0);
    const h2v b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 1);
    const h2v d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 2);
    const h2v e = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 3);
    const h8 out = {a[0], a[1], b[0], b[1], d[0], d[1], e[0], e[1]};
    return out;
}

// One block of UQ quads starting at quad q (nvalid of them real: the others re-read the last valid quad and are skipped).
template <int TT, int UQ, bool NORM>
__device__ __forceinline__ void w4_block(const W4Params& p, const int (&tile)[TT], int lane, int q, int nvalid, bool row_ok,
                                         const float* xrow, const _Float16* gam, GammaStage& gst, f4 (&acc)[TT], float& ss) {
    const int m = lane & 15;
    u32x4 raw[UQ][TT];
    uint32_t sc[UQ][TT];
    h8 xh[NORM ? 1 : UQ * 4], xl[NORM ? 1 : UQ * 4];
    f4 xa[NORM ? UQ * 4 : 1][2];
#pragma unroll
    for (int u = 0; u < UQ; ++u) {
        const int qq = q + (u < nvalid ? u : nvalid - 1);
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            const int64_t unit = (int64_t)tile[t] * p.KQ + qq;
            raw[u][t] = __builtin_nontemporal_load((const u32x4*)(p.codes + (unit * 64 + lane) * 16));   // 1 KiB / wave, streamed once
            sc[u][t] = p.scales[unit * 16 + m];
        }
    }
#pragma unroll
    for (int i = 0; i < UQ * 4; ++i) {
        if constexpr (NORM) { f4 z = {0.f, 0.f, 0.f, 0.f}; xa[i][0] = z; xa[i][1] = z; }
        else { h8 z = {0, 0, 0, 0, 0, 0, 0, 0}; xh[i] = z; xl[i] = z; }
    }
    if (row_ok) {                                   // pad rows cost no traffic; their columns are never stored
#pragma unroll
        for (int u = 0; u < UQ; ++u) {
            const int qq = q + (u < nvalid ? u : nvalid - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ks = qq * 4 + j;
                if constexpr (NORM) {
                    xa[u * 4 + j][0] = *(const f4*)(xrow + ks * 32);
                    xa[u * 4 + j][1] = *(const f4*)(xrow + ks * 32 + 4);
                } else {
                    const int64_t off = ((int64_t)ks * 64 + lane) * 8;
                    xh[u * 4 + j] = ldg_h8(p.g.xf_hi + off);
                    xl[u * 4 + j] = ldg_h8(p.g.xf_lo + off);
                }
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);              // the whole block's loads in flight before the first MFMA (see k_block)
    if constexpr (NORM) gst.commit();
#pragma unroll
    for (int u = 0; u < UQ; ++u) {
        if (u >= nvalid) continue;                  // (wave-uniform) a re-read quad contributes nothing
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h8 hi, lo;
            if constexpr (NORM) {
                const h8 gw = *(const h8*)(gam + ((q + u) * 4 + j) * 32);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xv = e < 4 ? xa[u * 4 + j][0][e] : xa[u * 4 + j][1][e - 4];
                    ss += xv * xv;
                    const float v = xv * (float)gw[e];
                    _Float16 vh, vl;
                    pc_split(v, vh, vl);
                    hi[e] = vh; lo[e] = vl;
                }
            } else {
                hi = xh[u * 4 + j]; lo = xl[u * 4 + j];
            }
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                const h8 wv = cvt_w4(raw[u][t][j], (sc[u][t] >> (8 * j)) & 0xffu);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv, hi, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv, lo, acc[t], 0, 0, 0);
            }
        }
    }
}

template <int T, int EPI, bool NORM>
__global__ __launch_bounds__(kThreads) void gemm_w4_kernel(const W4Params p) {
    constexpr int TT = (EPI == EPI_SILU) ? 2 * T : T;
    constexpr int UQ = TT <= 2 ? 4 : (TT <= 4 ? 2 : 1);          // quads per block: ~4 KiB of codes per wave in flight
    __shared__ __attribute__((aligned(16))) float red[kWaves][TT][64][4];
    __shared__ float ssl[kWaves][16];
    __shared__ __attribute__((aligned(16))) _Float16 gam_lds[NORM ? kWaves * kGamHalfs : 8];

    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = blockIdx.x;
    const int per = (p.KQ + kWaves - 1) / kWaves;                // quads per wave: a function of K alone
    const int q0 = wave * per < p.KQ ? wave * per : p.KQ;
    const int q1 = q0 + per < p.KQ ? q0 + per : p.KQ;
    int tile[TT];
    wg_tiles<T, EPI>(p.g, bx, tile);

    f4 acc[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) { f4 z = {0.f, 0.f, 0.f, 0.f}; acc[t] = z; }
    const int rows_live = p.g.m_dev ? (*p.g.m_dev < p.g.M ? *p.g.m_dev : p.g.M) : p.g.M;
    const bool row_ok = m < rows_live;
    float ss = 0.f;
    const float* xrow = nullptr;
    const _Float16* gam = nullptr;
    GammaStage gst;
    gst.done = true;
    if constexpr (NORM) {
        xrow = p.g.xn + (int64_t)m * (p.KQ * 128) + g * 8;       // (rows behind rows_live are never read)
        _Float16* gslice = gam_lds + wave * kGamHalfs;
        gst.issue(p.g.gamma + (int64_t)q0 * 128, gslice, (q1 - q0) * 128, lane);
        gam = gslice + g * 8 - q0 * 128;
    }
    int q = q0;
    for (; q + UQ <= q1; q += UQ) w4_block<TT, UQ, NORM>(p, tile, lane, q, UQ, row_ok, xrow, gam, gst, acc, ss);
    if (q < q1) w4_block<TT, UQ, NORM>(p, tile, lane, q, q1 - q, row_ok, xrow, gam, gst, acc, ss);
    if constexpr (NORM) {
        ss += __shfl_xor(ss, 16);
        ss += __shfl_xor(ss, 32);
        if (g == 0) ssl[wave][m] = ss;                           // this wave's share of sum(x^2) of row m
    }

    // ---- split-K reduction through LDS, fixed wave order; item = one output tile (a gate/up pair for SILU) ----
#pragma unroll
    for (int t = 0; t < TT; ++t) *(f4*)red[wave][t][lane] = acc[t];
    lds_barrier();
    if (wave < T) {
        f4 v = {0.f, 0.f, 0.f, 0.f}, u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const f4 x = *(const f4*)red[w][wave][lane];
            v[0] += x[0]; v[1] += x[1]; v[2] += x[2]; v[3] += x[3];
            if (EPI == EPI_SILU) {
                const f4 y = *(const f4*)red[w][T + wave][lane];
                u[0] += y[0]; u[1] += y[1]; u[2] += y[2]; u[3] += y[3];
            }
        }
        if constexpr (NORM) {
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) tot += ssl[w][m];
            const float rs = rsqrtf(tot / (float)(p.KQ * 128) + p.g.eps);
            v[0] *= rs; v[1] *= rs; v[2] *= rs; v[3] *= rs;
            u[0] *= rs; u[1] *= rs; u[2] *= rs; u[3] *= rs;
        }
        tile_epilogue<EPI>(p.g, v, u, m, bx * T + wave, g, 0);
    }
}

template <int T, int EPI, bool NORM>
int launch_w4(const W4Params& p, int units, hipStream_t s) {
    hipLaunchKernelGGL((gemm_w4_kernel<T, EPI, NORM>), dim3(pc_ceil_div(units, T)), dim3(kThreads), 0, s, p);
    return pc_check_launch("gemm_w4_kernel");
}

}  // namespace
}  // namespace pcg

using namespace pcg;

// Tiles per workgroup: the smallest instantiated T whose grid fits one round of 256 CUs, else the largest -- a function of
// (epilogue, source, N) only.  Twelve kernels: ADD {1, 2}; STORE {1, 2, 4} x {planes, norm}; SILU planes {1}, norm {1, 2, 3}.
PC_EXPORT int pc_gemm_w4(const pc_gemm_w4_args* a, void* stream) {
    PC_REQUIRE(a && a->struct_bytes == (uint32_t)sizeof(pc_gemm_w4_args), PC_ERR_ARG,
               "pc_gemm_w4: args is NULL or struct_bytes != sizeof(pc_gemm_w4_args) (ABI mismatch)");
    const int epi = a->epilogue, M = a->M, N = a->N, K = a->K;
    PC_REQUIRE(epi == PC_GEMM_EPI_STORE || epi == PC_GEMM_EPI_ADD || epi == PC_GEMM_EPI_SILU, PC_ERR_ARG,
               "pc_gemm_w4: epilogue %d is not store / add / SiLU", epi);
    PC_REQUIRE(M > 0 && M <= 16, PC_ERR_ARG, "pc_gemm_w4: M=%d outside 1..16 (more rows run pc_gemm on the fp16 image)", M);
    PC_REQUIRE(N > 0 && N % 16 == 0 && K > 0 && K % 128 == 0, PC_ERR_ARG, "pc_gemm_w4: need N%%16==0 and K%%128==0 (N=%d, K=%d)", N, K);
    PC_REQUIRE(a->codes && a->scales && ((uintptr_t)a->codes & 15) == 0 && ((uintptr_t)a->scales & 3) == 0, PC_ERR_ARG,
               "pc_gemm_w4: null or misaligned weight images");
    const bool norm = a->x != nullptr;
    PC_REQUIRE(norm ? (a->norm_weight && !a->xf_hi && !a->xf_lo) : (a->xf_hi && a->xf_lo), PC_ERR_ARG,
               "pc_gemm_w4: pass both activation planes or (x, norm_weight)");
    PC_REQUIRE(!norm || (K <= 128 * (kGamSteps / 4) * kWaves && epi != PC_GEMM_EPI_ADD), PC_ERR_ARG,
               "pc_gemm_w4: the fused-RMSNorm source needs K <= 16384 and the store or SiLU epilogue");
    W4Params p;
    memset(&p, 0, sizeof(p));
    p.codes = (const unsigned char*)a->codes; p.scales = (const uint32_t*)a->scales; p.KQ = K / 128;
    GemmParams& gp = p.g;
    gp.xf_hi = (const _Float16*)a->xf_hi; gp.xf_lo = (const _Float16*)a->xf_lo;
    gp.xn = a->x; gp.gamma = (const _Float16*)a->norm_weight; gp.eps = a->eps;
    gp.M = M; gp.m_dev = a->rows_dev; gp.ntiles = N / 16; gp.KS = K / 32; gp.kslices = 1;
    hipStream_t s = (hipStream_t)stream;
    if (epi == PC_GEMM_EPI_SILU) {
        PC_REQUIRE(N % 64 == 0 && a->of_hi && a->of_lo, PC_ERR_ARG, "pc_gemm_w4: the SiLU epilogue needs N = 2*inter with inter%%32==0 and output planes");
        gp.of_hi = (_Float16*)a->of_hi; gp.of_lo = (_Float16*)a->of_lo;
        gp.npairs = N / 32; gp.KSo = (N / 2) / 32;
        const int units = gp.npairs;
        if (!norm) return launch_w4<1, EPI_SILU, false>(p, units, s);
        if (units <= 256) return launch_w4<1, EPI_SILU, true>(p, units, s);
        if (units <= 512) return launch_w4<2, EPI_SILU, true>(p, units, s);
        return launch_w4<3, EPI_SILU, true>(p, units, s);
    }
    PC_REQUIRE(a->y && a->ldy >= N && a->ldy % 4 == 0, PC_ERR_ARG, "pc_gemm_w4: bad output");
    gp.y = a->y; gp.ldy = a->ldy; gp.slab_stride = (int64_t)M * a->ldy;
    const int units = gp.ntiles;
    if (epi == PC_GEMM_EPI_ADD) {
        if (units <= 256) return launch_w4<1, EPI_ADD, false>(p, units, s);
        return launch_w4<2, EPI_ADD, false>(p, units, s);
    }
    if (norm) {
        if (units <= 256) return launch_w4<1, EPI_STORE, true>(p, units, s);
        if (units <= 512) return launch_w4<2, EPI_STORE, true>(p, units, s);
        return launch_w4<4, EPI_STORE, true>(p, units, s);
    }
    if (units <= 256) return launch_w4<1, EPI_STORE, false>(p, units, s);
    if (units <= 512) return launch_w4<2, EPI_STORE, false>(p, units, s);
    return launch_w4<4, EPI_STORE, false>(p, units, s);
}
