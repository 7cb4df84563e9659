// pc_w4_expand -- the fp16 image of an MXFP4 weight, produced from the two 4-bit images of pc_gemm_w4 (include/promptcache_hip.h
// documents them).  The many-row projections (pc_gemm_dense on the row-major image, pc_gemm / gemm_rows_kernel on the fragment
// image) read a weight once per launch, so a model that keeps only the 4-bit images expands a projection into one scratch
// buffer right before its consumer (LlamaHIP keep_fp16=False).
//
// Contract.  out = W' = the dequantised weight, bit for bit what _native.dequantize_mxfp4 gives: a grid value times 2^e with e
// in [-13, 13] is an fp16 normal or zero, so the conversion rounds nothing.  Two output layouts:
//   FRAG      [N/16][K/32][64][8], the image of _native.to_weight_frags.  The 4-bit image is that image at 4 bits: lane L of
//             tile t, quad s holds in byte group j the eight values lane L of fragment (t, 4s + j) holds.  One 16-byte load and
//             four 16-byte stores per lane, each store 1 KiB contiguous over the wave.
//   ROWMAJOR  [N][ld_out]: lane 16g + m stores 16 bytes at row 16t + m, column 128s + 32j + 8g (columns behind K untouched).
// row_perm (optional): output row r holds source row row_perm[r]; the lane then reads the code bytes and the scale dword of lane
// (g, row_perm[r] % 16) of source tile row_perm[r] / 16.  An index outside [0, N) is out of contract (it is clamped: no read
// leaves the images).
//
// Kernel.  A unit = one (tile, quad) = 1 KiB of codes + 64 B of scales in, 4 KiB out, one wave.  Waves walk the units with a
// grid stride; the grid is sized to eight waves per SIMD over the whole chip.  No LDS, no scratch, ~20 VGPRs.
#include "pc_common.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kExpandThreads = 256;
constexpr int kExpandWaves = kExpandThreads / 64;
constexpr int kExpandMaxBlocks = 256 * 8;       // 256 CUs x 8 workgroups of 4 waves = 8 waves per SIMD

// the eight fp16 weights of one k-step of this lane: dword of codes (low nibble = lower feature), E8M0 byte (as pc_gemm_w4.hip)
__device__ __forceinline__ h8 cvt_w4_expand(uint32_t c, uint32_t e8) {
    const float sc = __uint_as_float(e8 << 23);
    const h2v a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 0);
    const h2v b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 1);
    const h2v d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 2);
    const h2v e = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 3);
    const h8 out = {a[0], a[1], b[0], b[1], d[0], d[1], e[0], e[1]};
    return out;
}

__global__ __launch_bounds__(kExpandThreads) void w4_expand_kernel(const unsigned char* __restrict__ codes,
                                                                   const uint32_t* __restrict__ scales,
                                                                   const int32_t* __restrict__ row_perm, _Float16* __restrict__ out,
                                                                   int ntiles, int KQ, int64_t ld_out, int rowmajor) {
    const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t units = (int64_t)ntiles * KQ;
    const int64_t stride = (int64_t)gridDim.x * kExpandWaves;
    for (int64_t u = (int64_t)blockIdx.x * kExpandWaves + wave; u < units; u += stride) {
        const int t = (int)(u / KQ), s = (int)(u - (int64_t)t * KQ);
        int st = t, sm = m;                                         // source tile and row in it
        if (row_perm) {
            int r = row_perm[t * 16 + m];
            r = r < 0 ? 0 : (r >= ntiles * 16 ? ntiles * 16 - 1 : r);
            st = r >> 4; sm = r & 15;
        }
        const int64_t su = (int64_t)st * KQ + s;
        const u32x4 raw = __builtin_nontemporal_load((const u32x4*)(codes + (su * 64 + g * 16 + sm) * 16));   // streamed once
        const uint32_t sc = scales[su * 16 + sm];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const h8 v = cvt_w4_expand(raw[j], (sc >> (8 * j)) & 0xffu);
            _Float16* dst = rowmajor ? out + (int64_t)(t * 16 + m) * ld_out + (s * 128 + j * 32 + g * 8)
                                     : out + (((int64_t)t * (KQ * 4) + (s * 4 + j)) * 64 + lane) * 8;
            *(h8*)dst = v;
        }
    }
}

}  // namespace

PC_EXPORT int pc_w4_expand(const pc_w4_expand_args* a, void* stream) {
    PC_REQUIRE(a && a->struct_bytes == (uint32_t)sizeof(pc_w4_expand_args), PC_ERR_ARG,
               "pc_w4_expand: args is NULL or struct_bytes != sizeof(pc_w4_expand_args) (ABI mismatch)");
    const int N = a->N, K = a->K;
    PC_REQUIRE(a->layout == PC_W4_EXPAND_FRAG || a->layout == PC_W4_EXPAND_ROWMAJOR, PC_ERR_ARG,
               "pc_w4_expand: layout %d is neither PC_W4_EXPAND_FRAG nor PC_W4_EXPAND_ROWMAJOR", a->layout);
    PC_REQUIRE(N > 0 && N % 16 == 0 && K > 0 && K % 128 == 0, PC_ERR_ARG, "pc_w4_expand: need N%%16==0 and K%%128==0 (N=%d, K=%d)", N, K);
    const bool rowmajor = a->layout == PC_W4_EXPAND_ROWMAJOR;
    PC_REQUIRE(!rowmajor || (a->ld_out >= K && a->ld_out % 8 == 0), PC_ERR_ARG,
               "pc_w4_expand: the row-major layout needs ld_out >= K and ld_out %% 8 == 0 (ld_out=%lld, K=%d)", (long long)a->ld_out, K);
    PC_REQUIRE(a->codes && a->scales && a->out, PC_ERR_ARG, "pc_w4_expand: null codes, scales or out");
    PC_REQUIRE((((uintptr_t)a->codes | (uintptr_t)a->scales | (uintptr_t)a->out) & 15) == 0, PC_ERR_ARG,
               "pc_w4_expand: codes, scales and out must be 16-byte aligned");
    PC_REQUIRE(((uintptr_t)a->row_perm & 3) == 0, PC_ERR_ARG, "pc_w4_expand: row_perm must be 4-byte aligned");
    const int ntiles = N / 16, KQ = K / 128;
    const int64_t units = (int64_t)ntiles * KQ;
    const int64_t want = (units + kExpandWaves - 1) / kExpandWaves;
    const int blocks = (int)(want < kExpandMaxBlocks ? want : kExpandMaxBlocks);
    hipLaunchKernelGGL(w4_expand_kernel, dim3(blocks), dim3(kExpandThreads), 0, (hipStream_t)stream, (const unsigned char*)a->codes,
                       (const uint32_t*)a->scales, a->row_perm, (_Float16*)a->out, ntiles, KQ, rowmajor ? a->ld_out : (int64_t)0,
                       rowmajor ? 1 : 0);
    return pc_check_launch("w4_expand_kernel");
}
