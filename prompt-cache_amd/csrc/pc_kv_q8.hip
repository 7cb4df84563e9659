// Int8 module KV store: the quantiser (fp16 segment store -> byte image) and the dequantising gather (images -> fp16 staged
// rows), the int8 counterpart of kv_copy_kernel (pc_gather.hip).
//
// Replaces  PromptCache.update      promptcache/cache_engine.py:135-151  (pc_kv_gather_q8: the copy loop, with the module KV
//                                                                         held at 0.516 of its fp16 bytes)
//           SchemaCache._process    promptcache/cache_engine.py:283-296  (pc_kv_quant_q8: what is kept of a stored slice;
//                                                                         pc_kv_quant_q8_rows: the same rows out of an arena
//                                                                         whose planes are `cap` rows apart)
//
// Image of one segment of n rows, P = n_layers * 2 * n_kv_heads planes, head dim D -- ONE contiguous byte run:
//   int8  codes [P][n][D]      plane p = (layer * 2 + k|v) * n_kv_heads + head      (the fp16 store's plane order)
//   fp32  scale [P][n]         starts at byte P*n*D
// P*n*(D+4) bytes against the fp16 store's P*n*2D.
//
// Quantisation of one (plane, row) from its D fp16 values x, every step in fp32, round to nearest even, nothing contracted
// (no step is a multiply followed by an add, so there is nothing for the compiler to fuse):
//   s     = max |x|                       (exact)
//   inv   = 127.0f / s     (s == 0: 0)
//   code  = (int8) rintf(x * inv)         |code| <= 127
//   scale = s / 127.0f
//   deq   = fp16_rn((float) code * scale)
// A row that holds a NaN or an infinity stores scale = NaN and codes 0: it dequantises to NaN (tests/kv_q8_ref.py restates
// all of this in numpy, bit for bit).
//
// The gather is bandwidth-bound and nothing else (link-bound when the images lie in pinned host memory): per staged row and
// plane it reads D + 4 bytes and writes 2D.  An image is plane-major with a plane's rows back to back, so its P*n (plane, row)
// pairs are ONE flat run of rows on the source side -- codes at g*D, scale at g -- whatever the segment's length; only the
// destination knows planes (p = g / n, r = g % n).  A wave takes kRun * 64/(D/16) consecutive flat rows per pass: kRun
// independent 16-byte code loads per lane, each wave-instruction reading 1 KiB contiguous (what a PCIe read wants: the first
// form of this kernel gave every 8-lane group its own row run, 128-byte pieces 1 KiB apart per instruction, and reached 42 GB/s
// from pinned memory where kv_copy_kernel reaches 55.6), the pass's scales as one contiguous run (one coalesced dword per lane,
// handed to the lanes of its row by a cross-lane read -- not one load per row), all issued before the first use; every code
// load becomes two 16-byte stores.  Plain stores: the attention that follows re-reads the staged rows, and plain stores keep
// the lines in L2 (kv_copy_kernel measured non-temporal stores slower inside the real step for the same reason).  The 1-token
// segments between PML tags cost nothing special: their 2048 flat rows are four workgroups.
#include "pc_common.h"
#include "pc_kv_q8_quant.h"

namespace {

constexpr int kQ8MaxSeg = 40;        // descriptors per launch (kernarg-resident, 32 B each)
constexpr int kQ8Threads = 256;
constexpr int kRun = 8;              // 16-byte code loads in flight per lane and pass
constexpr int kPasses = 2;           // passes per workgroup

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

struct Q8Seg {
    const char* src;          // image
    char* dst;                // staged buffer + dst_row * D * 2
    int32_t n;                // rows
    int32_t total;            // planes * n: flat rows of the image
    int32_t wg_start;         // first workgroup of this segment in the launch
    int32_t pad;
};

struct Q8GatherArgs {
    Q8Seg seg[kQ8MaxSeg];
    int32_t nseg;
    int32_t pad;
    int64_t dst_plane_stride; // bytes
};

// codes k*2 and k*2+1 of the dword (k = 0, 1) -> two fp16: the pinned fp32 product, then one rounding to fp16
__device__ __forceinline__ uint32_t deq_pair(uint32_t w, int k, float scale) {
    const int c0 = (int)(int8_t)(w >> (16 * k)), c1 = (int)(int8_t)(w >> (16 * k + 8));
    const h2 r = h2{(_Float16)__fmul_rn((float)c0, scale), (_Float16)__fmul_rn((float)c1, scale)};
    return __builtin_bit_cast(uint32_t, r);
}

// LG = log2(D / 16): lanes per row
template <int LG>
__global__ __launch_bounds__(kQ8Threads) void kv_gather_q8_kernel(const Q8GatherArgs a) {
    constexpr int D = 16 << LG;
    constexpr int kRowsPerInst = 64 >> LG;                  // rows one wave-wide code load covers
    constexpr int kWaveRows = kRun * kRowsPerInst;          // flat rows per wave and pass
    constexpr int kScaleLoads = (kWaveRows + 63) / 64;      // coalesced dword loads that fetch the pass's scale run
    const int wg = blockIdx.x;
    int s = 0;                                              // wave-uniform scan of the kernarg table, as kv_copy_kernel
    for (int i = 1; i < a.nseg; ++i) s = (a.seg[i].wg_start <= wg) ? i : s;
    const Q8Seg d = a.seg[s];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & ((1 << LG) - 1), rl = lane >> LG;  // 16-code column block, row inside one wave-wide load
    const float* scale_base = (const float*)(d.src + (int64_t)d.total * D);

#pragma unroll 1
    for (int pass = 0; pass < kPasses; ++pass) {
        const int64_t base64 = ((int64_t)(wg - d.wg_start) * kPasses + pass) * (kQ8Threads / 64 * kWaveRows) + wave * kWaveRows;
        if (base64 >= d.total) break;                       // (wave-uniform)
        const int base = (int)base64;
        const int left = d.total - base;                    // flat rows from `base` on, > 0
        u32x4 v[kRun];
        float sc[kScaleLoads];
        const u32x4* cp = (const u32x4*)(d.src + (int64_t)base * D) + lane;
#pragma unroll
        for (int u = 0; u < kRun; ++u)
            if (u * kRowsPerInst + rl < left) v[u] = cp[u * 64];
#pragma unroll
        for (int k = 0; k < kScaleLoads; ++k) {
            const int t = k * 64 + lane;
            sc[k] = (t < kWaveRows && t < left) ? scale_base[base + t] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kRun; ++u) {
            const int t = u * kRowsPerInst + rl;            // this lane's flat row inside the pass
            const float scale = __shfl(sc[(u * kRowsPerInst) >> 6], t & 63);   // (executed by every lane of the wave)
            if (t < left) {
                const int g = base + t;
                const int p = g / d.n, r = g - p * d.n;
                u32x4 lo, hi;
                lo[0] = deq_pair(v[u][0], 0, scale); lo[1] = deq_pair(v[u][0], 1, scale);
                lo[2] = deq_pair(v[u][1], 0, scale); lo[3] = deq_pair(v[u][1], 1, scale);
                hi[0] = deq_pair(v[u][2], 0, scale); hi[1] = deq_pair(v[u][2], 1, scale);
                hi[2] = deq_pair(v[u][3], 0, scale); hi[3] = deq_pair(v[u][3], 1, scale);
                u32x4* o = (u32x4*)(d.dst + (int64_t)p * a.dst_plane_stride + ((int64_t)r * D + j * 16) * 2);
                o[0] = lo;
                o[1] = hi;
            }
        }
    }
}

// ---- quantiser: one lane per 16 values (two 16-byte loads, one 16-byte code store), a row's D/16 lanes reduce its maximum with
// cross-lane swaps (pcq::quant_row16); rows are numbered plane-major over the n_rows quantised rows of every plane, g = p * n_rows
// + r.  Source planes lie src_plane_rows rows apart and image planes dst_plane_rows (pc_kv_quant_q8_rows: an arena of `cap` rows
// into an image of `qcap`); with both equal to n_rows (pc_kv_quant_q8) row g is row g on both sides and nothing is divided.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(kQ8Threads) void kv_quant_q8_kernel(const _Float16* __restrict__ src, int64_t total_rows, int n_rows,
                                                                 int64_t src_plane_rows, int64_t dst_plane_rows, int head_dim,
                                                                 int lg_cpr, int8_t* __restrict__ codes, float* __restrict__ scale) {
    const int lg = lg_cpr;
    const int64_t row = ((int64_t)blockIdx.x * kQ8Threads + threadIdx.x) >> lg;
    const int j = threadIdx.x & ((1 << lg) - 1);
    const bool live = row < total_rows;                     // (whole rows drop out together: a row's lanes share one wave)
    int64_t srow = row, drow = row;
    if (src_plane_rows != n_rows || dst_plane_rows != n_rows) {   // (uniform over the grid)
        const int64_t p = row / n_rows, r = row - p * n_rows;
        srow = p * src_plane_rows + r;
        drow = p * dst_plane_rows + r;
    }
    float x[16];
    if (live) {
        const h8* p = (const h8*)(src + srow * head_dim + j * 16);
        const h8 a0 = p[0], a1 = p[1];
#pragma unroll
        for (int i = 0; i < 8; ++i) { x[i] = (float)a0[i]; x[8 + i] = (float)a1[i]; }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) x[i] = 0.0f;
    }
    uint32_t w[4];
    float sc;
    pcq::quant_row16(x, lg, w, sc);
    if (!live) return;
    *(u32x4*)(codes + drow * head_dim + j * 16) = u32x4{w[0], w[1], w[2], w[3]};
    if (j == 0) scale[drow] = sc;
}

int lg_lanes_per_row(int head_dim) {
    switch (head_dim) {
        case 32: return 1; case 64: return 2; case 128: return 3;
        default: return -1;
    }
}

}  // namespace

PC_EXPORT int pc_kv_quant_q8_rows(const void* src, int32_t src_plane_rows, int32_t n_rows, int32_t n_planes, int32_t head_dim,
                                  void* dst_image, int32_t dst_plane_rows, void* stream) {
    PC_REQUIRE(n_rows >= 0 && n_planes > 0 && src_plane_rows >= n_rows && dst_plane_rows >= n_rows && dst_plane_rows >= 1, PC_ERR_ARG,
               "pc_kv_quant_q8_rows: bad sizes (0 <= n_rows <= src_plane_rows, dst_plane_rows; dst_plane_rows >= 1)");
    const int lg = lg_lanes_per_row(head_dim);
    PC_REQUIRE(lg >= 0, PC_ERR_ARG, "pc_kv_quant_q8_rows: head_dim must be 32, 64 or 128");
    if (n_rows == 0) return PC_OK;
    PC_REQUIRE(src && dst_image, PC_ERR_ARG, "pc_kv_quant_q8_rows: null pointer");
    PC_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst_image & 15) == 0, PC_ERR_ARG,
               "pc_kv_quant_q8_rows: pointers must be 16-byte aligned");
    const int64_t rows = (int64_t)n_planes * n_rows;
    const int64_t lanes = rows << lg;
    const int64_t blocks = (lanes + kQ8Threads - 1) / kQ8Threads;
    PC_REQUIRE(blocks < (1ll << 31), PC_ERR_ARG, "pc_kv_quant_q8_rows: segment too long");
    int8_t* codes = (int8_t*)dst_image;
    float* scale = (float*)(codes + (int64_t)n_planes * dst_plane_rows * head_dim);
    hipLaunchKernelGGL(kv_quant_q8_kernel, dim3((unsigned)blocks), dim3(kQ8Threads), 0, (hipStream_t)stream, (const _Float16*)src,
                       rows, n_rows, (int64_t)src_plane_rows, (int64_t)dst_plane_rows, head_dim, lg, codes, scale);
    return pc_check_launch("kv_quant_q8_kernel");
}

PC_EXPORT int pc_kv_quant_q8(const void* src, int32_t n_rows, int32_t n_planes, int32_t head_dim, void* dst_image, void* stream) {
    PC_REQUIRE(n_rows >= 0 && n_planes > 0, PC_ERR_ARG, "pc_kv_quant_q8: bad sizes");
    const int lg = lg_lanes_per_row(head_dim);
    PC_REQUIRE(lg >= 0, PC_ERR_ARG, "pc_kv_quant_q8: head_dim must be 32, 64 or 128");
    if (n_rows == 0) return PC_OK;
    PC_REQUIRE(src && dst_image, PC_ERR_ARG, "pc_kv_quant_q8: null pointer");
    PC_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst_image & 15) == 0, PC_ERR_ARG, "pc_kv_quant_q8: pointers must be 16-byte aligned");
    const int64_t rows = (int64_t)n_planes * n_rows;
    const int64_t lanes = rows << lg;
    const int64_t blocks = (lanes + kQ8Threads - 1) / kQ8Threads;
    PC_REQUIRE(blocks < (1ll << 31), PC_ERR_ARG, "pc_kv_quant_q8: segment too long");
    int8_t* codes = (int8_t*)dst_image;
    float* scale = (float*)(codes + rows * head_dim);
    hipLaunchKernelGGL(kv_quant_q8_kernel, dim3((unsigned)blocks), dim3(kQ8Threads), 0, (hipStream_t)stream, (const _Float16*)src,
                       rows, n_rows, (int64_t)n_rows, (int64_t)n_rows, head_dim, lg, codes, scale);   // both strides = n_rows
    return pc_check_launch("kv_quant_q8_kernel");
}

PC_EXPORT int pc_kv_gather_q8(const pc_kv_seg* segs, int32_t nseg, void* dst, int32_t n_layers, int32_t n_kv_heads,
                              int32_t head_dim, int32_t max_ctx, void* stream) {
    PC_REQUIRE(nseg >= 0 && n_layers > 0 && n_kv_heads > 0 && max_ctx > 0, PC_ERR_ARG, "pc_kv_gather_q8: bad sizes");
    const int lg = lg_lanes_per_row(head_dim);
    PC_REQUIRE(lg >= 0, PC_ERR_ARG, "pc_kv_gather_q8: head_dim must be 32, 64 or 128");
    if (nseg == 0) return PC_OK;
    PC_REQUIRE(segs && dst, PC_ERR_ARG, "pc_kv_gather_q8: null pointer");
    PC_REQUIRE(((uintptr_t)dst & 15) == 0, PC_ERR_ARG, "pc_kv_gather_q8: dst must be 16-byte aligned");
    const int planes = n_layers * 2 * n_kv_heads;
    const int wg_rows = kPasses * (kQ8Threads / 64) * kRun * (64 >> lg);   // flat rows one workgroup expands
    for (int s = 0; s < nseg; ++s) {                        // everything is checked before anything is launched
        PC_REQUIRE(segs[s].len >= 0 && segs[s].dst_row >= 0, PC_ERR_ARG, "pc_kv_gather_q8: negative segment field");
        PC_REQUIRE((int64_t)segs[s].dst_row + segs[s].len <= max_ctx, PC_ERR_BOUNDS,
                   "pc_kv_gather_q8: segment %d (row %d, len %d) exceeds max_ctx %d", s, segs[s].dst_row, segs[s].len, max_ctx);
        if (segs[s].len == 0) continue;
        PC_REQUIRE(segs[s].src != nullptr, PC_ERR_ARG, "pc_kv_gather_q8: null segment %d", s);
        PC_REQUIRE((int64_t)planes * segs[s].len < (1ll << 30), PC_ERR_ARG, "pc_kv_gather_q8: segment %d too long", s);
        PC_REQUIRE(((uintptr_t)segs[s].src & 15) == 0, PC_ERR_ARG, "pc_kv_gather_q8: segment %d image must be 16-byte aligned", s);
    }
    Q8GatherArgs a;
    a.pad = 0;
    a.dst_plane_stride = (int64_t)max_ctx * head_dim * 2;
    int n = 0;
    int64_t wgs = 0;
    for (int s = 0; s <= nseg; ++s) {
        if (s < nseg && segs[s].len > 0) {
            Q8Seg& d = a.seg[n++];
            d.src = (const char*)segs[s].src;
            d.dst = (char*)dst + (int64_t)segs[s].dst_row * head_dim * 2;
            d.n = segs[s].len;
            d.total = planes * segs[s].len;
            d.wg_start = (int32_t)wgs;
            d.pad = 0;
            wgs += (d.total + wg_rows - 1) / wg_rows;
        }
        if (n == kQ8MaxSeg || (s == nseg && n > 0)) {
            a.nseg = n;
            const dim3 grid((unsigned)wgs), block(kQ8Threads);
            if (lg == 1) hipLaunchKernelGGL(kv_gather_q8_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
            else if (lg == 2) hipLaunchKernelGGL(kv_gather_q8_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
            else hipLaunchKernelGGL(kv_gather_q8_kernel<3>, grid, block, 0, (hipStream_t)stream, a);
            const int rc = pc_check_launch("kv_gather_q8_kernel");
            if (rc != PC_OK) return rc;
            n = 0;
            wgs = 0;
        }
    }
    return PC_OK;
}
