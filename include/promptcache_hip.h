/*
 * promptcache_hip.h -- C-ABI of the MI355X-native prompt-cache prefill path (libpromptcache_hip.so).
 *
 * The reference (yale-sys/prompt-cache) is pure Python with no FFI; the seam this library sits
 * under is the `LanguageModel` adapter (promptcache/model/__init__.py:90-161) as consumed by
 * `CacheEngine` (promptcache/cache_engine.py:331-522) and `GenerationEngine`
 * (promptcache/generation_engine.py:61-209).  Each entry point below names the reference
 * op sequence (file:line) it replaces.  See INTEGRATION.md for the ctypes binding.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer owned by the caller (PyTorch-ROCm allocations);
 *     tables marked "host" are small host arrays read during the call;
 *   - `stream` is a hipStream_t passed as void*; nothing allocates, nothing synchronises, all
 *     launches are asynchronous on `stream` (hipGraph-capturable);
 *   - KV element type is IEEE fp16 (the reference stages KV as torch.half, cache_engine.py:105-106);
 *   - return 0 on success, a negative code on error; pc_last_error_string() describes the last
 *     error on the calling thread.
 */
#ifndef PROMPTCACHE_HIP_H
#define PROMPTCACHE_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PC_OK 0
#define PC_ERR_ARG (-1001)      /* bad argument (null pointer, unsupported head_dim, ...) */
#define PC_ERR_BOUNDS (-1002)   /* a segment / append would run past the destination capacity */
#define PC_ERR_WORKSPACE (-1003)/* workspace too small (query pc_attn_workspace_bytes) */
#define PC_ERR_HIP(e) (-(int)(e)) /* -hipError_t from a launch */

#define PC_ABI_VERSION 1

int pc_version(void);
const char* pc_last_error_string(void);

/* ---------------------------------------------------------------------------------------------
 * pc_kv_gather -- replaces PromptCache.update's copy loop, cache_engine.py:135-151
 *   (`tgt[:, st:ed, :].copy_(src)` x 2 x n_layers per segment) with ONE launch over a segment table.
 *
 *   seg_src[s]     device ptr to segment s's module KV, contiguous [n_layers][2][n_kv_heads][seg_len[s]][head_dim]
 *                  (index 0 of the "2" axis = K, 1 = V)                                    (host array)
 *   seg_len[s]     tokens in segment s                                                      (host array)
 *   seg_dst_off[s] first token row of segment s in the staged buffer                        (host array)
 *   dst            staged buffer [n_layers][2][n_kv_heads][max_ctx][head_dim] fp16 (cache_engine.py:104-107,
 *                  all layers in one allocation; layer i's K plane is the reference's device_cache[i][0])
 *   Segments with seg_dst_off + seg_len > max_ctx -> PC_ERR_BOUNDS (nothing is launched).
 * ------------------------------------------------------------------------------------------- */
int pc_kv_gather(const void* const* seg_src, const int32_t* seg_len, const int32_t* seg_dst_off,
                 int32_t nseg, void* dst, int32_t n_layers, int32_t n_kv_heads, int32_t head_dim,
                 int32_t max_ctx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * pc_kv_row_table -- the same staging plan as pc_kv_gather, expanded to ONE ENTRY PER STAGED ROW, for the attention
 *   that stages while it reads (pc_attn `gather_rows`): the first forward over a freshly assembled prompt then reads every
 *   key / value row from its module store and writes the staged row as it goes, so PromptCache.update's copy
 *   (cache_engine.py:135-151) and the attention's first read of the staged rows (llama2.py:361-388) move the K/V across the
 *   chip once -- read 1x + write 1x -- instead of read + write + read.
 *
 *   segs      DEVICE array of segment descriptors in staging order (dst_row ascending, rows of a segment contiguous):
 *             src = the segment's module KV [n_layers][2][n_kv_heads][len][head_dim] (as pc_kv_gather's seg_src)
 *   nseg_dev  DEVICE int32: number of descriptors (<= max_seg) -- both come out of the caller's packed per-call input
 *             block, so a captured hipGraph replays the expansion for every new prompt
 *   dst, max_ctx   the staged buffer of pc_kv_gather.  Rows [0, total_rows_dev[0]) that no segment covers (rows a previous
 *             prompt staged at the same place and this one keeps; rows the model itself appended) get an entry that points
 *             at the staged buffer itself with PC_KV_ROW_STAGED set: read in place, not written
 *   rows      out: max_ctx entries; entry r describes staged row r: `base` = address of its head_dim fp16 values in plane 0
 *             (layer 0, K, head 0) of its source, `plane_stride16` = distance between consecutive planes of that source in
 *             16-byte units (plane p = (layer * 2 + k|v) * n_kv_heads + head)
 * ------------------------------------------------------------------------------------------- */
typedef struct pc_kv_seg { const void* src; int32_t dst_row; int32_t len; } pc_kv_seg;
typedef struct pc_kv_row { uint64_t base; uint32_t plane_stride16; uint32_t flags; } pc_kv_row;
#define PC_KV_ROW_STAGED 1u   /* the row already lies in the staged buffer: the attention does not write it */
int pc_kv_row_table(const pc_kv_seg* segs, const int32_t* nseg_dev, int32_t max_seg, const int32_t* total_rows_dev,
                    const void* dst, int32_t n_kv_heads, int32_t head_dim, int32_t max_ctx, pc_kv_row* rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * pc_kv_slice_store -- replaces SchemaCache._process's slice-and-store, cache_engine.py:283-296
 *   (`k_cache[j, :, st:ed, :]` per layer per TokenSequence, then `.cpu()`): the module KV stays in HBM.
 *
 *   src            the encode pass's KV arena [n_layers][2][n_kv_heads][src_cap][head_dim] (one batch row)
 *   seg_src_off[s] first token row of segment s inside the arena (= position_ids.index(offset), :278)
 *   seg_dst[s]     device ptr to the segment store, contiguous [n_layers][2][n_kv_heads][seg_len[s]][head_dim]
 * ------------------------------------------------------------------------------------------- */
int pc_kv_slice_store(const void* src, int32_t src_cap, const int32_t* seg_src_off, const int32_t* seg_len,
                      void* const* seg_dst, int32_t nseg, int32_t n_layers, int32_t n_kv_heads,
                      int32_t head_dim, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Int8 module KV store (opt-in, CacheEngine(module_kv="int8")): a segment's module KV kept as ONE contiguous byte image
 *
 *     int8  codes [P][n][D]      P = n_layers * 2 * n_kv_heads planes in pc_kv_gather's plane order, n rows, D = head_dim
 *     fp32  scale [P][n]         starts at byte P*n*D (a multiple of 16)
 *
 *   P*n*(D+4) bytes against the fp16 store's P*n*2D (0.516 at D = 128).  One (plane, row) of D fp16 values x is quantised with
 *   every step in fp32, round to nearest even:  s = max|x|;  inv = 127.0f / s (0 when s == 0);  code = (int8) rintf(x * inv);
 *   scale = s / 127.0f;  and dequantised as  fp16_rn((float) code * scale).  A row holding a NaN or an infinity stores
 *   scale = NaN and codes 0, so it dequantises to NaN.  head_dim must be 32, 64 or 128; pointers 16-byte aligned.
 *
 * pc_kv_quant_q8 -- what SchemaCache._process keeps of a stored slice, cache_engine.py:283-296 (there: fp16 tensors moved to
 *   the CPU): the fp16 segment store [n_planes][n_rows][head_dim] (pc_kv_slice_store's seg_dst) -> its image.
 *
 * pc_kv_quant_q8_rows -- the same rows, cache_engine.py:283-296, out of a buffer whose planes lie further apart than the rows
 *   that are kept: rows [0, n_rows) of every plane of src [n_planes][src_plane_rows][head_dim] (a staged batch-1 arena:
 *   src_plane_rows = its capacity) -> rows [0, n_rows) of every plane of an image of dst_plane_rows rows per plane (codes
 *   [n_planes][dst_plane_rows][head_dim], scales at byte n_planes*dst_plane_rows*head_dim).  Image rows at and behind n_rows are
 *   not written.  The same kernel and the same bits as pc_kv_quant_q8, which is the case of both strides = n_rows.
 *   n_rows > src_plane_rows or > dst_plane_rows, dst_plane_rows < 1 -> PC_ERR_ARG.
 *
 * pc_kv_gather_q8 -- replaces PromptCache.update's copy loop, cache_engine.py:135-151, as pc_kv_gather does, for segments held
 *   as images: ONE launch over a segment table that writes dequantised fp16 rows into the staged buffer
 *   [n_layers][2][n_kv_heads][max_ctx][head_dim].
 *   segs      HOST array of nseg descriptors: src = the segment's image (HBM or pinned host memory, mixed freely),
 *             dst_row = its first staged row, len = its rows.  Rows that no segment covers are not written.
 *   A segment with dst_row + len > max_ctx -> PC_ERR_BOUNDS (nothing is launched).
 * ------------------------------------------------------------------------------------------- */
int pc_kv_quant_q8(const void* src, int32_t n_rows, int32_t n_planes, int32_t head_dim, void* dst_image, void* stream);
int pc_kv_quant_q8_rows(const void* src, int32_t src_plane_rows, int32_t n_rows, int32_t n_planes, int32_t head_dim,
                        void* dst_image, int32_t dst_plane_rows, void* stream);
int pc_kv_gather_q8(const pc_kv_seg* segs, int32_t nseg, void* dst, int32_t n_layers, int32_t n_kv_heads, int32_t head_dim,
                    int32_t max_ctx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * pc_rope_table -- replaces LlamaRotaryEmbedding's cos/sin table + the `cos[position_ids]` gather,
 *   llama2.py:129-147 and :204-207.  Only the rows the supplied position ids select are produced
 *   (fp32, angle = float(pos) * inv_freq, as the reference builds them before its dtype cast).
 *
 *   pos       int32 [n_tok]        position ids of the new tokens (arbitrary, gaps allowed)
 *   inv_freq  fp32  [head_dim/2]   theta^(-2i/D), computed by the caller exactly as llama2.py:121
 *   cs        fp32  [n_tok][head_dim/2][2]  (cos, sin) out
 * ------------------------------------------------------------------------------------------- */
int pc_rope_table(const int32_t* pos, const float* inv_freq, float* cs, int32_t n_tok, int32_t head_dim,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * pc_rope_append -- replaces apply_rotary_pos_emb (llama2.py:202-210) on q and k plus the
 *   `torch.cat([past, new], dim=2)` of llama2.py:361-364: rotated q goes to q_out (fp16), rotated k and
 *   v are written IN PLACE at token rows [past_len, past_len+q_len) of this layer's KV arena (the past
 *   is not re-copied).
 *
 *   q      [B][q_len][H][D] projection output, fp32 when in_is_f32 else fp16; token stride
 *          q_token_stride, batch stride q_batch_stride (elements of the input type)
 *   q_out  fp16 [B][q_len][H][D], strides qo_* (may alias q when the input is fp16: in-place rotation)
 *   q_out_lo  optional fp16 plane, same strides: fp16(q_rot - fp16(q_rot)), the low-order half of the
 *          split-precision q that pc_attn consumes in its small-q (HBM-bound) instantiation
 *   k_new  [B][q_len][Hkv][D] (pre-RoPE, same type as q), v_new likewise; strides kv_new_*
 *   k_arena, v_arena  fp16 [B][Hkv][cap][D]: head stride arena_head_stride, batch stride arena_batch_stride
 *   cs     from pc_rope_table, [B*q_len][D/2][2]
 *   past_len_dev: optional device int32*; when non-null the kernel reads past_len from it (graph replay)
 * ------------------------------------------------------------------------------------------- */
int pc_rope_append(const void* q, int64_t q_batch_stride, int64_t q_token_stride,
                   void* q_out, void* q_out_lo, int64_t qo_batch_stride, int64_t qo_token_stride,
                   const void* k_new, const void* v_new, int64_t kv_new_batch_stride, int64_t kv_new_token_stride,
                   void* k_arena, void* v_arena, int64_t arena_batch_stride, int64_t arena_head_stride,
                   const float* cs, int32_t B, int32_t H, int32_t Hkv, int32_t D, int32_t q_len,
                   int32_t past_len, int32_t cap, int32_t in_is_f32, const int32_t* past_len_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * pc_attn -- replaces llama2.py:368-398: repeat_kv, QK^T/sqrt(D), + mask, softmax(fp32), PV,
 *   transpose/reshape.  The mask of llama2.py:62-76 / :798-819 is implicit: new token i (input order)
 *   sees every staged key j < past_len and new keys past_len + i' with i' <= i.  fp32 softmax and
 *   accumulation, MFMA fp16 x fp16 -> fp32 for both contractions, flash-style (scores are never
 *   materialised), split over the KV axis when (heads x q-blocks) cannot fill the chip.
 *   ONE struct-taking entry point (rounds 1-2 exported pc_attn_fwd / _alibi / _ex / _var; they had no caller left and are
 *   gone since round 4).  Optional pointers are NULL when unused.
 *
 *   struct_bytes  sizeof(pc_attn_args) of the caller's header (ABI check)
 *   q, q_lo    fp16 [B][q_len][H][D], RoPE applied; q_lo: optional low-order plane (q = q_hi + q_lo: split precision)
 *   k, v       fp16 arena planes [B][Hkv][cap][D] holding past_len + q_len valid rows
 *   out, out_lo   fp16 [B][q_len][H*D] (token stride out_token_stride); out_lo: optional residual plane of out
 *   out_frag_hi / out_frag_lo   optional (both or neither; B*q_len <= 512): instead of `out`, the result as
 *              split-precision fragment planes [ceil(B*q_len/16)][H*D/32][64][8] consumed by pc_gemm (o_proj)
 *   workspace  >= pc_attn_workspace_bytes(...) bytes of device memory (split-KV partials)
 *   past_len_dev   optional device int32* (graph replay; `past_len` is then the upper bound that sizes the launch)
 *   past_lens  optional device int32[B]: ONE PAST LENGTH PER BATCH ROW (ragged-prefix batches of the schema encode: scaffold
 *              suffixes of different unions in one batch, each over its own trunk prefix -- the batched form of
 *              cache_engine.py:217-304's per-scaffold forwards); past_len = their maximum.  Batch row b attends to keys
 *              [0, past_lens[b]) plus the rows it appended, up to its own.  Excludes past_len_dev, ALiBi, fragment output;
 *              residual planes must be arena-shaped (lo_row0 = 0)
 *   key_pos, slopes_log2   the additive ALiBi term of the reference's MPT attention (promptcache/model/mpt.py:90-110 slopes,
 *              :160-175 bias gathered at the POSITION IDS of the keys): score[q][key] = q.k * softmax_scale + slope[h] *
 *              position_id[key] (the reference's extra -slope * max_pos is constant along a softmax row and drops out).
 *              key_pos: fp32 [B][key_pos_batch_stride] position id of every cached and new key, padded with anything finite
 *              up to a multiple of 64 entries past past_len + q_len, rows 16-byte aligned; slopes_log2: fp32 [H] = slope * log2 e
 *   k_lo, v_lo fp16 residuals of K / V rows from key index lo_row0 on ([B][Hkv][rows][D] with the lo strides; written by
 *              pc_rope_append_ex / pc_gemm): those rows enter the contractions in split precision, as in the reference's
 *              fp32 pass (llama2.py:361-388); staged rows (< lo_row0) are the fp16 values the reference stages
 *              (cache_engine.py:105-106).  lo_row0 = -1: "the rows of this pass" (= past_len, read from past_len_dev when
 *              given; passes of <= 32 rows then run one extra KV split whose workgroup computes the attention over the
 *              pass's own rows in fp32); -2: the residual tail starts at key past_len_dev[1] (decode steps)
 *   counters   optional: B * H uint32 words, ZERO before the first launch that sees them; every launch leaves them
 *              zero.  With them a pass of <= 16 query rows over a long staged cache is ONE launch: each workgroup writes its
 *              split-KV partial through to memory, arrives at its head's counter, and the last arriver merges the partials in
 *              split order (the result does not depend on the arrival order).  Without them the partials are merged by a
 *              second launch -- which measures no slower on MI355X, so since round 6 the PRODUCT library ignores
 *              `counters` (same bits, two launches) and only -DPC_DEV_SWEEPS builds carry the in-launch merge.  One launch at a
 *              time per workspace / counters.
 *   prefix_k, prefix_v   optional (with past_lens): a SHARED KEY PREFIX held somewhere else -- fp16 planes [Hkv][prefix rows][D]
 *              with head stride prefix_head_stride (one layer of the root scaffold's arena).  Batch row b then attends to
 *              prefix rows [0, past_lens[b]) followed by the rows of ITS pass, which `k` / `v` hold from row 0 on: a suffix
 *              batch of the schema encode reads the trunk in place instead of carrying a copy of it in every batch row.
 *              prefix_k_lo / prefix_v_lo: optional residual planes of the prefix rows (same strides); k_lo / v_lo then
 *              cover the pass's rows from their row 0 (lo_row0 = 0).  Many-row kernel only (q_lo given or q_len > 16)
 *   gather_rows, gather_k_plane, gather_v_plane   optional (B = 1; pc_attn_gather_ok says whether this launch shape takes
 *              it): STAGE WHILE READING.  Key row r < past_len is read from where gather_rows[r] (pc_kv_row_table) says it
 *              lies -- plane gather_k_plane + kv_head for K, gather_v_plane + kv_head for V: (layer * 2 + 0|1) * Hkv of this
 *              layer -- and, unless the entry carries PC_KV_ROW_STAGED, written to row r of `k` / `v`.  After the launch
 *              rows [0, past_len) of `k` / `v` hold exactly what pc_kv_gather would have left there.  Rows from past_len on
 *              (this pass's own) are read from `k` / `v` as always.  Implemented by the streaming kernel of <= 32-row passes
 *              (tail mode or >= 256 keys), the tail-mode 64-row kernel, and the ring kernel (33..512 split-precision rows, D = 128)
 *   defer_merge, nsplit_out   optional (B = 1, no counters): a launch of <= 16 query rows that splits the keys (2..8 splits) LEAVES
 *              its partials for a consumer that merges them in its own prologue (pc_gemm_q8 part_o: the o_proj of an LLM.int8
 *              decode step) instead of running the merge launch: part_o fp32 [H * nsplit * q_len][D] at the start of the
 *              workspace, part_ml (running maximum in log2 units, denominator) [H * nsplit * q_len][2] right behind;
 *              slot = (h * nsplit + split) * q_len + row.  *nsplit_out (a HOST word, written before pc_attn returns) = the
 *              partials per row, or 1 when this launch shape merged as usual and the output planes are final
 * ------------------------------------------------------------------------------------------- */
int64_t pc_attn_workspace_bytes(int32_t B, int32_t H, int32_t D, int32_t q_len, int32_t kv_len_max);

typedef struct pc_attn_args {
    uint32_t struct_bytes;
    const void* q; const void* q_lo; int64_t q_batch_stride, q_token_stride;
    const void* k; const void* v; int64_t kv_batch_stride, kv_head_stride;
    void* out; void* out_lo; int64_t out_batch_stride, out_token_stride;
    void* out_frag_hi; void* out_frag_lo;
    int32_t B, H, Hkv, D, q_len, past_len;
    float softmax_scale;
    void* workspace; int64_t workspace_bytes;
    const int32_t* past_len_dev;
    const int32_t* past_lens;
    const float* key_pos; int64_t key_pos_batch_stride; const float* slopes_log2;
    const void* k_lo; const void* v_lo; int64_t lo_batch_stride, lo_head_stride; int32_t lo_row0;
    uint32_t* counters;
    const void* prefix_k; const void* prefix_v; const void* prefix_k_lo; const void* prefix_v_lo; int64_t prefix_head_stride;
    const pc_kv_row* gather_rows; int32_t gather_k_plane, gather_v_plane;
    int32_t defer_merge; int32_t* nsplit_out;
} pc_attn_args;
int pc_attn(const pc_attn_args* args, void* stream);
/* 1 when pc_attn would run `args` (gather_rows ignored) on a kernel that implements gather_rows, else 0 */
int pc_attn_gather_ok(const pc_attn_args* args);

/* ---------------------------------------------------------------------------------------------
 * Elementwise / reduction pieces of the layer stack, fused for the small-q prefill (q_len rows):
 *   pc_rmsnorm      -- LlamaRMSNorm.forward, llama2.py:103-108 (fp32 statistics)
 *   pc_silu_mul     -- act_fn(gate) * up of LlamaMLP.forward, llama2.py:242 (gate_up: [rows][2*inter], fp32 or fp16)
 *   pc_embed_gather -- embed_tokens lookup, llama2.py:869
 * ------------------------------------------------------------------------------------------- */
int pc_rmsnorm(const void* x, const void* weight, void* out, int32_t rows, int32_t hidden, float eps,
               int32_t x_is_f32, void* stream);
int pc_silu_mul(const void* gate_up, void* out, int32_t rows, int32_t inter, int32_t in_is_f32, void* stream);
int pc_embed_gather(const void* table, const int64_t* ids, void* out, int32_t n_tok, int32_t hidden,
                    int32_t vocab, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight-streaming projections for the small-q regime (M = B*q_len <= 512), csrc/pc_gemm*.hip: ONE entry point, pc_gemm.
 *   M <= 64:  eight waves split K over the same output tiles; split-precision (hi + lo) activations.
 *   M <= 512: the waves split the rows, weight tiles are staged through LDS by dedicated waves (hi + lo planes when both given).
 *
 * Fragment-major layouts (register image of mfma_f32_16x16x32_f16 operands, fp16):
 *   weights      Wf[N/16][K/32][64][8]   lane l = 16*g + n  holds W[16*tile + n][32*ks + 8*g .. +8]
 *                (W is the nn.Linear [N][K] matrix; build once at load: view(N/16,16,K/32,4,8).permute(0,2,3,1,4))
 *   activations  Xf[M/16 rounded up][K/32][64][8]   lane l = 16*g + m  holds X[16*mt + m][32*ks + 8*g .. +8]
 *                two planes: hi = fp16(x), lo = fp16(x - hi)  (lo may be NULL: single-precision pass)
 *
 * pc_gemm replaces the nn.Linear calls of llama2.py:345-347 (q|k|v fused), :405 (+ residual add :638), :242 (gate/up +
 *   SiLU*up; down + residual add :644) and :1050 (lm_head) when M <= 512.  Fields of pc_gemm_args (NULL / 0 when unused):
 *   struct_bytes  sizeof(pc_gemm_args) of the caller's header (ABI check)
 *   epilogue   PC_GEMM_EPI_STORE     y[m][n]  = sum_k X[m][k] W[n][k]   fp32 [M][ldy]; kslices > 1: the K axis is also split
 *                                    across workgroups, slice s writes its partial sums to y + s*M*ldy (slabs [kslices][M][ldy];
 *                                    pc_rmsnorm_frag adds them to the residual stream in fixed order)
 *              PC_GEMM_EPI_ADD       y[m][n] += ...   fp32 residual stream, in place.  With ks_counters (M <= 32, fp16 weights;
 *                                    17..32 rows: ks_tiles 1, 2 or 4 and twice the scratch bytes):
 *                                    K is cut into `kslices` (1..8) slices that run as separate workgroups of `ks_tiles`
 *                                    (1, 2, 4, 8) output tiles each, and the partial tiles are added INSIDE the launch -- every
 *                                    workgroup writes its partial through to ks_scratch (>= pc_gemm_skinny_ks_scratch_bytes(N,
 *                                    kslices) bytes, 16-byte aligned), arrives at its tile group's counter, the last arriver adds
 *                                    the partials in slice order (deterministic), adds y and stores.  ks_counters: ceil(N/16/
 *                                    ks_tiles) uint32 words, ZERO before the first launch; every launch leaves them zero
 *              PC_GEMM_EPI_SILU      W = [gate ; up] (N = 2*inter): of[m][j] = silu(gate_j) * up_j as fragment planes
 *                                    [M/16][inter/32][64][8] (of_hi, of_lo) for the down projection
 *              PC_GEMM_EPI_GELU      of[m][n] = gelu(...) as fragment planes (Falcon / MPT MLP, falcon.py:726)
 *              PC_GEMM_EPI_QKV_ROPE  the fused q|k|v projection: llama2.py:345-347 (projections), :357-359 (RoPE at the
 *                                    supplied position ids) and :361-364 (KV concat) in ONE launch; N = (H + 2 Hkv) D, M = B q_len.
 *                                    wf: fragment image of the row-PERMUTED [q;k;v] weight: inside every head, tile j (16 rows)
 *                                    holds features 8j..8j+7 followed by their rotary partners D/2+8j..D/2+8j+7.  Outputs:
 *                                    rotated q as split planes q_hi/q_lo [B*q_len][H*D] (token stride q_token_stride); rotated k
 *                                    and v in place at rows [past_len, past_len+q_len) of the arena planes (cs: pc_rope_table);
 *                                    k_lo / v_lo (both or NULL): fp16 residuals of those new rows; the residual row of token tt
 *                                    is tt (lo_base -1: a buffer of this pass's rows), past_len + tt - lo_base (>= 0) or
 *                                    past_len + tt - past_len_dev[1] (-2: ONE residual tail per layer across a prefill and the
 *                                    decode steps after it; llama2.py:361-388 keeps those rows in fp32 for the whole generation)
 *   wf, w_scale   fp16 fragment image; or (w_scale != NULL, M <= 64, K % 64 == 0) an INT8 image [N/16][K/64][64][16] of
 *              offset-binary bytes (q + 128; a lane's 16 bytes = its 8 values of k-step 2s then of 2s + 1) with w_scale fp32 [N]
 *              (row order of the image, 16-byte aligned): q[n][k] = round(w / scale[n]), scale[n] = absmax_k |w[n][k]| / 127 --
 *              the row-wise quantiser LLM.int8 applies to weights (the reference's GPU configs pass load_in_8bit=True,
 *              config/llm_config_*.json:5, eval.py:36-42); y = scale[n] * sum_k q[n][k] x[k]
 *   xf_hi, xf_lo  activation planes; OR
 *   x, norm_weight, eps   (M <= 16, K <= 16384; epilogues STORE / SILU / QKV_ROPE) the fp32 residual stream x [M][K] itself:
 *              y = W . (norm_weight * x) * rsqrt(mean(x^2) + eps) -- LlamaRMSNorm (llama2.py:103-108) folded into the projection
 *              that consumes it, no launch and no pass over x of its own.  Needs |norm_weight * x| < 65504
 *   rows_dev   optional device int32*: the rows that really carry tokens (<= M; B = 1).  Rows behind it are pad rows of a
 *              row-bucketed hipGraph: their results are unspecified and their activations are not loaded
 *   x_scale, corr, ldc, corr_has   LLM.int8 activations (pc_quant_act_i8): the planes hold int8 CODES, x_scale[m] = SCA[m] / 127;
 *              y = (sum_k code_w code_x) * w_scale[n] * x_scale[m] (+ corr[m][n] when *corr_has: pc_outlier_corr); OR
 *              The products run on the int8 MFMA (v_mfma_i32_16x16x64_i8, int32 sums: igemmlt's arithmetic, exact for any K).
 *   x_codes8   (optional, with x_scale, M <= 64) the codes as the int8 operand image pc_quant_act_i8 / pc_rmsnorm_quant_i8 write
 *              next to the fp16 codes plane: the K loop then reads it instead of xf_hi (half the activation bytes, no packing)
 *   row_max_out, flags_out, out_threshold   (PC_GEMM_EPI_SILU, M <= 16) what pc_gemm_q8's down_proj form reads instead of running a
 *              quantiser launch: per output pair-tile and row the largest |fp16 value| below out_threshold, [N/32][16] floats, and one
 *              flag byte per intermediate feature holding an entry at or above it (set-only: the buffer must be zero)
 *   flags, x_raw, w_codes_t, ldt, row_perm   the outlier correction computed INSIDE the launch (M <= 64): the flag bytes of
 *              pc_quant_act_i8 (>= 16384 bytes, zero behind K), the fp16 activations (fragment plane), the transposed int8 weight
 *              codes [K][ldt] (original row order) and, for q|k|v, the image-row -> original-row permutation
 * ------------------------------------------------------------------------------------------- */
#define PC_GEMM_EPI_STORE 0
#define PC_GEMM_EPI_ADD 1
#define PC_GEMM_EPI_SILU 2
#define PC_GEMM_EPI_QKV_ROPE 3
#define PC_GEMM_EPI_GELU 4
typedef struct pc_gemm_args {
    uint32_t struct_bytes;
    int32_t epilogue;
    const void* wf; const float* w_scale;
    const void* xf_hi; const void* xf_lo;
    const float* x; const void* norm_weight; float eps;
    int32_t M, N, K;
    const int32_t* rows_dev;
    float* y; int64_t ldy; void* of_hi; void* of_lo;
    int32_t kslices;
    int32_t ks_tiles; void* ks_scratch; int64_t ks_scratch_bytes; void* ks_counters;
    const float* x_scale; const float* corr; int64_t ldc; const int32_t* corr_has;
    const void* flags; const void* x_raw; const void* w_codes_t; int64_t ldt; const int32_t* row_perm;
    const float* cs; void* q_hi; void* q_lo; int64_t q_token_stride; void* k_arena; void* v_arena;
    int64_t arena_batch_stride, arena_head_stride;
    int32_t B, H, Hkv, D, q_len, past_len, cap;
    const int32_t* past_len_dev; void* k_lo; void* v_lo; int64_t lo_batch_stride, lo_head_stride; int32_t lo_base;
    const void* x_codes8;
    float* row_max_out; void* flags_out; float out_threshold;
} pc_gemm_args;
int pc_gemm(const pc_gemm_args* args, void* stream);
int64_t pc_gemm_skinny_ks_scratch_bytes(int32_t N, int32_t kslices);
/* pc_gemm_part -- o_proj + residual (llama2.py:405, :638) of a ONE-ROW forward (a decode step) on the attention's split-KV
 *   PARTIALS: y[0][n] += sum_k merged[k] W[n][k], where merged = the H * D values attn_combine_kernel would have produced from
 *   part_o / part_ml (pc_attn with defer_merge: nsplit = *nsplit_out in 2..8, layout there), split into fp16 hi + lo as pc_attn's
 *   fragment planes hold them.  wf: the fp16 fragment image of W [N][K = H * D <= 4096].  Bit-identical to pc_attn + its merge
 *   launch + pc_gemm(PC_GEMM_EPI_ADD) on the merged planes; one launch less per layer and decode step (csrc/pc_gemm_part.hip). */
int pc_gemm_part(const void* wf, const float* part_o, const float* part_ml, int32_t nsplit, int32_t H, int32_t D, int32_t N, float* y,
                 void* stream);
/* pc_gemm_q8 -- LLM.int8 projection of M <= 16 rows with the vector-wise activation quantiser INSIDE the launch
 *   (csrc/pc_gemm_q8.h).  Same arithmetic as pc_rmsnorm_quant_i8 / pc_quant_act_i8 followed by pc_gemm with x_scale + flags
 *   (bitsandbytes Linear8bitLt as demo.py:27-29 loads it; llama2.py:345-347, :405, :242 are the projections), without the
 *   quantiser launches: codes, row scales and outlier flags are derived by every workgroup of the projection itself.
 *   wf, w_scale, w_codes_t, ldt, row_perm   the int8 weight image, its scales, the transposed codes (outlier correction) and, for
 *              q|k|v, the image-row -> original-row permutation: as in pc_gemm_args
 *   threshold  the outlier threshold (6.0; <= 0: no outlier columns)
 *   source     (x, norm_weight, eps): the fp32 residual stream, RMSNorm folded in (epilogues QKV_ROPE, SILU), K <= 6144; or
 *              xf_hi: the fp16 activations as a fragment plane [1][K/32][64][8] (epilogues ADD, STORE), K <= 6144; or
 *              xf_hi + row_max [row_max_units][16] + flags_in [>= 16384 bytes, zero behind K] (epilogue ADD, any K <= 16384):
 *              the producer already left the per-tile row maxima and the outlier-column flags (row_max_out / flags_out of the
 *              launch with the SiLU epilogue); K is then cut into kslices (1..8) workgroup slices of ks_tiles (2, 4, 8) output
 *              tiles with the reduction inside the launch (ks_scratch >= pc_gemm_skinny_ks_scratch_bytes(N, kslices), ks_counters:
 *              ceil(N/16/ks_tiles) zeroed uint32 words; as PC_GEMM_EPI_ADD with ks_counters in pc_gemm).  M <= 4 with kslices = 1
 *              and ks_tiles 1 or 2 (decode): the rows' codes are staged once in LDS, every workgroup keeps all of K, no scratch
 *              part_o, part_ml, part_nsplit, part_head_dim (epilogue ADD, M = 1, K = H * part_head_dim <= 4096): the split-KV partials a
 *              pc_attn launch with defer_merge left (2..8 per row) -- the o_proj of a decode step merges them in its prologue
 *              with attn_combine_kernel's arithmetic (same bits), and the merge launch disappears
 *              xf_hi + x_codes8, x_scale, x_flags (epilogues QKV_ROPE, SILU, ADD; K <= 6144): what a quantiser launch left
 *              (pc_quant_act_i8 / pc_rmsnorm_quant_i8: fp16 plane, codes8 operand image, row scales, >= 16384 flag bytes) -- no quantiser
 *              arithmetic in this launch, but this file's K loop (image copied to LDS once, activation operands read from there, two
 *              weight blocks in flight); bit-identical to pc_gemm with x_scale + flags.  The form of 5..16 rows, where quantising all
 *              rows in every workgroup costs more than the launch
 *   outputs    y / ldy (STORE, ADD), of_hi (+ optional of_lo) fragment planes (SILU), the q|k|v fields (QKV_ROPE) as in pc_gemm_args
 *   row_max_out, flags_out   (SILU) per output pair-tile and row the largest |fp16 value| below the threshold, [N/32][16] floats, and
 *              one flag byte per intermediate feature holding an entry at or above it (set-only: the buffer must be zero)
 *   flags_clear, clear_bytes   a flag buffer this launch zeroes on the side (a multiple of 16 bytes) -- the o_proj launch clears
 *              the buffer the following SiLU launch sets; the down_proj form clears the first quantiser's of the next layer
 *   dbg_codes, dbg_scale, dbg_flags   (tests) workgroup 0 writes its operand image [K/64][64][16] int8, x_scale [M] and the K flag bytes */
typedef struct pc_gemm_q8_args {
    uint32_t struct_bytes;
    int32_t epilogue;
    const void* wf; const float* w_scale; const void* w_codes_t; int64_t ldt; const int32_t* row_perm;
    float threshold;
    const float* x; const void* norm_weight; float eps;
    const void* xf_hi;
    const float* row_max; int32_t row_max_units; const void* flags_in;
    int32_t M, N, K;
    float* y; int64_t ldy; void* of_hi; void* of_lo;
    float* row_max_out; void* flags_out;
    void* flags_clear; int32_t clear_bytes;
    int32_t kslices, ks_tiles; void* ks_scratch; int64_t ks_scratch_bytes; void* ks_counters;
    const float* cs; void* q_hi; void* q_lo; int64_t q_token_stride; void* k_arena; void* v_arena;
    int64_t arena_batch_stride, arena_head_stride;
    int32_t B, H, Hkv, D, q_len, past_len, cap;
    const int32_t* past_len_dev; void* k_lo; void* v_lo; int64_t lo_batch_stride, lo_head_stride; int32_t lo_base;
    void* dbg_codes; float* dbg_scale; void* dbg_flags;
    const float* part_o; const float* part_ml; int32_t part_nsplit, part_head_dim;
    const void* x_codes8; const float* x_scale; const void* x_flags;
} pc_gemm_q8_args;
int pc_gemm_q8(const pc_gemm_q8_args* args, void* stream);
/* pc_gemm_w4 -- the projections of M <= 16 rows over MXFP4 weight images (csrc/pc_gemm_w4.hip): OCP MX blocks of 32 consecutive
 *   input features of one output row, FP4 E2M1 codes (bits s e e m; codes 0..7 = 0, .5, 1, 1.5, 2, 3, 4, 6) under one E8M0 scale
 *   byte (2^(byte - 127), block exponent clamped to [-13, 13] so that every dequantised weight is an fp16 normal or zero).
 *   y[m][n] = sum_k (hi + lo)[m][k] W'[n][k] with W' the dequantised weight: pc_gemm's arithmetic on the fp16 image of W'.
 *   Needs K % 128 == 0, N % 16 == 0.  The two images (_native.to_weight_frags_w4 from the quantiser's [N][K/2] codes -- low
 *   nibble = lower feature -- and [N][K/32] scale bytes):
 *   codes      [N/16][K/128][64][16 B]: lane l = 16*g + m of tile t holds, for the QUAD s of k-steps, row 16*t + m's features
 *              128*s + 32*j + 8*g .. + 7 for j = 0..3, four bytes per j: one 16-byte load per lane feeds four k-steps
 *   scales     [N/16][K/128][16] dwords: byte j of the dword of row m is the E8M0 byte of k-step 4*s + j (the four lanes of a
 *              row read the same dword)
 *   epilogue   PC_GEMM_EPI_STORE, PC_GEMM_EPI_ADD (y / ldy), PC_GEMM_EPI_SILU (of_hi, of_lo) as in pc_gemm_args
 *   source     xf_hi + xf_lo (both), or (x, norm_weight, eps): the fp32 residual stream with RMSNorm folded in (STORE / SILU,
 *              K <= 16384), as in pc_gemm_args
 *   rows_dev   as in pc_gemm_args
 *              (rows in [*rows_dev, M) are computed from zero activations and stored, as pc_gemm does)
 *   The summation order is fixed and a row's result depends neither on M nor on the other rows (K is split eight ways inside
 *   a workgroup as a function of K alone, never across workgroups). */
typedef struct pc_gemm_w4_args {
    uint32_t struct_bytes;
    int32_t epilogue;
    const void* codes; const void* scales;
    const void* xf_hi; const void* xf_lo;
    const float* x; const void* norm_weight; float eps;
    int32_t M, N, K;
    const int32_t* rows_dev;
    float* y; int64_t ldy; void* of_hi; void* of_lo;
} pc_gemm_w4_args;
int pc_gemm_w4(const pc_gemm_w4_args* args, void* stream);
/* pc_gemm_w4_rows -- the same projections for 1 <= M <= 64 rows over the SAME two MXFP4 images (csrc/pc_gemm_w4_rows.hip): the
 *   form of the 17..64-row steps (a cached step with a 17..64-token question, the slot-lookup verify step of S * (k + 1) rows).
 *   y[m][n] = sum_k (hi + lo)[m][k] W'[n][k].  Needs K % 128 == 0, N % 16 == 0.
 *   xf_hi, xf_lo   the split-precision activation planes [ceil(M/16)][K/32][64][8] (both; rows behind M are never read)
 *   epilogue   PC_GEMM_EPI_STORE: y / ldy, fp32 row-major; K is cut into kslices (1..8) workgroup slices, slice s owns the quads
 *              of k-steps [s * ceil(K/128 / kslices), ...) and writes slab y + s * M * ldy (the slabs pc_rmsnorm_frag folds in fixed
 *              order; a slice that owns no quad writes zeros).  PC_GEMM_EPI_SILU (N = 2 * inter, N % 64 == 0, kslices = 1):
 *              of_hi / of_lo fragment planes [ceil(M/16)][inter/32][64][8], as in pc_gemm_args
 *   The summation order is fixed (a slice's quads split eight ways over the waves in ascending order as a function of (K, kslices)
 *   alone, k-steps ascending inside a wave, waves added in order 0..7; no atomics).  A row's result depends neither on M, nor on
 *   the other rows, nor on its row tile; at kslices = 1 it is bit-identical to pc_gemm_w4 on that row (planes source). */
typedef struct pc_gemm_w4_rows_args {
    uint32_t struct_bytes;
    int32_t epilogue;
    const void* codes; const void* scales;
    const void* xf_hi; const void* xf_lo;
    int32_t M, N, K, kslices;
    float* y; int64_t ldy; void* of_hi; void* of_lo;
} pc_gemm_w4_rows_args;
int pc_gemm_w4_rows(const pc_gemm_w4_rows_args* args, void* stream);
/* pc_w4_expand -- the fp16 weight W' from the two MXFP4 images of pc_gemm_w4 (csrc/pc_w4_expand.hip), exact: every grid value
 *   times 2^(byte - 127) with the byte in [114, 140] is an fp16 normal or zero.  A scale byte outside 114..140 is OUT OF
 *   CONTRACT (the quantiser never emits one; the result would round, overflow or go subnormal).  Needs N % 16 == 0, K % 128 == 0;
 *   codes, scales and out 16-byte aligned.
 *   layout     PC_W4_EXPAND_FRAG: out = the fragment image [N/16][K/32][64][8] of _native.to_weight_frags (what pc_gemm
 *              streams); ld_out is ignored.  PC_W4_EXPAND_ROWMAJOR: out = [N][ld_out] fp16 with ld_out >= K, ld_out % 8 == 0
 *              (what pc_gemm_dense reads); columns at and behind K are not written.
 *   row_perm   optional device int32[N] (NULL = identity): output row r holds source row row_perm[r] (the q|k|v fragment image
 *              is kept in qkv_rope_row_perm order).  An index outside [0, N) is out of contract. */
#define PC_W4_EXPAND_FRAG 0
#define PC_W4_EXPAND_ROWMAJOR 1
typedef struct pc_w4_expand_args {
    uint32_t struct_bytes;
    int32_t layout;
    int32_t N, K;
    const void* codes; const void* scales;
    const int32_t* row_perm;
    void* out; int64_t ld_out;
} pc_w4_expand_args;
int pc_w4_expand(const pc_w4_expand_args* args, void* stream);
/* pc_rmsnorm_frag -- LlamaRMSNorm (llama2.py:103-108) on the fp32 residual stream, output as fragment planes;
 *   optional prologue x += slabs[0] + ... + slabs[nslabs-1] (each [rows][hidden], the residual adds of
 *   llama2.py:638 / :644 fed by a K-sliced pc_gemm), written back to x in place. */
int pc_rmsnorm_frag(float* x, const void* weight, void* xf_hi, void* xf_lo, int32_t rows, int32_t hidden,
                    float eps, const float* slabs, int32_t nslabs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Falcon adapter (promptcache/model/falcon.py; multi-query, parallel attention + MLP): the ops the Llama path does
 * not have.  Everything else (pc_kv_gather with Hkv = 1, pc_rope_*, pc_attn with H/Hkv = H, pc_gemm*) is shared.
 *   pc_layernorm       torch.nn.LayerNorm (falcon.py:757, :1020) of fp32 x [rows][hidden] -> fp16
 *   pc_layernorm_frag  the same, written as split-precision fragment planes, with the slab-folding prologue of
 *                      pc_rmsnorm_frag (x += slabs[0] + ... first: the o_proj and dense_4h_to_h partial sums)
 *                      (bias may be NULL in both: MPT's LayerNorm carries no bias, mpt.py:207, :215)
 *   pc_gelu            nn.GELU() (falcon.py:726, mpt.py:187: erf form) fp32 -> fp16, n elements (n % 8 == 0)
 *   pc_gemm epilogue PC_GEMM_EPI_GELU: of[m][j] = gelu(y[m][j]) as fragment planes [M/16][N/32][64][8] (dense_h_to_4h)
 * ------------------------------------------------------------------------------------------- */
int pc_layernorm(const float* x, const void* weight, const void* bias, void* out, int32_t rows, int32_t hidden,
                 float eps, void* stream);
int pc_layernorm_frag(float* x, const void* weight, const void* bias, void* xf_hi, void* xf_lo, int32_t rows,
                      int32_t hidden, float eps, const float* slabs, int32_t nslabs, void* stream);
int pc_gelu(const float* x, void* out, int64_t n, void* stream);


/* Split-precision variants for the dense (many-row) path.  fp16 activations cost 2^-11 per projection input; over 32
 * layers that alone moves 7b-shape logits by 2-3e-2 against the reference's fp32 path.  These write an activation as
 * hi = fp16(v) and lo = fp16(v - hi); the caller stacks [hi; lo] along the rows of one GEMM and adds the two halves of
 * the product (gate_up2 / x2 / pc_add3 take the second half):
 *   pc_rmsnorm_split, pc_layernorm_split   norm -> (hi, lo) [rows][hidden]
 *   pc_silu_mul_split   silu(g) * u of (gate_up + gate_up2) -> (hi, lo);  pc_gelu_split  gelu(x + x2) -> (hi, lo)
 *   pc_add3             x += a + b  (fp32 residual stream)
 *   (the attention takes the split planes through pc_attn: q_lo, out_lo, k_lo / v_lo) */
int pc_rmsnorm_split(const float* x, const void* weight, void* out_hi, void* out_lo, int32_t rows, int32_t hidden,
                     float eps, void* stream);
int pc_layernorm_split(const float* x, const void* weight, const void* bias, void* out_hi, void* out_lo, int32_t rows,
                       int32_t hidden, float eps, void* stream);
int pc_silu_mul_split(const float* gate_up, const float* gate_up2, void* out_hi, void* out_lo, int32_t rows,
                      int32_t inter, void* stream);
int pc_gelu_split(const float* x, const float* x2, void* out_hi, void* out_lo, int64_t n, void* stream);
int pc_add3(float* x, const float* a, const float* b, int64_t n, void* stream);
/* pc_rope_append_ex -- pc_rope_append that also writes the fp16 residuals of the appended K / V rows (k_lo, v_lo,
 *   both or neither: [B][Hkv][rows][D] with the given strides, row = key index - lo_row0; lo_row0 = past_len for a
 *   compact buffer of the new rows, 0 for an arena-shaped one that also carries residuals of earlier rows; -1 / -2: the offset is
 *   read on the device, as pc_attn's lo_row0 is: the past length the launch appends behind / past_len_dev[1], the base of a
 *   residual tail -- what a captured graph needs, which replays at other past lengths).  pc_attn consumes them: the keys / values a pass appends enter
 *   (in2_offset != 0: every q / k_new / v_new input element is x[i] + x[i + in2_offset], the two row halves a stacked
 *   [hi; lo] projection leaves)
 *   its own attention in split precision, as in the reference's fp32 pass (llama2.py:361-388), while the arena keeps the
 *   fp16 value the reference stages (cache_engine.py:105-106).  Staged rows (< past_len) have no residual. */
int pc_rope_append_ex(const void* q, int64_t q_batch_stride, int64_t q_token_stride, void* q_out, void* q_out_lo,
                      int64_t qo_batch_stride, int64_t qo_token_stride, const void* k_new, const void* v_new,
                      int64_t kv_new_batch_stride, int64_t kv_new_token_stride, void* k_arena, void* v_arena,
                      int64_t arena_batch_stride, int64_t arena_head_stride, const float* cs, int32_t B, int32_t H,
                      int32_t Hkv, int32_t D, int32_t q_len, int32_t past_len, int32_t cap, int32_t in_is_f32,
                      const int32_t* past_len_dev, void* k_lo, void* v_lo, int64_t lo_batch_stride,
                      int64_t lo_head_stride, int32_t lo_row0, int64_t in2_offset, void* stream);


/* Ragged-prefix batches (schema encode: scaffold suffixes of different unions in one batch, each over its own trunk
 * prefix -- the batched form of cache_engine.py:217-304's per-scaffold forwards): pc_rope_append_ex (and pc_attn.past_lens) with
 * ONE PAST LENGTH PER BATCH ROW.  past_lens: device int32[B]; past_len = their maximum (bounds check, KV-split sizing).
 * Batch row b appends its q_len new rows at arena rows [past_lens[b], past_lens[b] + q_len) and attends to keys
 * [0, past_lens[b]) plus the new rows up to its own (index-order mask, llama2.py:62-76).  Residual planes, when given,
 * are arena-shaped (lo_row0 = 0). */
int pc_rope_append_var(const void* q, int64_t q_batch_stride, int64_t q_token_stride, void* q_out, void* q_out_lo,
                       int64_t qo_batch_stride, int64_t qo_token_stride, const void* k_new, const void* v_new,
                       int64_t kv_new_batch_stride, int64_t kv_new_token_stride, void* k_arena, void* v_arena,
                       int64_t arena_batch_stride, int64_t arena_head_stride, const float* cs, int32_t B, int32_t H,
                       int32_t Hkv, int32_t D, int32_t q_len, int32_t past_len, int32_t cap, int32_t in_is_f32,
                       const int32_t* past_lens, void* k_lo, void* v_lo, int64_t lo_batch_stride, int64_t lo_head_stride,
                       int32_t lo_row0, void* stream);




/* Many-row projection (schema encode / no-cache prefill / long questions; MFMA-bound), csrc/pc_gemm_dense.hip:
 *     acc[m][n] = sum_k (x_hi[m][k] + x_lo[m][k]) * w[n][k]        fp16 operands, fp32 accumulation
 * x_hi / x_lo: split-precision activation planes [M][K] (row stride ldx halfs; x_lo may be NULL), w: the nn.Linear
 * weight [N][K] (row stride ldw), w_scale: optional fp32 per-output-row scale (int8 codes held in fp16).
 * Replaces the nn.Linear calls of promptcache/model/llama2.py:345-347 (q|k|v), :405 (o_proj), :242 (gate / up / down),
 * :1050 (lm_head) -- and falcon.py:393-405,:726-731 / mpt.py -- for passes of many rows, together with the ops
 * that follow them:
 *   epilogue 0  y[m][n]  = acc                                   (fp32, row stride ldy)
 *   epilogue 1  y[m][n] += acc                                   residual add, llama2.py:638 / :644
 *   epilogue 2  out[m][j] = silu(acc[m][j]) * acc[m][N/2 + j]    w = [gate; up] rows, llama2.py:242; out_hi / out_lo
 *                                                                split-precision planes [M][N/2] (row stride ldo)
 *   epilogue 4  out[m][n] = gelu(acc)                            nn.GELU(), falcon.py:726; planes [M][N]
 * K % 8 == 0, N % 4 == 0; operands 16-byte aligned.  Returns 0 or a negative PC_ERR_* code. */
int pc_gemm_dense(const void* x_hi, const void* x_lo, int64_t ldx, const void* w, int64_t ldw, const float* w_scale,
                  int32_t M, int32_t N, int32_t K, int32_t epilogue, float* y, int64_t ldy, void* out_hi, void* out_lo,
                  int64_t ldo, void* stream);

/* The fused q|k|v projection of a many-row pass (head_dim 128): replaces llama2.py:345-347 (q / k / v projections), :357-359 (RoPE at the
 * supplied position ids) and :361-364 (KV concat) for schema-encode passes, no-cache prefill and long questions -- one launch,
 * no [M][(H + 2 Hkv) D] fp32 intermediate.
 *   x_hi, x_lo   fp16 [M = B*q_len][K] activation planes (x_lo may be NULL), row stride ldx
 *   w            fp16 [(H + 2 Hkv) * 128][K] = [q; k; v] weight rows as nn.Linear holds them (NOT permuted), row stride ldw
 *   cs           fp32 [M][64][2] (cos, sin) from pc_rope_table at the position id of every row
 *   q_hi, q_lo   rotated q as split planes fp16 [M][q_token_stride] (q_lo may be NULL)
 *   k_arena, v_arena   layer planes [B][Hkv][cap][128] with the arena strides: rotated k and v of batch row b land at rows
 *                past + t (past = past_lens[b] when given, else past_len)
 *   k_lo, v_lo   optional residual planes of those rows ([B][Hkv][rows][128] with the lo strides, row = past + t - lo_row0) */
typedef struct pc_dense_qkv_args {
    uint32_t struct_bytes;
    const void* x_hi; const void* x_lo; int64_t ldx;
    const void* w; int64_t ldw; int32_t K;
    const float* cs;
    void* q_hi; void* q_lo; int64_t q_token_stride;
    void* k_arena; void* v_arena; int64_t arena_batch_stride, arena_head_stride;
    void* k_lo; void* v_lo; int64_t lo_batch_stride, lo_head_stride; int32_t lo_row0;
    int32_t B, H, Hkv, D, q_len, past_len, cap;
    const int32_t* past_lens;
    /* optional (round 5, instead of x_lo): the residual plane as int8 codes + row scales against an int8 weight image + row
     * scales (dev builds only: csrc/pc_dev.h, pc_gemm_dense_lo8) */
    const void* x_lo8; const float* x_lo8_scale; int64_t ldx8;
    const void* w8; const float* w8_scale; int64_t ldw8;
} pc_dense_qkv_args;
int pc_gemm_dense_qkv_rope(const pc_dense_qkv_args* args, void* stream);

/* pc_gemm_dense with a caller-owned scratch buffer (16-byte aligned, workspace_bytes long).  A plain-store / residual-add
 * launch whose tile grid would leave most of the 256 CUs idle -- the N = hidden projections (llama2.py:405 o_proj, :242
 * down_proj) at a few hundred rows -- cuts K into up to 8 slices: partial slabs [slices][M][N] fp32 in the workspace, added
 * in slice order by a second launch (deterministic).  When the slabs do not fit, or the grid is large enough, the call is
 * exactly pc_gemm_dense. */
int pc_gemm_dense_ws(const void* x_hi, const void* x_lo, int64_t ldx, const void* w, int64_t ldw, const float* w_scale,
                     int32_t M, int32_t N, int32_t K, int32_t epilogue, float* y, int64_t ldy, void* out_hi, void* out_lo,
                     int64_t ldo, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- LLM.int8(): int8 weights AND int8 activations with the fp16 outlier decomposition -------------------------------
 * What load_in_8bit=True means in the reference's GPU runs (demo.py:27-29, eval.py:36-42, config/llm_config_*.json:5 ->
 * transformers -> bitsandbytes.nn.Linear8bitLt(threshold = 6.0)).  bitsandbytes is not part of the reference tree: these
 * entry points implement its published algorithm (Dettmers et al., NeurIPS 2022, section 3; csrc/pc_int8.hip; CPU
 * restatement oracle/llmint8_oracle.py) and replace, per decoder-layer nn.Linear, the call Linear8bitLt.forward makes.
 *
 * pc_quant_act_i8: x = fp16 activations, row-major [T][ldx] (frag = 0) or a fragment-major plane [T/16][K/32][64][8]
 *   (frag = 1; pc_gemm.hip).  Per row: entries |x| >= threshold are outliers (their column gets flags_set[k] = 1), the
 *   rest is quantised vector-wise: codes = round_half_even(x * 127 / absmax_row) as fp16 values in the layout of x,
 *   x_scale[t] = absmax_row / 127.  flags_clear (optional, clear_len bytes): zeroed for the next activation slot.
 * pc_outlier_corr: corr[t][n] = sum over flagged columns k of x[t][k] * fp16(w_codes[r][k] * w_scale[r])
 *   - codes[t][k] * w_codes[r][k] * x_scale[t] * w_scale[r],  r = row_perm ? row_perm[n] : n  (w_codes_t: the int8 weight
 *   codes TRANSPOSED, [K][ldt], so that a weight column is contiguous); *has = 1 when any column is flagged, else 0 and
 *   corr is left untouched.
 * pc_gemm (x_scale != NULL) / pc_gemm_dense_a8: the projections over the codes,
 *   y = (sum_k w_code[n][k] * x_code[m][k]) * w_scale[n] * x_scale[m] + (*corr_has ? corr[m][n] : 0), then the epilogue
 *   (same epilogue codes and outputs as with fp16 operands). */
int pc_quant_act_i8(const void* x, int64_t ldx, int32_t frag, int32_t T, int32_t K, void* codes, float* x_scale, void* flags_set,
                    void* flags_clear, int32_t clear_len, float threshold, void* codes8, void* stream);
/* codes8 (optional; K % 64 == 0, 16-byte aligned, ceil(T/16) * K * 16 bytes): the same codes as the int8 MFMA's operand image
 * [T/16][K/64][64][16] -- a lane's 16 signed bytes = its eight codes of k-step 2s, then of 2s + 1, the byte order of the int8
 * weight image -- for pc_gemm's x_codes8: the projection then loads half the activation bytes and converts nothing. */
/* (pc_gemm with `flags` computes the outlier correction INSIDE the projection launch, M <= 64: every workgroup compacts the flags
 * and its eight waves share the outlier columns; equal to pc_outlier_corr + the corr form up to the fp32 summation order over the
 * outlier columns.  Saves one launch per projection, ~4 us even when no column is flagged.) */
/* pc_rmsnorm_frag + pc_quant_act_i8 in one launch (T <= 64 rows, fragment planes), for the two projection inputs that come out of
 * an RMSNorm (input_layernorm -> q|k|v, post_attention_layernorm -> gate|up; llama2.py:628, :640): bit-identical to the pair.
 * x: fp32 residual stream [T][hidden]; x_hi: the normalised fp16 activations (read by pc_outlier_corr), codes / x_scale / flags as
 * pc_quant_act_i8. */
int pc_rmsnorm_quant_i8(const float* x, const void* norm_weight, float eps, int32_t T, int32_t hidden, void* x_hi, void* codes,
                        float* x_scale, void* flags_set, void* flags_clear, int32_t clear_len, float threshold, void* codes8,
                        void* stream);
int pc_outlier_corr(const void* flags, int32_t K, const void* x, const void* codes, int64_t ldx, int32_t frag,
                    const float* x_scale, const void* w_codes_t, int64_t ldt, const float* w_scale, const int32_t* row_perm,
                    int32_t T, int32_t N, float* corr, int64_t ldc, int32_t* has, void* stream);
int pc_gemm_dense_a8(const void* xq, int64_t ldx, const void* w_codes, int64_t ldw, const float* w_scale, const float* x_scale,
                     const float* corr, int64_t ldc, const int32_t* corr_has, int32_t M, int32_t N, int32_t K, int32_t epilogue,
                     float* y, int64_t ldy, void* out_hi, void* out_lo, int64_t ldo, void* stream);

/* pc_fetch_block -- replaces the per-call uploads `torch.tensor(ids, device=)` / `torch.tensor(position_ids, device=)` of
 * generation_engine.py:96-97 (and :125-132 for every decode step): the FIRST node of a captured forward pulls the call's whole
 * input block -- token ids, position ids, past length, staging plan -- out of one pinned (device-mapped) host buffer into device
 * memory; per call the host writes that buffer and replays the graph, nothing else.  host_src: pinned host memory (8-byte
 * aligned, read with system-scope loads); nbytes: multiple of 8, <= 1 MiB.  The host must not rewrite the buffer before the
 * replay that reads it has finished. */
int pc_fetch_block(const void* host_src, void* dst, int32_t nbytes, void* stream);

/* pc_prefill_prologue -- everything a captured small-q forward does before its first layer, as ONE launch reading the call's pinned
 * host block (layout: int64 ids[n_tok] | int32 pos[n_tok] at o_pos | int32 words[8] at o_words = {past_len, tail base, live rows,
 * segments, rows of the row table, ...} | pc_kv_seg[max_seg] at o_segs): the block copied to its device twin (pc_fetch_block), the
 * embedding rows of the tokens as the fp32 residual stream x_out [n_tok][hidden] (embed_tokens, llama2.py:869), the (cos, sin)
 * rows of the supplied positions cs_out [n_tok][head_dim/2][2] (pc_rope_table; llama2.py:129-147, :204-207) and -- when `rows` is
 * given -- the staging plan expanded per staged row (pc_kv_row_table; words[3] segments, words[4] rows).  words[5] != 0: the
 * caller's ids / positions are DEVICE tensors (the reference's convention, generation_engine.py:96-97) that it copied into the
 * ids | pos region of dev_block on `stream` before this launch -- they are read there and that region is not overwritten (no
 * host read-back of device inputs).  Replaces the uploads of generation_engine.py:96-97 and four small launches per forward. */
int pc_prefill_prologue(const void* host_block, void* dev_block, int32_t nbytes, int32_t n_tok, int32_t o_pos, int32_t o_words,
                        int32_t o_segs, int32_t max_seg, const void* embed_table, int32_t hidden, int32_t vocab, float* x_out,
                        const float* inv_freq, int32_t head_dim, float* cs_out, pc_kv_row* rows, const void* dst, int32_t max_ctx,
                        void* stream);

/* Greedy decode without a host round trip per token (generation_engine.py:123-168, greedy branch :159): the tail of a
 * captured decode step.  token = argmax(logits[0..vocab)) (lowest index among equal maxima); ids[0] = token, pos[0] += 1,
 * past_len[0] += 1 -- the device words the NEXT replay of the same hipGraph reads its token id, position id and past
 * length from -- and ring[counter % ring_cap] = token, counter += 1 for the host to collect tokens when it wants them. */
int pc_greedy_advance(const float* logits, int32_t vocab, int64_t* ids, int32_t* pos, int32_t* past_len, int32_t* ring,
                      int32_t* counter, int32_t ring_cap, void* stream);

/* Sampled decode without a host round trip per token: the sampled counterpart of pc_greedy_advance, the last node of a
 * captured decode step.  The reference's chain (generation_engine.py:32-42: temperature, repetition penalty, top-p, top-k,
 * in that order, with their thresholds) applied to logits[0..vocab) and the draw of :149-168 (greedy rule :159: argmax when
 * temperature < 1e-5 or top_p < 1e-8; otherwise one sample of softmax over the kept tokens, taken here as Gumbel-max with
 * Philox4x32-10 keyed by `seed`, counter (token / 4, *counter, 0, 0)).  The penalty applies to tokens whose bit is set in
 * history_bits (ceil(vocab / 32) words); the drawn token's bit is set.  Then exactly pc_greedy_advance's contract: ids[0] =
 * token, pos[0] += 1, past_len[0] += 1, ring[counter % ring_cap] = token, counter += 1.  The parameters live in device memory
 * so that one captured graph serves every parameter set.  processed_out (optional, [vocab] fp32): the processed row, filtered
 * tokens as -inf.  logits need only be 4-byte aligned; vocab < 2^24. */
typedef struct pc_sample_params {
    float temperature;
    float repetition_penalty;
    float top_p;
    int32_t top_k;               /* <= 0: off */
    uint64_t seed;
} pc_sample_params;

int pc_sample_advance(const float* logits, int32_t vocab, const pc_sample_params* params_dev, uint32_t* history_bits, int64_t* ids,
                      int32_t* pos, int32_t* past_len, int32_t* ring, int32_t* counter, int32_t ring_cap, float* processed_out,
                      void* stream);

/* ---- prompt-lookup speculative decoding (csrc/pc_lookup.hip) ---------------------------------------------------------------------
 * Greedy decoding with up to k + 1 tokens per forward: the two ends of a captured step whose middle is the ordinary forward of
 * rows = k + 1 <= 16 tokens read from ids / pos / past_len.  All state lives in DEVICE words, so a replay needs no host input:
 *   hist int32[hist_cap], hist_len int32[1]   every token of the sequence so far (corpus, prompt, output); hist[hist_len - 1]
 *                                             is the token the step feeds and equals ids[0]
 *   ids int64[k + 1], pos int32[k + 1]        the forward's inputs: row 0 the fed token, rows 1..k the drafts
 *   ndraft int32[1]                           how many of rows 1..k are real drafts (the rest are pads)
 *
 * pc_lookup_draft: with h = hist, L = hist_len: for n = min(nmax, L - 1) down to 1, the candidates are the j in [0, L - n - 1]
 * with h[j..j+n) == h[L-n..L); the LARGEST j of the first n that has one is taken.  m = min(k, L - (j + n)); ids[1 + i] =
 * h[j + n + i] for i < m and ids[0] for m <= i < k (pad rows embed a valid token); pos[i] = pos[0] + i; ndraft = m, or 0 without
 * a candidate.  1 <= k <= 15, 1 <= nmax <= 8, hist_cap < 2^24.  One workgroup; nothing else is written.
 *
 * pc_lookup_verify: logits fp32 [rows][vocab] with row stride ldl (elements; 4-byte alignment suffices).  a[i] = argmax of row
 * i, the lowest index among equal maxima (pc_greedy_advance's rule), left in row_argmax int32[rows] (scratch).  acc = the
 * largest c <= ndraft with a[i] == ids[1 + i] for all i < c; emit = min(acc + 1, budget[0]).  The record
 * ring[(counter % ring_cap) * (rows + 1) ..] gets {emit, a[0..emit)} and counter += 1; when emit > 0: hist[L..L+emit) =
 * a[0..emit), hist_len += emit, ids[0] = a[emit - 1], pos[0] += emit, past_len[0] += emit, budget[0] -= emit.  With budget[0] = 0
 * the record is {0} and nothing else changes, so replays past the end of a generation are harmless.  At rows = 1 (ndraft = 0)
 * the token and the ids / pos / past_len / counter words are pc_greedy_advance's.  Two launches: rows workgroups, then one wave. */
int pc_lookup_draft(const int32_t* hist, const int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* ndraft,
                    int32_t k, int32_t nmax, void* stream);
int pc_lookup_verify(const float* logits, int64_t ldl, int32_t vocab, int32_t rows, int32_t* row_argmax, int32_t* hist,
                     int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* past_len, const int32_t* ndraft,
                     int32_t* budget, int32_t* ring, int32_t* counter, int32_t ring_cap, void* stream);

/* pc_lookup_verify_sample -- pc_lookup_verify for SAMPLED generations (csrc/pc_sample.hip): a prompt-lookup draft is a point
 * mass, so verifying it needs no rejection-sampling residual -- only pc_sample_advance's draw on every row, with a random stream
 * per TOKEN.  d = draws[0], nd = ndraft[0].  For every row i <= nd, t[i] = pc_sample_advance's draw on logits row i (same chain,
 * thresholds, Gumbel-max and greedy rule, from the parameter block) with the random stream (params->seed, step d + i) under the
 * penalty history history_bits + {ids[1], ..., ids[i]}: the draw the one-token loop makes for that position when drafts 1..i
 * were emitted.  Rows i > nd are pads: never accepted, not drawn; their row_token / processed_out rows are unspecified.  acc =
 * the largest c <= nd with t[i] == ids[1 + i] for all i < c; emit = min(acc + 1, budget[0]).  The record
 * ring[(counter % ring_cap) * (rows + 1) ..] gets {emit, t[0..emit)} and counter += 1; when emit > 0, pc_lookup_verify's state
 * updates on hist / hist_len / ids[0] / pos[0] / past_len[0] / budget[0] (the hist_cap clamp included), draws[0] += emit and the
 * bits of t[0..emit) are set in history_bits.  With budget[0] = 0 the record is {0} and nothing else changes.  The draws of
 * rejected rows are not consumed: step d + emit is drawn again by the next replay, for the token that then stands there, so
 * token number n of a generation is always drawn at step n -- on identical logits the tokens are pc_sample_advance's, one for
 * one.  row_bits uint32 [rows][ceil(vocab / 32)] and row_token int32 [rows] are scratch (row_bits must not alias history_bits);
 * processed_out (optional, fp32 [rows][vocab]): the processed rows, as in pc_sample_advance.  1 <= rows <= 16, vocab < 2^24,
 * ldl >= vocab; logits need only be 4-byte aligned.  Two launches: rows workgroups, then one wave.  At rows = 1 the token and the
 * ids / pos / past_len / history words are pc_sample_advance's at counter = draws. */
int pc_lookup_verify_sample(const float* logits, int64_t ldl, int32_t vocab, int32_t rows, const pc_sample_params* params_dev,
                            uint32_t* history_bits, uint32_t* row_bits, int32_t* draws, int32_t* row_token, int32_t* hist,
                            int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* past_len, const int32_t* ndraft,
                            int32_t* budget, int32_t* ring, int32_t* counter, int32_t ring_cap, float* processed_out, void* stream);

/* ---- batched decode over slots (csrc/pc_slots.hip, csrc/pc_sample.hip) ---------------------------------------------------------
 * A slot is one running sequence in a batch-1 KV arena of its own ([n_layers][2][Hkv][cap][head_dim] fp16, pc_kv_gather's dst).
 * Its state is one element of each of these DEVICE arrays over S <= 16 slots, so that one captured step serves every replay:
 *   kv_base uint64[S]  address of the slot's arena          cap  int32[S]  rows per plane of that arena
 *   len     int32[S]   rows the arena holds                 pos  int32[S]  position id of the token the slot feeds next
 *   ids     int64[S]   that token                           live int32[S]  0: the slot is idle -- every launch below skips it
 * A live slot with len >= cap is skipped like an idle one (nothing is written, nothing is read) and pc_sample_advance_slots
 * switches it off.  No slot's result depends on any other slot's data, on its index or on how many slots are live.
 *
 * pc_rope_append_slots: for every live slot b, RoPE with row b of cs [S][head_dim/2][2] (pc_rope_table) on the query and key
 * of row b of qkv (fp32 [S][ld], q | k | v head-major; in_layout 1: every head in the rotary-pair tile order of pc_gemm's
 * q|k|v weight image, i.e. a plain projection over that image), q to the split-precision pair q_hi / q_lo [S][q_token_stride],
 * K / V (rounded to fp16 once) to row len[b] of layer `layer` of the slot's arena -- the bits pc_rope_append_ex writes.
 *
 * pc_attn_decode_slots: for every live slot b and head, softmax(q k^T * softmax_scale) v over keys [0, len[b]] of the slot's
 * arena (the row pc_rope_append_slots just wrote included), fp32 softmax, K / V as stored.  The key axis is cut into `nsplit`
 * (1..32, chosen by the host from an upper bound of the lengths) equal shares of len[b] + 1 read from the device; partials go
 * to `workspace` (pc_attn_decode_slots_workspace_bytes) and are merged by a second launch into the fragment planes
 * out_frag_hi / out_frag_lo [1][H*head_dim/32][64][8] (row = slot) that pc_gemm's o_proj consumes.  head_dim 64 or 128; the
 * H / Hkv query heads of a kv head share its K / V reads.  Rows of idle slots are left as they are.
 *
 * pc_sample_advance_slots: pc_sample_advance per live slot, all slots concurrently: the chain of the ONE parameter block and
 * the draw on logits[b * logits_row_stride ..] with the random stream seeds[b], the step counters[b] and the history bitmap
 * history_bits[b * ceil(vocab/32) ..]; then ids[b] = token, pos[b] += 1, len[b] += 1, ring[b * ring_cap + counters[b] %
 * ring_cap] = token, counters[b] += 1, budget[b] -= 1, and live[b] = 0 when the token is one of stop_ids[0..8) (unused
 * entries: -1), budget[b] reached 0 or len[b] + 1 >= cap[b].  processed_out (optional, [S][vocab]) as in pc_sample_advance.
 *
 * pc_attn_decode_slots_trunk: pc_attn_decode_slots for slots that hold the same bytes in their first rows (prompts over one
 * schema).  Two more device arrays over the S slots: leader[b] = -1: slot b is on its own (keys [0, len[b]] of its own arena);
 * leader[b] = g: keys [0, trunk[b]) are read from the arena of slot g (kv_base[g], cap[g]), keys [trunk[b], len[b]] from b's own.
 * Host contract: leader[g] == g, trunk[b] == trunk[g] for every member, 0 < trunk[b] <= len[b].  A slot for which the contract
 * does not hold (or whose leader lies outside [0, S), has trunk[g] > cap[g] or a null arena) is treated as leader[b] = -1: its
 * result is the plain attention over its own arena.  The leader's rows are read whether or not the leader is live.  A trunk launch reads each group's shared rows once for all live members (MFMA tiles of 16
 * query rows = members x the kv head's query heads; `nsplit_trunk` shares of the trunk), an own launch does pc_attn_decode_slots'
 * arithmetic over the remaining keys in `nsplit_own` shares, and the merge takes nsplit_trunk + nsplit_own partials per (slot,
 * head) in key order.  A row's result depends on its own q, its keys, trunk and the two split counts only.  With leader = -1
 * everywhere the planes are bit-identical to pc_attn_decode_slots at nsplit = nsplit_own.
 *
 * pc_attn_decode_slots_q8 -- llama2.py:366-400 as pc_attn_decode_slots replaces it, with the keys of a slot read from an int8
 * image instead of its fp16 arena.  kvq_base (device, uint64[S]): per slot the 16-byte aligned address of ONE image in the
 * pc_kv_quant_q8 layout at qcap rows per plane and P = n_layers * 2 * Hkv planes in the arena's plane order (codes
 * [P][qcap][128], fp32 scales [P][qcap] at byte P*qcap*128 -- which is why the entry takes n_layers).  For a live slot, keys
 * [0, len[b]) are image rows, an element being (float) code * scale in fp32 with no fp16 rounding; key len[b], the row
 * pc_rope_append_slots just wrote, is read from the fp16 arena, exact.  The key axis is cut as pc_attn_decode_slots cuts it, the
 * workspace (pc_attn_decode_slots_workspace_bytes), the partial records, the merge launch and the fragment planes are that
 * entry's.  The workgroup that takes key len[b] also quantises that row (K and V of its kv head, the arithmetic of
 * pc_kv_quant_q8, bit for bit) into image row len[b]; no other image row is written, and none of the launch reads that one.
 * A slot's result depends on its own q, keys and nsplit only.  head_dim 128 only; a kv head with H / Hkv query heads is read
 * once per query head.  Host contract: qcap >= cap[b] for every slot (a slot with len[b] >= qcap is left alone: neither its
 * image nor its partials are touched and its output rows are undefined).  PC_ERR_ARG with nothing launched: head_dim != 128,
 * H % Hkv != 0, a null pointer, S outside 1..16, qcap < 1, layer outside [0, n_layers), nsplit outside 1..32, a workspace that
 * is too small.
 *
 * Int8-only residency (no fp16 arena per slot).  kv_base[b] is then the slot's FRESH-ROW buffer: fp16 [P][128], plane stride
 * head_dim, 16-byte aligned, holding the K / V row of the current step only; cap[b] keeps its meaning as the bound on len[b].
 * pc_rope_append_slots_q8: pc_rope_append_slots' arguments with kv_base read that way, plus kvq_base / qcap / n_layers as above.
 * For a live slot with 0 <= len[b] < cap[b] and len[b] < qcap: q_hi / q_lo are pc_rope_append_slots' bits (both in_layout
 * values); the rotated K row and the V row, rounded to fp16 as there, go to planes (layer*2)*Hkv + h and + Hkv of the fresh-row
 * buffer, and -- quantised with the arithmetic of pc_kv_quant_q8, bit for bit -- to image row len[b] (codes and scale).  Any
 * other slot is left alone: nothing is written anywhere.  PC_ERR_ARG with nothing launched: what pc_rope_append_slots refuses,
 * head_dim != 128, a null kvq_base, qcap < 1, layer outside [0, n_layers).
 * pc_attn_decode_slots_q8_fresh: pc_attn_decode_slots_q8 behind pc_rope_append_slots_q8 -- the exact row is read from the
 * fresh-row buffer (kv_base[b] + plane * 128) and nothing is staged: the launch writes no image byte.  Slices, order of
 * summation, records, merge and argument checks are pc_attn_decode_slots_q8's; on equal image rows [0, len) and an equal
 * exact row the planes are bit-equal to that entry's. */
int pc_rope_append_slots_q8(const float* qkv, int64_t ld, int32_t in_layout, void* q_hi, void* q_lo, int64_t q_token_stride,
                            const float* cs, const uint64_t* kv_base, const int32_t* cap, const int32_t* len, const int32_t* live,
                            int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D, const uint64_t* kvq_base, int32_t qcap,
                            int32_t n_layers, void* stream);
int pc_attn_decode_slots_q8_fresh(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                  const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t layer, int32_t H,
                                  int32_t Hkv, int32_t D, float softmax_scale, int32_t nsplit, void* workspace, int64_t workspace_bytes,
                                  void* out_frag_hi, void* out_frag_lo, const uint64_t* kvq_base, int32_t qcap, int32_t n_layers,
                                  void* stream);
/* Prompt-lookup drafts over int8 images: the k + 1 row step of pc_rope_append_slots_rows / pc_attn_verify_slots with a slot's keys
 * read from its image.  What the step computes is what pc_attn_decode_slots_q8 computes one token at a time: the token at
 * position p attends to rows [0, p) as IMAGE rows and to its own row p exactly -- so draft row i of a slot with length len sees
 * image keys [0, len + i), rows len .. len + i - 1 of which this step's append has just quantised, and key len + i in fp16.  The
 * result does not depend on where step boundaries fall.  `fresh` (0 | 1, uniform over a launch) says where the fp16 rows of the
 * step live: 0 = arena rows len + i behind kv_base[b] (plane stride cap[b]), 1 = a fresh-row buffer behind kv_base[b], fp16
 * [P][k + 1][128], row i.  A slot runs when it is live, 0 <= len, len + k + 1 <= cap[b] AND len + k + 1 <= qcap; any other slot
 * is left alone by both launches (the host keeps qcap >= len + k + 1 for every slot whose cap word lets it run).
 * pc_rope_append_slots_rows_q8: pc_rope_append_slots_rows' arguments plus kvq_base / qcap / n_layers / fresh, grid (draft row,
 * slot).  q_hi / q_lo and the fp16 K / V rows are pc_rope_append_slots_rows' bits (both in_layout values); every row also goes,
 * quantised with the arithmetic of pc_kv_quant_q8 bit for bit, to image row len + i (codes and scale).  Nothing else is written.
 * At k = 0, fresh = 1 it is pc_rope_append_slots_q8.  PC_ERR_ARG with nothing launched: what either parent refuses, head_dim !=
 * 128, k outside 0..15, S * (k + 1) > 64, fresh outside 0..1.
 * pc_attn_verify_slots_q8: pc_attn_verify_slots' arguments plus the same four.  Grid, tile columns and per-wave key slices are
 * that entry's, cut from the len + k image keys; codes enter the fp16 MFMA as fp16 values (exact), the K scale multiplies the
 * score together with the softmax scale, the V scale is folded into p in fp32 before p is split; code * scale is never rounded to
 * fp16.  The exact key is one more record per (row, head), index nsplit: m = q . k * scale * log2 e, l = 1, O = v, written by the
 * workgroups of split 0; the merge launch takes nsplit + 1 records, so the workspace is
 * pc_attn_verify_slots_q8_workspace_bytes.  The launch writes no image byte; a (slot, row, head) depends on that slot's words,
 * k and nsplit only.  PC_ERR_ARG with nothing launched: what pc_attn_decode_slots_q8 or pc_attn_verify_slots refuses, fresh
 * outside 0..1. */
int pc_rope_append_slots_rows_q8(const float* qkv, int64_t ld, int32_t in_layout, void* q_hi, void* q_lo, int64_t q_token_stride,
                                 const float* cs, const uint64_t* kv_base, const int32_t* cap, const int32_t* len,
                                 const int32_t* live, int32_t S, int32_t k, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                                 const uint64_t* kvq_base, int32_t qcap, int32_t n_layers, int32_t fresh, void* stream);
int64_t pc_attn_verify_slots_q8_workspace_bytes(int32_t S, int32_t k, int32_t H, int32_t D, int32_t nsplit);
int pc_attn_verify_slots_q8(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base, const int32_t* cap,
                            const int32_t* len, const int32_t* live, int32_t S, int32_t k, int32_t layer, int32_t H, int32_t Hkv,
                            int32_t D, float softmax_scale, int32_t nsplit, void* workspace, int64_t workspace_bytes,
                            void* out_frag_hi, void* out_frag_lo, const uint64_t* kvq_base, int32_t qcap, int32_t n_layers,
                            int32_t fresh, void* stream);
int pc_rope_append_slots(const float* qkv, int64_t ld, int32_t in_layout, void* q_hi, void* q_lo, int64_t q_token_stride,
                         const float* cs, const uint64_t* kv_base, const int32_t* cap, const int32_t* len, const int32_t* live,
                         int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D, void* stream);
int64_t pc_attn_decode_slots_workspace_bytes(int32_t S, int32_t H, int32_t D, int32_t nsplit);
int pc_attn_decode_slots(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base, const int32_t* cap,
                         const int32_t* len, const int32_t* live, int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                         float softmax_scale, int32_t nsplit, void* workspace, int64_t workspace_bytes, void* out_frag_hi,
                         void* out_frag_lo, void* stream);
int pc_attn_decode_slots_q8(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base, const int32_t* cap,
                            const int32_t* len, const int32_t* live, int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                            float softmax_scale, int32_t nsplit, void* workspace, int64_t workspace_bytes, void* out_frag_hi,
                            void* out_frag_lo, const uint64_t* kvq_base, int32_t qcap, int32_t n_layers, void* stream);
int64_t pc_attn_decode_slots_trunk_workspace_bytes(int32_t S, int32_t H, int32_t D, int32_t nsplit_own, int32_t nsplit_trunk);
int pc_attn_decode_slots_trunk(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                               const int32_t* cap, const int32_t* len, const int32_t* live, const int32_t* leader,
                               const int32_t* trunk, int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D, float softmax_scale,
                               int32_t nsplit_own, int32_t nsplit_trunk, void* workspace, int64_t workspace_bytes, void* out_frag_hi,
                               void* out_frag_lo, void* stream);
/* pc_attn_decode_slots_trunk_q8: pc_attn_decode_slots_q8 for slots that hold the same rows in front, with the leader / trunk words
 * of pc_attn_decode_slots_trunk.  Slot b has T shared rows when its leader g = leader[b] lies in [0, S), leader[g] == g,
 * trunk[b] == trunk[g] == T > 0, T <= len[b], T <= qcap and kvq_base[g] != 0; otherwise it has none and is on its own (the plain
 * attention over its own complete image).  For a live slot with T shared rows, keys [0, T) are rows of the LEADER's image -- read
 * once for all live members of the group, whether or not the leader is live --, keys [T, len[b]) rows of the slot's own image
 * (its own rows [0, T) are never read) and key len[b] the fp16 arena row just appended, exact, which the launch also quantises
 * into row len[b] of the slot's OWN image, as pc_attn_decode_slots_q8 does.  No image row below len[b] is written by anyone.
 * Three launches that ask one predicate: the trunk (MFMA tiles of 16 (member, query head) columns over the codes, key slices a
 * function of (T, nsplit_trunk), records 0 .. nsplit_trunk - 1), the own rows (the key axis [T, len] cut into nsplit_own chunks
 * of ceil((len + 1 - T) / nsplit_own), records nsplit_trunk ..) and the merge in record order.  A member's bits depend on its
 * own q, its keys, T and the two split counts only -- not on the size of its group, its column in the tile or its slot index.
 * With leader = -1 everywhere the planes and the staged rows are bit-identical to pc_attn_decode_slots_q8 at nsplit = nsplit_own.
 * Workspace: pc_attn_decode_slots_trunk_workspace_bytes, 16-byte aligned.  head_dim 128 only.  PC_ERR_ARG with nothing launched:
 * what pc_attn_decode_slots_q8 or pc_attn_decode_slots_trunk refuses. */
int pc_attn_decode_slots_trunk_q8(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                                  const int32_t* cap, const int32_t* len, const int32_t* live, const int32_t* leader,
                                  const int32_t* trunk, int32_t S, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                                  float softmax_scale, int32_t nsplit_own, int32_t nsplit_trunk, void* workspace,
                                  int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, const uint64_t* kvq_base,
                                  int32_t qcap, int32_t n_layers, void* stream);
int pc_sample_advance_slots(const float* logits, int64_t logits_row_stride, int32_t vocab, const pc_sample_params* params_dev,
                            const uint64_t* seeds, uint32_t* history_bits, int64_t* ids, int32_t* pos, int32_t* len,
                            const int32_t* cap, int32_t* live, int32_t* budget, const int32_t* stop_ids, int32_t* ring,
                            int32_t* counters, int32_t ring_cap, int32_t S, float* processed_out, void* stream);

/* pc_sample_advance_slots_each -- pc_sample_advance_slots with the sampling state PER SLOT (continuous batching: sequences with
 * different parameters share a step, and a sequence admitted into a running loop keeps the random stream it would have had
 * alone).  params_dev: pc_sample_params[S], slot b uses block b (a block in greedy mode -- temperature < 1e-5 or top_p < 1e-8 --
 * takes the argmax, lowest index among equal maxima); stop_ids: int32 [S][8], row b for slot b (unused entries: -1); draws:
 * int32 [S], the Philox step of slot b's stream (used where pc_sample_advance_slots uses counters[b]; draws[b] += 1 per draw);
 * counters[b] keeps its ring role only: ring[b * ring_cap + counters[b] % ring_cap] = token, counters[b] += 1.  Everything else
 * -- idle slots, full arenas, budget, history bitmap, processed_out, argument checks -- is pc_sample_advance_slots' contract.
 * With S equal blocks, S equal stop rows and draws == counters every output word equals pc_sample_advance_slots' bit for bit. */
int pc_sample_advance_slots_each(const float* logits, int64_t logits_row_stride, int32_t vocab, const pc_sample_params* params_dev,
                                 const uint64_t* seeds, uint32_t* history_bits, int64_t* ids, int32_t* pos, int32_t* len,
                                 const int32_t* cap, int32_t* live, int32_t* budget, const int32_t* stop_ids, int32_t* ring,
                                 int32_t* counters, int32_t* draws, int32_t ring_cap, int32_t S, float* processed_out, void* stream);

/* ---- prompt-lookup speculative decoding over slots (csrc/pc_lookup_slots.hip, csrc/pc_lookup.hip) ---------------------------------
 * The batched step with up to k + 1 tokens per sequence and weight stream: every slot feeds its token and k drafts, so row
 * r = b * (k + 1) + i of every activation is draft row i of slot b, R = S * (k + 1) <= 64 rows in all (1 <= k <= 15; the two
 * middle entries also take k = 0).  A slot keeps kv_base / cap / len / live of the section above and gains, each an array over S:
 *   hist int32[S][hist_cap], hist_len int32[S]   pc_lookup_draft's history, one row per slot
 *   ids int64[S][k + 1], pos int32[S][k + 1]     the forward's inputs: row 0 the fed token, rows 1..k the drafts
 *   ndraft int32[S], budget int32[S]             real drafts of this step; tokens the slot may still emit
 *   stop_ids int32[S][8]                         token ids that end the slot's sequence (unused entries: -1)
 *   ring int32[S][ring_cap][k + 2], ctr int32[S] one record {count, tokens...} per replay and slot
 * A slot RUNS when live[b] != 0 and 0 <= len[b] and len[b] + k + 1 <= cap[b].  For a slot that does not run nothing is read and
 * nothing is written by the first three entries; pc_lookup_verify_slots leaves it an EMPTY record (ring[b][ctr[b] % ring_cap] =
 * {0}, ctr[b] += 1: record c of every slot belongs to replay c) and sets live[b] = 0 -- the too-full slot is switched off.
 *
 * pc_lookup_draft_slots: pc_lookup_draft's rule, one workgroup per running slot on hist[b], hist_len[b], ids[b], pos[b],
 * ndraft[b].  With S = 1 every word written equals pc_lookup_draft's.
 *
 * pc_rope_append_slots_rows: pc_rope_append_slots for k + 1 rows per slot: row r of qkv (fp32 [R][ld], in_layout as there) is
 * rotated with row r of cs [R][head_dim/2][2]; q goes to row r of the split-precision pair q_hi / q_lo [R][q_token_stride], K / V
 * (rounded to fp16 once) to row len[b] + i of layer `layer` of the slot's arena.  The arithmetic is pc_rope_append_ex's; at k = 0
 * the bytes equal pc_rope_append_slots'.
 *
 * pc_attn_verify_slots: for every running slot b, draft row i and query head: softmax(q k^T * softmax_scale) v over keys
 * [0, len[b] + i] of the slot's arena -- the rows pc_rope_append_slots_rows just wrote included, row i does not see the draft
 * rows behind it.  mfma_f32_16x16x32_f16 tiles of 16 (draft row x query head of one kv head) columns with q and p as hi / lo pairs,
 * fp32 online softmax, K / V as stored.  The key axis [0, len[b] + k + 1) is cut into `nsplit` (1..32, from the host) shares
 * read from the device; a share in which a row sees no key contributes (m = -1e30, l = 0).  Partials go to `workspace`
 * (pc_attn_verify_slots_workspace_bytes) and are merged in key order by a second launch into the fragment planes out_frag_hi /
 * out_frag_lo [ceil(R/16)][H*head_dim/32][64][8] (row = r) that pc_gemm's o_proj consumes.  head_dim 64 or 128.  A row's result
 * depends on its own q, its own keys, k and nsplit only -- not on the other slots, the slot index or the live count.  Rows of
 * slots that do not run are left as they are.
 *
 * pc_attn_verify_slots_trunk: pc_attn_verify_slots for slots that hold the same bytes in their first rows, with the leader /
 * trunk words and the host contract of pc_attn_decode_slots_trunk (leader[g] == g, trunk[b] == trunk[g], 0 < trunk[b] <= len[b];
 * a slot for which it does not hold is treated as leader[b] = -1).  For a running slot b with T shared rows, draft row i takes
 * keys [0, T) from the arena of its leader and keys [T, len[b] + i] from its own; with T = 0 keys [0, len[b] + i] of its own.  The
 * leader's rows are read whether or not the leader is live or runs (no step rewrites rows below len >= T).  Three launches: a
 * trunk launch reads each group's shared rows once for all draft rows of all running members (tiles of 16 columns, column
 * (m * (k + 1) + i) * G + g = member m, draft row i, query head g of the kv head; no mask, every trunk key is visible to every
 * draft row; `nsplit_trunk` shares of the trunk), an own launch does pc_attn_verify_slots' arithmetic over keys [T, len[b] + k + 1)
 * in `nsplit_own` shares with the mask of the draft rows unchanged, and the merge takes nsplit_trunk + nsplit_own partials per
 * (row, head) in key order from `workspace` (pc_attn_verify_slots_trunk_workspace_bytes); a row of a slot on its own has no
 * trunk partials.  A row's result depends on its own q, its keys, k, T and the two split counts only -- not on the size of its
 * group, its place in a tile or the slot index.  With leader = -1 everywhere the planes are bit-identical to
 * pc_attn_verify_slots at nsplit = nsplit_own.  For slots that do not run nothing is read and nothing is written.
 *
 * pc_lookup_verify_slots: a[r] = argmax of row r of logits fp32 [R][vocab] (row stride ldl; pc_lookup_verify's rule) into
 * row_argmax int32[R], then per running slot pc_lookup_verify's rule on the slot's words with len[b] in the place of past_len and
 * two additions: emit is cut behind the first a[i], i < emit, that is one of stop_ids[b][0..8) -- that token is emitted and
 * live[b] = 0 --, and live[b] = 0 when budget[b] reached 0 or the new len[b] + k + 1 > cap[b].  With S = 1 and no stop ids
 * every word equals pc_lookup_verify's.  Ordinary vector stores only. */
int pc_lookup_draft_slots(const int32_t* hist, const int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* ndraft,
                          const int32_t* cap, const int32_t* len, const int32_t* live, int32_t S, int32_t k, int32_t nmax,
                          void* stream);
int pc_rope_append_slots_rows(const float* qkv, int64_t ld, int32_t in_layout, void* q_hi, void* q_lo, int64_t q_token_stride,
                              const float* cs, const uint64_t* kv_base, const int32_t* cap, const int32_t* len, const int32_t* live,
                              int32_t S, int32_t k, int32_t layer, int32_t H, int32_t Hkv, int32_t D, void* stream);
int64_t pc_attn_verify_slots_workspace_bytes(int32_t S, int32_t k, int32_t H, int32_t D, int32_t nsplit);
int pc_attn_verify_slots(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base, const int32_t* cap,
                         const int32_t* len, const int32_t* live, int32_t S, int32_t k, int32_t layer, int32_t H, int32_t Hkv,
                         int32_t D, float softmax_scale, int32_t nsplit, void* workspace, int64_t workspace_bytes, void* out_frag_hi,
                         void* out_frag_lo, void* stream);
int64_t pc_attn_verify_slots_trunk_workspace_bytes(int32_t S, int32_t k, int32_t H, int32_t D, int32_t nsplit_own,
                                                   int32_t nsplit_trunk);
int pc_attn_verify_slots_trunk(const void* q_hi, const void* q_lo, int64_t q_token_stride, const uint64_t* kv_base,
                               const int32_t* cap, const int32_t* len, const int32_t* live, const int32_t* leader,
                               const int32_t* trunk, int32_t S, int32_t k, int32_t layer, int32_t H, int32_t Hkv, int32_t D,
                               float softmax_scale, int32_t nsplit_own, int32_t nsplit_trunk, void* workspace,
                               int64_t workspace_bytes, void* out_frag_hi, void* out_frag_lo, void* stream);
int pc_lookup_verify_slots(const float* logits, int64_t ldl, int32_t vocab, int32_t S, int32_t k, int32_t* row_argmax, int32_t* hist,
                           int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* len, const int32_t* cap,
                           int32_t* live, const int32_t* ndraft, int32_t* budget, const int32_t* stop_ids, int32_t* ring,
                           int32_t* counters, int32_t ring_cap, void* stream);

/* pc_slot_arm -- admission of ONE sequence into a running slot loop: one launch writes every state word of slot `slot` (and its
 * history bitmap row) from a pinned host block, read with system-scope loads (pc_fetch_block's rule); live[slot] = 1 is the last
 * store.  The launch is ordered on `stream` behind the replays already enqueued: they saw the old words, later ones see the new
 * sequence.  No word or bitmap row of another slot is touched.  The block is pc_slot_arm_block followed by hist_words uint32 of
 * history bitmap; nbytes = sizeof(pc_slot_arm_block) + 4 * hist_words rounded up to a multiple of 8.  hist_words is the row length
 * of state->history_bits (ceil(vocab / 32)).  The host must not rewrite a block before its launch has finished. */
typedef struct pc_slot_arm_block {
    int32_t slot;                /* which of the S slots */
    int32_t cap;                 /* rows per plane of the arena */
    uint64_t kv_base;            /* address of the arena */
    int32_t len;                 /* rows the arena holds */
    int32_t pos;                 /* position id of the token fed next */
    int64_t id;                  /* that token */
    int32_t leader;              /* shared trunk: leading slot, -1: on its own */
    int32_t trunk;               /* shared rows */
    int32_t budget;              /* steps left */
    int32_t counter;             /* ring counter (the loop's, so that ring rows line up across slots) */
    int32_t draws;               /* Philox step of the sequence's own stream */
    int32_t hist_words;          /* uint32 words of history bitmap behind the struct */
    uint64_t seed;
    pc_sample_params params;
    int32_t stop_ids[8];         /* unused entries: -1 */
} pc_slot_arm_block;

typedef struct pc_slot_state {   /* the S-slot device arrays of the captured step */
    uint64_t* kv_base; int32_t* cap; int32_t* len; int32_t* pos; int64_t* ids; int32_t* live; int32_t* leader; int32_t* trunk;
    int32_t* budget; int32_t* counters; int32_t* draws; uint64_t* seeds; pc_sample_params* params; int32_t* stop_ids;
    uint32_t* history_bits;
} pc_slot_state;

int pc_slot_arm(const pc_slot_arm_block* host_block, int32_t nbytes, const pc_slot_state* state, int32_t S, void* stream);

/* ---- prompt-lookup drafts under continuous batching (csrc/pc_sample.hip, csrc/pc_lookup.hip) --------------------------------------
 * pc_lookup_verify_slots_each -- pc_lookup_verify_slots with the sampling state PER SLOT: pc_lookup_verify_sample's rule on the
 * slot words of the section above, so that greedy and sampled sequences share one S * (k + 1)-row step and a sequence admitted
 * into a running loop keeps the random stream it would have had alone.  Per slot b: params_dev[b] (pc_sample_params[S]; a block
 * in greedy mode takes the argmax of its processed row), seeds[b], draws[b] (int32[S], the Philox step of the slot's stream),
 * history_bits[b] (uint32 [S][ceil(vocab / 32)], the penalty history) and stop_ids[b][0..8).  For every RUNNING slot b and row
 * i <= ndraft[b], t[b][i] = pc_sample_advance's draw on logits row b * (k + 1) + i with the random stream (seeds[b], step
 * draws[b] + i) under the history history_bits[b] + {ids[b][1], ..., ids[b][i]}; pad rows (i > ndraft[b]) and rows of slots that
 * do not run are not drawn.  Then pc_lookup_verify_slots' rule per slot with t in the place of the argmax -- the EMPTY record
 * and ctr[b] += 1 for a slot that does not run, the cut behind the first emitted stop id (that token is emitted), live[b] = 0 on a
 * stop id, on budget[b] reaching 0 or when the new len[b] + k + 1 > cap[b] -- and two additions: the bits of the emitted tokens
 * are set in history_bits[b], and draws[b] += emit, counted behind the stop cut (the draws of rejected rows are not consumed:
 * token number n of a sequence is always drawn at step n).  row_bits uint32 [S * (k + 1)][ceil(vocab / 32)] and row_token int32
 * [S * (k + 1)] are scratch (row_bits must not alias history_bits).  1 <= S <= 16, 1 <= k <= 15, S * (k + 1) <= 64, vocab < 2^24,
 * ldl >= vocab; logits 4-byte, params and seeds 8-byte aligned.  Two launches: S * (k + 1) workgroups, then one wave per slot.
 * With every block plain greedy the words equal pc_lookup_verify_slots'; with S = 1 and no stop ids pc_lookup_verify_sample's; with
 * ndraft = 0 everywhere the token, ids[b][0], pos, len, budget, draws and bitmap equal pc_sample_advance_slots_each's.  Ordinary
 * vector stores only. */
int pc_lookup_verify_slots_each(const float* logits, int64_t ldl, int32_t vocab, int32_t S, int32_t k, const pc_sample_params* params_dev,
                                const uint64_t* seeds, uint32_t* history_bits, uint32_t* row_bits, int32_t* draws, int32_t* row_token,
                                int32_t* hist, int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos, int32_t* len,
                                const int32_t* cap, int32_t* live, const int32_t* ndraft, int32_t* budget, const int32_t* stop_ids,
                                int32_t* ring, int32_t* counters, int32_t ring_cap, void* stream);

/* pc_lookup_slot_arm -- pc_slot_arm for the words of the lookup step: ONE launch between two replays writes every word of slot
 * `slot` from a pinned host block, read with system-scope loads; live[slot] = 1 is the last store.  Written: kv_base, cap, len,
 * leader, trunk, budget, counters (the replays enqueued so far: record c of every slot then still belongs to replay c), draws = 1,
 * seed, parameter block, stop row, bitmap row (hist_words words), ids[slot][0], pos[slot][0], ndraft = 0, hist_len and the first
 * hist_len ids of hist[slot] (row stride hist_cap).  No word of another slot is touched.  The block is pc_lookup_slot_arm_block,
 * then hist_words uint32 of bitmap, then hist_len int32 of history ids; nbytes = sizeof(pc_lookup_slot_arm_block) + 4 * hist_words
 * + 4 * hist_len, the last two each rounded up to a multiple of 8.  1 <= hist_len <= hist_cap < 2^24; S and k as in
 * pc_lookup_verify_slots_each.  The host must not rewrite a block before its launch has finished. */
typedef struct pc_lookup_slot_arm_block {
    int32_t slot;                /* which of the S slots */
    int32_t cap;                 /* rows per plane of the arena */
    uint64_t kv_base;            /* address of the arena */
    int32_t len;                 /* rows the arena holds */
    int32_t pos;                 /* position id of the token fed next */
    int64_t id;                  /* that token */
    int32_t leader;              /* shared trunk: leading slot, -1: on its own */
    int32_t trunk;               /* shared rows */
    int32_t budget;              /* tokens left */
    int32_t counter;             /* ring counter (the loop's, so that ring records line up across slots) */
    int32_t hist_words;          /* uint32 words of history bitmap behind the struct */
    int32_t hist_len;            /* int32 history ids behind the bitmap (the last one is `id`) */
    uint64_t seed;
    pc_sample_params params;
    int32_t stop_ids[8];         /* unused entries: -1 */
} pc_lookup_slot_arm_block;

typedef struct pc_lookup_slot_state {   /* the S-slot device arrays of the captured lookup step */
    uint64_t* kv_base; int32_t* cap; int32_t* len; int32_t* live; int32_t* leader; int32_t* trunk; int64_t* ids; int32_t* pos;
    int32_t* ndraft; int32_t* budget; int32_t* hist_len; int32_t* counters; int32_t* draws; uint64_t* seeds; pc_sample_params* params;
    int32_t* stop_ids; uint32_t* history_bits; int32_t* hist;
} pc_lookup_slot_state;

int pc_lookup_slot_arm(const pc_lookup_slot_arm_block* host_block, int32_t nbytes, const pc_lookup_slot_state* state, int32_t S, int32_t k,
                       int32_t hist_cap, void* stream);

/* ---- forced rows: a request's question fed through the draft rows of the running step (csrc/pc_lookup_common.h) --------------------
 * One more word per slot, forced int32[S]: the prompt tokens still to be fed behind ids[b][0]; 0 for a slot armed by
 * pc_lookup_slot_arm.  Such a slot is armed with hist[L - 1] = ids[b][0] = t_0 (L = hist_len[b]) and hist[L .. L + forced[b]) =
 * t_1 .. -- the device reads those ids before it writes there.  A RUNNING slot with R = forced[b] > 0 takes, per step:
 *   draft   m = min(k, R); ids[b][1 + j] = hist[b][L + j] for j < m, pad rows and pos as pc_lookup_draft_slots, ndraft[b] = m; no
 *           n-gram search.
 *   rows    R > k: nothing is drawn.  R <= k: row R alone is drawn, as a sequence's first token is: pc_sample_advance's draw on
 *           logits row b * (k + 1) + R with (seeds[b], step draws[b]) under history_bits[b] as it stands (the rows in front are
 *           prompt tokens: no bits are added); a greedy block takes the argmax.
 *   accept  R > k: the record is EMPTY; hist_len[b] += k + 1, ids[b][0] = hist[b][L + k], pos[b][0] += k + 1, len[b] += k + 1,
 *           forced[b] = R - k - 1; budget, draws and bitmap stay.
 *           R <= k, g the token of row R: the record is {1, g}; hist[b][L + R] = g, hist_len[b] += R + 1, ids[b][0] = g,
 *           pos[b][0] += R + 1, len[b] += R + 1, forced[b] = 0, budget[b] -= 1, draws[b] = 1, the bit of g is set; live[b] = 0
 *           when g is one of stop_ids[b], the budget reached 0 or the new len[b] + k + 1 > cap[b].
 *   ctr[b] += 1 either way.  After the step that emits g every word of the slot but ctr[b] is what pc_lookup_slot_arm writes
 *   behind a prefill that drew g.  A slot that does not run takes the EMPTY record and live[b] = 0 of pc_lookup_verify_slots.
 * The host keeps L + R + budget <= hist_cap (indices are clamped into the buffer otherwise).  With forced all zero the draft and
 * verify entries write exactly the words of pc_lookup_draft_slots / pc_lookup_verify_slots_each; other arguments as there.
 *
 * pc_lookup_slot_arm_prompt: pc_lookup_slot_arm on the same block, whose hist_len ids run through the LAST question token, `id` /
 * `pos` are t_0 and its position, `len` the staged rows and `budget` the tokens the sequence may emit.  All hist_len ids are copied;
 * then hist_len[slot] = hist_len - n_forced, forced[slot] = n_forced and draws[slot] = 0 (the first token is still to be drawn).
 * 0 <= n_forced < hist_len.  Ordinary vector stores only. */
int pc_lookup_slot_arm_prompt(const pc_lookup_slot_arm_block* host_block, int32_t nbytes, const pc_lookup_slot_state* state,
                              int32_t* forced, int32_t n_forced, int32_t S, int32_t k, int32_t hist_cap, void* stream);
int pc_lookup_draft_slots_prompt(const int32_t* hist, const int32_t* hist_len, int32_t hist_cap, int64_t* ids, int32_t* pos,
                                 int32_t* ndraft, const int32_t* cap, const int32_t* len, const int32_t* live, const int32_t* forced,
                                 int32_t S, int32_t k, int32_t nmax, void* stream);
int pc_lookup_verify_slots_prompt(const float* logits, int64_t ldl, int32_t vocab, int32_t S, int32_t k,
                                  const pc_sample_params* params_dev, const uint64_t* seeds, uint32_t* history_bits, uint32_t* row_bits,
                                  int32_t* draws, int32_t* row_token, int32_t* hist, int32_t* hist_len, int32_t hist_cap, int64_t* ids,
                                  int32_t* pos, int32_t* len, const int32_t* cap, int32_t* live, const int32_t* ndraft, int32_t* budget,
                                  const int32_t* stop_ids, int32_t* ring, int32_t* counters, int32_t* forced, int32_t ring_cap,
                                  void* stream);

/* ---- per-token log-probabilities (csrc/pc_logprob.hip; no reference counterpart) -----------------------------------------------------
 * pc_token_logprobs: for each of `rows` rows of fp32 logits [rows][vocab] (row stride ldl elements, 4-byte aligned only, ldl may be
 * odd), the log-probability of the row's token and of the top_n most likely tokens.  Exactly one of tok64 / tok32 is non-null; the
 * token of row r is tok[r * tok_stride].  1 <= rows <= 64, 0 <= top_n <= PC_LOGPROBS_MAX_TOP, top_n < vocab < 2^24, ldl >= vocab,
 * tok_stride >= 1.
 *   The distribution is the log-softmax of the RAW logits, the model's own: m = max of the row, s = sum exp(x - m) in fp32,
 *   lp(j) = (x[j] - m) - log(s).  It comes BEFORE temperature, repetition penalty, top-p and top-k: what a sampler made of the row
 *   does not enter (a token that top-k would have removed still has its finite log-probability here).
 *   out_ids int32 [rows][1 + top_n], out_lp float [rows][1 + top_n]: entry 0 is the row's token and its lp, entries 1 .. top_n the
 *   top_n most likely tokens ordered by (value descending, index ascending) -- "lowest index among equal maxima", extended to the
 *   whole order.  The row's token may appear among them again.
 *   -inf entries contribute 0 to s; NaN entries are treated as -inf everywhere (they rank as -inf, in index order, with lp -inf).
 *   A row whose maximum is not finite (no finite entry, or a +inf) writes NaN log-probabilities and ids -1 in every entry.
 *   A token outside [0, vocab) writes id -1 and lp NaN in entry 0 and leaves entries 1 .. top_n correct: the guard for pad rows,
 *   whose token is unspecified, and for the stale rows of idle slots.
 * One launch, one workgroup per row; no state, no counter: nothing but the two output arrays is written (ordinary vector stores),
 * and the result of a row depends on that row alone.  Argument errors -> PC_ERR_ARG with nothing launched. */
#define PC_LOGPROBS_MAX_TOP 8
int pc_token_logprobs(const float* logits, int64_t ldl, int32_t vocab, int32_t rows, const int64_t* tok64, const int32_t* tok32,
                      int64_t tok_stride, int32_t top_n, int32_t* out_ids, float* out_lp, void* stream);

/* ---- token controls: logit_bias, banned / allowed ids, min_new_tokens (csrc/pc_logit_ctl.hip; no reference counterpart) ---------------
 * pc_logit_adjust: the ADJUSTED copy of S * rows_per_slot rows of fp32 logits, which a sampler then reads in place of the raw rows
 * (any of the advance / verify entries above, in front of their temperature / penalty / top-p / top-k / greedy rule).  Row
 * r = b * rows_per_slot + i of `out` is the adjusted form of row r of `logits` under slot b's block ctl[b] and allowed row
 * allowed_bits[b] (bit j & 31 of word j >> 5 set: token j may be drawn).  Per row, in this order:
 *   1. a[j] = x[j];
 *   2. for each of the first n_bias table entries, a[id] = x[id] + bias: one fp32 add, so a bias of -inf is a ban and a NaN stays
 *      a NaN.  The ids are distinct (host contract); an id outside [0, vocab) is skipped; n_bias is clamped into
 *      [0, PC_LOGIT_BIAS_MAX];
 *   3. with use_allowed != 0 (and allowed_bits non-null), every j whose bit is clear: a[j] = -inf -- a biased id included;
 *   4. while len[b] + i < stop_free_len, a[stop] = -inf for the stop_ids inside [0, vocab).  len[b] is the arena length the decode
 *      loops already keep (it grows by the tokens emitted; a null `len` reads as 0), i the draft row, so the boundary may fall
 *      between two rows of one slot.  A sequence that enters with length L0 and must not stop before its m-th generated token
 *      (the token of its prefill counts as the first) gets stop_free_len = L0 + m - 1; 0 (or anything <= len) is off.
 * S >= 1, 1 <= rows_per_slot <= 16, S * rows_per_slot <= 64, 1 <= vocab < 2^24, ldl >= vocab (4-byte aligned rows, ldl may be odd:
 * 16-byte loads where a row's base allows, scalar loads otherwise), `out` 16-byte aligned with ldo >= vocab, ldo % 4 == 0, and not
 * the logits themselves: it writes out of place, so pc_token_logprobs keeps seeing the model's own rows.  Columns [vocab, ldo) of
 * `out` are not written.
 * One launch, grid = column chunks x rows: a workgroup applies only the entries that fall into its columns, and orders the writes
 * to one element across workgroup barriers.  A row's result depends on that row, its slot's block and len[b] only -- not on other
 * slots, on live flags or on the slot index.  No state, no counter, no atomic: nothing but `out` is written (ordinary vector
 * stores).  Argument errors -> PC_ERR_ARG with nothing launched. */
#define PC_LOGIT_BIAS_MAX 64
#define PC_LOGIT_STOP_MAX 8
typedef struct pc_logit_ctl {        /* one per slot, device memory */
    int32_t n_bias;                  /* 0..64; the kernel clamps */
    int32_t use_allowed;             /* != 0: a token whose bit is clear in the slot's allowed row becomes -inf */
    int32_t stop_free_len;           /* stop_ids are -inf on draft row i while len[b] + i < stop_free_len */
    int32_t pad;
    int32_t stop_ids[8];             /* unused: -1 */
    int32_t bias_id[64];             /* distinct (host contract); ids outside [0, vocab) are skipped */
    float   bias[64];
} pc_logit_ctl;
int pc_logit_adjust(const float* logits, int64_t ldl, int32_t vocab, int32_t S, int32_t rows_per_slot, const pc_logit_ctl* ctl,
                    const uint32_t* allowed_bits, const int32_t* len, float* out, int64_t ldo, void* stream);

/* Diagnostics used by the GPU test-suite: dumps the MFMA C/D lane map and the LDS transpose-read
 * map the attention kernel relies on (probe_kernel in csrc/pc_misc.hip). */
/* dev hook (tools/gemm_trace.py): weight-streaming launches issued by this thread stamp per-wave wall-clock times
 * (entry, K loop done, reduced, done) into buf [workgroups][8][4] uint64; NULL switches it off.  No reference counterpart. */
int pc_dev_gemm_trace(void* buf);
int pc_dev_attn_trace(void* buf);   /* the same for attn_small_kernel: [workgroups][4][4] (entry, first tile scored, slice done, done) */
int pc_probe_layouts(float* out_mfma /*[16*16]*/, float* out_tr /*[512]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PROMPTCACHE_HIP_H */
