/*
 * sparse_amd.h — C ABI of libsparse_amd.so, the MI355X (gfx950) hot path behind the
 * pydata/sparse `numba_backend` dot / elementwise / reduction kernels.
 *
 * Boundary contract (mirrors the reference's kernel-factory boundary):
 *   - The reference exposes Python-callable kernels over *raw arrays*, keyed by a dtype
 *     pair (`_dot_csr_ndarray_type(dt1, dt2)(out_shape, a_data, a_indices, a_indptr, b)`,
 *     sparse/numba_backend/_common.py:720-755).  Here the dtype key is an explicit
 *     `val_dtype` / `idx_dtype` code and every array is a plain device pointer.
 *   - The CALLER owns every buffer (inputs, outputs, workspace).  Nothing is allocated
 *     behind the caller's back; data-dependent output sizes use the reference's own
 *     two-phase shape (count -> scan -> fill) as two entry points.
 *   - All pointers are DEVICE pointers (HBM) unless a parameter says "host".
 *   - Every entry point is asynchronous on `stream` (a hipStream_t passed as void*),
 *     stateless, re-entrant and thread-safe; it returns 0 on success, a positive
 *     hipError_t value if the HIP runtime reported one, or a negative SPAMD_E* code for
 *     an argument error.  It never throws and never synchronises the device.
 *   - No torch / C++ types cross this boundary.
 */
#ifndef SPARSE_AMD_H
#define SPARSE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dtype codes (shared by value and index arguments) */
#define SPAMD_F32 0
#define SPAMD_F64 1
#define SPAMD_I32 2
#define SPAMD_I64 3
#define SPAMD_BF16 4
#define SPAMD_U8 5 /* bool (0/1) — results of comparisons, any/all, astype(bool) */
#define SPAMD_C64 6  /* complex64: interleaved (re, im) float32 pairs - the products (spamd_spmm_csr_complex, spamd_spgemm_expand,
                      * spamd_segment_reduce with op = add), the complex elementwise / reduction entry points (spamd_cplx_*,
                      * spamd_merge_union_complex) and the complex SDDMM (spamd_sddmm_complex) */
#define SPAMD_C128 7 /* complex128: interleaved (re, im) float64 pairs - the same entry points */
#define SPAMD_F16 8  /* IEEE float16: dense operands of the SDDMM entry points only (spamd_sddmm, spamd_sddmm_panels,
                      * spamd_sddmm_mfma_tiles_typed) */

#define SPAMD_MAX_NDIM 16 /* largest array rank the key kernels accept */

/* error codes (negative; positive values are hipError_t) */
#define SPAMD_EINVAL (-1)  /* bad size / null pointer / misaligned */
#define SPAMD_ETYPE (-2)   /* unsupported dtype combination */
#define SPAMD_EWS (-3)     /* workspace too small */

/* flags */
#define SPAMD_TILED_GROUP_ENDS 2u /* spamd_spmm_tiled: blk_off has tiles + 1 entries per row group (spamd_spmm_tiled_inspect) */
#define SPAMD_EXACT_MULADD 1u /* separate IEEE mul + add (bit-exact vs the reference's
                                 non-contracted loop) instead of fused multiply-add */
#define SPAMD_TILED_INT32 8u /* spamd_spmm_tiled with val_dtype SPAMD_F32: the stream's values, B and the result are int32 BIT
                             * PATTERNS (the inspector only moves value bits: build the stream from the int32 values viewed
                             * as float32); products and sums wrap around like NumPy's int32 (`_dot_dtype`, _common.py:635) */
#define SPAMD_SPMM_ROWVEC 16u /* spamd_spmm_csr: results of at most 4 columns keep the row-vector kernel (lanes along a row) instead of the stream form */
#define SPAMD_SPMM_ROWGROUP 4u /* spamd_spmm_csr: the k-ascending row-group kernel whatever the shape (no row-vector, no LDS-resident-B path) */

/* Library/ABI version: major*10000 + minor*100 + patch. */
int spamd_version(void);

/* Name of the code object's target ("gfx950"). Host pointer to a static string. */
const char* spamd_target_arch(void);

/* ---------------------------------------------------------------------------------------
 * A1  CSR x dense -> dense        replaces `_dot_csr_ndarray`
 *                                  (sparse/numba_backend/_common.py:720-755; dispatch :386-389)
 *   out[i, j] = sum_{k in row i, ascending storage order} a_data[k] * b[a_indices[k], j]
 *   A is M x K in CSR (a_indptr has M+1 entries), B is K x N row-major with leading
 *   dimension ldb (elements), out is M x N row-major with leading dimension ldo.
 *   Every out element is WRITTEN (rows without stored elements get zeros): the caller
 *   does not pre-zero `out`.  Accumulation is in the value dtype (the reference's
 *   `dtr = dt1*dt2`; the host layer promotes mixed inputs), strictly in storage order
 *   per output element, so with SPAMD_EXACT_MULADD the result is bit-identical to the
 *   reference loop; without it each step is one fused multiply-add.
 *   Results of at most 4 columns (N = 1: the matrix-vector product) without SPAMD_EXACT_MULADD take the row-vector
 *   kernel instead: the lanes of a wave run along a row and a butterfly adds their partial sums, i.e. a fixed TREE
 *   order per row (deterministic; floating point within rounding of the k-ascending sum, integers identical).
 *   SPAMD_SPMM_ROWGROUP keeps the k-ascending kernel for those widths as well.
 *   val_dtype: F32 | F64 | I32 | I64.   idx_dtype: I32 | I64 (a_indices and a_indptr).
 * ------------------------------------------------------------------------------------- */
int spamd_spmm_csr(int val_dtype, int idx_dtype, int64_t M, int64_t K, int64_t N,
                   const void* a_data, const void* a_indices, const void* a_indptr,
                   const void* b, int64_t ldb, void* out, int64_t ldo,
                   unsigned flags, void* stream);

/* The same product for COMPLEX values (csrc/spmm_complex.hip): val_dtype C64 | C128, values stored as interleaved (re, im)
 * pairs as NumPy and torch store them; ldb / ldo count complex elements; a_data, b and out are at least 8-byte aligned
 * (SPAMD_EINVAL otherwise).  Same contract as spamd_spmm_csr: every out element is written once, by one lane, summed in
 * storage order.  One term is  re += ar*br - ai*bi; im += ar*bi + ai*br : four fused multiply-adds by default; with
 * SPAMD_EXACT_MULADD four rounded products, a rounded subtraction and a rounded addition, then the rounded accumulate -
 * NumPy's scalar complex multiply and add, bit-identical to the reference loop.  A lane reads 16 bytes of a B row per
 * access (one complex128 column, two complex64 columns) when b and out are 16-byte aligned (complex64: and N, ldb, ldo
 * even; complex128: and a_data), else 8 bytes.  Results of at most 4 complex64 / 2 complex128 columns without
 * SPAMD_EXACT_MULADD or SPAMD_SPMM_ROWGROUP take the row-vector form (lanes along a row, a butterfly: a fixed tree
 * order per row, deterministic).  The LDS-resident-B, stream, inspector/executor and hub-row forms are real-only.
 * idx_dtype: I32 | I64.  Other codes: SPAMD_ETYPE. */
int spamd_spmm_csr_complex(int val_dtype, int idx_dtype, int64_t M, int64_t K, int64_t N,
                           const void* a_data, const void* a_indices, const void* a_indptr,
                           const void* b, int64_t ldb, void* out, int64_t ldo,
                           unsigned flags, void* stream);

/* The same product with B RESIDENT IN LDS, for a short contracted axis (`_dot_csr_ndarray` / `_dot_coo_ndarray` as
 * tensordot uses them, `_common.py:720-755, 979-1014`; BASELINE config 3: K = 512): a 256-byte column panel of B —
 * (K + 1) * 256 bytes <= 160 KB, i.e. K <= 639 — is copied into LDS once per workgroup, 16 lanes own a row of A and read a
 * row of B per stored element from LDS instead of through the vector-memory path.  Sums run in storage order per output
 * element (bit-identical to spamd_spmm_csr's row-group kernel in both arithmetic modes; SPAMD_EXACT_MULADD as there).
 * spamd_spmm_csr itself takes this path when `spamd_spmm_csr_ldsb_fits` says 1, M >= 8192 and N * itemsize >= 128, unless
 * SPAMD_SPMM_ROWGROUP is set.  `..._fits`: K within the LDS budget, N / ldb / ldo multiples of 16 / itemsize, b and out
 * 16-byte aligned. */
int spamd_spmm_csr_ldsb_fits(int val_dtype, int64_t M, int64_t K, int64_t N, const void* b, int64_t ldb,
                             const void* out, int64_t ldo);
int spamd_spmm_csr_ldsb(int val_dtype, int idx_dtype, int64_t M, int64_t K, int64_t N,
                        const void* a_data, const void* a_indices, const void* a_indptr,
                        const void* b, int64_t ldb, void* out, int64_t ldo,
                        unsigned flags, void* stream);

/* The same product for results of at most 4 columns (N = 1: `x @ v`, the matrix-vector product) organised around the
 * CSR triplet's STREAM (`_dot_csr_ndarray`, `_common.py:744-753`, whose inner loop over one output column is this product):
 * every wave owns a piece of the stream that starts and ends on row boundaries, reads it once in 16-byte loads with four
 * 256-element subtiles in flight, takes B from LDS (K * N values <= 160 KB - 512 B), closes the rows with a segmented scan
 * over the lanes and stores `out` in row order.  A row's products are added in a fixed tree order (deterministic; floating
 * point within rounding of the storage-order sum, integers identical) - SPAMD_EXACT_MULADD is not accepted here.
 * spamd_spmm_csr takes this path for N <= 4 when `..._fits` says 1 and M >= 32768, unless SPAMD_SPMM_ROWGROUP,
 * SPAMD_SPMM_ROWVEC or (for floating point) SPAMD_EXACT_MULADD is set.  `..._fits`: N in 1..4 (1..3 for 8-byte values), M < 2^28, B within the LDS
 * budget, a_data and a_indices 16-byte aligned.  `nnz` = a_indptr[M] when the caller knows it, -1 otherwise (the kernel then reads it: one
 * more memory latency at the head of every wave).  flags bits 8..15 (tuning hint, 0 = default): workgroups per resident slot.
 * Round 6: `..._fits` returns the number of PASSES over A the product takes - ceil(N / w) for N up to 64 with w = the widest
 * chunk of columns (<= 4, 8-byte values: 3) whose K x w values fit the LDS; 0 = not this kernel - and spamd_spmm_csr_stream
 * runs them, one launch per chunk (b and out may be strided: ldb, ldo).  A pass costs A's stream whatever its width, so
 * spamd_spmm_csr takes up to 3 passes for 5 <= N <= SPAMD_STREAM_MULTI_MAX_N, up to 2 for N <= 4 columns of 8-byte values
 * and 1 for N <= 4 columns of 4-byte values, under the conditions above.
 * `spamd_spmm_csr_stream_passes`: that whole rule - the passes spamd_spmm_csr takes with these `flags`, 0 = another kernel
 * (host arithmetic only; a_data / a_indices are only tested for alignment). */
#define SPAMD_STREAM_MULTI_MAX_N 12
int spamd_spmm_csr_stream_fits(int val_dtype, int64_t M, int64_t K, int64_t N, const void* a_data, const void* a_indices);
int spamd_spmm_csr_stream_passes(int val_dtype, int64_t M, int64_t K, int64_t N, const void* a_data, const void* a_indices,
                                 unsigned flags);
int spamd_spmm_csr_stream(int val_dtype, int idx_dtype, int64_t M, int64_t K, int64_t N,
                          const void* a_data, const void* a_indices, const void* a_indptr,
                          const void* b, int64_t ldb, void* out, int64_t ldo,
                          int64_t nnz, unsigned flags, void* stream);

/* ---------------------------------------------------------------------------------------
 * A1 (inspector/executor form)   same product as spamd_spmm_csr for F32 (N % 128 == 0) and F64 (N % 64 == 0),
 *   both arithmetic modes, with a cached K-tiled copy of A — the role `cusparseSpMM_preprocess`-style
 *   inspection plays elsewhere; the reference's analogue is the memoised format conversion of
 *   `COO(cache=True)` (sparse/numba_backend/_coo/core.py:317-338).  Inspector (once per matrix):
 *     keys   = spamd_csr_to_keys(A)                      row*K + col
 *     tkeys  = spamd_spmm_tiled_keys(keys)               ((g*ntiles+t)*RG + row%RG)*KB + col%KB
 *     stable sort of (tkeys, values)                     spamd_sort_kv
 *     seg_start, nblk = spamd_spmm_tiled_lists(tkeys)    first element / blocks of list (g,t)
 *     blk_off = spamd_exclusive_scan(nblk)               int64[nseg + 1], nseg = groups*ntiles
 *     blk_off32 = spamd_convert(I64 -> I32)              what the executor reads (total blocks < 2^31)
 *     blocks  = spamd_spmm_tiled_pack(...)               64-byte blocks, d0 = col%KB << 9 | 2 + 2*(row%RG):
 *                                                        F32: eight (d0, value bits);
 *                                                        F64: five d0, one pad dword, five (value lo, value hi);
 *                                                        lists padded with zero entries
 *   where groups = ceil(ceil(M/RG) / GPB) * GPB (every wave of the executor grid has lists).
 *   Executor: spamd_spmm_tiled — a workgroup covers a panel of 512 bytes of the output rows (128 F32 or 64 F64
 *   columns; wider N = more panels); B streams through LDS in KB-row tiles (LDS-DMA), each wave pulls its blocks
 *   with scalar loads and keeps 32 rows of partial sums in a fixed VGPR block addressed with s_set_gpr_idx.
 *   RG / KB / GPB / entries per block / slack / panel width from spamd_spmm_tiled_params(val_dtype);
 *   `blocks` must hold total_blocks + slack blocks and be 64-byte aligned.
 *   flags: SPAMD_EXACT_MULADD as for spamd_spmm_csr; bits 8..15 (optional tuning hint, 0 = default): 64-byte lines of
 *   each list to prefetch into L2 two tile phases ahead (~1.5 x the mean blocks per list).  Results are bit-identical to spamd_spmm_csr with the
 *   same flags (sorted column indices), hence to the reference loop under SPAMD_EXACT_MULADD.
 * ------------------------------------------------------------------------------------- */
int spamd_spmm_tiled_params(int val_dtype, int* rows_per_group, int* tile_rows, int* groups_per_block,
                            int* entries_per_block, int* slack_blocks, int* direct_max_tiles, int* panel_cols);
/* Direct (sort-free) inspector for CSR with sorted column indices and ceil(K/KB) <= direct_max_tiles: the tiled
 * order is a stable partition by tile of every RG-row group of the CSR order.
 *   spamd_spmm_tiled_count: nblk[nseg+1] (blocks per list, ready for spamd_exclusive_scan), flags[0] = 1 if a row's
 *                           column indices are not ascending (then use the key-sort recipe above);
 *   spamd_spmm_tiled_fill:  writes the block stream from (a_data of val_dtype, a_indices, a_indptr) and blk_off. */
int spamd_spmm_tiled_count(int val_dtype, int idx_dtype, int64_t M, int64_t K, const void* a_indices,
                           const void* a_indptr, int64_t* nblk, int* flags, void* stream);
int spamd_spmm_tiled_fill(int val_dtype, int idx_dtype, int64_t M, int64_t K, const void* a_data, const void* a_indices,
                          const void* a_indptr, const int64_t* blk_off, int64_t total_blocks, int* blocks,
                          void* stream);
/* one-pass form of count + fill: every row group's first block follows from the row pointers alone (an upper bound of what
 * the groups before it need: no scan, no dependence between groups), so blk_off is int32[groups * (tiles + 1)] — per group
 * the first block of each of its lists and the end of the last one; pass SPAMD_TILED_GROUP_ENDS to spamd_spmm_tiled with
 * it.  `blocks` has room for ceil(nnz / entries_per_block) + lists + slack_blocks blocks (the blocks between groups are
 * zeroed); state = one 64-bit word; state[0] != 0 afterwards: unsorted column indices, outputs invalid (use the key-sort
 * recipe) */
int spamd_spmm_tiled_inspect(int val_dtype, int idx_dtype, int64_t M, int64_t K, const void* a_data, const void* a_indices,
                             const void* a_indptr, void* state, int* blk_off, int* blocks, void* stream);
/* The same outputs straight from a CSC operand (a_indices = row indices, a_indptr = K + 1 column pointers, rows ascending
 * inside every column) - no CSC -> CSR conversion: a K-tile is 160 whole columns of the CSC arrays and a workgroup's rows own
 * one short run per column.  ws = int32 workspace of spamd_spmm_tiled_inspect_csc_ws(M, K) words, 8-byte aligned;
 * state[0] != 0 afterwards: rows out of order - the lists are then EMPTY (blk_off all zero) and the caller converts to CSR.  Replaces, for `csc @ dense`, the reference's `_dot_csc_ndarray`
 * (_common.py:869-904) together with the conversion this backend needed before it. */
int64_t spamd_spmm_tiled_inspect_csc_ws(int64_t M, int64_t K);
int spamd_spmm_tiled_inspect_csc(int val_dtype, int idx_dtype, int64_t M, int64_t K, const void* a_data,
                                 const void* a_indices, const void* a_indptr, int* ws, void* state, int* blk_off,
                                 int* blocks, void* stream);
/* Balanced layouts for SKEWED matrices (round 5; the reference's loop, _common.py:744-753, is indifferent to row lengths -
 * one wave per 35 consecutive rows is not: Zipf row lengths cost 4x at config 2's size).  Rows are sorted by length and classed
 * against `cap` (a power of two; longer than cap/2: a group of its own, then 2 / 4 / 8 / 16 rows to a group, everything else 35),
 * so that the 16 groups of a workgroup are equally heavy; rows are read and stored through a row map; entries, lists and the
 * order of every output element's terms are unchanged (bit-identical products).
 *   spamd_spmm_tiled_map_stats   keys[M] = K - length of every row, rows[M] = 0..M-1, stats[8] (zeroed here): rows per class [0..5],
 *                                stored elements of the heaviest NATURAL 35-row group [6] (the caller's "is it skewed" test)
 *   (caller)                     stable sort of rows by keys (spamd_sort_kv: longest rows first), class counts read back
 *   spamd_spmm_tiled_map_groups  groups of the layout for these class counts (host arithmetic)
 *   spamd_spmm_tiled_map_build   rowmap[groups * rows_per_group + 16] (-1 = unused slot), gload[groups + 1] (stored elements
 *                                per group, then 0): the caller's exclusive scan of gload is `vstart`
 *   spamd_spmm_tiled_inspect_mapped / spamd_spmm_tiled_mapped: the one-pass inspector and the executor on that layout. */
int spamd_spmm_tiled_map_stats(int idx_dtype, int64_t M, int64_t K, int64_t cap, const void* a_indptr, int64_t* keys,
                               int* rows, int64_t* stats, void* stream);
int64_t spamd_spmm_tiled_map_groups(const int64_t* class_counts /* host, 6 entries */);
int spamd_spmm_tiled_map_build(int idx_dtype, int64_t M, int64_t cap, const void* a_indptr, const int* rows_sorted,
                               const int64_t* class_counts /* host */, int* rowmap, int64_t* gload, void* stream);
int spamd_spmm_tiled_inspect_mapped(int val_dtype, int idx_dtype, int64_t M, int64_t K, int64_t groups, const void* a_data,
                                    const void* a_indices, const void* a_indptr, const int* rowmap, const int64_t* vstart,
                                    void* state, int* blk_off, int* blocks, void* stream);
int spamd_spmm_tiled_mapped(int val_dtype, int64_t M, int64_t groups, int64_t K, int64_t N, const int* blocks,
                            const int* blk_off, const int* rowmap, const void* b, int64_t ldb, void* out, int64_t ldo,
                            unsigned flags, void* stream);
int spamd_spmm_tiled_keys(int64_t nnz, const int64_t* rowcol_keys, int64_t K, int64_t* tiled_keys, void* stream);
int spamd_spmm_tiled_lists(int val_dtype, int64_t nnz, const int64_t* tiled_keys_sorted, int64_t M, int64_t K,
                           int64_t* seg_start, int64_t* nblk, void* stream);
int spamd_spmm_tiled_pack(int val_dtype, int64_t nnz, const int64_t* tiled_keys_sorted, const void* vals_sorted,
                          const int64_t* seg_start, const int64_t* blk_off, int64_t total_blocks, int* blocks,
                          void* stream);
/* executor.  N = the PADDED width (whole panels; B provides that many columns, zero-padded).  flags: SPAMD_EXACT_MULADD,
 * SPAMD_TILED_GROUP_ENDS, SPAMD_TILED_INT32, bits 8..15 = lines of a list to prefetch (0: default), bits 16..23 = columns of the LAST panel
 * that are stored (0: all) - a narrower result is then written without padding: `out` holds N - panel + that many
 * columns per row (any count; until late round 4 float32 took even counts only). */
int spamd_spmm_tiled(int val_dtype, int64_t M, int64_t K, int64_t N, const int* blocks, const int* blk_off32,
                     const void* b, int64_t ldb, void* out, int64_t ldo, unsigned flags, void* stream);

/* ---------------------------------------------------------------------------------------
 * A10  NaN scan                    replaces `nan_check` (_common.py:51-69), the pass `matmul`
 *                                  runs over every operand before multiplying (:245-246).
 *   *flag (device int32) is set to 1 if any of the n values is NaN, else 0.  `data` must be
 *   16-byte aligned.  val_dtype: F32 | F64 (I32 | I64 accepted: flag = 0).
 * ------------------------------------------------------------------------------------- */
int spamd_has_nan(int val_dtype, int64_t n, const void* data, int* flag, void* stream);
/* The same scan, asynchronous: `host_flag` is the device-accessible address of a PINNED host int the caller has set
 * to 0; the kernel stores 1 there if it meets a NaN.  The caller records an event behind this call and reads the int
 * after waiting on that event alone, so the product queued behind the scan is not drained (reference: the blocking
 * `check_class_nan` pass of `matmul`, _common.py:245-246). */
int spamd_has_nan_async(int val_dtype, int64_t n, const void* data, int* host_flag, void* stream);

/* =======================================================================================
 * T1-T3 / A6  Canonicalisation and format conversion on 64-bit C-order linear keys.
 *   Replaces the reference's NumPy/numba integer pipeline: `linear_loc`
 *   (_coo/common.py:56-64), `COO._sort_indices/_sum_duplicates/_prune` (_coo/core.py:1294-1371),
 *   `_from_coo` (_compressed/compressed.py:25-77), `uncompress_dimension`/`_transpose`/
 *   `_convert_coords` (_compressed/convert.py:82-87,210-339), `COO.reshape/transpose`
 *   (_coo/core.py:725-807,1034-1111).  A sparse array is (keys[nnz] int64, data[nnz]);
 *   a transpose is a key permutation, a reshape is the identity on keys.
 *   All results are bit-exact integers.  `strides`/`dims`/`perm`/`axis_order` are HOST arrays
 *   of `ndim` (<= SPAMD_MAX_NDIM) entries, read during the call.
 * ===================================================================================== */

/* keys[p] = sum_d coords[axis_order[d]*coord_stride + p] * strides[d]   (coords: [ndim][nnz]) */
int spamd_coo_linearize(int idx_dtype, int ndim, int64_t nnz, const void* coords, int64_t coord_stride,
                        const int64_t* strides, const int32_t* axis_order, int64_t* keys, void* stream);
/* coords[d*coord_stride + p] = (keys[p] / strides[d]) % dims[d] */
int spamd_coo_delinearize(int idx_dtype, int ndim, int64_t nnz, const int64_t* keys, const int64_t* strides,
                          const int64_t* dims, void* coords, int64_t coord_stride, void* stream);
/* keys_out = C-order key after moving source axis perm[d] to destination position d */
int spamd_permute_keys(int ndim, int64_t nnz, const int64_t* keys_in, const int64_t* src_strides,
                       const int64_t* src_dims, const int32_t* perm, int64_t* keys_out, void* stream);
/* flag[0] = 1 if any coords[d][i] lies outside [0, dims[d]) (device int32[1]).  The reference constructor
 * (_coo/core.py:198-291) trusts its caller; this backend checks, because a bad coordinate becomes an
 * out-of-bounds key for spamd_scatter. */
int spamd_coords_check(int idx_dtype, int ndim, int64_t nnz, const void* coords, int64_t coord_stride,
                       const int64_t* dims, int* flag, void* stream);
/* flags2[0] = keys not non-decreasing, flags2[1] = some adjacent keys equal (device int32[2]) */
int spamd_keys_check(int64_t n, const int64_t* keys, int* flags2, void* stream);
/* flags[i] = 1 where a run of equal keys starts (int64 0/1, ready for spamd_exclusive_scan) */
int spamd_flag_heads(int64_t n, const int64_t* keys, int64_t* flags, void* stream);
/* flags[i] = 1 where data[i] is NOT bit-identical to the fill pattern (the reference's bit-wise
 * `equivalent`, _utils.py:448-452: -0.0 is not 0.0).  elem_bytes in {1,2,4,8,16}; fill_bits holds the element's low
 * 8 bytes, fill_bits_hi bytes 8..15 of a 16-byte element (complex128: the imaginary part) and is ignored otherwise. */
int spamd_flag_ne_bits(int elem_bytes, int64_t n, const void* data, uint64_t fill_bits, uint64_t fill_bits_hi,
                       int64_t* flags, void* stream);
/* *count (device int64) = number of elements bit-identical to the fill pattern: the cheap test that a prune has nothing
 * to do */
int spamd_count_eq_bits(int elem_bytes, int64_t n, const void* data, uint64_t fill_bits, uint64_t fill_bits_hi,
                        int64_t* count, void* stream);
/* dst[offsets[i]] = src[i] where flags[i] != 0  (stream compaction after an exclusive scan) */
int spamd_compact(int elem_bytes, int64_t n, const void* src, const int64_t* flags, const int64_t* offsets,
                  void* dst, void* stream);
/* dst[i] = src[perm[i]] ; dst[keys[i]] = src[i] */
int spamd_gather(int elem_bytes, int64_t n, const void* src, const int64_t* perm, void* dst, void* stream);
/* the same for every row of a [rows, n] matrix in one launch (the [ndim, nnz] coordinate matrix of a COO,
 * `coords[:, order]` / `coords[:, mask]` in the reference's `_sort_indices` / `_sum_duplicates`, _coo/core.py:1294-1353) */
int spamd_compact_rows(int elem_bytes, int rows, int64_t n, const void* src, int64_t ld_src, const int64_t* flags,
                       const int64_t* offsets, void* dst, int64_t ld_dst, void* stream);
int spamd_gather_rows(int elem_bytes, int rows, int64_t n, const void* src, int64_t ld_src, const int64_t* perm, void* dst,
                      int64_t ld_dst, void* stream);
int spamd_scatter(int elem_bytes, int64_t n, const void* src, const int64_t* keys, void* dst, void* stream);
/* sorted keys (row*C + col) -> indptr[R+1], indices[nnz]          (`_from_coo`, compressed.py:64-76) */
int spamd_keys_to_csr(int idx_dtype, int64_t nnz, const int64_t* keys, int64_t R, int64_t C, void* indptr,
                      void* indices, void* stream);
/* (indptr, indices) -> keys[p] = row(p)*C + indices[p]              (`uncompress_dimension`, convert.py:82-87) */
int spamd_csr_to_keys(int idx_dtype, int64_t R, int64_t nnz, const void* indptr, const void* indices, int64_t C,
                      int64_t* keys, void* stream);
/* sorted row ids -> int64 indptr[R+1]        (`cumsum(bincount(coords[0]))`, _common.py:452-458) */
int spamd_rows_to_indptr(int idx_dtype, int64_t nnz, const void* rows, int64_t R, int64_t* indptr, void* stream);
/* CSR <-> CSC of a 2-D compressed matrix with 4-byte values in one call: `GCXS.change_compressed_axes` / `_transpose`
 * (compressed.py:388-423, convert.py:210-273: uncompress, re-linearise, stable argsort, bincount + cumsum).  The input is
 * in (major, minor) order, so a stable sort on the minor index alone gives (minor, major) order.  data: nnz 4-byte values
 * (moved bit-wise), indices[nnz], indptr[n_major + 1] of idx_dtype; outputs of the same dtypes: out_data[nnz],
 * out_indices[nnz] (the major ids), out_indptr[n_minor + 1].  n_major, n_minor < 2^32; ws of spamd_csx_swap_ws_bytes(nnz). */
int64_t spamd_csx_swap_ws_bytes(int64_t nnz);
int spamd_csx_swap(int idx_dtype, int64_t n_major, int64_t n_minor, int64_t nnz, const void* data, const void* indices,
                   const void* indptr, void* out_data, void* out_indices, void* out_indptr, void* ws, int64_t ws_bytes,
                   void* stream);
/* the same for 8-byte values (float64 / int64: the reference's default value type): a 16-byte payload rides through the sort */
int64_t spamd_csx_swap8_ws_bytes(int64_t nnz);
int spamd_csx_swap8(int idx_dtype, int64_t n_major, int64_t n_minor, int64_t nnz, const void* data, const void* indices,
                   const void* indptr, void* out_data, void* out_indices, void* out_indptr, void* ws, int64_t ws_bytes,
                   void* stream);
/* Stable radix sort of (key, value) int64 pairs on key bits [0, end_bit); keys must be >= 0.
 * Replaces `np.argsort(linear, kind="mergesort")` (core.py:1315).  ws: spamd_sort_pairs_ws_bytes(n) bytes, which serve
 * every end_bit (SPAMD_EWS when ws_bytes is smaller: nothing is launched). */
int64_t spamd_sort_pairs_ws_bytes(int64_t n);
int spamd_sort_pairs(int64_t n, const int64_t* keys_in, int64_t* keys_out, const int64_t* vals_in,
                     int64_t* vals_out, int end_bit, void* ws, int64_t ws_bytes, void* stream);
/* The same stable sort carrying a 4- or 8-byte VALUE as payload (used by SpGEMM's expand-sort-compress).
 * ws: spamd_sort_kv_ws_bytes(val_bytes, n) bytes (SPAMD_EWS when ws_bytes is smaller). */
int64_t spamd_sort_kv_ws_bytes(int val_bytes, int64_t n);
int spamd_sort_kv(int val_bytes, int64_t n, const int64_t* keys_in, int64_t* keys_out, const void* vals_in,
                  void* vals_out, int end_bit, void* ws, int64_t ws_bytes, void* stream);
int spamd_iota(int64_t n, int64_t* out, void* stream);
/* out[i] = in[0] + ... + in[i-1] for i in [0, n]; both arrays hold n+1 entries (in[n] ignored).
 * spamd_scan_ws_bytes(n) is the workspace of spamd_exclusive_scan(n, ...), i.e. of a scan over the n + 1 items it
 * processes - pass the same n to both.  Arrays of at most 16384 entries are scanned by one workgroup and take no
 * workspace; beyond that, SPAMD_EWS when ws_bytes is smaller than the query's result (nothing is launched). */
int64_t spamd_scan_ws_bytes(int64_t n);
int spamd_exclusive_scan(int64_t n, const int64_t* in, int64_t* out, void* ws, int64_t ws_bytes, void* stream);
/* astype between F32/F64/I32/I64/U8 (C-cast, NumPy "unsafe"; to U8 = x != 0) */
int spamd_convert(int src_dtype, int dst_dtype, int64_t n, const void* src, void* dst, void* stream);

/* =======================================================================================
 * A7  Elementwise on canonical operands     replaces `_Elemwise` + `_match_arrays`
 *                                            (sparse/numba_backend/_umath.py:53-92,392-751)
 *   On sorted, duplicate-free linear keys the reference's mask enumeration / argsort / join /
 *   concatenate / re-sort collapses to one sorted-key UNION:
 *     out[k] = func(a[k] or fill_a, b[k] or fill_b), entries bit-equal to func(fill_a, fill_b)
 *     dropped afterwards (spamd_flag_ne_bits + spamd_compact).
 * ===================================================================================== */

/* pos[i] = number of h-keys < q[i]; match[i] = 1 iff q[i] occurs in h (h sorted + unique) */
int spamd_lower_bound_match(int64_t nq, const int64_t* q, int64_t nh, const int64_t* h, int64_t* pos,
                            int64_t* match, void* stream);
int spamd_invert_flags(int64_t n, const int64_t* in, int64_t* out, void* stream);
/* Output slot of every a / b element in the union and the union's keys.
 * posB/posA/matchB from spamd_lower_bound_match, ub = exclusive scan of (1 - matchB) (nb+1). */
int spamd_union_positions(int64_t na, const int64_t* ka, const int64_t* posB, int64_t nb, const int64_t* kb,
                          const int64_t* posA, const int64_t* matchB, const int64_t* ub, int64_t* slotA,
                          int64_t* slotB, int64_t* out_keys, void* stream);
int spamd_fill(int elem_bytes, int64_t n, void* out, uint64_t value_bits, void* stream);
/* out[i] = a[i] (op) b[i]; *_is_scalar broadcasts a 1-element device array.
 * op: 0 add 1 sub 2 mul 3 div 4 maximum 5 minimum 6 power 7 fmax 8 fmin 9 floor_divide 10 remainder 11 fmod (floats: NumPy's
 *     npy_divmod / npy_remainder statement for statement; integers: Python's floor rules, x // 0 = x % 0 = 0) 12 copysign
 *     13 hypot 14 arctan2 (12-14: F32 | F64 only) (out dtype = val_dtype);
 *     32 gt 33 ge 34 lt 35 le 36 eq 37 ne 38 logical_and 39 logical_or 40 logical_xor (out U8);
 *     64 bitwise_and 65 bitwise_or 66 bitwise_xor 67 left_shift 68 right_shift (integer dtypes; shift counts outside
 *     [0, bits) give 0 / the sign, as NumPy's).  No FMA contraction.  (reference: the ufunc itself, applied by
 *     `_elemwise_n_ary` sparse/numba_backend/_umath.py:420-470 to matched value arrays) */
int spamd_ewise_binary(int op, int val_dtype, int64_t n, const void* a, int a_is_scalar, const void* b,
                       int b_is_scalar, void* out, void* stream);
/* out[i] = f(a[i]); op: 0 negative 1 abs 2 sqrt 3 exp 4 expm1 5 log 6 log1p 7 sin 8 cos 9 tan 10 tanh
 *   11 sinh 12 cosh 13 arcsin 14 arctan 15 floor 16 ceil 17 rint 18 trunc 19 sign 20 square
 *   21 reciprocal 22 positive 23 log2 24 log10 25 exp2 26 arcsinh 27 arctanh 28 cbrt 29 deg2rad
 *   30 rad2deg (out dtype = val_dtype); 64 isnan 65 isinf 66 isfinite 67 logical_not 68 signbit (out U8) */
int spamd_ewise_unary(int op, int val_dtype, int64_t n, const void* a, void* out, void* stream);
/* out[i] = mask[i] ? a[i] : b[i] (`np.where` on aligned arrays of 1-, 4-, 8- or 16-byte elements, moved bit-wise; mask = 0/1 bytes;
 * *_is_scalar broadcasts a 1-element device array) */
int spamd_ewise_select(int elem_bytes, int64_t n, const void* mask_u8, const void* a, int a_is_scalar, const void* b,
                       int b_is_scalar, void* out, void* stream);

/* Merge-path form of the same union, fused with the function and the prune (the default path):
 *   nblocks = spamd_merge_num_blocks(na, nb);  part[nblocks+1] <- spamd_merge_partition;
 *   spamd_merge_union(fill=0, ...) -> counts[nblocks]; host: exclusive scan -> offsets, total;
 *   spamd_merge_union(fill=1, ...) -> out_keys[total] (strictly increasing), out_vals[total].
 *   out = func(a or fill_a, b or fill_b); entries bit-identical to fill_out are dropped.
 *   op codes as spamd_ewise_binary (6 = power and 9-14, 67, 68 are not available here); *_bits = raw bit patterns
 *   of the fill values in val_dtype (fill_out in the output dtype: U8 for ops 32..40).
 *   fill = 2 is the same union in a single pass: counts = nblocks + 2 int64 of workspace (zeroed by the call),
 *   counts[nblocks + 1] receives the number of outputs, out_keys / out_vals hold na + nb elements.
 *   Every form writes out_keys / out_vals [0, total) and nothing else: with room for na + nb elements, the elements from
 *   `total` on are left as they were.  part[nblocks + 1]: part[p] = number of A items among the first min(p * tile, na + nb)
 *   items of the merged order, equal keys taken from A first.
 *   Returns before any launch or memset: SPAMD_EINVAL for na < 0 or nb < 0; 0 for na + nb == 0 (nothing is written);
 *   SPAMD_ETYPE for a val_dtype other than F32 | F64 | I32 | I64 | U8, for op 6 (power) and for the bitwise ops 64..66 on
 *   F32 | F64. */
int64_t spamd_merge_num_blocks(int64_t na, int64_t nb);
int spamd_merge_partition(int64_t na, const int64_t* ka, int64_t nb, const int64_t* kb, int64_t* part,
                          void* stream);
int spamd_merge_union(int fill, int op, int val_dtype, int64_t na, const int64_t* ka, const void* va, int64_t nb,
                      const int64_t* kb, const void* vb, uint64_t fill_a_bits, uint64_t fill_b_bits,
                      uint64_t fill_out_bits, const int64_t* part, int64_t* counts, const int64_t* offsets,
                      int64_t* out_keys, void* out_vals, void* stream);
/* The same union in ONE launch and without a copy-back (csrc/merge.hip, MODE 3): every tile finds its own merge-path
 * diagonals, the tiles chain their output offsets by look-back, and the kernel leaves its workspace zeroed for the next
 * call.  ws = int64[3 + capacity], capacity >= spamd_merge_fused_blocks(na, nb), all zero before the first use; calls that
 * share a workspace must be ordered on one stream.  *total_dev (device) receives the number of outputs; total_host, if not
 * null, is pinned host memory mapped to the device that receives it too (system-scope release store) - the host may spin on
 * it.  out_keys / out_vals hold na + nb elements; only [0, total) is written.  A workspace of exactly
 * 3 + spamd_merge_fused_blocks(na, nb) words serves.  Returns before any launch (the workspace stays zero): SPAMD_EINVAL
 * for na < 0, nb < 0, a null ws or total_dev, and for na + nb == 0 - the caller returns the empty result itself; SPAMD_ETYPE
 * as spamd_merge_union.  Replaces `_match_arrays` + the mask loop of `_Elemwise`, _umath.py:53-92,576-654, for canonical
 * same-shape operands. */
/* tiles the fused form below runs (its workspace holds 3 + that many int64) */
int64_t spamd_merge_fused_blocks(int64_t na, int64_t nb);
int spamd_merge_union_fused(int op, int val_dtype, int64_t na, const int64_t* ka, const void* va, int64_t nb,
                            const int64_t* kb, const void* vb, uint64_t fill_a_bits, uint64_t fill_b_bits,
                            uint64_t fill_out_bits, int64_t* ws, int64_t* total_dev, int64_t* total_host, int64_t* out_keys,
                            void* out_vals, void* stream);

/* ---------------------------------------------------------------------------------------
 * A8  Grouped reduce     replaces `_calc_counts_invidx` + `_grouped_reduce` / `ufunc.reduceat`
 *                        (sparse/numba_backend/_coo/core.py:1601-1661; compressed.py:354-386)
 *   heads[i] = 1 where a run starts, offsets = its exclusive scan, nseg = number of runs.
 *   out[g] = data[s_g] op data[s_g+1] op ...; counts[g] = run length (may be NULL).
 *   Short runs: one thread per run, strictly left to right (bit-identical to reduceat).
 *   Long runs (n/nseg >= 24 and seg_start_ws != NULL, nseg+1 int64): one wave per run (tree order).
 *   op: 0 add 1 multiply 2 maximum 3 minimum 4 logical_or 5 logical_and 6 fmax 7 fmin (NaN-skipping).
 *   val_dtype C64 | C128: op add only (SPAMD_EINVAL otherwise), always one thread per run, left to right.
 * ------------------------------------------------------------------------------------- */
int spamd_segment_reduce(int op, int val_dtype, int64_t n, const void* data, const int64_t* heads,
                         const int64_t* offsets, int64_t nseg, void* out, int64_t* counts,
                         int64_t* seg_start_ws, void* stream);

/* A8 epilogue in one launch: fold the implicit fill entries of each group into vals[i] (reference
 * _sparse_array.py:405-422).  counts[i] = stored elements of group i, n_cols = elements per group; the fill value
 * is passed both as double and as int64 (the one matching val_dtype is used).  add/multiply use the closed form
 * in the work dtype (float64 for floating results), the other ops fold fv in once where counts[i] != n_cols. */
int spamd_reduce_fill(int op, int val_dtype, int64_t n, void* vals, const int64_t* counts, int64_t n_cols, double fill_f,
                      int64_t fill_i, void* stream);
/* The same fold-in with the number of groups still on the device (*n_dev, as spamd_group_reduce leaves it; the grid is
 * sized for n_max), plus *n_eq (device int64, zeroed here) = how many folded results are bit-identical to
 * result_fill_bits (n_eq == n_dev + 1, the second word of spamd_group_reduce's n_groups, is already zero and not cleared
 * again): the host reads both numbers in one copy, and the result container's prune (`COO(..., prune=True)`,
 * _coo/core.py:705-716) has nothing to do when *n_eq == 0. */
int spamd_reduce_fill_count(int op, int val_dtype, int64_t n_max, const int64_t* n_dev, void* vals, const int64_t* counts,
                            int64_t n_cols, double fill_f, int64_t fill_i, uint64_t result_fill_bits, int64_t* n_eq,
                            void* stream);
/* A8 in one pass: runs of equal (keys[i] / divisor) over SORTED keys are reduced together with their lengths
 * (two streaming passes, csrc/group_reduce.hip; fp sums in a fixed, reproducible order).  Outputs hold up to n entries;
 * n_groups = device int64[2]: [0] receives the number of runs, [1] is cleared (the counter spamd_reduce_fill_count then
 * accumulates into, so that the caller reads both numbers with one copy).  op as for spamd_segment_reduce;
 * val_dtype F32 | F64 | I32 | I64 | U8.  keys < key_bound (0 = unknown; below 2^53 the ids are computed in
 * double precision).  keys and data 16-byte aligned.  Workspace from spamd_group_reduce_ws_bytes. */
int64_t spamd_group_reduce_ws_bytes(int val_dtype, int64_t n);
int spamd_group_reduce(int op, int val_dtype, int64_t n, const int64_t* keys, int64_t divisor, int64_t key_bound,
                       const void* data, int64_t* group_ids, void* values, int64_t* counts, int64_t* n_groups, void* ws,
                       int64_t ws_bytes, void* stream);
/* The same reduction when EVERY axis is reduced (`x.sum()`, `x.max()`, ... with axis=None; reference _sparse_array.py:372-437
 * with axis = all axes: one group): the keys are not read.  Outputs in spamd_group_reduce's form, one entry each:
 * group_ids[0] = 0, values[0], counts[0] = n, n_groups = {1, 0} ({0, ...} for n == 0).  One launch; pieces of the values
 * are folded in a fixed order (reproducible).  ws: spamd_reduce_all_ws_bytes() bytes, 16-byte aligned, ZEROED once by the
 * caller and then reusable by successive calls on one stream (the kernel leaves its ticket word zero). */
int64_t spamd_reduce_all_ws_bytes(void);
int spamd_reduce_all(int op, int val_dtype, int64_t n, const void* data, int64_t* group_ids, void* values, int64_t* counts,
                     int64_t* n_groups, void* ws, int64_t ws_bytes, void* stream);

/* n (1..16) device int64 words to the host WITHOUT a blocking copy: queued behind the stream's work, one thread stores
 * dev_words[0 .. n-1] into host_words[0 .. n-1] and then, with release semantics, `marker` into host_words[n].
 * host_words = n + 1 int64 of PINNED host memory mapped to the device (hipHostMalloc / torch pin_memory); the caller picks a
 * marker host_words[n] does not hold (a per-call sequence number) and spins until it appears.  The read-backs of
 * data-dependent sizes (`SparseArray.reduce`'s group count, _coo/core.py:693-723) use it: a `.item()` costs a stream
 * synchronisation plus a copy command, ~20 us - as much as the kernels of a 10^6-element reduction. */
int spamd_deliver_words(const int64_t* dev_words, int n, int64_t* host_words, int64_t marker, void* stream);

/* out = in^T for a dense row-major matrix (elements of 1 / 2 / 4 / 8 bytes, moved bit-wise; ld_in >= cols, ld_out >= rows):
 * out[c * ld_out + r] = in[r * ld_in + c].  `dense @ sparse` runs as (sparse^T @ dense^T)^T (the reference's dispatch,
 * sparse/numba_backend/_common.py:339-503, hands the dense operand to the kernels transposed and contiguous,
 * `np.ascontiguousarray`, _common.py:744); this is that copy through 64 x 64 LDS tiles. */
int spamd_transpose_2d(int elem_bytes, int64_t rows, int64_t cols, const void* in, int64_t ld_in, void* out, int64_t ld_out,
                       void* stream);

/* Hub rows (round 6, csrc/hot_rows.hip): `_dot.py` multiplies an operand with a few rows far longer than the rest in two
 * parts - the matrix without them and the hot rows cut into pieces that are rows of their own - through the CSR x dense kernels
 * above (reference `_dot_csr_ndarray`, _common.py:720-755: one core walks such a row as one wave does here); this adds the
 * pieces' results into the hot rows of the result: out[rows[h], :] = sum over v in [vfirst[h], vfirst[h + 1]) of part[v, :],
 * in piece order.  val_dtype F32 | F64 | I32 | I64; vfirst has n_hot + 1 entries.  The sum starts from T(0) and adds the pieces
 * one after the other in the result type (integers wrap around); a hot row without pieces (vfirst[h] == vfirst[h + 1]) has its
 * row of `out` set to zero.  Rows of `out` that `rows` does not name and the columns from n_cols on (ld_part, ld_out >= n_cols)
 * are neither read nor written. */
int spamd_hot_rows_combine(int val_dtype, int64_t n_hot, int64_t n_cols, const void* part, int64_t ld_part,
                           const int64_t* vfirst, const int64_t* rows, void* out, int64_t ld_out, void* stream);

/* ---------------------------------------------------------------------------------------
 * A4 / A5  sparse x sparse     replaces `_csr_csr_count_nnz` + `_dot_csr_csr` / `_dot_coo_coo`
 *                              (sparse/numba_backend/_common.py:543-570,639-717,907-976)
 *   Expand-sort-compress: the two entry points below produce, for the A elements [p0, p0+np),
 *   (1) cnt[i] = nnz of B row a_indices[p0+i]; after the caller's exclusive scan (offsets, P):
 *   (2) keys[t] = a_rows[p]*n_col + b_col, vals[t] = 0 + a*b for every product t in [0, P): the reference's accumulator
 *   starts at +0, so a product of -0.0 enters it as +0.0 (every other value, and every integer, is a*b as it is).  The
 *   row-local, small and bitmap kernels below take their products the same way.
 *   A stable sort by key + spamd_segment_reduce(add) then gives every output element summed in
 *   the reference's order (bit-identical), with rows sorted by column.
 *   val_dtype of (2): F32 | F64 | I32 | I64 | C64 | C128; a complex product is the four rounded products, the rounded
 *   subtraction and the rounded addition of NumPy's scalar multiply (never contracted).
 * ------------------------------------------------------------------------------------- */
int spamd_spgemm_count(int idx_dtype, int64_t p0, int64_t np, const void* a_indices, const void* b_indptr,
                       int64_t* cnt, void* stream);
int spamd_spgemm_expand(int val_dtype, int idx_dtype, int64_t p0, int64_t np, const void* a_data,
                        const void* a_indices, const int64_t* a_rows, const void* b_data, const void* b_indices,
                        const void* b_indptr, const int64_t* offsets, int64_t P, int64_t n_col, int64_t* keys,
                        void* vals, void* stream);

/* A4 / A5, row-local form (csrc/spgemm_rows.hip): the products of an output row are expanded, ordered by column
 * (bucket by the high column bits, then rank inside the small buckets: hand-written, no library sort) and summed
 * inside LDS by one workgroup; bit-identical to the expand-sort-compress above, without writing or sorting the
 * products in HBM.  Rows with more products than spamd_spgemm_rows_capacity(...) are skipped and rows with a column that
 * collects more than 64 products are declined (nnz_row = -1): the caller computes those with the global form and merges
 * them with spamd_spgemm_unpack.  n_col < 2^31 - 1.
 *   spamd_spgemm_row_products: prod[n_row + 1] (last entry zeroed) and maxes[2] = {max prod, longest A row};
 *   caller: prod_off = spamd_exclusive_scan(prod), scratch tmp_cols/tmp_vals of prod_off[n_row] entries;
 *   spamd_spgemm_rows: rows of C into the scratch at prod_off[row], their lengths into nnz_row[n_row + 1];
 *   caller: out_indptr = spamd_exclusive_scan(nnz_row);
 *   spamd_spgemm_pack: scratch -> (out_indices int64, out_data), columns ascending inside every row; zero_count
 *     (optional, one device word, zeroed here) receives the number of all-zero-bits values written: what the
 *     `GCXS(..., prune=True)` of reference _common.py:374-379 then need not count in a pass of its own. */
int spamd_spgemm_row_products(int idx_dtype, int64_t n_row, const void* a_indptr, const void* a_indices,
                              const void* b_indptr, int64_t* prod, int64_t* maxes, void* stream);
int64_t spamd_spgemm_rows_capacity(int val_dtype, int64_t n_col, int64_t max_arow);
int spamd_spgemm_rows(int val_dtype, int idx_dtype, int64_t n_row, int64_t n_col, const void* a_indptr,
                      const void* a_indices, const void* a_data, const void* b_indptr, const void* b_indices,
                      const void* b_data, const int64_t* prod_off, int64_t max_prod, int64_t max_arow, int* tmp_cols,
                      void* tmp_vals, int64_t* nnz_row, void* stream);
/* which rows are left to the global form: flags[n_row + 1] for spamd_exclusive_scan + spamd_compact, counts[3] = {rows,
 * their products, rows heavy only by their A length}; nnz_row NULL before the row kernel, else rows with -1 count too */
int spamd_spgemm_classify_rows(int idx_dtype, int64_t n_row, const int64_t* prod, const void* a_indptr,
                               const int64_t* nnz_row, int64_t cap, int64_t* flags, int64_t* counts, void* stream);
/* rows too heavy for the row-local kernel: computed by the global form, given as CSR over all n_row rows (int64
 * columns), copied into the scratch at their product offset; nnz_row[row] is set for the listed rows */
int spamd_spgemm_unpack(int val_dtype, int64_t n_heavy, const int64_t* heavy_rows, const int64_t* src_indptr,
                        const int64_t* src_indices, const void* src_data, const int64_t* prod_off, int* tmp_cols,
                        void* tmp_vals, int64_t* nnz_row, void* stream);
int spamd_spgemm_pack(int val_dtype, int64_t n_row, const int64_t* prod_off, const int64_t* out_indptr,
                      const int* tmp_cols, const void* tmp_vals, int64_t* out_indices, void* out_data,
                      int64_t* zero_count, void* stream);

/* A4 / A5, row-local form for wide rows of a matrix with at most 2^20 columns (csrc/spgemm_bitmap.hip; replaces the same
 * reference functions, sparse/numba_backend/_common.py:543-570,639-717).  A persistent workgroup per CU keeps a bitmap
 * of the output row's columns in LDS: a column's position in the sorted row is a popcount, the row's length is known
 * before anything is written, rows take tickets and find their offset by a look-back over one state word per row, and
 * every row is written ONCE, in place - no scratch rows, no pack, no scan of row lengths.  Values are summed in the order
 * of A's elements (bit-identical to the other two forms).
 *   spamd_spgemm_bitmap_limits(val_dtype, which): 0 = products per row, 1 = A elements per row, 2 = columns,
 *     3 = products per row that may share an output element with an earlier product (checked inside the kernel),
 *     4 / 5 / 6 = products, columns and such products per PART of a row in the split form (below);
 *   spamd_spgemm_bitmap: out_indptr[n_row + 1]; out_indices (int64) / out_data with room for EVERY product (the caller
 *     trims to out_indptr[n_row]); work = n_row + 32 int64 words, zeroed here: afterwards work[1] != 0 = a row was outside
 *     the limits (discard the result, use spamd_spgemm_rows), work[2] = values written whose bits are all zero. */
int64_t spamd_spgemm_bitmap_limits(int val_dtype, int which);
/* A4 / A5 for SMALL operands (round 5): the reference's row loop (`_dot_csr_csr`, _common.py:639-717: a dense accumulator per
 * output row, the row's A elements in storage order) with a WAVE per output row, accumulator and touched-column bitmap in LDS,
 * rows written column-sorted to their final place through a look-back over the rows - ONE launch, one read-back.  The sizes
 * of the reference's own benchmark (benchmarks/test_benchmark_coo.py:9-40) are launch-bound on the general path.
 * out_indices / out_data: room for n_row * n_col entries; work: n_row + 4 words (zeroed here); afterwards work[1] != 0 = failed
 * (a B row not strictly ascending or out of range: discard, use the general path), work[2] = exact zeros written.
 * n_col <= spamd_spgemm_small_max_cols(val_dtype). */
int64_t spamd_spgemm_small_max_cols(int val_dtype);
int spamd_spgemm_small(int val_dtype, int idx_dtype, int64_t n_row, int64_t n_col, const void* a_indptr, const void* a_indices,
                       const void* a_data, const void* b_indptr, const void* b_indices, const void* b_data, int64_t* work,
                       int64_t* out_indptr, int64_t* out_indices, void* out_data, void* stream);

/* parts = 1: whole rows, one 1024-thread workgroup per CU (n_col <= limit 2).  parts > 1: every row in `parts`
 * column ranges (ceil(n_col / parts) rounded up to 256 <= limit 5), 512-thread workgroups, two per CU; bsplit = n_inner *
 * (parts - 1) words of the index type (workspace, filled here: where each B row crosses a range boundary), n_inner = rows
 * of B; limits 4 / 6 are per part.  work = n_row * parts + 32 int64 words. */
int spamd_spgemm_bitmap(int val_dtype, int idx_dtype, int64_t n_row, int64_t n_inner, int64_t n_col, int parts,
                        const void* a_indptr, const void* a_indices, const void* a_data, const void* b_indptr,
                        const void* b_indices, const void* b_data, void* bsplit, int64_t* work, int64_t* out_indptr,
                        int64_t* out_indices, void* out_data, void* stream);

/* A8 / A6 (round 5): keys of a canonical COO with its LEADING axes moved last, sorted, without a sort.  The reference's
 * reduction over axes 0 .. m-1 transposes the kept axes first and sorts every stored element (`COO.reduce` ->
 * `_reduce_calc`, _coo/core.py:693-723; `transpose` + `reshape`, :1601-1661).  Sorted keys = S sorted runs (one per index of the
 * leading axes), merged by ranges of kept cells in LDS (csrc/lead_rotate.hip).  keys[n] sorted and duplicate-free,
 * key = s * P + c; out_keys[n] = c * S + s ascending, out_vals in that order (val_bytes 4 / 8, bit-wise).
 * cells_per_range: a power of two <= spamd_keys_lead_last_limits(1); bounds: S * (ceil(P / cells_per_range) + 1) ints of
 * workspace; S <= limits(0); n < 2^31.  *failed (device, zeroed here) != 0: a range held more than limits(2) elements or a
 * cell more than 64 - out_* are incomplete, use spamd_permute_keys + spamd_sort_kv. */
int64_t spamd_keys_lead_last_limits(int which);
int spamd_keys_lead_last(int val_bytes, int64_t n, const int64_t* keys, const void* vals, int64_t S, int64_t P,
                         int64_t cells_per_range, int* bounds, int64_t* out_keys, void* out_vals, int64_t* failed, void* stream);

/* N3 / A7 (round 5): a canonical COO broadcast to a larger shape in one pass, sorted by construction (csrc/broadcast.hip).
 * Replaces the operand expansion of the reference's elementwise broadcasting (`broadcast_to`, _umath.py:344-389;
 * `_get_expanded_coords_data`, :96-167).  The target's axes, left to right, are [B0][K1][B1][K2][B2] - B: groups of broadcast
 * axes, K: groups of the operand's own axes, sizes b0 k1 b1 k2 b2 (1 for an empty group); keys[n] sorted and duplicate-free
 * over (K1, K2); out_keys[n b0 b1 b2] over the target's axes, ascending; out_vals the replicated values (val_bytes 1/2/4/8). */
int spamd_coo_broadcast(int val_bytes, int64_t n, const int64_t* keys, const void* vals, int64_t b0, int64_t k1, int64_t b1,
                        int64_t k2, int64_t b2, int64_t* out_keys, void* out_vals, void* stream);

/* N1 (round 5): a dense array's stored elements in one pass (reference `COO.from_numpy`, _coo/core.py:341-384: the elements not
 * equal to the fill value and their positions).  vals[n] (val_bytes 1 / 2 / 4 / 8); fill_bits: the fill value's bit pattern;
 * cmp_mask: the bits compared (all ones = bit-identity; a floating type's mask without the sign bit + fill 0 = `value != 0`, the
 * test of the reference's COO-returning products `_common.py:1049, 1139`);
 * out_keys / out_vals: room for n entries, the first work[1] are written (indices ascending); work:
 * spamd_dense_nonfill_work_words(n) int64 words, zeroed here (a ticket, the count, one look-back word per 2048 elements). */
int64_t spamd_dense_nonfill_work_words(int64_t n);
int spamd_dense_nonfill(int val_bytes, int64_t n, const void* vals, uint64_t fill_bits, uint64_t cmp_mask, int64_t* work,
                        int64_t* out_keys, void* out_vals, void* stream);

/* ---------------------------------------------------------------------------------------
 * A9  SDDMM      out[n] = s[n] * sum_k A[rows[n], k] * Bt[cols[n], k]
 *   replaces the reference's formulation `s * (a @ b)` (examples/sddmm_example.py:51-52: a dense
 *   BLAS GEMM of the full M x N product + `_Elemwise` gather, _umath.py:602-633).
 *   A is M x K row-major (lda), Bt = B^T is N x K row-major (ldb): both K-contiguous, 16-byte
 *   aligned rows.  in_dtype BF16|F16|F32 -> fp32 accumulate and F32 mask/out; F64 -> F64.
 * ------------------------------------------------------------------------------------- */
int spamd_sddmm(int in_dtype, int s_dtype, int idx_dtype, int64_t nnz, const void* rows, const void* cols,
                const void* s_data, const void* A, int64_t lda, const void* Bt, int64_t ldb, int64_t K, void* out,
                void* stream);

/* A9 in column-panel order (same result, element for element, as spamd_sddmm; same reference formulation,
 * examples/sddmm_example.py:51-52).  When Bt does not fit an XCD's L2, a mask walked in row-major order fetches every
 * Bt row from the Infinity Cache.  spamd_sddmm_panel_keys gives keys[n] = cols[n] / width; the caller sorts them
 * stably (spamd_sort_pairs) into `perm`, gathers rows/cols/values by it (rows_p, cols_p, s_p), and spamd_sddmm_panels
 * walks the mask one panel of `width` Bt rows at a time, lane groups taking `chunk` elements per turn (<= 0: default):
 * out[perm[n]] = s_p[n] * <A[rows_p[n]], Bt[cols_p[n]]>, i.e. out keeps the mask's own order.  perm/rows_p/cols_p
 * depend on the coordinates only.  SPAMD_EINVAL when K has no row-cached kernel (call spamd_sddmm).
 * XCD-private panels (optional): with per_xcd = ceil(panels / 8) the keys are XCD-major, (panel % 8) * per_xcd + panel / 8,
 * xcd_first = int64[9] (device) holds the first element of each XCD's range in the sorted order (and the total) and
 * xcd_max the longest range; workgroup b then takes piece b / 8 of the range of XCD b % 8 (the observed placement: for
 * speed only), so that a panel's Bt rows are fetched into one L2 instead of eight.  NULL = all XCDs share every panel. */
int spamd_sddmm_has_panels(int in_dtype, int64_t K); /* 1: spamd_sddmm_panels has a kernel for this K */
int spamd_sddmm_panel_keys(int idx_dtype, int64_t nnz, const void* cols, int64_t width, int64_t per_xcd, void* keys,
                           void* stream);
/* Rows of exactly 1 KB (fp32 K = 256, fp64 K = 128, bf16 / f16 K = 512): with `part` (nnz words of the accumulator type - fp32, or
 * fp64 for F64 operands - of caller-owned scratch) the product runs as TWO passes over 512-byte half-rows (the first leaves its
 * sums in `part` in panel order, the second adds its half and writes s * sum), so that a panel holds twice the Bt rows in the
 * same L2 bytes and A is streamed half as often (config 4 fp32: 6.4 GB -> ~2.5 GB of fabric traffic); the panels are then
 * built for the row length spamd_sddmm_panel_row_bytes() reports (512).  part = NULL, or any other row length: one pass. */
int64_t spamd_sddmm_panel_row_bytes(int in_dtype, int64_t K); /* bytes of a Bt row the panel width is computed for */
int spamd_sddmm_panels(int in_dtype, int s_dtype, int idx_dtype, int64_t nnz, const void* rows_p, const void* cols_p,
                       const int64_t* perm, const void* s_p, const void* A, int64_t lda, const void* Bt, int64_t ldb,
                       int64_t K, int64_t chunk, const int64_t* xcd_first, int64_t xcd_max, void* part, void* out,
                       void* stream);

/* A9, dense-tile form (north_star: "MFMA used only on the dense tile of SDDMM"): the 32 x 32 tiles of the mask that
 * hold at least `threshold` samples are computed as one 32 x 32 x K bf16 product on the matrix cores
 * (v_mfma_f32_32x32x16_bf16, fp32 accumulate) and sampled from LDS; every other sample goes to spamd_sddmm.
 * Same reference formulation (examples/sddmm_example.py:51-52).  Plan: spamd_sddmm_tile_keys -> stable sort of the keys
 * with the sample index as payload (spamd_sort_pairs) -> spamd_flag_heads / spamd_exclusive_scan / spamd_compact give
 * seg_start[nseg + 1] -> spamd_sddmm_tile_classify -> scan + compact give the list of dense tiles and of left-over
 * samples.  bf16 operands (float16: spamd_sddmm_mfma_tiles_typed), K a multiple of 16, 16-byte aligned rows. */
int spamd_sddmm_tile_size(void);
int spamd_sddmm_tile_keys(int idx_dtype, int64_t nnz, const void* rows, const void* cols, int64_t tile_cols,
                          int64_t* keys, void* stream);
int spamd_sddmm_tile_classify(int64_t nseg, const int64_t* seg_start, int64_t threshold, int64_t* tile_flag,
                              int64_t* sample_flag, void* stream);
int spamd_sddmm_mfma_tiles(int idx_dtype, int64_t ntiles, const int64_t* tiles, const int64_t* seg_start,
                           const int64_t* keys_sorted, const int64_t* perm, int64_t tile_cols, int64_t M, int64_t N,
                           const void* rows, const void* cols, const float* s_data, const void* A, int64_t lda,
                           const void* Bt, int64_t ldb, int64_t K, float* out, void* stream);
/* The same with the operands' element type as an argument: in_dtype BF16 (= spamd_sddmm_mfma_tiles) | F16
 * (v_mfma_f32_32x32x16_f16: the same lane maps, tile plan and cycles).  Any other in_dtype: SPAMD_EINVAL. */
int spamd_sddmm_mfma_tiles_typed(int in_dtype, int idx_dtype, int64_t ntiles, const int64_t* tiles, const int64_t* seg_start,
                                 const int64_t* keys_sorted, const int64_t* perm, int64_t tile_cols, int64_t M, int64_t N,
                                 const void* rows, const void* cols, const float* s_data, const void* A, int64_t lda,
                                 const void* Bt, int64_t ldb, int64_t K, float* out, void* stream);

/* A9 with an N-D mask [l_1 .. l_p, M, N] over operands A [(leading), M, K] and Bt [(leading), N, K] whose leading axes
 * broadcast against the mask's (the same sampled product; the reference's `s * (a @ b)`, examples/sddmm_example.py:51-52,
 * broadcasts the dense product the same way): the fold of every stored element to the 2-D pair
 *   rows[n] = (sum_d coords[d][n] * a_strides[d]) * M + coords[p][n],   cols[n] = (sum_d coords[d][n] * b_strides[d]) * N + coords[p + 1][n]
 * with which spamd_sddmm / spamd_sddmm_panels / spamd_sddmm_mfma_tiles run on A as [Ba * M, K] and Bt as [Bb * N, K].
 * coords: [nlead + 2, nnz] of idx_dtype (I32 | I64), row pitch ldc elements; a_strides / b_strides: nlead HOST words, the
 * stride of each leading axis in the operand's batch ordinal (0 where the operand is broadcast); rows / cols: nnz words of
 * out_dtype I32 (the caller knows Ba * M and Bb * N fit) | I64.  One pass over the coordinates. */
int spamd_sddmm_batch_fold(int idx_dtype, int out_dtype, int nlead, int64_t nnz, const void* coords, int64_t ldc,
                           const int64_t* a_strides, const int64_t* b_strides, int64_t M, int64_t N, void* rows, void* cols,
                           void* stream);

/* A9 with complex operands (csrc/sddmm_complex.hip): val_dtype C64 | C128 is the type of s_data, A, Bt and out alike, the
 * product is the reference's `s * (a @ b)` (examples/sddmm_example.py:51-52) without conjugation, complex64 accumulates in
 * fp32 and complex128 in fp64.  lda / ldb are in complex elements; A, Bt and their row pitches are 16-byte aligned.
 * perm == NULL: the mask's own order, out[n] = s_data[n] * <A[rows[n]], Bt[cols[n]]>.  perm != NULL: the column-panel
 * order of spamd_sddmm_panels - rows / cols / s_data in panel order, out[perm[n]] = ..., lane groups taking perm_chunk
 * elements per turn (<= 0: default), xstate / xmax = xcd_first / xcd_max (NULL / 0: all XCDs share every panel) - with
 * the same bits as the mask's own order.  Rows that have a row-cached kernel (spamd_sddmm_complex_has_rowcache: 16-byte
 * vectors = L * KS, L in 16 | 32 | 64, KS in 1..4) take it, every other K the gather kernel; SPAMD_EINVAL when perm is
 * given for a K without the row-cached kernel.  Returns before any launch: 0 for nnz == 0, SPAMD_ETYPE for any other
 * value or index code, SPAMD_EINVAL for negative sizes and misaligned operands or pitches. */
int spamd_sddmm_complex(int val_dtype, int idx_dtype, int64_t nnz, const void* rows, const void* cols, const void* s_data,
                        const void* A, int64_t lda, const void* Bt, int64_t ldb, int64_t K, void* out, const int64_t* perm,
                        int64_t perm_chunk, const int64_t* xstate, int64_t xmax, void* stream);
int spamd_sddmm_complex_has_rowcache(int val_dtype, int64_t K); /* 1: rows of K complex values have the row-cached kernel */

/* =======================================================================================
 * A11  Complex elementwise functions, conversions and reductions (val_dtype C64 | C128; SPAMD_ETYPE otherwise)
 *   The formulas are NumPy's own loops, statement for statement, so that results are bit-identical to the reference's
 *   (which applies the ufunc to matched value arrays, sparse/numba_backend/_umath.py:420-470):
 *     multiply  re = fma(ar, br, -(ai * bi)), im = fma(ar, bi, ai * br), inner products rounded (NumPy's ARRAY loop
 *               fuses; the products of spamd_spmm_csr_complex / spamd_spgemm_expand are the unfused SCALAR product);
 *               square is the same with b = a
 *     divide    Smith's form, unfused: if |br| >= |bi|: both zero -> (ar / |br|, ai / |bi|); else rat = bi / br,
 *               scl = 1 / (br + bi * rat), re = (ar + ai * rat) * scl, im = (ai - ar * rat) * scl; otherwise rat = br / bi,
 *               scl = 1 / (bi + br * rat), re = (ar * rat + ai) * scl, im = (ai * rat - ar) * scl
 *     abs       hypot(re, im) of the device library (spamd_ewise_binary's op 13): within 4 ulp, the only inexact op
 *     others    componentwise; isnan / isinf: either part, isfinite: both; equal: both parts equal
 *   Arrays need 8-byte alignment; where every array of a call is 16-byte aligned each lane moves 16 bytes per access.
 * ------------------------------------------------------------------------------------- */
/* out[i] = a[i] (op) b[i]; *_is_scalar broadcasts a 1-element device array.  op: 0 add 1 subtract 2 multiply 3 divide
 * (out: val_dtype); 36 equal 37 not_equal (out: U8).  Any other op (power, ordered comparisons, maximum, logical_*, ...):
 * SPAMD_EINVAL - those functions of complex values are not device functions. */
int spamd_cplx_binary(int op, int val_dtype, int64_t n, const void* a, int a_is_scalar, const void* b, int b_is_scalar,
                      void* out, void* stream);
/* out[i] = f(a[i]); op: 0 negative 20 square 22 positive 96 conjugate (out: val_dtype); 1 absolute 97 real 98 imag (out: F32
 * for C64, F64 for C128); 64 isnan 65 isinf 66 isfinite (out: U8).  Any other op: SPAMD_EINVAL. */
int spamd_cplx_unary(int op, int val_dtype, int64_t n, const void* a, void* out, void* stream);
/* astype to complex: src_dtype F32 | F64 | I32 | I64 | U8 (imaginary part 0) or C64 | C128 (each part converted);
 * dst_dtype C64 | C128. */
int spamd_cplx_convert(int src_dtype, int dst_dtype, int64_t n, const void* src, void* dst, void* stream);
/* out[i] = (re, im), rounded to float32 parts for C64 */
int spamd_cplx_fill(int val_dtype, int64_t n, void* out, double re, double im, void* stream);
/* The fused merge-path union (spamd_merge_union with fill = 2) for complex values: tiles cut by spamd_merge_partition,
 * counts = spamd_merge_num_blocks(na, nb) + 2 int64 of workspace (zeroed here), counts[nblocks + 1] receives the number of
 * outputs, out_keys / out_vals hold na + nb elements.  op as spamd_cplx_binary.  The fill values are passed by HOST
 * address: fill_a / fill_b point to one value of val_dtype, fill_out to one value of val_dtype (ops 0-3) or to one byte
 * (ops 36, 37); results bit-identical to *fill_out (both parts) are dropped.  Only out_keys / out_vals [0, total) are written.
 * Returns before any launch or memset: SPAMD_EINVAL for na < 0, nb < 0, a null fill pointer or an op outside 0-3, 36, 37;
 * SPAMD_ETYPE for a val_dtype other than C64 | C128; 0 for na + nb == 0. */
int spamd_merge_union_complex(int op, int val_dtype, int64_t na, const int64_t* ka, const void* va, int64_t nb,
                              const int64_t* kb, const void* vb, const void* fill_a, const void* fill_b, const void* fill_out,
                              const int64_t* part, int64_t* counts, int64_t* out_keys, void* out_vals, void* stream);
/* Reduce the runs data[starts[g] .. starts[g + 1]) (starts: int64[nseg + 1], ascending; empty runs are not written), one
 * thread per run, in the order of the reference's `ufunc.reduceat` (_coo/core.py:1660), bit for bit:
 *   op 0 (add)       out[g] = x0 + P(x1 .. x(m-1)) per component, P = NumPy's pairwise sum over c complex values:
 *                    c < 4: from -0.0, left to right; c <= 64: four accumulators a_j = x_j, a_j += x_(4t+j) over the whole
 *                    groups of four, (a0 + a1) + (a2 + a3), then the remaining c mod 4 values left to right;
 *                    c > 64: P(first c1) + P(the rest), c1 = (c - c mod 8) / 2
 *   op 1 (multiply)  left to right with the unfused product (re = ar*br - ai*bi, im = ar*bi + ai*br)
 * max_len > 0: runs longer than max_len are skipped (their out[g] is left alone: spamd_cplx_sum_long is for them).
 * (spamd_segment_reduce with C64 / C128 stays the strictly-left-to-right sum of the sparse x sparse products.) */
int spamd_cplx_segment_reduce(int op, int val_dtype, int64_t n, const void* data, const int64_t* starts, int64_t nseg,
                              int64_t max_len, void* out, void* stream);
/* One long run of m >= 2 values in the same order as op 0 above: the leaves of the tree (at most 64 values each) are
 * summed by one thread each, the joins above them are done in the tree's own order, 8 levels per launch.  ws: workspace
 * of spamd_cplx_sum_long_ws_bytes(m) bytes (SPAMD_EWS when smaller).  out: one value.  The result does not depend on the
 * launch geometry. */
int64_t spamd_cplx_sum_long_ws_bytes(int64_t m);
int spamd_cplx_sum_long(int val_dtype, int64_t m, const void* run, void* out, void* ws, int64_t ws_bytes, void* stream);

/* =======================================================================================
 * A12  MTTKRP: matricised tensor times Khatri-Rao product (csrc/mttkrp.hip) - the reference's
 *   sparse.sum(B[:, :, :, None] * D[None, None, :, :] * C[None, :, None, :], axis=(1, 2))   (examples/mttkrp_example.py)
 *   for any mode of an N-D COO tensor, 2 <= ndim <= 8, without the two broadcast intermediates:
 *     out[i, r] = sum over stored elements n with coords[mode][n] == i of data[n] * prod_{d != mode} U_d[coords[d][n], r]
 *   val_dtype F32 | F64 is the type of data, every factor, the workspace and out; idx_dtype I32 | I64 the type of coords
 *   ([ndim, nnz], row pitch ldc elements, read at that width).  factors / pitches: HOST arrays of ndim device pointers and
 *   row pitches in elements (>= R); the entries at `mode` are ignored.  The plan groups the stored elements by
 *   coords[mode]: rowptr (int64[nrows + 1], nrows = shape[mode]) bounds row i's positions in plan order, perm (int64[nnz])
 *   maps a plan position to a stored position, NULL = the stored order (mode 0 of a canonical COO).
 *   Contract (same spirit as spamd_spmm_csr): every out element is written exactly once, by one lane; no atomics; results
 *   are bitwise reproducible and do not depend on the launch geometry.
 *     a term   t = data[n]; for d ascending, d != mode: t = t * U_d[coords[d][n], r], every product rounded
 *     a row    its elements, in plan order, are cut into pieces of `chunk` elements; a piece is summed sequentially from
 *              +0.0 and the piece sums are added in piece order (a row of at most `chunk` elements: one sequential sum;
 *              an empty row: +0.0)
 *   flags: SPAMD_EXACT_MULADD rounds every multiply and add separately; without it the last multiply of a term and the
 *   accumulate are one fma.  ws: spamd_mttkrp_ws_bytes(val_dtype, nnz, R, chunk) bytes (0 when nnz <= chunk; SPAMD_EWS
 *   when smaller).  out: nrows rows of pitch ldo >= R elements.
 *   Returns before any launch: SPAMD_ETYPE for other type codes, SPAMD_EINVAL for negative sizes, ndim outside 2..8, mode
 *   outside 0..ndim-1, a pitch below R or chunk < 1, 0 for R == 0 or nrows == 0; nnz == 0 zero-fills out and returns 0.
 * ------------------------------------------------------------------------------------- */
int64_t spamd_mttkrp_ws_bytes(int val_dtype, int64_t nnz, int64_t R, int64_t chunk);
int spamd_mttkrp(int val_dtype, int idx_dtype, int ndim, int mode, int64_t nnz, int64_t R, const void* coords, int64_t ldc,
                 const void* data, const void* const* factors, const int64_t* pitches, const int64_t* perm,
                 const int64_t* rowptr, int64_t nrows, int64_t chunk, void* ws, int64_t ws_bytes, void* out, int64_t ldo,
                 unsigned flags, void* stream);

/* =======================================================================================
 * A13  Masked SpGEMM: sparse x sparse product sampled at a sparse mask (csrc/masked_spgemm.hip) - the reference's
 *   s * (a @ b) with all three operands sparse (examples/triangles_example.py: sparse.sum(a @ a * a) / 6), without the product:
 *     out[e] = m[e] * sum over the k stored in both row i of A and column j of B of A[i, k] * B[k, j],  (i, j) = mask position e
 *   The mask (M x N) and A (M x K) come as CSR - row pointers (M + 1), column indices, values -, B (K x N) as CSC, i.e. the CSR
 *   arrays of B^T: b_ptr has N + 1 entries, b_idx holds row ids.  Index lists ascend inside a row / column and hold no
 *   duplicates.  idx_dtype I32 | I64 is the type of all six index arrays, val_dtype F32 | F64 | I32 | I64 the type of the three
 *   value arrays and of out (nnz values, in the mask's CSR order).  nnz = s_ptr[M].
 *   Contract (same spirit as spamd_mttkrp): every out element is written exactly once, by one lane; no atomic touches a
 *   value; results are bitwise reproducible and depend neither on the launch geometry nor on group / cap / window.
 *     acc = +0;  for every common k, ascending:  acc = acc + A[i, k] * B[k, j];   out = m * acc
 *   flags: SPAMD_EXACT_MULADD rounds every multiply and add on its own; without it the multiply and add of a term are one
 *   fma.  The mask multiply is always its own operation.  Integers wrap.  A position without a common k gets +0 (all-zero
 *   bits) whatever m is - also for a NaN or infinite m -, so the prune of the result removes it.
 *   group: lanes that walk one column of B together, 8 | 16 | 32 | 64.  cap: a row of A of at most cap entries (1 .. 2048) is
 *   searched in LDS, a longer one in global memory.  window: mask elements per wave (>= 1; values above nnz mean nnz); rows
 *   are cut at window bounds.  The arrays are trusted, as by every product entry point: pointers ascend from 0, s_idx < N,
 *   a_idx and b_idx < K (K itself is only checked for its sign: no array is sized by it).
 *   zeros (device uint64, may be NULL): receives the number of out values whose bits are all zero (one integer add per wave;
 *   zeroed by the call).
 *   Returns before any launch: SPAMD_ETYPE for other type codes, SPAMD_EINVAL for negative sizes or group / cap / window
 *   outside the above, 0 for nnz == 0, M == 0 or N == 0.  No workspace.
 * ------------------------------------------------------------------------------------- */
int spamd_masked_spgemm(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t K, int64_t nnz, const void* s_ptr,
                        const void* s_idx, const void* s_val, const void* a_ptr, const void* a_idx, const void* a_val,
                        const void* b_ptr, const void* b_idx, const void* b_val, int group, int cap, int64_t window, void* out,
                        void* zeros, unsigned flags, void* stream);

/* =======================================================================================
 * A14  softmax over the stored elements of a sparse array (csrc/softmax.hip, csrc/exp_det.h): unstored positions count as
 *   minus infinity, so the result has the stored structure of the input - the step between the scores of spamd_sddmm and the
 *   product that follows.  The reference has no softmax; the meaning is scipy.special.softmax of the dense array with -inf
 *   at the unstored positions, read back at the stored ones.
 *   The stored elements come grouped: segptr (idx_dtype I32 | I64, nseg + 1 entries ascending from 0 to nnz) bounds group
 *   g's positions in plan order; perm (int64[nnz], may be NULL = the stored order) maps a plan position to a stored
 *   position.  x and out (val_dtype F32 | F64, nnz values, out != x) are indexed by stored position.  An empty group writes
 *   nothing.  has_scale != 0: t_i = (T)scale * x_i, one multiply in the value type, before anything else; else t_i = x_i.
 *   Contract: every out element is written exactly once; no atomic touches a value; results are bitwise reproducible and
 *   depend neither on the launch geometry nor on group / short_max / max_len.  For one group t_0 .. t_{n-1} in plan order:
 *     m    = the maximum of the t_i.  Exact; any NaN makes it NaN; known before any exponential is taken (no online
 *            rescaling of partial sums); the sign of a zero maximum changes no result
 *     d_i  = t_i - m
 *     e_i  = exp_det(d_i): csrc/exp_det.h - k = rint(d * log2 e), two-constant Cody-Waite reduction in fmas, a Taylor
 *            polynomial in Horner fmas, ldexp; exp_det(+-0) = 1, exp_det(d) = +0 below the underflow threshold (-inf
 *            included), NaN for NaN.  Not the device math library's exp: every step is one exactly rounded IEEE operation
 *     s    = the group is cut into pieces of `chunk` elements.  A piece is summed by 64 accumulators - accumulator l adds
 *            the piece's elements l, l + 64, l + 128, .. in order - folded by halving: a[l] = a[l] + a[l + h] for h = 32,
 *            16, 8, 4, 2, 1.  The piece sums are added in piece order.  A group of at most `chunk` elements is one piece,
 *            so `chunk` enters the order of longer groups only
 *     p_i  = e_i / s, one correctly rounded division
 *   Hence: a group that holds a NaN or +inf, or only -inf, is NaN throughout; -inf beside finite values gives +0.0.
 *   group: lanes that own one short group, 8 | 16 | 32 | 64.  short_max (0 .. 64): groups of at most short_max elements take
 *   the sub-group form, longer ones up to `chunk` a wave each, longer ones pieces (five launches, each of which ends before
 *   the next reads its results: no workgroup waits for another).  chunk: a multiple of 64 in 64 .. 1024.  max_len: the
 *   length of the longest group, 0 .. nnz (the caller knows it from building segptr); it only decides which launches are
 *   made - a group longer than max_len may be left unwritten, nothing is read or written out of bounds for it.
 *   ws: spamd_softmax_ws_bytes(val_dtype, nnz, chunk) bytes (0 when nnz <= chunk), needed when max_len > chunk (SPAMD_EWS).
 *   The arrays are trusted, as by every entry point: segptr ascends from 0 to nnz, perm holds positions below nnz.
 *   Returns before any launch: SPAMD_ETYPE for other type codes; SPAMD_EINVAL for negative sizes, max_len > nnz, group /
 *   short_max / chunk outside the above, null pointers with work to do or out == x; 0 for nseg == 0, nnz == 0 or
 *   max_len == 0.
 * ------------------------------------------------------------------------------------- */
int64_t spamd_softmax_ws_bytes(int val_dtype, int64_t nnz, int64_t chunk);
int spamd_softmax(int val_dtype, int idx_dtype, int64_t nseg, int64_t nnz, const void* segptr, const int64_t* perm,
                  const void* x, int has_scale, double scale, int group, int64_t short_max, int64_t chunk, int64_t max_len,
                  void* ws, int64_t ws_bytes, void* out, void* stream);

/* =======================================================================================
 * A15  sparse attention (csrc/attention.hip): for every head h,
 *     out[h] = softmax_over_stored(scale * (s (.) (q[h] k[h]^T))) @ v[h]
 *   over the stored positions of ONE 2-D mask s (M x N) - the scores of spamd_sddmm, the softmax of A14 and the product by v
 *   fused, the scores never written for rows of at most `chunk` elements.  An unstored position counts as minus infinity; a
 *   stored zero of s, or a score that comes out 0, takes part as the value 0; a row without stored elements gives +0.0.
 *   The mask comes as CSR: s_ptr (idx_dtype I32 | I64, M + 1 entries ascending from 0 to nnz), s_idx (column ids, same type),
 *   s_val (val_dtype F32 | F64).  "Stored order" below is the order of these arrays.  q (H, M, D), k (H, N, D), v (H, N, Dv)
 *   are dense arrays of val_dtype whose last axis is contiguous: row r of head h of q starts at q + h * q_head + r * q_pitch
 *   (elements), likewise k and v.  out is (H, M, Dv), contiguous, of val_dtype.
 *   Contract: every operation is rounded once (an fma counts as one; there is no EXACT variant, as in A14); every out element
 *   is written exactly once; no atomic touches a value; results are bitwise reproducible and depend neither on the launch
 *   geometry nor on group / short_max / max_len.  For row r of one head, stored elements i = 0 .. n-1, columns c_i:
 *     w_i   = dot(q[r], k[c_i]) by 64 accumulators: accumulator l starts at +0.0 and takes a_l = fma(q[r][l + 64 j],
 *             k[c_i][l + 64 j], a_l) for j ascending (an element past D contributes nothing), then the accumulators are folded
 *             by halving, a[l] = a[l] + a[l + h] for h = 32, 16, 8, 4, 2, 1 - the tree A14 uses for its sums
 *     t_i   = s_i * w_i, one multiply; has_scale != 0: t_i = (T)scale * t_i, one more
 *     p_i   = exactly A14's result for the group t_0 .. t_{n-1} without a further scale, at the same `chunk`: the maximum
 *             before any exponential, exp_det, 64 accumulators per piece of `chunk`, one correctly rounded division
 *     out[r][j]: the elements are cut into pieces of `chunk`; a piece starts at +0.0 and takes acc = fma(p_i, v[c_i][j], acc)
 *             for i ascending; the piece sums are added in piece order, the first piece's sum being the start.  A row of at
 *             most `chunk` elements is one piece, so `chunk` enters the order of longer rows only
 *   Hence: a row whose scores hold a NaN or +inf, or only -inf, is NaN throughout its output row.
 *   group: lanes that own one short (row, head), 8 | 16 | 32 | 64.  short_max (0 .. 64): rows of at most short_max elements
 *   take the sub-group form, longer ones up to `chunk` a wave each (scores in LDS), longer ones pieces through the workspace
 *   (six launches, each of which ends before the next reads its results: no workgroup waits for another).  chunk: a multiple
 *   of 64 in 64 .. 1024.  max_len: the length of the longest row, 0 .. nnz; it only decides which launches are made.
 *   ws: spamd_attention_ws_bytes(val_dtype, nnz, H, Dv, chunk) bytes (0 when nnz <= chunk), needed when max_len > chunk
 *   (SPAMD_EWS).  The arrays are trusted, as by every entry point: s_ptr ascends from 0 to nnz, s_idx < N (N itself is only
 *   checked for its sign).
 *   Returns before any launch: SPAMD_ETYPE for other type codes; SPAMD_EINVAL for negative sizes, pitches or strides,
 *   max_len > nnz, group / short_max / chunk outside the above, or null pointers with work to do; 0 for M == 0, H == 0 or
 *   Dv == 0.  nnz == 0 writes +0.0 everywhere.
 *   spamd_attention_bias: the same with an additive bias per stored element and head (an edge encoding, a relative-position
 *   bias, a per-head mask).  bias (val_dtype) is read at the stored (CSR) position: element i of row r of head h, at the
 *   position pos = s_ptr[r] + i, takes b_i = bias[h * bias_head + pos] (elements; bias_head == 0: every head shares one bias of
 *   nnz values).  One step follows the two of t_i:
 *     t_i   = t_i + b_i, one add, rounded once, after the scale
 *   and p_i and out follow from these t_i exactly as above.  The rest is arithmetic: a bias of -inf gives p_i = +0.0 (a mask
 *   of that head's own), a row whose t_i are all -inf or hold a NaN or +inf is NaN; a bias of +0.0 everywhere gives the bits of
 *   spamd_attention; in a row of at most `chunk` elements a bias of -inf on the trailing elements gives the bits of the mask
 *   without them (fma(+0.0, v, acc) = acc for finite v).  bias == NULL is spamd_attention itself, bit for bit; bias_head < 0 is
 *   SPAMD_EINVAL.  The workspace is spamd_attention_ws_bytes: the long form parks the biased scores.
 *   spamd_attention_dropout: the same (bias may be NULL) with dropout on the probabilities.  The keep decision of the stored
 *   (CSR) position pos = s_ptr[r] + i of head h is word 0, x, of Philox4x32-10 (Salmon et al., Random123: multipliers
 *   0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85) under the key (seed low 32 bits, seed high 32 bits)
 *   of the counter (pos low, pos high, hn low, hn high), hn = head0 + h as a 64-bit value: keep_i iff x >= thr, thr =
 *   (uint32) floor(rate * 2^32) computed in double (exact for 0 <= rate < 1; the drop probability is thr / 2^32).  It is a
 *   function of (seed, hn, pos) alone: no state, no atomics, the same in every form and launch geometry; `seed` carries the
 *   64 bits of the unsigned seed.  After p_i:
 *     c     = (T)(1.0 / (1.0 - rate)), the division in double, rounded once to T
 *     pd_i  = keep_i ? p_i * c : +0.0, one multiply
 *   and out is the output loop above with pd_i in the place of p_i: a dropped element still takes part, as the value +0.0 (no
 *   compaction).  NaN, infinity and a row whose elements are all dropped follow from the arithmetic; such a row is +0.0 for
 *   finite v.  rate == 0 gives the bits of spamd_attention / spamd_attention_bias (their kernels run).  rate outside [0, 1)
 *   or NaN, or head0 < 0, is SPAMD_EINVAL before any launch; every other argument rule is spamd_attention_bias's.  The
 *   workspace is spamd_attention_ws_bytes.
 *   spamd_attention_keep: the decisions by themselves, from the same device code: out[h * nnz + p] = 1 when position pos0 + p
 *   of head head0 + h is kept, else 0, for h < H, p < nnz.  Negative nnz, H, pos0 or head0, a rate outside [0, 1), or a null
 *   out with work to do is SPAMD_EINVAL.
 * ------------------------------------------------------------------------------------- */
int64_t spamd_attention_ws_bytes(int val_dtype, int64_t nnz, int64_t H, int64_t Dv, int64_t chunk);
int spamd_attention(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D, int64_t Dv,
                    const void* s_ptr, const void* s_idx, const void* s_val, const void* q, int64_t q_pitch, int64_t q_head,
                    const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch, int64_t v_head,
                    int has_scale, double scale, int group, int64_t short_max, int64_t chunk, int64_t max_len, void* ws,
                    int64_t ws_bytes, void* out, void* stream);
int spamd_attention_bias(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D, int64_t Dv,
                         const void* s_ptr, const void* s_idx, const void* s_val, const void* q, int64_t q_pitch, int64_t q_head,
                         const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch, int64_t v_head,
                         int has_scale, double scale, int group, int64_t short_max, int64_t chunk, int64_t max_len,
                         const void* bias, int64_t bias_head, void* ws, int64_t ws_bytes, void* out, void* stream);
int spamd_attention_dropout(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D, int64_t Dv,
                            const void* s_ptr, const void* s_idx, const void* s_val, const void* q, int64_t q_pitch,
                            int64_t q_head, const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch,
                            int64_t v_head, int has_scale, double scale, int group, int64_t short_max, int64_t chunk,
                            int64_t max_len, const void* bias, int64_t bias_head, double rate, int64_t seed, int64_t head0,
                            void* ws, int64_t ws_bytes, void* out, void* stream);
int spamd_attention_keep(int64_t nnz, int64_t H, int64_t pos0, int64_t head0, double rate, int64_t seed, uint8_t* out,
                         void* stream);

/* =======================================================================================
 * A16 the backward pass of sparse attention (csrc/attention_grad.hip): from g = d loss / d out (H, M, Dv) of A15, for every
 *   head, dq (H, M, D), dk (H, N, D) and dv (H, N, Dv).  The gradient with respect to the mask values is not computed.
 *   The mask, q, k, v, has_scale and scale are A15's.  g has its own row pitch and head stride, last axis contiguous.  The
 *   column grouping is state of the pattern alone, built by the caller: c_ptr (idx_dtype, N + 1 entries ascending from 0 to
 *   nnz) bounds column c's elements in column order; c_perm (int64[nnz]) maps a position of the column order to a stored
 *   position, ascending within a column (a stable grouping: well defined for unsorted rows too); c_row (idx_dtype, nnz) is
 *   the row id of every element in column order.  dq, dk and dv are contiguous, of val_dtype.
 *   Contract: every operation is rounded once (an fma counts as one; there is no EXACT variant); every element of dq, dk and
 *   dv is written exactly once; no atomic touches a value; results are bitwise reproducible and depend neither on the launch
 *   geometry nor on group / col_group / short_max / max_row / max_col.
 *   Row pass - row r of one head, stored elements i = 0 .. n-1, columns c_i:
 *     t_i, p_i  exactly A15's w_i, t_i and p_i: the same bits as spamd_attention computes for the same inputs and `chunk`
 *     e_i   = dot(g[r], v[c_i]) by A15's 64 accumulators over Dv: a_l = fma(g[r][l + 64 j], v[c_i][l + 64 j], a_l) for j
 *             ascending from +0.0, folded by halving, h = 32 .. 1
 *     u_i   = p_i * e_i, one multiply
 *     delta = the sum of the u_i in A14's order: pieces of `chunk`; in a piece accumulator l holds the piece's element l and
 *             adds its elements l + 64, l + 128, .. in order (an accumulator without an element is +0.0); the fold by halving;
 *             the piece sums added in piece order, the first piece's sum being the start
 *     z_i   = p_i * (e_i - delta), one subtraction, then one multiply
 *     y_i   = s_i * z_i, one multiply; has_scale != 0: y_i = (T)scale * y_i, one more
 *     dq[r][j]: the elements are cut into pieces of `chunk`; a piece starts at +0.0 and takes acc = fma(y_i, k[c_i][j], acc)
 *             for i ascending; the piece sums are added in piece order, the first piece's sum being the start
 *   Column pass - column c of one head, its stored elements in stored order: positions pos_0 < .. < pos_{m-1}, rows r_i, cut
 *   into pieces of `chunk` by the same rule:
 *     dv[c][j]: acc = fma(p[pos_i], g[r_i][j], acc);   dk[c][j]: acc = fma(y[pos_i], q[r_i][j], acc)
 *   A row without stored elements gives a dq row of +0.0, a column without stored elements dk and dv rows of +0.0; nnz == 0
 *   writes +0.0 everywhere.  NaN and infinity follow from the arithmetic: a row whose forward row is NaN has a NaN dq row and
 *   hands NaN to the dk and dv rows of its columns.
 *   group (row pass) and col_group (column pass): lanes that own one short row or column, 8 | 16 | 32 | 64.  short_max
 *   (0 .. 64): rows / columns of at most short_max elements take the sub-group form, longer ones up to `chunk` a wave each,
 *   longer ones pieces through the workspace (launches that each end before the next reads their results: no workgroup
 *   waits for another).  chunk: a multiple of 64 in 64 .. 1024.  max_row / max_col: the longest row / column, 0 .. nnz; they
 *   only decide which launches are made.
 *   ws: spamd_attention_grad_ws_bytes(val_dtype, nnz, H, D, Dv, chunk) bytes, needed whenever nnz > 0 (SPAMD_EWS): p_i and
 *   y_i per stored element and head - written once by the row pass, read once by the column pass -, and for nnz > chunk the
 *   piece forms' statistics and piece outputs.  The arrays are trusted: s_ptr and c_ptr ascend from 0 to nnz, s_idx < N,
 *   c_row < M, c_perm is a permutation of 0 .. nnz-1.
 *   Returns before any launch: SPAMD_ETYPE for other type codes; SPAMD_EINVAL for negative sizes, pitches or strides,
 *   max_row or max_col above nnz, group / col_group / short_max / chunk outside the above, or null pointers with work to
 *   do; SPAMD_EWS; 0 when H == 0 or dq, dk and dv are all empty.
 *   spamd_attention_grad_bias: the backward pass of spamd_attention_bias.  bias and bias_head are as there; t_i and p_i are
 *   recomputed with the bias, the same bits as the forward's; e_i, u_i, delta, z_i, y_i, dq, dk and dv are as above.  One
 *   more output, the gradient with respect to the bias:
 *     dbias[h][pos] = z_i
 *   dbias is (H, nnz) contiguous of val_dtype, always per head (a shared bias's gradient is the caller's sum over h); every
 *   element is written exactly once, by the row pass in each of its three forms, without an atomic: it is as reproducible and
 *   as independent of group / col_group / short_max / max_row / max_col as dq.  dbias == NULL skips the store.  bias == NULL
 *   is spamd_attention_grad itself, bit for bit, and dbias is then not written; bias_head < 0 is SPAMD_EINVAL.  The
 *   workspace is spamd_attention_grad_ws_bytes.
 *   spamd_attention_grad_dropout: the backward pass of spamd_attention_dropout (bias and dbias may be NULL).  rate, seed and
 *   head0 are as there; t_i and p_i are the forward's, keep_i is recomputed from (seed, head0 + h, pos), c and pd_i are as
 *   there.  In the row pass
 *     ed_i  = keep_i ? e_i * c : +0.0, one multiply
 *     u_i   = p_i * ed_i;  delta as above over these u_i;  z_i = p_i * (ed_i - delta)
 *   and y_i, dq and dbias = z_i follow as above.  The row pass parks pd_i, not p_i, so the column pass is unchanged: dv takes
 *   fma(pd[pos_i], g[r_i][j], acc) and dk takes y.  rate == 0 gives the bits of spamd_attention_grad /
 *   spamd_attention_grad_bias (their kernels run).  rate outside [0, 1) or NaN, or head0 < 0, is SPAMD_EINVAL before any
 *   launch; every other argument rule is spamd_attention_grad_bias's.
 * ------------------------------------------------------------------------------------- */
int64_t spamd_attention_grad_ws_bytes(int val_dtype, int64_t nnz, int64_t H, int64_t D, int64_t Dv, int64_t chunk);
int spamd_attention_grad(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D, int64_t Dv,
                         const void* s_ptr, const void* s_idx, const void* s_val, const void* c_ptr, const int64_t* c_perm,
                         const void* c_row, const void* q, int64_t q_pitch, int64_t q_head, const void* k, int64_t k_pitch,
                         int64_t k_head, const void* v, int64_t v_pitch, int64_t v_head, const void* g, int64_t g_pitch,
                         int64_t g_head, int has_scale, double scale, int group, int col_group, int64_t short_max,
                         int64_t chunk, int64_t max_row, int64_t max_col, void* ws, int64_t ws_bytes, void* dq, void* dk,
                         void* dv, void* stream);
int spamd_attention_grad_bias(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D, int64_t Dv,
                              const void* s_ptr, const void* s_idx, const void* s_val, const void* c_ptr, const int64_t* c_perm,
                              const void* c_row, const void* q, int64_t q_pitch, int64_t q_head, const void* k, int64_t k_pitch,
                              int64_t k_head, const void* v, int64_t v_pitch, int64_t v_head, const void* g, int64_t g_pitch,
                              int64_t g_head, int has_scale, double scale, int group, int col_group, int64_t short_max,
                              int64_t chunk, int64_t max_row, int64_t max_col, const void* bias, int64_t bias_head, void* dbias,
                              void* ws, int64_t ws_bytes, void* dq, void* dk, void* dv, void* stream);
int spamd_attention_grad_dropout(int val_dtype, int idx_dtype, int64_t M, int64_t N, int64_t nnz, int64_t H, int64_t D, int64_t Dv,
                                 const void* s_ptr, const void* s_idx, const void* s_val, const void* c_ptr,
                                 const int64_t* c_perm, const void* c_row, const void* q, int64_t q_pitch, int64_t q_head,
                                 const void* k, int64_t k_pitch, int64_t k_head, const void* v, int64_t v_pitch, int64_t v_head,
                                 const void* g, int64_t g_pitch, int64_t g_head, int has_scale, double scale, int group,
                                 int col_group, int64_t short_max, int64_t chunk, int64_t max_row, int64_t max_col,
                                 const void* bias, int64_t bias_head, void* dbias, double rate, int64_t seed, int64_t head0,
                                 void* ws, int64_t ws_bytes, void* dq, void* dk, void* dv, void* stream);

/* =======================================================================================
 * A17  semiring products sparse @ dense -> dense (csrc/semiring_spmm.hip): the "add" is min or max, the "mul" plus or times,
 *     out[i, j] = min | max over the stored (i, k) of   a[i, k] + b[k, j]   |   a[i, k] * b[k, j]
 *     arg[i, j] = the k that was picked (int64; the argument a backward pass scatters through), -1 for none
 *   - GraphBLAS mxm over the (min | max, plus | times) semirings with a dense right operand: max / min neighbourhood
 *   aggregation, one Bellman-Ford relaxation (min.+), Viterbi (max.+), most-reliable path (max.x).  An unstored position is
 *   ABSENT (not the value 0); a stored zero takes part as the value 0.
 *   a comes as CSR: a_ptr (idx_dtype I32 | I64, M + 1 entries ascending from 0 to nnz), a_idx (inner indices below K, same type),
 *   a_val (val_dtype F32 | F64 | I32 | I64, nnz values).  b (K x N), init (M x N, may be NULL), out (M x N) are of val_dtype
 *   with row pitches ldb, ldi, ldo in elements (>= N), last axis contiguous; arg (int64, M x N, pitch lda) may be NULL - the
 *   kernels without it carry no arg registers and make no arg stores.  init is only read.
 *   Contract, for output (i, j) of a MIN semiring (MAX mirrored): with the stored elements of row i in stored order,
 *   e = 0 .. n - 1, inner indices k_e,
 *     t_e   = a[i, k_e] + b[k_e, j] (one add) or a[i, k_e] * b[k_e, j] (one multiply); integers wrap in two's complement (the
 *             operation is done on the unsigned type)
 *     seq   = [init[i, j]] (only when an init is given) followed by t_0 .. t_{n-1}
 *     pick  = the element numpy.argmin picks on seq: the first NaN if there is one, else the FIRST element that attains the
 *             minimum; -0.0 and +0.0 compare equal, so the first of them wins and keeps its sign bit
 *     out   = its value (the payload and sign of a NaN are no result); arg = its k_e, or -1 when the init was picked
 *   An empty seq (a row without stored elements and no init) gives the identity of the add - +inf / -inf, the integer type's
 *   max / min - and arg -1.  "First NaN, else leftmost minimum" of the pieces of any in-order split, combined left to right, is
 *   that of the whole: the result depends neither on narrow / group / chunk / max_len nor on the launch geometry.  No atomic
 *   touches a value or an arg; every output is written exactly once.
 *   add: SPAMD_SEMIRING_MIN | _MAX; mul: SPAMD_SEMIRING_PLUS | _TIMES.  narrow != 0: the lanes run ALONG a row, `group` of them
 *   per output element (results of few columns; the matrix-vector product), else `group` lanes own a row and each lane 16 bytes
 *   of contiguous output columns.  group: 8 | 16 | 32 | 64.  Rows longer than `chunk` (a multiple of 64 in 64 .. 2^30) are cut
 *   into pieces of `chunk` elements whose states go to the workspace and are folded in piece order by a second launch that
 *   starts after the first has ended.  max_len: the longest row's length, 0 .. nnz; it only decides whether the piece launches
 *   are made.  ws: spamd_semiring_spmm_ws_bytes(val_dtype, nnz, N, chunk, arg != NULL) bytes (0 when nnz <= chunk), needed
 *   when max_len > chunk (SPAMD_EWS).  The arrays are trusted, as by every entry point.
 *   Returns before any launch: SPAMD_ETYPE for other type codes; SPAMD_EINVAL for other add / mul codes, negative sizes,
 *   max_len > nnz, group / chunk outside the above, a pitch below N, null pointers with work to do; 0 for M == 0 or N == 0.
 * ------------------------------------------------------------------------------------- */
#define SPAMD_SEMIRING_MIN 0
#define SPAMD_SEMIRING_MAX 1
#define SPAMD_SEMIRING_PLUS 0
#define SPAMD_SEMIRING_TIMES 1
int64_t spamd_semiring_spmm_ws_bytes(int val_dtype, int64_t nnz, int64_t N, int64_t chunk, int with_arg);
int spamd_semiring_spmm(int val_dtype, int idx_dtype, int add, int mul, int64_t M, int64_t K, int64_t N, int64_t nnz,
                        const void* a_ptr, const void* a_idx, const void* a_val, const void* b, int64_t ldb, const void* init,
                        int64_t ldi, int narrow, int group, int64_t chunk, int64_t max_len, void* ws, int64_t ws_bytes, void* out,
                        int64_t ldo, int64_t* arg, int64_t lda, void* stream);

/* =======================================================================================
 * A18  the backward pass of A17 (csrc/semiring_grad.hip): from g = d loss / d out (M x N) and the forward's arg (M x N, int64),
 *   da (nnz values: the gradient with respect to a_val, in CSR stored order), db (K x N) and dinit (M x N).  Only arg is needed,
 *   not the add.  a_ptr / a_idx / a_val, b, mul, M, K, N, nnz are A17's; val_dtype is F32 | F64 (min / max of integers has no
 *   gradient here: SPAMD_ETYPE).  c_ptr (idx_dtype, K + 1 entries), c_perm (int64[nnz]) and c_row (idx_dtype, nnz) are the
 *   column grouping of the pattern exactly as A16 defines it.  b, arg, g, db and dinit have row pitches ldb, lda, ldg, lddb, lddi
 *   in elements (>= N), last axis contiguous; da is contiguous.  Nothing but da, db, dinit and ws is written.
 *   For output (i, j) with k* = arg[i][j]: k* == -1 - the init or the identity was picked - credits no element of a or b, and
 *   dinit[i][j] = g[i][j].  Otherwise the CREDITED elements are the stored elements e of row i with k_e == k*: exactly one in a
 *   pattern without duplicate coordinates; with duplicates every one of them is credited (this is not detected).  On a tie the
 *   element the forward picked gets everything - the subgradient torch.max(dim=..) takes.  For plus d t / d a_e = 1 and
 *   d t / d b[k][j] = 1; for times d t / d a_e = b[k_e][j] and d t / d b[k_e][j] = a_e.  arg is only ever COMPARED with stored
 *   indices, never used as an address: a value that is no index of row i credits nothing.
 *   Contract, with hit(e, j) = (arg[i_e][j] == k_e): every operation is rounded once (an fma counts as one); every output
 *   element is written exactly once; no atomic touches a value; the result depends neither on group / col_group / short_max /
 *   max_col nor on the launch geometry (`chunk` is part of the order of db, as in A16).
 *     da[e], element e of row i, k = k_e, by A15's 64 accumulators over the N columns: accumulator l starts at +0.0 and takes
 *             j = l, l + 64, l + 128, .. in ascending order; on a hit a_l = a_l + g[i][j] (plus) or a_l = fma(g[i][j], b[k][j], a_l)
 *             (times), on no hit a_l is unchanged; the 64 accumulators are then folded by halving, h = 32 .. 1.  da[e] depends on
 *             its own row of arg / g and its own b row alone: there is no long-row form, the pass runs over windows of stored
 *             positions
 *     db[k][j], column k, its stored elements in stored order: positions pos_0 < .. < pos_{m-1} with rows r_i from c_ptr /
 *             c_perm / c_row, cut into pieces of `chunk` elements by A16's rule; a piece starts at +0.0; on a hit at (pos_i, j)
 *             acc = acc + g[r_i][j] (plus) or acc = fma(a_val[pos_i], g[r_i][j], acc) (times), on no hit acc is unchanged; the
 *             piece sums are added in piece order, the first piece's sum being the start.  A column without stored elements
 *             gives +0.0
 *     dinit[i][j] = arg[i][j] == -1 ? g[i][j] : +0.0
 *   NaN and infinity in g follow from the arithmetic and reach only credited elements (and, through dinit, the init).
 *   Any of da, db, dinit may be NULL: the pass that serves only a NULL output is not launched (element pass: da; column pass:
 *   db; one elementwise launch: dinit).  For plus neither a_val nor b is read and both may be NULL; the element pass reads
 *   neither a_val nor the column grouping, the column pass neither a_ptr, a_idx nor b.
 *   group (element pass): 8 | 16 | 32 | 64 lanes run along the columns of one stored element.  col_group (column pass):
 *   8 | 16 | 32 | 64 lanes own a column of at most short_max (0 .. 64) elements, 16 bytes of contiguous output columns a lane;
 *   col_group 1 (N <= 4 only): a lane owns all outputs of such a column.  Columns up to `chunk` (a multiple of 64 in
 *   64 .. 2^30) elements take a wave each, longer ones pieces through the workspace and a join launch that starts after the
 *   piece launch has ended: no workgroup waits for another.  max_col: the longest column, 0 .. nnz; it only decides which
 *   launches are made.  ws: spamd_semiring_grad_ws_bytes(val_dtype, nnz, N, chunk) bytes (0 when nnz <= chunk), needed when db
 *   is wanted and max_col > chunk (SPAMD_EWS).  The arrays are trusted, as by every entry point.
 *   Returns before any launch: SPAMD_ETYPE for other type codes (the integer value types too); SPAMD_EINVAL for another mul
 *   code, negative sizes, max_col > nnz, group / col_group / short_max / chunk outside the above, a pitch below N, null
 *   pointers with work to do; SPAMD_EWS; 0 when da, db and dinit are all NULL or empty.
 * ------------------------------------------------------------------------------------- */
int64_t spamd_semiring_grad_ws_bytes(int val_dtype, int64_t nnz, int64_t N, int64_t chunk);
int spamd_semiring_grad(int val_dtype, int idx_dtype, int mul, int64_t M, int64_t K, int64_t N, int64_t nnz, const void* a_ptr,
                        const void* a_idx, const void* a_val, const void* c_ptr, const int64_t* c_perm, const void* c_row,
                        const void* b, int64_t ldb, const int64_t* arg, int64_t lda, const void* g, int64_t ldg, int group,
                        int col_group, int64_t short_max, int64_t chunk, int64_t max_col, void* ws, int64_t ws_bytes, void* da,
                        void* db, int64_t lddb, void* dinit, int64_t lddi, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_AMD_H */
