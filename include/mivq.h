/*
 * mivq.h — C ABI of libmivq.so, the MI355X-native (gfx950) vector-quantization hot path.
 *
 * This is the drop-in boundary that replaces the faiss / numpy calls the reference's
 * quantizer classes make (citations are /root/reference/<path>:<line>).  Every entry
 * point is `extern "C"`, takes plain pointers and sizes, and is stream-ordered:
 *
 *   - Ownership: every buffer is caller-allocated DEVICE memory (e.g. a torch tensor's
 *     data_ptr()).  The library never allocates persistent memory; kernels that need
 *     scratch take an explicit workspace (size from the matching *_workspace_bytes()).
 *     A call writes its outputs and its workspace and nothing else, and does not depend on
 *     what the workspace or an output held before; a workspace that is null or smaller
 *     than the size query's is MIVQ_ERR_WORKSPACE, reported before any launch (DESIGN.md,
 *     "Buffer contract").
 *   - Errors: 0 on success, a negative MIVQ_ERR_* code otherwise; the message is kept in
 *     a thread-local buffer readable with mivq_last_error().  The Python host raises the
 *     same exception types the reference raises (AssertionError / ValueError /
 *     RuntimeError, see vector-quantization_amd/haag_vq/_native.py).
 *   - Threading: asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     legacy default stream of the current device).  Safe to call concurrently from
 *     several host threads on different streams or devices; no global mutable state
 *     besides the per-thread error string.  No call synchronises the device.
 *   - Codes: PQ codes follow faiss' ProductQuantizer layout (code_size = ceil(M*nbits/8)
 *     bytes per vector, sub-code m in bits [m*nbits, (m+1)*nbits) of the little-endian
 *     bit stream; nbits == 8 is one byte per subspace).  Centroids are laid out
 *     (M, ksub, dsub) f32, exactly `pq.centroids.reshape(M, ksub, dsub)` of
 *     product_quantization.py:72-73.
 */
#ifndef MIVQ_H
#define MIVQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define MIVQ_OK 0
#define MIVQ_ERR_INVALID (-1)     /* bad shape / argument            -> ValueError / AssertionError */
#define MIVQ_ERR_UNSUPPORTED (-2) /* configuration not implemented   -> ValueError */
#define MIVQ_ERR_HIP (-3)         /* HIP runtime / launch failure    -> RuntimeError */
#define MIVQ_ERR_WORKSPACE (-4)   /* workspace too small             -> RuntimeError */

#define MIVQ_ABI_VERSION 2 /* 2: mivq_adc_search takes flags */

/* PQ encode flags */
#define MIVQ_PQ_AUTO 0u        /* fp16-MFMA candidate filter + exact fp32 re-check when supported */
#define MIVQ_PQ_FORCE_EXACT 1u /* exact fp32 VALU scan of every centroid (canonical order)     */
#define MIVQ_PQ_LEGACY_MFMA 2u /* diagnostic: subspace-looping MFMA kernel + separate resolve */
#define MIVQ_PQ_LEGACY_EXACT 4u /* diagnostic: lane-per-row exact kernel instead of the tiled one */

/* Metric enum values follow faiss / haag_vq.utils.faiss_utils.MetricType (faiss_utils.py:3-5). */
#define MIVQ_METRIC_INNER_PRODUCT 0
#define MIVQ_METRIC_L2 1

/* ---------------------------------------------------------------- misc */
const char* mivq_last_error(void);
int mivq_abi_version(void);
/* Fills name (>= 64 bytes), compute units, LDS bytes per CU, and total HBM bytes of `device`. */
int mivq_device_info(int device, char* name, int32_t* cus, int64_t* lds_per_cu, int64_t* hbm_bytes);

/* ------------------------------------------------------ product quantizer
 * Replaces faiss.ProductQuantizer.compute_codes / decode behind
 * ProductQuantizer.compress / decompress (product_quantization.py:76-86).
 *
 * Canonical encode (what "bit-exact" is measured against, see oracle/mivq_oracle.c):
 *   cn[m][k]  = fmaf-chain over t ascending of c[m][k][t]^2
 *   dot       = fmaf-chain over t ascending of x[m*dsub+t] * c[m][k][t]   (starts at +0)
 *   score_k   = fl32(cn[m][k] - 2*dot)
 *   code[m]   = smallest k with the minimum score (scores that are NaN never win; an
 *               all-NaN row gives 0).
 */

/* Bytes of the derived codebook data ("prep") for mivq_pq_encode. */
size_t mivq_pq_prep_bytes(int32_t d, int32_t M, int32_t nbits);
/* Builds prep from centroids (device): canonical norms, the fp16 MFMA operand image and
 * the per-subspace rounding-bound constants.  Re-run whenever the centroids change. */
int mivq_pq_prepare(const float* centroids, int32_t d, int32_t M, int32_t nbits, void* prep,
                    void* stream);
size_t mivq_pq_encode_workspace_bytes(int64_t n, int32_t d, int32_t M, int32_t nbits);
/* x: (n, d) f32 row-major; codes: (n, code_size) u8; prep from mivq_pq_prepare (required;
 * the exact path reads its canonical norms and transposed codebook). */
int mivq_pq_encode(const float* x, int64_t n, int32_t d, int32_t M, int32_t nbits,
                   const float* centroids, const void* prep, void* workspace,
                   size_t workspace_bytes, uint8_t* codes, uint32_t flags, void* stream);
/* out: (n, d) f32: out[i, m*dsub:(m+1)*dsub] = centroids[m, code_m(i), :]. */
int mivq_pq_decode(const uint8_t* codes, int64_t n, int32_t d, int32_t M, int32_t nbits,
                   const float* centroids, float* out, void* stream);
/* faiss bit-stream <-> one byte per sub-code (identity copy for nbits == 8). */
int mivq_pq_unpack(const uint8_t* codes, int64_t n, int32_t M, int32_t nbits, uint8_t* out,
                   void* stream);

/* ---------------------------------------------------- k-means (PQ fit)
 * Deterministic centroid update for the per-subspace Lloyd iterations that replace
 * faiss' ProductQuantizer.train (product_quantization.py:67-68): sums[m][k][t] are
 * accumulated over assigned rows in ascending row order, centroids = sums / count for
 * non-empty clusters (empty clusters keep their previous value and report count 0).
 * assign: (n, M) u8 (one byte per subspace, the output of mivq_pq_encode with nbits 8
 * or of mivq_pq_unpack).  counts: (M, ksub) int32. */
int mivq_kmeans_update(const float* x, int64_t n, int32_t d, int32_t M, int32_t ksub,
                       const uint8_t* assign, float* centroids, int32_t* counts, void* stream);

/* ------------------------------------------------------ OPQ rotation
 * Replaces faiss.OPQMatrix.apply / reverse_transform
 * (optimized_product_quantization.py:26,31,34).  A is (d, d) f32 row-major.
 *   transpose == 0 : y = x . A^T   (apply)
 *   transpose == 1 : y = x . A     (reverse_transform of an orthonormal A) */
int mivq_opq_rotate(const float* x, int64_t n, int32_t d, const float* A, int32_t transpose,
                    float* y, void* stream);

/* The same rotation at f16-MFMA speed with fp32 accuracy (the product path of
 * OptimizedProductQuantizer): mivq_opq_prepare splits op(A) once into scaled f16 hi / lo
 * images (prep: mivq_opq_prep_bytes(d) bytes, 16-byte aligned; 0 when d % 8 != 0), and
 * mivq_opq_rotate_prepared computes y = x . op(A) as x_hi b_hi + x_hi b_lo + x_lo b_hi with
 * per-row power-of-two scales of x.  Workspace (16-byte aligned):
 * mivq_opq_rotate_workspace_bytes(n, d) = the row scales (4 n B, rounded up to 256 B). */
size_t mivq_opq_prep_bytes(int32_t d);
int mivq_opq_prepare(const float* A, int32_t d, int32_t transpose, void* prep, void* stream);
size_t mivq_opq_rotate_workspace_bytes(int64_t n, int32_t d);
int mivq_opq_rotate_prepared(const float* x, int64_t n, int32_t d, const void* prep, void* workspace,
                             size_t workspace_bytes, float* y, void* stream);
/* Training: G = X^T Y in fp64 (d, d) row-major for the OPQ orthogonal-Procrustes update
 * (OPQMatrix::train's X^T Yhat, optimized_product_quantization.py:21-28); x, y: (n, d) f32.
 * fp64 MFMA, split over rows, the parts added in a fixed order (deterministic).  Workspace:
 * mivq_opq_gram_workspace_bytes(n, d) bytes, 8-byte aligned. */
size_t mivq_opq_gram_workspace_bytes(int64_t n, int32_t d);
int mivq_opq_gram(const float* x, const float* y, int64_t n, int32_t d, void* workspace,
                  size_t workspace_bytes, double* G, void* stream);

/* ------------------------------------------------------ scalar quantizer
 * Replaces ScalarQuantizer._compress_block / decompress (scalar_quantization.py:52-90)
 * bit-for-bit, in the dtype numpy would compute in (f32 input -> f32 math, f64 -> f64).
 *   lo  = X.min(0), den = (X.max(0) - X.min(0)) + 1e-8 (computed by the caller exactly as
 *   numpy does); codes: u8 for nbits 4 (two dims per byte, even dim in the high nibble,
 *   odd d zero-padded) and 8, u16 for nbits 16.  Decode returns f32 for the f32 variant
 *   and f64 for the f64 variant (what numpy returns). */
int mivq_sq_encode_f32(const float* x, int64_t n, int32_t d, const float* lo, const float* den,
                       int32_t nbits, void* codes, void* stream);
int mivq_sq_encode_f64(const double* x, int64_t n, int32_t d, const double* lo,
                       const double* den, int32_t nbits, void* codes, void* stream);
int mivq_sq_decode_f32(const void* codes, int64_t n, int32_t d, const float* lo,
                       const float* den, int32_t nbits, float* out, void* stream);
int mivq_sq_decode_f64(const void* codes, int64_t n, int32_t d, const double* lo,
                       const double* den, int32_t nbits, double* out, void* stream);

/* ------------------------------------------------------ LVQ (1..8 bits, per-vector range)
 * Replaces LVQQuantizer.fit / compress / decompress (lvq_quantization.py:42-142) bit-for-bit,
 * fp32, one rounding per step; L = 2^nbits - 1, nbits in [1, 8] (else MIVQ_ERR_INVALID).
 *   column_mean: mean_t = (x_0t + x_1t + ... in ascending row order) / (float)n, what numpy's
 *                X.mean(axis=0) gives for a C-contiguous f32 array (the quantizer's mu); n >= 1.
 *   encode: r_t = x_t - mu_t, lo = min r, hi = max r, delta = (hi - lo) == 0 ? FLT_MIN :
 *           (hi - lo) / L, idx_t = clip((int)rint((r_t - lo) / delta), 0, L), rint half to even.
 *   Code row = ceil(d*nbits/8) index bytes (idx_t in bits [t*nbits, (t+1)*nbits) of the row's
 *           bit stream, MSB-first from byte 0 = np.packbits(bitorder='big'), padding bits 0)
 *           followed by f32 lo and f32 delta, little-endian; code_size = ceil(d*nbits/8) + 8.
 *   decode: out_t = (lo + (float)idx_t * delta) + mu_t.
 * Inputs are finite; a row holding NaN encodes to unspecified bytes of its own row. */
int mivq_column_mean(const float* x, int64_t n, int32_t d, float* mean, void* stream);
int mivq_lvq_encode(const float* x, int64_t n, int32_t d, const float* mu, int32_t nbits,
                    uint8_t* codes, void* stream);
int mivq_lvq_decode(const uint8_t* codes, int64_t n, int32_t d, const float* mu, int32_t nbits,
                    float* out, void* stream);

/* ------------------------------------------------------ two-level LVQ (LVQ-B1xB2)
 * A second level quantises what the first left over, on the interval the first level's step
 * fixes, so it stores no constants of its own.  B1 = nbits1 in [1, 8] (else MIVQ_ERR_INVALID),
 * B2 = nbits2 in {4, 8} (else MIVQ_ERR_UNSUPPORTED), L1 = 2^B1 - 1, L2 = 2^B2 - 1; fp32, one
 * rounding per step, every division IEEE:
 *   level 1: r_t, lo, delta, idx_t exactly as mivq_lvq_encode(x, ..., nbits1).
 *   level 2: a_t = lo + (float)idx_t * delta, e_t = r_t - a_t, lo2 = -0.5f * delta,
 *           delta2 = delta / (float)L2 (subnormal where delta is FLT_MIN: kept, not flushed),
 *           j_t = clip((int)rint((e_t - lo2) / delta2), 0, L2), rint half to even.
 *   codes1 = (n, ceil(d*B1/8) + 8): the rows of mivq_lvq_encode at nbits1, byte for byte.
 *   codes2 = (n, ceil(d*B2/8)): j_t in bits [t*B2, (t+1)*B2) of the row's bit stream, MSB-first
 *           from byte 0 (B2 = 4: the even dimension in the high nibble), padding bits 0, no
 *           trailer.  Either array at any byte alignment.
 *   decode: out_t = ((lo + (float)idx_t * delta) + (lo2 + (float)j_t * delta2)) + mu_t, lo2 and
 *           delta2 recomputed from the row's delta.
 * Inputs are finite; a row holding NaN encodes to unspecified bytes of its own two rows.  The
 * other checks are those of mivq_lvq_encode / mivq_lvq_decode. */
int mivq_lvq2_encode(const float* x, int64_t n, int32_t d, const float* mu, int32_t nbits1,
                     int32_t nbits2, uint8_t* codes1, uint8_t* codes2, void* stream);
int mivq_lvq2_decode(const uint8_t* codes1, const uint8_t* codes2, int64_t n, int32_t d,
                     const float* mu, int32_t nbits1, int32_t nbits2, float* out, void* stream);

/* ------------------------------------------------------ RaBitQ (1 bit)
 * Replaces faiss.RaBitQuantizer.compute_codes / decode (rabit_quantization.py:20-29).
 * Code row = ceil(d/8) sign bytes (bit j of dim j = (x_j - c_j) > 0, LSB-first) followed by
 * two f32 factors {||x-c||^2, dp_multiplier}; code_size = ceil(d/8) + 8.
 * centroid may be NULL (faiss' default: no centroid). */
int mivq_rabitq_encode(const float* x, int64_t n, int32_t d, const float* centroid,
                       int32_t metric, uint8_t* codes, void* stream);
int mivq_rabitq_decode(const uint8_t* codes, int64_t n, int32_t d, const float* centroid,
                       float* out, void* stream);
/* RaBitQ estimator search: replaces faiss.IndexRaBitQ.search behind RaBitQIndex
 * (methods/search/rabitq_index.py:42-70; qb = IndexRaBitQ.qb query bits, 0..8).  codes: (n,
 * code_size) rows from mivq_rabitq_encode with the same centroid (IndexRaBitQ's center);
 * q: (nq, d) f32.  Per query r = q - c is quantised to qb bits (min/max grid, round half up);
 * the estimate of ||q - x||^2 is  f0 + ||r||^2 - 2 f1 <r', bits>-term  (arithmetic:
 * oracle/mivq_oracle.c oracle_rabitq_est).  dists/ids: (nq, k) ascending keys, ties to the
 * smaller id; L2 keys are the distance estimates, INNER_PRODUCT keys the negated
 * inner-product estimates.  ids = id_offset + row.  Workspace from
 * mivq_rabitq_search_workspace_bytes.  With qb = 0, d % 32 != 0 or codes not 4-byte aligned
 * (the generic estimator, whose grid is (code blocks, nq)) a call takes nq <= 65535 queries
 * and returns MIVQ_ERR_UNSUPPORTED above that, before any launch; pass ranges of queries. */
size_t mivq_rabitq_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k);
int mivq_rabitq_search(const uint8_t* codes, int64_t n, int32_t d, const float* centroid,
                       const float* q, int64_t nq, int32_t qb, int32_t metric, int32_t k,
                       int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists,
                       uint32_t* ids, void* stream);

/* ------------------------------------------------------ Extended RaBitQ (B bits)
 * The element-wise / per-row steps of ExtendedRaBitQuantizer.compress / decompress
 * (extended_rabitq.py:125-199), fp64 like the reference, and the two D x D rotations
 * between them (o . P and o_hat . P^T, :140 and :196) as an fp64-MFMA GEMM.
 *   normalize : o = (x - c) / max(||x - c||, 1e-12), nrm = ||x - c||   (x f32 or f64)
 *   quantize  : s = s_raw * sqrt(D); idx = searchsorted(mid-levels, s); t = <s,s_hat>/<s_hat,s_hat>
 *               code row = MSB-first B-bit indices (ceil(D*B/8) bytes) ++ f32 nrm ++ f32 t
 *   dequantize: o_hat = (levels[idx] / sqrt(D)) * t
 *   finish    : x_hat = f32(y * nrm + c)  with y = o_hat . P^T */
int mivq_extrabitq_normalize(const void* x, int32_t x_is_f64, int64_t n, int32_t d,
                             const double* centroid, double* o, double* nrm, void* stream);
int mivq_extrabitq_quantize(const double* s_raw, int64_t n, int32_t d, const double* levels,
                            int32_t nbits, const double* nrm, uint8_t* codes, void* stream);
int mivq_extrabitq_dequantize(const uint8_t* codes, int64_t n, int32_t d, const double* levels,
                              int32_t nbits, double* o_hat, void* stream);
int mivq_extrabitq_finish(const double* y, int64_t n, int32_t d, const uint8_t* codes,
                          int32_t nbits, const double* centroid, float* out, void* stream);
/* s = o . P (transpose 0) or o . P^T (transpose 1); o, s: (n, d) f64 row-major, P: (d, d). */
int mivq_extrabitq_rotate(const double* o, int64_t n, int32_t d, const double* P, int32_t transpose,
                          double* s, void* stream);
/* Exact top-k over Extended RaBitQ codes, undecoded, in the rotated domain.  P is orthogonal and
 * x_hat = (o_hat . P^T) nrm + c, so ||q - x_hat||^2 = ||(q - c) P - y_hat||^2 and
 * <q, x_hat> = <q P, y_hat> + <q, c> with y_hat = o_hat nrm: the caller rotates the queries
 * (qy = (q - c) P for L2, q P for inner product; (nq, d) f32) and the rows are scanned as codes.
 *   o_hat_t = dmul(ddiv(levels[idx_t], sqrt((double)d)), (double)t)   the bits dequantize writes
 *   y_hat_t = (float)dmul(o_hat_t, (double)nrm)                       one more fp64 product, one rounding
 *   L2: dist = fmaf chain over t ascending of (qy_t - y_hat_t)^2, the difference rounded once
 *   IP: dist = -(fmaf chain over t ascending of qy_t * y_hat_t)
 * idx_t is the B bits at bit t*B of the row, MSB first; nrm and t are the two trailer floats in
 * that order; bits past d*B in the last code byte are ignored; rows may start at any byte.
 * The k smallest (dist, id) per query, every convention of mivq_flat_search (ascending, ties to
 * the smaller id, NaN as +inf, missing slots (+inf, 0xFFFFFFFF), id = id_offset + row): the
 * result is bit-identical to mivq_flat_search(qy, y_hat).  levels: 2^nbits f64 on the device,
 * nbits in [1, 8], k <= 256.  The workspace holds top-k lists or a block of keys, never rows. */
size_t mivq_extrabitq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k);
int mivq_extrabitq_flat_search(const float* qy, int64_t nq, const uint8_t* codes, int64_t n, int32_t d,
                               const double* levels, int32_t nbits, int32_t metric, int32_t k,
                               int64_t id_offset, void* workspace, size_t workspace_bytes,
                               float* dists, uint32_t* ids, void* stream);

/* ------------------------------------------------------ Rank-aware quantizer (PCA + bits per dimension)
 * The per-row steps of RankAwareQuantizer.compress / decompress (rank_aware_quantization.py),
 * fp64 like the reference; the two D x D products between them (xc . V, y_hat . V^T) are
 * mivq_extrabitq_rotate.  The code format is four device tables:
 *   lv     (T,)    f64    the level tables of all dimensions, concatenated (ascending within a
 *                         dimension; a 0-bit dimension has its one level)
 *   lv_off (d + 1,) int32 start of dimension j's 2^width[j] levels in lv
 *   width  (d,)    int32  bits of dimension j, 0..8
 *   pos    (d,)    int32  bit position of the most significant bit of j's field in the code row,
 *                         counted MSB-first from the start of the row (bit p is bit 7 - p % 8 of
 *                         byte p / 8); ignored where width is 0.  Fields do not overlap and
 *                         pos + width <= 8 * code_size (the caller's duty; a field that breaks
 *                         this, or a width outside 0..8, is treated as width 0).
 *   center    : xc = (double)x - mu                          x (n, d) f32 or f64, mu (d,) f64
 *   quantize  : idx_j = #{ q : 0.5 (L[q] + L[q+1]) < y_j },  L = lv + lv_off[j]
 *               (np.searchsorted, side left: a y on a mid-level takes the lower index, -inf
 *               gives 0, +inf and NaN give 2^w - 1); codes (n, code_size): idx_j in width[j]
 *               bits, MSB first, from bit pos[j]; every bit of no field is 0
 *   dequantize: y_hat_j = L[idx_j], idx_j the width[j] bits at pos[j] (0 for width 0); bits of
 *               no field are ignored, and no byte pattern indexes outside a dimension's levels
 *   finish    : out = (float)(z + mu)                        z (n, d) f64, out (n, d) f32
 * n < 0, d <= 0, code_size <= 0 or a null pointer with n > 0 return MIVQ_ERR_INVALID before any
 * launch; n == 0 returns MIVQ_OK without one; code_size above 48000 bytes (quantize, dequantize: the rows' codes
 * are held in LDS) is MIVQ_ERR_UNSUPPORTED. */
int mivq_rankaware_center(const void* x, int32_t x_is_f64, int64_t n, int32_t d, const double* mu,
                          double* xc, void* stream);
int mivq_rankaware_quantize(const double* y, int64_t n, int32_t d, const double* lv,
                            const int32_t* lv_off, const int32_t* pos, const int32_t* width,
                            int32_t code_size, uint8_t* codes, void* stream);
int mivq_rankaware_dequantize(const uint8_t* codes, int64_t n, int32_t d, const double* lv,
                              const int32_t* lv_off, const int32_t* pos, const int32_t* width,
                              int32_t code_size, double* y_hat, void* stream);
int mivq_rankaware_finish(const double* z, int64_t n, int32_t d, const double* mu, float* out,
                          void* stream);

/* Exact top-k over rank-aware codes in the rotated domain, without decoding them.  V is
 * orthogonal and x^ = y^ . V^T + mu, so ||q - x^||^2 = ||(q - mu) V - y^||^2 and
 * <q, x^> = <q V, y^> + <q, mu>: the caller passes the rotated queries qy (nq, d) f32 (L2:
 * (q - mu) V, IP: q V) and, for IP, adds <q, mu> to the scores it gets back.
 *   y^_{i,t} = lv32[lv_off[t] + idx_{i,t}], idx_{i,t} the width[t] bits at bit pos[t] of row i,
 *              read exactly as mivq_rankaware_dequantize reads them (width 0: index 0, the
 *              table's one entry; bits of no field are ignored; a field outside the row or a
 *              width outside 0..8 is width 0; no byte pattern indexes outside a table).
 *              lv32 is lv rounded to f32 (round to nearest), same offsets.
 *   L2: dist = fmaf chain over t ascending of (qy_t - y^_t)^2, the difference one rounding
 *   IP: dist = -(fmaf chain over t ascending of qy_t y^_t)
 * Zero-width dimensions keep their place in the chain.  The k smallest (dist, id) per query in
 * ascending (dist, id) order, id = id_offset + row, ties to the smaller id, NaN ranked as +inf,
 * missing slots (+inf, 0xFFFFFFFF): the chains and the order of mivq_flat_search, so dists and
 * ids are bit-identical to mivq_flat_search(qy, (float)mivq_rankaware_dequantize(codes)).  No
 * decoded row is written anywhere; the workspace holds top-k lists (few queries) or a block of
 * keys (nq >= 16 and n >= 4096), never rows.  Rows may start at any byte, and no byte past
 * codes + n * code_size is read.
 * nq < 0, n < 0, d <= 0, code_size <= 0, k <= 0, a metric that is neither MIVQ_METRIC_L2 nor
 * MIVQ_METRIC_INNER_PRODUCT, ids that overflow 32 bits, or a null pointer with nq, n > 0 return
 * MIVQ_ERR_INVALID before any launch; n == 0 fills dists / ids with the missing-slot values;
 * k > 256, code_size above 48000 bytes, and (few queries only) d above 16384 are
 * MIVQ_ERR_UNSUPPORTED.  Any widths are accepted: the level tables (up to 256 d floats) are
 * staged per slice of dimensions. */
size_t mivq_rankaware_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d,
                                                  int32_t code_size, int32_t k);
int mivq_rankaware_flat_search(const float* qy, int64_t nq, const uint8_t* codes, int64_t n,
                               int32_t d, const float* lv32, const int32_t* lv_off,
                               const int32_t* pos, const int32_t* width, int32_t code_size,
                               int32_t metric, int32_t k, int64_t id_offset, void* workspace,
                               size_t workspace_bytes, float* dists, uint32_t* ids, void* stream);

/* Data-fitted level tables for the rank-aware format: per dimension, 2^width[j] levels fitted to
 * that dimension's sample, by the globally optimal 1-D k-means (MIVQ_CB1D_EXACT, dynamic
 * programming with divide and conquer, O(2^w n log n)) or by k-means++ seeding and at most 50
 * Lloyd passes with empty-cell repair (MIVQ_CB1D_LLOYD).  Both are the sequential fp64 rule of
 * tests/_codebook1d_rule.py bit for bit: prefix sums added in ascending order, every product and
 * quotient rounded on its own, first minimum on ties.
 *   cols   (d, n) f32, device: row j = dimension j's values, ascending
 *   width  (d,)     int32, HOST: bits of dimension j, 0..8 (they size the launches)
 *   lv_off (d + 1,) int32, HOST: start of dimension j's levels; lv_off[j + 1] - lv_off[j] = 2^width[j]
 *   draws  (ndraws,) u64, device: the first raw outputs of the seeding's 64-bit generator
 *          (mt19937_64(0) for the reference's tables), ndraws >= 2^max width; every dimension
 *          reads them from the start.  Lloyd only; may be null for EXACT.
 *   levels (lv_off[d],) f32, device: ascending; fewer distinct levels than 2^w (a dimension with
 *          no more than 2^w distinct values gets exactly those) are padded with the last one
 *   sse    (d,) f64, device: the table's sum of squared errors on the sample (0 when padded
 *          because of too few distinct values)
 * Dimensions of width 0 are skipped: their level and sse entries are not written.  One workgroup
 * fits one dimension in one slot of the workspace, and a call keeps as many dimensions in flight
 * as the workspace has slots for, the widest dimensions first; there is no other limit.  A slot
 * is mivq_codebook1d_workspace_bytes(n, w, method, 1) bytes, w the widest of the dimensions in
 * flight (EXACT keeps (2^w - 1)(n + 1) int32 of argmins per slot), so the same bytes hold more
 * of the narrower dimensions that follow.  The result does not depend on the workspace size.
 * The first centre of a dimension takes one draw, or more where a draw is rejected (probability
 * n / 2^64 each), every further centre one; a dimension that runs out of draws reuses the last
 * one and rejects no more, so pass spare draws beyond 2^max width to keep the generator's
 * sequence.
 * A row that is not ascending or holds non-finite values gives unspecified levels but no access
 * outside the row, its slot and its levels.
 * n < 0, d < 0, an unknown method, a width outside 0..8, an lv_off that does not match the widths,
 * a null pointer or fewer than 2^max width draws return MIVQ_ERR_INVALID, a null workspace or one below
 * one slot of the widest dimension MIVQ_ERR_WORKSPACE and n above 2^26 MIVQ_ERR_UNSUPPORTED, all
 * before any launch; n == 0 or d == 0 returns MIVQ_OK without one.  The size query returns 0 for
 * arguments fit would refuse. */
#define MIVQ_CB1D_EXACT 0
#define MIVQ_CB1D_LLOYD 1
size_t mivq_codebook1d_workspace_bytes(int64_t n, int32_t max_width, int32_t method,
                                       int32_t dims_at_once);
int mivq_codebook1d_fit(const float* cols, int64_t n, int32_t d, const int32_t* width,
                        const int32_t* lv_off, int32_t method, const uint64_t* draws, int32_t ndraws,
                        void* workspace, size_t workspace_bytes, float* levels, double* sse,
                        void* stream);

/* ------------------------------------------------------ ADC search
 * Flat asymmetric-distance search over PQ codes; the GPU counterpart of
 * FlatQuantizedIndex.search_with_scores (methods/search/flat_quantized_index.py:45-76),
 * which decodes every code and ranks exact distances to the reconstructions.
 *   lut[q][m][k] = sum over t ascending of (q[m*dsub+t] - c[m][k][t])^2 (fmaf chain), or for
 *                  metric == MIVQ_METRIC_INNER_PRODUCT  -(fmaf chain of q * c)
 *   dist(q, i)   = ((lut[q][0][code_0] + lut[q][1][code_1]) + ...) + lut[q][M-1][code_M-1]
 * Results per query are the k smallest (dist, id) pairs in ascending (dist, id) order
 * (ties broken by the smaller global id = id_offset + row); missing slots (n < k) hold
 * dist = +inf, id = 0xFFFFFFFF. */
int mivq_adc_lut(const float* q, int64_t nq, int32_t d, int32_t M, int32_t nbits,
                 const float* centroids, int32_t metric, float* lut, void* stream);
size_t mivq_adc_search_workspace_bytes(int64_t nq, int64_t n, int32_t M, int32_t nbits, int32_t k);
/* codes: (n, M) one byte per sub-code (nbits <= 8; use mivq_pq_unpack for nbits < 8).
 * flags: MIVQ_ADC_AUTO (0) for every product call; the other bits are diagnostics / test
 * hooks and change no result except MIVQ_ADC_NO_RERUN (see below).  The workspace size does
 * not depend on flags. */
#define MIVQ_ADC_AUTO 0u          /* filtered search where the shape allows it, else the fp32 scan */
#define MIVQ_ADC_FORCE_EXACT 1u   /* diagnostic: the fp32 scan for every query (same results)      */
#define MIVQ_ADC_NO_RERUN 2u      /* test hook: queries the filter cannot certify are left NaN      */
#define MIVQ_ADC_SMALL_RERUN_GRID 4u /* test hook: the re-run of uncertified queries on one column of
                                        workgroups, each walking several list-slot blocks          */
int mivq_adc_search(const float* lut, int64_t nq, const uint8_t* codes, int64_t n, int32_t M,
                    int32_t nbits, int32_t k, int64_t id_offset, void* workspace,
                    size_t workspace_bytes, float* dists, uint32_t* ids, uint32_t flags, void* stream);
/* Exact brute-force top-k over an f32 database (ground truth; the decode-then-search path of
 * FlatQuantizedIndex, flat_quantized_index.py:57-76, for the quantizers without a code-domain
 * search below: f64-fitted SQ, Extended RaBitQ):
 *   L2: dist = fmaf chain over t of (q_t - x_t)^2;  IP: dist = -(fmaf chain of q_t * x_t)
 * ranked ascending by (dist, id) exactly like mivq_adc_search (callers negate IP back). */
size_t mivq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k);
int mivq_flat_search(const float* q, int64_t nq, const float* x, int64_t n, int32_t d,
                     int32_t metric, int32_t k, int64_t id_offset, void* workspace,
                     size_t workspace_bytes, float* dists, uint32_t* ids, void* stream);
/* The same exact search over SQ / RaBitQ-1 codes, without the fp32 database: the codes are
 * read once and dequantised in registers to the floats mivq_sq_decode_f32 / mivq_rabitq_decode
 * write, so dists and ids are bit-identical to decode + mivq_flat_search (same chains, same
 * (dist, id) order, NaN ranks as +inf, missing slots (+inf, 0xFFFFFFFF)).  The workspace holds
 * part lists / key blocks only, never decoded rows.
 *   SQ:     codes, lo, den, nbits as in mivq_sq_decode_f32 (16-bit codes 2-byte aligned);
 *           x^_t = (level / (2^nbits - 1)) * den_t + lo_t, one rounding per step.
 *   RaBitQ: codes (n, ceil(d/8) + 8) rows of mivq_rabitq_encode, centroid may be NULL;
 *           x^_t = +-(0.5 * mult * 2 * (1/sqrt(d))) + c_t (not the estimator of
 *           mivq_rabitq_search: the exact distance to the decoded row).
 * Rows need no alignment; 16-byte aligned rows are read with 16-byte loads. */
size_t mivq_sq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k);
int mivq_sq_flat_search(const float* q, int64_t nq, const void* codes, int64_t n, int32_t d,
                        const float* lo, const float* den, int32_t nbits, int32_t metric, int32_t k,
                        int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists,
                        uint32_t* ids, void* stream);
size_t mivq_rabitq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k);
int mivq_rabitq_flat_search(const float* q, int64_t nq, const uint8_t* codes, int64_t n, int32_t d,
                            const float* centroid, int32_t metric, int32_t k, int64_t id_offset,
                            void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids,
                            void* stream);
/* The same over LVQ codes: rows and mu as in mivq_lvq_decode, x^_t = (lo + idx_t * delta) + mu_t
 * with the row's lo and delta from its trailer; dists and ids bit-identical to mivq_lvq_decode +
 * mivq_flat_search.  8-byte aligned rows (code_size % 8 == 0, aligned base) with an even nbits
 * are read with 8-byte loads, 4-byte aligned rows with 4-byte loads, others byte-wise. */
size_t mivq_lvq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k);
int mivq_lvq_flat_search(const float* q, int64_t nq, const uint8_t* codes, int64_t n, int32_t d,
                         const float* mu, int32_t nbits, int32_t metric, int32_t k,
                         int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists,
                         uint32_t* ids, void* stream);
/* Re-ranking: the exact searches above restricted, per query, to a list of candidate rows (the
 * second stage of a two-stage search; faiss' IndexRefine).  cand is (nq, r) uint32 row-major on
 * the device: the global ids a first stage returned for each query.  The store arguments are
 * those of mivq_flat_search / mivq_sq_flat_search / mivq_lvq_flat_search: the same row formats,
 * parameters and alignment freedom.
 *   - the candidates of query a are the slots with id_offset <= cand[a][j] < id_offset + n, ids
 *     compared as unsigned; every other slot is skipped, 0xFFFFFFFF (the padding the searches
 *     write) among them;
 *   - each live slot is a candidate of its own: duplicates are not removed (a repeated id may
 *     appear twice in the output; callers pass distinct ids);
 *   - dist(a, c) is the chain of the matching flat search for row c - id_offset, with x^_t as
 *     that search dequantises it: L2 the fmaf chain over t ascending of (q_t - x^_t)^2, IP
 *     -(fmaf chain of q_t * x^_t);
 *   - out: the k smallest (dist, id) ascending, ties to the smaller id, NaN ranked and written as
 *     +inf, missing slots (+inf, 0xFFFFFFFF).
 * So dists are bit-identical to what mivq_*_flat_search reports for the same (query, row), and
 * the result is the flat search's restricted to the candidate set.  No decoded row and no
 * (nq, r, d) block is written anywhere: the workspace holds partial top-k lists only.
 * Checked before any launch.  MIVQ_ERR_INVALID: nq < 0, n < 0, r < 1, d <= 0, ids that overflow
 * 32 bits, 16-bit codes that are not 2-byte aligned, a null pointer with work to do.
 * MIVQ_ERR_UNSUPPORTED: k outside [1, 256], an unknown metric, nbits outside {4, 8, 16} (SQ) /
 * [1, 8] (LVQ), a d whose query and parameter rows (d rounded up to 4 floats each: f32 1, LVQ 2,
 * SQ 3) exceed 160 KiB of LDS.  MIVQ_ERR_WORKSPACE: a workspace below the size query's.
 * nq == 0 returns MIVQ_OK without a launch; n == 0 fills every row with the missing-slot
 * values.  Stream-ordered, no host synchronisation. */
size_t mivq_rerank_f32_workspace_bytes(int64_t nq, int64_t r, int32_t k);
int mivq_rerank_f32(const float* q, int64_t nq, const uint32_t* cand, int64_t r, const float* x,
                    int64_t n, int32_t d, int32_t metric, int32_t k, int64_t id_offset,
                    void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids,
                    void* stream);
size_t mivq_rerank_sq_workspace_bytes(int64_t nq, int64_t r, int32_t k);
int mivq_rerank_sq(const float* q, int64_t nq, const uint32_t* cand, int64_t r, const void* codes,
                   int64_t n, int32_t d, const float* lo, const float* den, int32_t nbits,
                   int32_t metric, int32_t k, int64_t id_offset, void* workspace,
                   size_t workspace_bytes, float* dists, uint32_t* ids, void* stream);
size_t mivq_rerank_lvq_workspace_bytes(int64_t nq, int64_t r, int32_t k);
int mivq_rerank_lvq(const float* q, int64_t nq, const uint32_t* cand, int64_t r,
                    const uint8_t* codes, int64_t n, int32_t d, const float* mu, int32_t nbits,
                    int32_t metric, int32_t k, int64_t id_offset, void* workspace,
                    size_t workspace_bytes, float* dists, uint32_t* ids, void* stream);
/* The same over two-level LVQ rows (mivq_lvq2_encode): the contract of mivq_rerank_lvq word for
 * word, with x^_t the two-level reconstruction of mivq_lvq2_decode, so dists are bit-identical to
 * mivq_lvq2_decode + mivq_flat_search for the same (query, row).  A unit of 32 dimensions is
 * nbits1 words of codes1 and nbits2 words of codes2; each array is read with 8-byte (codes1, even
 * nbits1) / 16-byte (codes2) loads, 4-byte loads or bytes, as its own base and row stride allow.
 * nbits1 outside [1, 8] is MIVQ_ERR_INVALID, nbits2 outside {4, 8} MIVQ_ERR_UNSUPPORTED; the
 * workspace is that of mivq_rerank_lvq. */
size_t mivq_rerank_lvq2_workspace_bytes(int64_t nq, int64_t r, int32_t k);
int mivq_rerank_lvq2(const float* q, int64_t nq, const uint32_t* cand, int64_t r,
                     const uint8_t* codes1, const uint8_t* codes2, int64_t n, int32_t d,
                     const float* mu, int32_t nbits1, int32_t nbits2, int32_t metric, int32_t k,
                     int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists,
                     uint32_t* ids, void* stream);
/* Merges `parts` sorted (nq, k) lists laid out (parts, nq, k) into one sorted (nq, k) list
 * with the same (dist, id) order (ids compared as uint32, NaN dists ranked and written as +inf)
 * — the on-device merge after the RCCL all-gather.  parts == 0 writes (+inf, 0xFFFFFFFF)
 * everywhere; k in [1, 256]. */
int mivq_topk_merge(const float* dists_in, const uint32_t* ids_in, int32_t parts, int64_t nq,
                    int32_t k, float* dists_out, uint32_t* ids_out, void* stream);

/* ------------------------------------------------------ IVF: coarse quantizer, lists, IVF-PQ
 * GPU counterpart of FaissIvfPqIndex (methods/search/faiss_ivfpq_index.py:46-76: faiss
 * IndexIVFPQ over an IndexFlatL2 / IndexFlatIP coarse quantizer, residual PQ) and of the
 * IVF build in benchmarks/ivf_benchmark.py:170-204.
 *
 * Exact pairwise distances, out (n, m) row-major (the coarse quantizer's exhaustive search
 * and the k-means assignment); the chains of mivq_flat_search:
 *   L2: out[i][j] = fmaf chain over t ascending of (x_i[t] - y_j[t])^2
 *   IP: out[i][j] = -(fmaf chain of x_i[t] * y_j[t]) */
int mivq_pairwise_distances(const float* x, int64_t n, const float* y, int64_t m, int32_t d,
                            int32_t metric, float* out, void* stream);
/* Per row of an (n, m) matrix, the k smallest (value, column) pairs ascending (NaN ranks as
 * +inf, ties to the smaller column); missing slots (m < k) hold (+inf, 0xFFFFFFFF). */
int mivq_topk_rows(const float* dist, int64_t n, int64_t m, int32_t k, float* out_d,
                   uint32_t* out_i, void* stream);
/* Stable bucket sort of assignments (n,) in [0, K), K <= 16384: offsets (K + 1) int64, the
 * rows of bucket l are order[offsets[l] .. offsets[l+1]) in ascending row order. */
size_t mivq_bucket_sort_workspace_bytes(int64_t n, int32_t K);
int mivq_bucket_sort(const uint32_t* assign, int64_t n, int32_t K, int64_t* offsets,
                     uint32_t* order, void* workspace, size_t workspace_bytes, void* stream);
/* k-means update from a bucket sort: centroids[l][t] = (f32 sum over the bucket's rows in
 * ascending row order of x[row][t]) / count for non-empty buckets (empty buckets keep their
 * value); counts (K,) int32. */
int mivq_centroid_update(const float* x, int64_t n, int32_t d, int32_t K, const int64_t* offsets,
                         const uint32_t* order, float* centroids, int32_t* counts, void* stream);
/* r[i][t] = x[i][t] - coarse[assign[i]][t] */
int mivq_ivf_residuals(const float* x, int64_t n, int32_t d, const float* coarse,
                       const uint32_t* assign, float* r, void* stream);
/* dst row i = src row order[i]; row_bytes a multiple of 4 */
int mivq_gather_rows(const void* src, int64_t row_bytes, const uint32_t* order, int64_t n,
                     void* dst, void* stream);
/* IVF-PQ L2 term per vector (faiss' precomputed table folded per code):
 *   tau_i = ((t_0 + t_1) + ...) + t_{M-1},  t_m = cn[m][k] + 2 * (fmaf chain over t of
 *   coarse[assign_i][m*dsub + t] * C[m][k][t]),  k = codes[i][m]
 * cn = the canonical ||C[m][k]||^2 of mivq_pq_prepare (first block of the prep buffer). */
int mivq_ivfpq_terms(const uint8_t* codes, int64_t n, int32_t d, int32_t M, int32_t nbits,
                     const float* pq_centroids, const float* cn, const float* coarse,
                     const uint32_t* assign, float* tau, void* stream);
/* IVF-PQ search over inverted lists in bucket order:
 *   lut (nq, M, ksub): mivq_adc_lut with MIVQ_METRIC_INNER_PRODUCT (= -(q . c) chains)
 *   probe_d, probe_l (nq, nprobe): coarse distances and list ids (mivq_topk_rows); list id
 *     0xFFFFFFFF slots are skipped
 *   offsets (nlist + 1), list_codes (N, M) u8, list_ids (N,), tau (N,) in bucket order
 *   S = ((lut[q][0][c_0] + lut[q][1][c_1]) + ...) + lut[q][M-1][c_{M-1}]
 *   L2: dist = (probe_d + tau) + 2 * S  (= ||q - coarse_l - r_hat||^2 expanded)
 *   IP: dist = probe_d + S              (= -(q . coarse_l + q . r_hat))
 * ranked like mivq_adc_search: ascending (dist, id) with id = the list_ids entry compared as
 * uint32, so ids >= 2^31 rank after the smaller ones.  A NaN dist ranks as +inf and keeps its
 * id; dists/ids (nq, k) are padded with (+inf, 0xFFFFFFFF) when fewer than k rows are probed
 * (skipped slots, empty lists), the pads after every real row.  The result does not depend on
 * the order of a query's probe slots.
 * Limits, checked on the host before any launch (MIVQ_ERR_UNSUPPORTED): k in [1, 256];
 * nbits in [1, 8]; M * 2^nbits * 4 <= 128 KiB (the query's table lives in LDS: M <= 128 at
 * nbits = 8); nq <= 65535 per call (the scan's grid is (probe splits, nq); a caller with more
 * queries passes ranges of them: queries are independent, so the rows are those of one call). */
size_t mivq_ivfpq_search_workspace_bytes(int64_t nq, int32_t nprobe, int32_t k);
int mivq_ivfpq_search(const float* lut, int64_t nq, int32_t M, int32_t nbits, const float* probe_d,
                      const uint32_t* probe_l, int32_t nprobe, int32_t nlist, const int64_t* offsets,
                      const uint8_t* list_codes, const uint32_t* list_ids, const float* tau,
                      int32_t metric, int32_t k, void* workspace, size_t workspace_bytes,
                      float* dists, uint32_t* ids, void* stream);

/* ------------------------------------------------------ IVF over RaBitQ-1 codes
 * Replaces faiss IVF{nlist},RaBitQ behind RaBitQIVFIndex (methods/search/rabitq_ivf_index.py).
 * mivq_ivf_rabitq_encode: row i gets the code row of mivq_rabitq_encode with centroid =
 * coarse[assign[i]] (same layout, bit-identical, factors included; against the oracle the
 * factors agree within 1e-5 relative, as for mivq_rabitq_encode).  coarse: (nlist, d);
 * assign[i] >= nlist is undefined behaviour (as for mivq_ivf_residuals). */
int mivq_ivf_rabitq_encode(const float* x, int64_t n, int32_t d, const float* coarse,
                           int32_t nlist, const uint32_t* assign, int32_t metric, uint8_t* codes,
                           void* stream);
/* Estimator search over the probed lists.  probe_l (nq, nprobe): list ids, 0xFFFFFFFF slots are
 * skipped; offsets (nlist + 1) int64, list_codes (n, code_size), list_ids (n,) in bucket order,
 * all on the device.  For every probed pair (query a, list l) and row i of the list the key is
 * oracle_rabitq_est of that code with centroid = coarse[l] (the query residual q_a - coarse[l]
 * is quantised to qb bits, 0..8, per pair); NaN keys rank as +inf.  dists/ids (nq, k): the k
 * smallest (key, list_ids[i]) over all probed lists, ascending, ties to the smaller id, padded
 * with (+inf, 0xFFFFFFFF); INNER_PRODUCT keys are the negated estimates.  k in [1, 256],
 * nlist <= 16383.  Stream-ordered, no host synchronisation; the workspace size depends on the
 * shape alone (queries are processed in chunks; at most 1 GiB) and is 0 for invalid sizes. */
size_t mivq_ivf_rabitq_search_workspace_bytes(int64_t nq, int64_t n, int32_t nlist,
                                              int32_t nprobe, int32_t d, int32_t k);
int mivq_ivf_rabitq_search(const float* q, int64_t nq, int32_t d, const float* coarse,
                           int32_t nlist, const uint32_t* probe_l, int32_t nprobe,
                           const int64_t* offsets, const uint8_t* list_codes,
                           const uint32_t* list_ids, int32_t qb, int32_t metric, int32_t k,
                           void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids,
                           void* stream);

/* ------------------------------------------------------ IVF over per-list SQ / LVQ codes
 * GPU counterpart of IvfQuantizedIndex (methods/search/ivf_quantized_index.py) for a
 * ScalarQuantizer (4 / 8 / 16 bits, f32) or an LVQQuantizer (1..8 bits) per list, fitted on the
 * list's residuals.  The parameters of all lists are (nlist, d) arrays; a row's are those of
 * its list l = assign[i], its centroid c = coarse[l].  Every operation is fp32, one rounding
 * per step:
 *   residual   r_t = x_t - c_t
 *   SQ fit     lo_l[t] = min, hi_l[t] = max over the list's rows of r_t (any order: exact),
 *              den_l[t] = (hi - lo) + 1e-8f; an empty list: lo = 0, den = 1e-8f
 *   LVQ fit    mu_l[t] = (f32 sum of r_t over the list's rows in ascending row order) /
 *              (float)count, 0 for an empty list: mivq_ivf_residuals + mivq_centroid_update on a
 *              zeroed output compute exactly this chain (no entry point of its own)
 *   SQ row     the row mivq_sq_encode_f32 writes for r with (lo_l, den_l) (same layout, odd d
 *              at 4 bits zero-padded)
 *   LVQ row    the row mivq_lvq_encode writes for r with mu = mu_l: the quantised value is
 *              (x - c) - mu_l, two roundings; the 8-byte trailer is unchanged
 *   x^_t       dec_t + c_t, dec_t the float mivq_sq_decode_f32 / mivq_lvq_decode writes for the
 *              row with its list's parameters (the decode entry points return x^)
 *   key        L2: the sequential fmaf chain over t ascending of (q_t - x^_t)^2;
 *              IP: -(fmaf chain of q_t * x^_t)                  (the chains of mivq_flat_search)
 * assign[i] >= nlist is undefined behaviour (as for mivq_ivf_residuals).  offsets / order: the
 * bucket sort of assign (mivq_bucket_sort). */
int mivq_ivf_sq_fit(const float* x, int64_t n, int32_t d, const float* coarse, int32_t nlist,
                    const int64_t* offsets, const uint32_t* order, float* lo, float* den,
                    void* stream);
int mivq_ivf_sq_encode(const float* x, int64_t n, int32_t d, const float* coarse, int32_t nlist,
                       const uint32_t* assign, const float* lo, const float* den, int32_t nbits,
                       void* codes, void* stream);
int mivq_ivf_sq_decode(const void* codes, int64_t n, int32_t d, const float* coarse,
                       int32_t nlist, const uint32_t* assign, const float* lo, const float* den,
                       int32_t nbits, float* out, void* stream);
int mivq_ivf_lvq_encode(const float* x, int64_t n, int32_t d, const float* coarse, int32_t nlist,
                        const uint32_t* assign, const float* mu, int32_t nbits, uint8_t* codes,
                        void* stream);
int mivq_ivf_lvq_decode(const uint8_t* codes, int64_t n, int32_t d, const float* coarse,
                        int32_t nlist, const uint32_t* assign, const float* mu, int32_t nbits,
                        float* out, void* stream);
/* Exact search over the probed lists.  probe_l (nq, nprobe): list ids; slots holding
 * 0xFFFFFFFF, or any id >= nlist, are skipped; a query's slots name distinct lists.  offsets
 * (nlist + 1) int64, list_codes (n, row bytes), list_ids (n,) in bucket order, lo / den / mu
 * (nlist, d), all on the device.  dists/ids (nq, k): the k smallest (key, id) over the rows of
 * the probed lists, ascending, id = the list_ids entry compared as uint32 (ids >= 2^31 rank
 * after the smaller ones on equal keys); a NaN key ranks as +inf; padded with
 * (+inf, 0xFFFFFFFF) after every real row.  The result does not depend on the order of a
 * query's probe slots, and is bit-identical to decoding each probed list (the decode entry
 * points above) and running mivq_flat_search over those rows.
 * Limits, checked on the host before any launch (MIVQ_ERR_UNSUPPORTED): k in [1, 256]; nlist <=
 * 16383; one query row plus the list's parameter rows and centroid (SQ 3, LVQ 2 rows of d
 * rounded up to 4 floats) within 160 KiB of LDS.  nbits outside {4, 8, 16} / [1, 8], bad sizes
 * and null pointers are MIVQ_ERR_INVALID.  Stream-ordered, no host synchronisation; the
 * workspace size depends on the shape alone (queries are processed in chunks; at most 1 GiB)
 * and is 0 for invalid or unsupported sizes. */
size_t mivq_ivf_sq_search_workspace_bytes(int64_t nq, int64_t n, int32_t nlist, int32_t nprobe,
                                          int32_t d, int32_t nbits, int32_t k);
int mivq_ivf_sq_search(const float* q, int64_t nq, int32_t d, const float* coarse, int32_t nlist,
                       const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets,
                       const void* list_codes, const uint32_t* list_ids, const float* lo,
                       const float* den, int32_t nbits, int32_t metric, int32_t k,
                       void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids,
                       void* stream);
size_t mivq_ivf_lvq_search_workspace_bytes(int64_t nq, int64_t n, int32_t nlist, int32_t nprobe,
                                           int32_t d, int32_t nbits, int32_t k);
int mivq_ivf_lvq_search(const float* q, int64_t nq, int32_t d, const float* coarse, int32_t nlist,
                        const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets,
                        const uint8_t* list_codes, const uint32_t* list_ids, const float* mu,
                        int32_t nbits, int32_t metric, int32_t k, void* workspace,
                        size_t workspace_bytes, float* dists, uint32_t* ids, void* stream);

/* ------------------------------------------------------ IVF with a PQ codebook per list
 * GPU counterpart of IvfQuantizedIndex (methods/search/ivf_quantized_index.py) around a
 * ProductQuantizer per list, each fitted on its own list's residuals (run_benchmarks' pq_ivf).
 * A row i belongs to list l = assign[i], whose centroid is c = coarse[l]; cb is the
 * (nlist, M, ksub, dsub) array of per-list codebooks, ksub = 2^nbits, dsub = d / M.  All
 * operations are fp32 with one rounding per step:
 *   residual      r_t = x_t - c_t                                  (mivq_ivf_residuals)
 *   fit, list l   cb[l] = train_pq(R_l, M, nbits, niter, seed) on the list's residuals R_l in
 *                 ascending row order; an empty list keeps zeros and is never read
 *   code row      mivq_pq_encode(R_l, cb[l]) of the row, stored one byte per sub-code (nbits < 8:
 *                 mivq_pq_unpack), i.e. list_codes (N, M) u8 in bucket order
 *   x^            e[m][j][t] = cb[l][m][j][t] + c[m*dsub + t]        (one add)
 *                 x^_{m*dsub+t} = e[m][code_m][t]                    (= mivq_pq_decode + c)
 *   table         T[m][j] = fmaf chain over t ascending of (q_{m*dsub+t} - e[m][j][t])^2        (L2)
 *                 T[m][j] = -(fmaf chain over t ascending of q_{m*dsub+t} * e[m][j][t])         (IP)
 *   key           ((T[0][code_0] + T[1][code_1]) + ...) + T[M-1][code_{M-1}]
 * By construction T is mivq_adc_lut(q, e, metric), and the key is mivq_adc_search's sum over the
 * list's codes.  The table is built on e = cb + c, not on the query residual q - c: the key is
 * the ADC distance to the reconstruction x^ (the reference's distance to decompress(codes) +
 * centroid, up to the fp32 reordering documented for mivq_adc_search).
 * There is no fit entry point: the fit is train_pq per list on the host side of the package.
 * mivq_ivf_listpq_decode writes x^ for rows in any order (codes (n, M) u8, assign (n,));
 * assign[i] >= nlist is undefined behaviour, a sub-code >= ksub is taken modulo ksub. */
int mivq_ivf_listpq_decode(const uint8_t* codes, int64_t n, int32_t d, int32_t M, int32_t nbits,
                           const float* codebooks, const float* coarse, int32_t nlist,
                           const uint32_t* assign, float* out, void* stream);
/* ADC search over the probed lists.  probe_l (nq, nprobe): list ids; offsets (nlist + 1) int64,
 * list_codes (n, M) u8, list_ids (n,) in bucket order, codebooks (nlist, M, ksub, dsub), coarse
 * (nlist, d), all on the device.  The result for a query is defined over the rows of its probed
 * lists: it holds the k smallest (key, id) over those rows, ascending; id is the list_ids entry
 * compared as uint32; a NaN key ranks as +inf; it is padded with (+inf, 0xFFFFFFFF) after every
 * real row; it is independent of the order of the probe slots; slots holding 0xFFFFFFFF or any
 * id >= nlist are skipped (a query's live slots name distinct lists).  This equals bit for bit
 * the composition: for every probed list, mivq_adc_lut on the shifted codebook e and
 * mivq_adc_search on that list's codes, merged by (dist, id).
 * Limits, checked on the host before any launch.  MIVQ_ERR_UNSUPPORTED: k outside [1, 256];
 * nlist > 16383; an unknown metric.  MIVQ_ERR_INVALID: d % M != 0; nbits outside [1, 8]; bad
 * sizes (d > 2^20 among them); null pointers.  Every M that divides d works, dsub = 1 included:
 * the tables are staged into LDS in chunks of subspaces, there is no M * ksub * 4 <= LDS limit.
 * nq = 0 and n = 0 return MIVQ_OK.  Stream-ordered, no host synchronisation.  The workspace
 * holds one M * ksub * 4 byte table per (query, probe slot) pair of a chunk of queries; its
 * size depends on the shape alone and is 0 for invalid sizes.  Queries go through in chunks
 * sized so that the workspace aims at 512 MiB and stays under 1 GiB; at large M * nprobe a
 * chunk holds few queries (one at the least: nprobe * M * ksub * 4 bytes are always needed). */
size_t mivq_ivf_listpq_search_workspace_bytes(int64_t nq, int64_t n, int32_t nlist, int32_t nprobe,
                                              int32_t d, int32_t M, int32_t nbits, int32_t k);
int mivq_ivf_listpq_search(const float* q, int64_t nq, int32_t d, int32_t M, int32_t nbits,
                           const float* codebooks, const float* coarse, int32_t nlist,
                           const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets,
                           const uint8_t* list_codes, const uint32_t* list_ids, int32_t metric,
                           int32_t k, void* workspace, size_t workspace_bytes, float* dists,
                           uint32_t* ids, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* MIVQ_H */
