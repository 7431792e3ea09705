// ivf_code.hip — IVF lists of SQ-4/8/16 and LVQ-1..8 codes for gfx950: per-list fit, encode and
// decode of the residuals x - coarse[list(x)], and the exact search over the probed lists.
//
// GPU counterpart of the reference's IvfQuantizedIndex (methods/search/ivf_quantized_index.py): one
// quantizer per list, fitted on the list's residuals; search decodes the probed lists, adds each
// list's centroid and ranks by the exact distance to the reconstruction.  Here the parameters
// of all lists are (nlist, d) arrays (SQ: lo, den; LVQ: mu), a row's are those of its list, and
// no list is ever decoded to memory: the key of (query, row) is the chain of mivq_flat_search
// on x^_t = dec_t + c_t formed in registers, so a search is bit-identical to decode + add +
// mivq_flat_search over the probed rows.
//
//   ivf_sq_fit_kernel     one workgroup per list: min / max of the residuals in every dimension.
//   sq_/lvq_encode_kernel, sq_/lvq_decode_kernel <PER_ROW>: the flat kernels (code_internal.h)
//                         with the parameters and the centroid of row i taken at assign[i].
//   ivf_prep_kernel       (ivf_internal.h) the driver's pair prologue, nothing else.
//   ivf_code_scan_kernel  the QB query rows and the list's parameter rows and centroid in LDS,
//                         lane = row, the row read once by scan_row (code_internal.h: the loads
//                         and chains of code_scan_kernel), WaveTopK selection inside the scan, the
//                         waves' lists merged in LDS into one list per (pair, range).
// The search runs on the probed-list driver (ivf_internal.h): pair sort, work items (QB pairs
// each), chunks of queries and the merge of the partial lists are its steps.
#include "adc_internal.h"
#include "code_internal.h"
#include "ivf_internal.h"
#include "mivq_common.h"
#include "topk.h"

#include <algorithm>

namespace mivq {
namespace {

// ---------------------------------------------------------------- fit
// lo[l][t] = min, hi = max over the rows i of list l of x[i][t] - coarse[l][t];
// den[l][t] = (hi - lo) + 1e-8f.  An empty list: lo = 0, den = 1e-8f.  One workgroup per list,
// thread = dimension (8 per pass), rows in bucket order (min and max do not depend on it).
__global__ __launch_bounds__(256) void ivf_sq_fit_kernel(const float* __restrict__ x, int d,
                                                         const float* __restrict__ coarse,
                                                         const int64_t* __restrict__ offsets,
                                                         const uint32_t* __restrict__ order, float* __restrict__ lo,
                                                         float* __restrict__ den) {
    __shared__ uint32_t rows[256];
    const int l = blockIdx.x;
    const int64_t beg = offsets[l], end = offsets[l + 1];
    constexpr int TPT = 8;  // dims per thread per pass
    for (int t0 = 0; t0 < d; t0 += 256 * TPT) {
        float mn[TPT], mx[TPT], c[TPT];
#pragma unroll
        for (int u = 0; u < TPT; ++u) {
            const int t = t0 + u * 256 + threadIdx.x;
            mn[u] = INFINITY;
            mx[u] = -INFINITY;
            c[u] = t < d ? coarse[(int64_t)l * d + t] : 0.0f;
        }
        for (int64_t r0 = beg; r0 < end; r0 += 256) {
            const int nc = (int)min<int64_t>(256, end - r0);
            __syncthreads();
            if ((int)threadIdx.x < nc) rows[threadIdx.x] = order[r0 + threadIdx.x];
            __syncthreads();
            for (int q = 0; q < nc; ++q) {
                const float* xr = x + (int64_t)rows[q] * d;
#pragma unroll
                for (int u = 0; u < TPT; ++u) {
                    const int t = t0 + u * 256 + threadIdx.x;
                    if (t < d) {
                        const float r = __fsub_rn(xr[t], c[u]);
                        mn[u] = fminf(mn[u], r);
                        mx[u] = fmaxf(mx[u], r);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < TPT; ++u) {
            const int t = t0 + u * 256 + threadIdx.x;
            if (t < d) {
                const bool any = end > beg;
                lo[(int64_t)l * d + t] = any ? mn[u] : 0.0f;
                den[(int64_t)l * d + t] = any ? __fadd_rn(__fsub_rn(mx[u], mn[u]), 1e-8f) : 1e-8f;
            }
        }
    }
}

template <bool VEC>
void launch_ivf_lvq_encode(const float* x, int64_t n, int d, const float* coarse, const uint32_t* assign,
                           const float* mu, int B, int sw, uint8_t* codes, hipStream_t st) {
    const int per_lane = (int)ceil_div((d + 7) / 8, 64);
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n, 4), (int64_t)device_cus() * 32));
    with_lvq_groups(per_lane, [&](auto G) {
        hipLaunchKernelGGL((lvq_encode_kernel<decltype(G)::value, VEC, true>), grid, dim3(256), 0, st, x, n, d, coarse,
                           assign, mu, B, sw, codes);
    });
}

// ---------------------------------------------------------------- search
constexpr int kIcWaves = 8;      // waves per scan workgroup: 512 rows per step
constexpr int kIcTile = kIcWaves * 64;

struct IcScan {
    IvfScan s;
    const float* q;       // (nqc, d) the chunk's queries
    const float* coarse;  // (nlist, d)
    const float* ga;      // (nlist, d) SQ den / LVQ mu
    const float* gb;      // (nlist, d) SQ lo
    int d, metric, wide, narrow;
};

// Grid (item bound, S), 512 threads.  Work item (list l, pairs [pb, pb + np)), row range s of the
// list (S equal ranges of whole 512-row steps).  LDS: [QB][dp] query rows, then the list's
// parameter rows (SQ: den, lo; LVQ: mu) and its centroid, dp = d rounded up to 4.  Lane = row:
// every wave keeps the WaveTopK lists of the QB pairs over its rows; afterwards the LDS is
// reused to merge the waves' lists, pair by pair, into wave 0's, which goes to part
// (probe slot) * S + s of the pair's query.
template <int FMT, int R, int QB>
__global__ __launch_bounds__(kIcWaves * 64) void ivf_code_scan_kernel(const IcScan A) {
    using F = Fmt<FMT>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (A.s.past_items()) return;
    const IvfItem it = ivf_item<QB, kIcTile>(A.s);
    if (it.empty()) return;
    const auto [l, pb0, np, rb, re] = it;
    const int d = A.d, dp = (d + 3) & ~3;
    float* qv = smem;                        // [QB][dp]
    float* pa = smem + QB * dp;              // SQ den / LVQ mu
    float* pb = pa + dp;                     // SQ lo
    float* pc = pa + F::kParams * dp;        // the list's centroid
    int64_t op[QB];  // the block's pairs (uniform); slots past np repeat pair 0 (in range), never stored
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) op[qq] = A.s.porder[pb0 + (qq < np ? qq : 0)];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        const float* qr = A.q + (op[qq] / A.s.nprobe) * d;
        for (int t = tid; t < d; t += kIcWaves * 64) qv[qq * dp + t] = qr[t];
    }
    for (int t = tid; t < d; t += kIcWaves * 64) {
        pa[t] = A.ga[(int64_t)l * d + t];
        if (F::kParams == 2) pb[t] = A.gb[(int64_t)l * d + t];
        pc[t] = A.coarse[(int64_t)l * d + t];
    }
    __syncthreads();
    WaveTopK<R> top[QB];
    float thr_d[QB];
    uint32_t thr_i[QB];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        top[qq].init();
        thr_d[qq] = INFINITY;
        thr_i[qq] = kNoId;
    }
    const bool l2 = A.metric == MIVQ_METRIC_L2;
    const int k = A.s.k;
    const int64_t stride = F::row_bytes(d);
    const ScanRows rows{qv, pa, pb, pc, dp};
    for (int64_t base = rb + (int64_t)wv * 64; base < re; base += kIcTile) {
        const int64_t row = base + lane;
        const bool valid = row < re;
        float dist[QB];
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) dist[qq] = 0.0f;
        uint32_t gid = kNoId;
        if (valid) {
            gid = A.s.ids[row];
            scan_row<FMT, QB, true>(A.s.codes + row * stride, d, rows, A.wide, A.narrow, l2, dist);
        }
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            if (qq >= np) break;
            float dv = l2 ? dist[qq] : -dist[qq];
            if (dv != dv) dv = INFINITY;
            top[qq].offer(valid, dv, gid, k, lane, thr_d[qq], thr_i[qq]);
        }
    }
    // the waves' lists -> one list per pair: waves 1.. write theirs to LDS (the rows are no longer
    // read), wave 0 takes them in, 64 candidates per offer
    __syncthreads();
    float* md = smem;
    uint32_t* mi = reinterpret_cast<uint32_t*>(smem + (kIcWaves - 1) * k);
    const int total = (kIcWaves - 1) * k;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        if (qq >= np) break;  // block-uniform
        if (wv > 0) top[qq].store(md + (wv - 1) * k, mi + (wv - 1) * k, k, lane);
        __syncthreads();
        if (wv == 0) {
            for (int e0 = 0; e0 < total; e0 += 64) {
                const int e = e0 + lane;
                const bool valid = e < total;
                top[qq].offer(valid, valid ? md[e] : INFINITY, valid ? mi[e] : kNoId, k, lane, thr_d[qq], thr_i[qq]);
            }
            const int64_t obase = A.s.part_base(op[qq], blockIdx.y);
            top[qq].store(A.s.pd + obase, A.s.pi + obase, k, lane);
        }
        __syncthreads();  // the buffer is rewritten for the next pair
    }
}

// The rows a scan workgroup keeps in LDS next to its queries: the format's parameter rows and
// the list's centroid; the budget is the one of the flat code scan (128 KiB, 160 at one query).
ScanPolicy ic_policy(bool lvq) { return ScanPolicy{(lvq ? 1 : 2) + 1, 128, true}; }

// Pairs per work item: the scan's query block, no wider than the pairs a list can expect (a
// workgroup computes all QB chains of a row); 0: d does not fit the LDS.
int ic_pairs_per_item(int64_t nq, int nlist, int nprobe, int d, bool lvq) {
    return ivf_pairs_per_item(scan_qb(d, ic_policy(lvq)), nq, nlist, nprobe);
}

// 0: d does not fit the LDS.
size_t ic_workspace_bytes(int64_t nq, int nlist, int nprobe, int d, int k, bool lvq) {
    const int QB = ic_pairs_per_item(nq, nlist, nprobe, d, lvq);
    return QB == 0 ? 0 : ivf_layout(nq, nlist, nprobe, k, QB, 0, 0, 16).total;
}

bool sq_bits_ok(int nbits) { return nbits == 4 || nbits == 8 || nbits == 16; }
bool lvq_bits_ok(int nbits) { return nbits >= 1 && nbits <= 8; }

template <int FMT, int R, int QB>
hipError_t launch_ic_scan(const IcScan& A, int64_t maxitems, hipStream_t st) {
    using F = Fmt<FMT>;
    const size_t rows = (size_t)(QB + F::kParams + 1) * ((A.d + 3) & ~3) * sizeof(float);
    const size_t smem = std::max(rows, (size_t)(kIcWaves - 1) * A.s.k * 8);
    auto kern = ivf_code_scan_kernel<FMT, R, QB>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)maxitems, (unsigned)A.s.S), dim3(kIcWaves * 64), smem, st, A);
    return hipGetLastError();
}

// The search of both kinds; ga / gb: SQ (den, lo), LVQ (mu, null).  Arguments are validated.
template <int FMT>
int ivf_code_search(const char* name, const float* q, int64_t nq, int d, const float* coarse, int nlist,
                    const uint32_t* probe_l, int nprobe, const int64_t* offsets, const uint8_t* list_codes,
                    const uint32_t* list_ids, const float* ga, const float* gb, int metric, int k, void* workspace,
                    size_t workspace_bytes, float* dists, uint32_t* ids, void* stream) {
    using F = Fmt<FMT>;
    hipStream_t st = as_stream(stream);
    const LoadModes lm = code_load_modes<FMT>(list_codes, d);
    return with_query_block(ic_pairs_per_item(nq, nlist, nprobe, d, F::kIsLvq), [&](auto QB) {
        constexpr int kQB = decltype(QB)::value;
        const IvfLayout L = ivf_layout(nq, nlist, nprobe, k, kQB, 0, 0, 16);
        return ivf_probed_search<kQB>(
            name, L, nq, nlist, nprobe, k, offsets, list_codes, list_ids, workspace, workspace_bytes, dists, ids, stream,
            [&](const IvfChunk& c) {
                hipLaunchKernelGGL(ivf_prep_kernel<64>, dim3((unsigned)c.pairs), dim3(64), 0, st,
                                   probe_l + c.a0 * nprobe, nlist, nprobe, c.nqc, L.S, k, c.keys, c.scan.pd, c.scan.pi);
                return hipGetLastError();
            },
            [&](const IvfChunk& c, int64_t maxitems) {
                const IcScan A{c.scan, q + c.a0 * d, coarse, ga, gb, d, metric, lm.wide, lm.narrow};
                return with_topk_regs(
                    k, [&](auto R) { return launch_ic_scan<FMT, decltype(R)::value, kQB>(A, maxitems, st); });
            });
    });
}

// The checks both searches share, before any launch.
int ic_search_prologue(const char* name, int64_t nq, int d, int nlist, int nprobe, bool bits_ok, int nbits, bool lvq,
                       int metric, int k) {
    const int rc = ivf_search_check(name, nq, d, 1 << 27, nlist, nprobe, k, metric);
    if (rc != MIVQ_OK) return rc;
    MIVQ_REQUIRE(bits_ok, MIVQ_ERR_INVALID, lvq ? "num_bits must be in [1, 8], got %d" : "num_bits must be 4, 8, or 16, got %d",
                 nbits);
    MIVQ_REQUIRE(scan_qb(d, ic_policy(lvq)) > 0, MIVQ_ERR_UNSUPPORTED, "%s: d=%d too large for LDS", name, d);
    return MIVQ_OK;
}

int ic_codec_check(const char* name, int64_t n, int d, int nlist) {
    MIVQ_REQUIRE(n >= 0 && d > 0 && d <= (1 << 27) && nlist > 0, MIVQ_ERR_INVALID, "%s: bad sizes n=%lld d=%d nlist=%d",
                 name, (long long)n, d, nlist);
    return MIVQ_OK;
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_ivf_sq_fit(const float* x, int64_t n, int32_t d, const float* coarse, int32_t nlist,
                               const int64_t* offsets, const uint32_t* order, float* lo, float* den, void* stream) {
    const int rc = ic_codec_check("ivf_sq_fit", n, d, nlist);
    if (rc != MIVQ_OK) return rc;
    MIVQ_REQUIRE(coarse && offsets && lo && den && (n == 0 || (x && order)), MIVQ_ERR_INVALID, "ivf_sq_fit: null pointer");
    hipLaunchKernelGGL(ivf_sq_fit_kernel, dim3((unsigned)nlist), dim3(256), 0, as_stream(stream), x, d, coarse, offsets,
                       order, lo, den);
    return check_launch("ivf_sq_fit");
}

extern "C" int mivq_ivf_sq_encode(const float* x, int64_t n, int32_t d, const float* coarse, int32_t nlist,
                                  const uint32_t* assign, const float* lo, const float* den, int32_t nbits, void* codes,
                                  void* stream) {
    const int rc = ic_codec_check("ivf_sq_encode", n, d, nlist);
    if (rc != MIVQ_OK) return rc;
    MIVQ_REQUIRE(sq_bits_ok(nbits), MIVQ_ERR_INVALID, "num_bits must be 4, 8, or 16, got %d", nbits);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(x && coarse && assign && lo && den && codes, MIVQ_ERR_INVALID, "ivf_sq_encode: null pointer");
    if (const int ra = sq16_aligned("ivf_sq_encode", nbits, codes)) return ra;
    const int64_t work = n * ((d + 7) / 8);
    hipLaunchKernelGGL((sq_encode_kernel<float, true>), dim3((unsigned)ceil_div(work, 256)), dim3(256), 0,
                       as_stream(stream), x, n, d, coarse, assign, lo, den, nbits, codes);
    return check_launch("ivf_sq_encode");
}

extern "C" int mivq_ivf_sq_decode(const void* codes, int64_t n, int32_t d, const float* coarse, int32_t nlist,
                                  const uint32_t* assign, const float* lo, const float* den, int32_t nbits, float* out,
                                  void* stream) {
    const int rc = ic_codec_check("ivf_sq_decode", n, d, nlist);
    if (rc != MIVQ_OK) return rc;
    MIVQ_REQUIRE(sq_bits_ok(nbits), MIVQ_ERR_INVALID, "num_bits must be 4, 8, or 16, got %d", nbits);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(codes && coarse && assign && lo && den && out, MIVQ_ERR_INVALID, "ivf_sq_decode: null pointer");
    if (const int ra = sq16_aligned("ivf_sq_decode", nbits, codes)) return ra;
    hipLaunchKernelGGL((sq_decode_kernel<float, true>), dim3((unsigned)ceil_div(n * (int64_t)d, 256)), dim3(256), 0,
                       as_stream(stream), codes, n, d, coarse, assign, lo, den, nbits, out);
    return check_launch("ivf_sq_decode");
}

extern "C" int mivq_ivf_lvq_encode(const float* x, int64_t n, int32_t d, const float* coarse, int32_t nlist,
                                   const uint32_t* assign, const float* mu, int32_t nbits, uint8_t* codes,
                                   void* stream) {
    const int rc = ic_codec_check("ivf_lvq_encode", n, d, nlist);
    if (rc != MIVQ_OK) return rc;
    MIVQ_REQUIRE(lvq_bits_ok(nbits), MIVQ_ERR_INVALID, "num_bits must be in [1, 8], got %d", nbits);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(x && coarse && assign && mu && codes, MIVQ_ERR_INVALID, "ivf_lvq_encode: null pointer");
    const int sw = lvq_store_width(codes, ((int64_t)d * nbits + 7) / 8 + 8, nbits);
    if (d % 4 == 0 && aligned16(x) && aligned16(mu) && aligned16(coarse))
        launch_ivf_lvq_encode<true>(x, n, d, coarse, assign, mu, nbits, sw, codes, as_stream(stream));
    else
        launch_ivf_lvq_encode<false>(x, n, d, coarse, assign, mu, nbits, sw, codes, as_stream(stream));
    return check_launch("ivf_lvq_encode");
}

extern "C" int mivq_ivf_lvq_decode(const uint8_t* codes, int64_t n, int32_t d, const float* coarse, int32_t nlist,
                                   const uint32_t* assign, const float* mu, int32_t nbits, float* out, void* stream) {
    const int rc = ic_codec_check("ivf_lvq_decode", n, d, nlist);
    if (rc != MIVQ_OK) return rc;
    MIVQ_REQUIRE(lvq_bits_ok(nbits), MIVQ_ERR_INVALID, "num_bits must be in [1, 8], got %d", nbits);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(codes && coarse && assign && mu && out, MIVQ_ERR_INVALID, "ivf_lvq_decode: null pointer");
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n * (int64_t)((d + 7) / 8), 256), 1 << 24));
    if (d % 4 == 0 && aligned16(mu) && aligned16(coarse) && aligned16(out))
        hipLaunchKernelGGL((lvq_decode_kernel<true, true>), grid, dim3(256), 0, as_stream(stream), codes, n, d, coarse,
                           assign, mu, nbits, out);
    else
        hipLaunchKernelGGL((lvq_decode_kernel<false, true>), grid, dim3(256), 0, as_stream(stream), codes, n, d, coarse,
                           assign, mu, nbits, out);
    return check_launch("ivf_lvq_decode");
}

extern "C" size_t mivq_ivf_sq_search_workspace_bytes(int64_t nq, int64_t n, int32_t nlist, int32_t nprobe, int32_t d,
                                                     int32_t nbits, int32_t k) {
    if (!ivf_shape_ok(nq, n, nlist, nprobe, d, k) || d > (1 << 27) || !sq_bits_ok(nbits)) return 0;
    return ic_workspace_bytes(nq, nlist, nprobe, d, k, false);
}

extern "C" size_t mivq_ivf_lvq_search_workspace_bytes(int64_t nq, int64_t n, int32_t nlist, int32_t nprobe, int32_t d,
                                                      int32_t nbits, int32_t k) {
    if (!ivf_shape_ok(nq, n, nlist, nprobe, d, k) || d > (1 << 27) || !lvq_bits_ok(nbits)) return 0;
    return ic_workspace_bytes(nq, nlist, nprobe, d, k, true);
}

extern "C" int mivq_ivf_sq_search(const float* q, int64_t nq, int32_t d, const float* coarse, int32_t nlist,
                                  const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets, const void* list_codes,
                                  const uint32_t* list_ids, const float* lo, const float* den, int32_t nbits,
                                  int32_t metric, int32_t k, void* workspace, size_t workspace_bytes, float* dists,
                                  uint32_t* ids, void* stream) {
    const int rc = ic_search_prologue("ivf_sq_search", nq, d, nlist, nprobe, sq_bits_ok(nbits), nbits, false, metric, k);
    if (rc != MIVQ_OK || nq == 0) return rc;
    MIVQ_REQUIRE(q && coarse && probe_l && offsets && list_codes && list_ids && lo && den && dists && ids,
                 MIVQ_ERR_INVALID, "ivf_sq_search: null pointer");
    if (const int ra = sq16_aligned("ivf_sq_search", nbits, list_codes)) return ra;
    return with_sq_bits(nbits, [&](auto F) {
        return ivf_code_search<decltype(F)::value>("ivf_sq_search", q, nq, d, coarse, nlist, probe_l, nprobe, offsets,
                                                   static_cast<const uint8_t*>(list_codes), list_ids, den, lo, metric, k,
                                                   workspace, workspace_bytes, dists, ids, stream);
    });
}

extern "C" int mivq_ivf_lvq_search(const float* q, int64_t nq, int32_t d, const float* coarse, int32_t nlist,
                                   const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets,
                                   const uint8_t* list_codes, const uint32_t* list_ids, const float* mu, int32_t nbits,
                                   int32_t metric, int32_t k, void* workspace, size_t workspace_bytes, float* dists,
                                   uint32_t* ids, void* stream) {
    const int rc = ic_search_prologue("ivf_lvq_search", nq, d, nlist, nprobe, lvq_bits_ok(nbits), nbits, true, metric, k);
    if (rc != MIVQ_OK || nq == 0) return rc;
    MIVQ_REQUIRE(q && coarse && probe_l && offsets && list_codes && list_ids && mu && dists && ids,
                 MIVQ_ERR_INVALID, "ivf_lvq_search: null pointer");
    return with_lvq_bits(nbits, [&](auto F) {
        return ivf_code_search<decltype(F)::value>("ivf_lvq_search", q, nq, d, coarse, nlist, probe_l, nprobe, offsets,
                                                   list_codes, list_ids, mu, nullptr, metric, k, workspace, workspace_bytes,
                                                   dists, ids, stream);
    });
}
