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
//   ivf_code_prep_kernel  per (query, probe slot) pair: its sort key (its list; skipped slots go
//                         to a bucket of their own) and the sentinel fill of its partial lists.
//   mivq_bucket_sort      stable sort of the pairs by list: the pairs probing a list are contiguous.
//   ivf_items_kernel      per-list pair counts -> work items (list, block of QB pairs).
//   ivf_code_scan_kernel  grid (item bound, S row ranges of the list): the QB query rows and the
//                         list's parameter rows and centroid in LDS, lane = row, the row read
//                         once by scan_row (code_internal.h: the loads and chains of
//                         code_scan_kernel), WaveTopK selection inside the scan, the waves' lists
//                         merged in LDS into one list per (pair, range).
//   topk_merge_kernel     merges the nprobe x S partial lists of every query.
// List sizes live on the device: the grids are sized from the shape, the kernels find their work
// from offsets and the item table.  Queries are processed in chunks so the workspace stays bounded.
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

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

template <bool VEC>
void launch_ivf_lvq_encode(const float* x, int64_t n, int d, const float* coarse, const uint32_t* assign,
                           const float* mu, int B, int sw, uint8_t* codes, hipStream_t st) {
    const int per_lane = (int)ceil_div((d + 7) / 8, 64);
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n, 4), (int64_t)device_cus() * 32));
#define MIVQ_IVF_LVQ_ENC(G) \
    hipLaunchKernelGGL((lvq_encode_kernel<G, VEC, true>), grid, dim3(256), 0, st, x, n, d, coarse, assign, mu, B, sw, codes)
    if (per_lane <= 1) MIVQ_IVF_LVQ_ENC(1);
    else if (per_lane == 2) MIVQ_IVF_LVQ_ENC(2);
    else if (per_lane == 3) MIVQ_IVF_LVQ_ENC(3);
    else if (per_lane == 4) MIVQ_IVF_LVQ_ENC(4);
    else if (per_lane <= kLvqMaxRegGroups) MIVQ_IVF_LVQ_ENC(kLvqMaxRegGroups);
    else MIVQ_IVF_LVQ_ENC(0);
#undef MIVQ_IVF_LVQ_ENC
}

// ---------------------------------------------------------------- search
constexpr int kIcWaves = 8;      // waves per scan workgroup: 512 rows per step
constexpr int kIcMaxSplit = 8;   // row ranges per list at most
constexpr int kIcTile = kIcWaves * 64;

// One workgroup per pair p = a * nprobe + j of the chunk.  keys[p]: the pair's list, nlist for a
// skipped slot (0xFFFFFFFF, or any id >= nlist).  The pair's S partial lists, part j * S + s of
// the (parts, nqc, k) layout, are set to the sentinel: the scan writes only the (pair, range)
// lists that hold rows.
__global__ __launch_bounds__(64) void ivf_code_prep_kernel(const uint32_t* __restrict__ probe_l, int nlist, int nprobe,
                                                           int64_t nqc, int S, int k, uint32_t* __restrict__ keys,
                                                           float* __restrict__ pd, uint32_t* __restrict__ pi) {
    const int64_t p = blockIdx.x;
    const int64_t a = p / nprobe;
    const int j = (int)(p - a * nprobe);
    const uint32_t l = probe_l[p];
    if (threadIdx.x == 0) keys[p] = l < (uint32_t)nlist ? l : (uint32_t)nlist;
    for (int s = 0; s < S; ++s) {
        const int64_t base = (((int64_t)j * S + s) * nqc + a) * k;
        for (int e = threadIdx.x; e < k; e += 64) {
            pd[base + e] = INFINITY;
            pi[base + e] = kNoId;
        }
    }
}

struct IcScan {
    const float* q;          // (nqc, d) the chunk's queries
    const float* coarse;     // (nlist, d)
    const float* ga;         // (nlist, d) SQ den / LVQ mu
    const float* gb;         // (nlist, d) SQ lo
    const int64_t* poff;     // sorted-pair offsets per list
    const uint32_t* porder;  // sorted position -> pair
    const uint2* items;
    const uint32_t* nitems;
    const int64_t* offsets;  // (nlist + 1) list offsets
    const uint8_t* codes;    // (n, row bytes) bucket order
    const uint32_t* ids;     // (n,)
    float* pd;               // (nprobe * S, nqc, k) partial lists
    uint32_t* pi;
    int64_t nqc;
    int d, nprobe, metric, k, S, wide, narrow;
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
    if (blockIdx.x >= *A.nitems) return;
    const uint2 item = A.items[blockIdx.x];
    const uint32_t l = item.x;
    const int64_t pb0 = item.y;
    const int np = (int)min<int64_t>(QB, A.poff[l + 1] - pb0);
    const int64_t beg = A.offsets[l], end = A.offsets[l + 1];
    const int s = blockIdx.y;
    const int64_t per = ((end - beg + A.S - 1) / A.S + kIcTile - 1) / kIcTile * kIcTile;
    const int64_t rb = beg + s * per, re = min<int64_t>(end, rb + per);
    if (np <= 0 || rb >= re) return;  // the range holds no rows: the sentinel lists stand
    const int d = A.d, dp = (d + 3) & ~3;
    float* qv = smem;                        // [QB][dp]
    float* pa = smem + QB * dp;              // SQ den / LVQ mu
    float* pb = pa + dp;                     // SQ lo
    float* pc = pa + F::kParams * dp;        // the list's centroid
    int64_t op[QB];  // the block's pairs (uniform); slots past np repeat pair 0 (in range), never stored
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) op[qq] = A.porder[pb0 + (qq < np ? qq : 0)];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        const float* qr = A.q + (op[qq] / A.nprobe) * d;
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
    const int k = A.k;
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
            gid = A.ids[row];
            scan_row<FMT, QB, true>(A.codes + row * stride, d, rows, A.wide, A.narrow, l2, dist);
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
            const int64_t a = op[qq] / A.nprobe;
            const int64_t j = op[qq] - a * A.nprobe;
            const int64_t obase = ((j * A.S + s) * A.nqc + a) * k;
            top[qq].store(A.pd + obase, A.pi + obase, k, lane);
        }
        __syncthreads();  // the buffer is rewritten for the next pair
    }
}

// The rows a scan workgroup keeps in LDS next to its queries: the format's parameter rows and
// the list's centroid; the budget is the one of the flat code scan (128 KiB, 160 at one query).
ScanPolicy ic_policy(bool lvq) { return ScanPolicy{(lvq ? 1 : 2) + 1, 128, true}; }

// Workspace of one search, sized on shape alone.  Queries are processed nqc at a time.
struct IcLayout {
    int64_t nqc;  // queries per chunk
    int S;        // row ranges per list
    int QB;       // pairs per work item; 0: d does not fit the LDS
    size_t keys, porder, poff, items, nitems, sortws, pd, pi, total;
};

constexpr size_t kIcBudget = (size_t)1 << 29;  // aim of the chunking: 512 MiB
constexpr size_t kIcCap = (size_t)1 << 30;     // never above 1 GiB

IcLayout ic_layout(int64_t nq, int nlist, int nprobe, int d, int k, bool lvq) {
    nq = std::max<int64_t>(nq, 1);
    IcLayout L{};
    L.QB = scan_qb(d, ic_policy(lvq));
    if (L.QB == 0) return L;
    // no wider than the pairs a list can expect: a workgroup computes all QB chains of a row
    const int64_t per_list = ceil_div(nq * nprobe, nlist);
    while (L.QB > 1 && L.QB / 2 >= per_list) L.QB /= 2;
    const int QB = L.QB;
    // few pairs: split the lists into row ranges so that the chip still has workgroups to run
    const int64_t blocks = ceil_div(nq * nprobe, QB);
    const int S = (int)std::max<int64_t>(1, std::min<int64_t>(kIcMaxSplit, ceil_div(2048, blocks)));
    auto build = [&](int64_t nqc) {
        IcLayout B{};
        B.nqc = nqc;
        B.S = S;
        B.QB = QB;
        const size_t P = (size_t)nqc * nprobe;
        size_t off = 0;
        B.keys = off;   off = align_up(off + P * 4, 256);
        B.porder = off; off = align_up(off + P * 4, 256);
        B.poff = off;   off = align_up(off + ((size_t)nlist + 2) * 8, 256);
        B.items = off;  off = align_up(off + ((size_t)ceil_div(P, QB) + nlist) * 8, 256);
        B.nitems = off; off += 256;
        B.sortws = off; off = align_up(off + mivq_bucket_sort_workspace_bytes((int64_t)P, nlist + 1), 256);
        B.pd = off;     off = align_up(off + P * S * k * 4, 256);
        B.pi = off;     off = align_up(off + P * S * k * 4, 256);
        B.total = off;
        return B;
    };
    const size_t per_query = (size_t)nprobe * (16 + (size_t)S * k * 8);
    int64_t nqc = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(kIcBudget / per_query)));
    L = build(nqc);
    while (L.total > kIcCap && nqc > 1) {
        nqc = (nqc + 1) / 2;
        L = build(nqc);
    }
    return L;
}

bool ic_sizes_ok(int64_t nq, int64_t n, int32_t nlist, int32_t nprobe, int32_t d) {
    return nq >= 0 && n >= 0 && nlist > 0 && nprobe > 0 && d > 0 && d <= (1 << 27);
}
bool sq_bits_ok(int nbits) { return nbits == 4 || nbits == 8 || nbits == 16; }
bool lvq_bits_ok(int nbits) { return nbits >= 1 && nbits <= 8; }

template <int FMT, int R, int QB>
hipError_t launch_ic_scan(const IcScan& A, int64_t maxitems, hipStream_t st) {
    using F = Fmt<FMT>;
    const size_t rows = (size_t)(QB + F::kParams + 1) * ((A.d + 3) & ~3) * sizeof(float);
    const size_t smem = std::max(rows, (size_t)(kIcWaves - 1) * A.k * 8);
    auto kern = ivf_code_scan_kernel<FMT, R, QB>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)maxitems, (unsigned)A.S), dim3(kIcWaves * 64), smem, st, A);
    return hipGetLastError();
}

template <int QB>
hipError_t launch_ic_items(const int64_t* poff, int nlist, uint2* items, uint32_t* nitems, hipStream_t st) {
    hipLaunchKernelGGL(ivf_items_kernel<QB>, dim3(1), dim3(1024), 0, st, poff, nlist, items, nitems);
    return hipGetLastError();
}

// The search of both kinds; ga / gb: SQ (den, lo), LVQ (mu, null).  Arguments are validated.
template <int FMT>
int ivf_code_search(const char* name, const float* q, int64_t nq, int d, const float* coarse, int nlist,
                    const uint32_t* probe_l, int nprobe, const int64_t* offsets, const uint8_t* list_codes,
                    const uint32_t* list_ids, const float* ga, const float* gb, int metric, int k, void* workspace,
                    size_t workspace_bytes, float* dists, uint32_t* ids, void* stream) {
    using F = Fmt<FMT>;
    const IcLayout L = ic_layout(nq, nlist, nprobe, d, k, F::kIsLvq);
    MIVQ_REQUIRE(workspace_bytes >= L.total, MIVQ_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", name, workspace_bytes,
                 L.total);
    hipStream_t st = as_stream(stream);
    unsigned char* p = static_cast<unsigned char*>(workspace);
    uint32_t* keys = reinterpret_cast<uint32_t*>(p + L.keys);
    uint32_t* porder = reinterpret_cast<uint32_t*>(p + L.porder);
    int64_t* poff = reinterpret_cast<int64_t*>(p + L.poff);
    uint2* items = reinterpret_cast<uint2*>(p + L.items);
    uint32_t* nitems = reinterpret_cast<uint32_t*>(p + L.nitems);
    float* pd = reinterpret_cast<float*>(p + L.pd);
    uint32_t* pi = reinterpret_cast<uint32_t*>(p + L.pi);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(list_codes);
    const int rbytes = F::row_bytes(d);
    const int wb = F::kWideWords * 4;
    const int wide = addr % wb == 0 && rbytes % wb == 0;
    const int narrow = addr % 4 == 0 && rbytes % 4 == 0;
    for (int64_t a0 = 0; a0 < nq; a0 += L.nqc) {
        const int64_t nqc = std::min<int64_t>(L.nqc, nq - a0);
        const int64_t P = nqc * nprobe;
        hipLaunchKernelGGL(ivf_code_prep_kernel, dim3((unsigned)P), dim3(64), 0, st, probe_l + a0 * nprobe, nlist, nprobe,
                           nqc, L.S, k, keys, pd, pi);
        int rc = check_launch(name);
        if (rc) return rc;
        rc = mivq_bucket_sort(keys, P, nlist + 1, poff, porder, p + L.sortws, L.pd - L.sortws, stream);
        if (rc) return rc;
        hipError_t e = with_query_block(L.QB, [&](auto QB) {
            return launch_ic_items<decltype(QB)::value>(poff, nlist, items, nitems, st);
        });
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (items): %s", name, hipGetErrorString(e));
        const IcScan A{q + a0 * d, coarse, ga, gb, poff, porder, items, nitems, offsets, list_codes, list_ids,
                       pd, pi, nqc, d, nprobe, metric, k, L.S, wide, narrow};
        e = with_topk_regs(k, [&](auto R) {
            return with_query_block(L.QB, [&](auto QB) {
                return launch_ic_scan<FMT, decltype(R)::value, decltype(QB)::value>(A, ceil_div(P, L.QB) + nlist, st);
            });
        });
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (scan): %s", name, hipGetErrorString(e));
        e = launch_topk_merge(pd, pi, nprobe * L.S, nqc, k, dists + a0 * k, ids + a0 * k, st);
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (merge): %s", name, hipGetErrorString(e));
    }
    return MIVQ_OK;
}

// The checks both searches share, before any launch; *done: nothing to do (nq == 0).
int ic_search_prologue(const char* name, int64_t nq, int d, int nlist, int nprobe, bool bits_ok, int nbits, bool lvq,
                       int metric, int k, bool* done) {
    *done = false;
    MIVQ_REQUIRE(ic_sizes_ok(nq, 0, nlist, nprobe, d), MIVQ_ERR_INVALID, "%s: bad sizes nq=%lld d=%d nlist=%d nprobe=%d",
                 name, (long long)nq, d, nlist, nprobe);
    MIVQ_REQUIRE(bits_ok, MIVQ_ERR_INVALID, lvq ? "num_bits must be in [1, 8], got %d" : "num_bits must be 4, 8, or 16, got %d",
                 nbits);
    MIVQ_REQUIRE(k >= 1 && k <= 256, MIVQ_ERR_UNSUPPORTED, "%s: k=%d not in [1, 256]", name, k);
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED, "%s: metric %d",
                 name, metric);
    MIVQ_REQUIRE(nlist <= 16383, MIVQ_ERR_UNSUPPORTED, "%s: nlist=%d > 16383", name, nlist);
    MIVQ_REQUIRE(scan_qb(d, ic_policy(lvq)) > 0, MIVQ_ERR_UNSUPPORTED, "%s: d=%d too large for LDS", name, d);
    *done = nq == 0;
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
    MIVQ_REQUIRE(nbits != 16 || reinterpret_cast<uintptr_t>(codes) % 2 == 0, MIVQ_ERR_INVALID,
                 "ivf_sq_encode: 16-bit codes must be 2-byte aligned");
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
    MIVQ_REQUIRE(nbits != 16 || reinterpret_cast<uintptr_t>(codes) % 2 == 0, MIVQ_ERR_INVALID,
                 "ivf_sq_decode: 16-bit codes must be 2-byte aligned");
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
    const int64_t cs = ((int64_t)d * nbits + 7) / 8 + 8;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(codes);
    int sw = 8;  // the widest store every group start of every row is aligned for
    while (sw > 1 && (nbits % sw != 0 || cs % sw != 0 || addr % sw != 0)) sw >>= 1;
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
    if (!ic_sizes_ok(nq, n, nlist, nprobe, d) || !sq_bits_ok(nbits) || k <= 0 || k > 256 || nlist > 16383) return 0;
    return ic_layout(nq, nlist, nprobe, d, k, false).total;
}

extern "C" size_t mivq_ivf_lvq_search_workspace_bytes(int64_t nq, int64_t n, int32_t nlist, int32_t nprobe, int32_t d,
                                                      int32_t nbits, int32_t k) {
    if (!ic_sizes_ok(nq, n, nlist, nprobe, d) || !lvq_bits_ok(nbits) || k <= 0 || k > 256 || nlist > 16383) return 0;
    return ic_layout(nq, nlist, nprobe, d, k, true).total;
}

extern "C" int mivq_ivf_sq_search(const float* q, int64_t nq, int32_t d, const float* coarse, int32_t nlist,
                                  const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets, const void* list_codes,
                                  const uint32_t* list_ids, const float* lo, const float* den, int32_t nbits,
                                  int32_t metric, int32_t k, void* workspace, size_t workspace_bytes, float* dists,
                                  uint32_t* ids, void* stream) {
    bool done = false;
    const int rc = ic_search_prologue("ivf_sq_search", nq, d, nlist, nprobe, sq_bits_ok(nbits), nbits, false, metric, k, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(q && coarse && probe_l && offsets && list_codes && list_ids && lo && den && dists && ids && workspace,
                 MIVQ_ERR_INVALID, "ivf_sq_search: null pointer");
    MIVQ_REQUIRE(nbits != 16 || reinterpret_cast<uintptr_t>(list_codes) % 2 == 0, MIVQ_ERR_INVALID,
                 "ivf_sq_search: 16-bit codes must be 2-byte aligned");
    const uint8_t* c = static_cast<const uint8_t*>(list_codes);
#define MIVQ_IVF_SQ_SEARCH(F)                                                                                        \
    ivf_code_search<F>("ivf_sq_search", q, nq, d, coarse, nlist, probe_l, nprobe, offsets, c, list_ids, den, lo, metric, \
                       k, workspace, workspace_bytes, dists, ids, stream)
    if (nbits == 4) return MIVQ_IVF_SQ_SEARCH(kSq4);
    if (nbits == 8) return MIVQ_IVF_SQ_SEARCH(kSq8);
    return MIVQ_IVF_SQ_SEARCH(kSq16);
#undef MIVQ_IVF_SQ_SEARCH
}

extern "C" int mivq_ivf_lvq_search(const float* q, int64_t nq, int32_t d, const float* coarse, int32_t nlist,
                                   const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets,
                                   const uint8_t* list_codes, const uint32_t* list_ids, const float* mu, int32_t nbits,
                                   int32_t metric, int32_t k, void* workspace, size_t workspace_bytes, float* dists,
                                   uint32_t* ids, void* stream) {
    bool done = false;
    const int rc = ic_search_prologue("ivf_lvq_search", nq, d, nlist, nprobe, lvq_bits_ok(nbits), nbits, true, metric, k, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(q && coarse && probe_l && offsets && list_codes && list_ids && mu && dists && ids && workspace,
                 MIVQ_ERR_INVALID, "ivf_lvq_search: null pointer");
#define MIVQ_IVF_LVQ_SEARCH(B)                                                                                        \
    case B:                                                                                                           \
        return ivf_code_search<kLvq + B - 1>("ivf_lvq_search", q, nq, d, coarse, nlist, probe_l, nprobe, offsets,      \
                                             list_codes, list_ids, mu, nullptr, metric, k, workspace, workspace_bytes, \
                                             dists, ids, stream)
    switch (nbits) {
        MIVQ_IVF_LVQ_SEARCH(1);
        MIVQ_IVF_LVQ_SEARCH(2);
        MIVQ_IVF_LVQ_SEARCH(3);
        MIVQ_IVF_LVQ_SEARCH(4);
        MIVQ_IVF_LVQ_SEARCH(5);
        MIVQ_IVF_LVQ_SEARCH(6);
        MIVQ_IVF_LVQ_SEARCH(7);
        MIVQ_IVF_LVQ_SEARCH(8);
        default: return MIVQ_ERR_INVALID;
    }
#undef MIVQ_IVF_LVQ_SEARCH
}
