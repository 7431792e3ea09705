// ivf_listpq.hip — IVF lists with one PQ codebook per list for gfx950: the decode of the list
// codes and the ADC search over the probed lists.
//
// GPU counterpart of the reference's IvfQuantizedIndex around a ProductQuantizer
// (run_benchmarks' pq_ivf): every list has its own (M, ksub, dsub) codebook, fitted on the list's
// residuals x - coarse[l].  The lookup table of a search therefore belongs to a (query, probed
// list) pair, T = mivq_adc_lut(q, cb[l] + coarse[l]), and the key of a row is mivq_adc_search's
// sum over its codes (include/mivq.h).  Building the tables is the dominant cost, so they are
// built once per pair, after the pairs are sorted by list, and kept in the driver's per-pair
// workspace region:
//
//   ivf_listpq_decode_kernel  thread = output float: the sub-centroid's float plus the centroid's.
//   ivf_prep_kernel           (ivf_internal.h) the driver's pair prologue, nothing else.
//   ivf_listpq_table_kernel   grid (item bound, groups of table units), 256 threads, thread =
//                             table entry (m, j): the list's codebook row is read once per work
//                             item and serves its QB pairs, whose query slices and the centroid
//                             slice sit in LDS (broadcast reads).  Scalar chains.
//   ivf_listpq_scan_kernel    grid (item bound, S), 512 threads, lane = 4 rows per 2048-row step.
//                             The tables of the QB pairs are staged into LDS in chunks of
//                             subspaces, interleaved [m][j][pair], so one LDS read serves the QB
//                             accumulators of a row; the key's sum is sequential in m, so chunking
//                             preserves it.  WaveTopK selection inside the scan, the waves' lists
//                             merged in LDS into one list per (pair, range).
// The search runs on the probed-list driver (ivf_internal.h).
#include "adc_internal.h"
#include "ivf_internal.h"
#include "mivq_common.h"
#include "topk.h"

#include <algorithm>

namespace mivq {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kLpMaxD = 1 << 20;      // M * ksub stays within 32 bits
constexpr int kLpMaxQB = 4;           // pairs per work item at most
constexpr int kLpWaves = 8;           // waves per scan workgroup
constexpr int kLpRows = 4;            // rows per lane per step
constexpr int kLpStep = kLpWaves * 64 * kLpRows;  // 2048 rows per step: a staged chunk serves 4 rows per lane
constexpr int kLpTile = 1024;         // the S row ranges of a list are whole multiples of this
constexpr int kLpChunkBytes = 64 * 1024;          // the scan's table chunk in LDS
constexpr int kLpTabThreads = 256;    // a table unit: 256 consecutive entries (m, j)
constexpr int kLpTabDims = 2048;      // floats per staged row of the table kernel

// ---------------------------------------------------------------- decode
// out[i][m*dsub + t] = cb[l][m][code_m][t] + coarse[l][m*dsub + t], l = assign[i].
__global__ __launch_bounds__(256) void ivf_listpq_decode_kernel(const uint8_t* __restrict__ codes, int64_t n, int d,
                                                                int M, int ksub, const float* __restrict__ cb,
                                                                const float* __restrict__ coarse,
                                                                const uint32_t* __restrict__ assign,
                                                                float* __restrict__ out) {
    const int dsub = d / M;
    const int64_t total = n * (int64_t)d;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / d;
        const int t = (int)(e - row * d);
        const int m = t / dsub, tt = t - m * dsub;
        const int64_t l = assign[row];
        const int code = codes[row * M + m] & (ksub - 1);
        out[e] = __fadd_rn(cb[((l * M + m) * ksub + code) * dsub + tt], coarse[l * d + t]);
    }
}

// ---------------------------------------------------------------- search
struct LpTab {
    IvfScan s;
    const float* q;       // (nqc, d) the chunk's queries
    const float* cb;      // (nlist, M, ksub, dsub)
    const float* coarse;  // (nlist, d)
    float* tab;           // (pairs, M * ksub): the table of the pair at sorted position p
    int d, M, nbits, metric;
    int tt;      // dims of a subspace per staged tile (dsub: the whole sub-vector)
    int group;   // units per staged window (1 unless tt == dsub)
    int vec;     // 16-B loads: dsub % 4 == 0 and the codebooks 16-B aligned
};

// Work item blockIdx.x = (list l, sorted pairs [pb, pb + np)), np <= QB.  The M * ksub entries of
// a table are cut into units of 256 consecutive entries (ksub = 256: one subspace; smaller ksub:
// 256 / ksub subspaces), thread = entry; a workgroup takes the groups of units blockIdx.y,
// blockIdx.y + gridDim.y, ...  Entry (m, j) of pair qq:
//     e_t = cb[l][m][j][t] + c[m*dsub + t];  L2: fmaf chain of (q_t - e_t)^2,  IP: -(chain of q_t e_t)
// over t ascending: mivq_adc_lut on the shifted codebook.  LDS: rows 0 .. QB-1 the pairs' query
// slices, row QB the centroid's, for the dims of the group's subspaces (tile [t0, t0 + tt) of
// each when a sub-vector is longer than the row).
template <int QB>
__global__ __launch_bounds__(kLpTabThreads) void ivf_listpq_table_kernel(const LpTab A) {
    __shared__ __attribute__((aligned(16))) float sm[(QB + 1) * kLpTabDims];
    if (A.s.past_items()) return;
    const int tid = threadIdx.x;
    const uint2 item = A.s.items[blockIdx.x];
    const uint32_t l = item.x;
    const int64_t pb = item.y;
    const int np = (int)min<int64_t>(QB, A.s.poff[l + 1] - pb);
    const int d = A.d, M = A.M, nbits = A.nbits, ksub = 1 << nbits, dsub = d / M, tt = A.tt;
    const int tabn = M * ksub;
    const int ms = max(1, kLpTabThreads >> nbits);  // subspaces per unit
    const int nunits = (tabn + kLpTabThreads - 1) / kLpTabThreads;
    const int ngroups = (nunits + A.group - 1) / A.group;
    const bool l2 = A.metric == MIVQ_METRIC_L2;
    const float* qr[QB + 1];  // the rows staged: the pairs' queries (slots past np repeat pair 0), the centroid
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) qr[qq] = A.q + (int64_t)(A.s.porder[pb + (qq < np ? qq : 0)] / A.s.nprobe) * d;
    qr[QB] = A.coarse + (int64_t)l * d;
    const float* cbl = A.cb + (int64_t)l * tabn * dsub;
    for (int g = blockIdx.y; g < ngroups; g += gridDim.y) {
        const int u0 = g * A.group, u1 = min(nunits, u0 + A.group);
        const int m0 = u0 * ms, m1 = min(M, u1 * ms);  // the group's subspaces
        for (int u = u0; u < u1; ++u) {
            const int e = u * kLpTabThreads + tid;
            const bool live = e < tabn;
            const int ml = live ? (e >> nbits) - m0 : 0;
            const float* crow = cbl + (int64_t)(live ? e : 0) * dsub;
            float acc[QB];
#pragma unroll
            for (int qq = 0; qq < QB; ++qq) acc[qq] = 0.0f;
            for (int t0 = 0; t0 < dsub; t0 += tt) {
                const int nt = min(tt, dsub - t0);
                if (tt < dsub || u == u0) {  // block-uniform: a window of whole sub-vectors serves the group
                    __syncthreads();
                    for (int x = tid; x < (m1 - m0) * nt; x += kLpTabThreads) {
                        const int mm = x / nt, t = x - mm * nt;
                        const int dim = (m0 + mm) * dsub + t0 + t;
#pragma unroll
                        for (int r = 0; r <= QB; ++r) sm[r * kLpTabDims + mm * tt + t] = qr[r][dim];
                    }
                    __syncthreads();
                }
                if (!live) continue;
                const float* qs = sm + ml * tt;
                auto step = [&](float cv, int t) __attribute__((always_inline)) {
                    const float ev = __fadd_rn(cv, qs[QB * kLpTabDims + t]);
#pragma unroll
                    for (int qq = 0; qq < QB; ++qq) {
                        const float qv = qs[qq * kLpTabDims + t];
                        if (l2) {
                            const float df = __fsub_rn(qv, ev);
                            acc[qq] = __builtin_fmaf(df, df, acc[qq]);
                        } else {
                            acc[qq] = __builtin_fmaf(qv, ev, acc[qq]);
                        }
                    }
                };
                if (A.vec) {  // nt % 4 == 0
                    for (int t = 0; t < nt; t += 4) {
                        const v4f c4 = *reinterpret_cast<const v4f*>(crow + t0 + t);
                        step(c4.x, t);
                        step(c4.y, t + 1);
                        step(c4.z, t + 2);
                        step(c4.w, t + 3);
                    }
                } else {
                    for (int t = 0; t < nt; ++t) step(crow[t0 + t], t);
                }
            }
            if (live) {
#pragma unroll
                for (int qq = 0; qq < QB; ++qq)
                    if (qq < np) A.tab[(pb + qq) * tabn + e] = l2 ? acc[qq] : -acc[qq];
            }
        }
    }
}

struct LpScan {
    IvfScan s;
    const float* tab;  // (pairs, M * ksub) by sorted position
    int M, nbits;
    int mc;     // subspaces per LDS chunk (M: the tables are staged once)
    int words;  // code rows read 4 bytes at a time
    int vec;    // tables staged with 16-B loads: ksub % 4 == 0 and the region 16-B aligned
};

// Grid (item bound, S), 512 threads.  Work item (list l, pairs [pb, pb + np)), row range s of the
// list (S equal ranges, whole multiples of 1024 rows, walked in 2048-row steps).  LDS: [mc][ksub][QB] table entries of the
// chunk's subspaces, the QB pairs' values of an entry adjacent.  Lane = kLpRows rows: the
// accumulators of (row, pair) take the chunk's lookups in ascending m, chunk after chunk, which
// is the sequential sum of the key.  Every wave keeps the WaveTopK lists of the QB pairs over its
// rows; afterwards the LDS is reused to merge the waves' lists, pair by pair, into wave 0's,
// which goes to part (probe slot) * S + s of the pair's query.
template <int R, int QB>
__global__ __launch_bounds__(kLpWaves * 64) void ivf_listpq_scan_kernel(const LpScan A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (A.s.past_items()) return;
    const IvfItem it = ivf_item<QB, kLpTile>(A.s);
    if (it.empty()) return;
    const auto [l, pb0, np, rb, re] = it;
    const int M = A.M, ksub = 1 << A.nbits, mc = A.mc;
    const int64_t tabn = (int64_t)M * ksub;
    const float* tp[QB];  // the pairs' tables; slots past np repeat pair 0 (in range), never stored
    int64_t op[QB];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        tp[qq] = A.tab + (pb0 + (qq < np ? qq : 0)) * tabn;
        op[qq] = A.s.porder[pb0 + (qq < np ? qq : 0)];
    }
    auto stage = [&](int m0, int nm) {
        const float* src[QB];
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) src[qq] = tp[qq] + (int64_t)m0 * ksub;
        if (A.vec) {  // 4 entries of every pair per thread, transposed in registers
            for (int x = tid * 4; x < nm * ksub; x += kLpWaves * 64 * 4) {
                v4f v[QB];
#pragma unroll
                for (int qq = 0; qq < QB; ++qq) v[qq] = *reinterpret_cast<const v4f*>(src[qq] + x);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int qq = 0; qq < QB; ++qq) smem[(x + j) * QB + qq] = v[qq][j];
                }
            }
        } else {
            for (int x = tid; x < nm * ksub; x += kLpWaves * 64) {
#pragma unroll
                for (int qq = 0; qq < QB; ++qq) smem[x * QB + qq] = src[qq][x];
            }
        }
    };
    const bool once = mc >= M;
    if (once) {
        stage(0, M);
        __syncthreads();
    }
    WaveTopK<R> top[QB];
    float thr_d[QB];
    uint32_t thr_i[QB];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        top[qq].init();
        thr_d[qq] = INFINITY;
        thr_i[qq] = kNoId;
    }
    const int k = A.s.k;
    for (int64_t base = rb; base < re; base += kLpStep) {  // block-uniform
        int64_t row[kLpRows];
        bool valid[kLpRows];
        float acc[kLpRows][QB];
#pragma unroll
        for (int r = 0; r < kLpRows; ++r) {
            row[r] = base + (r * kLpWaves + wv) * 64 + lane;
            valid[r] = row[r] < re;
#pragma unroll
            for (int qq = 0; qq < QB; ++qq) acc[r][qq] = 0.0f;
        }
        for (int m0 = 0; m0 < M; m0 += mc) {
            const int nm = min(mc, M - m0);
            if (!once) {
                __syncthreads();  // the previous chunk is consumed
                stage(m0, nm);
                __syncthreads();
            }
#pragma unroll
            for (int r = 0; r < kLpRows; ++r) {
                if (!valid[r]) continue;
                const uint8_t* cr = A.s.codes + row[r] * M + m0;
                auto look = [&](int mm, uint32_t code) __attribute__((always_inline)) {
                    const float* tv = smem + ((int64_t)mm * ksub + (code & (uint32_t)(ksub - 1))) * QB;
#pragma unroll
                    for (int qq = 0; qq < QB; ++qq) acc[r][qq] = __fadd_rn(acc[r][qq], tv[qq]);
                };
                if (A.words) {  // M % 4 == 0, so is mc when it is below M
                    for (int mm = 0; mm < nm; mm += 4) {
                        const uint32_t w = *reinterpret_cast<const uint32_t*>(cr + mm);
#pragma unroll
                        for (int bb = 0; bb < 4; ++bb) look(mm + bb, (w >> (8 * bb)) & 0xFFu);
                    }
                } else {
                    for (int mm = 0; mm < nm; ++mm) look(mm, cr[mm]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kLpRows; ++r) {
            const uint32_t gid = valid[r] ? A.s.ids[row[r]] : kNoId;
#pragma unroll
            for (int qq = 0; qq < QB; ++qq) {
                if (qq >= np) break;  // block-uniform
                float dv = acc[r][qq];
                if (dv != dv) dv = INFINITY;
                top[qq].offer(valid[r], dv, gid, k, lane, thr_d[qq], thr_i[qq]);
            }
        }
    }
    // the waves' lists -> one list per pair: waves 1.. write theirs to LDS (the tables are no
    // longer read), wave 0 takes them in, 64 candidates per offer
    __syncthreads();
    float* md = smem;
    uint32_t* mi = reinterpret_cast<uint32_t*>(smem + (kLpWaves - 1) * k);
    const int total = (kLpWaves - 1) * k;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        if (qq >= np) break;  // block-uniform
        if (wv > 0) top[qq].store(md + (wv - 1) * k, mi + (wv - 1) * k, k, lane);
        __syncthreads();
        if (wv == 0) {
            for (int e0 = 0; e0 < total; e0 += 64) {
                const int e = e0 + lane;
                const bool ok = e < total;
                top[qq].offer(ok, ok ? md[e] : INFINITY, ok ? mi[e] : kNoId, k, lane, thr_d[qq], thr_i[qq]);
            }
            const int64_t obase = A.s.part_base(op[qq], blockIdx.y);
            top[qq].store(A.s.pd + obase, A.s.pi + obase, k, lane);
        }
        __syncthreads();  // the buffer is rewritten for the next pair
    }
}

// ---------------------------------------------------------------- host side
// The table bytes of a pair are counted in the chunk estimate: the queries per chunk shrink with
// M * ksub, so the workspace stays under the driver's cap (one query per chunk at the least).
IvfLayout lp_layout(int64_t nq, int nlist, int nprobe, int k, int QB, int M, int nbits) {
    const size_t tab = (size_t)M * ((size_t)1 << nbits) * sizeof(float);
    return ivf_layout(nq, nlist, nprobe, k, QB, tab, 0, 16 + tab);
}

bool lp_shape_ok(int d, int M, int nbits) {
    return d > 0 && d <= kLpMaxD && M > 0 && d % M == 0 && nbits >= 1 && nbits <= 8;
}

template <int QB>
hipError_t launch_lp_tables(LpTab A, int64_t pairs, int64_t maxitems, hipStream_t st) {
    const int ksub = 1 << A.nbits, dsub = A.d / A.M;
    const int ms = std::max(1, kLpTabThreads >> A.nbits);
    const int64_t nunits = ceil_div((int64_t)A.M * ksub, kLpTabThreads);
    // enough workgroups for the chip when the items are few, long loops over units when many
    const int64_t want = std::min<int64_t>(nunits, std::max<int64_t>(1, ceil_div(8192, std::max<int64_t>(1, pairs / QB))));
    if ((int64_t)ms * dsub <= kLpTabDims) {
        A.tt = dsub;
        A.group = (int)std::min<int64_t>(kLpTabDims / (ms * dsub), ceil_div(nunits, want));
    } else {
        A.tt = kLpTabDims / ms;  // a power of two >= 16
        A.group = 1;
    }
    const int64_t ngroups = ceil_div(nunits, A.group);
    A.vec = dsub % 4 == 0 && reinterpret_cast<uintptr_t>(A.cb) % 16 == 0;
    hipLaunchKernelGGL(ivf_listpq_table_kernel<QB>, dim3((unsigned)maxitems, (unsigned)std::min<int64_t>(ngroups, 65535)),
                       dim3(kLpTabThreads), 0, st, A);
    return hipGetLastError();
}

template <int R, int QB>
hipError_t launch_lp_scan(LpScan A, int64_t maxitems, hipStream_t st) {
    const int ksub = 1 << A.nbits;
    const int fit = kLpChunkBytes / (QB * ksub * (int)sizeof(float));  // >= 16
    A.mc = A.M <= fit ? A.M : fit / 4 * 4;
    A.words = A.M % 4 == 0 && reinterpret_cast<uintptr_t>(A.s.codes) % 4 == 0;
    A.vec = ksub % 4 == 0 && reinterpret_cast<uintptr_t>(A.tab) % 16 == 0;
    const size_t chunk = (size_t)A.mc * ksub * QB * sizeof(float);
    const size_t smem = std::max(chunk, (size_t)(kLpWaves - 1) * A.s.k * 8);
    auto kern = ivf_listpq_scan_kernel<R, QB>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)maxitems, (unsigned)A.s.S), dim3(kLpWaves * 64), smem, st, A);
    return hipGetLastError();
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_ivf_listpq_decode(const uint8_t* codes, int64_t n, int32_t d, int32_t M, int32_t nbits,
                                      const float* codebooks, const float* coarse, int32_t nlist,
                                      const uint32_t* assign, float* out, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0 && d <= kLpMaxD && M > 0 && nlist > 0, MIVQ_ERR_INVALID,
                 "ivf_listpq_decode: bad sizes n=%lld d=%d M=%d nlist=%d", (long long)n, d, M, nlist);
    MIVQ_REQUIRE(d % M == 0, MIVQ_ERR_INVALID, "ivf_listpq_decode: d=%d must be divisible by M=%d", d, M);
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "ivf_listpq_decode: nbits=%d not in [1, 8]", nbits);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(codes && codebooks && coarse && assign && out, MIVQ_ERR_INVALID, "ivf_listpq_decode: null pointer");
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n * (int64_t)d, 256), 1 << 20));
    hipLaunchKernelGGL(ivf_listpq_decode_kernel, grid, dim3(256), 0, as_stream(stream), codes, n, d, M, 1 << nbits,
                       codebooks, coarse, assign, out);
    return check_launch("ivf_listpq_decode");
}

extern "C" size_t mivq_ivf_listpq_search_workspace_bytes(int64_t nq, int64_t n, int32_t nlist, int32_t nprobe,
                                                         int32_t d, int32_t M, int32_t nbits, int32_t k) {
    if (!ivf_shape_ok(nq, n, nlist, nprobe, d, k) || !lp_shape_ok(d, M, nbits)) return 0;
    return lp_layout(nq, nlist, nprobe, k, ivf_pairs_per_item(kLpMaxQB, nq, nlist, nprobe), M, nbits).total;
}

extern "C" int mivq_ivf_listpq_search(const float* q, int64_t nq, int32_t d, int32_t M, int32_t nbits,
                                      const float* codebooks, const float* coarse, int32_t nlist,
                                      const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets,
                                      const uint8_t* list_codes, const uint32_t* list_ids, int32_t metric, int32_t k,
                                      void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids,
                                      void* stream) {
    const char* name = "ivf_listpq_search";
    const int rc = ivf_search_check(name, nq, d, kLpMaxD, nlist, nprobe, k, metric);
    if (rc != MIVQ_OK) return rc;
    MIVQ_REQUIRE(M > 0 && d % M == 0, MIVQ_ERR_INVALID, "%s: d=%d must be divisible by M=%d", name, d, M);
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "%s: nbits=%d not in [1, 8]", name, nbits);
    if (nq == 0) return MIVQ_OK;
    MIVQ_REQUIRE(q && codebooks && coarse && probe_l && offsets && list_codes && list_ids && dists && ids,
                 MIVQ_ERR_INVALID, "%s: null pointer", name);
    hipStream_t st = as_stream(stream);
    return with_query_block<kLpMaxQB>(ivf_pairs_per_item(kLpMaxQB, nq, nlist, nprobe), [&](auto QB) {
        constexpr int kQB = decltype(QB)::value;
        const IvfLayout L = lp_layout(nq, nlist, nprobe, k, kQB, M, nbits);
        return ivf_probed_search<kQB>(
            name, L, nq, nlist, nprobe, k, offsets, list_codes, list_ids, workspace, workspace_bytes, dists, ids, stream,
            [&](const IvfChunk& c) {
                hipLaunchKernelGGL(ivf_prep_kernel<64>, dim3((unsigned)c.pairs), dim3(64), 0, st,
                                   probe_l + c.a0 * nprobe, nlist, nprobe, c.nqc, L.S, k, c.keys, c.scan.pd, c.scan.pi);
                return hipGetLastError();
            },
            [&](const IvfChunk& c, int64_t maxitems) {
                float* tab = reinterpret_cast<float*>(c.xa);
                const LpTab T{c.scan, q + c.a0 * d, codebooks, coarse, tab, d, M, nbits, metric, 0, 1, 0};
                const hipError_t e = launch_lp_tables<kQB>(T, c.pairs, maxitems, st);
                if (e != hipSuccess) return e;
                const LpScan A{c.scan, tab, M, nbits, 0, 0, 0};
                return with_topk_regs(k, [&](auto R) { return launch_lp_scan<decltype(R)::value, kQB>(A, maxitems, st); });
            });
    });
}
