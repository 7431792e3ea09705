// adc.hip — flat ADC (asymmetric distance) search over PQ codes on gfx950.
//
// GPU counterpart of FlatQuantizedIndex.search_with_scores
// (/root/reference/src/haag_vq/methods/search/flat_quantized_index.py:45-76), which decodes
// every code and ranks ||q - x_hat||^2; here the same quantity is assembled from per-query
// lookup tables, sum_m ||q_m - c_{m,code_m}||^2 (canonical order in include/mivq.h):
//   adc_scan_kernel    LUTs of QB queries live in LDS; each wavefront streams 64 code rows
//                      per step (one row per lane, 16-B loads), sums M table entries per
//                      (row, query) and keeps, per query, a wave-resident top-k (element e of
//                      the sorted list in lane e%64, register e/64) that a ballot screens and
//                      a shift-insert updates.  Exact (dist, id) order, so results are
//                      deterministic and identical for any row partition.
// The tables come from adc_lut.hip, the per-wave lists go through topk.hip's merge, and
// M = 16 / 32 searches of k <= 32 take adc_filtered.hip first: this scan then re-runs only the
// queries that path could not certify.
#include "adc_internal.h"
#include "topk.h"

namespace mivq {
namespace {

// Table group mk (= m*ksub + code) holds the QB queries' entries of (m, code) side by side.
// For QB = 8 a lookup is two ds_read_b128 of the group's 16-B halves, and odd lanes read the
// halves in the opposite order: in each 16-lane group of a ds_read_b128 the 8 even lanes then
// hit even 16-B slots of the 256-B bank row and the 8 odd lanes odd ones, two independent
// 8-into-8 draws instead of one 16-into-16 (random codes: 2.94 instead of 3.08 expected LDS
// cycles per lane group).  The lane keeps its two half-sums in lane order (lo = the half read
// first) and swaps them back once per row; each query's sum still runs over m in order.
template <int QB>
__device__ __forceinline__ void lut_add(const float* tab, uint32_t mk, float (&dist)[QB], uint32_t par) {
    const float* g = tab + (size_t)mk * QB;
    if constexpr (QB == 8) {
        const float4 t0 = *reinterpret_cast<const float4*>(g + 4 * par);
        const float4 t1 = *reinterpret_cast<const float4*>(g + 4 * (par ^ 1u));
        dist[0] += t0.x; dist[1] += t0.y; dist[2] += t0.z; dist[3] += t0.w;
        dist[4] += t1.x; dist[5] += t1.y; dist[6] += t1.z; dist[7] += t1.w;
    } else if constexpr (QB >= 4) {
#pragma unroll
        for (int v = 0; v < QB / 4; ++v) {
            const float4 t = *reinterpret_cast<const float4*>(g + 4 * v);
            dist[4 * v + 0] += t.x; dist[4 * v + 1] += t.y; dist[4 * v + 2] += t.z; dist[4 * v + 3] += t.w;
        }
    } else if constexpr (QB == 2) {
        const float2 t = *reinterpret_cast<const float2*>(g);
        dist[0] += t.x; dist[1] += t.y;
    } else {
        dist[0] += g[0];
    }
}

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const f32x4v lds_f4;

// Undoes the odd lanes' half order of lut_add<8> (identity for other QB).
template <int QB>
__device__ __forceinline__ void lut_unswap(float (&dist)[QB], uint32_t par) {
    if constexpr (QB == 8) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float a = dist[q], b = dist[q + 4];
            dist[q] = par ? b : a;
            dist[q + 4] = par ? a : b;
        }
    }
}

// grid (nchunks, ceil(nq / QB)), block kScanWaves waves sharing the QB LUTs in LDS (so the
// CU keeps 4 waves per SIMD despite the 128 KiB of tables).  Part index = chunk*kScanWaves + wave.
// MC > 0 (M = 16 MC, ksub = 256, 16-B aligned code rows): each lane's row of codes is MC
// 16-B loads issued one wave-step ahead, so the LDS lookups never wait on the code fetch
// (MC = 0: 4-B code words loaded in the step that uses them).
template <int R, int QB, int MC>
__device__ __forceinline__ void adc_scan_block(
    const float* __restrict__ lut, int64_t nq, const uint8_t* __restrict__ codes, int64_t n, int M,
    int ksub, int k, int64_t id_offset, int64_t chunk_rows, float* __restrict__ part_d,
    uint32_t* __restrict__ part_i, const int* __restrict__ qlist, const int* __restrict__ qcount, int64_t yb) {
    if constexpr (MC > 0) {
        M = 16 * MC;
        ksub = 256;
    }
    // qlist (the exact re-run of queries the filtered search could not certify, below): query
    // slot s of this launch is query qlist[s], s < *qcount; the lists are written per slot
    // [M][ksub][QB]: the QB queries' entries of one (m, code) are adjacent, so one 16-B LDS
    // read serves 4 queries (random codes: ~2x fewer bank-conflict cycles per lookup than
    // QB separate 4-B reads)
    extern __shared__ __attribute__((aligned(16))) float tab[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t q0 = yb * QB;
    int nqb = (int)min<int64_t>(QB, nq - q0);
    if (qlist != nullptr) {
        const int cnt = *qcount;
        if (q0 >= cnt) return;  // whole workgroup (the caller's loop ends too)
        nqb = (int)min<int64_t>(QB, cnt - q0);
    }
    const int64_t tab_elems = (int64_t)M * ksub;
    for (int64_t e = tid; e < tab_elems * QB; e += kScanWaves * 64) {
        const int64_t mk = e / QB;
        const int qq = (int)(e - mk * QB);
        const int64_t qsrc = qq < nqb ? (qlist != nullptr ? (int64_t)qlist[q0 + qq] : q0 + qq) : 0;
        tab[e] = qq < nqb ? lut[qsrc * tab_elems + mk] : 0.0f;
    }
    __syncthreads();

    WaveTopK<R> top[QB];
    float thr_d[QB];     // element k-1 of each list (wave-uniform)
    uint32_t thr_i[QB];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        top[qq].init();
        thr_d[qq] = INFINITY;
        thr_i[qq] = kNoId;
    }

    const int64_t rbeg = (int64_t)blockIdx.x * chunk_rows;
    const int64_t rend = min(n, rbeg + chunk_rows);
    const bool words = (M % 4) == 0;
    const uint32_t par = (uint32_t)lane & 1u;
    const uint32_t tbase = (uint32_t)(uintptr_t)tab + 16u * par;  // LDS byte address of the half read first
    uint4 cw[MC > 0 ? MC : 1];
    auto fetch = [&](int64_t row) __attribute__((always_inline)) {
        if constexpr (MC > 0) {
            const uint4* cr = reinterpret_cast<const uint4*>(codes + row * (16 * MC));
#pragma unroll
            for (int c = 0; c < MC; ++c) cw[c] = row < rend ? cr[c] : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    fetch(rbeg + (int64_t)wv * 64 + lane);
    for (int64_t base = rbeg + (int64_t)wv * 64; base < rend; base += kScanWaves * 64) {
        const int64_t row = base + lane;
        const bool valid = row < rend;
        float dist[QB];
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) dist[qq] = 0.0f;
        if constexpr (MC > 0) {
            uint4 cur[MC];
#pragma unroll
            for (int c = 0; c < MC; ++c) cur[c] = cw[c];
            fetch(row + kScanWaves * 64);
            // one word (4 sub-codes) per iteration, the queue of words rotating through
            // registers (a rolled loop: unrolled, the 16 MC lookups' reads and addresses
            // outgrow the 128 registers of the 16-wave workgroup)
            uint32_t wq[4 * MC];
#pragma unroll
            for (int c = 0; c < MC; ++c) {
                wq[4 * c + 0] = cur[c].x; wq[4 * c + 1] = cur[c].y;
                wq[4 * c + 2] = cur[c].z; wq[4 * c + 3] = cur[c].w;
            }
#pragma unroll 1
            for (int jw = 0; jw < 4 * MC; ++jw) {
                const uint32_t wrd = wq[0];
                if constexpr (QB == 8) {
                    // byte offsets: group (4 jw + b, code) at 32 (256 (4 jw + b) + code); the half
                    // read first at +16 par, the other at that ^ 16; the b term (a multiple of 32)
                    // goes to the instruction's offset field: 3 VALU per lookup for addresses
                    const uint32_t wofs = tbase + (uint32_t)jw * (4u * 256u * 32u);
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        // inline asm keeps the three ops as written (left to itself the compiler
                        // re-derives o2 from the pieces with more adds)
                        uint32_t cb, o1, o2;
                        asm("v_bfe_u32 %0, %1, %2, 8" : "=v"(cb) : "v"(wrd), "i"(8 * b));
                        asm("v_lshl_add_u32 %0, %1, 5, %2" : "=v"(o1) : "v"(cb), "v"(wofs));
                        asm("v_xor_b32 %0, 16, %1" : "=v"(o2) : "v"(o1));
                        const f32x4v t0 = *(reinterpret_cast<const lds_f4*>((uintptr_t)o1) + b * 512);
                        const f32x4v t1 = *(reinterpret_cast<const lds_f4*>((uintptr_t)o2) + b * 512);
                        dist[0] += t0.x; dist[1] += t0.y; dist[2] += t0.z; dist[3] += t0.w;
                        dist[4] += t1.x; dist[5] += t1.y; dist[6] += t1.z; dist[7] += t1.w;
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        lut_add<QB>(tab, (uint32_t)((4 * jw + b) * 256) + ((wrd >> (8 * b)) & 0xFFu), dist, par);
                }
#pragma unroll
                for (int t = 0; t + 1 < 4 * MC; ++t) wq[t] = wq[t + 1];
            }
            lut_unswap<QB>(dist, par);
        } else if (valid) {
            const uint8_t* cr = codes + row * M;
            if (words) {
                for (int m0 = 0; m0 < M; m0 += 4) {
                    const uint32_t wrd = *reinterpret_cast<const uint32_t*>(cr + m0);
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const uint32_t code = (wrd >> (8 * b)) & 0xFFu;
                        lut_add<QB>(tab, (uint32_t)((m0 + b) * ksub) + code, dist, par);
                    }
                }
            } else {
                for (int m = 0; m < M; ++m) lut_add<QB>(tab, (uint32_t)(m * ksub + cr[m]), dist, par);
            }
            lut_unswap<QB>(dist, par);
        }
        const uint32_t gid = (uint32_t)(id_offset + row);
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            if (qq >= nqb) break;
            float dv = dist[qq];
            if (dv != dv) dv = INFINITY;  // NaN ranks with +inf
            // screen against the cached k-th element; it only moves when something is inserted
            // (WaveTopK::offer and ::store written out: through the calls adc_scan_kernel<4, 8, 0>
            // spills 36 instead of 28 bytes and the QB = 1 variants take up to 3 more registers)
            unsigned long long mask = __ballot(valid && pair_less(dv, gid, thr_d[qq], thr_i[qq]));
            while (mask) {
                const int src = __builtin_ctzll(mask);
                mask &= mask - 1;
                const float cd = __shfl(dv, src);
                const uint32_t ci = __shfl(gid, src);
                if (!pair_less(cd, ci, thr_d[qq], thr_i[qq])) continue;
                top[qq].insert(cd, ci, k, lane);
                top[qq].kth(k, thr_d[qq], thr_i[qq]);
            }
        }
    }
    const int64_t part = (int64_t)blockIdx.x * kScanWaves + wv;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        if (qq >= nqb) break;
        float* od = part_d + (part * nq + q0 + qq) * k;
        uint32_t* oi = part_i + (part * nq + q0 + qq) * k;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = r * 64 + lane;
            if (e < k) { od[e] = top[qq].d[r]; oi[e] = top[qq].id[r]; }
        }
    }
}

// Query block blockIdx.y (fp32 scan of every query), or -- qlist, the re-run of the queries
// the filtered search could not certify -- list slots blockIdx.y, + gridDim.y, ... while they
// exist: a small grid whatever the count (0 failures: every workgroup returns at once).
template <int R, int QB, int MC>
__global__ __launch_bounds__(kScanWaves * 64) void adc_scan_kernel(
    const float* __restrict__ lut, int64_t nq, const uint8_t* __restrict__ codes, int64_t n, int M,
    int ksub, int k, int64_t id_offset, int64_t chunk_rows, float* __restrict__ part_d,
    uint32_t* __restrict__ part_i, const int* __restrict__ qlist, const int* __restrict__ qcount) {
    if (qlist == nullptr) {
        adc_scan_block<R, QB, MC>(lut, nq, codes, n, M, ksub, k, id_offset, chunk_rows, part_d, part_i, qlist, qcount,
                                  (int64_t)blockIdx.y);
        return;
    }
    const int cnt = *qcount;
    for (int64_t yb = blockIdx.y; yb * QB < cnt; yb += gridDim.y) {
        adc_scan_block<R, QB, MC>(lut, nq, codes, n, M, ksub, k, id_offset, chunk_rows, part_d, part_i, qlist, qcount,
                                  yb);
        __syncthreads();  // the next block's table overwrites this one's
    }
}

int adc_qb(int M, int ksub) {
    const int64_t per = (int64_t)M * ksub * 4;
    const int64_t budget = 128 * 1024;
    if (per * 8 <= budget) return 8;
    if (per * 4 <= budget) return 4;
    if (per * 2 <= budget) return 2;
    if (per <= 160 * 1024) return 1;
    return 0;
}

template <int R, int QB>
hipError_t launch_scan(const float* lut, int64_t nq, const uint8_t* codes, int64_t n, int M, int ksub, int k,
                       int64_t id_offset, int64_t nch, float* pd, uint32_t* pi, hipStream_t st,
                       const int* qlist = nullptr, const int* qcount = nullptr, bool small_grid = false) {
    const size_t smem = (size_t)QB * M * ksub * sizeof(float);
    const bool vec = ksub == 256 && reinterpret_cast<uintptr_t>(codes) % 16 == 0;
    auto kern = vec && M == 16 ? adc_scan_kernel<R, QB, 1> : vec && M == 32 ? adc_scan_kernel<R, QB, 2>
                                                                             : adc_scan_kernel<R, QB, 0>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    const int64_t chunk_rows = ceil_div(n, nch);
    // the re-run of uncertified queries: one round of workgroups looping over the list slots
    // (small_grid, a test hook: one column, so every workgroup walks several slot blocks)
    const int64_t qgrid = qlist != nullptr ? (small_grid ? 1 : std::max<int64_t>(1, std::min<int64_t>(ceil_div(nq, QB), 256 / nch)))
                                           : ceil_div(nq, QB);
    hipLaunchKernelGGL(kern, dim3((unsigned)nch, (unsigned)qgrid), dim3(kScanWaves * 64), smem, st, lut, nq, codes,
                       n, M, ksub, k, id_offset, chunk_rows, pd, pi, qlist, qcount);
    return hipGetLastError();
}

// Row chunks of the re-run of uncertified queries: ~32k rows each (one failed query costs a
// few tens of microseconds, not a whole-database workgroup), as long as the re-run's part
// lists -- sized for every query, since the host does not know how many fail -- stay within
// kRerunListBytes: (16 parts per chunk) x nq x k x 8 B per chunk.  At nq = 10,000, k = 32 that
// is 40 MB per chunk, so 6 chunks (a failed query then scans ~1/6 of the rows per workgroup:
// slower, never wrong); below 1,000 queries at k = 10 the 256 chunks fit.  (the
// unbounded form sized 10.5 GB at n = 10M, nq = 10k, k = 32.)
constexpr size_t kRerunListBytes = size_t(256) << 20;
int64_t adc_fallback_chunks(int64_t nq, int64_t n, int k) {
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(256, ceil_div(n, 32768)));
    const size_t per_chunk = (size_t)kScanWaves * (size_t)std::max<int64_t>(nq, 1) * (size_t)k * 8u;
    return std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)(kRerunListBytes / per_chunk)));
}

// The workspace of mivq_adc_search (nq, n > 0): the fp32 scan's part lists (parts, nq, k) --
// distances at pd, ids at pi, sized for the scan of every query (nch_exact chunks) and, on a
// filtered shape, for the re-run of the uncertified ones (nch_rerun) -- then the filtered
// path's regions F.  QB == 0: the tables do not fit LDS, no search.
struct AdcSearchLayout {
    int QB;
    bool fshape;
    int64_t nch_exact, nch_rerun, parts;
    size_t pd, pi, total;
    AdcFilteredLayout F;
};

AdcSearchLayout adc_search_layout(int64_t nq, int64_t n, int M, int nbits, int k) {
    AdcSearchLayout L{};
    L.QB = adc_qb(M, 1 << nbits);
    if (L.QB == 0) return L;
    L.fshape = adc_filtered_shape(M, 1 << nbits, k);
    L.nch_exact = adc_chunks(nq, n, L.QB);
    L.nch_rerun = L.fshape ? adc_fallback_chunks(nq, n, k) : 0;
    L.parts = std::max(L.nch_exact, L.nch_rerun) * kScanWaves;
    const size_t list = align_up((size_t)L.parts * nq * k * 4, 256);
    L.pd = 0;
    L.pi = list;
    L.total = 2 * list;
    if (L.fshape) {
        L.F = adc_filtered_layout(nq, n, M, k, L.total);
        L.total = L.F.total;
    }
    return L;
}

}  // namespace

// Row chunks per query block.  The scan workgroups (16 waves, up to 128 KiB of LDS) run one
// per CU, so the grid of nch * qblocks workgroups takes ceil(nch * qblocks / 256) rounds, each
// as long as one workgroup's table fill (about half a wave-step of 1024 rows) plus its
// ceil(n / nch / 1024) wave-steps: pick the nch of least total time (the smallest on ties:
// fewer partial lists; a larger count must gain 2 %: the model is coarse, and every chunk adds
// a part list per query).  nq = 1000 at QB = 8, n = 1M: 2 chunks, 250 workgroups in one round,
// instead of 625 in three of which the last is 44 % full.
int64_t adc_chunks(int64_t nq, int64_t n, int QB) {
    const int64_t qblocks = ceil_div(nq, QB);
    const int64_t step_rows = 64 * kScanWaves;
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(1024, ceil_div(n, step_rows)));
    int64_t best = 1;
    double best_cost = 0.0;
    for (int64_t nch = 1; nch <= cap; ++nch) {
        const double cost = (double)ceil_div(nch * qblocks, 256) * ((double)ceil_div(ceil_div(n, nch), step_rows) + 0.5);
        if (nch == 1 || cost < best_cost * 0.98) { best = nch; best_cost = cost; }
    }
    return best;
}

}  // namespace mivq

using namespace mivq;

extern "C" size_t mivq_adc_search_workspace_bytes(int64_t nq, int64_t n, int32_t M, int32_t nbits, int32_t k) {
    if (nq <= 0 || n <= 0 || M <= 0 || k <= 0 || nbits < 1 || nbits > 8) return 0;
    return adc_search_layout(nq, n, M, nbits, k).total;
}

extern "C" int mivq_adc_search(const float* lut, int64_t nq, const uint8_t* codes, int64_t n, int32_t M,
                               int32_t nbits, int32_t k, int64_t id_offset, void* workspace,
                               size_t workspace_bytes, float* dists, uint32_t* ids, uint32_t flags, void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && M > 0 && k > 0, MIVQ_ERR_INVALID,
                 "adc_search: bad sizes nq=%lld n=%lld M=%d k=%d", (long long)nq, (long long)n, M, k);
    MIVQ_REQUIRE((flags & ~(MIVQ_ADC_FORCE_EXACT | MIVQ_ADC_NO_RERUN | MIVQ_ADC_SMALL_RERUN_GRID)) == 0,
                 MIVQ_ERR_INVALID, "adc_search: unknown flags 0x%x", flags);
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_UNSUPPORTED, "adc_search: nbits=%d", nbits);
    MIVQ_REQUIRE(k <= 256, MIVQ_ERR_UNSUPPORTED, "adc_search: k=%d > 256", k);
    const int ksub = 1 << nbits;
    MIVQ_REQUIRE(adc_qb(M, ksub) > 0, MIVQ_ERR_UNSUPPORTED, "adc_search: M*ksub=%d tables do not fit LDS", M * ksub);
    MIVQ_REQUIRE(id_offset >= 0 && id_offset + n <= (int64_t)kNoId, MIVQ_ERR_INVALID,
                 "adc_search: global ids must fit uint32");
    if (nq == 0) return MIVQ_OK;
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        // nothing to rank: every slot is the sentinel
        MIVQ_REQUIRE(dists && ids, MIVQ_ERR_INVALID, "adc_search: null pointer");
        const hipError_t e = launch_topk_merge(nullptr, nullptr, 0, nq, k, dists, ids, st);
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "adc_search(empty): %s", hipGetErrorString(e));
        return MIVQ_OK;
    }
    MIVQ_REQUIRE(lut && codes && dists && ids, MIVQ_ERR_INVALID, "adc_search: null pointer");
    const AdcSearchLayout L = adc_search_layout(nq, n, M, nbits, k);
    MIVQ_REQUIRE(workspace && workspace_bytes >= L.total, MIVQ_ERR_WORKSPACE, "adc_search: workspace %zu < %zu",
                 workspace_bytes, L.total);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float* pd = reinterpret_cast<float*>(ws + L.pd);
    uint32_t* pi = reinterpret_cast<uint32_t*>(ws + L.pi);
    // the filtered path (integer-LUT scan + exact re-rank + certificate; the fp32 scan re-runs
    // only the uncertified queries): same results, ~half the LDS traffic per (query, row)
    const bool filtered = L.fshape && reinterpret_cast<uintptr_t>(codes) % 16 == 0 &&
                          reinterpret_cast<uintptr_t>(lut) % 16 == 0 && !(flags & MIVQ_ADC_FORCE_EXACT);
    const int* qlist = nullptr;
    const int* qcount = nullptr;
    hipError_t e;
    const bool no_fallback = (flags & MIVQ_ADC_NO_RERUN) != 0;  // test hook: certified queries only, the others NaN
    if (filtered) {
        MIVQ_REQUIRE(adc_filtered_offsets_fit(L.F, n, M), MIVQ_ERR_UNSUPPORTED,
                     "adc_search: %lld rows per chunk overflow the integer scan's 32-bit offsets",
                     (long long)ceil_div(n, L.F.nch));
        if (no_fallback) {
            e = hipMemsetAsync(dists, 0xFF, (size_t)nq * k * sizeof(float), st);
            if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "adc_search: %s", hipGetErrorString(e));
        }
        e = launch_filtered(M, lut, nq, codes, n, k, id_offset, ws, L.F, dists, ids, st);
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "adc_search (filtered): %s", hipGetErrorString(e));
        qcount = reinterpret_cast<const int*>(ws + L.F.fail);
        qlist = qcount + 1;
        if (no_fallback) return MIVQ_OK;
    }
    const int64_t nch = filtered ? L.nch_rerun : L.nch_exact;
    const int parts = (int)(nch * kScanWaves);
    const bool sg = filtered && (flags & MIVQ_ADC_SMALL_RERUN_GRID) != 0;
    e = with_topk_regs(k, [&](auto R) {
        return with_query_block(L.QB, [&](auto QB) {
            return launch_scan<decltype(R)::value, decltype(QB)::value>(lut, nq, codes, n, M, ksub, k, id_offset, nch, pd,
                                                                        pi, st, qlist, qcount, sg);
        });
    });
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "adc_scan: %s", hipGetErrorString(e));
    e = launch_topk_merge(pd, pi, parts, nq, k, dists, ids, st, qlist, qcount);
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "topk_merge: %s", hipGetErrorString(e));
    return MIVQ_OK;
}
