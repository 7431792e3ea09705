// exact_search.hip — exact brute-force search on gfx950 over an f32 database
// (mivq_flat_search, mivq_pairwise_distances) and over SQ-4/8/16, RaBitQ-1, LVQ-1..8 and
// Extended RaBitQ-1..8 codes.
//
// One distance chain, two paths, every row format.  A format (Fmt<>, code_internal.h) says how a
// row's floats are fetched; f32 is the format with no parameters and no dequantisation.  The packed codes
// are read once and dequantised in registers, so no fp32 copy of a coded database exists at
// any point.  Every reconstruction x^_t is the float the decode kernels write (sq.hip
// sq_decode_kernel, rabitq.hip rabitq_decode_kernel, lvq.hip lvq_decode_kernel; one rounding
// per step, -ffp-contract=off), so a code search's ids and distances are bit-identical to
// decode + mivq_flat_search.  Extended RaBitQ rows are searched in the rotated domain: the
// reconstruction is y^_t = (float)(o^_t nrm) with o^_t the f64 erq_dequantize_kernel writes
// (extrabitq.hip), the queries arrive rotated, and the result is mivq_flat_search(qy, y^).
//
//   code_scan_kernel      the streaming scan: grid (nchunks, ceil(nq / QB)); QB queries and the
//                         per-dimension parameters (SQ: den, lo; RaBitQ: centroid; LVQ: mu;
//                         f32: none; Extended RaBitQ: none, but its 2^B f64 levels) in LDS,
//                         lane = database row, distances as sequential fmaf chains over t,
//                         WaveTopK lists merged by launch_topk_merge.  A row is read with 16-B
//                         (RaBitQ, LVQ, Extended RaBitQ: 8-B) loads while whole loads fit and
//                         the rows are that aligned, then 4-B loads, then single code elements
//                         (the tail, and every row of an unaligned database).  An LVQ or
//                         Extended RaBitQ row is an MSB-first B-bit stream: 32 dimensions are B
//                         whole words, read as one unit, byte-swapped, the fields that cross a
//                         word funnel-shifted.
//   pairwise_kernel       exact (row, column) distances of two f32 matrices: pairwise_tile
//                         (pairwise_tile.h, shared with rankaware_search.hip;
//                         128 x 64 per 256-thread workgroup, 8 x 4 scalar chains per thread,
//                         k-slices of 16 staged transposed in LDS, double-buffered, prefetched
//                         into registers one slice ahead).  mivq_pairwise_distances (the coarse
//                         quantizer's exhaustive search, the k-means assignment) and, as
//                         launch_tiled_topk's TileFn, the tiled path of mivq_flat_search.
//   code_pairwise_kernel  the same tile as the TileFn of the code searches: the database side of
//                         a slice is fetched as codes and dequantised before it is stashed
//                         (Extended RaBitQ: against the workgroup's level table in LDS).
//
// The choice between the two paths is flat_use_tiled(nq, n); both produce the same chains.
#include "adc_internal.h"
#include "code_internal.h"
#include "pairwise_tile.h"
#include "topk.h"

namespace mivq {

bool flat_use_tiled(int64_t nq, int64_t n) { return nq >= 16 && n >= 4096; }

namespace {

// The level table of an Extended RaBitQ workgroup: tab[l] = ddiv(levels[l], sqrt(d)), the
// quotient erq_dequantize_kernel forms per element.  The f64 levels arrive in the place of the
// per-dimension parameters the format does not have (`ga`).
template <int B>
__device__ __forceinline__ void erq_stage_table(const float* ga, int d, double* tab, int tid, int nthreads) {
    const double* levels = reinterpret_cast<const double*>(ga);
    const double rd = sqrt((double)d);
    for (int l = tid; l < (1 << B); l += nthreads) tab[l] = __ddiv_rn(levels[l], rd);
}

// grid (nchunks, ceil(nq / QB)), block 1024.  LDS: [QB][dp] queries, then kParams x [dp]
// parameters (Extended RaBitQ: the 2^B f64 levels), dp = d rounded up to 4 (16-B aligned rows;
// the padding is never read).
// `wide` / `narrow`: every row start is aligned for the wide (16 / 8 B) / the 4-B loads.
template <int FMT, int R, int QB>
__global__ __launch_bounds__(kScanWaves * 64) void code_scan_kernel(
    const float* __restrict__ q, int64_t nq, const uint8_t* __restrict__ codes, int64_t n, int d,
    const float* __restrict__ ga, const float* __restrict__ gb, int metric, int k, int64_t id_offset, int64_t chunk_rows,
    int wide, int narrow, float* __restrict__ part_d, uint32_t* __restrict__ part_i) {
    using F = Fmt<FMT>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int dp = (d + 3) & ~3;
    float* qv = smem;             // [QB][dp]
    float* pa = smem + QB * dp;   // SQ den / RaBitQ centroid / LVQ mu
    float* pb = pa + dp;          // SQ lo
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.y * QB;
    const int nqb = (int)min<int64_t>(QB, nq - q0);
    for (int qq = 0; qq < nqb; ++qq)
        for (int t = tid; t < d; t += kScanWaves * 64) qv[qq * dp + t] = q[(q0 + qq) * d + t];
    if constexpr (F::kParams >= 1) {
        for (int t = tid; t < d; t += kScanWaves * 64) {
            pa[t] = ga ? ga[t] : 0.0f;
            if (F::kParams == 2) pb[t] = gb[t];
        }
    }
    if constexpr (F::kIsErq) erq_stage_table<F::kB>(ga, d, reinterpret_cast<double*>(pa), tid, kScanWaves * 64);
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
    const bool l2 = metric == MIVQ_METRIC_L2;
    const int64_t rbeg = (int64_t)blockIdx.x * chunk_rows;
    const int64_t rend = min(n, rbeg + chunk_rows);
    const int64_t stride = F::row_bytes(d);
    const ScanRows rows{qv, pa, pb, nullptr, dp, F::kIsErq ? reinterpret_cast<const double*>(pa) : nullptr};
    for (int64_t base = rbeg + (int64_t)wv * 64; base < rend; base += kScanWaves * 64) {
        const int64_t row = base + lane;
        const bool valid = row < rend;
        float dist[QB];
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) dist[qq] = 0.0f;
        if (valid) scan_row<FMT, QB, false>(codes + row * stride, d, rows, wide, narrow, l2, dist);
        const uint32_t gid = (uint32_t)(id_offset + row);
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            if (qq >= nqb) break;
            float dv = l2 ? dist[qq] : -dist[qq];
            if (dv != dv) dv = INFINITY;
            top[qq].offer(valid, dv, gid, k, lane, thr_d[qq], thr_i[qq]);
        }
    }
    const int64_t part = (int64_t)blockIdx.x * kScanWaves + wv;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        if (qq < nqb) top[qq].store(part_d + (part * nq + q0 + qq) * k, part_i + (part * nq + q0 + qq) * k, k, lane);
    }
}

template <int FMT, int R, int QB>
hipError_t launch_scan(const float* q, int64_t nq, const uint8_t* codes, int64_t n, int d, const float* ga,
                       const float* gb, int metric, int k, int64_t id_offset, int64_t nch, float* pd, uint32_t* pi,
                       hipStream_t st) {
    using F = Fmt<FMT>;
    const size_t smem = (size_t)(QB + F::kParams) * ((d + 3) & ~3) * sizeof(float) + (F::kIsErq ? sizeof(double) << F::kB : 0);
    auto kern = code_scan_kernel<FMT, R, QB>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    const LoadModes lm = code_load_modes<FMT>(codes, d);
    hipLaunchKernelGGL(kern, dim3((unsigned)nch, (unsigned)ceil_div(nq, QB)), dim3(kScanWaves * 64), smem, st, q, nq, codes,
                       n, d, ga, gb, metric, k, id_offset, ceil_div(n, nch), lm.wide, lm.narrow, pd, pi);
    return hipGetLastError();
}

// f32 y: the k-slice fully unrolled (a slice's LDS reads hoisted: ~255 VGPRs, one wave per SIMD).
template <bool IP, bool VEC>
__global__ __launch_bounds__(256) void pairwise_kernel(const float* __restrict__ x, int64_t n,
                                                       const float* __restrict__ y, int64_t m, int d,
                                                       float* __restrict__ out) {
    pairwise_tile<IP, PBK>(x, n, m, d, VEC, out, [&](int t) __attribute__((always_inline)) {
        const int64_t gc = (int64_t)blockIdx.y * PBN + (threadIdx.x >> 2);
        f32x4 py;
        if (VEC) {
            py = (gc < m && t < d) ? *reinterpret_cast<const f32x4*>(y + gc * d + t) : (f32x4){0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) py[j] = (gc < m && t + j < d) ? y[gc * d + t + j] : 0.0f;
        }
        return py;
    });
}

void launch_pairwise(const float* x, int64_t n, const float* y, int64_t m, int d, bool ip, hipStream_t st, float* out) {
    const bool vec = (d % 4) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0;
    const dim3 grid((unsigned)ceil_div(n, PBM), (unsigned)ceil_div(m, PBN));
    if (ip) {
        if (vec) hipLaunchKernelGGL((pairwise_kernel<true, true>), grid, dim3(256), 0, st, x, n, y, m, d, out);
        else hipLaunchKernelGGL((pairwise_kernel<true, false>), grid, dim3(256), 0, st, x, n, y, m, d, out);
    } else {
        if (vec) hipLaunchKernelGGL((pairwise_kernel<false, true>), grid, dim3(256), 0, st, x, n, y, m, d, out);
        else hipLaunchKernelGGL((pairwise_kernel<false, false>), grid, dim3(256), 0, st, x, n, y, m, d, out);
    }
}

// Exact top-k by tiles: pairwise chains for a column chunk, then launch_tiled_topk's
// segmented top-k and running merge.  Same chains and (dist, id) order as the streaming scan.
hipError_t launch_flat_tiled(const float* q, int64_t nq, const float* x, int64_t n, int d, int metric, int k,
                             int64_t id_offset, void* ws, float* dists, uint32_t* ids, hipStream_t st) {
    const bool ip = metric == MIVQ_METRIC_INNER_PRODUCT;
    return launch_tiled_topk(nq, n, k, id_offset, ws, dists, ids, st, [&](int64_t c0, int64_t m, float* buf) {
        launch_pairwise(q, nq, x + c0 * d, m, d, ip, st, buf);
        return hipGetLastError();
    });
}

// The tile against the reconstructions of code rows, dequantised as they are fetched.  `cal`:
// a thread's four dimensions of a row are one aligned load (SQ-8 4 B, SQ-16 8 B, SQ-4 2 B;
// RaBitQ reads the byte holding its four bits either way).  The k-slice by 8, not 16: fully
// unrolled, a slice's LDS reads are hoisted into 256 VGPRs (one wave per SIMD; scratch under a
// two-wave bound); by 8 it is 77-79 VGPRs at the same speed.
template <int FMT, bool IP>
__global__ __launch_bounds__(256, 2) void code_pairwise_kernel(const float* __restrict__ x, int64_t n,
                                                            const uint8_t* __restrict__ codes, int64_t m, int d,
                                                            const float* __restrict__ ga, const float* __restrict__ gb,
                                                            int xvec, int cal, float* __restrict__ out) {
    using F = Fmt<FMT>;
    // this thread's code row of every slice, and its RaBitQ scale
    const int64_t gc = (int64_t)blockIdx.y * PBN + (threadIdx.x >> 2);
    const bool yin = gc < m;
    const uint8_t* cr = codes + (yin ? gc : 0) * (int64_t)F::row_bytes(d);
    const float2 p = yin ? F::row_scale(cr, d) : make_float2(0.0f, 0.0f);
    const double* tab = nullptr;
    if constexpr (F::kIsErq) {
        __shared__ double levels_lds[1 << F::kB];
        erq_stage_table<F::kB>(ga, d, levels_lds, threadIdx.x, 256);
        __syncthreads();
        tab = levels_lds;
    }
    pairwise_tile<IP, 8>(x, n, m, d, xvec, out, [&](int t) __attribute__((always_inline)) {
        f32x4 py = {0.f, 0.f, 0.f, 0.f};
        if (yin && t < d) {
            uint32_t lv[4] = {0u, 0u, 0u, 0u};
            if (F::kIsStream) {
                // t % 4 == 0: the four fields are 4 kB bits from a byte or half-byte boundary on,
                // five bytes at most (those past the code bytes are the trailer's)
                const int o = t * F::kB, fb = o >> 3;
                uint64_t v = 0;
#pragma unroll
                for (int q = 0; q < (4 * F::kB + 4 + 7) / 8; ++q) v |= (uint64_t)cr[fb + q] << (32 - 8 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) lv[j] = (uint32_t)(v >> (40 - (o & 7) - F::kB * (j + 1))) & F::kMask;
            } else if (FMT == kRbq) {
                const uint32_t b = cr[t >> 3] >> (t & 7);  // t % 4 == 0: the four bits share a byte
#pragma unroll
                for (int j = 0; j < 4; ++j) lv[j] = (b >> j) & 1u;
            } else if (cal && t + 4 <= d) {
                if (FMT == kSq8) {
                    const uint32_t w[1] = {*reinterpret_cast<const uint32_t*>(cr + t)};
#pragma unroll
                    for (int j = 0; j < 4; ++j) lv[j] = Fmt<kSq8>::level(w, j);
                } else if (FMT == kSq16) {
                    const uint2 v = *reinterpret_cast<const uint2*>(cr + 2 * t);
                    const uint32_t w[2] = {v.x, v.y};
#pragma unroll
                    for (int j = 0; j < 4; ++j) lv[j] = Fmt<kSq16>::level(w, j);
                } else {
                    const uint32_t w[1] = {*reinterpret_cast<const uint16_t*>(cr + (t >> 1))};
#pragma unroll
                    for (int j = 0; j < 4; ++j) lv[j] = Fmt<kSq4>::level(w, j);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (t + j < d) lv[j] = F::level_at(cr, t + j);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (t + j < d) {
                    const float a = F::kParams >= 1 && ga ? ga[t + j] : 0.0f;
                    const float b = F::kParams == 2 ? gb[t + j] : 0.0f;
                    py[j] = F::dequant(lv[j], a, b, p, tab);
                }
            }
        }
        return py;
    });
}

template <int FMT>
hipError_t launch_code_tiled(const float* q, int64_t nq, const uint8_t* codes, int64_t n, int d, const float* ga,
                             const float* gb, int metric, int k, int64_t id_offset, void* ws, float* dists, uint32_t* ids,
                             hipStream_t st) {
    using F = Fmt<FMT>;
    const int xvec = (d % 4) == 0 && ((uintptr_t)q % 16) == 0;
    const int rb = F::row_bytes(d);
    const int lb = FMT == kSq8 ? 4 : FMT == kSq16 ? 8 : FMT == kSq4 ? 2 : 1;  // bytes of four dimensions (SQ)
    const int cal = (uintptr_t)codes % lb == 0 && rb % lb == 0;
    const bool ip = metric == MIVQ_METRIC_INNER_PRODUCT;
    return launch_tiled_topk(nq, n, k, id_offset, ws, dists, ids, st, [&](int64_t c0, int64_t m, float* buf) {
        const dim3 grid((unsigned)ceil_div(nq, PBM), (unsigned)ceil_div(m, PBN));
        const uint8_t* y = codes + c0 * rb;
        if (ip) hipLaunchKernelGGL((code_pairwise_kernel<FMT, true>), grid, dim3(256), 0, st, q, nq, y, m, d, ga, gb, xvec, cal, buf);
        else hipLaunchKernelGGL((code_pairwise_kernel<FMT, false>), grid, dim3(256), 0, st, q, nq, y, m, d, ga, gb, xvec, cal, buf);
        return hipGetLastError();
    });
}

// ---------------------------------------------------------------- workspace + dispatch
// The workspace of an exact search (nq, n > 0): the tiled path's (laid out by launch_tiled_topk:
// key block + part lists), or the streaming scan's part lists (parts, nq, k) of distances at
// pd and ids at pi.  Never decoded rows.  QB == 0 on the streaming path: d does not fit LDS.
struct SearchLayout {
    bool tiled;
    int QB;
    int64_t nch, parts;
    size_t pd, pi, total;
};

SearchLayout search_layout(int64_t nq, int64_t n, int d, int k, ScanPolicy P) {
    SearchLayout L{};
    L.tiled = flat_use_tiled(nq, n);
    L.QB = scan_qb(d, P);
    if (L.tiled) {
        L.total = flat_tiled_workspace_bytes(nq, n, k);
    } else if (L.QB > 0) {
        // no wider than the batch: a workgroup computes all QB chains of a row, and the scan is
        // bound by the LDS reads of the queries (nq = 1 at QB = 8: 2.5 ms per 1M x 3072 SQ-8)
        while (P.narrow && L.QB > 1 && L.QB / 2 >= nq) L.QB /= 2;
        L.nch = adc_chunks(nq, n, L.QB);
        L.parts = L.nch * kScanWaves;
        const size_t list = align_up((size_t)L.parts * nq * k * 4, 256);
        L.pd = 0;
        L.pi = list;
        L.total = 2 * list;
    }
    return L;
}

size_t search_workspace_bytes(int64_t nq, int64_t n, int d, int k, ScanPolicy P) {
    if (nq <= 0 || n <= 0 || d <= 0 || k <= 0) return 0;
    return search_layout(nq, n, d, k, P).total;
}

// Shared body of the entry points (arguments validated up to the format's own); an f32
// database arrives as its bytes.
template <int FMT>
int exact_flat_search(const char* name, const float* q, int64_t nq, const uint8_t* codes, int64_t n, int d,
                      const float* ga, const float* gb, int metric, int k, int64_t id_offset, void* workspace,
                      size_t workspace_bytes, float* dists, uint32_t* ids, hipStream_t st) {
    using F = Fmt<FMT>;
    const SearchLayout L = search_layout(nq, n, d, k, F::kPolicy);
    MIVQ_REQUIRE(workspace && workspace_bytes >= L.total, MIVQ_ERR_WORKSPACE, "%s: workspace %zu < %zu", name,
                 workspace_bytes, L.total);
    if (L.tiled) {
        hipError_t et;
        if constexpr (FMT == kF32)
            et = launch_flat_tiled(q, nq, reinterpret_cast<const float*>(codes), n, d, metric, k, id_offset, workspace, dists, ids, st);
        else
            et = launch_code_tiled<FMT>(q, nq, codes, n, d, ga, gb, metric, k, id_offset, workspace, dists, ids, st);
        if (et != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (tiled): %s", name, hipGetErrorString(et));
        return MIVQ_OK;
    }
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float* pd = reinterpret_cast<float*>(ws + L.pd);
    uint32_t* pi = reinterpret_cast<uint32_t*>(ws + L.pi);
    hipError_t e = with_topk_regs(k, [&](auto R) {
        return with_query_block(L.QB, [&](auto QB) {
            return launch_scan<FMT, decltype(R)::value, decltype(QB)::value>(q, nq, codes, n, d, ga, gb, metric, k,
                                                                             id_offset, L.nch, pd, pi, st);
        });
    });
    // (mivq_flat_search words its two launch failures its own way)
    if (e != hipSuccess && FMT == kF32) return set_error(MIVQ_ERR_HIP, "flat_scan: %s", hipGetErrorString(e));
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (scan): %s", name, hipGetErrorString(e));
    e = launch_topk_merge(pd, pi, (int)L.parts, nq, k, dists, ids, st);
    if (e != hipSuccess && FMT == kF32) return set_error(MIVQ_ERR_HIP, "topk_merge: %s", hipGetErrorString(e));
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (merge): %s", name, hipGetErrorString(e));
    return MIVQ_OK;
}

// The checks every exact search shares, in mivq_flat_search's order; *done is set when the
// call is complete without a scan (nq == 0, or n == 0: sentinel lists).
int search_prologue(const char* name, int64_t nq, int64_t n, int d, ScanPolicy P, int metric, int k, int64_t id_offset,
                    float* dists, uint32_t* ids, hipStream_t st, bool* done) {
    *done = false;
    MIVQ_REQUIRE(k <= 256, MIVQ_ERR_UNSUPPORTED, "%s: k=%d > 256", name, k);
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED, "%s: metric %d",
                 name, metric);
    MIVQ_REQUIRE(scan_qb(d, P) > 0 || flat_use_tiled(nq, n), MIVQ_ERR_UNSUPPORTED, "%s: d=%d too large for LDS", name, d);
    MIVQ_REQUIRE(id_offset >= 0 && id_offset + n <= (int64_t)kNoId, MIVQ_ERR_INVALID, "%s: ids overflow", name);
    if (nq == 0) {
        *done = true;
        return MIVQ_OK;
    }
    MIVQ_REQUIRE(dists && ids, MIVQ_ERR_INVALID, "%s: null pointer", name);
    if (n == 0) {
        *done = true;
        const hipError_t e = launch_topk_merge(nullptr, nullptr, 0, nq, k, dists, ids, st);
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s(empty): %s", name, hipGetErrorString(e));
    }
    return MIVQ_OK;
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_pairwise_distances(const float* x, int64_t n, const float* y, int64_t m, int32_t d,
                                       int32_t metric, float* out, void* stream) {
    MIVQ_REQUIRE(n >= 0 && m >= 0 && d > 0, MIVQ_ERR_INVALID, "pairwise_distances: bad sizes");
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED,
                 "pairwise_distances: metric %d", metric);
    MIVQ_REQUIRE(ceil_div(m, PBN) <= 65535, MIVQ_ERR_UNSUPPORTED, "pairwise_distances: m=%lld too large",
                 (long long)m);
    if (n == 0 || m == 0) return MIVQ_OK;
    MIVQ_REQUIRE(x && y && out, MIVQ_ERR_INVALID, "pairwise_distances: null pointer");
    launch_pairwise(x, n, y, m, d, metric == MIVQ_METRIC_INNER_PRODUCT, as_stream(stream), out);
    return check_launch("pairwise_distances");
}

extern "C" size_t mivq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k) {
    return search_workspace_bytes(nq, n, d, k, Fmt<kF32>::kPolicy);
}

extern "C" size_t mivq_sq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k) {
    return search_workspace_bytes(nq, n, d, k, Fmt<kSq8>::kPolicy);
}

extern "C" size_t mivq_rabitq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k) {
    return search_workspace_bytes(nq, n, d, k, Fmt<kRbq>::kPolicy);
}

extern "C" size_t mivq_lvq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k) {
    return search_workspace_bytes(nq, n, d, k, Fmt<kLvq>::kPolicy);
}

extern "C" int mivq_flat_search(const float* q, int64_t nq, const float* x, int64_t n, int32_t d, int32_t metric,
                                int32_t k, int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists,
                                uint32_t* ids, void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && d > 0 && k > 0, MIVQ_ERR_INVALID, "flat_search: bad sizes");
    hipStream_t st = as_stream(stream);
    bool done = false;
    const int rc = search_prologue("flat_search", nq, n, d, Fmt<kF32>::kPolicy, metric, k, id_offset, dists, ids, st, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(q && x, MIVQ_ERR_INVALID, "flat_search: null pointer");
    return exact_flat_search<kF32>("flat_search", q, nq, reinterpret_cast<const uint8_t*>(x), n, d, nullptr, nullptr, metric,
                                   k, id_offset, workspace, workspace_bytes, dists, ids, st);
}

extern "C" int mivq_sq_flat_search(const float* q, int64_t nq, const void* codes, int64_t n, int32_t d, const float* lo,
                                   const float* den, int32_t nbits, int32_t metric, int32_t k, int64_t id_offset,
                                   void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids, void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && d > 0 && k > 0, MIVQ_ERR_INVALID, "sq_flat_search: bad sizes");
    MIVQ_REQUIRE(nbits == 4 || nbits == 8 || nbits == 16, MIVQ_ERR_INVALID, "num_bits must be 4, 8, or 16, got %d", nbits);
    hipStream_t st = as_stream(stream);
    bool done = false;
    const int rc = search_prologue("sq_flat_search", nq, n, d, Fmt<kSq8>::kPolicy, metric, k, id_offset, dists, ids, st, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(q && codes && lo && den, MIVQ_ERR_INVALID, "sq_flat_search: null pointer");
    if (const int ra = sq16_aligned("sq_flat_search", nbits, codes)) return ra;
    return with_sq_bits(nbits, [&](auto F) {
        return exact_flat_search<decltype(F)::value>("sq_flat_search", q, nq, static_cast<const uint8_t*>(codes), n, d, den,
                                                     lo, metric, k, id_offset, workspace, workspace_bytes, dists, ids, st);
    });
}

extern "C" int mivq_rabitq_flat_search(const float* q, int64_t nq, const uint8_t* codes, int64_t n, int32_t d,
                                       const float* centroid, int32_t metric, int32_t k, int64_t id_offset, void* workspace,
                                       size_t workspace_bytes, float* dists, uint32_t* ids, void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && d > 0 && k > 0, MIVQ_ERR_INVALID, "rabitq_flat_search: bad sizes");
    hipStream_t st = as_stream(stream);
    bool done = false;
    const int rc = search_prologue("rabitq_flat_search", nq, n, d, Fmt<kRbq>::kPolicy, metric, k, id_offset, dists, ids, st, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(q && codes, MIVQ_ERR_INVALID, "rabitq_flat_search: null pointer");
    return exact_flat_search<kRbq>("rabitq_flat_search", q, nq, codes, n, d, centroid, nullptr, metric, k, id_offset,
                                  workspace, workspace_bytes, dists, ids, st);
}

extern "C" int mivq_lvq_flat_search(const float* q, int64_t nq, const uint8_t* codes, int64_t n, int32_t d, const float* mu,
                                    int32_t nbits, int32_t metric, int32_t k, int64_t id_offset, void* workspace,
                                    size_t workspace_bytes, float* dists, uint32_t* ids, void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && d > 0 && d <= (1 << 27) && k > 0, MIVQ_ERR_INVALID, "lvq_flat_search: bad sizes");
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "num_bits must be in [1, 8], got %d", nbits);
    hipStream_t st = as_stream(stream);
    bool done = false;
    const int rc = search_prologue("lvq_flat_search", nq, n, d, Fmt<kLvq>::kPolicy, metric, k, id_offset, dists, ids, st, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(q && codes && mu, MIVQ_ERR_INVALID, "lvq_flat_search: null pointer");
    return with_lvq_bits(nbits, [&](auto F) {
        return exact_flat_search<decltype(F)::value>("lvq_flat_search", q, nq, codes, n, d, mu, nullptr, metric, k, id_offset,
                                                     workspace, workspace_bytes, dists, ids, st);
    });
}

extern "C" size_t mivq_extrabitq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k) {
    return search_workspace_bytes(nq, n, d, k, Fmt<kErq>::kPolicy);
}

// qy: the queries in the rotated domain ((q - c) P for L2, q P for inner product).  The f64
// levels travel in the parameter slot of the shared kernels (erq_stage_table).
extern "C" int mivq_extrabitq_flat_search(const float* qy, int64_t nq, const uint8_t* codes, int64_t n, int32_t d,
                                          const double* levels, int32_t nbits, int32_t metric, int32_t k,
                                          int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists,
                                          uint32_t* ids, void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && d > 0 && d <= (1 << 27) && k > 0, MIVQ_ERR_INVALID, "extrabitq_flat_search: bad sizes");
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "num_bits must be in [1, 8], got %d", nbits);
    hipStream_t st = as_stream(stream);
    bool done = false;
    const int rc = search_prologue("extrabitq_flat_search", nq, n, d, Fmt<kErq>::kPolicy, metric, k, id_offset, dists, ids, st, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(qy && codes && levels, MIVQ_ERR_INVALID, "extrabitq_flat_search: null pointer");
    const float* lv = reinterpret_cast<const float*>(levels);
    return with_erq_bits(nbits, [&](auto F) {
        return exact_flat_search<decltype(F)::value>("extrabitq_flat_search", qy, nq, codes, n, d, lv, nullptr, metric, k,
                                                     id_offset, workspace, workspace_bytes, dists, ids, st);
    });
}
