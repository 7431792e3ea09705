// rankaware_search.hip — exact search over rank-aware codes in the rotated domain, on gfx950.
//
// x^ = y^ . V^T + mu with V orthogonal, so ||q - x^||^2 = ||(q - mu) V - y^||^2 and
// <q, x^> = <q V, y^> + <q, mu>: the caller rotates the queries (nq x D x D), and the database is
// scanned as it is stored.  y^_t = lv32[lv_off[t] + idx_t], idx_t the width[t] bits at bit pos[t]
// of the row (MSB-first), read exactly as ra_dequantize_kernel (rankaware.hip) reads them; lv32
// is the f64 level table rounded to f32.  The chains and the (dist, id) order are those of
// mivq_flat_search (exact_search.hip), so ids and distances are bit-identical to
// mivq_flat_search(qy, (float)mivq_rankaware_dequantize(codes)), and no decoded row reaches memory.
//
//   ra_scan_kernel      the streaming scan, for few queries: grid (nchunks, ceil(nq / QB)), 256
//                       threads, lane = database row.  A workgroup walks its chunk in tiles of
//                       rows whose codes it holds in LDS with the global layout of a row and an
//                       odd pitch in words (the lanes of a wave read the same byte of 64 rows:
//                       64 banks), staged with coalesced loads.  The level tables do not fit LDS
//                       (256 d floats at most), but the tables of consecutive dimensions are
//                       consecutive in lv32: per slice of kRsSlice dimensions the workgroup
//                       stages that range (16 KiB at most) and one descriptor per dimension
//                       {byte, shift, mask, table start}, both prefetched into registers while
//                       the slice before is scanned, so pos / width / lv_off are read once per
//                       slice and only the row's bytes and the table lookup are per lane, eight
//                       dimensions' in flight together.  QB queries in LDS, sequential fmaf
//                       chains over t, WaveTopK lists merged by launch_topk_merge.
//   ra_pairwise_kernel  the tile of the tiled path (pairwise_tile.h) with the database side of a
//                       slice fetched as fields and looked up before it is stashed: the lookups
//                       of a 64-row x 16-dimension slice serve 128 queries, the tables stay in L1.
//
// A field is at most 8 bits and lies in two bytes at most; the second byte's address is clamped
// to the row's last byte (its bits are shifted out when the field ends in the first), so no row,
// the last one included, is read past its code_size bytes.  Rows start at any byte.
#include "adc_internal.h"
#include "pairwise_tile.h"
#include "topk.h"

#include <algorithm>

namespace mivq {
namespace {

constexpr int kRsThreads = 256;
constexpr int kRsWaves = kRsThreads / 64;
constexpr int kRsSlice = 16;                     // dimensions per staged slice of the tables
constexpr int kRsTabSpan = kRsSlice * 256;       // floats a slice's tables can take
constexpr int kRsTab = kRsTabSpan + 256;         // staged floats: any start <= span plus any 8-bit index
constexpr int kRsPre = (kRsTab + kRsThreads - 1) / kRsThreads;  // table floats a thread prefetches
constexpr int kRsLdsBytes = 144 * 1024;          // per workgroup: queries + table slice + code rows
constexpr int kRsQueryBytes = 32 * 1024;         // queries, 64 KiB at one query
constexpr int kRsMaxCode = 48000;                // as mivq_rankaware_dequantize
constexpr int kRsMaxChunks = 768;                // workgroups per query block (three per CU)

__host__ __device__ inline int rs_pitch_words(int cs) { return ((cs + 3) >> 2) | 1; }

// The field of dimension t as ra_field (rankaware.hip) defines it: a field outside the row or a
// width outside 1..8 is width 0, index 0.  {first byte, right shift of the 16-bit big-endian
// window at that byte, mask}.
struct RsField {
    int byte, sh;
    uint32_t mask;
};
__device__ __forceinline__ RsField rs_field(int w, int p, int cs) {
    const bool ok = w > 0 && w <= 8 && p >= 0 && p <= 8 * cs - w;
    RsField f;
    f.byte = ok ? (p >> 3) : 0;
    f.sh = ok ? 16 - w - (p & 7) : 0;
    f.mask = ok ? (1u << w) - 1u : 0u;
    return f;
}
__device__ __forceinline__ uint32_t rs_index(const uint8_t* row, RsField f, int cs) {
    const uint32_t win = ((uint32_t)row[f.byte] << 8) | (uint32_t)row[min(f.byte + 1, cs - 1)];
    return (win >> f.sh) & f.mask;
}

// 4 NG consecutive dimensions from j on (j % 4 == 0) into the QB chains: the levels first, so that
// their lookups are in flight together, then the queries (q: the first query's dimension j) as
// 16-B LDS reads.
template <int NG, int QB, typename Level>
__device__ __forceinline__ void rs_chain(Level level, int j, const float* q, int dp, bool l2, float (&dist)[QB]) {
    float x[4 * NG];
#pragma unroll
    for (int u = 0; u < 4 * NG; ++u) x[u] = level(j + u);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            const float4 qf = *reinterpret_cast<const float4*>(q + qq * dp + 4 * g);
            if (l2) {
                float df = __fsub_rn(qf.x, x[4 * g]); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                df = __fsub_rn(qf.y, x[4 * g + 1]); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                df = __fsub_rn(qf.z, x[4 * g + 2]); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                df = __fsub_rn(qf.w, x[4 * g + 3]); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
            } else {
                dist[qq] = __builtin_fmaf(qf.x, x[4 * g], dist[qq]);
                dist[qq] = __builtin_fmaf(qf.y, x[4 * g + 1], dist[qq]);
                dist[qq] = __builtin_fmaf(qf.z, x[4 * g + 2], dist[qq]);
                dist[qq] = __builtin_fmaf(qf.w, x[4 * g + 3], dist[qq]);
            }
        }
    }
}

// LDS: [QB][dp] queries (dp = d rounded up to 4), the table slice, the slice's descriptors and
// table starts, then the code rows [rows_per][pitch words].
template <int R, int QB>
__global__ __launch_bounds__(kRsThreads) void ra_scan_kernel(
    const float* __restrict__ q, int64_t nq, const uint8_t* __restrict__ codes, int64_t n, int d,
    const float* __restrict__ lv32, const int32_t* __restrict__ lv_off, const int32_t* __restrict__ pos,
    const int32_t* __restrict__ width, int cs, int metric, int k, int64_t id_offset, int64_t chunk_rows, int rows_per,
    float* __restrict__ part_d, uint32_t* __restrict__ part_i) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int dp = (d + 3) & ~3;
    float* qv = smem;                                               // [QB][dp]
    float* tab = qv + QB * dp;                                      // [kRsTab]
    uint2* dsc = reinterpret_cast<uint2*>(tab + kRsTab);            // [kRsSlice] {byte | sh << 16 | mask << 24, table start}
    uint32_t* img = reinterpret_cast<uint32_t*>(dsc + kRsSlice);    // [rows_per][pw]
    uint8_t* sb = reinterpret_cast<uint8_t*>(img);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int pw = rs_pitch_words(cs);
    const int64_t q0 = (int64_t)blockIdx.y * QB;
    const int nqb = (int)min<int64_t>(QB, nq - q0);
    for (int qq = 0; qq < QB; ++qq)
        for (int t = tid; t < dp; t += kRsThreads) qv[qq * dp + t] = (qq < nqb && t < d) ? q[(q0 + qq) * d + t] : 0.0f;
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
    const uint8_t* row = sb + (size_t)tid * pw * 4;

    // The next slice's tables and this thread's descriptor, loaded into registers while the
    // current slice is scanned (and, for slice 0, while the tile's rows are staged).
    float pre[kRsPre];
    int pre_len = 0, pre_nd = 0, pre_w = 0, pre_p = 0, pre_o = 0;
    auto prefetch = [&](int t0) __attribute__((always_inline)) {
        pre_nd = min(kRsSlice, d - t0);
        const int base = lv_off[t0];
        pre_len = min(max(lv_off[t0 + pre_nd] - base, 0), kRsTab);
#pragma unroll
        for (int u = 0; u < kRsPre; ++u) {
            const int i = tid + kRsThreads * u;
            pre[u] = i < pre_len ? lv32[base + i] : 0.0f;
        }
        if (tid < pre_nd) {
            pre_w = width[t0 + tid];
            pre_p = pos[t0 + tid];
            pre_o = lv_off[t0 + tid] - base;
        }
    };
    auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < kRsPre; ++u) {
            const int i = tid + kRsThreads * u;
            if (i < pre_len) tab[i] = pre[u];
        }
        if (tid < pre_nd) {
            const RsField f = rs_field(pre_w, pre_p, cs);
            dsc[tid] = make_uint2((uint32_t)f.byte | ((uint32_t)f.sh << 16) | (f.mask << 24),
                                  (uint32_t)min(max(pre_o, 0), kRsTabSpan));
        }
    };
    auto level = [&](int j) __attribute__((always_inline)) {
        const uint2 ds = dsc[j];
        RsField f;
        f.byte = (int)(ds.x & 0xFFFFu);
        f.sh = (int)((ds.x >> 16) & 0xFFu);
        f.mask = ds.x >> 24;
        return tab[ds.y + rs_index(row, f, cs)];
    };

    for (int64_t r0 = rbeg; r0 < rend; r0 += rows_per) {
        const int rows = (int)min<int64_t>(rows_per, rend - r0);
        prefetch(0);
        __syncthreads();  // the previous tile is scanned
        // the tile's rows, four loads in flight per thread, 16-B or 4-B by alignment
        const uint8_t* in = codes + r0 * cs;
        const unsigned ucs = (unsigned)cs;
        if ((cs & 15) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0) {
            const uint4* in16 = reinterpret_cast<const uint4*>(in);
            const unsigned cv = ucs >> 4, total = (unsigned)rows * cv;
            for (unsigned v0 = tid; v0 < total; v0 += 4 * kRsThreads) {
                uint4 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (v0 + kRsThreads * u < total) x[u] = in16[v0 + kRsThreads * u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned v = v0 + kRsThreads * u;
                    if (v < total) {
                        const unsigned r = v / cv;
                        uint32_t* o = img + r * pw + 4 * (v - r * cv);
                        o[0] = x[u].x; o[1] = x[u].y; o[2] = x[u].z; o[3] = x[u].w;
                    }
                }
            }
        } else if ((cs & 3) == 0 && (reinterpret_cast<uintptr_t>(in) & 3) == 0) {
            const uint32_t* in32 = reinterpret_cast<const uint32_t*>(in);
            const unsigned cw = ucs >> 2, total = (unsigned)rows * cw;
            for (unsigned v0 = tid; v0 < total; v0 += 4 * kRsThreads) {
                uint32_t x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (v0 + kRsThreads * u < total) x[u] = in32[v0 + kRsThreads * u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned v = v0 + kRsThreads * u;
                    if (v < total) {
                        const unsigned r = v / cw;
                        img[r * pw + (v - r * cw)] = x[u];
                    }
                }
            }
        } else {
            // any row size at any byte: the aligned words inside the tile's bytes as 4-B loads, the
            // up to three bytes before the first and after the last of them one by one
            const unsigned total = (unsigned)rows * ucs;
            const unsigned lead = min((unsigned)(-reinterpret_cast<uintptr_t>(in) & 3), total);
            const unsigned nw = (total - lead) >> 2;
            const uint32_t* in32 = reinterpret_cast<const uint32_t*>(in + lead);
            auto put = [&](unsigned b, uint32_t v) __attribute__((always_inline)) {
                const unsigned r = b / ucs;
                sb[(size_t)r * pw * 4 + (b - r * ucs)] = (uint8_t)v;
            };
            for (unsigned v0 = tid; v0 < nw; v0 += 4 * kRsThreads) {
                uint32_t x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (v0 + kRsThreads * u < nw) x[u] = in32[v0 + kRsThreads * u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned v = v0 + kRsThreads * u;
                    if (v < nw) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) put(lead + 4 * v + e, x[u] >> (8 * e));
                    }
                }
            }
            if ((unsigned)tid < lead) put(tid, in[tid]);
            const unsigned tail = lead + 4 * nw + tid;
            if (tid < 4 && tail < total) put(tail, in[tail]);
        }
        const bool valid = tid < rows;
        float dist[QB];
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) dist[qq] = 0.0f;
        for (int t0 = 0; t0 < d; t0 += kRsSlice) {
            const int nd = min(kRsSlice, d - t0);
            __syncthreads();  // the previous slice is consumed (first trip: the rows are staged)
            commit();
            __syncthreads();
            if (t0 + kRsSlice < d) prefetch(t0 + kRsSlice);
            if (valid) {
                int j = 0;
                for (; j + 8 <= nd; j += 8) rs_chain<2, QB>(level, j, qv + t0 + j, dp, l2, dist);
                for (; j + 4 <= nd; j += 4) rs_chain<1, QB>(level, j, qv + t0 + j, dp, l2, dist);
                for (; j < nd; ++j) {
                    const float xh = level(j);
#pragma unroll
                    for (int qq = 0; qq < QB; ++qq) {
                        const float qt = qv[qq * dp + t0 + j];
                        if (l2) {
                            const float df = __fsub_rn(qt, xh);
                            dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                        } else {
                            dist[qq] = __builtin_fmaf(qt, xh, dist[qq]);
                        }
                    }
                }
            }
        }
        const uint32_t gid = (uint32_t)(id_offset + r0 + tid);
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            if (qq >= nqb) break;
            float dv = l2 ? dist[qq] : -dist[qq];
            if (dv != dv) dv = INFINITY;
            top[qq].offer(valid, dv, gid, k, lane, thr_d[qq], thr_i[qq]);
        }
    }
    const int64_t part = (int64_t)blockIdx.x * kRsWaves + wv;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        if (qq < nqb) top[qq].store(part_d + (part * nq + q0 + qq) * k, part_i + (part * nq + q0 + qq) * k, k, lane);
    }
}

// The k-slice by 8 as code_pairwise_kernel (exact_search.hip) has it.
template <bool IP>
__global__ __launch_bounds__(256, 2) void ra_pairwise_kernel(const float* __restrict__ x, int64_t n,
                                                             const uint8_t* __restrict__ codes, int64_t m, int d,
                                                             const float* __restrict__ lv32,
                                                             const int32_t* __restrict__ lv_off,
                                                             const int32_t* __restrict__ pos,
                                                             const int32_t* __restrict__ width, int cs, int xvec,
                                                             float* __restrict__ out) {
    const int64_t gc = (int64_t)blockIdx.y * PBN + (threadIdx.x >> 2);
    const bool yin = gc < m;
    const uint8_t* cr = codes + (yin ? gc : 0) * (int64_t)cs;
    pairwise_tile<IP, 8>(x, n, m, d, xvec, out, [&](int t) __attribute__((always_inline)) {
        f32x4 py = {0.f, 0.f, 0.f, 0.f};
        if (yin && t < d) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (t + j < d) {
                    const RsField f = rs_field(width[t + j], pos[t + j], cs);
                    py[j] = lv32[lv_off[t + j] + (int)rs_index(cr, f, cs)];
                }
            }
        }
        return py;
    });
}

// Where a search runs and what it needs (nq, n, d, cs, k > 0).  Tiled: launch_tiled_topk's
// workspace.  Scan: QB queries per workgroup (0: d does not fit the LDS), `rows` code rows per
// tile, nch row chunks, the part lists (parts, nq, k) of distances at pd and ids at pi.
struct RsLayout {
    bool tiled;
    int QB, rows;
    int64_t nch, parts;
    size_t lds, pd, pi, total;
};

RsLayout rs_layout(int64_t nq, int64_t n, int d, int cs, int k) {
    RsLayout L{};
    L.tiled = flat_use_tiled(nq, n);
    if (L.tiled) {
        L.total = flat_tiled_workspace_bytes(nq, n, k);
        return L;
    }
    const int64_t per = (int64_t)((d + 3) & ~3) * 4;
    L.QB = per * 8 <= kRsQueryBytes ? 8 : per * 4 <= kRsQueryBytes ? 4 : per * 2 <= kRsQueryBytes ? 2
           : per <= 2 * kRsQueryBytes ? 1 : 0;
    if (L.QB == 0 || cs > kRsMaxCode) return L;
    while (L.QB > 1 && L.QB / 2 >= nq) L.QB /= 2;  // no wider than the batch
    const int64_t fixed = L.QB * per + (int64_t)(kRsTab + 2 * kRsSlice) * 4;
    const int64_t pitch = (int64_t)rs_pitch_words(cs) * 4;
    L.rows = (int)std::min<int64_t>(kRsThreads, (kRsLdsBytes - fixed) / pitch);
    L.lds = (size_t)(fixed + L.rows * pitch);
    const int64_t qblocks = ceil_div(nq, L.QB);
    L.nch = std::min<int64_t>(ceil_div(n, L.rows), std::max<int64_t>(1, kRsMaxChunks / qblocks));
    L.parts = L.nch * kRsWaves;
    const size_t list = align_up((size_t)L.parts * nq * k * 4, 256);
    L.pd = 0;
    L.pi = list;
    L.total = 2 * list;
    return L;
}

template <int R, int QB>
hipError_t launch_ra_scan(const RsLayout& L, const float* q, int64_t nq, const uint8_t* codes, int64_t n, int d,
                          const float* lv32, const int32_t* lv_off, const int32_t* pos, const int32_t* width, int cs,
                          int metric, int k, int64_t id_offset, float* pd, uint32_t* pi, hipStream_t st) {
    auto kern = ra_scan_kernel<R, QB>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)L.nch, (unsigned)ceil_div(nq, QB)), dim3(kRsThreads), L.lds, st, q, nq, codes, n,
                       d, lv32, lv_off, pos, width, cs, metric, k, id_offset, ceil_div(n, L.nch), L.rows, pd, pi);
    return hipGetLastError();
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" size_t mivq_rankaware_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t code_size,
                                                             int32_t k) {
    if (nq <= 0 || n <= 0 || d <= 0 || code_size <= 0 || k <= 0) return 0;
    return rs_layout(nq, n, d, code_size, k).total;
}

extern "C" int mivq_rankaware_flat_search(const float* qy, int64_t nq, const uint8_t* codes, int64_t n, int32_t d,
                                          const float* lv32, const int32_t* lv_off, const int32_t* pos,
                                          const int32_t* width, int32_t code_size, int32_t metric, int32_t k,
                                          int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists,
                                          uint32_t* ids, void* stream) {
    const char* name = "rankaware_flat_search";
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && d > 0 && code_size > 0 && k > 0, MIVQ_ERR_INVALID,
                 "%s: bad sizes nq=%lld n=%lld d=%d code_size=%d k=%d", name, (long long)nq, (long long)n, d, code_size, k);
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_INVALID, "%s: metric %d", name,
                 metric);
    MIVQ_REQUIRE(k <= 256, MIVQ_ERR_UNSUPPORTED, "%s: k=%d > 256", name, k);
    MIVQ_REQUIRE(id_offset >= 0 && id_offset + n <= (int64_t)kNoId, MIVQ_ERR_INVALID, "%s: ids overflow", name);
    if (nq == 0) return MIVQ_OK;
    MIVQ_REQUIRE(dists && ids, MIVQ_ERR_INVALID, "%s: null pointer", name);
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        const hipError_t e = launch_topk_merge(nullptr, nullptr, 0, nq, k, dists, ids, st);
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s(empty): %s", name, hipGetErrorString(e));
        return MIVQ_OK;
    }
    MIVQ_REQUIRE(qy && codes && lv32 && lv_off && pos && width, MIVQ_ERR_INVALID, "%s: null pointer", name);
    MIVQ_REQUIRE(d < (1 << 28), MIVQ_ERR_UNSUPPORTED, "%s: d=%d too large", name, d);
    MIVQ_REQUIRE(code_size <= kRsMaxCode, MIVQ_ERR_UNSUPPORTED, "%s: code_size %d exceeds %d bytes", name, code_size,
                 kRsMaxCode);
    const RsLayout L = rs_layout(nq, n, d, code_size, k);
    if (!L.tiled) {
        MIVQ_REQUIRE(L.QB > 0, MIVQ_ERR_UNSUPPORTED, "%s: d=%d too large for LDS", name, d);
        MIVQ_REQUIRE(ceil_div(nq, L.QB) <= 65535, MIVQ_ERR_UNSUPPORTED, "%s: nq=%lld too large for n=%lld", name,
                     (long long)nq, (long long)n);
    }
    MIVQ_REQUIRE(workspace && workspace_bytes >= L.total, MIVQ_ERR_WORKSPACE, "%s: workspace %zu < %zu", name,
                 workspace_bytes, L.total);
    if (L.tiled) {
        const int xvec = (d % 4) == 0 && ((uintptr_t)qy % 16) == 0;
        const bool ip = metric == MIVQ_METRIC_INNER_PRODUCT;
        const hipError_t e =
            launch_tiled_topk(nq, n, k, id_offset, workspace, dists, ids, st, [&](int64_t c0, int64_t m, float* buf) {
                const dim3 grid((unsigned)ceil_div(nq, PBM), (unsigned)ceil_div(m, PBN));
                const uint8_t* y = codes + c0 * code_size;
                if (ip)
                    hipLaunchKernelGGL((ra_pairwise_kernel<true>), grid, dim3(256), 0, st, qy, nq, y, m, d, lv32, lv_off, pos,
                                       width, code_size, xvec, buf);
                else
                    hipLaunchKernelGGL((ra_pairwise_kernel<false>), grid, dim3(256), 0, st, qy, nq, y, m, d, lv32, lv_off, pos,
                                       width, code_size, xvec, buf);
                return hipGetLastError();
            });
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (tiled): %s", name, hipGetErrorString(e));
        return MIVQ_OK;
    }
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float* pd = reinterpret_cast<float*>(ws + L.pd);
    uint32_t* pi = reinterpret_cast<uint32_t*>(ws + L.pi);
    hipError_t e = with_topk_regs(k, [&](auto R) {
        return with_query_block(L.QB, [&](auto QB) {
            return launch_ra_scan<decltype(R)::value, decltype(QB)::value>(L, qy, nq, codes, n, d, lv32, lv_off, pos, width,
                                                                           code_size, metric, k, id_offset, pd, pi, st);
        });
    });
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (scan): %s", name, hipGetErrorString(e));
    e = launch_topk_merge(pd, pi, (int)L.parts, nq, k, dists, ids, st);
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (merge): %s", name, hipGetErrorString(e));
    return MIVQ_OK;
}
