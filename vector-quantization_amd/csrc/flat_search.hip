// flat_search.hip — exact brute-force search over an f32 database on gfx950.
#include "adc_internal.h"
#include "topk.h"

namespace mivq {
namespace {

// Exact brute force over an f32 database: grid (nchunks, ceil(nq / QB)), block 256.  The QB
// query vectors live in LDS; lane = database row, distances are sequential fmaf chains over t
// (16-B loads of the row), ranked with the same wave-resident top-k as adc_scan_kernel.
template <int R, int QB>
__global__ __launch_bounds__(kScanWaves * 64) void flat_scan_kernel(
    const float* __restrict__ q, int64_t nq, const float* __restrict__ x, int64_t n, int d, int metric, int k,
    int64_t id_offset, int64_t chunk_rows, float* __restrict__ part_d, uint32_t* __restrict__ part_i) {
    extern __shared__ __attribute__((aligned(16))) float qv[];  // [QB][d]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.y * QB;
    const int nqb = (int)min<int64_t>(QB, nq - q0);
    for (int64_t e = tid; e < (int64_t)nqb * d; e += kScanWaves * 64) qv[e] = q[q0 * d + e];
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
    const int64_t rbeg = (int64_t)blockIdx.x * chunk_rows;
    const int64_t rend = min(n, rbeg + chunk_rows);
    const bool vec = (d % 4) == 0;
    for (int64_t base = rbeg + (int64_t)wv * 64; base < rend; base += kScanWaves * 64) {
        const int64_t row = base + lane;
        const bool valid = row < rend;
        float dist[QB];
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) dist[qq] = 0.0f;
        if (valid) {
            const float* xr = x + row * d;
            if (vec) {
                for (int t = 0; t < d; t += 4) {
                    const float4 xv = *reinterpret_cast<const float4*>(xr + t);
#pragma unroll
                    for (int qq = 0; qq < QB; ++qq) {
                        const float4 qf = *reinterpret_cast<const float4*>(qv + qq * d + t);
                        if (metric == MIVQ_METRIC_L2) {
                            float df = __fsub_rn(qf.x, xv.x); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                            df = __fsub_rn(qf.y, xv.y); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                            df = __fsub_rn(qf.z, xv.z); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                            df = __fsub_rn(qf.w, xv.w); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                        } else {
                            dist[qq] = __builtin_fmaf(qf.x, xv.x, dist[qq]);
                            dist[qq] = __builtin_fmaf(qf.y, xv.y, dist[qq]);
                            dist[qq] = __builtin_fmaf(qf.z, xv.z, dist[qq]);
                            dist[qq] = __builtin_fmaf(qf.w, xv.w, dist[qq]);
                        }
                    }
                }
            } else {
                for (int t = 0; t < d; ++t) {
                    const float xs = xr[t];
#pragma unroll
                    for (int qq = 0; qq < QB; ++qq) {
                        if (metric == MIVQ_METRIC_L2) {
                            const float df = __fsub_rn(qv[qq * d + t], xs);
                            dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                        } else {
                            dist[qq] = __builtin_fmaf(qv[qq * d + t], xs, dist[qq]);
                        }
                    }
                }
            }
        }
        const uint32_t gid = (uint32_t)(id_offset + row);
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            if (qq >= nqb) break;
            float dv = metric == MIVQ_METRIC_L2 ? dist[qq] : -dist[qq];
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

int flat_qb(int d) {
    const int64_t per = (int64_t)d * 4;
    if (per * 8 <= 96 * 1024) return 8;
    if (per * 4 <= 96 * 1024) return 4;
    if (per * 2 <= 96 * 1024) return 2;
    if (per <= 160 * 1024) return 1;
    return 0;
}

template <int R, int QB>
hipError_t launch_flat(const float* q, int64_t nq, const float* x, int64_t n, int d, int metric, int k,
                       int64_t id_offset, int64_t nch, float* pd, uint32_t* pi, hipStream_t st) {
    const size_t smem = (size_t)QB * d * sizeof(float);
    auto kern = flat_scan_kernel<R, QB>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)nch, (unsigned)ceil_div(nq, QB)), dim3(kScanWaves * 64), smem, st, q, nq, x, n, d,
                       metric, k, id_offset, ceil_div(n, nch), pd, pi);
    return hipGetLastError();
}

}  // namespace

// The tiled path (pairwise chains on packed VALU + segmented top-k) wins once there are
// enough queries to fill a 128-row tile; the streaming scan keeps the small-batch cases.
// (Shared with code_search.hip, declared in topk.h.)
bool flat_use_tiled(int64_t nq, int64_t n) { return nq >= 16 && n >= 4096; }

namespace {

// The workspace of mivq_flat_search (nq, n > 0): the tiled path's (laid out by
// launch_tiled_topk), or the streaming scan's part lists (parts, nq, k) of distances at pd and
// ids at pi.  QB == 0 on the streaming path: d does not fit LDS, no search.
struct FlatSearchLayout {
    bool tiled;
    int QB;
    int64_t nch, parts;
    size_t pd, pi, total;
};

FlatSearchLayout flat_search_layout(int64_t nq, int64_t n, int d, int k) {
    FlatSearchLayout L{};
    L.tiled = flat_use_tiled(nq, n);
    L.QB = flat_qb(d);
    if (L.tiled) {
        L.total = flat_tiled_workspace_bytes(nq, n, k);
    } else if (L.QB > 0) {
        L.nch = adc_chunks(nq, n, L.QB);
        L.parts = L.nch * kScanWaves;
        const size_t list = align_up((size_t)L.parts * nq * k * 4, 256);
        L.pd = 0;
        L.pi = list;
        L.total = 2 * list;
    }
    return L;
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" size_t mivq_flat_search_workspace_bytes(int64_t nq, int64_t n, int32_t d, int32_t k) {
    if (nq <= 0 || n <= 0 || d <= 0 || k <= 0) return 0;
    return flat_search_layout(nq, n, d, k).total;
}

extern "C" int mivq_flat_search(const float* q, int64_t nq, const float* x, int64_t n, int32_t d, int32_t metric,
                                int32_t k, int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists,
                                uint32_t* ids, void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && d > 0 && k > 0, MIVQ_ERR_INVALID, "flat_search: bad sizes");
    MIVQ_REQUIRE(k <= 256, MIVQ_ERR_UNSUPPORTED, "flat_search: k=%d > 256", k);
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED,
                 "flat_search: metric %d", metric);
    MIVQ_REQUIRE(flat_qb(d) > 0 || flat_use_tiled(nq, n), MIVQ_ERR_UNSUPPORTED, "flat_search: d=%d too large for LDS", d);
    MIVQ_REQUIRE(id_offset >= 0 && id_offset + n <= (int64_t)kNoId, MIVQ_ERR_INVALID, "flat_search: ids overflow");
    if (nq == 0) return MIVQ_OK;
    hipStream_t st = as_stream(stream);
    MIVQ_REQUIRE(dists && ids, MIVQ_ERR_INVALID, "flat_search: null pointer");
    if (n == 0) {
        const hipError_t e = launch_topk_merge(nullptr, nullptr, 0, nq, k, dists, ids, st);
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "flat_search(empty): %s", hipGetErrorString(e));
        return MIVQ_OK;
    }
    MIVQ_REQUIRE(q && x, MIVQ_ERR_INVALID, "flat_search: null pointer");
    const FlatSearchLayout L = flat_search_layout(nq, n, d, k);
    MIVQ_REQUIRE(workspace && workspace_bytes >= L.total, MIVQ_ERR_WORKSPACE, "flat_search: workspace %zu < %zu",
                 workspace_bytes, L.total);
    if (L.tiled) {
        const hipError_t et = launch_flat_tiled(q, nq, x, n, d, metric, k, id_offset, workspace, dists, ids, st);
        if (et != hipSuccess) return set_error(MIVQ_ERR_HIP, "flat_search (tiled): %s", hipGetErrorString(et));
        return MIVQ_OK;
    }
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float* pd = reinterpret_cast<float*>(ws + L.pd);
    uint32_t* pi = reinterpret_cast<uint32_t*>(ws + L.pi);
    hipError_t e = with_topk_regs(k, [&](auto R) {
        return with_query_block(L.QB, [&](auto QB) {
            return launch_flat<decltype(R)::value, decltype(QB)::value>(q, nq, x, n, d, metric, k, id_offset, L.nch, pd,
                                                                        pi, st);
        });
    });
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "flat_scan: %s", hipGetErrorString(e));
    e = launch_topk_merge(pd, pi, (int)L.parts, nq, k, dists, ids, st);
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "topk_merge: %s", hipGetErrorString(e));
    return MIVQ_OK;
}
