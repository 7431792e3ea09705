// topk.hip — the launchers of topk.h: list merge, segmented top-k and the tiled top-k.
#include "topk.h"

namespace mivq {
namespace {

// One wave per query: the parts*k candidates (lists laid out (parts, nq, k)) stream through
// a wave-resident top-k, 64 at a time, screened against the cached k-th element.
template <int R>
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ in_d, const uint32_t* __restrict__ in_i,
                                                         int parts, int64_t nq, int k, float* __restrict__ out_d,
                                                         uint32_t* __restrict__ out_i, const int* __restrict__ qlist,
                                                         const int* __restrict__ qcount) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;  // whole wave
    if (qlist != nullptr && qi >= *qcount) return;
    const int64_t qo = qlist != nullptr ? (int64_t)qlist[qi] : qi;  // output row of list slot qi
    WaveTopK<R> top;
    top.init();
    float thr_d = INFINITY;
    uint32_t thr_i = kNoId;
    const int64_t total = (int64_t)parts * k;
    for (int64_t e0 = 0; e0 < total; e0 += 64) {
        const int64_t e = e0 + lane;
        const bool valid = e < total;
        float cd = INFINITY;
        uint32_t ci = kNoId;
        if (valid) {
            const int64_t p = e / k, j = e - p * k;
            cd = in_d[(p * nq + qi) * k + j];
            ci = in_i[(p * nq + qi) * k + j];
            if (cd != cd) cd = INFINITY;
        }
        top.offer(valid, cd, ci, k, lane, thr_d, thr_i);
    }
    // (written out: through WaveTopK::store the address arithmetic comes out four instructions longer)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = r * 64 + lane;
        if (e < k) { out_d[qo * k + e] = top.d[r]; out_i[qo * k + e] = top.id[r]; }
    }
}

// Segmented row top-k for the tiled exact search: the (rows, S*L) block is read as rows*S
// segments of L columns; segment (row, s) writes its k best (value, base + s*L + col) to part
// part0 + s of the (parts, rows, k) list layout that topk_merge_kernel consumes.
template <int R>
__global__ __launch_bounds__(256) void topk_seg_kernel(const float* __restrict__ dist, int64_t rows, int64_t ld,
                                                       int64_t ncols, int L, int S, int k, int64_t base,
                                                       int part0, float* __restrict__ part_d,
                                                       uint32_t* __restrict__ part_i) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= rows * S) return;
    const int64_t row = g / S;
    const int s = (int)(g - row * S);
    const int64_t c0 = (int64_t)s * L;
    const int64_t c1 = min<int64_t>(ncols, c0 + L);
    const float* dr = dist + row * ld;
    WaveTopK<R> top;
    top.init();
    float thr_d = INFINITY;
    uint32_t thr_i = kNoId;
    // 256 columns per step, four coalesced dword loads per lane, the next step's in flight while
    // this one is screened; a step none of whose values beats the current k-th element costs one
    // ballot (round 6: the loop was one dependent 4-B load per 64 columns).  The list is exact
    // in (dist, id), so the order the candidates are offered in does not change it.
    float v[4], vn[4];
    auto ldv = [&](int64_t j0, float (&dst)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t j = j0 + 64 * t + lane;
            dst[t] = j < c1 ? dr[j] : INFINITY;
        }
    };
    ldv(c0, v);
    for (int64_t j0 = c0; j0 < c1; j0 += 256) {
        ldv(j0 + 256, vn);
        bool any = false;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t j = j0 + 64 * t + lane;
            if (v[t] != v[t]) v[t] = INFINITY;
            any = any || (j < c1 && pair_less(v[t], (uint32_t)(base + j), thr_d, thr_i));
        }
        if (__ballot(any) != 0ull) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int64_t j = j0 + 64 * t + lane;
                top.offer(j < c1, v[t], (uint32_t)(base + j), k, lane, thr_d, thr_i);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = vn[t];
    }
    // (written out like topk_merge_kernel's: the flat search leg measured 0.3 % slower through store())
    float* od = part_d + ((int64_t)(part0 + s) * rows + row) * k;
    uint32_t* oi = part_i + ((int64_t)(part0 + s) * rows + row) * k;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = r * 64 + lane;
        if (e < k) { od[e] = top.d[r]; oi[e] = top.id[r]; }
    }
}

// columns per segment (round 6: 16384 measured 3 % faster on the 1000 x 1M estimator search,
// 1024 30 % slower, profiles/r06_s6; 4096 kept: flat_tiled_cols never goes below one segment,
// so a longer segment would also raise the distance buffer's floor to nq x kSegL floats)
constexpr int kSegL = 4096;

int64_t flat_tiled_cols(int64_t nq, int64_t n) {
    int64_t bc = ((int64_t)1 << 26) / std::max<int64_t>(nq, 1);  // <= 256 MiB of distances per chunk
    bc = std::max<int64_t>(kSegL, bc / kSegL * kSegL);
    return std::min<int64_t>(bc, ceil_div(n, kSegL) * kSegL);
}

template <int R>
hipError_t launch_topk_seg(const float* dist, int64_t rows, int64_t ld, int64_t ncols, int S, int k, int64_t base,
                           int part0, float* pd, uint32_t* pi, hipStream_t st) {
    hipLaunchKernelGGL(topk_seg_kernel<R>, dim3((unsigned)ceil_div(rows * S, 4)), dim3(256), 0, st, dist, rows, ld,
                       ncols, kSegL, S, k, base, part0, pd, pi);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_topk_merge(const float* pd, const uint32_t* pi, int parts, int64_t nq, int k, float* od, uint32_t* oi,
                        hipStream_t st, const int* qlist, const int* qcount) {
    const dim3 grid((unsigned)ceil_div(nq, 4)), block(256);
    with_topk_regs(k, [&](auto R) {
        hipLaunchKernelGGL(topk_merge_kernel<decltype(R)::value>, grid, block, 0, st, pd, pi, parts, nq, k, od, oi, qlist,
                           qcount);
    });
    return hipGetLastError();
}

int64_t tiled_topk_cols(int64_t nq, int64_t n) { return flat_tiled_cols(nq, n); }

size_t flat_tiled_workspace_bytes(int64_t nq, int64_t n, int k) {
    const int64_t bc = flat_tiled_cols(nq, n);
    const int64_t S = bc / kSegL;
    return align_up((size_t)nq * bc * 4, 256) + 2 * align_up((size_t)(S + 1) * nq * k * 4, 256) +
           2 * align_up((size_t)nq * k * 4, 256);
}

// Top-k by tiles: `tile(c0, m, buf)` writes the (nq, m) key block of columns [c0, c0 + m)
// (row stride m) into buf; a segmented top-k and a running merge (part 0 = the result so
// far) follow each block.  Keys rank ascending, ties by the smaller id.
hipError_t launch_tiled_topk(int64_t nq, int64_t n, int k, int64_t id_offset, void* ws, float* dists,
                             uint32_t* ids, hipStream_t st, const TileFn& tile) {
    const int64_t bc = flat_tiled_cols(nq, n);
    const int S = (int)(bc / kSegL);
    unsigned char* p = static_cast<unsigned char*>(ws);
    float* buf = reinterpret_cast<float*>(p);
    p += align_up((size_t)nq * bc * 4, 256);
    float* pd = reinterpret_cast<float*>(p);
    p += align_up((size_t)(S + 1) * nq * k * 4, 256);
    uint32_t* pi = reinterpret_cast<uint32_t*>(p);
    p += align_up((size_t)(S + 1) * nq * k * 4, 256);
    float* rd = reinterpret_cast<float*>(p);
    p += align_up((size_t)nq * k * 4, 256);
    uint32_t* ri = reinterpret_cast<uint32_t*>(p);
    hipError_t e = hipSuccess;
    int nparts = 0;  // parts holding data in pd/pi (part 0 = running result once set)
    for (int64_t c0 = 0; c0 < n; c0 += bc) {
        const int64_t m = std::min<int64_t>(bc, n - c0);
        e = tile(c0, m, buf);
        if (e != hipSuccess) return e;
        const int Sc = (int)ceil_div(m, kSegL);
        const int part0 = nparts == 0 ? 0 : 1;
        e = with_topk_regs(k, [&](auto R) {
            return launch_topk_seg<decltype(R)::value>(buf, nq, m, m, Sc, k, id_offset + c0, part0, pd, pi, st);
        });
        if (e != hipSuccess) return e;
        nparts = part0 + Sc;
        const bool last = c0 + bc >= n;
        e = launch_topk_merge(pd, pi, nparts, nq, k, last ? dists : rd, last ? ids : ri, st);
        if (e != hipSuccess) return e;
        if (!last) {  // the merged list becomes part 0
            e = hipMemcpyAsync(pd, rd, (size_t)nq * k * 4, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(pi, ri, (size_t)nq * k * 4, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return e;
            nparts = 1;
        }
    }
    return e;
}

}  // namespace mivq

using namespace mivq;

extern "C" int mivq_topk_merge(const float* dists_in, const uint32_t* ids_in, int32_t parts, int64_t nq, int32_t k,
                               float* dists_out, uint32_t* ids_out, void* stream) {
    MIVQ_REQUIRE(parts >= 0 && nq >= 0 && k > 0, MIVQ_ERR_INVALID, "topk_merge: bad sizes");
    if (nq == 0) return MIVQ_OK;
    MIVQ_REQUIRE((parts == 0 || (dists_in && ids_in)) && dists_out && ids_out, MIVQ_ERR_INVALID,
                 "topk_merge: null pointer");
    MIVQ_REQUIRE(k <= 256, MIVQ_ERR_UNSUPPORTED, "topk_merge: k=%d > 256", k);
    const hipError_t e = launch_topk_merge(dists_in, ids_in, parts, nq, k, dists_out, ids_out, as_stream(stream));
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "topk_merge: %s", hipGetErrorString(e));
    return MIVQ_OK;
}
