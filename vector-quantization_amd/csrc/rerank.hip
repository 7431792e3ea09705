// rerank.hip — exact distances of every query to its own list of candidate rows, over an f32
// database or SQ-4/8/16 / LVQ-1..8 codes (mivq_rerank_f32, mivq_rerank_sq, mivq_rerank_lvq): the
// second stage of a two-stage search.  A first stage names cand[a][0 .. r) global ids per
// query; the result is what mivq_*_flat_search reports, restricted to those rows.
//
// No new arithmetic: a row's floats are fetched and dequantised by Fmt<> and its chain is
// scan_row<FMT, 1, false> (code_internal.h), the body of the streaming scan of exact_search.hip,
// so a distance is bit-identical to the flat search's for the same (query, row).  No decoded row
// and no (nq, r, d) block exists at any point; the workspace holds partial top-k lists.
//
//   rerank_kernel   grid (nq, S slices of the candidate list), block 256.  The query and the
//                   format's parameter rows (SQ: den, lo; LVQ: mu; f32: none) are staged in LDS
//                   once; lanes stride over the slice's slots, a lane owns one gathered row (the
//                   chain is sequential over t); slots outside [id_offset, id_offset + n) are
//                   skipped.  Every wave keeps a WaveTopK list and writes it as one part;
//                   launch_topk_merge merges the 4 S parts of a query.
#include "code_internal.h"
#include "rerank_internal.h"
#include "topk.h"

#include <algorithm>

namespace mivq {
namespace {

// LDS: [dp] query, then kParams x [dp] parameters, dp = d rounded up to 4.  `off`: id_offset;
// a slot is live when off <= id < off + n as unsigned numbers (off + n <= 0xFFFFFFFF, so the
// padding id is never live).  `wide` / `narrow`: every row start is aligned for the wide
// (16 / 8 B) / the 4-B loads.
template <int FMT, int R>
__global__ __launch_bounds__(kRerankWaves * 64) void rerank_kernel(
    const float* __restrict__ q, const uint32_t* __restrict__ cand, int64_t r, const uint8_t* __restrict__ codes,
    int64_t n, int d, const float* __restrict__ ga, const float* __restrict__ gb, int metric, int k, uint32_t off,
    int64_t slice_slots, int wide, int narrow, float* __restrict__ part_d, uint32_t* __restrict__ part_i) {
    using F = Fmt<FMT>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int dp = (d + 3) & ~3;
    float* qv = smem;
    float* pa = smem + dp;
    float* pb = pa + dp;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t qi = blockIdx.x, nq = gridDim.x;
    for (int t = tid; t < d; t += kRerankWaves * 64) {
        qv[t] = q[qi * d + t];
        if constexpr (F::kParams >= 1) pa[t] = ga[t];
        if constexpr (F::kParams == 2) pb[t] = gb[t];
    }
    __syncthreads();
    WaveTopK<R> top;
    top.init();
    float thr_d = INFINITY;
    uint32_t thr_i = kNoId;
    const bool l2 = metric == MIVQ_METRIC_L2;
    const int64_t stride = F::row_bytes(d);
    const ScanRows rows{qv, pa, pb, nullptr, dp, nullptr};
    const uint32_t* cq = cand + qi * r;
    const int64_t sbeg = (int64_t)blockIdx.y * slice_slots;
    const int64_t send = min(r, sbeg + slice_slots);
    for (int64_t base = sbeg + (int64_t)wv * 64; base < send; base += kRerankWaves * 64) {
        const int64_t slot = base + lane;
        const uint32_t id = slot < send ? cq[slot] : kNoId;
        const uint32_t row = id - off;  // wraps for id < off: then row >= 2^32 - off > n
        const bool valid = slot < send && id >= off && (int64_t)row < n;
        float dist[1] = {0.0f};
        if (valid) scan_row<FMT, 1, false>(codes + (int64_t)row * stride, d, rows, wide, narrow, l2, dist);
        float dv = l2 ? dist[0] : -dist[0];
        if (dv != dv) dv = INFINITY;
        top.offer(valid, dv, id, k, lane, thr_d, thr_i);
    }
    const int64_t part = (int64_t)blockIdx.y * kRerankWaves + wv;
    top.store(part_d + (part * nq + qi) * k, part_i + (part * nq + qi) * k, k, lane);
}

template <int FMT, int R>
hipError_t launch_rerank(const float* q, int64_t nq, const uint32_t* cand, int64_t r, const uint8_t* codes, int64_t n,
                         int d, const float* ga, const float* gb, int metric, int k, int64_t id_offset,
                         const RerankLayout& L, float* pd, uint32_t* pi, hipStream_t st) {
    using F = Fmt<FMT>;
    const size_t smem = (size_t)(1 + F::kParams) * ((d + 3) & ~3) * sizeof(float);
    auto kern = rerank_kernel<FMT, R>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    const LoadModes lm = code_load_modes<FMT>(codes, d);
    // whole waves per slice, so that no wave straddles two slices
    const int64_t slice_slots = ceil_div(ceil_div(r, L.S), 64) * 64;
    hipLaunchKernelGGL(kern, dim3((unsigned)nq, (unsigned)L.S), dim3(kRerankWaves * 64), smem, st, q, cand, r, codes, n, d,
                       ga, gb, metric, k, (uint32_t)id_offset, slice_slots, lm.wide, lm.narrow, pd, pi);
    return hipGetLastError();
}

template <int FMT>
int rerank(const char* name, const float* q, int64_t nq, const uint32_t* cand, int64_t r, const uint8_t* codes, int64_t n,
           int d, const float* ga, const float* gb, int metric, int k, int64_t id_offset, void* workspace, float* dists,
           uint32_t* ids, hipStream_t st) {
    const RerankLayout L = rerank_layout(nq, r, k);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float* pd = reinterpret_cast<float*>(ws + L.pd);
    uint32_t* pi = reinterpret_cast<uint32_t*>(ws + L.pi);
    hipError_t e = with_topk_regs(k, [&](auto R) {
        return launch_rerank<FMT, decltype(R)::value>(q, nq, cand, r, codes, n, d, ga, gb, metric, k, id_offset, L, pd, pi, st);
    });
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (scan): %s", name, hipGetErrorString(e));
    e = launch_topk_merge(pd, pi, (int)L.parts, nq, k, dists, ids, st);
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s (merge): %s", name, hipGetErrorString(e));
    return MIVQ_OK;
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" size_t mivq_rerank_f32_workspace_bytes(int64_t nq, int64_t r, int32_t k) {
    return rerank_workspace_bytes(nq, r, k);
}

extern "C" size_t mivq_rerank_sq_workspace_bytes(int64_t nq, int64_t r, int32_t k) {
    return rerank_workspace_bytes(nq, r, k);
}

extern "C" size_t mivq_rerank_lvq_workspace_bytes(int64_t nq, int64_t r, int32_t k) {
    return rerank_workspace_bytes(nq, r, k);
}

extern "C" int mivq_rerank_f32(const float* q, int64_t nq, const uint32_t* cand, int64_t r, const float* x, int64_t n,
                               int32_t d, int32_t metric, int32_t k, int64_t id_offset, void* workspace,
                               size_t workspace_bytes, float* dists, uint32_t* ids, void* stream) {
    hipStream_t st = as_stream(stream);
    bool done = false;
    const int rc = rerank_prologue("rerank_f32", q, nq, cand, r, n, d, Fmt<kF32>::kPolicy, metric, k, id_offset, workspace,
                                   workspace_bytes, dists, ids, st, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(x, MIVQ_ERR_INVALID, "rerank_f32: null pointer");
    return rerank<kF32>("rerank_f32", q, nq, cand, r, reinterpret_cast<const uint8_t*>(x), n, d, nullptr, nullptr, metric, k,
                        id_offset, workspace, dists, ids, st);
}

extern "C" int mivq_rerank_sq(const float* q, int64_t nq, const uint32_t* cand, int64_t r, const void* codes, int64_t n,
                              int32_t d, const float* lo, const float* den, int32_t nbits, int32_t metric, int32_t k,
                              int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids,
                              void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && r >= 1 && d > 0, MIVQ_ERR_INVALID, "rerank_sq: bad sizes");
    MIVQ_REQUIRE(nbits == 4 || nbits == 8 || nbits == 16, MIVQ_ERR_UNSUPPORTED, "num_bits must be 4, 8, or 16, got %d",
                 nbits);
    hipStream_t st = as_stream(stream);
    bool done = false;
    const int rc = rerank_prologue("rerank_sq", q, nq, cand, r, n, d, Fmt<kSq8>::kPolicy, metric, k, id_offset, workspace,
                                   workspace_bytes, dists, ids, st, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(codes && lo && den, MIVQ_ERR_INVALID, "rerank_sq: null pointer");
    if (const int ra = sq16_aligned("rerank_sq", nbits, codes)) return ra;
    return with_sq_bits(nbits, [&](auto F) {
        return rerank<decltype(F)::value>("rerank_sq", q, nq, cand, r, static_cast<const uint8_t*>(codes), n, d, den, lo,
                                          metric, k, id_offset, workspace, dists, ids, st);
    });
}

extern "C" int mivq_rerank_lvq(const float* q, int64_t nq, const uint32_t* cand, int64_t r, const uint8_t* codes,
                               int64_t n, int32_t d, const float* mu, int32_t nbits, int32_t metric, int32_t k,
                               int64_t id_offset, void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids,
                               void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && r >= 1 && d > 0, MIVQ_ERR_INVALID, "rerank_lvq: bad sizes");
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_UNSUPPORTED, "num_bits must be in [1, 8], got %d", nbits);
    hipStream_t st = as_stream(stream);
    bool done = false;
    const int rc = rerank_prologue("rerank_lvq", q, nq, cand, r, n, d, Fmt<kLvq>::kPolicy, metric, k, id_offset, workspace,
                                   workspace_bytes, dists, ids, st, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(codes && mu, MIVQ_ERR_INVALID, "rerank_lvq: null pointer");
    return with_lvq_bits(nbits, [&](auto F) {
        return rerank<decltype(F)::value>("rerank_lvq", q, nq, cand, r, codes, n, d, mu, nullptr, metric, k, id_offset,
                                          workspace, dists, ids, st);
    });
}
