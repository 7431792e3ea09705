// rerank_internal.h — the host side the re-ranking entry points share (rerank.hip: f32 / SQ /
// LVQ stores; lvq2.hip: two-level LVQ): how a candidate list is cut into slices, the workspace
// that follows from it, and the argument checks made before any launch.
#pragma once

#include "code_internal.h"
#include "topk.h"

#include <algorithm>

namespace mivq {

constexpr int kRerankWaves = 4;

// Slices of the candidate list (grid.y): a slice is at least one slot per lane of a workgroup,
// and a batch is cut into slices only while it is too small to give every CU a few workgroups
// on its own (1024 workgroups in all).  A function of the shape alone: the workspace follows it.
inline int64_t rerank_slices(int64_t nq, int64_t r) {
    const int64_t by_len = ceil_div(r, kRerankWaves * 64);
    const int64_t by_batch = nq >= 1024 ? 1 : 1024 / nq;
    return std::max<int64_t>(1, std::min<int64_t>(std::min(by_len, by_batch), 4096));
}

struct RerankLayout {
    int64_t S, parts;
    size_t pd, pi, total;
};

inline RerankLayout rerank_layout(int64_t nq, int64_t r, int k) {
    RerankLayout L{};
    L.S = rerank_slices(nq, r);
    L.parts = L.S * kRerankWaves;
    const size_t list = align_up((size_t)L.parts * nq * k * 4, 256);
    L.pd = 0;
    L.pi = list;
    L.total = 2 * list;
    return L;
}

inline size_t rerank_workspace_bytes(int64_t nq, int64_t r, int k) {
    if (nq <= 0 || r <= 0 || k <= 0 || k > 256) return 0;
    return rerank_layout(nq, r, k).total;
}

// The checks the entry points share, made before any launch; *done is set when the call is
// complete without the kernel (nq == 0, or n == 0: sentinel lists).
inline int rerank_prologue(const char* name, const float* q, int64_t nq, const uint32_t* cand, int64_t r, int64_t n,
                           int d, ScanPolicy P, int metric, int k, int64_t id_offset, const void* workspace,
                           size_t workspace_bytes, float* dists, uint32_t* ids, hipStream_t st, bool* done) {
    *done = false;
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && r >= 1 && d > 0, MIVQ_ERR_INVALID, "%s: bad sizes", name);
    MIVQ_REQUIRE(k >= 1 && k <= 256, MIVQ_ERR_UNSUPPORTED, "%s: k=%d outside [1, 256]", name, k);
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED, "%s: metric %d",
                 name, metric);
    MIVQ_REQUIRE(scan_qb(d, P) > 0, MIVQ_ERR_UNSUPPORTED, "%s: d=%d too large for LDS", name, d);
    MIVQ_REQUIRE(id_offset >= 0 && id_offset + n <= (int64_t)kNoId, MIVQ_ERR_INVALID, "%s: ids overflow", name);
    MIVQ_REQUIRE(nq <= 0x7FFFFFFF, MIVQ_ERR_UNSUPPORTED, "%s: nq=%lld too large", name, (long long)nq);
    if (nq == 0) {
        *done = true;
        return MIVQ_OK;
    }
    MIVQ_REQUIRE(q && cand && dists && ids, MIVQ_ERR_INVALID, "%s: null pointer", name);
    if (n == 0) {
        *done = true;
        const hipError_t e = launch_topk_merge(nullptr, nullptr, 0, nq, k, dists, ids, st);
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s(empty): %s", name, hipGetErrorString(e));
        return MIVQ_OK;
    }
    const size_t need = rerank_layout(nq, r, k).total;
    MIVQ_REQUIRE(workspace && workspace_bytes >= need, MIVQ_ERR_WORKSPACE, "%s: workspace %zu < %zu", name,
                 workspace_bytes, need);
    return MIVQ_OK;
}

}  // namespace mivq
