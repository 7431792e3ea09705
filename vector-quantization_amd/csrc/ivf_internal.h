// ivf_internal.h — the probed-list driver of the searches over IVF lists of codes (ivf_rabitq.hip,
// ivf_code.hip, ivf_listpq.hip), and the workgroup scan it shares with ivf.hip.
//
// One search, per chunk of queries (ivf_probed_search):
//   the caller's prep   one workgroup per (query, probe slot) pair: ivf_pair_prologue gives the pair
//                       its sort key (its list; skipped slots go to bucket nlist) and fills its S
//                       partial lists with the sentinel.
//   mivq_bucket_sort    stable sort of the pairs by list: the pairs probing a list are contiguous.
//   ivf_items_kernel    per-list pair counts -> work items (list, block of PPI pairs).
//   the caller's scan   grid (item bound, S row ranges of the list): ivf_item finds the workgroup's
//                       list, pairs and rows; the top-k of every (pair, range) is selected inside
//                       the scan and goes to IvfScan::part_base.
//   topk_merge_kernel   merges the nprobe x S partial lists of every query.
// List sizes live on the device: the grids are sized from the shape, the kernels find their work
// from offsets and the item table.  Queries go through in chunks so the workspace stays bounded.
//
// Every translation unit is linked without relocatable device code: a __global__ function here
// must be a template (or sit in an unnamed namespace).
#pragma once

#include "mivq_common.h"
#include "topk.h"

#include <algorithm>

namespace mivq {

constexpr int kIvfMaxSplit = 8;                 // row ranges per list at most
constexpr size_t kIvfBudget = (size_t)1 << 29;  // aim of the chunking: 512 MiB
constexpr size_t kIvfCap = (size_t)1 << 30;     // never above 1 GiB (adc_filtered_shape's cap)
// The pairs are sorted into nlist + 1 buckets, and mivq_bucket_sort keeps one int64 slot per
// bucket in LDS: 16384 buckets at most.
constexpr int kIvfMaxLists = 16383;

// Exclusive prefix of v over the 1024 threads of the workgroup (Hillis-Steele in part[1024]) on
// top of *carry, which then advances by the workgroup's sum.  part and carry are in LDS.
__device__ inline int64_t scan1024_carry(int64_t v, int64_t* part, int64_t* carry) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t add = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    const int64_t first = *carry + part[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) *carry = first + v;
    __syncthreads();
    return first;
}

// poff: the bucket offsets of the sorted pairs (nlist + 2 entries; bucket nlist = skipped slots).
// items[i] = (list, first sorted pair of the block of PPI pairs), nitems = their count
// (<= ceil(pairs / PPI) + nlist).  One workgroup.
template <int PPI>
__global__ __launch_bounds__(1024) void ivf_items_kernel(const int64_t* __restrict__ poff, int nlist,
                                                         uint2* __restrict__ items, uint32_t* __restrict__ nitems) {
    __shared__ int64_t part[1024];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nlist; base += 1024) {
        const int l = base + threadIdx.x;
        const int64_t p0 = l < nlist ? poff[l] : 0;
        const int64_t v = l < nlist ? (poff[l + 1] - p0 + PPI - 1) / PPI : 0;
        const int64_t first = scan1024_carry(v, part, &carry);
        for (int64_t b = 0; b < v; ++b) items[first + b] = make_uint2((uint32_t)l, (uint32_t)(p0 + b * PPI));
    }
    if (threadIdx.x == 0) *nitems = (uint32_t)carry;
}

// ---------------------------------------------------------------- device side
// First element of the partial list of (query a of the chunk, probe slot j) and row range s:
// part j * S + s of the (nprobe * S, nqc, k) layout.
__device__ inline int64_t ivf_part_base(int64_t a, int64_t j, int s, int S, int64_t nqc, int k) {
    return ((j * S + s) * nqc + a) * k;
}

// One workgroup per pair p = blockIdx.x of the chunk (probe_l: the chunk's first row).  keys[p]:
// the pair's list, nlist for a skipped slot (0xFFFFFFFF, or any id >= nlist).  The pair's S
// partial lists are set to the sentinel: the scan writes only the (pair, range) lists that hold
// rows.  Returns the key (block-uniform: the list of a live slot); *query = a.
__device__ inline uint32_t ivf_pair_prologue(const uint32_t* __restrict__ probe_l, int nlist, int nprobe, int64_t nqc,
                                             int S, int k, uint32_t* __restrict__ keys, float* __restrict__ pd,
                                             uint32_t* __restrict__ pi, int64_t* query) {
    const int64_t p = blockIdx.x;
    const int64_t a = *query = p / nprobe;
    const int64_t j = p - a * nprobe;
    const uint32_t l = min(probe_l[p], (uint32_t)nlist);
    if (threadIdx.x == 0) keys[p] = l;
    for (int s = 0; s < S; ++s) {
        const int64_t base = ivf_part_base(a, j, s, S, nqc, k);
        for (int e = threadIdx.x; e < k; e += blockDim.x) {
            pd[base + e] = INFINITY;
            pi[base + e] = kNoId;
        }
    }
    return l;
}

// The prep of a search whose pairs need the prologue and nothing else (ivf_code.hip,
// ivf_listpq.hip): THREADS = its workgroup.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void ivf_prep_kernel(const uint32_t* __restrict__ probe_l, int nlist, int nprobe,
                                                           int64_t nqc, int S, int k, uint32_t* __restrict__ keys,
                                                           float* __restrict__ pd, uint32_t* __restrict__ pi) {
    int64_t a;
    ivf_pair_prologue(probe_l, nlist, nprobe, nqc, S, k, keys, pd, pi, &a);
}

// What every scan over probed lists takes; the caller's argument struct embeds it.
struct IvfScan {
    int64_t* poff;           // sorted-pair offsets per list
    uint32_t* porder;        // sorted position -> pair
    uint2* items;            // the work items and their count
    uint32_t* nitems;
    const int64_t* offsets;  // (nlist + 1) list offsets
    const uint8_t* codes;    // (n, row bytes) bucket order
    const uint32_t* ids;     // (n,)
    float* pd;               // (nprobe * S, nqc, k) partial lists
    uint32_t* pi;
    int64_t nqc;
    int nprobe, k, S;

    __device__ int64_t part_base(int64_t pair, int s) const {
        const int64_t a = pair / nprobe;
        return ivf_part_base(a, pair - a * nprobe, s, S, nqc, k);
    }
    __device__ bool past_items() const { return blockIdx.x >= *nitems; }  // the grid is a bound on the items
};

// The work of scan workgroup (blockIdx.x, blockIdx.y = s): list l, its sorted pairs
// [pb, pb + np), np <= PPI, and rows [rb, re): range s of the list's S equal ranges of whole
// TILE-row steps.
struct IvfItem {
    uint32_t l;
    int64_t pb;
    int np;
    int64_t rb, re;
    __device__ bool empty() const { return np <= 0 || rb >= re; }  // no rows: the sentinel lists stand
};

// Of a workgroup that is not past_items().  A scan begins
//     if (A.past_items()) return;  it = ivf_item<PPI, TILE>(A);  if (it.empty()) return;
// The two exits stay in the kernel: folded into this function they merge into one branch, and
// the RaBitQ scan kernels then take 2 to 4 more VGPRs (R = 3 loses a wave of occupancy).
template <int PPI, int TILE>
__device__ __forceinline__ IvfItem ivf_item(const IvfScan& A) {
    const uint2 item = A.items[blockIdx.x];
    const uint32_t l = item.x;
    const int64_t pb = item.y, beg = A.offsets[l], end = A.offsets[l + 1];
    const int64_t per = ((end - beg + A.S - 1) / A.S + TILE - 1) / TILE * TILE;
    const int64_t rb = beg + (int)blockIdx.y * per;
    return IvfItem{l, pb, (int)min<int64_t>(PPI, A.poff[l + 1] - pb), rb, min<int64_t>(end, rb + per)};
}

// ---------------------------------------------------------------- host side
// Workspace of one search, sized on shape alone.  Queries are processed nqc at a time.
struct IvfLayout {
    int64_t nqc;  // queries per chunk
    int S;        // row ranges per list
    size_t xa, xb, keys, porder, poff, items, nitems, sortws, pd, pi, total;
};

// ppi: pairs per work item.  xa, xb: bytes per pair of the caller's own two regions, placed
// first.  fixed: the bytes per pair that the chunk estimate counts next to the partial lists;
// the two searches count them differently (RaBitQ: its rows + 8, codes: 16) for no deeper
// reason than that their workspace sizes stay what they were.
inline IvfLayout ivf_layout(int64_t nq, int nlist, int nprobe, int k, int ppi, size_t xa, size_t xb, size_t fixed) {
    nq = std::max<int64_t>(nq, 1);
    // few pairs: split the lists into row ranges so that the chip still has workgroups to run
    const int64_t blocks = ceil_div(nq * nprobe, ppi);
    const int S = (int)std::max<int64_t>(1, std::min<int64_t>(kIvfMaxSplit, ceil_div(2048, blocks)));
    auto build = [&](int64_t nqc) {
        IvfLayout L{nqc, S};
        const size_t P = (size_t)nqc * nprobe;
        size_t off = 0;
        L.xa = off;     off = align_up(off + P * xa, 256);
        L.xb = off;     off = align_up(off + P * xb, 256);
        L.keys = off;   off = align_up(off + P * 4, 256);
        L.porder = off; off = align_up(off + P * 4, 256);
        L.poff = off;   off = align_up(off + ((size_t)nlist + 2) * 8, 256);
        L.items = off;  off = align_up(off + ((size_t)ceil_div(P, ppi) + nlist) * 8, 256);
        L.nitems = off; off += 256;
        L.sortws = off; off = align_up(off + mivq_bucket_sort_workspace_bytes((int64_t)P, nlist + 1), 256);
        L.pd = off;     off = align_up(off + P * S * k * 4, 256);
        L.pi = off;     off = align_up(off + P * S * k * 4, 256);
        L.total = off;
        return L;
    };
    const size_t per_query = (size_t)nprobe * (fixed + (size_t)S * k * 8);
    int64_t nqc = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(kIvfBudget / per_query)));
    IvfLayout L = build(nqc);
    while (L.total > kIvfCap && nqc > 1) {
        nqc = (nqc + 1) / 2;
        L = build(nqc);
    }
    return L;
}

// Pairs per work item: max_qb (a power of two; 0 stays 0), narrowed to the pairs a list can
// expect, since a scan workgroup computes the chains of all its pairs for every row.
inline int ivf_pairs_per_item(int max_qb, int64_t nq, int nlist, int nprobe) {
    int QB = max_qb;
    const int64_t per_list = ceil_div(std::max<int64_t>(nq, 1) * nprobe, nlist);
    while (QB > 1 && QB / 2 >= per_list) QB /= 2;
    return QB;
}

// The argument checks of the searches and of their workspace queries.
inline bool ivf_sizes_ok(int64_t nq, int64_t n, int nlist, int nprobe, int d) {
    return nq >= 0 && n >= 0 && nlist > 0 && nprobe > 0 && d > 0;
}
inline bool ivf_shape_ok(int64_t nq, int64_t n, int nlist, int nprobe, int d, int k) {
    return ivf_sizes_ok(nq, n, nlist, nprobe, d) && k >= 1 && k <= 256 && nlist <= kIvfMaxLists;
}
// max_d: the caller's own limit on d, reported as a bad size too.
inline int ivf_search_check(const char* name, int64_t nq, int d, int max_d, int nlist, int nprobe, int k, int metric) {
    MIVQ_REQUIRE(ivf_sizes_ok(nq, 0, nlist, nprobe, d) && d <= max_d, MIVQ_ERR_INVALID,
                 "%s: bad sizes nq=%lld d=%d nlist=%d nprobe=%d", name, (long long)nq, d, nlist, nprobe);
    MIVQ_REQUIRE(k >= 1 && k <= 256, MIVQ_ERR_UNSUPPORTED, "%s: k=%d not in [1, 256]", name, k);
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED, "%s: metric %d",
                 name, metric);
    MIVQ_REQUIRE(nlist <= kIvfMaxLists, MIVQ_ERR_UNSUPPORTED, "%s: nlist=%d > %d", name, nlist, kIvfMaxLists);
    return MIVQ_OK;
}

// One chunk of queries [a0, a0 + nqc) as the caller's prep and scan see it.
struct IvfChunk {
    int64_t a0, nqc, pairs;
    unsigned char *xa, *xb;  // the caller's per-pair regions
    uint32_t* keys;
    IvfScan scan;
};

// Runs a search whose arguments are validated.  prep(chunk) launches the caller's pair kernel on
// chunk.pairs workgroups, scan(chunk, item bound) the caller's scan; both return a hipError_t.
template <int PPI, class Prep, class Scan>
int ivf_probed_search(const char* name, const IvfLayout& L, int64_t nq, int nlist, int nprobe, int k,
                      const int64_t* offsets, const uint8_t* list_codes, const uint32_t* list_ids, void* workspace,
                      size_t workspace_bytes, float* dists, uint32_t* ids, void* stream, Prep&& prep, Scan&& scan) {
    MIVQ_REQUIRE(workspace && workspace_bytes >= L.total, MIVQ_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", name,
                 workspace_bytes, L.total);
    auto fail = [&](const char* step, hipError_t e) {
        return set_error(MIVQ_ERR_HIP, "%s (%s): %s", name, step, hipGetErrorString(e));
    };
    hipStream_t st = as_stream(stream);
    unsigned char* p = static_cast<unsigned char*>(workspace);
    IvfChunk c{0, 0, 0, p + L.xa, p + L.xb, reinterpret_cast<uint32_t*>(p + L.keys)};
    IvfScan& A = c.scan;
    A = IvfScan{reinterpret_cast<int64_t*>(p + L.poff), reinterpret_cast<uint32_t*>(p + L.porder),
                reinterpret_cast<uint2*>(p + L.items), reinterpret_cast<uint32_t*>(p + L.nitems), offsets, list_codes,
                list_ids, reinterpret_cast<float*>(p + L.pd), reinterpret_cast<uint32_t*>(p + L.pi), 0, nprobe, k, L.S};
    for (; c.a0 < nq; c.a0 += L.nqc) {
        c.nqc = A.nqc = std::min<int64_t>(L.nqc, nq - c.a0);
        c.pairs = c.nqc * nprobe;
        hipError_t e;
        if ((e = prep(c)) != hipSuccess) return fail("prep", e);
        const int rc = mivq_bucket_sort(c.keys, c.pairs, nlist + 1, A.poff, A.porder, p + L.sortws, L.pd - L.sortws, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(ivf_items_kernel<PPI>, dim3(1), dim3(1024), 0, st, A.poff, nlist, A.items, A.nitems);
        if ((e = hipGetLastError()) != hipSuccess) return fail("items", e);
        if ((e = scan(c, ceil_div(c.pairs, PPI) + nlist)) != hipSuccess) return fail("scan", e);
        e = launch_topk_merge(A.pd, A.pi, nprobe * L.S, c.nqc, k, dists + c.a0 * k, ids + c.a0 * k, st);
        if (e != hipSuccess) return fail("merge", e);
    }
    return MIVQ_OK;
}

}  // namespace mivq
