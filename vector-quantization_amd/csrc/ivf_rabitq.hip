// ivf_rabitq.hip — IVF over RaBitQ-1 codes (faiss IVF{nlist},RaBitQ) for gfx950: the encode whose
// centre is the row's list centroid, and the estimator search over the probed lists.
//
// GPU counterpart of the reference's RaBitQIVFIndex (methods/search/rabitq_ivf_index.py).  The
// key of (query a, row i of list l) is oracle_rabitq_est on the code oracle_rabitq_encode makes
// with centroid = coarse[l]: the encode kernels and the query preparation's body are the ones
// of the flat entry points (rabitq_internal.h), so the two agree bit for bit; faiss is absent
// here, so parity with faiss itself is unpinned.
//
//   rabitq_encode_*<PER_ROW> the flat encode kernels (rabitq_internal.h), centroid = coarse[assign[row]].
//   ivf_rabitq_prep_kernel  one workgroup per (query, probe) pair: the query residual against the
//                           probed list's centroid, quantised to qb bits (int8 row + 8 factors),
//                           the pair's sort key (its list; skipped slots go to a bucket of their
//                           own) and the sentinel fill of the pair's partial lists.
//   mivq_bucket_sort        stable sort of the pairs by list: the pairs probing a list are contiguous.
//   ivf_items_kernel        per-list pair counts -> work items (list, block of 32 pairs); ivf_internal.h.
//   ivf_rabitq_scan_kernel  grid (item bound, S code ranges): the integer dots of 32 pairs x 256
//                           codes per step (v_mfma_i32_32x32x32_i8 when d % 32 == 0 and qb >= 1,
//                           as rabitq_est_mfma_kernel; one thread per code otherwise), the
//                           estimator epilogue into an LDS key tile, and the selection from it:
//                           each wave keeps the WaveTopK lists of four pairs.  No (pair x code)
//                           key matrix goes through HBM.
//   topk_merge_kernel       merges the nprobe x S partial lists of every query.
// List sizes live on the device: the grids are sized from the shape, the kernels find their work
// from offsets and the item table.  Queries are processed in chunks so the workspace stays bounded.
#include "ivf_internal.h"
#include "mivq_common.h"
#include "rabitq_internal.h"
#include "topk.h"

#include <algorithm>

namespace mivq {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));  // code rows are 4-B aligned

// ---------------------------------------------------------------- search
constexpr int kIrWaves = 8;     // waves per scan workgroup
constexpr int kIrPairs = 32;    // (query, probe) pairs per work item
constexpr int kIrTile = 256;    // codes per step: one 32-code MFMA tile per wave
constexpr int kIrPitch = 260;   // floats per key-tile row (16-B aligned rows)
constexpr int kIrMaxSplit = 8;  // code ranges per list at most
// LDS of the scan: key tile, the tile's ids, the pairs' factors, the pairs' source rows
constexpr int kIrLdsIds = kIrPairs * kIrPitch * 4;
constexpr int kIrLdsInfo = kIrLdsIds + kIrTile * 4;
constexpr int kIrLdsSrc = kIrLdsInfo + kIrPairs * kQfStride * 4;
constexpr int kIrLdsRows = kIrLdsSrc + kIrPairs * 4;  // MFMA path: the pairs' int8 rows, pitch d + 16
static_assert(kIrLdsIds % 16 == 0 && kIrLdsInfo % 16 == 0 && kIrLdsSrc % 16 == 0 && kIrLdsRows % 16 == 0, "LDS carve");
static_assert(kIrPairs % kIrWaves == 0 && kIrTile == kIrWaves * 32, "tile split");

// One workgroup per pair p = a * nprobe + j of the chunk (q, probe_l: the chunk's first row).
// keys[p]: the pair's list, nlist for a skipped slot (0xFFFFFFFF, or any id >= nlist).  The
// pair's S partial lists, part j * S + s of the (parts, nqc, k) layout, are set to the sentinel:
// the scan writes only the (pair, range) lists that hold rows.
__global__ __launch_bounds__(256) void ivf_rabitq_prep_kernel(const float* __restrict__ q, int d,
                                                              const float* __restrict__ coarse, int nlist,
                                                              const uint32_t* __restrict__ probe_l, int nprobe,
                                                              int64_t nqc, int qb, int S, int k,
                                                              int8_t* __restrict__ qq, float* __restrict__ qf,
                                                              uint32_t* __restrict__ keys, float* __restrict__ pd,
                                                              uint32_t* __restrict__ pi) {
    const int64_t p = blockIdx.x;
    const int64_t a = p / nprobe;
    const int j = (int)(p - a * nprobe);
    const uint32_t l = probe_l[p];
    const bool live = l < (uint32_t)nlist;  // block-uniform
    if (threadIdx.x == 0) keys[p] = live ? l : (uint32_t)nlist;
    for (int s = 0; s < S; ++s) {
        const int64_t base = (((int64_t)j * S + s) * nqc + a) * k;
        for (int e = threadIdx.x; e < k; e += 256) {
            pd[base + e] = INFINITY;
            pi[base + e] = kNoId;
        }
    }
    if (!live) return;
    rabitq_qprep_row(q + a * d, d, coarse + (int64_t)l * d, qb, qq + p * d, nullptr, qf + p * kQfStride);
}

struct IrScan {
    const float* q;         // (nqc, d) the chunk's queries (qb = 0: the residual is formed in the scan)
    const float* coarse;    // (nlist, d)
    const int8_t* qq;       // (pairs, d) q' - off per pair
    const float* qf;        // (pairs, kQfStride)
    const int64_t* poff;    // sorted-pair offsets per list
    const uint32_t* porder; // sorted position -> pair
    const uint2* items;
    const uint32_t* nitems;
    const int64_t* offsets; // (nlist + 1) list offsets
    const uint8_t* codes;   // (n, code_size) bucket order
    const uint32_t* ids;    // (n,)
    float* pd;              // (nprobe * S, nqc, k) partial lists
    uint32_t* pi;
    int64_t nqc;
    int d, nprobe, qb, metric, k, S;
};

// Grid (item bound, S), 512 threads.  Work item (list l, pairs [pb, pb + np)), code range s of the
// list (S equal ranges of whole 256-code tiles).  Per 256-code step the workgroup fills the
// (32 pairs, 256 codes) key tile in LDS, then wave w offers the tile's rows w, w + 8, w + 16,
// w + 24 to those pairs' WaveTopK lists; the lists go to part (probe slot) * S + s of the pair's
// query.  MFMA: lane (r, h) of wave w owns code r of the wave's 32-code tile and k-half h, exactly
// as rabitq_est_mfma_kernel (sign bits expanded to int8 in registers, the pairs' int8 rows in LDS,
// popcounts and factors to the accumulator lanes by shuffles); integer sums are exact, the
// epilogue is the oracle's.  !MFMA (any d, qb = 0): thread = code, 16 pairs each.
template <int R, bool MFMA>
__global__ __launch_bounds__(kIrWaves * 64) void ivf_rabitq_scan_kernel(const IrScan A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* tkey = reinterpret_cast<float*>(smem);
    uint32_t* tids = reinterpret_cast<uint32_t*>(smem + kIrLdsIds);
    float* pinfo = reinterpret_cast<float*>(smem + kIrLdsInfo);
    uint32_t* psrc = reinterpret_cast<uint32_t*>(smem + kIrLdsSrc);
    int8_t* qs = reinterpret_cast<int8_t*>(smem + kIrLdsRows);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    if (blockIdx.x >= *A.nitems) return;
    const uint2 item = A.items[blockIdx.x];
    const uint32_t l = item.x;
    const int64_t pb = item.y;
    const int np = (int)min<int64_t>(kIrPairs, A.poff[l + 1] - pb);
    const int64_t beg = A.offsets[l], end = A.offsets[l + 1];
    const int s = blockIdx.y;
    const int64_t per = ((end - beg + A.S - 1) / A.S + kIrTile - 1) / kIrTile * kIrTile;
    const int64_t rb = beg + s * per, re = min<int64_t>(end, rb + per);
    if (np <= 0 || rb >= re) return;  // the range holds no rows: the sentinel lists stand
    const int d = A.d, nb = (d + 7) >> 3, cs = nb + 8;
    const int QP = d + 16;
    if (tid < kIrPairs) {  // rows past np repeat pair 0 (in range); their keys are never offered
        const uint32_t op = A.porder[pb + (tid < np ? tid : 0)];
        psrc[tid] = op;
        const float* f = A.qf + (int64_t)op * kQfStride;
        *reinterpret_cast<float4*>(pinfo + tid * kQfStride) = *reinterpret_cast<const float4*>(f);
        *reinterpret_cast<float4*>(pinfo + tid * kQfStride + 4) = *reinterpret_cast<const float4*>(f + 4);
    }
    __syncthreads();
    if (MFMA) {
        const int qch = d >> 4;
        for (int e = tid; e < kIrPairs * qch; e += kIrWaves * 64) {
            const int row = e / qch, c = e - row * qch;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row < np) v = *reinterpret_cast<const uint4*>(A.qq + (int64_t)psrc[row] * d + 16 * c);
            *reinterpret_cast<uint4*>(qs + row * QP + 16 * c) = v;
        }
        __syncthreads();
    }
    const bool ip = A.metric == MIVQ_METRIC_INNER_PRODUCT;
    const int k = A.k;
    constexpr int PW = kIrPairs / kIrWaves;  // pairs per wave
    WaveTopK<R> top[PW];
    float thr_d[PW];
    uint32_t thr_i[PW];
#pragma unroll
    for (int i = 0; i < PW; ++i) {
        top[i].init();
        thr_d[i] = INFINITY;
        thr_i[i] = kNoId;
    }
    for (int64_t c0 = rb; c0 < re; c0 += kIrTile) {
        if (tid < kIrTile) tids[tid] = c0 + tid < re ? A.ids[c0 + tid] : kNoId;
        if (MFMA) {
            const int64_t cb = c0 + 32 * w;
            const int nc = (int)max<int64_t>(0, min<int64_t>(32, re - cb));
            if (nc > 0) {  // wave-uniform
                // rows past the range read row 0 of the tile (in range); their keys are never offered
                const uint8_t* crow = A.codes + (cb + (r < nc ? r : 0)) * cs;
                const int8_t* qrow = qs + r * QP + 16 * h;
                const int sh = 16 * h;
                const int nks = d >> 5, n4 = nks >> 2;
                v16i acc = {};
                int pc = 0;
                auto kstep = [&](uint32_t dw, int ks) __attribute__((always_inline)) {
                    const uint32_t b16 = (dw >> sh) & 0xFFFFu;
                    pc += __builtin_popcount(b16);
                    const v4i av = rabitq_sign_bytes(b16);
                    const v4i bq = *reinterpret_cast<const v4i*>(qrow + 32 * ks);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bq, acc, 0, 0, 0);
                };
                if (n4 > 0) {
                    u32x4a4 cur = *reinterpret_cast<const u32x4a4*>(crow);  // cs % 4 == 0: 4-B aligned rows
                    for (int g = 0; g < n4; ++g) {
                        const u32x4a4 nxt = g + 1 < n4 ? *reinterpret_cast<const u32x4a4*>(crow + 16 * (g + 1)) : cur;
                        kstep(cur[0], 4 * g + 0);
                        kstep(cur[1], 4 * g + 1);
                        kstep(cur[2], 4 * g + 2);
                        kstep(cur[3], 4 * g + 3);
                        cur = nxt;
                    }
                }
                for (int ks = 4 * n4; ks < nks; ++ks) kstep(*reinterpret_cast<const uint32_t*>(crow + 4 * ks), ks);
                const float fr = *reinterpret_cast<const float*>(crow + nb + 4 * h);  // h = 0: f0, 1: f1 of code r
                const float* f = pinfo + r * kQfStride;  // accumulator column r = pair r
                const float c1 = f[0], c2 = f[1], c34 = f[2], qc = f[3], qn = f[4];
                const int off = (int)f[6];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float kv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int ci = 8 * g + 4 * h + u;  // code row of accumulator 4g + u
                        const int pop = __shfl(pc, ci) + __shfl(pc, ci + 32);
                        const float f0 = __shfl(fr, ci), f1 = __shfl(fr, ci + 32);
                        const int dot = acc[4 * g + u] + off * pop;
                        const float fd = __builtin_fmaf(c1, (float)dot, __builtin_fmaf(c2, (float)pop, -c34));
                        const float key = rabitq_key(fd, f0, f1, qc, qn, ip);
                        kv[u] = key != key ? INFINITY : key;
                    }
                    *reinterpret_cast<float4*>(tkey + r * kIrPitch + 32 * w + 8 * g + 4 * h) =
                        make_float4(kv[0], kv[1], kv[2], kv[3]);
                }
            }
        } else {
            const int col = tid & (kIrTile - 1), half = tid >> 8;
            const int64_t ci = c0 + col;
            if (ci < re) {
                const uint8_t* code = A.codes + ci * cs;
                const float f0 = load_f32(code + nb), f1 = load_f32(code + nb + 4);
                const int p1 = min(np, (half + 1) * (kIrPairs / 2));
                for (int pr = half * (kIrPairs / 2); pr < p1; ++pr) {
                    const float* f = pinfo + pr * kQfStride;
                    const int64_t op = psrc[pr];
                    float fd;
                    if (A.qb > 0) {
                        const int8_t* qv = A.qq + op * d;
                        const int off = (int)f[6];
                        int dot = 0, pop = 0;
                        for (int j = 0; j < d; ++j) {
                            const int b = (code[j >> 3] >> (j & 7)) & 1;
                            dot += b ? (int)qv[j] + off : 0;
                            pop += b;
                        }
                        fd = __builtin_fmaf(f[0], (float)dot, __builtin_fmaf(f[1], (float)pop, -f[2]));
                    } else {
                        const float* qv = A.q + (op / A.nprobe) * d;
                        const float* cv = A.coarse + (int64_t)l * d;
                        float sum = 0.0f;
                        for (int j = 0; j < d; ++j) {
                            const float rj = __fsub_rn(qv[j], cv[j]);
                            sum = __fadd_rn(sum, ((code[j >> 3] >> (j & 7)) & 1) ? rj : -rj);
                        }
                        fd = __fmul_rn(sum, f[5]);
                    }
                    const float key = rabitq_key(fd, f0, f1, f[3], f[4], ip);
                    tkey[pr * kIrPitch + col] = key != key ? INFINITY : key;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            const int pr = w + kIrWaves * i;
            if (pr < np) {  // wave-uniform
#pragma unroll
                for (int t = 0; t < kIrTile / 64; ++t) {
                    const int col = 64 * t + lane;
                    const bool valid = c0 + col < re;
                    top[i].offer(valid, tkey[pr * kIrPitch + col], tids[col], k, lane, thr_d[i], thr_i[i]);
                }
            }
        }
        __syncthreads();  // the tile is rewritten by the next step
    }
#pragma unroll
    for (int i = 0; i < PW; ++i) {
        const int pr = w + kIrWaves * i;
        if (pr < np) {
            const int64_t op = psrc[pr];
            const int64_t a = op / A.nprobe;
            const int64_t j = op - a * A.nprobe;
            const int64_t base = ((j * A.S + s) * A.nqc + a) * k;
            top[i].store(A.pd + base, A.pi + base, k, lane);
        }
    }
}

// Workspace of one search, sized on shape alone.  Queries are processed nqc at a time.
struct IrLayout {
    int64_t nqc;  // queries per chunk
    int S;        // code ranges per list
    size_t qq, qf, keys, porder, poff, items, nitems, sortws, pd, pi, total;
};

constexpr size_t kIrBudget = (size_t)1 << 29;  // aim of the chunking: 512 MiB
constexpr size_t kIrCap = (size_t)1 << 30;     // never above 1 GiB (adc_filtered_shape's cap)

IrLayout ir_layout(int64_t nq, int nlist, int nprobe, int d, int k) {
    nq = std::max<int64_t>(nq, 1);
    // few pairs: split the lists into code ranges so that the chip still has workgroups to run
    const int64_t blocks = ceil_div(nq * nprobe, kIrPairs);
    const int S = (int)std::max<int64_t>(1, std::min<int64_t>(kIrMaxSplit, ceil_div(2048, blocks)));
    auto build = [&](int64_t nqc) {
        IrLayout L{};
        L.nqc = nqc;
        L.S = S;
        const size_t P = (size_t)nqc * nprobe;
        size_t off = 0;
        L.qq = off;     off = align_up(off + P * d, 256);
        L.qf = off;     off = align_up(off + P * kQfStride * 4, 256);
        L.keys = off;   off = align_up(off + P * 4, 256);
        L.porder = off; off = align_up(off + P * 4, 256);
        L.poff = off;   off = align_up(off + ((size_t)nlist + 2) * 8, 256);
        L.items = off;  off = align_up(off + ((size_t)ceil_div(P, kIrPairs) + nlist) * 8, 256);
        L.nitems = off; off += 256;
        L.sortws = off; off = align_up(off + mivq_bucket_sort_workspace_bytes((int64_t)P, nlist + 1), 256);
        L.pd = off;     off = align_up(off + P * S * k * 4, 256);
        L.pi = off;     off = align_up(off + P * S * k * 4, 256);
        L.total = off;
        return L;
    };
    const size_t per_query = (size_t)nprobe * ((size_t)d + kQfStride * 4 + 8 + (size_t)S * k * 8);
    int64_t nqc = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(kIrBudget / per_query)));
    IrLayout L = build(nqc);
    while (L.total > kIrCap && nqc > 1) {
        nqc = (nqc + 1) / 2;
        L = build(nqc);
    }
    return L;
}

bool ir_sizes_ok(int64_t nq, int32_t nlist, int32_t nprobe, int32_t d) {
    return nq >= 0 && nlist > 0 && nprobe > 0 && d > 0;
}

template <int R>
hipError_t launch_ir_scan(bool mfma, const IrScan& A, int64_t maxitems, hipStream_t st) {
    const size_t smem = mfma ? (size_t)kIrLdsRows + (size_t)kIrPairs * (A.d + 16) : (size_t)kIrLdsRows;
    const void* fn = mfma ? (const void*)ivf_rabitq_scan_kernel<R, true> : (const void*)ivf_rabitq_scan_kernel<R, false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)maxitems, (unsigned)A.S), block(kIrWaves * 64);
    if (mfma) hipLaunchKernelGGL((ivf_rabitq_scan_kernel<R, true>), grid, block, smem, st, A);
    else hipLaunchKernelGGL((ivf_rabitq_scan_kernel<R, false>), grid, block, smem, st, A);
    return hipGetLastError();
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_ivf_rabitq_encode(const float* x, int64_t n, int32_t d, const float* coarse, int32_t nlist,
                                      const uint32_t* assign, int32_t metric, uint8_t* codes, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0 && nlist > 0, MIVQ_ERR_INVALID, "ivf_rabitq_encode: bad sizes n=%lld d=%d nlist=%d",
                 (long long)n, d, nlist);
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED,
                 "ivf_rabitq_encode: metric %d", metric);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(x && coarse && assign && codes, MIVQ_ERR_INVALID, "ivf_rabitq_encode: null pointer");
    const bool vec = (d % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0);
    const int ni = d / 512;
    const bool wide = vec && d % 512 == 0 && reinterpret_cast<uintptr_t>(coarse) % 16 == 0;
    const dim3 grid((unsigned)ceil_div(n, 4)), block(256);
    hipStream_t st = as_stream(stream);
    if (wide && ni % 6 == 0)
        hipLaunchKernelGGL((rabitq_encode_wide_kernel<6, true>), grid, block, 0, st, x, n, d, coarse, assign, metric, codes);
    else if (wide && ni % 4 == 0)
        hipLaunchKernelGGL((rabitq_encode_wide_kernel<4, true>), grid, block, 0, st, x, n, d, coarse, assign, metric, codes);
    else if (wide && ni % 3 == 0)
        hipLaunchKernelGGL((rabitq_encode_wide_kernel<3, true>), grid, block, 0, st, x, n, d, coarse, assign, metric, codes);
    else if (wide && ni % 2 == 0)
        hipLaunchKernelGGL((rabitq_encode_wide_kernel<2, true>), grid, block, 0, st, x, n, d, coarse, assign, metric, codes);
    else if (vec)
        hipLaunchKernelGGL((rabitq_encode_kernel<true, true>), grid, block, 0, st, x, n, d, coarse, assign, metric, codes);
    else
        hipLaunchKernelGGL((rabitq_encode_kernel<false, true>), grid, block, 0, st, x, n, d, coarse, assign, metric, codes);
    return check_launch("ivf_rabitq_encode");
}

extern "C" size_t mivq_ivf_rabitq_search_workspace_bytes(int64_t nq, int64_t n, int32_t nlist, int32_t nprobe,
                                                         int32_t d, int32_t k) {
    if (!ir_sizes_ok(nq, nlist, nprobe, d) || n < 0 || k <= 0 || k > 256 || nlist > 16383) return 0;
    return ir_layout(nq, nlist, nprobe, d, k).total;
}

extern "C" int mivq_ivf_rabitq_search(const float* q, int64_t nq, int32_t d, const float* coarse, int32_t nlist,
                                      const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets,
                                      const uint8_t* list_codes, const uint32_t* list_ids, int32_t qb, int32_t metric,
                                      int32_t k, void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids,
                                      void* stream) {
    MIVQ_REQUIRE(ir_sizes_ok(nq, nlist, nprobe, d), MIVQ_ERR_INVALID,
                 "ivf_rabitq_search: bad sizes nq=%lld d=%d nlist=%d nprobe=%d", (long long)nq, d, nlist, nprobe);
    MIVQ_REQUIRE(k >= 1 && k <= 256, MIVQ_ERR_UNSUPPORTED, "ivf_rabitq_search: k=%d not in [1, 256]", k);
    MIVQ_REQUIRE(qb >= 0 && qb <= 8, MIVQ_ERR_UNSUPPORTED, "ivf_rabitq_search: qb=%d not in [0, 8]", qb);
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED,
                 "ivf_rabitq_search: metric %d", metric);
    MIVQ_REQUIRE(nlist <= 16383, MIVQ_ERR_UNSUPPORTED, "ivf_rabitq_search: nlist=%d > 16383", nlist);
    if (nq == 0) return MIVQ_OK;
    MIVQ_REQUIRE(q && coarse && probe_l && offsets && list_codes && list_ids && dists && ids && workspace,
                 MIVQ_ERR_INVALID, "ivf_rabitq_search: null pointer");
    const IrLayout L = ir_layout(nq, nlist, nprobe, d, k);
    MIVQ_REQUIRE(workspace_bytes >= L.total, MIVQ_ERR_WORKSPACE, "ivf_rabitq_search: workspace %zu < %zu bytes",
                 workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    unsigned char* p = static_cast<unsigned char*>(workspace);
    int8_t* qq = reinterpret_cast<int8_t*>(p + L.qq);
    float* qf = reinterpret_cast<float*>(p + L.qf);
    uint32_t* keys = reinterpret_cast<uint32_t*>(p + L.keys);
    uint32_t* porder = reinterpret_cast<uint32_t*>(p + L.porder);
    int64_t* poff = reinterpret_cast<int64_t*>(p + L.poff);
    uint2* items = reinterpret_cast<uint2*>(p + L.items);
    uint32_t* nitems = reinterpret_cast<uint32_t*>(p + L.nitems);
    float* pd = reinterpret_cast<float*>(p + L.pd);
    uint32_t* pi = reinterpret_cast<uint32_t*>(p + L.pi);
    // the MFMA scan: d % 32 == 0 (whole k-steps, 4-B aligned code rows), qb >= 1, the 32 int8 rows in LDS
    const bool mfma = qb > 0 && d % 32 == 0 && reinterpret_cast<uintptr_t>(list_codes) % 4 == 0 &&
                      (size_t)kIrLdsRows + (size_t)kIrPairs * (d + 16) <= 160 * 1024;
    for (int64_t a0 = 0; a0 < nq; a0 += L.nqc) {
        const int64_t nqc = std::min<int64_t>(L.nqc, nq - a0);
        const int64_t P = nqc * nprobe;
        hipLaunchKernelGGL(ivf_rabitq_prep_kernel, dim3((unsigned)P), dim3(256), 0, st, q + a0 * d, d, coarse, nlist,
                           probe_l + a0 * nprobe, nprobe, nqc, qb, L.S, k, qq, qf, keys, pd, pi);
        int rc = check_launch("ivf_rabitq_prep");
        if (rc) return rc;
        rc = mivq_bucket_sort(keys, P, nlist + 1, poff, porder, p + L.sortws, L.pd - L.sortws, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(ivf_items_kernel<kIrPairs>, dim3(1), dim3(1024), 0, st, poff, nlist, items, nitems);
        rc = check_launch("ivf_rabitq_items");
        if (rc) return rc;
        const IrScan A{q + a0 * d, coarse, qq, qf, poff, porder, items, nitems, offsets, list_codes, list_ids,
                       pd, pi, nqc, d, nprobe, qb, metric, k, L.S};
        hipError_t e = with_topk_regs(k, [&](auto R) {
            return launch_ir_scan<decltype(R)::value>(mfma, A, ceil_div(P, kIrPairs) + nlist, st);
        });
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "ivf_rabitq_scan: %s", hipGetErrorString(e));
        e = launch_topk_merge(pd, pi, nprobe * L.S, nqc, k, dists + a0 * k, ids + a0 * k, st);
        if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "ivf_rabitq merge: %s", hipGetErrorString(e));
    }
    return MIVQ_OK;
}
