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
//   ivf_rabitq_prep_kernel  the driver's pair prologue, then the query residual against the probed
//                           list's centroid, quantised to qb bits (int8 row + 8 factors).
//   ivf_rabitq_scan_kernel  the integer dots of 32 pairs x 256 codes per step
//                           (v_mfma_i32_32x32x32_i8 when d % 32 == 0 and qb >= 1, as
//                           rabitq_est_mfma_kernel; one thread per code otherwise), the
//                           estimator epilogue into an LDS key tile, and the selection from it:
//                           each wave keeps the WaveTopK lists of four pairs.  No (pair x code)
//                           key matrix goes through HBM.
// The search runs on the probed-list driver (ivf_internal.h): pair sort, work items, chunks of
// queries and the merge of the partial lists are its steps.
#include "ivf_internal.h"
#include "mivq_common.h"
#include "rabitq_internal.h"
#include "topk.h"

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
// LDS of the scan: key tile, the tile's ids, the pairs' factors, the pairs' source rows
constexpr int kIrLdsIds = kIrPairs * kIrPitch * 4;
constexpr int kIrLdsInfo = kIrLdsIds + kIrTile * 4;
constexpr int kIrLdsSrc = kIrLdsInfo + kIrPairs * kQfStride * 4;
constexpr int kIrLdsRows = kIrLdsSrc + kIrPairs * 4;  // MFMA path: the pairs' int8 rows, pitch d + 16
static_assert(kIrLdsIds % 16 == 0 && kIrLdsInfo % 16 == 0 && kIrLdsSrc % 16 == 0 && kIrLdsRows % 16 == 0, "LDS carve");
static_assert(kIrPairs % kIrWaves == 0 && kIrTile == kIrWaves * 32, "tile split");

// One workgroup per pair p = a * nprobe + j of the chunk (q, probe_l: the chunk's first row).
__global__ __launch_bounds__(256) void ivf_rabitq_prep_kernel(const float* __restrict__ q, int d,
                                                              const float* __restrict__ coarse, int nlist,
                                                              const uint32_t* __restrict__ probe_l, int nprobe,
                                                              int64_t nqc, int qb, int S, int k,
                                                              int8_t* __restrict__ qq, float* __restrict__ qf,
                                                              uint32_t* __restrict__ keys, float* __restrict__ pd,
                                                              uint32_t* __restrict__ pi) {
    int64_t a;
    const uint32_t l = ivf_pair_prologue(probe_l, nlist, nprobe, nqc, S, k, keys, pd, pi, &a);
    if (l == (uint32_t)nlist) return;  // a skipped slot
    const int64_t p = blockIdx.x;
    rabitq_qprep_row(q + a * d, d, coarse + (int64_t)l * d, qb, qq + p * d, nullptr, qf + p * kQfStride);
}

struct IrScan {
    IvfScan s;
    const float* q;       // (nqc, d) the chunk's queries (qb = 0: the residual is formed in the scan)
    const float* coarse;  // (nlist, d)
    const int8_t* qq;     // (pairs, d) q' - off per pair
    const float* qf;      // (pairs, kQfStride)
    int d, qb, metric;
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
    if (A.s.past_items()) return;
    const IvfItem it = ivf_item<kIrPairs, kIrTile>(A.s);
    if (it.empty()) return;
    const auto [l, pb, np, rb, re] = it;
    const int d = A.d, nb = (d + 7) >> 3, cs = nb + 8;
    const int QP = d + 16;
    if (tid < kIrPairs) {  // rows past np repeat pair 0 (in range); their keys are never offered
        const uint32_t op = A.s.porder[pb + (tid < np ? tid : 0)];
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
    const int k = A.s.k;
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
        if (tid < kIrTile) tids[tid] = c0 + tid < re ? A.s.ids[c0 + tid] : kNoId;
        if (MFMA) {
            const int64_t cb = c0 + 32 * w;
            const int nc = (int)max<int64_t>(0, min<int64_t>(32, re - cb));
            if (nc > 0) {  // wave-uniform
                // rows past the range read row 0 of the tile (in range); their keys are never offered
                const uint8_t* crow = A.s.codes + (cb + (r < nc ? r : 0)) * cs;
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
                const uint8_t* code = A.s.codes + ci * cs;
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
                        const float* qv = A.q + (op / A.s.nprobe) * d;
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
            const int64_t base = A.s.part_base(psrc[pr], blockIdx.y);
            top[i].store(A.s.pd + base, A.s.pi + base, k, lane);
        }
    }
}

// The driver's layout with the pairs' int8 rows and factors in front.
IvfLayout ir_layout(int64_t nq, int nlist, int nprobe, int d, int k) {
    return ivf_layout(nq, nlist, nprobe, k, kIrPairs, (size_t)d, kQfStride * 4, (size_t)d + kQfStride * 4 + 8);
}

template <int R>
hipError_t launch_ir_scan(bool mfma, const IrScan& A, int64_t maxitems, hipStream_t st) {
    const size_t smem = mfma ? (size_t)kIrLdsRows + (size_t)kIrPairs * (A.d + 16) : (size_t)kIrLdsRows;
    const void* fn = mfma ? (const void*)ivf_rabitq_scan_kernel<R, true> : (const void*)ivf_rabitq_scan_kernel<R, false>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)maxitems, (unsigned)A.s.S), block(kIrWaves * 64);
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
    if (!ivf_shape_ok(nq, n, nlist, nprobe, d, k)) return 0;
    return ir_layout(nq, nlist, nprobe, d, k).total;
}

extern "C" int mivq_ivf_rabitq_search(const float* q, int64_t nq, int32_t d, const float* coarse, int32_t nlist,
                                      const uint32_t* probe_l, int32_t nprobe, const int64_t* offsets,
                                      const uint8_t* list_codes, const uint32_t* list_ids, int32_t qb, int32_t metric,
                                      int32_t k, void* workspace, size_t workspace_bytes, float* dists, uint32_t* ids,
                                      void* stream) {
    const int rc = ivf_search_check("ivf_rabitq_search", nq, d, INT32_MAX, nlist, nprobe, k, metric);
    if (rc != MIVQ_OK) return rc;
    MIVQ_REQUIRE(qb >= 0 && qb <= 8, MIVQ_ERR_UNSUPPORTED, "ivf_rabitq_search: qb=%d not in [0, 8]", qb);
    if (nq == 0) return MIVQ_OK;
    MIVQ_REQUIRE(q && coarse && probe_l && offsets && list_codes && list_ids && dists && ids,
                 MIVQ_ERR_INVALID, "ivf_rabitq_search: null pointer");
    // the MFMA scan: d % 32 == 0 (whole k-steps, 4-B aligned code rows), qb >= 1, the 32 int8 rows in LDS
    const bool mfma = qb > 0 && d % 32 == 0 && reinterpret_cast<uintptr_t>(list_codes) % 4 == 0 &&
                      (size_t)kIrLdsRows + (size_t)kIrPairs * (d + 16) <= 160 * 1024;
    hipStream_t st = as_stream(stream);
    const IvfLayout L = ir_layout(nq, nlist, nprobe, d, k);
    return ivf_probed_search<kIrPairs>(
        "ivf_rabitq_search", L, nq, nlist, nprobe, k, offsets, list_codes, list_ids, workspace, workspace_bytes, dists,
        ids, stream,
        [&](const IvfChunk& c) {
            hipLaunchKernelGGL(ivf_rabitq_prep_kernel, dim3((unsigned)c.pairs), dim3(256), 0, st, q + c.a0 * d, d, coarse,
                               nlist, probe_l + c.a0 * nprobe, nprobe, c.nqc, qb, L.S, k, reinterpret_cast<int8_t*>(c.xa),
                               reinterpret_cast<float*>(c.xb), c.keys, c.scan.pd, c.scan.pi);
            return hipGetLastError();
        },
        [&](const IvfChunk& c, int64_t maxitems) {
            const IrScan A{c.scan, q + c.a0 * d, coarse, reinterpret_cast<const int8_t*>(c.xa),
                           reinterpret_cast<const float*>(c.xb), d, qb, metric};
            return with_topk_regs(k, [&](auto R) { return launch_ir_scan<decltype(R)::value>(mfma, A, maxitems, st); });
        });
}
