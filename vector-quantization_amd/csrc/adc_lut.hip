// adc_lut.hip — per-query ADC lookup tables on gfx950: lut[q][m][code] = the canonical
// distance term of query q's sub-vector m to centroid (m, code) (order in include/mivq.h).
//   adc_lut_pk_kernel  ksub = 256, dsub % 4 == 0, aligned codebook: packed fp32, no LDS.
//   adc_lut_kernel     every other shape: one block per (subspace, 16 queries), one lane
//                      per centroid.
#include "mivq_common.h"

namespace mivq {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));  // native vector: HIP's float4 struct copies can defeat SROA
typedef float float2v __attribute__((ext_vector_type(2)));

// L2: lut[q][m][k] = fmaf chain over t of (q_t - c_t)^2;  IP: -(fmaf chain of q_t * c_t)
// grid (M, ceil(nq / kLutQ)), block 256: thread = centroid k of subspace m, looping over a
// block of kLutQ queries whose sub-vectors sit in LDS (broadcast reads).  The centroid row
// is read 4 floats at a time and every query's chain advances over those 4 dims in order,
// so each (query, k) chain is the canonical sequential one.  Stores are coalesced along k.
// 16 queries per workgroup (round 5: 57 -> 46 us for 1000 queries at M = 16 against 32 -- twice
// the workgroups to spread over the CUs; 8: 50 us; profiles/r05_s24)
constexpr int kLutQ = 16;

__global__ __launch_bounds__(256) void adc_lut_kernel(const float* __restrict__ q, int64_t nq, int d, int M, int ksub,
                                                       int dsub, const float* __restrict__ C, int metric,
                                                       int vec16, float* __restrict__ lut) {
    extern __shared__ __attribute__((aligned(16))) float qs[];  // [kLutQ][dsub]
    const int m = blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * kLutQ;
    const int nqb = (int)min<int64_t>(kLutQ, nq - q0);
    for (int e = threadIdx.x; e < nqb * dsub; e += blockDim.x) {
        const int qq = e / dsub, t = e - qq * dsub;
        qs[e] = q[(q0 + qq) * d + (int64_t)m * dsub + t];
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= ksub) return;
    const float* c = C + ((int64_t)m * ksub + k) * dsub;
    float acc[kLutQ];
#pragma unroll
    for (int qq = 0; qq < kLutQ; ++qq) acc[qq] = 0.0f;
    const bool l2 = metric == MIVQ_METRIC_L2;
    auto step = [&](float c0, float c1, float c2, float c3, int t0, int nt) __attribute__((always_inline)) {
#pragma unroll
        for (int qq = 0; qq < kLutQ; ++qq) {
            const float* qr = qs + qq * dsub + t0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float cj = j == 0 ? c0 : j == 1 ? c1 : j == 2 ? c2 : c3;
                if (j < nt) {
                    if (l2) {
                        const float df = __fsub_rn(qr[j], cj);
                        acc[qq] = __builtin_fmaf(df, df, acc[qq]);
                    } else {
                        acc[qq] = __builtin_fmaf(qr[j], cj, acc[qq]);
                    }
                }
            }
        }
    };
    if (vec16) {  // dsub % 4 == 0 and C 16-B aligned (host-side test: views may start anywhere)
        // 16-B loads of the centroid row, the next one in flight while this one is used.  (Round
        // 2 replaced these by dword loads while chasing a two-stream mismatch in lanes 48..63;
        // the cause was the LDS-DMA OPQ GEMM on the other stream corrupting packed-fp32 results,
        // since removed from the library: DESIGN §8.  The load form was never involved.)
        v4f cur = *reinterpret_cast<const v4f*>(c);
        for (int t0 = 0; t0 < dsub; t0 += 4) {
            const v4f nxt = (t0 + 4 < dsub) ? *reinterpret_cast<const v4f*>(c + t0 + 4) : cur;
            step(cur.x, cur.y, cur.z, cur.w, t0, 4);
            cur = nxt;
        }
    } else {
        for (int t0 = 0; t0 < dsub; t0 += 4) {
            const int nt = min(4, dsub - t0);
            const float c0 = c[t0], c1 = nt > 1 ? c[t0 + 1] : 0.0f;
            const float c2 = nt > 2 ? c[t0 + 2] : 0.0f, c3 = nt > 3 ? c[t0 + 3] : 0.0f;
            step(c0, c1, c2, c3, t0, nt);
        }
    }
#pragma unroll
    for (int qq = 0; qq < kLutQ; ++qq)
        if (qq < nqb) lut[((q0 + qq) * M + m) * ksub + k] = l2 ? acc[qq] : -acc[qq];
}

// ksub = 256, dsub % 4 == 0, C 16-B aligned (round 6): packed fp32.  Grid (M, ceil(nq / 8)),
// block 128: thread k takes centroids k and k + 128 as the two halves of v_pk_add_f32 /
// v_pk_fma_f32 (both chains exactly the scalar ones: the same sub, then fma, over t ascending),
// and the 8 queries' values come through the scalar cache as the broadcast operand -- no LDS,
// so no packed instruction reads an LDS-loaded register.  Half the VALU of the
// scalar kernel, and no LDS reads at all.
constexpr int kLutPkQ = 8;
template <bool L2, int DS>
__global__ __launch_bounds__(128) void adc_lut_pk_kernel(const float* __restrict__ q, int64_t nq, int d, int M,
                                                          int dsub, const float* __restrict__ C,
                                                          float* __restrict__ lut) {
    const int m = blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * kLutPkQ;
    const int nqb = (int)min<int64_t>(kLutPkQ, nq - q0);
    const int k = threadIdx.x;
    const float* ca = C + ((int64_t)m * 256 + k) * dsub;
    const float* cb = ca + (int64_t)128 * dsub;
    const float* qr[kLutPkQ];
#pragma unroll
    for (int qq = 0; qq < kLutPkQ; ++qq) qr[qq] = q + (q0 + min(qq, nqb - 1)) * d + (int64_t)m * dsub;  // in range
    float2v acc[kLutPkQ];
#pragma unroll
    for (int qq = 0; qq < kLutPkQ; ++qq) acc[qq] = (float2v){0.0f, 0.0f};
    auto body = [&](const v4f& a, const v4f& b, int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2v cc = {a[j], b[j]};
#pragma unroll
            for (int qq = 0; qq < kLutPkQ; ++qq) {
                const float qv = qr[qq][t0 + j];
                const float2v qq2 = {qv, qv};
                if constexpr (L2) {
                    const float2v df = qq2 - cc;
                    acc[qq] = __builtin_elementwise_fma(df, df, acc[qq]);
                } else {
                    acc[qq] = __builtin_elementwise_fma(qq2, cc, acc[qq]);
                }
            }
        }
    };
    if constexpr (DS > 0) {
        // compile-time dsub: both centroid rows are loaded up front (DS / 2 16-B loads per thread,
        // all in flight at once) and consumed in order as they land, instead of one 16-B step
        // ahead with a wait at every loop latch
        // (a window of W steps ahead instead spills: the scheduler hoists every load regardless)
        v4f ra[DS / 4], rb[DS / 4];
#pragma unroll
        for (int i = 0; i < DS / 4; ++i) {
            ra[i] = *reinterpret_cast<const v4f*>(ca + 4 * i);
            rb[i] = *reinterpret_cast<const v4f*>(cb + 4 * i);
        }
#pragma unroll
        for (int i = 0; i < DS / 4; ++i) body(ra[i], rb[i], 4 * i);
    } else {
    v4f a = *reinterpret_cast<const v4f*>(ca), b = *reinterpret_cast<const v4f*>(cb);
    for (int t0 = 0; t0 < dsub; t0 += 4) {
        const bool more = t0 + 4 < dsub;
        const v4f an = more ? *reinterpret_cast<const v4f*>(ca + t0 + 4) : a;
        const v4f bn = more ? *reinterpret_cast<const v4f*>(cb + t0 + 4) : b;
        body(a, b, t0);
        a = an;
        b = bn;
    }
    }
#pragma unroll
    for (int qq = 0; qq < kLutPkQ; ++qq) {
        if (qq < nqb) {
            float* o = lut + ((q0 + qq) * M + m) * 256;
            o[k] = L2 ? acc[qq].x : -acc[qq].x;
            o[k + 128] = L2 ? acc[qq].y : -acc[qq].y;
        }
    }
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_adc_lut(const float* q, int64_t nq, int32_t d, int32_t M, int32_t nbits,
                            const float* centroids, int32_t metric, float* lut, void* stream) {
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED,
                 "adc_lut: metric %d", metric);
    MIVQ_REQUIRE(nq >= 0 && M > 0 && d > 0 && d % M == 0, MIVQ_ERR_INVALID, "adc_lut: bad sizes");
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_UNSUPPORTED, "adc_lut: nbits=%d", nbits);
    if (nq == 0) return MIVQ_OK;
    MIVQ_REQUIRE(q && centroids && lut, MIVQ_ERR_INVALID, "adc_lut: null pointer");
    const int ksub = 1 << nbits;
    if (ksub == 256 && (d / M) % 4 == 0 && reinterpret_cast<uintptr_t>(centroids) % 16 == 0) {
        const dim3 grid((unsigned)M, (unsigned)ceil_div(nq, kLutPkQ));
        const int ds = d / M;
        // compile-time dsub for the benchmarked shapes (round 6, profiles/r06_s36; bit-exact tests, r06_s37):
        // 1000 queries, dsub 96 35.5 -> 34 us, 10,000 queries dsub 64 224 -> 197 us, dsub 48
        // 33.5 -> 26.5 us
        const int dsk = ds == 48 || ds == 64 || ds == 96 ? ds : 0;
#define MIVQ_LUT_GO(L2V, DSV)                                                                                  \
    hipLaunchKernelGGL((adc_lut_pk_kernel<L2V, DSV>), grid, dim3(128), 0, as_stream(stream), q, nq, d, M, ds, \
                       centroids, lut)
        const bool l2 = metric == MIVQ_METRIC_L2;
        switch (dsk) {
            case 48: if (l2) MIVQ_LUT_GO(true, 48); else MIVQ_LUT_GO(false, 48); break;
            case 64: if (l2) MIVQ_LUT_GO(true, 64); else MIVQ_LUT_GO(false, 64); break;
            case 96: if (l2) MIVQ_LUT_GO(true, 96); else MIVQ_LUT_GO(false, 96); break;
            default: if (l2) MIVQ_LUT_GO(true, 0); else MIVQ_LUT_GO(false, 0); break;
        }
#undef MIVQ_LUT_GO
        return check_launch("adc_lut");
    }
    const size_t smem = (size_t)kLutQ * (d / M) * sizeof(float);
    MIVQ_REQUIRE(smem <= 64 * 1024, MIVQ_ERR_UNSUPPORTED, "adc_lut: dsub=%d too large", d / M);
    hipLaunchKernelGGL(adc_lut_kernel, dim3((unsigned)M, (unsigned)ceil_div(nq, kLutQ)), dim3(256), smem,
                       as_stream(stream), q, nq, d, M, ksub, d / M, centroids, metric,
                       (d / M) % 4 == 0 && reinterpret_cast<uintptr_t>(centroids) % 16 == 0 ? 1 : 0, lut);
    return check_launch("adc_lut");
}
