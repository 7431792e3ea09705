// rabitq_internal.h — the kernels of the RaBitQ-1 encode and the device code of the estimator's
// query preparation and epilogue, shared by the flat entry points (rabitq.hip, rabitq_search.hip: one
// centre for all rows / queries) and the IVF ones (ivf_rabitq.hip: the centre is the row's list
// centroid / the probed list's centroid).  One body each, so the two callers agree bit for bit.
#pragma once

#include "mivq_common.h"

#include <float.h>
#include <math.h>

namespace mivq {

typedef int rq_v4i __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- encode (one wave per row)
// One wavefront per row: lane L owns byte L, L+64, ... (8 dims each, two 16-B loads), so a
// wave streams 2 KiB of contiguous row data per step; the three sums are wave-reduced.
// PER_ROW: cen is the (nlist, d) coarse table and the row's centre is cen[assign[row]] (the IVF
// encode, ivf_rabitq.hip); otherwise cen is the one centre of all rows, or null (rabitq.hip).
template <bool VEC, bool PER_ROW>
__global__ __launch_bounds__(256) void rabitq_encode_kernel(const float* __restrict__ x, int64_t n, int d,
                                                            const float* __restrict__ cen,
                                                            const uint32_t* __restrict__ assign, int metric,
                                                            uint8_t* __restrict__ codes) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* __restrict__ centroid = PER_ROW ? cen + (int64_t)assign[row] * d : cen;
    const int nb = (d + 7) / 8, cs = nb + 8;
    const float* xr = x + row * d;
    uint8_t* code = codes + row * cs;
    float l2 = 0.0f, orl2 = 0.0f, dp = 0.0f;
    for (int byte = lane; byte < nb; byte += 64) {
        const int j0 = byte * 8;
        float v[8];
        if (VEC && j0 + 8 <= d) {
            const float4 a = *reinterpret_cast<const float4*>(xr + j0);
            const float4 b = *reinterpret_cast<const float4*>(xr + j0 + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = (j0 + u < d) ? xr[j0 + u] : 0.0f;
        }
        uint32_t bits = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (j0 + u >= d) break;
            const float xv = v[u];
            const float rr = centroid ? __fsub_rn(xv, centroid[j0 + u]) : xv;
            l2 = __builtin_fmaf(rr, rr, l2);
            orl2 = __builtin_fmaf(xv, xv, orl2);
            const bool b = rr > 0.0f;
            dp = __fadd_rn(dp, b ? rr : -rr);
            bits |= (uint32_t)b << u;
        }
        code[byte] = (uint8_t)bits;
    }
    l2 = wave_sum(l2);
    orl2 = wave_sum(orl2);
    dp = wave_sum(dp);
    if (lane == 0) {
        const float inv_d_sqrt = d == 0 ? 1.0f : __fdiv_rn(1.0f, sqrtf((float)d));
        const float inv_norm = fabsf(l2) < FLT_EPSILON ? 1.0f : __fdiv_rn(1.0f, sqrtf(l2));
        const float ndp = __fmul_rn(__fmul_rn(dp, inv_norm), inv_d_sqrt);
        const float inv_dp = fabsf(ndp) < FLT_EPSILON ? 1.0f : __fdiv_rn(1.0f, ndp);
        const float f0 = metric == MIVQ_METRIC_INNER_PRODUCT ? __fsub_rn(l2, orl2) : l2;
        const float f1 = __fmul_rn(inv_dp, sqrtf(l2));
        // the trailer is 4-byte aligned only when nb % 4 == 0: write bytes
        const uint32_t u0 = __float_as_uint(f0), u1 = __float_as_uint(f1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            code[nb + q] = (uint8_t)(u0 >> (8 * q));
            code[nb + 4 + q] = (uint8_t)(u1 >> (8 * q));
        }
    }
}

// d % 512 == 0 (every lane owns NI = d / 512 bytes), x and the centroid (every row of the table) 16-B aligned: the same
// per-lane arithmetic in the same order as rabitq_encode_kernel (identical codes and factors),
// with the loads of G of a lane's bytes (x and centroid, 16-B loads) issued before any of them is
// used -- the generic loop waited for each byte's loads before issuing the next byte's (one
// 2 KiB step in flight per wave).  1M x 3072: 2.44 -> 2.33 ms (0.65 -> 0.68 of 8 TB/s,
// profiles/r04_s15).
template <int G, bool PER_ROW>
__global__ __launch_bounds__(256) void rabitq_encode_wide_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                 const float* __restrict__ cen,
                                                                 const uint32_t* __restrict__ assign, int metric,
                                                                 uint8_t* __restrict__ codes) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* __restrict__ centroid = PER_ROW ? cen + (int64_t)assign[row] * d : cen;
    const int nb = d / 8, cs = nb + 8, NI = nb / 64;
    const float* xr = x + row * d;
    uint8_t* code = codes + row * cs;
    const bool has_c = centroid != nullptr;
    float l2 = 0.0f, orl2 = 0.0f, dp = 0.0f;
    for (int i0 = 0; i0 < NI; i0 += G) {
        float4 xv[G][2], cv[G][2];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int j0 = (lane + 64 * (i0 + g)) * 8;
            xv[g][0] = *reinterpret_cast<const float4*>(xr + j0);
            xv[g][1] = *reinterpret_cast<const float4*>(xr + j0 + 4);
            if (has_c) {
                cv[g][0] = *reinterpret_cast<const float4*>(centroid + j0);
                cv[g][1] = *reinterpret_cast<const float4*>(centroid + j0 + 4);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v[8] = {xv[g][0].x, xv[g][0].y, xv[g][0].z, xv[g][0].w,
                                xv[g][1].x, xv[g][1].y, xv[g][1].z, xv[g][1].w};
            const float c[8] = {cv[g][0].x, cv[g][0].y, cv[g][0].z, cv[g][0].w,
                                cv[g][1].x, cv[g][1].y, cv[g][1].z, cv[g][1].w};
            uint32_t bits = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float xu = v[u];
                const float rr = has_c ? __fsub_rn(xu, c[u]) : xu;
                l2 = __builtin_fmaf(rr, rr, l2);
                orl2 = __builtin_fmaf(xu, xu, orl2);
                const bool b = rr > 0.0f;
                dp = __fadd_rn(dp, b ? rr : -rr);
                bits |= (uint32_t)b << u;
            }
            code[lane + 64 * (i0 + g)] = (uint8_t)bits;
        }
    }
    l2 = wave_sum(l2);
    orl2 = wave_sum(orl2);
    dp = wave_sum(dp);
    if (lane == 0) {
        const float inv_d_sqrt = __fdiv_rn(1.0f, sqrtf((float)d));
        const float inv_norm = fabsf(l2) < FLT_EPSILON ? 1.0f : __fdiv_rn(1.0f, sqrtf(l2));
        const float ndp = __fmul_rn(__fmul_rn(dp, inv_norm), inv_d_sqrt);
        const float inv_dp = fabsf(ndp) < FLT_EPSILON ? 1.0f : __fdiv_rn(1.0f, ndp);
        const float f0 = metric == MIVQ_METRIC_INNER_PRODUCT ? __fsub_rn(l2, orl2) : l2;
        const float f1 = __fmul_rn(inv_dp, sqrtf(l2));
        const uint32_t u0 = __float_as_uint(f0), u1 = __float_as_uint(f1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            code[nb + q] = (uint8_t)(u0 >> (8 * q));
            code[nb + 4 + q] = (uint8_t)(u1 >> (8 * q));
        }
    }
}

// ---------------------------------------------------------------- estimator: query preparation
constexpr int kQfStride = 8;  // floats per query: c1, c2, c34, qc, qn, 1/sqrt(d), off, 0

// One workgroup of 256 threads per query row (every thread calls it): r = q - c, its min / max,
// the qb-bit quantised r' (int8, minus 128 when qb = 8) to qq_row, r itself to qr_row when qb = 0
// and qr_row is given, and the factors {c1, c2, c34, ||r||^2, ||q||^2, 1/sqrt(d), off, 0} to qf_row.
__device__ __forceinline__ void rabitq_qprep_row(const float* __restrict__ qrow, int d,
                                                 const float* __restrict__ centroid, int qb,
                                                 int8_t* __restrict__ qq_row, float* __restrict__ qr_row,
                                                 float* __restrict__ qf_row) {
    __shared__ float red_lo[256], red_hi[256];
    __shared__ int red_sum;
    const int tid = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    for (int j = tid; j < d; j += 256) {
        const float r = __fsub_rn(qrow[j], centroid ? centroid[j] : 0.0f);
        lo = fminf(lo, r);
        hi = fmaxf(hi, r);
        if (qb == 0 && qr_row) qr_row[j] = r;
    }
    red_lo[tid] = lo;
    red_hi[tid] = hi;
    if (tid == 0) red_sum = 0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            red_lo[tid] = fminf(red_lo[tid], red_lo[tid + s]);
            red_hi[tid] = fmaxf(red_hi[tid], red_hi[tid + s]);
        }
        __syncthreads();
    }
    const float vmin = red_lo[0], vmax = red_hi[0];
    const float isd = __fdiv_rn(1.0f, sqrtf((float)d));
    float delta = 0.0f;
    const int off = qb == 8 ? 128 : 0;
    if (qb > 0) {
        const int top = (1 << qb) - 1;
        delta = __fdiv_rn(__fsub_rn(vmax, vmin), (float)top);
        const float inv_delta = delta > 0.0f ? __fdiv_rn(1.0f, delta) : 0.0f;
        int part = 0;
        for (int j = tid; j < d; j += 256) {
            const float r = __fsub_rn(qrow[j], centroid ? centroid[j] : 0.0f);
            const float t = __fmul_rn(__fsub_rn(r, vmin), inv_delta);
            int v = (int)floorf(__fadd_rn(t, 0.5f));
            v = v < 0 ? 0 : (v > top ? top : v);
            part += v;
            qq_row[j] = (int8_t)(v - off);
        }
        atomicAdd(&red_sum, part);  // integer: order-free
    }
    __syncthreads();
    if (tid < 64) {
        // the oracle's sequential chains, both in lane 0, over the row staged in LDS 1024
        // elements at a time by the whole wave: the global loads of a piece are in flight at
        // once instead of one round trip per element of a serial loop
        __shared__ __attribute__((aligned(16))) float s_q[1024], s_c[1024];
        float qc = 0.0f, qn = 0.0f;
        for (int j0 = 0; j0 < d; j0 += 1024) {
            const int nj = min(1024, d - j0);
            for (int t = tid; t < nj; t += 64) {
                s_q[t] = qrow[j0 + t];
                s_c[t] = centroid ? centroid[j0 + t] : 0.0f;
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's own LDS stores
            __builtin_amdgcn_wave_barrier();
            if (tid == 0) {  // both chains in lane 0, 16-B LDS reads running ahead of the fmas
                int t = 0;
#pragma unroll 4
                for (; t + 4 <= nj; t += 4) {
                    const float4 qv = *reinterpret_cast<const float4*>(s_q + t);
                    const float4 cv = *reinterpret_cast<const float4*>(s_c + t);
                    float r = __fsub_rn(qv.x, cv.x); qc = __builtin_fmaf(r, r, qc); qn = __builtin_fmaf(qv.x, qv.x, qn);
                    r = __fsub_rn(qv.y, cv.y); qc = __builtin_fmaf(r, r, qc); qn = __builtin_fmaf(qv.y, qv.y, qn);
                    r = __fsub_rn(qv.z, cv.z); qc = __builtin_fmaf(r, r, qc); qn = __builtin_fmaf(qv.z, qv.z, qn);
                    r = __fsub_rn(qv.w, cv.w); qc = __builtin_fmaf(r, r, qc); qn = __builtin_fmaf(qv.w, qv.w, qn);
                }
                for (; t < nj; ++t) {
                    const float r = __fsub_rn(s_q[t], s_c[t]);
                    qc = __builtin_fmaf(r, r, qc);
                    qn = __builtin_fmaf(s_q[t], s_q[t], qn);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        float c1 = 0.0f, c2 = 0.0f, c34 = 0.0f;
        if (qb > 0) {
            c1 = __fmul_rn(__fmul_rn(2.0f, delta), isd);
            c2 = __fmul_rn(__fmul_rn(2.0f, vmin), isd);
            c34 = __fmul_rn(isd, __fadd_rn(__fmul_rn(delta, (float)red_sum), __fmul_rn((float)d, vmin)));
        }
        if (tid == 0) {
            float* f = qf_row;
            f[0] = c1; f[1] = c2; f[2] = c34; f[3] = qc; f[4] = qn; f[5] = isd; f[6] = (float)off; f[7] = 0.0f;
        }
    }
}

// ---------------------------------------------------------------- estimator: epilogue
// The estimator epilogue shared by every kernel (oracle order).
__device__ __forceinline__ float rabitq_key(float fd, float f0, float f1, float qc, float qn, bool ip) {
    const float pre = __builtin_fmaf(__fmul_rn(-2.0f, f1), fd, __fadd_rn(f0, qc));
    return ip ? __fmul_rn(0.5f, __fsub_rn(pre, qn)) : pre;
}

__device__ __forceinline__ float load_f32(const unsigned char* p) {
    uint32_t u = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) u |= (uint32_t)p[b] << (8 * b);
    return __uint_as_float(u);
}

// 16 sign bits -> 16 int8 {0, 1} (the A operand of one v_mfma_i32_32x32x32_i8 k-half):
// nibble * 0x204081 & 0x01010101 spreads four bits over four bytes.
__device__ __forceinline__ rq_v4i rabitq_sign_bytes(uint32_t b16) {
    rq_v4i av;
#pragma unroll
    for (int j = 0; j < 4; ++j) av[j] = (int)(__umul24((b16 >> (4 * j)) & 0xFu, 0x204081u) & 0x01010101u);
    return av;
}

}  // namespace mivq
