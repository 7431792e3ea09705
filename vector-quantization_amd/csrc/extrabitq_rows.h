// extrabitq_rows.h — the per-row bodies of the Extended RaBitQ steps, as device functions.
//
// The staged kernels of extrabitq.hip and the fused Hadamard kernels of fht.hip call the same
// bodies, so a fused call and the staged composition give the same bits: the same operations,
// the same reduction order (lane t % 64 owns element t, a sequential chain per lane, then the
// xor tree of wave_sum_d).  All fp64; the file is compiled with -ffp-contract=off.
#pragma once

#include "mivq_common.h"

namespace mivq {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// A row held in memory (global or LDS): slot k of lane `lane` is element lane + 64 k.
struct MemRow {
    double* p;
    int lane;
    __device__ __forceinline__ double get(int k) const { return p[lane + 64 * k]; }
    __device__ __forceinline__ void set(int k, double v) const { p[lane + 64 * k] = v; }
};

// normalize: o = (x - c) / max(||x - c||, 1e-12) into `o` (slots 0 .. nk-1, nk = ceil(d / 64));
// returns ||x - c||.  One wavefront; every lane gets the norm.
template <typename T, typename Row>
__device__ __forceinline__ double erq_normalize_row(const T* __restrict__ x, int d, int nk, const double* __restrict__ c,
                                                    int lane, Row& o) {
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < nk; ++k) {
        const int j = lane + 64 * k;
        if (j < d) {
            const double r = __dsub_rn((double)x[j], c[j]);
            o.set(k, r);
            ss = __fma_rn(r, r, ss);
        }
    }
    ss = wave_sum_d(ss);
    const double nr = sqrt(ss);
    const double inv = fmax(nr, 1e-12);
#pragma unroll
    for (int k = 0; k < nk; ++k)
        if (lane + 64 * k < d) o.set(k, __ddiv_rn(o.get(k), inv));
    return nr;
}

// quantize: s_raw (d fp64, global or LDS) -> one code row.  One wavefront.
__device__ __forceinline__ void erq_quantize_row(const double* s_raw, int d, const double* __restrict__ levels, int nbits,
                                                 double nr, uint8_t* __restrict__ code, int lane) {
    const int L = 1 << nbits;
    const int ib = (d * nbits + 7) / 8;
    const double sq = sqrt((double)d);
    double num = 0.0, den = 0.0;
    // lane owns groups of 8 dims: 8 B-bit indices are exactly nbits whole bytes of the
    // MSB-first stream (np.packbits order), bits past d*nbits stay 0
    const int groups = (d + 7) / 8;
    for (int g = lane; g < groups; g += 64) {
        uint64_t bits = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = g * 8 + u;
            int idx = 0;
            if (j < d) {
                const double s = __dmul_rn(s_raw[j], sq);
                for (int q = 0; q + 1 < L; ++q) {
                    const double mid = __dmul_rn(0.5, __dadd_rn(levels[q], levels[q + 1]));
                    idx += (mid < s) ? 1 : 0;  // searchsorted(side="left")
                }
                const double sh = levels[idx];
                num = __fma_rn(s, sh, num);
                den = __fma_rn(sh, sh, den);
            }
            bits = (bits << nbits) | (uint64_t)idx;
        }
        for (int b = 0; b < nbits; ++b) {
            const int byte = g * nbits + b;
            if (byte < ib) code[byte] = (uint8_t)(bits >> (8 * (nbits - 1 - b)));
        }
    }
    num = wave_sum_d(num);
    den = wave_sum_d(den);
    if (lane == 0) {
        const double t = den > 1e-12 ? __ddiv_rn(num, den) : 1.0;
        const float nf = (float)nr, tf = (float)t;
        const uint32_t u0 = __float_as_uint(nf), u1 = __float_as_uint(tf);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            code[ib + q] = (uint8_t)(u0 >> (8 * q));
            code[ib + 4 + q] = (uint8_t)(u1 >> (8 * q));
        }
    }
}

// the f32 at byte `at` of a code row (the trailer holds nrm at ib, t at ib + 4), as fp64
__device__ __forceinline__ double erq_trailer(const uint8_t* __restrict__ code, int at) {
    uint32_t u = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) u |= (uint32_t)code[at + q] << (8 * q);
    return (double)__uint_as_float(u);
}

// dequantize, element j of a code row: (levels[idx_j] / sqrt(D)) * t
__device__ __forceinline__ double erq_dequantize_elem(const uint8_t* __restrict__ code, int j, int d,
                                                      const double* __restrict__ levels, int nbits, double t) {
    int idx = 0;
    for (int u = 0; u < nbits; ++u) {
        const int gb = j * nbits + u;
        idx = (idx << 1) | ((code[gb >> 3] >> (7 - (gb & 7))) & 1);
    }
    return __dmul_rn(__ddiv_rn(levels[idx], sqrt((double)d)), t);
}

// finish, one element: f32(y * nrm + c)
__device__ __forceinline__ float erq_finish_elem(double y, double nr, double cj) {
    return (float)__dadd_rn(__dmul_rn(y, nr), cj);
}

}  // namespace mivq
