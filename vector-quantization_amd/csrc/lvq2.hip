// lvq2.hip — two-level LVQ (LVQ-B1xB2): encode, decode, and the re-ranking of candidate lists on
// both levels (mivq_lvq2_encode, mivq_lvq2_decode, mivq_rerank_lvq2).
//
// Level 1 is lvq.hip's code, byte for byte.  Level 2 quantises what level 1 left over on the
// interval level 1's step fixes, so it stores no constants of its own.  fp32, one rounding per
// step (the library builds with -ffp-contract=off), L1 = 2^B1 - 1, L2 = 2^B2 - 1, B1 in [1, 8],
// B2 in {4, 8}:
//   level 1 : r_t = x_t - mu_t, lo, delta, idx_t as mivq_lvq_encode
//   level 2 : a_t = lo + (float)idx_t * delta, e_t = r_t - a_t, lo2 = -0.5 * delta,
//             delta2 = delta / L2 (IEEE; subnormal for delta = FLT_MIN, and kept),
//             j_t = clip((int)rint((e_t - lo2) / delta2), 0, L2)            (rint: half to even)
//   rows    : codes1 the LVQ row (index stream, lo, delta); codes2 ceil(d B2 / 8) bytes, j_t in
//             bits [t B2, (t + 1) B2) MSB-first from byte 0 (B2 = 4: the even dimension in the
//             high nibble), padding bits 0, no trailer
//   decode  : x^_t = ((lo + (float)idx_t * delta) + (lo2 + (float)j_t * delta2)) + mu_t
//
// Encode is lvq_encode_kernel's layout (one wavefront per row, lane l owns the groups of 8
// dimensions l, l + 64, ...; a group is B1 bytes of codes1 and B2 bytes of codes2), with both
// levels quantised from the residuals in registers: x is read once up to d = 3072, beyond that a
// second time.  B1 and B2 are run-time values there, as B is in lvq_encode_kernel.
//
// Re-rank is rerank_kernel's design (query and mu in LDS, a lane owns one gathered candidate, a
// WaveTopK part per wave, launch_topk_merge).  B1 and B2 are both template parameters of
// rerank_lvq2_kernel (8 x 2 widths x 4 list sizes = 64 instantiations): the field positions of
// both streams are compile-time shifts, as Fmt<>::level's are in the single-level scan.
#include "code_internal.h"
#include "rerank_internal.h"
#include "topk.h"

#include <algorithm>

namespace mivq {
namespace {

__device__ __forceinline__ float lvq2_lo(float delta) { return __fmul_rn(-0.5f, delta); }

// x^_t of the two levels' fields
__device__ __forceinline__ float lvq2_value(uint32_t idx, uint32_t j, float lo, float delta, float lo2, float delta2,
                                            float mu) {
    const float a = __fadd_rn(lo, __fmul_rn((float)idx, delta));
    const float b = __fadd_rn(lo2, __fmul_rn((float)j, delta2));
    return __fadd_rn(__fadd_rn(a, b), mu);
}

// ---------------------------------------------------------------- encode
// Both quotients go by lvq_quotient<true> (code_internal.h, Markstein's correction of a rcp) when
// delta <= 2^50 and delta2 >= 2^-60, by IEEE division otherwise.
//   Level 1: delta >= delta2 >= 2^-60, so lvq_delta_ok(delta) holds and its argument stands.
//   Level 2: the same argument with (delta2, L2) for (delta, L).  delta2 <= delta <= 2^50, rcp2 is
//   normal.  e_t lies within half a step of 0 but for the roundings of a_t and e_t, so
//   a = e_t - lo2 <= delta (1 + 2^-20) < 2^51 and q0 = RN(a rcp2) < 2^9: nothing overflows.  For
//   a >= 2^-62 the residual a - delta2 q0 is a multiple of ulp(delta2) ulp(q0) >= 2^-46 a / 4
//   >= 2^-110, far above the subnormals, so the fma forms it exactly and q is the correctly
//   rounded quotient.  An |a| below 2^-62 is below delta2 / 4, where any q near a / delta2 rounds
//   to 0 (a slightly negative a, from the rounding of a_t, gives -0 and clips to 0).
// Either path returns the correctly rounded quotient, so no byte depends on which one ran.
__device__ __forceinline__ bool lvq2_fast_ok(float delta, float delta2) { return delta <= 0x1p50f && delta2 >= 0x1p-60f; }

// The 8 fields of a group, half[0] the first four, as its B bytes at p (`nbytes` of them for the
// ragged last group): the stores of lvq_emit.  `sw`: every group start of every row is aligned for
// stores of that many bytes (8, 4, 2 or 1), and B is a multiple of it.
__device__ __forceinline__ void lvq2_store_group(const uint32_t (&half)[2], int B, int nbytes, int sw,
                                                 uint8_t* __restrict__ p) {
    const uint64_t acc = ((uint64_t)half[0] << (4 * B)) | half[1];
    // the group's big-endian image, left-aligned, as the little-endian word that stores it
    const uint64_t w = __builtin_bswap64(acc << (64 - 8 * B));
    if (nbytes == B && sw == 8) {
        *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
    } else if (nbytes == B && sw == 4) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)w;
        if (B == 8) *reinterpret_cast<uint32_t*>(p + 4) = (uint32_t)(w >> 32);
    } else if (nbytes == B && sw == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (2 * k < B) *reinterpret_cast<uint16_t*>(p + 2 * k) = (uint16_t)(w >> (16 * k));
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nbytes) p[k] = (uint8_t)(w >> (8 * k));
    }
}

struct Lvq2Row {  // what a wave knows of its row after the min / max pass, the same in every lane
    float lo, delta, rcp, lo2, delta2, rcp2;
};

// Quantises group g on both levels and writes its B1 + B2 bytes.  The elements past d of a ragged
// last group hold a copy of the group's first residual (lvq2_pad): they are quantised like any other
// and their fields cleared afterwards, so no lane condition per element lives across the group.
template <bool FAST>
__device__ __forceinline__ void lvq2_emit(const float (&r)[8], int d, int g, const Lvq2Row& R, int B1, int B2, int ib1,
                                          int ib2, int sw1, int sw2, uint8_t* __restrict__ code1,
                                          uint8_t* __restrict__ code2) {
    const float L1f = (float)((1 << B1) - 1), L2f = (float)((1 << B2) - 1);
    uint32_t h1[2] = {0u, 0u}, h2[2] = {0u, 0u};  // four fields each: 4 B <= 32 bits
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        // clipped before the cast (NaN -> 0): the fields are always in [0, L]
        const float q1 = lvq_quotient<FAST>(__fsub_rn(r[u], R.lo), R.delta, R.rcp);
        const float fi = fminf(fmaxf(rintf(q1), 0.0f), L1f);
        const float a = __fadd_rn(R.lo, __fmul_rn(fi, R.delta));
        const float e = __fsub_rn(r[u], a);
        const float q2 = lvq_quotient<FAST>(__fsub_rn(e, R.lo2), R.delta2, R.rcp2);
        const float fj = fminf(fmaxf(rintf(q2), 0.0f), L2f);
        h1[u >> 2] = (h1[u >> 2] << B1) | (uint32_t)fi;
        h2[u >> 2] = (h2[u >> 2] << B2) | (uint32_t)fj;
    }
    const int pad = 8 - min(8, d - g * 8);  // fields past d: the low pad * B bits of the group
    h1[1] = (uint32_t)(((uint64_t)h1[1] >> (pad * B1)) << (pad * B1));
    h2[1] = (uint32_t)(((uint64_t)h2[1] >> (pad * B2)) << (pad * B2));
    if (pad > 4) {
        h1[0] = (h1[0] >> ((pad - 4) * B1)) << ((pad - 4) * B1);
        h2[0] = (h2[0] >> ((pad - 4) * B2)) << ((pad - 4) * B2);
    }
    lvq2_store_group(h1, B1, min(B1, ib1 - g * B1), sw1, code1 + (int64_t)g * B1);
    lvq2_store_group(h2, B2, min(B2, ib2 - g * B2), sw2, code2 + (int64_t)g * B2);
}

// r[u] = r[0] for the elements past d of group g, and the group's part in the row's min / max.
__device__ __forceinline__ void lvq2_pad_minmax(float (&r)[8], int d, int g, float& lo, float& hi) {
    const int nv = d - g * 8;
#pragma unroll
    for (int u = 1; u < 8; ++u) r[u] = u < nv ? r[u] : r[0];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        lo = fminf(lo, r[u]);
        hi = fmaxf(hi, r[u]);
    }
}

// 4 rows (waves) per workgroup, grid-stride over rows.  G > 0: the lane's G groups and its part
// of mu in registers (64 * 8 * G >= d), mu loaded once for all the rows the wave walks; G == 0:
// any d, the row (and mu) read twice.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void lvq2_encode_kernel(const float* __restrict__ x, int64_t n, int d,
                                                          const float* __restrict__ mu, int B1, int B2, int sw1,
                                                          int sw2, uint8_t* __restrict__ codes1,
                                                          uint8_t* __restrict__ codes2) {
    const int lane = threadIdx.x & 63;
    const int groups = (d + 7) >> 3;
    const int64_t cs1 = (((int64_t)d * B1 + 7) >> 3) + 8, cs2 = ((int64_t)d * B2 + 7) >> 3;
    const float L1f = (float)((1 << B1) - 1), L2f = (float)((1 << B2) - 1);
    float m[G > 0 ? G : 1][8];
    if constexpr (G > 0) {
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (lane + 64 * i < groups) lvq_load8<VEC>(mu, d, lane + 64 * i, m[i]);
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
        const float* xr = x + row * d;
        uint8_t* code1 = codes1 + row * cs1;
        uint8_t* code2 = codes2 + row * cs2;
        // d again, opaque once per row: the lane conditions that depend on the shape alone (g < groups,
        // the ragged group's, which of its stores a group takes) are then formed where they are used.
        // Left row-invariant they are hoisted out of the row loop, two SGPRs each, and spilled (up
        // to 468 at G = 6).
        int dl = d;
        asm volatile("" : "+s"(dl));
        const int gl = (dl + 7) >> 3;
        const int ib1 = (int)(((int64_t)dl * B1 + 7) >> 3), ib2 = (int)(((int64_t)dl * B2 + 7) >> 3);
        float lo = INFINITY, hi = -INFINITY;
        float r[G > 0 ? G : 1][8];
        if constexpr (G > 0) {
#pragma unroll
            for (int i = 0; i < G; ++i)
                if (lane + 64 * i < gl) lvq_load8<VEC>(xr, dl, lane + 64 * i, r[i]);
#pragma unroll
            for (int i = 0; i < G; ++i) {
                if (lane + 64 * i < gl) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) r[i][u] = __fsub_rn(r[i][u], m[i][u]);
                    lvq2_pad_minmax(r[i], dl, lane + 64 * i, lo, hi);
                }
            }
        } else {
            for (int g = lane; g < gl; g += 64) {
                lvq_residual8<VEC, false>(xr, nullptr, mu, dl, g, r[0]);
                lvq2_pad_minmax(r[0], dl, g, lo, hi);
            }
        }
        lo = wave_min(lo);
        hi = wave_max(hi);
        const float span = __fsub_rn(hi, lo);
        Lvq2Row R;
        R.lo = lo;
        R.delta = span == 0.0f ? FLT_MIN : __fdiv_rn(span, L1f);
        R.rcp = __fdiv_rn(1.0f, R.delta);
        R.lo2 = lvq2_lo(R.delta);
        R.delta2 = __fdiv_rn(R.delta, L2f);
        R.rcp2 = __fdiv_rn(1.0f, R.delta2);
        const bool fast = lvq2_fast_ok(R.delta, R.delta2);  // the same in every lane
        if constexpr (G > 0) {
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int g = lane + 64 * i;
                if (g < gl) {
                    if (fast) lvq2_emit<true>(r[i], dl, g, R, B1, B2, ib1, ib2, sw1, sw2, code1, code2);
                    else lvq2_emit<false>(r[i], dl, g, R, B1, B2, ib1, ib2, sw1, sw2, code1, code2);
                }
            }
        } else {
            for (int g = lane; g < gl; g += 64) {
                lvq_residual8<VEC, false>(xr, nullptr, mu, dl, g, r[0]);
                lvq2_pad_minmax(r[0], dl, g, lo, hi);  // (lo and hi are the row's already)
                if (fast) lvq2_emit<true>(r[0], dl, g, R, B1, B2, ib1, ib2, sw1, sw2, code1, code2);
                else lvq2_emit<false>(r[0], dl, g, R, B1, B2, ib1, ib2, sw1, sw2, code1, code2);
            }
        }
        if (lane == 0) {  // the trailer sits at any byte offset
            const uint32_t u0 = __float_as_uint(R.lo), u1 = __float_as_uint(R.delta);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                code1[ib1 + q] = (uint8_t)(u0 >> (8 * q));
                code1[ib1 + 4 + q] = (uint8_t)(u1 >> (8 * q));
            }
        }
    }
}

// ---------------------------------------------------------------- decode
// One lane per group of 8 dimensions: its B1 + B2 bytes and the row's trailer byte-wise in, two
// 16-B stores out (VEC: d % 4 == 0, mu and out 16-B aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void lvq2_decode_kernel(const uint8_t* __restrict__ codes1,
                                                          const uint8_t* __restrict__ codes2, int64_t n, int d,
                                                          const float* __restrict__ mu, int B1, int B2,
                                                          float* __restrict__ out) {
    const int groups = (d + 7) >> 3;
    const int ib1 = (int)(((int64_t)d * B1 + 7) >> 3);
    const int ib2 = (int)(((int64_t)d * B2 + 7) >> 3);
    const int64_t cs1 = (int64_t)ib1 + 8;
    const uint32_t L1 = (1u << B1) - 1u, L2 = (1u << B2) - 1u;
    const int64_t total = n * groups;
    for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256) {
        const int64_t i = gid / groups;
        const int g = (int)(gid - i * groups);
        const int j0 = g * 8;
        const uint8_t* code1 = codes1 + i * cs1;
        const uint8_t* code2 = codes2 + i * (int64_t)ib2;
        const int nb1 = min(B1, ib1 - g * B1), nb2 = min(B2, ib2 - g * B2);
        uint64_t v1 = 0, v2 = 0;  // the group's bits of each level, left-aligned
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < nb1) v1 |= (uint64_t)code1[(int64_t)g * B1 + k] << (56 - 8 * k);
            if (k < nb2) v2 |= (uint64_t)code2[(int64_t)g * B2 + k] << (56 - 8 * k);
        }
        uint32_t u0 = 0, u1 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u0 |= (uint32_t)code1[ib1 + q] << (8 * q);
            u1 |= (uint32_t)code1[ib1 + 4 + q] << (8 * q);
        }
        const float lo = __uint_as_float(u0), delta = __uint_as_float(u1);
        const float lo2 = lvq2_lo(delta), delta2 = __fdiv_rn(delta, (float)L2);
        float mv[8];
        lvq_load8<VEC>(mu, d, g, mv);
        float o[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t idx = (uint32_t)(v1 >> (64 - B1 * (u + 1))) & L1;
            const uint32_t j = (uint32_t)(v2 >> (64 - B2 * (u + 1))) & L2;
            o[u] = lvq2_value(idx, j, lo, delta, lo2, delta2, mv[u]);
        }
        float* orow = out + i * d + j0;
        if (VEC && j0 + 8 <= d) {
            reinterpret_cast<float4*>(orow)[0] = make_float4(o[0], o[1], o[2], o[3]);
            reinterpret_cast<float4*>(orow)[1] = make_float4(o[4], o[5], o[6], o[7]);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + u < d) orow[u] = o[u];
        }
    }
}

// ---------------------------------------------------------------- re-rank
// How a lane reads the words of a unit: kWide whole 8-B (codes1) / 16-B (codes2) loads, k4B
// 4-B loads, kBytes single bytes.  Chosen per array on the host from its base and row stride.
enum : int { kBytes = 0, k4B = 1, kWide = 2 };

// NW little-endian words from p.  WW: words of a wide load (2 or 4), taken when NW is a multiple.
template <int NW, int WW>
__device__ __forceinline__ void lvq2_load_words(const uint8_t* __restrict__ p, int mode, uint32_t (&w)[NW]) {
    if constexpr (NW % WW == 0) {
        if (mode == kWide) {
#pragma unroll
            for (int i = 0; i < NW / WW; ++i) {
                if constexpr (WW == 4) {
                    const uint4 v = reinterpret_cast<const uint4*>(p)[i];
                    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
                } else {
                    const uint2 v = reinterpret_cast<const uint2*>(p)[i];
                    w[2 * i] = v.x; w[2 * i + 1] = v.y;
                }
            }
            return;
        }
    }
    if (mode != kBytes) {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i)
            w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 |
                   (uint32_t)p[4 * i + 3] << 24;
    }
}

// The chain of one candidate against the query in LDS: scan_row's, over the two-level x^_t.
// A unit of 32 dimensions is B1 words of the row in codes1 (byte-swapped, the fields taken by
// Fmt<kLvq + B1 - 1>::level) and B2 words of the row in codes2, read in step; a level-2 field
// never crosses a byte, so its words stay little-endian and are read as SQ-4 / SQ-8 levels (the
// same nibble order).  The dimensions past the last whole unit go one at a time.
template <int B1, int B2>
__device__ __forceinline__ float lvq2_scan_row(const uint8_t* __restrict__ c1, const uint8_t* __restrict__ c2, int d,
                                               const float* qv, const float* mv, int mode1, int mode2, bool l2) {
    using F1 = Fmt<kLvq + B1 - 1>;
    using F2 = Fmt<B2 == 4 ? kSq4 : kSq8>;
    const float2 p = F1::row_scale(c1, d);
    const float lo = p.x, delta = p.y;
    const float lo2 = lvq2_lo(delta), delta2 = __fdiv_rn(delta, (float)((1 << B2) - 1));
    float dist = 0.0f;
    int t = 0;
    for (; t + 32 <= d; t += 32) {
        uint32_t w1[B1], w2[B2];
        lvq2_load_words<B1, 2>(c1 + (t >> 3) * B1, mode1, w1);
        lvq2_load_words<B2, 4>(c2 + (t >> 3) * B2, mode2, w2);
#pragma unroll
        for (int i = 0; i < B1; ++i) w1[i] = __builtin_bswap32(w1[i]);
#pragma unroll
        for (int g = 0; g < 32; g += 4) {
            const float4 m4 = *reinterpret_cast<const float4*>(mv + t + g);
            const float4 qf = *reinterpret_cast<const float4*>(qv + t + g);
            const float x0 = lvq2_value(F1::level(w1, g + 0), F2::level(w2, g + 0), lo, delta, lo2, delta2, m4.x);
            const float x1 = lvq2_value(F1::level(w1, g + 1), F2::level(w2, g + 1), lo, delta, lo2, delta2, m4.y);
            const float x2 = lvq2_value(F1::level(w1, g + 2), F2::level(w2, g + 2), lo, delta, lo2, delta2, m4.z);
            const float x3 = lvq2_value(F1::level(w1, g + 3), F2::level(w2, g + 3), lo, delta, lo2, delta2, m4.w);
            if (l2) {
                float df = __fsub_rn(qf.x, x0); dist = __builtin_fmaf(df, df, dist);
                df = __fsub_rn(qf.y, x1); dist = __builtin_fmaf(df, df, dist);
                df = __fsub_rn(qf.z, x2); dist = __builtin_fmaf(df, df, dist);
                df = __fsub_rn(qf.w, x3); dist = __builtin_fmaf(df, df, dist);
            } else {
                dist = __builtin_fmaf(qf.x, x0, dist);
                dist = __builtin_fmaf(qf.y, x1, dist);
                dist = __builtin_fmaf(qf.z, x2, dist);
                dist = __builtin_fmaf(qf.w, x3, dist);
            }
        }
    }
    for (; t < d; ++t) {  // level_at: codes1 may read the trailer's first byte, codes2 only the field's own byte
        const float xh = lvq2_value(F1::level_at(c1, t), F2::level_at(c2, t), lo, delta, lo2, delta2, mv[t]);
        if (l2) {
            const float df = __fsub_rn(qv[t], xh);
            dist = __builtin_fmaf(df, df, dist);
        } else {
            dist = __builtin_fmaf(qv[t], xh, dist);
        }
    }
    return dist;
}

// rerank_kernel with two stores.  LDS: [dp] query, [dp] mu, dp = d rounded up to 4.  `off`:
// id_offset; a slot is live when off <= id < off + n as unsigned numbers.
template <int B1, int B2, int R>
__global__ __launch_bounds__(kRerankWaves * 64) void rerank_lvq2_kernel(
    const float* __restrict__ q, const uint32_t* __restrict__ cand, int64_t r, const uint8_t* __restrict__ codes1,
    const uint8_t* __restrict__ codes2, int64_t n, int d, const float* __restrict__ mu, int metric, int k, uint32_t off,
    int64_t slice_slots, int mode1, int mode2, float* __restrict__ part_d, uint32_t* __restrict__ part_i) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int dp = (d + 3) & ~3;
    float* qv = smem;
    float* mv = smem + dp;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t qi = blockIdx.x, nq = gridDim.x;
    for (int t = tid; t < d; t += kRerankWaves * 64) {
        qv[t] = q[qi * d + t];
        mv[t] = mu[t];
    }
    __syncthreads();
    WaveTopK<R> top;
    top.init();
    float thr_d = INFINITY;
    uint32_t thr_i = kNoId;
    const bool l2 = metric == MIVQ_METRIC_L2;
    const int64_t stride1 = Fmt<kLvq + B1 - 1>::row_bytes(d);
    const int64_t stride2 = ((int64_t)d * B2 + 7) >> 3;
    const uint32_t* cq = cand + qi * r;
    const int64_t sbeg = (int64_t)blockIdx.y * slice_slots;
    const int64_t send = min(r, sbeg + slice_slots);
    for (int64_t base = sbeg + (int64_t)wv * 64; base < send; base += kRerankWaves * 64) {
        const int64_t slot = base + lane;
        const uint32_t id = slot < send ? cq[slot] : kNoId;
        const uint32_t row = id - off;  // wraps for id < off: then row >= 2^32 - off > n
        const bool valid = slot < send && id >= off && (int64_t)row < n;
        float dist = 0.0f;
        if (valid)
            dist = lvq2_scan_row<B1, B2>(codes1 + (int64_t)row * stride1, codes2 + (int64_t)row * stride2, d, qv, mv,
                                         mode1, mode2, l2);
        float dv = l2 ? dist : -dist;
        if (dv != dv) dv = INFINITY;
        top.offer(valid, dv, id, k, lane, thr_d, thr_i);
    }
    const int64_t part = (int64_t)blockIdx.y * kRerankWaves + wv;
    top.store(part_d + (part * nq + qi) * k, part_i + (part * nq + qi) * k, k, lane);
}

// the widest of the three ways every row start of an array is aligned for
int load_mode(const void* base, int64_t stride, int wide_bytes, bool wide_ok) {
    const LoadModes lm = load_modes(base, stride, wide_bytes);
    return wide_ok && lm.wide ? kWide : lm.narrow ? k4B : kBytes;
}

template <int B1, int B2>
int rerank_lvq2(const float* q, int64_t nq, const uint32_t* cand, int64_t r, const uint8_t* codes1, const uint8_t* codes2,
                int64_t n, int d, const float* mu, int metric, int k, int64_t id_offset, void* workspace, float* dists,
                uint32_t* ids, hipStream_t st) {
    const RerankLayout L = rerank_layout(nq, r, k);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float* pd = reinterpret_cast<float*>(ws + L.pd);
    uint32_t* pi = reinterpret_cast<uint32_t*>(ws + L.pi);
    const size_t smem = (size_t)2 * ((d + 3) & ~3) * sizeof(float);
    const int mode1 = load_mode(codes1, Fmt<kLvq + B1 - 1>::row_bytes(d), 8, B1 % 2 == 0);
    const int mode2 = load_mode(codes2, ((int64_t)d * B2 + 7) / 8, 16, true);
    // whole waves per slice, so that no wave straddles two slices
    const int64_t slice_slots = ceil_div(ceil_div(r, L.S), 64) * 64;
    hipError_t e = with_topk_regs(k, [&](auto R) {
        auto kern = rerank_lvq2_kernel<B1, B2, decltype(R)::value>;
        hipError_t a = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (a != hipSuccess) return a;
        hipLaunchKernelGGL(kern, dim3((unsigned)nq, (unsigned)L.S), dim3(kRerankWaves * 64), smem, st, q, cand, r, codes1,
                           codes2, n, d, mu, metric, k, (uint32_t)id_offset, slice_slots, mode1, mode2, pd, pi);
        return hipGetLastError();
    });
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "rerank_lvq2 (scan): %s", hipGetErrorString(e));
    e = launch_topk_merge(pd, pi, (int)L.parts, nq, k, dists, ids, st);
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "rerank_lvq2 (merge): %s", hipGetErrorString(e));
    return MIVQ_OK;
}

// ---------------------------------------------------------------- host
template <bool VEC>
void launch_lvq2_encode(const float* x, int64_t n, int d, const float* mu, int B1, int B2, uint8_t* codes1,
                        uint8_t* codes2, hipStream_t st) {
    const int per_lane = (int)ceil_div((d + 7) / 8, 64);
    const int sw1 = lvq_store_width(codes1, ((int64_t)d * B1 + 7) / 8 + 8, B1);
    const int sw2 = lvq_store_width(codes2, ((int64_t)d * B2 + 7) / 8, B2);
    // 32 workgroups per CU at most, as launch_lvq_encode
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n, 4), (int64_t)device_cus() * 32));
    // (no G = 1: that instantiation alone spilled 18 SGPRs; at d <= 512 the second group is predicated off)
    with_lvq_groups<2>(per_lane, [&](auto G) {
        hipLaunchKernelGGL((lvq2_encode_kernel<decltype(G)::value, VEC>), grid, dim3(256), 0, st, x, n, d, mu, B1, B2, sw1,
                           sw2, codes1, codes2);
    });
}

int lvq2_bits_check(int32_t nbits1, int32_t nbits2) {
    MIVQ_REQUIRE(nbits1 >= 1 && nbits1 <= 8, MIVQ_ERR_INVALID, "primary num_bits must be in [1, 8], got %d", nbits1);
    MIVQ_REQUIRE(nbits2 == 4 || nbits2 == 8, MIVQ_ERR_UNSUPPORTED, "residual num_bits must be 4 or 8, got %d", nbits2);
    return MIVQ_OK;
}

int lvq2_check(const char* name, int64_t n, int32_t d, int32_t nbits1, int32_t nbits2) {
    MIVQ_REQUIRE(n >= 0 && d > 0 && d <= (1 << 27), MIVQ_ERR_INVALID, "%s: bad sizes n=%lld d=%d", name, (long long)n, d);
    return lvq2_bits_check(nbits1, nbits2);
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_lvq2_encode(const float* x, int64_t n, int32_t d, const float* mu, int32_t nbits1, int32_t nbits2,
                                uint8_t* codes1, uint8_t* codes2, void* stream) {
    const int rc = lvq2_check("lvq2_encode", n, d, nbits1, nbits2);
    if (rc != MIVQ_OK || n == 0) return rc;
    MIVQ_REQUIRE(x && mu && codes1 && codes2, MIVQ_ERR_INVALID, "lvq2_encode: null pointer");
    if (d % 4 == 0 && aligned16(x) && aligned16(mu))
        launch_lvq2_encode<true>(x, n, d, mu, nbits1, nbits2, codes1, codes2, as_stream(stream));
    else
        launch_lvq2_encode<false>(x, n, d, mu, nbits1, nbits2, codes1, codes2, as_stream(stream));
    return check_launch("lvq2_encode");
}

extern "C" int mivq_lvq2_decode(const uint8_t* codes1, const uint8_t* codes2, int64_t n, int32_t d, const float* mu,
                                int32_t nbits1, int32_t nbits2, float* out, void* stream) {
    const int rc = lvq2_check("lvq2_decode", n, d, nbits1, nbits2);
    if (rc != MIVQ_OK || n == 0) return rc;
    MIVQ_REQUIRE(codes1 && codes2 && mu && out, MIVQ_ERR_INVALID, "lvq2_decode: null pointer");
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n * (int64_t)((d + 7) / 8), 256), 1 << 24));
    if (d % 4 == 0 && aligned16(mu) && aligned16(out))
        hipLaunchKernelGGL(lvq2_decode_kernel<true>, grid, dim3(256), 0, as_stream(stream), codes1, codes2, n, d, mu, nbits1,
                           nbits2, out);
    else
        hipLaunchKernelGGL(lvq2_decode_kernel<false>, grid, dim3(256), 0, as_stream(stream), codes1, codes2, n, d, mu, nbits1,
                           nbits2, out);
    return check_launch("lvq2_decode");
}

extern "C" size_t mivq_rerank_lvq2_workspace_bytes(int64_t nq, int64_t r, int32_t k) {
    return rerank_workspace_bytes(nq, r, k);
}

extern "C" int mivq_rerank_lvq2(const float* q, int64_t nq, const uint32_t* cand, int64_t r, const uint8_t* codes1,
                                const uint8_t* codes2, int64_t n, int32_t d, const float* mu, int32_t nbits1,
                                int32_t nbits2, int32_t metric, int32_t k, int64_t id_offset, void* workspace,
                                size_t workspace_bytes, float* dists, uint32_t* ids, void* stream) {
    MIVQ_REQUIRE(nq >= 0 && n >= 0 && r >= 1 && d > 0, MIVQ_ERR_INVALID, "rerank_lvq2: bad sizes");
    int rc = lvq2_bits_check(nbits1, nbits2);
    if (rc != MIVQ_OK) return rc;
    hipStream_t st = as_stream(stream);
    bool done = false;
    rc = rerank_prologue("rerank_lvq2", q, nq, cand, r, n, d, Fmt<kLvq>::kPolicy, metric, k, id_offset, workspace,
                         workspace_bytes, dists, ids, st, &done);
    if (rc != MIVQ_OK || done) return rc;
    MIVQ_REQUIRE(codes1 && codes2 && mu, MIVQ_ERR_INVALID, "rerank_lvq2: null pointer");
    return with_lvq_bits(nbits1, [&](auto F) {
        constexpr int B1 = Fmt<decltype(F)::value>::kB;
        if (nbits2 == 4)
            return rerank_lvq2<B1, 4>(q, nq, cand, r, codes1, codes2, n, d, mu, metric, k, id_offset, workspace, dists, ids, st);
        return rerank_lvq2<B1, 8>(q, nq, cand, r, codes1, codes2, n, d, mu, metric, k, id_offset, workspace, dists, ids, st);
    });
}
