// code_internal.h — what the SQ / LVQ code paths share: the row formats of the exact searches
// (exact_search.hip over a flat database, ivf_code.hip over probed lists), the scan of one code
// row against the queries in LDS, and the SQ / LVQ encode and decode kernels, which sq.hip and
// lvq.hip launch with one parameter row for the database and ivf_code.hip with the parameter
// rows and the centroid of each row's list (PER_ROW, the pattern of rabitq_internal.h).  Host side:
// the dispatch from a run-time code width to a format (with_sq_bits / with_lvq_bits /
// with_erq_bits), the load modes of a code array, and the G and store width of an LVQ encode.
#pragma once

#include "mivq_common.h"

#include <float.h>

#include <type_traits>

namespace mivq {

// kLvq + B - 1 is LVQ with B bits per dimension, B = 1 .. 8; kF32 is the database itself;
// kErq + B - 1 is Extended RaBitQ with B bits per dimension, in the rotated domain
enum : int { kSq4 = 0, kSq8 = 1, kSq16 = 2, kRbq = 3, kLvq = 4, kF32 = 12, kErq = 13 };

constexpr int kErqTableBytes = 256 * 8;  // the 2^B level table of a workgroup, at B = 8

// Queries per scan workgroup: the queries and the `params` parameter rows of dp = d rounded up
// to 4 floats share the LDS, within `lds_kib` at 8, 4 or 2 queries and 160 KiB at one, less
// the `table` bytes a format keeps there besides.
struct ScanPolicy {
    int params;
    int lds_kib;
    bool narrow;  // no wider than the batch (search_layout)
    int table = 0;
};

// Queries per scan workgroup under policy P, before narrowing; 0: d does not fit the LDS.
inline int scan_qb(int d, ScanPolicy P) {
    const int64_t per = (int64_t)((d + 3) & ~3) * 4;
    const int64_t budget = (int64_t)P.lds_kib * 1024 - P.table;
    if (per * (8 + P.params) <= budget) return 8;
    if (per * (4 + P.params) <= budget) return 4;
    if (per * (2 + P.params) <= budget) return 2;
    if (per * (1 + P.params) <= 160 * 1024 - P.table) return 1;
    return 0;
}

// ---------------------------------------------------------------- row formats
template <int FMT>
struct Fmt {
    static constexpr bool kIsLvq = FMT >= kLvq && FMT < kLvq + 8;
    static constexpr bool kIsErq = FMT >= kErq && FMT < kErq + 8;
    // LVQ and Extended RaBitQ rows are the same stream: ceil(d kB / 8) bytes of MSB-first kB-bit
    // fields, then a trailer of two f32 (LVQ {lo, delta}, Extended RaBitQ {nrm, t})
    static constexpr bool kIsStream = kIsLvq || kIsErq;
    static constexpr int kB = kIsLvq ? FMT - kLvq + 1 : kIsErq ? FMT - kErq + 1 : 0;  // bits per dimension
    static constexpr uint32_t kMask = (1u << kB) - 1u;
    // dims per 32-bit word of codes (a stream: per unit of kB words)
    static constexpr int kWordDims = FMT == kSq4 ? 8 : FMT == kSq8 ? 4 : FMT == kSq16 ? 2 : FMT == kF32 ? 1 : 32;
    // words per wide load of the scan (16 B; 8 B for RaBitQ and the streams, whose rows of d % 64 == 0
    // are 8-B aligned: the 8-byte trailer follows a multiple of 8 code bytes)
    static constexpr int kWideWords = FMT == kRbq || kIsStream ? 2 : 4;
    // per-dimension parameter arrays: SQ {den, lo}, RaBitQ {centroid}, LVQ {mu}, f32 and
    // Extended RaBitQ none (its one table of 2^kB levels is shared by all dimensions)
    static constexpr int kParams = FMT == kF32 || kIsErq ? 0 : FMT == kRbq || kIsLvq ? 1 : 2;
    // The f32 scan keeps the launch policy it had as a kernel of its own: 96 KiB where the code
    // formats take 128, and a query block that is not narrowed to the batch.  The difference is
    // inherited, not measured: nobody has timed either format under the other's policy.
    static constexpr ScanPolicy kPolicy = {kParams, FMT == kF32 ? 96 : 128, FMT != kF32, kIsErq ? kErqTableBytes : 0};
    static constexpr float kLevels = FMT == kSq4 ? 15.0f : FMT == kSq8 ? 255.0f : 65535.0f;
    static constexpr float kRcpLevels = 1.0f / kLevels;  // RN(1 / L)

    __host__ __device__ static int code_bytes(int d) {
        if (kIsStream) return (int)(((int64_t)d * kB + 7) / 8);
        return FMT == kSq4 ? (d + 1) / 2 : FMT == kSq8 ? d : FMT == kSq16 ? 2 * d : FMT == kF32 ? 4 * d : (d + 7) / 8;
    }
    __host__ __device__ static int row_bytes(int d) { return code_bytes(d) + (FMT == kRbq || kIsStream ? 8 : 0); }
    // byte offset of dimension t (a multiple of kWordDims) in a row
    __device__ static int byte_of(int t) {
        return FMT == kSq4 ? t >> 1 : FMT == kSq8 ? t : FMT == kSq16 ? 2 * t : FMT == kF32 ? 4 * t : t >> 3;
    }

    // level (SQ) / sign bit (RaBitQ) / float bits (f32) of dimension u of the little-endian words w[]
    template <int NW>
    __device__ __forceinline__ static uint32_t level(const uint32_t (&w)[NW], int u) {
        if (kIsStream) {  // w[]: the unit's words byte-swapped, field u at bits [u kB, (u + 1) kB) from the top
            const int o = u * kB, wi = o >> 5, end = (o & 31) + kB;
            if (end <= 32) return (w[wi] >> (32 - end)) & kMask;
            return ((w[wi] << (end - 32)) | (w[wi + 1 < NW ? wi + 1 : wi] >> (64 - end))) & kMask;
        }
        if (FMT == kF32) return w[u];
        if (FMT == kSq8) return (w[u >> 2] >> (8 * (u & 3))) & 0xFFu;
        if (FMT == kSq16) return (w[u >> 1] >> (16 * (u & 1))) & 0xFFFFu;
        if (FMT == kSq4) {  // even dimension in the high nibble
            const uint32_t b = (w[u >> 3] >> (8 * ((u >> 1) & 3))) & 0xFFu;
            return (u & 1) ? (b & 0x0Fu) : (b >> 4);
        }
        return (w[u >> 5] >> (u & 31)) & 1u;
    }
    // the same for dimension t of row `cr`, one code element at a time
    __device__ __forceinline__ static uint32_t level_at(const uint8_t* cr, int t) {
        if (kIsStream) {  // the field lies in two bytes at most (the byte after the last is the trailer's)
            const int o = t * kB, fb = o >> 3;
            const uint32_t v = (uint32_t)cr[fb] << 8 | cr[fb + 1];
            return (v >> (16 - (o & 7) - kB)) & kMask;
        }
        if (FMT == kF32) return reinterpret_cast<const uint32_t*>(cr)[t];
        if (FMT == kSq8) return cr[t];
        if (FMT == kSq16) return reinterpret_cast<const uint16_t*>(cr)[t];
        if (FMT == kSq4) {
            const uint32_t b = cr[t >> 1];
            return (t & 1) ? (b & 0x0Fu) : (b >> 4);
        }
        return (cr[t >> 3] >> (t & 7)) & 1u;
    }
    // x^_t.  SQ: a = den_t, b = lo_t, fadd(fmul(fdiv(level, L), den_t), lo_t) with the division as
    // the reciprocal sequence of div_rn_rcp (RN(level / L) for every level 0 .. L).
    // RaBitQ: a = c_t (0 without a centroid), p.x the row's fmul(fmul(fmul(0.5, mult), 2), 1/sqrt(d)).
    // LVQ: a = mu_t, p = the row's {lo, delta}: fadd(fadd(lo, fmul(idx, delta)), mu_t).
    // f32: the word is x_t.
    // Extended RaBitQ: tab[l] = ddiv(levels[l], sqrt(d)), p = the row's {nrm, t}:
    // (float)dmul(dmul(tab[idx], t), nrm), the level erq_dequantize_kernel writes times nrm.
    __device__ __forceinline__ static float dequant(uint32_t lv, float a, float b, float2 p,
                                                    const double* tab = nullptr) {
        if (FMT == kF32) return __uint_as_float(lv);
        if (kIsErq) {
            // The empty asm keeps the first products of a group of four in program order.  Left
            // free, the scheduler holds all four f64 pairs at once, and the scan at 4 list
            // registers and 8 queries (128 VGPRs allowed) spilled 8 / 16 bytes at B = 3 / 7.
            double v = __dmul_rn(tab[lv], (double)p.y);
            asm volatile("" : "+v"(v));
            return (float)__dmul_rn(v, (double)p.x);
        }
        if (kIsLvq) return __fadd_rn(__fadd_rn(p.x, __fmul_rn((float)lv, p.y)), a);
        if (FMT == kRbq) return __fadd_rn(lv ? p.x : -p.x, a);
        const float f = (float)lv;
        const float q0 = __fmul_rn(f, kRcpLevels);
        const float e = __builtin_fmaf(-q0, kLevels, f);
        const float s = __builtin_fmaf(e, kRcpLevels, q0);
        return __fadd_rn(__fmul_rn(s, a), b);
    }
    // The row's own parameters from its trailer (read byte-wise: rows are unaligned).  RaBitQ: p
    // in .x, from mult, the second trailer float; LVQ: {lo, delta}, Extended RaBitQ: {nrm, t}, the
    // two trailer floats.
    __device__ __forceinline__ static float2 row_scale(const uint8_t* cr, int d) {
        if (FMT != kRbq && !kIsStream) return make_float2(0.0f, 0.0f);
        const int nb = code_bytes(d);
        uint32_t u0 = 0, u1 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (kIsStream) u0 |= (uint32_t)cr[nb + q] << (8 * q);
            u1 |= (uint32_t)cr[nb + 4 + q] << (8 * q);
        }
        if (kIsStream) return make_float2(__uint_as_float(u0), __uint_as_float(u1));
        const float inv_d_sqrt = __fdiv_rn(1.0f, sqrtf((float)d));
        return make_float2(__fmul_rn(__fmul_rn(__fmul_rn(0.5f, __uint_as_float(u1)), 2.0f), inv_d_sqrt), 0.0f);
    }
};

// ---------------------------------------------------------------- host side: format dispatch
// f(std::integral_constant<int, FMT>) for the format of a code width the caller has checked, so
// that an entry point names its template once (the pattern of with_topk_regs): LVQ and Extended
// RaBitQ at nbits = 1 .. 8, SQ at 4 / 8 / 16.
template <int BASE, typename F>
auto with_stream_bits(int nbits, F&& f) {
    switch (nbits) {
        case 1: return f(std::integral_constant<int, BASE + 0>{});
        case 2: return f(std::integral_constant<int, BASE + 1>{});
        case 3: return f(std::integral_constant<int, BASE + 2>{});
        case 4: return f(std::integral_constant<int, BASE + 3>{});
        case 5: return f(std::integral_constant<int, BASE + 4>{});
        case 6: return f(std::integral_constant<int, BASE + 5>{});
        case 7: return f(std::integral_constant<int, BASE + 6>{});
        default: return f(std::integral_constant<int, BASE + 7>{});
    }
}
template <typename F>
auto with_lvq_bits(int nbits, F&& f) { return with_stream_bits<kLvq>(nbits, f); }
template <typename F>
auto with_erq_bits(int nbits, F&& f) { return with_stream_bits<kErq>(nbits, f); }
template <typename F>
auto with_sq_bits(int nbits, F&& f) {
    switch (nbits) {
        case 4: return f(std::integral_constant<int, kSq4>{});
        case 8: return f(std::integral_constant<int, kSq8>{});
        default: return f(std::integral_constant<int, kSq16>{});
    }
}

// SQ-16 codes are read and written as uint16: MIVQ_OK, or the error of `name`.
inline int sq16_aligned(const char* name, int nbits, const void* codes) {
    MIVQ_REQUIRE(nbits != 16 || reinterpret_cast<uintptr_t>(codes) % 2 == 0, MIVQ_ERR_INVALID,
                 "%s: 16-bit codes must be 2-byte aligned", name);
    return MIVQ_OK;
}

// How scan_row may load the rows of an array: `wide` when every row start is aligned for loads
// of wide_bytes, `narrow` for 4-byte loads.
struct LoadModes {
    int wide, narrow;
};
inline LoadModes load_modes(const void* base, int64_t row_bytes, int wide_bytes) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(base);
    return {addr % wide_bytes == 0 && row_bytes % wide_bytes == 0, addr % 4 == 0 && row_bytes % 4 == 0};
}
template <int FMT>
LoadModes code_load_modes(const void* base, int d) {
    return load_modes(base, Fmt<FMT>::row_bytes(d), Fmt<FMT>::kWideWords * 4);
}

// ---------------------------------------------------------------- one row against QB queries
// Where a workgroup's LDS rows are: [QB][dp] queries at qv, the parameter rows pa (SQ den /
// RaBitQ centroid / LVQ mu) and pb (SQ lo), and with CENT the row pc that is added to every
// reconstruction (the list's centroid: x^_t = dequant + pc_t, one more fadd); tab: the
// Extended RaBitQ level table (Fmt<>::dequant).
struct ScanRows {
    const float* qv;
    const float* pa;
    const float* pb;
    const float* pc;
    int dp;
    const double* tab = nullptr;
};

template <int FMT, bool CENT>
__device__ __forceinline__ float scan_value(uint32_t lv, float a, float b, float c, float2 p, const double* tab) {
    const float x = Fmt<FMT>::dequant(lv, a, b, p, tab);
    if constexpr (CENT) return __fadd_rn(x, c);
    return x;
}

// NW loaded words = NW * kWordDims (a multiple of 4) dimensions from t0 (a multiple of 4) on:
// four at a time, the parameters and the queries as 16-B LDS reads.  LVQ: the kB byte-swapped
// words of one unit, 32 dimensions; Extended RaBitQ the same.
template <int FMT, int NW, int QB, bool CENT>
__device__ __forceinline__ void scan_words(const uint32_t (&w)[NW], int t0, const ScanRows& S, float2 p, bool l2,
                                           float (&dist)[QB]) {
    constexpr int ND = Fmt<FMT>::kIsStream ? 32 : NW * Fmt<FMT>::kWordDims;
    static_assert(ND % 4 == 0, "whole groups of four dimensions");
#pragma unroll
    for (int g = 0; g < ND; g += 4) {
        float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f), b4 = a4, c4 = a4;
        if constexpr (Fmt<FMT>::kParams >= 1) a4 = *reinterpret_cast<const float4*>(S.pa + t0 + g);
        if constexpr (Fmt<FMT>::kParams == 2) b4 = *reinterpret_cast<const float4*>(S.pb + t0 + g);
        if constexpr (CENT) c4 = *reinterpret_cast<const float4*>(S.pc + t0 + g);
        const float x0 = scan_value<FMT, CENT>(Fmt<FMT>::level(w, g + 0), a4.x, b4.x, c4.x, p, S.tab);
        const float x1 = scan_value<FMT, CENT>(Fmt<FMT>::level(w, g + 1), a4.y, b4.y, c4.y, p, S.tab);
        const float x2 = scan_value<FMT, CENT>(Fmt<FMT>::level(w, g + 2), a4.z, b4.z, c4.z, p, S.tab);
        const float x3 = scan_value<FMT, CENT>(Fmt<FMT>::level(w, g + 3), a4.w, b4.w, c4.w, p, S.tab);
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            const float4 qf = *reinterpret_cast<const float4*>(S.qv + qq * S.dp + t0 + g);
            if (l2) {
                float df = __fsub_rn(qf.x, x0); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                df = __fsub_rn(qf.y, x1); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                df = __fsub_rn(qf.z, x2); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
                df = __fsub_rn(qf.w, x3); dist[qq] = __builtin_fmaf(df, df, dist[qq]);
            } else {
                dist[qq] = __builtin_fmaf(qf.x, x0, dist[qq]);
                dist[qq] = __builtin_fmaf(qf.y, x1, dist[qq]);
                dist[qq] = __builtin_fmaf(qf.z, x2, dist[qq]);
                dist[qq] = __builtin_fmaf(qf.w, x3, dist[qq]);
            }
        }
    }
}

// The chains of code row `cr` against the QB queries, into dist[] (zeroed by the caller).  The
// row is read once: with 16-B (RaBitQ, LVQ: 8-B) loads while whole loads fit and every row start
// is that aligned (`wide`), then 4-B loads (`narrow`), then single code elements (the tail, and
// every row of an unaligned database).  A stream row (LVQ, Extended RaBitQ) is MSB-first B-bit
// fields: 32 dimensions are B whole words, read as one unit, byte-swapped, the fields that cross
// a word funnel-shifted.
template <int FMT, int QB, bool CENT>
__device__ __forceinline__ void scan_row(const uint8_t* cr, int d, const ScanRows& S, int wide, int narrow, bool l2,
                                         float (&dist)[QB]) {
    using F = Fmt<FMT>;
    constexpr int NDW = F::kWideWords * F::kWordDims;
    const int twide = wide ? d / NDW * NDW : 0;  // dimensions covered by whole wide loads
    const float2 p = F::row_scale(cr, d);
    int t = 0;
    if constexpr (F::kIsStream) {
        // whole units of 32 dimensions = kB words: 8-B loads (even kB, 8-B aligned rows) or
        // 4-B loads; the rest of the row, and every row of an unaligned database, below
        constexpr int B = F::kB;
        const int tunit = narrow ? d / 32 * 32 : 0;
        for (; t < tunit; t += 32) {
            uint32_t w[B];
            const uint8_t* cu = cr + (t >> 3) * B;
            if (B % 2 == 0 && wide) {
#pragma unroll
                for (int i = 0; i < B / 2; ++i) {
                    const uint2 v = reinterpret_cast<const uint2*>(cu)[i];
                    w[2 * i] = v.x;
                    w[2 * i + (B > 1 ? 1 : 0)] = v.y;
                }
            } else {
#pragma unroll
                for (int i = 0; i < B; ++i) w[i] = reinterpret_cast<const uint32_t*>(cu)[i];
            }
#pragma unroll
            for (int i = 0; i < B; ++i) w[i] = __builtin_bswap32(w[i]);
            scan_words<FMT, B, QB, CENT>(w, t, S, p, l2, dist);
        }
    } else {
        for (; t < twide; t += NDW) {
            uint32_t w[F::kWideWords];
            if constexpr (F::kWideWords == 4) {
                const uint4 v = *reinterpret_cast<const uint4*>(cr + F::byte_of(t));
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
                const uint2 v = *reinterpret_cast<const uint2*>(cr + F::byte_of(t));
                w[0] = v.x; w[1] = v.y;
            }
            scan_words<FMT, F::kWideWords, QB, CENT>(w, t, S, p, l2, dist);
        }
        if constexpr (F::kWordDims % 4 == 0) {  // (an SQ-16 word is half a group: no 4-B step)
            if (narrow) {
                for (; t + F::kWordDims <= d; t += F::kWordDims) {
                    const uint32_t w[1] = {*reinterpret_cast<const uint32_t*>(cr + F::byte_of(t))};
                    scan_words<FMT, 1, QB, CENT>(w, t, S, p, l2, dist);
                }
            }
        }
    }
    for (; t < d; ++t) {
        const float xh = scan_value<FMT, CENT>(F::level_at(cr, t), F::kParams >= 1 ? S.pa[t] : 0.0f,
                                               F::kParams == 2 ? S.pb[t] : 0.0f, CENT ? S.pc[t] : 0.0f, p, S.tab);
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            if (l2) {
                const float df = __fsub_rn(S.qv[qq * S.dp + t], xh);
                dist[qq] = __builtin_fmaf(df, df, dist[qq]);
            } else {
                dist[qq] = __builtin_fmaf(S.qv[qq * S.dp + t], xh, dist[qq]);
            }
        }
    }
}

// ---------------------------------------------------------------- SQ encode / decode (generic path)
template <typename T>
__device__ __forceinline__ uint32_t np_cast_uint(T r) {
    if (!(r >= (T)-2147483648.0 && r < (T)2147483648.0)) return 0u;
    return (uint32_t)(int32_t)r;
}

__device__ __forceinline__ float sq_step(float x, float lo, float den, float L) {
    const float a = __fsub_rn(x, lo);
    const float b = __fdiv_rn(a, den);
    return rintf(__fmul_rn(b, L));
}
__device__ __forceinline__ double sq_step(double x, double lo, double den, double L) {
    const double a = __dsub_rn(x, lo);
    const double b = __ddiv_rn(a, den);
    return rint(__dmul_rn(b, L));
}

// Each thread: row i, dims [8g, 8g+8).  Output written as bytes / u16.  PER_ROW (f32): the row
// quantised is x_i - coarse[assign[i]], with row assign[i] of lo / den ((nlist, d) arrays).
template <typename T, bool PER_ROW>
__global__ void sq_encode_kernel(const T* __restrict__ x, int64_t n, int d, const T* __restrict__ coarse,
                                 const uint32_t* __restrict__ assign, const T* __restrict__ lo,
                                 const T* __restrict__ den, int nbits, void* __restrict__ codes) {
    const int groups = (d + 7) / 8;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n * groups) return;
    const int64_t i = gid / groups;
    const int j0 = (int)(gid % groups) * 8;
    const int64_t po = PER_ROW ? (int64_t)assign[i] * d : 0;  // the row's parameter row
    const T L = (T)((1 << nbits) - 1);
    uint32_t q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int j = j0 + u;
        if (j < d) {
            T v = x[i * d + j];
            if constexpr (PER_ROW) v = __fsub_rn(v, coarse[po + j]);
            q[u] = np_cast_uint(sq_step(v, lo[po + j], den[po + j], L));
        } else {
            q[u] = 0u;
        }
    }
    if (nbits == 8) {
        uint8_t* o = static_cast<uint8_t*>(codes) + i * d + j0;
#pragma unroll
        for (int u = 0; u < 8; ++u) if (j0 + u < d) o[u] = (uint8_t)q[u];
    } else if (nbits == 16) {
        uint16_t* o = static_cast<uint16_t*>(codes) + i * d + j0;
#pragma unroll
        for (int u = 0; u < 8; ++u) if (j0 + u < d) o[u] = (uint16_t)q[u];
    } else {  // 4-bit: (q[:,0::2] << 4) | q[:,1::2] in uint8 arithmetic, odd d zero-padded
        const int cw = (d + 1) / 2;
        uint8_t* o = static_cast<uint8_t*>(codes) + i * cw + j0 / 2;
#pragma unroll
        for (int u = 0; u < 8; u += 2)
            if ((j0 + u) / 2 < cw) o[u / 2] = (uint8_t)(((uint8_t)q[u] << 4) | (uint8_t)q[u + 1]);
    }
}

__device__ __forceinline__ float sq_level(const void* codes, int64_t i, int j, int d, int nbits) {
    if (nbits == 16) return (float)static_cast<const uint16_t*>(codes)[i * d + j];
    if (nbits == 8) return (float)static_cast<const uint8_t*>(codes)[i * d + j];
    const uint8_t b = static_cast<const uint8_t*>(codes)[i * ((d + 1) / 2) + (j >> 1)];
    return (float)((j & 1) ? (b & 0x0F) : (b >> 4));
}

// PER_ROW (f32): row assign[i] of lo / den, and coarse[assign[i]] added to the decoded value.
template <typename T, bool PER_ROW>
__global__ void sq_decode_kernel(const void* __restrict__ codes, int64_t n, int d, const T* __restrict__ coarse,
                                 const uint32_t* __restrict__ assign, const T* __restrict__ lo,
                                 const T* __restrict__ den, int nbits, T* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * (int64_t)d) return;
    const int64_t i = e / d;
    const int j = (int)(e % d);
    const int64_t po = PER_ROW ? (int64_t)assign[i] * d : 0;
    const float L = (float)((1 << nbits) - 1);
    const float s = __fdiv_rn(sq_level(codes, i, j, d, nbits), L);
    if constexpr (sizeof(T) == 4) {
        const float v = __fadd_rn(__fmul_rn(s, den[po + j]), lo[po + j]);
        if constexpr (PER_ROW) out[e] = __fadd_rn(v, coarse[po + j]);
        else out[e] = v;
    } else {
        out[e] = __dadd_rn(__dmul_rn((double)s, den[j]), lo[j]);
    }
}

// ---------------------------------------------------------------- LVQ encode / decode
constexpr int kLvqMaxRegGroups = 6;  // groups of 8 dims a lane keeps in registers: d <= 3072

// Host side: f(std::integral_constant<int, G>) for the G of an LVQ encode kernel whose lanes hold
// per_lane groups each: per_lane itself up to 4 (MIN_G at the least: a smaller row leaves the
// other groups predicated off), kLvqMaxRegGroups up to that, 0 (the row read twice) beyond.
template <int MIN_G = 1, typename F>
void with_lvq_groups(int per_lane, F&& f) {
    if constexpr (MIN_G <= 1) {
        if (per_lane <= 1) return f(std::integral_constant<int, 1>{});
    }
    if (per_lane <= 2) return f(std::integral_constant<int, 2>{});
    if (per_lane == 3) return f(std::integral_constant<int, 3>{});
    if (per_lane == 4) return f(std::integral_constant<int, 4>{});
    if (per_lane <= kLvqMaxRegGroups) return f(std::integral_constant<int, kLvqMaxRegGroups>{});
    return f(std::integral_constant<int, 0>{});
}

// The widest store (8, 4, 2 or 1 bytes) every group start of every row of an array of B-bit
// codes is aligned for (lvq_emit's `sw`).
inline int lvq_store_width(const void* base, int64_t row_bytes, int B) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(base);
    int sw = 8;
    while (sw > 1 && (B % sw != 0 || row_bytes % sw != 0 || addr % sw != 0)) sw >>= 1;
    return sw;
}

// rint((r - lo) / delta) needs the correctly rounded quotient only where it can land on or next
// to a tie.  With rcp = RN(1 / delta): q0 = RN(a rcp), the exact residual e = a - delta q0 (one
// fma), q = RN(q0 + e rcp) is the correctly rounded a / delta (Markstein; sq.hip's div_rn_rcp)
// as long as nothing over- or underflows.  A row takes this path when its delta lies in
// [2^-60, 2^50]: then a = r - lo <= L delta < 2^58, and an a below 2^-62 is below delta / 4, where
// any q near a / delta rounds to index 0.  Other rows (delta = FLT_MIN among them) divide in IEEE.
__device__ __forceinline__ bool lvq_delta_ok(float delta) { return delta >= 0x1p-60f && delta <= 0x1p50f; }

template <bool FAST>
__device__ __forceinline__ float lvq_quotient(float a, float delta, float rcp) {
    if (FAST) {
        const float q0 = __fmul_rn(a, rcp);
        const float e = __builtin_fmaf(-q0, delta, a);
        return __builtin_fmaf(e, rcp, q0);
    }
    return __fdiv_rn(a, delta);
}

// v[u] = p[8 g + u], 0 beyond d (VEC: d % 4 == 0 and p 16-B aligned)
template <bool VEC>
__device__ __forceinline__ void lvq_load8(const float* __restrict__ p, int d, int g, float (&v)[8]) {
    const int j0 = g * 8;
    if (VEC && j0 + 8 <= d) {
        const float4 a = *reinterpret_cast<const float4*>(p + j0), b = *reinterpret_cast<const float4*>(p + j0 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (j0 + u < d) ? p[j0 + u] : 0.0f;
    }
}

__device__ __forceinline__ void lvq_minmax(const float (&r)[8], int d, int g, float& lo, float& hi) {
    const int nv = min(8, d - g * 8);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (u < nv) {
            lo = fminf(lo, r[u]);
            hi = fmaxf(hi, r[u]);
        }
    }
}

// Quantises group g and writes its bytes: B of them, fewer for the ragged last group.  `sw`:
// every group start of every row is aligned for stores of that many bytes (8, 4, 2 or 1), and
// B is a multiple of it.
template <bool FAST>
__device__ __forceinline__ void lvq_emit(const float (&r)[8], int d, int g, float lo, float delta, float rcp, int B,
                                         int ib, int sw, uint8_t* __restrict__ code) {
    const float Lf = (float)((1 << B) - 1);
    const int nv = min(8, d - g * 8);
    uint32_t half[2] = {0u, 0u};  // four indices each: 4 B <= 32 bits
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float q = lvq_quotient<FAST>(__fsub_rn(r[u], lo), delta, rcp);
        // clipped before the cast (NaN -> 0): the index is always in [0, L]
        const uint32_t idx = u < nv ? (uint32_t)fminf(fmaxf(rintf(q), 0.0f), Lf) : 0u;
        half[u >> 2] = (half[u >> 2] << B) | idx;
    }
    const uint64_t acc = ((uint64_t)half[0] << (4 * B)) | half[1];
    // the group's big-endian image, left-aligned, as the little-endian word that stores it
    const uint64_t w = __builtin_bswap64(acc << (64 - 8 * B));
    const int nbytes = min(B, ib - g * B);
    uint8_t* p = code + (int64_t)g * B;
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

// The residual of group g of a row.  !PER_ROW: r = x - mu.  PER_ROW: r = (x - c) - mu with c
// and mu the rows of the row's list, two roundings.
template <bool VEC, bool PER_ROW>
__device__ __forceinline__ void lvq_residual8(const float* __restrict__ xr, const float* __restrict__ cr,
                                              const float* __restrict__ mr, int d, int g, float (&r)[8]) {
    float m[8];
    lvq_load8<VEC>(xr, d, g, r);
    lvq_load8<VEC>(mr, d, g, m);
    if constexpr (PER_ROW) {
        float c[8];
        lvq_load8<VEC>(cr, d, g, c);
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = __fsub_rn(r[u], c[u]);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) r[u] = __fsub_rn(r[u], m[u]);
}

// 4 rows (waves) per workgroup, grid-stride over rows.  G > 0: the lane's G groups in registers
// (64 * 8 * G >= d), and (!PER_ROW) its part of mu too, loaded once for all the rows the wave
// walks; G == 0: any d, the row (and mu) read twice.  PER_ROW: mu is (nlist, d), the row's is
// row assign[row], and coarse[assign[row]] is subtracted first.
template <int G, bool VEC, bool PER_ROW>
__global__ __launch_bounds__(256) void lvq_encode_kernel(const float* __restrict__ x, int64_t n, int d,
                                                         const float* __restrict__ coarse,
                                                         const uint32_t* __restrict__ assign,
                                                         const float* __restrict__ mu, int B, int sw,
                                                         uint8_t* __restrict__ codes) {
    const int lane = threadIdx.x & 63;
    const int groups = (d + 7) >> 3;
    const int ib = (int)(((int64_t)d * B + 7) >> 3);
    const int64_t cs = (int64_t)ib + 8;
    const float Lf = (float)((1 << B) - 1);
    float m[G > 0 && !PER_ROW ? G : 1][8];
    if constexpr (G > 0 && !PER_ROW) {
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (lane + 64 * i < groups) lvq_load8<VEC>(mu, d, lane + 64 * i, m[i]);
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
        const float* xr = x + row * d;
        const int64_t po = PER_ROW ? (int64_t)assign[row] * d : 0;
        const float* mr = mu + po;
        const float* cr = PER_ROW ? coarse + po : nullptr;
        uint8_t* code = codes + row * cs;
        float lo = INFINITY, hi = -INFINITY;
        float r[G > 0 ? G : 1][8];
        if constexpr (G > 0 && !PER_ROW) {
#pragma unroll
            for (int i = 0; i < G; ++i)
                if (lane + 64 * i < groups) lvq_load8<VEC>(xr, d, lane + 64 * i, r[i]);
#pragma unroll
            for (int i = 0; i < G; ++i) {
                if (lane + 64 * i < groups) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) r[i][u] = __fsub_rn(r[i][u], m[i][u]);
                    lvq_minmax(r[i], d, lane + 64 * i, lo, hi);
                }
            }
        } else if constexpr (G > 0) {
#pragma unroll
            for (int i = 0; i < G; ++i) {
                if (lane + 64 * i < groups) {
                    lvq_residual8<VEC, true>(xr, cr, mr, d, lane + 64 * i, r[i]);
                    lvq_minmax(r[i], d, lane + 64 * i, lo, hi);
                }
            }
        } else {
            for (int g = lane; g < groups; g += 64) {
                lvq_residual8<VEC, PER_ROW>(xr, cr, mr, d, g, r[0]);
                lvq_minmax(r[0], d, g, lo, hi);
            }
        }
        lo = wave_min(lo);
        hi = wave_max(hi);
        const float span = __fsub_rn(hi, lo);
        const float delta = span == 0.0f ? FLT_MIN : __fdiv_rn(span, Lf);
        const float rcp = __fdiv_rn(1.0f, delta);
        const bool fast = lvq_delta_ok(delta);  // the same in every lane
        if constexpr (G > 0) {
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int g = lane + 64 * i;
                if (g < groups) {
                    if (fast) lvq_emit<true>(r[i], d, g, lo, delta, rcp, B, ib, sw, code);
                    else lvq_emit<false>(r[i], d, g, lo, delta, rcp, B, ib, sw, code);
                }
            }
        } else {
            for (int g = lane; g < groups; g += 64) {
                lvq_residual8<VEC, PER_ROW>(xr, cr, mr, d, g, r[0]);
                if (fast) lvq_emit<true>(r[0], d, g, lo, delta, rcp, B, ib, sw, code);
                else lvq_emit<false>(r[0], d, g, lo, delta, rcp, B, ib, sw, code);
            }
        }
        if (lane == 0) {  // the trailer sits at any byte offset
            const uint32_t u0 = __float_as_uint(lo), u1 = __float_as_uint(delta);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                code[ib + q] = (uint8_t)(u0 >> (8 * q));
                code[ib + 4 + q] = (uint8_t)(u1 >> (8 * q));
            }
        }
    }
}

// One lane per group of 8 dimensions: its B bytes and the row's trailer byte-wise in, two
// 16-B stores out (VEC: d % 4 == 0, mu (PER_ROW: and coarse) and out 16-B aligned).  PER_ROW:
// mu is row assign[i] of (nlist, d), and coarse[assign[i]] is added to the decoded value.
template <bool VEC, bool PER_ROW>
__global__ __launch_bounds__(256) void lvq_decode_kernel(const uint8_t* __restrict__ codes, int64_t n, int d,
                                                         const float* __restrict__ coarse,
                                                         const uint32_t* __restrict__ assign,
                                                         const float* __restrict__ mu, int B, float* __restrict__ out) {
    const int groups = (d + 7) >> 3;
    const int ib = (int)(((int64_t)d * B + 7) >> 3);
    const int64_t cs = (int64_t)ib + 8;
    const uint32_t L = (1u << B) - 1u;
    const int64_t total = n * groups;
    for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256) {
        const int64_t i = gid / groups;
        const int g = (int)(gid - i * groups);
        const int j0 = g * 8;
        const uint8_t* code = codes + i * cs;
        const int64_t po = PER_ROW ? (int64_t)assign[i] * d : 0;
        const int nbytes = min(B, ib - g * B);
        uint64_t v = 0;  // the group's bits, left-aligned
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nbytes) v |= (uint64_t)code[(int64_t)g * B + k] << (56 - 8 * k);
        uint32_t u0 = 0, u1 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u0 |= (uint32_t)code[ib + q] << (8 * q);
            u1 |= (uint32_t)code[ib + 4 + q] << (8 * q);
        }
        const float lo = __uint_as_float(u0), delta = __uint_as_float(u1);
        float mv[8], cv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        lvq_load8<VEC>(mu + po, d, g, mv);
        if constexpr (PER_ROW) lvq_load8<VEC>(coarse + po, d, g, cv);
        float o[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t idx = (uint32_t)(v >> (64 - B * (u + 1))) & L;
            o[u] = __fadd_rn(__fadd_rn(lo, __fmul_rn((float)idx, delta)), mv[u]);
            if constexpr (PER_ROW) o[u] = __fadd_rn(o[u], cv[u]);
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

}  // namespace mivq
