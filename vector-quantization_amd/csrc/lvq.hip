// lvq.hip — single-level LVQ (locally-adaptive vector quantization) encode / decode and the
// fp32 column mean of its fit, bit-exact with numpy.
//
// Restates LVQQuantizer.fit / compress / decompress
// (/root/reference/src/haag_vq/methods/lvq_quantization.py:42-142) one fp32 rounding per step
// (the library builds with -ffp-contract=off), L = 2^B - 1, B = nbits in [1, 8]:
//   fit    : mu_t = (x_0t + x_1t + ... in ascending row order, fp32) / (float)n
//   encode : r_t = x_t - mu_t, lo = min r, hi = max r, span = hi - lo,
//            delta = span == 0 ? FLT_MIN : span / L,
//            idx_t = clip((int)rint((r_t - lo) / delta), 0, L)        (rint: half to even)
//   row    : ceil(d B / 8) index bytes (idx_t in bits [t B, (t + 1) B) of the row's bit stream,
//            MSB-first from byte 0, padding bits 0) ++ f32 lo ++ f32 delta (little-endian, at
//            any byte offset: read and written byte-wise)
//   decode : x^_t = (lo + (float)idx_t * delta) + mu_t
//
// Encode layout: one wavefront per row.  Eight consecutive dimensions pack to exactly B bytes,
// so lane l owns the groups of 8 dimensions l, l + 64, ...: 32 contiguous bytes of x in, B
// contiguous bytes out, no bits merged across lanes.  Up to d = 3072 (6 groups per lane) the
// residuals stay in registers between the min/max pass and the quantisation, so x is read
// once; beyond that the row is read a second time (from L2).
#include <algorithm>
#include <float.h>

#include "mivq_common.h"

namespace mivq {
namespace {

constexpr int kLvqMaxRegGroups = 6;  // groups of 8 dims a lane keeps in registers: d <= 3072

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

// 4 rows (waves) per workgroup, grid-stride over rows.  G > 0: the lane's G groups in registers
// (64 * 8 * G >= d), and its part of mu too, loaded once for all the rows the wave walks; G == 0:
// any d, the row (and mu) read twice.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void lvq_encode_kernel(const float* __restrict__ x, int64_t n, int d,
                                                         const float* __restrict__ mu, int B, int sw,
                                                         uint8_t* __restrict__ codes) {
    const int lane = threadIdx.x & 63;
    const int groups = (d + 7) >> 3;
    const int ib = (int)(((int64_t)d * B + 7) >> 3);
    const int64_t cs = (int64_t)ib + 8;
    const float Lf = (float)((1 << B) - 1);
    float m[G > 0 ? G : 1][8];
    if constexpr (G > 0) {
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (lane + 64 * i < groups) lvq_load8<VEC>(mu, d, lane + 64 * i, m[i]);
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
        const float* xr = x + row * d;
        uint8_t* code = codes + row * cs;
        float lo = INFINITY, hi = -INFINITY;
        float r[G > 0 ? G : 1][8];
        if constexpr (G > 0) {
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
        } else {
            for (int g = lane; g < groups; g += 64) {
                lvq_load8<VEC>(xr, d, g, r[0]);
                lvq_load8<VEC>(mu, d, g, m[0]);
#pragma unroll
                for (int u = 0; u < 8; ++u) r[0][u] = __fsub_rn(r[0][u], m[0][u]);
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
                lvq_load8<VEC>(xr, d, g, r[0]);
                lvq_load8<VEC>(mu, d, g, m[0]);
#pragma unroll
                for (int u = 0; u < 8; ++u) r[0][u] = __fsub_rn(r[0][u], m[0][u]);
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
// 16-B stores out (VEC: d % 4 == 0, mu and out 16-B aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void lvq_decode_kernel(const uint8_t* __restrict__ codes, int64_t n, int d,
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
        float o[8];
        float* orow = out + i * d + j0;
        if (VEC && j0 + 8 <= d) {
            const float4 ma = *reinterpret_cast<const float4*>(mu + j0), mb = *reinterpret_cast<const float4*>(mu + j0 + 4);
            const float mv[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t idx = (uint32_t)(v >> (64 - B * (u + 1))) & L;
                o[u] = __fadd_rn(__fadd_rn(lo, __fmul_rn((float)idx, delta)), mv[u]);
            }
            reinterpret_cast<float4*>(orow)[0] = make_float4(o[0], o[1], o[2], o[3]);
            reinterpret_cast<float4*>(orow)[1] = make_float4(o[4], o[5], o[6], o[7]);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (j0 + u < d) {
                    const uint32_t idx = (uint32_t)(v >> (64 - B * (u + 1))) & L;
                    orow[u] = __fadd_rn(__fadd_rn(lo, __fmul_rn((float)idx, delta)), mu[j0 + u]);
                }
            }
        }
    }
}

// mean_c = (fp32 sum of column c in ascending row order) / (float)n, what numpy's
// X.mean(axis=0) computes for a C-contiguous f32 array.  A workgroup owns kCmCols columns:
// all 256 threads load the next kCmRows x kCmCols tile while kCmCols lanes add the current one
// from LDS in row order, so the chain per column stays sequential and the columns spread over
// ceil(d / kCmCols) workgroups.
constexpr int kCmCols = 16, kCmRows = 256;

template <bool VEC>
__global__ __launch_bounds__(256) void column_mean_kernel(const float* __restrict__ x, int64_t n, int d,
                                                          float* __restrict__ mean) {
    __shared__ __attribute__((aligned(16))) float tile[kCmRows][kCmCols];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kCmCols;
    float v[16];
    auto fetch = [&](int64_t r0) __attribute__((always_inline)) {
        if (VEC) {  // d % 4 == 0, x 16-B aligned: 4 threads per row, 64 rows per pass
            const int c = c0 + 4 * (tid & 3);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int64_t row = r0 + (tid >> 2) + 64 * p;
                float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < n && c < d) t = *reinterpret_cast<const float4*>(x + row * d + c);
                v[4 * p] = t.x; v[4 * p + 1] = t.y; v[4 * p + 2] = t.z; v[4 * p + 3] = t.w;
            }
        } else {  // 16 threads per row, 16 rows per pass
            const int c = c0 + (tid & 15);
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const int64_t row = r0 + (tid >> 4) + 16 * p;
                v[p] = (row < n && c < d) ? x[row * d + c] : 0.0f;
            }
        }
    };
    auto stash = [&]() __attribute__((always_inline)) {
        if (VEC) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                *reinterpret_cast<float4*>(&tile[(tid >> 2) + 64 * p][4 * (tid & 3)]) =
                    make_float4(v[4 * p], v[4 * p + 1], v[4 * p + 2], v[4 * p + 3]);
        } else {
#pragma unroll
            for (int p = 0; p < 16; ++p) tile[(tid >> 4) + 16 * p][tid & 15] = v[p];
        }
    };
    float acc = 0.0f;
    fetch(0);
    for (int64_t r0 = 0; r0 < n; r0 += kCmRows) {
        stash();
        __syncthreads();
        if (r0 + kCmRows < n) fetch(r0 + kCmRows);
        if (tid < kCmCols) {
            const int m = (int)min<int64_t>(kCmRows, n - r0);
#pragma unroll 8
            for (int r = 0; r < m; ++r) acc = __fadd_rn(acc, tile[r][tid]);
        }
        __syncthreads();
    }
    if (tid < kCmCols && c0 + tid < d) mean[c0 + tid] = __fdiv_rn(acc, (float)n);
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

template <bool VEC>
void launch_lvq_encode(const float* x, int64_t n, int d, const float* mu, int B, int sw, uint8_t* codes, hipStream_t st) {
    const int per_lane = (int)ceil_div((d + 7) / 8, 64);
    // 32 workgroups per CU at most: a wave walks several rows with its part of mu in registers
    // (and grid.x stays far below its limit for any n)
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n, 4), (int64_t)device_cus() * 32));
#define MIVQ_LVQ_ENC(G) \
    hipLaunchKernelGGL((lvq_encode_kernel<G, VEC>), grid, dim3(256), 0, st, x, n, d, mu, B, sw, codes)
    if (per_lane <= 1) MIVQ_LVQ_ENC(1);
    else if (per_lane == 2) MIVQ_LVQ_ENC(2);
    else if (per_lane == 3) MIVQ_LVQ_ENC(3);
    else if (per_lane == 4) MIVQ_LVQ_ENC(4);
    else if (per_lane <= kLvqMaxRegGroups) MIVQ_LVQ_ENC(kLvqMaxRegGroups);
    else MIVQ_LVQ_ENC(0);
#undef MIVQ_LVQ_ENC
}

int lvq_check(const char* name, int64_t n, int32_t d, int32_t nbits) {
    MIVQ_REQUIRE(n >= 0 && d > 0 && d <= (1 << 27), MIVQ_ERR_INVALID, "%s: bad sizes n=%lld d=%d", name, (long long)n, d);
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "num_bits must be in [1, 8], got %d", nbits);
    return MIVQ_OK;
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_column_mean(const float* x, int64_t n, int32_t d, float* mean, void* stream) {
    MIVQ_REQUIRE(n > 0 && d > 0, MIVQ_ERR_INVALID, "column_mean: bad sizes n=%lld d=%d", (long long)n, d);
    MIVQ_REQUIRE(x && mean, MIVQ_ERR_INVALID, "column_mean: null pointer");
    const dim3 grid((unsigned)ceil_div(d, kCmCols));
    if (d % 4 == 0 && aligned16(x))
        hipLaunchKernelGGL(column_mean_kernel<true>, grid, dim3(256), 0, as_stream(stream), x, n, d, mean);
    else
        hipLaunchKernelGGL(column_mean_kernel<false>, grid, dim3(256), 0, as_stream(stream), x, n, d, mean);
    return check_launch("column_mean");
}

extern "C" int mivq_lvq_encode(const float* x, int64_t n, int32_t d, const float* mu, int32_t nbits, uint8_t* codes,
                               void* stream) {
    const int rc = lvq_check("lvq_encode", n, d, nbits);
    if (rc != MIVQ_OK || n == 0) return rc;
    MIVQ_REQUIRE(x && mu && codes, MIVQ_ERR_INVALID, "lvq_encode: null pointer");
    const int64_t cs = ((int64_t)d * nbits + 7) / 8 + 8;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(codes);
    int sw = 8;  // the widest store every group start of every row is aligned for
    while (sw > 1 && (nbits % sw != 0 || cs % sw != 0 || addr % sw != 0)) sw >>= 1;
    if (d % 4 == 0 && aligned16(x) && aligned16(mu))
        launch_lvq_encode<true>(x, n, d, mu, nbits, sw, codes, as_stream(stream));
    else
        launch_lvq_encode<false>(x, n, d, mu, nbits, sw, codes, as_stream(stream));
    return check_launch("lvq_encode");
}

extern "C" int mivq_lvq_decode(const uint8_t* codes, int64_t n, int32_t d, const float* mu, int32_t nbits, float* out,
                               void* stream) {
    const int rc = lvq_check("lvq_decode", n, d, nbits);
    if (rc != MIVQ_OK || n == 0) return rc;
    MIVQ_REQUIRE(codes && mu && out, MIVQ_ERR_INVALID, "lvq_decode: null pointer");
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n * (int64_t)((d + 7) / 8), 256), 1 << 24));
    if (d % 4 == 0 && aligned16(mu) && aligned16(out))
        hipLaunchKernelGGL(lvq_decode_kernel<true>, grid, dim3(256), 0, as_stream(stream), codes, n, d, mu, nbits, out);
    else
        hipLaunchKernelGGL(lvq_decode_kernel<false>, grid, dim3(256), 0, as_stream(stream), codes, n, d, mu, nbits, out);
    return check_launch("lvq_decode");
}
