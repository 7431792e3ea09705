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
// once; beyond that the row is read a second time (from L2).  The kernels are in
// code_internal.h, shared with the per-list encode / decode of ivf_code.hip.
#include <algorithm>
#include "code_internal.h"

namespace mivq {
namespace {

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

template <bool VEC>
void launch_lvq_encode(const float* x, int64_t n, int d, const float* mu, int B, int sw, uint8_t* codes, hipStream_t st) {
    const int per_lane = (int)ceil_div((d + 7) / 8, 64);
    // 32 workgroups per CU at most: a wave walks several rows with its part of mu in registers
    // (and grid.x stays far below its limit for any n)
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n, 4), (int64_t)device_cus() * 32));
    with_lvq_groups(per_lane, [&](auto G) {
        hipLaunchKernelGGL((lvq_encode_kernel<decltype(G)::value, VEC, false>), grid, dim3(256), 0, st, x, n, d, nullptr,
                           nullptr, mu, B, sw, codes);
    });
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
    const int sw = lvq_store_width(codes, ((int64_t)d * nbits + 7) / 8 + 8, nbits);
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
        hipLaunchKernelGGL((lvq_decode_kernel<true, false>), grid, dim3(256), 0, as_stream(stream), codes, n, d, nullptr, nullptr, mu, nbits, out);
    else
        hipLaunchKernelGGL((lvq_decode_kernel<false, false>), grid, dim3(256), 0, as_stream(stream), codes, n, d, nullptr, nullptr, mu, nbits, out);
    return check_launch("lvq_decode");
}
