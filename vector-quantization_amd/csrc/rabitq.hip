// rabitq.hip — 1-bit RaBitQ encode / decode (faiss RaBitQuantizer layout).
//
// Restates faiss.RaBitQuantizer.compute_codes / decode as called by RaBitQuantizer
// (/root/reference/src/haag_vq/methods/rabit_quantization.py:20-29); see
// oracle/mivq_oracle.c for the scalar restatement this kernel is tested against.
//   code row = ceil(d/8) sign bytes (bit j = (x_j - c_j) > 0, LSB-first) ++ f32 {l2, mult}
// The sign bits are bit-exact; the two factors are reduced in a different (parallel) order
// than the sequential restatement, so they — and the decoded values — agree within 1e-6
// relative (the contract is 1e-5).
//
// The encode kernels (one wavefront per row) live in rabitq_internal.h, shared with the
// per-row-centroid encode of ivf_rabitq.hip.
#include "mivq_common.h"
#include "rabitq_internal.h"

namespace mivq {
namespace {

// One thread per output float: x_j = (bit - 0.5f) * mult * 2 * (1/sqrt(d)) + c_j.
__global__ void rabitq_decode_kernel(const uint8_t* __restrict__ codes, int64_t n, int d,
                                     const float* __restrict__ centroid, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * (int64_t)d) return;
    const int64_t i = e / d;
    const int j = (int)(e % d);
    const int nb = (d + 7) / 8, cs = nb + 8;
    const uint8_t* code = codes + i * cs;
    uint32_t mu = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) mu |= (uint32_t)code[nb + 4 + q] << (8 * q);
    const float mult = __uint_as_float(mu);
    const float inv_d_sqrt = __fdiv_rn(1.0f, sqrtf((float)d));
    const float bit = ((code[j >> 3] >> (j & 7)) & 1u) ? 1.0f : 0.0f;
    const float a = __fmul_rn(__fsub_rn(bit, 0.5f), mult);
    const float b = __fmul_rn(a, 2.0f);
    const float c = __fmul_rn(b, inv_d_sqrt);
    out[e] = __fadd_rn(c, centroid ? centroid[j] : 0.0f);
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_rabitq_encode(const float* x, int64_t n, int32_t d, const float* centroid, int32_t metric,
                                  uint8_t* codes, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0, MIVQ_ERR_INVALID, "rabitq_encode: bad sizes n=%lld d=%d", (long long)n, d);
    MIVQ_REQUIRE(metric == MIVQ_METRIC_L2 || metric == MIVQ_METRIC_INNER_PRODUCT, MIVQ_ERR_UNSUPPORTED,
                 "RaBitQuantizer supports METRIC_L2 / METRIC_INNER_PRODUCT only, got %d", metric);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(x && codes, MIVQ_ERR_INVALID, "rabitq_encode: null pointer");
    const bool vec = (d % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0);
    const int ni = d / 512;
    const bool wide = vec && d % 512 == 0 && reinterpret_cast<uintptr_t>(centroid) % 16 == 0;
    const dim3 grid((unsigned)ceil_div(n, 4));
    if (wide && ni % 6 == 0)
        hipLaunchKernelGGL((rabitq_encode_wide_kernel<6, false>), grid, dim3(256), 0, as_stream(stream), x, n, d,
                           centroid, nullptr, metric, codes);
    else if (wide && ni % 4 == 0)
        hipLaunchKernelGGL((rabitq_encode_wide_kernel<4, false>), grid, dim3(256), 0, as_stream(stream), x, n, d,
                           centroid, nullptr, metric, codes);
    else if (wide && ni % 3 == 0)
        hipLaunchKernelGGL((rabitq_encode_wide_kernel<3, false>), grid, dim3(256), 0, as_stream(stream), x, n, d,
                           centroid, nullptr, metric, codes);
    else if (wide && ni % 2 == 0)
        hipLaunchKernelGGL((rabitq_encode_wide_kernel<2, false>), grid, dim3(256), 0, as_stream(stream), x, n, d,
                           centroid, nullptr, metric, codes);
    else if (vec)
        hipLaunchKernelGGL((rabitq_encode_kernel<true, false>), dim3((unsigned)ceil_div(n, 4)), dim3(256), 0,
                           as_stream(stream), x, n, d, centroid, nullptr, metric, codes);
    else
        hipLaunchKernelGGL((rabitq_encode_kernel<false, false>), dim3((unsigned)ceil_div(n, 4)), dim3(256), 0,
                           as_stream(stream), x, n, d, centroid, nullptr, metric, codes);
    return check_launch("rabitq_encode");
}

extern "C" int mivq_rabitq_decode(const uint8_t* codes, int64_t n, int32_t d, const float* centroid, float* out,
                                  void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0, MIVQ_ERR_INVALID, "rabitq_decode: bad sizes");
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(codes && out, MIVQ_ERR_INVALID, "rabitq_decode: null pointer");
    hipLaunchKernelGGL(rabitq_decode_kernel, dim3((unsigned)ceil_div(n * (int64_t)d, 256)), dim3(256), 0,
                       as_stream(stream), codes, n, d, centroid, out);
    return check_launch("rabitq_decode");
}
