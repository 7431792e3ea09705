// extrabitq.hip — multi-bit ("Extended") RaBitQ encode / decode steps on gfx950.
//
// Restates ExtendedRaBitQuantizer.compress / decompress
// (/root/reference/src/haag_vq/methods/extended_rabitq.py:125-199), all in fp64 like numpy:
//   encode: r = x - c; nrm = ||r||; o = r / max(nrm, 1e-12)                 [normalize]
//           s = (o . P) * sqrt(D)   (the D x D product: mivq_extrabitq_rotate, fp64 MFMA)
//           idx = searchsorted(mid-levels, s) (left); s_hat = levels[idx]
//           t = <s, s_hat> / <s_hat, s_hat>  (1 when the denominator <= 1e-12)
//           row = B-bit idx packed MSB-first (np.packbits) ++ f32 nrm ++ f32 t   [quantize]
//   decode: o_hat = (levels[idx] / sqrt(D)) * t                              [dequantize]
//           x_hat = f32((o_hat . P^T) * nrm + c)                             [finish]
// The two D x D rotations (o . P, o_hat . P^T; extended_rabitq.py:140,196) run on the library's
// fp64 MFMA GEMM, mivq_extrabitq_rotate in gemm_f64.hip; this file holds the per-row steps.
// The per-row bodies are the device functions of extrabitq_rows.h, shared with the fused
// Hadamard-rotation kernels of fht.hip.  One wavefront per row for the reductions (tree order: the factors match numpy to ~1e-15
// relative, the indices are exact except where s lies within rounding of a level midpoint).
#include "extrabitq_rows.h"

namespace mivq {
namespace {

template <typename T>
__global__ __launch_bounds__(256) void erq_normalize_kernel(const T* __restrict__ x, int64_t n, int d,
                                                            const double* __restrict__ c, double* __restrict__ o,
                                                            double* __restrict__ nrm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    MemRow r{o + row * d, lane};
    const double nr = erq_normalize_row(x + row * d, d, (d + 63) / 64, c, lane, r);
    if (lane == 0) nrm[row] = nr;
}

// s_raw: (n, d) = o . P.  One wave per row.
__global__ __launch_bounds__(256) void erq_quantize_kernel(const double* __restrict__ s_raw, int64_t n, int d,
                                                           const double* __restrict__ levels, int nbits,
                                                           const double* __restrict__ nrm, uint8_t* __restrict__ codes) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int cs = (d * nbits + 7) / 8 + 8;
    erq_quantize_row(s_raw + row * d, d, levels, nbits, nrm[row], codes + row * cs, lane);
}

__global__ void erq_dequantize_kernel(const uint8_t* __restrict__ codes, int64_t n, int d,
                                      const double* __restrict__ levels, int nbits, double* __restrict__ o_hat) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * (int64_t)d) return;
    const int ib = (d * nbits + 7) / 8;
    const uint8_t* code = codes + (e / d) * (ib + 8);
    o_hat[e] = erq_dequantize_elem(code, (int)(e % d), d, levels, nbits, erq_trailer(code, ib + 4));
}

__global__ void erq_finish_kernel(const double* __restrict__ y, int64_t n, int d, const uint8_t* __restrict__ codes,
                                  int nbits, const double* __restrict__ c, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * (int64_t)d) return;
    const int ib = (d * nbits + 7) / 8;
    out[e] = erq_finish_elem(y[e], erq_trailer(codes + (e / d) * (ib + 8), ib), c[e % d]);
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_extrabitq_normalize(const void* x, int32_t x_is_f64, int64_t n, int32_t d, const double* centroid,
                                        double* o, double* nrm, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0, MIVQ_ERR_INVALID, "extrabitq_normalize: bad sizes");
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(x && centroid && o && nrm, MIVQ_ERR_INVALID, "extrabitq_normalize: null pointer");
    const dim3 grid((unsigned)ceil_div(n, 4));
    if (x_is_f64)
        hipLaunchKernelGGL(erq_normalize_kernel<double>, grid, dim3(256), 0, as_stream(stream),
                           static_cast<const double*>(x), n, d, centroid, o, nrm);
    else
        hipLaunchKernelGGL(erq_normalize_kernel<float>, grid, dim3(256), 0, as_stream(stream),
                           static_cast<const float*>(x), n, d, centroid, o, nrm);
    return check_launch("extrabitq_normalize");
}

extern "C" int mivq_extrabitq_quantize(const double* s_raw, int64_t n, int32_t d, const double* levels, int32_t nbits,
                                       const double* nrm, uint8_t* codes, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0, MIVQ_ERR_INVALID, "extrabitq_quantize: bad sizes");
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "num_bits must be in [1, 8]");
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(s_raw && levels && nrm && codes, MIVQ_ERR_INVALID, "extrabitq_quantize: null pointer");
    hipLaunchKernelGGL(erq_quantize_kernel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, as_stream(stream), s_raw, n,
                       d, levels, nbits, nrm, codes);
    return check_launch("extrabitq_quantize");
}

extern "C" int mivq_extrabitq_dequantize(const uint8_t* codes, int64_t n, int32_t d, const double* levels,
                                         int32_t nbits, double* o_hat, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0 && nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "extrabitq_dequantize: bad args");
    if (n == 0) return MIVQ_OK;
    hipLaunchKernelGGL(erq_dequantize_kernel, dim3((unsigned)ceil_div(n * (int64_t)d, 256)), dim3(256), 0,
                       as_stream(stream), codes, n, d, levels, nbits, o_hat);
    return check_launch("extrabitq_dequantize");
}

extern "C" int mivq_extrabitq_finish(const double* y, int64_t n, int32_t d, const uint8_t* codes, int32_t nbits,
                                     const double* centroid, float* out, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0 && nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "extrabitq_finish: bad args");
    if (n == 0) return MIVQ_OK;
    hipLaunchKernelGGL(erq_finish_kernel, dim3((unsigned)ceil_div(n * (int64_t)d, 256)), dim3(256), 0,
                       as_stream(stream), y, n, d, codes, nbits, centroid, out);
    return check_launch("extrabitq_finish");
}
