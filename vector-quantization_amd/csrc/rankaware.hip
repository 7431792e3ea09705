// rankaware.hip — the per-row steps of RankAwareQuantizer.compress / decompress on gfx950.
//
// The quantizer (PCA rotation, a different number of bits per rotated dimension, a Gaussian-
// optimal level table per dimension scaled by sqrt(var_d)) is, per row and all in fp64 like numpy:
//   encode: xc = x - mu                                                       [center]
//           y  = xc . V              (mivq_extrabitq_rotate, the fp64 MFMA GEMM of gemm_f64.hip)
//           idx_d = searchsorted(mid-levels of dimension d, y_d), side left
//           row = the idx_d as width_d-bit fields, MSB first, at bit pos_d     [quantize]
//   decode: y_hat_d = levels_d[idx_d]                                          [dequantize]
//           z  = y_hat . V^T         (mivq_extrabitq_rotate, transpose 1)
//           x_hat = f32(z + mu)                                                [finish]
// The format is four tables: lv (all level tables, concatenated), lv_off (d + 1 starts), width
// (bits per dimension, 0..8) and pos (bit position of each field's MSB in the row, MSB-first).
// Dense packing (fields back to back) and FFD packing (fields whole inside bytes, in another
// order) differ only in pos, so one kernel pair serves both.
//
// quantize: a workgroup owns kQRows consecutive rows.  y arrives in chunks of kQDims dimensions,
// loaded coalesced and transposed through LDS so that in the search a lane is a ROW: the 32 lanes
// of a half-wave walk ONE dimension's level table (step 1 reads one address, step s at most
// 2^(s-1)), instead of 64 lanes walking 64 tables (64 cache lines per load instruction: that
// version ran at 0.05 of HBM, profiles/rankaware_ab_run1.log).  Fields are OR-ed into a zeroed
// LDS image of the rows' codes (32-bit LDS atomics, row pitch an odd number of words so the lanes
// of a half-wave hit 32 banks) and the image leaves as coalesced dword stores: no byte is
// scattered to global memory and no global atomic is used.
// dequantize: lane = dimension; the rows' codes are staged in LDS with the global layout
// (16-byte loads), every field is one 16-bit window read.
#include "mivq_common.h"

namespace mivq {
namespace {

constexpr int kRaThreads = 256;
constexpr int kRaRows = 16;          // rows per workgroup of dequantize (16 | tile bytes)
constexpr int kRaLdsBytes = 64 * 1024;
constexpr int kRaMaxCode = 48000;    // longest code row both kernels hold in LDS
constexpr int kQRows = 32;           // quantize: rows per workgroup = lanes of a half-wave
constexpr int kQDims = 64;           // quantize: dimensions per chunk of y
constexpr int kQPitch = kQRows + 1;  // tile[dim][row] pitch in doubles
constexpr int kQTileWords = kQDims * kQPitch * 2;
constexpr int kEwRows = 8;           // rows per workgroup of center / finish

typedef unsigned int ra_u32x4 __attribute__((ext_vector_type(4)));
typedef float ra_f32x4 __attribute__((ext_vector_type(4)));
typedef double ra_f64x2 __attribute__((ext_vector_type(2)));

struct RaField {
    int w;      // bits, 0 when the dimension has no field (or its table entry is out of range)
    int byte;   // first byte of the field in the row
    int sh;     // right shift that takes the field out of the 16-bit big-endian window at `byte`
    int off;    // start of the dimension's levels in lv
};

// A field outside [0, 8 * cs) or wider than 8 bits is treated as width 0: no table can make a
// thread touch LDS outside its row (the Python side refuses such tables before they get here).
__device__ __forceinline__ RaField ra_field(int j, const int32_t* __restrict__ lv_off,
                                            const int32_t* __restrict__ pos, const int32_t* __restrict__ width,
                                            int cs) {
    RaField f;
    const int w = width[j], p = pos[j];
    const bool ok = w > 0 && w <= 8 && p >= 0 && p <= 8 * cs - w;
    f.w = ok ? w : 0;
    f.byte = ok ? (p >> 3) : 0;
    f.sh = ok ? 16 - w - (p & 7) : 0;
    f.off = lv_off[j];
    return f;
}

// Image row pitch in 32-bit words: covers cs bytes, odd.
__host__ __device__ inline int ra_pitch_words(int cs) { return ((cs + 3) >> 2) | 1; }

// The search is idx = #{ q : 0.5 (L[q] + L[q + 1]) < y } over the 2^w - 1 mid-levels, i.e.
// np.searchsorted(side="left"), by bisection.  !(y <= mid) is (mid < y) for numbers and true for
// a NaN y, which numpy sorts past every number.  Four dimensions of a thread step together so
// that four table reads are in flight.
__global__ __launch_bounds__(kRaThreads) void ra_quantize_kernel(const double* __restrict__ y, int64_t n, int d,
                                                                 const double* __restrict__ lv,
                                                                 const int32_t* __restrict__ lv_off,
                                                                 const int32_t* __restrict__ pos,
                                                                 const int32_t* __restrict__ width, int cs, int rows_per,
                                                                 uint8_t* __restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ra_lds[];
    double* tile = reinterpret_cast<double*>(ra_lds);     // [kQDims][kQPitch]
    uint32_t* img = ra_lds + kQTileWords;                 // [rows][pw]
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per;
    const int rows = (int)(n - r0 < rows_per ? n - r0 : rows_per);
    const int pw = ra_pitch_words(cs);
    for (int i = tid; i < rows * pw; i += kRaThreads) img[i] = 0u;

    // loader: thread t takes column t & 63 of rows (t >> 6) + 4 u of the chunk (a wave reads 512
    // contiguous bytes of one row); searcher: row t & 31, dimensions (t >> 5) + 8 u of the chunk
    const double* yt = y + r0 * d;
    const int lc = tid & 63, lr = tid >> 6;
    const int row = tid & 31, slot = tid >> 5;
    double v[8];
    auto gload = [&](int j0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = lr + 4 * u;
            v[u] = (r < rows && j0 + lc < d) ? yt[(int64_t)r * d + j0 + lc] : 0.0;
        }
    };
    gload(0);
    for (int j0 = 0; j0 < d; j0 += kQDims) {
        __syncthreads();   // the previous chunk is searched (first trip: the image is zeroed)
#pragma unroll
        for (int u = 0; u < 8; ++u) tile[lc * kQPitch + lr + 4 * u] = v[u];
        if (j0 + kQDims < d) gload(j0 + kQDims);   // in flight during the search
        __syncthreads();
        if (row < rows) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                RaField f[4];
                double yv[4];
                int idx[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = slot + 8 * (4 * h + u), j = j0 + c;
                    f[u] = ra_field(j < d ? j : d - 1, lv_off, pos, width, cs);
                    if (j >= d) f[u].w = 0;
                    yv[u] = tile[c * kQPitch + row];
                    idx[u] = 0;
                }
                for (int it = 1; it <= 8; ++it) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int s = (1 << f[u].w) >> it;
                        if (s) {
                            const double* L = lv + f[u].off + idx[u] + s - 1;
                            const double mid = __dmul_rn(0.5, __dadd_rn(L[0], L[1]));
                            idx[u] += !(yv[u] <= mid) ? s : 0;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (f[u].w == 0) continue;
                    const uint32_t win = (uint32_t)idx[u] << f[u].sh;
                    const int a = row * pw * 4 + f[u].byte;
                    atomicOr(&img[a >> 2], (win >> 8) << (8 * (a & 3)));
                    if (f[u].sh < 8)   // the field reaches into the next byte
                        atomicOr(&img[(a + 1) >> 2], (win & 0xffu) << (8 * ((a + 1) & 3)));
                }
            }
        }
    }
    __syncthreads();

    // the image, row pitch 4 pw, to the rows' contiguous cs-byte codes
    uint8_t* out = codes + r0 * cs;
    const uint8_t* ib = reinterpret_cast<const uint8_t*>(img);
    const unsigned bytes = (unsigned)rows * (unsigned)cs, ucs = (unsigned)cs;
    const unsigned words = (reinterpret_cast<uintptr_t>(out) & 3) == 0 ? bytes >> 2 : 0u;
    if ((cs & 3) == 0) {
        for (unsigned k = tid; k < words; k += kRaThreads) {
            const unsigned b = 4 * k, r = b / ucs;
            reinterpret_cast<uint32_t*>(out)[k] = img[r * pw + ((b - r * ucs) >> 2)];
        }
    } else {
        for (unsigned k = tid; k < words; k += kRaThreads) {
            uint32_t wv = 0;
#pragma unroll
            for (unsigned q = 0; q < 4; ++q) {
                const unsigned b = 4 * k + q, r = b / ucs;
                wv |= (uint32_t)ib[r * pw * 4 + (b - r * ucs)] << (8 * q);
            }
            reinterpret_cast<uint32_t*>(out)[k] = wv;
        }
    }
    for (unsigned b = 4 * words + tid; b < bytes; b += kRaThreads) {
        const unsigned r = b / ucs;
        out[b] = ib[r * pw * 4 + (b - r * ucs)];
    }
}

__global__ __launch_bounds__(kRaThreads) void ra_dequantize_kernel(const uint8_t* __restrict__ codes, int64_t n, int d,
                                                                   const double* __restrict__ lv,
                                                                   const int32_t* __restrict__ lv_off,
                                                                   const int32_t* __restrict__ pos,
                                                                   const int32_t* __restrict__ width, int cs,
                                                                   int rows_per, double* __restrict__ y_hat) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ra_lds[];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per;
    const int rows = (int)(n - r0 < rows_per ? n - r0 : rows_per);
    const int bytes = rows * cs;
    uint8_t* sb = reinterpret_cast<uint8_t*>(ra_lds);
    const uint8_t* in = codes + r0 * cs;
    if ((reinterpret_cast<uintptr_t>(in) & 15) == 0) {
        const int lines = bytes >> 4;
        const ra_u32x4* src = reinterpret_cast<const ra_u32x4*>(in);
        ra_u32x4* dst = reinterpret_cast<ra_u32x4*>(ra_lds);
        for (int i = tid; i < lines; i += kRaThreads) dst[i] = src[i];
        for (int i = (lines << 4) + tid; i < bytes; i += kRaThreads) sb[i] = in[i];
    } else {
        for (int i = tid; i < bytes; i += kRaThreads) sb[i] = in[i];
    }
    if (tid == 0) sb[bytes] = 0;   // the window of a field in the tile's last byte reads one byte on
    __syncthreads();

    double* yt = y_hat + r0 * d;
    for (int j = tid; j < d; j += kRaThreads) {
        const RaField f = ra_field(j, lv_off, pos, width, cs);
        const double* L = lv + f.off;
        const uint32_t mask = (1u << f.w) - 1u;
        for (int r = 0; r < rows; ++r) {
            const int a = r * cs + f.byte;
            const uint32_t win = ((uint32_t)sb[a] << 8) | (uint32_t)sb[a + 1];
            yt[(int64_t)r * d + j] = L[(win >> f.sh) & mask];
        }
    }
}

// center / finish: element-wise over a tile of kEwRows rows (one flat range of the array).  V = 4
// (d % 4 == 0 and 16-byte aligned arrays): 16-byte loads and stores, a group never leaves its row.
template <typename T, int V>
__global__ __launch_bounds__(kRaThreads) void ra_center_kernel(const T* __restrict__ x, int64_t n, int d,
                                                               const double* __restrict__ mu, double* __restrict__ xc) {
    const int64_t r0 = (int64_t)blockIdx.x * kEwRows;
    const int rows = (int)(n - r0 < kEwRows ? n - r0 : kEwRows);
    const unsigned total = (unsigned)rows * (unsigned)d;
    const T* xt = x + r0 * d;
    double* ot = xc + r0 * d;
    if (V == 4) {
        for (unsigned t = 4 * threadIdx.x; t < total; t += 4 * kRaThreads) {
            const unsigned j = t % (unsigned)d;
            double v[4];
            if (sizeof(T) == 4) {
                const ra_f32x4 a = *reinterpret_cast<const ra_f32x4*>(xt + t);
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = (double)a[u];
            } else {
                const ra_f64x2 a = *reinterpret_cast<const ra_f64x2*>(xt + t);
                const ra_f64x2 b = *reinterpret_cast<const ra_f64x2*>(xt + t + 2);
                v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
            }
            const ra_f64x2 m0 = *reinterpret_cast<const ra_f64x2*>(mu + j);
            const ra_f64x2 m1 = *reinterpret_cast<const ra_f64x2*>(mu + j + 2);
            ra_f64x2 o0, o1;
            o0[0] = __dsub_rn(v[0], m0[0]); o0[1] = __dsub_rn(v[1], m0[1]);
            o1[0] = __dsub_rn(v[2], m1[0]); o1[1] = __dsub_rn(v[3], m1[1]);
            *reinterpret_cast<ra_f64x2*>(ot + t) = o0;
            *reinterpret_cast<ra_f64x2*>(ot + t + 2) = o1;
        }
    } else {
        for (unsigned t = threadIdx.x; t < total; t += kRaThreads)
            ot[t] = __dsub_rn((double)xt[t], mu[t % (unsigned)d]);
    }
}

template <int V>
__global__ __launch_bounds__(kRaThreads) void ra_finish_kernel(const double* __restrict__ z, int64_t n, int d,
                                                               const double* __restrict__ mu, float* __restrict__ out) {
    const int64_t r0 = (int64_t)blockIdx.x * kEwRows;
    const int rows = (int)(n - r0 < kEwRows ? n - r0 : kEwRows);
    const unsigned total = (unsigned)rows * (unsigned)d;
    const double* zt = z + r0 * d;
    float* ot = out + r0 * d;
    if (V == 4) {
        for (unsigned t = 4 * threadIdx.x; t < total; t += 4 * kRaThreads) {
            const unsigned j = t % (unsigned)d;
            const ra_f64x2 a = *reinterpret_cast<const ra_f64x2*>(zt + t);
            const ra_f64x2 b = *reinterpret_cast<const ra_f64x2*>(zt + t + 2);
            const ra_f64x2 m0 = *reinterpret_cast<const ra_f64x2*>(mu + j);
            const ra_f64x2 m1 = *reinterpret_cast<const ra_f64x2*>(mu + j + 2);
            ra_f32x4 o;
            o[0] = (float)__dadd_rn(a[0], m0[0]); o[1] = (float)__dadd_rn(a[1], m0[1]);
            o[2] = (float)__dadd_rn(b[0], m1[0]); o[3] = (float)__dadd_rn(b[1], m1[1]);
            *reinterpret_cast<ra_f32x4*>(ot + t) = o;
        }
    } else {
        for (unsigned t = threadIdx.x; t < total; t += kRaThreads)
            ot[t] = (float)__dadd_rn(zt[t], mu[t % (unsigned)d]);
    }
}


// Rows per workgroup: as many as the 64 KiB of LDS hold beside the kernel's other use of it, at
// most the kernel's tile (>= 1 for every code_size <= kRaMaxCode).
inline int ra_quantize_rows(int32_t cs) {
    const int fit = (kRaLdsBytes - kQTileWords * 4) / (ra_pitch_words(cs) * 4);
    return fit < kQRows ? fit : kQRows;
}
inline int ra_dequantize_rows(int32_t cs) {
    const int fit = (kRaLdsBytes - 16) / cs;
    return fit < kRaRows ? fit : kRaRows;
}

int ra_check(const char* what, const void* a, int64_t n, int32_t d, const void* lv, const void* lv_off, const void* pos,
             const void* width, int32_t cs, const void* b, int rows) {
    MIVQ_REQUIRE(n >= 0 && d > 0 && cs > 0, MIVQ_ERR_INVALID, "%s: bad sizes n=%lld d=%d code_size=%d", what,
                 (long long)n, d, cs);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(a && lv && lv_off && pos && width && b, MIVQ_ERR_INVALID, "%s: null pointer", what);
    MIVQ_REQUIRE(cs <= kRaMaxCode, MIVQ_ERR_UNSUPPORTED, "%s: code_size %d exceeds %d bytes", what, cs, kRaMaxCode);
    MIVQ_REQUIRE(ceil_div(n, rows) < ((int64_t)1 << 31), MIVQ_ERR_UNSUPPORTED, "%s: n=%lld too large", what,
                 (long long)n);
    return MIVQ_OK;
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_rankaware_center(const void* x, int32_t x_is_f64, int64_t n, int32_t d, const double* mu, double* xc,
                                     void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0, MIVQ_ERR_INVALID, "rankaware_center: bad sizes n=%lld d=%d", (long long)n, d);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(x && mu && xc, MIVQ_ERR_INVALID, "rankaware_center: null pointer");
    MIVQ_REQUIRE(d < (1 << 28) && ceil_div(n, kEwRows) < ((int64_t)1 << 31), MIVQ_ERR_UNSUPPORTED,
                 "rankaware_center: n=%lld d=%d too large", (long long)n, d);
    const dim3 grid((unsigned)ceil_div(n, kEwRows)), block(kRaThreads);
    hipStream_t st = as_stream(stream);
    const bool vec = d % 4 == 0 && aligned16(x) && aligned16(mu) && aligned16(xc);
    if (x_is_f64) {
        const double* xd = static_cast<const double*>(x);
        if (vec) hipLaunchKernelGGL((ra_center_kernel<double, 4>), grid, block, 0, st, xd, n, d, mu, xc);
        else hipLaunchKernelGGL((ra_center_kernel<double, 1>), grid, block, 0, st, xd, n, d, mu, xc);
    } else {
        const float* xf = static_cast<const float*>(x);
        if (vec) hipLaunchKernelGGL((ra_center_kernel<float, 4>), grid, block, 0, st, xf, n, d, mu, xc);
        else hipLaunchKernelGGL((ra_center_kernel<float, 1>), grid, block, 0, st, xf, n, d, mu, xc);
    }
    return check_launch("rankaware_center");
}

extern "C" int mivq_rankaware_quantize(const double* y, int64_t n, int32_t d, const double* lv, const int32_t* lv_off,
                                       const int32_t* pos, const int32_t* width, int32_t code_size, uint8_t* codes,
                                       void* stream) {
    const int rows = code_size > 0 && code_size <= kRaMaxCode ? ra_quantize_rows(code_size) : 1;
    const int rc = ra_check("rankaware_quantize", y, n, d, lv, lv_off, pos, width, code_size, codes, rows);
    if (rc != MIVQ_OK || n == 0) return rc;
    const size_t lds = (size_t)kQTileWords * 4 + (size_t)rows * ra_pitch_words(code_size) * 4;
    hipLaunchKernelGGL(ra_quantize_kernel, dim3((unsigned)ceil_div(n, rows)), dim3(kRaThreads), lds, as_stream(stream),
                       y, n, d, lv, lv_off, pos, width, code_size, rows, codes);
    return check_launch("rankaware_quantize");
}

extern "C" int mivq_rankaware_dequantize(const uint8_t* codes, int64_t n, int32_t d, const double* lv,
                                         const int32_t* lv_off, const int32_t* pos, const int32_t* width,
                                         int32_t code_size, double* y_hat, void* stream) {
    const int rows = code_size > 0 && code_size <= kRaMaxCode ? ra_dequantize_rows(code_size) : 1;
    const int rc = ra_check("rankaware_dequantize", codes, n, d, lv, lv_off, pos, width, code_size, y_hat, rows);
    if (rc != MIVQ_OK || n == 0) return rc;
    const size_t lds = align_up((size_t)rows * code_size, 16) + 16;
    hipLaunchKernelGGL(ra_dequantize_kernel, dim3((unsigned)ceil_div(n, rows)), dim3(kRaThreads), lds,
                       as_stream(stream), codes, n, d, lv, lv_off, pos, width, code_size, rows, y_hat);
    return check_launch("rankaware_dequantize");
}

extern "C" int mivq_rankaware_finish(const double* z, int64_t n, int32_t d, const double* mu, float* out, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0, MIVQ_ERR_INVALID, "rankaware_finish: bad sizes n=%lld d=%d", (long long)n, d);
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(z && mu && out, MIVQ_ERR_INVALID, "rankaware_finish: null pointer");
    MIVQ_REQUIRE(d < (1 << 28) && ceil_div(n, kEwRows) < ((int64_t)1 << 31), MIVQ_ERR_UNSUPPORTED,
                 "rankaware_finish: n=%lld d=%d too large", (long long)n, d);
    const dim3 grid((unsigned)ceil_div(n, kEwRows)), block(kRaThreads);
    if (d % 4 == 0 && aligned16(z) && aligned16(mu) && aligned16(out))
        hipLaunchKernelGGL((ra_finish_kernel<4>), grid, block, 0, as_stream(stream), z, n, d, mu, out);
    else
        hipLaunchKernelGGL((ra_finish_kernel<1>), grid, block, 0, as_stream(stream), z, n, d, mu, out);
    return check_launch("rankaware_finish");
}
