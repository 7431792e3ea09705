// fht.hip — the fast Hadamard rotation of Extended RaBitQ on gfx950, alone and fused with the
// encode / decode steps of extrabitq.hip.
//
// The rotation (include/mivq.h states the rule): `rounds` rounds of  sign flips -> Sylvester
// Hadamard transform of a window of T = 2^floor(log2 D) elements, scaled by 1/sqrt(T) -> for
// T < D a mix of the two halves of the row.  Every step is orthogonal and its own inverse; the
// inverse rotation runs the steps of a round backwards and the rounds in reverse.  All fp64.
//
// Two layouts of a row, chosen by D alone, so that a fused call and the staged composition
// always take the same one and agree bit for bit:
//   registers  D = 64 NR for NR in {4, 6, 8, 12, 16, 24, 32} (D <= 2048, 64 VGPRs of row).  One
//              wavefront per row, element t in lane t % 64, register t / 64: the mapping of the
//              normalize step.  Index bits 0..5 of the transform cross lanes (DPP quad
//              permutes for 1 and 2, the swizzle crossbar for 4, 8, 16, a permute for 32), the
//              higher bits are register-to-register butterflies; the window offset D - T and
//              the mix distance D / 2 are whole registers, so nothing is indexed at run time.
//              The sign bits of all rounds sit in LDS as one NR-bit mask per (round, lane),
//              built once per workgroup, which then walks rows in a grid-stride loop.
//   LDS        every other D up to 16384 (128 KiB of row): one workgroup per row, the row in
//              LDS, one radix-2 stage per barrier; the sign bits packed 32 to a word beside it.
// The quantize step wants 8 consecutive elements per lane, so the fused register-path encode
// hands the rotated row over through a per-wave LDS slab; decode needs no LDS at all.
#include <type_traits>

#include "extrabitq_rows.h"

namespace mivq {
namespace {

constexpr int kFhtMaxD = 16384;
constexpr int kFhtMaxRounds = 8;
constexpr int kFhtMaxBlocks = 4096;
constexpr double kInvSqrt2 = 0.70710678118654752440;

constexpr int pow2_floor(int v) {
    int t = 1;
    while (2 * t <= v) t *= 2;
    return t;
}

__device__ __forceinline__ double fht_scale(int T) { return __ddiv_rn(1.0, sqrt((double)T)); }

__device__ __forceinline__ double flip_if(double v, uint32_t bit) {  // bit: 0 or 1
    return __hiloint2double(__double2hiint(v) ^ (int)(bit << 31), __double2loint(v));
}

// ---------------------------------------------------------------- register layout
template <int M>
__device__ __forceinline__ int lane_xor_i(int v) {
    if constexpr (M == 1) return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);       // quad_perm [1,0,3,2]
    else if constexpr (M == 2) return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
    else if constexpr (M <= 16) return __builtin_amdgcn_ds_swizzle(v, (M << 10) | 0x1F);  // lane ^ M in 32
    else return __shfl_xor(v, 32);
}

// one transform stage across lanes: lanes with bit M clear get a + b, the others a - b
template <int M>
__device__ __forceinline__ double lane_butterfly(double v, int lane) {
    const double o = __hiloint2double(lane_xor_i<M>(__double2hiint(v)), lane_xor_i<M>(__double2loint(v)));
    return __dadd_rn(flip_if(v, (lane & M) ? 1u : 0u), o);  // a - b as (-b) + a
}

template <int NR>
struct RegRow {
    double v[NR];
    __device__ __forceinline__ double get(int k) const { return v[k]; }
    __device__ __forceinline__ void set(int k, double x) { v[k] = x; }
};

template <int NR>
__device__ __forceinline__ void reg_signs(RegRow<NR>& r, uint32_t m) {
#pragma unroll
    for (int k = 0; k < NR; ++k) r.v[k] = flip_if(r.v[k], (m >> k) & 1u);
}

template <int NR, int OFF>
__device__ __forceinline__ void reg_hadamard(RegRow<NR>& r, int lane, double scale) {
    constexpr int TR = pow2_floor(NR);
#pragma unroll
    for (int k = OFF; k < OFF + TR; ++k) {
        double x = r.v[k];
        x = lane_butterfly<1>(x, lane);
        x = lane_butterfly<2>(x, lane);
        x = lane_butterfly<4>(x, lane);
        x = lane_butterfly<8>(x, lane);
        x = lane_butterfly<16>(x, lane);
        x = lane_butterfly<32>(x, lane);
        r.v[k] = x;
    }
#pragma unroll
    for (int len = 1; len < TR; len *= 2) {
#pragma unroll
        for (int i = 0; i < TR / 2; ++i) {
            const int lo = OFF + (((i & ~(len - 1)) << 1) | (i & (len - 1)));
            const double a = r.v[lo], b = r.v[lo + len];
            r.v[lo] = __dadd_rn(a, b);
            r.v[lo + len] = __dsub_rn(a, b);
            if (2 * len == TR) {  // the last stage carries the 1 / sqrt(T)
                r.v[lo] = __dmul_rn(r.v[lo], scale);
                r.v[lo + len] = __dmul_rn(r.v[lo + len], scale);
            }
        }
    }
}

template <int NR>
__device__ __forceinline__ void reg_mix(RegRow<NR>& r) {
#pragma unroll
    for (int k = 0; k < NR / 2; ++k) {
        const double a = r.v[k], b = r.v[k + NR / 2];
        r.v[k] = __dmul_rn(__dadd_rn(a, b), kInvSqrt2);
        r.v[k + NR / 2] = __dmul_rn(__dsub_rn(a, b), kInvSqrt2);
    }
}

// smask: (rounds, 64) words in LDS, bit k of word (r, lane) = signs[r, lane + 64 k]
template <int NR>
__device__ __forceinline__ void reg_rotate(RegRow<NR>& r, const uint32_t* smask, int rounds, bool inverse, int lane) {
    constexpr int TR = pow2_floor(NR), OFF = NR - TR;
    static_assert(TR >= 2 && NR % 2 == 0 && NR <= 32, "whole registers for the window and the mix, a 32-bit mask");
    const double scale = fht_scale(64 * TR);
    for (int i = 0; i < rounds; ++i) {
        const int rd = inverse ? rounds - 1 - i : i;
        const uint32_t m = smask[rd * 64 + lane];
        if (!inverse) reg_signs(r, m);
        if (inverse && OFF) reg_mix(r);
        if (OFF && (rd & 1)) reg_hadamard<NR, OFF>(r, lane, scale);
        else reg_hadamard<NR, 0>(r, lane, scale);
        if (!inverse && OFF) reg_mix(r);
        if (inverse) reg_signs(r, m);
    }
}

template <int NR>
__device__ __forceinline__ void reg_load_masks(uint32_t* smask, const uint8_t* __restrict__ signs, int rounds) {
    for (int p = threadIdx.x; p < rounds * 64; p += blockDim.x) {
        const uint8_t* s = signs + (size_t)(p >> 6) * (64 * NR) + (p & 63);
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < NR; ++k) m |= (uint32_t)(s[64 * k] & 1) << k;
        smask[p] = m;
    }
    __syncthreads();
}

// waves per workgroup on the register path: 2 where a row is more than 32 VGPRs, so that the
// encode slab stays at 32 KiB
template <int NR>
constexpr int reg_waves() { return NR > 16 ? 2 : 4; }

template <int NR>
__global__ __launch_bounds__(64 * reg_waves<NR>()) void fht_rotate_reg_kernel(const double* in, int64_t n,
                                                                              const uint8_t* __restrict__ signs,
                                                                              int rounds, int inverse, double* out) {
    constexpr int D = 64 * NR, WPB = reg_waves<NR>();
    __shared__ uint32_t smask[kFhtMaxRounds * 64];
    reg_load_masks<NR>(smask, signs, rounds);
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * WPB) {
        RegRow<NR> r;
#pragma unroll
        for (int k = 0; k < NR; ++k) r.v[k] = in[row * D + lane + 64 * k];
        reg_rotate(r, smask, rounds, inverse != 0, lane);
#pragma unroll
        for (int k = 0; k < NR; ++k) out[row * D + lane + 64 * k] = r.v[k];
    }
}

template <int NR, typename T>
__global__ __launch_bounds__(64 * reg_waves<NR>()) void erq_encode_fht_reg_kernel(
    const T* __restrict__ x, int64_t n, const double* __restrict__ c, const uint8_t* __restrict__ signs, int rounds,
    const double* __restrict__ levels, int nbits, uint8_t* __restrict__ codes) {
    constexpr int D = 64 * NR, WPB = reg_waves<NR>();
    __shared__ uint32_t smask[kFhtMaxRounds * 64];
    __shared__ double slab[WPB * D];
    reg_load_masks<NR>(smask, signs, rounds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cs = (D * nbits + 7) / 8 + 8;
    double* mine = slab + wave * D;
    // every wave of the workgroup takes the same number of trips: the barriers are uniform
    for (int64_t base = (int64_t)blockIdx.x * WPB; base < n; base += (int64_t)gridDim.x * WPB) {
        const int64_t row = base + wave;
        double nr = 0.0;
        if (row < n) {
            RegRow<NR> r;
            nr = erq_normalize_row(x + row * D, D, NR, c, lane, r);
            reg_rotate(r, smask, rounds, false, lane);
#pragma unroll
            for (int k = 0; k < NR; ++k) mine[lane + 64 * k] = r.v[k];
        }
        __syncthreads();
        if (row < n) erq_quantize_row(mine, D, levels, nbits, nr, codes + row * cs, lane);
        __syncthreads();
    }
}

template <int NR>
__global__ __launch_bounds__(64 * reg_waves<NR>()) void erq_decode_fht_reg_kernel(
    const uint8_t* __restrict__ codes, int64_t n, const double* __restrict__ c, const uint8_t* __restrict__ signs,
    int rounds, const double* __restrict__ levels, int nbits, float* __restrict__ out) {
    constexpr int D = 64 * NR, WPB = reg_waves<NR>();
    __shared__ uint32_t smask[kFhtMaxRounds * 64];
    reg_load_masks<NR>(smask, signs, rounds);
    const int lane = threadIdx.x & 63;
    const int ib = (D * nbits + 7) / 8;
    for (int64_t row = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * WPB) {
        const uint8_t* code = codes + row * (ib + 8);
        const double nr = erq_trailer(code, ib), t = erq_trailer(code, ib + 4);
        RegRow<NR> r;
#pragma unroll
        for (int k = 0; k < NR; ++k) r.v[k] = erq_dequantize_elem(code, lane + 64 * k, D, levels, nbits, t);
        reg_rotate(r, smask, rounds, true, lane);
#pragma unroll
        for (int k = 0; k < NR; ++k) out[row * D + lane + 64 * k] = erq_finish_elem(r.v[k], nr, c[lane + 64 * k]);
    }
}

// ---------------------------------------------------------------- LDS layout
// Dynamic LDS of the LDS-path kernels: the row (d fp64), then the sign words (rounds, W) u32 with
// bit b of word (r, w) = signs[r, 32 w + b], W = ceil(d / 32).
inline size_t lds_path_bytes(int d, int rounds) { return (size_t)d * 8 + (size_t)rounds * ((d + 31) / 32) * 4; }
inline int lds_path_threads(int d) { return pow2_floor(d) <= 256 ? 64 : 256; }

__device__ __forceinline__ void lds_load_signs(uint32_t* sw, const uint8_t* __restrict__ signs, int d, int rounds) {
    const int W = (d + 31) / 32;
    for (int p = threadIdx.x; p < rounds * W; p += blockDim.x) {
        const int w = p % W;
        const uint8_t* s = signs + (size_t)(p / W) * d;
        uint32_t m = 0;
        for (int b = 0; b < 32; ++b)
            if (32 * w + b < d) m |= (uint32_t)(s[32 * w + b] & 1) << b;
        sw[p] = m;
    }
    __syncthreads();
}

__device__ __forceinline__ void lds_signs(double* row, const uint32_t* sw, int d) {
    for (int t = threadIdx.x; t < d; t += blockDim.x) row[t] = flip_if(row[t], (sw[t >> 5] >> (t & 31)) & 1u);
    __syncthreads();
}

__device__ __forceinline__ void lds_hadamard(double* win, int T) {
    const double scale = fht_scale(T);
    for (int len = 1; len < T; len *= 2) {
        for (int i = threadIdx.x; i < T / 2; i += blockDim.x) {
            const int lo = ((i & ~(len - 1)) << 1) | (i & (len - 1));
            const double a = win[lo], b = win[lo + len];
            double s = __dadd_rn(a, b), e = __dsub_rn(a, b);
            if (2 * len == T) {  // the last stage carries the 1 / sqrt(T)
                s = __dmul_rn(s, scale);
                e = __dmul_rn(e, scale);
            }
            win[lo] = s;
            win[lo + len] = e;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void lds_mix(double* row, int d) {
    const int h = d / 2;
    for (int i = threadIdx.x; i < h; i += blockDim.x) {
        const double a = row[i], b = row[i + d - h];
        row[i] = __dmul_rn(__dadd_rn(a, b), kInvSqrt2);
        row[i + d - h] = __dmul_rn(__dsub_rn(a, b), kInvSqrt2);
    }
    __syncthreads();
}

// The whole workgroup rotates the row in LDS; the row is visible to all on entry and on return.
__device__ __forceinline__ void lds_rotate(double* row, const uint32_t* sw, int d, int T, int rounds, bool inverse) {
    const int W = (d + 31) / 32;
    for (int i = 0; i < rounds; ++i) {
        const int rd = inverse ? rounds - 1 - i : i;
        if (!inverse) lds_signs(row, sw + rd * W, d);
        if (inverse && T < d) lds_mix(row, d);
        lds_hadamard(row + ((rd & 1) ? d - T : 0), T);
        if (!inverse && T < d) lds_mix(row, d);
        if (inverse) lds_signs(row, sw + rd * W, d);
    }
}

__global__ __launch_bounds__(256) void fht_rotate_lds_kernel(const double* in, int64_t n, int d, int T,
                                                             const uint8_t* __restrict__ signs, int rounds, int inverse,
                                                             double* out) {
    extern __shared__ double fht_lds[];
    double* row = fht_lds;
    uint32_t* sw = reinterpret_cast<uint32_t*>(row + d);
    lds_load_signs(sw, signs, d, rounds);
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        for (int t = threadIdx.x; t < d; t += blockDim.x) row[t] = in[i * d + t];
        __syncthreads();
        lds_rotate(row, sw, d, T, rounds, inverse != 0);
        for (int t = threadIdx.x; t < d; t += blockDim.x) out[i * d + t] = row[t];
        __syncthreads();
    }
}

// The reductions of normalize and quantize keep their one-wavefront order: wave 0 runs them on
// the LDS row, the whole workgroup runs the rotation between them.
template <typename T_>
__global__ __launch_bounds__(256) void erq_encode_fht_lds_kernel(const T_* __restrict__ x, int64_t n, int d, int T,
                                                                 const double* __restrict__ c,
                                                                 const uint8_t* __restrict__ signs, int rounds,
                                                                 const double* __restrict__ levels, int nbits,
                                                                 uint8_t* __restrict__ codes) {
    extern __shared__ double fht_lds[];
    double* row = fht_lds;
    uint32_t* sw = reinterpret_cast<uint32_t*>(row + d);
    lds_load_signs(sw, signs, d, rounds);
    const int cs = (d * nbits + 7) / 8 + 8;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        double nr = 0.0;
        if (threadIdx.x < 64) {
            MemRow r{row, (int)threadIdx.x};
            nr = erq_normalize_row(x + i * d, d, (d + 63) / 64, c, (int)threadIdx.x, r);
        }
        __syncthreads();
        lds_rotate(row, sw, d, T, rounds, false);
        if (threadIdx.x < 64) erq_quantize_row(row, d, levels, nbits, nr, codes + i * cs, (int)threadIdx.x);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void erq_decode_fht_lds_kernel(const uint8_t* __restrict__ codes, int64_t n, int d,
                                                                 int T, const double* __restrict__ c,
                                                                 const uint8_t* __restrict__ signs, int rounds,
                                                                 const double* __restrict__ levels, int nbits,
                                                                 float* __restrict__ out) {
    extern __shared__ double fht_lds[];
    double* row = fht_lds;
    uint32_t* sw = reinterpret_cast<uint32_t*>(row + d);
    lds_load_signs(sw, signs, d, rounds);
    const int ib = (d * nbits + 7) / 8;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint8_t* code = codes + i * (ib + 8);
        const double nr = erq_trailer(code, ib), t = erq_trailer(code, ib + 4);
        for (int j = threadIdx.x; j < d; j += blockDim.x) row[j] = erq_dequantize_elem(code, j, d, levels, nbits, t);
        __syncthreads();
        lds_rotate(row, sw, d, T, rounds, true);
        for (int j = threadIdx.x; j < d; j += blockDim.x) out[i * d + j] = erq_finish_elem(row[j], nr, c[j]);
        __syncthreads();
    }
}

// ---------------------------------------------------------------- host side
// Calls f(integral_constant<NR>) when d has a register layout; false when the row goes to LDS.
template <typename F>
bool with_reg_rows(int d, F&& f) {
    switch (d) {
#define MIVQ_FHT_NR(NR) \
    case 64 * NR: f(std::integral_constant<int, NR>{}); return true;
        MIVQ_FHT_NR(4) MIVQ_FHT_NR(6) MIVQ_FHT_NR(8) MIVQ_FHT_NR(12) MIVQ_FHT_NR(16) MIVQ_FHT_NR(24) MIVQ_FHT_NR(32)
#undef MIVQ_FHT_NR
        default: return false;
    }
}

template <int NR>
dim3 reg_grid(int64_t n) {
    return dim3((unsigned)std::min<int64_t>(ceil_div(n, reg_waves<NR>()), kFhtMaxBlocks));
}

int check_fht(const char* what, int64_t n, int d, int rounds) {
    MIVQ_REQUIRE(n >= 0 && d > 0, MIVQ_ERR_INVALID, "%s: bad sizes", what);
    MIVQ_REQUIRE(rounds >= 1 && rounds <= kFhtMaxRounds, MIVQ_ERR_UNSUPPORTED, "%s: rounds=%d, supported are 1..%d", what,
                 rounds, kFhtMaxRounds);
    MIVQ_REQUIRE(d <= kFhtMaxD, MIVQ_ERR_UNSUPPORTED, "%s: d=%d, the row must fit LDS (d <= %d)", what, d, kFhtMaxD);
    return MIVQ_OK;
}

// LDS-path launch: sets the kernel's dynamic LDS limit, then launches one workgroup per row.
template <typename K, typename... A>
int launch_lds(const char* what, K kern, int64_t n, int d, int rounds, hipStream_t st, A... args) {
    const size_t smem = lds_path_bytes(d, rounds);
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return set_error(MIVQ_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(n, kFhtMaxBlocks)), dim3(lds_path_threads(d)), smem, st,
                       args...);
    return check_launch(what);
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_fht_rotate(const double* in, int64_t n, int32_t d, const uint8_t* signs, int32_t rounds,
                               int32_t inverse, double* out, void* stream) {
    if (int rc = check_fht("fht_rotate", n, d, rounds)) return rc;
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(in && signs && out, MIVQ_ERR_INVALID, "fht_rotate: null pointer");
    const hipStream_t st = as_stream(stream);
    if (with_reg_rows(d, [&](auto NR) {
            constexpr int kNR = decltype(NR)::value;
            hipLaunchKernelGGL(fht_rotate_reg_kernel<kNR>, reg_grid<kNR>(n), dim3(64 * reg_waves<kNR>()), 0, st, in, n,
                               signs, rounds, inverse, out);
        }))
        return check_launch("fht_rotate");
    return launch_lds("fht_rotate", fht_rotate_lds_kernel, n, d, rounds, st, in, n, d, pow2_floor(d), signs, rounds,
                      inverse, out);
}

extern "C" int mivq_extrabitq_encode_fht(const void* x, int32_t x_is_f64, int64_t n, int32_t d, const double* centroid,
                                         const uint8_t* signs, int32_t rounds, const double* levels, int32_t nbits,
                                         uint8_t* codes, void* stream) {
    if (int rc = check_fht("extrabitq_encode_fht", n, d, rounds)) return rc;
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "num_bits must be in [1, 8]");
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(x && centroid && signs && levels && codes, MIVQ_ERR_INVALID, "extrabitq_encode_fht: null pointer");
    const hipStream_t st = as_stream(stream);
    const float* xf = static_cast<const float*>(x);
    const double* xd = static_cast<const double*>(x);
    if (with_reg_rows(d, [&](auto NR) {
            constexpr int kNR = decltype(NR)::value;
            const dim3 grid = reg_grid<kNR>(n), block(64 * reg_waves<kNR>());
            if (x_is_f64)
                hipLaunchKernelGGL((erq_encode_fht_reg_kernel<kNR, double>), grid, block, 0, st, xd, n, centroid, signs,
                                   rounds, levels, nbits, codes);
            else
                hipLaunchKernelGGL((erq_encode_fht_reg_kernel<kNR, float>), grid, block, 0, st, xf, n, centroid, signs,
                                   rounds, levels, nbits, codes);
        }))
        return check_launch("extrabitq_encode_fht");
    if (x_is_f64)
        return launch_lds("extrabitq_encode_fht", erq_encode_fht_lds_kernel<double>, n, d, rounds, st, xd, n, d,
                          pow2_floor(d), centroid, signs, rounds, levels, nbits, codes);
    return launch_lds("extrabitq_encode_fht", erq_encode_fht_lds_kernel<float>, n, d, rounds, st, xf, n, d, pow2_floor(d),
                      centroid, signs, rounds, levels, nbits, codes);
}

extern "C" int mivq_extrabitq_decode_fht(const uint8_t* codes, int64_t n, int32_t d, const double* centroid,
                                         const uint8_t* signs, int32_t rounds, const double* levels, int32_t nbits,
                                         float* out, void* stream) {
    if (int rc = check_fht("extrabitq_decode_fht", n, d, rounds)) return rc;
    MIVQ_REQUIRE(nbits >= 1 && nbits <= 8, MIVQ_ERR_INVALID, "num_bits must be in [1, 8]");
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(codes && centroid && signs && levels && out, MIVQ_ERR_INVALID, "extrabitq_decode_fht: null pointer");
    const hipStream_t st = as_stream(stream);
    if (with_reg_rows(d, [&](auto NR) {
            constexpr int kNR = decltype(NR)::value;
            hipLaunchKernelGGL(erq_decode_fht_reg_kernel<kNR>, reg_grid<kNR>(n), dim3(64 * reg_waves<kNR>()), 0, st, codes,
                               n, centroid, signs, rounds, levels, nbits, out);
        }))
        return check_launch("extrabitq_decode_fht");
    return launch_lds("extrabitq_decode_fht", erq_decode_fht_lds_kernel, n, d, rounds, st, codes, n, d, pow2_floor(d),
                      centroid, signs, rounds, levels, nbits, out);
}
