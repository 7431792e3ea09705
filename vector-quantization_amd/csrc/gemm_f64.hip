// gemm_f64.hip — the library's fp64 GEMMs on v_mfma_f64_16x16x4_f64 (gfx950).
//
// Two entry points, one workgroup shape: 256 threads own a 128 x 128 output tile as four
// F64WaveTile (gemm_f64.h: 64 x 64 per wave, operand map and sum order documented there), with K
// in slices of 16 through two LDS stages.  Each kernel adds its loader, pipeline and store.
//   mivq_extrabitq_rotate: s = o . op(P), (n, d) x (d, d) fp64.  The rotations of Extended RaBitQ
//     (extrabitq.hip) and of the rank-aware quantizer (rankaware.hip), and the products of the
//     OPQ fit's Newton-Schulz polar factor.  erq_rotate_fast_kernel (d % 32 == 0) or
//     erq_rotate_kernel (any d).
//   mivq_opq_gram: G = X^T Y, (n, d) f32 rows, fp64 sums, split over rows with an ordered reduce.
//     The OPQ fit's Procrustes step and the rank-aware quantizer's PCA.
#include <algorithm>

#include "gemm_f64.h"

namespace mivq {
namespace {

// ---------------------------------------------------------------- rotation s = o . op(P)
// op(P) = P (transpose 0) or P^T (transpose 1).  A stage = 128 rows x 16 k of o, B stage = 16 k
// x 128 columns of op(P); rows past n / columns past d are masked.
constexpr int kRotT = 128, kRotK = 16;
constexpr int kRotAP = kRotK + 1;   // A stage row pitch (doubles): [row][k]
constexpr int kRotBP = kRotT + 1;   // B stage row pitch (doubles): [k][col]

// Tile of workgroup b: the workgroups of one XCD (b % 8, dealt round-robin) take a contiguous
// range of tiles, so the column tiles of one 128-row block run side by side on one XCD and
// share its L2 copy of the o strip (3 MB at D = 3072); the round-3 order (b itself) spread
// them over all eight XCDs, each fetching the strip again.
__device__ __forceinline__ int64_t erq_tile(int64_t b, int64_t G) {
    const int64_t x = b & 7, j = b >> 3, q = G >> 3, r = G & 7;
    return x * q + (x < r ? x : r) + j;
}

// The two LDS stages of a rotation kernel.  At file scope so that the shared staging and slice
// code below names them directly: handed down as a pointer or reference, the same reads paired
// into fewer ds_read2_b64 and erq_rotate_fast_kernel<0> took two more VGPRs.
__shared__ double rotAs[2][kRotT * kRotAP];
__shared__ double rotBs[2][kRotK * kRotBP];

// What the two rotation kernels share: the workgroup's tile, the wave's quarter of it, and the
// staging map.  Each thread stages 8 doubles of A (row ar, k ak ..) and 8 of B: row bk of the
// slice, columns bj .. (TR 0: B[k][j] = P[k][j], 8 consecutive columns of a row of P) or
// column bj, k bk .. (TR 1: B[k][j] = P[j][k], column j of op(P) is row j of P).
template <int TR>
struct RotBlock {
    int64_t r0;
    int c0, wr, wc, ar, ak, bk, bj;

    __device__ __forceinline__ explicit RotBlock(int64_t ctiles) {
        const int tid = threadIdx.x, w = tid >> 6;
        const int64_t t = erq_tile(blockIdx.x, gridDim.x);
        r0 = (t / ctiles) * kRotT;
        c0 = (int)(t % ctiles) * kRotT;
        wr = w >> 1, wc = w & 1;  // wave tile: rows wr*64.., cols wc*64..
        ar = tid >> 1, ak = 8 * (tid & 1);
        bk = TR ? 8 * (tid & 1) : tid >> 4, bj = TR ? tid >> 1 : 8 * (tid & 15);
    }
    __device__ __forceinline__ void sstore(int st, const double (&ra)[8], const double (&rb)[8]) const {
#pragma unroll
        for (int u = 0; u < 8; ++u) rotAs[st][ar * kRotAP + ak + u] = ra[u];
#pragma unroll
        for (int u = 0; u < 8; ++u) rotBs[st][TR ? (bk + u) * kRotBP + bj : bk * kRotBP + bj + u] = rb[u];
    }
    __device__ __forceinline__ void slice(F64WaveTile& T, int st) const {
        T.slice<kRotK>([&](int i, int k) { return rotAs[st][(wr * 64 + i + T.fi) * kRotAP + k + T.fk]; },
                       [&](int k, int j) { return rotBs[st][(k + T.fk) * kRotBP + wc * 64 + j + T.fi]; });
    }
    __device__ __forceinline__ void store(const F64WaveTile& T, int64_t n, int d, double* __restrict__ s) const {
        // column first: s + col is shared by the 16 stores of a block column (s[row * d + col] cost
        // one more 64-bit add per store)
        T.store(r0 + wr * 64, c0 + wc * 64, [&](int64_t row, int col, double v) {
            if (row < n && col < d) (s + col)[row * d] = v;
        });
    }
};

// Any d: per-element guarded loads, one slice ahead.
template <int TR>
__global__ __launch_bounds__(256) void erq_rotate_kernel(const double* __restrict__ o, int64_t n, int d,
                                                         const double* __restrict__ P, double* __restrict__ s,
                                                         int64_t ctiles) {
    const RotBlock<TR> B(ctiles);
    F64WaveTile T(threadIdx.x & 63);
    double ra[8], rb[8];
    auto gload = [&](int k0) __attribute__((always_inline)) {
        const int64_t gr = B.r0 + B.ar;
#pragma unroll
        for (int u = 0; u < 8; ++u) ra[u] = (gr < n && k0 + B.ak + u < d) ? o[gr * d + k0 + B.ak + u] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            rb[u] = TR ? ((B.c0 + B.bj < d && k0 + B.bk + u < d) ? P[(int64_t)(B.c0 + B.bj) * d + k0 + B.bk + u] : 0.0)
                       : ((k0 + B.bk < d && B.c0 + B.bj + u < d) ? P[(int64_t)(k0 + B.bk) * d + B.c0 + B.bj + u] : 0.0);
    };
    const int nk = (d + kRotK - 1) / kRotK;
    gload(0);
    B.sstore(0, ra, rb);
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const int st = ks & 1;
        if (ks + 1 < nk) gload((ks + 1) * kRotK);
        B.slice(T, st);
        if (ks + 1 < nk) B.sstore(st ^ 1, ra, rb);
        __syncthreads();
    }
    B.store(T, n, d, s);
}

// d % 32 == 0 (every BASELINE width): the same tile, slices and MFMA order as erq_rotate_kernel
// (identical results), with the global side rebuilt: each thread's 8-double chunks are in or out
// of range as a whole, so they load as 16-B buffer loads (range-checked: rows past n read zeros,
// no branches), and the loads run TWO slices ahead through two register stages (slice ks + 2
// loads while slice ks computes; slice ks + 1, loaded a slice earlier, goes to LDS after it).
// The generic kernel's per-element guarded 8-B loads compiled to a branch per load and a
// vmcnt(0) in the middle of its loads.
typedef unsigned int erq_u32x4 __attribute__((ext_vector_type(4)));
template <int TR>
__global__ __launch_bounds__(256, 2) void erq_rotate_fast_kernel(const double* __restrict__ o, int64_t n, int d,
                                                              const double* __restrict__ P,
                                                              double* __restrict__ s, int64_t ctiles) {
    const RotBlock<TR> B(ctiles);
    F64WaveTile T(threadIdx.x & 63);
    constexpr int kOob = (int)0x80000000u;
    const int rows = (int)(n - B.r0 < kRotT ? n - B.r0 : kRotT);
    // o rows r0 .. r0 + rows of this tile (< 4 GiB: 128 rows); P whole (d^2 * 8 < 2^31 checked)
    const __amdgpu_buffer_rsrc_t ors =
        __builtin_amdgcn_make_buffer_rsrc((void*)(o + B.r0 * d), 0, rows * d * 8, 0x00020000);
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc((void*)P, 0, d * d * 8, 0x00020000);
    auto gload = [&](int k0, double (&ra)[8], double (&rb)[8]) __attribute__((always_inline)) {
        const int va = k0 + B.ak < d ? (B.ar * d + k0 + B.ak) * 8 : kOob;
        const int vb = TR ? ((B.c0 + B.bj < d && k0 + B.bk < d) ? ((B.c0 + B.bj) * d + k0 + B.bk) * 8 : kOob)
                          : ((k0 + B.bk < d && B.c0 + B.bj < d) ? ((k0 + B.bk) * d + B.c0 + B.bj) * 8 : kOob);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const erq_u32x4 ua = __builtin_amdgcn_raw_buffer_load_b128(ors, va == kOob ? kOob : va + 16 * q, 0, 0);
            const erq_u32x4 ub = __builtin_amdgcn_raw_buffer_load_b128(prs, vb == kOob ? kOob : vb + 16 * q, 0, 0);
            ra[2 * q] = __hiloint2double((int)ua[1], (int)ua[0]);
            ra[2 * q + 1] = __hiloint2double((int)ua[3], (int)ua[2]);
            rb[2 * q] = __hiloint2double((int)ub[1], (int)ub[0]);
            rb[2 * q + 1] = __hiloint2double((int)ub[3], (int)ub[2]);
        }
    };
    const int nk = (d + kRotK - 1) / kRotK;
    double ra0[8], rb0[8], ra1[8], rb1[8];
    gload(0, ra0, rb0);
    gload(kRotK, ra1, rb1);
    B.sstore(0, ra0, rb0);
    // two slices per trip (nk is even: d % 32 == 0) so the register stages stay static and no
    // branch splits the loop; loads past d read zeros, and stores of them are never read.
    // Stage first: each half-trip stores the next slice (loaded a half-trip and more ago)
    // BEFORE its MFMAs, then issues the loads of the slice three ahead into the freed stage
    // (load, MFMAs, then store: 61.8 against 58.6 ms, profiles/r04_s25)
    gload(2 * kRotK, ra0, rb0);
    __syncthreads();
    for (int ks = 0; ks < nk; ks += 2) {
        B.sstore(1, ra1, rb1);    // slice ks + 1
        gload((ks + 3) * kRotK, ra1, rb1);
        B.slice(T, 0);            // slice ks
        __syncthreads();
        B.sstore(0, ra0, rb0);    // slice ks + 2 (past nk: zeros, never read)
        gload((ks + 4) * kRotK, ra0, rb0);
        B.slice(T, 1);            // slice ks + 1
        __syncthreads();
    }
    B.store(T, n, d, s);
}

// ------------------------------------------------------------ Gram matrix G = X^T Y (training)
// faiss OPQMatrix::train's X^T Yhat before its SVD
// (/root/reference/src/haag_vq/methods/optimized_product_quantization.py:21-28): X, Y (n, d) f32
// rows, each product exact in fp64 (24 + 24 bits).  Split K: workgroup (tile, s) sums rows
// [s R, (s + 1) R) of a 128 x 128 tile of G into part[s]; opq_gram_reduce_kernel adds the parts
// in s order (deterministic).  Both operands are staged as [k][i].
constexpr int GR_T = 128, GR_K = 16, GR_P = GR_T + 2;  // LDS rows of 130 doubles: [k][i]

__global__ __launch_bounds__(256) void opq_gram_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                         int64_t n, int d, int64_t rows_per_split, int ctiles,
                                                         double* __restrict__ part) {
    __shared__ double As[2][GR_K * GR_P];
    __shared__ double Bs[2][GR_K * GR_P];
    const int tid = threadIdx.x, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1;
    const int tile = blockIdx.x, sp = blockIdx.y;
    const int i0 = (tile / ctiles) * GR_T, j0 = (tile % ctiles) * GR_T;
    const int64_t ra = (int64_t)sp * rows_per_split;
    const int64_t rb = min(n, ra + rows_per_split);
    F64WaveTile T(tid & 63);
    // staging: thread t loads rows k = t >> 4 of the 16-row step, columns 8 (t & 15) .. +7 of the
    // tile (two float4 of X, two of Y); out-of-range rows / columns read as 0
    const int kr = tid >> 4, cc = 8 * (tid & 15);
    float xa[8], yb[8];
    auto gload = [&](int64_t r) __attribute__((always_inline)) {
        const int64_t row = r + kr;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int ci = i0 + cc + u, cj = j0 + cc + u;
            xa[u] = (row < rb && ci < d) ? X[row * d + ci] : 0.0f;
            yb[u] = (row < rb && cj < d) ? Y[row * d + cj] : 0.0f;
        }
    };
    auto sstore = [&](int st) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            As[st][kr * GR_P + cc + u] = (double)xa[u];
            Bs[st][kr * GR_P + cc + u] = (double)yb[u];
        }
    };
    auto put = [&](int i, int j, double v) {
        if (i < d && j < d) part[((int64_t)sp * d + i) * d + j] = v;
    };
    // No split is empty: gram_splits keeps splits <= ceil(n / 64), so (splits - 1) ceil(n / splits)
    // < n.  The early-out stays all the same: without it the kernel, its K loop unchanged, ran 2 %
    // slower at 100000 x 1536 (profiles/gemm_f64_refactor/ab.log).
    const int64_t nk = (rb - ra + GR_K - 1) / GR_K;
    if (nk <= 0) {
        T.store(i0 + wr * 64, j0 + wc * 64, put);  // zeros
        return;
    }
    gload(ra);
    sstore(0);
    __syncthreads();
    for (int64_t ks = 0; ks < nk; ++ks) {
        const int st = (int)(ks & 1);
        if (ks + 1 < nk) gload(ra + (ks + 1) * GR_K);
        T.slice<GR_K>([&](int i, int k) { return As[st][(k + T.fk) * GR_P + wr * 64 + i + T.fi]; },
                      [&](int k, int j) { return Bs[st][(k + T.fk) * GR_P + wc * 64 + j + T.fi]; });
        if (ks + 1 < nk) sstore(st ^ 1);
        __syncthreads();
    }
    T.store(i0 + wr * 64, j0 + wc * 64, put);
}

__global__ __launch_bounds__(256) void opq_gram_reduce_kernel(const double* __restrict__ part, int splits, int64_t dd,
                                                                double* __restrict__ G) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= dd) return;
    double s = part[e];
    for (int p = 1; p < splits; ++p) s += part[(int64_t)p * dd + e];
    G[e] = s;
}

int gram_splits(int64_t n, int d) {
    const int64_t tiles = ceil_div(d, GR_T) * ceil_div(d, GR_T);
    int64_t s = std::max<int64_t>(1, ceil_div(512, tiles));          // >= 2 rounds of workgroups
    s = std::min<int64_t>(s, std::max<int64_t>(1, ceil_div(n, 4 * GR_K)));  // >= 4 K steps each
    return (int)std::min<int64_t>(s, 64);
}

template <class K>
void launch_rotate(K kern, int64_t tiles, hipStream_t st, const double* o, int64_t n, int d, const double* P, double* s,
                   int64_t ct) {
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), 0, st, o, n, d, P, s, ct);
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" int mivq_extrabitq_rotate(const double* o, int64_t n, int32_t d, const double* P, int32_t transpose,
                                     double* s, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0, MIVQ_ERR_INVALID, "extrabitq_rotate: bad sizes n=%lld d=%d", (long long)n, d);
    MIVQ_REQUIRE(transpose == 0 || transpose == 1, MIVQ_ERR_INVALID, "extrabitq_rotate: transpose must be 0 or 1");
    if (n == 0) return MIVQ_OK;
    MIVQ_REQUIRE(o && P && s && o != s, MIVQ_ERR_INVALID, "extrabitq_rotate: null or aliased pointer");
    const int64_t ct = ceil_div(d, kRotT), tiles = ceil_div(n, kRotT) * ct;
    MIVQ_REQUIRE(tiles < ((int64_t)1 << 31), MIVQ_ERR_UNSUPPORTED, "extrabitq_rotate: n=%lld too large", (long long)n);
    // the fast kernel's buffer offsets are 32-bit: d^2 * 8 bytes of P and 128 rows of o
    const bool fast = d % 32 == 0 && (int64_t)d * d * 8 < ((int64_t)1 << 31);
    if (fast)
        launch_rotate(transpose ? erq_rotate_fast_kernel<1> : erq_rotate_fast_kernel<0>, tiles, as_stream(stream), o, n,
                      d, P, s, ct);
    else
        launch_rotate(transpose ? erq_rotate_kernel<1> : erq_rotate_kernel<0>, tiles, as_stream(stream), o, n, d, P, s,
                      ct);
    return check_launch("extrabitq_rotate");
}

extern "C" size_t mivq_opq_gram_workspace_bytes(int64_t n, int32_t d) {
    if (n <= 0 || d <= 0) return 0;
    return (size_t)gram_splits(n, d) * (size_t)d * d * sizeof(double);
}

extern "C" int mivq_opq_gram(const float* x, const float* y, int64_t n, int32_t d, void* workspace,
                             size_t workspace_bytes, double* G, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d > 0, MIVQ_ERR_INVALID, "opq_gram: bad sizes n=%lld d=%d", (long long)n, d);
    MIVQ_REQUIRE(G && (n == 0 || (x && y)), MIVQ_ERR_INVALID, "opq_gram: null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t dd = (int64_t)d * d;
    if (n == 0) {
        hipError_t e = hipMemsetAsync(G, 0, (size_t)dd * sizeof(double), st);
        return e == hipSuccess ? MIVQ_OK : set_error(MIVQ_ERR_HIP, "opq_gram: %s", hipGetErrorString(e));
    }
    const size_t need = mivq_opq_gram_workspace_bytes(n, d);
    MIVQ_REQUIRE(workspace && workspace_bytes >= need, MIVQ_ERR_WORKSPACE, "opq_gram: workspace %zu < %zu",
                 workspace_bytes, need);
    const int splits = gram_splits(n, d);
    const int ct = (int)ceil_div(d, GR_T);
    const int64_t rps = ceil_div(n, splits);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(opq_gram_kernel, dim3((unsigned)(ct * ct), (unsigned)splits), dim3(256), 0, st, x, y, n, d, rps,
                       ct, part);
    int rc = check_launch("opq_gram");
    if (rc) return rc;
    hipLaunchKernelGGL(opq_gram_reduce_kernel, dim3((unsigned)ceil_div(dd, 256)), dim3(256), 0, st, part, splits, dd, G);
    return check_launch("opq_gram_reduce");
}
