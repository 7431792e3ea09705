// pairwise_tile.h — the 128 x 64 distance tile of the exact searches' tiled path, shared by
// exact_search.hip (f32 rows and SQ / RaBitQ-1 / LVQ codes) and rankaware_search.hip (rank-aware
// codes), and the choice between that path and the streaming scan.
#pragma once

#include "mivq_common.h"

namespace mivq {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The tiled path (pairwise chains + segmented top-k) wins once there are enough queries to
// fill a 128-row tile; the streaming scan keeps the small-batch cases.  (exact_search.hip)
bool flat_use_tiled(int64_t nq, int64_t n);

// ---------------------------------------------------------------- tiled path
constexpr int PBM = 128, PBN = 64, PBK = 16, PPAD = 4;

// The tile of both pairwise kernels, for the workgroup's 128 rows of x and 64 rows of y:
// out[i][j] = L2: fmaf chain over t of (x_i[t] - y_j[t])^2;  IP: -(fmaf chain of x_i[t] y_j[t]).
// yfetch(t) is dimensions t .. t + 3 (t % 4 == 0) of this thread's y row, row tid >> 2 of the
// 64.  `xvec`: 16-B loads of x.  UNROLL: the unroll factor of a k-slice, the kernel's choice.
template <bool IP, int UNROLL, typename YFetch>
__device__ __forceinline__ void pairwise_tile(const float* x, int64_t n, int64_t m, int d, int xvec, float* out,
                                              YFetch yfetch) {
    __shared__ __attribute__((aligned(16))) float xs[2][PBK][PBM + PPAD];
    __shared__ __attribute__((aligned(16))) float ys[2][PBK][PBN + PPAD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * PBM;
    const int64_t c0 = (int64_t)blockIdx.y * PBN;
    const int yrow = tid >> 2, yq4 = tid & 3;

    // global -> register slice loads: x slice = 128 rows x 16 t (2 float4 per thread), y slice =
    // 64 rows x 16 t (4 dimensions per thread); out-of-range rows and dimensions are 0 on both
    // sides, which leaves every chain unchanged (fmaf(0, 0, a) == a)
    f32x4 px[2], py;
    auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = tid + 256 * u, row = f >> 2, q4 = f & 3;
            const int64_t gr = r0 + row;
            const int t = k0 + 4 * q4;
            if (xvec) {
                px[u] = (gr < n && t < d) ? *reinterpret_cast<const f32x4*>(x + gr * d + t) : (f32x4){0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) px[u][j] = (gr < n && t + j < d) ? x[gr * d + t + j] : 0.0f;
            }
        }
        py = yfetch(k0 + 4 * yq4);
    };
    auto stash = [&](int b) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = tid + 256 * u, row = f >> 2, q4 = f & 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) xs[b][4 * q4 + j][row] = px[u][j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ys[b][4 * yq4 + j][yrow] = py[j];
    };

    // scalar fp32 chains: packed fp32 math must not consume LDS-loaded registers (DESIGN.md §8,
    // tools/isa_audit.py)
    float acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0f;

    fetch(0);
    stash(0);
    __syncthreads();
    int b = 0;
    for (int k0 = 0; k0 < d; k0 += PBK) {
        const bool more = k0 + PBK < d;
        if (more) fetch(k0 + PBK);
#pragma unroll UNROLL
        for (int t = 0; t < PBK; ++t) {
            const f32x4 xa = *reinterpret_cast<const f32x4*>(&xs[b][t][ty * 8]);
            const f32x4 xb = *reinterpret_cast<const f32x4*>(&xs[b][t][ty * 8 + 4]);
            const f32x4 yv = *reinterpret_cast<const f32x4*>(&ys[b][t][tx * 4]);
            const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
            const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (IP) {
                        acc[i][j] = __builtin_fmaf(xv[i], yy[j], acc[i][j]);
                    } else {
                        const float df = __fsub_rn(xv[i], yy[j]);
                        acc[i][j] = __builtin_fmaf(df, df, acc[i][j]);
                    }
                }
            }
        }
        if (more) {
            stash(b ^ 1);
            __syncthreads();
            b ^= 1;
        }
    }
    const int64_t gc = c0 + tx * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t gr = r0 + ty * 8 + i;
        if (gr >= n) continue;
        f32x4 v = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        if (IP) v = -v;
        float* o = out + gr * m + gc;
        if ((m & 3) == 0 && gc + 3 < m) {
            *reinterpret_cast<f32x4*>(o) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (gc + j < m) o[j] = v[j];
        }
    }
}

}  // namespace mivq
