// gemm_f64.h — the fp64 MFMA wave tile of the library's fp64 GEMMs (gemm_f64.hip), device-only.
//
// One wavefront owns a 64 x 64 tile of D = A . B as 4 x 4 blocks of v_mfma_f64_16x16x4_f64:
// 16 accumulators of 4 doubles per lane.  Operand map of the instruction for lane l
// (cdna_hip_programming.md, f64 MFMA): A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15],
// D: column l & 15, rows (l >> 4) + 4 g for register g.  Every product is an exact fp64 FMA
// accumulation; the sum order is the MFMA's over k, then the callers' slices in ascending order.
// The kernels differ in how they stage A and B in LDS, so the tile reads its operands through
// accessors.  They get the origin of a block inside the wave tile and the staged slice, and add
// the lane's own place (fi, fk): a_at(i, k) = A[i + fi][k + fk], b_at(k, j) = B[k + fk][j + fi],
// i and j in {0, 16, 32, 48}, k in {0, 4, .., KS - 4}.
#pragma once
#include "mivq_common.h"

namespace mivq {

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct F64WaveTile {
    f64x4 acc[4][4];
    const int fi, fk;  // the lane's place in a 16 x 16 block: l & 15, l >> 4

    __device__ __forceinline__ explicit F64WaveTile(int lane) : fi(lane & 15), fk(lane >> 4) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
    }

    // One K slice of KS (a multiple of 4): per k4 the 4 + 4 operand reads, then 16 MFMAs, a outer.
    template <int KS, class FA, class FB>
    __device__ __forceinline__ void slice(FA a_at, FB b_at) {
#pragma unroll
        for (int k4 = 0; k4 < KS; k4 += 4) {
            double af[4], bf[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) af[a] = a_at(a * 16, k4);
#pragma unroll
            for (int b = 0; b < 4; ++b) bf[b] = b_at(k4, b * 16);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
        }
    }

    // Epilogue: st(row, col, value) for the lane's 64 outputs, (row0, col0) the wave tile's origin.
    // Row is whatever integer type the caller's addressing uses, so that the caller's
    // row * pitch + col stays one expression the compiler can strength-reduce over the 64 stores.
    template <class Row, class FS>
    __device__ __forceinline__ void store(Row row0, int col0, FS st) const {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int g = 0; g < 4; ++g) st(row0 + a * 16 + fk + 4 * g, col0 + b * 16 + fi, acc[a][b][g]);
    }
};

}  // namespace mivq
