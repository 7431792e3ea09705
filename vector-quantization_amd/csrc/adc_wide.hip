// adc_wide.hip — the flat ADC scan for product quantizers whose per-query lookup table does not
// fit one workgroup's LDS (M * ksub * 4 B > 160 KiB: M >= 161 at 8 bits), on gfx950.
//
// mivq_adc_search (adc.hip) sends here exactly the shapes its resident-table scan refuses; the
// key is the header's: dist(q, i) = ((lut[q][0][c_0] + lut[q][1][c_1]) + ...) + lut[q][M-1][c_M-1],
// one fp32 add per step in ascending m, NaN ranked as +inf, ties to the smaller id.
//
//   adc_wide_scan_kernel  grid (query blocks of 8, row ranges), 1024 threads (16 waves).  A
//       workgroup walks its row range in tiles of 2048 rows: lane = 2 rows, whose 2 x 8 running
//       sums stay in registers for the whole tile.  The subspaces are walked in runs of 64: a
//       lane first loads the run's 64 code bytes of each of its rows into registers (4 x 16-B
//       loads when base and row stride allow, else 4-B words, else bytes; never past a row's
//       last byte), so that a 128-B line of codes is fetched from memory twice at the most.
//       Within a run the workgroup stages the tables of the 8 queries chunk by chunk (mc = 8
//       subspaces at 7 / 8 bits, 32 below: at most 64 KiB) from the (nq, M, ksub) LUT into LDS,
//       transposed to [m][code][query], and every lane adds the chunk's mc lookups to its rows:
//       one lookup is two ds_read_b128 serving the 8 queries, odd lanes reading the two halves
//       in the opposite order (the parity layout of adc.hip's lut_add<8>).  The sum of a
//       (row, query) is therefore sequential in m across chunks and runs: the canonical order.
//       Afterwards every wave offers its rows to its 8 WaveTopK lists, which live across the
//       tiles of the range and go to part (range * 16 + wave); topk.hip merges the parts.
//
// Bytes per (query, row): the lookups read M * 4 B from LDS.  Every tile re-stages the whole
// table block of its 8 queries, 8 * M * ksub * 4 B read from L2 and written to LDS once each, for
// 2048 * M * 32 B of lookups: ksub / 2048 of the lookup bytes, 12.5 % at 8 bits (6.25 % at 7,
// 3.1 % at 6, 0.8 % at 4).  The codes cost M / 8 B per (query, row) from memory (one byte per
// subspace, shared by 8 queries), up to twice that where the two 64-B halves of a line are fetched
// separately.
#include "adc_internal.h"
#include "topk.h"

#include <algorithm>

namespace mivq {
namespace {

typedef float f32x4w __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const f32x4w lds_f4w;

constexpr int kWideQB = 8;                                  // queries per workgroup
constexpr int kWideRows = 2;                                // rows per lane per tile
constexpr int kWideTile = kScanWaves * 64 * kWideRows;      // 2048 rows
constexpr int kWideRun = 64;                                // code bytes per row held in registers
constexpr int kWideLdsBytes = 64 * 1024;                    // the table chunk in LDS
// The MI355X's CU count: workgroups of one round (one per CU).  A constant, since the size query makes
// no HIP call; it decides how the rows are cut into ranges and so the part count of the workspace,
// never a result (exact lists, merged: the same for any partition).
constexpr int kWideCus = 256;

struct WideScan {
    const float* lut;      // (nq, M, ksub)
    const uint8_t* codes;  // (n, M)
    int64_t nq, n, id_offset;
    int64_t range_rows;    // rows per row range, a multiple of kWideTile
    float* pd;             // (parts, nq, k)
    uint32_t* pi;
    int M, nbits, k;
    int wbytes;  // code loads: 16 (base and M multiples of 16), 4 (of 4) or 1
    int vec;     // tables staged with 16-B loads: ksub % 4 == 0 and the LUT 16-B aligned
};

// MCW: words (4 subspaces) per staged chunk, mc = 4 MCW subspaces; a run is up to 16 / MCW chunks.
template <int R, int MCW>
__global__ __launch_bounds__(kScanWaves * 64) void adc_wide_scan_kernel(const WideScan A) {
    constexpr int QB = kWideQB, mc = 4 * MCW;
    extern __shared__ __attribute__((aligned(16))) float wtab[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int M = A.M, ksub = 1 << A.nbits, k = A.k;
    const uint32_t kmask = (uint32_t)ksub - 1u;
    const int64_t q0 = (int64_t)blockIdx.x * QB;
    const int nqb = (int)min<int64_t>(QB, A.nq - q0);
    const int64_t tabn = (int64_t)M * ksub;

    // the chunk [m0, m0 + nm) of the QB tables -> wtab[(mm * ksub + code) * QB + query]; query
    // slots past nqb repeat query q0 (in range) and are never stored
    auto stage = [&](int m0, int nm) {
        const int cnt = nm * ksub;
        if (A.vec) {  // thread = 4 entries of 4 queries, transposed in registers
            const int h = tid & 1;
            const float* src[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qq = 4 * h + i;
                src[i] = A.lut + (q0 + (qq < nqb ? qq : 0)) * tabn + (int64_t)m0 * ksub;
            }
            for (int x = (tid >> 1) * 4; x < cnt; x += kScanWaves * 64 * 2) {
                f32x4w v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const f32x4w*>(src[i] + x);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4w o;
                    o.x = v[0][j]; o.y = v[1][j]; o.z = v[2][j]; o.w = v[3][j];
                    *reinterpret_cast<f32x4w*>(wtab + (x + j) * QB + 4 * h) = o;
                }
            }
        } else {
            for (int e = tid; e < cnt * QB; e += kScanWaves * 64) {
                const int x = e / QB, qq = e - x * QB;
                wtab[e] = A.lut[(q0 + (qq < nqb ? qq : 0)) * tabn + (int64_t)m0 * ksub + x];
            }
        }
    };

    WaveTopK<R> top[QB];
    float thr_d[QB];
    uint32_t thr_i[QB];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        top[qq].init();
        thr_d[qq] = INFINITY;
        thr_i[qq] = kNoId;
    }
    const uint32_t par = (uint32_t)lane & 1u;
    const uint32_t tbase = (uint32_t)(uintptr_t)wtab + 16u * par;  // LDS byte address of the half read first

    const int64_t rbeg = (int64_t)blockIdx.y * A.range_rows;
    const int64_t rend = min(A.n, rbeg + A.range_rows);
    for (int64_t base = rbeg; base < rend; base += kWideTile) {  // block-uniform
        int64_t row[kWideRows];
        bool valid[kWideRows];
        float acc[kWideRows][QB];  // odd lanes: the two halves swapped until the tile ends
#pragma unroll
        for (int r = 0; r < kWideRows; ++r) {
            row[r] = base + (r * kScanWaves + wv) * 64 + lane;
            valid[r] = row[r] < rend;
#pragma unroll
            for (int qq = 0; qq < QB; ++qq) acc[r][qq] = 0.0f;
        }
        for (int r0 = 0; r0 < M; r0 += kWideRun) {
            const int nrun = min(kWideRun, M - r0);
            // the run's code bytes [r0, r0 + nrun) of the lane's rows, zero past nrun and for rows
            // past the range (code 0 is a valid lookup; such sums are never offered)
            uint32_t cw[kWideRows][kWideRun / 4];
#pragma unroll
            for (int r = 0; r < kWideRows; ++r) {
#pragma unroll
                for (int j = 0; j < kWideRun / 4; ++j) cw[r][j] = 0u;
                if (!valid[r]) continue;
                const uint8_t* p = A.codes + row[r] * M + r0;
                if (A.wbytes == 16) {  // nrun % 16 == 0
#pragma unroll
                    for (int j = 0; j < kWideRun / 16; ++j) {
                        if (16 * j < nrun) {
                            const uint4 v = *reinterpret_cast<const uint4*>(p + 16 * j);
                            cw[r][4 * j + 0] = v.x; cw[r][4 * j + 1] = v.y;
                            cw[r][4 * j + 2] = v.z; cw[r][4 * j + 3] = v.w;
                        }
                    }
                } else if (A.wbytes == 4) {  // nrun % 4 == 0
#pragma unroll
                    for (int j = 0; j < kWideRun / 4; ++j)
                        if (4 * j < nrun) cw[r][j] = *reinterpret_cast<const uint32_t*>(p + 4 * j);
                } else {
#pragma unroll
                    for (int j = 0; j < kWideRun / 4; ++j) {
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            if (4 * j + b < nrun) cw[r][j] |= (uint32_t)p[4 * j + b] << (8 * b);
                    }
                }
            }
            // chunk after chunk, the queue of code words moving down so that the chunk's words are
            // cw[r][0 .. MCW) (a rolled loop: one copy of the staging and of the mc lookups)
#pragma unroll 1
            for (int c0 = 0; c0 < nrun; c0 += mc) {  // block-uniform
                const int nm = min(mc, nrun - c0);
                __syncthreads();  // the previous chunk is consumed
                stage(r0 + c0, nm);
                __syncthreads();
#pragma unroll
                for (int jw = 0; jw < MCW; ++jw) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int mm = 4 * jw + b;
                        if (mm >= nm) break;  // block-uniform: the ragged end of the last chunk
                        const uint32_t tb = tbase + (uint32_t)(mm * ksub) * (QB * 4u);
#pragma unroll
                        for (int r = 0; r < kWideRows; ++r) {
                            const uint32_t code = (cw[r][jw] >> (8 * b)) & kmask;
                            const uint32_t o1 = tb + (code << 5), o2 = o1 ^ 16u;
                            const f32x4w t0 = *reinterpret_cast<lds_f4w*>((uintptr_t)o1);
                            const f32x4w t1 = *reinterpret_cast<lds_f4w*>((uintptr_t)o2);
                            acc[r][0] = __fadd_rn(acc[r][0], t0.x); acc[r][1] = __fadd_rn(acc[r][1], t0.y);
                            acc[r][2] = __fadd_rn(acc[r][2], t0.z); acc[r][3] = __fadd_rn(acc[r][3], t0.w);
                            acc[r][4] = __fadd_rn(acc[r][4], t1.x); acc[r][5] = __fadd_rn(acc[r][5], t1.y);
                            acc[r][6] = __fadd_rn(acc[r][6], t1.z); acc[r][7] = __fadd_rn(acc[r][7], t1.w);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < kWideRows; ++r) {
#pragma unroll
                    for (int t = 0; t + MCW < kWideRun / 4; ++t) cw[r][t] = cw[r][t + MCW];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kWideRows; ++r) {
            const uint32_t gid = (uint32_t)(A.id_offset + row[r]);
#pragma unroll
            for (int qq = 0; qq < QB; ++qq) {
                if (qq >= nqb) break;  // block-uniform
                // odd lanes hold query qq's sum in the other half
                float dv = par ? acc[r][qq ^ 4] : acc[r][qq];
                if (dv != dv) dv = INFINITY;  // NaN ranks with +inf
                top[qq].offer(valid[r], dv, gid, k, lane, thr_d[qq], thr_i[qq]);
            }
        }
    }
    const int64_t part = (int64_t)blockIdx.y * kScanWaves + wv;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        if (qq >= nqb) break;
        const int64_t o = (part * A.nq + q0 + qq) * k;
        top[qq].store(A.pd + o, A.pi + o, k, lane);
    }
}

template <int R, int MCW>
hipError_t launch_wide(const WideScan& A, int64_t nch, hipStream_t st) {
    const size_t smem = (size_t)4 * MCW * ((size_t)1 << A.nbits) * kWideQB * sizeof(float);  // <= kWideLdsBytes
    auto kern = adc_wide_scan_kernel<R, MCW>;
    // per launch, like adc.hip's launch_scan: the attribute is per device, and the call keeps no state
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(A.nq, kWideQB), (unsigned)nch), dim3(kScanWaves * 64), smem, st, A);
    return hipGetLastError();
}

// Tiles per row range: enough ranges that the query blocks x ranges fill the chip once, whole tiles.
int64_t wide_range_tiles(int64_t nq, int64_t n) {
    const int64_t tiles = ceil_div(n, kWideTile);
    const int64_t want = std::max<int64_t>(1, kWideCus / ceil_div(nq, kWideQB));
    return ceil_div(tiles, std::min(tiles, want));
}

}  // namespace

int64_t adc_wide_chunks(int64_t nq, int64_t n) {
    return ceil_div(ceil_div(n, kWideTile), wide_range_tiles(nq, n));
}

hipError_t launch_adc_wide(const float* lut, int64_t nq, const uint8_t* codes, int64_t n, int M, int nbits, int k,
                           int64_t id_offset, float* pd, uint32_t* pi, hipStream_t st) {
    WideScan A{};
    A.lut = lut;
    A.codes = codes;
    A.nq = nq;
    A.n = n;
    A.id_offset = id_offset;
    A.range_rows = wide_range_tiles(nq, n) * kWideTile;
    A.pd = pd;
    A.pi = pi;
    A.M = M;
    A.nbits = nbits;
    A.k = k;
    const uintptr_t cb = reinterpret_cast<uintptr_t>(codes);
    A.wbytes = (cb % 16 == 0 && M % 16 == 0) ? 16 : (cb % 4 == 0 && M % 4 == 0) ? 4 : 1;
    A.vec = nbits >= 2 && aligned16(lut);
    const int64_t nch = adc_wide_chunks(nq, n);
    // 8 subspaces per chunk at 7 / 8 bits (32 / 64 KiB), 32 below (64 KiB at 6 bits)
    static_assert(8 * 256 * kWideQB * 4 <= kWideLdsBytes && 32 * 64 * kWideQB * 4 <= kWideLdsBytes, "chunk fits");
    return with_topk_regs(k, [&](auto R) {
        return nbits >= 7 ? launch_wide<decltype(R)::value, 2>(A, nch, st) : launch_wide<decltype(R)::value, 8>(A, nch, st);
    });
}

}  // namespace mivq
