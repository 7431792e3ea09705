// adc_filtered.hip — the filtered ADC search on gfx950 (M = 16 / 32, ksub = 256, k <= 32): the
// same canonical fp32 top-k as adc.hip's scan, found in two passes.
//
// 1. adc_qstats_kernel / adc_qtab_kernel quantise every query's LUT to 6-bit integers:
//      q[m][c] = min(63, floor((lut[m][c] - min_m) / delta)),  delta = min(range, 2 w) / 63
//    (range = max_m range_m, w = the largest mean offset above min_m: the grid is fine where the
//    rows near the top live, entries above it clamp), one byte per query, 16 queries per 16-B
//    table entry.  A row's sum S = sum_m q[m][code_m] < 2^11 (M <= 32).
// 2. adc_qscan_kernel: four lookups add up inside the bytes (4 x 63 < 256) before one v_perm
//    unpack to u16 pairs, so a (query, row) costs M / 8 byte-adds + M / 4 unpacks + M / 4
//    16-bit adds; every lane keeps, per query, the three smallest keys (S << 16 | step) of its
//    own rows (v_med3 / v_min, registers only), and each wave ("part") finally lists the
//    candidates below a ballot-searched threshold plus its bound B (every unlisted row of the
//    part has S >= B).
// 3. adc_rerank_kernel (one wave per query) evaluates the canonical fp32 distance (the sum over
//    m in order of the fp32 LUT entries, include/mivq.h) of every listed row and keeps the exact
//    top-k.  It is the canonical answer if no row outside the lists can beat its k-th element
//    (E_k): a row part p did not list has S >= B(p), and, with q*delta <= lut - min, its
//    canonical distance is >= LB(S) = base + delta * S - margin (base = sum_m min_m, margin >=
//    the fp32 summation error gamma_M * sum_m max_c |lut[m][c]| plus fp64 slack).  So the query
//    is certified when LB(B(p)) > E_k for every part p; a query that is not (or whose LUT is
//    not finite) is listed for
// 4. the fp32 scan (adc_scan_kernel) re-run on the listed queries only (query indirection; the
//    workgroups of empty slots return at once) and its merge.
// Results are identical to the fp32 scan's for every input.
#include "adc_internal.h"
#include "topk.h"

#include <limits.h>

namespace mivq {
namespace {

typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const u32x4v lds_u4;

struct AdcQStat {
    double base, delta, margin;
    int bad, pad;
};

// Integer table: 6-bit entries in bytes (round 5, A/B-measured against 8- and 7-bit entries and
// u16 entries: 6 bits lets four lookups share one unpack, and certified as many queries once the
// grid span followed the mean offset); lanes keep 3 keys per query (2 left ~2 % of the queries
// uncertified on Gaussian rows, 3 none).
// (5 bits, eight lookups per unpack: 3-5 % faster on clustered rows and the config #5 shape, but
// 1.6x slower on 1M x 1536 Gaussian rows, whose queries it mostly fails to certify; r05_s22)
constexpr int kAdcBits = 6;
// (round 6, with the scan VALU-bound: 2 keys -- one v_med3 less per row and query -- measured
// 2.4x / 1.23x slower at 1000 x 1M / the config #5 shape: the uncertified queries' fp32 re-runs)
constexpr int kLaneKeys = 3;
constexpr double kAdcSpan = 2.0;  // the grid's span in mean offsets above the minimum
__host__ __device__ constexpr int adc_qmax() { return (1 << kAdcBits) - 1; }
constexpr int kQB = 16;  // queries per integer-table block

// grid nq, block 256: per (query, m) the minimum and range (mins[q][m] = min_m), then the
// query's {base, delta, margin, bad}.
__global__ __launch_bounds__(256) void adc_qstats_kernel(const float* __restrict__ lut, int64_t nq, int M,
                                                         float* __restrict__ mins, AdcQStat* __restrict__ qs) {
    __shared__ double s_min[64], s_rng[64], s_abs[64], s_wid[64];
    __shared__ int s_bad;
    const int64_t qi = blockIdx.x;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    for (int m = w; m < M; m += 4) {
        const float4 v = *reinterpret_cast<const float4*>(lut + (qi * M + m) * 256 + 4 * l);
        const bool fin = isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w);
        const float mn = wave_min(fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
        const float mx = wave_max(fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        const float ab = wave_max(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        // mean offset above the minimum (the scale the rows near the top live on)
        const float wid = wave_sum((v.x - mn) + (v.y - mn) + (v.z - mn) + (v.w - mn)) * (1.0f / 256.0f);
        const bool bad = __ballot(!fin) != 0ull;
        if (l == 0) {
            s_min[m] = mn;
            s_wid[m] = wid;
            s_rng[m] = (double)mx - (double)mn;
            s_abs[m] = ab;
            mins[qi * M + m] = mn;
            if (bad) s_bad = 1;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double base = 0.0, rng = 0.0, mag = 0.0, wid = 0.0;
        for (int m = 0; m < M; ++m) {
            base += s_min[m];
            rng = fmax(rng, s_rng[m]);
            mag += s_abs[m];
            wid = fmax(wid, s_wid[m]);
        }
        AdcQStat st;
        st.base = base;
        // the integer grid spans kAdcSpan x the largest mean offset: entries above it clamp to
        // QMAX (a clamped q still has q delta <= lut - min, so every bound stays a lower bound),
        // and the rows near the top -- small entries in most subspaces -- get a finer grid than
        // the full range would give (round 5: range / 255 certified too few queries on
        // k-means codebooks, whose far centroids stretch the range)
        const double span = fmin(rng, kAdcSpan * wid);
        st.delta = span > 0.0 ? span / (double)adc_qmax() : (rng > 0.0 ? rng / (double)adc_qmax() : 1.0);
        // fp32 canonical sum: |fl(sum) - sum| <= gamma_{M-1} sum |t| <= gamma_M mag; 2x that, plus
        // fp64 slack for base and delta * S
        st.margin = 2.0 * (double)M * 5.9604644775390625e-8 * mag + 1e-12 * (mag + fabs(base));
        st.bad = s_bad || !isfinite(base) || !isfinite(mag) || !(st.delta > 0.0);
        st.pad = 0;
        qs[qi] = st;
    }
}

// grid (ceil(nq / QB), M), block 256 (code c): one 16-B entry per (m, c) holding the 16 queries'
// bytes; dword w holds queries (4w, 4w + 2, 4w + 1, 4w + 3) in bytes 0..3, so the two byte-pair
// unpacks give the u16 pairs (4w, 4w + 1) and (4w + 2, 4w + 3).  q <= (lut - min) / delta (the
// ratio is shrunk by 2^-50 before the floor, so fp64 rounding never rounds it up past an
// integer).  Entry order (round 6): [m / 16][c][m % 16] -- the 16 subspaces of a half side by
// side in one 256-B bank row per code, so that lanes reading 16 DIFFERENT subspaces hit 16
// different bank slots whatever their codes (adc_qscan_kernel).
template <int QB>
__global__ __launch_bounds__(256) void adc_qtab_kernel(const float* __restrict__ lut, int64_t nq, int M,
                                                       const float* __restrict__ mins,
                                                       const AdcQStat* __restrict__ qs, uint32_t* __restrict__ tab) {
    static_assert(QB % 16 == 0, "whole 16-B entries");
    constexpr int NWD = QB / 4;
    const int64_t qb = blockIdx.x;
    const int m = blockIdx.y, c = threadIdx.x;
    const int qmax = adc_qmax();
    uint32_t w[NWD];
#pragma unroll
    for (int j = 0; j < NWD; ++j) w[j] = 0u;
    // every load of the block's QB queries first (rows past nq clamped to the last query, their
    // bytes zeroed below), then the arithmetic: one memory round trip instead of one per query
    // behind the per-query branches
    float lv[QB], mv[QB];
    double dl[QB];
    int bd[QB];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        const int64_t qi = min(qb * QB + qq, nq - 1);
        lv[qq] = lut[(qi * M + m) * 256 + c];
        mv[qq] = mins[qi * M + m];
        dl[qq] = qs[qi].delta;
        bd[qq] = qs[qi].bad;
    }
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        const double x = ((double)lv[qq] - (double)mv[qq]) / dl[qq] * (1.0 - 8.881784197001252e-16);
        uint32_t v = x >= (double)qmax ? (uint32_t)qmax : x > 0.0 ? (uint32_t)floor(x) : 0u;
        if (qb * QB + qq >= nq || bd[qq]) v = 0u;
        const int r = qq & 3;
        w[qq >> 2] |= v << (8 * (((r & 1) << 1) | (r >> 1)));
    }
    uint32_t* dst = tab + (((qb * (M / 16) + (m >> 4)) * 256 + c) * 16 + (m & 15)) * NWD;
#pragma unroll
    for (int j = 0; j < NWD; j += 4) *reinterpret_cast<uint4*>(dst + j) = make_uint4(w[j], w[j + 1], w[j + 2], w[j + 3]);
}

// grid (nchunks, ceil(nq / 16)), block kScanWaves waves (the fp32 scan's structure): the byte
// tables of 16 queries in LDS (M * 4 KiB), M = 16 MC, each lane one row per wave-step with its
// code row loaded a step ahead.  No wave-level list during the scan: every lane keeps, per
// query, the kLaneKeys smallest keys (S << 16 | wave-step) of its own rows (v_med3 + v_min per
// row and query, registers only).  At the end each wave ("part") selects from its 192 lane
// candidates per query those with S below T = the largest value with at most K1 candidates
// below it (binary search on ballot counts), writes them (float(S), id) -- the rest of the K1
// slots sentinels -- and its bound B = min(T, min over lanes of the lane's last key's S): every
// row of the part that is not listed has S >= B (a lane's other rows are >= its last kept
// key, a dropped candidate is >= T).  (The round-5 first cut kept wave-resident exact lists
// updated by ballot + shuffle inserts: those inserts were most of its LDS instructions.)

__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

template <int MC, bool PIN>
__global__ __launch_bounds__(kScanWaves * 64) void adc_qscan_kernel(
    const uint32_t* __restrict__ qtab, int64_t nq, const uint8_t* __restrict__ codes, int64_t n, int k1,
    int64_t id_offset, int64_t chunk_rows, float* __restrict__ part_d, uint32_t* __restrict__ part_i,
    float* __restrict__ part_b) {
    constexpr int M = 16 * MC;
    constexpr int QB = kQB;
    constexpr int NWD = QB / 4;   // dwords per (m, code) entry (u8 per query)
    constexpr int NACC = QB / 2;  // u16-pair accumulators (queries 2j, 2j + 1)
    extern __shared__ __attribute__((aligned(16))) uint32_t qt[];  // [M][256][NWD]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.y * QB;
    const int nqb = (int)min<int64_t>(QB, nq - q0);
    {
        const uint4* src = reinterpret_cast<const uint4*>(qtab + (int64_t)blockIdx.y * M * 256 * NWD);
        uint4* dst = reinterpret_cast<uint4*>(qt);
        for (int e = tid; e < M * 256 * NWD / 4; e += kScanWaves * 64) dst[e] = src[e];
    }
    __syncthreads();

    // per query: the lane's kLaneKeys smallest keys (S << 16 | step) in increasing order, ~0u = none
    uint32_t mk[kLaneKeys][QB];
#pragma unroll
    for (int t = 0; t < kLaneKeys; ++t)
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) mk[t][qq] = 0xFFFFFFFFu;

    const int64_t rbeg = (int64_t)blockIdx.x * chunk_rows;
    const int64_t rend = min(n, rbeg + chunk_rows);
    uint4 cw[MC];
    // Conflict-free lookups (round 6).  A ds_read_b128 is served in four 16-lane groups, one LDS
    // cycle per group when its 16 lanes hit 16 different 16-B slots of the 256-B bank row
    // (MI355X_MICROARCH.md §LDS); with the table [m][code], slot = code % 16 is random and a group
    // took ~3 cycles.  With the table [m / 16][code][m % 16] the slot is m % 16, so at every
    // lookup step the lanes of a group read 16 different subspaces: lane l (r = l % 16, rd = r / 4,
    // rb = r % 4; every 16-lane group of ds_read_b128 holds each r once) takes at step (word k,
    // byte b) subspace mm = 4 ((k + rd) % 4) + (b + rb) % 4 of the half.  The integer sums do
    // not depend on the order of their terms.  Per lookup the address is still ONE VALU: a
    // v_perm builds code << 8 | mm << 4 from the code word (byte (b + rb) % 4 of its dword
    // rotated by rd) and a per-lane register of the four mm << 4 values of word k.
    const uint32_t rl = (uint32_t)lane & 15u, rd = rl >> 2, rb = rl & 3u;
    uint32_t mo[4], psel[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t v = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= ((4u * ((k + rd) & 3u) + ((b + rb) & 3u)) << 4) << (8 * b);
        mo[k] = v;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)  // byte0 <- mo byte b (S1), byte1 <- code byte (b + rb) % 4 (S0), bytes 2, 3 <- 0
        psel[b] = (uint32_t)b | ((4u + ((b + rb) & 3u)) << 8) | 0x0C0C0000u;
    // The code row's dwords come rotated by rd straight from memory: four dword buffer loads per
    // 16-B half with per-lane offsets fixed for the whole kernel (the lane's row and rotation)
    // and the wave-step in the scalar soffset, range-checked over the chunk (rows past it read
    // zeros), so neither the rotation nor the row address costs VALU.  The size and the offsets
    // are int: adc_filtered_offsets_fit.
    // (16-B row loads rotated by two select levels per half: slower at M = 16; at M = 32 the
    // buffer loads win 2-3 % at 1000 / 4000 x 1M and 10,000 x 6.65M in the pinned kernel,
    // profiles/r06_s34, and spill in the unpinned one, which launch_qscan never takes there)
    static_assert(MC == 1 || PIN, "M = 32: the unpinned kernel spills");
    // the even-query unpack (bytes 0 and 2 -> the u16 pair) is a mask: with the mask in an SGPR it
    // is a 32-bit v_and instead of a 64-bit v_perm (the scan is VALU-issue bound, DESIGN 3.3;
    // 1.2-1.5 % faster at M = 16 / 32, 1000 x 1M and the config #5 shape, profiles/r06_s35)
    uint32_t mlo;
    asm volatile("s_mov_b32 %0, 0xff00ff" : "=s"(mlo));
    const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(codes + rbeg * (16 * MC)), 0, (int)(max<int64_t>(0, rend - rbeg) * (16 * MC)), 0x00020000);
    int voffc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) voffc[i] = (wv * 64 + lane) * (16 * MC) + 4 * (int)((i + rd) & 3u);
    auto fetchb_to = [&](int64_t base, uint4 (&dst)[MC]) __attribute__((always_inline)) {
        const int so = (int)(base - rbeg) * (16 * MC);
#pragma unroll
        for (int c = 0; c < MC; ++c) {
            dst[c].x = __builtin_amdgcn_raw_buffer_load_b32(crs, voffc[0], so + 16 * c, 0);
            dst[c].y = __builtin_amdgcn_raw_buffer_load_b32(crs, voffc[1], so + 16 * c, 0);
            dst[c].z = __builtin_amdgcn_raw_buffer_load_b32(crs, voffc[2], so + 16 * c, 0);
            dst[c].w = __builtin_amdgcn_raw_buffer_load_b32(crs, voffc[3], so + 16 * c, 0);
        }
    };
    auto fetchb = [&](int64_t base) __attribute__((always_inline)) { fetchb_to(base, cw); };
    // entries of kAdcBits < 8 bits: 2^(8 - bits) lookups add up in the bytes themselves (no carry
    // crosses a byte) before one unpack to the u16 pairs
    constexpr int UNP = 1 << (8 - kAdcBits);
    static_assert(UNP == 1 || UNP == 2 || UNP == 4 || UNP == 8, "entry bits");
    const int64_t first = rbeg + (int64_t)wv * 64;
    fetchb(rbeg);
    uint32_t step = 0;
    for (int64_t base = first; base < rend; base += kScanWaves * 64, ++step) {
        const int64_t row = base + lane;
        uint32_t acc[NACC];
#pragma unroll
        for (int j = 0; j < NACC; ++j) acc[j] = 0u;
        uint4 cur[MC];
#pragma unroll
        for (int c = 0; c < MC; ++c) cur[c] = cw[c];
        fetchb(base - (int64_t)wv * 64 + kScanWaves * 64);
        // PIN (round 6): the next row's loads issue here, at the top of the step, so they have the
        // whole step to land (the compiler otherwise places them ~30 % into it, and the copy at
        // the loop latch waits for them): 8 % faster at the config #5 shape, 2 % slower when one
        // round of workgroups covers the search (1000 x 1M), so launch_qscan picks it by shape
        if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
        uint32_t wq[4 * MC];
#pragma unroll
        for (int c = 0; c < MC; ++c) {
            wq[4 * c + 0] = cur[c].x; wq[4 * c + 1] = cur[c].y;
            wq[4 * c + 2] = cur[c].z; wq[4 * c + 3] = cur[c].w;
        }
        // unrolled over the code words (round 5: 0.560 -> 0.531 ms per 1000 x 1M at M = 16,
        // profiles/r05_s20): word jw is read straight from its register wq[jw]
        uint32_t a8[4] = {0u, 0u, 0u, 0u};  // byte sums of up to UNP lookups (across words)
#pragma unroll
        for (int jw = 0; jw < 4 * MC; ++jw) {
            const uint32_t wrd = wq[jw];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                // code << 8 | mm << 4 in ONE v_perm; the half's 64 KiB (M = 32) is one more op
                // (the ds_read offset field holds 16 bits); qt is this kernel's only LDS, so the
                // dynamic segment starts at address 0 (guarded at the bound store below)
                uint32_t o1 = __builtin_amdgcn_perm(wrd, mo[jw & 3], psel[b]);
                if (jw >= 4) o1 |= (uint32_t)(jw >> 2) << 16;
                const u32x4v t0 = *(reinterpret_cast<const lds_u4*>((uintptr_t)o1));
                const uint32_t tv[4] = {t0.x, t0.y, t0.z, t0.w};
#pragma unroll
                for (int wd = 0; wd < 4; ++wd) a8[wd] = ((4 * jw + b) % UNP == 0) ? tv[wd] : a8[wd] + tv[wd];
                if ((4 * jw + b + 1) % UNP == 0) {
#pragma unroll
                    for (int wd = 0; wd < 4; ++wd) {  // bytes (4w, 4w+2, 4w+1, 4w+3) -> u16 pairs
                        acc[2 * wd] += a8[wd] & mlo;
                        acc[2 * wd + 1] += __builtin_amdgcn_perm(a8[wd], a8[wd], 0x0C030C01u);
                    }
                }
            }
        }
        // a row past the chunk takes part in nothing (the last step only)
        const uint32_t inval = row < rend ? 0u : 0xFFFFFFFFu;
        auto insert = [&](int qq, uint32_t key) __attribute__((always_inline)) {
            // sorted insert into (m0 <= m1 [<= m2]): med3 / min per slot
            if constexpr (kLaneKeys == 3) mk[2][qq] = umed3(mk[1][qq], mk[2][qq], key);
            mk[1][qq] = umed3(mk[0][qq], mk[1][qq], key);
            mk[0][qq] = min(mk[0][qq], key);
        };
        // the row's low half once per row: each key is then one v_lshl_or / v_and_or
        const uint32_t lo16 = step | inval;
#pragma unroll
        for (int j = 0; j < NACC; ++j) {
            insert(2 * j, (acc[j] << 16) | lo16);                 // query 2j
            insert(2 * j + 1, (acc[j] & 0xFFFF0000u) | lo16);     // query 2j + 1
        }
    }
    // per query: select the candidates below T, the bound B, write K1 slots.  A lane's unlisted
    // rows have keys >= its last kept key, so B = min(T, min over lanes of that key's S).
    const int64_t part = (int64_t)blockIdx.x * kScanWaves + wv;
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        if (qq >= nqb) continue;
        uint32_t sv[kLaneKeys];
#pragma unroll
        for (int t = 0; t < kLaneKeys; ++t) sv[t] = mk[t][qq] >> 16;  // 0xFFFF: no candidate
        // T: the largest t in [0, 0xFFFF] with #{candidates with S < t} <= k1.  Real sums are at
        // most kSMax = M * QMAX (keys of rows past the chunk have S = 0xFFFF: never candidates),
        // so the search runs over [0, kSMax + 1] (11 steps at M = 16 instead of 16) and a result
        // of kSMax + 1 (every kept key listed) stands for 0xFFFF
        constexpr uint32_t kSMax = (uint32_t)M * ((1u << kAdcBits) - 1u);
        uint32_t lo = 0, hi = kSMax + 1;
        while (lo < hi) {  // wave-uniform
            const uint32_t mid = (lo + hi + 1) >> 1;
            int cnt = 0;
#pragma unroll
            for (int t = 0; t < kLaneKeys; ++t) cnt += __popcll(__ballot(sv[t] < mid));
            if (cnt <= k1) lo = mid; else hi = mid - 1;
        }
        const uint32_t T = lo > kSMax ? 0xFFFFu : lo;
        // min over lanes of the last kept key's S: a wave reduction, not a ballot search
        uint32_t blo = sv[kLaneKeys - 1];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) blo = min(blo, (uint32_t)__shfl_xor((int)blo, o));
        const uint32_t B = min(T, blo);
        float* od = part_d + (part * nq + q0 + qq) * k1;
        uint32_t* oi = part_i + (part * nq + q0 + qq) * k1;
        int used = 0;
#pragma unroll
        for (int t = 0; t < kLaneKeys; ++t) {
            const bool take = sv[t] < T;
            const uint64_t bt = __ballot(take);
            if (take) {
                const int at = used + __popcll(bt & below);
                od[at] = (float)sv[t];
                oi[at] = (uint32_t)(id_offset + first + (int64_t)(mk[t][qq] & 0xFFFFu) * (kScanWaves * 64) + lane);
            }
            used += __popcll(bt);
        }
        for (int e = used + lane; e < k1; e += 64) { od[e] = INFINITY; oi[e] = kNoId; }
        // B = 0xFFFF: every row of the part is listed
        // (the lookups take the table at LDS address 0, i.e. no static LDS in this kernel; were
        // there any, every bound reads 0 and every query goes to the fp32 re-run: slow, never wrong)
        if (lane == 0)
            part_b[part * nq + q0 + qq] = __builtin_amdgcn_groupstaticsize() != 0 ? 0.0f : B >= 0xFFFFu ? INFINITY : (float)B;
    }
}

// The rerank's first 64 entries all beat the empty list's +inf threshold: instead of ~28
// sequential wave inserts (each a ballot and four cross-lane moves in a dependent chain) they are
// sorted at once -- bitonic, 21 compare-exchange stages on (dist, id) -- and become the list
// (R = 1, k <= 64: element e in lane e).  The k smallest pairs are unique, so the list equals the
// one the inserts build.
__device__ __forceinline__ void rr_seed(WaveTopK<1>& top, bool valid, float dv, uint32_t id, int k, int lane,
                                        float& thr_d, uint32_t& thr_i) {
    float d = valid ? dv : INFINITY;
    uint32_t i = valid ? id : kNoId;
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const float od = __shfl_xor(d, stride);
            const uint32_t oi = (uint32_t)__shfl_xor((int)i, stride);
            const bool up = (lane & size) == 0 || size == 64;  // ascending run
            const bool lower = (lane & stride) == 0;
            const bool take = lower == up ? pair_less(od, oi, d, i) : pair_less(d, i, od, oi);
            d = take ? od : d;
            i = take ? oi : i;
        }
    }
    top.d[0] = d;
    top.id[0] = i;
    top.kth(k, thr_d, thr_i);
}

// One wave per query: canonical fp32 distances of the listed rows, exact top-k, certificate.
// k <= 32 (adc_filtered_shape): one list register.
template <int MC>
__global__ __launch_bounds__(256) void adc_rerank_kernel(const float* __restrict__ lut, int64_t nq,
                                                         const uint8_t* __restrict__ codes, int64_t id_offset,
                                                         const uint32_t* __restrict__ pi, const float* __restrict__ pb,
                                                         int parts, int k1, int k, const AdcQStat* __restrict__ qs,
                                                         float* __restrict__ out_d, uint32_t* __restrict__ out_i,
                                                         int* __restrict__ fail_list, int* __restrict__ fail_count,
                                                         int lut16) {
    constexpr int M = 16 * MC;
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;  // whole wave
    const AdcQStat st = qs[qi];
    WaveTopK<1> top;
    top.init();
    float thr_d = INFINITY;
    uint32_t thr_i = kNoId;
    // the wave's query LUT staged in LDS (coalesced), so the candidates' M lookups each are LDS
    // reads instead of random 4-B global reads (wave-private region: no workgroup barrier;
    // round 5: 0.478 -> 0.468 ms per 1000 x 1M search at M = 16, 0.826 -> 0.794 at M = 32,
    // 3.07 -> 2.95 ms at the config #5 shape, profiles/r05_s32)
    extern __shared__ __attribute__((aligned(16))) float rls[];
    float* lq = rls + (threadIdx.x >> 6) * M * 256;
    {
        const float* src = lut + qi * M * 256;
        if (lut16) {
#pragma unroll
            for (int i = 0; i < M; ++i)
                reinterpret_cast<float4*>(lq)[i * 64 + lane] = reinterpret_cast<const float4*>(src)[i * 64 + lane];
        } else {
            for (int i = lane; i < M * 256; i += 64) lq[i] = src[i];
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the wave's own stores
        __builtin_amdgcn_wave_barrier();
    }
    const int64_t total = (int64_t)parts * k1;
    auto eval = [&](bool valid, const uint4 (&cw)[MC]) __attribute__((always_inline)) {
        float dv = INFINITY;
        if (valid) {
            float t[M];
#pragma unroll
            for (int c = 0; c < MC; ++c) {
                const uint32_t wd[4] = {cw[c].x, cw[c].y, cw[c].z, cw[c].w};
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    t[16 * c + j] = lq[(16 * c + j) * 256 + ((wd[j >> 2] >> (8 * (j & 3))) & 0xFFu)];
            }
            dv = 0.0f;
#pragma unroll
            for (int m = 0; m < M; ++m) dv += t[m];  // the canonical order
            if (dv != dv) dv = INFINITY;
        }
        return dv;
    };
    auto offer = [&](bool first, bool valid, float dv, uint32_t id) __attribute__((always_inline)) {
        // (round 6 split, profiling builds traced in r06_s39: 33 us per 1000 x 1M search, of which
        // ~12.5 us were the sequential wave inserts -- the first step's now one sort, r06_s40)
        if (first) rr_seed(top, valid, dv, id, k, lane, thr_d, thr_i);
        else top.offer(valid, dv, id, k, lane, thr_d, thr_i);
    };
    // (round 6: ids and code rows by range-checked buffer loads in chunks of 8 steps -- all of a
    // chunk's gathers in flight at once -- measured 26.5 -> 23.9 us here but neutral to 0.3 %
    // slower end to end at M = 32 and the config #5 shape, r06_s41: not kept)
    // three-stage pipeline over the list in steps of 64 entries (round 6): the ids two steps
    // ahead and the code rows (which need those ids) one step ahead are in flight while a step
    // is evaluated, instead of an id load -> row gather -> lookups round trip per step
    auto ld_id = [&](int64_t e0) __attribute__((always_inline)) {
        const int64_t e = e0 + lane;
        uint32_t id = kNoId;
        if (e < total) {
            const int64_t p = e / k1, j = e - p * k1;
            id = pi[(p * nq + qi) * k1 + j];
        }
        return id;
    };
    auto ld_row = [&](uint32_t id, uint4 (&cw)[MC]) __attribute__((always_inline)) {
        const uint4* cr = reinterpret_cast<const uint4*>(codes + ((int64_t)(id != kNoId ? id : (uint32_t)id_offset) - id_offset) * M);
#pragma unroll
        for (int c = 0; c < MC; ++c) cw[c] = id != kNoId ? cr[c] : make_uint4(0u, 0u, 0u, 0u);
    };
    uint32_t id_cur = ld_id(0), id_nxt = ld_id(64);
    uint4 cw_cur[MC];
    ld_row(id_cur, cw_cur);
    for (int64_t e0 = 0; e0 < total; e0 += 64) {
        const uint32_t id_far = ld_id(e0 + 128);
        uint4 cw_nxt[MC];
        ld_row(id_nxt, cw_nxt);
        const uint32_t id = id_cur;
        const bool valid = id != kNoId;
        offer(e0 == 0, valid, eval(valid, cw_cur), id);
        id_cur = id_nxt;
        id_nxt = id_far;
#pragma unroll
        for (int c = 0; c < MC; ++c) cw_cur[c] = cw_nxt[c];
    }
    // certificate: every part's bound B (its unlisted rows have S >= B) must put them above E_k
    bool ok = !st.bad;
    for (int p0 = 0; p0 < parts; p0 += 64) {
        const int p = p0 + lane;
        bool f = false;
        if (p < parts) {
            const float B = pb[(int64_t)p * nq + qi];
            if (B < INFINITY) {
                const double lb = st.base + st.delta * (double)B - st.margin;
                f = !(lb > (double)thr_d);
            }
        }
        if (__ballot(f) != 0ull) ok = false;
    }
    if (ok) {
        top.store(out_d + qi * k, out_i + qi * k, k, lane);
    } else if (lane == 0) {
        fail_list[atomicAdd(fail_count, 1)] = (int)qi;
    }
}

// Part lists keep K1 = k + kListSlack entries (at most 256): the certificate bounds the rows a
// part did NOT list by its K1-th entry, so a part holding some of the k best rows still
// certifies when its K1-th row is clearly worse (with K1 = k, the part holding the best row of
// a k = 1 search never could).
constexpr int kListSlack = 4;
int adc_k1(int k) { return k + kListSlack; }

// Row chunks of the filtered (integer) scan: the cost model's, then, when its grid fits one round
// of the CUs, at least 4 chunks and at most 1024 wave-steps per chunk (the grid then takes several
// rounds and launch_qscan the pinned-prefetch kernel).  Measured (round 6, profiles/r06_s30, 1M
// rows unless noted; results identical): 2000 queries 0.99 -> 0.79 ms, 4000 queries 1.77 ->
// 1.44 ms, 1000 x 6.65M 2.65 -> 2.20 ms, 3000 x 6.65M 6.57 -> 6.18 ms, while 500 / 1000 queries
// over 1M-4M rows (model already at 4+ chunks, <= 1024 steps) and the multi-round config #5 grid
// keep the model's count (more chunks there measured 1-17 % slower).
int64_t adc_qscan_chunks(int64_t nq, int64_t n) {
    int64_t nch = adc_chunks(nq, n, kQB);
    const int64_t qblocks = ceil_div(nq, kQB), step_rows = 64 * kScanWaves;
    const int64_t most = std::max<int64_t>(1, std::min<int64_t>(1024, ceil_div(n, step_rows)));
    if (nch * qblocks <= 256)
        while (nch < most && (nch < 4 || ceil_div(ceil_div(n, nch), step_rows) > 1024)) nch = std::min(most, 2 * nch);
    return nch;
}

// M = 16: the pinned prefetch when the workgroups take more than one round of the chip's CUs
// (adc_qscan_kernel: 8 % faster there, 2 % slower in one round).  M = 32: always.
template <int MC>
hipError_t launch_qscan(const uint32_t* tab, int64_t nq, const uint8_t* codes, int64_t n, int k1, int64_t id_offset,
                        const AdcFilteredLayout& L, float* p1d, uint32_t* p1i, float* p1b, hipStream_t st) {
    constexpr bool kAlways = MC == 2;
    auto kern = L.nch * ceil_div(nq, kQB) > 256 ? adc_qscan_kernel<MC, true> : adc_qscan_kernel<MC, kAlways>;
    const int smem = 16 * MC * 256 * kQB;
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)L.nch, (unsigned)ceil_div(nq, kQB)), dim3(kScanWaves * 64), smem, st, tab,
                       nq, codes, n, k1, id_offset, ceil_div(n, L.nch), p1d, p1i, p1b);
    return hipGetLastError();
}

template <int MC>
hipError_t launch_rerank(const float* lut, int64_t nq, const uint8_t* codes, int64_t id_offset, const uint32_t* p1i,
                         const float* p1b, const AdcFilteredLayout& L, int k, const AdcQStat* qs, float* dists,
                         uint32_t* ids, int* fail_list, int* fail_count, hipStream_t st) {
    const int lut16 = reinterpret_cast<uintptr_t>(lut) % 16 == 0;
    const size_t rsm = (size_t)4 * 16 * MC * 256 * sizeof(float);  // four query LUTs: 64 / 128 KiB
    const hipError_t e = hipFuncSetAttribute((const void*)adc_rerank_kernel<MC>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)rsm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(adc_rerank_kernel<MC>, dim3((unsigned)ceil_div(nq, 4)), dim3(256), rsm, st, lut, nq, codes,
                       id_offset, p1i, p1b, (int)L.parts, L.k1, k, qs, dists, ids, fail_list, fail_count, lut16);
    return hipGetLastError();
}

}  // namespace

// k <= 32: a part's 192 lane candidates (kLaneKeys = 3 per lane) carry the k best rows with room to spare;
// for larger k the per-lane bound (a lane's second-best) sits too close to the k-th distance to
// certify, and the fp32 scan serves those searches.  (The diagnostic flag MIVQ_ADC_FORCE_EXACT
// runs the fp32 scan for every query in the same workspace.)
bool adc_filtered_shape(int M, int ksub, int k) { return ksub == 256 && (M == 16 || M == 32) && k <= 32; }

AdcFilteredLayout adc_filtered_layout(int64_t nq, int64_t n, int M, int k, size_t off) {
    AdcFilteredLayout L{};
    L.k1 = adc_k1(k);
    // the part lists stay within ~1 GiB where the chunk model would ask for more (100k queries:
    // 2 chunks instead of 12, at the same modelled time), and a lane's step index is 16 bits: at
    // most 65535 wave-steps (of 1024 rows) per chunk (adc_filtered_offsets_fit: the scan's
    // 32-bit byte offsets over a chunk)
    const size_t per_chunk = (size_t)kScanWaves * (size_t)nq * (size_t)L.k1 * 8u;
    const int64_t cap = std::max<int64_t>(1, (int64_t)((size_t(1) << 30) / per_chunk));
    L.nch = std::max<int64_t>(std::min<int64_t>(adc_qscan_chunks(nq, n), cap), ceil_div(n, (int64_t)65535 * kScanWaves * 64));
    L.parts = L.nch * kScanWaves;
    L.stats = off;  off = align_up(off + (size_t)nq * sizeof(AdcQStat), 256);
    L.mins = off;   off = align_up(off + (size_t)nq * M * sizeof(float), 256);
    L.tab = off;    off = align_up(off + (size_t)ceil_div(nq, kQB) * M * 256 * kQB, 256);
    L.p1d = off;    off = align_up(off + (size_t)L.parts * nq * L.k1 * sizeof(float), 256);
    L.p1i = off;    off = align_up(off + (size_t)L.parts * nq * L.k1 * sizeof(uint32_t), 256);
    L.p1b = off;    off = align_up(off + (size_t)L.parts * nq * sizeof(float), 256);
    L.fail = off;   off = align_up(off + (size_t)(nq + 1) * sizeof(int), 256);
    L.total = off;
    return L;
}

// adc_qscan_kernel holds the chunk's byte size and its scalar offsets -- up to one wave-step
// (kScanWaves * 64 rows of M bytes) past the chunk -- in int.
bool adc_filtered_offsets_fit(const AdcFilteredLayout& L, int64_t n, int M) {
    return ceil_div(n, L.nch) * M + (int64_t)kScanWaves * 64 * M <= (int64_t)INT_MAX;
}

hipError_t launch_filtered(int M, const float* lut, int64_t nq, const uint8_t* codes, int64_t n, int k,
                           int64_t id_offset, unsigned char* ws, const AdcFilteredLayout& L, float* dists,
                           uint32_t* ids, hipStream_t st) {
    auto* qs = reinterpret_cast<AdcQStat*>(ws + L.stats);
    auto* mins = reinterpret_cast<float*>(ws + L.mins);
    auto* tab = reinterpret_cast<uint32_t*>(ws + L.tab);
    auto* p1d = reinterpret_cast<float*>(ws + L.p1d);
    auto* p1i = reinterpret_cast<uint32_t*>(ws + L.p1i);
    auto* p1b = reinterpret_cast<float*>(ws + L.p1b);
    int* fail_count = reinterpret_cast<int*>(ws + L.fail);
    int* fail_list = fail_count + 1;
    hipError_t e = hipMemsetAsync(fail_count, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    // (round 6: the two launches fused into one workgroup per 16-query block measured slower --
    // 0.422 vs 0.406 ms per 1000 x 1M search: 63 workgroups leave most CUs idle; profiles/r06_s5)
    hipLaunchKernelGGL(adc_qstats_kernel, dim3((unsigned)nq), dim3(256), 0, st, lut, nq, M, mins, qs);
    hipLaunchKernelGGL(adc_qtab_kernel<kQB>, dim3((unsigned)ceil_div(nq, kQB), (unsigned)M), dim3(256), 0, st, lut, nq, M,
                       mins, qs, tab);
    e = M == 16 ? launch_qscan<1>(tab, nq, codes, n, L.k1, id_offset, L, p1d, p1i, p1b, st)
                : launch_qscan<2>(tab, nq, codes, n, L.k1, id_offset, L, p1d, p1i, p1b, st);
    if (e != hipSuccess) return e;
    return M == 16 ? launch_rerank<1>(lut, nq, codes, id_offset, p1i, p1b, L, k, qs, dists, ids, fail_list, fail_count, st)
                   : launch_rerank<2>(lut, nq, codes, id_offset, p1i, p1b, L, k, qs, dists, ids, fail_list, fail_count, st);
}

}  // namespace mivq

