// adc_internal.h — what adc.hip, adc_filtered.hip and exact_search.hip share; the query-block
// dispatch serves the searches over probed lists too (ivf_code.hip, ivf_listpq.hip).
#pragma once

#include "mivq_common.h"

#include <type_traits>

namespace mivq {

constexpr int kScanWaves = 16;  // waves per scan workgroup (adc and flat)

// Row chunks per query block of a scan with QB queries per workgroup (adc.hip).
int64_t adc_chunks(int64_t nq, int64_t n, int QB);

// Host side: f(std::integral_constant<int, QB>) for the queries per scan workgroup, 8, 4, 2 or 1
// (MAX_QB = 4: a caller whose blocks are never wider, so that it has no kernel for 8).
template <int MAX_QB = 8, typename F>
auto with_query_block(int QB, F&& f) {
    if constexpr (MAX_QB >= 8) {
        if (QB == 8) return f(std::integral_constant<int, 8>{});
    }
    switch (QB) {
        case 4: return f(std::integral_constant<int, 4>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: return f(std::integral_constant<int, 1>{});
    }
}

// ---------------------------------------------------------------- filtered search (adc_filtered.hip)
// Eligibility by shape: the workspace is sized on shape alone.
bool adc_filtered_shape(int M, int ksub, int k);

// Byte offsets of the filtered path's workspace regions, starting at `off`.
struct AdcFilteredLayout {
    size_t stats, mins, tab, p1d, p1i, p1b, fail, total;
    int64_t nch, parts;
    int k1;
};
AdcFilteredLayout adc_filtered_layout(int64_t nq, int64_t n, int M, int k, size_t off);

// The integer scan's 32-bit buffer offsets cover a chunk of this layout.
bool adc_filtered_offsets_fit(const AdcFilteredLayout& L, int64_t n, int M);

// Certified queries' top-k into (dists, ids); the others listed at ws + L.fail as {count, ids...}.
hipError_t launch_filtered(int M, const float* lut, int64_t nq, const uint8_t* codes, int64_t n, int k,
                           int64_t id_offset, unsigned char* ws, const AdcFilteredLayout& L, float* dists,
                           uint32_t* ids, hipStream_t st);

}  // namespace mivq
