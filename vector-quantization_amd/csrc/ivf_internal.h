// ivf_internal.h — what the searches over probed lists share (ivf_rabitq.hip, ivf_code.hip): the
// (query, probe slot) pairs are sorted by list, and each list's pairs are cut into work items.
#pragma once

#include "mivq_common.h"

namespace mivq {

// poff: the bucket offsets of the sorted pairs (nlist + 2 entries; bucket nlist = skipped slots).
// items[i] = (list, first sorted pair of the block of PPI pairs), nitems = their count
// (<= ceil(pairs / PPI) + nlist).  One workgroup.
template <int PPI>
__global__ __launch_bounds__(1024) void ivf_items_kernel(const int64_t* __restrict__ poff, int nlist,
                                                         uint2* __restrict__ items, uint32_t* __restrict__ nitems) {
    __shared__ int64_t part[1024];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nlist; base += 1024) {
        const int l = base + threadIdx.x;
        const int64_t p0 = l < nlist ? poff[l] : 0;
        const int64_t v = l < nlist ? (poff[l + 1] - p0 + PPI - 1) / PPI : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
            const int64_t add = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        const int64_t first = carry + part[threadIdx.x] - v;
        for (int64_t b = 0; b < v; ++b) items[first + b] = make_uint2((uint32_t)l, (uint32_t)(p0 + b * PPI));
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *nitems = (uint32_t)carry;
}

}  // namespace mivq
