// codebook1d.hip — data-fitted per-dimension level tables of RankAwareQuantizer on gfx950:
// the globally optimal 1-D k-means (dynamic programming) and k-means++ / Lloyd, bit for bit the
// sequential fp64 arithmetic of the rule in tests/_codebook1d_rule.py.
//
// One workgroup owns one dimension: its n sorted f32 values (a row of cols) and one slot of the
// workspace.  The dimensions are independent, so a launch carries as many as the workspace has
// slots for; each slot's header names its dimension (cb1d_table_kernel writes the headers).
//
//   prefix   ps, pq: the running sums have to be added one value after the other, so the
//            workgroup stages 2048 values in LDS with coalesced loads and lane 0 walks them (two
//            independent add chains); the other lanes only move data.  Also counts the distinct
//            values, which decides the degenerate case of both methods.
//   exact    levels kp = 2 .. k in sequence.  The divide and conquer of one level is walked
//            breadth-first: depth t has the 2^t nodes of a balanced split of [kp, n], whose ranges
//            do not depend on the data (a node finds (mlo, mhi) by t halvings from the root) and
//            whose candidate windows are bounded by the argmins of the two neighbouring ancestors,
//            A[mlo - 1] and A[mhi + 1], written at an earlier depth.  A node is served by a group
//            of G lanes, G the power of two nearest the depth's mean window (64 near the root, 1
//            at the leaves); the first four depths, with fewer nodes than the workgroup has waves,
//            cut each window into one slice per wave.  Each lane keeps the first strict minimum
//            of its stride, lanes and slices combine with ties to the smaller j, which is the
//            sequential scan's answer.
//   seed     k-means++: per centre one sequential sum over the squared distances, staged like
//            the prefix sums; the running sums are kept, so the draw's index is a bisection for
//            the first running sum >= target instead of a second sequential pass.  The
//            update of the distances by the centre just chosen is folded into the next load.
//   lloyd    <= 50 passes of k binary searches and k cell means (lane = cell), the empty-cell
//            repair and the orderings on lane 0 or as a rank sort; k <= 256 = the workgroup.
//
// Every product, quotient and sum is a separate rounding (__d*_rn; the build has
// -ffp-contract=off as well).  No index is formed from the data without a clamp: an unsorted or
// non-finite row gives unspecified levels but touches nothing outside its row and slot.
#include "mivq_common.h"

namespace mivq {
namespace {

constexpr int kCbThreads = 256;
constexpr int kCbExactThreads = 1024;  // the DP's workgroup: 16 waves share a shallow node's window
constexpr int kCbExactWaves = kCbExactThreads / 64;
constexpr int kCbChunk = 2048;       // values staged per step of a sequential sum
constexpr int kCbMaxK = 256;         // 2^8 levels
constexpr int kCbMaxBatch = 256;     // table entries per launch of cb1d_table_kernel
constexpr int64_t kCbMaxN = (int64_t)1 << 26;
constexpr int kCbPasses = 50;
constexpr size_t kCbHeader = 4096;   // per slot: ndist (int32) at 0, its CbEntry at 16, the seeded centres (256 f64) at 2048

struct CbEntry {
    int32_t dim, off, w;             // the dimension a slot serves, the start of its levels, its width 1..8
};

// The host's part of a batch's table, 256 entries to a launch of cb1d_table_kernel (a kernel
// argument, so that nothing is copied from host memory): it goes into the slots' headers, which is
// where the fitting kernels read it, so a batch is as large as the workspace allows.
struct CbBatch {
    int32_t dim[kCbMaxBatch];
    int32_t off[kCbMaxBatch];
    uint8_t w[kCbMaxBatch];
};

struct CbSlot {
    size_t ps, pq, a0, a1, big, total;   // byte offsets; a0/a1: D_prev/D_cur (exact), d2/acc (lloyd); big: A
};

inline CbSlot cb_slot(int64_t n, int32_t w, int32_t method) {
    CbSlot L{};
    const size_t row = align_up(sizeof(double) * (size_t)(n + 1), 256);
    size_t off = kCbHeader;
    L.ps = off; off += row;
    L.pq = off; off += row;
    L.a0 = off; off += row;
    L.a1 = off; off += row;
    L.big = off;
    if (method == MIVQ_CB1D_EXACT) off += align_up(sizeof(int32_t) * (size_t)(n + 1) * (size_t)((1 << w) - 1), 256);
    L.total = off;
    return L;
}

struct CbPtrs {
    const float* s;
    int32_t* ndist;
    double* seeds;
    double *ps, *pq, *a0, *a1;
    int32_t* A;
};

__device__ __forceinline__ CbPtrs cb_ptrs(const float* cols, int64_t n, int dim, char* ws, size_t slot_bytes, CbSlot L) {
    char* base = ws + (size_t)blockIdx.x * slot_bytes;
    CbPtrs p;
    p.s = cols + (int64_t)dim * n;
    p.ndist = reinterpret_cast<int32_t*>(base);
    p.seeds = reinterpret_cast<double*>(base + 2048);
    p.ps = reinterpret_cast<double*>(base + L.ps);
    p.pq = reinterpret_cast<double*>(base + L.pq);
    p.a0 = reinterpret_cast<double*>(base + L.a0);
    p.a1 = reinterpret_cast<double*>(base + L.a1);
    p.A = reinterpret_cast<int32_t*>(base + L.big);
    return p;
}

__device__ __forceinline__ CbEntry cb_entry(const char* ws, size_t slot_bytes) {
    return *reinterpret_cast<const CbEntry*>(ws + (size_t)blockIdx.x * slot_bytes + 16);
}

__global__ __launch_bounds__(kCbMaxBatch) void cb1d_table_kernel(CbBatch bt, int cnt, int slot0, char* __restrict__ ws,
                                                                 size_t slot_bytes) {
    const int b = threadIdx.x;
    if (b < cnt) {
        CbEntry e;
        e.dim = bt.dim[b]; e.off = bt.off[b]; e.w = bt.w[b];
        *reinterpret_cast<CbEntry*>(ws + (size_t)(slot0 + b) * slot_bytes + 16) = e;
    }
}

__device__ __forceinline__ double cb_mean(const double* __restrict__ ps, int i, int j) {
    return __ddiv_rn(__dsub_rn(ps[j], ps[i]), (double)(j - i));
}

__device__ __forceinline__ double cb_sse(const double* __restrict__ ps, const double* __restrict__ pq, int i, int j) {
    const double S = __dsub_rn(ps[j], ps[i]);
    return __dsub_rn(__dsub_rn(pq[j], pq[i]), __ddiv_rn(__dmul_rn(S, S), (double)(j - i)));
}

// std::upper_bound: the number of values <= v in a sorted row (always in [0, n]).
__device__ __forceinline__ int cb_upper(const float* __restrict__ s, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = lo + ((hi - lo) >> 1);
        if (v < s[m]) hi = m; else lo = m + 1;
    }
    return lo;
}

// Lane 0: the distinct values ascending, padded with the last one to k.
__device__ void cb_degenerate(const float* __restrict__ s, int n, int k, float* __restrict__ out) {
    int pos = 0, cnt = 0;
    float last = 0.f;
    while (pos < n && cnt < k) {
        last = s[pos];
        out[cnt++] = last;
        const int nx = cb_upper(s, n, last);
        pos = nx > pos ? nx : pos + 1;
    }
    for (; cnt < k; ++cnt) out[cnt] = last;
}

// Lane 0: drop equal neighbours of lv[0..k) and pad with the last one.
__device__ void cb_unique_pad(const float* lv, int k, float* __restrict__ out) {
    int cnt = 0;
    float last = 0.f;
    for (int i = 0; i < k; ++i) {
        const float v = lv[i];
        if (i == 0 || v != last) { out[cnt++] = v; last = v; }
    }
    for (; cnt < k; ++cnt) out[cnt] = last;
}

// ------------------------------------------------------------------ prefix sums
__global__ __launch_bounds__(kCbThreads) void cb1d_prefix_kernel(const float* __restrict__ cols, int64_t n64,
                                                                 char* __restrict__ ws, size_t slot_bytes,
                                                                 CbSlot L) {
    __shared__ double bs[kCbChunk];
    __shared__ double bq[kCbChunk];
    __shared__ int changes;
    const int tid = threadIdx.x, n = (int)n64;
    const CbPtrs p = cb_ptrs(cols, n64, cb_entry(ws, slot_bytes).dim, ws, slot_bytes, L);
    if (tid == 0) { changes = 0; p.ps[0] = 0.0; p.pq[0] = 0.0; }
    double sum_s = 0.0, sum_q = 0.0;   // lane 0's
    int mine = 0;
    for (int base = 0; base < n; base += kCbChunk) {
        const int len = n - base < kCbChunk ? n - base : kCbChunk;
        __syncthreads();   // the previous chunk has left LDS
        for (int i = tid; i < len; i += kCbThreads) {
            const float f = p.s[base + i];
            const double v = (double)f;
            bs[i] = v;
            bq[i] = __dmul_rn(v, v);
            if (base + i > 0 && f != p.s[base + i - 1]) ++mine;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll 8
            for (int i = 0; i < len; ++i) {
                sum_s = __dadd_rn(sum_s, bs[i]);
                sum_q = __dadd_rn(sum_q, bq[i]);
                bs[i] = sum_s;
                bq[i] = sum_q;
            }
        }
        __syncthreads();
        for (int i = tid; i < len; i += kCbThreads) {
            p.ps[base + i + 1] = bs[i];
            p.pq[base + i + 1] = bq[i];
        }
    }
    if (mine) atomicAdd(&changes, mine);
    __syncthreads();
    if (tid == 0) *p.ndist = changes + 1;
}

// ------------------------------------------------------------------ exact
struct CbNode {
    int mid, lo, hi, arg;   // arg: jlo, the answer when no candidate is a strict minimum
    bool live;
};

// Node `node` of depth t of level kp: t halvings from the root [kp, n], the node index's bits from
// the top; then its window from the argmins of the neighbouring ancestors.
__device__ __forceinline__ CbNode cb_node(const int32_t* A, int n, int kp, int t, int node, bool live) {
    int mlo = kp, mhi = n;
    for (int b = t - 1; b >= 0 && live; --b) {
        const int mid = mlo + ((mhi - mlo) >> 1);
        if ((node >> b) & 1) { mlo = mid + 1; live = mlo <= mhi; }
        else { live = mid > mlo; mhi = mid - 1; }
    }
    CbNode nd;
    nd.live = live;
    nd.mid = mlo + ((mhi - mlo) >> 1);
    nd.lo = 0; nd.hi = -1; nd.arg = 0;
    if (live) {
        const int jlo = mlo == kp ? kp - 1 : A[mlo - 1];
        const int jhi = mhi == n ? n - 1 : A[mhi + 1];
        nd.lo = jlo > kp - 1 ? jlo : kp - 1;
        nd.hi = jhi < nd.mid - 1 ? jhi : nd.mid - 1;
        nd.lo = nd.lo < 0 ? 0 : nd.lo;             // these three hold for every input; kept as guards
        nd.hi = nd.hi > n - 1 ? n - 1 : nd.hi;
        nd.arg = jlo < 0 ? 0 : (jlo > nd.mid - 1 ? nd.mid - 1 : jlo);
    }
    return nd;
}

// The first strict minimum of D_prev[j] + sse(j, mid) over j = a, a + step, .. <= b, continuing
// (best, arg).  Four candidates' loads are issued before the first is used: the chain of compares
// is short, the three loads per candidate are what a lane would otherwise wait for one by one.
__device__ __forceinline__ void cb_scan(const double* Dprev, const double* __restrict__ ps,
                                        const double* __restrict__ pq, int mid, int a, int b, int step,
                                        double& best, int& arg) {
    const double psm = ps[mid], pqm = pq[mid];
    for (int j = a; j <= b; j += 4 * step) {
        double dv[4], sv[4], qv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j + u * step, jc = jj <= b ? jj : b;
            dv[u] = Dprev[jc]; sv[u] = ps[jc]; qv[u] = pq[jc];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j + u * step;
            if (jj <= b) {
                const double S = __dsub_rn(psm, sv[u]);
                const double e = __dsub_rn(__dsub_rn(pqm, qv[u]), __ddiv_rn(__dmul_rn(S, S), (double)(mid - jj)));
                const double v = __dadd_rn(dv[u], e);
                if (v < best) { best = v; arg = jj; }
            }
        }
    }
}

__global__ __launch_bounds__(kCbExactThreads) void cb1d_exact_kernel(const float* __restrict__ cols, int64_t n64,
                                                                     char* __restrict__ ws,
                                                                     size_t slot_bytes, CbSlot L,
                                                                     float* __restrict__ levels,
                                                                     double* __restrict__ sse) {
    __shared__ float lv[kCbMaxK];
    __shared__ double red_v[kCbExactWaves];
    __shared__ int red_j[kCbExactWaves];
    const int tid = threadIdx.x, n = (int)n64;
    const CbEntry en = cb_entry(ws, slot_bytes);
    const int dim = en.dim, w = en.w, k = 1 << w;
    const CbPtrs p = cb_ptrs(cols, n64, dim, ws, slot_bytes, L);
    float* out = levels + en.off;
    if (k >= *p.ndist) {
        if (tid == 0) { cb_degenerate(p.s, n, k, out); sse[dim] = 0.0; }
        return;
    }
    const double* __restrict__ ps = p.ps;
    const double* __restrict__ pq = p.pq;
    double* Dprev = p.a0;
    double* Dcur = p.a1;
    const size_t arow = (size_t)n + 1;
    for (int m = 1 + tid; m <= n; m += kCbExactThreads) Dprev[m] = cb_sse(ps, pq, 0, m);
    __syncthreads();

    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const int wave = tid >> 6, lane = tid & 63;
    for (int kp = 2; kp <= k; ++kp) {
        int32_t* A = p.A + (size_t)(kp - 2) * arow;
        const int R = n - kp + 1;   // >= 1: n > ndist > k >= kp
        for (int t = 0; ((int64_t)1 << t) <= R; ++t) {
            const int nodes = 1 << t;
            if (nodes < kCbExactWaves) {
                // fewer nodes than waves: a node's window is cut into one slice per wave, the slices'
                // minima combined in ascending order (a later slice wins only when strictly smaller)
                const int parts = kCbExactWaves / nodes, node = wave / parts, part = wave % parts;
                const CbNode nd = cb_node(A, n, kp, t, node, true);
                double best = inf;
                int arg = nd.arg;
                if (nd.live) {
                    const int len = nd.hi - nd.lo + 1;
                    const int chunk = len > 0 ? (len + parts - 1) / parts : 0;
                    const int a = nd.lo + part * chunk;
                    const int b = a + chunk - 1 < nd.hi ? a + chunk - 1 : nd.hi;
                    cb_scan(Dprev, ps, pq, nd.mid, a + lane, b, 64, best, arg);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double vo = __shfl_xor(best, o);
                    const int jo = __shfl_xor(arg, o);
                    if (vo < best || (vo == best && jo < arg)) { best = vo; arg = jo; }
                }
                if (lane == 0) { red_v[wave] = best; red_j[wave] = arg; }
                __syncthreads();
                if (nd.live && part == 0 && lane == 0) {
                    for (int q = 1; q < parts; ++q)
                        if (red_v[wave + q] < best) { best = red_v[wave + q]; arg = red_j[wave + q]; }
                    Dcur[nd.mid] = best;
                    A[nd.mid] = arg;
                }
            } else {
                const int avg = R / nodes + 1;
                int G = 1;
                while (G < 64 && G < avg) G <<= 1;
                const int per = kCbExactThreads / G, gi = tid / G, gl = tid % G;
                for (int nb = 0; nb < nodes; nb += per) {
                    const int node = nb + gi;
                    const CbNode nd = cb_node(A, n, kp, t, node, node < nodes);
                    double best = inf;
                    int arg = nd.arg;
                    if (nd.live) cb_scan(Dprev, ps, pq, nd.mid, nd.lo + gl, nd.hi, G, best, arg);
                    for (int o = G >> 1; o > 0; o >>= 1) {
                        const double vo = __shfl_xor(best, o);
                        const int jo = __shfl_xor(arg, o);
                        if (vo < best || (vo == best && jo < arg)) { best = vo; arg = jo; }
                    }
                    if (nd.live && gl == 0) { Dcur[nd.mid] = best; A[nd.mid] = arg; }
                }
            }
            __syncthreads();   // this depth's A bounds the next depth's windows
        }
        double* sw = Dprev; Dprev = Dcur; Dcur = sw;
    }

    if (tid == 0) {
        int m = n;
        for (int kk = k; kk >= 1; --kk) {
            int j = kk > 1 ? p.A[(size_t)(kk - 2) * arow + m] : 0;
            j = j < kk - 1 ? kk - 1 : j;
            j = j > m - 1 ? m - 1 : j;
            lv[kk - 1] = (float)cb_mean(ps, j, m);
            m = j;
        }
        cb_unique_pad(lv, k, out);
        sse[dim] = Dprev[n];
    }
}

// ------------------------------------------------------------------ k-means++ seeding
// A uniform index in [0, n) from raw 64-bit draws: the high half of draw * n, a draw whose low half
// falls under 2^64 mod n rejected (the draws that remain bound the retries).
__device__ int cb_draw_index(const uint64_t* __restrict__ draws, int ndraws, int& at, uint32_t n) {
    uint64_t r = draws[at < ndraws ? at : ndraws - 1];
    ++at;
    uint64_t low = r * (uint64_t)n;
    if (low < n) {
        const uint64_t thr = (0ull - (uint64_t)n) % n;
        while (low < thr && at < ndraws) {
            r = draws[at++];
            low = r * (uint64_t)n;
        }
    }
    const uint64_t idx = __umul64hi(r, (uint64_t)n);
    return idx < n ? (int)idx : (int)n - 1;
}

// Rank sort of v[0..k) (lane = element, ties by index) into out; the caller synchronises.
template <typename T>
__device__ __forceinline__ void cb_rank_sort(const T* v, int k, T* out, int tid) {
    if (tid < k) {
        const T x = v[tid];
        int r = 0;
        for (int j = 0; j < k; ++j) r += (v[j] < x || (v[j] == x && j < tid)) ? 1 : 0;
        out[r] = x;
    }
}

// Lane 0: c[i] = c[i-1] + max(1e-9, |c[i-1]| 1e-6) wherever c[i] <= c[i-1].
__device__ void cb_nudge(double* c, int k) {
    for (int i = 1; i < k; ++i) {
        if (c[i] <= c[i - 1]) {
            const double g = __dmul_rn(fabs(c[i - 1]), 1e-6);
            c[i] = __dadd_rn(c[i - 1], 1e-9 < g ? g : 1e-9);
        }
    }
}

__global__ __launch_bounds__(kCbThreads) void cb1d_seed_kernel(const float* __restrict__ cols, int64_t n64,
                                                               char* __restrict__ ws, size_t slot_bytes, CbSlot L,
                                                               const uint64_t* __restrict__ draws, int ndraws) {
    __shared__ double buf[kCbChunk];
    __shared__ double cen[kCbMaxK];
    __shared__ double srt[kCbMaxK];
    __shared__ int sh_chosen;
    const int tid = threadIdx.x, n = (int)n64;
    const CbEntry en = cb_entry(ws, slot_bytes);
    const int k = 1 << en.w;
    const CbPtrs p = cb_ptrs(cols, n64, en.dim, ws, slot_bytes, L);
    if (k >= *p.ndist) return;
    const float* __restrict__ s = p.s;
    double* d2 = p.a0;
    double* acc = p.a1;
    int at = 0;   // lane 0's place in the draws
    if (tid == 0) sh_chosen = cb_draw_index(draws, ndraws, at, (uint32_t)n);
    __syncthreads();
    for (int c = 1; c <= k; ++c) {
        const double cv = (double)s[sh_chosen];   // centre c - 1
        if (tid == 0) cen[c - 1] = cv;
        if (c == k) break;
        // one pass: fold centre c - 1 into d2, keep the running sums
        double sum = 0.0;   // lane 0's
        for (int base = 0; base < n; base += kCbChunk) {
            const int len = n - base < kCbChunk ? n - base : kCbChunk;
            __syncthreads();
            for (int i = tid; i < len; i += kCbThreads) {
                const double diff = __dsub_rn((double)s[base + i], cv);
                double dd = __dmul_rn(diff, diff);
                if (c > 1) {
                    const double old = d2[base + i];
                    dd = dd < old ? dd : old;
                }
                d2[base + i] = dd;
                buf[i] = dd;
            }
            __syncthreads();
            if (tid == 0) {
#pragma unroll 8
                for (int i = 0; i < len; ++i) {
                    sum = __dadd_rn(sum, buf[i]);
                    buf[i] = sum;
                }
            }
            __syncthreads();
            for (int i = tid; i < len; i += kCbThreads) acc[base + i] = buf[i];
        }
        __syncthreads();
        if (tid == 0) {
            if (sum <= 0.0) {
                sh_chosen = cb_draw_index(draws, ndraws, at, (uint32_t)n);
            } else {
                const uint64_t r = draws[at < ndraws ? at : ndraws - 1];
                ++at;
                double u = __ddiv_rn((double)r, 18446744073709551616.0);
                if (!(u < 1.0)) u = 0x1.fffffffffffffp-1;   // the largest double below 1
                const double target = __dmul_rn(u, sum);
                // the first running sum >= target (n - 1 if none): sums of non-negative terms do not
                // decrease, so they are bisected
                int lo = 0, hi = n;
                while (lo < hi) {
                    const int m = lo + ((hi - lo) >> 1);
                    if (acc[m] >= target) hi = m; else lo = m + 1;
                }
                sh_chosen = lo < n ? lo : n - 1;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    cb_rank_sort(cen, k, srt, tid);
    __syncthreads();
    if (tid == 0) cb_nudge(srt, k);
    __syncthreads();
    if (tid < k) p.seeds[tid] = srt[tid];
}

// ------------------------------------------------------------------ Lloyd passes
__global__ __launch_bounds__(kCbThreads) void cb1d_lloyd_kernel(const float* __restrict__ cols, int64_t n64,
                                                                char* __restrict__ ws, size_t slot_bytes, CbSlot L,
                                                                float* __restrict__ levels, double* __restrict__ sse) {
    __shared__ double c[kCbMaxK];
    __shared__ double tmp[kCbMaxK];    // moves, then cell costs, then the sort's output
    __shared__ float lv[kCbMaxK];
    __shared__ float lvs[kCbMaxK];
    __shared__ int bnd[kCbMaxK + 1];
    __shared__ int sh_state;           // 0: next pass, 1: repaired, 2: converged
    const int tid = threadIdx.x, n = (int)n64;
    const CbEntry en = cb_entry(ws, slot_bytes);
    const int dim = en.dim, w = en.w, k = 1 << w;
    const CbPtrs p = cb_ptrs(cols, n64, dim, ws, slot_bytes, L);
    float* out = levels + en.off;
    if (k >= *p.ndist) {
        if (tid == 0) { cb_degenerate(p.s, n, k, out); sse[dim] = 0.0; }
        return;
    }
    const float* __restrict__ s = p.s;
    const double* __restrict__ ps = p.ps;
    const double* __restrict__ pq = p.pq;
    if (tid < k) c[tid] = p.seeds[tid];
    __syncthreads();

    // bnd[i] = #{ s <= (float)(0.5 (c[i-1] + c[i])) }, made non-decreasing; bnd[0] = 0, bnd[k] = n
    auto assign = [&]() __attribute__((always_inline)) {
        if (tid >= 1 && tid < k) bnd[tid] = cb_upper(s, n, (float)__dmul_rn(0.5, __dadd_rn(c[tid - 1], c[tid])));
        if (tid == 0) { bnd[0] = 0; bnd[k] = n; }
        __syncthreads();
        if (tid == 0)
            for (int i = 1; i < k; ++i)
                if (bnd[i] < bnd[i - 1]) bnd[i] = bnd[i - 1];
        __syncthreads();
    };

    int repairs = 0;   // lane 0's
    const double tol = (double)1e-6f;
    for (int pass = 0; pass < kCbPasses; ++pass) {
        assign();
        if (tid < k) {
            const int a = bnd[tid], b = bnd[tid + 1];
            const double nc = b > a ? cb_mean(ps, a, b) : c[tid];
            tmp[tid] = fabs(__dsub_rn(nc, c[tid]));
            c[tid] = nc;   // a lane reads and writes its own centre only
        }
        __syncthreads();
        if (tid == 0) {
            double maxmove = 0.0;
            for (int i = 0; i < k; ++i) maxmove = maxmove < tmp[i] ? tmp[i] : maxmove;
            int state = maxmove < tol ? 2 : 0;
            if (repairs < 2 * k) {
                int e = k;
                for (int i = 0; i < k; ++i)
                    if (bnd[i + 1] <= bnd[i]) { e = i; break; }
                if (e < k) {
                    int best = k;
                    double bsse = -1.0;
                    for (int j = 0; j < k; ++j) {
                        const int a = bnd[j], b = bnd[j + 1];
                        if (b > a + 1) {
                            const double v = cb_sse(ps, pq, a, b);
                            if (v > bsse) { bsse = v; best = j; }
                        }
                    }
                    if (best < k) {
                        const int a = bnd[best], b = bnd[best + 1], m = a + ((b - a) >> 1);
                        c[best] = cb_mean(ps, a, m);
                        c[e] = cb_mean(ps, m, b);
                        ++repairs;
                        state = 1;
                    }
                }
            }
            sh_state = state;
        }
        __syncthreads();
        const int state = sh_state;
        if (state == 1) {
            cb_rank_sort(c, k, tmp, tid);
            __syncthreads();
            if (tid == 0) cb_nudge(tmp, k);
            __syncthreads();
            if (tid < k) c[tid] = tmp[tid];
            __syncthreads();
            continue;
        }
        if (state == 2) break;
    }

    assign();
    if (tid < k) {
        const int a = bnd[tid], b = bnd[tid + 1];
        tmp[tid] = b > a ? cb_sse(ps, pq, a, b) : 0.0;
        lv[tid] = (float)c[tid];
    }
    __syncthreads();
    cb_rank_sort(lv, k, lvs, tid);
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int i = 0; i < k; ++i)
            if (bnd[i + 1] > bnd[i]) total = __dadd_rn(total, tmp[i]);
        sse[dim] = total;
        cb_unique_pad(lvs, k, out);
    }
}

}  // namespace
}  // namespace mivq

using namespace mivq;

extern "C" size_t mivq_codebook1d_workspace_bytes(int64_t n, int32_t max_width, int32_t method, int32_t dims_at_once) {
    if (n < 0 || n > kCbMaxN || max_width < 0 || max_width > 8 || dims_at_once < 1) return 0;
    if (method != MIVQ_CB1D_EXACT && method != MIVQ_CB1D_LLOYD) return 0;
    return cb_slot(n, max_width, method).total * (size_t)dims_at_once;
}

extern "C" int mivq_codebook1d_fit(const float* cols, int64_t n, int32_t d, const int32_t* width, const int32_t* lv_off,
                                   int32_t method, const uint64_t* draws, int32_t ndraws, void* workspace,
                                   size_t workspace_bytes, float* levels, double* sse, void* stream) {
    MIVQ_REQUIRE(n >= 0 && d >= 0, MIVQ_ERR_INVALID, "codebook1d_fit: bad sizes n=%lld d=%d", (long long)n, d);
    MIVQ_REQUIRE(method == MIVQ_CB1D_EXACT || method == MIVQ_CB1D_LLOYD, MIVQ_ERR_INVALID,
                 "codebook1d_fit: unknown method %d", method);
    if (n == 0 || d == 0) return MIVQ_OK;
    MIVQ_REQUIRE(width && lv_off, MIVQ_ERR_INVALID, "codebook1d_fit: null width / lv_off");
    int32_t maxw = 0;
    for (int32_t j = 0; j < d; ++j) {
        MIVQ_REQUIRE(width[j] >= 0 && width[j] <= 8, MIVQ_ERR_INVALID, "codebook1d_fit: width[%d]=%d outside 0..8", j,
                     width[j]);
        MIVQ_REQUIRE(lv_off[j] >= 0 && lv_off[j + 1] - lv_off[j] == (1 << width[j]), MIVQ_ERR_INVALID,
                     "codebook1d_fit: lv_off[%d..] does not hold 2^%d levels", j, width[j]);
        maxw = width[j] > maxw ? width[j] : maxw;
    }
    if (maxw == 0) return MIVQ_OK;
    MIVQ_REQUIRE(n <= kCbMaxN, MIVQ_ERR_UNSUPPORTED, "codebook1d_fit: n=%lld above %lld", (long long)n,
                 (long long)kCbMaxN);
    MIVQ_REQUIRE(workspace && workspace_bytes >= cb_slot(n, maxw, method).total, MIVQ_ERR_WORKSPACE,
                 "codebook1d_fit: workspace %zu < %zu bytes for one dimension of %d bits", workspace_bytes,
                 cb_slot(n, maxw, method).total, maxw);
    MIVQ_REQUIRE(cols && levels && sse, MIVQ_ERR_INVALID, "codebook1d_fit: null pointer");
    MIVQ_REQUIRE(method != MIVQ_CB1D_LLOYD || (draws && ndraws >= (1 << maxw)), MIVQ_ERR_INVALID,
                 "codebook1d_fit: lloyd needs at least %d draws, got %d", 1 << maxw, ndraws);

    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    // dimensions by descending width (index order within a width), so that the long fits start
    // first and a batch's slots are sized by its first dimension
    int cw = 8;
    int32_t cj = 0;
    auto next = [&]() -> int32_t {
        for (; cw >= 1; --cw, cj = 0)
            for (; cj < d; ++cj)
                if (width[cj] == cw) return cj++;
        return -1;
    };
    int32_t first = next();
    while (first >= 0) {
        const int bw = width[first];
        const CbSlot L = cb_slot(n, bw, method);
        const size_t room = workspace_bytes / L.total;   // >= 1: the workspace holds a slot of the widest
        const int64_t cap = room < (size_t)0x7fffffff ? (int64_t)room : 0x7fffffff;
        int64_t cnt = 0;
        while (first >= 0 && cnt < cap) {
            CbBatch bt;
            int c = 0;
            for (; first >= 0 && c < kCbMaxBatch && cnt + c < cap; ++c, first = next()) {
                bt.dim[c] = first;
                bt.off[c] = lv_off[first];
                bt.w[c] = (uint8_t)width[first];
            }
            hipLaunchKernelGGL(cb1d_table_kernel, dim3(1), dim3(kCbMaxBatch), 0, st, bt, c, (int)cnt, ws, L.total);
            cnt += c;
        }
        if (cnt == 0) break;
        const dim3 grid((unsigned)cnt), block(kCbThreads);
        hipLaunchKernelGGL(cb1d_prefix_kernel, grid, block, 0, st, cols, n, ws, L.total, L);
        if (method == MIVQ_CB1D_EXACT) {
            hipLaunchKernelGGL(cb1d_exact_kernel, grid, dim3(kCbExactThreads), 0, st, cols, n, ws, L.total, L, levels, sse);
        } else {
            hipLaunchKernelGGL(cb1d_seed_kernel, grid, block, 0, st, cols, n, ws, L.total, L, draws, (int)ndraws);
            hipLaunchKernelGGL(cb1d_lloyd_kernel, grid, block, 0, st, cols, n, ws, L.total, L, levels, sse);
        }
        const int rc = check_launch("codebook1d_fit");
        if (rc != MIVQ_OK) return rc;
    }
    return MIVQ_OK;
}
