// hdbscan.hip -- density-adaptive clusters beside dbscan.hip: HDBSCAN over 3-D points, for the label generators and the ICP-Flow baseline
// (`ssl_label.hdbscan`; the SeFlow papers name HDBSCAN for this step, himo_amd/seflow/ssl_label.py).
//
// PARITY UNPINNED: the reference's label generator is in the absent OpenSceneFlow submodule.  This is this build's own rule, checked
// bit for bit against a numpy restatement of it (tests/hdbscan_ref.py), and against sklearn.cluster.HDBSCAN only as far as the tie
// order allows (tests/test_hdbscan_cpu.py).
//
// The rule -- "HDBSCAN, v1" (normative; also the module docstring of ssl_label.hdbscan)
//   Inputs: xyz [n][pitch >= 3] float32, optional skip [n], min_cluster_size m >= 2, min_samples k with 1 <= k <= 32.  A point whose
//   skip flag is set, or that holds a NaN, takes no part and gets label 0.  P = the participating points.  |P| < max(k, 2): every
//   label is 0.
//    1. Squared distance.  d2(i,j) = (dx*dx + dy*dy) + dz*dz in float32, every operation rounding on its own (this file is built with
//       -ffp-contract=off), dx = x_i - x_j.  All comparisons are on squared values; no square root is taken on the device.
//    2. Core.  core2(i) = the k-th smallest of {d2(i,j) : j in P}, the point itself counting (k = 1 gives 0: sklearn's convention).
//    3. Mutual reachability.  w(i,j) = max(core2(i), core2(j), d2(i,j)).
//    4. Edge order.  Edges are totally ordered by (w, lo, hi), lo < hi the ORIGINAL point indices.  Ties in w are the normal case
//       (every neighbour inside a point's core radius ties), so the order is part of the rule.
//    5. Tree.  The MST is the unique minimum spanning tree of the complete graph on P under that strict order.
//    6. Dendrogram.  The MST edges in ascending order, merged: the component holding lo is the LEFT child, the one holding hi the
//       RIGHT child; the node's distance is sqrt((double)w).
//    7. Condensed tree.  Walk from the root with an explicit stack, right pushed before left; lambda = 1 / max(distance, 1e-9).
//       Both children >= m: two new clusters are born at lambda, left numbered before right.  Both < m: all their points fall out of
//       the current cluster at lambda.  Otherwise the small side's points fall out and the big side continues under the same id.
//    8. Stability.  Float64: S(c) = sum over c's rows of (lambda_row - lambda_birth(c)) * size_row, in the order the walk emitted them.
//    9. Selection (excess of mass).  Clusters from the highest id down; the root is never selected.  A leaf is selected.  An inner
//       cluster whose children's S sum is > its own takes that sum and stays unselected; otherwise it is selected and all its
//       descendants are deselected (allow_single_cluster = False, no selection epsilon).
//   10. Labels.  A point gets the nearest selected ancestor of the cluster it fell out of, or 0; clusters are numbered 1..K by their
//       lowest point index.  The result is a pure function of the input.
//
// Structure.  himo_hdbscan_mst (device, steps 1-5, never synchronises) and himo_hdbscan_tree (host, plain C++, steps 6-10).
//   compaction   P is compacted IN INDEX ORDER (block counts, then a block scan: two launches), so comparing compacted indices is
//                comparing original ones; the original index rides along and is what the edge list holds.
//   core2        THE BRUTE-FORCE FORM SHIPPED: every point scans all of P in LDS tiles and keeps its k smallest squared distances in a
//                sorted list (LDS, one column per thread: no bank conflicts; an insertion only when a distance beats the k-th).  Exact
//                by construction; one quadratic pass.  The ring search over dbscan.hip's BEV cell grid is not built (grid_w / grid_h
//                of himo_hdbscan_workspace_bytes are kept for it).
//   Boruvka      ceil(log2 n) rounds launched unconditionally; a round whose component count is already 1 (or a call with
//                |P| < max(k, 2)) returns at once from a device word.  Per round: (a) tiled all-pairs search, the hot path: a block
//                stages 256 rows of (x, y, z, core2) and their component ids in LDS, every lane reads the SAME row at a time (a
//                broadcast read), a thread carries 4 query points in registers so each LDS read feeds 4 pairs; the candidate range
//                is split over blockIdx.y and merged with a 64-bit atomicMin on (w bits << 32 | j) -- for a fixed point that IS the
//                order (w, lo, hi); (b) per-component minimum in two passes: atomicMin on w's bits (non-negative floats order as
//                integers), then atomicMin on (lo << 32 | hi) among the points that hold that w; (c) hook along the chosen edges with
//                unionfind.h (a root ends as its component's lowest index), each edge emitted once -- when both components chose
//                it, by the one that holds lo -- through a counter; (d) flatten the component ids and count the components.
//   cost         QUADRATIC per round, by decision: rounds x |P|^2 pairs at ~14 vector operations each.  No pruning.
// No kernel waits on another block; no loop is unbounded apart from the union-find's own retry (unionfind.h).
#include "himo_common.h"
#include "blockops.h"
#include "unionfind.h"
#include <math.h>
#include <algorithm>
#include <vector>

namespace himo {

constexpr int kHdTile = 256;           // candidate rows staged per LDS tile (4 KB + 1 KB of component ids)
constexpr int kHdQ = 4;                // query points a thread of the search kernel carries
constexpr int kHdMaxK = 32;
constexpr unsigned long long kHdNone = ~0ull;
// device words: [r] = the components alive at the start of round r (0 = nothing to do); n < 2^31 takes 31 rounds at most
constexpr int kHdWords = 64;

// participating points of every block of 1024; core2 of every point starts at +inf (what a point that takes no part keeps)
__global__ __launch_bounds__(1024) void hd_count_kernel(int n, const float* __restrict__ xyz, int pitch, const unsigned char* __restrict__ skip,
                                                        int* __restrict__ block_sum, float* __restrict__ core2_out) {
    __shared__ int wsum[16];
    const int i = blockIdx.x * 1024 + threadIdx.x;
    const bool in = i < n && db_takes_part(xyz, pitch, skip, i);
    if (i < n && core2_out) core2_out[i] = INFINITY;
    const int c = __popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < 16; ++k) t += wsum[k];
        block_sum[blockIdx.x] = t;
    }
}

// every participating point to its rank among them; the state of round 0: every point its own component
__global__ __launch_bounds__(1024) void hd_compact_kernel(int n, const float* __restrict__ xyz, int pitch, const unsigned char* __restrict__ skip,
                                                          const int* __restrict__ block_sum, int min_samples, float4* __restrict__ rows,
                                                          int* __restrict__ index, int* __restrict__ parent, int* __restrict__ comp,
                                                          unsigned long long* __restrict__ best, unsigned* __restrict__ compw,
                                                          unsigned long long* __restrict__ complh, int* __restrict__ words, int* __restrict__ counts) {
    __shared__ int wsum[16];
    __shared__ int s_before, s_all;
    if (threadIdx.x < 64) {                                     // one wave: the blocks before this one, and all of them
        int before, all;
        tiles_before_and_all(block_sum, before, all);
        if (threadIdx.x == 0) { s_before = before; s_all = all; }
    }
    const int i = blockIdx.x * 1024 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool in = i < n && db_takes_part(xyz, pitch, skip, i);
    const unsigned long long mask = __ballot(in);
    if (lane == 0) wsum[w] = __popcll(mask);
    __syncthreads();
    if (in) {
        int pos = s_before + __popcll(mask & ((1ull << lane) - 1ull));
        for (int k = 0; k < w; ++k) pos += wsum[k];
        rows[pos] = float4{xyz[(int64_t)i * pitch], xyz[(int64_t)i * pitch + 1], xyz[(int64_t)i * pitch + 2], __int_as_float(i)};
        index[pos] = i; parent[pos] = pos; comp[pos] = pos;
        best[pos] = kHdNone; compw[pos] = 0xffffffffu; complh[pos] = kHdNone;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int need = min_samples > 2 ? min_samples : 2;
        words[0] = s_all >= need ? s_all : 0;
        counts[0] = s_all; counts[1] = 0; counts[2] = 0; counts[3] = 0;
    }
}

// core2: one thread per point, all of P in tiles; the k smallest squared distances in a sorted LDS column per thread
__global__ __launch_bounds__(256) void hd_core_kernel(const int* __restrict__ counts, const float4* __restrict__ rows, int k,
                                                      float* __restrict__ core2c, float* __restrict__ core2_out) {
    __shared__ float4 tile[kHdTile];
    __shared__ float lst[kHdMaxK * 256];
    const int np = counts[0];
    if ((int)blockIdx.x * 256 >= np) return;
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool valid = i < np;
    const float4 p = rows[valid ? i : 0];
    for (int s = 0; s < k; ++s) lst[s * 256 + tid] = INFINITY;
    float kth = INFINITY;
    for (int j0 = 0; j0 < np; j0 += kHdTile) {
        __syncthreads();
        if (j0 + tid < np) tile[tid] = rows[j0 + tid];
        __syncthreads();
        const int cnt = np - j0 < kHdTile ? np - j0 : kHdTile;
        if (!valid) continue;
        for (int jj = 0; jj < cnt; ++jj) {
            const float4 q = tile[jj];
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < kth) {
                int s = k - 1;
                while (s > 0 && lst[(s - 1) * 256 + tid] > d2) { lst[s * 256 + tid] = lst[(s - 1) * 256 + tid]; --s; }
                lst[s * 256 + tid] = d2;
                kth = lst[(k - 1) * 256 + tid];
            }
        }
    }
    if (valid) {
        core2c[i] = kth;
        if (core2_out) core2_out[__float_as_int(p.w)] = kth;
    }
}

// (a) every point's least edge (w, j) to a point of another component, over the candidate chunk of blockIdx.y
__global__ __launch_bounds__(256) void hd_search_kernel(const int* __restrict__ words, int round, const int* __restrict__ counts,
                                                        const float4* __restrict__ rows, const float* __restrict__ core2c,
                                                        const int* __restrict__ comp, int chunk, unsigned long long* __restrict__ best) {
    __shared__ float4 tile[kHdTile];
    __shared__ int tcomp[kHdTile];
    if (words[round] <= 1) return;
    const int np = counts[0], tid = threadIdx.x;
    const int q0 = blockIdx.x * (256 * kHdQ), j_begin = blockIdx.y * chunk;
    if (q0 >= np || j_begin >= np) return;
    const int j_end = j_begin + chunk < np ? j_begin + chunk : np;
    float px[kHdQ], py[kHdQ], pz[kHdQ], pc[kHdQ], bw[kHdQ];
    int mine[kHdQ], bj[kHdQ];
#pragma unroll
    for (int r = 0; r < kHdQ; ++r) {
        const int i = q0 + r * 256 + tid;
        const bool valid = i < np;
        const float4 p = rows[valid ? i : 0];
        px[r] = p.x; py[r] = p.y; pz[r] = p.z;
        pc[r] = core2c[valid ? i : 0];
        mine[r] = valid ? comp[i] : -1;
        bw[r] = INFINITY; bj[r] = -1;
    }
    for (int j0 = j_begin; j0 < j_end; j0 += kHdTile) {
        __syncthreads();
        if (j0 + tid < j_end) {
            const float4 q = rows[j0 + tid];
            tile[tid] = float4{q.x, q.y, q.z, core2c[j0 + tid]};
            tcomp[tid] = comp[j0 + tid];
        }
        __syncthreads();
        const int cnt = j_end - j0 < kHdTile ? j_end - j0 : kHdTile;
        for (int jj = 0; jj < cnt; ++jj) {
            const float4 q = tile[jj];                          // the same address in every lane: a broadcast read
            const int qc = tcomp[jj];
#pragma unroll
            for (int r = 0; r < kHdQ; ++r) {
                const float dx = px[r] - q.x, dy = py[r] - q.y, dz = pz[r] - q.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                const float cc = pc[r] > q.w ? pc[r] : q.w;
                const float w = cc > d2 ? cc : d2;
                // j ascends, so a strict < keeps the lowest j among equal w; w <= +inf: bj < 0 admits a first edge of infinite weight
                if (qc != mine[r] && (w < bw[r] || bj[r] < 0)) { bw[r] = w; bj[r] = j0 + jj; }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kHdQ; ++r) {
        const int i = q0 + r * 256 + tid;
        if (i < np && bj[r] >= 0)
            atomicMin(&best[i], ((unsigned long long)__float_as_uint(bw[r]) << 32) | (unsigned)bj[r]);
    }
}

// (b) first pass: the least w of every component
__global__ __launch_bounds__(256) void hd_compw_kernel(const int* __restrict__ words, int round, const int* __restrict__ counts,
                                                       const int* __restrict__ comp, const unsigned long long* __restrict__ best,
                                                       unsigned* __restrict__ compw) {
    if (words[round] <= 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= counts[0]) return;
    const unsigned long long b = best[i];
    if (b != kHdNone) atomicMin(&compw[comp[i]], (unsigned)(b >> 32));
}
// (b) second pass: the least (lo, hi) among the component's points that hold that w
__global__ __launch_bounds__(256) void hd_complh_kernel(const int* __restrict__ words, int round, const int* __restrict__ counts,
                                                        const int* __restrict__ comp, const unsigned long long* __restrict__ best,
                                                        const unsigned* __restrict__ compw, unsigned long long* __restrict__ complh) {
    if (words[round] <= 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= counts[0]) return;
    const unsigned long long b = best[i];
    if (b == kHdNone || (unsigned)(b >> 32) != compw[comp[i]]) return;
    const unsigned j = (unsigned)b, lo = (unsigned)i < j ? (unsigned)i : j, hi = (unsigned)i < j ? j : (unsigned)i;
    atomicMin(&complh[comp[i]], ((unsigned long long)lo << 32) | hi);
}
// (c) every component hooks along its edge; the edge is emitted once
__global__ __launch_bounds__(256) void hd_hook_kernel(const int* __restrict__ words, int round, int* __restrict__ counts, const int* __restrict__ comp,
                                                      const unsigned* __restrict__ compw, const unsigned long long* __restrict__ complh,
                                                      const int* __restrict__ index, int* __restrict__ parent, int cap,
                                                      unsigned* __restrict__ edges) {
    if (words[round] <= 1) return;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= counts[0] || comp[c] != c) return;
    const unsigned long long lh = complh[c];
    if (lh == kHdNone) return;
    const int lo = (int)(lh >> 32), hi = (int)(unsigned)lh;
    const int c_lo = comp[lo], c_hi = comp[hi];
    const int other = c_lo == c ? c_hi : c_lo;
    if (complh[other] != lh || c_lo == c) {                     // chosen by both: the component that holds lo emits
        const int slot = atomicAdd(&counts[1], 1);
        if (slot < cap) {
            edges[(size_t)slot * 3] = compw[c]; edges[(size_t)slot * 3 + 1] = (unsigned)index[lo]; edges[(size_t)slot * 3 + 2] = (unsigned)index[hi];
        }
    }
    db_union(parent, lo, hi);
}
// (d) component ids for the next round, their number, and the round's per-point and per-component minima cleared
__global__ __launch_bounds__(256) void hd_flatten_kernel(int* __restrict__ words, int round, int* __restrict__ counts, const int* __restrict__ parent,
                                                         int* __restrict__ comp, unsigned long long* __restrict__ best, unsigned* __restrict__ compw,
                                                         unsigned long long* __restrict__ complh) {
    if (words[round] <= 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) counts[2] = round + 1;
    if (i >= counts[0]) return;
    const int root = db_find(parent, i);
    comp[i] = root;
    if (root == i) atomicAdd(&words[round + 1], 1);
    best[i] = kHdNone; compw[i] = 0xffffffffu; complh[i] = kHdNone;
}

struct HdLayout {
    size_t words, block_sum, rows, core2c, parent, comp, best, compw, complh, total;
};
static HdLayout hd_layout(int n) {
    HdLayout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += round_up(bytes, 256); return at; };
    L.words = take(kHdWords * 4); L.block_sum = take(((size_t)n / 1024 + 2) * 4); L.rows = take((size_t)n * 16);
    L.core2c = take((size_t)n * 4); L.parent = take((size_t)n * 4); L.comp = take((size_t)n * 4); L.best = take((size_t)n * 8);
    L.compw = take((size_t)n * 4); L.complh = take((size_t)n * 8);
    L.total = o;
    return L;
}

}  // namespace himo

using namespace himo;

// (grid_w, grid_h: the BEV cell grid of the ring search for core2, which is not built -- the brute-force form keeps no cell table;
// they are checked like himo_dbscan's so that a caller is ready for it)
extern "C" size_t himo_hdbscan_workspace_bytes(int n, int grid_w, int grid_h) {
    if (n < 0 || grid_w < 1 || grid_h < 1) return 0;
    return hd_layout(n).total + 256;
}

extern "C" int himo_hdbscan_mst(int n, const float* d_xyz, int pitch, const unsigned char* d_skip, int min_samples, int32_t* d_counts,
                                int32_t* d_index, float* d_core2, uint32_t* d_edges, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || pitch < 3 || min_samples < 1 || min_samples > kHdMaxK || !d_counts) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!d_xyz || !d_index)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 1 && !d_edges) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_workspace || workspace_bytes < hd_layout(n).total + 256 || !aligned16(d_workspace)) return HIMO_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIMO_HIP(hipMemsetAsync(d_counts, 0, 16, s));
        return HIMO_OK;
    }
    const HdLayout L = hd_layout(n);
    char* w = reinterpret_cast<char*>(d_workspace);
    int* words = reinterpret_cast<int*>(w + L.words); int* block_sum = reinterpret_cast<int*>(w + L.block_sum);
    float4* rows = reinterpret_cast<float4*>(w + L.rows); float* core2c = reinterpret_cast<float*>(w + L.core2c);
    int* parent = reinterpret_cast<int*>(w + L.parent); int* comp = reinterpret_cast<int*>(w + L.comp);
    unsigned long long* best = reinterpret_cast<unsigned long long*>(w + L.best); unsigned* compw = reinterpret_cast<unsigned*>(w + L.compw);
    unsigned long long* complh = reinterpret_cast<unsigned long long*>(w + L.complh);
    const int nb = (n + 255) / 256, nb1k = (n + 1023) / 1024;
    {
        ProfScope ps("hdbscan_core", s);
        HIMO_HIP(hipMemsetAsync(words, 0, kHdWords * 4, s));
        hipLaunchKernelGGL(hd_count_kernel, dim3(nb1k), dim3(1024), 0, s, n, d_xyz, pitch, d_skip, block_sum, d_core2);
        hipLaunchKernelGGL(hd_compact_kernel, dim3(nb1k), dim3(1024), 0, s, n, d_xyz, pitch, d_skip, block_sum, min_samples, rows, d_index, parent,
                           comp, best, compw, complh, words, d_counts);
        hipLaunchKernelGGL(hd_core_kernel, dim3(nb), dim3(256), 0, s, d_counts, rows, min_samples, core2c, d_core2);
        HIMO_LAUNCH_CHECK("hdbscan core kernels");
    }
    int rounds = 0;
    while ((1ll << rounds) < n) ++rounds;                       // ceil(log2 n) >= ceil(log2 |P|): every round at least halves the components
    // the search grid: 1024 query points per block in x; the candidates in chunks of whole tiles in y, enough blocks to fill the chip
    const int qblocks = (n + 256 * kHdQ - 1) / (256 * kHdQ), tiles = (n + kHdTile - 1) / kHdTile;
    int ysplit = 2048 / qblocks;
    ysplit = ysplit < 1 ? 1 : (ysplit > tiles ? tiles : ysplit);
    const int chunk = (tiles + ysplit - 1) / ysplit * kHdTile;
    ysplit = (n + chunk - 1) / chunk;
    {
        ProfScope ps("hdbscan_rounds", s);
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(hd_search_kernel, dim3(qblocks, ysplit), dim3(256), 0, s, words, r, d_counts, rows, core2c, comp, chunk, best);
            hipLaunchKernelGGL(hd_compw_kernel, dim3(nb), dim3(256), 0, s, words, r, d_counts, comp, best, compw);
            hipLaunchKernelGGL(hd_complh_kernel, dim3(nb), dim3(256), 0, s, words, r, d_counts, comp, best, compw, complh);
            hipLaunchKernelGGL(hd_hook_kernel, dim3(nb), dim3(256), 0, s, words, r, d_counts, comp, compw, complh, d_index, parent, n - 1, d_edges);
            hipLaunchKernelGGL(hd_flatten_kernel, dim3(nb), dim3(256), 0, s, words, r, d_counts, parent, comp, best, compw, complh);
        }
        HIMO_LAUNCH_CHECK("hdbscan round kernels");
    }
    return HIMO_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the host phase: steps 6-10.  Plain C++, no HIP call.  O(n log n): one sort by the total order, one union-find, one walk.
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
struct HdEdge { uint32_t w; int lo, hi; };                      // lo, hi: ranks among the participating points
}

extern "C" int himo_hdbscan_tree(int n, int n_part, const int32_t* h_index, int n_edges, const uint32_t* h_edges, int min_cluster_size,
                                 int min_samples, int32_t* h_labels, int32_t* h_n_clusters) {
    if (n < 0 || n_part < 0 || n_part > n || n_edges < 0 || min_cluster_size < 2 || min_samples < 1 || min_samples > kHdMaxK)
        return HIMO_ERR_INVALID_ARGUMENT;
    if ((n > 0 && !h_labels) || (n_part > 0 && !h_index) || (n_edges > 0 && !h_edges)) return HIMO_ERR_INVALID_ARGUMENT;
    std::vector<int> rank_of((size_t)n, -1);
    for (int p = 0; p < n_part; ++p) {                          // the original indices: ascending, inside [0, n)
        const int i = h_index[p];
        if (i < 0 || i >= n || (p > 0 && i <= h_index[p - 1])) return HIMO_ERR_INVALID_ARGUMENT;
        rank_of[i] = p;
    }
    const int P = n_part;
    if (P < (min_samples > 2 ? min_samples : 2)) {
        if (n_edges != 0) return HIMO_ERR_INVALID_ARGUMENT;
        for (int i = 0; i < n; ++i) h_labels[i] = 0;
        if (h_n_clusters) *h_n_clusters = 0;
        return HIMO_OK;
    }
    if (n_edges != P - 1) return HIMO_ERR_INVALID_ARGUMENT;
    std::vector<HdEdge> e((size_t)n_edges);
    for (int t = 0; t < n_edges; ++t) {
        const uint32_t w = h_edges[(size_t)t * 3], lo = h_edges[(size_t)t * 3 + 1], hi = h_edges[(size_t)t * 3 + 2];
        if (w > 0x7f800000u || lo >= hi || hi >= (uint32_t)n || rank_of[lo] < 0 || rank_of[hi] < 0) return HIMO_ERR_INVALID_ARGUMENT;
        e[t] = HdEdge{w, rank_of[lo], rank_of[hi]};
    }
    std::sort(e.begin(), e.end(), [](const HdEdge& a, const HdEdge& b) {
        return a.w != b.w ? a.w < b.w : (a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi);
    });
    // step 6: nodes 0 .. P-1 are the points, P .. 2P-2 the merges
    const int nodes = 2 * P - 1, root = nodes - 1;
    std::vector<int> left((size_t)nodes, -1), right((size_t)nodes, -1), size((size_t)nodes, 1), uf((size_t)P), node_of((size_t)P);
    std::vector<double> dist((size_t)nodes, 0.0);
    for (int p = 0; p < P; ++p) { uf[p] = p; node_of[p] = p; }
    auto find = [&](int x) {
        while (uf[x] != x) { uf[x] = uf[uf[x]]; x = uf[x]; }
        return x;
    };
    for (int t = 0; t < n_edges; ++t) {
        const int a = find(e[t].lo), b = find(e[t].hi);
        if (a == b) return HIMO_ERR_INVALID_ARGUMENT;           // a cycle: not a spanning tree
        const int v = P + t;
        left[v] = node_of[a]; right[v] = node_of[b];
        size[v] = size[left[v]] + size[right[v]];
        dist[v] = sqrt((double)__builtin_bit_cast(float, e[t].w));
        uf[b] = a; node_of[a] = v;
    }
    // steps 7 and 8: the condensed tree, cluster 0 the root
    const int m = min_cluster_size;
    std::vector<int> cl_parent(1, -1), cl_child(1, -1);         // a cluster's parent, and its LEFT child (the right one is + 1), -1: a leaf
    std::vector<double> birth(1, 0.0), S(1, 0.0);
    std::vector<int> fell((size_t)P, 0);                        // the cluster every point fell out of
    std::vector<int> stack, cl_of((size_t)nodes, 0), sub;
    auto fall = [&](int v, int c, double lambda) {              // every point below node v falls out of cluster c at lambda
        sub.assign(1, v);
        while (!sub.empty()) {
            const int u = sub.back(); sub.pop_back();
            if (u < P) { fell[u] = c; S[c] += (lambda - birth[c]) * 1.0; }
            else { sub.push_back(right[u]); sub.push_back(left[u]); }
        }
    };
    stack.push_back(root);
    while (!stack.empty()) {
        const int v = stack.back(); stack.pop_back();
        const int c = cl_of[v], l = left[v], r = right[v];
        const double d = dist[v] > 1e-9 ? dist[v] : 1e-9, lambda = 1.0 / d;
        if (size[l] >= m && size[r] >= m) {
            const int kid = (int)cl_parent.size();
            cl_child[c] = kid;
            for (int side = 0; side < 2; ++side) {
                const int u = side ? r : l;
                cl_parent.push_back(c); cl_child.push_back(-1); birth.push_back(lambda); S.push_back(0.0);
                S[c] += (lambda - birth[c]) * (double)size[u];
                cl_of[u] = kid + side;
            }
            stack.push_back(r); stack.push_back(l);
        } else if (size[l] < m && size[r] < m) {
            fall(l, c, lambda); fall(r, c, lambda);
        } else {
            const int big = size[l] >= m ? l : r, small = size[l] >= m ? r : l;
            fall(small, c, lambda);
            cl_of[big] = c;
            stack.push_back(big);
        }
    }
    // step 9
    const int C = (int)cl_parent.size();
    std::vector<char> selected((size_t)C, 1);
    selected[0] = 0;
    for (int c = C - 1; c >= 1; --c) {
        if (cl_child[c] < 0) continue;
        const double kids = S[cl_child[c]] + S[cl_child[c] + 1];
        if (kids > S[c]) { S[c] = kids; selected[c] = 0; }
        else {
            sub.assign(1, cl_child[c]); sub.push_back(cl_child[c] + 1);
            while (!sub.empty()) {
                const int u = sub.back(); sub.pop_back();
                selected[u] = 0;
                if (cl_child[u] >= 0) { sub.push_back(cl_child[u]); sub.push_back(cl_child[u] + 1); }
            }
        }
    }
    // step 10: a parent's id is below its children's, so one ascending pass resolves the nearest selected ancestor
    std::vector<int> home((size_t)C, -1), number((size_t)C, 0);
    for (int c = 1; c < C; ++c) home[c] = selected[c] ? c : home[cl_parent[c]];
    for (int i = 0; i < n; ++i) h_labels[i] = 0;
    int K = 0;
    for (int p = 0; p < P; ++p) {
        const int c = home[fell[p]];
        if (c < 0) continue;
        if (!number[c]) number[c] = ++K;
        h_labels[h_index[p]] = number[c];
    }
    if (h_n_clusters) *h_n_clusters = K;
    return HIMO_OK;
}
