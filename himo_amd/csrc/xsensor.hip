// xsensor.hip -- cross-sensor consistency per cluster ("cross-sensor consistency, v1"; the rule is the module docstring of
// himo_amd/eval_xsensor.py) for gfx950.  PARITY UNPINNED: the reference has no such stage; this one is checked against the numpy
// restatement of the written rule (tests/xsensor_ref.py).  Timing on synthetic sweeps: profiles/xsensor.txt.
//
// Inside every cluster, the distance from each point to the nearest point another sensor recorded: large where the sensors' copies of
// a moving object are displaced, the sampling spacing where they lie on top of one another.  No labels from a person are read.
//
// The labelled rows arrive SORTED BY LABEL, as in boxfit.hip and rigidrefine.hip: cluster k owns the sorted rows offsets[k] ..
// offsets[k + 1], and d_rows[i] is the row of the point buffer behind sorted row i.  One clear of the count table and THREE launches a
// call, whatever the clusters:
//   count   (rules A, B) one lane per sorted row: reads the row, decides USABLE, and stages it as float4 (x, y, z, 1 << group as the
//           bits of w; a row that is not usable: zeros, whose bit test never passes) in the workspace; n_g meets in int32 atomics on
//           the count table [C][8].
//   search  (rule C, the hot path) the shape of nn.hip: a block owns 256 CONSECUTIVE sorted rows, one per lane, and streams the row
//           range of their clusters through LDS in chunks of HIMO_XSENSOR_CHUNK float4.  Every lane of a wave inside one cluster
//           reads the SAME LDS address at a time, a broadcast: one 16-byte read feeds 64 distance evaluations.  A cluster of 8192
//           rows is spread over 32 (33 when it straddles a tile edge) blocks; small clusters are PACKED, about 256 / n of them to
//           a block, each lane walking its own cluster's rows, so 2000 clusters of 12 rows are 94 blocks and not 2000 nearly idle
//           ones.  A query carries mask = (live groups) & ~(its own group); candidate j counts iff mask & w_j: one AND, one compare
//           and one select beside the eight float operations of d2, and nothing else decides -- a row that is not usable (w = 0) or
//           of a group that is not live (its bit is not in any mask) can never win.  The minimum is order-free: the same bits however
//           the rows are tiled.
//   reduce  (rules D, E) one block per cluster: sqrt, clip and q() per query row in float64, q(dt) and the motion per usable row,
//           summed as int64 in LDS integer atomics (any order, the same bits), then written with ordinary stores: info, rec and mot
//           are written whole by this phase, so the caller's buffers need no clearing.
// No floating-point atomics anywhere.  LDS: 16 KB a search block.  Occupancy is not the limit: the loop is VALU-bound (twelve
// operations to one LDS read a candidate).
//
// Built with -ffp-contract=off: every float operation rounds on its own, as numpy does; sqrt is correctly rounded.
#include "himo_common.h"
#include "blockops.h"
#include "xsensor_rows.h"
#include <limits.h>
#include <math.h>

namespace himo {

constexpr int kXsChunk = HIMO_XSENSOR_CHUNK;         // (kXsThreads, kXsGroups and rules A and B: xsensor_rows.h)
constexpr double kXsUnit = 16777216.0;         // 2^24: the unit of eval_flow's q()
constexpr double kXsClip = 1024.0;             // |dt| [s] and the motion length [m] are clipped here before q()
static_assert(kXsChunk % kXsThreads == 0, "xsensor tiling");

struct XsArgs {
    int64_t n;                       // rows of the point buffer
    const float* pts;                // [n][pitch]
    int pitch;
    const int32_t* labels;           // [n]
    const uint8_t* group;            // [n]
    const float* dt;                 // [n] or nullptr
    const float* motion;             // [n][3] or nullptr
    const int64_t* rows;             // [nc]
    const int64_t* offsets;          // [C + 1]
    int nc, C;
    float trunc, near;
    int min_group, min_points, max_points;
    float4* staged;                  // [nc] workspace
    float* m;                        // [nc] min d2 per sorted row (the caller's buffer, or workspace)
    int32_t* cnt;                    // [C][8] workspace
    int32_t* info;                   // [C][4]
    long long* rec;                  // [C][8][4]
    long long* mot;                  // [C][2]
};

__device__ inline void xs_range(const XsArgs& p, int k, int& lo, int& hi) { xs_range(p.offsets, p.nc, k, lo, hi); }

// ---- count: rules A and B's counts ----
__global__ __launch_bounds__(kXsThreads) void xs_count_kernel(XsArgs p) {
    const int64_t i64 = (int64_t)blockIdx.x * kXsThreads + threadIdx.x;
    if (i64 >= p.nc) return;
    const int i = (int)i64;
    p.staged[i] = xs_stage_row(p.n, p.pts, p.pitch, p.labels, p.group, p.dt, p.rows, p.offsets, p.C, i, p.cnt);
}

// ---- search: rule C ----
__global__ __launch_bounds__(kXsThreads) void xs_search_kernel(XsArgs p) {
    __shared__ float4 tile[kXsChunk];
    __shared__ int s_lo, s_hi;
    const int t = (int)threadIdx.x;
    const int64_t i64 = (int64_t)blockIdx.x * kXsThreads + t;
    const bool have = i64 < p.nc;
    const int i = have ? (int)i64 : 0;

    float qx = 0.f, qy = 0.f, qz = 0.f, best = INFINITY;
    int mask = 0, rs = 0, re = 0;
    if (have) {
        const float4 me = p.staged[i];
        const int bit = __float_as_int(me.w);
        if (bit) {
            const int k = segment_of(p.offsets, p.C, i);
            int n, live;
            if (xs_state(p.cnt + kXsGroups * (size_t)k, p.min_group, p.min_points, p.max_points, n, live) == HIMO_XSENSOR_SCORED && (live & bit)) {
                mask = live & ~bit;                                  // (not 0: a SCORED cluster has two live groups)
                qx = me.x; qy = me.y; qz = me.z;
                xs_range(p, k, rs, re);
            }
        }
    }
    if (t == 0) { s_lo = INT_MAX; s_hi = 0; }
    __syncthreads();
    if (mask && re > rs) { atomicMin(&s_lo, rs); atomicMax(&s_hi, re); }
    __syncthreads();
    const int blo = s_lo, bhi = s_hi;

    for (int t0 = blo; t0 < bhi; t0 += kXsChunk) {                  // (blo = INT_MAX without a query: no pass)
        __syncthreads();
        const int tcount = min(kXsChunk, bhi - t0);
        for (int j = t; j < kXsChunk; j += kXsThreads)
            tile[j] = j < tcount ? p.staged[t0 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        if (mask) {
            const int jlo = max(rs - t0, 0), jhi = min(re - t0, tcount);
#pragma unroll 4
            for (int j = jlo; j < jhi; ++j) {
                const float4 v = tile[j];
                const float dx = qx - v.x, dy = qy - v.y, dz = qz - v.z;
                const float d = (dx * dx + dy * dy) + dz * dz;
                const bool other = (mask & __float_as_int(v.w)) != 0;
                best = (other && d < best) ? d : best;
            }
        }
    }
    if (have) p.m[i] = best;                                        // +inf for a row that is not a query
}

// ---- reduce: rules D and E ----
__global__ __launch_bounds__(kXsThreads) void xs_reduce_kernel(XsArgs p) {
    __shared__ unsigned long long s_acc[kXsGroups][3];              // q(dt), q(c), NEAR per group
    __shared__ unsigned long long s_mot[2];
    __shared__ int s_queries;
    const int t = (int)threadIdx.x, k = (int)blockIdx.x;
    const int32_t* cnt = p.cnt + kXsGroups * (size_t)k;
    int n, live;
    const int state = xs_state(cnt, p.min_group, p.min_points, p.max_points, n, live);
    if (t < kXsGroups * 3) (&s_acc[0][0])[t] = 0ull;
    if (t < 2) s_mot[t] = 0ull;
    if (t == 0) s_queries = 0;
    __syncthreads();
    if (state == HIMO_XSENSOR_SCORED) {                             // (block-uniform)
        int lo, hi;
        xs_range(p, k, lo, hi);
        const double trunc = (double)p.trunc, near = (double)p.near;
        for (int i = lo + t; i < hi; i += kXsThreads) {
            const int bit = __float_as_int(p.staged[i].w);
            if (!bit) continue;
            const int g = __ffs(bit) - 1;
            const int64_t r = p.rows[i];                            // (in range: the count phase staged the row)
            if (p.dt) {
                double v = (double)p.dt[r];
                v = v < -kXsClip ? -kXsClip : (v > kXsClip ? kXsClip : v);
                atomicAdd(&s_acc[g][0], (unsigned long long)llrint(v * kXsUnit));
            }
            if (live & bit) {
                const double d = sqrt((double)p.m[i]);
                const double c = d < trunc ? d : trunc;
                atomicAdd(&s_acc[g][1], (unsigned long long)llrint(c * kXsUnit));
                if (d <= near) atomicAdd(&s_acc[g][2], 1ull);
                atomicAdd(&s_queries, 1);
            }
            if (p.motion) {
                const float* mv = p.motion + 3 * r;
                const float m0 = mv[0], m1 = mv[1], m2 = mv[2];
                if (xs_finite(m0) && xs_finite(m1) && xs_finite(m2)) {
                    const double s = sqrt(((double)m0 * (double)m0 + (double)m1 * (double)m1) + (double)m2 * (double)m2);
                    atomicAdd(&s_mot[0], 1ull);
                    atomicAdd(&s_mot[1], (unsigned long long)llrint((s < kXsClip ? s : kXsClip) * kXsUnit));
                }
            }
        }
    }
    __syncthreads();
    const bool scored = state == HIMO_XSENSOR_SCORED;
    if (t < 4) p.info[4 * (size_t)k + t] = t == 0 ? state : (t == 1 ? n : (scored ? (t == 2 ? live : s_queries) : 0));
    if (t < kXsGroups * 4) {
        const int g = t >> 2, f = t & 3;
        p.rec[32 * (size_t)k + t] = f == 0 ? (long long)cnt[g] : (long long)s_acc[g][f - 1];
    }
    if (t < 2) p.mot[2 * (size_t)k + t] = (long long)s_mot[t];
}

static bool xs_params_ok(const himo_xsensor_params* p) {
    if (!p) return false;
    if (!isfinite(p->trunc) || !(p->trunc > 0.f) || p->trunc > 1024.f) return false;
    if (!isfinite(p->near) || !(p->near >= 0.f)) return false;
    return p->min_group >= 1 && p->min_points >= 2 && p->max_points >= p->min_points && p->max_points <= (1 << 20);
}

// the workspace: staged float4 [nc] | m float [nc] | cnt int32 [C][8], each part rounded up to 256 bytes
static size_t xs_part_staged(int64_t nc) { return round_up((size_t)(nc > 0 ? nc : 1) * sizeof(float4), 256); }
static size_t xs_part_m(int64_t nc) { return round_up((size_t)(nc > 0 ? nc : 1) * sizeof(float), 256); }
static size_t xs_part_cnt(int C) { return round_up((size_t)(C > 0 ? C : 1) * kXsGroups * sizeof(int32_t), 256); }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_xsensor_workspace_bytes(int64_t n_clustered, int n_clusters) {
    if (n_clustered < 0 || n_clustered > 0x7fffffffLL || n_clusters < 0) return 0;
    return xs_part_staged(n_clustered) + xs_part_m(n_clustered) + xs_part_cnt(n_clusters);
}

extern "C" int himo_xsensor(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, const uint8_t* d_group, const float* d_dt,
                            const float* d_motion, int64_t n_clustered, const int64_t* d_rows, int n_clusters, const int64_t* h_offsets,
                            const int64_t* d_offsets, const himo_xsensor_params* params, int32_t* d_info, int64_t* d_rec, int64_t* d_mot,
                            float* d_min_d2, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || n_clustered < 0 || n_clustered > n || n_clusters < 0 || pitch < 3) return HIMO_ERR_INVALID_ARGUMENT;
    if (!xs_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n_clusters == 0) return n_clustered == 0 ? HIMO_OK : HIMO_ERR_INVALID_ARGUMENT;
    if (!h_offsets || !d_offsets || !xs_offsets_ok(n_clustered, n_clusters, h_offsets)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_info || !d_rec || !d_mot || xs_misaligned(d_info, 4) || xs_misaligned(d_rec, 8) || xs_misaligned(d_mot, 8) || xs_misaligned(d_offsets, 8))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (n_clustered > 0 && (!d_pts || !d_labels || !d_group || !d_rows)) return HIMO_ERR_INVALID_ARGUMENT;
    if (xs_misaligned(d_pts, 4) || xs_misaligned(d_labels, 4) || xs_misaligned(d_rows, 8) || xs_misaligned(d_dt, 4) || xs_misaligned(d_motion, 4) ||
        xs_misaligned(d_min_d2, 4))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < himo_xsensor_workspace_bytes(n_clustered, n_clusters)) return HIMO_ERR_WORKSPACE;

    char* ws = reinterpret_cast<char*>(d_workspace);
    XsArgs p;
    p.n = n; p.pts = d_pts; p.pitch = pitch; p.labels = d_labels; p.group = d_group; p.dt = d_dt; p.motion = d_motion; p.rows = d_rows;
    p.offsets = d_offsets; p.nc = (int)n_clustered; p.C = n_clusters;
    p.trunc = params->trunc; p.near = params->near; p.min_group = params->min_group; p.min_points = params->min_points; p.max_points = params->max_points;
    p.staged = reinterpret_cast<float4*>(ws);
    float* ws_m = reinterpret_cast<float*>(ws + xs_part_staged(n_clustered));
    p.m = d_min_d2 ? d_min_d2 : ws_m;
    p.cnt = reinterpret_cast<int32_t*>(ws + xs_part_staged(n_clustered) + xs_part_m(n_clustered));
    p.info = d_info; p.rec = reinterpret_cast<long long*>(d_rec); p.mot = reinterpret_cast<long long*>(d_mot);

    hipStream_t s = (hipStream_t)stream;
    HIMO_HIP(hipMemsetAsync(p.cnt, 0, (size_t)n_clusters * kXsGroups * sizeof(int32_t), s));
    const unsigned row_blocks = (unsigned)((n_clustered + kXsThreads - 1) / kXsThreads);
    if (row_blocks) {
        {
            ProfScope ps("xs_count_kernel", s);
            hipLaunchKernelGGL(xs_count_kernel, dim3(row_blocks), dim3(kXsThreads), 0, s, p);
        }
        HIMO_LAUNCH_CHECK("xs_count_kernel");
        {
            ProfScope ps("xs_search_kernel", s);
            hipLaunchKernelGGL(xs_search_kernel, dim3(row_blocks), dim3(kXsThreads), 0, s, p);
        }
        HIMO_LAUNCH_CHECK("xs_search_kernel");
    }
    {
        ProfScope ps("xs_reduce_kernel", s);
        hipLaunchKernelGGL(xs_reduce_kernel, dim3((unsigned)n_clusters), dim3(kXsThreads), 0, s, p);
    }
    HIMO_LAUNCH_CHECK("xs_reduce_kernel");
    return HIMO_OK;
}
