// icpflow.hip -- the ICP-Flow baseline ("cluster-rigid ICP, v1"; the rule is the module docstring of himo_amd/icpflow.py) for gfx950.
// PARITY UNPINNED: the reference's ICP-Flow code lives in its absent submodule (only the result key `icpflow` is in its tree);
// this stage is checked against the numpy restatement of the written rule (tests/icpflow_ref.py).
//
// The clustered points arrive SORTED BY LABEL: cluster k (label k + 1) owns the rows offsets[k] .. offsets[k + 1] of the sorted
// order.  Four kernels, sequenced by the host around the existing exact nearest-neighbour search (himo_nn_grid):
//   icp_vote_kernel     rule 2.  The target sweep is binned on the BEV cell grid of nngrid.hip (its own build step).  A block owns 64
//                       consecutive sorted points, a wave one point at a time: the cells the vote window can reach are, row by row of
//                       the grid, ONE contiguous run of candidates, which the lanes walk with coalesced 16-byte loads.  Votes for the
//                       block's first cluster go to an LDS histogram (integer LDS atomics) that is flushed once with integer global
//                       atomics; the votes of a block that straddles clusters, and every vote when the histogram does not fit the LDS
//                       array (half > 44), go to the global counters directly.  Integer sums: independent of order.
//   icp_peak_kernel     one wave per cluster: the peak as the maximum of ONE 64-bit key (count, then smallest kx^2 + ky^2, then
//                       lowest (ky, kx)); writes the start transform and the status word.
//   icp_moments_kernel  rule 3's sums, one 256-thread block per cluster in a FIXED shape: thread t adds rows t, t + 256, ... of the
//                       cluster in ascending order, then a fixed LDS tree (128, 64, ... 1).  No floating-point atomics: the same
//                       inputs give the same bytes on every run.  Two passes (centroids, then A and B about them).
//   icp_solve_kernel    one thread per cluster: the closed form, the composition, failed / accepted / rejected.
//   icp_apply_kernel    m_i = float32(R a_i + t) in float64 for the next search, or the flow m_i - pc0_i.
//
// Built with -ffp-contract=off: every float operation rounds on its own, as numpy does.  Only sqrt and division appear (float32
// division in the vote, float64 elsewhere), both correctly rounded.
#include "nngrid.h"
#include "blockops.h"
#include <math.h>

namespace himo {

constexpr int kIcpThreads = 256;
constexpr int kVotePts = 64;                 // sorted points per block
constexpr int kVoteWaves = kIcpThreads / 64;
constexpr int kVoteLdsBins = 8192;           // 32 KB: (2 half + 1)^2 fits up to half = 44
constexpr int kMomDoubles = 10;              // n, m_bar xyz, q_bar xyz, A, B, (pad)
// the BEV cell grid the target sweep is binned on: the one the package's searches use (himo_amd/ssl_loss.py)
constexpr float kIcpGridX0 = -52.f, kIcpGridY0 = -52.f, kIcpGridCell = 1.f;
constexpr int kIcpGridW = 104, kIcpGridH = 104;

struct VoteArgs {
    int64_t n;
    const float* pts;
    int pitch;
    int C;
    const int64_t* offsets;
    const int* cell_offset;          // [cells + 1] of the binned target sweep (row-major cell order)
    const float4* sorted;            // its rows in that order
    NnGrid g;
    float bin, z_gate;
    int half;
    int* counts;                     // [C][(2 half + 1)^2]
};

__global__ __launch_bounds__(kIcpThreads) void icp_vote_kernel(VoteArgs a) {
    __shared__ int hist[kVoteLdsBins];
    const int W = 2 * a.half + 1, WW = W * W;
    const bool use_lds = WW <= kVoteLdsBins;
    const int64_t base = (int64_t)blockIdx.x * kVotePts;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k0 = segment_of(a.offsets, a.C, base);
    if (use_lds) {
        for (int b = threadIdx.x; b < WW; b += kIcpThreads) hist[b] = 0;
        __syncthreads();
    }
    const float fhalf = (float)a.half;
    for (int p = wave; p < kVotePts; p += kVoteWaves) {
        const int64_t i = base + p;
        if (i >= a.n) break;
        const int k = segment_of(a.offsets, a.C, i);
        const float* q = a.pts + i * a.pitch;
        const float ax = q[0], ay = q[1], az = q[2];
        // every target point that can vote lies within (half + 1/2) bins in x and in y, up to float32 rounding: half a bin and a
        // relative 1e-4 of the coordinates more cover that
        const float reach = (fhalf + 1.f) * a.bin + 1e-4f * (fabsf(ax) + fabsf(ay) + 1.f);
        const int cx0 = nng_cell_x(a.g, ax - reach), cx1 = nng_cell_x(a.g, ax + reach);
        const int cy0 = nng_cell_y(a.g, ay - reach), cy1 = nng_cell_y(a.g, ay + reach);
        int* const mine = a.counts + (size_t)k * WW;
        const bool to_lds = use_lds && k == k0;
        for (int cy = cy0; cy <= cy1; ++cy) {
            const int r0 = a.cell_offset[cy * a.g.gw + cx0], r1 = a.cell_offset[cy * a.g.gw + cx1 + 1];
            for (int j = r0 + lane; j < r1; j += 64) {
                const float4 c = a.sorted[j];
                const float dz = c.z - az;
                if (!(fabsf(dz) <= a.z_gate)) continue;
                const float kx = rintf((c.x - ax) / a.bin), ky = rintf((c.y - ay) / a.bin);
                if (!(fabsf(kx) <= fhalf && fabsf(ky) <= fhalf)) continue;
                const int b = ((int)ky + a.half) * W + ((int)kx + a.half);
                if (to_lds) atomicAdd(&hist[b], 1);
                else atomicAdd(&mine[b], 1);
            }
        }
    }
    if (use_lds) {
        __syncthreads();
        int* const dst = a.counts + (size_t)k0 * WW;
        for (int b = threadIdx.x; b < WW; b += kIcpThreads) {
            const int v = hist[b];
            if (v) atomicAdd(&dst[b], v);
        }
    }
}

// rule 2's peak and rule 3's start.  One wave per cluster.
__global__ __launch_bounds__(64) void icp_peak_kernel(int C, int half, float bin, const int* __restrict__ counts, int* __restrict__ peak,
                                                      double* __restrict__ T, int* __restrict__ status) {
    const int k = blockIdx.x, W = 2 * half + 1, WW = W * W;
    const int* c = counts + (size_t)k * WW;
    unsigned long long best = 0ull;
    for (int b = threadIdx.x; b < WW; b += 64) {
        const int ky = b / W - half, kx = b % W - half;
        // higher count first; then the smaller kx^2 + ky^2, then the lower (ky, kx) = the lower bin index: both inverted
        const unsigned rank = ((unsigned)(kx * kx + ky * ky) << 15) | (unsigned)b;
        const unsigned long long key = ((unsigned long long)(unsigned)c[b] << 32) | (0xffffffffu - rank);
        best = key > best ? key : best;
    }
    best = wave_max_u64(best);
    if (threadIdx.x == 0) {
        const int b = (int)((0xffffffffu - (unsigned)best) & 0x7fffu);
        const int ky = b / W - half, kx = b % W - half;
        peak[2 * k] = kx; peak[2 * k + 1] = ky;
        double* t = T + 5 * (size_t)k;
        t[0] = 1.0; t[1] = 0.0; t[2] = (double)kx * (double)bin; t[3] = (double)ky * (double)bin; t[4] = 0.0;
        int* s = status + 4 * (size_t)k;
        s[0] = HIMO_ICP_ACCEPTED; s[1] = 0; s[2] = kx; s[3] = ky;
    }
}

struct StepArgs {
    int64_t n;
    const float* m;                  // [n][3] the moved points of this pass
    const float* tgt;                // [n_tgt][3]
    int64_t n_tgt;
    const int* idx;
    const float* d2;
    int C;
    const int64_t* offsets;
    float max_d2;
    int min_inliers;
    double min_ratio;
    int final_pass;
    double* T;
    int* status;
    uint8_t* inlier;                 // [n] or nullptr
    double* mom;                     // [C][kMomDoubles]
};

__global__ __launch_bounds__(kIcpThreads) void icp_moments_kernel(StepArgs a) {
    __shared__ double sh[kIcpThreads];
    const int k = blockIdx.x;
    const int64_t lo = a.offsets[k], hi = a.offsets[k + 1];
    auto is_in = [&](int64_t i) { const int j = a.idx[i]; return a.d2[i] <= a.max_d2 && j >= 0 && (int64_t)j < a.n_tgt; };
    double cnt = 0.0, sm[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0};
    for (int64_t i = lo + threadIdx.x; i < hi; i += kIcpThreads) {
        const bool in = is_in(i);
        if (a.inlier) a.inlier[i] = (uint8_t)in;
        if (!in) continue;
        const float* m = a.m + 3 * i;
        const float* q = a.tgt + 3 * (int64_t)a.idx[i];
        cnt += 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { sm[c] = sm[c] + (double)m[c]; sq[c] = sq[c] + (double)q[c]; }
    }
    const double n = group_sum<kIcpThreads>(cnt, sh);
    double mb[3], qb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double s0 = group_sum<kIcpThreads>(sm[c], sh), s1 = group_sum<kIcpThreads>(sq[c], sh);
        mb[c] = n > 0.0 ? s0 / n : 0.0;
        qb[c] = n > 0.0 ? s1 / n : 0.0;
    }
    double A = 0.0, B = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kIcpThreads) {
        if (!is_in(i)) continue;
        const float* m = a.m + 3 * i;
        const float* q = a.tgt + 3 * (int64_t)a.idx[i];
        const double mx = (double)m[0] - mb[0], my = (double)m[1] - mb[1], qx = (double)q[0] - qb[0], qy = (double)q[1] - qb[1];
        A = A + (mx * qx + my * qy);
        B = B + (mx * qy - my * qx);
    }
    A = group_sum<kIcpThreads>(A, sh);
    B = group_sum<kIcpThreads>(B, sh);
    if (threadIdx.x == 0) {
        double* o = a.mom + (size_t)k * kMomDoubles;
        o[0] = n; o[1] = mb[0]; o[2] = mb[1]; o[3] = mb[2]; o[4] = qb[0]; o[5] = qb[1]; o[6] = qb[2]; o[7] = A; o[8] = B; o[9] = 0.0;
    }
}

__global__ __launch_bounds__(kIcpThreads) void icp_solve_kernel(StepArgs a) {
    const int k = blockIdx.x * kIcpThreads + threadIdx.x;
    if (k >= a.C) return;
    int* st = a.status + 4 * (size_t)k;
    if (st[0] == HIMO_ICP_FAILED) return;                     // a failed cluster has stopped
    const double* o = a.mom + (size_t)k * kMomDoubles;
    const int n = (int)o[0];
    st[1] = n;
    if (a.final_pass) {                                       // rule 4
        const int64_t size = a.offsets[k + 1] - a.offsets[k];
        st[0] = (size > 0 && (double)n / (double)size >= a.min_ratio) ? HIMO_ICP_ACCEPTED : HIMO_ICP_REJECTED;
        return;
    }
    if (n < a.min_inliers) { st[0] = HIMO_ICP_FAILED; return; }
    const double A = o[7], B = o[8];
    const double h = sqrt(A * A + B * B);
    const double dc = h == 0.0 ? 1.0 : A / h, ds = h == 0.0 ? 0.0 : B / h;
    const double dtx = o[4] - (dc * o[1] - ds * o[2]), dty = o[5] - (ds * o[1] + dc * o[2]), dtz = o[6] - o[3];
    double* t = a.T + 5 * (size_t)k;
    const double c = t[0], s = t[1], tx = t[2], ty = t[3], tz = t[4];
    t[0] = dc * c - ds * s;
    t[1] = ds * c + dc * s;
    t[2] = (dc * tx - ds * ty) + dtx;
    t[3] = (ds * tx + dc * ty) + dty;
    t[4] = tz + dtz;
}

__global__ __launch_bounds__(kIcpThreads) void icp_apply_kernel(int64_t n, const float* __restrict__ pts, int pitch, const int* __restrict__ labels,
                                                                int C, const double* __restrict__ T, const int* __restrict__ status, int mode,
                                                                const float* __restrict__ base, int base_pitch, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kIcpThreads + threadIdx.x;
    if (i >= n) return;
    const float* p = pts + i * pitch;
    float mx = p[0], my = p[1], mz = p[2];
    const int l = labels ? labels[i] : 0;
    // a label outside 1 .. C, and in flow mode a cluster that was not accepted, is the identity: the point itself, bit for bit
    if (l >= 1 && l <= C && (mode == HIMO_ICP_MOVED || status[4 * (size_t)(l - 1)] == HIMO_ICP_ACCEPTED)) {
        const double* t = T + 5 * (size_t)(l - 1);
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        mx = (float)((t[0] * x - t[1] * y) + t[2]);
        my = (float)((t[1] * x + t[0] * y) + t[3]);
        mz = (float)(z + t[4]);
    }
    float* o = out + 3 * i;
    if (mode == HIMO_ICP_FLOW) {
        const float* b = base + i * base_pitch;
        o[0] = mx - b[0]; o[1] = my - b[1]; o[2] = mz - b[2];
    } else {
        o[0] = mx; o[1] = my; o[2] = mz;
    }
}

static bool icp_params_ok(const himo_icp_params* p) {
    if (!p) return false;
    const float fl[4] = {p->bin, p->z_gate, p->max_dist, p->min_ratio};
    for (float v : fl)
        if (!isfinite(v) || !(v > 0.f)) return false;
    return p->half >= 1 && p->half <= 64 && p->min_inliers >= 1 && p->iters >= 1;
}

static bool icp_offsets_ok(int64_t n, int C, const int64_t* h) {
    if (h[0] != 0 || h[C] != n) return false;
    for (int k = 0; k < C; ++k)
        if (h[k] < 0 || h[k + 1] < h[k]) return false;
    return true;
}

static bool icp_misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

static size_t icp_grid_bytes(int64_t n_target) { return round_up(nng_workspace_bytes(1, n_target, kIcpGridW * kIcpGridH), 256); }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_icp_workspace_bytes(int64_t n_target, int n_clusters) {
    if (n_target < 0 || n_target > 0x7fffffffLL || n_clusters < 0) return 0;
    return icp_grid_bytes(n_target) + round_up((size_t)(n_clusters > 0 ? n_clusters : 1) * kMomDoubles * sizeof(double), 256);
}

extern "C" int himo_icp_vote(int64_t n, const float* d_pts, int pitch, int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets,
                             int64_t n_target, const float* d_target, const himo_icp_params* params, int32_t* d_counts,
                             int32_t* d_peak, double* d_transform, int32_t* d_status, void* d_workspace, size_t workspace_bytes,
                             void* stream) {
    if (n < 0 || n_target < 0 || n_clusters < 0 || !icp_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (pitch != 3 && pitch != 4) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL || n_target > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n == 0 || n_clusters == 0) return HIMO_OK;
    if (!h_offsets || !d_offsets || !icp_offsets_ok(n, n_clusters, h_offsets)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_counts || !d_peak || !d_transform || !d_status || (n > 0 && !d_pts) || (n_target > 0 && !d_target)) return HIMO_ERR_INVALID_ARGUMENT;
    if (icp_misaligned(d_pts, 4) || icp_misaligned(d_target, 4) || icp_misaligned(d_counts, 4) || icp_misaligned(d_peak, 4) ||
        icp_misaligned(d_transform, 8) || icp_misaligned(d_status, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < himo_icp_workspace_bytes(n_target, n_clusters)) return HIMO_ERR_WORKSPACE;

    hipStream_t s = (hipStream_t)stream;
    const int W = 2 * params->half + 1;
    HIMO_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_clusters * W * W * sizeof(int32_t), s));
    if (n > 0 && n_target > 0) {
        const NnGrid g{kIcpGridX0, kIcpGridY0, 1.0f / kIcpGridCell, kIcpGridCell, kIcpGridW, kIcpGridH};
        NngSet set;
        const float* pts[1] = {d_target};
        const int cnt[1] = {(int)n_target}, searched[1] = {0};
        nng_carve(d_workspace, &set, 1, pts, cnt, searched, kIcpGridW * kIcpGridH);
        const int st = nng_build(&set, 1, g, s);
        if (st != HIMO_OK) return st;
        VoteArgs a;
        a.n = n; a.pts = d_pts; a.pitch = pitch; a.C = n_clusters; a.offsets = d_offsets; a.cell_offset = set.offset; a.sorted = set.sorted;
        a.g = g; a.bin = params->bin; a.z_gate = params->z_gate; a.half = params->half; a.counts = d_counts;
        {
            ProfScope ps("icp_vote_kernel", s);
            hipLaunchKernelGGL(icp_vote_kernel, dim3((unsigned)((n + kVotePts - 1) / kVotePts)), dim3(kIcpThreads), 0, s, a);
        }
        HIMO_LAUNCH_CHECK("icp_vote_kernel");
    }
    {
        ProfScope ps("icp_peak_kernel", s);
        hipLaunchKernelGGL(icp_peak_kernel, dim3((unsigned)n_clusters), dim3(64), 0, s, n_clusters, params->half, params->bin, d_counts, d_peak,
                           d_transform, d_status);
    }
    HIMO_LAUNCH_CHECK("icp_peak_kernel");
    return HIMO_OK;
}

extern "C" int himo_icp_step(int64_t n, const float* d_moved, int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets,
                             int64_t n_target, const float* d_target, const int32_t* d_nn_idx, const float* d_nn_dist2,
                             const himo_icp_params* params, int final_pass, double* d_transform, int32_t* d_status, uint8_t* d_inlier,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || n_target < 0 || n_clusters < 0 || !icp_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL || n_target > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n == 0 || n_clusters == 0) return HIMO_OK;
    if (!h_offsets || !d_offsets || !icp_offsets_ok(n, n_clusters, h_offsets)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_transform || !d_status || (n > 0 && (!d_moved || !d_nn_idx || !d_nn_dist2)) || (n_target > 0 && !d_target)) return HIMO_ERR_INVALID_ARGUMENT;
    if (icp_misaligned(d_moved, 4) || icp_misaligned(d_target, 4) || icp_misaligned(d_nn_idx, 4) || icp_misaligned(d_nn_dist2, 4) ||
        icp_misaligned(d_transform, 8) || icp_misaligned(d_status, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < himo_icp_workspace_bytes(n_target, n_clusters)) return HIMO_ERR_WORKSPACE;

    hipStream_t s = (hipStream_t)stream;
    StepArgs a;
    a.n = n; a.m = d_moved; a.tgt = d_target; a.n_tgt = n_target; a.idx = d_nn_idx; a.d2 = d_nn_dist2; a.C = n_clusters; a.offsets = d_offsets;
    a.max_d2 = params->max_dist * params->max_dist; a.min_inliers = params->min_inliers; a.min_ratio = (double)params->min_ratio;
    a.final_pass = final_pass != 0; a.T = d_transform; a.status = d_status; a.inlier = d_inlier;
    a.mom = reinterpret_cast<double*>(reinterpret_cast<char*>(d_workspace) + icp_grid_bytes(n_target));
    {
        ProfScope ps("icp_moments_kernel", s);
        hipLaunchKernelGGL(icp_moments_kernel, dim3((unsigned)n_clusters), dim3(kIcpThreads), 0, s, a);
    }
    HIMO_LAUNCH_CHECK("icp_moments_kernel");
    {
        ProfScope ps("icp_solve_kernel", s);
        hipLaunchKernelGGL(icp_solve_kernel, dim3((unsigned)((n_clusters + kIcpThreads - 1) / kIcpThreads)), dim3(kIcpThreads), 0, s, a);
    }
    HIMO_LAUNCH_CHECK("icp_solve_kernel");
    return HIMO_OK;
}

extern "C" int himo_icp_apply(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, int n_clusters, const double* d_transform,
                              const int32_t* d_status, int mode, const float* d_base, int base_pitch, float* d_out, void* stream) {
    if (n < 0 || n_clusters < 0 || (pitch != 3 && pitch != 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (mode != HIMO_ICP_MOVED && mode != HIMO_ICP_FLOW) return HIMO_ERR_INVALID_ARGUMENT;
    if (mode == HIMO_ICP_FLOW && base_pitch != 3 && base_pitch != 4) return HIMO_ERR_INVALID_ARGUMENT;
    if (n == 0) return HIMO_OK;
    if (!d_pts || !d_out || (mode == HIMO_ICP_FLOW && !d_base)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_clusters > 0 && (!d_labels || !d_transform || !d_status)) return HIMO_ERR_INVALID_ARGUMENT;
    if (icp_misaligned(d_pts, 4) || icp_misaligned(d_out, 4) || icp_misaligned(d_base, 4) || icp_misaligned(d_labels, 4) ||
        icp_misaligned(d_transform, 8) || icp_misaligned(d_status, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("icp_apply_kernel", s);
        hipLaunchKernelGGL(icp_apply_kernel, dim3((unsigned)((n + kIcpThreads - 1) / kIcpThreads)), dim3(kIcpThreads), 0, s, n, d_pts, pitch,
                           n_clusters > 0 ? d_labels : nullptr, n_clusters, d_transform, d_status, mode, d_base, base_pitch, d_out);
    }
    HIMO_LAUNCH_CHECK("icp_apply_kernel");
    return HIMO_OK;
}
