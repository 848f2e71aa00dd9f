// rigidrefine.hip -- cluster-rigid flow refinement ("cluster-rigid refinement, v1"; the rule is the module docstring of
// himo_amd/rigid_refine.py) for gfx950.  PARITY UNPINNED: the reference has no such stage; this one is checked against the numpy
// restatement of the written rule (tests/rigidrefine_ref.py).
//
// The clustered rows arrive SORTED BY LABEL, as in icpflow.hip: cluster k (label k + 1) owns the sorted rows offsets[k] ..
// offsets[k + 1], and d_rows[i] is the sweep row behind sorted row i.  Four launches per sweep, whatever the number of clusters, their
// sizes or the parameters:
//   rr_gather_kernel   a_s = a[rows], q_s = pc0[rows] + flow[rows] (one float32 addition per coordinate), packed [n_clustered][3].
//   rr_fit_kernel<64>  ALL of rule 2 -- every round's vote, passes, acceptance, static snap and claim -- for the clusters of at most
//                      kWaveMax rows: ONE WAVE owns a cluster, four clusters to a 256-thread block.  A sweep has thousands of 8-50
//                      point clusters; none of them takes a block, and no wave ever waits for another (no block barrier is used).
//   rr_fit_kernel<1024> the same code for the clusters above kWaveMax rows: one 1024-thread block owns a cluster.
//   rr_write_kernel    rules 2e and 3 over ALL N rows: a claimed row gets float32(R a + t) - pc0, every other row the bytes of its
//                      input flow.  The output is complete without a prior copy.
// Both fit kernels are launched over every cluster; a group whose cluster belongs to the other kernel returns at once.
//
// How the work is split, and why.  A group (wave or block) owns its cluster for the whole of rule 2, and lane l of the group owns the
// sorted rows lo + l, lo + l + NT, ... in every pass of every round.  So
//   - the per-row claim byte is written and read back by the same thread only (ordinary vector stores, program order), and the model
//     never leaves registers: rounds and passes need no launch and no traffic between groups;
//   - the votes are integer LDS atomics into the group's own histogram (a wave's quarter of the block's array, or the whole array);
//     nothing is flushed, because no cluster is shared between groups.  A histogram that does not fit ((2 half + 1)^2 > 2048 for a
//     wave, > 8192 for a block) lives in the workspace instead and takes integer global atomics, read back past the L1;
//   - the float64 sums have a FIXED shape: thread-strided partials in ascending row order, then a fixed tree (xor butterfly over the
//     wave; LDS tree 512, 256, ... 1 over the block).  No floating-point atomics: the same inputs give the same bytes on every run.
// A large cluster (one building: tens of thousands of rows) stays with ONE block of 1024 threads: a pass costs a few dozen float64
// operations per row, 40 rows per thread at 40k rows, and the whole of rule 2 stays one launch.  Splitting a cluster over blocks would
// put a grid-wide hand-off (or a launch) between every two of the models * (iters + 1) passes, each dearer than the pass itself.
//
// Built with -ffp-contract=off: every float operation rounds on its own, as numpy does.  Only sqrt and division appear (float32
// division in the vote, float64 elsewhere), both correctly rounded.
#include "himo_common.h"
#include "blockops.h"
#include <math.h>

namespace himo {

constexpr int kRrWaveMax = 1024;             // rows: up to here a wave owns the cluster (16 rows per lane), above it a block
constexpr int kRrBlockThreads = 1024;
constexpr int kRrWaveBlock = 256;            // four wave-owned clusters per block
constexpr int kRrLdsBins = 8192;             // 32 KB of counters per block: one histogram of a block group, four of wave groups
constexpr int kRrGatherThreads = 256;

struct RrArgs {
    int C;
    const int64_t* offsets;          // [C + 1]
    const int64_t* rows;             // [n_clustered] sweep row of every sorted row
    const float* a_s;                // [n_clustered][3]
    const float* q_s;                // [n_clustered][3]
    uint8_t* claim_s;                // [n_clustered] 0 = unclaimed, j = claimed by round j (each byte belongs to one thread)
    int8_t* claim;                   // [n] the same per sweep row (zeroed before the launch)
    int* counts;                     // [C][(2 half + 1)^2] zeroed, or nullptr when every histogram fits the LDS
    float bin;
    int half, iters, min_inliers, models;
    double tol2, min_ratio, static2;
    double* T;                       // [C][models][5]
    int* status;                     // [C][models][4]
};

// the group's earlier LDS / global writes and atomics are done and seen by the whole group
template <int NT> __device__ inline void rr_sync() {
    if constexpr (NT == 64) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

template <int NT> __global__ __launch_bounds__(NT == 64 ? kRrWaveBlock : NT) void rr_fit_kernel(RrArgs p) {
    constexpr int kGroups = NT == 64 ? kRrWaveBlock / 64 : 1;
    __shared__ int lds_hist[kRrLdsBins];
    __shared__ double red[NT == 64 ? 1 : NT];                                // blockops.h: the block group's tree; a wave uses none
    unsigned long long* const red_u = reinterpret_cast<unsigned long long*>(red);
    const int lane = (int)threadIdx.x % NT, group = (int)threadIdx.x / NT;
    const int k = (int)blockIdx.x * kGroups + group;
    if (k >= p.C) return;                                     // (a whole group: wave groups use no block barrier)
    const int64_t lo = p.offsets[k], hi = p.offsets[k + 1];
    const int64_t size = hi - lo;
    if ((size <= kRrWaveMax) != (NT == 64)) return;

    const int W = 2 * p.half + 1, WW = W * W;
    const bool in_lds = WW <= kRrLdsBins / kGroups;
    int* const lh = lds_hist + group * (kRrLdsBins / kGroups);             // the group's counters: here when they fit,
    int* const gh = in_lds ? nullptr : p.counts + (size_t)k * WW;            // else in the workspace (zeroed by the host)
    if (in_lds) {
        for (int b = lane; b < WW; b += NT) lh[b] = 0;
    }
    const float fhalf = (float)p.half;
    // every round starts as "not run" under the identity
    for (int j = lane; j < p.models; j += NT) {
        int* st = p.status + 4 * ((size_t)k * p.models + j);
        st[0] = HIMO_RIGID_NOT_RUN; st[1] = 0; st[2] = 0; st[3] = 0;
        double* t = p.T + 5 * ((size_t)k * p.models + j);
        t[0] = 1.0; t[1] = 0.0; t[2] = 0.0; t[3] = 0.0; t[4] = 0.0;
    }
    for (int64_t i = lo + lane; i < hi; i += NT) p.claim_s[i] = 0;
    rr_sync<NT>();

    for (int j = 0; j < p.models; ++j) {
        // ---- 2a: the vote of the unclaimed rows (integers) ----
        for (int64_t i = lo + lane; i < hi; i += NT) {
            if (p.claim_s[i]) continue;
            const float* a = p.a_s + 3 * i;
            const float* q = p.q_s + 3 * i;
            const float rx = q[0] - a[0], ry = q[1] - a[1];
            const float kx = rintf(rx / p.bin), ky = rintf(ry / p.bin);
            if (!(fabsf(kx) <= fhalf && fabsf(ky) <= fhalf)) continue;
            const int b = ((int)ky + p.half) * W + ((int)kx + p.half);
            if (in_lds) atomicAdd(&lh[b], 1);
            else atomicAdd(&gh[b], 1);
        }
        rr_sync<NT>();
        // the peak as the maximum of one key: higher count, then smaller kx^2 + ky^2, then lower (ky, kx) = lower bin index (both
        // inverted); every bin goes back to zero for the next round, cleared by the lane that read it
        unsigned long long best = 0ull;
        for (int b = lane; b < WW; b += NT) {
            const int cnt = in_lds ? lh[b] : __hip_atomic_load(&gh[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cnt) {
                if (in_lds) lh[b] = 0;
                else gh[b] = 0;
            }
            const int by = b / W - p.half, bx = b % W - p.half;
            const unsigned rank = ((unsigned)(bx * bx + by * by) << 15) | (unsigned)b;
            const unsigned long long key = ((unsigned long long)(unsigned)cnt << 32) | (0xffffffffu - rank);
            best = key > best ? key : best;
        }
        best = group_max_u64<NT>(best, red_u);
        rr_sync<NT>();
        const int pb = (int)((0xffffffffu - (unsigned)best) & 0x7fffu);
        const int pky = pb / W - p.half, pkx = pb % W - p.half;
        double c = 1.0, s = 0.0, tx = (double)pkx * (double)p.bin, ty = (double)pky * (double)p.bin, tz = 0.0;

        // ---- 2b: passes 0 .. iters ----
        int n = 0;
        bool failed = false;
        for (int pass = 0; pass <= p.iters; ++pass) {
            double cnt = 0.0, sa[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0};
            auto inlier = [&](int64_t i) {
                if (p.claim_s[i]) return false;
                const float* a = p.a_s + 3 * i;
                const float* q = p.q_s + 3 * i;
                const double x = (double)a[0], y = (double)a[1], z = (double)a[2];
                const double dx = (double)q[0] - ((c * x - s * y) + tx), dy = (double)q[1] - ((s * x + c * y) + ty);
                double e2 = dx * dx + dy * dy;
                if (pass > 0) {                                  // the start has no z
                    const double dz = (double)q[2] - (z + tz);
                    e2 = e2 + dz * dz;
                }
                return e2 <= p.tol2;
            };
            for (int64_t i = lo + lane; i < hi; i += NT) {
                if (!inlier(i)) continue;
                const float* a = p.a_s + 3 * i;
                const float* q = p.q_s + 3 * i;
                cnt += 1.0;
#pragma unroll
                for (int d = 0; d < 3; ++d) { sa[d] = sa[d] + (double)a[d]; sq[d] = sq[d] + (double)q[d]; }
            }
            n = (int)group_sum<NT>(cnt, red);                    // whole numbers below 2^31: exact in any order
            if (pass == p.iters) break;
            if (n < p.min_inliers) { failed = true; break; }
            double ab[3], qb[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                ab[d] = group_sum<NT>(sa[d], red) / (double)n;
                qb[d] = group_sum<NT>(sq[d], red) / (double)n;
            }
            double A = 0.0, B = 0.0;
            for (int64_t i = lo + lane; i < hi; i += NT) {
                if (!inlier(i)) continue;
                const float* a = p.a_s + 3 * i;
                const float* q = p.q_s + 3 * i;
                const double ax = (double)a[0] - ab[0], ay = (double)a[1] - ab[1], qx = (double)q[0] - qb[0], qy = (double)q[1] - qb[1];
                A = A + (ax * qx + ay * qy);
                B = B + (ax * qy - ay * qx);
            }
            A = group_sum<NT>(A, red);
            B = group_sum<NT>(B, red);
            const double h = sqrt(A * A + B * B);
            c = h == 0.0 ? 1.0 : A / h;
            s = h == 0.0 ? 0.0 : B / h;
            tx = qb[0] - (c * ab[0] - s * ab[1]);
            ty = qb[1] - (s * ab[0] + c * ab[1]);
            tz = qb[2] - ab[2];
        }

        // ---- 2c, 2d: acceptance and the static snap ----
        int state = HIMO_RIGID_ACCEPTED;
        if (failed) state = HIMO_RIGID_FAILED;
        else if (n < p.min_inliers || !((double)n / (double)size >= p.min_ratio)) state = HIMO_RIGID_REJECTED;
        if (state == HIMO_RIGID_ACCEPTED) {
            double far = 0.0;
            for (int64_t i = lo + lane; i < hi; i += NT) {
                if (p.claim_s[i]) continue;
                const float* a = p.a_s + 3 * i;
                const float* q = p.q_s + 3 * i;
                const double x = (double)a[0], y = (double)a[1], z = (double)a[2];
                const double mx = (c * x - s * y) + tx, my = (s * x + c * y) + ty, mz = z + tz;
                const double ex = (double)q[0] - mx, ey = (double)q[1] - my, ez = (double)q[2] - mz;
                if (!((ex * ex + ey * ey) + ez * ez <= p.tol2)) continue;
                const double ux = mx - x, uy = my - y, uz = mz - z;
                const double d2 = (ux * ux + uy * uy) + uz * uz;
                far = d2 > far ? d2 : far;
                p.claim_s[i] = (uint8_t)(j + 1);                 // 2e: the claim (this thread's own byte)
                p.claim[p.rows[i]] = (int8_t)(j + 1);
            }
            far = __builtin_bit_cast(double, group_max_u64<NT>(__builtin_bit_cast(unsigned long long, far), red_u));
            if (far < p.static2) {
                state = HIMO_RIGID_STATIC;
                c = 1.0; s = 0.0; tx = 0.0; ty = 0.0; tz = 0.0;
            }
        }
        if (lane == 0) {
            int* st = p.status + 4 * ((size_t)k * p.models + j);
            st[0] = state; st[1] = n; st[2] = pkx; st[3] = pky;
            double* t = p.T + 5 * ((size_t)k * p.models + j);
            t[0] = c; t[1] = s; t[2] = tx; t[3] = ty; t[4] = tz;
        }
        if (state == HIMO_RIGID_FAILED || state == HIMO_RIGID_REJECTED) break;     // claims nothing and ends the cluster
    }
}

__global__ __launch_bounds__(kRrGatherThreads) void rr_gather_kernel(int64_t nc, const int64_t* __restrict__ rows, const float* __restrict__ a,
                                                                     const float* __restrict__ pc0, int pitch, const float* __restrict__ flow,
                                                                     float* __restrict__ a_s, float* __restrict__ q_s) {
    const int64_t i = (int64_t)blockIdx.x * kRrGatherThreads + threadIdx.x;
    if (i >= nc) return;
    const int64_t r = rows[i];
    const float* pa = a + 3 * r;
    const float* pp = pc0 + r * pitch;
    const float* pf = flow + 3 * r;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        a_s[3 * i + d] = pa[d];
        q_s[3 * i + d] = pp[d] + pf[d];
    }
}

__global__ __launch_bounds__(kRrGatherThreads) void rr_write_kernel(int64_t n, const float* __restrict__ a, const float* __restrict__ pc0, int pitch,
                                                                    const uint32_t* __restrict__ flow, const int* __restrict__ labels,
                                                                    const int8_t* __restrict__ claim, int C, int models,
                                                                    const double* __restrict__ T, uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kRrGatherThreads + threadIdx.x;
    if (i >= n) return;
    const int j = (int)claim[i];
    const int l = j > 0 ? labels[i] : 0;
    if (j >= 1 && j <= models && l >= 1 && l <= C) {
        const double* t = T + 5 * ((size_t)(l - 1) * models + (j - 1));
        const float* pa = a + 3 * i;
        const float* pp = pc0 + i * pitch;
        const double x = (double)pa[0], y = (double)pa[1], z = (double)pa[2];
        const float mx = (float)((t[0] * x - t[1] * y) + t[2]);
        const float my = (float)((t[1] * x + t[0] * y) + t[3]);
        const float mz = (float)(z + t[4]);
        out[3 * i + 0] = __builtin_bit_cast(uint32_t, mx - pp[0]);
        out[3 * i + 1] = __builtin_bit_cast(uint32_t, my - pp[1]);
        out[3 * i + 2] = __builtin_bit_cast(uint32_t, mz - pp[2]);
    } else {                                                   // rule 3: the bytes of the input
        out[3 * i + 0] = flow[3 * i + 0];
        out[3 * i + 1] = flow[3 * i + 1];
        out[3 * i + 2] = flow[3 * i + 2];
    }
}

static bool rr_params_ok(const himo_rigid_params* p) {
    if (!p) return false;
    const float fl[4] = {p->bin, p->tol, p->min_ratio, p->static_disp};
    for (float v : fl)
        if (!isfinite(v) || !(v > 0.f)) return false;
    return p->half >= 1 && p->half <= 64 && p->iters >= 1 && p->min_inliers >= 1 && p->models >= 1 && p->models <= HIMO_RIGID_MAX_MODELS;
}

static bool rr_offsets_ok(int64_t n, int C, const int64_t* h) {
    if (h[0] != 0 || h[C] != n) return false;
    for (int k = 0; k < C; ++k)
        if (h[k] < 0 || h[k + 1] < h[k]) return false;
    return true;
}

static bool rr_misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

static bool rr_counts_in_workspace(int half) { const int W = 2 * half + 1; return W * W > kRrLdsBins / (kRrWaveBlock / 64); }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_rigid_refine_workspace_bytes(int64_t n_clustered, int n_clusters, int half, int models) {
    if (n_clustered < 0 || n_clustered > 0x7fffffffLL || n_clusters < 0 || half < 1 || half > 64 || models < 1 || models > HIMO_RIGID_MAX_MODELS) return 0;
    const int W = 2 * half + 1;
    size_t bytes = 2 * round_up((size_t)n_clustered * 3 * sizeof(float), 256) + round_up((size_t)n_clustered, 256);
    if (rr_counts_in_workspace(half)) bytes += round_up((size_t)n_clusters * W * W * sizeof(int32_t), 256);
    return bytes > 256 ? bytes : 256;
}

extern "C" int himo_rigid_refine(int64_t n, const float* d_pc0, int pitch, const float* d_flow, const float* d_moved, const int32_t* d_labels,
                                 int64_t n_clustered, const int64_t* d_rows, int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets,
                                 const himo_rigid_params* params, int32_t* d_status, double* d_transform, int8_t* d_claim, float* d_out,
                                 void* d_workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || n_clustered < 0 || n_clustered > n || n_clusters < 0 || !rr_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (pitch != 3 && pitch != 4) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n == 0) return HIMO_OK;
    if (n_clusters == 0 && n_clustered != 0) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_pc0 || !d_flow || !d_moved || !d_claim || !d_out) return HIMO_ERR_INVALID_ARGUMENT;
    if (rr_misaligned(d_pc0, 4) || rr_misaligned(d_flow, 4) || rr_misaligned(d_moved, 4) || rr_misaligned(d_out, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_clusters > 0) {
        if (!h_offsets || !d_offsets || !rr_offsets_ok(n_clustered, n_clusters, h_offsets)) return HIMO_ERR_INVALID_ARGUMENT;
        if (!d_labels || !d_status || !d_transform || (n_clustered > 0 && !d_rows)) return HIMO_ERR_INVALID_ARGUMENT;
        if (rr_misaligned(d_labels, 4) || rr_misaligned(d_rows, 8) || rr_misaligned(d_offsets, 8) || rr_misaligned(d_status, 4) ||
            rr_misaligned(d_transform, 8)) return HIMO_ERR_INVALID_ARGUMENT;
        if (!d_workspace || !aligned16(d_workspace) ||
            workspace_bytes < himo_rigid_refine_workspace_bytes(n_clustered, n_clusters, params->half, params->models)) return HIMO_ERR_WORKSPACE;
    }

    hipStream_t s = (hipStream_t)stream;
    HIMO_HIP(hipMemsetAsync(d_claim, 0, (size_t)n, s));
    if (n_clusters > 0) {
        char* w = reinterpret_cast<char*>(d_workspace);
        float* a_s = reinterpret_cast<float*>(w);
        w += round_up((size_t)n_clustered * 3 * sizeof(float), 256);
        float* q_s = reinterpret_cast<float*>(w);
        w += round_up((size_t)n_clustered * 3 * sizeof(float), 256);
        uint8_t* claim_s = reinterpret_cast<uint8_t*>(w);
        w += round_up((size_t)n_clustered, 256);
        int* counts = nullptr;
        const int W = 2 * params->half + 1;
        if (rr_counts_in_workspace(params->half)) {
            counts = reinterpret_cast<int*>(w);
            HIMO_HIP(hipMemsetAsync(counts, 0, (size_t)n_clusters * W * W * sizeof(int32_t), s));
        }
        if (n_clustered > 0) {
            ProfScope ps("rr_gather_kernel", s);
            hipLaunchKernelGGL(rr_gather_kernel, dim3((unsigned)((n_clustered + kRrGatherThreads - 1) / kRrGatherThreads)), dim3(kRrGatherThreads), 0, s,
                               n_clustered, d_rows, d_moved, d_pc0, pitch, d_flow, a_s, q_s);
        }
        HIMO_LAUNCH_CHECK("rr_gather_kernel");
        RrArgs p;
        p.C = n_clusters; p.offsets = d_offsets; p.rows = d_rows; p.a_s = a_s; p.q_s = q_s; p.claim_s = claim_s; p.claim = d_claim; p.counts = counts;
        p.bin = params->bin; p.half = params->half; p.iters = params->iters; p.min_inliers = params->min_inliers; p.models = params->models;
        p.tol2 = (double)params->tol * (double)params->tol;
        p.min_ratio = (double)params->min_ratio;
        p.static2 = (double)params->static_disp * (double)params->static_disp;
        p.T = d_transform; p.status = d_status;
        {
            ProfScope ps("rr_fit_kernel_wave", s);
            constexpr int per_block = kRrWaveBlock / 64;
            hipLaunchKernelGGL(rr_fit_kernel<64>, dim3((unsigned)((n_clusters + per_block - 1) / per_block)), dim3(kRrWaveBlock), 0, s, p);
        }
        HIMO_LAUNCH_CHECK("rr_fit_kernel_wave");
        {
            ProfScope ps("rr_fit_kernel_block", s);
            hipLaunchKernelGGL(rr_fit_kernel<kRrBlockThreads>, dim3((unsigned)n_clusters), dim3(kRrBlockThreads), 0, s, p);
        }
        HIMO_LAUNCH_CHECK("rr_fit_kernel_block");
    }
    {
        ProfScope ps("rr_write_kernel", s);
        hipLaunchKernelGGL(rr_write_kernel, dim3((unsigned)((n + kRrGatherThreads - 1) / kRrGatherThreads)), dim3(kRrGatherThreads), 0, s, n, d_moved,
                           d_pc0, pitch, reinterpret_cast<const uint32_t*>(d_flow), d_labels, d_claim, n_clusters, params->models, d_transform,
                           reinterpret_cast<uint32_t*>(d_out));
    }
    HIMO_LAUNCH_CHECK("rr_write_kernel");
    return HIMO_OK;
}
