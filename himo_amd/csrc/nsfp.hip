// nsfp.hip -- stage "NSFP, v1" (himo_amd/nsfp.py is the specification; PARITY UNPINNED): the truncated-Chamfer objective of the
// Neural Scene Flow Prior family for the fused coordinate-MLP kernels of csrc/nsffused.hip, and the early-stopping / keep-best rule
// held on the device.
//
//   L = (1/n0) sum_i [a_i <= tau^2] a_i + (1/n1) sum_j [b_j <= tau^2] b_j,  a_i = |moved_i - NN_pc1(moved_i)|^2, b_j = |pc1_j - NN_moved(pc1_j)|^2
//
// Once per sweep pair (himo_nsfp_prepare): pc1 is binned on the search grid (csrc/nngrid.h nng_build) as a searched set AND as a
// query set; it stays binned for the whole fit.  Per iteration (himo_nsfp_objective):
//   nsfp_moved_kernel   moved = x0 + out (the [n_pad][4] buffers of the fused path -> [n0][3]);
//   nng_build           of the moved points only;
//   nng_query           ONE launch, two jobs: moved -> pc1 and pc1 -> moved (exact, ties to the lowest row);
//   nsfp_b_kernel       the pc1 -> moved half: every pc1 row adds its pull to ITS nearest moved row -- many rows may share one -- as
//                       2^-40 fixed-point integers (integer atomics: the sum does not depend on the order; csrc/fastnsf.hip
//                       chamfer_trunc_b_kernel's scheme), and the half's loss sums per block;
//   nsfp_a_kernel       the moved -> pc1 half, the gathered fixed-point sums, d loss / d out, per-tile loss and count sums.
// Scaling.  himo_nsf_update divides the summed gradients and the summed loss by the summed counts.  Here the counts are the real rows
// of each tile (sum: n0), d_dout = n0 * d L / d out, and the loss list holds sum a (per tile) followed by (n0 / n1) sum b (per block of
// 256 pc1 rows, count 0): loss / n0 and gradient / n0 are L and its gradient -- himo_nsf_backward and himo_nsf_update run unchanged.
//
//   nsfp_keep_best_kernel   the stop rule (nsfp.py: best, best_iter, stale, stopped_at) as four float64 values in two slots: step t reads
//                       slot (t - 1) & 1 -- every thread for itself -- and thread 0 writes slot t & 1; when the rule says "improved"
//                       the iteration's MLP output is copied to best_out.  No host read is involved.
#include "nngrid.h"
#include "blockops.h"
#include <math.h>

namespace himo {

constexpr double kNsfpScatScale = 1099511627776.0;              // 2^40

struct NsfpArgs {
    int n0, n1, tiles;
    const float* x0; const float* out;                          // [n_pad][4]
    const float* pc1;                                           // [n1][3]
    float* moved;                                               // [n0][3]
    const float* d_a; const int* i_a;                           // moved -> pc1
    const float* d_b; const int* i_b;                           // pc1 -> moved
    float trunc2;
    double wb;                                                  // n0 / n1: what direction b carries
    float* dout;                                                // [n_pad][4]
    double* loss_partial; int* count_partial;                   // [tiles + ceil(n1 / 256)]
    unsigned long long* scat;                                   // [n0][3], zero between objective steps
};

__global__ __launch_bounds__(256) void nsfp_moved_kernel(NsfpArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n0) return;
    const float4 x = *reinterpret_cast<const float4*>(a.x0 + (size_t)i * 4), o = *reinterpret_cast<const float4*>(a.out + (size_t)i * 4);
    a.moved[(size_t)i * 3] = x.x + o.x; a.moved[(size_t)i * 3 + 1] = x.y + o.y; a.moved[(size_t)i * 3 + 2] = x.z + o.z;
}

__global__ __launch_bounds__(256) void nsfp_b_kernel(NsfpArgs a) {
    __shared__ double s_w[4];
    const int j = blockIdx.x * 256 + threadIdx.x;
    double t = 0.0;
    if (j < a.n1) {
        const float d = a.d_b[j];
        if (d <= a.trunc2) {
            t = (double)d;
            const int i = a.i_b[j];                             // (n0 > 0: the search found a row)
            const double w = 2.0 * a.wb * kNsfpScatScale;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                atomicAdd(a.scat + (size_t)i * 3 + c, (unsigned long long)__double2ll_rn((double)(a.moved[(size_t)i * 3 + c] - a.pc1[(size_t)j * 3 + c]) * w));
        }
    }
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        a.loss_partial[a.tiles + blockIdx.x] = ((s_w[0] + s_w[1]) + (s_w[2] + s_w[3])) * a.wb;
        a.count_partial[a.tiles + blockIdx.x] = 0;
    }
}

// a block = four tiles of 64 rows (the buffers hold whole blocks of four tiles), a wave = one tile
__global__ __launch_bounds__(256) void nsfp_a_kernel(NsfpArgs a) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    const bool real = row < a.n0;
    float g[3] = {0.f, 0.f, 0.f};
    double t = 0.0;
    if (real) {
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = a.moved[(size_t)row * 3 + c];
        if (a.n1 > 0) {
            const float d = a.d_a[row];
            if (d <= a.trunc2) {
                t = (double)d;
                const int j = a.i_a[row];
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] = 2.0f * (m[c] - a.pc1[(size_t)j * 3 + c]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned long long sc = a.scat[(size_t)row * 3 + c];
                if (sc) {
                    g[c] += (float)((double)(long long)sc * (1.0 / kNsfpScatScale));
                    a.scat[(size_t)row * 3 + c] = 0ull;         // (left clear for the next objective step)
                }
            }
        }
    }
    *reinterpret_cast<float4*>(a.dout + (size_t)row * 4) = float4{g[0], g[1], g[2], 0.f};       // (padding rows: zeros)
    t = wave_sum(t);
    const int cnt = __popcll(__ballot(real));
    if ((threadIdx.x & 63) == 0) {
        const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
        a.loss_partial[tile] = t;
        a.count_partial[tile] = cnt;
    }
}

__global__ __launch_bounds__(256) void nsfp_keep_best_kernel(int64_t n4, const float4* __restrict__ out, float4* __restrict__ best_out,
                                                             const double* __restrict__ loss, double* __restrict__ state, int step,
                                                             int patience, double min_delta) {
    const double* prev = state + ((step - 1) & 1) * 4;
    const double best = prev[0], L = *loss;
    const bool stopped = prev[3] != 0.0;
    const bool improved = !stopped && L < best - min_delta;    // (false for a NaN loss)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (improved && i < n4) best_out[i] = out[i];
    if (i == 0) {
        double* next = state + (step & 1) * 4;
        const double stale = improved ? 0.0 : prev[2] + 1.0;
        next[0] = improved ? L : best;
        next[1] = improved ? (double)step : prev[1];
        next[2] = stopped ? prev[2] : stale;
        next[3] = stopped ? prev[3] : ((!improved && patience > 0 && stale >= (double)patience) ? (double)step : 0.0);
    }
}

}  // namespace himo

using namespace himo;

static bool nsfp_grid_ok(int64_t n0, int64_t n1, float cell, int grid_w, int grid_h, int& status) {
    status = HIMO_OK;
    if (n0 < 0 || n1 < 0 || grid_w < 1 || grid_h < 1 || !(cell > 0.f)) status = HIMO_ERR_INVALID_ARGUMENT;
    else if (n0 > 0x7fffffff || n1 > 0x7fffffff || (int64_t)grid_w * grid_h > (1 << 20)) status = HIMO_ERR_UNSUPPORTED;
    return status == HIMO_OK;
}

static size_t nsfp_nng_bytes(int64_t n0, int64_t n1, int cells) { return nng_workspace_bytes(2, n0 > n1 ? n0 : n1, cells); }

// set 0 = pc1, set 1 = the moved points; both searched (and both queried); the fixed-point sums follow the search's workspace
static void nsfp_carve(void* ws, int n0, int n1, const float* pc1, const float* moved, int cells, NngSet* sets, unsigned long long** scat) {
    const float* pts[2] = {pc1, moved};
    const int n[2] = {n1, n0}, searched[2] = {1, 1};
    nng_carve(ws, sets, 2, pts, n, searched, cells);
    *scat = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + nsfp_nng_bytes(n0, n1, cells));
}

extern "C" size_t himo_nsfp_workspace_bytes(int64_t n0, int64_t n1, int grid_w, int grid_h) {
    if (n0 < 0 || n1 < 0 || grid_w < 1 || grid_h < 1) return 0;
    return nsfp_nng_bytes(n0, n1, grid_w * grid_h) + (size_t)(n0 > 0 ? n0 : 1) * 24 + 64;
}

// entries of the loss / count lists an objective step writes: one per 64-row tile of the padded moved set, one per 256 pc1 rows
extern "C" int64_t himo_nsfp_partials(int64_t n0, int64_t n1) {
    if (n0 < 0 || n1 < 0) return 0;
    return himo_nsf_padded_rows(n0) / 64 + (n1 + 255) / 256;
}

extern "C" int himo_nsfp_prepare(int64_t n0, int64_t n1, const float* d_pc1, float x0, float y0, float cell, int grid_w, int grid_h,
                                 void* d_workspace, size_t workspace_bytes, void* stream) {
    int st;
    if (!nsfp_grid_ok(n0, n1, cell, grid_w, grid_h, st)) return st;
    if (n0 == 0) return HIMO_OK;
    if (!d_workspace || !aligned16(d_workspace) || (n1 > 0 && !d_pc1)) return HIMO_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < himo_nsfp_workspace_bytes(n0, n1, grid_w, grid_h)) return HIMO_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    NngSet sets[2];
    unsigned long long* scat;
    nsfp_carve(d_workspace, (int)n0, (int)n1, d_pc1, nullptr, grid_w * grid_h, sets, &scat);
    HIMO_HIP(hipMemsetAsync(scat, 0, (size_t)n0 * 24, s));
    const NnGrid g{x0, y0, 1.0f / cell, cell, grid_w, grid_h};
    return nng_build(&sets[0], 1, g, s);
}

extern "C" int himo_nsfp_objective(int64_t n0, int64_t n1, const float* d_x0, const float* d_out, const float* d_pc1, float x0, float y0,
                                   float cell, int grid_w, int grid_h, float trunc_dist, float* d_moved, float* d_dist_a, int32_t* d_idx_a,
                                   float* d_dist_b, int32_t* d_idx_b, float* d_dout, double* d_loss_partial, int* d_count_partial,
                                   void* d_workspace, size_t workspace_bytes, void* stream) {
    int st;
    if (!nsfp_grid_ok(n0, n1, cell, grid_w, grid_h, st)) return st;
    if (n0 == 0) return HIMO_OK;
    if (!d_x0 || !d_out || !d_moved || !d_dist_a || !d_idx_a || !d_dout || !d_loss_partial || !d_count_partial || !d_workspace ||
        (n1 > 0 && (!d_pc1 || !d_dist_b || !d_idx_b)) || !(trunc_dist >= 0.f))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (!aligned16(d_x0) || !aligned16(d_out) || !aligned16(d_dout) || !aligned16(d_workspace)) return HIMO_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < himo_nsfp_workspace_bytes(n0, n1, grid_w, grid_h)) return HIMO_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    NngSet sets[2];
    NsfpArgs a{};
    nsfp_carve(d_workspace, (int)n0, (int)n1, d_pc1, d_moved, grid_w * grid_h, sets, &a.scat);
    const int64_t n_pad = himo_nsf_padded_rows(n0);
    a.n0 = (int)n0; a.n1 = (int)n1; a.tiles = (int)(n_pad / 64);
    a.x0 = d_x0; a.out = d_out; a.pc1 = d_pc1; a.moved = d_moved;
    a.d_a = d_dist_a; a.i_a = d_idx_a; a.d_b = d_dist_b; a.i_b = d_idx_b;
    a.trunc2 = trunc_dist * trunc_dist; a.wb = n1 > 0 ? (double)n0 / (double)n1 : 0.0;
    a.dout = d_dout; a.loss_partial = d_loss_partial; a.count_partial = d_count_partial;
    const NnGrid g{x0, y0, 1.0f / cell, cell, grid_w, grid_h};
    {
        ProfScope ps("nsfp_moved_kernel", s);
        hipLaunchKernelGGL(nsfp_moved_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, s, a);
    }
    HIMO_LAUNCH_CHECK("nsfp_moved_kernel");
    st = nng_build(&sets[1], 1, g, s);
    if (st != HIMO_OK) return st;
    const NngJob jobs[2] = {{1, 0, d_dist_a, d_idx_a}, {0, 1, d_dist_b, d_idx_b}};
    st = nng_query(sets, 2, jobs, n1 > 0 ? 2 : 1, g, s);
    if (st != HIMO_OK) return st;
    if (n1 > 0) {
        ProfScope ps("nsfp_b_kernel", s);
        hipLaunchKernelGGL(nsfp_b_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, a);
    }
    {
        ProfScope ps("nsfp_a_kernel", s);
        hipLaunchKernelGGL(nsfp_a_kernel, dim3((unsigned)(n_pad / 256)), dim3(256), 0, s, a);
    }
    HIMO_LAUNCH_CHECK("nsfp objective kernels");
    return HIMO_OK;
}

// One step of the stop / keep-best rule.  d_state: eight float64 (two slots of best, best_iter, stale, stopped_at; slot 0 starts as
// +inf, 0, 0, 0; after step t the state is slot t & 1); d_loss: L_t; d_out / d_best_out: himo_nsf_padded_rows(n) rows of 4 floats.
extern "C" int himo_nsfp_keep_best(int64_t n, const float* d_out, float* d_best_out, const double* d_loss, double* d_state, int step,
                                   int patience, double min_delta, void* stream) {
    if (n < 0 || step < 1 || !d_loss || !d_state || (n > 0 && (!d_out || !d_best_out))) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!aligned16(d_out) || !aligned16(d_best_out))) return HIMO_ERR_INVALID_ARGUMENT;
    const int64_t n4 = himo_nsf_padded_rows(n);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("nsfp_keep_best_kernel", s);
    hipLaunchKernelGGL(nsfp_keep_best_kernel, dim3((unsigned)(n4 > 0 ? n4 / 256 : 1)), dim3(256), 0, s, n4,
                       reinterpret_cast<const float4*>(d_out), reinterpret_cast<float4*>(d_best_out), d_loss, d_state, step, patience, min_delta);
    HIMO_LAUNCH_CHECK("nsfp_keep_best_kernel");
    return HIMO_OK;
}
