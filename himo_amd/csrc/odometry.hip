// odometry.hip -- one iteration of whole-sweep, 6-DoF scan-to-map ICP ("sweep odometry, v1"; the rule is the module docstring of
// himo_amd/odometry.py) for gfx950.  PARITY UNPINNED: the reference has no such stage; this one is checked against the numpy restatement
// of the written rule (tests/odometry_ref.py).
//
// The map (one centroid per voxel, himo_accum_emit's rows) is binned ONCE per sweep on a BEV cell grid whose cell edge is max_dist
// (nng_build of nngrid.h, the row-major copy only).  An iteration is then three launches and no rebinning:
//   odom_step_kernel    a lane per source row, grid-stride over a capped grid.  m = float32(T p) evaluated in float64; the 3 x 3 cells
//                       around m's cell are, row by row of the grid, ONE contiguous run of candidates (16-byte loads); the nearest is the
//                       minimum of ONE 64-bit key (float32 d2 bits, then the row: ties keep the lowest row, whatever order the counting
//                       sort left the cell in).  Inliers add their 17 distinct weighted terms and the count to float64 registers; one
//                       block_sum (blockops.h) per block writes the block's partials.
//   odom_solve_kernel   one block: thread t adds the partials of blocks t, t + 256, ... in ascending order, the same fixed LDS tree, then
//                       thread 0 alone expands the sums, runs the unpivoted Cholesky, the Cayley update and the status.
// No floating-point atomics: the same inputs give the same bytes on every run.  A step on a state that is not RUNNING writes nothing
// (both kernels read the status word first), so `iters` steps are enqueued back to back with no host wait in between.
//
// Built with -ffp-contract=off: every operation rounds on its own, as numpy does.  Only + - * / and sqrt appear, all correctly rounded.
#include "nngrid.h"
#include "blockops.h"
#include <math.h>

namespace himo {

constexpr int kOdomThreads = 256;
constexpr int kOdomMaxBlocks = 1024;         // the step's grid cap: 4 blocks a CU
// the distinct sums of a pass: w, w mx, w my, w mz | H33 H34 H35 H44 H45 H55 | g0 .. g5 | cost | count
constexpr int kOdomSums = 18;
constexpr unsigned long long kOdomNone = 0x7f800000ffffffffull;       // (+inf, row -1): no candidate

struct OdomStepArgs {
    int64_t n;
    const float* src;
    int pitch;
    const float* map;                // [n_map][3]
    const int* cell_offset;          // [cells + 1] of the binned map (row-major cell order)
    const float4* sorted;            // its rows in that order: x, y, z, original row
    NnGrid g;
    float max_d2;
    double gm;
    const himo_odom_state* state;
    int* nn_idx;                     // [n] or nullptr
    float* nn_d2;                    // [n] or nullptr
    double* partial;                 // [gridDim.x][kOdomSums]
};

__global__ __launch_bounds__(kOdomThreads) void odom_step_kernel(OdomStepArgs a) {
    if (a.state->status != HIMO_ODOM_RUNNING) return;          // the same word for every thread of the grid
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = a.state->T[k];
    double acc[kOdomSums];
#pragma unroll
    for (int k = 0; k < kOdomSums; ++k) acc[k] = 0.0;
    const NnGrid& g = a.g;
    const int64_t stride = (int64_t)gridDim.x * kOdomThreads;
    for (int64_t i = (int64_t)blockIdx.x * kOdomThreads + threadIdx.x; i < a.n; i += stride) {
        const float* p = a.src + i * a.pitch;
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        const float mx = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
        const float my = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
        const float mz = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
        unsigned long long best = kOdomNone;
        if (isfinite(mx) && isfinite(my) && isfinite(mz)) {
            const int cx = nng_cell_x(g, mx), cy = nng_cell_y(g, my);
            const int xa = max(cx - 1, 0), xb = min(cx + 1, g.gw - 1), ya = max(cy - 1, 0), yb = min(cy + 1, g.gh - 1);
            for (int yy = ya; yy <= yb; ++yy) {
                const int r0 = a.cell_offset[yy * g.gw + xa], r1 = a.cell_offset[yy * g.gw + xb + 1];
                for (int j = r0; j < r1; ++j) {
                    const float4 c = a.sorted[j];
                    const float dx = c.x - mx, dy = c.y - my, dz = c.z - mz;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(c.w);
                    best = key < best ? key : best;
                }
            }
        }
        const float d2 = __uint_as_float((unsigned)(best >> 32));
        const int row = (int)(unsigned)best;
        if (a.nn_idx) a.nn_idx[i] = row;
        if (a.nn_d2) a.nn_d2[i] = d2;
        if (!(best != kOdomNone && d2 <= a.max_d2)) continue;
        const float* q = a.map + 3 * (int64_t)row;
        const double ax = (double)mx, ay = (double)my, az = (double)mz;
        const double rx = (double)q[0] - ax, ry = (double)q[1] - ay, rz = (double)q[2] - az;
        const double rr = (rx * rx + ry * ry) + rz * rz;
        const double u = a.gm / (a.gm + rr);
        const double w = u * u;
        acc[0] = acc[0] + w;
        acc[1] = acc[1] + w * ax;
        acc[2] = acc[2] + w * ay;
        acc[3] = acc[3] + w * az;
        acc[4] = acc[4] + w * (ay * ay + az * az);
        acc[5] = acc[5] + -(w * (ax * ay));
        acc[6] = acc[6] + -(w * (ax * az));
        acc[7] = acc[7] + w * (ax * ax + az * az);
        acc[8] = acc[8] + -(w * (ay * az));
        acc[9] = acc[9] + w * (ax * ax + ay * ay);
        acc[10] = acc[10] + w * rx;
        acc[11] = acc[11] + w * ry;
        acc[12] = acc[12] + w * rz;
        acc[13] = acc[13] + w * (ay * rz - az * ry);
        acc[14] = acc[14] + w * (az * rx - ax * rz);
        acc[15] = acc[15] + w * (ax * ry - ay * rx);
        acc[16] = acc[16] + w * rr;
        acc[17] = acc[17] + 1.0;
    }
    block_sum<kOdomThreads, kOdomSums>(acc, a.partial + (size_t)blockIdx.x * kOdomSums);
}

struct OdomSolveArgs {
    int n_blocks;
    const double* partial;
    double* total;                   // [kOdomSums] scratch
    int min_pairs;
    double eps_t2, eps_r2;
    himo_odom_state* state;
};

// the 21 upper entries of H (row-major), the 6 of g and the cost from the distinct sums: the entries that repeat a sum, negate one or are
// structurally zero are written out here
__device__ inline void odom_expand(const double* u, double* s) {
    s[0] = u[0];  s[1] = 0.0;   s[2] = 0.0;   s[3] = 0.0;    s[4] = u[3];   s[5] = -u[2];
    s[6] = u[0];  s[7] = 0.0;   s[8] = -u[3]; s[9] = 0.0;    s[10] = u[1];
    s[11] = u[0]; s[12] = u[2]; s[13] = -u[1]; s[14] = 0.0;
    s[15] = u[4]; s[16] = u[5]; s[17] = u[6];
    s[18] = u[7]; s[19] = u[8];
    s[20] = u[9];
#pragma unroll
    for (int k = 0; k < 7; ++k) s[21 + k] = u[10 + k];
}

// H xi = g by an unpivoted Cholesky; false when a pivot is not finite or not > 0, or a component of xi is not finite
__device__ inline bool odom_cholesky(const double* s, double* xi) {
    double H[6][6], L[6][6], yv[6];
    int at = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) H[i][j] = s[at++];
    for (int j = 0; j < 6; ++j) {
        double d = H[j][j];
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(isfinite(d) && d > 0.0)) return false;
        L[j][j] = sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double v = H[j][i];
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double v = s[21 + i];
        for (int k = 0; k < i; ++k) v = v - L[i][k] * yv[k];
        yv[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = yv[i];
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * xi[k];
        xi[i] = v / L[i][i];
    }
    for (int i = 0; i < 6; ++i)
        if (!isfinite(xi[i])) return false;
    return true;
}

__global__ __launch_bounds__(kOdomThreads) void odom_solve_kernel(OdomSolveArgs a) {
    himo_odom_state* st = a.state;
    if (st->status != HIMO_ODOM_RUNNING) return;
    double acc[kOdomSums];
#pragma unroll
    for (int k = 0; k < kOdomSums; ++k) acc[k] = 0.0;
    for (int b = threadIdx.x; b < a.n_blocks; b += kOdomThreads)
#pragma unroll
        for (int k = 0; k < kOdomSums; ++k) acc[k] = acc[k] + a.partial[(size_t)b * kOdomSums + k];
    block_sum<kOdomThreads, kOdomSums>(acc, a.total);
    if (threadIdx.x != 0) return;
    double s[28];
    odom_expand(a.total, s);
    const int n = (int)a.total[17];
#pragma unroll
    for (int k = 0; k < 28; ++k) st->sums[k] = s[k];
    st->cost = s[27];
    st->pairs = n;
    st->iters = st->iters + 1;
    if (n < a.min_pairs) { st->status = HIMO_ODOM_FAILED_PAIRS; return; }
    double xi[6];
    if (!odom_cholesky(s, xi)) { st->status = HIMO_ODOM_FAILED_SOLVE; return; }
#pragma unroll
    for (int k = 0; k < 6; ++k) st->xi[k] = xi[k];
    // the Cayley map of omega: a = omega / 2, D = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a)
    const double ax = 0.5 * xi[3], ay = 0.5 * xi[4], az = 0.5 * xi[5];
    const double bx = 2.0 * ax, by = 2.0 * ay, bz = 2.0 * az;
    const double aa = (ax * ax + ay * ay) + az * az;
    const double one = 1.0 - aa, den = 1.0 + aa;
    double D[9];
    D[0] = (one + bx * ax) / den; D[1] = (bx * ay - bz) / den;  D[2] = (bx * az + by) / den;
    D[3] = (by * ax + bz) / den;  D[4] = (one + by * ay) / den; D[5] = (by * az - bx) / den;
    D[6] = (bz * ax - by) / den;  D[7] = (bz * ay + bx) / den;  D[8] = (one + bz * az) / den;
    double T[12], N[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = st->T[k];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) N[4 * i + j] = (D[3 * i] * T[j] + D[3 * i + 1] * T[4 + j]) + D[3 * i + 2] * T[8 + j];
        N[4 * i + 3] = ((D[3 * i] * T[3] + D[3 * i + 1] * T[7]) + D[3 * i + 2] * T[11]) + xi[i];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) st->T[k] = N[k];
    const double tt = (xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2];
    const double oo = (xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5];
    if (tt < a.eps_t2 && oo < a.eps_r2) st->status = HIMO_ODOM_CONVERGED;
}

__global__ void odom_init_kernel(himo_odom_state init, const double* vote, himo_odom_state* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (vote) { init.T[3] = vote[2]; init.T[7] = vote[3]; }
    *out = init;
}

static bool odom_params_ok(const himo_odom_params* p) {
    if (!p) return false;
    const float fl[4] = {p->x0, p->y0, p->max_dist, p->gm_scale};
    for (float v : fl)
        if (!isfinite(v)) return false;
    if (!(p->max_dist > 0.f) || !(p->gm_scale > 0.f) || !isfinite(1.0f / p->max_dist) || !isfinite(p->max_dist * p->max_dist)) return false;
    if (!isfinite(p->eps_t2) || !isfinite(p->eps_r2) || !(p->eps_t2 > 0.0) || !(p->eps_r2 > 0.0)) return false;
    return p->gw >= 1 && p->gh >= 1 && p->min_pairs >= 1 && p->iters >= 1 && p->iters <= 1024;
}

static bool odom_misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

static size_t odom_grid_bytes(int64_t n_map, int cells) { return round_up(nng_workspace_bytes(1, n_map, cells), 256); }

// everything the three entry points refuse alike; HIMO_OK: the call may launch
static int odom_admit(int64_t n, const float* d_src, int pitch, int64_t n_map, const float* d_map, const himo_odom_params* p,
                      const himo_odom_state* d_state, const int32_t* d_nn_idx, const float* d_nn_d2, const void* d_workspace,
                      size_t workspace_bytes, bool with_src) {
    if (n < 0 || n_map < 0 || !odom_params_ok(p)) return HIMO_ERR_INVALID_ARGUMENT;
    if (with_src && pitch != 3 && pitch != 4) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL || n_map > 0x7fffffffLL || (int64_t)p->gw * p->gh > (1 << 20)) return HIMO_ERR_UNSUPPORTED;
    if ((with_src && (!d_state || (n > 0 && !d_src))) || (n_map > 0 && !d_map)) return HIMO_ERR_INVALID_ARGUMENT;
    if (odom_misaligned(d_src, 4) || odom_misaligned(d_map, 4) || odom_misaligned(d_state, 8) || odom_misaligned(d_nn_idx, 4) ||
        odom_misaligned(d_nn_d2, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < himo_odom_workspace_bytes(n_map, p)) return HIMO_ERR_WORKSPACE;
    return HIMO_OK;
}

static NnGrid odom_grid(const himo_odom_params* p) { return NnGrid{p->x0, p->y0, 1.0f / p->max_dist, p->max_dist, p->gw, p->gh}; }

static int odom_map(int64_t n_map, const float* d_map, const himo_odom_params* p, void* d_workspace, hipStream_t s) {
    NngSet set;
    const float* pts[1] = {d_map};
    const int cnt[1] = {(int)n_map}, searched[1] = {0};
    nng_carve(d_workspace, &set, 1, pts, cnt, searched, p->gw * p->gh);
    return nng_build(&set, 1, odom_grid(p), s);
}

static int odom_step(int64_t n, const float* d_src, int pitch, int64_t n_map, const float* d_map, const himo_odom_params* p,
                     himo_odom_state* d_state, int32_t* d_nn_idx, float* d_nn_d2, void* d_workspace, hipStream_t s) {
    NngSet set;
    const float* pts[1] = {d_map};
    const int cnt[1] = {(int)n_map}, searched[1] = {0};
    nng_carve(d_workspace, &set, 1, pts, cnt, searched, p->gw * p->gh);
    double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(d_workspace) + odom_grid_bytes(n_map, p->gw * p->gh));
    const int64_t want = (n + kOdomThreads - 1) / kOdomThreads;
    const int blocks = (int)(want < 1 ? 1 : (want > kOdomMaxBlocks ? kOdomMaxBlocks : want));
    OdomStepArgs a;
    a.n = n; a.src = d_src; a.pitch = pitch; a.map = d_map; a.cell_offset = set.offset; a.sorted = set.sorted; a.g = odom_grid(p);
    a.max_d2 = p->max_dist * p->max_dist; a.gm = (double)p->gm_scale; a.state = d_state; a.nn_idx = d_nn_idx; a.nn_d2 = d_nn_d2;
    a.partial = partial;
    {
        ProfScope ps("odom_step_kernel", s);
        hipLaunchKernelGGL(odom_step_kernel, dim3((unsigned)blocks), dim3(kOdomThreads), 0, s, a);
    }
    HIMO_LAUNCH_CHECK("odom_step_kernel");
    OdomSolveArgs b;
    b.n_blocks = blocks; b.partial = partial; b.total = partial + (size_t)kOdomMaxBlocks * kOdomSums; b.min_pairs = p->min_pairs;
    b.eps_t2 = p->eps_t2; b.eps_r2 = p->eps_r2; b.state = d_state;
    {
        ProfScope ps("odom_solve_kernel", s);
        hipLaunchKernelGGL(odom_solve_kernel, dim3(1), dim3(kOdomThreads), 0, s, b);
    }
    HIMO_LAUNCH_CHECK("odom_solve_kernel");
    return HIMO_OK;
}

}  // namespace himo

using namespace himo;

extern "C" size_t himo_odom_workspace_bytes(int64_t n_map, const himo_odom_params* params) {
    if (n_map < 0 || n_map > 0x7fffffffLL || !odom_params_ok(params) || (int64_t)params->gw * params->gh > (1 << 20)) return 0;
    return odom_grid_bytes(n_map, params->gw * params->gh) + round_up((size_t)(kOdomMaxBlocks + 1) * kOdomSums * sizeof(double), 256);
}

extern "C" int himo_odom_init(const double* h_transform, const double* d_vote, himo_odom_state* d_state, void* stream) {
    if (!d_state || odom_misaligned(d_state, 8) || odom_misaligned(d_vote, 8)) return HIMO_ERR_INVALID_ARGUMENT;
    himo_odom_state init = {};
    init.T[0] = init.T[5] = init.T[10] = 1.0;
    if (h_transform)
        for (int k = 0; k < 12; ++k) {
            if (!isfinite(h_transform[k])) return HIMO_ERR_INVALID_ARGUMENT;
            init.T[k] = h_transform[k];
        }
    init.status = HIMO_ODOM_RUNNING;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(odom_init_kernel, dim3(1), dim3(1), 0, s, init, d_vote, d_state);
    HIMO_LAUNCH_CHECK("odom_init_kernel");
    return HIMO_OK;
}

extern "C" int himo_odom_map(int64_t n_map, const float* d_map, const himo_odom_params* params, void* d_workspace, size_t workspace_bytes,
                             void* stream) {
    const int st = odom_admit(0, nullptr, 3, n_map, d_map, params, nullptr, nullptr, nullptr, d_workspace, workspace_bytes, false);
    if (st != HIMO_OK) return st;
    return odom_map(n_map, d_map, params, d_workspace, (hipStream_t)stream);
}

extern "C" int himo_odom_step(int64_t n, const float* d_src, int pitch, int64_t n_map, const float* d_map, const himo_odom_params* params,
                              himo_odom_state* d_state, int32_t* d_nn_idx, float* d_nn_d2, void* d_workspace, size_t workspace_bytes,
                              void* stream) {
    const int st = odom_admit(n, d_src, pitch, n_map, d_map, params, d_state, d_nn_idx, d_nn_d2, d_workspace, workspace_bytes, true);
    if (st != HIMO_OK) return st;
    return odom_step(n, d_src, pitch, n_map, d_map, params, d_state, d_nn_idx, d_nn_d2, d_workspace, (hipStream_t)stream);
}

extern "C" int himo_odom_register(int64_t n, const float* d_src, int pitch, int64_t n_map, const float* d_map, const himo_odom_params* params,
                                  himo_odom_state* d_state, void* d_workspace, size_t workspace_bytes, void* stream) {
    int st = odom_admit(n, d_src, pitch, n_map, d_map, params, d_state, nullptr, nullptr, d_workspace, workspace_bytes, true);
    if (st != HIMO_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    st = odom_map(n_map, d_map, params, d_workspace, s);
    for (int it = 0; st == HIMO_OK && it < params->iters; ++it)
        st = odom_step(n, d_src, pitch, n_map, d_map, params, d_state, nullptr, nullptr, d_workspace, s);
    return st;
}
