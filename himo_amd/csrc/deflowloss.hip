// deflowloss.hip -- the supervised loss on ground-truth flow ("DeFlow loss, v1", himo_amd/deflow_loss.py) and its gradient
// with respect to the estimated flow, for gfx950.
//
// PARITY UNPINNED: `deflowLoss` lives in the absent OpenSceneFlow submodule.  What follows is this build's own written rule,
// after the published DeFlow formulation (end-point error averaged inside three speed bands, the bands summed).  No claim
// about the reference's numbers.  The float64 statement of the rule is tests/deflowloss_ref.py.
//
// Per row i of pc0 (p = raw pc0 xyz, m = the same point in pc1's frame as the network saw it, gt = the dataset's flow with
// ego motion, est = the network's residual flow), all in IEEE double on the float32 inputs, every operation rounded on its
// own (-ffp-contract=off):
//   counted  <=>  (no pid or pid >= 0)  and  (no valid or valid != 0)  and  gt finite in all three components
//   g     = (p + gt) - m                                 the ground-truth residual in pc1's frame (= gt - pose_flow)
//   s     = sqrt((gx gx + gy gy) + gz gz)
//   band  = 0 when s < 0.4 dt | 1 when s <= 1.0 dt | 2 otherwise          (both products in double from (double)sensor_dt)
//   d     = est - g,   e = sqrt((dx dx + dy dy) + dz dz)
//   term_b = mean of e over the counted rows of band b (0 when the band is empty);   total = (term_0 + term_1) + term_2
//   d total / d est_i = (d_i / e_i) / count_band(i), computed in double and rounded once to float32; exactly 0 for an
//   uncounted row and for a counted row with e_i = 0.  A non-finite est in a counted row is NOT filtered: that row's gradient,
//   its band's term and the total come out non-finite (the trainer's non-finite watch exists for this); other rows' gradients
//   do not change.
//
// Three launches, no atomics, no host read-back, nothing kept between calls:
//   1. deflow_band_kernel   one row per lane, 256-thread blocks: band and e per row, the band byte stashed (3 = uncounted),
//                           per-block counts and sums of e per band through a wave64 shuffle butterfly and a fixed-order sum
//                           of the four waves' words in LDS
//   2. deflow_fold_kernel   ONE block: lane t adds the blocks t, t + 256, ... in that order, then the same block reduction:
//                           a fixed two-level tree of doubles (as loss_final_kernel of sslloss.hip) -> d_counts, d_loss
//   3. deflow_grad_kernel   reads the band byte and, for counted rows, the four input rows again; the counts come from device
//                           memory
// so loss and gradient are bit-identical from run to run.
//
// Traffic per row (pitch 3 / pitch 4 rows of pc0 and est): pass 1 reads 12|16 (pc0) + 12 (moved) + 12 (gt) + 12|16 (est) +
// 4 (pid) + 1 (valid) = 53..61 B and writes 1 B; pass 3 reads the byte and, for a counted row, the same four rows (48..56 B)
// and writes 12 B: 115..131 B per row in all, against 66 B per row more for the alternative of stashing d and e as doubles
// (33 B written and read back) -- and that form still needs the counts before it can divide.  Timing unmeasured.
#include "himo_common.h"
#include "blockops.h"
#include <math.h>

namespace himo {

constexpr int kDeflowThreads = 256;          // rows per block of the two row passes; also the fold kernel's width
constexpr int kDeflowUncounted = 3;

struct DeflowArgs {
    int64_t n;
    const float* pc0; int pc0_pitch;
    const float* moved;                      // [n][3]
    const float* gt;                         // [n][3]
    const float* est; int est_pitch;
    const int32_t* pid;                      // nullable
    const uint8_t* valid;                    // nullable
    double t0, t1;                           // 0.4 dt, 1.0 dt
    uint8_t* band;                           // [n]
    double* psum;                            // [blocks][3]
    int64_t* pcnt;                           // [blocks][3]
    int64_t n_blocks;
    double* loss;                            // [4]
    int64_t* counts;                         // [3]
    float* grad;                             // [n][3]
};

// g = (p + gt) - m of row i, and whether gt is finite
__device__ inline bool deflow_residual(const DeflowArgs& a, int64_t i, double (&g)[3]) {
    const float* p = a.pc0 + (size_t)i * a.pc0_pitch;
    const float* m = a.moved + (size_t)i * 3;
    const float* t = a.gt + (size_t)i * 3;
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float tc = t[c];
        finite = finite && isfinite(tc);
        g[c] = ((double)p[c] + (double)tc) - (double)m[c];
    }
    return finite;
}

// d = est - g of row i; returns e
__device__ inline double deflow_error(const DeflowArgs& a, int64_t i, const double (&g)[3], double (&d)[3]) {
    const float* f = a.est + (size_t)i * a.est_pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (double)f[c] - g[c];
    return sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// sums of v[0..2] and c[0..2] over the block, valid on thread 0: butterfly inside each wave (blockops.h), then
// ((w0 + w1) + w2) + w3
__device__ inline void deflow_block_sum(double (&v)[3], int64_t (&c)[3]) {
    __shared__ double s_v[3][kDeflowThreads / 64];
    __shared__ int64_t s_c[3][kDeflowThreads / 64];
#pragma unroll
    for (int k = 0; k < 3; ++k) wave_sum2(v[k], c[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_v[k][threadIdx.x >> 6] = v[k]; s_c[k][threadIdx.x >> 6] = c[k]; }
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = ((s_v[k][0] + s_v[k][1]) + s_v[k][2]) + s_v[k][3];
            c[k] = ((s_c[k][0] + s_c[k][1]) + s_c[k][2]) + s_c[k][3];
        }
}

__global__ __launch_bounds__(kDeflowThreads) void deflow_band_kernel(const DeflowArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kDeflowThreads + threadIdx.x;
    int band = kDeflowUncounted;
    double e = 0.0;
    if (i < a.n) {
        const bool kept = (!a.pid || a.pid[i] >= 0) && (!a.valid || a.valid[i] != 0);
        double g[3], d[3];
        const bool finite = deflow_residual(a, i, g);
        if (kept && finite) {
            const double s = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
            band = s < a.t0 ? 0 : (s <= a.t1 ? 1 : 2);
            e = deflow_error(a, i, g, d);
        }
        a.band[i] = (uint8_t)band;
    }
    double v[3];
    int64_t c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { v[k] = band == k ? e : 0.0; c[k] = band == k ? 1 : 0; }
    deflow_block_sum(v, c);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) { a.psum[(size_t)blockIdx.x * 3 + k] = v[k]; a.pcnt[(size_t)blockIdx.x * 3 + k] = c[k]; }
}

__global__ __launch_bounds__(kDeflowThreads) void deflow_fold_kernel(const DeflowArgs a) {
    double v[3] = {0.0, 0.0, 0.0};
    int64_t c[3] = {0, 0, 0};
    for (int64_t b = threadIdx.x; b < a.n_blocks; b += kDeflowThreads)
#pragma unroll
        for (int k = 0; k < 3; ++k) { v[k] += a.psum[(size_t)b * 3 + k]; c[k] += a.pcnt[(size_t)b * 3 + k]; }
    deflow_block_sum(v, c);
    if (threadIdx.x == 0) {
        double term[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a.counts[k] = c[k];
            term[k] = c[k] > 0 ? v[k] / (double)c[k] : 0.0;
            a.loss[k] = term[k];
        }
        a.loss[3] = (term[0] + term[1]) + term[2];
    }
}

__global__ __launch_bounds__(kDeflowThreads) void deflow_grad_kernel(const DeflowArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kDeflowThreads + threadIdx.x;
    if (i >= a.n) return;
    const int band = a.band[i];
    float out[3] = {0.f, 0.f, 0.f};
    if (band != kDeflowUncounted) {
        double g[3], d[3];
        deflow_residual(a, i, g);
        const double e = deflow_error(a, i, g, d);
        const double cnt = (double)a.counts[band];
        if (e != 0.0)                                            // (a NaN e goes through: the row's gradient is NaN)
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = (float)((d[c] / e) / cnt);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.grad[(size_t)i * 3 + c] = out[c];
}

struct DeflowLayout { size_t psum, pcnt, band, end; };

static DeflowLayout deflow_layout(int64_t n) {
    DeflowLayout L;
    const size_t N = (size_t)(n > 0 ? n : 1), blocks = (N + kDeflowThreads - 1) / kDeflowThreads;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += round_up(bytes, 16); return at; };
    L.psum = take(blocks * 3 * sizeof(double));
    L.pcnt = take(blocks * 3 * sizeof(int64_t));
    L.band = take(N);
    L.end = o;
    return L;
}

}  // namespace himo

using namespace himo;

extern "C" size_t himo_deflow_loss_workspace_bytes(int64_t n) {
    return deflow_layout(n).end;
}

extern "C" int himo_deflow_loss(int64_t n, const float* d_pc0, int pc0_pitch, const float* d_moved, const float* d_gt,
                                const float* d_est, int est_pitch, const int32_t* d_pid, const uint8_t* d_valid, float sensor_dt,
                                double* d_loss, int64_t* d_counts, float* d_grad, void* d_workspace, size_t workspace_bytes,
                                void* stream) {
    if (n < 0 || pc0_pitch < 3 || est_pitch < 3 || !d_loss || !d_counts) return HIMO_ERR_INVALID_ARGUMENT;
    if (!(sensor_dt > 0.f) || !isfinite(sensor_dt)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > (int64_t)0x7fffffff) return HIMO_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {
        HIMO_HIP(hipMemsetAsync(d_loss, 0, 4 * sizeof(double), s));
        HIMO_HIP(hipMemsetAsync(d_counts, 0, 3 * sizeof(int64_t), s));
        return HIMO_OK;
    }
    if (!d_pc0 || !d_moved || !d_gt || !d_est || !d_grad) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < himo_deflow_loss_workspace_bytes(n)) return HIMO_ERR_WORKSPACE;
    const DeflowLayout L = deflow_layout(n);
    char* ws = reinterpret_cast<char*>(d_workspace);
    DeflowArgs a{};
    a.n = n;
    a.pc0 = d_pc0; a.pc0_pitch = pc0_pitch; a.moved = d_moved; a.gt = d_gt; a.est = d_est; a.est_pitch = est_pitch;
    a.pid = d_pid; a.valid = d_valid;
    a.t0 = 0.4 * (double)sensor_dt;
    a.t1 = 1.0 * (double)sensor_dt;
    a.psum = reinterpret_cast<double*>(ws + L.psum);
    a.pcnt = reinterpret_cast<int64_t*>(ws + L.pcnt);
    a.band = reinterpret_cast<uint8_t*>(ws + L.band);
    a.n_blocks = (n + kDeflowThreads - 1) / kDeflowThreads;
    a.loss = d_loss; a.counts = d_counts; a.grad = d_grad;
    {
        ProfScope ps("deflow_loss_kernels", s);
        hipLaunchKernelGGL(deflow_band_kernel, dim3((unsigned)a.n_blocks), dim3(kDeflowThreads), 0, s, a);
        hipLaunchKernelGGL(deflow_fold_kernel, dim3(1), dim3(kDeflowThreads), 0, s, a);
        hipLaunchKernelGGL(deflow_grad_kernel, dim3((unsigned)a.n_blocks), dim3(kDeflowThreads), 0, s, a);
    }
    HIMO_LAUNCH_CHECK("deflow_loss_kernels");
    return HIMO_OK;
}
