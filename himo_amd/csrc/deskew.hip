// deskew.hip -- ego-motion de-skew ("ego de-skew, v1"; the rule is the module docstring of himo_amd/deskew.py) for gfx950: every row of
// a ragged batch of sweeps is moved along its sweep's constant body twist from its own capture time to the sweep's reference time.
// PARITY UNPINNED: the reference has no such stage; this one is checked against the numpy restatement of the written rule
// (tests/deskew_ref.py).
//
//   deskew_tref_kernel   one block per sweep: the greatest (least) finite lidar_dt of the sweep as the maximum of integer keys
//                        (float_to_key orders floats as unsigned integers; group_max_u64 of blockops.h); 0 for a sweep without a finite
//                        one and in mode "zero".
//   deskew_clear_kernel  zeroes the per-sweep counts and max_disp.
//   deskew_rows_kernel   a lane per row of the flat batch; its sweep by segment_of (blockops.h).  The row is read whole before anything
//                        is written, so input and output may be one buffer when the pitches are equal.  A pitch-3 row is three 4-byte
//                        loads a lane: a wave's three loads cover 768 contiguous bytes, so every fetched line is used whole; a pitch-4 row
//                        whose buffer is 16-byte aligned is ONE 16-byte load (store).  The move is float64, one sincos (of phi / 2) per
//                        moved row.  A wave whose lanes all belong to one sweep adds its counts and takes its maximum once (integer
//                        atomics after a wave reduction); a wave that straddles sweeps does so lane by lane.
// No floating-point atomics: integer sums and an integer max of non-negative float bits give the same bytes on every run.
//
// Built with -ffp-contract=off: every operation rounds on its own, as numpy does.  sin / cos of the scalar phi / 2 in float64 are the one
// transcendental pair (the rule's docstring says why); everything else is + - * / and sqrt.
#include "himo_common.h"
#include "blockops.h"
#include <math.h>

namespace himo {

constexpr int kDeskewThreads = 256;
constexpr int kDeskewTrefThreads = 1024;
constexpr double kDeskewSmallWW = 1e-16;      // w.w below this: the first-order form

__global__ __launch_bounds__(kDeskewTrefThreads) void deskew_tref_kernel(const int64_t* __restrict__ offsets, const float* __restrict__ dt,
                                                                          int mode, float* __restrict__ tref) {
    __shared__ unsigned long long red[kDeskewTrefThreads];
    const int b = blockIdx.x;
    // the least is the greatest of the inverted keys; the key of a finite float is neither 0 nor 0xffffffff, so 0 means "none"
    const bool want_max = mode == HIMO_DESKEW_REF_MAX;
    unsigned best = 0u;
    if (mode != HIMO_DESKEW_REF_ZERO) {
        const int64_t lo = offsets[b], hi = offsets[b + 1];
        for (int64_t i = lo + threadIdx.x; i < hi; i += kDeskewTrefThreads) {
            const float v = dt[i];
            if (isfinite(v)) {
                const unsigned k = want_max ? float_to_key(v) : ~float_to_key(v);
                best = k > best ? k : best;
            }
        }
    }
    const unsigned k = (unsigned)group_max_u64<kDeskewTrefThreads>(best, red);
    if (threadIdx.x == 0) tref[b] = k == 0u ? 0.0f : key_to_float(want_max ? k : ~k);
}

__global__ void deskew_clear_kernel(int n_sweeps, int32_t* __restrict__ counts, unsigned* __restrict__ max_disp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_sweeps) return;
    counts[2 * b] = 0;
    counts[2 * b + 1] = 0;
    max_disp[b] = 0u;
}

struct DeskewRowsArgs {
    int n_sweeps;
    int64_t n;
    const int64_t* offsets;
    const unsigned* pts;             // the rows as 32-bit words: a row that passes through keeps its bytes
    const float* dt;
    const double* twists;            // [n_sweeps][8]: v, w, span, spare
    const float* tref;
    int inverse;
    unsigned* out;
    int32_t* counts;                 // [n_sweeps][2]: moved, passed through
    unsigned* max_disp;              // [n_sweeps] float bits, non-negative
};

template <int PIN, int POUT, bool VEC>
__global__ __launch_bounds__(kDeskewThreads) void deskew_rows_kernel(DeskewRowsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kDeskewThreads + threadIdx.x;
    const bool live = i < a.n;
    int b = 0, moved = 0, passed = 0;
    unsigned disp_bits = 0u;
    if (live) {
        b = segment_of(a.offsets, a.n_sweeps, i);
        unsigned w0, w1, w2, w3 = 0u;
        if constexpr (PIN == 4 && VEC) {
            const uint4 r = reinterpret_cast<const uint4*>(a.pts)[i];
            w0 = r.x; w1 = r.y; w2 = r.z; w3 = r.w;
        } else {
            const unsigned* p = a.pts + i * PIN;
            w0 = p[0]; w1 = p[1]; w2 = p[2];
            if constexpr (PIN == 4) w3 = p[3];
        }
        const float px = __uint_as_float(w0), py = __uint_as_float(w1), pz = __uint_as_float(w2);
        const float dt = a.dt[i];
        const double* tw = a.twists + 8 * (int64_t)b;
        const double vx = tw[0], vy = tw[1], vz = tw[2], wx = tw[3], wy = tw[4], wz = tw[5], span = tw[6];
        const bool zero_twist = vx == 0.0 && vy == 0.0 && vz == 0.0 && wx == 0.0 && wy == 0.0 && wz == 0.0;
        const double s = ((double)a.tref[b] - (double)dt) / span;
        if (!(isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(dt)) || s == 0.0 || zero_twist) {
            passed = 1;
        } else {
            moved = 1;
            const double g = a.inverse ? s : -s;
            const double x = (double)px, y = (double)py, z = (double)pz;
            const double ww = (wx * wx + wy * wy) + wz * wz;
            double dx, dy, dz;
            if (ww < kDeskewSmallWW) {
                const double cx = wy * z - wz * y, cy = wz * x - wx * z, cz = wx * y - wy * x;
                dx = g * cx + g * vx; dy = g * cy + g * vy; dz = g * cz + g * vz;
            } else {
                const double theta = sqrt(ww);
                const double nx = wx / theta, ny = wy / theta, nz = wz / theta;
                const double Ax = ny * vz - nz * vy, Ay = nz * vx - nx * vz, Az = nx * vy - ny * vx;
                const double Bx = ny * Az - nz * Ay, By = nz * Ax - nx * Az, Bz = nx * Ay - ny * Ax;
                const double phi = g * theta;
                const double half = 0.5 * phi;
                const double sh = sin(half), ch = cos(half);
                const double sn = (2.0 * sh) * ch, k1 = (2.0 * sh) * sh;      // sin(phi), 1 - cos(phi) without the cancellation
                const double qx = ny * z - nz * y, qy = nz * x - nx * z, qz = nx * y - ny * x;         // n x p
                const double rx = ny * qz - nz * qy, ry = nz * qx - nx * qz, rz = nx * qy - ny * qx;   // n x (n x p)
                const double ca = k1 / theta, cb = (phi - sn) / theta;
                dx = (((sn * qx + k1 * rx) + g * vx) + ca * Ax) + cb * Bx;
                dy = (((sn * qy + k1 * ry) + g * vy) + ca * Ay) + cb * By;
                dz = (((sn * qz + k1 * rz) + g * vz) + ca * Az) + cb * Bz;
            }
            w0 = __float_as_uint((float)(x + dx));
            w1 = __float_as_uint((float)(y + dy));
            w2 = __float_as_uint((float)(z + dz));
            disp_bits = __float_as_uint((float)sqrt((dx * dx + dy * dy) + dz * dz));
        }
        if constexpr (POUT == 4 && VEC) {
            reinterpret_cast<uint4*>(a.out)[i] = make_uint4(w0, w1, w2, w3);
        } else {
            unsigned* q = a.out + i * POUT;
            q[0] = w0; q[1] = w1; q[2] = w2;
            if constexpr (POUT == 4) q[3] = w3;
        }
    }
    // the per-sweep outputs: once a wave where the wave is inside one sweep (dead lanes carry zeros and the first lane's sweep)
    const int b0 = __shfl(b, 0, 64);
    if (!live) b = b0;
    if (__all(b == b0)) {
        wave_sum2(moved, passed);
        const unsigned m = (unsigned)wave_max_u64(disp_bits);
        if ((threadIdx.x & 63) == 0 && (moved | passed)) {
            if (moved) atomicAdd(a.counts + 2 * b0, moved);
            if (passed) atomicAdd(a.counts + 2 * b0 + 1, passed);
            if (m) atomicMax(a.max_disp + b0, m);
        }
    } else if (live) {
        if (moved) atomicAdd(a.counts + 2 * b, 1);
        if (passed) atomicAdd(a.counts + 2 * b + 1, 1);
        if (disp_bits) atomicMax(a.max_disp + b, disp_bits);
    }
}

static bool deskew_misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

// offsets on the host: start at 0, never decrease, end at the row count
static bool deskew_offsets_ok(int n_sweeps, int64_t n, const int64_t* h_offsets) {
    if (!h_offsets || h_offsets[0] != 0) return false;
    for (int b = 0; b < n_sweeps; ++b)
        if (h_offsets[b + 1] < h_offsets[b]) return false;
    return h_offsets[n_sweeps] == n;
}

template <int PIN, int POUT>
static void deskew_launch(const DeskewRowsArgs& a, bool vec, unsigned blocks, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((deskew_rows_kernel<PIN, POUT, true>), dim3(blocks), dim3(kDeskewThreads), 0, s, a);
    else hipLaunchKernelGGL((deskew_rows_kernel<PIN, POUT, false>), dim3(blocks), dim3(kDeskewThreads), 0, s, a);
}

}  // namespace himo

using namespace himo;

extern "C" int himo_deskew_tref(int n_sweeps, int64_t n, const int64_t* h_offsets, const int64_t* d_offsets, const float* d_lidar_dt,
                                int mode, float* d_tref, void* stream) {
    if (n_sweeps < 0 || n < 0) return HIMO_ERR_INVALID_ARGUMENT;
    if (mode != HIMO_DESKEW_REF_MAX && mode != HIMO_DESKEW_REF_MIN && mode != HIMO_DESKEW_REF_ZERO) return HIMO_ERR_INVALID_ARGUMENT;
    if (!deskew_offsets_ok(n_sweeps, n, h_offsets)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (deskew_misaligned(d_offsets, 8) || deskew_misaligned(d_lidar_dt, 4) || deskew_misaligned(d_tref, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_sweeps == 0) return HIMO_OK;
    if (!d_offsets || !d_tref || (n > 0 && !d_lidar_dt)) return HIMO_ERR_INVALID_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("deskew_tref_kernel", s);
        hipLaunchKernelGGL(deskew_tref_kernel, dim3((unsigned)n_sweeps), dim3(kDeskewTrefThreads), 0, s, d_offsets, d_lidar_dt, mode, d_tref);
    }
    HIMO_LAUNCH_CHECK("deskew_tref_kernel");
    return HIMO_OK;
}

extern "C" int himo_deskew_rows(int n_sweeps, int64_t n, const int64_t* h_offsets, const int64_t* d_offsets, const float* d_pts, int in_pitch,
                                const float* d_lidar_dt, const double* h_twists, const double* d_twists, const float* d_tref, int inverse,
                                float* d_out, int out_pitch, int32_t* d_counts, float* d_max_disp, void* stream) {
    if (n_sweeps < 0 || n < 0) return HIMO_ERR_INVALID_ARGUMENT;
    if ((in_pitch != 3 && in_pitch != 4) || (out_pitch != 3 && out_pitch != 4) || (inverse != 0 && inverse != 1)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!deskew_offsets_ok(n_sweeps, n, h_offsets)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (deskew_misaligned(d_offsets, 8) || deskew_misaligned(d_pts, 4) || deskew_misaligned(d_lidar_dt, 4) || deskew_misaligned(h_twists, 8) ||
        deskew_misaligned(d_twists, 8) || deskew_misaligned(d_tref, 4) || deskew_misaligned(d_out, 4) || deskew_misaligned(d_counts, 4) ||
        deskew_misaligned(d_max_disp, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_sweeps == 0) return HIMO_OK;
    if (!d_offsets || !h_twists || !d_twists || !d_tref || !d_counts || !d_max_disp) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!d_pts || !d_lidar_dt || !d_out)) return HIMO_ERR_INVALID_ARGUMENT;
    for (int b = 0; b < n_sweeps; ++b) {
        const double* tw = h_twists + 8 * (size_t)b;
        for (int k = 0; k < 7; ++k)
            if (!isfinite(tw[k])) return HIMO_ERR_INVALID_ARGUMENT;
        if (!(tw[6] > 0.0)) return HIMO_ERR_INVALID_ARGUMENT;
    }
    if (n > 0) {
        // one buffer for both is the in-place run (equal pitches only); any other overlap would have rows read after they were written
        const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_pts), in1 = in0 + (uintptr_t)n * in_pitch * 4u;
        const uintptr_t out0 = reinterpret_cast<uintptr_t>(d_out), out1 = out0 + (uintptr_t)n * out_pitch * 4u;
        const bool overlap = in0 < out1 && out0 < in1;
        if (overlap && !(in0 == out0 && in_pitch == out_pitch)) return HIMO_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("deskew_clear_kernel", s);
        hipLaunchKernelGGL(deskew_clear_kernel, dim3((unsigned)((n_sweeps + 255) / 256)), dim3(256), 0, s, n_sweeps, d_counts,
                           reinterpret_cast<unsigned*>(d_max_disp));
    }
    HIMO_LAUNCH_CHECK("deskew_clear_kernel");
    if (n == 0) return HIMO_OK;
    DeskewRowsArgs a;
    a.n_sweeps = n_sweeps; a.n = n; a.offsets = d_offsets; a.pts = reinterpret_cast<const unsigned*>(d_pts); a.dt = d_lidar_dt;
    a.twists = d_twists; a.tref = d_tref; a.inverse = inverse; a.out = reinterpret_cast<unsigned*>(d_out); a.counts = d_counts;
    a.max_disp = reinterpret_cast<unsigned*>(d_max_disp);
    const unsigned blocks = (unsigned)((n + kDeskewThreads - 1) / kDeskewThreads);
    // the 16-byte row accesses need every pitch-4 buffer aligned to them; one flag covers both sides
    const bool vec = (in_pitch != 4 || aligned16(d_pts)) && (out_pitch != 4 || aligned16(d_out));
    {
        ProfScope ps("deskew_rows_kernel", s);
        if (in_pitch == 3 && out_pitch == 3) deskew_launch<3, 3>(a, false, blocks, s);
        else if (in_pitch == 3) deskew_launch<3, 4>(a, vec, blocks, s);
        else if (out_pitch == 3) deskew_launch<4, 3>(a, vec, blocks, s);
        else deskew_launch<4, 4>(a, vec, blocks, s);
    }
    HIMO_LAUNCH_CHECK("deskew_rows_kernel");
    return HIMO_OK;
}
