// boxiou.h -- the ONE statement of rules A (the library's side), B, C and D of "box evaluation, v1" (the module docstring of
// himo_amd/eval_box.py) as device code: the validity of a rect, the rotated BEV IoU and the 3-D IoU of a pair of rects, and the
// locally-dominant rounds that give the greedy matching.  boxeval.hip (box evaluation) and boxtrack.hip (box tracking) include it;
// both are built with -ffp-contract=off, so every float64 operation below rounds on its own in both, and a pair of rects gives the
// same bits in either.  Only + - * / and comparisons.  tests/test_box_eval_gpu.py compares every bit of what these functions give
// with tests/boxeval_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "blockops.h"

namespace himo {

__device__ inline bool be_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// rule A, the library's side: INVALID iff a value is not finite, the area is negative or zhi < zlo
__device__ inline bool be_valid(const double (&r)[12]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok && be_finite(r[k]);
    return ok && r[10] >= 0.0 && r[9] >= r[8];
}

// append (vx, vy) at position c of a polygon of at most NOUT vertices when `on` (rule B4: a vertex beyond NOUT is dropped): selects on
// the count, no runtime index
template <int NOUT> __device__ inline void be_emit(double (&ox)[8], double (&oy)[8], int& c, double vx, double vy, bool on) {
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        const bool here = on && c == k;
        ox[k] = here ? vx : ox[k];
        oy[k] = here ? vy : oy[k];
    }
    c += on && c < NOUT ? 1 : 0;
}

// rules B3, B4: one Sutherland-Hodgman pass of the polygon (x, y)[0 .. n), n <= NIN, against the edge (px, py) -> (qx, qy)
template <int NIN> __device__ inline void be_clip(double (&x)[8], double (&y)[8], int& n, double px, double py, double qx, double qy) {
    const double ex = qx - px, ey = qy - py;
    double d[NIN];
#pragma unroll
    for (int m = 0; m < NIN; ++m) d[m] = ex * (y[m] - py) - ey * (x[m] - px);
    double ox[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, oy[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int c = 0;
#pragma unroll
    for (int m = 0; m < NIN; ++m) {
        constexpr int kNone = 0;
        const int nx = m + 1 < NIN ? m + 1 : kNone;                 // (a constant once unrolled)
        const bool on = m < n, wrap = m + 1 >= n || m + 1 >= NIN;
        const double sx = x[m], sy = y[m], ds = d[m];
        const double tx = wrap ? x[0] : x[nx], ty = wrap ? y[0] : y[nx], de = wrap ? d[0] : d[nx];
        const bool is = ds >= 0.0, ie = de >= 0.0;
        be_emit<NIN + 1>(ox, oy, c, sx, sy, on && is);
        const bool cross = on && is != ie;
        double cx = 0.0, cy = 0.0;
        if (cross) {
            const double t = ds / (ds - de);
            cx = sx + t * (tx - sx);
            cy = sy + t * (ty - sy);
        }
        be_emit<NIN + 1>(ox, oy, c, cx, cy, cross);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { x[k] = ox[k]; y[k] = oy[k]; }
    n = c;
}

// rules B and C for one pair: A the subject, B the clip polygon
__device__ inline void be_pair(const double (&A)[12], const double (&B)[12], bool valid, double& iou, double& iou3) {
    iou = 0.0; iou3 = 0.0;
    if (!valid) return;
    // B1: everything relative to A's corner 0
    const double ox = A[0], oy = A[1];
    double x[8], y[8], qx[4], qy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        x[k] = A[2 * k] - ox; y[k] = A[2 * k + 1] - oy;
        qx[k] = B[2 * k] - ox; qy[k] = B[2 * k + 1] - oy;
        x[4 + k] = 0.0; y[4 + k] = 0.0;
    }
    // B2: the bounds, strictly disjoint in x or y
    double axl = x[0], axh = x[0], ayl = y[0], ayh = y[0], bxl = qx[0], bxh = qx[0], byl = qy[0], byh = qy[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        axl = x[k] < axl ? x[k] : axl; axh = x[k] > axh ? x[k] : axh;
        ayl = y[k] < ayl ? y[k] : ayl; ayh = y[k] > ayh ? y[k] : ayh;
        bxl = qx[k] < bxl ? qx[k] : bxl; bxh = qx[k] > bxh ? qx[k] : bxh;
        byl = qy[k] < byl ? qy[k] : byl; byh = qy[k] > byh ? qy[k] : byh;
    }
    if (axh < bxl || bxh < axl || ayh < byl || byh < ayl) return;
    // B3, B4: the four passes, in edge order
    int n = 4;
    be_clip<4>(x, y, n, qx[0], qy[0], qx[1], qy[1]);
    be_clip<5>(x, y, n, qx[1], qy[1], qx[2], qy[2]);
    be_clip<6>(x, y, n, qx[2], qy[2], qx[3], qy[3]);
    be_clip<7>(x, y, n, qx[3], qy[3], qx[0], qy[0]);
    // B5, B6
    if (n < 3) return;
    double acc = 0.0;
#pragma unroll
    for (int m = 1; m < 7; ++m)
        if (m + 1 < n) acc = acc + ((x[m] - x[0]) * (y[m + 1] - y[0]) - (x[m + 1] - x[0]) * (y[m] - y[0]));
    double inter = 0.5 * acc;
    const double aa = A[10], ab = B[10];
    const double lim = aa < ab ? aa : ab;
    if (!(inter >= 0.0)) inter = 0.0;
    if (inter > lim) inter = lim;
    // C
    const double uni = (aa + ab) - inter;
    iou = uni > 0.0 ? inter / uni : 0.0;
    const double top = A[9] < B[9] ? A[9] : B[9], bot = A[8] > B[8] ? A[8] : B[8];
    const double dz = top - bot;
    const double hz = dz > 0.0 ? dz : 0.0;
    const double inter3 = inter * hz;
    const double den = (aa * (A[9] - A[8]) + ab * (B[9] - B[8])) - inter3;
    iou3 = den > 0.0 ? inter3 / den : 0.0;
}

__device__ inline void be_load(const double* __restrict__ r, double (&v)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = r[k];
}

// Rule D for one workgroup of NT threads (a multiple of 64): the greedy matching of the Fa x Fb candidate matrix M (row pitch `pitch`;
// the BEV IoU where it is a candidate, else 0) out of rounds of LOCALLY DOMINANT pairs: a pair that is first in the rule's total order
// both in its row and in its column, among the rows and columns still free, is in the greedy matching, and all such pairs of a round
// are kept at once.  A round: a wave per free row whose best is unknown or was taken takes the row's best (greatest IoU, then lowest
// j) with the fixed-order 64-bit wave maxima of blockops.h -- an IoU is a non-negative double, which orders as its bit pattern; a
// thread per free column walks its column in ascending i (greatest IoU, then lowest i: strict comparisons); a pair is kept iff each
// names the other.  Every round with a candidate left keeps at least one pair, so there are at most min(Fa, Fb) keeping rounds; the loop
// runs min(Fa, Fb) + 1 times at the most BY ITS BOUND and leaves earlier when a round kept nothing.
// The caller has set s_rb[i] = s_cb[j] = -2 (not looked at yet) and s_ma[i] = s_mb[j] = -1 for i < Fa, j < Fb, behind a barrier, and M
// is visible to the workgroup.  EVERY thread of the workgroup calls this with the SAME Fa, Fb (there are barriers inside).  Ends on a
// barrier: s_ma (the j of row i or -1) and s_mb (the i of column j or -1) may be read by any thread afterwards.
template <int NT> __device__ inline void be_match_rounds(const double* __restrict__ M, int pitch, int Fa, int Fb, int* s_rb, int* s_cb, int* s_ma,
                                                         int* s_mb) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int bound = (Fa < Fb ? Fa : Fb) + 1;
    for (int round = 0; round < bound; ++round) {
        // a wave per free row whose best is unknown or taken: the greatest key, then the lowest j
        for (int i = wave; i < Fa; i += NT / 64) {
            const int had = s_rb[i];
            if (s_ma[i] >= 0 || had == -1 || (had >= 0 && s_mb[had] < 0)) continue;       // (wave-uniform)
            unsigned long long best = 0ull;
            int bj = 0x7fffffff;
            for (int j = lane; j < Fb; j += 64) {
                const unsigned long long k = s_mb[j] < 0 ? (unsigned long long)__double_as_longlong(M[(size_t)i * pitch + j]) : 0ull;
                if (k > best) { best = k; bj = j; }
            }
            const unsigned long long top = wave_max_u64(best);
            const unsigned long long low = wave_max_u64(top > 0ull && best == top ? (unsigned long long)(0xffffffffu - (unsigned)bj) : 0ull);
            if (lane == 0) s_rb[i] = top > 0ull ? (int)(0xffffffffu - (unsigned)low) : -1;
        }
        // a thread per free column whose best is unknown or taken: the greatest key, then the lowest i
        for (int j = t; j < Fb; j += NT) {
            const int had = s_cb[j];
            if (s_mb[j] >= 0 || had == -1 || (had >= 0 && s_ma[had] < 0)) continue;
            unsigned long long best = 0ull;
            int bi = -1;
            for (int i = 0; i < Fa; ++i) {
                const unsigned long long k = s_ma[i] < 0 ? (unsigned long long)__double_as_longlong(M[(size_t)i * pitch + j]) : 0ull;
                if (k > best) { best = k; bi = i; }
            }
            s_cb[j] = bi;
        }
        __syncthreads();
        int kept = 0;
        for (int i = t; i < Fa; i += NT) {
            const int j = s_rb[i];
            if (s_ma[i] < 0 && j >= 0 && s_cb[j] == i) { s_ma[i] = j; s_mb[j] = i; kept = 1; }      // (s_cb[j] == i names one row a column)
        }
        if (!__syncthreads_or(kept)) break;                         // (a barrier; the same answer in every thread)
    }
}

}  // namespace himo
