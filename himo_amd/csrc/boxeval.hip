// boxeval.hip -- rotated BEV IoU of oriented boxes and their greedy matching per sweep ("box evaluation, v1"; the rule is the module
// docstring of himo_amd/eval_box.py) for gfx950.  PARITY UNPINNED: the reference has no such stage; this one is checked bit for bit
// against the pure-Python restatement of the written rule (tests/boxeval_ref.py).  Timing on synthetic sweeps: profiles/box_eval.txt.
//
// A batch of S sweeps arrives as two packed tables of rects (double [12] a box: four BEV corners, zlo, zhi, area, 0; the host makes
// them, the library calls no transcendental) with offsets per side, on the host (validation) and on the device.  TWO launches a call:
//   pair phase   be_pair_kernel, grid (column tiles, row groups, sweeps), 256 threads: ONE LANE PER PAIR (i of A, j of B).  The
//                block stages a tile of HIMO_BOXEVAL_TILE rects of B in LDS, one array per rect word (lane c reads word k of rect c
//                at s_b[k][c]: consecutive lanes, consecutive banks), keeps its rect of B in registers and walks kBeRows rows of A,
//                two at a time.  Rule B runs in registers: the polygon is two arrays of 8 doubles that are only ever indexed by
//                unrolled loop counters; "append a vertex" is a chain of selects on the running count, and the four clip passes
//                are four instantiations (4, 5, 6, 7 vertices in).  No scratch (the compiler's resource report is quoted in
//                profiles/box_eval.txt).  Most pairs leave at rule B2, the bounds test, which comes before everything else.
//                The candidate store is DENSE: M[row of A in the packed table][j], pitch = the largest Fb of the call, float64:
//                the BEV IoU where it is >= min_iou, else 0 -- (rows of A in the call) x (largest Fb) x 8 bytes, the whole workspace.
//   match phase  be_match_kernel, ONE 512-thread workgroup per sweep.  The greedy matching of rule D comes out of rounds of LOCALLY
//                DOMINANT pairs: a pair that is first in the rule's total order both in its row and in its column, among the rows and
//                columns still free, is in the greedy matching, and all such pairs of a round are kept at once.  A round: a wave per
//                free row whose best is unknown or was taken takes the row's best (greatest IoU, then lowest j) with the fixed-order
//                64-bit wave maxima of blockops.h -- an IoU is a non-negative double, which orders as its bit pattern; a thread per
//                free column walks its column in ascending i (greatest IoU, then lowest i: strict comparisons); a pair is kept iff
//                each names the other.  Every round with a candidate left keeps at least one pair (the first free pair of the total
//                order), so there are at most min(Fa, Fb) keeping rounds; the loop runs min(Fa, Fb) + 1 times at the most BY ITS
//                BOUND and leaves earlier when a round kept nothing.  Then a thread per row evaluates rules B and C again for its
//                kept pair (the same operations: the same bits) and writes match_a, iou_a; a thread per column writes match_b.
// himo_box_iou_pairs (rule G): one lane per listed pair, one launch.
// Nothing here depends on arrival order: no floating-point atomics, no atomics at all; two runs give the same bytes.  The device
// offsets are clamped to the host's totals and to the cap, so a device table that disagrees with the host's can make a wrong answer
// but no access outside the tables.
//
// Built with -ffp-contract=off: every float64 operation rounds on its own, as in the restatement.  Only + - * / and comparisons.
#include "himo_common.h"
#include "blockops.h"
#include <math.h>

namespace himo {

constexpr int kBeTile = HIMO_BOXEVAL_TILE;       // rects of B a pair block stages in LDS = columns of a block
constexpr int kBeRows = 16;                      // rows of A a pair block walks
constexpr int kBePairThreads = 256;
constexpr int kBeMatchThreads = 512;
constexpr int kBeMax = HIMO_BOXEVAL_MAX_BOXES;
constexpr int kBeListThreads = 256;
static_assert(kBePairThreads % kBeTile == 0 && kBeRows % (kBePairThreads / kBeTile) == 0 && kBeMatchThreads % 64 == 0, "boxeval tiling");

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

struct BeArgs {
    int S, sweep0;                   // sweeps of the call; the first sweep of this launch
    const double* ra; const int64_t* offa; int64_t na;       // rects of A [na][12], device offsets [S + 1], the host's total
    const double* rb; const int64_t* offb; int64_t nb;
    int pitch;                       // the largest Fb of the call: the row pitch of M
    double min_iou;
    double* M;                       // [na][pitch]
    int32_t* match_a; int32_t* match_b; double* iou_a;
};

// the rows and columns of sweep s, clamped to the tables and to the cap
__device__ inline void be_extent(const BeArgs& p, int s, int64_t& a0, int& Fa, int64_t& b0, int& Fb) {
    int64_t lo = p.offa[s], hi = p.offa[s + 1];
    lo = lo < 0 ? 0 : (lo > p.na ? p.na : lo);
    hi = hi < lo ? lo : (hi > p.na ? p.na : hi);
    a0 = lo; Fa = (int)(hi - lo < kBeMax ? hi - lo : kBeMax);
    lo = p.offb[s]; hi = p.offb[s + 1];
    lo = lo < 0 ? 0 : (lo > p.nb ? p.nb : lo);
    hi = hi < lo ? lo : (hi > p.nb ? p.nb : hi);
    b0 = lo; Fb = (int)(hi - lo < p.pitch ? hi - lo : p.pitch);
}

__device__ inline void be_load(const double* __restrict__ r, double (&v)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = r[k];
}

__global__ __launch_bounds__(kBePairThreads) void be_pair_kernel(BeArgs p) {
    __shared__ double s_b[12][kBeTile];
    const int t = (int)threadIdx.x, s = p.sweep0 + (int)blockIdx.z;
    int64_t a0, b0;
    int Fa, Fb;
    be_extent(p, s, a0, Fa, b0, Fb);
    const int j0 = (int)blockIdx.x * kBeTile, i0 = (int)blockIdx.y * kBeRows;
    if (j0 >= Fb || i0 >= Fa) return;                               // (the whole block)
    const int cols = Fb - j0 < kBeTile ? Fb - j0 : kBeTile;
    const double* src = p.rb + 12 * (b0 + j0);
    for (int e = t; e < 12 * cols; e += kBePairThreads) s_b[e % 12][e / 12] = src[e];
    __syncthreads();
    const int c = t % kBeTile, r = t / kBeTile;
    if (c >= cols) return;                                          // (no barrier follows)
    double B[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) B[k] = s_b[k][c];
    const bool validB = be_valid(B);
    const int i1 = i0 + kBeRows < Fa ? i0 + kBeRows : Fa;
    for (int i = i0 + r; i < i1; i += kBePairThreads / kBeTile) {
        double A[12];
        be_load(p.ra + 12 * (a0 + i), A);
        double iou, iou3;
        be_pair(A, B, validB && be_valid(A), iou, iou3);
        p.M[(size_t)(a0 + i) * (size_t)p.pitch + (size_t)(j0 + c)] = iou >= p.min_iou ? iou : 0.0;
    }
}

__global__ __launch_bounds__(kBeMatchThreads) void be_match_kernel(BeArgs p) {
    __shared__ int s_rb[kBeMax], s_cb[kBeMax], s_ma[kBeMax], s_mb[kBeMax];      // a row's best column, a column's best row, the matching
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, s = p.sweep0 + (int)blockIdx.x;
    int64_t a0, b0;
    int Fa, Fb;
    be_extent(p, s, a0, Fa, b0, Fb);
    if (Fa == 0 && Fb == 0) return;
    for (int i = t; i < kBeMax; i += kBeMatchThreads) { s_rb[i] = -2; s_cb[i] = -2; s_ma[i] = -1; s_mb[i] = -1; }      // -2: not looked at yet
    __syncthreads();
    const double* M = p.M + (size_t)a0 * (size_t)p.pitch;
    const int bound = (Fa < Fb ? Fa : Fb) + 1;
    for (int round = 0; round < bound; ++round) {
        // a wave per free row whose best is unknown or taken: the greatest key, then the lowest j
        for (int i = wave; i < Fa; i += kBeMatchThreads / 64) {
            const int had = s_rb[i];
            if (s_ma[i] >= 0 || had == -1 || (had >= 0 && s_mb[had] < 0)) continue;       // (wave-uniform)
            unsigned long long best = 0ull;
            int bj = 0x7fffffff;
            for (int j = lane; j < Fb; j += 64) {
                const unsigned long long k = s_mb[j] < 0 ? (unsigned long long)__double_as_longlong(M[(size_t)i * p.pitch + j]) : 0ull;
                if (k > best) { best = k; bj = j; }
            }
            const unsigned long long top = wave_max_u64(best);
            const unsigned long long low = wave_max_u64(top > 0ull && best == top ? (unsigned long long)(0xffffffffu - (unsigned)bj) : 0ull);
            if (lane == 0) s_rb[i] = top > 0ull ? (int)(0xffffffffu - (unsigned)low) : -1;
        }
        // a thread per free column whose best is unknown or taken: the greatest key, then the lowest i
        for (int j = t; j < Fb; j += kBeMatchThreads) {
            const int had = s_cb[j];
            if (s_mb[j] >= 0 || had == -1 || (had >= 0 && s_ma[had] < 0)) continue;
            unsigned long long best = 0ull;
            int bi = -1;
            for (int i = 0; i < Fa; ++i) {
                const unsigned long long k = s_ma[i] < 0 ? (unsigned long long)__double_as_longlong(M[(size_t)i * p.pitch + j]) : 0ull;
                if (k > best) { best = k; bi = i; }
            }
            s_cb[j] = bi;
        }
        __syncthreads();
        int kept = 0;
        for (int i = t; i < Fa; i += kBeMatchThreads) {
            const int j = s_rb[i];
            if (s_ma[i] < 0 && j >= 0 && s_cb[j] == i) { s_ma[i] = j; s_mb[j] = i; kept = 1; }      // (s_cb[j] == i names one row a column)
        }
        if (!__syncthreads_or(kept)) break;                         // (a barrier; the same answer in every thread)
    }
    // the kept pairs: rules B and C once more, the same operations as in the pair phase
    for (int i = t; i < Fa; i += kBeMatchThreads) {
        const int j = s_ma[i];
        double iou = 0.0, iou3 = 0.0;
        if (j >= 0) {
            double A[12], B[12];
            be_load(p.ra + 12 * (a0 + i), A);
            be_load(p.rb + 12 * (b0 + j), B);
            be_pair(A, B, be_valid(A) && be_valid(B), iou, iou3);
        }
        p.match_a[a0 + i] = j;
        p.iou_a[2 * (a0 + i)] = iou;
        p.iou_a[2 * (a0 + i) + 1] = iou3;
    }
    for (int j = t; j < Fb; j += kBeMatchThreads) p.match_b[b0 + j] = s_mb[j];
}

__global__ __launch_bounds__(kBeListThreads) void be_list_kernel(int64_t n, const double* __restrict__ ra, int64_t na, const double* __restrict__ rb,
                                                                 int64_t nb, const int64_t* __restrict__ pairs, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kBeListThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t ia = pairs[2 * e], ib = pairs[2 * e + 1];
    double iou = 0.0, iou3 = 0.0;
    if (ia >= 0 && ia < na && ib >= 0 && ib < nb) {
        double A[12], B[12];
        be_load(ra + 12 * ia, A);
        be_load(rb + 12 * ib, B);
        be_pair(A, B, be_valid(A) && be_valid(B), iou, iou3);
    }
    out[2 * e] = iou;
    out[2 * e + 1] = iou3;
}

// offsets [S + 1] that start at 0 and never decrease, no sweep above the cap: 0 ok, 1 malformed, 2 above the cap
static int be_offsets(int S, const int64_t* h, int64_t& total, int& most) {
    total = 0; most = 0;
    if (!h || h[0] != 0) return 1;
    for (int s = 0; s < S; ++s)
        if (h[s + 1] < h[s]) return 1;
    for (int s = 0; s < S; ++s) {
        const int64_t f = h[s + 1] - h[s];
        if (f > kBeMax) return 2;
        if ((int)f > most) most = (int)f;
    }
    total = h[S];
    return 0;
}

static bool be_misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_boxeval_workspace_bytes(int n_sweeps, const int64_t* h_off_a, const int64_t* h_off_b) {
    if (n_sweeps < 0) return 0;
    if (n_sweeps == 0) return 256;
    int64_t na, nb;
    int fa, fb;
    if (be_offsets(n_sweeps, h_off_a, na, fa) || be_offsets(n_sweeps, h_off_b, nb, fb)) return 0;
    const size_t bytes = round_up((size_t)na * (size_t)fb * sizeof(double), 256);
    return bytes > 256 ? bytes : 256;
}

extern "C" int himo_boxeval_match(int n_sweeps, const double* d_rect_a, const int64_t* h_off_a, const int64_t* d_off_a, const double* d_rect_b,
                                  const int64_t* h_off_b, const int64_t* d_off_b, const himo_boxeval_params* params, int32_t* d_match_a,
                                  int32_t* d_match_b, double* d_iou_a, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (n_sweeps < 0 || !params) return HIMO_ERR_INVALID_ARGUMENT;
    if (!isfinite(params->min_iou) || !(params->min_iou > 0.0) || !(params->min_iou <= 1.0)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_sweeps == 0) return HIMO_OK;
    int64_t na, nb;
    int fa, fb;
    const int sa = be_offsets(n_sweeps, h_off_a, na, fa), sb = be_offsets(n_sweeps, h_off_b, nb, fb);
    if (sa == 1 || sb == 1) return HIMO_ERR_INVALID_ARGUMENT;
    if (sa == 2 || sb == 2) return HIMO_ERR_UNSUPPORTED;
    if (na == 0 && nb == 0) return HIMO_OK;
    if (!d_off_a || !d_off_b || be_misaligned(d_off_a, 8) || be_misaligned(d_off_b, 8)) return HIMO_ERR_INVALID_ARGUMENT;
    if (na > 0 && (!d_rect_a || !d_match_a || !d_iou_a)) return HIMO_ERR_INVALID_ARGUMENT;
    if (nb > 0 && (!d_rect_b || !d_match_b)) return HIMO_ERR_INVALID_ARGUMENT;
    if (be_misaligned(d_rect_a, 8) || be_misaligned(d_rect_b, 8) || be_misaligned(d_match_a, 4) || be_misaligned(d_match_b, 4) ||
        be_misaligned(d_iou_a, 8))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < himo_boxeval_workspace_bytes(n_sweeps, h_off_a, h_off_b))
        return HIMO_ERR_WORKSPACE;

    BeArgs p;
    p.S = n_sweeps; p.sweep0 = 0;
    p.ra = d_rect_a; p.offa = d_off_a; p.na = na; p.rb = d_rect_b; p.offb = d_off_b; p.nb = nb;
    p.pitch = fb; p.min_iou = params->min_iou; p.M = reinterpret_cast<double*>(d_workspace);
    p.match_a = d_match_a; p.match_b = d_match_b; p.iou_a = d_iou_a;
    hipStream_t s = (hipStream_t)stream;
    constexpr int kSlab = 32768;                                    // sweeps a launch (the grid's third dimension holds 65535)
    if (fa > 0 && fb > 0) {
        ProfScope ps("be_pair_kernel", s);
        for (int s0 = 0; s0 < n_sweeps; s0 += kSlab) {
            p.sweep0 = s0;
            const int ns = n_sweeps - s0 < kSlab ? n_sweeps - s0 : kSlab;
            hipLaunchKernelGGL(be_pair_kernel, dim3((unsigned)((fb + kBeTile - 1) / kBeTile), (unsigned)((fa + kBeRows - 1) / kBeRows), (unsigned)ns),
                               dim3(kBePairThreads), 0, s, p);
        }
    }
    HIMO_LAUNCH_CHECK("be_pair_kernel");
    {
        ProfScope ps("be_match_kernel", s);
        p.sweep0 = 0;
        hipLaunchKernelGGL(be_match_kernel, dim3((unsigned)n_sweeps), dim3(kBeMatchThreads), 0, s, p);
    }
    HIMO_LAUNCH_CHECK("be_match_kernel");
    return HIMO_OK;
}

extern "C" int himo_box_iou_pairs(int64_t n_pairs, const double* d_rect_a, int64_t n_a, const double* d_rect_b, int64_t n_b, const int64_t* d_pairs,
                                  double* d_iou, void* stream) {
    if (n_pairs < 0 || n_a < 0 || n_b < 0) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_pairs > 0x7fffffffLL * (int64_t)kBeListThreads) return HIMO_ERR_UNSUPPORTED;
    if (n_pairs == 0) return HIMO_OK;
    if (!d_pairs || !d_iou || (n_a > 0 && !d_rect_a) || (n_b > 0 && !d_rect_b)) return HIMO_ERR_INVALID_ARGUMENT;
    if (be_misaligned(d_pairs, 8) || be_misaligned(d_iou, 8) || be_misaligned(d_rect_a, 8) || be_misaligned(d_rect_b, 8)) return HIMO_ERR_INVALID_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("be_list_kernel", s);
        hipLaunchKernelGGL(be_list_kernel, dim3((unsigned)((n_pairs + kBeListThreads - 1) / kBeListThreads)), dim3(kBeListThreads), 0, s, n_pairs,
                           d_rect_a, n_a, d_rect_b, n_b, d_pairs, d_iou);
    }
    HIMO_LAUNCH_CHECK("be_list_kernel");
    return HIMO_OK;
}
