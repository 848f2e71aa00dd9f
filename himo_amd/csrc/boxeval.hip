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
// The device functions of rules A to D (be_valid, be_pair, be_match_rounds, ...) are in boxiou.h, which boxtrack.hip shares.
#include "himo_common.h"
#include "blockops.h"
#include "boxiou.h"
#include <math.h>

namespace himo {

constexpr int kBeTile = HIMO_BOXEVAL_TILE;       // rects of B a pair block stages in LDS = columns of a block
constexpr int kBeRows = 16;                      // rows of A a pair block walks
constexpr int kBePairThreads = 256;
constexpr int kBeMatchThreads = 512;
constexpr int kBeMax = HIMO_BOXEVAL_MAX_BOXES;
constexpr int kBeListThreads = 256;
static_assert(kBePairThreads % kBeTile == 0 && kBeRows % (kBePairThreads / kBeTile) == 0 && kBeMatchThreads % 64 == 0, "boxeval tiling");

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
    const int t = (int)threadIdx.x, s = p.sweep0 + (int)blockIdx.x;
    int64_t a0, b0;
    int Fa, Fb;
    be_extent(p, s, a0, Fa, b0, Fb);
    if (Fa == 0 && Fb == 0) return;
    for (int i = t; i < kBeMax; i += kBeMatchThreads) { s_rb[i] = -2; s_cb[i] = -2; s_ma[i] = -1; s_mb[i] = -1; }      // -2: not looked at yet
    __syncthreads();
    const double* M = p.M + (size_t)a0 * (size_t)p.pitch;
    be_match_rounds<kBeMatchThreads>(M, p.pitch, Fa, Fb, s_rb, s_cb, s_ma, s_mb);
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
