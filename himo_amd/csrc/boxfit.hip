// boxfit.hip -- one oriented box per cluster by the search-based L-shape fit ("cluster boxes, v1"; the rule is the module docstring
// of himo_amd/box_fit.py) for gfx950.  PARITY UNPINNED: the reference has no such stage; this one is checked against the numpy
// restatement of the written rule (tests/boxfit_ref.py).  Timing on a synthetic sweep: profiles/box_fit.txt.
//
// The labelled rows arrive SORTED BY LABEL, as in rigidrefine.hip: cluster k (label k + 1) owns the sorted rows offsets[k] ..
// offsets[k + 1], and d_rows[i] is the sweep row behind sorted row i.  ONE launch per call, ONE 256-thread workgroup per cluster:
//   phase A  (rule A, B, F) every thread walks the cluster's sorted rows lo + t, lo + t + 256, ...: reads the row, decides USABLE,
//            quantises, and keeps (X, Y) -- or a mark for a row that is not usable -- in the workspace, 8 bytes a sorted row.  The
//            count, the four integer extremes and the two z extremes (as order-preserving keys) meet in LDS integer atomics: min,
//            max and add give the same bits in any order.  The float64 motion sums take a FIXED shape: thread-strided partials in
//            ascending row order, then the block tree of blockops.h -- the same bytes on every run, no floating-point atomics.
//   phase B  (rule C) ONE DIRECTION PER LANE: thread t owns direction t & 127 and the points of part t >> 7 (waves 0, 1 take the
//            even groups of four points, waves 2, 3 the odd ones).  The cluster's (X', Y') are staged in LDS in chunks of kBfChunk
//            points, one packed word each (X' | Y' << 14: both are below 2^14 under rule B), and every lane of a wave reads the SAME
//            16 bytes -- four points a broadcast read, no bank conflict, no cross-lane reduction at all: a lane's umin, umax, vmin,
//            vmax and its inlier count never leave its registers until the two parts are combined through LDS (one exchange a pass).
//            Two passes over the chunks: the extremes first, the inlier count against the final extremes second.  Operands fit the
//            24-bit multiply (|a|, |b| <= 2^12, X', Y' < 2^14); every u, v fits int32 (< 2^27).
//   phase D  wave 0 chooses k: the largest S, then the smallest A, then the lowest k, as three 64-bit wave maxima (blockops.h).
//   phase E  thread 0 evaluates the box in float64 and writes info[12] and box[10] with ordinary stores.
// Why this mapping.  K is at most 128 and a cluster has tens to thousands of points, so the K x n products are the work and every
// reduction of rule C runs along n.  Putting n on the lanes would need 5 K cross-lane reductions a cluster; putting K on the lanes
// needs none, and the points, which every direction reads alike, come from LDS at one read per four points a wave.  Two parts use the
// block's four waves when K > 64 and halve a large cluster's walk; with K = 90 the second wave of a part runs 26 of its 64 lanes.
// LDS: 4 KB chunk + 2.5 KB per-direction exchange (four extremes and a count for 128 directions) + 2 KB float64 tree + a few words:
// 8736 bytes a block, so LDS never limits residency.  A cluster above the chunk is staged in passes; `max_points` bounds the tail
// one large cluster can cause (a cluster above it is TOO_LARGE after phase A and costs one walk).  The direction table travels BY VALUE in the kernel arguments (int16
// pairs, 512 bytes): the host pointer is read before the call returns and nothing is copied to the device.
//
// Built with -ffp-contract=off: every float operation rounds on its own, as numpy does.  Only sqrt and division appear, both
// correctly rounded; the library calls no transcendental.
#include "himo_common.h"
#include "blockops.h"
#include <limits.h>
#include <math.h>

namespace himo {

constexpr int kBfThreads = 256;
constexpr int kBfDirLanes = 128;             // = HIMO_BOXFIT_MAX_DIRS: one direction per lane of a part
constexpr int kBfParts = kBfThreads / kBfDirLanes;
constexpr int kBfChunk = HIMO_BOXFIT_CHUNK;  // points staged in LDS at a time (a multiple of 4 * kBfParts)
constexpr unsigned kBfNone = 0xffffffffu;    // a staged word that is no point (X' | Y' << 14 stays below 2^28)
static_assert(kBfDirLanes == HIMO_BOXFIT_MAX_DIRS && kBfChunk % (4 * kBfParts) == 0 && kBfChunk % kBfThreads == 0, "boxfit tiling");

struct BfDirs { short ab[kBfDirLanes][2]; };

struct BfArgs {
    int64_t n;                       // rows of the sweep
    const float* pts;                // [n][pitch]
    int pitch;
    const int32_t* labels;           // [n]
    const int64_t* rows;             // [n_clustered] sweep row of every sorted row
    const int64_t* offsets;          // [C + 1]
    int64_t nc;                      // n_clustered: the kernel clamps the device offsets to it
    const float* motion;             // [n][3] or nullptr
    int K;
    float scale;
    int tol_q, min_points, max_points;
    int2* q;                         // [n_clustered] workspace: (X, Y) of a usable sorted row, X = INT_MIN otherwise
    int32_t* info;                   // [C][12]
    double* box;                     // [C][10]
};

__device__ inline bool bf_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

__global__ __launch_bounds__(kBfThreads) void bf_fit_kernel(BfArgs p, BfDirs dirs) {
    __shared__ __attribute__((aligned(16))) unsigned s_pts[kBfChunk];
    __shared__ int s_ext[4][kBfDirLanes];                                    // umin, umax, vmin, vmax of a direction
    __shared__ int s_cnt[kBfDirLanes];
    __shared__ double red[kBfThreads];
    __shared__ int s_n, s_mn, s_xmin, s_xmax, s_ymin, s_ymax;
    __shared__ unsigned s_zmin, s_zmax;
    const int t = (int)threadIdx.x, k = (int)blockIdx.x;
    int64_t lo = p.offsets[k], hi = p.offsets[k + 1];               // (validated on the host; the device copy is clamped all the same)
    lo = lo < 0 ? 0 : (lo > p.nc ? p.nc : lo);
    hi = hi < lo ? lo : (hi > p.nc ? p.nc : hi);

    if (t == 0) {
        s_n = 0; s_mn = 0;
        s_xmin = INT_MAX; s_xmax = INT_MIN; s_ymin = INT_MAX; s_ymax = INT_MIN;
        s_zmin = 0xffffffffu; s_zmax = 0u;
    }
    __syncthreads();

    // ---- phase A: rules A, B and F ----
    int n = 0, mn = 0, xmin = INT_MAX, xmax = INT_MIN, ymin = INT_MAX, ymax = INT_MIN;
    unsigned zmin = 0xffffffffu, zmax = 0u;
    double sm[3] = {0.0, 0.0, 0.0};
    for (int64_t i = lo + t; i < hi; i += kBfThreads) {
        const int64_t r = p.rows[i];
        int2 xy = make_int2(INT_MIN, 0);
        if (r >= 0 && r < p.n && p.labels[r] > 0) {
            const float* row = p.pts + r * p.pitch;
            const float x = row[0], y = row[1], z = row[2];
            const float fx = x * p.scale, fy = y * p.scale;
            if (bf_finite(x) && bf_finite(y) && bf_finite(z) && fabsf(fx) < 4194304.f && fabsf(fy) < 4194304.f) {
                xy.x = (int)floorf(fx);
                xy.y = (int)floorf(fy);
                ++n;
                xmin = min(xmin, xy.x); xmax = max(xmax, xy.x);
                ymin = min(ymin, xy.y); ymax = max(ymax, xy.y);
                const unsigned zk = float_to_key(z);
                zmin = min(zmin, zk); zmax = max(zmax, zk);
                if (p.motion) {
                    const float* m = p.motion + 3 * r;
                    const float m0 = m[0], m1 = m[1], m2 = m[2];
                    if (bf_finite(m0) && bf_finite(m1) && bf_finite(m2)) {
                        ++mn;
                        sm[0] = sm[0] + (double)m0; sm[1] = sm[1] + (double)m1; sm[2] = sm[2] + (double)m2;
                    }
                }
            }
        }
        p.q[i] = xy;
    }
    if (n) {
        atomicAdd(&s_n, n);
        atomicMin(&s_xmin, xmin); atomicMax(&s_xmax, xmax);
        atomicMin(&s_ymin, ymin); atomicMax(&s_ymax, ymax);
        atomicMin(&s_zmin, zmin); atomicMax(&s_zmax, zmax);
    }
    if (mn) atomicAdd(&s_mn, mn);
    double msum[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) msum[d] = group_sum<kBfThreads>(sm[d], red);          // (its barriers also publish the atomics and q)
    n = s_n; mn = s_mn;
    xmin = s_xmin; xmax = s_xmax; ymin = s_ymin; ymax = s_ymax;

    int state = HIMO_BOXFIT_FITTED;
    if (n < p.min_points) state = HIMO_BOXFIT_TOO_FEW;
    else if (n > p.max_points || xmax - xmin >= 16384 || ymax - ymin >= 16384) state = HIMO_BOXFIT_TOO_LARGE;
    int32_t* info = p.info + 12 * (size_t)k;
    double* box = p.box + 10 * (size_t)k;
    if (state != HIMO_BOXFIT_FITTED) {                          // (the whole block: no barrier follows)
        if (t < 12) info[t] = t == 0 ? state : (t == 1 ? n : 0);
        if (t < 10) box[t] = 0.0;
        return;
    }

    // ---- phase B: rule C, one direction per lane ----
    const int dl = t & (kBfDirLanes - 1), part = t / kBfDirLanes;
    const bool live = dl < p.K;
    const int a = live ? (int)dirs.ab[dl][0] : 1, b = live ? (int)dirs.ab[dl][1] : 0;
    const int tol = p.tol_q << 12;
    int umin = INT_MAX, umax = INT_MIN, vmin = INT_MAX, vmax = INT_MIN, cnt = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t base = lo; base < hi; base += kBfChunk) {
            __syncthreads();                                     // the previous chunk's readers are through
            for (int j = t; j < kBfChunk; j += kBfThreads) {
                unsigned w = kBfNone;
                if (base + j < hi) {
                    const int2 xy = p.q[base + j];
                    if (xy.x != INT_MIN) w = (unsigned)(xy.x - xmin) | ((unsigned)(xy.y - ymin) << 14);
                }
                s_pts[j] = w;
            }
            __syncthreads();
            const int64_t left = hi - base;
            const int groups = (int)((left < kBfChunk ? left : kBfChunk) + 3) / 4;
            for (int g = part; g < groups; g += kBfParts) {
                const uint4 four = *reinterpret_cast<const uint4*>(&s_pts[4 * g]);       // the same address in every lane: a broadcast
                const unsigned w4[4] = {four.x, four.y, four.z, four.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (w4[e] == kBfNone) continue;              // (wave-uniform)
                    const int X = (int)(w4[e] & 0x3fffu), Y = (int)(w4[e] >> 14);
                    const int u = __mul24(a, X) + __mul24(b, Y), v = __mul24(a, Y) - __mul24(b, X);
                    if (pass == 0) {
                        umin = min(umin, u); umax = max(umax, u);
                        vmin = min(vmin, v); vmax = max(vmax, v);
                    } else {
                        const int d = min(min(u - umin, umax - u), min(v - vmin, vmax - v));
                        cnt += d <= tol ? 1 : 0;
                    }
                }
            }
        }
        // the two parts of a direction meet: part 1 hands over, part 0 combines and hands back
        __syncthreads();
        if (part == 1) {
            if (pass == 0) { s_ext[0][dl] = umin; s_ext[1][dl] = umax; s_ext[2][dl] = vmin; s_ext[3][dl] = vmax; }
            else s_cnt[dl] = cnt;
        }
        __syncthreads();
        if (part == 0) {
            if (pass == 0) {
                umin = min(umin, s_ext[0][dl]); umax = max(umax, s_ext[1][dl]);
                vmin = min(vmin, s_ext[2][dl]); vmax = max(vmax, s_ext[3][dl]);
                s_ext[0][dl] = umin; s_ext[1][dl] = umax; s_ext[2][dl] = vmin; s_ext[3][dl] = vmax;
            } else {
                cnt += s_cnt[dl];
                s_cnt[dl] = cnt;
            }
        }
        __syncthreads();
        if (pass == 0) { umin = s_ext[0][dl]; umax = s_ext[1][dl]; vmin = s_ext[2][dl]; vmax = s_ext[3][dl]; }
    }

    // ---- phase D: the choice, by wave 0 (its lanes hold directions l and l + 64) ----
    if (t >= 64) return;
    unsigned long long bestS = 0ull, bestA = 0ull;
    int bestK = -1;
    for (int kk = t; kk < p.K; kk += 64) {
        const unsigned long long S = (unsigned long long)(unsigned)s_cnt[kk];
        const long long A = (long long)(s_ext[1][kk] - s_ext[0][kk]) * (long long)(s_ext[3][kk] - s_ext[2][kk]);
        const unsigned long long nA = ~(unsigned long long)A;                    // the smaller area is the larger key
        if (bestK < 0 || S > bestS || (S == bestS && nA > bestA)) { bestS = S; bestA = nA; bestK = kk; }
    }
    const unsigned long long topS = wave_max_u64(bestK >= 0 ? bestS : 0ull);
    const bool inS = bestK >= 0 && bestS == topS;
    const unsigned long long topA = wave_max_u64(inS ? bestA : 0ull);
    const bool inA = inS && bestA == topA;
    const int kc = (int)(0xffffffffu - (unsigned)wave_max_u64(inA ? (unsigned long long)(0xffffffffu - (unsigned)bestK) : 0ull));

    // ---- phase E: the box, float64, every operation on its own ----
    if (t != 0) return;
    const int ca = (int)dirs.ab[kc][0], cb = (int)dirs.ab[kc][1];
    const int cumin = s_ext[0][kc], cumax = s_ext[1][kc], cvmin = s_ext[2][kc], cvmax = s_ext[3][kc];
    const double scale = (double)p.scale;
    const double n2 = (double)(ca * ca + cb * cb), r = sqrt(n2);
    const double su = (double)(cumin + cumax) * 0.5, sv = (double)(cvmin + cvmax) * 0.5;
    const double px = ((double)ca * su - (double)cb * sv) / n2, py = ((double)cb * su + (double)ca * sv) / n2;
    const double fzmin = (double)key_to_float(s_zmin), fzmax = (double)key_to_float(s_zmax);
    info[0] = state; info[1] = n; info[2] = kc; info[3] = s_cnt[kc]; info[4] = xmin; info[5] = ymin;
    info[6] = cumin; info[7] = cumax; info[8] = cvmin; info[9] = cvmax; info[10] = mn; info[11] = 0;
    box[0] = (((double)xmin + px) + 0.5) / scale;
    box[1] = (((double)ymin + py) + 0.5) / scale;
    box[2] = (fzmin + fzmax) * 0.5;
    box[3] = (double)(cumax - cumin) / (r * scale);
    box[4] = (double)(cvmax - cvmin) / (r * scale);
    box[5] = fzmax - fzmin;
#pragma unroll
    for (int d = 0; d < 3; ++d) box[6 + d] = mn > 0 ? msum[d] / (double)mn : 0.0;
    box[9] = 0.0;
}

static bool bf_params_ok(const himo_boxfit_params* p) {
    if (!p) return false;
    if (!isfinite(p->scale) || !(p->scale > 0.f)) return false;
    return p->tol_q >= 0 && p->tol_q <= 1024 && p->min_points >= 1 && p->max_points >= p->min_points && p->max_points <= (1 << 20);
}

static bool bf_dirs_ok(const int32_t* h, int K) {
    if (!h || K < 1 || K > HIMO_BOXFIT_MAX_DIRS) return false;
    for (int k = 0; k < K; ++k) {
        const int32_t a = h[2 * k], b = h[2 * k + 1];
        if (a < -4096 || a > 4096 || b < -4096 || b > 4096 || (a == 0 && b == 0)) return false;
    }
    return true;
}

static bool bf_offsets_ok(int64_t n, int C, const int64_t* h) {
    if (h[0] != 0 || h[C] != n) return false;
    for (int k = 0; k < C; ++k)
        if (h[k] < 0 || h[k + 1] < h[k]) return false;
    return true;
}

static bool bf_misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_boxfit_workspace_bytes(int64_t n_clustered, int n_clusters, int n_dirs) {
    if (n_clustered < 0 || n_clustered > 0x7fffffffLL || n_clusters < 0 || n_dirs < 1 || n_dirs > HIMO_BOXFIT_MAX_DIRS) return 0;
    const size_t bytes = round_up((size_t)n_clustered * sizeof(int2), 256);
    return bytes > 256 ? bytes : 256;
}

extern "C" int himo_boxfit(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, int64_t n_clustered, const int64_t* d_rows,
                           int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets, const float* d_motion, const int32_t* h_dirs,
                           int n_dirs, const himo_boxfit_params* params, int32_t* d_info, double* d_box, void* d_workspace,
                           size_t workspace_bytes, void* stream) {
    if (n < 0 || n_clustered < 0 || n_clustered > n || n_clusters < 0 || pitch < 3) return HIMO_ERR_INVALID_ARGUMENT;
    if (!bf_params_ok(params) || !bf_dirs_ok(h_dirs, n_dirs)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n_clusters == 0) return n_clustered == 0 ? HIMO_OK : HIMO_ERR_INVALID_ARGUMENT;
    if (!h_offsets || !d_offsets || !bf_offsets_ok(n_clustered, n_clusters, h_offsets)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_info || !d_box || bf_misaligned(d_info, 4) || bf_misaligned(d_box, 8) || bf_misaligned(d_offsets, 8)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_clustered > 0 && (!d_pts || !d_labels || !d_rows)) return HIMO_ERR_INVALID_ARGUMENT;
    if (bf_misaligned(d_pts, 4) || bf_misaligned(d_labels, 4) || bf_misaligned(d_rows, 8) || bf_misaligned(d_motion, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < himo_boxfit_workspace_bytes(n_clustered, n_clusters, n_dirs))
        return HIMO_ERR_WORKSPACE;

    BfArgs p;
    p.n = n; p.pts = d_pts; p.pitch = pitch; p.labels = d_labels; p.rows = d_rows; p.offsets = d_offsets; p.nc = n_clustered; p.motion = d_motion;
    p.K = n_dirs; p.scale = params->scale; p.tol_q = params->tol_q; p.min_points = params->min_points; p.max_points = params->max_points;
    p.q = reinterpret_cast<int2*>(d_workspace); p.info = d_info; p.box = d_box;
    BfDirs dirs;
    for (int k = 0; k < kBfDirLanes; ++k) {
        dirs.ab[k][0] = k < n_dirs ? (short)h_dirs[2 * k] : (short)1;
        dirs.ab[k][1] = k < n_dirs ? (short)h_dirs[2 * k + 1] : (short)0;
    }
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("bf_fit_kernel", s);
        hipLaunchKernelGGL(bf_fit_kernel, dim3((unsigned)n_clusters), dim3(kBfThreads), 0, s, p, dirs);
    }
    HIMO_LAUNCH_CHECK("bf_fit_kernel");
    return HIMO_OK;
}
