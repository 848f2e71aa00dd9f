// xalign.hip -- cross-sensor alignment per cluster ("cross-sensor alignment, v1"; the rule is the module docstring of
// himo_amd/xalign.py) for gfx950.  PARITY UNPINNED: the reference has no such stage; this one is checked against the numpy restatement
// of the written rule (tests/xalign_ref.py).  Timing on synthetic sweeps: profiles/xalign.txt.
//
// The planar velocity of an object from the capture times inside ONE sweep: several sensors record the same vehicle at different
// instants, r_i = P + v tau_i, so the v that lays the sensors' copies on top of one another is the object's.  A vote over pairs of rows
// of different sensors starts it, a robust nearest-neighbour least-squares iteration refines it, the cross-sensor distance of
// eval_xsensor before and after decides whether it is kept.
//
// The labelled rows arrive SORTED BY LABEL, as in xsensor.hip, and rules A and B are xsensor.hip's own (xsensor_rows.h).  One clear of
// the count table and TWO launches a call, whatever the clusters:
//   count    (rules A, B) one lane per sorted row: stages the row as float4 (x, y, z, 1 << group as the bits of w; zeros when it is
//            not usable) and its capture time in the workspace; n_g meets in int32 atomics on the count table [C][8].
//   cluster  (rules B-F) one 256-thread workgroup per cluster runs the whole estimate, so a call of 300 clusters is one launch.
//            One LDS buffer of 60 KB serves two phases in turn: the vote table nb x nb int32 (121 x 121 = 58.6 KB at the defaults;
//            LDS integer atomics), then the tile of HIMO_XALIGN_CHUNK moved rows the nearest-neighbour passes stream the cluster
//            through, as xsensor.hip's search does.  A lane owns a query row; every lane reads the SAME tile address at a time, a
//            broadcast.  The nearest row with its tie rule is ONE 64-bit minimum of (bits of d2 << 32 | sorted row).  The sums of
//            rule D and E are int64: a butterfly per wave (blockops.h), one LDS integer atomic per wave, any order, the same bits.
//            Every lane then forms v_{k+1} from the same sums, so nothing is broadcast.  A cluster passes 2 + iterations times over
//            its n^2 pairs; the states that end early (most clusters of a sweep: TOO_FEW) leave at once.
//   apply    (rule G) himo_xalign_apply, one lane per row of a point buffer.
// No floating-point atomics anywhere; plain C++ and vector stores only.
//
// Built with -ffp-contract=off: every float operation rounds on its own, as numpy does; division and sqrt are correctly rounded.
#include "himo_common.h"
#include "blockops.h"
#include "rigid_math.h"
#include "xsensor_rows.h"
#include <limits.h>
#include <math.h>

namespace himo {

constexpr int kXaChunk = HIMO_XALIGN_CHUNK;
constexpr int kXaBuf = HIMO_XALIGN_TABLE_CELLS;      // int32 cells of the LDS buffer: the vote table, then the tile
constexpr double kXaUnitX = 16777216.0;             // 2^24: the unit of the score sums, eval_xsensor's
constexpr double kXaUnitS = 1099511627776.0;        // 2^40: the unit of rule D's sums
constexpr double kXaClipT = 1024.0;                 // a capture time is clipped here before its mean is taken
constexpr double kXaClipS = 256.0;                  // a term of rule D is clipped here: 256 * 2^40 * 2^14 rows = 2^62 fits
constexpr unsigned kXaNan = 0x7FC00000u;            // every NaN orders as this one: after +inf
static_assert(kXaChunk % kXsThreads == 0 && kXaChunk * 4 <= kXaBuf, "xalign tiling");

struct XaArgs {
    int64_t n;                       // rows of the point buffer
    const float* pts;                // [n][pitch]
    int pitch;
    const int32_t* labels;           // [n]
    const uint8_t* group;            // [n]
    const float* tau;                // [n]
    const int64_t* rows;             // [nc]
    const int64_t* offsets;          // [C + 1]
    int nc, C, nb;
    himo_xalign_params prm;
    float4* staged;                  // [nc] workspace
    float* stau;                     // [nc] workspace: the capture time per sorted row
    int32_t* cnt;                    // [C][8] workspace
    int32_t* info;                   // [C][8]
    float* v;                        // [C][4]
    long long* x;                    // [C][2]
};

// ---- count: rules A and B's counts ----
__global__ __launch_bounds__(kXsThreads) void xa_count_kernel(XaArgs p) {
    const int64_t i64 = (int64_t)blockIdx.x * kXsThreads + threadIdx.x;
    if (i64 >= p.nc) return;
    const int i = (int)i64;
    const float4 s = xs_stage_row(p.n, p.pts, p.pitch, p.labels, p.group, p.tau, p.rows, p.offsets, p.C, i, p.cnt);
    p.staged[i] = s;
    p.stau[i] = __float_as_int(s.w) ? p.tau[p.rows[i]] : 0.f;
}

// One pass of the cluster's rows over the cluster's rows at the velocity (vx, vy) (float32): per query the nearest moved row of
// another live group.  STEP: rule D's sums -> acc[0..3] = A, b_x, b_y, pairs.  Otherwise rule E's -> acc[0] = the sum of q(min(d, trunc)).
// Every thread of the block calls it; the sums are in acc[] (LDS) for every thread when it returns.
template <bool STEP>
__device__ inline void xa_pass(const XaArgs& p, int lo, int hi, int live, float vx, float vy, float4* tile, unsigned long long* acc) {
    const int t = (int)threadIdx.x;
    __syncthreads();                                                 // (the pass before this one has been read)
    if (t < 4) acc[t] = 0ull;
    const double trunc = (double)p.prm.trunc, s2 = (double)p.prm.sigma * (double)p.prm.sigma;
    long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int q0 = lo; q0 < hi; q0 += kXsThreads) {                   // (block-uniform)
        const int i = q0 + t;
        float4 me = make_float4(0.f, 0.f, 0.f, 0.f);
        float mt = 0.f;
        if (i < hi) { me = p.staged[i]; mt = p.stau[i]; }
        const int bit = __float_as_int(me.w);
        const int mask = (bit & live) ? (live & ~bit) : 0;           // (0: no query in this lane)
        const float qx = me.x - vx * mt, qy = me.y - vy * mt, qz = me.z;
        unsigned long long best = ~0ull;
        for (int t0 = lo; t0 < hi; t0 += kXaChunk) {
            __syncthreads();
            const int tcount = min(kXaChunk, hi - t0);
            for (int j = t; j < kXaChunk; j += kXsThreads) {
                float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j < tcount) {
                    c = p.staged[t0 + j];
                    const float ct = p.stau[t0 + j];
                    c.x = c.x - vx * ct; c.y = c.y - vy * ct;
                }
                tile[j] = c;
            }
            __syncthreads();
            if (mask) {
#pragma unroll 4
                for (int j = 0; j < tcount; ++j) {
                    const float4 c = tile[j];
                    const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const unsigned bits = d2 != d2 ? kXaNan : __float_as_uint(d2);
                    const unsigned long long key = ((unsigned long long)bits << 32) | (unsigned)(t0 + j);
                    const bool other = (mask & __float_as_int(c.w)) != 0;
                    best = (other && key < best) ? key : best;
                }
            }
        }
        if (mask) {
            const double d = sqrt((double)__uint_as_float((unsigned)(best >> 32)));
            if (STEP) {
                if (d <= trunc) {                                    // (a NaN is dropped)
                    const int j = (int)(unsigned)best;               // (in lo .. hi: a key that won came from the tile)
                    const float4 o = p.staged[j];
                    const double w0 = s2 / (s2 + d * d), w = w0 * w0;
                    const double dtau = (double)mt - (double)p.stau[j];
                    const double wd = w * dtau;
                    double e0 = wd * dtau, e1 = wd * ((double)me.x - (double)o.x), e2 = wd * ((double)me.y - (double)o.y);
                    e0 = e0 < -kXaClipS ? -kXaClipS : (e0 > kXaClipS ? kXaClipS : e0);
                    e1 = e1 < -kXaClipS ? -kXaClipS : (e1 > kXaClipS ? kXaClipS : e1);
                    e2 = e2 < -kXaClipS ? -kXaClipS : (e2 > kXaClipS ? kXaClipS : e2);
                    a0 += llrint(e0 * kXaUnitS); a1 += llrint(e1 * kXaUnitS); a2 += llrint(e2 * kXaUnitS); a3 += 1;
                }
            } else {
                a0 += llrint((d <= trunc ? d : trunc) * kXaUnitX);
            }
        }
    }
    a0 = wave_sum(a0);
    if (STEP) { a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3); }
    __syncthreads();                                                 // (acc was cleared; the last tile is read)
    if ((t & 63) == 0) {
        atomicAdd(&acc[0], (unsigned long long)a0);
        if (STEP) { atomicAdd(&acc[1], (unsigned long long)a1); atomicAdd(&acc[2], (unsigned long long)a2); atomicAdd(&acc[3], (unsigned long long)a3); }
    }
    __syncthreads();
}

// ---- cluster: rules B-F ----
__global__ __launch_bounds__(kXsThreads) void xa_cluster_kernel(XaArgs p) {
    __shared__ __attribute__((aligned(16))) int s_buf[kXaBuf];
    __shared__ unsigned long long s_red[kXsThreads];
    __shared__ unsigned long long s_time[kXsGroups];
    __shared__ unsigned long long s_acc[4];
    __shared__ int s_votes;
    const int t = (int)threadIdx.x, k = (int)blockIdx.x;
    const int32_t* cnt = p.cnt + kXsGroups * (size_t)k;
    int n, live;
    int state = xs_state(cnt, p.prm.min_group, p.prm.min_points, p.prm.max_points, n, live);      // (block-uniform, as all below)
    int rows = 0, votes = 0, flat = 0, used = 0, pairs = 0;
    long long x0 = 0, x1 = 0;
    double vx = 0.0, vy = 0.0, speed = 0.0;
    int lo = 0, hi = 0;
    if (state == HIMO_XSENSOR_SCORED) {
        state = HIMO_XALIGN_ALIGNED;
        xs_range(p.offsets, p.nc, k, lo, hi);
        // rule B: the mean capture time of every live group
        if (t < kXsGroups) s_time[t] = 0ull;
        if (t == 0) s_votes = 0;
        __syncthreads();
        for (int i = lo + t; i < hi; i += kXsThreads) {
            const int bit = __float_as_int(p.staged[i].w);
            if (!(bit & live)) continue;
            double c = (double)p.stau[i];
            c = c < -kXaClipT ? -kXaClipT : (c > kXaClipT ? kXaClipT : c);
            atomicAdd(&s_time[__ffs(bit) - 1], (unsigned long long)llrint(c * kXaUnitX));
        }
        __syncthreads();
        double tmin = INFINITY, tmax = -INFINITY;
#pragma unroll
        for (int g = 0; g < kXsGroups; ++g) {
            if (!(live >> g & 1)) continue;
            rows += cnt[g];
            const double tg = (double)(long long)s_time[g] / (kXaUnitX * (double)cnt[g]);
            tmin = tg < tmin ? tg : tmin; tmax = tg > tmax ? tg : tmax;
        }
        if (!(tmax - tmin >= (double)p.prm.tau_min)) state = HIMO_XALIGN_NO_BASELINE;
    } else {
        live = 0;
    }
    if (state == HIMO_XALIGN_ALIGNED) {
        // rule C: the vote
        const int nb = p.nb, cells = nb * nb;
        for (int b = t; b < cells; b += kXsThreads) s_buf[b] = 0;
        __syncthreads();
        const double bin = (double)p.prm.bin, mid = (double)nb * 0.5, side = (double)nb;
        int mine = 0;
        for (int q0 = lo; q0 < hi; q0 += kXsThreads) {
            const int i = q0 + t;
            float4 me = make_float4(0.f, 0.f, 0.f, 0.f);
            float mt = 0.f;
            if (i < hi) { me = p.staged[i]; mt = p.stau[i]; }
            const int bit = __float_as_int(me.w);
            const int above = (bit & live) ? (live & ~((bit << 1) - 1)) : 0;       // the live groups after this row's
            for (int j = lo; j < hi; ++j) {                          // (every lane reads the same row: a broadcast)
                const float4 c = p.staged[j];
                const float ct = p.stau[j];
                if (!(above & __float_as_int(c.w))) continue;
                if (!(fabsf(mt - ct) >= p.prm.tau_min) || !(fabsf(me.z - c.z) < p.prm.z_gate)) continue;
                const double dtau = (double)mt - (double)ct;
                const double fx = floor(((double)me.x - (double)c.x) / dtau / bin + mid);
                const double fy = floor(((double)me.y - (double)c.y) / dtau / bin + mid);
                if (fx >= 0.0 && fx < side && fy >= 0.0 && fy < side) {
                    atomicAdd(&s_buf[(int)fx * nb + (int)fy], 1);
                    mine += 1;
                }
            }
        }
        mine = wave_sum(mine);
        if ((t & 63) == 0 && mine) atomicAdd(&s_votes, mine);
        __syncthreads();
        votes = s_votes;
        unsigned long long key = 0ull;
        for (int b = t; b < cells; b += kXsThreads) {
            const int bx = b / nb, by = b - bx * nb;
            unsigned score = 0u;
            for (int ax = max(bx - 1, 0); ax <= min(bx + 1, nb - 1); ++ax)
                for (int ay = max(by - 1, 0); ay <= min(by + 1, nb - 1); ++ay) score += (unsigned)s_buf[ax * nb + ay];
            const unsigned long long mk = ((unsigned long long)score << 32) | (0xFFFFFFFFu - (unsigned)b);   // ties: the smallest b
            key = mk > key ? mk : key;
        }
        key = group_max_u64<kXsThreads>(key, s_red);
        if (votes == 0) {
            state = HIMO_XALIGN_NO_BASELINE;
        } else {
            flat = (int)(0xFFFFFFFFu - (unsigned)key);
            const int half = (nb - 1) / 2;
            vx = (double)(flat / nb - half) * bin;
            vy = (double)(flat % nb - half) * bin;
        }
    }
    if (state == HIMO_XALIGN_ALIGNED) {
        float4* tile = reinterpret_cast<float4*>(s_buf);
        // rule E at v = 0
        xa_pass<false>(p, lo, hi, live, 0.f, 0.f, tile, s_acc);
        x0 = (long long)s_acc[0];
        // rule D
        const double tol = (double)p.prm.tol;
        long long A = 0;
        for (int it = 0; it < p.prm.iters; ++it) {
            xa_pass<true>(p, lo, hi, live, (float)vx, (float)vy, tile, s_acc);
            A = (long long)s_acc[0];
            const long long bx = (long long)s_acc[1], by = (long long)s_acc[2];
            used = it + 1; pairs = (int)s_acc[3];
            if (A == 0) break;
            const double nx = (double)bx / (double)A, ny = (double)by / (double)A;
            const double dx = nx - vx, dy = ny - vy;
            vx = nx; vy = ny;
            if (sqrt(dx * dx + dy * dy) < tol) break;
        }
        if (A == 0) {
            state = HIMO_XALIGN_NO_BASELINE;
            x0 = 0;
        } else {
            // rules E and F at the final v
            xa_pass<false>(p, lo, hi, live, (float)vx, (float)vy, tile, s_acc);
            x1 = (long long)s_acc[0];
            speed = sqrt(vx * vx + vy * vy);
            if (speed > (double)p.prm.v_max || (double)x1 > (1.0 - (double)p.prm.min_gain) * (double)x0) state = HIMO_XALIGN_REJECTED;
            else if (speed < (double)p.prm.static_speed) state = HIMO_XALIGN_STATIC;
        }
    }
    const bool moving = state == HIMO_XALIGN_ALIGNED;
    if (t < 8) {
        const int f[8] = {state, n, live, rows, votes, flat, used, pairs};
        int out = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) out = t == e ? f[e] : out;
        p.info[8 * (size_t)k + t] = out;
    }
    if (t < 4) p.v[4 * (size_t)k + t] = !moving ? 0.f : (t == 0 ? (float)vx : (t == 1 ? (float)vy : (t == 2 ? 0.f : (float)speed)));
    if (t < 2) p.x[2 * (size_t)k + t] = t == 0 ? x0 : x1;
}

// ---- apply: rule G ----
struct XaApplyArgs {
    int64_t n;
    const float* pts; int pitch;
    const int32_t* labels;
    int C;
    const int32_t* info; const float* v;
    int n_sweeps;
    const int64_t* pt_off; const float* E;
    const uint32_t* base;            // [n][3] or nullptr: the ego-motion flow itself
    float sensor_dt;
    uint32_t* out;
};

__global__ __launch_bounds__(kXsThreads) void xa_apply_kernel(XaApplyArgs p) {
    const int64_t i = (int64_t)blockIdx.x * kXsThreads + threadIdx.x;
    if (i >= p.n) return;
    const float* row = p.pts + i * p.pitch;
    const float x = row[0], y = row[1], z = row[2];
    const int lab = p.labels[i];
    const bool hit = lab >= 1 && lab <= p.C && xs_finite(x) && xs_finite(y) && xs_finite(z) && p.info[8 * (size_t)(lab - 1)] == HIMO_XALIGN_ALIGNED;
    uint32_t o[3];
    if (p.base && !hit) {
#pragma unroll
        for (int e = 0; e < 3; ++e) o[e] = p.base[3 * i + e];
    } else {
        float a[3];
        rigid_apply(p.E + 12 * (size_t)segment_of(p.pt_off, p.n_sweeps, i), x, y, z, a);
        float f[3] = {a[0] - x, a[1] - y, a[2] - z};
        if (hit) {
            const float* v = p.v + 4 * (size_t)(lab - 1);
#pragma unroll
            for (int e = 0; e < 3; ++e) f[e] = f[e] + v[e] * p.sensor_dt;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) o[e] = __float_as_uint(f[e]);
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) p.out[3 * i + e] = o[e];
}

// the side of the vote table, or 0 where it is refused
static int xa_table_side(float v_max, float bin) {
    if (!isfinite(v_max) || !(v_max > 0.f) || !isfinite(bin) || !(bin > 0.f)) return 0;
    const double half = ceil((double)v_max / (double)bin);
    if (!(half >= 1.0) || half > 4096.0) return 0;
    const int nb = 2 * (int)half + 1;
    return (int64_t)nb * nb <= kXaBuf ? nb : 0;
}

static bool xa_in(float v, float lo, float hi) { return isfinite(v) && v >= lo && v <= hi; }

static bool xa_params_ok(const himo_xalign_params* p) {
    if (!p) return false;
    if (!(p->min_group >= 1 && p->min_points >= 2 && p->max_points >= p->min_points && p->max_points <= HIMO_XALIGN_MAX_POINTS)) return false;
    if (!xa_in(p->v_max, 0.f, 1024.f) || !xa_table_side(p->v_max, p->bin)) return false;
    if (!xa_in(p->tau_min, 0.f, 1024.f) || !(p->tau_min > 0.f) || !xa_in(p->z_gate, 0.f, 3.0e38f) || !(p->z_gate > 0.f)) return false;
    if (!xa_in(p->sigma, 0.f, 1024.f) || !(p->sigma > 0.f) || !xa_in(p->trunc, 0.f, 1024.f) || !(p->trunc > 0.f)) return false;
    // one workgroup walks (iters + 2) max_points^2 pairs at the most: the product is bounded so that no launch runs for minutes
    if (p->iters < 1 || p->iters > HIMO_XALIGN_MAX_ITERS || (int64_t)p->iters * p->max_points * p->max_points > HIMO_XALIGN_MAX_WORK) return false;
    if (!xa_in(p->tol, 0.f, 3.0e38f)) return false;
    return xa_in(p->min_gain, 0.f, 1.f) && p->min_gain < 1.f && xa_in(p->static_speed, 0.f, 3.0e38f);
}

// the workspace: staged float4 [nc] | tau float [nc] | cnt int32 [C][8], each part rounded up to 256 bytes
static size_t xa_part_staged(int64_t nc) { return round_up((size_t)(nc > 0 ? nc : 1) * sizeof(float4), 256); }
static size_t xa_part_tau(int64_t nc) { return round_up((size_t)(nc > 0 ? nc : 1) * sizeof(float), 256); }
static size_t xa_part_cnt(int C) { return round_up((size_t)(C > 0 ? C : 1) * kXsGroups * sizeof(int32_t), 256); }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_xalign_workspace_bytes(int64_t n_clustered, int n_clusters) {
    if (n_clustered < 0 || n_clustered > 0x7fffffffLL || n_clusters < 0) return 0;
    return xa_part_staged(n_clustered) + xa_part_tau(n_clustered) + xa_part_cnt(n_clusters);
}

extern "C" int himo_xalign(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, const uint8_t* d_group, const float* d_tau,
                           int64_t n_clustered, const int64_t* d_rows, int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets,
                           const himo_xalign_params* params, int32_t* d_info, float* d_v, int64_t* d_x, void* d_workspace,
                           size_t workspace_bytes, void* stream) {
    if (n < 0 || n_clustered < 0 || n_clustered > n || n_clusters < 0 || pitch < 3) return HIMO_ERR_INVALID_ARGUMENT;
    if (!xa_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n_clusters == 0) return n_clustered == 0 ? HIMO_OK : HIMO_ERR_INVALID_ARGUMENT;
    if (!h_offsets || !d_offsets || !xs_offsets_ok(n_clustered, n_clusters, h_offsets)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_info || !d_v || !d_x || xs_misaligned(d_info, 4) || xs_misaligned(d_v, 4) || xs_misaligned(d_x, 8) || xs_misaligned(d_offsets, 8))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (n_clustered > 0 && (!d_pts || !d_labels || !d_group || !d_rows || !d_tau)) return HIMO_ERR_INVALID_ARGUMENT;
    if (xs_misaligned(d_pts, 4) || xs_misaligned(d_labels, 4) || xs_misaligned(d_rows, 8) || xs_misaligned(d_tau, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < himo_xalign_workspace_bytes(n_clustered, n_clusters)) return HIMO_ERR_WORKSPACE;

    char* ws = reinterpret_cast<char*>(d_workspace);
    XaArgs p;
    p.n = n; p.pts = d_pts; p.pitch = pitch; p.labels = d_labels; p.group = d_group; p.tau = d_tau; p.rows = d_rows;
    p.offsets = d_offsets; p.nc = (int)n_clustered; p.C = n_clusters;
    p.prm = *params; p.nb = xa_table_side(params->v_max, params->bin);
    p.staged = reinterpret_cast<float4*>(ws);
    p.stau = reinterpret_cast<float*>(ws + xa_part_staged(n_clustered));
    p.cnt = reinterpret_cast<int32_t*>(ws + xa_part_staged(n_clustered) + xa_part_tau(n_clustered));
    p.info = d_info; p.v = d_v; p.x = reinterpret_cast<long long*>(d_x);

    hipStream_t s = (hipStream_t)stream;
    HIMO_HIP(hipMemsetAsync(p.cnt, 0, (size_t)n_clusters * kXsGroups * sizeof(int32_t), s));
    const unsigned row_blocks = (unsigned)((n_clustered + kXsThreads - 1) / kXsThreads);
    if (row_blocks) {
        {
            ProfScope ps("xa_count_kernel", s);
            hipLaunchKernelGGL(xa_count_kernel, dim3(row_blocks), dim3(kXsThreads), 0, s, p);
        }
        HIMO_LAUNCH_CHECK("xa_count_kernel");
    }
    {
        ProfScope ps("xa_cluster_kernel", s);
        hipLaunchKernelGGL(xa_cluster_kernel, dim3((unsigned)n_clusters), dim3(kXsThreads), 0, s, p);
    }
    HIMO_LAUNCH_CHECK("xa_cluster_kernel");
    return HIMO_OK;
}

extern "C" int himo_xalign_apply(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, int n_clusters, const int32_t* d_info,
                                 const float* d_v, int n_sweeps, const int64_t* h_pt_off, const int64_t* d_pt_off, const float* d_E,
                                 const float* d_base, float sensor_dt, float* d_out, void* stream) {
    if (n < 0 || pitch < 3 || n_clusters < 0 || n_sweeps < 0 || !isfinite(sensor_dt) || !(sensor_dt > 0.f)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL * (int64_t)kXsThreads) return HIMO_ERR_UNSUPPORTED;
    if (n == 0) return HIMO_OK;
    if (n_sweeps == 0 || !h_pt_off || !d_pt_off || !d_E || !xs_offsets_ok(n, n_sweeps, h_pt_off)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_pts || !d_labels || !d_out || (n_clusters > 0 && (!d_info || !d_v))) return HIMO_ERR_INVALID_ARGUMENT;
    if (xs_misaligned(d_pts, 4) || xs_misaligned(d_labels, 4) || xs_misaligned(d_out, 4) || xs_misaligned(d_info, 4) || xs_misaligned(d_v, 4) ||
        xs_misaligned(d_pt_off, 8) || xs_misaligned(d_E, 4) || xs_misaligned(d_base, 4))
        return HIMO_ERR_INVALID_ARGUMENT;
    XaApplyArgs p;
    p.n = n; p.pts = d_pts; p.pitch = pitch; p.labels = d_labels; p.C = n_clusters; p.info = d_info; p.v = d_v;
    p.n_sweeps = n_sweeps; p.pt_off = d_pt_off; p.E = d_E;
    p.base = reinterpret_cast<const uint32_t*>(d_base); p.sensor_dt = sensor_dt; p.out = reinterpret_cast<uint32_t*>(d_out);
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("xa_apply_kernel", s);
        hipLaunchKernelGGL(xa_apply_kernel, dim3((unsigned)((n + kXsThreads - 1) / kXsThreads)), dim3(kXsThreads), 0, s, p);
    }
    HIMO_LAUNCH_CHECK("xa_apply_kernel");
    return HIMO_OK;
}
