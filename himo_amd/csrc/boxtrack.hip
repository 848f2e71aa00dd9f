// boxtrack.hip -- box identities over time ("box tracking, v1"; the rule is the module docstring of himo_amd/track.py) for gfx950.
// PARITY UNPINNED: the reference has no such stage; this one is checked bit for bit against the pure-Python restatement of the
// written rule (tests/boxtrack_ref.py).  Timing on synthetic scenes: profiles/box_track.txt.
//
// A batch of scenes arrives as one packed table of detection rows (double [12] a box: x, y, z, l, w, h, c, s, vx, vy, 0, 0 in the
// scene frame; the host makes them, the library calls no transcendental), offsets scenes -> sweeps and sweeps -> rows on the host
// (validation) and on the device, and the time step of every sweep.  ONE launch a call (one per kBtSlab scenes): bt_track_kernel, ONE
// 512-thread workgroup per scene, walks the scene's sweeps in order -- the dependence between sweeps is inherent; the parallelism is
// across scenes and inside a step.  A step:
//   predict   a thread per live track: px = x + vx dt, py likewise (rule C1), and the track's rect at (px, py) (rule C2); a thread per
//             detection: its validity and its rect, by the same device function.
//   pairs     one lane per (track, detection) pair, looping over tiles of 128 detections x 4 tracks: the tile's detection rects are
//             staged in LDS one array per rect word (as be_pair_kernel does), a lane keeps its detection's rect in registers and
//             walks the tracks.  Rules B and C of box evaluation v1 (boxiou.h: the bounds test B2 first).  Candidates go to the DENSE
//             float64 matrix M[track slot][j], pitch = the largest F of the call: the BEV IoU where it is >= min_iou, else 0.
//   match     the locally-dominant rounds of rule D (be_match_rounds of boxiou.h), bounded by min(T, F) + 1.
//   update    a thread per track: rule C5 for a matched track (the IoU of the kept pair is evaluated once more: the same operations,
//             the same bits) or C6; the survivors are compacted in slot order with block_inclusive_scan (blockops.h); a thread per
//             detection: rule C7 in ascending j with a second scan, ids from the scene's counter, up to max_tracks live tracks.
// WHERE THE STATE LIVES.  Everything of a scene that is indexed by track or detection and is float64 lives in the scene's slice of
// the WORKSPACE, not in LDS: M [max_tracks][pitch], the track rects [max_tracks][12], the sweep's detection rects [pitch][12], the
// track state x, y, z, l, w, h, c, s, vx, vy TWICE [2][max_tracks][10] (a step reads one copy and compacts into the other) and id,
// hits, misses int32 [2][max_tracks][3].  LDS holds the matching's four int tables, the detections' validity, the scan's buffer, the
// staged tile and the step's block-uniform scalars (24.3 KiB; the compiler's resource report is quoted in profiles/box_track.txt).
// BARRIERS.  Every barrier sits in block-uniform control flow: the scene's sweep range, F_k, dt_k and the live count T are written to
// LDS by thread 0 and read by all threads after a barrier; the survivor and birth counts are read from the scan's buffer after its
// last barrier; a round's "kept anything" comes out of __syncthreads_or.  What one phase writes to the workspace, other threads read
// only after a barrier.
// No atomics; nothing depends on arrival order; two runs give the same bytes.  The device offsets are clamped to the host's totals
// and to the cap, and every loop bound comes from the clamped values: a device table that disagrees with the host's can make a wrong
// answer but no access outside the tables and no unbounded loop.
//
// Built with -ffp-contract=off: every float64 operation rounds on its own, as in the restatement.  Only + - * / and comparisons.
#include "himo_common.h"
#include "blockops.h"
#include "boxiou.h"
#include <math.h>

namespace himo {

constexpr int kBtThreads = 512;
constexpr int kBtMax = HIMO_BOXTRACK_MAX;        // live tracks of a scene, detections of a sweep
constexpr int kBtTile = 128;                     // detection rects a tile stages in LDS
constexpr int kBtSlab = 32768;                   // scenes a launch
static_assert(kBtMax <= kBtThreads && kBtThreads % kBtTile == 0 && kBtThreads % 64 == 0, "boxtrack tiling");

struct BtArgs {
    int scene0;                      // the first scene of this launch
    int64_t n_sweeps, n_rows;        // the host's totals
    const double* det; const int64_t* sweep_off; const int64_t* det_off; const double* dt;
    double min_iou, alpha, beta;
    int max_age, max_tracks, vel_mode;
    int pitch;                       // the largest F of the call (at least 1): the row pitch of M
    int32_t* track_id; int32_t* age; double* state; double* iou; int32_t* live; int32_t* scene_info;
    char* ws; size_t slice;          // a scene's slice of the workspace, bytes
};

// a scene's slice: M, the track rects, the detection rects, the state twice (doubles), then id, hits, misses twice (int32)
__host__ __device__ inline size_t bt_slice_doubles(int max_tracks, int pitch) {
    return (size_t)max_tracks * (size_t)pitch + 12u * (size_t)max_tracks + 12u * (size_t)pitch + 20u * (size_t)max_tracks;
}
static size_t bt_slice_bytes(int max_tracks, int pitch) {
    return round_up(bt_slice_doubles(max_tracks, pitch) * sizeof(double) + 6u * (size_t)max_tracks * sizeof(int32_t), 256);
}

// rule C2 = rule A of box evaluation v1 with c, s given: the four corners counter-clockwise from (+l/2, +w/2), zlo, zhi, area, 0
__device__ inline void bt_rect(double x, double y, double z, double l, double w, double h, double c, double s, double (&r)[12]) {
    const double hl = l * 0.5, hw = w * 0.5;
    const double dx[4] = {hl, -hl, -hl, hl}, dy[4] = {hw, hw, -hw, -hw};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r[2 * k] = x + (dx[k] * c - dy[k] * s);
        r[2 * k + 1] = y + (dx[k] * s + dy[k] * c);
    }
    r[8] = z - h * 0.5;
    r[9] = z + h * 0.5;
    r[10] = l * w;
    r[11] = 0.0;
}

__device__ inline int64_t bt_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kBtThreads) void bt_track_kernel(BtArgs p) {
    __shared__ double s_b[12][kBtTile];
    __shared__ int s_rb[kBtMax], s_cb[kBtMax], s_ma[kBtMax], s_mb[kBtMax];      // a row's best column, a column's best row, the matching
    __shared__ int s_dv[kBtMax], s_part[kBtThreads];                           // a detection is valid; the scans' buffer
    __shared__ long long s_k0, s_k1, s_d0;                                     // the scene's sweeps; the sweep's first row
    __shared__ int s_F, s_T, s_next, s_over;                                   // detections; live tracks; the next id; the overflow count
    __shared__ double s_dt;
    const int t = (int)threadIdx.x, scene = p.scene0 + (int)blockIdx.x, mt = p.max_tracks, pitch = p.pitch;
    double* const M = reinterpret_cast<double*>(p.ws + (size_t)blockIdx.x * p.slice + (size_t)p.scene0 * p.slice);
    double* const trect = M + (size_t)mt * (size_t)pitch;
    double* const drect = trect + 12 * (size_t)mt;
    double* const state = drect + 12 * (size_t)pitch;               // [2][mt][10]
    int32_t* const meta = reinterpret_cast<int32_t*>(state + 20 * (size_t)mt);      // [2][mt][3]

    if (t == 0) {
        const int64_t lo = bt_clamp(p.sweep_off[scene], 0, p.n_sweeps);
        s_k0 = lo;
        s_k1 = bt_clamp(p.sweep_off[scene + 1], lo, p.n_sweeps);
        s_T = 0; s_next = 0; s_over = 0;
    }
    __syncthreads();
    const int64_t k0 = s_k0, k1 = s_k1;                             // (block-uniform: read from LDS behind the barrier)
    int cur = 0;
    for (int64_t k = k0; k < k1; ++k) {
        if (t == 0) {
            const int64_t lo = bt_clamp(p.det_off[k], 0, p.n_rows), hi = bt_clamp(p.det_off[k + 1], lo, p.n_rows);
            s_d0 = lo;
            s_F = (int)(hi - lo < pitch ? hi - lo : pitch);
            s_dt = p.dt[k];
        }
        __syncthreads();
        const int T = s_T, F = s_F, next = s_next;                  // (block-uniform, as above)
        const int64_t d0 = s_d0;
        const double dt = s_dt;
        double* const st = state + (size_t)cur * 10 * (size_t)mt;
        double* const st2 = state + (size_t)(cur ^ 1) * 10 * (size_t)mt;
        int32_t* const me = meta + (size_t)cur * 3 * (size_t)mt;
        int32_t* const me2 = meta + (size_t)(cur ^ 1) * 3 * (size_t)mt;

        // C1, C2: predict; the rects of tracks and detections
        if (t < T) {
            double* q = st + 10 * t;
            const double px = q[0] + q[8] * dt, py = q[1] + q[9] * dt;
            q[0] = px; q[1] = py;
            double r[12];
            bt_rect(px, py, q[2], q[3], q[4], q[5], q[6], q[7], r);
#pragma unroll
            for (int e = 0; e < 12; ++e) trect[12 * t + e] = r[e];
        }
        if (t < F) {
            double v[12], r[12];
            be_load(p.det + 12 * (d0 + t), v);
            bool ok = true;
#pragma unroll
            for (int e = 0; e < 12; ++e) ok = ok && be_finite(v[e]);
            ok = ok && v[3] >= 0.0 && v[4] >= 0.0 && v[5] >= 0.0;
            bt_rect(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], r);
#pragma unroll
            for (int e = 0; e < 12; ++e) drect[12 * t + e] = ok ? r[e] : __longlong_as_double(0x7ff8000000000000LL);
            s_dv[t] = ok ? 1 : 0;
        }
        s_rb[t] = -2; s_cb[t] = -2; s_ma[t] = -1; s_mb[t] = -1;      // (kBtMax <= kBtThreads) -2: not looked at yet
        __syncthreads();

        // C3, C4: the candidate matrix, then the matching
        if (T > 0 && F > 0) {                                       // (block-uniform)
            for (int j0 = 0; j0 < F; j0 += kBtTile) {
                const int cols = F - j0 < kBtTile ? F - j0 : kBtTile;
                for (int e = t; e < 12 * cols; e += kBtThreads) s_b[e % 12][e / 12] = drect[12 * j0 + e];
                __syncthreads();
                const int c = t % kBtTile, r = t / kBtTile;
                if (c < cols) {
                    double B[12];
#pragma unroll
                    for (int e = 0; e < 12; ++e) B[e] = s_b[e][c];
                    const bool validB = be_valid(B);
                    for (int i = r; i < T; i += kBtThreads / kBtTile) {
                        double A[12];
                        be_load(trect + 12 * i, A);
                        double iou, iou3;
                        be_pair(A, B, validB && be_valid(A), iou, iou3);
                        M[(size_t)i * (size_t)pitch + (size_t)(j0 + c)] = iou >= p.min_iou ? iou : 0.0;
                    }
                }
                __syncthreads();
            }
            be_match_rounds<kBtThreads>(M, pitch, T, F, s_rb, s_cb, s_ma, s_mb);
        }

        // C5, C6: a thread per track; the survivors keep their order
        double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int id = 0, hits = 0, misses = 0, alive = 0;
        if (t < T) {
#pragma unroll
            for (int e = 0; e < 10; ++e) q[e] = st[10 * t + e];
            id = me[3 * t]; hits = me[3 * t + 1]; misses = me[3 * t + 2];
            const int j = s_ma[t];
            if (j >= 0) {
                double A[12], B[12], d[12], iou, iou3;
                be_load(trect + 12 * t, A);
                be_load(drect + 12 * j, B);
                be_pair(A, B, be_valid(A) && be_valid(B), iou, iou3);
                be_load(p.det + 12 * (d0 + j), d);
                const double rx = d[0] - q[0], ry = d[1] - q[1];
                if (p.vel_mode == 0) {
                    q[8] = q[8] + p.beta * (d[8] - q[8]);
                    q[9] = q[9] + p.beta * (d[9] - q[9]);
                } else {
                    q[8] = q[8] + p.beta * (rx / dt);
                    q[9] = q[9] + p.beta * (ry / dt);
                }
                q[0] = q[0] + p.alpha * rx;
                q[1] = q[1] + p.alpha * ry;
#pragma unroll
                for (int e = 2; e < 8; ++e) q[e] = d[e];
                hits += 1; misses = 0; alive = 1;
                const int64_t row = d0 + j;
                p.track_id[row] = id;
                p.age[row] = hits;
                p.state[4 * row] = q[0]; p.state[4 * row + 1] = q[1]; p.state[4 * row + 2] = q[8]; p.state[4 * row + 3] = q[9];
                p.iou[row] = iou;
            } else {
                misses += 1;
                alive = misses <= p.max_age ? 1 : 0;
            }
        }
        const int pos = block_inclusive_scan<kBtThreads>(alive, s_part);
        const int nS = s_part[kBtThreads - 1];                     // the survivors (block-uniform: read behind the scan's barrier)
        if (alive) {
#pragma unroll
            for (int e = 0; e < 10; ++e) st2[10 * (pos - 1) + e] = q[e];
            me2[3 * (pos - 1)] = id; me2[3 * (pos - 1) + 1] = hits; me2[3 * (pos - 1) + 2] = misses;
        }
        __syncthreads();                                            // (every thread has read s_part before the next scan writes it)

        // C7: a thread per detection; births in ascending j
        const bool loose = t < F && s_mb[t] < 0;
        const int born = loose && s_dv[t] ? 1 : 0;
        const int pos2 = block_inclusive_scan<kBtThreads>(born, s_part);
        const int nNew = s_part[kBtThreads - 1];
        const int nB = nNew < mt - nS ? nNew : mt - nS;             // the births the table has room for
        if (loose) {
            const int64_t row = d0 + t;
            if (born && pos2 - 1 < nB) {
                double d[12];
                be_load(p.det + 12 * row, d);
                const int slot = nS + pos2 - 1;
                const double vx = p.vel_mode == 0 ? d[8] : 0.0, vy = p.vel_mode == 0 ? d[9] : 0.0;
#pragma unroll
                for (int e = 0; e < 8; ++e) st2[10 * slot + e] = d[e];
                st2[10 * slot + 8] = vx; st2[10 * slot + 9] = vy;
                me2[3 * slot] = next + pos2 - 1; me2[3 * slot + 1] = 1; me2[3 * slot + 2] = 0;
                p.track_id[row] = next + pos2 - 1;
                p.age[row] = 1;
                p.state[4 * row] = d[0]; p.state[4 * row + 1] = d[1]; p.state[4 * row + 2] = vx; p.state[4 * row + 3] = vy;
            } else {
                p.track_id[row] = -1;
                p.age[row] = 0;
                p.state[4 * row] = 0.0; p.state[4 * row + 1] = 0.0; p.state[4 * row + 2] = 0.0; p.state[4 * row + 3] = 0.0;
            }
            p.iou[row] = 0.0;
        }
        // C8
        if (t == 0) {
            s_T = nS + nB;
            s_next = next + nB;
            s_over += nNew - nB;
            p.live[k] = nS + nB;
        }
        cur ^= 1;
    }
    if (t == 0) {                                                   // (thread 0 wrote both itself)
        p.scene_info[2 * scene] = s_next;
        p.scene_info[2 * scene + 1] = s_over;
    }
}

// offsets [n + 1] that start at 0 and never decrease: 0 ok, 1 malformed
static int bt_offsets(int64_t n, const int64_t* h) {
    if (!h || h[0] != 0) return 1;
    for (int64_t s = 0; s < n; ++s)
        if (h[s + 1] < h[s]) return 1;
    return 0;
}

static bool bt_misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

static bool bt_params_ok(const himo_boxtrack_params* q) {
    if (!q) return false;
    if (!isfinite(q->min_iou) || !(q->min_iou > 0.0) || !(q->min_iou <= 1.0)) return false;
    if (!isfinite(q->alpha) || !(q->alpha >= 0.0) || !(q->alpha <= 1.0)) return false;
    if (!isfinite(q->beta) || !(q->beta >= 0.0) || !(q->beta <= 1.0)) return false;
    return q->max_age >= 0 && q->max_age <= 255 && q->max_tracks >= 1 && q->max_tracks <= kBtMax && (q->vel_mode == 0 || q->vel_mode == 1);
}

// the host tables of a call: HIMO_OK and the totals, or the status that refuses them
static int bt_tables(int n_scenes, const int64_t* h_sweep_off, const int64_t* h_det_off, int64_t& n_sweeps, int64_t& n_rows, int& most) {
    n_sweeps = 0; n_rows = 0; most = 0;
    if (bt_offsets(n_scenes, h_sweep_off)) return HIMO_ERR_INVALID_ARGUMENT;
    n_sweeps = h_sweep_off[n_scenes];
    if (n_sweeps > 0x7ffffffeLL) return HIMO_ERR_UNSUPPORTED;
    if (bt_offsets(n_sweeps, h_det_off)) return HIMO_ERR_INVALID_ARGUMENT;
    for (int64_t k = 0; k < n_sweeps; ++k) {
        const int64_t f = h_det_off[k + 1] - h_det_off[k];
        if (f > kBtMax) return HIMO_ERR_UNSUPPORTED;
        if ((int)f > most) most = (int)f;
    }
    n_rows = h_det_off[n_sweeps];
    return HIMO_OK;
}

static int bt_run(int n_scenes, const double* d_det, const int64_t* h_sweep_off, const int64_t* d_sweep_off, const int64_t* h_det_off,
                  const int64_t* d_det_off, const double* h_dt, const double* d_dt, const himo_boxtrack_params* params, int32_t* d_track_id,
                  int32_t* d_age, double* d_state, double* d_iou, int32_t* d_live, int32_t* d_scene_info, void* d_workspace, size_t workspace_bytes,
                  int slab, void* stream) {
    if (n_scenes < 0 || slab < 1 || !bt_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_scenes == 0) return HIMO_OK;
    int64_t n_sweeps, n_rows;
    int most;
    const int st = bt_tables(n_scenes, h_sweep_off, h_det_off, n_sweeps, n_rows, most);
    if (st != HIMO_OK) return st;
    if (n_sweeps > 0 && !h_dt) return HIMO_ERR_INVALID_ARGUMENT;
    for (int s = 0; s < n_scenes; ++s)
        for (int64_t k = h_sweep_off[s] + 1; k < h_sweep_off[s + 1]; ++k)       // (dt of a scene's first sweep is not read)
            if (!isfinite(h_dt[k]) || !(h_dt[k] > 0.0)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_sweep_off || !d_det_off || bt_misaligned(d_sweep_off, 8) || bt_misaligned(d_det_off, 8)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_scene_info || bt_misaligned(d_scene_info, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_sweeps > 0 && (!d_dt || !d_live)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_rows > 0 && (!d_det || !d_track_id || !d_age || !d_state || !d_iou)) return HIMO_ERR_INVALID_ARGUMENT;
    if (bt_misaligned(d_dt, 8) || bt_misaligned(d_live, 4) || bt_misaligned(d_det, 8) || bt_misaligned(d_track_id, 4) || bt_misaligned(d_age, 4) ||
        bt_misaligned(d_state, 8) || bt_misaligned(d_iou, 8))
        return HIMO_ERR_INVALID_ARGUMENT;
    const int pitch = most > 0 ? most : 1;
    const size_t slice = bt_slice_bytes(params->max_tracks, pitch);
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < slice * (size_t)n_scenes) return HIMO_ERR_WORKSPACE;

    BtArgs p;
    p.scene0 = 0; p.n_sweeps = n_sweeps; p.n_rows = n_rows;
    p.det = d_det; p.sweep_off = d_sweep_off; p.det_off = d_det_off; p.dt = d_dt;
    p.min_iou = params->min_iou; p.alpha = params->alpha; p.beta = params->beta;
    p.max_age = params->max_age; p.max_tracks = params->max_tracks; p.vel_mode = params->vel_mode;
    p.pitch = pitch;
    p.track_id = d_track_id; p.age = d_age; p.state = d_state; p.iou = d_iou; p.live = d_live; p.scene_info = d_scene_info;
    p.ws = reinterpret_cast<char*>(d_workspace); p.slice = slice;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("bt_track_kernel", s);
        for (int s0 = 0; s0 < n_scenes; s0 += slab) {
            p.scene0 = s0;
            const int ns = n_scenes - s0 < slab ? n_scenes - s0 : slab;
            hipLaunchKernelGGL(bt_track_kernel, dim3((unsigned)ns), dim3(kBtThreads), 0, s, p);
        }
    }
    HIMO_LAUNCH_CHECK("bt_track_kernel");
    return HIMO_OK;
}

}  // namespace himo

using namespace himo;

extern "C" size_t himo_boxtrack_workspace_bytes(int n_scenes, const int64_t* h_sweep_off, const int64_t* h_det_off, const himo_boxtrack_params* params) {
    if (n_scenes < 0 || !bt_params_ok(params)) return 0;
    if (n_scenes == 0) return 256;
    int64_t n_sweeps, n_rows;
    int most;
    if (bt_tables(n_scenes, h_sweep_off, h_det_off, n_sweeps, n_rows, most) != HIMO_OK) return 0;
    return bt_slice_bytes(params->max_tracks, most > 0 ? most : 1) * (size_t)n_scenes;
}

extern "C" int himo_boxtrack(int n_scenes, const double* d_det, const int64_t* h_sweep_off, const int64_t* d_sweep_off, const int64_t* h_det_off,
                             const int64_t* d_det_off, const double* h_dt, const double* d_dt, const himo_boxtrack_params* params,
                             int32_t* d_track_id, int32_t* d_age, double* d_state, double* d_iou, int32_t* d_live, int32_t* d_scene_info,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
    return bt_run(n_scenes, d_det, h_sweep_off, d_sweep_off, h_det_off, d_det_off, h_dt, d_dt, params, d_track_id, d_age, d_state, d_iou, d_live,
                  d_scene_info, d_workspace, workspace_bytes, kBtSlab, stream);
}

extern "C" int himo_boxtrack_slabbed(int n_scenes, const double* d_det, const int64_t* h_sweep_off, const int64_t* d_sweep_off,
                                     const int64_t* h_det_off, const int64_t* d_det_off, const double* h_dt, const double* d_dt,
                                     const himo_boxtrack_params* params, int32_t* d_track_id, int32_t* d_age, double* d_state, double* d_iou,
                                     int32_t* d_live, int32_t* d_scene_info, void* d_workspace, size_t workspace_bytes, int slab_scenes, void* stream) {
    return bt_run(n_scenes, d_det, h_sweep_off, d_sweep_off, h_det_off, d_det_off, h_dt, d_dt, params, d_track_id, d_age, d_state, d_iou, d_live,
                  d_scene_info, d_workspace, workspace_bytes, slab_scenes, stream);
}
