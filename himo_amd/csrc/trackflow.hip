// trackflow.hip -- tracked velocities back into per-point flow ("track flow, v1"; the rule is the module docstring of
// himo_amd/track_flow.py) for gfx950.  PARITY UNPINNED: the reference has no such stage; this one is checked bit for bit against the
// pure-Python restatement of the written rule (tests/trackflow_ref.py).  Timing on synthetic tables: profiles/track_flow.txt (plan 0.56 ms and
// apply 3.87 ms per call of 16 scenes of 150 sweeps of 300 boxes and 120k points).
//
// A batch of scenes arrives as packed per-box tables in the row order of BoxTracker.tables (scenes -> sweeps -> box rows): the track id
// (int32, -1 = none), the box velocity in the scene frame w (double [3], made on the host from box rows and poses), the box rows
// themselves (float [12], columns 7..9 the float32 velocity) and per sweep U = inv(T_k)[:3,:3] (double [9]).  Three kernels, all
// asynchronous on the caller's stream, no host wait between them:
//   tf_length_kernel  rule B: a thread per box row; a USABLE row adds 1 to its id's word of the scene's slice of the workspace (integer
//                     atomics: exact in any order).  The slice is zeroed on the stream first.
//   tf_plan_kernel    rules C-D: ONE 512-thread workgroup per (scene, sweep).  The ids of the window's sweeps (at most 2*8+1 = 17 of at
//                     most 512 rows) are staged in LDS, -1 where the row is not USABLE; a thread per box row of the sweep walks the staged
//                     sweeps in ascending order and scans each for its id (every lane reads the same LDS word: a broadcast).  S += w_j in
//                     that order, wbar = S / m, u = U wbar, d_s, d_b, the state and the two float32 vectors.
//   tf_apply_kernel   rule E: a streaming pass over the packed point rows of several sweeps, 1024 rows a block of 256 threads (four rows
//                     a thread, 256 apart: 256 rows a block took 3.3 times himo_accum_motion's time at 18M rows, the staging below
//                     being 7 KB beside 11 KB of rows; profiles/track_flow.txt).  The block's flow rows go through LDS so that global
//                     loads and stores are 16 bytes a lane where the table is 16-byte aligned (a tile is 12288 bytes, so every whole
//                     tile of an aligned table is); pc0 is read as one 16-byte load a row at pitch 4.
//                     A tile may cross sweeps: the block walks the sweeps it touches (segment_of, blockops.h), stages that sweep's sorted
//                     label ids with the plan's state and vector in LDS once and every row of the sweep finds its box by binary search
//                     (the lower bound: among equal ids the lowest row).  A row that is not rewritten keeps its input bytes.  The two
//                     counts of a sweep: a sum per wave, an LDS sum per block, one integer atomic per block and count.
// BARRIERS sit in block-uniform control flow: the window, the sweeps a tile touches and every F come from values all threads compute
// alike from the clamped device tables.  The device offsets are clamped to the host's totals and to the cap; ids outside a scene's
// slice count as not USABLE; a sorted row index outside its sweep finds no box: a device table that disagrees with the host's can make a
// wrong answer but no access outside the tables and no unbounded loop.
// The only atomics are integer adds, so two runs give the same bytes.
//
// Built with -ffp-contract=off: every operation rounds on its own, as in the restatement.  Only + - * / and comparisons; the move
// a = E p is rigid_math.h's written sequence (himo_rigid_transform), which no flag changes.
#include "himo_common.h"
#include "blockops.h"
#include "rigid_math.h"
#include <math.h>

namespace himo {

constexpr int kTfMax = HIMO_BOXTRACK_MAX;        // box rows of a sweep
constexpr int kTfHalfMax = 8;
constexpr int kTfWindow = 2 * kTfHalfMax + 1;
constexpr int kTfPlanThreads = 512;
constexpr int kTfThreads = 256;                  // length and apply
constexpr int kTfPer = 4;                        // point rows a thread of apply
constexpr int kTfTile = kTfThreads * kTfPer;     // point rows a block of apply
constexpr int kTfWide = 3 * kTfTile / 4 / kTfThreads;      // 16-byte words of a whole tile's flow a thread
constexpr int kTfNone = 0, kTfMoving = 1, kTfStatic = 2;
static_assert(kTfMax <= kTfPlanThreads && kTfWide == 3 && 4 * kTfWide * kTfThreads == 3 * kTfTile && kTfThreads % 64 == 0, "trackflow tiling");

__device__ inline int64_t tf_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ inline bool tf_finite(double v) { return v - v == 0.0; }
__device__ inline bool tf_finite(float v) { return v - v == 0.0f; }

struct TfPlanArgs {
    int n_scenes;
    int64_t n_sweeps, n_rows, n_ids;                 // the host's totals
    const int64_t* sweep_off; const int64_t* det_off; const int64_t* id_off;
    const int32_t* id; const double* w; const float* boxes; const double* U;
    double sensor_dt, motion_min;
    int half, min_len;
    int32_t* len;                                    // the workspace: int32 [n_ids]
    int32_t* state; int32_t* m; float* shift; float* disp; double* u;
};

// the row's id if the row is USABLE inside the scene's slice [0, n) of the id table, else -1
__device__ inline int tf_usable_id(const TfPlanArgs& p, int64_t row, int64_t n) {
    const int id = p.id[row];
    if (id < 0 || (int64_t)id >= n) return -1;
    const double* w = p.w + 3 * row;
    return tf_finite(w[0]) && tf_finite(w[1]) && tf_finite(w[2]) ? id : -1;
}

// rule B
__global__ __launch_bounds__(kTfThreads) void tf_length_kernel(TfPlanArgs p) {
    const int64_t row = (int64_t)blockIdx.x * kTfThreads + threadIdx.x;
    if (row >= p.n_rows) return;
    const int q = segment_of(p.det_off, (int)p.n_sweeps, row);
    if (!(p.det_off[q] <= row && row < p.det_off[q + 1])) return;
    const int scene = segment_of(p.sweep_off, p.n_scenes, (int64_t)q);
    if (!(p.sweep_off[scene] <= q && q < p.sweep_off[scene + 1])) return;
    const int64_t i0 = tf_clamp(p.id_off[scene], 0, p.n_ids), i1 = tf_clamp(p.id_off[scene + 1], i0, p.n_ids);
    const int id = tf_usable_id(p, row, i1 - i0);
    if (id >= 0) atomicAdd(p.len + i0 + id, 1);
}

// rules C and D: a workgroup per (scene, sweep)
__global__ __launch_bounds__(kTfPlanThreads) void tf_plan_kernel(TfPlanArgs p) {
    __shared__ int s_id[kTfWindow][kTfMax];
    const int t = (int)threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x;
    // every thread computes the same window from the clamped tables (block-uniform)
    const int scene = segment_of(p.sweep_off, p.n_scenes, q);
    const int64_t k0 = tf_clamp(p.sweep_off[scene], 0, p.n_sweeps), k1 = tf_clamp(p.sweep_off[scene + 1], k0, p.n_sweeps);
    if (q < k0 || q >= k1) return;
    const int64_t i0 = tf_clamp(p.id_off[scene], 0, p.n_ids), i1 = tf_clamp(p.id_off[scene + 1], i0, p.n_ids);
    const int64_t j0 = q - p.half > k0 ? q - p.half : k0, j1 = q + p.half < k1 - 1 ? q + p.half : k1 - 1;
    const int nw = (int)(j1 - j0 + 1) < kTfWindow ? (int)(j1 - j0 + 1) : kTfWindow;
    for (int s = 0; s < nw; ++s) {
        const int64_t lo = tf_clamp(p.det_off[j0 + s], 0, p.n_rows), hi = tf_clamp(p.det_off[j0 + s + 1], lo, p.n_rows);
        const int F = (int)(hi - lo < kTfMax ? hi - lo : kTfMax);
        if (t < F) s_id[s][t] = tf_usable_id(p, lo + t, i1 - i0);
    }
    __syncthreads();
    const int64_t d0 = tf_clamp(p.det_off[q], 0, p.n_rows), d1 = tf_clamp(p.det_off[q + 1], d0, p.n_rows);
    const int F = (int)(d1 - d0 < kTfMax ? d1 - d0 : kTfMax);
    if (t >= F) return;
    const int64_t row = d0 + t;
    const int id = s_id[(int)(q - j0)][t];
    int state = kTfNone, m = 0;
    double u[3] = {0.0, 0.0, 0.0};
    float shift[3] = {0.f, 0.f, 0.f}, disp[3] = {0.f, 0.f, 0.f};
    if (id >= 0 && p.len[i0 + id] >= p.min_len) {
        double S[3] = {0.0, 0.0, 0.0};
        for (int s = 0; s < nw; ++s) {
            const int64_t lo = tf_clamp(p.det_off[j0 + s], 0, p.n_rows), hi = tf_clamp(p.det_off[j0 + s + 1], lo, p.n_rows);
            const int Fs = (int)(hi - lo < kTfMax ? hi - lo : kTfMax);
            int pos = -1;
            for (int c = 0; c < Fs; ++c)
                if (s_id[s][c] == id) { pos = c; break; }            // the lowest such row
            if (pos >= 0) {
                const double* w = p.w + 3 * (lo + pos);
                S[0] = S[0] + w[0]; S[1] = S[1] + w[1]; S[2] = S[2] + w[2];
                m += 1;
            }
        }
        const double dm = (double)m;                                // m >= 1: the sweep itself counts
        const double wb[3] = {S[0] / dm, S[1] / dm, S[2] / dm};
        const double* U = p.U + 9 * q;
        double ds[3], db[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            u[e] = (U[3 * e] * wb[0] + U[3 * e + 1] * wb[1]) + U[3 * e + 2] * wb[2];
            ds[e] = u[e] * p.sensor_dt;
            db[e] = (double)p.boxes[12 * row + 7 + e] * p.sensor_dt;
            shift[e] = (float)(ds[e] - db[e]);
            disp[e] = (float)ds[e];
        }
        const double d2 = (ds[0] * ds[0] + ds[1] * ds[1]) + ds[2] * ds[2];
        state = d2 < p.motion_min * p.motion_min ? kTfStatic : kTfMoving;
    }
    p.state[row] = state;
    p.m[row] = m;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        p.shift[3 * row + e] = shift[e];
        p.disp[3 * row + e] = disp[e];
        p.u[3 * row + e] = u[e];
    }
}

struct TfApplyArgs {
    int n_sweeps;
    int64_t n_rows, n_box_rows;                      // the host's totals
    const int64_t* pt_off; const int64_t* box_off;
    const float* pc0; int pitch; bool pc0_wide, flow_wide;
    const uint32_t* flow; const int32_t* label; const float* E;
    const int32_t* sorted_id; const int32_t* sorted_row;
    const int32_t* state; const float* vec;          // shift (mode 0) or disp (mode 1)
    int mode;
    uint32_t* out; int32_t* counts;
};

// rule E
__global__ __launch_bounds__(kTfThreads) void tf_apply_kernel(TfApplyArgs p) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flow[3 * kTfTile];
    __shared__ int s_id[kTfMax], s_state[kTfMax];
    __shared__ float s_vec[3][kTfMax];
    __shared__ int s_cnt[2][kTfThreads / 64];
    const int t = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kTfTile;
    const int rows = (int)(p.n_rows - row0 < kTfTile ? p.n_rows - row0 : kTfTile);      // >= 1 by the grid

    // every load that depends on no table is issued first: the tile's flow rows (16 bytes a lane where the tile is whole and the table
    // aligned; they go through LDS), the labels and points of the thread's rows t, t + 256, ...
    const bool wide = p.flow_wide && rows == kTfTile;               // (block-uniform)
    uint4 fw0 = make_uint4(0u, 0u, 0u, 0u), fw1 = fw0, fw2 = fw0;   // (named, not an array: an array of them went to scratch)
    if (wide) {
        const uint4* src = reinterpret_cast<const uint4*>(p.flow + 3 * row0) + t;
        fw0 = src[0]; fw1 = src[kTfThreads]; fw2 = src[2 * kTfThreads];
    }
    int lab[kTfPer], mine[kTfPer];
    float x[kTfPer], y[kTfPer], z[kTfPer];
#pragma unroll
    for (int j = 0; j < kTfPer; ++j) {
        const int r = j * kTfThreads + t;
        lab[j] = 0; mine[j] = -1; x[j] = 0.f; y[j] = 0.f; z[j] = 0.f;
        if (r < rows) {
            const int64_t i = row0 + r;
            lab[j] = p.label[i];
            if (p.pc0_wide) {
                const float4 v = *reinterpret_cast<const float4*>(p.pc0 + 4 * i);
                x[j] = v.x; y[j] = v.y; z[j] = v.z;
            } else {
                const float* q = p.pc0 + i * p.pitch;
                x[j] = q[0]; y[j] = q[1]; z[j] = q[2];
            }
        }
    }
    // the sweeps this tile touches (block-uniform: the same search in every thread) and the sweep of each of the thread's rows: a
    // search of its own only where the tile crosses sweeps
    const int kf = segment_of(p.pt_off, p.n_sweeps, row0), kl = segment_of(p.pt_off, p.n_sweeps, row0 + rows - 1);
#pragma unroll
    for (int j = 0; j < kTfPer; ++j) {
        const int r = j * kTfThreads + t;
        if (r < rows) {
            const int64_t i = row0 + r;
            const int k = kf == kl ? kf : segment_of(p.pt_off, p.n_sweeps, i);
            if (p.pt_off[k] <= i && i < p.pt_off[k + 1]) mine[j] = k;
        }
    }
    if (wide) {
        uint4* dst = reinterpret_cast<uint4*>(s_flow) + t;
        dst[0] = fw0; dst[kTfThreads] = fw1; dst[2 * kTfThreads] = fw2;
    } else {
        for (int e = t; e < 3 * rows; e += kTfThreads) s_flow[e] = p.flow[3 * row0 + e];
    }
    __syncthreads();
    for (int k = kf; k <= kl; ++k) {
        const int64_t b0 = tf_clamp(p.box_off[k], 0, p.n_box_rows), b1 = tf_clamp(p.box_off[k + 1], b0, p.n_box_rows);
        const int F = (int)(b1 - b0 < kTfMax ? b1 - b0 : kTfMax);
        if (F == 0) continue;                                       // (block-uniform) no box: every row of the sweep keeps its bytes
        for (int c = t; c < F; c += kTfThreads) {
            const int r = p.sorted_row[b0 + c];
            const bool ok = r >= 0 && r < F;
            s_id[c] = p.sorted_id[b0 + c];
            s_state[c] = ok ? p.state[b0 + r] : kTfNone;
#pragma unroll
            for (int e = 0; e < 3; ++e) s_vec[e][c] = ok ? p.vec[3 * (b0 + r) + e] : 0.f;
        }
        __syncthreads();
        int nm = 0, ns = 0;                                         // this thread's rows written as MOVING, as STATIC
#pragma unroll
        for (int j = 0; j < kTfPer; ++j) {
            if (mine[j] != k || lab[j] <= 0) continue;
            const int r = j * kTfThreads + t;
            int lo = 0, hi = F;                                     // the lower bound of the label in s_id[0, F)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_id[mid] < lab[j]) lo = mid + 1; else hi = mid;
            }
            if (!(lo < F && s_id[lo] == lab[j] && s_state[lo] != kTfNone)) continue;
            const float f0 = __builtin_bit_cast(float, s_flow[3 * r]), f1 = __builtin_bit_cast(float, s_flow[3 * r + 1]),
                        f2 = __builtin_bit_cast(float, s_flow[3 * r + 2]);
            if (!(tf_finite(f0) && tf_finite(f1) && tf_finite(f2))) continue;
            float o[3];
            const bool still = s_state[lo] == kTfStatic;
            if (!still && p.mode == 0) {
                o[0] = f0 + s_vec[0][lo]; o[1] = f1 + s_vec[1][lo]; o[2] = f2 + s_vec[2][lo];
            } else {
                float a[3];
                rigid_apply(p.E + 12 * k, x[j], y[j], z[j], a);
                o[0] = a[0] - x[j]; o[1] = a[1] - y[j]; o[2] = a[2] - z[j];
                if (!still) { o[0] = o[0] + s_vec[0][lo]; o[1] = o[1] + s_vec[1][lo]; o[2] = o[2] + s_vec[2][lo]; }
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) s_flow[3 * r + e] = __builtin_bit_cast(uint32_t, o[e]);
            if (still) ns += 1; else nm += 1;
        }
        // the sweep's two counts: a sum per wave (blockops.h), summed by thread 0, one atomic per count that is not zero
        wave_sum2(nm, ns);
        if ((t & 63) == 0) { s_cnt[0][t >> 6] = nm; s_cnt[1][t >> 6] = ns; }
        __syncthreads();                                            // (also: every thread is done with the staged tables)
        if (t == 0) {
            int cm = 0, cs = 0;
#pragma unroll
            for (int wv = 0; wv < kTfThreads / 64; ++wv) { cm += s_cnt[0][wv]; cs += s_cnt[1][wv]; }
            if (cm) atomicAdd(p.counts + 2 * k, cm);
            if (cs) atomicAdd(p.counts + 2 * k + 1, cs);
        }
        __syncthreads();                                            // (s_cnt is read before the next sweep writes it)
    }
    __syncthreads();
    if (wide) {
#pragma unroll
        for (int j = 0; j < kTfWide; ++j)
            reinterpret_cast<uint4*>(p.out + 3 * row0)[j * kTfThreads + t] = reinterpret_cast<const uint4*>(s_flow)[j * kTfThreads + t];
    } else {
        for (int e = t; e < 3 * rows; e += kTfThreads) p.out[3 * row0 + e] = s_flow[e];
    }
}

// offsets [n + 1] that start at 0 (from_zero) or at any value >= 0 and never decrease: 0 ok, 1 malformed
static int tf_offsets(int64_t n, const int64_t* h, bool from_zero) {
    if (!h || h[0] < 0 || (from_zero && h[0] != 0)) return 1;
    for (int64_t s = 0; s < n; ++s)
        if (h[s + 1] < h[s]) return 1;
    return 0;
}

static bool tf_misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

static bool tf_params_ok(const himo_trackflow_params* q) {
    if (!q) return false;
    if (!isfinite(q->sensor_dt) || !(q->sensor_dt > 0.0)) return false;
    if (!isfinite(q->motion_min) || !(q->motion_min >= 0.0)) return false;
    return q->half >= 0 && q->half <= kTfHalfMax && q->min_len >= 1 && (q->mode == 0 || q->mode == 1) && q->reserved == 0;
}

// the host tables of a plan call: HIMO_OK and the totals, or the status that refuses them
static int tf_tables(int n_scenes, const int64_t* h_sweep_off, const int64_t* h_det_off, const int64_t* h_id_off, int64_t& n_sweeps,
                     int64_t& n_rows, int64_t& n_ids) {
    n_sweeps = 0; n_rows = 0; n_ids = 0;
    if (tf_offsets(n_scenes, h_sweep_off, true) || tf_offsets(n_scenes, h_id_off, true)) return HIMO_ERR_INVALID_ARGUMENT;
    n_sweeps = h_sweep_off[n_scenes];
    n_ids = h_id_off[n_scenes];
    if (n_sweeps > 0x7ffffffeLL || n_ids > 0x7ffffffeLL) return HIMO_ERR_UNSUPPORTED;
    if (tf_offsets(n_sweeps, h_det_off, true)) return HIMO_ERR_INVALID_ARGUMENT;
    for (int64_t k = 0; k < n_sweeps; ++k)
        if (h_det_off[k + 1] - h_det_off[k] > kTfMax) return HIMO_ERR_UNSUPPORTED;
    n_rows = h_det_off[n_sweeps];
    return HIMO_OK;
}

}  // namespace himo

using namespace himo;

extern "C" size_t himo_trackflow_workspace_bytes(int n_scenes, const int64_t* h_sweep_off, const int64_t* h_det_off, const int64_t* h_id_off) {
    if (n_scenes < 0) return 0;
    if (n_scenes == 0) return 256;
    int64_t n_sweeps, n_rows, n_ids;
    if (tf_tables(n_scenes, h_sweep_off, h_det_off, h_id_off, n_sweeps, n_rows, n_ids) != HIMO_OK) return 0;
    return round_up((size_t)(n_ids > 0 ? n_ids : 1) * sizeof(int32_t), 256);
}

extern "C" int himo_trackflow_plan(int n_scenes, const int64_t* h_sweep_off, const int64_t* d_sweep_off, const int64_t* h_det_off,
                                   const int64_t* d_det_off, const int64_t* h_id_off, const int64_t* d_id_off, const int32_t* d_id,
                                   const double* d_w, const float* d_boxes, const double* d_U, const himo_trackflow_params* params,
                                   int32_t* d_state, int32_t* d_m, float* d_shift, float* d_disp, double* d_u, void* d_workspace,
                                   size_t workspace_bytes, void* stream) {
    if (n_scenes < 0 || !tf_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_scenes == 0) return HIMO_OK;
    int64_t n_sweeps, n_rows, n_ids;
    const int st = tf_tables(n_scenes, h_sweep_off, h_det_off, h_id_off, n_sweeps, n_rows, n_ids);
    if (st != HIMO_OK) return st;
    if (!d_sweep_off || !d_det_off || !d_id_off || tf_misaligned(d_sweep_off, 8) || tf_misaligned(d_det_off, 8) || tf_misaligned(d_id_off, 8))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (n_sweeps > 0 && !d_U) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_rows > 0 && (!d_id || !d_w || !d_boxes || !d_state || !d_m || !d_shift || !d_disp || !d_u)) return HIMO_ERR_INVALID_ARGUMENT;
    if (tf_misaligned(d_U, 8) || tf_misaligned(d_id, 4) || tf_misaligned(d_w, 8) || tf_misaligned(d_boxes, 4) || tf_misaligned(d_state, 4) ||
        tf_misaligned(d_m, 4) || tf_misaligned(d_shift, 4) || tf_misaligned(d_disp, 4) || tf_misaligned(d_u, 8))
        return HIMO_ERR_INVALID_ARGUMENT;
    const size_t need = round_up((size_t)(n_ids > 0 ? n_ids : 1) * sizeof(int32_t), 256);
    if (!d_workspace || !aligned16(d_workspace) || workspace_bytes < need) return HIMO_ERR_WORKSPACE;
    if (n_rows == 0) return HIMO_OK;                                // sweeps without a box: nothing to plan

    TfPlanArgs p;
    p.n_scenes = n_scenes; p.n_sweeps = n_sweeps; p.n_rows = n_rows; p.n_ids = n_ids;
    p.sweep_off = d_sweep_off; p.det_off = d_det_off; p.id_off = d_id_off;
    p.id = d_id; p.w = d_w; p.boxes = d_boxes; p.U = d_U;
    p.sensor_dt = params->sensor_dt; p.motion_min = params->motion_min; p.half = params->half; p.min_len = params->min_len;
    p.len = reinterpret_cast<int32_t*>(d_workspace);
    p.state = d_state; p.m = d_m; p.shift = d_shift; p.disp = d_disp; p.u = d_u;
    hipStream_t s = (hipStream_t)stream;
    HIMO_HIP(hipMemsetAsync(d_workspace, 0, need, s));
    {
        ProfScope ps("tf_length_kernel", s);
        hipLaunchKernelGGL(tf_length_kernel, dim3((unsigned)((n_rows + kTfThreads - 1) / kTfThreads)), dim3(kTfThreads), 0, s, p);
    }
    HIMO_LAUNCH_CHECK("tf_length_kernel");
    {
        ProfScope ps("tf_plan_kernel", s);
        hipLaunchKernelGGL(tf_plan_kernel, dim3((unsigned)n_sweeps), dim3(kTfPlanThreads), 0, s, p);
    }
    HIMO_LAUNCH_CHECK("tf_plan_kernel");
    return HIMO_OK;
}

extern "C" int himo_trackflow_apply(int n_sweeps, const int64_t* h_pt_off, const int64_t* d_pt_off, const float* d_pc0, int pitch,
                                    const float* d_flow, const int32_t* d_label, const float* d_E, const int64_t* h_box_off,
                                    const int64_t* d_box_off, int64_t n_box_rows, const int32_t* d_sorted_id, const int32_t* d_sorted_row,
                                    const int32_t* d_state, const float* d_shift, const float* d_disp, const himo_trackflow_params* params,
                                    float* d_out, int32_t* d_counts, void* stream) {
    if (n_sweeps < 0 || pitch < 3 || n_box_rows < 0 || !tf_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_sweeps == 0) return HIMO_OK;
    if (tf_offsets(n_sweeps, h_pt_off, true) || tf_offsets(n_sweeps, h_box_off, false) || h_box_off[n_sweeps] > n_box_rows)
        return HIMO_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < n_sweeps; ++k)
        if (h_box_off[k + 1] - h_box_off[k] > kTfMax) return HIMO_ERR_UNSUPPORTED;
    const int64_t n_rows = h_pt_off[n_sweeps], boxes = h_box_off[n_sweeps] - h_box_off[0];
    if ((n_rows + kTfTile - 1) / kTfTile > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (!d_pt_off || !d_box_off || !d_E || !d_counts || tf_misaligned(d_pt_off, 8) || tf_misaligned(d_box_off, 8) || tf_misaligned(d_E, 4) ||
        tf_misaligned(d_counts, 4))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (n_rows > 0 && (!d_pc0 || !d_flow || !d_label || !d_out)) return HIMO_ERR_INVALID_ARGUMENT;
    if (boxes > 0 && (!d_sorted_id || !d_sorted_row || !d_state || !d_shift || !d_disp)) return HIMO_ERR_INVALID_ARGUMENT;
    if (tf_misaligned(d_pc0, 4) || tf_misaligned(d_flow, 4) || tf_misaligned(d_label, 4) || tf_misaligned(d_out, 4) || tf_misaligned(d_sorted_id, 4) ||
        tf_misaligned(d_sorted_row, 4) || tf_misaligned(d_state, 4) || tf_misaligned(d_shift, 4) || tf_misaligned(d_disp, 4))
        return HIMO_ERR_INVALID_ARGUMENT;

    hipStream_t s = (hipStream_t)stream;
    HIMO_HIP(hipMemsetAsync(d_counts, 0, 2 * (size_t)n_sweeps * sizeof(int32_t), s));
    if (n_rows == 0) return HIMO_OK;
    TfApplyArgs p;
    p.n_sweeps = n_sweeps; p.n_rows = n_rows; p.n_box_rows = n_box_rows;
    p.pt_off = d_pt_off; p.box_off = d_box_off;
    p.pc0 = d_pc0; p.pitch = pitch;
    p.pc0_wide = pitch == 4 && !tf_misaligned(d_pc0, 16);
    p.flow_wide = !tf_misaligned(d_flow, 16) && !tf_misaligned(d_out, 16);
    p.flow = reinterpret_cast<const uint32_t*>(d_flow); p.label = d_label; p.E = d_E;
    p.sorted_id = d_sorted_id; p.sorted_row = d_sorted_row; p.state = d_state;
    p.vec = params->mode == 0 ? d_shift : d_disp; p.mode = params->mode;
    p.out = reinterpret_cast<uint32_t*>(d_out); p.counts = d_counts;
    {
        ProfScope ps("tf_apply_kernel", s);
        hipLaunchKernelGGL(tf_apply_kernel, dim3((unsigned)((n_rows + kTfTile - 1) / kTfTile)), dim3(kTfThreads), 0, s, p);
    }
    HIMO_LAUNCH_CHECK("tf_apply_kernel");
    return HIMO_OK;
}
