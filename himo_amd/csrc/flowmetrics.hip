// flowmetrics.hip -- the scene-flow evaluator's integer tables ("flow metrics, v1", himo_amd/eval_flow.py) for gfx950.
//
//   pc0 + ground-truth flow + R estimated flows + category / ground / valid bytes + poses of a packed batch of sweeps
//       ->  int64 buckets[R][5][51][3] (+=),  int64 threeway[F][R][3][2] (+=),  int64 rejected[R] (+=)
//           and, through himo_flow_metrics_batch_ex,  int64 accuracy[R][4][3] (+=)
//
// PARITY UNPINNED: the reference scores flow in its absent OpenSceneFlow submodule; this is the package's own written rule,
// following the published three-way EPE and the Argoverse-2 bucketed normalised EPE.  No claim about the reference's numbers.
//
// The rule per counted point (eval_mask_point of compdis_math.h: BEV range, not ground, outside the ego box, flow_is_valid
// with HIMO_FLAG_SCANIA), all in IEEE double on the float32 inputs, every operation rounded on its own (-ffp-contract=off):
//     g     = gt - pose_flow                      pose_flow = T p - p, the k-ordered chain of pose_flow_f64
//     speed = sqrt((gx gx + gy gy) + gz gz)
//     d_r   = est_r - gt   (raw: d = -g)          epe_r = sqrt((dx dx + dy dy) + dz dz)
//     rejected for r: a non-finite est component or not epe_r < 1024 m (so a NaN error -- non-finite ground truth -- is
//                     rejected too, not summed)
//     q(x)  = llrint(x * 2^24)                    every sum is an int64 sum of q(epe) or q(speed): order cannot change a digit
//     class = lut[category] (0..4 bucketed, 5 = foreground in no bucket);   bucket = #{k in 1..50 : speed >= k * w}
//     kind  = FD (class != 0, speed > thr) | FS (class != 0, not) | BS (class == 0, not) | none (background, dynamic)
//
// Work split: a block owns ONE contiguous run of the packed points (total / blocks, a multiple of 256) and walks it 256 points
// at a time, one point per lane -- not an interleaved grid stride, because the per-sweep three-way words then stay in LDS: a
// block meets its sweeps one after the other, keeps the words of the sweep its current 256 points start in, and writes them
// out (one 64-bit global atomic per non-zero word) when that sweep changes.  Points of a later sweep inside the same 256
// (boundaries, sweeps smaller than a block) go to the global words directly.  Interleaved, every wave of the grid would add
// to the same half dozen global words at once; one word takes an atomic about every 11 ns.
// The bucket table is R x 255 x 3 int64 per block in LDS (48 960 B at R = 8), flushed once at the end, one global atomic per
// non-zero word.
//
// Most points of a real sweep share one bin (background, bucket 0) and 64 lanes on one LDS address serialise, so lanes are
// aggregated inside the wave first: the first pending lane's key is broadcast and the lanes that share it are balloted; eight
// or more have their count and sums reduced by shuffles and added by that one lane, fewer add their own values (a reduction
// is six dependent shuffles of two dwords per sum; reducing every key cost 435 instead of 230 us at R = 4).  After kFlowRounds
// keys the lanes still pending add their own values.  The same scheme keyed by (sweep, kind) feeds the three-way words.  No
// float atomics anywhere.
//
// Measured (profiles/eval_flow.txt): 32 x 120 000 points in 128 us at R = 1, 230 us at R = 4 -- 1.3 TB/s, a quarter of the
// comp_dis kernel's rate: the double chain (a correctly rounded double sqrt per result) and the shuffles, not bandwidth.
//
// Two additions to the rule (himo_flow_metrics_batch_ex; both PARITY UNPINNED, the package's own rule), compile-time switches of
// the one kernel -- the (accuracy off, residual off) instantiation is the v1 kernel and does the work it always did:
//     rule 3b, residual estimates (HIMO_FLAG_EST_RESIDUAL): est_r is the ego-motion-free part of a result (the network's own
//              output rows, before pose_flow is added): d_r = (double)res_r - g; rejected as in v1 (non-finite component, not
//              epe < 1024).  An all-zero residual is the raw result (d = -g).  Rows of est_stride >= 3 floats are read in place.
//     rule 9,  accuracy table (d_accuracy != NULL): gn = sqrt((gx gx + gy gy) + gz gz) of the STORED ground truth (ego motion
//              included), strict iff epe < 0.05 || epe < 0.05 * gn, relaxed iff epe < 0.1 || epe < 0.1 * gn (the doubles nearest
//              0.05 and 0.1, every product rounded once); groups 0 = ALL (every counted non-rejected point), 1 = FD, 2 = FS,
//              3 = BS; int64 accuracy[R][4][3] = count, strict, relaxed (+=).
// The accuracy words take the path of the three-way words: the wave's lanes are counted by ballot, one lane adds the counts to
// R x 12 words of LDS, and the block ends with one 64-bit global atomic per non-zero word.
// LDS per block (-Rpass-analysis=kernel-resource-usage, R = 1..8, no scratch in any of the 32 instantiations): 6 176 R + 256 B
// without the accuracy table (6 432 B at R = 1, 49 664 B at R = 8: the 48 960 B bucket table, 384 B of three-way words, 64 B of
// rejected counts and the 256 B class table), 96 R more with it (6 528 B at R = 1, 50 432 B at R = 8).  77 .. 137 VGPRs; the v1
// instantiations compile to the instructions they had before the switches existed.
//
// Traffic: 12 (gt) + 3 (category, ground, valid) + 16 or 12 (pc0 row) + 12 R bytes per point = 31 + 12 R with the row's
// padding; the transforms (96 B per sweep) come from the per-sweep prep of compdis.hip (launch_frame_prep with no points: it
// reads no lidar_dt then).
#include "compdis_math.h"

namespace himo {

typedef unsigned long long ull;

constexpr int kFlowThreads = 256;
constexpr int kFlowMaxBlocks = 1024;         // 4 per CU, as kSegMaxBlocks (8 per CU measured no faster); bounds the flush at 765 R x 1024 atomics
constexpr int kFlowBins = HIMO_FLOWM_CLASSES * HIMO_FLOWM_BUCKETS;   // 255
constexpr int kFlowRounds = 6;               // keys retired one after the other before the rest go lane by lane
constexpr int kFlowMinGroup = 8;             // lanes sharing a key below which they add their own values instead of reducing
constexpr double kFlowScale = 16777216.0;    // 2^24 units per metre
constexpr double kFlowReject = 1024.0;
constexpr double kFlowStrict = 0.05, kFlowRelaxed = 0.1;     // rule 9: the doubles nearest 0.05 and 0.1
constexpr int kFlowAccWords = 12;            // 4 groups x (count, strict, relaxed)

struct FlowmArgs {
    int n_frames;
    int pc_stride;
    int64_t total;
    int64_t chunk;                           // points per block, a multiple of kFlowThreads
    const int64_t* offsets;
    const FrameXf* xf;
    const float* pc0;
    const float* gt;
    const float* est[HIMO_FLOWM_MAX_RESULTS];   // nullptr = raw
    const uint8_t* category;
    const uint8_t* ground;
    const uint8_t* valid;                    // nullptr: not used
    double dyn_thr;                          // 0.5 * sensor_dt
    double w;                                // 0.4 * sensor_dt
    float bmin[3], bmax[3];
    float close_distance;
    ull* buckets;
    ull* threeway;
    ull* rejected;
    unsigned lut[64];                        // uint8[256]
};

// ... and what the instantiations with an addition take on top (the v1 instantiation keeps the argument block it always had)
struct FlowmArgsEx : FlowmArgs {
    ull* accuracy;                           // [R][4][3], nullptr: not written
    int est_stride;                          // floats per estimate row (v1 rows have 3)
};
template <bool EX> struct FlowmArgsOf { typedef FlowmArgs type; };
template <> struct FlowmArgsOf<true> { typedef FlowmArgsEx type; };

__device__ inline int flow_bucket(double speed, double w) {
    int b = speed >= w ? (int)fmin(speed / w, (double)(HIMO_FLOWM_BUCKETS - 1)) : 0;   // a guess, then the rule itself
    while (b < HIMO_FLOWM_BUCKETS - 1 && speed >= (double)(b + 1) * w) ++b;
    while (b > 0 && speed < (double)b * w) --b;
    return b;
}

// Add every pending lane's (1, qe[r], qs) to the words `emit` addresses for its key: kFlowRounds rounds that each retire all
// lanes sharing the first pending lane's key through ONE lane, then the rest lane by lane.  Called by whole waves.
// emit(key, r, count, sum of qe, sum of qs) runs on one lane per key and r.
template <int R, bool SPEED, typename Emit>
__device__ inline void wave_accumulate(bool pending, int key, const bool (&ok)[R], const ull (&qe)[R], ull qs, Emit emit) {
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int round = 0; round < kFlowRounds; ++round) {
        const ull todo = __ballot(pending);
        if (todo == 0) return;
        const int leader = __ffsll((long long)todo) - 1;
        const int key0 = __shfl(key, leader, 64);
        const bool same = pending && key == key0;
        if (__popcll(__ballot(same)) < kFlowMinGroup) {               // (wave-uniform) a few lanes: their own atomics cost less
            if (same) {                                               // than the shuffles of a reduction
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (ok[r]) emit(key, r, 1ull, qe[r], qs);
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool take = same && ok[r];
                const ull members = __ballot(take);
                if (members == 0) continue;                           // (wave-uniform)
                const ull se = wave_sum(take ? qe[r] : 0ull);
                const ull ss = SPEED ? wave_sum(take ? qs : 0ull) : 0ull;
                if (lane == leader) emit(key0, r, (ull)__popcll(members), se, ss);
            }
        }
        pending = pending && !same;
    }
    if (pending) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (ok[r]) emit(key, r, 1ull, qe[r], qs);
    }
}

// ACC: rule 9's table beside the v1 tables.  RESID: rule 3b, every non-null estimate is a residual.  Either one also reads the
// estimates' rows at a.est_stride; without both the rows have 3 floats, as in v1.
template <int R, bool ACC, bool RESID>
__global__ __launch_bounds__(kFlowThreads) void flow_metrics_kernel(const typename FlowmArgsOf<ACC || RESID>::type a) {
    __shared__ ull s_bins[R * kFlowBins * 3];
    __shared__ ull s_tw[R * 6];
    __shared__ ull s_rej[R];
    __shared__ ull s_acc[ACC ? R * kFlowAccWords : 1];
    __shared__ unsigned s_lut[64];
    const int tid = threadIdx.x, lane = tid & 63;
    int est_stride = 3;
    if constexpr (ACC || RESID) est_stride = a.est_stride;
    for (int k = tid; k < R * kFlowBins * 3; k += kFlowThreads) s_bins[k] = 0;
    if (tid < R * 6) s_tw[tid] = 0;
    if (ACC && tid < R * kFlowAccWords) s_acc[tid] = 0;
    if (tid < R) s_rej[tid] = 0;
    if (tid < 64) s_lut[tid] = a.lut[tid];
    __syncthreads();
    const uint8_t* lut = reinterpret_cast<const uint8_t*>(s_lut);

    const int64_t start = (int64_t)blockIdx.x * a.chunk;
    const int64_t end = start + a.chunk < a.total ? start + a.chunk : a.total;
    int fcur = -1;                                                    // the sweep whose three-way words s_tw holds
    for (int64_t i0 = start; i0 < end; i0 += kFlowThreads) {
        const int fit = __builtin_amdgcn_readfirstlane(segment_of(a.offsets, a.n_frames, i0));
        if (fit != fcur) {                                            // (block-uniform)
            __syncthreads();
            if (fcur >= 0 && tid < R * 6) {
                const ull v = s_tw[tid];
                if (v != 0) atomicAdd(a.threeway + (size_t)fcur * (R * 6) + tid, v);
                s_tw[tid] = 0;
            }
            __syncthreads();
            fcur = fit;
        }
        const int64_t i = i0 + tid;
        bool counted = false;
        int f = fit;
        // every array of the point is loaded before the mask is known: one round trip to memory per step instead of two (the
        // lines of the points that turn out uncounted are fetched for their counted neighbours anyway)
        float px = 0.f, py = 0.f, pz = 0.f, gtf[3] = {0.f, 0.f, 0.f}, e[R][3];
        uint8_t cat = 0;
        XfRegs x;
        if (i < end) {
            while (f + 1 < a.n_frames && a.offsets[f + 1] <= i) ++f;
            const float* row = a.pc0 + (size_t)i * a.pc_stride;
            px = row[0]; py = row[1]; pz = row[2];
            const uint8_t gm = a.ground[i], vb = a.valid ? a.valid[i] : (uint8_t)1;
            cat = a.category[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) gtf[c] = a.gt[(size_t)i * 3 + c];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float* er = a.est[r];                           // (a kernel argument: uniform)
#pragma unroll
                for (int c = 0; c < 3; ++c) e[r][c] = er ? er[(size_t)i * est_stride + c] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) x.R[k] = a.xf[f].R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) x.t[k] = a.xf[f].t[k];
            x.fmax = 0.f;
            counted = eval_mask_point(a.bmin, a.bmax, a.close_distance, px, py, pz, gm, vb) != 0;
        }
        int cls = 5, bucket = 0, kind = 3;
        ull qs = 0, qe[R];
        bool ok[R], strict[R], relaxed[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { ok[r] = false; qe[r] = 0; strict[r] = false; relaxed[r] = false; }
        if (counted) {
            const double p[3] = {(double)px, (double)py, (double)pz};
            double gtd[3], g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gtd[c] = (double)gtf[c];
                g[c] = gtd[c] - pose_flow_f64(x, p, c, false);
            }
            const double speed = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
            cls = lut[cat];
            bucket = flow_bucket(speed, a.w);
            const bool dynamic = speed > a.dyn_thr;
            kind = cls != 0 ? (dynamic ? 0 : 1) : (dynamic ? 3 : 2);
            qs = (ull)llrint(speed * kFlowScale);
            double lim_strict = 0.0, lim_relaxed = 0.0;
            if (ACC) {
                const double gn = sqrt((gtd[0] * gtd[0] + gtd[1] * gtd[1]) + gtd[2] * gtd[2]);
                lim_strict = kFlowStrict * gn;
                lim_relaxed = kFlowRelaxed * gn;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double d[3];
                bool finite = true;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    d[c] = a.est[r] ? (double)e[r][c] - (RESID ? g[c] : gtd[c]) : -g[c];
                    finite = finite && (a.est[r] == nullptr || isfinite(e[r][c]));
                }
                const double epe = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
                ok[r] = finite && epe < kFlowReject;
                qe[r] = ok[r] ? (ull)llrint(epe * kFlowScale) : 0ull;
                if (ACC) {
                    strict[r] = ok[r] && (epe < kFlowStrict || epe < lim_strict);
                    relaxed[r] = ok[r] && (epe < kFlowRelaxed || epe < lim_relaxed);
                }
            }
        }
        if (ACC) {                                                    // the wave's lanes counted by ballot, added by one lane
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int grp = 0; grp < 4; ++grp) {
                    const bool in = ok[r] && (grp == 0 || kind == grp - 1);
                    const ull n = __ballot(in);
                    if (n == 0) continue;                             // (wave-uniform)
                    const ull ns = __ballot(in && strict[r]), nr = __ballot(in && relaxed[r]);
                    if (lane == 0) {
                        ull* word = s_acc + (r * 4 + grp) * 3;
                        atomicAdd(word, (ull)__popcll(n));
                        if (ns != 0) atomicAdd(word + 1, (ull)__popcll(ns));
                        if (nr != 0) atomicAdd(word + 2, (ull)__popcll(nr));
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const ull rej = __ballot(counted && !ok[r]);
            if (rej != 0 && lane == 0) atomicAdd(&s_rej[r], (ull)__popcll(rej));
        }
        wave_accumulate<R, true>(counted && cls < HIMO_FLOWM_CLASSES, cls * HIMO_FLOWM_BUCKETS + bucket, ok, qe, qs,
                                 [&](int key, int r, ull n, ull se, ull ss) {
                                     ull* word = s_bins + ((size_t)r * kFlowBins + key) * 3;
                                     atomicAdd(word, n);
                                     atomicAdd(word + 1, se);
                                     atomicAdd(word + 2, ss);
                                 });
        wave_accumulate<R, false>(counted && kind < 3, f * 4 + kind, ok, qe, qs,
                                  [&](int key, int r, ull n, ull se, ull) {
                                      const int fk = key >> 2, at = r * 6 + (key & 3) * 2;
                                      if (fk == fcur) {
                                          atomicAdd(&s_tw[at], n);
                                          atomicAdd(&s_tw[at + 1], se);
                                      } else {
                                          ull* word = a.threeway + (size_t)fk * (R * 6) + at;
                                          atomicAdd(word, n);
                                          atomicAdd(word + 1, se);
                                      }
                                  });
    }
    __syncthreads();
    if (fcur >= 0 && tid < R * 6) {
        const ull v = s_tw[tid];
        if (v != 0) atomicAdd(a.threeway + (size_t)fcur * (R * 6) + tid, v);
    }
    if (tid < R && s_rej[tid] != 0) atomicAdd(a.rejected + tid, s_rej[tid]);
    if constexpr (ACC) {
        if (a.accuracy && tid < R * kFlowAccWords) {
            const ull v = s_acc[tid];
            if (v != 0) atomicAdd(a.accuracy + tid, v);
        }
    }
    for (int k = tid; k < R * kFlowBins * 3; k += kFlowThreads) {
        const ull v = s_bins[k];
        if (v != 0) atomicAdd(a.buckets + k, v);
    }
}

template <int R>
static void launch_flowm(const FlowmArgsEx& a, bool acc, bool resid, unsigned blocks, hipStream_t s) {
    const dim3 g(blocks), b(kFlowThreads);
    if (acc && resid) hipLaunchKernelGGL((flow_metrics_kernel<R, true, true>), g, b, 0, s, a);
    else if (acc) hipLaunchKernelGGL((flow_metrics_kernel<R, true, false>), g, b, 0, s, a);
    else if (resid) hipLaunchKernelGGL((flow_metrics_kernel<R, false, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((flow_metrics_kernel<R, false, false>), g, b, 0, s, static_cast<const FlowmArgs&>(a));
}

}  // namespace himo

using namespace himo;

extern "C" size_t himo_flow_metrics_workspace_bytes(int n_frames) {
    if (n_frames < 1) n_frames = 1;
    return keys_bytes(n_frames) + (size_t)n_frames * sizeof(FrameXf);
}

extern "C" int himo_flow_metrics_batch_ex(int n_frames, int64_t total_points, const int64_t* d_offsets, const double* d_pose0,
                                          const double* d_pose1, const float* d_pc0, int pc_stride, const float* d_gt,
                                          const float* const* h_est, int n_results, int est_stride, const uint8_t* d_category,
                                          const uint8_t* d_ground, const uint8_t* d_valid, const uint8_t* h_class_lut,
                                          double sensor_dt, unsigned flags, int64_t* d_buckets, int64_t* d_threeway,
                                          int64_t* d_rejected, int64_t* d_accuracy, void* d_workspace, void* stream) {
    if (est_stride < 3) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_frames < 1 || total_points < 0 || total_points > (int64_t)0x7fffffff || pc_stride < 3) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_results < 1 || n_results > HIMO_FLOWM_MAX_RESULTS || !h_est || !h_class_lut) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_offsets || !d_pose0 || !d_buckets || !d_threeway || !d_rejected || !d_workspace) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_pose1 && !(flags & HIMO_FLAG_POSE_IS_EGO)) return HIMO_ERR_INVALID_ARGUMENT;
    if (!(sensor_dt > 0.0)) return HIMO_ERR_INVALID_ARGUMENT;
    FlowmArgsEx a{};
    for (int k = 0; k < 256; ++k) {
        if (h_class_lut[k] > HIMO_FLOWM_CLASSES) return HIMO_ERR_INVALID_ARGUMENT;
        a.lut[k >> 2] |= (unsigned)h_class_lut[k] << (8 * (k & 3));
    }
    if (total_points == 0) return HIMO_OK;
    if (!d_pc0 || !d_gt || !d_category || !d_ground) return HIMO_ERR_INVALID_ARGUMENT;
    if ((flags & HIMO_FLAG_SCANIA) && !d_valid) return HIMO_ERR_INVALID_ARGUMENT;
    if (!aligned16(d_workspace)) return HIMO_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    {   // the per-sweep transforms: compdis.hip's prep with no points to take a maximum over (it reads no lidar_dt then)
        int st = launch_frame_prep(n_frames, 0, d_offsets, d_pose0, d_pose1, flags, nullptr, d_workspace, s);
        if (st != HIMO_OK) return st;
    }
    a.n_frames = n_frames; a.pc_stride = pc_stride; a.total = total_points;
    a.offsets = d_offsets; a.xf = carve(d_workspace, n_frames).xf;
    a.pc0 = d_pc0; a.gt = d_gt;
    for (int r = 0; r < n_results; ++r) a.est[r] = h_est[r];
    a.est_stride = est_stride;
    a.accuracy = reinterpret_cast<ull*>(d_accuracy);
    // the v1 instantiation reads rows of 3 floats: other pitches go through the accuracy instantiation, which writes no table
    // without d_accuracy
    const bool resid = (flags & HIMO_FLAG_EST_RESIDUAL) != 0, acc = d_accuracy != nullptr || (!resid && est_stride != 3);
    a.category = d_category; a.ground = d_ground;
    a.valid = (flags & HIMO_FLAG_SCANIA) ? d_valid : nullptr;          // eval.py:293-296, as himo_compdis_batch
    a.dyn_thr = 0.5 * sensor_dt;
    a.w = 0.4 * sensor_dt;
    // the evaluation mask's bounds, as himo_amd/compdis.py hands them to the comp_dis kernel per data set
    const bool scania = (flags & HIMO_FLAG_SCANIA) != 0;
    const double lo[2][3] = {{-1.5, -1.5, -2.0}, {-9.5, -3.0 / 2, 0.0}}, hi[2][3] = {{1.5, 1.5, 2.0}, {5.0, 2.760004 / 2, 5.0}};
    for (int c = 0; c < 3; ++c) { a.bmin[c] = (float)lo[scania][c]; a.bmax[c] = (float)hi[scania][c]; }
    a.close_distance = 35.0f;
    a.buckets = reinterpret_cast<ull*>(d_buckets);
    a.threeway = reinterpret_cast<ull*>(d_threeway);
    a.rejected = reinterpret_cast<ull*>(d_rejected);

    int64_t blocks = (total_points + kFlowThreads - 1) / kFlowThreads;
    blocks = blocks > kFlowMaxBlocks ? kFlowMaxBlocks : blocks;
    a.chunk = ((total_points + blocks - 1) / blocks + kFlowThreads - 1) / kFlowThreads * kFlowThreads;
    {
        ProfScope ps("flow_metrics_kernel", s);
        switch (n_results) {
            case 1: launch_flowm<1>(a, acc, resid, (unsigned)blocks, s); break;
            case 2: launch_flowm<2>(a, acc, resid, (unsigned)blocks, s); break;
            case 3: launch_flowm<3>(a, acc, resid, (unsigned)blocks, s); break;
            case 4: launch_flowm<4>(a, acc, resid, (unsigned)blocks, s); break;
            case 5: launch_flowm<5>(a, acc, resid, (unsigned)blocks, s); break;
            case 6: launch_flowm<6>(a, acc, resid, (unsigned)blocks, s); break;
            case 7: launch_flowm<7>(a, acc, resid, (unsigned)blocks, s); break;
            default: launch_flowm<8>(a, acc, resid, (unsigned)blocks, s); break;
        }
    }
    HIMO_LAUNCH_CHECK("flow_metrics_kernel");
    return HIMO_OK;
}

extern "C" int himo_flow_metrics_batch(int n_frames, int64_t total_points, const int64_t* d_offsets, const double* d_pose0,
                                       const double* d_pose1, const float* d_pc0, int pc_stride, const float* d_gt,
                                       const float* const* h_est, int n_results, const uint8_t* d_category,
                                       const uint8_t* d_ground, const uint8_t* d_valid, const uint8_t* h_class_lut,
                                       double sensor_dt, unsigned flags, int64_t* d_buckets, int64_t* d_threeway,
                                       int64_t* d_rejected, void* d_workspace, void* stream) {
    return himo_flow_metrics_batch_ex(n_frames, total_points, d_offsets, d_pose0, d_pose1, d_pc0, pc_stride, d_gt, h_est, n_results, 3,
                                      d_category, d_ground, d_valid, h_class_lut, sensor_dt, flags & ~HIMO_FLAG_EST_RESIDUAL, d_buckets,
                                      d_threeway, d_rejected, nullptr, d_workspace, stream);
}
