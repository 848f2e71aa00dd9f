// compdis_gt.hip -- the ground-truth sweep writer's device half (tools/test/save_zip_gt.py:141-178) for gfx950.
//
//   flow + pc0 + lidar_dt + poses + gm0 [+ flow_is_valid] [+ labels]  ->  the BODY of one Arrow record batch per sweep
//
// The arithmetic is compdis.hip's (point_math / eval_mask_point of compdis_math.h, after the same frame_prep_kernel launch);
// what this kernel adds is the per-point norm of the compensated flow, the pass-through columns and the layout: ten columns
// per sweep, each starting at a multiple of 8 bytes inside that sweep's body, pad bytes zero (gt_layout below; the host builds
// the Feather framing around it from the schema and the row count alone).  About 39 bytes in and 34 out per point.
//
// Work split: as compdis_kernel, a block owns 1024 consecutive points of the ragged batch and finds its sweep once with a
// wave-uniform search.  Inside a block that lies in one sweep the lanes take groups of four points aligned to the SWEEP's row
// index (not the batch's), so that every float column moves as one 16-byte store at an 8-byte aligned address and the four
// uint8 values of a group as one 4-byte store; the loads on the other side are then only 4-byte aligned (multi-dword global
// accesses need no more than that).  The group cut by the block's edge, the sweep's tail of n % 4 rows and blocks that
// straddle sweeps go one point at a time; the lane that writes a sweep's last row also zeroes the pad bytes of its columns.
//
// Compiled with -ffp-contract=off like compdis.hip: every fused multiply-add of the chain is explicit.
#include "compdis_math.h"

namespace himo {

constexpr int kGtCd = 0, kGtMask = 3, kGtCat = 4, kGtInst = 5, kGtNorm = 6, kGtPc = 7;

__host__ __device__ inline int64_t pad8(int64_t bytes) { return (bytes + 7) & ~(int64_t)7; }

// byte offset of every column inside a sweep's body (-1: absent) and the body's size
struct GtLayout {
    int64_t start[HIMO_GT_MAX_COLUMNS];
    int64_t bytes;
};

__host__ __device__ inline GtLayout gt_layout(int64_t n, unsigned columns) {
    const int64_t w4 = pad8(4 * n), w1 = pad8(n);
    GtLayout l;
    int64_t at = 0;
#pragma unroll
    for (int c = 0; c < HIMO_GT_MAX_COLUMNS; ++c) {
        const bool one_byte = c == kGtMask || c == kGtCat;
        const bool present = (c != kGtCat || (columns & HIMO_GT_HAS_CATEGORY)) && (c != kGtInst || (columns & HIMO_GT_HAS_INSTANCE));
        l.start[c] = present ? at : -1;
        if (present) at += one_byte ? w1 : w4;
    }
    l.bytes = at;
    return l;
}

struct GtArgs {
    int n_frames;
    int64_t total;
    const int64_t* offsets;
    const unsigned* keys;
    const FrameXf* xf;
    const float* pc0;
    int pc_stride;
    const float* flow;
    const float* lidar_dt;
    double sensor_dt;
    const uint8_t* gm0;
    const uint8_t* valid;        // may be nullptr
    const uint8_t* category;     // nullptr <=> no such column
    const uint32_t* instance;    // nullptr <=> no such column
    float bmin[3], bmax[3];
    float close_distance;
    const int64_t* body_offsets;
    uint8_t* body;
};

// where one sweep's columns start, and which rows of the batch it owns
struct SweepCols {
    int64_t first, n;            // rows [first, first + n) of the batch
    float* cd[3];
    uint8_t* mask;
    uint8_t* cat;
    uint32_t* inst;
    float* norm;
    float* pc[3];
};

__device__ inline SweepCols sweep_cols(const GtArgs& a, int f) {
    SweepCols s;
    s.first = a.offsets[f];
    s.n = a.offsets[f + 1] - s.first;
    const unsigned columns = (a.category ? HIMO_GT_HAS_CATEGORY : 0u) | (a.instance ? HIMO_GT_HAS_INSTANCE : 0u);
    const GtLayout l = gt_layout(s.n, columns);
    uint8_t* base = a.body + a.body_offsets[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.cd[c] = reinterpret_cast<float*>(base + l.start[kGtCd + c]);
        s.pc[c] = reinterpret_cast<float*>(base + l.start[kGtPc + c]);
    }
    s.mask = base + l.start[kGtMask];
    s.cat = a.category ? base + l.start[kGtCat] : nullptr;
    s.inst = a.instance ? reinterpret_cast<uint32_t*>(base + l.start[kGtInst]) : nullptr;
    s.norm = reinterpret_cast<float*>(base + l.start[kGtNorm]);
    return s;
}

// the pad bytes after row n - 1 of every column: 4 bytes of a 4-byte column when n is odd, (-n) % 8 bytes of a 1-byte column
__device__ inline void zero_pads(const SweepCols& s) {
    if (s.n & 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s.cd[c][s.n] = 0.f; s.pc[c][s.n] = 0.f; }
        s.norm[s.n] = 0.f;
        if (s.inst) s.inst[s.n] = 0u;
    }
    for (int64_t k = s.n; k < pad8(s.n); ++k) {
        s.mask[k] = 0;
        if (s.cat) s.cat[k] = 0;
    }
}

template <bool F32>
__device__ inline void gt_point(const GtArgs& a, const XfRegs& x, const SweepCols& s, int64_t i) {
    const float* p = a.pc0 + i * (int64_t)a.pc_stride;
    const float px = p[0], py = p[1], pz = p[2];
    float cd[3], rf[3], nrm;
    point_math<F32, true>(x, px, py, pz, a.flow[i * 3], a.flow[i * 3 + 1], a.flow[i * 3 + 2], a.lidar_dt[i], a.sensor_dt,
                           false, cd, rf, &nrm, s.n == 1);
    const int64_t j = i - s.first;
    s.cd[0][j] = cd[0]; s.cd[1][j] = cd[1]; s.cd[2][j] = cd[2];
    s.mask[j] = eval_mask_point(a.bmin, a.bmax, a.close_distance, px, py, pz, a.gm0[i], a.valid ? a.valid[i] : (uint8_t)1);
    if (s.cat) s.cat[j] = a.category[i];
    if (s.inst) s.inst[j] = a.instance[i];
    s.norm[j] = nrm;
    s.pc[0][j] = px; s.pc[1][j] = py; s.pc[2][j] = pz;
    if (j == s.n - 1) zero_pads(s);
}

// four-element vectors at less than their natural alignment: a multi-dword global access needs 4-byte alignment only
typedef float f4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float f4_a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef unsigned u4_a8 __attribute__((ext_vector_type(4), aligned(8)));

__device__ inline unsigned pack4(uint8_t b0, uint8_t b1, uint8_t b2, uint8_t b3) {
    return (unsigned)b0 | ((unsigned)b1 << 8) | ((unsigned)b2 << 16) | ((unsigned)b3 << 24);
}

// rows [4q, 4q + 4) of the sweep, cut to the block's rows [lo, hi) of it
template <int STRIDE, bool F32>
__device__ inline void gt_group(const GtArgs& a, const XfRegs& x, const SweepCols& s, int64_t q, int64_t lo, int64_t hi) {
    const int64_t j0 = q * 4;
    const int64_t jb = j0 > lo ? j0 : lo, je = j0 + 4 < hi ? j0 + 4 : hi;
    if (jb >= je) return;
    if (je - jb < 4) {
        for (int64_t j = jb; j < je; ++j) gt_point<F32>(a, x, s, s.first + j);
        return;
    }
    const int64_t i0 = s.first + j0;
    float px[4], py[4], pz[4];
    if (STRIDE == 4) {
        const float4* src = reinterpret_cast<const float4*>(a.pc0) + i0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float4 v = src[k]; px[k] = v.x; py[k] = v.y; pz[k] = v.z; }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* p = a.pc0 + (i0 + k) * (int64_t)a.pc_stride;
            px[k] = p[0]; py[k] = p[1]; pz[k] = p[2];
        }
    }
    const f4_a4* fsrc = reinterpret_cast<const f4_a4*>(a.flow + i0 * 3);
    const f4_a4 v0 = fsrc[0], v1 = fsrc[1], v2 = fsrc[2];
    const float fl[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
    const f4_a4 dtv = *reinterpret_cast<const f4_a4*>(a.lidar_dt + i0);
    const float dt[4] = {dtv.x, dtv.y, dtv.z, dtv.w};

    float cd[12], rf[3], nrm[4];
    uint8_t m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        point_math<F32, true>(x, px[k], py[k], pz[k], fl[3 * k], fl[3 * k + 1], fl[3 * k + 2], dt[k], a.sensor_dt, false,
                               cd + 3 * k, rf, nrm + k);
        m[k] = eval_mask_point(a.bmin, a.bmax, a.close_distance, px[k], py[k], pz[k], a.gm0[i0 + k],
                               a.valid ? a.valid[i0 + k] : (uint8_t)1);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f4_a8 v = {cd[c], cd[3 + c], cd[6 + c], cd[9 + c]};
        *reinterpret_cast<f4_a8*>(s.cd[c] + j0) = v;
    }
    *reinterpret_cast<unsigned*>(s.mask + j0) = pack4(m[0], m[1], m[2], m[3]);
    if (s.cat) {
        const uint8_t* c = a.category + i0;
        *reinterpret_cast<unsigned*>(s.cat + j0) = pack4(c[0], c[1], c[2], c[3]);
    }
    if (s.inst) *reinterpret_cast<u4_a8*>(s.inst + j0) = *reinterpret_cast<const u4_a4*>(a.instance + i0);
    { f4_a8 v = {nrm[0], nrm[1], nrm[2], nrm[3]}; *reinterpret_cast<f4_a8*>(s.norm + j0) = v; }
    { f4_a8 v = {px[0], px[1], px[2], px[3]}; *reinterpret_cast<f4_a8*>(s.pc[0] + j0) = v; }
    { f4_a8 v = {py[0], py[1], py[2], py[3]}; *reinterpret_cast<f4_a8*>(s.pc[1] + j0) = v; }
    { f4_a8 v = {pz[0], pz[1], pz[2], pz[3]}; *reinterpret_cast<f4_a8*>(s.pc[2] + j0) = v; }
    if (j0 + 4 == s.n) zero_pads(s);
}

// STRIDE = 4: xyzi rows at 16-byte aligned addresses; STRIDE = 0: any row stride / alignment
template <int STRIDE, bool F32>
__global__ __launch_bounds__(kThreads) void compdis_gt_kernel(GtArgs a) {
    const int64_t bstart = (int64_t)blockIdx.x * kBlockPts;
    const int64_t bend = bstart + kBlockPts < a.total ? bstart + kBlockPts : a.total;
    const int f0 = __builtin_amdgcn_readfirstlane(segment_of(a.offsets, a.n_frames, bstart));
    const bool uniform = a.offsets[f0 + 1] >= bend;

    if (!uniform) {
        // a sweep boundary inside the block: one point at a time, the sweep looked up as the rows go by
        const int64_t g = bstart + (int64_t)threadIdx.x * kPtsPerThread;
        int f = f0, have = -1;
        SweepCols s;
        XfRegs x;
        for (int64_t i = g; i < g + kPtsPerThread && i < bend; ++i) {
            while (i >= a.offsets[f + 1]) ++f;
            if (f != have) { s = sweep_cols(a, f); x = load_xf(a.xf, a.keys, f); have = f; }
            gt_point<F32>(a, x, s, i);
        }
        return;
    }

    const SweepCols s = sweep_cols(a, f0);
    const XfRegs x = load_xf(a.xf, a.keys, f0);
    const int64_t lo = bstart - s.first, hi = bend - s.first;       // the block's rows of the sweep
    const int64_t q0 = lo >> 2;
    gt_group<STRIDE, F32>(a, x, s, q0 + threadIdx.x, lo, hi);
    // 1024 rows that do not start on a group boundary touch 257 groups: the last, cut, one goes to lane 0
    if (threadIdx.x == 0) gt_group<STRIDE, F32>(a, x, s, q0 + kThreads, lo, hi);
}

}  // namespace himo

using namespace himo;

extern "C" size_t himo_gt_body_bytes(int64_t n_points, unsigned columns) {
    return n_points > 0 ? (size_t)gt_layout(n_points, columns).bytes : 0;
}

extern "C" size_t himo_gt_column_starts(int64_t n_points, unsigned columns, int64_t* h_starts) {
    const GtLayout l = gt_layout(n_points > 0 ? n_points : 0, columns);
    if (h_starts)
        for (int c = 0; c < HIMO_GT_MAX_COLUMNS; ++c) h_starts[c] = l.start[c];
    return (size_t)l.bytes;
}

extern "C" int himo_compdis_gt_batch(int n_frames, int64_t total_points, const int64_t* d_offsets, const double* d_pose0,
                                     const double* d_pose1, const float* d_pc0, int pc_stride, const float* d_flow,
                                     const float* d_lidar_dt, double sensor_dt, unsigned flags, const uint8_t* d_gm0,
                                     const uint8_t* d_flow_is_valid, const uint8_t* d_category, const uint32_t* d_instance,
                                     unsigned columns, const float* h_mask_bounds, float close_distance,
                                     const int64_t* d_body_offsets, uint8_t* d_body, void* d_workspace,
                                     size_t workspace_bytes, void* stream) {
    if (n_frames < 1 || total_points < 0 || pc_stride < 3) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_offsets || !d_pose0 || !d_workspace || !h_mask_bounds || !d_body_offsets) return HIMO_ERR_INVALID_ARGUMENT;
    if (!d_pose1 && !(flags & HIMO_FLAG_POSE_IS_EGO)) return HIMO_ERR_INVALID_ARGUMENT;
    if (flags & HIMO_FLAG_RAW) return HIMO_ERR_INVALID_ARGUMENT;                       // save_zip_gt.py:167 reads data['flow']
    if (columns & ~(HIMO_GT_HAS_CATEGORY | HIMO_GT_HAS_INSTANCE)) return HIMO_ERR_INVALID_ARGUMENT;
    if (total_points > 0 && (!d_pc0 || !d_flow || !d_lidar_dt || !d_gm0 || !d_body)) return HIMO_ERR_INVALID_ARGUMENT;
    if (total_points > 0 && (columns & HIMO_GT_HAS_CATEGORY) && !d_category) return HIMO_ERR_INVALID_ARGUMENT;
    if (total_points > 0 && (columns & HIMO_GT_HAS_INSTANCE) && !d_instance) return HIMO_ERR_INVALID_ARGUMENT;
    if ((flags & HIMO_FLAG_SCANIA) && !d_flow_is_valid) return HIMO_ERR_INVALID_ARGUMENT;
    if (!(sensor_dt != 0.0)) return HIMO_ERR_INVALID_ARGUMENT;
    auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (misaligned(d_body, 8) || misaligned(d_pc0, 4) || misaligned(d_flow, 4) || misaligned(d_lidar_dt, 4) || misaligned(d_instance, 4))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < himo_compdis_workspace_bytes(n_frames) || !aligned16(d_workspace)) return HIMO_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;

    WorkspaceLayout w = carve(d_workspace, n_frames);
    {
        int st = launch_frame_prep(n_frames, total_points, d_offsets, d_pose0, d_pose1, flags, d_lidar_dt, d_workspace, s);
        if (st != HIMO_OK) return st;
    }
    if (total_points == 0) return HIMO_OK;

    GtArgs a;
    a.n_frames = n_frames; a.total = total_points; a.offsets = d_offsets; a.keys = w.keys; a.xf = w.xf;
    a.pc0 = d_pc0; a.pc_stride = pc_stride; a.flow = d_flow; a.lidar_dt = d_lidar_dt; a.sensor_dt = sensor_dt;
    a.gm0 = d_gm0; a.valid = (flags & HIMO_FLAG_SCANIA) ? d_flow_is_valid : nullptr;     // save_zip_gt.py:151-154
    a.category = (columns & HIMO_GT_HAS_CATEGORY) ? d_category : nullptr;
    a.instance = (columns & HIMO_GT_HAS_INSTANCE) ? d_instance : nullptr;
    for (int i = 0; i < 3; ++i) { a.bmin[i] = h_mask_bounds[i]; a.bmax[i] = h_mask_bounds[3 + i]; }
    a.close_distance = close_distance;
    a.body_offsets = d_body_offsets; a.body = d_body;

    const bool rows16 = pc_stride == 4 && aligned16(d_pc0);
    const bool f32 = (flags & HIMO_FLAG_F32_CHAIN) != 0;
    const dim3 grid((unsigned)((total_points + kBlockPts - 1) / kBlockPts)), block(kThreads);
#define HIMO_GO(S, F) hipLaunchKernelGGL((compdis_gt_kernel<S, F>), grid, block, 0, s, a)
    {
        ProfScope ps("compdis_gt_kernel", s);
        if (rows16) { if (f32) HIMO_GO(4, true); else HIMO_GO(4, false); }
        else { if (f32) HIMO_GO(0, true); else HIMO_GO(0, false); }
    }
#undef HIMO_GO
    HIMO_LAUNCH_CHECK("compdis_gt_kernel");
    return HIMO_OK;
}
