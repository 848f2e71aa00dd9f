// boxlabel.hip -- the labelling step of the Scania extractor (dataprocess/extract_sca.py:95-145) for gfx950.
//
//   pc (T,4) + per-sweep ego1_SE3_ego0 + per-sweep box rows  ->  flow (T,3) f32, flow_is_valid u8, category u8, instance u32
//
// What it replaces: the float64 pose flow of :97, the `mmcv.ops.points_in_boxes_part` call of :117 on double tensors (the one
// device call the reference makes in-tree), the object flow / validity of :120-134 and the class / instance columns of :137-140.
// The pose flow is compdis_math.h's chain (pose_flow_f64, the expression save_zip.py:116 shares with :97); membership is
//     outside if fabs(z - cz_centre) > hz;   local_x = sx*cosa + sy*(-sina), local_y = sx*sina + sy*cosa  (sx = x - cx, sy = y - cy)
//     inside iff local_x > -hx && local_x < hx && local_y > -hy && local_y < hy;   the FIRST box in list order wins
// with cz_centre, the half sizes, cosa = cos(-rz) and sina = sin(-rz) prepared by the host, so no device transcendental takes part in
// a decision.  Built with -ffp-contract=off like compdis.hip: a contracted local_x would round once instead of twice.
// (Parity of this rule with mmcv's own kernel is NOT pinned -- mmcv is not available to the project)
//
// Work split: as compdis_kernel, a block owns 1024 consecutive points of the ragged batch (4 consecutive points per lane: the xyzi
// rows come in as four 16-byte loads, flow leaves as three 16-byte stores, the two byte columns as one 4-byte store each, the
// instance ids as one 16-byte store) and finds its sweep once with a wave-uniform search.  A block inside one sweep stages that
// sweep's box geometry (8 doubles a box) through LDS in chunks of 256 boxes, so any box count works; every lane reads the same LDS
// row at a time (a broadcast).  Per box the z test comes first and the rotation is skipped when no lane of the wave passes it; lanes
// whose point already has its box are masked, not branched; a wave leaves the box loop once all its points have a box (ballot).
// Blocks that straddle a sweep boundary take one point at a time and read the box rows from global memory.
//
// Bounds: 34 B/point of HBM traffic (16 read, 12 + 1 + 1 + 4 written) against up to ~15 float64 operations per (point, box)
// pair (4 for the z test; 11 more where a lane of the wave passes it).
//
// MEASURED (profiles/extract_sca.txt; MI355X, 32 sweeps x 120 000 points per launch): 71 / 357 / 1301 us at 16 / 128 / 512 boxes
// per sweep -- linear in the box count, 2.5 us per box, over a 31 us intercept that is the 34 B/point pass at 4.2 TB/s.  So the
// BOX LOOP bounds all three: at 16 boxes the kernel moves its bytes at 1.8 - 2.2 TB/s, 0.31 - 0.38 of compdis_gt_kernel's rate on
// the same points (5.86 TB/s), at 128 and 512 boxes at 6 % and 1.7 % of it.  The loop runs 1.5 T (point, box) pairs/s, held there
// by its per-box fixed cost per wave (LDS row read and wait, ballot branch per point of the lane), not by float64 throughput;
// nothing was tuned after the measurement.
#include "compdis_math.h"

namespace himo {

constexpr int kBoxChunk = 256;          // boxes staged per round: 256 x 64 B = 16 KB of LDS
constexpr int kGeom = 8;                // cx cy cz_centre hx hy hz cosa sina

struct BoxLabelArgs {
    int n_frames;
    int64_t total;
    const int64_t* offsets;
    const double* xf;                   // [F][3][4] rows of ego1_SE3_ego0
    const float* pc;                    // [T][4]
    const int* box_offsets;             // [F+1]
    const double* geom;                 // [B][8]
    const float* obj_flow;              // [B][3]
    const uint8_t* box_class;           // [B]
    const uint8_t* vel_finite;          // [B]
    uint8_t background;
    float* flow;                        // [T][3]
    uint8_t* valid;                     // [T]
    uint8_t* category;                  // [T]
    uint32_t* instance;                 // [T]
};

__device__ inline XfRegs load_xf34(const double* __restrict__ xf, int f) {
    XfRegs x;
    const double* e = xf + 12 * (size_t)f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) x.R[r * 3 + c] = e[r * 4 + c];
        x.t[r] = e[r * 4 + 3];
    }
    x.fmax = 0.f;
    return x;
}

// the membership rule for one (point, box row) pair; g = the row's 8 doubles
__device__ inline bool z_inside(const double* g, double z) { return !(fabs(z - g[2]) > g[5]); }

__device__ inline bool xy_inside(const double* g, double x, double y) {
    const double sx = x - g[0], sy = y - g[1];
    const double lx = sx * g[6] + sy * (-g[7]);
    const double ly = sx * g[7] + sy * g[6];
    return (lx > -g[3]) & (lx < g[3]) & (ly > -g[4]) & (ly < g[4]);
}

struct PointOut {
    float fl[3];
    uint8_t valid, cat;
    uint32_t inst;
};

// everything after the membership decision: hit = box index within the sweep or -1 (extract_sca.py:97, :120-140)
__device__ inline PointOut finish_point(const BoxLabelArgs& a, const XfRegs& x, int box0, float px, float py, float pz, int hit,
                                        bool single_row) {
    const double p[3] = {(double)px, (double)py, (double)pz};
    PointOut o;
    const int64_t b = (int64_t)box0 + (hit < 0 ? 0 : hit);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double pf = pose_flow_f64(x, p, c, single_row);
        if (hit >= 0) pf = pf + (double)a.obj_flow[b * 3 + c];          // :134 float64 += float32
        o.fl[c] = (float)pf;                                            // :85
    }
    o.valid = hit >= 0 ? (uint8_t)(a.vel_finite[b] != 0) : (uint8_t)1;  // :125
    o.cat = hit >= 0 ? a.box_class[b] : a.background;                   // :137-139
    o.inst = (uint32_t)(hit + 1);                                       // :140
    return o;
}

__device__ inline void store_point(const BoxLabelArgs& a, int64_t i, const PointOut& o) {
    a.flow[i * 3] = o.fl[0]; a.flow[i * 3 + 1] = o.fl[1]; a.flow[i * 3 + 2] = o.fl[2];
    a.valid[i] = o.valid;
    a.category[i] = o.cat;
    a.instance[i] = o.inst;
}

// VEC: pc / flow / instance 16-byte aligned, valid / category 4-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kThreads) void box_label_kernel(BoxLabelArgs a) {
    __shared__ double s_geom[kBoxChunk * kGeom];
    const int64_t bstart = (int64_t)blockIdx.x * kBlockPts;
    const int64_t bend = bstart + kBlockPts < a.total ? bstart + kBlockPts : a.total;
    const int f0 = __builtin_amdgcn_readfirstlane(segment_of(a.offsets, a.n_frames, bstart));
    const bool uniform = a.offsets[f0 + 1] >= bend;
    const int64_t g = bstart + (int64_t)threadIdx.x * kPtsPerThread;

    if (!uniform) {
        // a sweep boundary inside the block: one point at a time, the sweep looked up as the rows go by, box rows from global memory
        int f = f0;
        for (int64_t i = g; i < g + kPtsPerThread && i < bend; ++i) {
            while (i >= a.offsets[f + 1]) ++f;
            const XfRegs x = load_xf34(a.xf, f);
            const int box0 = a.box_offsets[f], nb = a.box_offsets[f + 1] - box0;
            const float* p = a.pc + i * 4;
            const float px = p[0], py = p[1], pz = p[2];
            int hit = -1;
            for (int b = 0; b < nb && hit < 0; ++b) {
                const double* row = a.geom + ((int64_t)box0 + b) * kGeom;
                double r[kGeom];
#pragma unroll
                for (int k = 0; k < kGeom; ++k) r[k] = row[k];
                if (z_inside(r, (double)pz) && xy_inside(r, (double)px, (double)py)) hit = b;
            }
            store_point(a, i, finish_point(a, x, box0, px, py, pz, hit, a.offsets[f + 1] - a.offsets[f] == 1));
        }
        return;
    }

    // the whole block lies in sweep f0: every thread helps staging, lanes past the block's end carry no point
    const XfRegs x = load_xf34(a.xf, f0);
    const int box0 = a.box_offsets[f0], nb = a.box_offsets[f0 + 1] - box0;
    const bool single_row = a.offsets[f0 + 1] - a.offsets[f0] == 1;
    const int nvalid = g >= bend ? 0 : (bend - g < kPtsPerThread ? (int)(bend - g) : kPtsPerThread);
    const bool full = VEC && nvalid == kPtsPerThread;

    float px[4] = {0.f, 0.f, 0.f, 0.f}, py[4] = {0.f, 0.f, 0.f, 0.f}, pz[4] = {0.f, 0.f, 0.f, 0.f};
    if (full) {
        const float4* src = reinterpret_cast<const float4*>(a.pc) + g;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float4 v = src[k]; px[k] = v.x; py[k] = v.y; pz[k] = v.z; }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nvalid) { const float* p = a.pc + (g + k) * 4; px[k] = p[0]; py[k] = p[1]; pz[k] = p[2]; }
    }
    int hit[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) hit[k] = k < nvalid ? -1 : 0;            // (a lane's missing points count as settled)
    double dx[4], dy[4], dz[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { dx[k] = (double)px[k]; dy[k] = (double)py[k]; dz[k] = (double)pz[k]; }

    bool open = __ballot((hit[0] < 0) | (hit[1] < 0) | (hit[2] < 0) | (hit[3] < 0)) != 0;       // wave-uniform
    for (int c0 = 0; c0 < nb; c0 += kBoxChunk) {
        const int nc = nb - c0 < kBoxChunk ? nb - c0 : kBoxChunk;
        __syncthreads();                                                 // the previous chunk is no longer read
        for (int e = threadIdx.x; e < nc * kGeom; e += kThreads) s_geom[e] = a.geom[((int64_t)box0 + c0) * kGeom + e];
        __syncthreads();
        for (int b = 0; b < nc && open; ++b) {
            const double* row = s_geom + b * kGeom;
            double r[kGeom];
#pragma unroll
            for (int k = 0; k < kGeom; ++k) r[k] = row[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool cand = (hit[k] < 0) & z_inside(r, dz[k]);
                if (__ballot(cand) != 0) {
                    const bool in = cand & xy_inside(r, dx[k], dy[k]);
                    hit[k] = in ? c0 + b : hit[k];
                }
            }
            open = __ballot((hit[0] < 0) | (hit[1] < 0) | (hit[2] < 0) | (hit[3] < 0)) != 0;
        }
    }
    if (nvalid == 0) return;

    PointOut o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < nvalid) o[k] = finish_point(a, x, box0, px[k], py[k], pz[k], hit[k], single_row);
    if (full) {
        float4* dst = reinterpret_cast<float4*>(a.flow + g * 3);
        dst[0] = make_float4(o[0].fl[0], o[0].fl[1], o[0].fl[2], o[1].fl[0]);
        dst[1] = make_float4(o[1].fl[1], o[1].fl[2], o[2].fl[0], o[2].fl[1]);
        dst[2] = make_float4(o[2].fl[2], o[3].fl[0], o[3].fl[1], o[3].fl[2]);
        *reinterpret_cast<uchar4*>(a.valid + g) = make_uchar4(o[0].valid, o[1].valid, o[2].valid, o[3].valid);
        *reinterpret_cast<uchar4*>(a.category + g) = make_uchar4(o[0].cat, o[1].cat, o[2].cat, o[3].cat);
        *reinterpret_cast<uint4*>(a.instance + g) = make_uint4(o[0].inst, o[1].inst, o[2].inst, o[3].inst);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nvalid) store_point(a, g + k, o[k]);
    }
}

}  // namespace himo

using namespace himo;

extern "C" int himo_box_label_batch(int n_frames, int64_t total_points, const int64_t* h_offsets, const int64_t* d_offsets,
                                    const double* d_ego1_SE3_ego0, const float* d_pc, int n_boxes, const int* h_box_offsets,
                                    const int* d_box_offsets, const double* d_box_geom, const float* d_box_flow,
                                    const uint8_t* d_box_class, const uint8_t* d_box_vel_finite, int background_class,
                                    float* d_flow, uint8_t* d_flow_is_valid, uint8_t* d_category, uint32_t* d_instance,
                                    void* stream) {
    if (n_frames < 1 || total_points < 0 || n_boxes < 0 || background_class < 0 || background_class > 255)
        return HIMO_ERR_INVALID_ARGUMENT;
    if (!h_offsets || !d_offsets || !d_ego1_SE3_ego0 || !h_box_offsets || !d_box_offsets) return HIMO_ERR_INVALID_ARGUMENT;
    if (h_offsets[0] != 0 || h_offsets[n_frames] != total_points) return HIMO_ERR_INVALID_ARGUMENT;
    if (h_box_offsets[0] != 0 || h_box_offsets[n_frames] != n_boxes) return HIMO_ERR_INVALID_ARGUMENT;
    for (int f = 0; f < n_frames; ++f) {
        if (h_offsets[f] < 0 || h_offsets[f + 1] < h_offsets[f]) return HIMO_ERR_INVALID_ARGUMENT;
        if (h_box_offsets[f] < 0 || h_box_offsets[f + 1] < h_box_offsets[f]) return HIMO_ERR_INVALID_ARGUMENT;
    }
    if (n_boxes > 0 && (!d_box_geom || !d_box_flow || !d_box_class || !d_box_vel_finite)) return HIMO_ERR_INVALID_ARGUMENT;
    if (total_points > 0 && (!d_pc || !d_flow || !d_flow_is_valid || !d_category || !d_instance)) return HIMO_ERR_INVALID_ARGUMENT;
    auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (misaligned(d_pc, 4) || misaligned(d_flow, 4) || misaligned(d_instance, 4) || misaligned(d_box_geom, 8) ||
        misaligned(d_ego1_SE3_ego0, 8) || misaligned(d_box_flow, 4))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (total_points == 0) return HIMO_OK;

    BoxLabelArgs a;
    a.n_frames = n_frames; a.total = total_points; a.offsets = d_offsets; a.xf = d_ego1_SE3_ego0; a.pc = d_pc;
    a.box_offsets = d_box_offsets; a.geom = d_box_geom; a.obj_flow = d_box_flow; a.box_class = d_box_class;
    a.vel_finite = d_box_vel_finite; a.background = (uint8_t)background_class;
    a.flow = d_flow; a.valid = d_flow_is_valid; a.category = d_category; a.instance = d_instance;

    const bool vec = aligned16(d_pc) && aligned16(d_flow) && aligned16(d_instance) && !misaligned(d_flow_is_valid, 4) &&
                     !misaligned(d_category, 4);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((total_points + kBlockPts - 1) / kBlockPts)), block(kThreads);
    {
        ProfScope ps("box_label_kernel", s);
        if (vec) hipLaunchKernelGGL((box_label_kernel<true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((box_label_kernel<false>), grid, block, 0, s, a);
    }
    HIMO_LAUNCH_CHECK("box_label_kernel");
    return HIMO_OK;
}
