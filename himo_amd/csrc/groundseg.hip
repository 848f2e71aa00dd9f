// groundseg.hip -- the ground segmenter ("ray ground filter, v1"; the rule is the module docstring of himo_amd/ground_seg.py) for
// gfx950.  PARITY UNPINNED: the reference's own segmenter lives in its absent submodule; this stage is checked against the numpy
// restatement of the written rule (tests/groundseg_ref.py), which it equals bit for bit.
//
//   xyz (T, pitch) float32 of a packed, ragged batch of sweeps  ->  ground_mask uint8[T]  (+ the cells' ground heights)
//
// Three kernels over one workspace laid out [frame][bin][segment] (keys uint64, then heights float32):
//   ground_bin_kernel       every point computes its cell and offers (ordered bits of z) << 32 | point index to the cell's key with
//                           a 64-bit atomicMin: the minimum is the point of lowest z, the lowest index among equals.  Lanes of a
//                           wave that share a cell are reduced in the wave first (one atomic per distinct cell of the wave): near
//                           the sensor hundreds of points fall in one cell.
//   ground_walk_kernel      one thread per (frame, segment) walks the bins outwards in float64; adjacent lanes read adjacent keys.
//                           The keys and the prototypes' x, y are fetched kWalkChunk bins ahead of the serial slope test, so the
//                           dependent-load latency is paid once per chunk, not once per bin.
//   ground_classify_kernel  recomputes the cell per point (cheaper than 4 B/point of stored cell ids), reads the height, writes a byte.
//
// Built with -ffp-contract=off: x*x + y*y, (r - r_min) / bin_size, t * K and max_slope * (r - r_prev) + step_tol must round after every
// operation, as numpy does.  sqrtf and the float32 divisions are the correctly rounded ones (hipcc's default).  No transcendental
// takes part in a decision.
//
// Traffic: two reads of xyz and one byte written per point (25 B/point at pitch 3, 33 B/point at pitch 4), plus 12 B per CELL and
// sweep (key memset, key read, height write: 1.1 MB a sweep at the defaults) and one random 8-byte read per occupied cell.
#include "himo_common.h"
#include "blockops.h"
#include <math.h>

namespace himo {

constexpr int kGsThreads = 256;
constexpr int kGsPtsPerThread = 4;
constexpr int kGsBlockPts = kGsThreads * kGsPtsPerThread;
constexpr int kWalkChunk = 8;
constexpr unsigned long long kEmptyKey = ~0ull;

struct GroundArgs {
    int n_frames;
    int64_t total;
    const int64_t* offsets;
    const float* xyz;
    int pitch;
    himo_ground_params p;
    int S;                                  // segments: 8 K
    unsigned long long* keys;               // [F][n_bins][S]
    float* G;                               // [F][n_bins][S]
    float* G_out;                           // the caller's copy, or nullptr
    uint8_t* mask;
};

// rule A: the cell of a point inside its sweep's table, bin * S + segment, or -1 for an unbinned point
__device__ inline int cell_of(const himo_ground_params& p, int S, float x, float y, float z) {
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return -1;
    const float r = sqrtf(x * x + y * y);
    if (r < p.r_min) return -1;
    const float q = (r - p.r_min) / p.bin_size;
    if (!(q < (float)p.n_bins)) return -1;               // (int)q >= n_bins, and a range that overflowed to infinity
    const int b = (int)q;
    const float ax = fabsf(x), ay = fabsf(y);
    const bool steep = ay > ax;
    const float mx = steep ? ay : ax, mn = steep ? ax : ay;
    if (!(mx > 0.f)) return -1;                          // (cannot happen with r >= r_min > 0)
    const float t = mn / mx;
    int k = (int)(t * (float)p.K);
    k = k < p.K - 1 ? k : p.K - 1;
    // octants counted round the circle from +x towards +y; the table is indexed by (x<0) | (y<0)<<1 | (|y|>|x|)<<2
    const int oct = (0x56214730u >> (4 * ((x < 0.f ? 1 : 0) | (y < 0.f ? 2 : 0) | (steep ? 4 : 0)))) & 7;
    const int seg = oct * p.K + ((oct & 1) ? p.K - 1 - k : k);
    return b * S + seg;
}

__device__ inline void load_xyz(const float* __restrict__ xyz, int pitch, int64_t i, float& x, float& y, float& z) {
    const float* q = xyz + i * pitch;
    x = q[0]; y = q[1]; z = q[2];
}

// VEC4: pitch 4 and a 16-byte aligned base: one 16-byte load per point
template <bool VEC4>
__global__ __launch_bounds__(kGsThreads) void ground_bin_kernel(GroundArgs a) {
    const int64_t bstart = (int64_t)blockIdx.x * kGsBlockPts;
    const int64_t g = bstart + (int64_t)threadIdx.x * kGsPtsPerThread;
    int f = __builtin_amdgcn_readfirstlane(segment_of(a.offsets, a.n_frames, bstart));
    const int64_t cells = (int64_t)a.p.n_bins * a.S;
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int j = 0; j < kGsPtsPerThread; ++j) {
        const int64_t i = g + j;
        int64_t slot = -1;                               // the key this lane's point offers to, -1: none
        unsigned long long key = kEmptyKey;
        if (i < a.total) {
            while (i >= a.offsets[f + 1]) ++f;
            float x, y, z;
            if (VEC4) { const float4 v = reinterpret_cast<const float4*>(a.xyz)[i]; x = v.x; y = v.y; z = v.z; }
            else load_xyz(a.xyz, a.pitch, i, x, y, z);
            const int c = cell_of(a.p, a.S, x, y, z);
            if (c >= 0) {
                slot = (int64_t)f * cells + c;
                key = ((unsigned long long)float_to_key(z) << 32) | (unsigned)i;
            }
        }
        // one atomic per distinct cell of the wave
        bool pending = slot >= 0;
        while (true) {
            const unsigned long long todo = __ballot(pending);
            if (todo == 0) break;
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned s_lo = (unsigned)__shfl((int)(unsigned)slot, leader, 64);
            const unsigned s_hi = (unsigned)__shfl((int)(unsigned)((unsigned long long)slot >> 32), leader, 64);
            const int64_t s0 = (int64_t)(((unsigned long long)s_hi << 32) | s_lo);
            const bool mine = pending && slot == s0;
            const unsigned long long same = __ballot(mine);
            if (__popcll(same) == 1) {
                if (mine) atomicMin(a.keys + s0, key);
            } else {
                unsigned long long m = mine ? key : kEmptyKey;
#pragma unroll
                for (int w = 32; w >= 1; w >>= 1) {
                    const unsigned long long o = shfl_xor_u64(m, w);
                    m = o < m ? o : m;
                }
                if (lane == leader) atomicMin(a.keys + s0, m);
            }
            pending = pending && !mine;
        }
    }
}

// rule C.  One thread per (frame, segment); a sweep without points is left alone.
__global__ __launch_bounds__(kGsThreads) void ground_walk_kernel(GroundArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kGsThreads + threadIdx.x;
    if (t >= (int64_t)a.n_frames * a.S) return;
    const int f = (int)(t / a.S), seg = (int)(t % a.S);
    if (a.offsets[f + 1] <= a.offsets[f]) return;
    const int64_t base = (int64_t)f * a.p.n_bins * a.S + seg;
    const double slope = (double)a.p.max_slope, tol = (double)a.p.step_tol;
    double r_prev = 0.0;
    float g_prev = -a.p.sensor_height;
    for (int b0 = 0; b0 < a.p.n_bins; b0 += kWalkChunk) {
        unsigned long long key[kWalkChunk];
        float px[kWalkChunk], py[kWalkChunk];
#pragma unroll
        for (int u = 0; u < kWalkChunk; ++u)
            key[u] = b0 + u < a.p.n_bins ? a.keys[base + (int64_t)(b0 + u) * a.S] : kEmptyKey;
#pragma unroll
        for (int u = 0; u < kWalkChunk; ++u) {
            px[u] = 0.f; py[u] = 0.f;
            if (key[u] != kEmptyKey) {
                const float* q = a.xyz + (int64_t)(unsigned)key[u] * a.pitch;
                px[u] = q[0]; py[u] = q[1];
            }
        }
#pragma unroll
        for (int u = 0; u < kWalkChunk; ++u) {
            if (b0 + u >= a.p.n_bins) break;
            if (key[u] != kEmptyKey) {
                const float z = key_to_float((unsigned)(key[u] >> 32));
                const float r = sqrtf(px[u] * px[u] + py[u] * py[u]);
                if (fabs((double)z - (double)g_prev) <= slope * ((double)r - r_prev) + tol) {
                    g_prev = z;
                    r_prev = (double)r;
                }
            }
            const int64_t at = base + (int64_t)(b0 + u) * a.S;
            a.G[at] = g_prev;
            if (a.G_out) a.G_out[at] = g_prev;
        }
    }
}

// rule D.  VEC4 as above; VECOUT: the mask base is 4-byte aligned (a full lane stores its four bytes at once)
template <bool VEC4, bool VECOUT>
__global__ __launch_bounds__(kGsThreads) void ground_classify_kernel(GroundArgs a) {
    const int64_t bstart = (int64_t)blockIdx.x * kGsBlockPts;
    const int64_t g = bstart + (int64_t)threadIdx.x * kGsPtsPerThread;
    if (g >= a.total) return;
    int f = segment_of(a.offsets, a.n_frames, g);
    const int64_t cells = (int64_t)a.p.n_bins * a.S;
    uint8_t out[kGsPtsPerThread];
#pragma unroll
    for (int j = 0; j < kGsPtsPerThread; ++j) {
        const int64_t i = g + j;
        out[j] = 0;
        if (i < a.total) {
            while (i >= a.offsets[f + 1]) ++f;
            float x, y, z;
            if (VEC4) { const float4 v = reinterpret_cast<const float4*>(a.xyz)[i]; x = v.x; y = v.y; z = v.z; }
            else load_xyz(a.xyz, a.pitch, i, x, y, z);
            const int c = cell_of(a.p, a.S, x, y, z);
            if (c >= 0) out[j] = (uint8_t)(z - a.G[(int64_t)f * cells + c] <= a.p.ground_thresh);
        }
    }
    if (VECOUT && g + kGsPtsPerThread <= a.total) {
        *reinterpret_cast<uchar4*>(a.mask + g) = make_uchar4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kGsPtsPerThread; ++j)
            if (g + j < a.total) a.mask[g + j] = out[j];
    }
}

static bool params_ok(const himo_ground_params* p) {
    if (!p) return false;
    const float fl[6] = {p->sensor_height, p->r_min, p->bin_size, p->max_slope, p->step_tol, p->ground_thresh};
    for (float v : fl)
        if (!isfinite(v)) return false;
    return p->r_min > 0.f && p->bin_size > 0.f && p->n_bins >= 1 && p->n_bins <= 4096 && p->K >= 1 && p->K <= 512;
}

static size_t cells_of(int n_frames, const himo_ground_params* p) { return (size_t)n_frames * (size_t)p->n_bins * 8u * (size_t)p->K; }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_ground_seg_workspace_bytes(int n_frames, const himo_ground_params* params) {
    if (n_frames < 1 || !params_ok(params)) return 0;
    const size_t cells = cells_of(n_frames, params);
    return round_up(cells * sizeof(unsigned long long), 256) + round_up(cells * sizeof(float), 256);
}

extern "C" int himo_ground_seg_batch(int n_frames, int64_t total_points, const int64_t* h_offsets, const int64_t* d_offsets,
                                     const float* d_xyz, int pitch, const himo_ground_params* params, uint8_t* d_mask,
                                     float* d_cell_ground, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (n_frames < 1 || total_points < 0 || !h_offsets || !d_offsets || !params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (pitch != 3 && pitch != 4) return HIMO_ERR_INVALID_ARGUMENT;
    if (h_offsets[0] != 0 || h_offsets[n_frames] != total_points) return HIMO_ERR_INVALID_ARGUMENT;
    for (int f = 0; f < n_frames; ++f)
        if (h_offsets[f] < 0 || h_offsets[f + 1] < h_offsets[f]) return HIMO_ERR_INVALID_ARGUMENT;
    if (total_points > 0 && (!d_xyz || !d_mask)) return HIMO_ERR_INVALID_ARGUMENT;
    auto misaligned = [](const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; };
    if (misaligned(d_xyz, 4) || misaligned(d_cell_ground, 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (total_points > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (total_points == 0) return HIMO_OK;
    if (!d_workspace || misaligned(d_workspace, 16) || workspace_bytes < himo_ground_seg_workspace_bytes(n_frames, params))
        return HIMO_ERR_WORKSPACE;

    const size_t cells = cells_of(n_frames, params);
    GroundArgs a;
    a.n_frames = n_frames; a.total = total_points; a.offsets = d_offsets; a.xyz = d_xyz; a.pitch = pitch; a.p = *params;
    a.S = 8 * params->K;
    a.keys = reinterpret_cast<unsigned long long*>(d_workspace);
    a.G = reinterpret_cast<float*>(reinterpret_cast<char*>(d_workspace) + round_up(cells * sizeof(unsigned long long), 256));
    a.G_out = d_cell_ground;
    a.mask = d_mask;

    hipStream_t s = (hipStream_t)stream;
    HIMO_HIP(hipMemsetAsync(a.keys, 0xFF, cells * sizeof(unsigned long long), s));
    const bool vec4 = pitch == 4 && aligned16(d_xyz);
    const dim3 block(kGsThreads), grid((unsigned)((total_points + kGsBlockPts - 1) / kGsBlockPts));
    {
        ProfScope ps("ground_bin_kernel", s);
        if (vec4) hipLaunchKernelGGL((ground_bin_kernel<true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ground_bin_kernel<false>), grid, block, 0, s, a);
    }
    HIMO_LAUNCH_CHECK("ground_bin_kernel");
    {
        ProfScope ps("ground_walk_kernel", s);
        const int64_t walkers = (int64_t)n_frames * a.S;
        hipLaunchKernelGGL(ground_walk_kernel, dim3((unsigned)((walkers + kGsThreads - 1) / kGsThreads)), block, 0, s, a);
    }
    HIMO_LAUNCH_CHECK("ground_walk_kernel");
    {
        ProfScope ps("ground_classify_kernel", s);
        const bool vout = !misaligned(d_mask, 4);
        if (vec4 && vout) hipLaunchKernelGGL((ground_classify_kernel<true, true>), grid, block, 0, s, a);
        else if (vec4) hipLaunchKernelGGL((ground_classify_kernel<true, false>), grid, block, 0, s, a);
        else if (vout) hipLaunchKernelGGL((ground_classify_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ground_classify_kernel<false, false>), grid, block, 0, s, a);
    }
    HIMO_LAUNCH_CHECK("ground_classify_kernel");
    return HIMO_OK;
}
