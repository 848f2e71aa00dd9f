// raymap.hip -- the free-space labeller ("free-space ray map, v1"; the rule is the module docstring of himo_amd/raymap.py) for gfx950.
// PARITY UNPINNED: the reference's label generator lives in its absent submodule; this stage is checked against the numpy
// restatement of the written rule (tests/raymap_ref.py), which it equals bit for bit.
//
//   rays (origin of their sweep -> a return of that sweep, in the map's frame)  ->  one uint32 per voxel: FREE bits 0..15, HIT bits 16..31
//   target points + the map                                                      ->  free votes, hit votes, DYNAMIC (a byte each)
//
// Three kernels:
//   raymap_slots_kernel   reads every slot byte of a carve call; a byte in 16..254 stamps the call's flag word with the call's
//                         sequence number and sets the device's sticky refusal word (himo_raymap_status).
//   raymap_carve_kernel   one ray per lane, 256-thread blocks.  Leaves at once when the call's flag word carries the call's number.
//                         The walk is integer only: per axis the crossing parameter of the next voxel boundary is num / den, compared
//                         by one 32x32->64 multiply per side (num < 2^23 + 2^9, den < 2^23: products below 2^48).  The map word is
//                         read with a plain load and the atomic OR issued only when the bit is missing -- a stale read costs a
//                         redundant atomic, never a wrong map.  Lanes of a wave diverge in step count (accepted in v1); a ray stops
//                         once it has left the grid on the axis it steps along, in the direction of that step: every voxel after
//                         that, the end voxel included, is outside the grid.
//   raymap_query_kernel   one point per lane: quantise, read the word, two popcounts, three bytes out.
//
// Built with -ffp-contract=off: (c - min) * scale rounds after the subtraction and after the multiplication, as numpy does.
#include "himo_common.h"
#include <math.h>
#include <atomic>
#include <mutex>

namespace himo {

constexpr int kRmThreads = 256;
constexpr int kRmRing = 1024;               // flag words handed to successive carve calls in turn
constexpr int kRmMaxDevices = 64;

// rule A: sub-voxel coordinates (256 per voxel) of a point, false = UNUSABLE
__device__ inline bool rm_quantise(const himo_raymap_params& p, float x, float y, float z, int u[3]) {
    const float f0 = (x - p.x0) * p.scale, f1 = (y - p.y0) * p.scale, f2 = (z - p.z0) * p.scale;
    if (!(fabsf(f0) < 4194304.0f) || !(fabsf(f1) < 4194304.0f) || !(fabsf(f2) < 4194304.0f)) return false;      // NaN and inf too
    u[0] = (int)floorf(f0); u[1] = (int)floorf(f1); u[2] = (int)floorf(f2);
    return true;
}

__device__ inline bool rm_in_grid(const himo_raymap_params& p, int vx, int vy, int vz) {
    return (unsigned)vx < (unsigned)p.nx && (unsigned)vy < (unsigned)p.ny && (unsigned)vz < (unsigned)p.nz;
}

__device__ inline void rm_mark(uint32_t* __restrict__ map, const himo_raymap_params& p, int vx, int vy, int vz, uint32_t bit) {
    uint32_t* w = map + ((int64_t)vz * p.ny + vy) * p.nx + vx;
    if (!(*w & bit)) atomicOr(w, bit);
}

__global__ __launch_bounds__(kRmThreads) void raymap_slots_kernel(int64_t n, const unsigned char* __restrict__ slot, uint32_t* flag,
                                                                   uint32_t* sticky, uint32_t seq) {
    const int64_t i = (int64_t)blockIdx.x * kRmThreads + threadIdx.x;
    const bool bad = i < n && slot[i] > 15 && slot[i] != 255;
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) {           // one pair of stores per wave that saw one
        atomicExch(flag, seq);
        atomicOr(sticky, 1u);
    }
}

__global__ __launch_bounds__(kRmThreads) void raymap_carve_kernel(int64_t n, const float* __restrict__ pts, int pitch,
                                                                   const unsigned char* __restrict__ slot, const float* __restrict__ origins,
                                                                   himo_raymap_params p, uint32_t* __restrict__ map,
                                                                   const uint32_t* __restrict__ flag, uint32_t seq) {
    if (*flag == seq) return;                                        // the call was refused: a slot byte in 16..254
    const int64_t i = (int64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned s = slot[i];
    if (s > 15) return;                                              // 255: the ray takes no part
    const float* q = pts + i * pitch;
    const float* o = origins + 3 * s;
    int A[3], B[3];
    if (!rm_quantise(p, o[0], o[1], o[2], A) || !rm_quantise(p, q[0], q[1], q[2], B)) return;
    const int n_ax[3] = {p.nx, p.ny, p.nz};
    int v[3], e[3], step[3], r[3];
    unsigned num[3], den[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = A[k] >> 8; e[k] = B[k] >> 8;
        const int d = B[k] - A[k];
        step[k] = d > 0 ? 1 : (d < 0 ? -1 : 0);
        den[k] = (unsigned)(d < 0 ? -d : d);
        r[k] = e[k] >= v[k] ? e[k] - v[k] : v[k] - e[k];
        const int edge = (v[k] + (step[k] > 0 ? 1 : 0)) * 256 - A[k];
        num[k] = (unsigned)(edge < 0 ? -edge : edge);
    }
    const uint32_t free_bit = 1u << s, hit_bit = 1u << (16 + s);
    while ((r[0] | r[1] | r[2]) != 0) {                              // (every r is >= 0)
        const int cheb = max(r[0], max(r[1], r[2]));                 // |e - v| on an axis IS the steps still owed on it
        if (cheb > p.guard && rm_in_grid(p, v[0], v[1], v[2])) rm_mark(map, p, v[0], v[1], v[2], free_bit);
        // the axis, among those that still owe steps, whose next boundary comes first; a tie goes to the lowest axis
        int a = r[0] > 0 ? 0 : (r[1] > 0 ? 1 : 2);
        if (a == 0 && r[1] > 0 && (uint64_t)num[1] * den[0] < (uint64_t)num[0] * den[1]) a = 1;
        if (a != 2 && r[2] > 0) {
            const unsigned na = a == 0 ? num[0] : num[1], da = a == 0 ? den[0] : den[1];
            if ((uint64_t)num[2] * da < (uint64_t)na * den[2]) a = 2;
        }
        bool left = false;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k == a) {
                v[k] += step[k]; num[k] += 256u; r[k] -= 1;
                left = step[k] > 0 ? v[k] >= n_ax[k] : v[k] < 0;
            }
        if (left) return;                                            // outside for good, and so is the end voxel
    }
    if (rm_in_grid(p, e[0], e[1], e[2])) rm_mark(map, p, e[0], e[1], e[2], hit_bit);
}

__global__ __launch_bounds__(kRmThreads) void raymap_query_kernel(int64_t n, const float* __restrict__ pts, int pitch,
                                                                   const unsigned char* __restrict__ skip, himo_raymap_params p,
                                                                   const uint32_t* __restrict__ map, unsigned char* __restrict__ fv_out,
                                                                   unsigned char* __restrict__ hv_out, unsigned char* __restrict__ dyn_out) {
    const int64_t i = (int64_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (i >= n) return;
    int fv = 0, hv = 0;
    if (!(skip && skip[i])) {
        const float* q = pts + i * pitch;
        int u[3];
        if (rm_quantise(p, q[0], q[1], q[2], u)) {
            const int vx = u[0] >> 8, vy = u[1] >> 8, vz = u[2] >> 8;
            if (rm_in_grid(p, vx, vy, vz)) {
                const uint32_t w = map[((int64_t)vz * p.ny + vy) * p.nx + vx];
                fv = __popc((w & 0xFFFFu) & ~(w >> 16));
                hv = __popc(w >> 16);
            }
        }
    }
    if (fv_out) fv_out[i] = (unsigned char)fv;
    if (hv_out) hv_out[i] = (unsigned char)hv;
    if (dyn_out) dyn_out[i] = (unsigned char)(fv >= p.min_votes && fv > hv);      // (fv = 0 for a skipped, unusable or outside point)
}

static bool rm_params_ok(const himo_raymap_params* p) {
    if (!p) return false;
    const float fl[5] = {p->x0, p->y0, p->z0, p->voxel, p->scale};
    for (float f : fl)
        if (!isfinite(f)) return false;
    if (!(p->voxel > 0.f) || p->scale != (float)(256.0 / (double)p->voxel)) return false;
    if (p->nx < 1 || p->nx > 1024 || p->ny < 1 || p->ny > 1024 || p->nz < 1 || p->nz > 64) return false;
    if ((int64_t)p->nx * p->ny * p->nz > (int64_t)1 << 24) return false;
    return p->guard >= 0 && p->guard <= 8 && p->min_votes >= 1 && p->min_votes <= 16;
}

// the flag words of a device: [0] the sticky refusal word, [1 + k] the word of the carve calls whose sequence number is k mod kRmRing
static std::mutex g_rm_lock;
static uint32_t* g_rm_flags[kRmMaxDevices];
static std::atomic<uint32_t> g_rm_seq{0};

static int rm_flags(uint32_t** out) {
    int dev = 0;
    HIMO_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kRmMaxDevices) return HIMO_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> hold(g_rm_lock);
    if (!g_rm_flags[dev]) {
        uint32_t* w = nullptr;
        HIMO_HIP(hipMalloc(&w, (1 + kRmRing) * sizeof(uint32_t)));
        const hipError_t e = hipMemset(w, 0, (1 + kRmRing) * sizeof(uint32_t));
        if (e != hipSuccess) { (void)hipFree(w); return check_hip(e, "hipMemset(raymap flags)"); }
        g_rm_flags[dev] = w;
    }
    *out = g_rm_flags[dev];
    return HIMO_OK;
}

static bool rm_misaligned4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) != 0; }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_raymap_map_bytes(const himo_raymap_params* params) {
    if (!rm_params_ok(params)) return 0;
    return sizeof(uint32_t) * (size_t)params->nx * (size_t)params->ny * (size_t)params->nz;
}

extern "C" int himo_raymap_carve(int64_t n_rays, const float* d_pts, int pitch, const unsigned char* d_slot, const float* d_origins,
                                 const himo_raymap_params* params, uint32_t* d_map, void* stream) {
    if (n_rays < 0 || (pitch != 3 && pitch != 4) || !rm_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_rays > 0 && (!d_pts || !d_slot || !d_origins || !d_map)) return HIMO_ERR_INVALID_ARGUMENT;
    if (rm_misaligned4(d_pts) || rm_misaligned4(d_origins) || rm_misaligned4(d_map)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_rays > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n_rays == 0) return HIMO_OK;
    uint32_t* flags = nullptr;
    const int st = rm_flags(&flags);
    if (st != HIMO_OK) return st;
    uint32_t seq = ++g_rm_seq;
    if (seq == 0) seq = ++g_rm_seq;                                  // 0 is what an unused flag word holds
    uint32_t* flag = flags + 1 + seq % kRmRing;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(kRmThreads), grid((unsigned)((n_rays + kRmThreads - 1) / kRmThreads));
    {
        ProfScope ps("raymap_slots_kernel", s);
        hipLaunchKernelGGL(raymap_slots_kernel, grid, block, 0, s, n_rays, d_slot, flag, flags, seq);
    }
    HIMO_LAUNCH_CHECK("raymap_slots_kernel");
    {
        ProfScope ps("raymap_carve_kernel", s);
        hipLaunchKernelGGL(raymap_carve_kernel, grid, block, 0, s, n_rays, d_pts, pitch, d_slot, d_origins, *params, d_map,
                           (const uint32_t*)flag, seq);
    }
    HIMO_LAUNCH_CHECK("raymap_carve_kernel");
    return HIMO_OK;
}

extern "C" int himo_raymap_query(int64_t n, const float* d_pts, int pitch, const unsigned char* d_skip, const himo_raymap_params* params,
                                 const uint32_t* d_map, unsigned char* d_free_votes, unsigned char* d_hit_votes, unsigned char* d_dynamic,
                                 void* stream) {
    if (n < 0 || (pitch != 3 && pitch != 4) || !rm_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!d_pts || !d_map)) return HIMO_ERR_INVALID_ARGUMENT;
    if (rm_misaligned4(d_pts) || rm_misaligned4(d_map)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n == 0) return HIMO_OK;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("raymap_query_kernel", s);
        hipLaunchKernelGGL(raymap_query_kernel, dim3((unsigned)((n + kRmThreads - 1) / kRmThreads)), dim3(kRmThreads), 0, s, n, d_pts,
                           pitch, d_skip, *params, d_map, d_free_votes, d_hit_votes, d_dynamic);
    }
    HIMO_LAUNCH_CHECK("raymap_query_kernel");
    return HIMO_OK;
}

extern "C" int himo_raymap_status(void* stream) {
    uint32_t* flags = nullptr;
    const int st = rm_flags(&flags);
    if (st != HIMO_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    uint32_t host = 0;
    HIMO_HIP(hipMemcpyAsync(&host, flags, sizeof(host), hipMemcpyDeviceToHost, s));
    HIMO_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t), s));
    HIMO_HIP(hipStreamSynchronize(s));
    return host ? HIMO_ERR_INVALID_ARGUMENT : HIMO_OK;
}
