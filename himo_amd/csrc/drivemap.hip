// drivemap.hip -- the whole-drive free-space map ("free-space drive map, v1"; the rule is the module docstring of himo_amd/drivemap.py)
// for gfx950.  PARITY UNPINNED: the reference has no such stage; this one is checked against the numpy restatement of the written rule
// (tests/drivemap_ref.py), which it equals bit for bit.
//
//   rays of sweep s (an origin of that sweep -> a return of it, in the map's frame)  ->  one uint64 per voxel:
//         stamp (s + 1) : 16 [63..48] | 0 : 14 | HIT : 1 [33] | FREE : 1 [32] | free_n : 16 [31..16] | hit_n : 16 [15..0]
//   points + the map                                                                 ->  free_n, hit_n (uint16 each), DYNAMIC (a byte)
//   the map                                                                          ->  the STATIC voxels, in ascending voxel index
//
// Rules A-C (quantisation, ray set-up, the integer walk) are those of "free-space ray map, v1" and are restated here line for line
// from raymap.hip, which stays as it is.  What is new is the mark: a voxel's word says what the sweep that touched it last (the stamp)
// did to it -- FREE, or HIT, never both -- and how many sweeps so far ended as FREE-and-not-HIT (free_n) and as HIT (hit_n):
//     another stamp                     -> the stamp, the arriving state, its counter + 1
//     the same stamp, FREE arriving     -> nothing (FREE already, or HIT, which voids the sweep's free vote)
//     the same stamp, HIT after HIT     -> nothing
//     the same stamp, HIT after FREE    -> state HIT, free_n - 1, hit_n + 1
// so the word after a sweep depends on the SET of its marks only: not on ray order, on the split over calls, or on carving rays twice;
// equal calls give equal bytes on every run.  Sweep numbers on one map must not decrease from call to call (the stamp is compared for
// equality only).  The word is read with a plain load and changed by a 64-bit compare-and-swap on the whole word, issued only when the
// word would change: a stale read is an OLDER word of the voxel, and an older word never asks for less than the current one does (under
// the same stamp the state only goes FREE -> HIT), so it costs a redundant atomic and a retry, never a wrong word.
//
// Six kernels:
//   drivemap_src_kernel    reads every src byte of a carve call; a byte in 16..254 stamps the call's flag word and the sticky refusal word
//   drivemap_carve_kernel  one ray per lane, 256-thread blocks; leaves at once when the call was refused.  Lanes diverge in step count.
//   drivemap_query_kernel  one point per lane: quantise, one 8-byte load, three values out
//   drivemap_count_kernel  STATIC voxels of each tile of 2048 consecutive voxels (8 per thread, thread-contiguous)
//   drivemap_scan_kernel   one block: the tile counts become the rows before each tile, in tile order; the total goes to *count
//   drivemap_write_kernel  every tile again: thread t's rows start at rows-before-the-tile + STATIC voxels of threads 0 .. t-1
// No atomic ticket orders the rows: the order is ascending linear voxel index by construction.
//
// Built with -ffp-contract=off: (c - min) * scale and ((float)v + 0.5f) * voxel + x0 round after every operation, as numpy does.
#include "himo_common.h"
#include "blockops.h"
#include <math.h>
#include <atomic>
#include <mutex>

namespace himo {

constexpr int kDmThreads = 256;
constexpr int kDmPerThread = 8;                                  // voxels of a tile each thread owns, contiguous
constexpr int kDmTile = kDmThreads * kDmPerThread;
constexpr int kDmRing = 1024;                                    // flag words handed to successive carve calls in turn
constexpr int kDmMaxDevices = 64;

constexpr uint64_t kDmFree = 1ull << 32, kDmHit = 1ull << 33;

// rule A: sub-voxel coordinates (256 per voxel) of a point, false = UNUSABLE
__device__ inline bool dm_quantise(const himo_drivemap_params& p, float x, float y, float z, int u[3]) {
    const float f0 = (x - p.x0) * p.scale, f1 = (y - p.y0) * p.scale, f2 = (z - p.z0) * p.scale;
    if (!(fabsf(f0) < 4194304.0f) || !(fabsf(f1) < 4194304.0f) || !(fabsf(f2) < 4194304.0f)) return false;      // NaN and inf too
    u[0] = (int)floorf(f0); u[1] = (int)floorf(f1); u[2] = (int)floorf(f2);
    return true;
}

__device__ inline bool dm_in_grid(const himo_drivemap_params& p, int vx, int vy, int vz) {
    return (unsigned)vx < (unsigned)p.nx && (unsigned)vy < (unsigned)p.ny && (unsigned)vz < (unsigned)p.nz;
}

// rule D': the word after a FREE / HIT mark of the sweep with stamp `st` (the table above)
__device__ inline uint64_t dm_next(uint64_t w, uint64_t st, bool hit) {
    if ((w >> 48) == st) {
        if (!hit || (w & kDmHit)) return w;
        return ((w & ~kDmFree) | kDmHit) - (1ull << 16) + 1ull;
    }
    const uint64_t counts = (w & 0xFFFFFFFFull) | (st << 48);
    return hit ? (counts | kDmHit) + 1ull : (counts | kDmFree) + (1ull << 16);
}

__device__ inline void dm_mark(uint64_t* __restrict__ map, const himo_drivemap_params& p, int vx, int vy, int vz, uint64_t st, bool hit) {
    unsigned long long* q = reinterpret_cast<unsigned long long*>(map + ((int64_t)vz * p.ny + vy) * p.nx + vx);
    unsigned long long w = *q;
    for (;;) {
        const unsigned long long nw = dm_next(w, st, hit);
        if (nw == w) return;
        const unsigned long long got = atomicCAS(q, w, nw);
        if (got == w) return;
        w = got;
    }
}

// rule S
__device__ inline bool dm_static(uint64_t w, const himo_drivemap_params& p) {
    const int hv = (int)(w & 0xFFFFu), fv = (int)((w >> 16) & 0xFFFFu);
    return hv >= p.min_hits && !(fv >= p.min_votes && fv > hv);
}

__global__ __launch_bounds__(kDmThreads) void drivemap_src_kernel(int64_t n, const unsigned char* __restrict__ src, uint32_t* flag,
                                                                   uint32_t* sticky, uint32_t seq) {
    const int64_t i = (int64_t)blockIdx.x * kDmThreads + threadIdx.x;
    const bool bad = i < n && src[i] > 15 && src[i] != 255;
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) {           // one pair of stores per wave that saw one
        atomicExch(flag, seq);
        atomicOr(sticky, 1u);
    }
}

__global__ __launch_bounds__(kDmThreads) void drivemap_carve_kernel(int64_t n, const float* __restrict__ pts, int pitch,
                                                                     const unsigned char* __restrict__ src, const float* __restrict__ origins,
                                                                     uint64_t st, himo_drivemap_params p, uint64_t* __restrict__ map,
                                                                     const uint32_t* __restrict__ flag, uint32_t seq) {
    if (*flag == seq) return;                                        // the call was refused: a src byte in 16..254
    const int64_t i = (int64_t)blockIdx.x * kDmThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned s = src[i];
    if (s > 15) return;                                              // 255: the ray takes no part
    const float* q = pts + i * pitch;
    const float* o = origins + 3 * s;
    int A[3], B[3];
    if (!dm_quantise(p, o[0], o[1], o[2], A) || !dm_quantise(p, q[0], q[1], q[2], B)) return;
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
    while ((r[0] | r[1] | r[2]) != 0) {                              // (every r is >= 0)
        const int cheb = max(r[0], max(r[1], r[2]));                 // |e - v| on an axis IS the steps still owed on it
        if (cheb > p.guard && dm_in_grid(p, v[0], v[1], v[2])) dm_mark(map, p, v[0], v[1], v[2], st, false);
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
    if (dm_in_grid(p, e[0], e[1], e[2])) dm_mark(map, p, e[0], e[1], e[2], st, true);
}

__global__ __launch_bounds__(kDmThreads) void drivemap_query_kernel(int64_t n, const float* __restrict__ pts, int pitch,
                                                                     const unsigned char* __restrict__ skip, himo_drivemap_params p,
                                                                     const uint64_t* __restrict__ map, uint16_t* __restrict__ fv_out,
                                                                     uint16_t* __restrict__ hv_out, unsigned char* __restrict__ dyn_out) {
    const int64_t i = (int64_t)blockIdx.x * kDmThreads + threadIdx.x;
    if (i >= n) return;
    int fv = 0, hv = 0;
    if (!(skip && skip[i])) {
        const float* q = pts + i * pitch;
        int u[3];
        if (dm_quantise(p, q[0], q[1], q[2], u)) {
            const int vx = u[0] >> 8, vy = u[1] >> 8, vz = u[2] >> 8;
            if (dm_in_grid(p, vx, vy, vz)) {
                const uint64_t w = map[((int64_t)vz * p.ny + vy) * p.nx + vx];
                fv = (int)((w >> 16) & 0xFFFFu);
                hv = (int)(w & 0xFFFFu);
            }
        }
    }
    if (fv_out) fv_out[i] = (uint16_t)fv;
    if (hv_out) hv_out[i] = (uint16_t)hv;
    if (dyn_out) dyn_out[i] = (unsigned char)(fv >= p.min_votes && fv > hv);      // (fv = 0 for a skipped, unusable or outside point)
}

// the STATIC voxels among the kDmPerThread this thread owns, as a bit mask (bit j: voxel first + j)
__device__ inline unsigned dm_static_bits(const uint64_t* __restrict__ map, int64_t cells, const himo_drivemap_params& p, int64_t first) {
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < kDmPerThread; ++j)
        if (first + j < cells && dm_static(map[first + j], p)) bits |= 1u << j;
    return bits;
}

__global__ __launch_bounds__(kDmThreads) void drivemap_count_kernel(himo_drivemap_params p, const uint64_t* __restrict__ map, int64_t cells,
                                                                     int* __restrict__ tile_rows) {
    const int64_t first = (int64_t)blockIdx.x * kDmTile + (int64_t)threadIdx.x * kDmPerThread;
    int c = wave_sum(__popc(dm_static_bits(map, cells, p, first)));
    __shared__ int per_wave[kDmThreads / 64];
    if ((threadIdx.x & 63) == 0) per_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int all = 0;
        for (int w = 0; w < kDmThreads / 64; ++w) all += per_wave[w];
        tile_rows[blockIdx.x] = all;
    }
}

// one block: tile_rows[t] becomes the rows of the tiles before t; the total goes to *count
__global__ __launch_bounds__(kDmThreads) void drivemap_scan_kernel(int* __restrict__ tile_rows, int n_tiles, int64_t* __restrict__ count) {
    __shared__ int part[kDmThreads];
    int64_t carry = 0;
    for (int lo = 0; lo < n_tiles; lo += kDmThreads) {
        const int t = lo + (int)threadIdx.x;
        const int x = t < n_tiles ? tile_rows[t] : 0;
        const int incl = block_inclusive_scan<kDmThreads>(x, part);
        if (t < n_tiles) tile_rows[t] = (int)carry + incl - x;
        carry += part[kDmThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(kDmThreads) void drivemap_write_kernel(himo_drivemap_params p, const uint64_t* __restrict__ map, int64_t cells,
                                                                     const int* __restrict__ tile_rows, int64_t capacity,
                                                                     float* __restrict__ rows, int32_t* __restrict__ hits,
                                                                     int32_t* __restrict__ free_n) {
    __shared__ int part[kDmThreads];
    const int64_t first = (int64_t)blockIdx.x * kDmTile + (int64_t)threadIdx.x * kDmPerThread;
    const unsigned bits = dm_static_bits(map, cells, p, first);
    const int c = __popc(bits);
    int64_t row = (int64_t)tile_rows[blockIdx.x] + (block_inclusive_scan<kDmThreads>(c, part) - c);
#pragma unroll
    for (int j = 0; j < kDmPerThread; ++j) {
        if (!(bits & (1u << j))) continue;
        if (row < capacity) {
            const int64_t i = first + j;
            const uint64_t w = map[i];
            const int vx = (int)(i % p.nx), vy = (int)((i / p.nx) % p.ny), vz = (int)(i / ((int64_t)p.nx * p.ny));
            float* o = rows + 4 * row;
            o[0] = ((float)vx + 0.5f) * p.voxel + p.x0;
            o[1] = ((float)vy + 0.5f) * p.voxel + p.y0;
            o[2] = ((float)vz + 0.5f) * p.voxel + p.z0;
            o[3] = 0.0f;
            hits[row] = (int32_t)(w & 0xFFFFu);
            free_n[row] = (int32_t)((w >> 16) & 0xFFFFu);
        }
        ++row;
    }
}

static bool dm_params_ok(const himo_drivemap_params* p) {
    if (!p) return false;
    const float fl[5] = {p->x0, p->y0, p->z0, p->voxel, p->scale};
    for (float f : fl)
        if (!isfinite(f)) return false;
    if (!(p->voxel > 0.f) || p->scale != (float)(256.0 / (double)p->voxel)) return false;
    if (p->nx < 1 || p->nx > 16384 || p->ny < 1 || p->ny > 16384 || p->nz < 1 || p->nz > 256) return false;
    if ((int64_t)p->nx * p->ny * p->nz > (int64_t)1 << 29) return false;
    return p->guard >= 0 && p->guard <= 8 && p->min_votes >= 1 && p->min_votes <= 65535 && p->min_hits >= 1 && p->min_hits <= 65535;
}

static int64_t dm_cells(const himo_drivemap_params* p) { return (int64_t)p->nx * p->ny * p->nz; }
static int dm_tiles(const himo_drivemap_params* p) { return (int)((dm_cells(p) + kDmTile - 1) / kDmTile); }

// the flag words of a device: [0] the sticky refusal word, [1 + k] the word of the carve calls whose sequence number is k mod kDmRing
static std::mutex g_dm_lock;
static uint32_t* g_dm_flags[kDmMaxDevices];
static std::atomic<uint32_t> g_dm_seq{0};

static int dm_flags(uint32_t** out) {
    int dev = 0;
    HIMO_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kDmMaxDevices) return HIMO_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> hold(g_dm_lock);
    if (!g_dm_flags[dev]) {
        uint32_t* w = nullptr;
        HIMO_HIP(hipMalloc(&w, (1 + kDmRing) * sizeof(uint32_t)));
        const hipError_t e = hipMemset(w, 0, (1 + kDmRing) * sizeof(uint32_t));
        if (e != hipSuccess) { (void)hipFree(w); return check_hip(e, "hipMemset(drivemap flags)"); }
        g_dm_flags[dev] = w;
    }
    *out = g_dm_flags[dev];
    return HIMO_OK;
}

static bool dm_misaligned(const void* q, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(q) & (bytes - 1)) != 0; }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_drivemap_bytes(const himo_drivemap_params* params) {
    if (!dm_params_ok(params)) return 0;
    return sizeof(uint64_t) * (size_t)dm_cells(params);
}

extern "C" int himo_drivemap_carve(int64_t n_rays, const float* d_pts, int pitch, const unsigned char* d_src, const float* d_origins,
                                   int sweep, const himo_drivemap_params* params, uint64_t* d_map, void* stream) {
    if (n_rays < 0 || (pitch != 3 && pitch != 4) || sweep < 0 || sweep > 65534 || !dm_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_rays > 0 && (!d_pts || !d_src || !d_origins || !d_map)) return HIMO_ERR_INVALID_ARGUMENT;
    if (dm_misaligned(d_pts, 4) || dm_misaligned(d_origins, 4) || dm_misaligned(d_map, 8)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n_rays > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n_rays == 0) return HIMO_OK;
    uint32_t* flags = nullptr;
    const int st = dm_flags(&flags);
    if (st != HIMO_OK) return st;
    uint32_t seq = ++g_dm_seq;
    if (seq == 0) seq = ++g_dm_seq;                                  // 0 is what an unused flag word holds
    uint32_t* flag = flags + 1 + seq % kDmRing;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(kDmThreads), grid((unsigned)((n_rays + kDmThreads - 1) / kDmThreads));
    {
        ProfScope ps("drivemap_src_kernel", s);
        hipLaunchKernelGGL(drivemap_src_kernel, grid, block, 0, s, n_rays, d_src, flag, flags, seq);
    }
    HIMO_LAUNCH_CHECK("drivemap_src_kernel");
    {
        ProfScope ps("drivemap_carve_kernel", s);
        hipLaunchKernelGGL(drivemap_carve_kernel, grid, block, 0, s, n_rays, d_pts, pitch, d_src, d_origins, (uint64_t)(sweep + 1), *params,
                           d_map, (const uint32_t*)flag, seq);
    }
    HIMO_LAUNCH_CHECK("drivemap_carve_kernel");
    return HIMO_OK;
}

extern "C" int himo_drivemap_query(int64_t n, const float* d_pts, int pitch, const unsigned char* d_skip, const himo_drivemap_params* params,
                                   const uint64_t* d_map, uint16_t* d_free_n, uint16_t* d_hit_n, unsigned char* d_dynamic, void* stream) {
    if (n < 0 || (pitch != 3 && pitch != 4) || !dm_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!d_pts || !d_map)) return HIMO_ERR_INVALID_ARGUMENT;
    if (dm_misaligned(d_pts, 4) || dm_misaligned(d_map, 8) || dm_misaligned(d_free_n, 2) || dm_misaligned(d_hit_n, 2))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n == 0) return HIMO_OK;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("drivemap_query_kernel", s);
        hipLaunchKernelGGL(drivemap_query_kernel, dim3((unsigned)((n + kDmThreads - 1) / kDmThreads)), dim3(kDmThreads), 0, s, n, d_pts,
                           pitch, d_skip, *params, d_map, d_free_n, d_hit_n, d_dynamic);
    }
    HIMO_LAUNCH_CHECK("drivemap_query_kernel");
    return HIMO_OK;
}

extern "C" size_t himo_drivemap_emit_workspace_bytes(const himo_drivemap_params* params) {
    if (!dm_params_ok(params)) return 0;
    return sizeof(int) * (size_t)dm_tiles(params);
}

extern "C" int himo_drivemap_emit(const himo_drivemap_params* params, const uint64_t* d_map, int64_t capacity, float* d_rows4, int32_t* d_hits,
                                  int32_t* d_free_n, int64_t* d_count, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!dm_params_ok(params) || capacity < 0 || !d_map || !d_count || !d_workspace) return HIMO_ERR_INVALID_ARGUMENT;
    if (capacity > 0 && (!d_rows4 || !d_hits || !d_free_n)) return HIMO_ERR_INVALID_ARGUMENT;
    if (dm_misaligned(d_map, 8) || dm_misaligned(d_count, 8) || dm_misaligned(d_rows4, 4) || dm_misaligned(d_hits, 4) ||
        dm_misaligned(d_free_n, 4) || dm_misaligned(d_workspace, 4))
        return HIMO_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < himo_drivemap_emit_workspace_bytes(params)) return HIMO_ERR_WORKSPACE;
    const int64_t cells = dm_cells(params);
    const int n_tiles = dm_tiles(params);
    int* tile_rows = static_cast<int*>(d_workspace);
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("drivemap_count_kernel", s);
        hipLaunchKernelGGL(drivemap_count_kernel, dim3((unsigned)n_tiles), dim3(kDmThreads), 0, s, *params, d_map, cells, tile_rows);
    }
    HIMO_LAUNCH_CHECK("drivemap_count_kernel");
    {
        ProfScope ps("drivemap_scan_kernel", s);
        hipLaunchKernelGGL(drivemap_scan_kernel, dim3(1), dim3(kDmThreads), 0, s, tile_rows, n_tiles, d_count);
    }
    HIMO_LAUNCH_CHECK("drivemap_scan_kernel");
    if (capacity == 0) return HIMO_OK;                               // the count alone
    {
        ProfScope ps("drivemap_write_kernel", s);
        hipLaunchKernelGGL(drivemap_write_kernel, dim3((unsigned)n_tiles), dim3(kDmThreads), 0, s, *params, d_map, cells,
                           (const int*)tile_rows, capacity, d_rows4, d_hits, d_free_n);
    }
    HIMO_LAUNCH_CHECK("drivemap_write_kernel");
    return HIMO_OK;
}

extern "C" int himo_drivemap_status(void* stream) {
    uint32_t* flags = nullptr;
    const int st = dm_flags(&flags);
    if (st != HIMO_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    uint32_t host = 0;
    HIMO_HIP(hipMemcpyAsync(&host, flags, sizeof(host), hipMemcpyDeviceToHost, s));
    HIMO_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t), s));
    HIMO_HIP(hipStreamSynchronize(s));
    return host ? HIMO_ERR_INVALID_ARGUMENT : HIMO_OK;
}
