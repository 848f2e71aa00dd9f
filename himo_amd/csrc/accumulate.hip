// accumulate.hip -- multi-sweep accumulation ("sweep accumulation, v1", and its opt-in additions, "sweep accumulation, v2"; the rule is
// the module docstring of himo_amd/accumulate.py) for gfx950.  PARITY UNPINNED, v1 and v2 alike: the reference has no such program in
// its tree; this stage is checked against the numpy restatements of the written rule (tests/accumulate_ref.py, tests/accumulate2_ref.py),
// which it equals bit for bit.
//
//   source rows (own frame) + a 4x4 transform + a lag  ->  a hash table of voxels: count, three sub-voxel offset sums, the least lag
//   the table                                          ->  one row per occupied voxel: key, centroid, lag, count (in any order)
//
// The table.  capacity + 1 slots of 8 uint32 (32 bytes, so the five atomics of a row land in one 32-byte sector and a slot never
// straddles a cache line): [0] key, [1] count, [2..4] Sx Sy Sz, [5] least lag, [6] Sa, the sum of the rows' quantised attributes, [7] the
// greatest tag ((255 - lag) << 24 | label) of its rows -- both v2's, written by himo_accum_insert_ex alone and only for the calls that
// carry an attribute or a label: to v1's entry points they are the two unused words they always were.  A cleared slot has key and lag
// 0xFFFFFFFF and the rest 0.  The key (iz << 24) | (iy << 12) | ix of the largest admitted grid's last voxel IS 0xFFFFFFFF, the
// empty mark, so that one key does not enter the probing at all: it owns slot [capacity], which is occupied when its count is not 0.
// Hash: Fibonacci multiplicative, (key * 0x9E3779B1) >> (32 - log2 capacity) -- neighbouring voxels differ in the key's low bits and
// the product spreads those over the high bits -- then linear probing, (h + i) & (capacity - 1).  Probing a neighbouring slot stays
// in the same 128-byte line three times out of four.  The loop is bounded by the capacity: a row that has seen every slot taken by
// other keys sets the device's sticky refusal word (himo_accum_status) and leaves; nothing ever spins.
// A slot's key is read with a plain load first and the compare-and-swap issued only when the slot looks empty: keys never change once
// written, so a stale read costs one more atomic, never a wrong slot.
//
// Neighbouring lanes.  LiDAR rows that follow each other often fall into one voxel, so a wave first merges every run of
// NEIGHBOURING lanes with one key (a segmented suffix sum over the run: 6 shuffle steps for Sx, Sy and Sz; the count is the run's
// length and a call has one lag) and only the run's first lane probes and issues the five atomics.  A wave whose 64 keys all differ from their
// neighbours skips the merge.  Everything is integer, so merged or not, in any order of arrival, a voxel's five quantities are the same
// (which slot it sits in is not).
// Only 32-bit integer vector atomics on global memory are used (compare-and-swap, add, min, max, or); no float atomics.
//
// v2 (himo_accum_insert_ex, himo_accum_emit_ex) is the SAME code: the insert and the emit are function templates on a bool, and the
// v1 entry points launch the instantiation in which every v2 statement is compiled out -- no load, shuffle or atomic more than before.
// With EX a row is first advected (rule A2: x' = fmaf(lag, mx, x) when its motion is finite and at least motion_min long), carries a
// quantised attribute 0..255 and a tag; the merge of a run sums the attributes and takes the greatest tag beside the three offset
// sums, and a run's head issues up to seven atomics into its one 32-byte slot (add x5, min, max).  accum_motion_kernel is rule I: a
// stored flow less the ego motion of its sweep pair, m = flow - (E p - p).
//
// Three kernels (the insert and the emit twice, once per instantiation), and rule I's: accum_clear_kernel (16 bytes a lane), accum_insert_kernel (a row a lane, 256-thread blocks), accum_emit_kernel (8
// slots a lane, 2048 a block: the occupied ones are counted by ballots, ONE atomic add on the row counter per block reserves their
// rows -- one per wave, 65 536 adds on one word for a 2^22-slot table, took 0.75 ms of the emit -- and a second pass reads the
// occupied slots whole and writes the rows; the centroid in float64, one rounding to float32).
//
// Built with -ffp-contract=off: (c - min) * scale and the float64 centroid round after every operation, as numpy does; the move
// q = R p + t is rigid_math.h's written sequence (its fused multiply-adds are explicit).
#include "himo_common.h"
#include "rigid_math.h"
#include <math.h>
#include <mutex>

namespace himo {

constexpr int kAcThreads = 256;
constexpr int kAcSlotWords = 8;
constexpr int kAcEmitPer = 8;                // slots a lane of the emit walks
constexpr uint32_t kAcEmpty = 0xFFFFFFFFu;
constexpr int kAcMaxDevices = 64;

struct AcTransform { float m[12]; };         // the first three rows of the 4x4, by value in the launch

__device__ inline uint32_t ac_hash(uint32_t key, int shift) { return (key * 0x9E3779B1u) >> shift; }

__global__ __launch_bounds__(kAcThreads) void accum_clear_kernel(uint4* __restrict__ table, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * kAcThreads + threadIdx.x;
    if (i >= n16) return;
    // words 0..3 of a slot: key empty, count and Sx, Sy 0; words 4..7: Sz 0, lag all ones, two unused
    table[i] = (i & 1) ? make_uint4(0u, kAcEmpty, 0u, 0u) : make_uint4(kAcEmpty, 0u, 0u, 0u);
}

// what a v2 insert carries beside v1's arguments (rules A2 and H); any of the three pointers may be NULL
struct AcExtras {
    const float* motion;         // [n][3], the row's own displacement per sweep period
    const float* attr;           // [n] at a stride of attr_stride floats
    const int32_t* label;        // [n]
    float motion_min2, attr_scale;
    int attr_stride;
};

// rules A2 and H for row i of a v2 insert: advects (x, y, z), quantises the attribute into `sa` and builds `tag`; false = the row
// takes no part (a non-finite motion)
__device__ __forceinline__ bool ac_row_extras(const AcExtras& ex, int64_t i, uint32_t lag, float& x, float& y, float& z, uint32_t& sa,
                                              uint32_t& tag) {
    if (ex.motion) {                                                 // rule A2
        const float* m = ex.motion + i * 3;
        const float mx = m[0], my = m[1], mz = m[2];
        if (!(isfinite(mx) && isfinite(my) && isfinite(mz))) return false;
        const float s = (mx * mx + my * my) + mz * mz;
        if (s >= ex.motion_min2) {
            const float fl = (float)lag;
            x = __builtin_fmaf(fl, mx, x); y = __builtin_fmaf(fl, my, y); z = __builtin_fmaf(fl, mz, z);
        }
    }
    if (ex.attr) {                                                   // rule H: the attribute in 0..255
        const float g = ex.attr[i * (int64_t)ex.attr_stride] * ex.attr_scale;
        sa = !(g > 0.f) ? 0u : g >= 255.f ? 255u : (uint32_t)floorf(g + 0.5f);
    }
    if (ex.label) {
        const int32_t l = ex.label[i];
        tag = ((255u - lag) << 24) | (l > 0 && l < (1 << 24) ? (uint32_t)l : 0u);
    }
    return true;
}

// EX = false is v1 as it always was: every statement under `if constexpr (EX)` is compiled out, and `ex` is never read
template <bool EX>
__device__ __forceinline__ void accum_insert_body(int64_t n, const float* __restrict__ pts, int pitch, const unsigned char* __restrict__ skip,
                                                  AcTransform T, uint32_t lag, himo_accum_params p, uint32_t* __restrict__ table,
                                                  uint32_t capacity, int shift, uint32_t* __restrict__ sticky, AcExtras ex) {
    const int64_t i = (int64_t)blockIdx.x * kAcThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool valid = false;
    uint32_t key = 0, sx = 0, sy = 0, sz = 0;
    [[maybe_unused]] uint32_t sa = 0, tag = 0;
    if (i < n && !(skip && skip[i])) {
        const float* r = pts + i * pitch;
        float x = r[0], y = r[1], z = r[2];
        const bool in_ego = x > p.ego_min[0] && x < p.ego_max[0] && y > p.ego_min[1] && y < p.ego_max[1] && z > p.ego_min[2] && z < p.ego_max[2];
        if (isfinite(x) && isfinite(y) && isfinite(z) && !in_ego) {                       // rule A, on the row as given
            bool part = true;
            if constexpr (EX) part = ac_row_extras(ex, i, lag, x, y, z, sa, tag);        // rules A2 and H
            if (part) {
                float q[3];
                rigid_apply(T.m, x, y, z, q);                                             // rule B
                const float f0 = (q[0] - p.x0) * p.scale, f1 = (q[1] - p.y0) * p.scale, f2 = (q[2] - p.z0) * p.scale;      // rule C
                if (fabsf(f0) < 4194304.0f && fabsf(f1) < 4194304.0f && fabsf(f2) < 4194304.0f) {        // (false for NaN and inf)
                    const int u0 = (int)floorf(f0), u1 = (int)floorf(f1), u2 = (int)floorf(f2);
                    const int ix = u0 >> 8, iy = u1 >> 8, iz = u2 >> 8;
                    if ((unsigned)ix < (unsigned)p.nx && (unsigned)iy < (unsigned)p.ny && (unsigned)iz < (unsigned)p.nz) {
                        valid = true;
                        key = ((uint32_t)iz << 24) | ((uint32_t)iy << 12) | (uint32_t)ix;
                        sx = (uint32_t)(u0 & 255); sy = (uint32_t)(u1 & 255); sz = (uint32_t)(u2 & 255);
                    }
                }
            }
        }
    }
    // runs of neighbouring lanes with one key: a lane is a run's head when it is lane 0, invalid, or differs from the lane before
    const uint32_t prev_key = __shfl_up(key, 1);
    const int prev_valid = __shfl_up((int)valid, 1);
    const bool head = lane == 0 || !valid || !prev_valid || prev_key != key;
    const uint64_t heads = __ballot(head);
    uint32_t count = 1;
    if (heads != ~0ull) {                                            // (wave-uniform)
        const uint64_t after = lane == 63 ? 0ull : heads >> (lane + 1);
        const int run = after ? __ffsll((unsigned long long)after) : 64 - lane;          // lanes of my run from me to its end
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ax = __shfl_down(sx, d), ay = __shfl_down(sy, d), az = __shfl_down(sz, d);
            if (d < run) { sx += ax; sy += ay; sz += az; }
            if constexpr (EX) {                                      // rule H: the run's attribute sum and its greatest tag
                const uint32_t aa = __shfl_down(sa, d), at = __shfl_down(tag, d);
                if (d < run) { sa += aa; tag = max(tag, at); }
            }
        }
        count = (uint32_t)run;                                       // (every lane of a run of two or more is valid)
    }
    if (!head || !valid) return;
    uint32_t* slot = nullptr;
    if (key == kAcEmpty) {
        slot = table + (size_t)capacity * kAcSlotWords;             // the one key that is the empty mark: its own slot
    } else {
        const uint32_t mask = capacity - 1, h = ac_hash(key, shift);
        for (uint32_t k = 0; k < capacity; ++k) {                    // bounded: every slot is looked at once at most
            uint32_t* s = table + (size_t)((h + k) & mask) * kAcSlotWords;
            uint32_t cur = __atomic_load_n(s, __ATOMIC_RELAXED);
            if (cur == kAcEmpty) cur = atomicCAS(s, kAcEmpty, key);
            if (cur == key || cur == kAcEmpty) { slot = s; break; }
        }
    }
    if (!slot) {                                                     // the table is full of other keys: a refusal, not a fault
        atomicOr(sticky, 1u);
        return;
    }
    atomicAdd(slot + 1, count);
    atomicAdd(slot + 2, sx);
    atomicAdd(slot + 3, sy);
    atomicAdd(slot + 4, sz);
    atomicMin(slot + 5, lag);
    if constexpr (EX) {                                              // a call without the attribute or the label leaves its word alone
        if (ex.attr) atomicAdd(slot + 6, sa);
        if (ex.label) atomicMax(slot + 7, tag);
    }
}

__global__ __launch_bounds__(kAcThreads) void accum_insert_kernel(int64_t n, const float* __restrict__ pts, int pitch,
                                                                   const unsigned char* __restrict__ skip, AcTransform T, uint32_t lag,
                                                                   himo_accum_params p, uint32_t* __restrict__ table, uint32_t capacity,
                                                                   int shift, uint32_t* __restrict__ sticky) {
    accum_insert_body<false>(n, pts, pitch, skip, T, lag, p, table, capacity, shift, sticky, AcExtras{});
}

__global__ __launch_bounds__(kAcThreads) void accum_insert_ex_kernel(int64_t n, const float* __restrict__ pts, int pitch,
                                                                      const unsigned char* __restrict__ skip, AcTransform T, uint32_t lag,
                                                                      himo_accum_params p, uint32_t* __restrict__ table, uint32_t capacity,
                                                                      int shift, uint32_t* __restrict__ sticky, AcExtras ex) {
    accum_insert_body<true>(n, pts, pitch, skip, T, lag, p, table, capacity, shift, sticky, ex);
}

// rule I: the motion of a stored flow, m = flow - (E p - p); a row a lane
__global__ __launch_bounds__(kAcThreads) void accum_motion_kernel(int64_t n, const float* __restrict__ pts, int pitch,
                                                                   const float* __restrict__ flow, AcTransform E, float* __restrict__ motion) {
    const int64_t i = (int64_t)blockIdx.x * kAcThreads + threadIdx.x;
    if (i >= n) return;
    const float* r = pts + i * pitch;
    const float x = r[0], y = r[1], z = r[2];
    float q[3];
    rigid_apply(E.m, x, y, z, q);
    const float d0 = q[0] - x, d1 = q[1] - y, d2 = q[2] - z;
    motion[i * 3 + 0] = flow[i * 3 + 0] - d0;
    motion[i * 3 + 1] = flow[i * 3 + 1] - d1;
    motion[i * 3 + 2] = flow[i * 3 + 2] - d2;
}

// EX = false is v1's emit; with EX words 6 and 7 of a slot are read too and, where the pointers are not NULL, rule E2's columns written
template <bool EX>
__device__ __forceinline__ void accum_emit_body(const uint32_t* __restrict__ table, int64_t slots, himo_accum_params p, int64_t max_rows,
                                                int32_t* __restrict__ n_rows, uint32_t* __restrict__ keys, float* __restrict__ xyz,
                                                unsigned char* __restrict__ lag_out, int32_t* __restrict__ count_out, float attr_scale,
                                                float* __restrict__ attr_out, int32_t* __restrict__ label_out) {
    __shared__ int32_t wave_rows[kAcThreads / 64];
    __shared__ int32_t block_row0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t first = (int64_t)blockIdx.x * (kAcThreads * kAcEmitPer) + threadIdx.x;
    // pass 1: which of the block's slots are occupied (a ballot per wave and step) -- the key word alone is read
    uint64_t occ[kAcEmitPer];
    int32_t mine = 0;
#pragma unroll
    for (int j = 0; j < kAcEmitPer; ++j) {
        const int64_t i = first + (int64_t)j * kAcThreads;
        bool occupied = false;
        if (i < slots)          // the last slot belongs to the key that equals the empty mark: occupied when it has been counted into
            occupied = i == slots - 1 ? table[i * kAcSlotWords + 1] != 0u : table[i * kAcSlotWords] != kAcEmpty;
        occ[j] = __ballot(occupied);
        mine += (int32_t)__popcll(occ[j]);
    }
    if (lane == 0) wave_rows[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {                                          // one atomic on the row counter per block that has rows
        int32_t all = 0;
        for (int w = 0; w < kAcThreads / 64; ++w) all += wave_rows[w];
        block_row0 = all ? atomicAdd(n_rows, all) : 0;
    }
    __syncthreads();
    int64_t row0 = block_row0;
    for (int w = 0; w < wave; ++w) row0 += wave_rows[w];
    // pass 2: the occupied slots' rows, consecutive within the block
#pragma unroll
    for (int j = 0; j < kAcEmitPer; ++j) {
        const int64_t i = first + (int64_t)j * kAcThreads;
        const int64_t row = row0 + __popcll(occ[j] & ((1ull << lane) - 1ull));
        row0 += __popcll(occ[j]);
        if (!((occ[j] >> lane) & 1ull) || row >= max_rows) continue;
        const uint4 a = *reinterpret_cast<const uint4*>(table + i * kAcSlotWords);
        const uint2 b = *reinterpret_cast<const uint2*>(table + i * kAcSlotWords + 4);
        const uint32_t key = i == slots - 1 ? kAcEmpty : a.x;
        const uint32_t idx[3] = {key & 4095u, (key >> 12) & 4095u, key >> 24}, sum[3] = {a.z, a.w, b.x};
        const float mn[3] = {p.x0, p.y0, p.z0};
        const double unit = (double)p.voxel / 256.0, cnt = (double)a.y;
#pragma unroll
        for (int c = 0; c < 3; ++c)                                  // rule E: every operation rounds on its own, then one rounding to float32
            xyz[row * 3 + c] = (float)((double)mn[c] + (((double)(256u * idx[c]) + 0.5) + (double)sum[c] / cnt) * unit);
        keys[row] = key;
        lag_out[row] = (unsigned char)b.y;
        count_out[row] = (int32_t)a.y;
        if constexpr (EX) {                                          // rule E2
            const uint2 c = *reinterpret_cast<const uint2*>(table + i * kAcSlotWords + 6);
            if (attr_out) attr_out[row] = (float)(((double)c.x / cnt) / (double)attr_scale);
            if (label_out) label_out[row] = (int32_t)(c.y & 0xFFFFFFu);
        }
    }
}

__global__ __launch_bounds__(kAcThreads) void accum_emit_kernel(const uint32_t* __restrict__ table, int64_t slots, himo_accum_params p,
                                                                 int64_t max_rows, int32_t* __restrict__ n_rows, uint32_t* __restrict__ keys,
                                                                 float* __restrict__ xyz, unsigned char* __restrict__ lag_out,
                                                                 int32_t* __restrict__ count_out) {
    accum_emit_body<false>(table, slots, p, max_rows, n_rows, keys, xyz, lag_out, count_out, 1.f, nullptr, nullptr);
}

__global__ __launch_bounds__(kAcThreads) void accum_emit_ex_kernel(const uint32_t* __restrict__ table, int64_t slots, himo_accum_params p,
                                                                    int64_t max_rows, int32_t* __restrict__ n_rows, uint32_t* __restrict__ keys,
                                                                    float* __restrict__ xyz, unsigned char* __restrict__ lag_out,
                                                                    int32_t* __restrict__ count_out, float attr_scale,
                                                                    float* __restrict__ attr_out, int32_t* __restrict__ label_out) {
    accum_emit_body<true>(table, slots, p, max_rows, n_rows, keys, xyz, lag_out, count_out, attr_scale, attr_out, label_out);
}

static bool ac_params_ok(const himo_accum_params* p) {
    if (!p) return false;
    const float fl[11] = {p->x0, p->y0, p->z0, p->voxel, p->scale, p->ego_min[0], p->ego_min[1], p->ego_min[2], p->ego_max[0], p->ego_max[1],
                          p->ego_max[2]};
    for (float f : fl)
        if (!isfinite(f)) return false;
    if (!(p->voxel > 0.f) || p->scale != (float)(256.0 / (double)p->voxel)) return false;
    return p->nx >= 1 && p->nx <= 4096 && p->ny >= 1 && p->ny <= 4096 && p->nz >= 1 && p->nz <= 256;
}

// log2 of an admitted capacity (a power of two in 2^4 .. 2^26), else -1
static int ac_log2(int64_t capacity) {
    if (capacity < 16 || capacity > ((int64_t)1 << 26) || (capacity & (capacity - 1)) != 0) return -1;
    int k = 0;
    while (((int64_t)1 << k) < capacity) ++k;
    return k;
}

// the sticky refusal word of a device
static std::mutex g_ac_lock;
static uint32_t* g_ac_flag[kAcMaxDevices];

static int ac_flag(uint32_t** out) {
    int dev = 0;
    HIMO_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kAcMaxDevices) return HIMO_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> hold(g_ac_lock);
    if (!g_ac_flag[dev]) {
        uint32_t* w = nullptr;
        HIMO_HIP(hipMalloc(&w, sizeof(uint32_t)));
        const hipError_t e = hipMemset(w, 0, sizeof(uint32_t));
        if (e != hipSuccess) { (void)hipFree(w); return check_hip(e, "hipMemset(accumulate flag)"); }
        g_ac_flag[dev] = w;
    }
    *out = g_ac_flag[dev];
    return HIMO_OK;
}

static bool ac_misaligned(const void* q, unsigned mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; }

}  // namespace himo

using namespace himo;

extern "C" size_t himo_accum_table_bytes(int64_t capacity) {
    if (ac_log2(capacity) < 0) return 0;
    return ((size_t)capacity + 1) * kAcSlotWords * sizeof(uint32_t);
}

extern "C" int himo_accum_clear(void* d_table, int64_t capacity, void* stream) {
    if (ac_log2(capacity) < 0 || !d_table || ac_misaligned(d_table, 15u)) return HIMO_ERR_INVALID_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n16 = (capacity + 1) * 2;
    {
        ProfScope ps("accum_clear_kernel", s);
        hipLaunchKernelGGL(accum_clear_kernel, dim3((unsigned)((n16 + kAcThreads - 1) / kAcThreads)), dim3(kAcThreads), 0, s,
                           reinterpret_cast<uint4*>(d_table), n16);
    }
    HIMO_LAUNCH_CHECK("accum_clear_kernel");
    return HIMO_OK;
}

// both inserts: ex == nullptr is v1's entry point and launches v1's instantiation
static int ac_insert(int64_t n, const float* d_pts, int pitch, const unsigned char* d_skip, const float* h_transform, int lag,
                     const himo_accum_params* params, void* d_table, int64_t capacity, const AcExtras* ex, void* stream) {
    const int log2cap = ac_log2(capacity);
    if (ex) {
        if (ex->attr && !(isfinite(ex->attr_scale) && ex->attr_scale > 0.f)) return HIMO_ERR_INVALID_ARGUMENT;
        if (ex->attr_stride < 1 || !(isfinite(ex->motion_min2) && ex->motion_min2 >= 0.f)) return HIMO_ERR_INVALID_ARGUMENT;
        if (ac_misaligned(ex->motion, 3u) || ac_misaligned(ex->attr, 3u) || ac_misaligned(ex->label, 3u)) return HIMO_ERR_INVALID_ARGUMENT;
    }
    if (n < 0 || (pitch != 3 && pitch != 4) || lag < 0 || lag > 255 || log2cap < 0 || !ac_params_ok(params)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!d_pts || !h_transform || !d_table)) return HIMO_ERR_INVALID_ARGUMENT;
    if (ac_misaligned(d_pts, 3u) || ac_misaligned(d_table, 15u)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n == 0) return HIMO_OK;
    uint32_t* flag = nullptr;
    const int st = ac_flag(&flag);
    if (st != HIMO_OK) return st;
    AcTransform T;
    for (int k = 0; k < 12; ++k) T.m[k] = h_transform[k];
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + kAcThreads - 1) / kAcThreads));
    if (ex) {
        {
            ProfScope ps("accum_insert_ex_kernel", s);
            hipLaunchKernelGGL(accum_insert_ex_kernel, grid, dim3(kAcThreads), 0, s, n, d_pts, pitch, d_skip, T, (uint32_t)lag, *params,
                               reinterpret_cast<uint32_t*>(d_table), (uint32_t)capacity, 32 - log2cap, flag, *ex);
        }
        HIMO_LAUNCH_CHECK("accum_insert_ex_kernel");
        return HIMO_OK;
    }
    {
        ProfScope ps("accum_insert_kernel", s);
        hipLaunchKernelGGL(accum_insert_kernel, grid, dim3(kAcThreads), 0, s, n, d_pts, pitch,
                           d_skip, T, (uint32_t)lag, *params, reinterpret_cast<uint32_t*>(d_table), (uint32_t)capacity, 32 - log2cap, flag);
    }
    HIMO_LAUNCH_CHECK("accum_insert_kernel");
    return HIMO_OK;
}

extern "C" int himo_accum_insert(int64_t n, const float* d_pts, int pitch, const unsigned char* d_skip, const float* h_transform, int lag,
                                 const himo_accum_params* params, void* d_table, int64_t capacity, void* stream) {
    return ac_insert(n, d_pts, pitch, d_skip, h_transform, lag, params, d_table, capacity, nullptr, stream);
}

extern "C" int himo_accum_insert_ex(int64_t n, const float* d_pts, int pitch, const unsigned char* d_skip, const float* h_transform, int lag,
                                    const himo_accum_params* params, void* d_table, int64_t capacity, const float* d_motion,
                                    float motion_min2, const float* d_attr, int attr_stride, float attr_scale, const int32_t* d_label,
                                    void* stream) {
    AcExtras ex;
    ex.motion = d_motion; ex.attr = d_attr; ex.label = d_label;
    ex.motion_min2 = motion_min2; ex.attr_scale = attr_scale; ex.attr_stride = attr_stride;
    return ac_insert(n, d_pts, pitch, d_skip, h_transform, lag, params, d_table, capacity, &ex, stream);
}

extern "C" int himo_accum_motion(int64_t n, const float* d_pts, int pitch, const float* d_flow, const float* h_ego, float* d_motion,
                                 void* stream) {
    if (n < 0 || (pitch != 3 && pitch != 4)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!d_pts || !d_flow || !h_ego || !d_motion)) return HIMO_ERR_INVALID_ARGUMENT;
    if (ac_misaligned(d_pts, 3u) || ac_misaligned(d_flow, 3u) || ac_misaligned(d_motion, 3u)) return HIMO_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffffLL) return HIMO_ERR_UNSUPPORTED;
    if (n == 0) return HIMO_OK;
    AcTransform E;
    for (int k = 0; k < 12; ++k) E.m[k] = h_ego[k];
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("accum_motion_kernel", s);
        hipLaunchKernelGGL(accum_motion_kernel, dim3((unsigned)((n + kAcThreads - 1) / kAcThreads)), dim3(kAcThreads), 0, s, n, d_pts, pitch,
                           d_flow, E, d_motion);
    }
    HIMO_LAUNCH_CHECK("accum_motion_kernel");
    return HIMO_OK;
}

// both emits: ex = false is v1's entry point and launches v1's instantiation
static int ac_emit(const void* d_table, int64_t capacity, const himo_accum_params* params, int64_t max_rows, int32_t* d_n_rows,
                   uint32_t* d_keys, float* d_xyz, unsigned char* d_lag, int32_t* d_count, bool ex, float attr_scale, float* d_attr,
                   int32_t* d_label, void* stream) {
    if (ex && d_attr && !(isfinite(attr_scale) && attr_scale > 0.f)) return HIMO_ERR_INVALID_ARGUMENT;
    if (ex && (ac_misaligned(d_attr, 3u) || ac_misaligned(d_label, 3u))) return HIMO_ERR_INVALID_ARGUMENT;
    if (ac_log2(capacity) < 0 || !ac_params_ok(params) || max_rows < 0 || !d_table || !d_n_rows) return HIMO_ERR_INVALID_ARGUMENT;
    if (max_rows > 0 && (!d_keys || !d_xyz || !d_lag || !d_count)) return HIMO_ERR_INVALID_ARGUMENT;
    if (ac_misaligned(d_table, 15u) || ac_misaligned(d_n_rows, 3u) || ac_misaligned(d_keys, 3u) || ac_misaligned(d_xyz, 3u) ||
        ac_misaligned(d_count, 3u))
        return HIMO_ERR_INVALID_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    HIMO_HIP(hipMemsetAsync(d_n_rows, 0, sizeof(int32_t), s));
    const int64_t slots = capacity + 1;
    const dim3 grid((unsigned)((slots + kAcThreads * kAcEmitPer - 1) / (kAcThreads * kAcEmitPer)));
    if (ex) {
        {
            ProfScope ps("accum_emit_ex_kernel", s);
            hipLaunchKernelGGL(accum_emit_ex_kernel, grid, dim3(kAcThreads), 0, s, reinterpret_cast<const uint32_t*>(d_table), slots, *params,
                               max_rows, d_n_rows, d_keys, d_xyz, d_lag, d_count, attr_scale, d_attr, d_label);
        }
        HIMO_LAUNCH_CHECK("accum_emit_ex_kernel");
        return HIMO_OK;
    }
    {
        ProfScope ps("accum_emit_kernel", s);
        hipLaunchKernelGGL(accum_emit_kernel, grid, dim3(kAcThreads), 0, s,
                           reinterpret_cast<const uint32_t*>(d_table), slots, *params, max_rows, d_n_rows, d_keys, d_xyz, d_lag, d_count);
    }
    HIMO_LAUNCH_CHECK("accum_emit_kernel");
    return HIMO_OK;
}

extern "C" int himo_accum_emit(const void* d_table, int64_t capacity, const himo_accum_params* params, int64_t max_rows, int32_t* d_n_rows,
                               uint32_t* d_keys, float* d_xyz, unsigned char* d_lag, int32_t* d_count, void* stream) {
    return ac_emit(d_table, capacity, params, max_rows, d_n_rows, d_keys, d_xyz, d_lag, d_count, false, 1.f, nullptr, nullptr, stream);
}

extern "C" int himo_accum_emit_ex(const void* d_table, int64_t capacity, const himo_accum_params* params, int64_t max_rows, int32_t* d_n_rows,
                                  uint32_t* d_keys, float* d_xyz, unsigned char* d_lag, int32_t* d_count, float attr_scale,
                                  float* d_intensity, int32_t* d_label, void* stream) {
    return ac_emit(d_table, capacity, params, max_rows, d_n_rows, d_keys, d_xyz, d_lag, d_count, true, attr_scale, d_intensity, d_label, stream);
}

extern "C" int himo_accum_status(void* stream) {
    uint32_t* flag = nullptr;
    const int st = ac_flag(&flag);
    if (st != HIMO_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    uint32_t host = 0;
    HIMO_HIP(hipMemcpyAsync(&host, flag, sizeof(host), hipMemcpyDeviceToHost, s));
    HIMO_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t), s));
    HIMO_HIP(hipStreamSynchronize(s));
    return host ? HIMO_ERR_INVALID_ARGUMENT : HIMO_OK;
}
