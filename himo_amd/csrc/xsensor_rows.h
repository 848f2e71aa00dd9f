// xsensor_rows.h -- the ONE statement of rules A and B of "cross-sensor consistency, v1" (himo_amd/eval_xsensor.py): which sorted rows
// are USABLE, how they are staged, the counts per sensor, and the state and live groups those counts give (device code), and the
// host checks of offsets and alignment that both entry points make.
// xsensor.hip scores the clusters by it; xalign.hip ("cross-sensor alignment, v1") takes the same rows, groups and states, word for word.
#pragma once
#include "himo_common.h"
#include "blockops.h"

namespace himo {

constexpr int kXsThreads = 256;
constexpr int kXsGroups = HIMO_XSENSOR_GROUPS;
static_assert(kXsGroups == 8, "xsensor groups");

__device__ inline bool xs_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// rule B from a cluster's eight counts: the state, n and the live mask
__device__ inline int xs_state(const int32_t* __restrict__ c, int min_group, int min_points, int max_points, int& n, int& live) {
    const int4 a = *reinterpret_cast<const int4*>(c), b = *reinterpret_cast<const int4*>(c + 4);
    const int g[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    n = 0; live = 0;
    int lives = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        n += g[k];
        if (g[k] >= min_group) { live |= 1 << k; ++lives; }
    }
    if (n < min_points) return HIMO_XSENSOR_TOO_FEW;
    if (n > max_points) return HIMO_XSENSOR_TOO_LARGE;
    if (lives < 2) return HIMO_XSENSOR_ONE_SENSOR;
    return HIMO_XSENSOR_SCORED;
}

// the sorted rows of cluster k (validated on the host; clamped all the same)
__device__ inline void xs_range(const int64_t* __restrict__ offsets, int nc, int k, int& lo, int& hi) {
    int64_t a = offsets[k], b = offsets[k + 1];
    a = a < 0 ? 0 : (a > nc ? nc : a);
    b = b < a ? a : (b > nc ? nc : b);
    lo = (int)a; hi = (int)b;
}

// rule A for sorted row i (< the sorted rows of the call): x, y, z and 1 << group as the bits of w when the row is USABLE, its count
// added to the table cnt [C][8]; zeros, whose bit test never passes, when it is not.  dt may be NULL.
__device__ inline float4 xs_stage_row(int64_t n, const float* __restrict__ pts, int pitch, const int32_t* __restrict__ labels,
                                      const uint8_t* __restrict__ group, const float* __restrict__ dt, const int64_t* __restrict__ rows,
                                      const int64_t* __restrict__ offsets, int C, int i, int32_t* cnt) {
    const int64_t r = rows[i];
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r >= 0 && r < n) {
        const int lab = labels[r];
        const unsigned g = group[r];
        const float* row = pts + r * pitch;
        const float x = row[0], y = row[1], z = row[2];
        bool ok = lab >= 1 && lab <= C && g < (unsigned)kXsGroups && xs_finite(x) && xs_finite(y) && xs_finite(z);
        if (ok && dt) ok = xs_finite(dt[r]);
        if (ok) {
            out = make_float4(x, y, z, __int_as_float(1 << g));
            atomicAdd(&cnt[kXsGroups * (size_t)segment_of(offsets, C, i) + g], 1);
        }
    }
    return out;
}

// ---- host side: what both entry points refuse alike ----
// segment offsets [C + 1] on the host: start at 0, never decrease, end at n
inline bool xs_offsets_ok(int64_t n, int C, const int64_t* h) {
    if (h[0] != 0 || h[C] != n) return false;
    for (int k = 0; k < C; ++k)
        if (h[k] < 0 || h[k + 1] < h[k]) return false;
    return true;
}

inline bool xs_misaligned(const void* q, uintptr_t al) { return (reinterpret_cast<uintptr_t>(q) & (al - 1)) != 0; }

}  // namespace himo
