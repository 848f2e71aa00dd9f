// unionfind.h -- what the clustering kernels (dbscan.hip, hdbscan.hip) share: which rows take part, and the lock-free union-find:
// components over point indices, hooked with atomicMin so that a component's root ends as its lowest index, whatever the order the
// hooks land in.
#pragma once
#include <hip/hip_runtime.h>

namespace himo {

// whether row i takes part in the clustering: not flagged in `skip` and no NaN coordinate (both stages give such a row label 0)
__device__ inline bool db_takes_part(const float* __restrict__ xyz, int pitch, const unsigned char* __restrict__ skip, int i) {
    const float x = xyz[(int64_t)i * pitch], y = xyz[(int64_t)i * pitch + 1], z = xyz[(int64_t)i * pitch + 2];
    return !(skip && skip[i]) && x == x && y == y && z == z;
}

__device__ inline int db_find(const int* __restrict__ parent, int x) {
    int p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    return x;
}
// find with path halving: every visited node is re-pointed at its grandparent.  Safe without locks beside the atomicMin hooks below:
// a store only ever targets a NON-root (its parent differs from itself, and a hooked node never becomes a root again) and writes an
// ancestor of that node -- a lower index of the same component -- so no link a hook relies on is lost (a hook onto a non-root
// re-joins that node's old parent itself, see db_union) and no cycle can form.  Components, and their lowest index, are unchanged;
// the trees become flat, which is what the second and later unions of a dense object's points wait for
__device__ inline int db_find_halve(int* __restrict__ parent, int x) {
    int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        const int gp = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gp != p) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p; p = gp;
    }
    return x;
}
__device__ inline void db_union(int* __restrict__ parent, int a, int b) {
    while (true) {
        a = db_find_halve(parent, a); b = db_find_halve(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }            // hook the larger root a under the smaller b
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;                                   // a was still a root: hooked
        a = old;                                                // somebody hooked a meanwhile: carry on from there
    }
}

}  // namespace himo
