// The lock-free union-find of the voxel graph, shared by regions.hip (components of a mask) and superpoints.hip (region growing on normals): which
// edges join is the caller's business, how two trees are joined is one decision and lives here once.
//
// parent[v] starts as v.  A parent is always below its child, so a walk descends strictly, cannot cycle, and ends at the lowest rank of the tree;
// parents are read and written with agent-scope atomics only.  The root of a finished tree is the lowest rank of its component, whatever order the
// waves arrived in.  Every loop has a bound derived from V (a walk descends at least one rank per step; a failed hook lowers one of its two ends):
// a logic error ends as a wrong answer.
#pragma once
#include "common.h"

__device__ __forceinline__ int region_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// x's root.  Every step goes to a strictly lower rank; `budget` (shared by all walks of one hook) only ever matters if that invariant were broken.
__device__ __forceinline__ int region_find(const int* parent, int x, int& budget) {
    while (budget-- > 0) {
        const int p = region_load(parent + x);
        if (p == x) break;
        x = p;
    }
    return x;
}

// Joins the trees of a and b: both ends are walked to their roots and the higher root is hooked under the lower by compare-and-swap.
__device__ __forceinline__ void region_union(int* par, int a, int b, int V) {
    // a + b falls with every walk step and every failed hook, and both stay >= 0: 2 V + 2 rounds and 4 V + 16 loads are never reached
    int budget = 4 * V + 16;
    for (int round = 0; round < 2 * V + 2 && budget > 0; ++round) {
        a = region_find(par, a, budget);
        b = region_find(par, b, budget);
        if (a == b) break;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(&par[a], a, b);              // hook the higher root under the lower, if it still is a root
        if (old == a) break;
        a = old;                                               // somebody hooked it first, under a lower rank: go on from there
    }
}

// Shortens v's own path for the flatten pass: its root is one of its ancestors and never above its parent.
__device__ __forceinline__ void region_shorten(int* par, int v, int V) {
    int budget = V + 1;
    const int r = region_find(par, v, budget);
    if (r != v) atomicMin(&par[v], r);
}

// parent[v] = root(v), returned.  Others store roots meanwhile: still ancestors, still descending.
__device__ __forceinline__ int region_flatten(int* par, int v, int V) {
    int budget = V + 1;
    const int r = region_find(par, v, budget);
    __hip_atomic_store(&par[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return r;
}
