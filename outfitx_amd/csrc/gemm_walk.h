// The order in which the GEMM kernels' blocks walk their output tiles: one copy for every kernel (included by gemm_common.h).
// Plain integer arithmetic on scalars, nothing of HIP but the function qualifiers, so a host compiler builds it alone
// (tests/test_gemm_walk.py checks both functions over a lattice of grids).
#pragma once

#if defined(__HIP__)
#define OFX_WALK_FN __host__ __device__ inline __attribute__((always_inline))      // = __forceinline__, without needing hip_runtime.h first
#else
#define OFX_WALK_FN inline __attribute__((always_inline))
#endif

// XCD-aware bijective remap of a 1-D grid of nwg blocks.  The hardware deals consecutive block ids round robin to the 8 XCDs (blocks
// b and b + 8 share an XCD, each XCD has its own 4 MiB L2), so XCD x receives ids x, x + 8, ...  The remap hands XCD x a CONTIGUOUS
// range of remapped ids instead (the first nwg % 8 XCDs get one more): blocks that are neighbours in the walk below run on one XCD
// and find each other's operand panels in its L2.
OFX_WALK_FN int xcd_remap(int bid, int nwg) {
    const int nx = 8, q = nwg / nx, r = nwg % nx, x = bid % nx, i = bid / nx;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// Grouped rasterisation of tiles_m x tiles_n tiles: consecutive ids (= the blocks resident on one XCD at a time) cover group_m row
// panels x several column tiles, row-fastest inside the group, so BOTH the A panels and the W tiles they touch fit the XCD's 4 MiB L2
// (a plain row-major walk would stream every W tile past each row panel).  The last group holds the tiles_m % group_m left-over panels.
OFX_WALK_FN void grouped_tile(int bid, int group_m, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int per_group = group_m * tiles_n;
    const int gidx = bid / per_group, first = gidx * group_m;
    const int gm = group_m < tiles_m - first ? group_m : tiles_m - first;
    const int r = bid - gidx * per_group;
    tm = first + r % gm;
    tn = r / gm;
}
