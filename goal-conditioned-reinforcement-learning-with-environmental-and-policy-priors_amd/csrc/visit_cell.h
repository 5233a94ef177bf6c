// visit_cell.h -- device routines shared by visitation.hip and exploration_bonus.hip: the cell of a position and the
// wavefront-grouped LDS histogram add.
#ifndef TWOARMY_VISIT_CELL_H
#define TWOARMY_VISIT_CELL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int VISIT_MAX_SIDE = 32;
constexpr int VISIT_GROUP_ROUNDS = 4;

// values_matrix[y][x] of heatmap.py:63, row-major; every position outside the grid (NaN and +-inf fail the float
// comparisons) is the extra bin width * height.
__device__ __forceinline__ int visit_cell(float y, float x, int width, int height) {
    const bool ok = y >= 0.f && y < (float)height && x >= 0.f && x < (float)width;
    return ok ? (int)y * width + (int)x : width * height;
}

__host__ __device__ inline bool visit_grid_ok(int width, int height) {
    return width >= 1 && width <= VISIT_MAX_SIDE && height >= 1 && height <= VISIT_MAX_SIDE;
}

// hist[c] += 1 for every pending lane of a wavefront, equal bins grouped first: the lowest pending lane broadcasts its
// bin, the lanes that hold the same bin are counted with one ballot, and the leader adds the count once.
// VISIT_GROUP_ROUNDS such rounds take the few crowded bins; whatever is still pending after them is spread thinly and
// goes through plain LDS adds.  Every lane of the wavefront must call this (the ballots need all of them).
__device__ __forceinline__ void visit_grouped_add(uint32_t *hist, int c, bool pending, int lane) {
#pragma unroll
    for (int r = 0; r < VISIT_GROUP_ROUNDS; ++r) {
        const unsigned long long todo = __ballot(pending);
        if (todo == 0ull) break;
        const int leader = __ffsll(todo) - 1;
        const int lc = __shfl(c, leader, 64);
        const unsigned long long same = __ballot(pending && c == lc);
        if (lane == leader) atomicAdd(&hist[lc], (uint32_t)__popcll(same));
        if (c == lc) pending = false;
    }
    if (pending) atomicAdd(&hist[c], 1u);
}

#endif  // TWOARMY_VISIT_CELL_H
