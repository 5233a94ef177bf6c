// view_map.h -- the agent's view window in closed form, shared by minigrid_view.hip
// (mg_gen_obs) and minigrid_render.hip (mg_render_pov): get_view_exts (minigrid.py:1262-1293) and the agent_dir + 1
// rotate_left calls of gen_obs_grid (:1455-1458) as an index map.
#ifndef TWOARMY_VIEW_MAP_H
#define TWOARMY_VIEW_MAP_H
#include <hip/hip_runtime.h>

// Top-left world cell of the V x V window Grid.slice cuts for an agent at (ax, ay) facing dir (0 right, 1 down, 2 left,
// 3 up); the window may reach outside the world.
__device__ __forceinline__ void mg_view_top(int ax, int ay, int dir, int V, int &topx, int &topy) {
    const int half = V / 2;
    topx = dir == 0 ? ax : (dir == 2 ? ax - V + 1 : ax - half);
    topy = dir == 1 ? ay : (dir == 3 ? ay - V + 1 : ay - half);
}

// View cell (i, j) <- window cell (si, sj) after k = (dir + 1) & 3 applications of rotate_left, which maps old (a, b)
// to new (b, V-1-a); inverted k times.
__device__ __forceinline__ void mg_view_to_slice(int k, int V, int i, int j, int &si, int &sj) {
    si = k == 0 ? i : (k == 1 ? V - 1 - j : (k == 2 ? V - 1 - i : j));
    sj = k == 0 ? j : (k == 1 ? i : (k == 2 ? V - 1 - j : V - 1 - i));
}

// The inverse: window cell (si, sj) -> view cell (i, j); inside the view exactly when the window cell is inside the window.
__device__ __forceinline__ void mg_view_from_slice(int k, int V, int si, int sj, int &i, int &j) {
    i = (k & 1) ? sj : si;                                  // k odd swaps the axes; then i flips for k = 2, 3,
    j = (k & 1) ? si : sj;                                  // j for k = 1, 2
    if (k & 2) i = V - 1 - i;
    if ((k + 1) & 2) j = V - 1 - j;
}

#endif  // TWOARMY_VIEW_MAP_H
