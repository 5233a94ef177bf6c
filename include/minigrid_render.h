/*
 * minigrid_render.h -- C ABI of the device renderer (libtwoarmy_hip.so, <package>/csrc/minigrid_render.hip): the
 * RGB frames of MiniGridEnv.get_full_render and get_pov_render for N worlds resident in HBM, byte for byte what the
 * reference draws.
 *
 * Replaces (paths relative to the reference root)
 *   gym_minigrid/rendering.py          fill_coords, point_in_rect / circle / triangle, rotate_fn, highlight_img,
 *                                      downsample (3 x 3 supersampling)
 *   Grid.render_tile                   gym_minigrid/minigrid.py:662-710
 *   Grid.render                        :712-747
 *   MiniGridEnv.get_pov_render         :1498-1512 (mg_render_pov)
 *   MiniGridEnv.get_full_render        :1514-1563 (the highlight loop :1521-1553 is mg_highlight_mask)
 *   WorldObj.render of Wall, Floor, Door (open / closed / locked), Key, Ball, Box, Goal   :357-551
 *
 * Two stages.  mg_render_build_atlas rasterises every drawable tile once per tile size, in float64 and in the
 * reference's operation order (grid lines, object, agent triangle, highlight blend at sample resolution, the
 * two-stage mean of the downsample, truncating cast); the agent's tile is the object under the agent with the triangle
 * rasterised over it BEFORE the downsample, so the atlas holds every object with every agent direction.  mg_render and
 * mg_render_pov are then pure gathers, one kernel instantiated twice: frame bytes <- atlas bytes, selected by the world
 * planes, or by the agent's rotated view of them.
 *
 * Atlas layout: MG_RENDER_TILES tiles of [tile_size][tile_size][3] bytes; tile index
 *   ((kind * 6 + colour) * 5 + (agent_dir + 1)) * 2 + highlight          agent_dir -1 = no agent
 *   kind: 0 empty (type 0 and 1), 1 wall, 2 floor, 3 door open, 4 door closed, 5 door locked, 6 key, 7 ball, 8 box,
 *         9 goal.  As WorldObj.decode does: an empty cell ignores its colour (slot 0), a goal is always green (slot 1),
 *         a door whose state is neither 0 (open) nor 2 (locked) is closed, other types ignore the state.
 *
 * Not drawn (out of scope): lava (type 9; its point_in_line mixes float32 and float64 through np.dot and
 * np.linalg.norm), type codes 10, 11 and above, colour codes above 5; the matplotlib window and render_mode="human".
 *
 * Conventions as in minigrid_view.h / twoarmy.h: device pointers, caller-owned, `stream` = hipStream_t as void*,
 * asynchronous, 0 = ok / negative = TW_E_*; TW_E_ARG is returned before anything is launched.
 */
#ifndef MINIGRID_RENDER_H
#define MINIGRID_RENDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_RENDER_KINDS 10
#define MG_RENDER_TILES (MG_RENDER_KINDS * 6 * 5 * 2)   /* 600 */
#define MG_RENDER_MAX_TILE 256                          /* tile sizes 1..256 */
#define MG_RENDER_NCONST 18

/* Atlas tile index of a cell (host function, no device needed), or -1 for a cell this renderer does not draw.
 * agent_dir -1 = no agent, else taken modulo 4; highlight 0 / non-zero. */
int mg_render_tile_index(int type, int colour, int state, int agent_dir, int highlight);

/* Bytes of the atlas for one tile size (MG_RENDER_TILES * tile_size^2 * 3), or TW_E_ARG. */
int64_t mg_render_atlas_bytes(int tile_size);

/* The 18 doubles the rasteriser takes from the host instead of computing them on the device (host function):
 * [0..3] cos(-0.5*pi*dir), [4..7] sin(-0.5*pi*dir) from libm, the values Python's math.cos / math.sin return;
 * [8..17] the agent triangle in float32 as rendering.point_in_triangle holds it, widened: a.x, a.y, v0 = c - a (x, y),
 * v1 = b - a (x, y), dot00, dot01, dot11, inv_denom = 1 / (dot00 * dot11 - dot01 * dot01), all float32 arithmetic. */
int mg_render_constants(double *out18);

/* Rasterise all MG_RENDER_TILES tiles of `tile_size` into atlas (device, mg_render_atlas_bytes(tile_size) bytes). */
int mg_render_build_atlas(int tile_size, uint8_t *atlas, void *stream);

/* Grid.render for n_out frames.
 *   type, colour, state   uint8[n_envs][height*width], cell (x, y) at y*width + x (state nullable = all 0)
 *   agent_x, agent_y, agent_dir   int32, element e of env e at [e * agent_stride]: agent_stride 1 for dense arrays,
 *                         TW_REC_WORDS to read TW_AX / TW_AY / TW_DIR straight out of the engine's records.  An agent
 *                         outside the world is not drawn; agent_dir is taken modulo 4.
 *   env_index             int32[n_out], frame o shows env env_index[o] (any order, repeats allowed); NULL = frame o
 *                         shows env o (n_out <= n_envs)
 *   highlight             uint8[n_envs][height*width] in world coordinates, non-zero = highlighted (nullable = none)
 *   atlas                 mg_render_build_atlas(tile_size) output
 *   frame                 uint8[n_out][frame_pitch]: the [height*tile_size][width*tile_size][3] image in the first
 *                         height*width*tile_size^2*3 bytes of each row; frame_pitch 0 = dense.  No alignment is asked
 *                         of frame or frame_pitch; nothing outside those bytes is written (the body goes out as
 *                         aligned 16-byte stores, both ends of every frame byte by byte).
 *   error                 int32[n_out] (nullable): 0 ok; 1 the world holds a cell this renderer does not draw (such a
 *                         cell is drawn as an empty tile); 2 env_index[o] is outside 0..n_envs-1 (the frame is left
 *                         untouched).
 * TW_E_ARG: a NULL non-nullable pointer, a size <= 0, tile_size outside 1..MG_RENDER_MAX_TILE, agent_stride <= 0,
 * env_index NULL with n_out > n_envs, 0 < frame_pitch < frame bytes, a frame of 2^31 bytes or more. */
int mg_render(const uint8_t *type, const uint8_t *colour, const uint8_t *state, int n_envs, int width, int height,
              const int32_t *agent_x, const int32_t *agent_y, const int32_t *agent_dir, int agent_stride,
              const int32_t *env_index, int n_out, const uint8_t *highlight, const uint8_t *atlas, int tile_size,
              uint8_t *frame, int64_t frame_pitch, int32_t *error, void *stream);

/* get_pov_render for n_out frames: Grid.render of the V x V grid gen_obs_grid returns, V = view_size.
 *   type, colour, state, agent_*, agent_stride, env_index, atlas, error: as in mg_render, except that ANY agent position
 *                         is valid (Grid.slice pads the window with walls) and agent_dir is taken modulo 4 as mg_gen_obs
 *                         takes it
 *   view cell (i, j)      shows the world cell mg_gen_obs puts there (get_view_exts, agent_dir + 1 rotate_left calls); a
 *                         world cell outside the world is a grey wall (2, 5, 0).  The agent's own cell (V / 2, V - 1)
 *                         shows the carried object under the agent triangle of direction 3, whatever the mask says
 *                         there.  Every other cell the mask hides is drawn as an empty, unlit tile: process_vis clears
 *                         such cells in the grid gen_obs_grid returns (minigrid.py:827-830), so the reference's picture
 *                         does not show them.
 *   carrying              uint8[n_envs][3] = WorldObj.encode() of the carried object, type 0 = nothing (nullable)
 *   vis_mask              uint8[n_envs][V*V] indexed [i][j] as mg_gen_obs emits it: cell (i, j) is highlighted iff
 *                         non-zero; NULL = every cell (see_through_walls)
 *   frame                 uint8[n_out][frame_pitch]: the [V*tile_size][V*tile_size][3] image, view cell (i, j) at pixel
 *                         rows j*tile_size.. and pixel columns i*tile_size.., in the first V*V*tile_size^2*3 bytes of
 *                         each row; alignment and the bytes written as in mg_render
 *   error                 1: a view cell the mask does not hide (the carried object included) is one this renderer does
 *                         not draw; 2 as in mg_render
 * TW_E_ARG as in mg_render, and for view_size outside 1..MG_MAX_VIEW. */
int mg_render_pov(const uint8_t *type, const uint8_t *colour, const uint8_t *state, int n_envs, int width, int height,
                  const int32_t *agent_x, const int32_t *agent_y, const int32_t *agent_dir, int agent_stride,
                  const uint8_t *carrying, const int32_t *env_index, int n_out, const uint8_t *vis_mask, int view_size,
                  const uint8_t *atlas, int tile_size, uint8_t *frame, int64_t frame_pitch, int32_t *error, void *stream);

/* The highlight loop of get_full_render (minigrid.py:1521-1553): view-space vis_mask uint8[n_envs][V*V] indexed [i][j]
 * as mg_gen_obs emits it (NULL = every view cell visible, Twoarmy's see_through_walls) -> world-space
 * out uint8[n_envs][height*width] (1 / 0, cell (x, y) at y*width + x); view cells outside the world are dropped.
 * Every byte of `out` is written.  view_size 1..MG_MAX_VIEW; agent_* as in mg_render. */
int mg_highlight_mask(const uint8_t *vis_mask, int n_envs, int width, int height, const int32_t *agent_x,
                      const int32_t *agent_y, const int32_t *agent_dir, int agent_stride, int view_size, uint8_t *out,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MINIGRID_RENDER_H */
