/*
 * minigrid_obs.h -- C ABI of the observation wrappers (libtwoarmy_hip.so, <package>/csrc/minigrid_obs.hip): the
 * observations the reference's gym_minigrid/wrappers.py builds on the host, for N worlds resident in HBM, byte for
 * byte what the reference returns.
 *
 * Replaces (paths relative to the reference root)
 *   OneHotPartialObsWrapper.observation   gym_minigrid/wrappers.py:117-154   mg_obs_onehot
 *   FullyObsWrapper.observation           :220-246                           mg_obs_full
 *   FlatObsWrapper.observation            :367-425                           mg_obs_flat (the mission tail is the caller's)
 *   DirectionObsWrapper.reset/observation :463-494                           mg_obs_goal_index, mg_obs_goal_direction
 *   SymbolicObsWrapper.observation        :497-526                           mg_obs_symbolic
 *
 * Out of scope: the pixel wrappers (RGBImgObsWrapper, RGBImgPartialObsWrapper), DictObservationSpaceWrapper.
 *
 * Conventions as in minigrid_view.h / twoarmy.h: device pointers, caller-owned, `stream` = hipStream_t as void*,
 * asynchronous, 0 = ok / negative = TW_E_*; TW_E_ARG is returned before anything is launched.  World planes are
 * uint8[n_envs][height*width] with cell (x, y) at y*width + x; agent_x / agent_y / agent_dir are int32 with element e
 * at [e * agent_stride] (1 for dense arrays, TW_REC_WORDS to read TW_AX / TW_AY / TW_DIR out of the engine's records),
 * as in minigrid_render.h.  Every output leaves as aligned 16-byte stores with both ends of the written range stored
 * element by element; nothing outside the bytes named below is written.
 */
#ifndef MINIGRID_OBS_H
#define MINIGRID_OBS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OBS_ONEHOT_BITS 21     /* len(OBJECT_TO_IDX) 12 ("subgoal": 11 included) + 6 colours + 3 states */
#define MG_OBS_TYPE_BITS 12
#define MG_OBS_COLOUR_BITS 6
#define MG_OBS_SLOPE 0
#define MG_OBS_ANGLE 1

/* One-hot of an encoded image.
 *   image   uint8[n_envs][image_pitch]: n_cells * 3 bytes (type, colour, state) per row; image_pitch 0 = dense.  No
 *           alignment is asked of it.
 *   out     uint8[n_envs][out_pitch]: n_cells * 21 bytes per row, every one written 0 or 1; out_pitch 0 = dense.  No
 *           alignment is asked of out or out_pitch.
 *   error   int32[n_envs] (nullable): 0 ok, 1 an index of that env was 21 or more (the reference's IndexError).
 * The reference's index semantics, not a one-hot per field: the bytes set in a cell are those at index type,
 * 12 + colour and 18 + state, so type 12..20 lands in the colour / state fields; an index of 21 or more sets nothing.
 * TW_E_ARG: NULL image / out, n_envs <= 0, n_cells <= 0, a pitch that is neither 0 nor at least a row, a row of 2^31
 * bytes or more. */
int mg_obs_onehot(const uint8_t *image, int64_t image_pitch, int n_envs, int n_cells, uint8_t *out, int64_t out_pitch,
                  int32_t *error, void *stream);

/* Grid.encode() of the whole world with the agent stamped in.
 *   type, colour, state   world planes (state nullable = all 0)
 *   out     uint8[n_envs][out_pitch]: [width][height][3] x-major in the first width*height*3 bytes of each row;
 *           out_pitch 0 = dense.  An empty cell (plane type 0 or 1) is (1, 0, 0) as in mg_gen_obs; the agent's cell
 *           is then (10, 0, agent_dir).
 *   error   int32[n_envs] (nullable): 0 ok, 2 the agent lies outside the world (nothing is stamped).
 * TW_E_ARG: a NULL non-nullable pointer, a size <= 0, agent_stride <= 0, 0 < out_pitch < a row, width*height*3 >= 2^31. */
int mg_obs_full(const uint8_t *type, const uint8_t *colour, const uint8_t *state, int n_envs, int width, int height,
                const int32_t *agent_x, const int32_t *agent_y, const int32_t *agent_dir, int agent_stride, uint8_t *out,
                int64_t out_pitch, int32_t *error, void *stream);

/* The symbolic grid: out int32[n_envs][width][height][3] (dense, 4-byte aligned) = (x, y, idx), idx -1 for an empty
 * cell (plane type 0 or 1); no agent.  As in the reference the flat cell list (index j*width + i) is reshaped as
 * (width, height): element [x][y] holds the object at FLAT index x*height + y -- the transposed world on a square
 * grid, no transpose at all otherwise.
 * TW_E_ARG: NULL type / out, a size <= 0, out not 4-byte aligned, n_envs*width*height*3 >= 2^31. */
int mg_obs_symbolic(const uint8_t *type, int n_envs, int width, int height, int32_t *out, void *stream);

/* The flat observation: out float32[n_envs][out_pitch] (pitch in floats, 0 = dense; out 4-byte aligned) = the n_img
 * image bytes of the row widened to float, then the n_tail floats of `tail` (the one-hot of the mission string, built
 * by the caller; n_tail 0 = none, tail then nullable).  image uint8[n_envs][image_pitch], pitch 0 = dense.
 * TW_E_ARG: NULL image / out, NULL tail with n_tail > 0, n_envs <= 0, n_img <= 0, n_tail < 0, a pitch that is neither
 * 0 nor at least a row, out not 4-byte aligned, a row of 2^29 floats or more. */
int mg_obs_flat(const uint8_t *image, int64_t image_pitch, int n_envs, int n_img, const float *tail, int n_tail,
                float *out, int64_t out_pitch, void *stream);

/* goal_index int32[n_envs]: the first flat index k (= y*width + x) of a goal (type 8) in each env's plane, or -1. */
int mg_obs_goal_index(const uint8_t *type, int n_envs, int width, int height, int32_t *goal_index, void *stream);

/* Doubles in the angle table of a width x height world: (width + height - 1) * (2 * width - 1), or TW_E_ARG.
 * Entry [(p + height - 1) * (2 * width - 1) + (q + width - 1)] holds arctan(p / q) as the host's numpy evaluates it
 * (p / q in IEEE double, q = 0 included) for p in -(height-1)..width-1 and q in -(width-1)..width-1: every pair an
 * agent inside the world can produce.  Host function. */
int mg_obs_angle_table_size(int width, int height);

/* out double[n_envs]: with goal_position = (k / height, k % width) of the env's goal_index k -- the reference's mix of
 * coordinates, (2, 14) for Twoarmy's goal at (14, 2) -- p = goal_position[1] - agent_y, q = goal_position[0] - agent_x:
 *   mode MG_OBS_SLOPE   (double)p / (double)q with its IEEE result kept (-0.0, +-inf, NaN for 0 / 0)
 *   mode MG_OBS_ANGLE   angle_table[...] of (p, q) (device pointer, mg_obs_angle_table_size doubles)
 *   error   int32[n_envs] (nullable): 0 ok, 1 no goal (goal_index < 0 or >= width*height), 2 the agent lies outside
 *           the world; out is NaN for both.
 * TW_E_ARG: a NULL non-nullable pointer, angle_table NULL in mode MG_OBS_ANGLE, a size <= 0, agent_stride <= 0, another
 * mode. */
int mg_obs_goal_direction(const int32_t *goal_index, int n_envs, int width, int height, const int32_t *agent_x,
                          const int32_t *agent_y, int agent_stride, int mode, const double *angle_table, double *out,
                          int32_t *error, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MINIGRID_OBS_H */
