/*
 * minigrid_nav.h -- C ABI of the shortest-path kernels (libtwoarmy_hip.so, <package>/csrc/minigrid_nav.hip): how many
 * moves every cell of N grid worlds lies from the goal, and which move an agent on a shortest path makes next.
 *
 * The reference has nothing of the kind (its progress signals are the sparse return and the visited cells); on the host
 * this is one breadth-first search per env and query.  Here it is one launch for all envs.
 *
 * Conventions as in minigrid_view.h / minigrid_obs.h: device pointers, caller-owned, `stream` = hipStream_t as void*,
 * asynchronous, 0 = ok / negative = TW_E_*; TW_E_ARG is returned before anything is launched.
 *
 * World and moves.  The world is the `type` / `state` planes of minigrid_view.h: uint8[n_envs][height*width], cell
 * (x, y) at y*width + x, `state` nullable (NULL = every door open).  1 <= width, height <= MG_NAV_MAX_SIDE.  Moves are
 * the four absolute moves of mg_step: 0 left (x - 1), 1 right (x + 1), 2 up (y - 1), 3 down (y + 1).
 *
 * Enterable cells.  A cell is enterable iff bit `type` of the 16-bit mask pass_types is set; a door (type 4) must in
 * addition be open (state == 0) unless MG_NAV_DOORS_OPEN is given; a type code >= 16 is never enterable.
 * MG_NAV_PASS_DEFAULT is the rule of mg_step (mg_step_kernel, csrc/minigrid_view.hip): types 0, 1 (empty), 3 (floor),
 * 8 (goal), 9 (lava), 11 (subgoal) and open doors.  Clear bit 9 to keep out of the lava; set bit 6 to walk through the
 * balls (the prior of the static map).
 *
 * Sources.  goal_x / goal_y: int32, env e at [e * goal_stride], one source cell per env.  Both NULL: the sources are
 * all cells of type 8 (goal) of that env -- a multi-source search.
 *
 * Distance.  dist[c] = the least number of moves from cell c to a source through enterable cells only.  A source is 0,
 * but only if it is enterable itself.  Every cell that is not enterable or not connected to a source is
 * MG_NAV_UNREACHABLE.  Distances are uint16 (a serpentine in a 32 x 32 world is longer than 255 moves).
 *
 * Expert action of an agent at (agent_x, agent_y) (int32, env e at [e * agent_stride]): 6 (done / stay) at distance
 * 0; otherwise the first of 0 left, 1 right, 2 up, 3 down whose neighbour cell has distance dist - 1; -1 if the agent's
 * cell is unreachable.  agent_dist is the distance of the agent's cell as int32 (MG_NAV_UNREACHABLE = 65535 included).
 *
 * error int32[n_envs] (nullable), one code per env, the first that applies of
 *   2  a given source lies outside the world             (the whole field is MG_NAV_UNREACHABLE)
 *   1  no source: no goal cell in the plane, or no source that is enterable   (the same)
 *   3  the agent lies outside the world: agent_dist = MG_NAV_UNREACHABLE, agent_action = -1, the field is computed
 *   0  ok
 *
 * Reads.  The planes are read as 4-byte-aligned words, as mg_gen_obs reads them: the words that hold the first and the
 * last byte of a plane array are read whole, i.e. up to 3 bytes before its start / after its end inside the same
 * aligned word (always inside the caller's allocation when that starts and ends on 4-byte boundaries, as hipMalloc /
 * torch allocations do).  Those neighbour bytes never reach a result.
 * Writes.  Each field row leaves as aligned 16-byte stores (8 distances), its first and last chunk element by element
 * (csrc/row_store.h); dist needs 2-byte alignment only, and nothing outside the first width*height elements of a row
 * is written.
 */
#ifndef MINIGRID_NAV_H
#define MINIGRID_NAV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_NAV_MAX_SIDE 32
#define MG_NAV_UNREACHABLE 0xFFFF
#define MG_NAV_PASS_DEFAULT 0x0B1B   /* bits 0, 1, 3, 4 (doors: open ones), 8, 9, 11 */
#define MG_NAV_DOORS_OPEN 1          /* flags: treat every door as open, whatever `state` says */
#define MG_NAV_ACTION_STAY 6
#define MG_NAV_ACTION_NONE (-1)

/* One launch: the field of every env and / or the distance and expert action of its agent.
 *   dist          uint16[n_envs][dist_pitch] (nullable; dist_pitch in elements, 0 = dense width*height)
 *   agent_dist    int32[n_envs] (nullable), agent_action int32[n_envs] (nullable): need agent_x and agent_y
 * With dist NULL and the agent outputs given nothing but those 8 bytes per env (and error) is written.
 * TW_E_ARG: n_envs <= 0, a side <= 0 or > MG_NAV_MAX_SIDE, NULL type, pass_types > 0xFFFF, flags other than
 * MG_NAV_DOORS_OPEN, 0 < dist_pitch < width*height or dist_pitch < 0, dist not 2-byte aligned, only one of goal_x /
 * goal_y or of agent_x / agent_y, agent outputs without agent arrays, a stride <= 0 of arrays that are given. */
int mg_nav_field(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height, uint32_t pass_types,
                 int flags, const int32_t *goal_x, const int32_t *goal_y, int goal_stride, const int32_t *agent_x,
                 const int32_t *agent_y, int agent_stride, uint16_t *dist, int64_t dist_pitch, int32_t *agent_dist,
                 int32_t *agent_action, int32_t *error, void *stream);

/* The distance at every step of a rollout from ONE field per env: pos float[T][n_envs][2] = (y, x) after each step
 * (8-byte aligned), the stream ppo_visit_hist reads, with its cell rule (csrc/visit_cell.h: truncation inside the
 * world; NaN, +-inf and everything outside are no cell); out uint16[T][n_envs] = dist[n][cell], or
 * MG_NAV_UNREACHABLE for a position outside the world.  One launch; T == 0 launches nothing.
 * TW_E_ARG: NULL dist / pos / out, n_envs <= 0, T < 0, a side <= 0 or > MG_NAV_MAX_SIDE, 0 < dist_pitch < width*height
 * or dist_pitch < 0, dist or out not 2-byte aligned, pos not 8-byte aligned, T * n_envs >= 2^40. */
int mg_nav_lookup(const uint16_t *dist, int64_t dist_pitch, int n_envs, int width, int height, const float *pos, int T,
                  uint16_t *out, void *stream);

/* The SET of optimal moves at every acting state of a rollout, from ONE field per env (as mg_nav_lookup takes it).
 *   pos       float[T][n_envs][2] = (y, x) BEFORE step t (8-byte aligned)
 *   age       int32[T][n_envs] (nullable): steps taken in the running episode before step t
 *   init_pos  float[2] on the device, the position after a reset; required when age is given
 * The acting position of (t, n) is age[t][n] <= 0 ? init_pos : pos[t][n] -- the rule by which ppo_gather_stack fills the
 * newest slot of a stack -- and its cell comes from the rule of the visit counters (csrc/visit_cell.h), as in
 * mg_nav_lookup.  With d = the distance of that cell:
 *   moves uint8[T][n_envs]:  bit k (k = 0..3: left, right, up, down, the moves of mg_step) is set iff the neighbour in
 *       direction k lies inside the world and has distance d - 1; bit MG_NAV_MOVE_STAY_BIT (and no other) is set iff
 *       d == 0; the value is 0 where the position is no cell or the cell is MG_NAV_UNREACHABLE.
 *   acting_dist uint16[T][n_envs] (nullable): d, or MG_NAV_UNREACHABLE where the position is no cell.
 * Invariant: the lowest set bit of moves, with bit 4 read as MG_NAV_ACTION_STAY, is the agent_action mg_nav_field
 * reports for an agent on that cell of the same field; 0 corresponds to MG_NAV_ACTION_NONE.
 * One launch; T == 0 launches nothing.  Both outputs leave as aligned 16-byte stores, element by element only in the
 * first and last chunk of a workgroup's share (csrc/row_store.h); moves needs no alignment, and nothing outside the
 * first T * n_envs elements of either output is written.
 * TW_E_ARG: NULL dist / pos / moves, n_envs <= 0, T < 0, a side <= 0 or > MG_NAV_MAX_SIDE, 0 < dist_pitch < width*height
 * or dist_pitch < 0, dist or acting_dist not 2-byte aligned, pos not 8-byte aligned, age or init_pos not 4-byte aligned,
 * age without init_pos, T * n_envs >= 2^40. */
#define MG_NAV_MOVE_STAY_BIT 4
int mg_nav_optimal_moves(const uint16_t *dist, int64_t dist_pitch, int n_envs, int width, int height, const float *pos,
                         const int32_t *age, const float *init_pos, int T, uint8_t *moves, uint16_t *acting_dist,
                         void *stream);

/* The same move sets for records that each name their OWN goal (hindsight records): one launch floods the goal of every
 * run of records on the device and labels the run, and no field reaches memory.
 *   rec_t, rec_n  int32[n_records]: the step and the env of a record;  rec_goal float[n_records][2] = (y, x): its goal
 *                 -- the t, n and goal arrays ppo_her_relabel writes (twoarmy_ppo.h)
 *   pos, age, init_pos, T: exactly as in mg_nav_optimal_moves (pos BEFORE step t; the acting position of record b is
 *                 age[t][n] <= 0 ? init_pos : pos[t][n] with t = rec_t[b], n = rec_n[b])
 *   type, state, n_envs, width, height, pass_types, flags: the world, its moves and its enterable cells exactly as in
 *                 mg_nav_field (state nullable)
 * The goal cell and the acting cell come from the rule of the visit counters (visit_cell, csrc/visit_cell.h).  Per
 * record: the result of record b depends on record b alone, never on its neighbours, the order of the records or how
 * they are grouped.  Let F be the field mg_nav_field computes for env rec_n[b] with the goal cell as its single source;
 * moves[b] and acting_dist[b] are what mg_nav_optimal_moves gives for the acting cell in F: bits 0..3 set iff that
 * neighbour lies inside the world and one move nearer, bit MG_NAV_MOVE_STAY_BIT alone at distance 0, the value 0 where
 * the acting cell is unreachable.
 * moves[b] = 0 and acting_dist[b] = MG_NAV_UNREACHABLE when rec_t[b] is outside [0, T), rec_n[b] is outside
 * [0, n_envs), the goal is no cell (NaN, +-inf, outside the world), the goal cell is not enterable, or the acting
 * position is no cell.  No such record addresses any memory outside its arrays.
 *   moves uint8[n_records];  acting_dist uint16[n_records] (nullable)
 * Invariant: for records that share one goal per env the outputs equal mg_nav_field(goal_x, goal_y) followed by
 * mg_nav_optimal_moves on the same positions.
 * One launch, no atomics; n_records == 0 returns 0 and launches nothing.  A workgroup owns 1024 consecutive records and
 * floods once per run of equal (env, goal cell) among them, so records sorted into such runs (ppo_her_relabel's
 * emission order) cost the fewest floods; the results do not depend on it.
 * Reads: the planes by the over-read rule above (the aligned words that hold the first and the last byte of a world
 * row are read whole).  Writes: both outputs leave as aligned 16-byte stores, element by element only in the first and
 * last chunk of a workgroup's share (csrc/row_store.h); moves needs no alignment, and nothing outside the first
 * n_records elements of either output is written.
 * TW_E_ARG: NULL type / rec_t / rec_n / rec_goal / pos / moves, n_envs <= 0, a side <= 0 or > MG_NAV_MAX_SIDE,
 * pass_types > 0xFFFF, flags other than MG_NAV_DOORS_OPEN, pos not 8-byte aligned, rec_t, rec_n, rec_goal, age or
 * init_pos not 4-byte aligned, acting_dist not 2-byte aligned, age without init_pos, T < 0, n_records < 0,
 * n_records >= 2^40. */
int mg_nav_goal_moves(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                      uint32_t pass_types, int flags, const int32_t *rec_t, const int32_t *rec_n,
                      const float *rec_goal, int64_t n_records, const float *pos, const int32_t *age,
                      const float *init_pos, int T, uint8_t *moves, uint16_t *acting_dist, void *stream);

/* ---- Time-expanded fields: blockers that move with a period (the balls of Twoarmy's door gap).
 *
 * The world, the moves, the enterable cells, pass_types, flags, the sources (a given cell per env, or all goal cells)
 * and the over-read rule are exactly those of mg_nav_field.  New are a period P, 1 <= P <= MG_NAV_MAX_PERIOD, and a
 * schedule of the cells that are occupied at each of the P phases.
 *
 * Schedule.  blocked: uint32[.][P][height] (4-byte aligned); word y of phase p has bit x set iff cell (x, y) is occupied
 * at phase p.  Bits at or above `width` are ignored.  blocked_env_stride, in words: 0 = one schedule shared by all envs;
 * otherwise it is at least P*height and env e reads from e*blocked_env_stride.
 *
 * Free cells.  free[p] = the enterable cells that are not blocked at phase p.
 *
 * Transition.  From (c, p) the agent goes to (c', (p + 1) mod P), where c' is c itself (it waits) or one of c's four
 * neighbours inside the world; the transition exists iff c' is in free[(p + 1) mod P].  This one condition says all of:
 * the blockers move before the agent does, a blocker keeps the agent out of its cell, and a blocker that moves onto a
 * waiting agent hits it.
 *
 * Distance.  dist[p][c] = the least number of transitions from (c, p) to any state whose cell is a source.  It is
 * defined for c in free[p] only: a source in free[p] is 0, every other state -- not free, or with no path to a source
 * -- is MG_NAV_UNREACHABLE.  Distances are below width*height*P <= 16384.
 *
 * Phase from the clock.  The phase of a clock value k (int32) is k <= 0 ? 0 : k mod P -- the rule by which `age` selects
 * init_pos in mg_nav_optimal_moves.  The engine's TW_STEP_MOVE word and the trainer's age array are such clocks.
 *
 * Expert action at (c, p) with d = dist[p][c]: 6 if d == 0; otherwise the first of 0 left, 1 right, 2 up, 3 down whose
 * c' lies inside the world and has dist[(p + 1) mod P][c'] == d - 1; otherwise 6 (wait: then dist[(p + 1) mod P][c] ==
 * d - 1 holds); -1 if d is MG_NAV_UNREACHABLE.  Move set: bits 0..3 on the same condition as the four moves, bit
 * MG_NAV_MOVE_STAY_BIT iff d == 0 (then alone) or waiting is optimal.  Invariant: the lowest set bit of the move set,
 * with bit 4 read as 6, is the expert action; a move set of 0 corresponds to -1.
 *
 * error: the codes of mg_nav_field; 1 = no source that is free at any phase (the whole field is MG_NAV_UNREACHABLE). */
#define MG_NAV_MAX_PERIOD 16

/* One launch for all envs: the P fields of every env and / or the distance and expert action of its agent.
 *   dist         uint16[n_envs][P][dist_pitch] (nullable; dist_pitch in elements, 0 = dense width*height); each of the
 *                n_envs * P rows is written as mg_nav_field writes a row
 *   agent_clock  int32, env e at [e * agent_stride] like agent_x / agent_y (nullable: phase 0)
 *   agent_dist, agent_action int32[n_envs] (nullable): need agent_x and agent_y
 * The flood ends after at most width*height*P rounds whatever the input.
 * TW_E_ARG: the cases of mg_nav_field; period outside 1..MG_NAV_MAX_PERIOD; NULL or misaligned blocked;
 * blocked_env_stride < 0 or 0 < blocked_env_stride < P*height; agent_clock without agent_x / agent_y. */
int mg_nav_timed_field(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                       uint32_t pass_types, int flags, const uint32_t *blocked, int64_t blocked_env_stride, int period,
                       const int32_t *goal_x, const int32_t *goal_y, int goal_stride, const int32_t *agent_x,
                       const int32_t *agent_y, const int32_t *agent_clock, int agent_stride, uint16_t *dist,
                       int64_t dist_pitch, int32_t *agent_dist, int32_t *agent_action, int32_t *error, void *stream);

/* mg_nav_optimal_moves for a timed field: dist uint16[n_envs][P][dist_pitch] as mg_nav_timed_field writes it, and age
 * (required, with init_pos) is also the clock: the state of (t, n) is the acting cell -- age[t][n] <= 0 ? init_pos :
 * pos[t][n], by the rule of the visit counters -- at the phase of age[t][n].
 *   moves uint8[T][n_envs]: the move set above; 0 where the position is no cell or the state is unreachable.
 *   acting_dist uint16[T][n_envs] (nullable): the state's distance; MG_NAV_UNREACHABLE in the same places.
 * One launch; T == 0 launches nothing.  Stores, alignment and sizes as in mg_nav_optimal_moves.
 * TW_E_ARG: the cases of mg_nav_optimal_moves; NULL age or init_pos; period outside 1..MG_NAV_MAX_PERIOD. */
int mg_nav_timed_moves(const uint16_t *dist, int64_t dist_pitch, int period, int n_envs, int width, int height,
                       const float *pos, const int32_t *age, const float *init_pos, int T, uint8_t *moves,
                       uint16_t *acting_dist, void *stream);

/* mg_nav_goal_moves over (cell, phase): the timed move sets of records that each name their OWN goal (hindsight records
 * of a world whose blockers move).  One launch floods the goal of every run of records over (cell, phase) on the device
 * and labels the run; no field reaches memory.
 *   type, state, n_envs, width, height, pass_types, flags: the world, its moves, its enterable cells and the over-read
 *                 rule exactly as in mg_nav_field (state nullable)
 *   blocked, blocked_env_stride, period: the schedule; free cells, transition, distance, phase from the clock, move set
 *                 and stay bit exactly as in the "time-expanded fields" block above
 *   rec_t, rec_n, rec_goal, n_records, pos, age, init_pos, T: the records and the acting positions exactly as in
 *                 mg_nav_goal_moves, except that age and init_pos are REQUIRED, as in mg_nav_timed_moves, and
 *                 age[t][n] is also the record's clock (t = rec_t[b], n = rec_n[b])
 * Per record: the result of record b depends on record b alone, never on its neighbours, the order of the records or how
 * they are grouped.  Let F be what mg_nav_timed_field computes for env rec_n[b] with the record's goal cell (visit_cell
 * of rec_goal[b]) as its single source -- a source is 0 in every phase in which it is free.  moves[b] and acting_dist[b]
 * are what mg_nav_timed_moves gives in F for the acting cell (age[t][n] <= 0 ? init_pos : pos[t][n], by the rule of the
 * visit counters) at the phase of age[t][n]: bits 0..3 set iff that neighbour lies inside the world and one transition
 * nearer at the next phase, bit MG_NAV_MOVE_STAY_BIT iff the distance is 0 (then alone) or waiting is optimal.
 * moves[b] = 0 and acting_dist[b] = MG_NAV_UNREACHABLE when rec_t[b] is outside [0, T), rec_n[b] is outside
 * [0, n_envs), the goal is no cell (NaN, +-inf, outside the world), the goal cell is free at no phase, the acting
 * position is no cell, or the state is unreachable (the acting cell is not free at its phase, or no path exists).  No
 * such record addresses any memory outside its arrays.
 *   moves uint8[n_records];  acting_dist uint16[n_records] (nullable)
 * Invariants: (a) for records that share one goal per env the outputs equal mg_nav_timed_field(goal_x, goal_y) followed
 * by mg_nav_timed_moves on the same positions; (b) with period = 1 and an all-zero schedule the outputs equal
 * mg_nav_goal_moves'.
 * One launch, no atomics; n_records == 0 returns 0 and launches nothing.  A workgroup owns 1024 consecutive records and
 * floods once per run of equal (env, goal cell) among them -- the phase is no part of the key, one flood serves the
 * records of every phase -- so records in ppo_her_relabel's emission order cost the fewest floods; the results do not
 * depend on it.  A flood ends after at most width*height*P rounds whatever the input.  Every (width, height, period)
 * the limits allow works: how many of a workgroup's 8 half wavefronts flood at a time (mg_nav_timed_goal_floods) follows
 * from the size of one image, P * width*height distances.
 * Reads and writes as in mg_nav_goal_moves: the planes by the over-read rule, both outputs as aligned 16-byte stores,
 * element by element only in the first and last chunk of a workgroup's share; moves needs no alignment, and nothing
 * outside the first n_records elements of either output is written.
 * TW_E_ARG: the cases of mg_nav_goal_moves; NULL age or init_pos; period outside 1..MG_NAV_MAX_PERIOD; NULL or
 * misaligned blocked; blocked_env_stride < 0 or 0 < blocked_env_stride < P*height. */
int mg_nav_timed_goal_moves(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                            uint32_t pass_types, int flags, const uint32_t *blocked, int64_t blocked_env_stride,
                            int period, const int32_t *rec_t, const int32_t *rec_n, const float *rec_goal,
                            int64_t n_records, const float *pos, const int32_t *age, const float *init_pos, int T,
                            uint8_t *moves, uint16_t *acting_dist, void *stream);

/* Host only, no launch: how many floods a workgroup of mg_nav_timed_goal_moves runs at a time at this size and period --
 * 8, 4, 2 or 1, the most whose images fit 64 KiB of LDS next to the workgroup's staging (32 x 32 with P = 16: 1).
 * TW_E_ARG: a side <= 0 or > MG_NAV_MAX_SIDE, period outside 1..MG_NAV_MAX_PERIOD. */
int mg_nav_timed_goal_floods(int width, int height, int period);

/* ---- Reward shaping: the distance as a potential (Ng, Harada, Russell 1999).
 *
 * r' = r + gamma * Phi(s') - Phi(s) with Phi(s) = -scale * dist(s).  The world, moves, enterable cells, fields, visit_cell
 * rule, acting-position rule (age <= 0 ? init_pos : pos) and phase rule (the phase of a clock, above) are the existing ones.
 *
 * Potential.  For a state with distance d (uint16): phi = -(scale * (float)d) in float32, with one rounding; phi = 0
 * exactly (+0.0f) at d == 0.
 *
 * Shaping term.  F = (gamma * phi_after) - phi_before; out = reward + F.  Both are float32, with one IEEE rounding per
 * operation: the kernels are compiled with fp contraction off around them, a fused multiply-add would round differently.
 *
 * Unshaped elements.  An element is unshaped if either state is no cell or has distance MG_NAV_UNREACHABLE (a wall
 * dropped onto it, a cell not free at its phase).  An unshaped element has F = 0 (+0.0f), passes `reward` through bit for
 * bit (a -0.0f or a NaN payload stays) and has mask = 0; mask = 1 elsewhere.
 *
 * Terminal rule.  With flag MG_NAV_SHAPE_ZERO_TERMINAL and done != 0, phi_after = 0; such an element is shaped iff the
 * acting state is reachable.  Without the flag the terminal position's own potential is used: that matches a target
 * r + gamma * V(s') with no done mask.
 *
 * Timed fields (period > 1).  The acting state is (acting cell, phase of age); the after state is (after cell, phase of
 * (age <= 0 ? 0 : age) + 1), i.e. the phase that follows the acting one. */
#define MG_NAV_SHAPE_ZERO_TERMINAL 2 /* flags: shares the flag space with MG_NAV_DOORS_OPEN */

/* The rollout, from ONE field per env.
 *   dist        uint16[n_envs][period][dist_pitch]: with period == 1 what mg_nav_field writes, otherwise what
 *               mg_nav_timed_field writes (dist_pitch in elements, 0 = dense width*height)
 *   pos_before, pos_after  float[T][n_envs][2] = (y, x) before / after step t (8-byte aligned): exactly the two streams
 *               mg_nav_optimal_moves and mg_nav_lookup take.  The age rule applies to pos_before only.
 *   age, init_pos  as in mg_nav_optimal_moves; nullable together when period == 1, required when period > 1
 *   done        uint8[T][n_envs]: required with MG_NAV_SHAPE_ZERO_TERMINAL, ignored without it
 *   reward      float[T][n_envs] (nullable; then reward_out must be NULL as well)
 *   reward_out, shaping (F), mask (uint8)  [T][n_envs], each nullable, at least one given.  reward_out == reward (the
 *               same pointer) is allowed and defined: the reward is shaped in place.  Any other overlap is the caller's
 *               error.
 * One launch covers all envs; T == 0 launches nothing.  All outputs leave as aligned 16-byte stores (4 floats, 16 mask
 * bytes), element by element only in the first and last chunk of a workgroup's share (csrc/row_store.h); the float
 * arrays need 4-byte alignment, mask none, and nothing outside the first T * n_envs elements of an output is written.
 * flags: MG_NAV_SHAPE_ZERO_TERMINAL only (the doors are the field's business).
 * TW_E_ARG: the cases of mg_nav_optimal_moves (period == 1) / mg_nav_timed_moves (period > 1) with pos_before and
 * pos_after for pos; period outside 1..MG_NAV_MAX_PERIOD; reward, reward_out or shaping not 4-byte aligned; no output
 * given; reward_out without reward; MG_NAV_SHAPE_ZERO_TERMINAL without done; unknown flag bits; a non-finite scale or
 * gamma. */
int mg_nav_shape(const uint16_t *dist, int64_t dist_pitch, int period, int n_envs, int width, int height,
                 const float *pos_before, const float *pos_after, const int32_t *age, const float *init_pos,
                 const uint8_t *done, const float *reward, int T, float scale, float gamma, int flags,
                 float *reward_out, float *shaping, uint8_t *mask, void *stream);

/* Hindsight records, each under its OWN goal.  Per record b: let F be the field mg_nav_field computes for env rec_n[b]
 * with visit_cell(rec_goal[b]) as its single source.  The acting state is taken exactly as in mg_nav_goal_moves (the
 * acting position of t = rec_t[b], n = rec_n[b]); the after state is visit_cell(pos_after[t][n]); both distances are
 * read in F and shaped as above.
 *   rec_done    uint8[n_records]: required with MG_NAV_SHAPE_ZERO_TERMINAL, ignored without it
 *   rec_reward  float[n_records] (nullable; then reward_out must be NULL as well)
 *   reward_out, shaping, mask  per record, each nullable, at least one given; reward_out == rec_reward is allowed (in
 *               place), any other overlap is the caller's error
 * A record is unshaped (F = 0, reward passed through, mask = 0) for every reason mg_nav_goal_moves gives an empty label
 * -- rec_t or rec_n out of range, a goal that is no cell or not enterable, an acting position that is no cell or has no
 * path -- and also when the after state is no cell or unreachable.  No such record addresses memory outside its arrays.
 * As in mg_nav_goal_moves: the result of record b depends on record b alone; one launch, no atomics (none for
 * n_records == 0); a workgroup owns 1024 consecutive records and floods once per run of equal (env, goal cell); the
 * planes are read by the over-read rule; the outputs leave by the store rule of mg_nav_shape, nothing outside the first
 * n_records elements is written.
 * Invariant: for records that share one goal per env the outputs equal mg_nav_field(goal_x, goal_y) followed by
 * mg_nav_shape on the same elements.
 * flags: MG_NAV_DOORS_OPEN | MG_NAV_SHAPE_ZERO_TERMINAL.
 * TW_E_ARG: the cases of mg_nav_goal_moves (pos_before and pos_after for pos, the three outputs for moves); rec_reward,
 * reward_out or shaping not 4-byte aligned; no output given; reward_out without rec_reward; MG_NAV_SHAPE_ZERO_TERMINAL
 * without rec_done; unknown flag bits; a non-finite scale or gamma. */
int mg_nav_goal_shape(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                      uint32_t pass_types, int flags, const int32_t *rec_t, const int32_t *rec_n,
                      const float *rec_goal, const uint8_t *rec_done, const float *rec_reward, int64_t n_records,
                      const float *pos_before, const float *pos_after, const int32_t *age, const float *init_pos,
                      int T, float scale, float gamma, float *reward_out, float *shaping, uint8_t *mask,
                      void *stream);

/* mg_nav_goal_shape over (cell, phase): hindsight records, each under its OWN goal, shaped with the potential of a world
 * whose blockers move -- the potential mg_nav_shape uses with a timed field, so that a rollout and its hindsight records
 * agree around the blockers.  Nothing here is new: every rule is one of the blocks above.
 *   type, state, n_envs, width, height, pass_types: the world exactly as in mg_nav_field (state nullable)
 *   blocked, blocked_env_stride, period: the schedule; free cells, transition, distance and phase from the clock exactly
 *                 as in the "time-expanded fields" block
 *   rec_t, rec_n, rec_goal, n_records, pos_before, age, init_pos, T: the records and the acting positions exactly as in
 *                 mg_nav_timed_goal_moves (pos_before for pos); age and init_pos are REQUIRED, age[t][n] is also the clock
 *   pos_after, rec_done, rec_reward, scale, gamma, reward_out, shaping, mask: exactly as in mg_nav_goal_shape
 * Per record b, with t = rec_t[b], n = rec_n[b]: let F be what mg_nav_timed_field computes for env n with
 * visit_cell(rec_goal[b]) as its single source -- a source is 0 in every phase in which it is free.  The acting state is
 * the acting cell of mg_nav_timed_goal_moves (age[t][n] <= 0 ? init_pos : pos_before[t][n], by the rule of the visit
 * counters) at the phase of age[t][n]; the after state is visit_cell(pos_after[t][n]) at the phase that follows (the
 * "Timed fields" paragraph of the shaping block).  Both distances are read in F; phi, the shaping term, out, the unshaped
 * rule (F = +0.0f, the reward passed through bit for bit, mask = 0) and the terminal rule (MG_NAV_SHAPE_ZERO_TERMINAL
 * with rec_done) are exactly those of mg_nav_goal_shape.
 * A record is unshaped for every reason mg_nav_timed_goal_moves gives an empty label -- rec_t or rec_n out of range, a
 * goal that is no cell or free at no phase, an acting state that is no cell, not free at its phase or without a path --
 * and also when the after state is no cell, not free at its phase (a ball that moved onto the agent) or unreachable,
 * unless the terminal rule applies.  No such record addresses memory outside its arrays.
 * Invariants: (a) for records that share one goal per env the outputs equal mg_nav_timed_field(goal_x, goal_y) followed
 * by mg_nav_shape with that period on the same elements; (b) with period = 1 and an all-zero schedule the outputs equal
 * mg_nav_goal_shape's; (c) mask[b] != 0 implies that mg_nav_timed_goal_moves gives record b a non-empty move set, with
 * the acting_dist the shaping used.
 * As in mg_nav_timed_goal_moves: the result of record b depends on record b alone; one launch, no atomics (none for
 * n_records == 0); a workgroup owns 1024 consecutive records and floods once per run of equal (env, goal cell) -- the
 * phase is no part of the key; a flood ends after at most width*height*P rounds; every (width, height, period) the
 * limits allow works (mg_nav_timed_goal_shape_floods).  The planes are read by the over-read rule; the outputs leave by
 * the store rule of mg_nav_shape, nothing outside the first n_records elements is written.
 * flags: MG_NAV_DOORS_OPEN | MG_NAV_SHAPE_ZERO_TERMINAL.
 * TW_E_ARG: the cases of mg_nav_timed_goal_moves (pos_before and pos_after for pos, the three outputs for moves) and
 * those of mg_nav_goal_shape: NULL age or init_pos; period outside 1..MG_NAV_MAX_PERIOD; NULL or misaligned blocked;
 * blocked_env_stride < 0 or 0 < blocked_env_stride < P*height; rec_reward, reward_out or shaping not 4-byte aligned; no
 * output given; reward_out without rec_reward; MG_NAV_SHAPE_ZERO_TERMINAL without rec_done; unknown flag bits; a
 * non-finite scale or gamma. */
int mg_nav_timed_goal_shape(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                            uint32_t pass_types, int flags, const uint32_t *blocked, int64_t blocked_env_stride,
                            int period, const int32_t *rec_t, const int32_t *rec_n, const float *rec_goal,
                            const uint8_t *rec_done, const float *rec_reward, int64_t n_records, const float *pos_before,
                            const float *pos_after, const int32_t *age, const float *init_pos, int T, float scale,
                            float gamma, float *reward_out, float *shaping, uint8_t *mask, void *stream);

/* Host only, no launch: how many floods a workgroup of mg_nav_timed_goal_shape runs at a time at this size and period.
 * With cells = width*height rounded up to a multiple of 8 (whole 16-byte chunks per phase image), it is the largest f of
 * 8, 4, 2, 1 with  MG_NAV_TIMED_GOAL_SHAPE_LDS + f * period * cells * 2 <= 65536,  and 1 if none is (one image always
 * fits: 32 x 32 with P = 16 gives 1).  MG_NAV_TIMED_GOAL_SHAPE_LDS is the workgroup's staging in bytes -- the move sets'
 * keys and heads, a phase byte per record, the three outputs on their way out, and 64 bytes for aligning them -- which is
 * larger than that of mg_nav_timed_goal_moves, so the two counts differ.
 * TW_E_ARG: a side <= 0 or > MG_NAV_MAX_SIDE, period outside 1..MG_NAV_MAX_PERIOD. */
#define MG_NAV_TIMED_GOAL_SHAPE_LDS 25968
int mg_nav_timed_goal_shape_floods(int width, int height, int period);

/* ---- Look-ahead: where a shortest path leads in k steps (the k-step counterpart of the move sets).
 *
 * The world, moves, fields, visit_cell rule, acting-position rule (age <= 0 ? init_pos : pos) and phase rule are the
 * existing ones.  1 <= steps <= MG_NAV_AHEAD_MAX_STEPS.
 *
 * Label.  A uint64_t: bit (dy + 3) * MG_NAV_AHEAD_SIDE + (dx + 3) stands for the displacement (dy, dx) = (y' - y, x' - x)
 * from the acting cell (x, y) -- the order of `pos` and of the classes displacement + 3 of the orientation head.  Bit 24 is
 * "same cell"; bits 49..63 are always 0.
 *
 * Look-ahead of an acting state s0 = (c, phase) with distance d in a field, for steps = k:
 *   S_0 = {s0};  S_(j+1) = the union of the successors of the states in S_j;  the label = { c' - c : (c', .) in S_k }.
 *   Successors.  A state at distance 0 has itself as its only successor: the episode has ended there, and the position
 *   stays (the rule pos[min(t + k, end + 1)] of a realised trajectory) -- whether or not the cell is free at the next phase.
 *   Any other state has exactly the members of its move set (mg_nav_optimal_moves / mg_nav_timed_moves): a neighbour inside
 *   the world whose distance, read in the row the move arrives in, is one less, and the cell itself where waiting is
 *   optimal in a timed field.  The row the move arrives in is the same row for period 1, the row of phase + 1 mod P otherwise.
 *   The label is 0 where the acting position is no cell or its state is MG_NAV_UNREACHABLE.
 * Two consequences: all members of S_j share one phase and one distance, max(d - j, 0), so the expansion simply stops after
 * min(k, d) steps; and S_j lies within Manhattan radius j <= 3, so one 64-bit word holds every frontier.
 *
 * Invariants.  (a) At steps = 1 the label is the image of the move set: left -> bit 23, right -> 25, up -> 17, down -> 31,
 * stay -> 24.  (b) Every cell of the label has distance max(d - k, 0) -- at phase + k for a timed field -- unless d < k.
 * (c) The label at k is the union, over the cells of the label at k - 1, of their labels at 1 at the phase that follows;
 * cells at distance 0 are carried over.  (d) label != 0 iff acting_dist != MG_NAV_UNREACHABLE.  (b) - (d) hold on fields the
 * field kernels wrote; on an array of distances that is no field (no neighbour one nearer) a label can be 0 at a reachable
 * acting_dist: the frontier then simply dies, and nothing is read outside the arrays either way. */
#define MG_NAV_AHEAD_MAX_STEPS 3
#define MG_NAV_AHEAD_SIDE 7

/* The rollout, from ONE field per env.
 *   dist, dist_pitch, period, age, init_pos: exactly as mg_nav_shape takes them (period 1 = what mg_nav_field writes, age and
 *               init_pos nullable together; period > 1 = what mg_nav_timed_field writes, age is the clock, both required)
 *   pos         float[T][n_envs][2] = (y, x) BEFORE step t (8-byte aligned), as in mg_nav_optimal_moves
 *   ahead       uint64[T][n_envs], 8-byte aligned;  acting_dist uint16[T][n_envs] (nullable): as in mg_nav_optimal_moves
 * One launch, no atomics; T == 0 launches nothing.  Both outputs leave as aligned 16-byte stores (2 labels, 8 distances),
 * element by element only in the first and last chunk of a workgroup's share (csrc/row_store.h); nothing outside the first
 * T * n_envs elements of either output is written, and nothing outside the arrays is read for any position, NaN included.
 * TW_E_ARG: the cases of mg_nav_optimal_moves (period == 1) / mg_nav_timed_moves (period > 1) with ahead for moves; period
 * outside 1..MG_NAV_MAX_PERIOD; steps outside 1..MG_NAV_AHEAD_MAX_STEPS; ahead not 8-byte aligned. */
int mg_nav_ahead(const uint16_t *dist, int64_t dist_pitch, int period, int n_envs, int width, int height,
                 const float *pos, const int32_t *age, const float *init_pos, int T, int steps, uint64_t *ahead,
                 uint16_t *acting_dist, void *stream);

/* Hindsight records, each under its OWN goal, on the static map.  Per record b: let F be the field mg_nav_field computes for
 * env rec_n[b] with visit_cell(rec_goal[b]) as its single source; ahead[b] and acting_dist[b] are what mg_nav_ahead gives
 * for the record's acting cell in F.  The records, the acting positions, the records that name nothing (label 0,
 * MG_NAV_UNREACHABLE, no access outside the arrays), the independence of a record from its neighbours and their order, the
 * workgroup's 1024 records and its one flood per run of equal (env, goal cell), the reads and the store rule are those of
 * mg_nav_goal_moves.
 *   ahead uint64[n_records], 8-byte aligned;  acting_dist uint16[n_records] (nullable)
 * Invariant: for records that share one goal per env the outputs equal mg_nav_field(goal_x, goal_y) followed by mg_nav_ahead
 * on the same positions.  One launch, no atomics; n_records == 0 returns 0 and launches nothing.
 * TW_E_ARG: the cases of mg_nav_goal_moves with ahead for moves; steps outside 1..MG_NAV_AHEAD_MAX_STEPS; ahead not 8-byte
 * aligned. */
int mg_nav_goal_ahead(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                      uint32_t pass_types, int flags, const int32_t *rec_t, const int32_t *rec_n,
                      const float *rec_goal, int64_t n_records, const float *pos, const int32_t *age,
                      const float *init_pos, int T, int steps, uint64_t *ahead, uint16_t *acting_dist, void *stream);

/* mg_nav_goal_ahead over (cell, phase): the look-ahead labels of hindsight records, each under its OWN goal, in a world whose
 * blockers move -- the labels mg_nav_ahead gives a rollout from a timed field, so that a rollout and its hindsight records
 * agree around the blockers.  Nothing here is new: every rule is one of the blocks above.  Per record b: let F be what
 * mg_nav_timed_field computes for env rec_n[b] with visit_cell(rec_goal[b]) as its single source; ahead[b] and acting_dist[b]
 * are what mg_nav_ahead gives, with that period and `steps`, for the record's acting cell in F -- age[t][n] <= 0 ? init_pos :
 * pos[t][n], at the phase of age[t][n].  The world, the schedule, the records, the REQUIRED age and init_pos, the records that
 * name nothing (label 0, MG_NAV_UNREACHABLE, no access outside the arrays), the independence of a record from its neighbours
 * and their order, the one launch without atomics, the workgroup's 1024 records, its one flood per run of equal (env, goal
 * cell) for every phase, the at most width*height*P rounds of a flood and the reads are those of mg_nav_timed_goal_moves; the
 * outputs and the store rule are those of mg_nav_goal_ahead.
 *   ahead uint64[n_records], 8-byte aligned;  acting_dist uint16[n_records] (nullable)
 * Invariants: (a) for records that share one goal per env the outputs equal mg_nav_timed_field(goal_x, goal_y) followed by
 * mg_nav_ahead with that period on the same positions; (b) with period = 1 and an all-zero schedule they equal
 * mg_nav_goal_ahead's; (c) at steps = 1 the label is the image of mg_nav_timed_goal_moves' move set (invariant (a) of the
 * look-ahead block), with the same acting_dist; (d) ahead[b] != 0 iff acting_dist[b] != MG_NAV_UNREACHABLE.
 * n_records == 0 returns 0 and launches nothing.
 * TW_E_ARG: the cases of mg_nav_timed_goal_moves with ahead for moves; steps outside 1..MG_NAV_AHEAD_MAX_STEPS; ahead not
 * 8-byte aligned. */
int mg_nav_timed_goal_ahead(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                            uint32_t pass_types, int flags, const uint32_t *blocked, int64_t blocked_env_stride,
                            int period, const int32_t *rec_t, const int32_t *rec_n, const float *rec_goal,
                            int64_t n_records, const float *pos, const int32_t *age, const float *init_pos, int T,
                            int steps, uint64_t *ahead, uint16_t *acting_dist, void *stream);

/* Host only, no launch: how many floods a workgroup of mg_nav_timed_goal_ahead runs at a time at this size and period: by the
 * formula of mg_nav_timed_goal_shape_floods with MG_NAV_TIMED_GOAL_AHEAD_LDS, the workgroup's staging in bytes -- the move
 * sets' keys and heads, a phase byte per record, 8 bytes of label per record on their way out, and 64 bytes for aligning
 * them (32 x 32 with P = 16 gives 1).
 * TW_E_ARG: a side <= 0 or > MG_NAV_MAX_SIDE, period outside 1..MG_NAV_MAX_PERIOD. */
#define MG_NAV_TIMED_GOAL_AHEAD_LDS 22864
int mg_nav_timed_goal_ahead_floods(int width, int height, int period);

/* ---- Path efficiency: how good a trajectory was, per episode (success weighted by path length, steps off the path).
 *
 * The world, the fields (dist uint16[n_envs][period][dist_pitch], period 1 = what mg_nav_field writes), the visit_cell
 * rule, the acting-position rule (age <= 0 ? init_pos : pos) and the phase rule (the phase of a clock) are the existing ones.
 *
 * Per step.  d_before and d_after are the two distances mg_nav_shape reads WITHOUT MG_NAV_SHAPE_ZERO_TERMINAL: d_before is
 * the acting state's, at the phase of age; d_after is the after cell's, in the one field at period 1 and in the field of the
 * phase that follows the acting one otherwise ("Reward shaping", "Timed fields").  A done step is no exception: the terminal
 * position's own distance is d_after.  A position that is no cell has distance MG_NAV_UNREACHABLE.
 * A step is ON PATH iff d_before is reachable, d_before >= 1 and d_after == d_before - 1.  In a timed field an optimal wait
 * is therefore on path; walking into a blocker, or being hit by one (the after state is not free: unreachable), is not.
 *
 * Episodes.  An episode ends with a step whose terminated | truncated is set; the next step of that env opens a new one.
 * Per env four carries hold the running episode: start (d_before of its first step), best (the least distance it has
 * stood at), off (its steps that were not on path) and steps (its steps so far).  steps == 0 means that no episode is
 * running -- all-zero carries are the state after a reset -- and the other three carries are then meaningless.
 *
 * Everything is integer: the results do not depend on scheduling or on how a rollout is cut into launches. */

/* The scan, one launch for all envs (none for T == 0), no atomics.  For every env n, for t = 0 .. T - 1 in this order:
 *     if (steps == 0) { start = best = d_before; off = 0; }
 *     steps += 1;   off += 1 unless the step is on path;   best = min(best, d_after);
 *     ep_start[t][n] = start, ep_best[t][n] = best, ep_off[t][n] = off, ep_steps[t][n] = steps;
 *     if (terminated[t][n] | truncated[t][n]) steps = 0;
 * and the four carries are written back afterwards (start, best and off as they stand, also behind a done step).
 * MG_NAV_UNREACHABLE is the largest uint16, so an unreachable d_after never lowers best, and an episode that starts on an
 * unreachable state has start = MG_NAV_UNREACHABLE until it ends.  At a done step the four outputs describe the episode that
 * ends there, wherever -- in this launch or in an earlier one -- it began.  T launches of one step each give the bits of
 * one launch of T steps, carries included.
 *   dist, dist_pitch, period, pos_before, pos_after, age, init_pos: exactly as mg_nav_shape takes them (age and init_pos
 *               nullable together when period == 1, required when period > 1)
 *   terminated, truncated  uint8[T][n_envs]
 *   carry_start, carry_best  uint16[n_envs];  carry_off, carry_steps  int32[n_envs]: in and out
 *   ep_start, ep_best  uint16[T][n_envs];  ep_off, ep_steps  int32[T][n_envs]: each nullable, at least one given
 * A lane owns an env; the rows [t][.] are read and written coalesced, element by element.  Nothing outside the first
 * T * n_envs elements of an output or outside the n_envs elements of a carry is written, and nothing outside the arrays
 * is read for any position, NaN included.
 * TW_E_ARG: the cases of mg_nav_shape that concern dist, dist_pitch, period, n_envs, width, height, pos_before, pos_after,
 * age, init_pos and T; NULL terminated / truncated / carry; a uint16 array not 2-byte aligned, an int32 array not 4-byte
 * aligned; no output given. */
int mg_nav_path_scan(const uint16_t *dist, int64_t dist_pitch, int period, int n_envs, int width, int height,
                     const float *pos_before, const float *pos_after, const int32_t *age, const float *init_pos,
                     const uint8_t *terminated, const uint8_t *truncated, int T, uint16_t *carry_start,
                     uint16_t *carry_best, int32_t *carry_off, int32_t *carry_steps, uint16_t *ep_start,
                     uint16_t *ep_best, int32_t *ep_off, int32_t *ep_steps, void *stream);

/* What the episodes that ended in a rollout looked like: summary double[MG_NAV_PATH_SUMMARY] over the done steps of the
 * scan's four outputs [T][N] (all four required).  An episode is RATED iff its start is reachable.
 *   0  episodes                                   1  successes (terminated != 0)
 *   2  rated episodes                             3  the sum of SPL over the rated: terminated ? start / max(steps, start) : 0
 *   4  the sum of start over the rated            5  the sum of best over the rated
 *   6  the sum of (start - best) / start over the rated with start >= 1
 *   7  the sum of off over all episodes           8  the sum of steps over all episodes
 *   9  the least best over the rated, +inf when there is none
 * The two quotients are float64 divisions of the integers.  Deterministic in the way of ppo_episode_summary (twoarmy_ppo.h):
 * the grid depends on (T, N) alone, a thread folds a contiguous run of the row-major (t, then n) index range in order, lanes,
 * wavefronts and workgroups are combined in index order -- lanes as a binary tree -- each workgroup leaves one partial of
 * MG_NAV_PATH_SUMMARY doubles in `workspace`, and one wavefront of a second kernel combines the partials in block order.
 * Entries 0 - 2, 4, 5 and 7 - 9 are exact (integers below 2^53, a minimum); 3 and 6 are that tree of float64 additions.
 *   workspace   double[mg_nav_path_summary_workspace(T, N)], 8-byte aligned like summary
 * mg_nav_path_summary_workspace: host only, the number of doubles.
 * TW_E_ARG: a NULL array; T <= 0 or N <= 0; T * N >= 2^40; ep_start or ep_best not 2-byte aligned, ep_off or ep_steps not
 * 4-byte aligned, summary or workspace not 8-byte aligned. */
#define MG_NAV_PATH_SUMMARY 10
int mg_nav_path_summary_workspace(int T, int N);
int mg_nav_path_summary(const uint16_t *ep_start, const uint16_t *ep_best, const int32_t *ep_off, const int32_t *ep_steps,
                        const uint8_t *terminated, const uint8_t *truncated, int T, int N, double *summary,
                        double *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MINIGRID_NAV_H */
